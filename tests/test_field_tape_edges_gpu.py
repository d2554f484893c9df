"""The field tape on the device at the inputs of tests/field_tape_cases.py: grid shapes against the tile edges, fields with exact ties,
translated origins and metric units, receivers that share nodes, long relaxations, more events than slots.  On the device's own fields:
tape.field and tt are those of raytrace; vjp (receiver, field and both cotangents) is bit-equal to tests/adjoint_reference.py under the
tiled schedule, under global Jacobi and on a second tiled run; jvp with its fields is bit-equal to tests/tangent_reference.py under both
schedules; gauss_newton(v, rw) has the bits of vjp(rw * jvp(v)); <w, J v> = <J^T w, v> to rounding.  tests/test_field_tape_edges.py checks
the same restatements against the oracle on the same inputs."""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_tape_cases as FC  # noqa: E402
from field_tape_cases import DOT_TOL, _bits_equal  # noqa: E402

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
KINDS = ("receivers", "field", "both")


def _grid(case, dt, **kw):
    import ttcr_amd

    axes = [case.origin[a] + np.arange(case.nn[a]) * case.dx for a in range(3)]
    g = ttcr_amd.Grid3d(*axes, cell_slowness=0, method="FSM", dtype=dt, weno=0, tt_from_rp=0, **kw)
    g.set_slowness(case.s.reshape(case.nn, order="F"))
    return g


def _tape(case, dt, **kw):
    """the tape of one raytrace_adjoint call for the events of the case, its tt and fields checked against raytrace"""
    src, rcv, agg, rows = FC.call_arrays(case, np.random.default_rng(61))
    g = _grid(case, dt, **kw)
    tt, tape = g.raytrace_adjoint(src, rcv, aggregate_src=agg)
    n_nodes = int(np.prod(case.nn))
    assert (tape.n_events, tape.n_data, tape.n_cols) == (len(case.events), rcv.shape[0], n_nodes) and tape.nbytes > 0
    _bits_equal(tt, g.raytrace(src, rcv, aggregate_src=agg))
    fields = []
    for e, ev in enumerate(case.events):   # every event on its own: the field the grid holds after it
        one = np.column_stack([np.full(ev["pts"].shape[0], ev["t0"]), ev["pts"]])
        _bits_equal(tt[rows[e]], g.raytrace(one, rcv[rows[e]], aggregate_src=True))
        fields.append(tape.field(e))
        _bits_equal(fields[e], g.get_grid_traveltimes().flatten("F"))
    return g, tape, rcv, rows, fields


def _inputs(case, dt, rcv):
    """cotangents and perturbations of a case: w and rw per receiver row, fc per event and node, ds per node"""
    rng = np.random.default_rng(67)
    n_nodes = int(np.prod(case.nn))
    w = FC.wide_weights(rng, rcv.shape[0], dt)
    fc = rng.standard_normal((len(case.events), n_nodes)).astype(dt)
    ds = (case.s * rng.standard_normal(n_nodes)).astype(dt)
    rw = rng.uniform(0.5, 2.0, rcv.shape[0]).astype(dt)
    return w, fc, ds, rw


def _check_vjp(tape, case, dt, rcv, rows, fields, w, fc, kinds=KINDS):
    """restatement == tiled == Jacobi == a second tiled run, to the bit; {kind: (gradient, tiled passes, Jacobi passes)}"""
    out = {}
    for kind in kinds:
        ww, ff = {"receivers": (w, None), "field": (None, fc), "both": (w, fc)}[kind]
        ref = FC.reference_vjp(fields, case, dt, rcv, rows, ww, ff)
        assert np.all(np.isfinite(ref)) and np.any(ref != 0)
        gt = tape.vjp(ww, ff)
        pt = tape.passes
        _bits_equal(gt, ref)
        gj = tape.vjp(ww, ff, schedule="jacobi")
        pj = tape.passes
        _bits_equal(gj, ref)
        _bits_equal(tape.vjp(ww, ff, schedule="tiled"), ref)
        assert pt >= 1 and pj >= 1 and tape.passes >= 1
        out[kind] = (gt, pt, pj)
    return out


def _check_jvp(tape, case, dt, rcv, rows, fields, ds):
    """restatement == tiled == Jacobi, to the bit, receivers and fields; (dtt, mu, tiled passes, Jacobi passes)"""
    ref_dtt, ref_mu = FC.reference_jvp(fields, case, dt, rcv, rows, ds)
    assert np.all(np.isfinite(ref_mu)) and np.any(ref_mu != 0) and np.any(ref_dtt != 0)
    passes = {}
    for schedule in ("tiled", "jacobi"):
        dtt, mu = tape.jvp(ds, return_fields=True, schedule=schedule)
        passes[schedule] = tape.passes
        assert tape.passes >= 1 and mu.shape == (tape.n_events, tape.n_cols)
        _bits_equal(dtt, ref_dtt)
        _bits_equal(mu, ref_mu)
    return dtt, mu, passes["tiled"], passes["jacobi"]


def _check_gauss_newton(tape, dt, ds, rw, dtt):
    for schedule in ("tiled", "jacobi"):
        gn = tape.gauss_newton(ds, rw, schedule=schedule)
        assert isinstance(tape.passes, tuple) and len(tape.passes) == 2 and min(tape.passes) >= 1
        assert (rw * dtt).dtype == dt
        _bits_equal(gn, tape.vjp(rw * dtt, schedule=schedule))
    return gn


def _check_everything(case, dt, label, **kw):
    """every check of this file on one case; returns what a caller may want to compare between configurations"""
    dtype = np.dtype(dt)
    g, tape, rcv, rows, fields = _tape(case, dt, **kw)
    w, fc, ds, rw = _inputs(case, dt, rcv)
    grads = _check_vjp(tape, case, dt, rcv, rows, fields, w, fc)
    dtt, mu, jt, jj = _check_jvp(tape, case, dt, rcv, rows, fields, ds)
    gn = _check_gauss_newton(tape, dt, ds, rw, dtt)
    # the dot-product identity with the moduli of the same inputs: every term of the four sums is then positive, and the figure measures
    # the rounding of J and J^T, not the cancellation of a random sum (with signed inputs the fp32 RESTATEMENT alone reached 5.7e-5 on
    # the metric grid with an on-node source)
    wp, fcp, dsp = np.abs(w), np.abs(fc), np.abs(ds)
    dtt_p, mu_p = tape.jvp(dsp, return_fields=True)
    e_rcv, e_fld = FC.dot_errors(wp, dtt_p, tape.vjp(wp), fcp, mu_p, tape.vjp(None, fcp), dsp)
    print("%s, %s: %d events, %d rows; passes tiled / Jacobi: vjp %d / %d, jvp %d / %d; device <w, J v> against <J^T w, v>: receivers "
          "%.2e, field %.2e (bound %.0e)" % (label, dtype.name, tape.n_events, rcv.shape[0], grads["both"][1], grads["both"][2], jt, jj,
                                             e_rcv, e_fld, DOT_TOL[dtype]))
    assert e_rcv <= DOT_TOL[dtype] and e_fld <= DOT_TOL[dtype], (e_rcv, e_fld)
    return dict(fields=fields, grads={k: v[0] for k, v in grads.items()}, dtt=dtt, mu=mu, gn=gn)


# ---- a. grid shapes against the tile edges
@DTYPES
@pytest.mark.parametrize("nn", FC.SHAPES, ids=lambda nn: "x".join(map(str, nn)))
def test_shapes_against_the_tile_edges(nn, dt):
    case = FC.shape_case(nn)
    # every 8^3 tile (so every workgroup of every relaxation kernel) holds two receivers of each event or more
    for ev in case.events:
        tiles = np.floor((ev["rcv"] - np.array(case.origin)) / case.dx / 8 + 1e-9).astype(int)
        counts = {}
        for t in map(tuple, tiles):
            counts[t] = counts.get(t, 0) + 1
        assert len(counts) == int(np.prod([-(-n // 8) for n in nn])) and min(counts.values()) >= 2, counts
    _check_everything(case, dt, "shape " + case.name)


# ---- b. ties
@DTYPES
@pytest.mark.parametrize("name", sorted(FC.TIES))
def test_fields_with_ties(name, dt):
    case = FC.tie_case(name)
    out = _check_everything(case, dt, "ties " + name)
    decisive, total = FC.count_ties(out["fields"][0], case.nn)
    print("ties %s, %s: %d equal lower / upper neighbour pairs on the device field, %d of them upwind of the node between"
          % (name, np.dtype(dt).name, total, decisive))
    assert total > 0   # (without ties the case has lost its point)
    assert decisive > 0 or name not in FC.DECISIVE_TIES


# ---- c. origin and units
@DTYPES
@pytest.mark.parametrize("name", FC.ORIGIN_CASES)
def test_translated_origin_and_metric_units(name, dt):
    _check_everything(FC.origin_case(name), dt, "origin " + name)


# ---- d. receivers that share nodes
@DTYPES
@pytest.mark.parametrize("name", FC.SHARED_CASES)
def test_receivers_that_share_nodes(name, dt):
    case = FC.shared_case(name)
    assert sorted(ev["rcv"].shape[0] for ev in case.events)[0] == (449 if name == "one_event" else 1)
    _check_everything(case, dt, "shared " + name, n_threads=1 if name == "one_event" else 2)


# ---- e. long runs
@DTYPES
def test_long_runs_with_events_that_finish_far_apart(dt):
    """Three events on a grid whose Jacobi relaxation takes far more passes than the flag ring has rows (a source in a corner cell gives
    a dependency chain of nnx + nny + nnz - 3 nodes or more, one pass per link), with the centre event done long before the corner one."""
    case = FC.long_case(dt)
    dtype = np.dtype(dt)
    t0 = time.time()
    g, tape, rcv, rows, fields = _tape(case, dt, n_threads=3)
    w, fc, ds, rw = _inputs(case, dt, rcv)
    t1 = time.time()
    grads = _check_vjp(tape, case, dt, rcv, rows, fields, w, fc, kinds=("both",))
    t2 = time.time()
    dtt, mu, jt, jj = _check_jvp(tape, case, dt, rcv, rows, fields, ds)
    t3 = time.time()
    print("long runs, %s, %s nodes, 3 events: passes tiled / Jacobi: vjp %d / %d, jvp %d / %d; seconds: solves %.1f, vjp with its "
          "restatement %.1f, jvp with its restatement %.1f" % (dtype.name, "x".join(map(str, case.nn)), grads["both"][1], grads["both"][2],
                                                              jt, jj, t1 - t0, t2 - t1, t3 - t2))
    assert grads["both"][2] > 2 * FC.ADJ_RING and jj > 2 * FC.ADJ_RING, (grads["both"][2], jj)
    assert grads["both"][1] >= 1 and jt >= 1   # (the tiled counts depend on the scheduling of the tiles, by design)


# ---- f. more events than slots
@DTYPES
def test_more_events_than_slots(dt):
    case = FC.slots_case()
    assert len(case.events) == 11
    first = None
    for n_threads in (1, 4, 16):
        if first is None:
            first = _check_everything(case, dt, "11 events, n_threads %d" % n_threads, n_threads=n_threads)
            continue
        g, tape, rcv, rows, fields = _tape(case, dt, n_threads=n_threads)
        w, fc, ds, rw = _inputs(case, dt, rcv)
        _bits_equal(np.stack(fields), np.stack(first["fields"]))
        for kind, (ww, ff) in {"receivers": (w, None), "field": (None, fc), "both": (w, fc)}.items():
            for schedule in ("tiled", "jacobi"):
                _bits_equal(tape.vjp(ww, ff, schedule=schedule), first["grads"][kind])
        for schedule in ("tiled", "jacobi"):
            dtt, mu = tape.jvp(ds, return_fields=True, schedule=schedule)
            _bits_equal(dtt, first["dtt"])
            _bits_equal(mu, first["mu"])
            _bits_equal(tape.gauss_newton(ds, rw, schedule=schedule), first["gn"])
