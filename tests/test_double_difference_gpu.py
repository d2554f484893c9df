"""The double-difference rows of the field tape on the device (FieldTape.set_row_pairs, pair_difference, pair_adjoint, row_operator, the
keyword pair_weight of the four products and the three solves, release_pairs and inversion.double_difference_step).  Every
comparison is to the bit, against the numpy restatement of tests/dd_reference.py on the device's own fields, for fp32 and fp64 and, where a
relaxation runs, under both schedules.  The grids are 6k's (tests/test_receiver_derivative_gpu.py: the reciprocal layout, every event
sees the same points); what can go wrong here are the launch blocks of the two kernels (pair and row counts around 256), the CSR by row
(rows without entries, a row with hundreds, repeated pairs), the order of a row's chain, and the array the adjoint half reads."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import adjoint_reference as AR  # noqa: E402
import dd_reference as DD  # noqa: E402
import field_tape_cases as FC  # noqa: E402
import hessian_reference as HR  # noqa: E402
import joint_reference as JR  # noqa: E402
import normal_reference as NR  # noqa: E402
import receiver_reference as RR  # noqa: E402
from field_tape_cases import _bits_equal  # noqa: E402
from test_receiver_derivative_gpu import ORIGIN, RDAMP, SCALE, SOLVE_NN, WEIGHTS, Run, _restated_halves, _rows_to_data  # noqa: E402

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
SCHEDULES = ("tiled", "jacobi")
SDAMP = (1e-2, 1e-1, 1.0, 1e-1)
CASES = {
    "2x2x2": dict(nn=(2, 2, 2)),
    "17x14x19": dict(nn=SOLVE_NN),
    "cells": dict(nn=(9, 8, 10), wrt="cells"),
    "translated": dict(nn=(9, 8, 10), origin=ORIGIN, translate=True),
    "five_events_1": dict(nn=(9, 8, 10), n_events=5, n_threads=1),
    "five_events_4": dict(nn=(9, 8, 10), n_events=5, n_threads=4),
}


def _in_child(fn, *args):
    """Run _torch_<fn>(*args) of this module in a fresh process that initialises torch's device before the first grid"""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_double_difference_gpu as t; t._torch_%s(*%r)"
            % (HERE, ROOT, fn, args))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def make_pairs(run, n_pairs, seed, long_row=0):
    """(row_a, row_b, pair_weight) in data rows: pairs inside one event and across events in turn, repeated pairs among them, the last
    two data rows of the tape's first event in no pair, a fifth of the weights zero; long_row: that many copies of one pair in front"""
    rng = np.random.default_rng(seed)
    rows = [np.asarray(r) for r in run.rows]
    spare = set(rows[0][-2:].tolist())
    rows = [np.array([x for x in r if x not in spare]) for r in rows]
    a, b = np.zeros(n_pairs, dtype=np.int64), np.zeros(n_pairs, dtype=np.int64)
    for p in range(n_pairs):
        e = int(rng.integers(len(rows)))
        f = e if (p % 2 == 0 or len(rows) == 1) else int((e + 1 + rng.integers(len(rows) - 1)) % len(rows))
        while True:
            a[p], b[p] = rng.choice(rows[e]), rng.choice(rows[f])
            if a[p] != b[p]:
                break
    if n_pairs > 6:                       # repeated pairs, one of them the other way round
        a[3], b[3] = a[0], b[0]
        a[5], b[5] = b[1], a[1]
    if long_row:
        a = np.concatenate([np.full(long_row, a[0]), a])
        b = np.concatenate([np.full(long_row, b[0]), b])
    pw = rng.uniform(0.1, 3.0, a.size)
    pw[rng.choice(a.size, a.size // 5, replace=False)] = 0.0
    return a, b, pw.astype(run.dt)


def to_tape(tape, a, b):
    """the pairs in tape rows (every data row of these runs is on the tape)"""
    inv = np.full(tape.n_data, -1, dtype=np.int64)
    inv[tape._rows] = np.arange(tape.n_rows)
    return inv[a], inv[b]


def from_tape(tape, rows_tape):
    out = np.zeros(tape.n_data, dtype=rows_tape.dtype)
    out[tape._rows] = rows_tape
    return out


def check_operators(tape, dt, a, b, pw, x, y, rw):
    """pair_difference, pair_adjoint and row_operator to the bit, arguments in data rows"""
    r = tape._rows
    ta, tb = to_tape(tape, a, b)
    d = tape.pair_difference(x)
    assert d.dtype == dt and d.shape == (a.size,)
    _bits_equal(d, DD.pair_difference(x[r], ta, tb))
    q = tape.pair_adjoint(y)
    assert q.dtype == dt and q.shape == (tape.n_data,)
    _bits_equal(q, from_tape(tape, DD.pair_adjoint(y, tape.n_rows, ta, tb)))
    for w_r in (rw, None):
        for w_p in (pw, None):
            got = tape.row_operator(x, w_r, w_p)
            _bits_equal(got, from_tape(tape, DD.row_operator(x[r], ta, tb, None if w_r is None else w_r[r], w_p)))
    return ta, tb


# ---- 1. the operators: pair counts around the launch block, rows without entries, a row with 300 entries
@DTYPES
@pytest.mark.parametrize("name", sorted(CASES))
def test_pair_operators_bits(name, dt):
    run = Run(dt=dt, **CASES[name])
    tape, n = run.tape, run.rcv.shape[0]
    rng = np.random.default_rng(5)
    x, rw = FC.wide_weights(rng, n, dt), run.rw
    before = tape.nbytes
    assert tape.n_pairs == 0 and tape.row_pairs.shape == (0, 2)
    with pytest.raises(ValueError, match="no row pairs"):
        tape.pair_difference(x)
    for n_pairs, long_row in ((0, 0), (1, 0), (255, 0), (256, 0), (257, 0), (40, 300)):
        a, b, pw = make_pairs(run, n_pairs, 100 + n_pairs, long_row)
        tape.set_row_pairs(a, b)
        assert n_pairs > 0 or tape.nbytes == before      # (the lists are on the host until the first call that uses them)
        assert tape.n_pairs == a.size and np.array_equal(tape.row_pairs, np.stack([a, b], axis=1))
        y = FC.wide_weights(rng, a.size, dt)
        ta, tb = check_operators(tape, dt, a, b, pw, x, y, rw)
        off, _ = DD.csr(tape.n_rows, ta, tb)
        deg = np.diff(off)
        assert n_pairs == 0 or (deg.min() == 0 and deg.max() >= (300 if long_row else 1))
        const = tape.pair_difference(np.full(n, 0.3712, dtype=dt))
        assert not np.any(const) and not np.any(np.signbit(const))
    tape.release_pairs()
    tape.free()


@DTYPES
def test_nbytes_of_the_pair_arrays(dt):
    run = Run(nn=(9, 8, 10), dt=dt)
    tape, n = run.tape, run.rcv.shape[0]
    elem = np.dtype(dt).itemsize
    x = FC.wide_weights(np.random.default_rng(7), n, dt)
    before = tape.nbytes
    a, b, pw = make_pairs(run, 57, 3)
    tape.set_row_pairs(a, b)
    assert tape.nbytes == before
    d = tape.pair_difference(x)                            # host x in w_tmp, no row_weight: the pair arrays alone
    m = 57
    dd_bytes = 2 * 4 * m + 4 * (n + 1) + 8 * m + 2 * m * elem + n * elem
    assert tape.nbytes == before + dd_bytes
    _bits_equal(tape.pair_adjoint(pw), tape.pair_adjoint(pw))
    assert tape.nbytes == before + dd_bytes
    tape.release_pairs()
    assert tape.nbytes == before and tape.n_pairs == 57   # (the pairs stay as set)
    tape.release_pairs()                                   # (a second release is a no-op)
    assert tape.nbytes == before
    _bits_equal(tape.pair_difference(x), d)
    assert tape.nbytes == before + dd_bytes
    tape.set_row_pairs(a[:5], b[:5])                       # a new list frees what the old one held
    assert tape.nbytes == before and tape.n_pairs == 5
    with pytest.raises(ValueError, match=r"pair 1 \(data rows %d, %d\) joins a row to itself" % (a[0], a[0])):
        tape.set_row_pairs([a[0], a[0]], [b[0], a[0]])
    assert tape.n_pairs == 5
    tape.free()


@DTYPES
def test_a_tape_with_257_rows(dt):
    """one event with 257 receivers: the row kernel's second block holds one row"""
    import ttcr_amd

    nn, dx = (9, 8, 10), FC.DX
    rng = np.random.default_rng(11)
    rcv = FC.random_receivers(nn, dx, FC.ZERO, rng, 257)
    grid = ttcr_amd.Grid3d(*[np.arange(k) * dx for k in nn], cell_slowness=0, method="FSM", dtype=dt, weno=0, tt_from_rp=0)
    grid.set_slowness(FC.model(nn, dx, FC.ZERO, "rough").reshape(nn, order="F"))
    src = np.array([[0.0, 1.3 * dx, 2.6 * dx, 3.2 * dx]])
    _, tape = grid.raytrace_adjoint(src, rcv, aggregate_src=True)
    assert tape.n_rows == tape.n_data == 257 and np.array_equal(tape._rows, np.arange(257))
    a = np.concatenate([rng.integers(0, 255, 300), [256, 255, 256, 0]])
    b = np.concatenate([(a[:300] + 1 + rng.integers(0, 250, 300)) % 255, [255, 256, 0, 256]])
    assert not np.any(a == b)
    pw = rng.uniform(0.0, 2.0, a.size).astype(dt)
    x, y, rw = FC.wide_weights(rng, 257, dt), FC.wide_weights(rng, a.size, dt), rng.uniform(0.5, 2.0, 257).astype(dt)
    tape.set_row_pairs(a, b)
    check_operators(tape, dt, a, b, pw, x, y, rw)
    v = (0.5 * rng.standard_normal(tape.n_cols)).astype(dt)
    for schedule in SCHEDULES:
        g = tape.gauss_newton(v, rw, schedule=schedule, pair_weight=pw)
        _bits_equal(g, tape.vjp(tape.row_operator(tape.jvp(v), rw, pw)))
    tape.free()


# ---- 2. the four products
def _scaled(sc, v, dt):
    return v if sc is None else (np.broadcast_to(np.asarray(sc, dtype=dt), v.shape) * v).astype(dt)


@DTYPES
@pytest.mark.parametrize("wrt", ["nodes", "cells"])
def test_products_with_pairs_bits(wrt, dt):
    run = Run(nn=SOLVE_NN, dt=dt, wrt=wrt)
    tape = run.tape
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    r = tape._rows
    a, b, pw = make_pairs(run, 90, 17)
    tape.set_row_pairs(a, b)
    ta, tb = to_tape(tape, a, b)
    vs = np.random.default_rng(19).standard_normal((tape.n_points, 4)).astype(dt)
    jvp_ref, vjp_ref = _restated_halves(run)
    first = True
    for rw in (run.rw, None):
        rw_t = None if rw is None else rw[r]
        # gauss_newton: both schedules, the hand composition, the restatement (once with the slowness half restated too)
        for schedule in SCHEDULES:
            g = tape.gauss_newton(run.v, rw, schedule=schedule, pair_weight=pw)
            assert isinstance(tape.passes, tuple) and min(tape.passes) >= 1 and g.dtype == dt
            _bits_equal(g, tape.vjp(tape.row_operator(tape.jvp(run.v, schedule=schedule), rw, pw), schedule=schedule))
        halves = (jvp_ref, vjp_ref) if first else (lambda v: tape.jvp(v)[r], lambda w: tape.vjp(_rows_to_data(run, w)))
        first = False
        _bits_equal(g, DD.gauss_newton(*halves, run.v, ta, tb, rw_t, pw))
        assert not np.array_equal(g, tape.gauss_newton(run.v, rw))
        for sc in (SCALE, None):
            # the source joint product
            for schedule in SCHEDULES:
                g, ge = tape.gauss_newton_joint(run.v, vs, row_weight=rw, source_scale=sc, schedule=schedule, pair_weight=pw)
                w = tape.row_operator(tape.jvp_joint(run.v, _scaled(sc, vs, dt), schedule=schedule), rw, pw)
                h, he = tape.vjp(w, return_source_grad=True, schedule=schedule)
                _bits_equal(g, h)
                _bits_equal(ge, _scaled(sc, he, dt))
            ref, ref_e = DD.joint_product(lambda v, ve: tape.jvp_joint(v, ve)[r],
                                          lambda w: tape.vjp(_rows_to_data(run, w), return_source_grad=True), run.v, vs, ta, tb, dt, rw_t, pw, sc)
            _bits_equal(g, ref)
            _bits_equal(ge, ref_e)
            # the receiver joint product
            for schedule in SCHEDULES:
                g, ge = tape.gauss_newton_receiver_joint(run.v, run.ve, row_weight=rw, rcv_scale=sc, schedule=schedule, pair_weight=pw)
                w = tape.row_operator(tape.jvp_joint_receiver(run.v, _scaled(sc, run.ve, dt), schedule=schedule), rw, pw)
                h, he = tape.vjp(w, return_receiver_grad=True, schedule=schedule)
                _bits_equal(g, h)
                _bits_equal(ge, _scaled(sc, he, dt))
            ref, ref_e = DD.receiver_joint_product(lambda v: tape.jvp(v)[r], lambda w: tape.vjp(_rows_to_data(run, w)), run.G[r], run.por[r],
                                                   run.n_rcv_points, run.v, run.ve, ta, tb, rw_t, pw, sc)
            _bits_equal(g, ref)
            _bits_equal(ge, ref_e)
            assert np.any(g != 0) and np.any(ge != 0)
    # newton after hold on two events: the two schedules agree, the Gauss-Newton rows follow the pairs
    tape.hold(run.w)
    n1 = tape.newton(run.v, run.rw, pair_weight=pw)
    _bits_equal(tape.newton(run.v, run.rw, schedule="jacobi", pair_weight=pw), n1)
    assert not np.array_equal(n1, tape.newton(run.v, run.rw))
    tape.free()


@DTYPES
def test_newton_with_pairs_is_the_composition(dt):
    """one event: newton(v, W, P) == vjp(B J v, field_cotangent=q) with r added at the nodes that are not frozen, q and r (the held part,
    untouched by the pairs) from the restatement on the device's field"""
    run = Run(nn=(9, 8, 10), dt=dt, n_events=1)
    tape, case = run.tape, run.case
    a, b, pw = make_pairs(run, 30, 23)
    tape.set_row_pairs(a, b)
    fr = AR.frozen_nodes(dt, case.nn, case.dx, case.origin, case.events[0]["pts"])
    _, lam, q, rr, _ = HR.product_event(run.fields[0], run.s, case.dx, case.nn, case.origin, fr, run.rcv, run.w, None, run.v)
    fz = np.zeros(run.s.size, dtype=bool)
    fz[list(fr)] = True
    tape.hold(run.w)
    dtt = tape.jvp(run.v)
    for rw in (run.rw, None):
        for schedule in SCHEDULES:
            comp = tape.vjp(tape.row_operator(dtt, rw, pw), q[None, :], schedule=schedule)
            comp[~fz] = (comp[~fz] + rr[~fz]).astype(dt)
            _bits_equal(tape.newton(run.v, rw, schedule=schedule, pair_weight=pw), comp)
    tape.release()
    with pytest.raises(ValueError):
        tape.newton(run.v, run.rw, pair_weight=pw)
    tape.free()


# ---- 3. the consequences
@DTYPES
def test_empty_pair_list_and_the_common_origin_time_shift(dt):
    run = Run(nn=(9, 8, 10), dt=dt)
    tape = run.tape
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    rng = np.random.default_rng(29)
    vs = rng.standard_normal((tape.n_points, 4)).astype(dt)
    rhs, rhs_s, rhs_r = run.v, vs[::-1].copy(), run.ve[::-1].copy()
    skw = dict(row_weight=run.rw, smooth=2e-2, smooth_weights=WEIGHTS, damp=1e-1, maxiter=3, return_info=True)
    tape.hold(run.w)
    calls = [lambda **k: (tape.gauss_newton(run.v, run.rw, **k),), lambda **k: (tape.newton(run.v, run.rw, **k),),
             lambda **k: tape.gauss_newton_joint(run.v, vs, run.rw, SCALE, **k),
             lambda **k: tape.gauss_newton_receiver_joint(run.v, run.ve, run.rw, SCALE, **k),
             lambda **k: tape.solve_normal(rhs, **skw, **k),
             lambda **k: tape.solve_joint(rhs, rhs_s, source_damp=SDAMP, source_scale=SCALE, **skw, **k),
             lambda **k: tape.solve_receiver_joint(rhs, rhs_r, rcv_damp=RDAMP, rcv_scale=SCALE, **skw, **k)]
    plain = [c() for c in calls]
    for c in calls:
        with pytest.raises(ValueError, match="no row pairs"):
            c(pair_weight=np.zeros(0, dtype=dt))
    tape.set_row_pairs([], [])
    assert tape.n_pairs == 0
    for c, want in zip(calls, plain):
        got = c(pair_weight=np.zeros(0, dtype=dt))
        for g, w in zip(got, want):
            if isinstance(w, dict):
                assert g == w
            else:
                _bits_equal(g, w)
    # one common dt0 on every receiver point, v = 0, all-zero row_weight: dtt == dt0 on every row, zeros throughout
    a, b, pw = make_pairs(run, 120, 31)
    tape.set_row_pairs(a, b)
    v_rcv = np.zeros((run.n_rcv_points, 4), dtype=dt)
    v_rcv[:, 0] = dt(0.3712)
    zero_v, zero_w = np.zeros(tape.n_cols, dtype=dt), np.zeros(tape.n_data, dtype=dt)
    assert np.array_equal(tape.jvp_joint_receiver(zero_v, v_rcv), np.full(tape.n_data, dt(0.3712)))
    for schedule in SCHEDULES:
        g, g_rcv = tape.gauss_newton_receiver_joint(zero_v, v_rcv, row_weight=zero_w, schedule=schedule, pair_weight=pw)
        assert g.shape == (tape.n_cols,) and g_rcv.shape == (run.n_rcv_points, 4) and not np.any(g) and not np.any(g_rcv)
    g, g_rcv = tape.gauss_newton_receiver_joint(zero_v, v_rcv, row_weight=run.rw, pair_weight=pw)   # (absolute data do see the shift)
    assert np.any(g != 0) and np.any(g_rcv != 0)
    tape.free()


# ---- 4. the solves
def _smooth_op(run):
    return lambda p: NR.smooth(p, run.params(), run.dx, WEIGHTS, dtype=run.dt)


def _same(got, ref):
    *xs, info = got
    *xr, inf_r = ref
    for g, w in zip(xs, xr):
        _bits_equal(g, w)
    assert info["status"] == inf_r["status"] and info["iterations"] == inf_r["iterations"], (info, inf_r)
    assert info["rho"] == inf_r["rho"] and info["pq"] == inf_r["pq"], (info, inf_r)
    assert len(info["passes"]) == len(info["pq"]) and all(min(p) >= 1 for p in info["passes"])


def _solve_and_reference(run, system, rhs, rhs_b, rw, pw, smooth, damp, bdamp, scale, maxiter, rtol=1e-6, schedule="tiled"):
    """(the device's solve, the restated recurrence around the device's own product with pairs)"""
    tape, dt = run.tape, run.dt
    kw = dict(smooth=smooth, smooth_weights=WEIGHTS, damp=damp, maxiter=maxiter, rtol=rtol, return_info=True)
    ref_kw = dict(smooth_op=_smooth_op(run), smooth=smooth, damp=damp, maxiter=maxiter, rtol=rtol)
    if system == "model":
        got = tape.solve_normal(rhs, row_weight=rw, pair_weight=pw, schedule=schedule, **kw)
        ref = NR.cg(lambda p: tape.gauss_newton(p, rw, pair_weight=pw), rhs, dt, **ref_kw)
    elif system == "joint":
        got = tape.solve_joint(rhs, rhs_b, row_weight=rw, pair_weight=pw, source_damp=bdamp, source_scale=scale, schedule=schedule, **kw)
        ref = JR.cg(lambda p, pe: tape.gauss_newton_joint(p, pe, row_weight=rw, source_scale=scale, pair_weight=pw), rhs, rhs_b, dt,
                    source_damp=bdamp, source_scale=scale, **ref_kw)
    else:
        got = tape.solve_receiver_joint(rhs, rhs_b, row_weight=rw, pair_weight=pw, rcv_damp=bdamp, rcv_scale=scale, schedule=schedule, **kw)
        ref = RR.cg(lambda p, pe: tape.gauss_newton_receiver_joint(p, pe, row_weight=rw, rcv_scale=scale, pair_weight=pw), rhs, rhs_b, dt,
                    rcv_damp=bdamp, rcv_scale=scale, **ref_kw)
    return got, ref


def _block_rhs(run, system, seed):
    n = {"model": 0, "joint": run.tape.n_points, "receiver_joint": run.n_rcv_points}[system]
    rng = np.random.default_rng(seed)
    return rng.standard_normal(run.tape.n_cols).astype(run.dt), rng.standard_normal((n, 4)).astype(run.dt)


@DTYPES
@pytest.mark.parametrize("system", ["model", "joint", "receiver_joint"])
def test_solves_with_pairs_bits(system, dt):
    run = Run(nn=SOLVE_NN, dt=dt)
    tape = run.tape
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    a, b, pw = make_pairs(run, 90, 37)
    tape.set_row_pairs(a, b)
    rhs, rhs_b = _block_rhs(run, system, 59)
    zero_w = np.zeros(tape.n_data, dtype=dt)
    for (smooth, damp), bdamp, scale, rw in (((2e-2, 1e-1), RDAMP, SCALE, run.rw), ((0.0, 1e-1), RDAMP, None, zero_w), ((2e-2, 0.0), 0.5, SCALE, None)):
        for maxiter in (1, 2, 3, 4):
            got, ref = _solve_and_reference(run, system, rhs, rhs_b, rw, pw, smooth, damp, bdamp, scale, maxiter)
            _same(got, ref)
            assert got[-1]["status"] == 1 and got[-1]["iterations"] == maxiter
        got, _ = _solve_and_reference(run, system, rhs, rhs_b, rw, pw, smooth, damp, bdamp, scale, 4, schedule="jacobi")
        _same(got, ref)
    assert not np.array_equal(got[0], tape.solve_normal(rhs, smooth=2e-2, smooth_weights=WEIGHTS, maxiter=4))
    tape.free()


@DTYPES
@pytest.mark.parametrize("nn", [(11, 31, 3), (16, 8, 8)], ids=["seam_inside_a_chunk", "seam_on_a_chunk_boundary"])
def test_joint_solves_with_pairs_block_seam(nn, dt):
    run = Run(nn=nn, dt=dt, n_events=1)
    tape = run.tape
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    assert tape.n_cols in (1023, 1024)
    a, b, pw = make_pairs(run, 20, 41)
    tape.set_row_pairs(a, b)
    for system, nb, bdamp in (("joint", tape.n_points, SDAMP), ("receiver_joint", run.n_rcv_points, RDAMP)):
        rhs = FC.wide_weights(np.random.default_rng(67), tape.n_cols, dt)
        rhs_b = FC.wide_weights(np.random.default_rng(68), 4 * nb, dt).reshape(-1, 4)
        for maxiter in (1, 4):
            got, ref = _solve_and_reference(run, system, rhs, rhs_b, run.rw, pw, 2e-2, 1e-1, bdamp, (1.0, 0.05, 0.05, 0.1), maxiter)
            _same(got, ref)
    tape.free()


@DTYPES
def test_solves_with_pairs_statuses(dt):
    run = Run(nn=SOLVE_NN, dt=dt)
    tape = run.tape
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    a, b, pw = make_pairs(run, 90, 43)
    tape.set_row_pairs(a, b)
    zero_w, zero_p = np.zeros(tape.n_data, dtype=dt), np.zeros(90, dtype=dt)
    for system in ("model", "joint", "receiver_joint"):
        rhs, rhs_b = _block_rhs(run, system, 61)
        got, ref = _solve_and_reference(run, system, rhs, rhs_b, zero_w, pw, 1e-3, 50.0, 50.0, SCALE, 30, rtol=1e-4)
        _same(got, ref)
        info = got[-1]
        assert info["status"] == 0 and 1 <= info["iterations"] < 30 and info["rho"][-1] <= 1e-8 * info["rho"][0]
        # all weights zero and no regularisation: <p, A p> = 0, no update, x stays zero
        got, _ = _solve_and_reference(run, system, rhs, rhs_b, zero_w, zero_p, 0.0, 0.0, 0.0, None, 4)
        info = got[-1]
        assert info["status"] == 2 and info["iterations"] == 0 and info["pq"] == [0.0] and len(info["rho"]) == 2
        assert all(not np.any(x) for x in got[:-1])
    tape.free()


# ---- 5. the other calls around the pair calls, and the host glue
@DTYPES
def test_other_calls_keep_their_bits_and_nbytes_and_the_glue(dt):
    from ttcr_amd.inversion import double_difference_step

    run = Run(nn=SOLVE_NN, dt=dt)
    tape = run.tape
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    rng = np.random.default_rng(79)
    rhs, rhs_r = _block_rhs(run, "receiver_joint", 79)
    rhs_s = rng.standard_normal((tape.n_points, 4)).astype(dt)
    nkw = dict(row_weight=run.rw, smooth=2e-2, smooth_weights=WEIGHTS, damp=1e-1, maxiter=3, return_info=True)
    others = [lambda: (tape.gauss_newton(run.v, run.rw),), lambda: tape.solve_normal(rhs, **nkw),
              lambda: tape.solve_joint(rhs, rhs_s, source_damp=SDAMP, source_scale=SCALE, **nkw),
              lambda: tape.solve_receiver_joint(rhs, rhs_r, rcv_damp=RDAMP, rcv_scale=SCALE, **nkw)]
    first = [c() for c in others]
    before = tape.nbytes
    n, elem, m = tape.n_rows, np.dtype(dt).itemsize, 90
    a, b, pw = make_pairs(run, m, 47)
    tape.set_row_pairs(a, b)
    assert tape.nbytes == before
    dd_bytes = 2 * 4 * m + 4 * (n + 1) + 8 * m + 2 * m * elem + n * elem
    g = tape.gauss_newton(run.v, run.rw, pair_weight=pw)
    assert tape.nbytes == before + dd_bytes
    for c in (lambda: tape.solve_normal(rhs, pair_weight=pw, **nkw), lambda: tape.solve_receiver_joint(rhs, rhs_r, pair_weight=pw, **nkw)):
        c()
        assert tape.nbytes == before + dd_bytes
    for c, want in zip(others, first):
        got = c()
        for x, y in zip(got, want):
            if isinstance(y, dict):
                assert x == y
            else:
                _bits_equal(x, y)
        assert tape.nbytes == before + dd_bytes
    tape.release_pairs()
    assert tape.nbytes == before
    _bits_equal(tape.gauss_newton(run.v, run.rw, pair_weight=pw), g)
    assert tape.nbytes == before + dd_bytes
    # the host glue: double_difference_step equal to the calls composed by hand, mixed weights and pure double-difference data
    residual = (1e-2 * rng.standard_normal(tape.n_data)).astype(dt)
    pres = (1e-3 * rng.standard_normal(m)).astype(dt)
    model = rng.uniform(0.4, 0.7, tape.n_cols).astype(dt)
    kw = dict(smooth=dt(2e-2), smooth_weights=WEIGHTS, damp=dt(1e-1), maxiter=3, return_info=True)
    w = (run.rw * residual + tape.pair_adjoint(pw * pres)).astype(dt)
    smooth_term = dt(2e-2) * tape.smooth(model, WEIGHTS)
    want = tape.solve_normal(tape.vjp(w) - smooth_term, row_weight=run.rw, pair_weight=pw, **kw)
    _same(double_difference_step(tape, residual, pres, model, row_weight=run.rw, pair_weight=pw, **kw), want)
    w = tape.pair_adjoint(pres)
    zero_w = np.zeros(tape.n_data, dtype=dt)
    ones = np.ones(m, dtype=dt)
    bs, bb = tape.vjp(w, return_source_grad=True)
    want = tape.solve_joint(bs - smooth_term, bb, row_weight=zero_w, pair_weight=ones, source_damp=SDAMP, source_scale=SCALE, **kw)
    _same(double_difference_step(tape, None, pres, model, system="joint", block_damp=SDAMP, block_scale=SCALE, **kw), want)
    bs, bb = tape.vjp(w, return_receiver_grad=True)
    want = tape.solve_receiver_joint(bs - smooth_term, bb, row_weight=zero_w, pair_weight=ones, rcv_damp=RDAMP, rcv_scale=SCALE, **kw)
    got = double_difference_step(tape, None, pres, model, system="receiver_joint", block_damp=RDAMP, block_scale=SCALE, **kw)
    _same(got, want)
    assert np.any(got[0] != 0) and np.any(got[1] != 0)
    tape.free()


# ---- 6. device tensors (a child process)
def _torch_tensors(dtname):
    import torch

    dt = np.dtype(dtname).type
    run = Run(nn=(9, 8, 10), dt=dt)
    tape = run.tape
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    a, b, pw = make_pairs(run, 70, 53)
    tape.set_row_pairs(torch.as_tensor(a), torch.as_tensor(b))
    dev = lambda x: torch.as_tensor(x, device="cuda")   # noqa: E731
    rng = np.random.default_rng(83)
    x, y = FC.wide_weights(rng, tape.n_data, dt), FC.wide_weights(rng, 70, dt)
    for got, want in ((tape.pair_difference(dev(x)), tape.pair_difference(x)), (tape.pair_adjoint(dev(y)), tape.pair_adjoint(y)),
                      (tape.row_operator(dev(x), dev(run.rw), dev(pw)), tape.row_operator(x, run.rw, pw)),
                      (tape.row_operator(dev(x)), tape.row_operator(x)),
                      (tape.gauss_newton(dev(run.v), dev(run.rw), pair_weight=dev(pw)), tape.gauss_newton(run.v, run.rw, pair_weight=pw))):
        assert got.is_cuda
        _bits_equal(got.cpu().numpy(), want)
    ref = tape.gauss_newton_receiver_joint(run.v, run.ve, run.rw, SCALE, pair_weight=pw)
    t_pw = dev(pw)
    g, ge = tape.gauss_newton_receiver_joint(dev(run.v), dev(run.ve), dev(run.rw), SCALE, pair_weight=t_pw)
    assert g.is_cuda and ge.is_cuda
    _bits_equal(g.cpu().numpy(), ref[0])
    _bits_equal(ge.cpu().numpy(), ref[1])
    _bits_equal(t_pw.cpu().numpy(), pw)                    # (the arguments are read, not used as work arrays)
    rhs, rhs_e = _block_rhs(run, "receiver_joint", 71)
    kw = dict(smooth=2e-2, smooth_weights=WEIGHTS, damp=1e-1, rcv_damp=RDAMP, rcv_scale=SCALE, maxiter=3, return_info=True)
    ref = tape.solve_receiver_joint(rhs, rhs_e, row_weight=run.rw, pair_weight=pw, **kw)
    xs, xe, info = tape.solve_receiver_joint(dev(rhs), dev(rhs_e), row_weight=dev(run.rw), pair_weight=dev(pw), **kw)
    assert xs.is_cuda and xe.is_cuda and info == ref[2]
    _bits_equal(xs.cpu().numpy(), ref[0])
    _bits_equal(xe.cpu().numpy(), ref[1])
    bad = dev(pw).clone()
    bad[3] = -1.0
    try:
        tape.gauss_newton(dev(run.v), pair_weight=bad)
    except ValueError as e:
        assert "pair_weight" in str(e)
    else:
        raise AssertionError("no ValueError")


@DTYPES
def test_pair_calls_with_device_tensors(dt):
    _in_child("tensors", np.dtype(dt).name)
