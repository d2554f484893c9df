"""The receiver-point derivatives and the receiver joint system of the field tape on the device (FieldTape.receiver_eval,
receiver_jacobian, set_receiver_points, jvp_receiver, vjp(..., return_receiver_grad=True), jvp_joint_receiver,
gauss_newton_receiver_joint, solve_receiver_joint, release_receiver, inversion.reciprocal_gauss_newton_step and the torch operators'
derivative in rcv).  Every comparison is to the bit, against the numpy restatement of tests/receiver_reference.py run on the
device's own fields, for fp32 and fp64 and, where a relaxation is involved, under both schedules.  The grids are small: what can go wrong
are the on-plane branches, the clamp at the last planes, the map from rows to points and the seam between the two blocks of the joint
vector."""
import ctypes as C
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
import cell_reference as CR  # noqa: E402
import field_tape_cases as FC  # noqa: E402
import normal_reference as NR  # noqa: E402
import receiver_reference as RR  # noqa: E402
import tangent_reference as TR  # noqa: E402
from field_tape_cases import _bits_equal  # noqa: E402

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
SCHEDULES = ("tiled", "jacobi")
SOLVE_NN = (17, 14, 19)
WEIGHTS = (1.0, 0.5, 2.0)
SCALE = (1.0, 0.05, 0.0, 0.1)          # one entry 0: that coordinate of every point is fixed
RDAMP = (1e-2, 1e-1, 1.0, 1e-1)
ORIGIN = (-37.25, 1200.5, -3.125)


def _in_child(fn, *args):
    """Run _torch_<fn>(*args) of this module in a fresh process that initialises torch's device before the first grid"""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_receiver_derivative_gpu as t; t._torch_%s(*%r)"
            % (HERE, ROOT, fn, args))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def hypocentres(nn, dx, origin, dt, rng, n_generic=4):
    """the receiver points of a case, as values of the grid dtype: generic points, points on one, two and three planes, on the far faces,
    in the last cell of the far corner and one rounding error below the last plane of every axis (the clamp)"""
    hi = [n - 1 for n in nn]
    c = [h // 3 for h in hi]
    f = [min(c[a] + 0.6, hi[a] - 0.4) for a in range(3)]
    idx = [[f[0], f[1], f[2]], [c[0], f[1], f[2]], [f[0], c[1], f[2]], [f[0], f[1], c[2]], [c[0], c[1], f[2]], [c[0], f[1], c[2]],
           [f[0], c[1], c[2]], [c[0], c[1], c[2]], [hi[0], f[1], f[2]], [f[0], hi[1], hi[2]], hi, [0, 0, 0],
           [hi[a] - (0.7, 0.4, 0.8)[a] for a in range(3)]]
    pts = np.vstack([FC.at(nn, dx, origin, idx), FC.random_receivers(nn, dx, origin, rng, n_generic)]).astype(dt)
    last = FC.at(nn, dx, origin, hi).astype(dt)
    # one rounding error below the last plane, in the grid dtype.  The lower index becomes the last node without the point being on
    # the plane (the clamp) where the distance is above the 1e-8 plane tolerance and the quotient still reaches the last index: for
    # dx > 1 in fp64 a distance of 1e-7, in fp32 one ulp of a coordinate that is small against its distance to the origin
    below = np.nextafter(last, dt(-np.inf)) if dt == np.float32 or dx <= 1 else last - dt(1e-7)
    clamp = np.tile(FC.at(nn, dx, origin, f).astype(dt), (4, 1))
    for a in range(3):
        clamp[a, a] = below[a]
    clamp[3] = below
    return np.vstack([pts, clamp]).astype(np.float64)              # (exact: every value is one of the grid dtype)


class Run:
    """one raytrace_adjoint call in the reciprocal layout: every event (a station) sees the same receiver points (the hypocentres), event
    0 one point more that no other event sees; one further receiver point has no row at all"""

    def __init__(self, nn, dt, wrt="nodes", n_events=2, origin=FC.ZERO, translate=False, n_threads=1, dx=FC.DX, scale=1.0):
        import ttcr_amd
        from oracle import oracle as O

        self.nn, self.dt, self.wrt, self.dx, self.origin, self.translate = nn, dt, wrt, dx, origin, translate
        rng = np.random.default_rng(sum(nn) + n_events)
        hyp = hypocentres(nn, dx, origin, dt, rng)
        lone = FC.random_receivers(nn, dx, origin, rng, 1).astype(dt).astype(np.float64)
        hi = np.array(nn) - 1.0
        srcs = [[np.floor(0.4 * (nn[a] - 1)) + (0.3, 0.6, 0.2)[a] for a in range(3)], [nn[a] - 1 - (0.7, 0.4, 0.8)[a] for a in range(3)]]
        srcs += [list(rng.uniform(0.2, hi - 0.2)) for _ in range(n_events - 2)]
        events = [FC._event(FC.at(nn, dx, origin, [srcs[e]]), np.vstack([hyp, lone]) if e == 0 else hyp, 0.125 * e)
                  for e in range(n_events)]
        self.case = FC.Case("reciprocal", nn, dx, origin, FC.model(nn, dx, origin, "rough", scale), events)
        self.src, self.rcv, agg, self.rows = FC.call_arrays(self.case, np.random.default_rng(61))
        self.n_hyp = hyp.shape[0]
        # the point of every data row: hypocentre k for every event, the lone point, and one point more that has no row
        point = np.concatenate([np.concatenate([np.arange(self.n_hyp), [self.n_hyp]]) if e == 0 else np.arange(self.n_hyp)
                                for e in range(n_events)])
        # (call_arrays deals the rows of several events with the first permutation of its generator)
        self.por = point[np.random.default_rng(61).permutation(point.size)] if n_events > 1 else point
        first = {}
        for r, q in enumerate(self.por):   # rows that share a point hold the same receiver, to the bit
            assert np.array_equal(self.rcv[first.setdefault(int(q), r)], self.rcv[r])
        self.n_rcv_points = self.n_hyp + 2
        self.event_of_row = np.zeros(self.rcv.shape[0], dtype=np.int64)
        for e, r in enumerate(self.rows):
            self.event_of_row[r] = e
        axes = [origin[a] + np.arange(nn[a]) * dx for a in range(3)]
        self.nc = tuple(n - 1 for n in nn)
        cells = wrt == "cells"
        self.grid = ttcr_amd.Grid3d(*axes, n_threads=n_threads, cell_slowness=1 if cells else 0, method="FSM", dtype=dt, weno=0,
                                    tt_from_rp=0, translate_grid=translate)
        if cells:
            sc = np.random.default_rng(67).uniform(0.4, 0.7, int(np.prod(self.nc))).astype(dt)
            self.grid.set_slowness(sc.reshape(self.nc, order="F"))
            self.s = O.cells_to_nodes3d(dt, self.nc, sc)
            self.to_nodes = lambda v: O.cells_to_nodes3d(dt, self.nc, np.asarray(v, dtype=dt))
        else:
            self.grid.set_slowness(self.case.s.reshape(nn, order="F"))
            self.s = np.asarray(self.case.s, dtype=dt)
            self.to_nodes = lambda v: np.asarray(v, dtype=dt)
        self.tt, self.tape = self.grid.raytrace_adjoint(self.src, self.rcv, aggregate_src=agg, wrt=wrt)
        t = self.tape
        assert t.n_events == n_events and t.n_rows == t.n_data == self.rcv.shape[0]
        assert np.array_equal(t._rows, np.concatenate(self.rows))           # tape row order: the events in turn, rcv order within one
        self.fields = [t.field(e) for e in range(n_events)]
        # what the solver sees: the origin of a translated grid subtracted in the grid dtype, and interpolation from zero
        o = np.asarray(origin, dtype=dt)
        self.seen = (self.rcv.astype(dt) - o).astype(dt) if translate else self.rcv.astype(dt)
        self.mn = FC.ZERO if translate else origin
        rng = np.random.default_rng(71)
        self.v = (rng.uniform(0.4, 0.7, t.n_cols) * rng.standard_normal(t.n_cols)).astype(dt)
        self.ve = rng.standard_normal((self.n_rcv_points, 4)).astype(dt)
        self.w = FC.wide_weights(rng, self.rcv.shape[0], dt)
        self.rw = rng.uniform(0.5, 2.0, self.rcv.shape[0]).astype(dt)
        self.ref_tt, self.G = RR.evaluate_points(self.fields, nn, self.dx, self.mn, self.seen, self.event_of_row)   # data row order

    # the restated halves in tape row order (data rows of the tape rows: tape._rows)
    def fwd(self, drcv):
        r = self.tape._rows
        out = np.zeros(self.rcv.shape[0], dtype=self.dt)
        out[r] = RR.forward(self.G[r], self.por[r], drcv)
        return out

    def rev(self, w):
        r = self.tape._rows
        return RR.reverse(self.G[r], self.por[r], self.n_rcv_points, np.asarray(w, dtype=self.dt)[r])

    def params(self):
        return self.nc if self.wrt == "cells" else self.nn


CASES = {
    "2x2x2": dict(nn=(2, 2, 2)),
    "17x14x19": dict(nn=SOLVE_NN),
    "edge": dict(nn=None),                   # one axis of 2 edge + 1 of the tangent tile (10 / 8), a receiver in the last cell of the far corner
    "origin": dict(nn=(9, 8, 10), origin=ORIGIN),
    "translated": dict(nn=(9, 8, 10), origin=ORIGIN, translate=True),
    "one_event": dict(nn=(9, 8, 10), n_events=1),
    "clamp": dict(nn=(9, 8, 10), n_events=1, origin=(-175.0, 2000.0, -500.0), dx=25.0, scale=1e-3),   # metres: see hypocentres
    "cells": dict(nn=(9, 8, 10), wrt="cells"),
    "five_events_1": dict(nn=(9, 8, 10), n_events=5, n_threads=1),
    "five_events_4": dict(nn=(9, 8, 10), n_events=5, n_threads=4),
}


# ---- 1. evaluation, rows and chains
@DTYPES
@pytest.mark.parametrize("name", sorted(CASES))
def test_receiver_rows_bits(name, dt):
    kw = dict(CASES[name])
    if name == "edge":
        e = FC.TAN_EDGE[np.dtype(dt)]
        kw["nn"] = (e + 1, 2 * e + 1, e + 1)
    run = Run(dt=dt, **kw)
    tape, n = run.tape, run.rcv.shape[0]
    assert tape.n_rcv_points == n and np.array_equal(tape.rcv_point_of_row[tape._rows], np.arange(n))   # the default: a point per row
    before = tape.nbytes
    # receiver_eval at the tape's own receivers: the call's traveltimes, the restated gradient
    _bits_equal(run.ref_tt, run.tt)
    tt, G = tape.receiver_eval(run.rcv.astype(dt), run.event_of_row)
    elem = np.dtype(dt).itemsize
    stage = 7 * n * elem + 4 * n                              # points, gradients, traveltimes, events: one buffer that only grows
    assert tape.nbytes == before + stage                      # (arbitrary points need nothing of the tape's receiver arrays)
    assert tt.dtype == dt and G.dtype == dt and G.shape == (n, 3)
    _bits_equal(tt, run.tt)
    _bits_equal(G, run.G)
    _bits_equal(tape.receiver_eval(run.rcv.astype(dt), run.event_of_row, return_grad=False), run.tt)
    tape.receiver_eval(run.rcv.astype(dt)[:3], run.event_of_row[:3])
    assert tape.nbytes == before + stage                      # (a smaller call: the same buffer)
    on = np.array([RR.axis_terms(dt, run.nn, run.dx, run.mn, p)[1] for p in run.seen])
    assert np.all(run.G[on] == 0) and not np.any(np.signbit(run.G[on])) and on.sum(axis=1).max() == 3 and np.any(on.sum(axis=1) == 0)
    if name == "clamp":                                       # the lower index is the last node, the point is not on its plane: G is +0
        lo = np.array([RR.axis_terms(dt, run.nn, run.dx, run.mn, p)[0] for p in run.seen])
        clamped = (lo == np.array(run.nn) - 1) & ~on
        assert clamped[:, 0].any() and np.all(run.G[clamped] == 0) and not np.any(np.signbit(run.G[clamped]))
    if tape.n_events == 1:                                    # the grid's own interpolation of the field it still holds
        out = np.empty(n, dtype=dt)
        pts = np.ascontiguousarray(run.rcv, dtype=dt)
        assert run.grid._lib.ttcr_fsm_interp(run.grid._h, 0, n, pts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
        _bits_equal(tt, out)
    # receiver_jacobian: the same values, kept on the tape; three unit jvp_receiver calls give its columns
    J = tape.receiver_jacobian()
    _bits_equal(J, run.G)
    assert tape.nbytes == before + stage + 7 * n * elem + 3 * n * 4 + (n + 1) * 4 + 16 * n * elem
    for a in range(3):
        unit = np.zeros((n, 4), dtype=dt)
        unit[:, 1 + a] = 1
        col = tape.jvp_receiver(unit)                         # (default map: point q is tape row q)
        assert np.array_equal(col[tape._rows], J[tape._rows, a])
    # the reciprocal map
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    assert tape.nbytes == before and tape.n_rcv_points == run.n_rcv_points and np.array_equal(tape.rcv_point_of_row, run.por)
    dtt = tape.jvp_receiver(run.ve)
    assert dtt.dtype == dt and dtt.shape == (n,)
    _bits_equal(dtt, run.fwd(run.ve))
    _bits_equal(tape.receiver_jacobian(), run.G)
    # reverse: with vjp's gradient bits, and composed with the source gradient
    g_ref = tape.vjp(run.w)
    g, grcv = tape.vjp(run.w, return_receiver_grad=True)
    _bits_equal(g, g_ref)
    ref = run.rev(run.w)
    assert grcv.dtype == dt and grcv.shape == (run.n_rcv_points, 4)
    _bits_equal(grcv, ref)
    assert not np.any(grcv[-1]) and not np.any(np.signbit(grcv[-1]))             # the point without rows: +0
    lone = np.nonzero(run.por == run.n_hyp)[0]
    assert lone.size == 1 and grcv[run.n_hyp, 0] == run.w[lone[0]]               # the point with one row
    for q in range(run.n_rcv_points):                                            # t0: the sums of w in tape row order
        acc = dt(0)
        for r in tape._rows:
            if run.por[r] == q:
                acc = dt(acc + run.w[r])
        assert grcv[q, 0] == acc
    g3 = tape.vjp(run.w, return_source_grad=True, return_receiver_grad=True)
    g2 = tape.vjp(run.w, return_source_grad=True)
    assert len(g3) == 3
    _bits_equal(g3[0], g2[0])
    _bits_equal(g3[1], g2[1])
    _bits_equal(g3[2], ref)
    fc = np.random.default_rng(3).standard_normal((tape.n_events, tape.n_nodes)).astype(dt)
    gf, zero = tape.vjp(None, fc, return_receiver_grad=True)                     # no w: nothing reaches the receivers
    _bits_equal(gf, tape.vjp(None, fc))
    assert zero.shape == (run.n_rcv_points, 4) and not np.any(zero)
    # the joint tangent
    zero_v, zero_e = np.zeros_like(run.v), np.zeros_like(run.ve)
    for schedule in SCHEDULES:
        j, mu = tape.jvp(run.v, return_fields=True, schedule=schedule)
        both, mu2 = tape.jvp_joint_receiver(run.v, run.ve, return_fields=True, schedule=schedule)
        ref = np.zeros(n, dtype=dt)
        ref[tape._rows] = RR.joint_tangent(j[tape._rows], run.G[tape._rows], run.por[tape._rows], run.ve)
        _bits_equal(both, ref)
        _bits_equal(mu2, mu)
        _bits_equal(tape.jvp_joint_receiver(run.v, run.ve, schedule=schedule), ref)
        assert np.array_equal(tape.jvp_joint_receiver(run.v, zero_e, schedule=schedule), j)
        assert np.array_equal(tape.jvp_joint_receiver(zero_v, run.ve, schedule=schedule), dtt)
    # rows that share a point have to hold the same receiver
    bad = run.por.copy()
    r0, r1 = int(tape._rows[0]), int(tape._rows[1])
    bad[r1] = bad[r0]
    with pytest.raises(ValueError, match="data rows %d and %d share" % (r0, r1)):
        tape.set_receiver_points(bad)
    assert tape.n_rcv_points == run.n_rcv_points and np.array_equal(tape.rcv_point_of_row, run.por)   # (nothing changed)
    held = tape.nbytes                                        # (the jvp and the source gradient have allocated their own by now)
    tape.release_receiver()
    assert tape.nbytes == held - (7 * n * elem + 3 * n * 4 + (run.n_rcv_points + 1) * 4 + 16 * run.n_rcv_points * elem)
    tape.release_receiver()                                   # (a second release is a no-op)
    assert tape.nbytes == held - (7 * n * elem + 3 * n * 4 + (run.n_rcv_points + 1) * 4 + 16 * run.n_rcv_points * elem)
    _bits_equal(tape.jvp_receiver(run.ve), dtt)
    assert tape.nbytes == held
    tape.free()


@DTYPES
def test_receiver_eval_at_other_points(dt):
    """arbitrary points inside the grid, in any event's field, on a translated grid: the grid's own interpolation and the restatement"""
    run = Run(nn=(9, 8, 10), dt=dt, origin=ORIGIN, translate=True, n_events=1)
    tape = run.tape
    rng = np.random.default_rng(7)
    pts = np.vstack([FC.random_receivers(run.nn, run.dx, ORIGIN, rng, 300), hypocentres(run.nn, run.dx, ORIGIN, dt, rng)]).astype(dt)
    ev = np.zeros(len(pts), dtype=np.int64)
    tt, G = tape.receiver_eval(pts, ev)
    seen = (pts - np.asarray(ORIGIN, dtype=dt)).astype(dt)
    ref_tt, ref_G = RR.evaluate_points(run.fields, run.nn, run.dx, FC.ZERO, seen, ev)
    _bits_equal(tt, ref_tt)
    _bits_equal(G, ref_G)
    out = np.empty(len(pts), dtype=dt)
    assert run.grid._lib.ttcr_fsm_interp(run.grid._h, 0, len(pts), pts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
    _bits_equal(tt, out)
    e0 = tape.receiver_eval(pts[:0], ev[:0])
    assert e0[0].shape == (0,) and e0[1].shape == (0, 3)
    with pytest.raises(ValueError, match="event_of_pt"):
        tape.receiver_eval(pts, ev + 1)
    tape.free()


# ---- 2. the product
def _restated_halves(run):
    """(jvp, vjp) of the slowness half restated on the device's fields, in tape row order"""
    case, dt = run.case, run.dt
    assert not run.translate
    rcvs = [run.rcv[r] for r in run.rows]
    geo = (run.s, run.dx, run.nn, run.mn, [e["pts"] for e in case.events])

    def jvp(v):
        _, dtts = TR.tangent(run.fields, *geo, run.to_nodes(v), rcvs=rcvs)
        return np.concatenate(dtts)

    def vjp(w):
        ws, k = [], 0
        for r in run.rows:
            ws.append(w[k:k + len(r)])
            k += len(r)
        g = AR.adjoint(run.fields, *geo, rcvs=rcvs, ws=ws)
        return CR.nodes_to_cells(dt, run.nc, g) if run.wrt == "cells" else g
    return jvp, vjp


@DTYPES
@pytest.mark.parametrize("wrt", ["nodes", "cells"])
def test_gauss_newton_receiver_joint_bits(wrt, dt):
    run = Run(nn=SOLVE_NN, dt=dt, wrt=wrt)
    tape = run.tape
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    r = tape._rows
    per_point = np.tile(np.array(SCALE, dtype=dt), (run.n_rcv_points, 1))
    per_point[1] = per_point[1][::-1]
    per_point[2, 0] = 0
    jvp_ref, vjp_ref = _restated_halves(run)
    first = True
    for rw in (run.rw, None):
        for sc in (per_point, SCALE, None):
            for schedule in SCHEDULES:
                g, ge = tape.gauss_newton_receiver_joint(run.v, run.ve, row_weight=rw, rcv_scale=sc, schedule=schedule)
                assert isinstance(tape.passes, tuple) and min(tape.passes) >= 1 and g.dtype == dt and ge.dtype == dt
                if schedule == "tiled":
                    g0, ge0 = g, ge
                _bits_equal(g, g0)
                _bits_equal(ge, ge0)
            assert np.any(g != 0) and np.any(ge != 0) and ge.shape == (run.n_rcv_points, 4)
            if sc is not None:
                assert np.all(ge[np.broadcast_to(np.asarray(sc), ge.shape) == 0] == 0)
            # the restatement: the slowness half restated too (once: it is the slow part), else the device's own jvp and vjp
            halves = (jvp_ref, vjp_ref) if first else (lambda v: tape.jvp(v)[r], lambda w: tape.vjp(_rows_to_data(run, w)))
            first = False
            ref, ref_e = RR.joint_product(*halves, run.G[r], run.por[r], run.n_rcv_points, run.v, run.ve,
                                          row_weight=None if rw is None else rw[r], rcv_scale=sc)
            _bits_equal(g, ref)
            _bits_equal(ge, ref_e)
            # ... and the calls it replaces, composed by hand
            ve = run.ve if sc is None else (np.broadcast_to(np.asarray(sc, dtype=dt), run.ve.shape) * run.ve).astype(dt)
            dtt = tape.jvp_joint_receiver(run.v, ve)
            h, he = tape.vjp(dtt if rw is None else (rw * dtt).astype(dt), return_receiver_grad=True)
            _bits_equal(g, h)
            _bits_equal(ge, he if sc is None else (np.broadcast_to(np.asarray(sc, dtype=dt), he.shape) * he).astype(dt))
    tape.free()


def _rows_to_data(run, w_tape):
    w = np.zeros(run.rcv.shape[0], dtype=run.dt)
    w[run.tape._rows] = w_tape
    return w


# ---- 3. the solve
def _reference(run, rhs, rhs_e, rw, smooth, damp, rdamp, scale, maxiter, rtol=1e-6, schedule="tiled"):
    tape, dt = run.tape, run.dt
    return RR.cg(lambda ps, pe: tape.gauss_newton_receiver_joint(ps, pe, row_weight=rw, rcv_scale=scale, schedule=schedule), rhs, rhs_e, dt,
                 smooth_op=lambda p: NR.smooth(p, run.params(), run.dx, WEIGHTS, dtype=dt), smooth=smooth, damp=damp,
                 rcv_damp=rdamp, rcv_scale=scale, maxiter=maxiter, rtol=rtol)


def _same(got, ref):
    x, xe, info = got
    xr, xer, inf_r = ref
    _bits_equal(x, xr)
    _bits_equal(xe, xer)
    assert info["status"] == inf_r["status"] and info["iterations"] == inf_r["iterations"], (info, inf_r)
    assert info["rho"] == inf_r["rho"] and info["pq"] == inf_r["pq"], (info, inf_r)
    assert len(info["passes"]) == len(info["pq"]) and all(min(p) >= 1 for p in info["passes"])


def _rhs(run, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(run.tape.n_cols).astype(run.dt), rng.standard_normal((run.n_rcv_points, 4)).astype(run.dt)


@DTYPES
@pytest.mark.parametrize("wrt", ["nodes", "cells"])
def test_solve_receiver_joint_bits(wrt, dt):
    run = Run(nn=SOLVE_NN, dt=dt, wrt=wrt)
    tape = run.tape
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    rhs, rhs_e = _rhs(run, 59)
    for (smooth, damp), rdamp, scale, rw in (((2e-2, 1e-1), RDAMP, SCALE, run.rw), ((0.0, 0.0), 0.0, None, None), ((2e-2, 0.0), 0.5, None, run.rw),
                                             ((0.0, 1e-1), 0.0, SCALE, None)):
        kw = dict(smooth=smooth, smooth_weights=WEIGHTS, damp=damp, return_info=True)
        for maxiter in (1, 2, 3, 4):
            ref = _reference(run, rhs, rhs_e, rw, smooth, damp, rdamp, scale, maxiter)
            got = tape.solve_receiver_joint(rhs, rhs_e, row_weight=rw, rcv_damp=rdamp, rcv_scale=scale, maxiter=maxiter, **kw)
            _same(got, ref)
            assert got[2]["status"] == 1 and got[2]["iterations"] == maxiter and got[1].shape == (run.n_rcv_points, 4)
            if scale is not None:
                assert np.all(got[1][:, 2] == 0) and np.any(got[1][:, :2] != 0)
        _same(tape.solve_receiver_joint(rhs, rhs_e, row_weight=rw, rcv_damp=rdamp, rcv_scale=scale, maxiter=4, schedule="jacobi", **kw), ref)
    tape.free()


@DTYPES
@pytest.mark.parametrize("nn", [(11, 31, 3), (16, 8, 8)], ids=["seam_inside_a_chunk", "seam_on_a_chunk_boundary"])
def test_solve_receiver_joint_block_seam(nn, dt):
    run = Run(nn=nn, dt=dt, n_events=1)
    tape = run.tape
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    assert tape.n_cols in (1023, 1024) and (tape.n_cols + 4 * run.n_rcv_points) // 1024 == 1
    rhs = FC.wide_weights(np.random.default_rng(67), tape.n_cols, dt)
    rhs_e = FC.wide_weights(np.random.default_rng(68), 4 * run.n_rcv_points, dt).reshape(-1, 4)
    for maxiter in (1, 4):
        got = tape.solve_receiver_joint(rhs, rhs_e, row_weight=run.rw, smooth=2e-2, smooth_weights=WEIGHTS, damp=1e-1, rcv_damp=RDAMP,
                                        rcv_scale=(1.0, 0.05, 0.05, 0.1), maxiter=maxiter, return_info=True)
        _same(got, _reference(run, rhs, rhs_e, run.rw, 2e-2, 1e-1, RDAMP, (1.0, 0.05, 0.05, 0.1), maxiter))
    tape.free()


@DTYPES
def test_solve_receiver_joint_statuses_and_the_all_zero_scale(dt):
    run = Run(nn=SOLVE_NN, dt=dt)
    tape = run.tape
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    rhs, rhs_e = _rhs(run, 61)
    kw = dict(smooth=1e-3, smooth_weights=WEIGHTS, damp=50.0, rcv_damp=50.0, rcv_scale=SCALE, maxiter=30, rtol=1e-4)
    got = tape.solve_receiver_joint(rhs, rhs_e, return_info=True, **kw)
    _same(got, _reference(run, rhs, rhs_e, None, 1e-3, 50.0, 50.0, SCALE, 30, rtol=1e-4))
    info = got[2]
    assert info["status"] == 0 and 1 <= info["iterations"] < 30 and info["rho"][-1] <= 1e-8 * info["rho"][0]
    # row_weight = 0 and no regularisation: <p, A p> = 0, no update, x stays zero
    zero = np.zeros(tape.n_data, dtype=dt)
    x, xe, info = tape.solve_receiver_joint(rhs, rhs_e, row_weight=zero, maxiter=4, return_info=True)
    assert info["status"] == 2 and info["iterations"] == 0 and info["pq"] == [0.0] and len(info["rho"]) == 2
    assert not np.any(x) and not np.any(xe)
    # rcv_scale all zeros: the slowness block is solve_normal's, element for element
    for rw in (None, run.rw):
        for rdamp in (0.0, RDAMP):
            x, xe, info = tape.solve_receiver_joint(rhs, rhs_e, row_weight=rw, smooth=2e-2, smooth_weights=WEIGHTS, damp=1e-1, rcv_damp=rdamp,
                                                    rcv_scale=(0.0, 0.0, 0.0, 0.0), maxiter=4, return_info=True)
            xn, info_n = tape.solve_normal(rhs, row_weight=rw, smooth=2e-2, smooth_weights=WEIGHTS, damp=1e-1, maxiter=4, return_info=True)
            assert not np.any(xe) and np.array_equal(x, xn) and np.any(xn != 0)
            assert info["rho"] == info_n["rho"] and info["pq"] == info_n["pq"] and info["iterations"] == info_n["iterations"] == 4
    with pytest.raises(ValueError, match="hessian"):
        tape.solve_receiver_joint(rhs, rhs_e, hessian="newton")
    tape.free()


@DTYPES
@pytest.mark.parametrize("wrt", ["nodes", "cells"])
def test_nbytes_and_the_other_solvers_unchanged(wrt, dt):
    from ttcr_amd.inversion import reciprocal_gauss_newton_step

    run = Run(nn=SOLVE_NN, dt=dt, wrt=wrt)
    tape = run.tape
    rng = np.random.default_rng(79)
    rhs, rhs_e = _rhs(run, 79)
    rhs_src = rng.standard_normal((tape.n_points, 4)).astype(dt)
    nkw = dict(smooth=2e-2, smooth_weights=WEIGHTS, damp=1e-1, maxiter=3, return_info=True)
    jkw = dict(row_weight=run.rw, source_damp=RDAMP, source_scale=SCALE, **nkw)
    xn, info_n = tape.solve_normal(rhs, row_weight=run.rw, **nkw)
    xj, xje, info_j = tape.solve_joint(rhs, rhs_src, **jkw)
    before = tape.nbytes
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    assert tape.nbytes == before                               # (the map is on the host until the first receiver call)
    n, npts, elem = tape.n_rows, run.n_rcv_points, np.dtype(dt).itemsize
    rcv_bytes = 7 * n * elem + 3 * n * 4 + (npts + 1) * 4 + 16 * npts * elem
    tape.jvp_receiver(run.ve)
    assert tape.nbytes == before + rcv_bytes
    kw = dict(row_weight=run.rw, rcv_damp=RDAMP, rcv_scale=SCALE, **nkw)
    x, xe, info = tape.solve_receiver_joint(rhs, rhs_e, **kw)
    n_joint = tape.n_cols + 4 * npts
    solver_bytes = 5 * n_joint * elem + 3 * 4 * npts * elem + 8 * -(-n_joint // 1024) + 48
    assert tape.nbytes == before + rcv_bytes + solver_bytes
    # the other solvers on the same tape: the same bits, and no more memory
    xn2, info_n2 = tape.solve_normal(rhs, row_weight=run.rw, **nkw)
    xj2, xje2, info_j2 = tape.solve_joint(rhs, rhs_src, **jkw)
    _bits_equal(xn2, xn)
    _bits_equal(xj2, xj)
    _bits_equal(xje2, xje)
    assert info_n2 == info_n and info_j2 == info_j and tape.nbytes == before + rcv_bytes + solver_bytes
    tape.release_joint()
    tape.release_solve()
    released = tape.nbytes
    assert released < before + rcv_bytes + solver_bytes
    tape.release_receiver()
    assert tape.nbytes == released - rcv_bytes - solver_bytes
    x2, xe2, info2 = tape.solve_receiver_joint(rhs, rhs_e, **kw)
    _bits_equal(x2, x)
    _bits_equal(xe2, xe)
    assert info2 == info and tape.nbytes == released
    # the host glue
    residual = (1e-2 * rng.standard_normal(tape.n_data)).astype(dt)
    model = rng.uniform(0.4, 0.7, tape.n_cols).astype(dt)
    b, b_e = tape.vjp(run.rw * residual, return_receiver_grad=True)
    b = b - dt(2e-2) * tape.smooth(model, WEIGHTS)
    assert b.dtype == dt
    kw = dict(row_weight=run.rw, smooth=dt(2e-2), smooth_weights=WEIGHTS, damp=dt(1e-1), rcv_damp=RDAMP, rcv_scale=SCALE, maxiter=3,
              return_info=True)
    want = tape.solve_receiver_joint(b, b_e, **kw)
    got = reciprocal_gauss_newton_step(tape, residual, model, **kw)
    _bits_equal(got[0], want[0])
    _bits_equal(got[1], want[1])
    assert got[2] == want[2] and np.any(got[1] != 0)
    tape.free()


# ---- 4. device tensors and the torch operators (child processes)
def _torch_tensors(dtname):
    import torch

    dt = np.dtype(dtname).type
    run = Run(nn=(9, 8, 10), dt=dt)
    tape = run.tape
    tape.set_receiver_points(run.por, n_points=run.n_rcv_points)
    dev = lambda a: torch.as_tensor(a, device="cuda")   # noqa: E731
    rhs, rhs_e = _rhs(run, 71)
    tt, G = tape.receiver_eval(dev(run.rcv.astype(dt)), run.event_of_row)
    assert tt.is_cuda and G.is_cuda
    _bits_equal(tt.cpu().numpy(), run.tt)
    _bits_equal(G.cpu().numpy(), run.G)
    d = tape.jvp_receiver(dev(run.ve))
    assert d.is_cuda
    _bits_equal(d.cpu().numpy(), tape.jvp_receiver(run.ve))
    ref = tape.vjp(run.w, return_receiver_grad=True)
    g, ge = tape.vjp(dev(run.w), return_receiver_grad=True)
    assert g.is_cuda and ge.is_cuda
    _bits_equal(g.cpu().numpy(), ref[0])
    _bits_equal(ge.cpu().numpy(), ref[1])
    _bits_equal(tape.jvp_joint_receiver(dev(run.v), dev(run.ve)).cpu().numpy(), tape.jvp_joint_receiver(run.v, run.ve))
    ref = tape.gauss_newton_receiver_joint(run.v, run.ve, run.rw, SCALE)
    t_v, t_ve = dev(run.v), dev(run.ve)
    g, ge = tape.gauss_newton_receiver_joint(t_v, t_ve, dev(run.rw), SCALE)
    assert g.is_cuda and ge.is_cuda and ge.shape == (run.n_rcv_points, 4)
    _bits_equal(g.cpu().numpy(), ref[0])
    _bits_equal(ge.cpu().numpy(), ref[1])
    _bits_equal(t_v.cpu().numpy(), run.v)         # (the arguments are read, not used as work arrays)
    _bits_equal(t_ve.cpu().numpy(), run.ve)
    kw = dict(smooth=2e-2, smooth_weights=WEIGHTS, damp=1e-1, rcv_damp=RDAMP, rcv_scale=SCALE, maxiter=3, return_info=True)
    ref = tape.solve_receiver_joint(rhs, rhs_e, row_weight=run.rw, **kw)
    x, xe, info = tape.solve_receiver_joint(dev(rhs), dev(rhs_e), row_weight=dev(run.rw), **kw)
    assert x.is_cuda and xe.is_cuda and info == ref[2]
    _bits_equal(x.cpu().numpy(), ref[0])
    _bits_equal(xe.cpu().numpy(), ref[1])


@DTYPES
def test_receiver_calls_with_device_tensors(dt):
    _in_child("tensors", np.dtype(dt).name)


def _torch_operator():
    import torch
    import torch.autograd.forward_ad as fwAD

    import ttcr_amd
    import ttcr_amd.autograd as ag

    dt = np.float64
    nn = (9, 8, 10)
    rng = np.random.default_rng(13)
    hi = (np.array(nn) - 1) * FC.DX
    v = rng.uniform(1.0, 2.0, nn).astype(dt)
    src = np.array([[0.0, 0.1, 1.3, 1.6, 2.2], [1.0, 0.0, 2.9, 1.1, 3.4]])
    eor = np.array([0, 1, 0, 1, 1, 0, 0])
    rcv = rng.uniform(0.7 * FC.DX, hi - 0.7 * FC.DX, (7, 3))
    rcv[2, 0] = 2 * FC.DX                                  # on a plane: no derivative along x
    source = np.column_stack([eor.astype(float), src[eor][:, 1:]])
    g = ttcr_amd.Grid3d(*[np.arange(n) * FC.DX for n in nn], cell_slowness=0, method="FSM", dtype=dt, weno=0, tt_from_rp=0)
    vel = torch.tensor(v, device="cuda", requires_grad=True)
    r_t = torch.tensor(rcv, device="cuda", requires_grad=True)
    plain = ag.raytrace_adjoint(g, vel.detach(), source, rcv)
    tt = ag.raytrace_adjoint(g, vel, source, r_t)
    _bits_equal(tt.detach().cpu().numpy(), plain.cpu().numpy())
    c = rng.standard_normal(7)
    gv, gr = torch.autograd.grad((torch.from_numpy(c).cuda() * tt).sum(), (vel, r_t), create_graph=True)
    _, tape = g.raytrace_adjoint(source, rcv)
    G = tape.receiver_jacobian()
    _bits_equal(gr.detach().cpu().numpy(), c[:, None] * G)
    assert gr[2, 0] == 0
    gv_plain = torch.autograd.grad((torch.from_numpy(c).cuda() * ag.raytrace_adjoint(g, vel, source, rcv)).sum(), vel)[0]
    _bits_equal(gv.detach().cpu().numpy(), gv_plain.cpu().numpy())           # (the velocity gradient is what it was)
    try:                                                                      # a second derivative through rcv raises
        torch.autograd.grad(gr.sum(), r_t)
    except RuntimeError:
        pass
    else:
        raise AssertionError("no RuntimeError")
    t_r = rng.standard_normal((7, 3))
    tv = v * rng.standard_normal(nn)
    with fwAD.dual_level():
        only = fwAD.unpack_dual(ag.raytrace_adjoint(g, vel.detach(), source, fwAD.make_dual(r_t.detach(), torch.from_numpy(t_r).cuda()))).tangent
        both = fwAD.unpack_dual(ag.raytrace_adjoint(g, fwAD.make_dual(vel.detach(), torch.from_numpy(tv).cuda()), source,
                                                    fwAD.make_dual(r_t.detach(), torch.from_numpy(t_r).cuda()))).tangent
        only, both = only.cpu().numpy(), both.cpu().numpy()
    drcv = np.zeros((7, 4))
    drcv[:, 1:] = t_r[tape._rows]
    ref = tape.jvp_receiver(drcv)
    _bits_equal(only, ref)
    _bits_equal(both, tape.jvp((-(tv / (v * v))).flatten("F")) + ref)        # forward mode adds the rows as fl(a + b)
    # central differences of the operator itself in the receiver positions
    step = 1e-6
    fd = (ag.raytrace_adjoint(g, vel.detach(), source, rcv + step * t_r) - ag.raytrace_adjoint(g, vel.detach(), source, rcv - step * t_r)) / (2 * step)
    fd = fd.cpu().numpy()
    keep = np.arange(7) != 2   # (row 2 moves off its plane: the code's derivative along x is 0 there by definition, not the slope)
    err = np.linalg.norm(only[keep] - fd[keep]) / np.linalg.norm(fd[keep])
    print("raytrace_adjoint, d tt / d rcv against central differences: %.2e (bound 1e-06)" % err)
    assert err <= 1e-6, err
    # raytrace_events: the same term
    ev = torch.tensor(src[:, 1:].copy(), device="cuda", requires_grad=True)
    tt_e = ag.raytrace_events(g, vel, ev, eor, r_t)
    ge, gr_e = torch.autograd.grad((torch.from_numpy(c).cuda() * tt_e).sum(), (ev, r_t))
    _bits_equal(gr_e.cpu().numpy(), c[:, None] * G)
    assert np.any(ge.cpu().numpy() != 0)


def test_torch_operators_are_differentiable_in_rcv():
    _in_child("operator")
