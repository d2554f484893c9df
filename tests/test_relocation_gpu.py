"""Moving the receiver points of the field tape and the relocation-only system on the device (FieldTape.move_receiver_points,
receiver_points, vjp_receiver, gauss_newton_receiver, solve_receiver and inversion.relocate).  The contract of a move: the
moved tape is, to the bit and in every result, the tape a fresh raytrace_adjoint builds with the moved coordinates in rcv -- so the moved
tape is compared with exactly that tape, product by product, for fp32 and fp64 and, where a relaxation runs, under both schedules.  The
relocation-only product and solve are held, to the bit, to tests/relocation_reference.py on the device's own fields.  All layouts are
reciprocal: every event (a station) sees every receiver point (a hypocentre); rows are event-major, so data rows are tape rows."""
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
import field_tape_cases as FC  # noqa: E402
import relocation_reference as LR  # noqa: E402
import test_relocation as CPU  # noqa: E402
from field_tape_cases import _bits_equal  # noqa: E402
from test_receiver_derivative_gpu import ORIGIN, RDAMP, SCALE, hypocentres  # noqa: E402

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
SCHEDULES = ("tiled", "jacobi")
N_POINTS = 100   # receiver points with rows; one more has none


def _in_child(fn, *args):
    """Run _torch_<fn>(*args) of this module in a fresh process that initialises torch's device before the first grid"""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_relocation_gpu as t; t._torch_%s(*%r)"
            % (HERE, ROOT, fn, args))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


class Scene:
    """a grid, three events (stations) and a row of every event for each of n_points receiver points, plus one point without rows"""

    def __init__(self, nn, dt, kind="rough", origin=FC.ZERO, dx=FC.DX, translate=False, wrt="nodes", model_shape=None, n_events=3,
                 n_points=N_POINTS, scale=1.0, grouped=True):
        import ttcr_amd

        self.nn, self.dt, self.dx, self.origin, self.translate, self.wrt, self.model_shape = nn, dt, dx, origin, translate, wrt, model_shape
        self.n_events, self.P, self.grouped = n_events, n_points, grouped
        rng = np.random.default_rng(sum(nn) + n_events)
        hi = np.array(nn) - 1.0
        self.src_idx = [[np.floor(0.4 * (nn[a] - 1)) + (0.3, 0.6, 0.2)[a] for a in range(3)], [nn[a] - 1 - (0.7, 0.4, 0.8)[a] for a in range(3)]]
        self.src_idx += [list(rng.uniform(0.2, hi - 0.2)) for _ in range(n_events - 2)]
        self.src_idx = self.src_idx[:n_events]
        self.src_xyz = FC.at(nn, dx, origin, self.src_idx)
        self.source = np.vstack([np.tile(np.concatenate([[0.125 * e], self.src_xyz[e]]), (n_points, 1)) for e in range(n_events)])
        self.event_of_row = np.repeat(np.arange(n_events), n_points)
        # grouped: the rows of point q in every event share it (the reciprocal grouping) and one more point has no row; else the tape's default
        self.por = np.tile(np.arange(n_points), n_events) if grouped else np.arange(n_events * n_points)
        self.n_rcv_points = n_points + 1 if grouped else n_events * n_points
        axes = [origin[a] + np.arange(nn[a]) * dx for a in range(3)]
        cells = wrt == "cells"
        self.grid = ttcr_amd.Grid3d(*axes, n_threads=1, cell_slowness=1 if cells else 0, method="FSM", dtype=dt, weno=0, tt_from_rp=0,
                                    translate_grid=translate)
        if cells:
            nc = tuple(n - 1 for n in nn)
            self.grid.set_slowness((scale * np.random.default_rng(67).uniform(0.4, 0.7, int(np.prod(nc)))).astype(dt).reshape(nc, order="F"))
        else:
            self.grid.set_slowness(FC.model(nn, dx, origin, kind, scale).reshape(nn, order="F"))
        n = self.source.shape[0]
        r2 = np.random.default_rng(71)
        self.w = FC.wide_weights(r2, n, dt)
        self.rw = r2.uniform(0.5, 2.0, n).astype(dt)
        self.ve = r2.standard_normal((self.n_rcv_points, 4)).astype(dt)
        self.rhs_rcv = r2.standard_normal((self.n_rcv_points, 4)).astype(dt)
        n_pairs = min(60, n * (n - 1) // 2)
        self.pa = r2.integers(0, max(n, 1), n_pairs)
        self.pb = (self.pa + 1 + r2.integers(0, max(n - 1, 1), n_pairs)) % max(n, 1)
        self.pw = r2.uniform(0.1, 3.0, n_pairs).astype(dt)
        self.n_cols = None

    def points(self, xyz):
        """xyz (n_points [+ 1], 3) as values of the grid dtype, held in float64"""
        return np.asarray(xyz, dtype=self.dt).astype(np.float64)

    def rcv(self, xyz):
        return xyz[self.por]

    def fresh(self, xyz):
        """(tt, tape) of a new raytrace_adjoint with the receivers xyz[point], the point map and the pairs set"""
        tt, tape = self.grid.raytrace_adjoint(self.source, self.rcv(xyz), wrt=self.wrt, model_shape=self.model_shape)
        assert tape.n_events == self.n_events and np.array_equal(tape._rows, np.arange(self.source.shape[0]))
        if self.grouped:
            tape.set_receiver_points(self.por, self.n_rcv_points)
        if len(self.pa):
            tape.set_row_pairs(self.pa, self.pb)
        if self.n_cols is None:
            self.n_cols = tape.n_cols
            r3 = np.random.default_rng(73)
            self.v = (r3.uniform(0.4, 0.7, tape.n_cols) * r3.standard_normal(tape.n_cols)).astype(self.dt)
            self.rhs = r3.standard_normal(tape.n_cols).astype(self.dt)
        return tt, tape

    def products(self, tape, full=True):
        out = {"G": tape.receiver_jacobian()}
        pw = self.pw if len(self.pa) else None
        for sch in SCHEDULES:
            out["vjp_" + sch], out["grcv_" + sch] = tape.vjp(self.w, schedule=sch, return_receiver_grad=True)
            out["jvp_" + sch] = tape.jvp(self.v, schedule=sch)
            if full:
                out["gn_" + sch], out["gn_rcv_" + sch] = tape.gauss_newton_receiver_joint(self.v, self.ve, self.rw, SCALE, schedule=sch,
                                                                                        pair_weight=pw)
        if full:
            out["block"] = tape.vjp_block(np.stack([self.w, self.rw]))
            tape.hold(self.w)
            out["hvp"] = tape.hvp(self.v)
            tape.release()
            x, xr, info = tape.solve_receiver_joint(self.rhs, self.rhs_rcv, row_weight=self.rw, damp=1e-2, rcv_damp=RDAMP, rcv_scale=SCALE,
                                                    maxiter=3, return_info=True, pair_weight=pw)
            out["x"], out["x_rcv"], out["rho"], out["pq"] = x, xr, np.array(info["rho"]), np.array(info["pq"])
        return out


def same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        _bits_equal(got[k], want[k])


def special_points(sc, rng):
    """generic points, points on one, two and three planes, on the far faces, the corners, one rounding below the last planes (the clamp),
    a frozen node of event 0, its source itself, the source of event 1 (in the last cell of the far corner); the rest random"""
    pts = [hypocentres(sc.nn, sc.dx, sc.origin, sc.dt, rng), FC.at(sc.nn, sc.dx, sc.origin, [np.floor(sc.src_idx[0])]), sc.src_xyz[:2]]
    pts = np.vstack(pts)
    assert len(pts) <= sc.n_rcv_points
    return sc.points(np.vstack([pts, FC.random_receivers(sc.nn, sc.dx, sc.origin, rng, sc.n_rcv_points - len(pts))]))


def pile_points(sc, rng):
    """50 points onto one point, 40 into one cell, the rest random: a node's run of the seed list then holds up to 270 rows whose order
    decides the bits of the seed"""
    c = [max((n - 1) // 2 - 1, 0) for n in sc.nn]
    one = FC.at(sc.nn, sc.dx, sc.origin, [[c[0] + 0.3, c[1] + 0.6, c[2] + 0.45]])
    cell = FC.at(sc.nn, sc.dx, sc.origin, np.array(c) + rng.uniform(0.05, 0.95, (40, 3)))
    rest = FC.random_receivers(sc.nn, sc.dx, sc.origin, rng, sc.n_rcv_points - 90)
    return sc.points(np.vstack([np.tile(one, (50, 1)), cell, rest]))


def plane_points(sc, rng, n_on):
    """every point on n_on grid planes: 4, 2 or 1 stencil entries per row"""
    idx = rng.uniform(0.3, np.array(sc.nn) - 1.3, (sc.n_rcv_points, 3))
    idx[:, :n_on] = np.floor(idx[:, :n_on])
    return sc.points(FC.at(sc.nn, sc.dx, sc.origin, idx))


SCENES = {
    "15x13x17-rough": dict(nn=(15, 13, 17), kind="rough"),
    "15x13x17-layers": dict(nn=(15, 13, 17), kind="two_layers"),
    "29x11x12-rough": dict(nn=(29, 11, 12), kind="rough"),
    "29x11x12-layers": dict(nn=(29, 11, 12), kind="two_layers"),
    "origin": dict(nn=(9, 8, 10), origin=ORIGIN, dx=25.0, scale=1e-3),
    "translated": dict(nn=(9, 8, 10), origin=ORIGIN, dx=25.0, scale=1e-3, translate=True),
    "cells": dict(nn=(9, 8, 10), wrt="cells"),
    "model": dict(nn=(9, 8, 10), wrt="model", model_shape=(1, 1, 5)),
}


# ---- 1. a moved tape against a fresh one
@DTYPES
@pytest.mark.parametrize("name", sorted(SCENES))
def test_move_against_a_fresh_tape(name, dt):
    sc = Scene(dt=dt, **SCENES[name])
    rng = np.random.default_rng(5)
    start = sc.points(FC.random_receivers(sc.nn, sc.dx, sc.origin, rng, sc.n_rcv_points))
    tt0, tape = sc.fresh(start)
    first = sc.products(tape)
    pts = tape.receiver_points()                            # before any move: the receivers of the rows, NaN for the point without rows
    assert pts.dtype == dt and np.isnan(pts[-1]).all()
    if sc.translate:                                        # (the origin is subtracted and added again in the grid dtype)
        assert np.allclose(pts[:-1], start[:-1], rtol=0, atol=4 * np.finfo(dt).eps * 1300)
    else:
        assert np.array_equal(pts[:-1], start[:-1].astype(dt))
    for xyz, full in ((special_points(sc, rng), True), (pile_points(sc, rng), True), (plane_points(sc, rng, 1), False),
                      (plane_points(sc, rng, 2), False), (plane_points(sc, rng, 3), False)):
        tt = tape.move_receiver_points(xyz)                 # (each one a move from the points of the move before)
        tt_f, fresh = sc.fresh(xyz)
        assert tt.dtype == dt and tt.shape == tt_f.shape
        _bits_equal(tt, tt_f)
        assert np.array_equal(tape.receiver_points(), xyz.astype(dt))
        same(sc.products(tape, full), sc.products(fresh, full))
        fresh.free()
    _bits_equal(tape.move_receiver_points(start), tt0)      # a move back restores the first tape's bits
    same(sc.products(tape), first)
    assert np.array_equal(tape.receiver_points(), start.astype(dt))
    assert tape.n_pairs == len(sc.pa) and np.array_equal(tape.rcv_point_of_row, sc.por)
    tape.free()


# ---- 2. row counts around a workgroup of the point kernel and the single-block path of the radix sort (1 to 8 entries per row)
@DTYPES
@pytest.mark.parametrize("n_rows", [1, 255, 256, 257, 2100])
def test_row_counts(n_rows, dt):
    n_events = 3 if n_rows % 3 == 0 else 1
    sc = Scene((9, 8, 10), dt, n_events=n_events, n_points=n_rows // n_events, grouped=False)
    rng = np.random.default_rng(n_rows)
    start = sc.points(FC.random_receivers(sc.nn, sc.dx, sc.origin, rng, sc.n_rcv_points))
    _, tape = sc.fresh(start)
    assert tape.n_rows == n_rows == tape.n_rcv_points
    idx = rng.uniform(0.3, np.array(sc.nn) - 1.3, (n_rows, 3))
    for k in range(n_rows):                                  # 8, 4, 2 and 1 entries in turn
        idx[k, :k % 4] = np.floor(idx[k, :k % 4])
    xyz = sc.points(FC.at(sc.nn, sc.dx, sc.origin, idx))
    tt = tape.move_receiver_points(xyz)
    tt_f, fresh = sc.fresh(xyz)
    _bits_equal(tt, tt_f)
    same(sc.products(tape, n_rows < 2000), sc.products(fresh, n_rows < 2000))
    tape.free()
    fresh.free()


def test_a_tape_without_rows():
    """an event without receivers, through the C entry (the Python layer takes no empty rcv): a move of no points"""
    from ttcr_amd import _lib
    from ttcr_amd.rgrid import FieldTape, _ptr

    sc = Scene((9, 8, 10), np.float32, n_events=1, n_points=1)
    tx = np.ascontiguousarray(sc.src_xyz[:1], dtype=np.float32)
    t0, off = np.zeros(1, dtype=np.float32), np.zeros(2, dtype=np.int32)
    tx_off = np.array([0, 1], dtype=np.int32)
    rx, out = np.zeros((1, 3), dtype=np.float32), np.zeros(1, dtype=np.float32)
    h = C.c_void_p()
    _lib.check(sc.grid._lib.ttcr_fsm_raytrace_multi_adjoint(sc.grid._h, 1, _ptr(tx_off), _ptr(tx), _ptr(t0), _ptr(off), _ptr(rx), _ptr(out),
                                                            C.byref(h)))
    tape = FieldTape(sc.grid._lib, h, np.float32, np.zeros(0, dtype=np.int64), 0)
    assert tape.n_rows == 0 and tape.n_rcv_points == 0
    tt = tape.move_receiver_points(np.zeros((0, 3)))
    assert tt.shape == (0,) and tape.receiver_points().shape == (0, 3)
    before = tape.nbytes
    tape.move_receiver_points(np.zeros((0, 3)))
    assert tape.nbytes == before
    v = np.ones(tape.n_cols, dtype=np.float32)
    assert tape.jvp(v).shape == (0,)
    assert tape.gauss_newton_receiver(np.zeros((0, 4))).shape == (0, 4)
    tape.free()


# ---- 3. what a move keeps, what it releases, what it allocates; argument errors leave the tape as it was
@DTYPES
def test_after_a_move(dt):
    sc = Scene((9, 8, 10), dt)
    rng = np.random.default_rng(11)
    start = sc.points(FC.random_receivers(sc.nn, sc.dx, sc.origin, rng, sc.n_rcv_points))
    _, tape = sc.fresh(start)
    before = sc.products(tape)
    d0 = tape.pair_difference(sc.w)
    tape.hold(sc.w)
    held = tape.nbytes
    bad = start.copy()
    bad[3, 1] = np.nan
    far = start.copy()
    far[-1, 2] = sc.origin[2] + sc.nn[2] * sc.dx               # (the point without rows is checked too)
    for xyz, msg in ((bad, "finite"), (far, "^Receiver outside grid$"), (start[:-1], "xyz should be"), (start.astype(complex), "real numbers")):
        with pytest.raises(ValueError, match=msg):
            tape.move_receiver_points(xyz)
    assert tape.nbytes == held
    _bits_equal(tape.hvp(sc.v), before["hvp"])                # (the held cotangent is still there: nothing was touched)
    tape.release()
    same(sc.products(tape), before)
    tape.hold(sc.w)
    xyz = special_points(sc, rng)
    tape.move_receiver_points(xyz)
    with pytest.raises(ValueError, match="hold"):
        tape.hvp(sc.v)
    with pytest.raises(ValueError, match="hold"):
        tape.newton(sc.v)
    grown = tape.nbytes
    elem, cap = np.dtype(dt).itemsize, 8 * tape.n_rows
    # the hold arrays left; both lists had 8 entries per row already (generic points), so what came is the three index arrays of 8 n_rows
    # ints and the sort's workspace
    extra = grown - (held - 2 * tape.n_events * tape.n_nodes * elem)
    assert 3 * cap * 4 < extra < 3 * cap * 4 + (1 << 20)
    assert tape.n_pairs == len(sc.pa) and np.array_equal(tape.rcv_point_of_row, sc.por)
    _bits_equal(tape.pair_difference(sc.w), d0)
    tape.move_receiver_points(pile_points(sc, rng))
    tape.move_receiver_points(xyz)
    assert tape.nbytes == grown                                # once, not per move
    # release_receiver frees the receiver arrays; the next call rebuilds them from the moved points
    tape.release_receiver()
    _, fresh = sc.fresh(xyz)
    same(sc.products(tape), sc.products(fresh))
    # a new point map forgets the moved coordinates of the points, not of the rows
    tape.set_receiver_points(sc.por, sc.n_rcv_points)
    pts = tape.receiver_points()
    assert np.isnan(pts[-1]).all() and np.array_equal(pts[:-1], xyz[:-1].astype(dt))
    tape.free()
    fresh.free()


# ---- 4. the relocation-only product and solve against the restatement
def layout_of(sc, tape, xyz):
    fields = [tape.field(e) for e in range(tape.n_events)]
    pairs = (sc.pa, sc.pb) if len(sc.pa) else None
    return LR.Layout(fields, sc.nn, sc.dx, sc.origin, sc.event_of_row, sc.por, sc.n_rcv_points, translate=sc.translate, pairs=pairs)


@DTYPES
@pytest.mark.parametrize("name", ["plain", "translated", "cells"])
def test_gauss_newton_receiver_and_solve_receiver_bits(name, dt):
    kw = dict(plain=dict(nn=(9, 8, 10)), translated=SCENES["translated"], cells=SCENES["cells"])[name]
    sc = Scene(dt=dt, n_points=30, **kw)
    rng = np.random.default_rng(17)
    _, tape = sc.fresh(sc.points(FC.random_receivers(sc.nn, sc.dx, sc.origin, rng, sc.n_rcv_points)))
    xyz = special_points(sc, rng)
    tt = tape.move_receiver_points(xyz)
    lay = layout_of(sc, tape, xyz)
    ref_tt, G, _ = LR.move(lay, xyz)
    _bits_equal(tt, ref_tt)
    _bits_equal(tape.receiver_jacobian(), G)
    _bits_equal(tape.vjp_receiver(sc.w), LR.RR.reverse(G, sc.por, sc.n_rcv_points, sc.w))
    zero = np.zeros(tape.n_cols, dtype=dt)
    for rw, scale, pw in ((None, None, None), (sc.rw, SCALE, None), (sc.rw, SCALE, sc.pw), (None, None, sc.pw)):
        got = tape.gauss_newton_receiver(sc.ve, row_weight=rw, rcv_scale=scale, pair_weight=pw)
        assert tape.passes == (0, 0) and got.dtype == dt
        _bits_equal(got, LR.product(lay, G, sc.ve, rw, scale, pw))
        _, joint = tape.gauss_newton_receiver_joint(zero, sc.ve, rw, scale, pair_weight=pw)
        assert np.array_equal(got, joint)                      # (the sign of a zero may differ)
    before = tape.nbytes
    for rw, scale, damp, pw, maxiter, rtol in ((sc.rw, SCALE, RDAMP, sc.pw, 6, 1e-6), (None, None, 1e-2, None, 4, 1e-6),
                                               (sc.rw, (1., 0.5, 0.5, 0.5), (0.5, 2., 2., 2.), sc.pw, 60, 1e-3), (sc.rw, None, 0.0, sc.pw, 2, 1e-6)):
        x, info = tape.solve_receiver(sc.rhs_rcv, row_weight=rw, rcv_damp=damp, rcv_scale=scale, maxiter=maxiter, rtol=rtol, return_info=True,
                                      pair_weight=pw)
        ref, rinfo = LR.cg(lambda p: LR.product(lay, G, p, rw, scale, pw), sc.rhs_rcv, dt, rcv_damp=damp, rcv_scale=scale, maxiter=maxiter,
                           rtol=rtol)
        _bits_equal(x, ref)
        assert (info["status"], info["iterations"], info["rho"], info["pq"]) == (rinfo["status"], rinfo["iterations"], rinfo["rho"], rinfo["pq"])
        assert all(p == (0, 0) for p in info["passes"]) and len(info["passes"]) == len(info["pq"]) and info["passes_x0"] is None
        assert tape.passes == (0, 0)
    assert {0, 1} <= {tape.solve_receiver(sc.rhs_rcv, sc.rw, (0.5, 2., 2., 2.), (1., 0.5, 0.5, 0.5), m, 1e-3, True, sc.pw)[1]["status"] for m in (1, 60)}
    # pure double-difference data, no damping: the common origin-time shift is a null vector and the solve says so (status 2)
    shift = np.zeros((sc.n_rcv_points, 4), dtype=dt)
    shift[:, 0] = 1
    x, info = tape.solve_receiver(shift, row_weight=np.zeros_like(sc.rw), pair_weight=sc.pw, return_info=True)
    assert info["status"] == 2 and info["iterations"] == 0 and info["pq"] == [0.0] and not np.any(x)
    assert not np.any(tape.solve_receiver(sc.rhs_rcv, sc.rw, RDAMP, (0., 0., 0., 0.)))     # rcv_scale all zeros: zeros
    work = tape.nbytes - before
    assert work > 0
    tape.solve_receiver(sc.rhs_rcv, sc.rw, RDAMP, SCALE)
    assert tape.nbytes == before + work
    tape.release_receiver()
    assert tape.nbytes < before
    tape.free()


# ---- 5. inversion.relocate on the CPU recovery case: the device loop against the restated loop on the device's fields
def _recovery(dt):
    import ttcr_amd

    axes = [np.arange(n) * CPU.DX for n in CPU.NN]
    grid = ttcr_amd.Grid3d(*axes, n_threads=1, cell_slowness=0, method="FSM", dtype=dt, weno=0, tt_from_rp=0)
    grid.set_slowness(CPU.gradient_model().reshape(CPU.NN, order="F"))
    E, P = len(CPU.STATIONS), len(CPU.TRUE)
    source = np.vstack([np.tile(np.concatenate([[0.0], CPU.STATIONS[e]]), (P, 1)) for e in range(E)])
    start = np.asarray(CPU.TRUE + CPU.OFFSET, dtype=dt).astype(np.float64)
    por = np.tile(np.arange(P), E)
    _, tape = grid.raytrace_adjoint(source, start[por])
    tape.set_receiver_points(por)
    return tape, start


def _recovery_data(tape, dt, pairs):
    lay = CPU.layout_of([tape.field(e) for e in range(tape.n_events)], pairs, dtype=dt)
    t_obs, pair_dt = CPU.data_of(lay)
    if pairs:
        tape.set_row_pairs(*lay.pairs)
    return lay, np.asarray(t_obs, dtype=dt), None if pair_dt is None else np.asarray(pair_dt, dtype=dt)


@DTYPES
@pytest.mark.parametrize("mode", ["absolute", "pairs"])
def test_relocate_is_the_restated_loop(mode, dt):
    from ttcr_amd import inversion

    tape, start = _recovery(dt)
    lay, t_obs, pair_dt = _recovery_data(tape, dt, mode == "pairs")
    t0 = np.zeros(len(CPU.TRUE), dtype=dt)
    kw = dict(pair_dt=pair_dt, n_iter=10, rcv_damp=1e-3)
    t0r, xyzr, histr, infor = LR.relocate(lay, start, t_obs, t0, **kw)
    t0g, xyzg, histg, infog = inversion.relocate(tape, t_obs, t0, **kw)
    print("relocate[%s, %s]: %d iterations, halvings %s, misfit %.3e -> %.3e, location error %.3e dx"
          % (mode, np.dtype(dt).name, infog["iterations"], infog["halvings"], histg[0], histg[-1], float(np.max(np.abs(xyzg - CPU.TRUE))) / CPU.DX))
    _bits_equal(xyzg, xyzr)
    _bits_equal(t0g, t0r)
    assert histg == histr and infog["halvings"] == infor["halvings"]
    assert all(b <= a for a, b in zip(histg, histg[1:]))
    assert np.array_equal(tape.receiver_points(), xyzg)
    if dt == np.float64:
        assert float(np.max(np.abs(xyzg - CPU.TRUE))) <= 10 * CPU.MEASURED[mode]
    tape.free()


def _torch_relocate(dtname):
    import torch

    from ttcr_amd import inversion

    dt = np.dtype(dtname).type
    tape, start = _recovery(dt)
    lay, t_obs, pair_dt = _recovery_data(tape, dt, True)
    t0 = np.zeros(len(CPU.TRUE), dtype=dt)
    kw = dict(n_iter=10, rcv_damp=1e-3)
    t0n, xyzn, histn, infon = inversion.relocate(tape, t_obs, t0, pair_dt=pair_dt, **kw)
    tape.move_receiver_points(start)
    dev = torch.device("cuda", tape.device)
    t0t, xyzt, histt, infot = inversion.relocate(tape, torch.as_tensor(t_obs, device=dev), torch.as_tensor(t0, device=dev),
                                                 pair_dt=torch.as_tensor(pair_dt, device=dev), **kw)
    assert xyzt.is_cuda and t0t.is_cuda and xyzt.dtype == (torch.float32 if dt == np.float32 else torch.float64)
    # the steps are the same device calls; the misfits are float64 sums whose order differs between numpy and torch: equal to a few
    # roundings of a sum of 30 + 30 non-negative terms, and the accepted steps -- hence the points -- are the same to the bit
    assert infot["halvings"] == infon["halvings"]
    assert np.array_equal(xyzt.cpu().numpy(), xyzn) and np.array_equal(t0t.cpu().numpy(), t0n)
    assert np.allclose(histt, histn, rtol=64 * np.finfo(np.float64).eps, atol=0)
    assert np.array_equal(tape.receiver_points(), xyzn)
    # device tensors through the new methods themselves
    ve = torch.ones((tape.n_rcv_points, 4), dtype=xyzt.dtype, device=dev)
    g = tape.gauss_newton_receiver(ve, pair_weight=torch.ones(tape.n_pairs, dtype=xyzt.dtype, device=dev))
    assert g.is_cuda and np.array_equal(g.cpu().numpy(), tape.gauss_newton_receiver(np.ones((tape.n_rcv_points, 4), dtype=dt),
                                                                                   pair_weight=np.ones(tape.n_pairs, dtype=dt)))
    tt = tape.move_receiver_points(xyzt)
    assert tt.is_cuda and np.array_equal(tt.cpu().numpy(), tape.move_receiver_points(xyzn))
    with torch.no_grad():
        far = xyzt.clone()
        far[0, 0] = -1.0
    with np.testing.assert_raises(ValueError):
        tape.move_receiver_points(far)
    tape.free()


@DTYPES
def test_relocate_with_device_tensors(dt):
    _in_child("relocate", np.dtype(dt).name)
