"""The joint hypocentre-velocity system of the field tape on the device (FieldTape.jvp_joint, gauss_newton_joint, solve_joint,
release_joint and inversion.joint_gauss_newton_step).  Every comparison is to the bit, against the numpy restatement of
tests/joint_reference.py run on the device's own fields -- the restated recurrence is driven by the device's own gauss_newton_joint, so
that what is compared there is the solver, not the product --, for fp32 and fp64 and under both schedules.  The grids are small: what can
go wrong are tile seams, frozen nodes on tile faces, the seam between the two blocks of the joint vector and chunk boundaries."""
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
import joint_reference as JR  # noqa: E402
import normal_reference as NR  # noqa: E402
from field_tape_cases import _bits_equal  # noqa: E402

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
WRT = pytest.mark.parametrize("wrt", ["nodes", "cells"])
SCHEDULES = ("tiled", "jacobi")
SOLVE_NN = (17, 14, 19)
WEIGHTS = (1.0, 0.5, 2.0)
REG = {"both": (2e-2, 1e-1), "smooth": (2e-2, 0.0), "damp": (0.0, 1e-1), "none": (0.0, 0.0)}
SCALE = (1.0, 0.05, 0.0, 0.1)          # one entry 0: that coordinate of every point is fixed
SDAMP = (1e-2, 1e-1, 1.0, 1e-1)


def _in_child(fn, *args):
    """Run _torch_<fn>(*args) of this module in a fresh process that initialises torch's device before the first grid (as
    tests/test_normal_solve_gpu.py does)."""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_joint_solve_gpu as t; t._torch_%s(*%r)"
            % (HERE, ROOT, fn, args))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


class Run:
    """one raytrace_adjoint call for the events of a case -- a node tape, or the cell tape of the same nodes --, with the device's
    fields and what the restatement needs"""

    def __init__(self, case, dt, wrt="nodes"):
        import ttcr_amd
        from oracle import oracle as O

        self.case, self.dt, self.wrt = case, dt, wrt
        self.src, self.rcv, agg, self.rows = FC.call_arrays(case, np.random.default_rng(61))
        axes = [case.origin[a] + np.arange(case.nn[a]) * case.dx for a in range(3)]
        self.nc = tuple(n - 1 for n in case.nn)
        cells = wrt == "cells"
        self.grid = ttcr_amd.Grid3d(*axes, cell_slowness=1 if cells else 0, method="FSM", dtype=dt, weno=0, tt_from_rp=0)
        if cells:
            sc = np.random.default_rng(67).uniform(0.4, 0.7, int(np.prod(self.nc))).astype(dt)
            self.grid.set_slowness(sc.reshape(self.nc, order="F"))
            self.s = O.cells_to_nodes3d(dt, self.nc, sc)
            self.to_nodes = lambda v: O.cells_to_nodes3d(dt, self.nc, np.asarray(v, dtype=dt))
        else:
            self.grid.set_slowness(case.s.reshape(case.nn, order="F"))
            self.s = np.asarray(case.s, dtype=dt)
            self.to_nodes = lambda v: np.asarray(v, dtype=dt)
        self.tt, self.tape = self.grid.raytrace_adjoint(self.src, self.rcv, aggregate_src=agg, wrt=wrt)
        t = self.tape
        self.sources = [e["pts"] for e in case.events]
        self.n_points = sum(p.shape[0] for p in self.sources)
        assert t.n_points == self.n_points and t.n_events == len(case.events) and t.wrt == wrt
        self.fields = [t.field(e) for e in range(t.n_events)]
        rng = np.random.default_rng(71)
        self.v = (rng.uniform(0.4, 0.7, t.n_cols) * rng.standard_normal(t.n_cols)).astype(dt)
        self.ve = rng.standard_normal((self.n_points, 4)).astype(dt)
        self.rw = rng.uniform(0.5, 2.0, self.rcv.shape[0]).astype(dt)
        self.geo = (self.s, case.dx, case.nn, case.origin, self.sources)

    def ref_jvp(self, v, ve):
        """the restatement: (dtt in rcv order, (n_events, n_nodes) field tangents)"""
        mus, dtts = JR.joint_tangent(self.fields, *self.geo, self.to_nodes(v), ve, rcvs=[self.rcv[r] for r in self.rows])
        dtt = np.zeros(self.rcv.shape[0], dtype=self.dt)
        for r, d in zip(self.rows, dtts):
            dtt[r] = d
        return dtt, np.stack(mus)

    def ref_gn(self, v, ve, rw, scale):
        return JR.joint_product(self.fields, *self.geo, [self.rcv[r] for r in self.rows], v, ve,
                                row_weights=None if rw is None else [rw[r] for r in self.rows], source_scale=scale,
                                cells=self.nc if self.wrt == "cells" else None, to_nodes=self.to_nodes)

    def params(self):
        return self.nc if self.wrt == "cells" else self.case.nn


def _edge_shapes(dt):
    e = FC.TAN_EDGE[np.dtype(dt)]
    return [tuple(2 * e + 1 if a == b else e + 1 for b in range(3)) for a in range(3)]


def _case21(pts, name):
    nn = (21, 21, 21)
    rcv = np.random.default_rng(5).uniform(0.6, 20 * FC.DX - 0.6, (30, 3))
    return FC.Case(name, nn, FC.DX, FC.ZERO, FC.model(nn, FC.DX, FC.ZERO, "smooth"), [FC._event(pts, rcv, 0.125)])


def _jvp_case(name, dt):
    if name.startswith("edge"):
        nn = _edge_shapes(dt)[int(name[-1])]
        assert nn in ([(21, 11, 11), (11, 21, 11), (11, 11, 21)] if dt == np.float32 else [(17, 9, 9), (9, 17, 9), (9, 9, 17)])
        return FC.shape_case(nn), "nodes"
    return {"2x2x2": lambda: (FC.shape_case((2, 2, 2)), "nodes"),
            "17x14x19": lambda: (FC.shape_case(SOLVE_NN), "nodes"),
            "two_points": lambda: (_case21([[3.3, 4.1, 5.7], [3.6, 4.2, 5.4]], name), "nodes"),     # the boxes overlap
            "on_node": lambda: (_case21([[4.0, 5.5, 3.0]], name), "nodes"),
            "translated": lambda: (FC.origin_case("translated-off_node"), "nodes"),
            "cells": lambda: (FC.shape_case(SOLVE_NN), "cells")}[name]()


# ---- 1. jvp_joint
@DTYPES
@pytest.mark.parametrize("name", ["2x2x2", "17x14x19", "edge0", "edge1", "edge2", "two_points", "on_node", "translated", "cells"])
def test_jvp_joint_bits(name, dt):
    case, wrt = _jvp_case(name, dt)
    if name.startswith("edge") or name in ("2x2x2", "17x14x19", "cells"):   # the second source sits in the last cell of the far corner
        assert len(case.events) == 2 and all(case.events[1]["pts"][0, a] > (case.nn[a] - 2) * case.dx for a in range(3))
    run = Run(case, dt, wrt)
    tape = run.tape
    ref_dtt, ref_mu = run.ref_jvp(run.v, run.ve)
    assert np.all(np.isfinite(ref_mu)) and np.any(ref_mu != 0) and np.any(ref_dtt != 0)
    zero_v, zero_e = np.zeros_like(run.v), np.zeros_like(run.ve)
    for schedule in SCHEDULES:
        dtt, mu = tape.jvp_joint(run.v, run.ve, return_fields=True, schedule=schedule)
        assert tape.passes >= 1 and mu.shape == (tape.n_events, tape.n_nodes) and dtt.dtype == dt and dtt.shape == (run.rcv.shape[0],)
        _bits_equal(dtt, ref_dtt)
        _bits_equal(mu, ref_mu)
        _bits_equal(tape.jvp_joint(run.v, run.ve, schedule=schedule), ref_dtt)
        # one operand zero: the values of the separate call (the sign of a zero may differ)
        a, fa = tape.jvp_joint(run.v, zero_e, return_fields=True, schedule=schedule)
        b, fb = tape.jvp(run.v, return_fields=True, schedule=schedule)
        assert np.array_equal(a, b) and np.array_equal(fa, fb) and np.any(b != 0)
        a, fa = tape.jvp_joint(zero_v, run.ve, return_fields=True, schedule=schedule)
        b, fb = tape.jvp_source(run.ve, return_fields=True, schedule=schedule)
        assert np.array_equal(a, b) and np.array_equal(fa, fb) and np.any(b != 0)
    tape.free()


# ---- 2. gauss_newton_joint
@DTYPES
@WRT
def test_gauss_newton_joint_bits(wrt, dt):
    run = Run(FC.shape_case(SOLVE_NN), dt, wrt)
    tape = run.tape
    scale = np.array(SCALE, dtype=dt)
    per_point = np.stack([scale, scale[::-1]]).astype(dt)   # (n_points, 4): a scale of its own per point
    assert per_point.shape == (tape.n_points, 4)
    for rw in (None, run.rw):
        for sc in (None, SCALE, per_point):
            ref_s, ref_e = run.ref_gn(run.v, run.ve, rw, sc)
            assert np.any(ref_s != 0) and np.any(ref_e != 0) and ref_e.shape == (tape.n_points, 4)
            if sc is not None:
                assert np.all(ref_e[np.broadcast_to(np.asarray(sc), ref_e.shape) == 0] == 0)
            for schedule in SCHEDULES:
                g_s, g_e = tape.gauss_newton_joint(run.v, run.ve, row_weight=rw, source_scale=sc, schedule=schedule)
                assert isinstance(tape.passes, tuple) and min(tape.passes) >= 1 and g_s.dtype == dt and g_e.dtype == dt
                _bits_equal(g_s, ref_s)
                _bits_equal(g_e, ref_e)
            # ... and the three calls it replaces, composed by hand
            ve = run.ve if sc is None else (np.broadcast_to(np.asarray(sc, dtype=dt), run.ve.shape) * run.ve).astype(dt)
            dtt = tape.jvp_joint(run.v, ve)
            h_s, h_e = tape.vjp(dtt if rw is None else (rw * dtt).astype(dt), return_source_grad=True)
            _bits_equal(g_s, h_s)
            _bits_equal(g_e, h_e if sc is None else (np.broadcast_to(np.asarray(sc, dtype=dt), h_e.shape) * h_e).astype(dt))
    tape.free()


# ---- 3. solve_joint
def _reference(run, rhs, rhs_e, rw, smooth, damp, sdamp, scale, maxiter, rtol=1e-6, schedule="tiled"):
    tape, dt = run.tape, run.dt
    return JR.cg(lambda ps, pe: tape.gauss_newton_joint(ps, pe, row_weight=rw, source_scale=scale, schedule=schedule), rhs, rhs_e, dt,
                 smooth_op=lambda p: NR.smooth(p, run.params(), run.case.dx, WEIGHTS, dtype=dt), smooth=smooth, damp=damp,
                 source_damp=sdamp, source_scale=scale, maxiter=maxiter, rtol=rtol)


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
    return rng.standard_normal(run.tape.n_cols).astype(run.dt), rng.standard_normal((run.n_points, 4)).astype(run.dt)


@DTYPES
@WRT
@pytest.mark.parametrize("reg", sorted(REG))
def test_solve_joint_bits(reg, wrt, dt):
    run = Run(FC.shape_case(SOLVE_NN), dt, wrt)
    tape = run.tape
    smooth, damp = REG[reg]
    rhs, rhs_e = _rhs(run, 59)
    kw = dict(smooth=smooth, smooth_weights=WEIGHTS, damp=damp, return_info=True)
    for sdamp, scale in ((0.0, None), (SDAMP, SCALE), (0.5, None), (0.0, SCALE)):
        for rw in (None, run.rw):
            for maxiter in (1, 2, 3, 4):
                ref = _reference(run, rhs, rhs_e, rw, smooth, damp, sdamp, scale, maxiter)
                got = tape.solve_joint(rhs, rhs_e, row_weight=rw, source_damp=sdamp, source_scale=scale, maxiter=maxiter, **kw)
                _same(got, ref)
                assert got[2]["status"] == 1 and got[2]["iterations"] == maxiter and got[1].shape == (run.n_points, 4)
                if scale is not None:
                    assert np.all(got[1][:, 2] == 0) and np.any(got[1][:, :2] != 0)
            _same(tape.solve_joint(rhs, rhs_e, row_weight=rw, source_damp=sdamp, source_scale=scale, maxiter=4, schedule="jacobi", **kw), ref)
    x, xe = tape.solve_joint(rhs, rhs_e, row_weight=run.rw, smooth=smooth, smooth_weights=WEIGHTS, damp=damp, source_scale=SCALE, maxiter=4)
    _bits_equal(x, ref[0])
    _bits_equal(xe, ref[1])
    tape.free()


def _one_event(nn):
    rng = np.random.default_rng(sum(nn))
    src = [np.floor(0.4 * (nn[a] - 1)) + (0.3, 0.6, 0.2)[a] for a in range(3)]
    return FC.Case("x".join(map(str, nn)), nn, FC.DX, FC.ZERO, FC.model(nn, FC.DX, FC.ZERO, "rough"),
                   [FC._event(FC.at(nn, FC.DX, FC.ZERO, [src]), FC.receivers(nn, FC.DX, FC.ZERO, rng, 6), 0.125)])


@DTYPES
@pytest.mark.parametrize("nn", [(11, 31, 3), (16, 8, 8)], ids=["seam_inside_a_chunk", "seam_on_a_chunk_boundary"])
def test_solve_joint_block_seam(nn, dt):
    run = Run(_one_event(nn), dt)
    tape = run.tape
    assert tape.n_cols in (1023, 1024) and tape.n_cols + 4 * tape.n_points == tape.n_cols + 4
    rhs = FC.wide_weights(np.random.default_rng(67), tape.n_cols, dt)
    rhs_e = FC.wide_weights(np.random.default_rng(68), 4, dt).reshape(1, 4)
    smooth, damp = REG["both"]
    for maxiter in (1, 4):
        got = tape.solve_joint(rhs, rhs_e, row_weight=run.rw, smooth=smooth, smooth_weights=WEIGHTS, damp=damp, source_damp=SDAMP,
                               source_scale=(1.0, 0.05, 0.05, 0.1), maxiter=maxiter, return_info=True)
        _same(got, _reference(run, rhs, rhs_e, run.rw, smooth, damp, SDAMP, (1.0, 0.05, 0.05, 0.1), maxiter))
    tape.free()


@DTYPES
def test_solve_joint_statuses_and_the_all_zero_scale(dt):
    run = Run(FC.shape_case(SOLVE_NN), dt)
    tape = run.tape
    rhs, rhs_e = _rhs(run, 61)
    # heavy damping of both blocks: the residual test is met within a few iterations
    kw = dict(smooth=1e-3, smooth_weights=WEIGHTS, damp=50.0, source_damp=50.0, source_scale=SCALE, maxiter=30, rtol=1e-4)
    got = tape.solve_joint(rhs, rhs_e, return_info=True, **kw)
    _same(got, _reference(run, rhs, rhs_e, None, 1e-3, 50.0, 50.0, SCALE, 30, rtol=1e-4))
    info = got[2]
    assert info["status"] == 0 and 1 <= info["iterations"] < 30 and info["rho"][-1] <= 1e-8 * info["rho"][0]
    # row_weight = 0 and no regularisation: <p, A p> = 0, no update, x stays zero
    zero = np.zeros(tape.n_data, dtype=dt)
    x, xe, info = tape.solve_joint(rhs, rhs_e, row_weight=zero, maxiter=4, return_info=True)
    assert info["status"] == 2 and info["iterations"] == 0 and info["pq"] == [0.0] and len(info["rho"]) == 2
    assert not np.any(x) and not np.any(xe)
    _same((x, xe, info), _reference(run, rhs, rhs_e, zero, 0.0, 0.0, 0.0, None, 4))
    # source_scale all zeros: the slowness block is solve_normal's, element for element
    smooth, damp = REG["both"]
    for rw in (None, run.rw):
        for sdamp in (0.0, SDAMP):
            x, xe, info = tape.solve_joint(rhs, rhs_e, row_weight=rw, smooth=smooth, smooth_weights=WEIGHTS, damp=damp, source_damp=sdamp,
                                           source_scale=(0.0, 0.0, 0.0, 0.0), maxiter=4, return_info=True)
            xn, info_n = tape.solve_normal(rhs, row_weight=rw, smooth=smooth, smooth_weights=WEIGHTS, damp=damp, maxiter=4, return_info=True)
            assert not np.any(xe) and np.array_equal(x, xn) and np.any(xn != 0)
            assert info["rho"] == info_n["rho"] and info["pq"] == info_n["pq"] and info["iterations"] == info_n["iterations"] == 4
    with pytest.raises(ValueError, match="hessian"):
        tape.solve_joint(rhs, rhs_e, hessian="newton")
    tape.free()


@DTYPES
@WRT
def test_release_joint_and_solve_normal_unchanged(wrt, dt):
    run = Run(FC.shape_case(SOLVE_NN), dt, wrt)
    tape = run.tape
    rhs, rhs_e = _rhs(run, 79)
    nkw = dict(smooth=2e-2, smooth_weights=WEIGHTS, damp=1e-1, maxiter=3, return_info=True)
    tape.gauss_newton_joint(run.v, run.ve, run.rw, SCALE)     # (what the products allocate is not the solver's)
    xn, info_n = tape.solve_normal(rhs, row_weight=run.rw, **nkw)
    before = tape.nbytes
    kw = dict(row_weight=run.rw, source_damp=SDAMP, source_scale=SCALE, **nkw)
    x, xe, info = tape.solve_joint(rhs, rhs_e, **kw)
    elem = np.dtype(dt).itemsize
    n_joint = tape.n_cols + 4 * tape.n_points
    joint_bytes = 5 * n_joint * elem + 3 * 4 * tape.n_points * elem + 8 * -(-n_joint // 1024) + 48
    assert tape.nbytes == before + joint_bytes
    # solve_normal on the same tape: the same bits, and no more memory
    xn2, info_n2 = tape.solve_normal(rhs, row_weight=run.rw, **nkw)
    _bits_equal(xn2, xn)
    assert info_n2 == info_n and tape.nbytes == before + joint_bytes
    tape.release_solve()
    after_release_solve = tape.nbytes
    normal_bytes = 5 * tape.n_cols * elem + 8 * -(-tape.n_cols // 1024) + 48
    assert after_release_solve == before + joint_bytes - normal_bytes   # (the joint arrays are not solve_normal's, and stay)
    tape.release_joint()
    assert tape.nbytes == after_release_solve - joint_bytes
    tape.release_joint()                         # (a second release is a no-op)
    assert tape.nbytes == after_release_solve - joint_bytes
    x2, xe2, info2 = tape.solve_joint(rhs, rhs_e, **kw)
    _bits_equal(x2, x)
    _bits_equal(xe2, xe)
    assert info2 == info and tape.nbytes == after_release_solve
    _bits_equal(tape.solve_normal(rhs, row_weight=run.rw, **nkw)[0], xn)
    assert tape.nbytes == before + joint_bytes
    tape.free()


@DTYPES
def test_joint_gauss_newton_step(dt):
    from ttcr_amd.inversion import joint_gauss_newton_step

    run = Run(FC.shape_case(SOLVE_NN), dt)
    tape = run.tape
    rng = np.random.default_rng(83)
    residual = (1e-2 * rng.standard_normal(tape.n_data)).astype(dt)
    model = rng.uniform(0.4, 0.7, tape.n_cols).astype(dt)
    smooth, damp = dt(2e-2), dt(1e-1)
    for weight in (None, run.rw):
        b, b_e = tape.vjp(residual if weight is None else weight * residual, return_source_grad=True)
        b = b - smooth * tape.smooth(model, WEIGHTS)
        assert b.dtype == dt
        kw = dict(smooth=smooth, smooth_weights=WEIGHTS, damp=damp, source_damp=SDAMP, source_scale=SCALE, maxiter=4, return_info=True)
        want = tape.solve_joint(b, b_e, row_weight=weight, **kw)
        got = joint_gauss_newton_step(tape, residual, model, row_weight=weight, **kw)
        _bits_equal(got[0], want[0])
        _bits_equal(got[1], want[1])
        assert got[2] == want[2] and got[2]["iterations"] == 4 and np.any(got[1] != 0)
    tape.free()


# ---- 4. device tensors
def _torch_joint(dtname):
    import torch

    dt = np.dtype(dtname).type
    run = Run(FC.shape_case(SOLVE_NN), dt)
    tape = run.tape
    rhs, rhs_e = _rhs(run, 71)
    dev = lambda a: torch.as_tensor(a, device="cuda")   # noqa: E731
    ref = tape.jvp_joint(run.v, run.ve, return_fields=True)
    dtt, mu = tape.jvp_joint(dev(run.v), dev(run.ve), return_fields=True)
    assert dtt.is_cuda and mu.is_cuda
    _bits_equal(dtt.cpu().numpy(), ref[0])
    _bits_equal(mu.cpu().numpy(), ref[1])
    ref = tape.gauss_newton_joint(run.v, run.ve, run.rw, SCALE)
    t_v, t_ve = dev(run.v), dev(run.ve)
    g_s, g_e = tape.gauss_newton_joint(t_v, t_ve, dev(run.rw), SCALE)
    assert g_s.is_cuda and g_e.is_cuda and g_e.shape == (run.n_points, 4)
    _bits_equal(g_s.cpu().numpy(), ref[0])
    _bits_equal(g_e.cpu().numpy(), ref[1])
    _bits_equal(t_v.cpu().numpy(), run.v)         # (the arguments are read, not used as work arrays)
    _bits_equal(t_ve.cpu().numpy(), run.ve)
    kw = dict(smooth=2e-2, smooth_weights=WEIGHTS, damp=1e-1, source_damp=SDAMP, source_scale=SCALE, maxiter=3, return_info=True)
    ref = tape.solve_joint(rhs, rhs_e, row_weight=run.rw, **kw)
    t_rhs, t_rhs_e = dev(rhs), dev(rhs_e)
    x, xe, info = tape.solve_joint(t_rhs, t_rhs_e, row_weight=dev(run.rw), **kw)
    assert x.is_cuda and xe.is_cuda and info == ref[2]
    _bits_equal(x.cpu().numpy(), ref[0])
    _bits_equal(xe.cpu().numpy(), ref[1])
    _bits_equal(t_rhs.cpu().numpy(), rhs)
    _bits_equal(t_rhs_e.cpu().numpy(), rhs_e)
    x, xe, info = tape.solve_joint(rhs, t_rhs_e, row_weight=run.rw, **kw)   # mixed: the result lives with the first tensor
    assert x.is_cuda and xe.is_cuda and info == ref[2]
    _bits_equal(xe.cpu().numpy(), ref[1])


@DTYPES
def test_joint_calls_with_device_tensors(dt):
    _in_child("joint", np.dtype(dt).name)
