"""The coarse model grid of a field tape on the device (Grid3d.raytrace_adjoint(..., wrt='model', model_shape=...)).  On six
pairs of fine and model shapes, two events each (an off-node source and an on-node one): the fields are those of a NODE tape of the same
grid and slowness, and every product of the model tape is bit-equal to the node tape's product composed call by call with the restated P
and P^T (tests/model_reference.py); prolong and restrict on the tape and on the grid, host and device arguments; smooth and the three
solves against tests/normal_reference.py / tests/joint_reference.py driven with the composed product and the per-axis R;
<w, J v> = <J^T w, v> to rounding on the device; the torch operators; refusals, lengths, lifetime and device lists.

The issue's table names a fine grid of 9 x 9 x 1 nodes; a grid needs two nodes per axis, so the thin axis here has two (model 3 x 3 x 1:
the model is still constant along it)."""
import ctypes as C
import gc
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
import model_reference as MR  # noqa: E402
import normal_reference as NR  # noqa: E402
import receiver_reference as RR  # noqa: E402
from field_tape_cases import DOT_TOL, _bits_equal  # noqa: E402  (fp32 5e-5, fp64 1e-12: the bounds of tests/test_cell_tape_gpu.py)

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
SCHEDULES = ("tiled", "jacobi")
DX, ZERO = FC.DX, FC.ZERO
# fine shape, model shape
CASES = [((5, 7, 4), (2, 3, 2)),        # smallest general case
         ((17, 9, 11), (4, 3, 5)),      # non-integer ratios
         ((13, 13, 13), (1, 1, 4)),     # layered 1-D model
         ((9, 9, 2), (3, 3, 1)),        # thin fine axis
         ((9, 9, 9), (9, 9, 9)),        # identity
         ((37, 35, 41), (5, 4, 6))]     # several workgroups per stage, the last partly filled


def _ids(v):
    return "x".join(map(str, v))


CASE_IDS = ["%s_%s" % (_ids(n), _ids(m)) for n, m in CASES]


def _in_child(fn, *args):
    """Run _torch_<fn>(*args) of this module in a fresh process that initialises torch's device before the first grid"""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_model_grid_gpu as t; t._torch_%s(*%r)"
            % (HERE, ROOT, fn, args))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def _grid(nn, dt, s, **kw):
    import ttcr_amd

    axes = [np.arange(n) * DX for n in nn]
    kw.setdefault("weno", 0)
    g = ttcr_amd.Grid3d(*axes, cell_slowness=0, method="FSM", dtype=dt, tt_from_rp=0, **kw)
    g.set_slowness(np.asarray(s).reshape(nn, order="F"))
    return g


def events(nn):
    """event 0: an off-node source; event 1: a source on a node; FC.receivers for each"""
    rng = np.random.default_rng(3000 + nn[0] * 10000 + nn[1] * 100 + nn[2])
    src0 = [np.floor(0.4 * (nn[a] - 1)) + (0.3, 0.6, 0.2)[a] for a in range(3)]
    src0 = [min(src0[a], nn[a] - 1 - 0.25) for a in range(3)]
    src1 = [(2 * (nn[a] - 1)) // 3 for a in range(3)]
    ev = [dict(pts=FC.at(nn, DX, ZERO, [p]), t0=t0, rcv=FC.receivers(nn, DX, ZERO, rng)) for p, t0 in ((src0, 0.125), (src1, 0.0))]
    return FC.Case(_ids(nn), nn, DX, ZERO, FC.model(nn, DX, ZERO, "rough"), ev)


class Pair:
    """the model tape of a case and the node tape of the same grid and slowness (which is not in the range of P)"""

    def __init__(self, nn, m, dt, **kw):
        case = events(nn)
        self.dt, self.nn, self.m = np.dtype(dt), nn, m
        self.n_nodes, self.n_model = int(np.prod(nn)), int(np.prod(m))
        self.s = np.asarray(case.s, dtype=dt)
        self.src, self.rcv, agg, self.rows = FC.call_arrays(case, np.random.default_rng(61))
        self.grid = _grid(nn, dt, self.s, **kw)
        tt, self.model = self.grid.raytrace_adjoint(self.src, self.rcv, aggregate_src=agg, wrt="model", model_shape=m)
        t = self.model
        assert (t.wrt, t.model_shape, t.n_events, t.n_data, t.n_cols, t.n_nodes) == ("model", tuple(m), 2, self.rcv.shape[0], self.n_model,
                                                                                      self.n_nodes) and t.nbytes > 0
        tt_n, self.node = self.grid.raytrace_adjoint(self.src, self.rcv, aggregate_src=agg)
        assert (self.node.wrt, self.node.model_shape, self.node.n_cols) == ("nodes", None, self.n_nodes)
        _bits_equal(tt_n, tt)
        for e in range(2):
            _bits_equal(t.field(e), self.node.field(e))
        # the model tape holds the staged model vector, the axis tables and the two intermediates of P^T more than the node tape
        el = self.dt.itemsize
        extra = (max(self.n_model * el, 1) + max(nn[0] * nn[1] * m[2] * el, 1) + max(nn[0] * m[1] * m[2] * el, 1) + sum(nn) * 4 + 2 * sum(nn) * el)
        assert t.nbytes == self.node.nbytes + extra, (t.nbytes, self.node.nbytes, extra)
        rng = np.random.default_rng(67)
        self.w = FC.wide_weights(rng, self.rcv.shape[0], dt)
        self.fc = rng.standard_normal((2, self.n_nodes)).astype(dt)
        self.v = rng.standard_normal(self.n_model).astype(dt)
        self.rw = rng.uniform(0.5, 2.0, self.rcv.shape[0]).astype(dt)

    def P(self, v):
        return MR.prolong(np.asarray(v, dtype=self.dt), self.nn, self.m, self.dt)

    def Pt(self, g):
        assert g.dtype == self.dt and g.shape == (self.n_nodes,)
        return MR.restrict(g, self.nn, self.m, self.dt)

    def check_maps(self):
        t, g = self.model, self.grid
        u = np.random.default_rng(71).standard_normal(self.n_nodes).astype(self.dt)
        Pv, Ptu = self.P(self.v), self.Pt(u)
        assert np.any(Pv != 0) and np.any(Ptu != 0)
        for got in (t.prolong(self.v), g.prolong(self.v, self.m)):
            assert isinstance(got, np.ndarray)
            _bits_equal(got, Pv)
        for got in (t.restrict(u), g.restrict(u, self.m)):
            _bits_equal(got, Ptu)
        if self.m == self.nn:
            _bits_equal(Pv, self.v)
            _bits_equal(Ptu, u)

    def check_products(self):
        c, n, dt = self.model, self.node, self.dt
        Pv = self.P(self.v)
        out = {}
        for schedule in SCHEDULES:
            for kind, (ww, ff) in {"receivers": (self.w, None), "field": (None, self.fc), "both": (self.w, self.fc)}.items():
                g = c.vjp(ww, ff, schedule=schedule)
                assert g.shape == (self.n_model,) and g.dtype == dt and c.passes >= 1
                _bits_equal(g, self.Pt(n.vjp(ww, ff, schedule=schedule)))
                out[kind] = g
            dtt, mu = c.jvp(self.v, return_fields=True, schedule=schedule)
            ref_dtt, ref_mu = n.jvp(Pv, return_fields=True, schedule=schedule)
            _bits_equal(dtt, ref_dtt)
            _bits_equal(mu, ref_mu)
            gn = c.gauss_newton(self.v, self.rw, schedule=schedule)
            assert isinstance(c.passes, tuple) and gn.shape == (self.n_model,)
            _bits_equal(gn, self.Pt(n.vjp(self.rw * ref_dtt, schedule=schedule)))
            _bits_equal(gn, self.Pt(n.gauss_newton(Pv, self.rw, schedule=schedule)))
            # hold / hvp / newton: P^T H P
            gh = c.hold(self.w, self.fc, return_grad=True, schedule=schedule)
            n.hold(self.w, self.fc, schedule=schedule)
            _bits_equal(gh, out["both"])
            _bits_equal(c.hvp(self.v, schedule=schedule), self.Pt(n.hvp(Pv, schedule=schedule)))
            _bits_equal(c.newton(self.v, self.rw, schedule=schedule), self.Pt(n.newton(Pv, self.rw, schedule=schedule)))
            # the joint products: the model block through the maps, the other block as it is
            vs = np.random.default_rng(73).standard_normal((c.n_points, 4)).astype(dt)
            a, b = c.gauss_newton_joint(self.v, vs, self.rw, schedule=schedule), n.gauss_newton_joint(Pv, vs, self.rw, schedule=schedule)
            _bits_equal(a[0], self.Pt(b[0]))
            _bits_equal(a[1], b[1])
            vr = np.random.default_rng(79).standard_normal((c.n_rcv_points, 4)).astype(dt)
            a = c.gauss_newton_receiver_joint(self.v, vr, self.rw, schedule=schedule)
            b = n.gauss_newton_receiver_joint(Pv, vr, self.rw, schedule=schedule)
            _bits_equal(a[0], self.Pt(b[0]))
            _bits_equal(a[1], b[1])
        c.release()
        n.release()
        assert all(np.all(np.isfinite(g)) and np.any(g != 0) for g in out.values()) and np.any(ref_dtt != 0)
        return out

    def check_pairs(self):
        """gauss_newton with pair_weight: B = diag(rw) + Q^T diag(pw) Q between the two relaxations"""
        c, n = self.model, self.node
        nd = self.rcv.shape[0]
        rng = np.random.default_rng(83)
        a = rng.integers(0, nd, 9)
        b = (a + 1 + rng.integers(0, nd - 1, 9)) % nd
        pw = rng.uniform(0.5, 2.0, 9).astype(self.dt)
        for t in (c, n):
            t.set_row_pairs(a, b)
        Pv = self.P(self.v)
        for schedule in SCHEDULES:
            _bits_equal(c.gauss_newton(self.v, self.rw, schedule=schedule, pair_weight=pw),
                        self.Pt(n.gauss_newton(Pv, self.rw, schedule=schedule, pair_weight=pw)))
        for t in (c, n):
            t.release_pairs()

    def check_blocks(self):
        c, n, dt = self.model, self.node, self.dt
        rng = np.random.default_rng(89)
        for K in (1, 3, 5):
            V = rng.standard_normal((K, self.n_model)).astype(dt)
            W = np.stack([FC.wide_weights(rng, self.rcv.shape[0], dt) for _ in range(K)])
            PV = np.stack([self.P(v) for v in V])
            for schedule in SCHEDULES:
                a, b = c.jvp_block(V, return_fields=True, schedule=schedule), n.jvp_block(PV, return_fields=True, schedule=schedule)
                _bits_equal(a[0], b[0])
                _bits_equal(a[1], b[1])
                _bits_equal(c.vjp_block(W, schedule=schedule), np.stack([self.Pt(g) for g in n.vjp_block(W, schedule=schedule)]))
                _bits_equal(c.gauss_newton_block(V, self.rw, schedule=schedule),
                            np.stack([self.Pt(g) for g in n.gauss_newton_block(PV, self.rw, schedule=schedule)]))
        c.release_block()
        n.release_block()

    def check_dot(self):
        """<w, J v> against <J^T w, v> on the device with the moduli of the inputs (FC.dot_errors)"""
        c = self.model
        wp, fcp, vp = np.abs(self.w), np.abs(self.fc), np.abs(self.v)
        dtt_p, mu_p = c.jvp(vp, return_fields=True)
        e_rcv, e_fld = FC.dot_errors(wp, dtt_p, c.vjp(wp), fcp, mu_p, c.vjp(None, fcp), vp)
        print("model %s on %s, %s: device <w, J v> against <J^T w, v>: receivers %.2e, field %.2e (bound %.0e)"
              % (_ids(self.m), _ids(self.nn), self.dt.name, e_rcv, e_fld, DOT_TOL[self.dt]))
        assert e_rcv <= DOT_TOL[self.dt] and e_fld <= DOT_TOL[self.dt], (e_rcv, e_fld)


@DTYPES
@pytest.mark.parametrize("nn,m", CASES, ids=CASE_IDS)
def test_model_tape_against_the_node_tape(nn, m, dt):
    p = Pair(nn, m, dt)
    if nn == CASES[-1][0]:   # every stage of P^T and P itself: more than one workgroup, the last one partly filled
        for count in (p.n_nodes, nn[0] * nn[1] * m[2], nn[0] * m[1] * m[2]):
            assert count > 256 and count % 256 != 0
    p.check_maps()
    p.check_products()
    p.check_pairs()
    p.check_dot()


@DTYPES
@pytest.mark.parametrize("nn,m", CASES, ids=CASE_IDS)
def test_model_tape_block_products(nn, m, dt):
    Pair(nn, m, dt).check_blocks()


# ---- smooth and the solves
SOLVES = [((17, 9, 11), (4, 3, 5), (1.0, 0.5, 2.0)), ((13, 13, 13), (1, 1, 4), (0.0, 0.0, 1.0))]
SMOOTH, DAMP = 2e-2, 1e-1


def _same(got, ref):
    assert len(got) == len(ref)
    for a, b in zip(got[:-1], ref[:-1]):
        _bits_equal(a, b)
    info, inf_r = got[-1], ref[-1]
    assert info["status"] == inf_r["status"] and info["iterations"] == inf_r["iterations"], (info, inf_r)
    assert info["rho"] == inf_r["rho"] and info["pq"] == inf_r["pq"], (info, inf_r)


@DTYPES
@pytest.mark.parametrize("nn,m,weights", SOLVES, ids=["%s_%s" % (_ids(s[0]), _ids(s[1])) for s in SOLVES])
def test_smooth_and_solves_bits(nn, m, weights, dt):
    p = Pair(nn, m, dt)
    c, n = p.model, p.node
    rng = np.random.default_rng(59)
    R = lambda v: MR.smooth(v, nn, m, DX, weights, dt)   # noqa: E731
    _bits_equal(c.smooth(p.v, weights), R(p.v))
    assert np.any(R(p.v) != 0)
    rhs = rng.standard_normal(c.n_cols).astype(dt)
    x0 = (0.1 * rng.standard_normal(c.n_cols)).astype(dt)
    kw = dict(smooth=SMOOTH, smooth_weights=weights, damp=DAMP, return_info=True)
    for rw in (None, p.rw):
        H = lambda v, sch="tiled": p.Pt(n.gauss_newton(p.P(v), rw, schedule=sch))   # noqa: E731
        for start in (None, x0):
            for maxiter in (1, 3):
                ref = NR.cg(H, rhs, dt, smooth_op=R, smooth=SMOOTH, damp=DAMP, x0=start, maxiter=maxiter)
                _same(c.solve_normal(rhs, row_weight=rw, x0=start, maxiter=maxiter, **kw), ref)
            _same(c.solve_normal(rhs, row_weight=rw, x0=start, maxiter=3, schedule="jacobi", **kw), ref)
        rhs_s = rng.standard_normal((c.n_points, 4)).astype(dt)
        Hj = lambda v, ve: (lambda g: (p.Pt(g[0]), g[1]))(n.gauss_newton_joint(p.P(v), ve, row_weight=rw))   # noqa: E731
        ref = JR.cg(Hj, rhs, rhs_s, dt, smooth_op=R, smooth=SMOOTH, damp=DAMP, source_damp=0.5, maxiter=3)
        _same(c.solve_joint(rhs, rhs_s, row_weight=rw, source_damp=0.5, maxiter=3, **kw), ref)
        rhs_r = rng.standard_normal((c.n_rcv_points, 4)).astype(dt)
        Hr = lambda v, ve: (lambda g: (p.Pt(g[0]), g[1]))(n.gauss_newton_receiver_joint(p.P(v), ve, row_weight=rw))   # noqa: E731
        ref = RR.cg(Hr, rhs, rhs_r, dt, smooth_op=R, smooth=SMOOTH, damp=DAMP, rcv_damp=0.5, maxiter=3)
        _same(c.solve_receiver_joint(rhs, rhs_r, row_weight=rw, rcv_damp=0.5, maxiter=3, **kw), ref)
    if min(m) < 3:   # a short axis takes weight 0: refused before the device, by smooth and by a solve that smooths; not without smoothing
        for bad in ((1.0, 0.0, 1.0), (0.0, 0.5, 1.0)):
            with pytest.raises(ValueError, match="weight 0"):
                c.smooth(p.v, bad)
            with pytest.raises(ValueError, match="weight 0"):
                c.solve_normal(rhs, smooth=1.0, smooth_weights=bad)
        assert c.solve_normal(rhs, smooth=0.0, smooth_weights=(1.0, 1.0, 1.0), damp=1.0, maxiter=2).shape == (c.n_cols,)


@DTYPES
def test_gauss_newton_step_and_update_on_a_model_tape(dt):
    from ttcr_amd import inversion

    nn, m, weights = SOLVES[0]
    p = Pair(nn, m, dt)
    c = p.model
    res = np.random.default_rng(97).standard_normal(c.n_data).astype(dt)
    model = np.random.default_rng(98).uniform(0.3, 0.6, c.n_cols).astype(dt)
    x = inversion.gauss_newton_step(c, res, model, row_weight=p.rw, smooth=SMOOTH, damp=DAMP, smooth_weights=weights, maxiter=3)
    b = c.vjp(p.rw * res) - SMOOTH * c.smooth(model, weights)
    _bits_equal(x, c.solve_normal(b, row_weight=p.rw, smooth=SMOOTH, damp=DAMP, smooth_weights=weights, maxiter=3))
    _bits_equal(inversion.apply_model_update(c, p.s, x), p.s + p.P(x))
    xs, ys, zs = c.model_coordinates()
    assert np.array_equal(xs, np.arange(m[0]) * (DX * (nn[0] - 1) / (m[0] - 1))) and ys[-1] == DX * (nn[1] - 1) and zs.shape == (m[2],)


# ---- refusals and lengths
def test_refusals_and_lengths():
    import ttcr_amd
    from ttcr_amd import _lib
    from ttcr_amd.rgrid import _ptr

    nn, m, dt = (9, 8, 7), (3, 2, 4), np.float32
    p = Pair(nn, m, dt)
    src, rcv, g = p.src, p.rcv, p.grid
    with pytest.raises(ValueError, match="model_shape goes with"):
        g.raytrace_adjoint(src, rcv, model_shape=m)
    with pytest.raises(ValueError, match="needs model_shape"):
        g.raytrace_adjoint(src, rcv, wrt="model")
    for bad in ((0, 2, 4), (3, 9, 4), (3, 2)):
        with pytest.raises(ValueError, match="model_shape"):
            g.raytrace_adjoint(src, rcv, wrt="model", model_shape=bad)
        with pytest.raises(ValueError, match="model_shape"):
            g.prolong(p.v, bad)
    # the C entries: a shape outside the range and a cell grid are value errors, 2-D and WENO grids unsupported
    vTx, vt0, vRx, iRx = g._split_sources(src, rcv, False)
    tx_off, tx, t0, rx_off, rx, out = g._event_arrays(vTx, vt0, vRx)
    args = (len(vTx), _ptr(tx_off), _ptr(tx), _ptr(t0), _ptr(rx_off), _ptr(rx), _ptr(out))
    h = C.c_void_p()
    buf_m, buf_n = np.zeros(p.n_model, dtype=dt), np.zeros(p.n_nodes, dtype=dt)
    lib = g._lib
    for bad in ((3, 2, 8), (0, 2, 4)):
        shape = (C.c_int * 3)(*bad)
        assert lib.ttcr_fsm_model_raytrace_multi_adjoint(g._h, *args, C.byref(h), shape) == _lib.ERR_VALUE and not h.value
        assert "model_shape" in _lib.last_error()
        assert lib.ttcr_fsm_model_prolong(g._h, shape, _ptr(buf_m), 0, _ptr(buf_n), 0) == _lib.ERR_VALUE
        assert lib.ttcr_fsm_model_restrict(g._h, shape, _ptr(buf_n), 0, _ptr(buf_m), 0) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_model_raytrace_multi_adjoint(g._h, *args, C.byref(h), None) == _lib.ERR_VALUE and "null model_shape" in _lib.last_error()
    shape = (C.c_int * 3)(*m)
    axes = [np.arange(k) * DX for k in nn]
    gcell = ttcr_amd.Grid3d(*axes, cell_slowness=1, method="FSM", dtype=dt, tt_from_rp=0, weno=0)
    gweno = ttcr_amd.Grid3d(*axes, cell_slowness=0, method="FSM", dtype=dt, tt_from_rp=0, weno=1)
    g2 = ttcr_amd.Grid2d(axes[0], axes[2], cell_slowness=0, method="FSM", dtype=dt)
    for grid, status, word in ((gcell, _lib.ERR_VALUE, "cells"), (gweno, _lib.ERR_UNSUPPORTED, "weno"), (g2, _lib.ERR_UNSUPPORTED, "3-D")):
        assert lib.ttcr_fsm_model_raytrace_multi_adjoint(grid._h, *args, C.byref(h), shape) == status and not h.value
        assert word in _lib.last_error()
        assert lib.ttcr_fsm_model_prolong(grid._h, shape, _ptr(buf_m), 0, _ptr(buf_n), 0) == status
        assert lib.ttcr_fsm_model_restrict(grid._h, shape, _ptr(buf_n), 0, _ptr(buf_m), 0) == status
    with pytest.raises(ValueError, match="at the nodes"):
        gcell.raytrace_adjoint(src, rcv, wrt="model", model_shape=m)
    with pytest.raises(NotImplementedError, match="weno"):
        gweno.raytrace_adjoint(src, rcv, wrt="model", model_shape=m)
    with pytest.raises(NotImplementedError, match="weno"):
        gweno.prolong(p.v, m)
    # a node tape has no model grid; ttcr_fsm_adjoint_model keeps its answers
    for call in (lambda: p.node.prolong(p.v), lambda: p.node.restrict(buf_n), p.node.model_coordinates):
        with pytest.raises(ValueError, match="no coarse model grid"):
            call()
    assert lib.ttcr_fsm_model_tape_prolong(p.node._h, _ptr(buf_m), 0, _ptr(buf_n), 0) == _lib.ERR_VALUE
    cells, npar, nno = C.c_int(7), C.c_size_t(0), C.c_size_t(0)
    for tape, want in ((p.node, p.n_nodes), (p.model, p.n_model)):
        assert lib.ttcr_fsm_adjoint_model(tape._h, C.byref(cells), C.byref(npar), C.byref(nno)) == 0
        assert (cells.value, npar.value, nno.value) == (0, want, p.n_nodes)
    # lengths: the model vector has n_cols values, rows n_data, fields n_nodes
    c = p.model
    for bad in (np.ones(p.n_nodes, dtype=dt), np.ones(p.n_model + 1, dtype=dt), np.ones(3, dtype=dt)):
        for call in (c.jvp, c.gauss_newton, c.prolong, c.smooth, lambda b: c.solve_normal(b, damp=1.0), lambda b: c.dot(b, b),
                     lambda b: c.jvp_block(b[None, :]), lambda b: c.gauss_newton_joint(b, np.zeros((c.n_points, 4), dtype=dt))):
            with pytest.raises(ValueError, match="per model node|should be"):
                call(bad)
    with pytest.raises(ValueError, match="per node"):
        c.restrict(np.ones(p.n_model, dtype=dt))
    with pytest.raises(ValueError, match="field_cotangent"):
        c.vjp(None, np.ones((2, p.n_model), dtype=dt))
    assert c.vjp(None, np.ones((2, p.n_nodes), dtype=dt)).shape == (p.n_model,)


# ---- lifetime and several devices
def test_model_tape_after_set_slowness_and_without_its_grid():
    nn, m, dt = (13, 11, 12), (4, 3, 5), np.float64
    p = Pair(nn, m, dt)
    c = p.model
    g0, d0, n0, f0, pv = c.vjp(p.w, p.fc), c.jvp(p.v), c.gauss_newton(p.v, p.rw), c.field(1), c.prolong(p.v)
    p.grid.set_slowness((1.3 * p.s).reshape(nn, order="F"))
    _, other = p.grid.raytrace_adjoint(p.src, p.rcv, wrt="model", model_shape=m)
    assert not np.array_equal(other.vjp(p.w, p.fc), g0)
    del p.grid
    gc.collect()
    _bits_equal(c.vjp(p.w, p.fc), g0)
    _bits_equal(c.jvp(p.v), d0)
    _bits_equal(c.gauss_newton(p.v, p.rw), n0)
    _bits_equal(c.field(1), f0)
    _bits_equal(c.prolong(p.v), pv)
    c.free()
    c.free()
    with pytest.raises(ValueError):
        c.vjp(p.w)
    with pytest.raises(ValueError):
        c.prolong(p.v)


def _device_lists():
    from ttcr_amd import _lib

    lists = [[0, 0]]
    if _lib.load().ttcr_fsm_device_count() >= 2:   # (as tests/test_multi_device_gpu.py: distinct devices where the box has them)
        lists.append([0, 1])
    return lists


@DTYPES
def test_model_tape_on_device_lists(dt):
    nn, m = (17, 21, 15), (4, 1, 6)
    one = Pair(nn, m, dt, n_threads=4)
    ref = one.check_products()
    for devs in _device_lists():
        p = Pair(nn, m, dt, n_threads=4, device=devs)
        assert p.grid.n_devices == 2 and p.model.device == devs[0]
        _bits_equal(p.model.field(0), one.model.field(0))
        for schedule in SCHEDULES:
            _bits_equal(p.model.vjp(p.w, p.fc, schedule=schedule), ref["both"])
            _bits_equal(p.model.jvp(p.v, schedule=schedule), one.model.jvp(p.v, schedule=schedule))
            _bits_equal(p.model.gauss_newton(p.v, p.rw, schedule=schedule), one.model.gauss_newton(p.v, p.rw, schedule=schedule))
        _bits_equal(p.grid.prolong(p.v, m), one.P(p.v))


# ---- torch (child processes)
def _torch_maps(dtname):
    """device and CPU tensors through prolong / restrict of the tape and the grid; the autograd operators: backward of prolong is restrict
    and the other way round, forward_ad, double backward"""
    import torch
    import torch.autograd.forward_ad as fwAD

    import ttcr_amd.autograd as ag

    dt = np.dtype(dtname).type
    nn, m = (17, 9, 11), (4, 3, 5)
    p = Pair(nn, m, dt)
    t, g = p.model, p.grid
    u = np.random.default_rng(71).standard_normal(p.n_nodes).astype(dt)
    Pv, Ptu = p.P(p.v), p.Pt(u)
    for arg, to in ((torch.from_numpy(p.v), "cpu"), (torch.from_numpy(p.v).cuda(), "cuda")):
        for got in (t.prolong(arg), g.prolong(arg, m)):
            assert got.device.type == to
            _bits_equal(got.cpu().numpy(), Pv)
    for arg, to in ((torch.from_numpy(u), "cpu"), (torch.from_numpy(u).cuda(), "cuda")):
        for got in (t.restrict(arg), g.restrict(arg, m)):
            assert got.device.type == to
            _bits_equal(got.cpu().numpy(), Ptu)
    if torch.cuda.device_count() >= 2:   # a tensor of another device: moved to the grid's device, the result comes back to its own
        far = torch.from_numpy(p.v).to("cuda:1")
        got = g.prolong(far, m)
        assert got.device == far.device
        _bits_equal(got.cpu().numpy(), Pv)
        got = g.restrict(torch.from_numpy(u).to("cuda:1"), m)
        assert got.device == far.device
        _bits_equal(got.cpu().numpy(), Ptu)
    # device tensors in place through the products
    vd, rwd = torch.from_numpy(p.v).cuda(), torch.from_numpy(p.rw).cuda()
    for got, want in ((t.jvp(vd), t.jvp(p.v)), (t.gauss_newton(vd, rwd), t.gauss_newton(p.v, p.rw)),
                      (t.vjp(torch.from_numpy(p.w).cuda()), t.vjp(p.w)), (t.smooth(vd), t.smooth(p.v))):
        assert got.is_cuda
        _bits_equal(got.cpu().numpy(), want)
    for bad in (torch.ones(t.n_nodes, device="cuda"), torch.ones(3, device="cuda")):
        for call in (t.jvp, t.gauss_newton, t.prolong):
            try:
                call(bad)
            except ValueError:
                continue
            raise AssertionError("no ValueError")
    # the operators, in the (x, y, z) C-order layout of the torch side
    mt = torch.tensor(p.v.reshape(m, order="F"), device="cuda", requires_grad=True)
    ct = torch.from_numpy(u.reshape(nn, order="F").copy()).cuda()
    s = ag.prolong(g, mt, m)
    assert s.shape == nn and s.is_cuda
    _bits_equal(s.detach().cpu().numpy(), Pv.reshape(nn, order="F"))
    (grad,) = torch.autograd.grad((ct * s).sum(), mt, create_graph=True)
    _bits_equal(grad.detach().cpu().numpy(), Ptu.reshape(m, order="F"))
    # the backward is differentiable in its cotangent: d <c2, P^T ct> / d ct = P c2
    ctr = ct.clone().requires_grad_(True)
    (g2,) = torch.autograd.grad((ctr * ag.prolong(g, mt, m)).sum(), mt, create_graph=True)
    c2 = torch.from_numpy(np.random.default_rng(5).standard_normal(m).astype(dt)).cuda()
    (back,) = torch.autograd.grad((c2 * g2).sum(), ctr)
    _bits_equal(back.cpu().numpy(), p.P(c2.cpu().numpy().flatten("F")).reshape(nn, order="F"))
    gt = torch.from_numpy(u.reshape(nn, order="F").copy()).cuda().requires_grad_(True)
    r = ag.restrict(g, gt, m)
    _bits_equal(r.detach().cpu().numpy(), Ptu.reshape(m, order="F"))
    cm = torch.from_numpy(p.v.reshape(m, order="F").copy()).cuda()
    (gr,) = torch.autograd.grad((cm * r).sum(), gt)
    _bits_equal(gr.cpu().numpy(), Pv.reshape(nn, order="F"))
    tv = np.random.default_rng(7).standard_normal(m).astype(dt)
    with fwAD.dual_level():
        out = ag.prolong(g, fwAD.make_dual(mt.detach(), torch.from_numpy(tv).cuda()), m)
        tang = fwAD.unpack_dual(out).tangent.detach().clone()
    _bits_equal(tang.cpu().numpy(), p.P(tv.flatten("F")).reshape(nn, order="F"))


def _torch_chain():
    """raytrace_adjoint(grid, 1 / prolong(grid, m, shape)) differentiated in m: the model tape's vjp, to the rounding of the chain
    d(1 / s) = -1 / s^2 against the operator's own -1 / v^2.  Per node the two factors cancel within the roundings of the operator's
    product and quotient and of torch's backward of the division, 8 u at most; P^T then runs on node gradients that differ by that, and
    each of the two computed P^T is within (L_x + L_y + L_z + 3) u of its exact value (three products, L - 1 additions per stage).  The
    bar on every model value: (8 + 2 (L_x + L_y + L_z + 3)) u times P^T of the moduli of the node gradient."""
    import torch

    import ttcr_amd.autograd as ag

    dt = np.float32
    nn, m = (17, 9, 11), (4, 3, 5)
    p = Pair(nn, m, dt)
    rng = np.random.default_rng(17)
    mv = rng.uniform(0.3, 0.7, m).astype(dt)                       # model slowness, (mx, my, mz)
    mt = torch.tensor(mv, device="cuda", requires_grad=True)
    tt = ag.raytrace_adjoint(p.grid, 1.0 / ag.prolong(p.grid, mt, m), p.src, p.rcv)
    c_tt = rng.standard_normal(p.rcv.shape[0]).astype(dt)
    (torch.from_numpy(c_tt).cuda() * tt).sum().backward()
    s = p.grid.prolong(mv.flatten("F"), m)
    p.grid.set_velocity((1.0 / s).astype(dt).reshape(nn, order="F"))
    tt_ref, tape = p.grid.raytrace_adjoint(p.src, p.rcv, wrt="model", model_shape=m)
    _bits_equal(tt.detach().cpu().numpy(), tt_ref)
    want = tape.vjp(c_tt).astype(np.float64)
    L = MR.stage_lengths(nn, m)
    bound = (8 + 2 * (sum(L) + 3)) * (np.finfo(dt).eps / 2) * p.grid.restrict(np.abs(_node_vjp(p, c_tt)), m).astype(np.float64)
    got = mt.grad.cpu().numpy().flatten("F").astype(np.float64)
    err = np.abs(got - want)
    print("chain through 1 / prolong: worst |grad - model vjp| / bound = %.3f" % float(np.max(err / bound)))
    assert np.all(err <= bound)


def _node_vjp(p, c_tt):
    _, node = p.grid.raytrace_adjoint(p.src, p.rcv)
    return node.vjp(c_tt)


@DTYPES
def test_torch_maps_and_device_tensors(dt):
    _in_child("maps", np.dtype(dt).name)


def test_torch_chain_through_prolong():
    _in_child("chain")
