"""The field tape of 3-D cell grids on the device (Grid3d.raytrace_adjoint(..., wrt='cells')).  On the shapes of
tests/field_tape_cases.py with cells = nodes - 1: traveltimes and fields are those of raytrace and of the oracle; every product of the
cell tape is bit-equal to the same product of a NODE tape of the same geometry and node slowness A sc composed with the oracle's A
(cells_to_nodes3d) or the restated A^T (tests/cell_reference.py); <w, J v> = <J^T w, v> to rounding on the device; the torch operators
with wrt='cells'; refusals, lengths, lifetime and device lists."""
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
import cell_reference as CR  # noqa: E402
import field_tape_cases as FC  # noqa: E402
from field_tape_cases import DOT_TOL, _bits_equal  # noqa: E402  (fp32 5e-5, fp64 1e-12: the bounds of the existing edge tests)

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
SCHEDULES = ("tiled", "jacobi")
DX, ZERO = FC.DX, FC.ZERO
# node counts: the shapes of the edge tests (1 x 1 x 1 to 28 x 40 x 30 cells, every axis the short one once) and 17 x 9 x 11 cells, 1683 of
# them: seven workgroups of the A^T kernel, the last one partly filled
SHAPES = FC.SHAPES + [(18, 10, 12)]


def _in_child(fn, *args):
    """Run _torch_<fn>(*args) of this module in a fresh process that initialises torch's device before the first grid"""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_cell_tape_gpu as t; t._torch_%s(*%r)"
            % (HERE, ROOT, fn, args))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def _cells(nn):
    return tuple(n - 1 for n in nn)


def cell_model(nn, kind):
    """cell slowness, flat, x fastest: `rough` a smooth trend times 1 +- 30 % noise, `homogeneous` 0.5, `two_layers` 0.5 in the cell
    layers below ncz // 2 and 0.25 above"""
    nc = _cells(nn)
    ax = [0.5 * (np.arange(n) + 0.5) for n in nc]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    if kind == "rough":
        s = 0.5 + 0.02 * X + 0.015 * Y + 0.03 * Z + 0.05 * np.sin(0.9 * X) * np.cos(0.7 * Y + 0.3 * Z)
        s = s * (1.0 + 0.30 * np.random.default_rng(13).uniform(-1, 1, s.shape))
    elif kind == "homogeneous":
        s = np.full(X.shape, 0.5)
    elif kind == "two_layers":
        s = np.where(np.arange(nc[2])[None, None, :] < nc[2] // 2, 0.5, 0.25) * np.ones(X.shape)
    else:
        raise ValueError(kind)
    return s.flatten("F")


def _grid(nn, dt, cell, s, **kw):
    import ttcr_amd

    axes = [np.arange(n) * DX for n in nn]
    kw.setdefault("weno", 0)
    g = ttcr_amd.Grid3d(*axes, cell_slowness=1 if cell else 0, method="FSM", dtype=dt, tt_from_rp=0, **kw)
    g.set_slowness(np.asarray(s).reshape(_cells(nn) if cell else nn, order="F"))
    return g


def shape_events(nn):
    """the two sources of FC.shape_case (off node; in the last cell of the far corner), FC.receivers for each"""
    rng = np.random.default_rng(2000 + nn[0] * 10000 + nn[1] * 100 + nn[2])
    case = FC.shape_case(nn)
    ev = [dict(pts=e["pts"], t0=e["t0"], rcv=FC.receivers(nn, DX, ZERO, rng)) for e in case.events]
    return FC.Case(case.name, nn, DX, ZERO, None, ev)


class Pair:
    """the cell tape of a case and the node tape of the same geometry whose slowness is the oracle's A sc"""

    def __init__(self, case, dt, sc, oracle_fields=True, **kw):
        from oracle import oracle as O

        self.O, self.dt, self.nn, self.nc = O, np.dtype(dt), case.nn, _cells(case.nn)
        self.n_nodes, self.n_cells = int(np.prod(self.nn)), int(np.prod(self.nc))
        self.sc = np.asarray(sc, dtype=dt)
        self.src, self.rcv, agg, self.rows = FC.call_arrays(case, np.random.default_rng(61))
        gc_ = _grid(self.nn, dt, True, self.sc, **kw)
        tt, self.cell = gc_.raytrace_adjoint(self.src, self.rcv, aggregate_src=agg, wrt="cells")
        t = self.cell
        assert (t.wrt, t.n_events, t.n_data, t.n_cols, t.n_nodes) == ("cells", len(case.events), self.rcv.shape[0], self.n_cells,
                                                                     self.n_nodes) and t.nbytes > 0
        # 1. traveltimes and fields: raytrace on the same grid, get_grid_traveltimes, the oracle
        _bits_equal(tt, gc_.raytrace(self.src, self.rcv, aggregate_src=agg))
        self.fields = []
        for e, ev in enumerate(case.events):
            one = np.column_stack([np.full(ev["pts"].shape[0], ev["t0"]), ev["pts"]])
            _bits_equal(tt[self.rows[e]], gc_.raytrace(one, self.rcv[self.rows[e]], aggregate_src=True))
            self.fields.append(t.field(e))
            _bits_equal(self.fields[e], gc_.get_grid_traveltimes().flatten("F"))
            if oracle_fields:
                o = O.solve3d(dt, self.nc, DX, ZERO, self.sc, ev["pts"], t0=np.full(ev["pts"].shape[0], ev["t0"]),
                              rcv=self.rcv[self.rows[e]], cell_slowness=True)
                _bits_equal(self.fields[e], o["tt"])
                _bits_equal(tt[self.rows[e]], o["tt_rcv"])
        # 2. the node grid of the same geometry
        self.sn = O.cells_to_nodes3d(dt, self.nc, self.sc)
        gn = _grid(self.nn, dt, False, self.sn, **kw)
        tt_n, self.node = gn.raytrace_adjoint(self.src, self.rcv, aggregate_src=agg)
        assert (self.node.wrt, self.node.n_cols, self.node.n_nodes) == ("nodes", self.n_nodes, self.n_nodes)
        _bits_equal(tt_n, tt)
        for e in range(len(case.events)):
            _bits_equal(self.node.field(e), self.fields[e])
        self.grid = gc_
        rng = np.random.default_rng(67)
        self.w = FC.wide_weights(rng, self.rcv.shape[0], dt)
        self.fc = rng.standard_normal((len(case.events), self.n_nodes)).astype(dt)
        self.ds = (self.sc * rng.standard_normal(self.n_cells)).astype(dt)
        self.rw = rng.uniform(0.5, 2.0, self.rcv.shape[0]).astype(dt)

    def A(self, v):
        return self.O.cells_to_nodes3d(self.dt, self.nc, np.asarray(v, dtype=self.dt))

    def At(self, g):
        assert g.dtype == self.dt and g.shape == (self.n_nodes,)
        return CR.nodes_to_cells(self.dt, self.nc, g)

    def check_products(self):
        c, n, dt = self.cell, self.node, self.dt
        out = {}
        for schedule in SCHEDULES:
            for kind, (ww, ff) in {"receivers": (self.w, None), "field": (None, self.fc), "both": (self.w, self.fc)}.items():
                g = c.vjp(ww, ff, schedule=schedule)
                assert g.shape == (self.n_cells,) and g.dtype == dt and c.passes >= 1
                _bits_equal(g, self.At(n.vjp(ww, ff, schedule=schedule)))
                out[kind] = g
            dtt, mu = c.jvp(self.ds, return_fields=True, schedule=schedule)
            assert mu.shape == (c.n_events, self.n_nodes) and c.passes >= 1
            ref_dtt, ref_mu = n.jvp(self.A(self.ds), return_fields=True, schedule=schedule)
            _bits_equal(dtt, ref_dtt)
            _bits_equal(mu, ref_mu)
            _bits_equal(c.jvp(self.ds, schedule=schedule), ref_dtt)
            gn = c.gauss_newton(self.ds, self.rw, schedule=schedule)
            assert isinstance(c.passes, tuple) and len(c.passes) == 2 and gn.shape == (self.n_cells,)
            assert (self.rw * ref_dtt).dtype == dt
            _bits_equal(gn, self.At(n.vjp(self.rw * ref_dtt, schedule=schedule)))
            _bits_equal(c.gauss_newton(self.ds, schedule=schedule), self.At(n.vjp(ref_dtt, schedule=schedule)))
            # the source-point derivatives do not involve the model vector
            g, gsrc = c.vjp(self.w, self.fc, schedule=schedule, return_source_grad=True)
            gn_, gsrc_n = n.vjp(self.w, self.fc, schedule=schedule, return_source_grad=True)
            _bits_equal(g, out["both"])
            _bits_equal(gsrc, gsrc_n)
            dsrc = np.random.default_rng(73).standard_normal((3, c.n_points, 4)).astype(dt)
            for d in (dsrc[0], dsrc):
                a, b = (t.jvp_source(d, return_fields=True, schedule=schedule) for t in (c, n))
                _bits_equal(a[0], b[0])
                _bits_equal(a[1], b[1])
            if c.n_points == c.n_events:
                _bits_equal(c.source_jacobian(schedule=schedule), n.source_jacobian(schedule=schedule))
        assert all(np.all(np.isfinite(g)) and np.any(g != 0) for g in out.values()) and np.any(ref_dtt != 0)
        return out

    def check_dot(self, label):
        """3. <w, J_cells v> against <J_cells^T w, v> with the moduli of the inputs: every term of the four sums is positive, the figure
        measures the rounding of J and J^T (FC.dot_errors, as tests/test_field_tape_edges_gpu.py takes it)"""
        c = self.cell
        wp, fcp, dsp = np.abs(self.w), np.abs(self.fc), np.abs(self.ds)
        dtt_p, mu_p = c.jvp(dsp, return_fields=True)
        e_rcv, e_fld = FC.dot_errors(wp, dtt_p, c.vjp(wp), fcp, mu_p, c.vjp(None, fcp), dsp)
        print("%s, %s, %s cells: device <w, J v> against <J^T w, v>: receivers %.2e, field %.2e (bound %.0e)"
              % (label, self.dt.name, "x".join(map(str, self.nc)), e_rcv, e_fld, DOT_TOL[self.dt]))
        assert e_rcv <= DOT_TOL[self.dt] and e_fld <= DOT_TOL[self.dt], (e_rcv, e_fld)


# ---- 1. to 4.: shapes (the last one: cells across workgroups)
@DTYPES
@pytest.mark.parametrize("nn", SHAPES, ids=lambda nn: "x".join(str(n - 1) for n in nn))
def test_cell_tape_on_the_shapes(nn, dt):
    p = Pair(shape_events(nn), dt, cell_model(nn, "rough"))
    if nn == SHAPES[-1]:
        assert p.n_cells % 256 != 0 and p.n_cells > 4 * 256
    p.check_products()
    p.check_dot("shape")


# ---- 5. other models: homogeneous and two layers with an on-node source (fields with exact ties), wide-range cotangents throughout
MODELS = {"homogeneous": [[10, 8, 12]], "two_layers": [[10, 8, 4]]}


@DTYPES
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_cell_tape_on_models_with_ties(kind, dt):
    nn = FC.NN
    rng = np.random.default_rng(41)
    rcv = np.vstack([FC.receivers(nn, DX, ZERO, rng), FC.at(nn, DX, ZERO, FC.PLANE_RCV)])
    case = FC.Case(kind, nn, DX, ZERO, None, [dict(pts=FC.at(nn, DX, ZERO, MODELS[kind]), t0=0.0, rcv=rcv)])
    p = Pair(case, dt, cell_model(nn, kind))
    decisive, total = FC.count_ties(p.fields[0], nn)
    print("%s, %s: %d equal lower / upper neighbour pairs on the device field" % (kind, np.dtype(dt).name, total))
    assert total > 0   # (without ties the case has lost its point)
    assert np.ptp(np.log2(np.abs(p.w[p.w != 0]))) > 12   # (the cotangents span many binades)
    p.check_products()
    p.check_dot(kind)


# ---- 7. refusals and lengths
def test_refusals_and_lengths():
    import ttcr_amd

    nn = (9, 8, 7)
    dt = np.float32
    case = shape_events(nn)
    p = Pair(case, dt, cell_model(nn, "rough"), oracle_fields=False)
    src, rcv = p.src, p.rcv
    gnode = _grid(nn, dt, False, p.sn)
    with pytest.raises(ValueError, match="cells"):
        gnode.raytrace_adjoint(src, rcv, wrt="cells")
    with pytest.raises(NotImplementedError, match="cells"):
        p.grid.raytrace_adjoint(src, rcv, wrt="nodes")
    with pytest.raises(NotImplementedError, match="cells"):
        p.grid.raytrace_adjoint(src, rcv)
    for g in (gnode, p.grid):
        with pytest.raises(ValueError, match="wrt"):
            g.raytrace_adjoint(src, rcv, wrt="faces")
    # the C entry itself on a node grid: a value error that names the other entry
    import ctypes as C
    from ttcr_amd import _lib
    from ttcr_amd.rgrid import _ptr

    vTx, vt0, vRx, iRx = gnode._split_sources(src, rcv, False)
    tx_off, tx, t0, rx_off, rx, out = gnode._event_arrays(vTx, vt0, vRx)
    h = C.c_void_p()
    st = gnode._lib.ttcr_fsm_raytrace_multi_adjoint_cells(gnode._h, len(vTx), _ptr(tx_off), _ptr(tx), _ptr(t0), _ptr(rx_off), _ptr(rx),
                                                          _ptr(out), C.byref(h))
    assert st == _lib.ERR_VALUE and "ttcr_fsm_raytrace_multi_adjoint" in _lib.last_error() and not h.value
    st = p.grid._lib.ttcr_fsm_raytrace_multi_adjoint(p.grid._h, len(vTx), _ptr(tx_off), _ptr(tx), _ptr(t0), _ptr(rx_off), _ptr(rx),
                                                     _ptr(out), C.byref(h))
    assert st == _lib.ERR_UNSUPPORTED and "cells" in _lib.last_error() and not h.value
    # lengths: the model vector has n_cells values, rows n_data, fields n_nodes
    c = p.cell
    for bad in (np.ones(p.n_nodes, dtype=dt), np.ones(p.n_cells + 1, dtype=dt), np.ones(3, dtype=dt)):
        with pytest.raises(ValueError, match="per cell"):
            c.jvp(bad)
        with pytest.raises(ValueError, match="per cell"):
            c.gauss_newton(bad)
    with pytest.raises(ValueError):
        c.vjp(np.ones(3, dtype=dt))
    with pytest.raises(ValueError):
        c.gauss_newton(p.ds, np.ones(3, dtype=dt))
    with pytest.raises(ValueError, match="field_cotangent"):
        c.vjp(None, np.ones((c.n_events, p.n_cells), dtype=dt))
    with pytest.raises(ValueError, match="field_cotangent"):
        c.vjp(p.w, np.ones((c.n_events, p.n_cells), dtype=dt))
    assert c.vjp(None, np.ones((c.n_events, p.n_nodes), dtype=dt)).shape == (p.n_cells,)
    # 2-D and WENO grids refuse as before
    x = np.arange(9) * 1.0
    g2 = ttcr_amd.Grid2d(x, x, cell_slowness=1, method="FSM", dtype=np.float32)
    with pytest.raises(NotImplementedError, match="3-D"):
        g2.raytrace_adjoint(np.array([[3.1, 3.3]]), np.array([[1.0, 1.0], [6.5, 5.0]]), wrt="cells")
    gw = _grid(nn, dt, True, p.sc, weno=1)
    with pytest.raises(NotImplementedError, match="weno"):
        gw.raytrace_adjoint(src, rcv, wrt="cells")


# ---- 8. lifetime and several devices
def test_cell_tape_outlives_the_grid():
    nn = (13, 11, 12)
    dt = np.float64
    p = Pair(shape_events(nn), dt, cell_model(nn, "rough"), oracle_fields=False)
    c = p.cell
    g0, d0, n0, f0 = c.vjp(p.w, p.fc), c.jvp(p.ds), c.gauss_newton(p.ds, p.rw), c.field(1)
    p.grid.set_slowness((1.3 * p.sc).reshape(p.nc, order="F"))
    _, other = p.grid.raytrace_adjoint(p.src, p.rcv, wrt="cells")
    p.grid.raytrace(p.src, p.rcv)
    assert not np.array_equal(other.vjp(p.w, p.fc), g0)
    del p.grid
    gc.collect()
    _bits_equal(c.vjp(p.w, p.fc), g0)
    _bits_equal(c.jvp(p.ds), d0)
    _bits_equal(c.gauss_newton(p.ds, p.rw), n0)
    _bits_equal(c.field(1), f0)
    c.free()
    c.free()
    with pytest.raises(ValueError):
        c.vjp(p.w)


def _device_lists():
    from ttcr_amd import _lib

    lists = [[0, 0]]
    if _lib.load().ttcr_fsm_device_count() >= 2:   # (as tests/test_multi_device_gpu.py: distinct devices where the box has them)
        lists.append([0, 1])
    return lists


@DTYPES
def test_cell_tape_on_device_lists(dt):
    nn = (17, 21, 15)
    sc = cell_model(nn, "rough")
    # four events: the sources of two shape cases
    ev = shape_events(nn).events
    rng = np.random.default_rng(83)
    ev = ev + [dict(pts=FC.at(nn, DX, ZERO, [[3.4, 12.7, 6.1]]), t0=0.25, rcv=FC.receivers(nn, DX, ZERO, rng)),
               dict(pts=FC.at(nn, DX, ZERO, [[12, 4, 9]]), t0=0.0, rcv=FC.receivers(nn, DX, ZERO, rng))]
    case = FC.Case("lists", nn, DX, ZERO, None, ev)
    one = Pair(case, dt, sc, n_threads=4)
    ref = one.check_products()
    for devs in _device_lists():
        p = Pair(case, dt, sc, oracle_fields=False, n_threads=4, device=devs)
        assert p.grid.n_devices == 2 and p.cell.device == devs[0]
        _bits_equal(np.stack(p.fields), np.stack(one.fields))
        for schedule in SCHEDULES:
            _bits_equal(p.cell.vjp(p.w, p.fc, schedule=schedule), ref["both"])
            a, b = (t.jvp(p.ds, return_fields=True, schedule=schedule) for t in (p.cell, one.cell))
            _bits_equal(a[0], b[0])
            _bits_equal(a[1], b[1])
            _bits_equal(p.cell.gauss_newton(p.ds, p.rw, schedule=schedule), one.cell.gauss_newton(p.ds, p.rw, schedule=schedule))


# ---- 6. torch (child processes)
def _torch_setup(dt, nn, n_ev, seed, **kw):
    rng = np.random.default_rng(seed)
    nc = _cells(nn)
    v = rng.uniform(1.0, 2.0, nc).astype(dt)                                 # cell velocities, (ncx, ncy, ncz)
    g = _grid(nn, dt, True, (1.0 / v).flatten("F"), **kw)
    hi = (np.array(nn) - 1) * DX
    ev = np.column_stack([rng.uniform(0, 0.5, n_ev).round(3),
                          (np.floor(rng.uniform(2, np.array(nn) - 3, (n_ev, 3))) + rng.uniform(0.2, 0.8, (n_ev, 3))) * DX]).astype(dt)
    n_rcv = 4 * n_ev
    eor = np.concatenate([np.arange(n_ev), rng.integers(0, n_ev, n_rcv - n_ev)])[rng.permutation(n_rcv)]
    rcv = rng.uniform(0.7 * DX, hi - 0.7 * DX, (n_rcv, 3))
    return rng, g, v, ev, eor, rcv


def _torch_op(flat):
    """backward = -(cell vjp) / v^2 in velocity's layout, forward_ad = cell jvp, device tensors in give device tensors out"""
    import torch
    import torch.autograd.forward_ad as fwAD

    import ttcr_amd.autograd as ag

    dt = np.float32
    nn = (21, 23, 19)
    nc = _cells(nn)
    rng, g, v, ev, eor, rcv = _torch_setup(dt, nn, 4, 11, n_threads=2)
    src = np.column_stack([eor, ev[eor]])
    shape = (-1,) if flat else nc
    vel = torch.tensor(v.reshape(shape), device="cuda", requires_grad=True)
    c_tt = torch.from_numpy(rng.standard_normal(rcv.shape[0]).astype(dt)).cuda()
    c_f = torch.from_numpy(rng.standard_normal((4,) + nn).astype(dt)).cuda()
    tt, fields = ag.raytrace_adjoint(g, vel, src, rcv, return_fields=True, wrt="cells")
    assert tt.is_cuda and tt.dtype == torch.float32 and fields.shape == (4,) + nn
    ((c_tt * tt).sum() + (c_f * fields).sum()).backward()
    assert vel.grad.is_cuda and vel.grad.shape == vel.shape
    g.set_velocity(v)
    tt_ref, tape = g.raytrace_adjoint(src, rcv, wrt="cells")
    assert tape.wrt == "cells" and tape.n_cols == int(np.prod(nc))
    _bits_equal(tt.detach().cpu().numpy(), tt_ref)
    _bits_equal(fields.detach().cpu().numpy(), np.stack([tape.field(e).reshape(nn, order="F") for e in range(4)]))
    fc = np.ascontiguousarray(c_f.cpu().numpy().transpose(0, 3, 2, 1)).reshape(4, -1)   # (n_events, nx, ny, nz) -> node order
    gs = tape.vjp(c_tt.cpu().numpy(), fc).reshape(nc, order="F")             # cell order, x fastest -> (ncx, ncy, ncz)
    _bits_equal(vel.grad.cpu().numpy(), (-gs / (v * v)).reshape(shape))
    # forward mode
    tv = (v * rng.standard_normal(nc)).astype(dt)
    with fwAD.dual_level():
        out = ag.raytrace_adjoint(g, fwAD.make_dual(vel.detach(), torch.tensor(tv.reshape(shape), device="cuda")), src, rcv,
                                  return_fields=True, wrt="cells")
        tang = [fwAD.unpack_dual(o).tangent.detach().clone() for o in out]
    assert all(t.is_cuda for t in tang)
    ds = (-(tv / (v * v))).flatten("F")
    assert ds.dtype == dt
    ref = tape.jvp(ds, return_fields=True)
    _bits_equal(tang[0].cpu().numpy(), ref[0])
    _bits_equal(tang[1].cpu().numpy(), np.stack([m.reshape(nn, order="F") for m in ref[1]]))
    # device tensors used in place; wrong lengths on the device path
    ds_dev = torch.from_numpy(ds).cuda()
    for got, want in ((tape.jvp(ds_dev), ref[0]), (tape.gauss_newton(ds_dev), tape.gauss_newton(ds)),
                      (tape.vjp(c_tt, torch.from_numpy(fc).cuda()), tape.vjp(c_tt.cpu().numpy(), fc))):
        assert got.is_cuda
        _bits_equal(got.cpu().numpy(), want)
    for bad in (torch.ones(tape.n_nodes, device="cuda"), torch.ones(3, device="cuda")):
        for call in (tape.jvp, tape.gauss_newton):
            try:
                call(bad)
            except ValueError:
                continue
            raise AssertionError("no ValueError")
    try:
        tape.vjp(c_tt, torch.ones((4, tape.n_cols), device="cuda"))
    except ValueError:
        pass
    else:
        raise AssertionError("no ValueError")
    # forward mode and backward agree
    lhs = float((c_tt.double() * tang[0].double()).sum() + (c_f.double() * tang[1].double()).sum())
    rhs = float((vel.grad.double().reshape(-1) * torch.from_numpy(tv.reshape(-1)).cuda().double()).sum())
    err = abs(lhs - rhs) / abs(rhs)
    print("cells, forward_ad against backward, flat=%s: relative %.2e (bound %.0e)" % (flat, err, DOT_TOL[np.dtype(dt)]))
    assert err <= DOT_TOL[np.dtype(dt)], (lhs, rhs)
    # the refusals of the operator
    gnode = _grid(nn, dt, False, np.ones(int(np.prod(nn))))
    for grid, kw, exc in ((gnode, dict(wrt="cells"), ValueError), (g, dict(), NotImplementedError), (g, dict(wrt="faces"), ValueError)):
        try:
            ag.raytrace_adjoint(grid, vel, src, rcv, **kw)
        except exc:
            continue
        raise AssertionError("no %s" % exc.__name__)


def _torch_events():
    """raytrace_events(..., wrt='cells') is differentiable in velocity and events, both modes"""
    import torch
    import torch.autograd.forward_ad as fwAD

    import ttcr_amd.autograd as ag

    dt = np.float32
    nn = (13, 15, 11)
    nc = _cells(nn)
    rng, g, v, ev, eor, rcv = _torch_setup(dt, nn, 3, 13, n_threads=2)
    vel = torch.tensor(v, device="cuda", requires_grad=True)
    evt = torch.tensor(ev, device="cuda", requires_grad=True)
    tt, fields = ag.raytrace_events(g, vel, evt, eor, rcv, return_fields=True, wrt="cells")
    assert tt.is_cuda and fields.shape == (3,) + nn
    c_tt = rng.standard_normal(rcv.shape[0]).astype(dt)
    c_f = rng.standard_normal((3,) + nn).astype(dt)
    ((torch.from_numpy(c_tt).cuda() * tt).sum() + (torch.from_numpy(c_f).cuda() * fields).sum()).backward()
    g.set_velocity(v)
    tt_ref, tape = g.raytrace_adjoint(np.column_stack([eor, ev[eor]]), rcv, wrt="cells")
    _bits_equal(tt.detach().cpu().numpy(), tt_ref)
    fc = np.ascontiguousarray(c_f.transpose(0, 3, 2, 1)).reshape(3, -1)
    grad, gsrc = tape.vjp(c_tt, fc, return_source_grad=True)
    assert grad.shape == (int(np.prod(nc)),)
    _bits_equal(evt.grad.cpu().numpy(), gsrc)
    _bits_equal(vel.grad.cpu().numpy(), -grad.reshape(nc, order="F") / (v * v))
    gd = tape.vjp(torch.from_numpy(c_tt).cuda(), torch.from_numpy(fc).cuda(), return_source_grad=True)
    assert gd[0].is_cuda and gd[1].is_cuda
    _bits_equal(gd[0].cpu().numpy(), grad)
    _bits_equal(gd[1].cpu().numpy(), gsrc)
    tv = (v * rng.standard_normal(nc)).astype(dt)
    te = rng.standard_normal((3, 4)).astype(dt)
    with fwAD.dual_level():
        out = ag.raytrace_events(g, fwAD.make_dual(vel.detach(), torch.from_numpy(tv).cuda()),
                                 fwAD.make_dual(evt.detach(), torch.from_numpy(te).cuda()), eor, rcv, return_fields=True, wrt="cells")
        tang = [fwAD.unpack_dual(o).tangent.detach().clone() for o in out]
    ds = (-(tv / (v * v))).flatten("F")
    a, b = tape.jvp(ds, return_fields=True), tape.jvp_source(te, return_fields=True)
    _bits_equal(tang[0].cpu().numpy(), a[0] + b[0])
    _bits_equal(tang[1].cpu().numpy(), np.stack([m.reshape(nn, order="F") for m in a[1] + b[1]]))
    lhs = float(c_tt.astype(np.float64) @ tang[0].cpu().numpy().astype(np.float64) +
                c_f.astype(np.float64).ravel() @ tang[1].cpu().numpy().astype(np.float64).ravel())
    rhs = float(vel.grad.cpu().numpy().astype(np.float64).ravel() @ tv.astype(np.float64).ravel() +
                gsrc.astype(np.float64).ravel() @ te.astype(np.float64).ravel())
    err = abs(lhs - rhs) / abs(rhs)
    print("cells, raytrace_events, forward against backward: %.2e (bound %.0e)" % (err, DOT_TOL[np.dtype(dt)]))
    assert err <= DOT_TOL[np.dtype(dt)], (lhs, rhs)


@pytest.mark.parametrize("flat", [False, True], ids=["3-D", "flat C order"])
def test_torch_op_with_cells(flat):
    _in_child("op", flat)


def test_torch_raytrace_events_with_cells():
    _in_child("events")
