"""The adjoint-state gradient on the device (Grid3d.raytrace_adjoint, FieldTape, ttcr_amd.autograd.raytrace_adjoint): FieldTape.vjp
is bit-equal to the numpy restatement of the definition (tests/adjoint_reference.py) run on the device's own fields, whatever the
schedule (tiled or global Jacobi), n_threads, the device list or the number of runs; its fp64 values are the derivative of what the
oracle computes (central finite differences, 1e-6 relative); the torch operator's backward is -(vjp) / velocity**2 in velocity's layout."""
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
import adjoint_reference as AR  # noqa: E402

MN = (0.0, 0.0, 0.0)
TOL = 1e-6    # finite differences against the adjoint (set by the issue; the CPU prototype measured <= 1.8e-8 for step 1e-6)
STEP = 1e-6


def _in_child(fn, *args):
    """Run _torch_<fn>(*args) of this module in a fresh process that initialises torch's device before the first grid (torch ships a
    HIP runtime of its own; a process whose first device user was the library finds no device through torch afterwards)."""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_adjoint_gpu as t; t._torch_%s(*%r)"
            % (HERE, ROOT, fn, args))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))


def _model(nn, dx, kind):
    """node slowness, flat, x fastest"""
    ax = [np.arange(n) * dx for n in nn]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    s = 0.5 + 0.02 * X + 0.015 * Y + 0.03 * Z + 0.05 * np.sin(0.9 * X) * np.cos(0.7 * Y + 0.3 * Z)
    if kind == "rough":
        s = s * (1.0 + 0.15 * np.random.default_rng(11).uniform(-1, 1, s.shape))
    return s.flatten("F")


def _grid(nn, dx, dt, s, **kw):
    import ttcr_amd

    axes = [np.arange(n) * dx for n in nn]
    kw.setdefault("weno", 0)
    kw.setdefault("tt_from_rp", 0)
    g = ttcr_amd.Grid3d(*axes, cell_slowness=0, method="FSM", dtype=dt, **kw)
    g.set_slowness(s.reshape(nn, order="F"))
    return g


def _events(n_ev, nn, dx, rng, n_rcv=(3, 8)):
    """5-column rows (event id, t0, x, y, z) with the events' receiver rows interleaved; tape rows = events ascending, rcv order within"""
    hi = (np.array(nn) - 1) * dx
    ev_src = rng.uniform(1.5 * dx, hi - 1.5 * dx, (n_ev, 3))
    ev_t0 = rng.uniform(0, 0.5, n_ev).round(3)
    ids = np.concatenate([np.full(int(k), e) for e, k in enumerate(rng.integers(n_rcv[0], n_rcv[1], n_ev))])
    ids = ids[rng.permutation(ids.size)]
    src = np.column_stack([ids, ev_t0[ids], ev_src[ids]])
    rcv = rng.uniform(0.7 * dx, hi - 0.7 * dx, (ids.size, 3))
    rows = [np.nonzero(ids == e)[0] for e in range(n_ev)]
    return src, rcv, [ev_src[e:e + 1] for e in range(n_ev)], rows


def _reference(tape, dt, nn, dx, s, ev_src, ev_rows, rcv, w, fc):
    """the restatement on the fields the device holds"""
    fields = [tape.field(e) for e in range(tape.n_events)]
    assert all(f.dtype == dt and f.size == int(np.prod(nn)) for f in fields)
    return AR.adjoint(fields, np.asarray(s, dtype=dt), dx, nn, MN, ev_src, rcvs=[rcv[r] for r in ev_rows],
                      ws=None if w is None else [w[r] for r in ev_rows], field_cot=fc)


def _check_all_cotangents(tape, dt, nn, dx, s, ev_src, ev_rows, rcv, rng):
    """receiver-only, field-only and both cotangents: restatement == tiled == Jacobi == a second run, to the bit"""
    w = rng.standard_normal(rcv.shape[0]).astype(dt)
    fc = rng.standard_normal((tape.n_events, tape.n_cols)).astype(dt)
    out = {}
    for kind, (ww, ff) in {"receivers": (w, None), "field": (None, fc), "both": (w, fc)}.items():
        ref = _reference(tape, dt, nn, dx, s, ev_src, ev_rows, rcv, ww, ff)
        assert np.all(np.isfinite(ref)) and np.any(ref != 0)
        gt = tape.vjp(ww, ff)
        assert tape.passes >= 1
        _bits_equal(gt, ref)
        gj = tape.vjp(ww, ff, schedule="jacobi")
        assert tape.passes >= 1
        _bits_equal(gj, ref)
        _bits_equal(tape.vjp(ww, ff), ref)
        out[kind] = gt
    return out


NN, DX = (21, 17, 25), 0.5   # a non-cubic grid: x 0..10, y 0..8, z 0..12; two relaxation tiles or more along every axis
SOURCES = {
    "off_node": [[3.3, 4.1, 5.7]],
    "on_node": [[4.0, 5.5, 3.0]],
    "multi_point": [[3.3, 4.1, 5.7], [3.6, 4.2, 5.4], [8.0, 2.0, 9.5]],
    "corner_cell": [[0.2, 0.3, 0.1]],
    "on_face": [[0.0, 4.1, 5.7]],
    "far_face": [[10.0, 3.3, 12.0]],
}
# receivers on a node, on a plane, on an edge, on the last planes, in the last corner
SPECIAL_RCV = [[2.0, 3.0, 4.0], [2.0, 3.3, 4.7], [2.0, 3.0, 4.7], [10.0, 3.3, 4.7], [3.3, 8.0, 12.0], [10.0, 8.0, 12.0], [0.0, 0.0, 0.0]]


def _receivers(rng, n=6):
    hi = (np.array(NN) - 1) * DX
    return np.vstack([rng.uniform(0.3, hi - 0.3, (n, 3)), np.array(SPECIAL_RCV)])


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("kind", ["smooth", "rough"])
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_vjp_bits_one_event(source, kind, dt):
    rng = np.random.default_rng(17)
    s = _model(NN, DX, kind)
    src = np.array(SOURCES[source])
    rcv = _receivers(rng)
    g = _grid(NN, DX, dt, s)
    tt, tape = g.raytrace_adjoint(src, rcv, aggregate_src=True)
    assert (tape.n_events, tape.n_data, tape.n_cols) == (1, rcv.shape[0], int(np.prod(NN))) and tape.nbytes > 0
    _bits_equal(tt, g.raytrace(src, rcv, aggregate_src=True))
    _bits_equal(tape.field(0), g.get_grid_traveltimes().flatten("F"))
    # the stencil: sum(weight * T) is the interpolated traveltime with its 8-term sum re-associated
    T = tape.field(0)
    for r in range(rcv.shape[0]):
        nodes, wts = AR.stencil(dt, NN, DX, MN, rcv[r])
        v = sum(np.float64(wt) * np.float64(T[m]) for m, wt in zip(nodes, wts))
        assert abs(v - np.float64(tt[r])) <= 16 * np.spacing(dt(tt[r])), (r, v, tt[r])
    _check_all_cotangents(tape, dt, NN, DX, s, [src], [np.arange(rcv.shape[0])], rcv, rng)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_vjp_bits_four_events_threads_and_device_lists(dt):
    rng = np.random.default_rng(23)
    nn, dx = (33, 29, 31), 0.5
    s = _model(nn, dx, "rough")
    src, rcv, ev_src, ev_rows = _events(4, nn, dx, rng)
    grads = []
    for kw in (dict(n_threads=1), dict(n_threads=4), dict(n_threads=4, device=[0]), dict(n_threads=4, device=[0, 0])):
        g = _grid(nn, dx, dt, s, **kw)
        tt, tape = g.raytrace_adjoint(src, rcv)
        _bits_equal(tt, g.raytrace(src, rcv))
        assert tape.n_events == 4 and tape.device == 0
        grads.append(_check_all_cotangents(tape, dt, nn, dx, s, ev_src, ev_rows, rcv, np.random.default_rng(99)))
    assert _grid(nn, dx, dt, s, n_threads=4, device=[0, 0]).n_devices == 2
    for other in grads[1:]:
        for kind in other:
            _bits_equal(other[kind], grads[0][kind])


def test_tt_is_the_interpolated_one_whatever_the_grid_says():
    rng = np.random.default_rng(4)
    s = _model(NN, DX, "smooth")
    src = np.array(SOURCES["off_node"])
    rcv = _receivers(rng)
    g0 = _grid(NN, DX, np.float64, s, tt_from_rp=0)
    g1 = _grid(NN, DX, np.float64, s, tt_from_rp=1)
    tt1, tape1 = g1.raytrace_adjoint(src, rcv)
    _bits_equal(tt1, g0.raytrace(src, rcv))
    w = rng.standard_normal(rcv.shape[0])
    _bits_equal(tape1.vjp(w), g0.raytrace_adjoint(src, rcv)[1].vjp(w))
    assert not np.array_equal(g1.raytrace(src, rcv), tt1)   # (the grid's own setting is back after the call)


# ---- against the oracle's finite differences (fp64, 21^3, eps 1e-15) and fp32 against fp64
N = 21
FD_CASES = {
    "off_node": ([[3.3, 4.1, 5.7]], "smooth"),
    "on_node": ([[4.0, 5.5, 3.0]], "smooth"),
    "two_points": ([[3.3, 4.1, 5.7], [3.6, 4.2, 5.4]], "smooth"),
    "rough": ([[6.2, 2.9, 4.4]], "rough"),
}


def _oracle(dt, s, src, rcv):
    from oracle import oracle as O

    o = O.solve3d(dt, (N - 1,) * 3, DX, MN, s, src, rcv=rcv, eps=1e-15, maxit=200)
    assert o["niter"] < 200 and o["change"][-1] == 0
    return o


@pytest.mark.parametrize("case", sorted(FD_CASES))
def test_fp64_gradient_against_oracle_finite_differences(case):
    src, kind = FD_CASES[case]
    src = np.array(src)
    nn = (N, N, N)
    s = _model(nn, DX, kind)
    rng = np.random.default_rng(5)
    rcv = rng.uniform(0.6, (N - 1) * DX - 0.6, (30, 3))
    w = rng.standard_normal(30)
    gf = rng.standard_normal(N ** 3)
    ds = s * rng.standard_normal(s.size)
    g = _grid(nn, DX, np.float64, s, eps=1e-15, maxit=200)
    tt, tape = g.raytrace_adjoint(src, rcv, aggregate_src=True)
    o = _oracle(np.float64, s, src, rcv)
    _bits_equal(tape.field(0), o["tt"])
    _bits_equal(tt, o["tt_rcv"])
    op, om = _oracle(np.float64, s + STEP * ds, src, rcv), _oracle(np.float64, s - STEP * ds, src, rcv)
    fd_rcv = (w @ op["tt_rcv"] - w @ om["tt_rcv"]) / (2 * STEP)
    fd_fld = (gf @ op["tt"] - gf @ om["tt"]) / (2 * STEP)
    e_rcv = abs(tape.vjp(w) @ ds - fd_rcv) / abs(fd_rcv)
    e_fld = abs(tape.vjp(None, gf[None, :]) @ ds - fd_fld) / abs(fd_fld)
    print("device adjoint vs oracle finite differences, %s: receivers %.2e, field %.2e (bound %.0e)" % (case, e_rcv, e_fld, TOL))
    assert e_rcv <= TOL and e_fld <= TOL, (e_rcv, e_fld)


@pytest.mark.parametrize("case", sorted(FD_CASES))
def test_fp32_gradient_against_fp64(case):
    """relative L2 difference of the fp32 and the fp64 gradient; bound: 10 x what the two CPU restatements (fp32 on the fp32 oracle field,
    fp64 on the fp64 one) give for this very case -- computed here, not taken from the device"""
    src, kind = FD_CASES[case]
    src = np.array(src)
    nn = (N, N, N)
    s = _model(nn, DX, kind)
    rng = np.random.default_rng(5)
    rcv = rng.uniform(0.6, (N - 1) * DX - 0.6, (30, 3))
    w = rng.standard_normal(30)
    ref = {}
    dev = {}
    for dt in (np.float32, np.float64):
        from oracle import oracle as O

        o = O.solve3d(dt, (N - 1,) * 3, DX, MN, s.astype(dt), src.astype(dt), rcv=rcv.astype(dt), eps=1e-15, maxit=200)
        ref[dt] = AR.adjoint([o["tt"]], s.astype(dt), DX, nn, MN, [src], rcvs=[rcv], ws=[w.astype(dt)]).astype(np.float64)
        g = _grid(nn, DX, dt, s, eps=1e-15, maxit=200)
        dev[dt] = g.raytrace_adjoint(src, rcv, aggregate_src=True)[1].vjp(w.astype(dt)).astype(np.float64)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))   # noqa: E731
    bound = 10 * rel(ref[np.float32], ref[np.float64])
    got = rel(dev[np.float32], dev[np.float64])
    print("fp32 vs fp64 gradient, %s: device %.2e, restatements %.2e (bound %.2e)" % (case, got, bound / 10, bound))
    assert 0 < bound < 1e-3 and got <= bound, (got, bound)


def test_tape_outlives_the_grid_and_refuses_when_freed():
    rng = np.random.default_rng(3)
    dt = np.float64
    s = _model(NN, DX, "rough")
    src = np.array(SOURCES["multi_point"])
    rcv = _receivers(rng)
    w = rng.standard_normal(rcv.shape[0])
    g = _grid(NN, DX, dt, s, n_threads=2)
    tt_a, ta = g.raytrace_adjoint(src, rcv, aggregate_src=True)
    ga = ta.vjp(w)
    fa = ta.field(0)
    g.set_slowness((s * 1.3).reshape(NN, order="F"))
    _, tc = g.raytrace_adjoint(src, rcv, aggregate_src=True)
    g.raytrace(src, rcv, aggregate_src=True)
    assert not np.array_equal(tc.vjp(w), ga)
    del g
    gc.collect()
    _bits_equal(ta.vjp(w), ga)
    _bits_equal(ta.field(0), fa)
    with pytest.raises(ValueError):
        ta.vjp()                                 # nothing to back-propagate
    with pytest.raises(ValueError):
        ta.vjp(np.ones(3))                       # wrong length
    with pytest.raises(ValueError):
        ta.vjp(w, schedule="fastest")
    ta.free()
    ta.free()
    with pytest.raises(ValueError):
        ta.vjp(w)
    with pytest.raises(ValueError):
        ta.field(0)


def test_refusals():
    import ttcr_amd

    x = np.arange(9) * 1.0
    src = np.array([[3.1, 3.2, 3.3]])
    rcv = np.array([[1.0, 1.0, 1.0], [6.5, 6.0, 5.0]])
    gcell = ttcr_amd.Grid3d(x, x, x, cell_slowness=1, method="FSM", tt_from_rp=0, weno=0, dtype=np.float32)
    with pytest.raises(NotImplementedError, match="cells"):
        gcell.raytrace_adjoint(src, rcv)
    gw = ttcr_amd.Grid3d(x, x, x, cell_slowness=0, method="FSM", tt_from_rp=0, weno=1, dtype=np.float32)
    gw.set_slowness(np.ones((9, 9, 9)))
    with pytest.raises(NotImplementedError, match="weno"):
        gw.raytrace_adjoint(src, rcv)
    g2 = ttcr_amd.Grid2d(x, x, cell_slowness=0, method="FSM", dtype=np.float32)
    with pytest.raises(NotImplementedError, match="3-D"):
        g2.raytrace_adjoint(np.array([[3.1, 3.3]]), np.array([[1.0, 1.0], [6.5, 5.0]]))


# ---- the torch operator (child processes)
def _torch_op(flat):
    import torch

    import ttcr_amd.autograd as ag

    rng = np.random.default_rng(11)
    dt = np.float32
    nn, dx = (21, 23, 19), 0.5
    v = rng.uniform(1.0, 2.0, nn).astype(dt)
    src, rcv, ev_src, ev_rows = _events(4, nn, dx, rng)
    g = _grid(nn, dx, dt, 1.0 / v.flatten("F"), n_threads=2)
    vel = torch.tensor(v.reshape(-1) if flat else v, device="cuda", requires_grad=True)
    d = torch.from_numpy(rng.uniform(0.5, 4.0, rcv.shape[0]).astype(dt)).cuda()
    tt = ag.raytrace_adjoint(g, vel, src, rcv)
    assert tt.is_cuda and tt.dtype == torch.float32
    g.set_velocity(v)
    tt_ref, tape = g.raytrace_adjoint(src, rcv)
    _bits_equal(tt.detach().cpu().numpy(), tt_ref)
    loss = ((tt - d) ** 2).sum()
    loss.backward(retain_graph=True)
    w = (2 * (tt - d)).detach().cpu().numpy()
    gs = tape.vjp(w).reshape(nn, order="F")                                 # node order, x fastest -> (nx, ny, nz)
    ref_v = -gs / (v * v)
    ref_v = ref_v.reshape(-1) if flat else ref_v
    assert vel.grad.shape == vel.shape
    _bits_equal(vel.grad.cpu().numpy(), ref_v)
    first = vel.grad.clone()
    vel.grad = None
    loss.backward()
    _bits_equal(vel.grad.cpu().numpy(), first.cpu().numpy())


def _torch_directional(return_fields):
    """gradcheck-style: the directional derivative of a loss of the operator's outputs, by autograd and by central differences of the
    operator itself, fp64, a grid solved to its fixed point"""
    import torch

    import ttcr_amd.autograd as ag

    rng = np.random.default_rng(12)
    dt = np.float64
    nn, dx = (N, N, N), DX
    v = 1.0 / _model(nn, dx, "smooth").reshape(nn, order="F")
    src = np.array([[3.3, 4.1, 5.7]])
    rcv = rng.uniform(0.6, (N - 1) * dx - 0.6, (30, 3))
    w = torch.from_numpy(rng.standard_normal(30)).cuda()
    gf = torch.from_numpy(rng.standard_normal((1,) + nn)).cuda()
    dv = torch.from_numpy(v * rng.standard_normal(nn)).cuda()
    g = _grid(nn, dx, dt, 1.0 / v.flatten("F"), eps=1e-15, maxit=200)

    def loss_of(vel):
        if not return_fields:
            return (w * ag.raytrace_adjoint(g, vel, src, rcv)).sum()
        tt, fields = ag.raytrace_adjoint(g, vel, src, rcv, return_fields=True)
        assert fields.shape == (1,) + nn
        return (w * tt).sum() + (gf * fields).sum()

    vel = torch.tensor(v, device="cuda", requires_grad=True)
    loss_of(vel).backward()
    ad = float((vel.grad * dv).sum())
    with torch.no_grad():
        fd = float(loss_of(vel + STEP * dv) - loss_of(vel - STEP * dv)) / (2 * STEP)
    err = abs(ad - fd) / abs(fd)
    print("torch op, return_fields=%s: autograd %.12e, finite differences %.12e, relative %.2e" % (return_fields, ad, fd, err))
    assert err <= TOL, (ad, fd, err)


@pytest.mark.parametrize("flat", [False, True], ids=["3-D", "flat C order"])
def test_torch_op_backward_is_minus_vjp_over_v_squared(flat):
    _in_child("op", flat)


@pytest.mark.parametrize("return_fields", [False, True], ids=["tt", "tt and fields"])
def test_torch_op_directional_derivative(return_fields):
    _in_child("directional", return_fields)
