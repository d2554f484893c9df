"""The forward mode of the field tape on the device (FieldTape.jvp, FieldTape.gauss_newton, torch.autograd.forward_ad through
ttcr_amd.autograd.raytrace_adjoint): jvp is bit-equal to the numpy restatement of the definition (tests/tangent_reference.py) run on the
device's own fields, whatever the schedule (tiled or global Jacobi), n_threads, the device list or the number of runs; gauss_newton has the
bits of vjp(row_weight * jvp(v)); the fp64 values are the directional derivative of what the oracle computes (central finite differences,
1e-6 relative); jvp and vjp are transposes of each other to rounding."""
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
import tangent_reference as TR  # noqa: E402

MN = (0.0, 0.0, 0.0)
TOL = 1e-6    # finite differences (the project's bound; the CPU prototype measured <= 3.2e-9 for step 1e-6)
STEP = 1e-6
DOT_TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 5e-5}   # set by the issue (measured on the CPU: 2.4e-14 and 4.8e-6)


def _in_child(fn, *args):
    """Run _torch_<fn>(*args) of this module in a fresh process that initialises torch's device before the first grid (torch ships a
    HIP runtime of its own; a process whose first device user was the library finds no device through torch afterwards)."""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_tangent_gpu as t; t._torch_%s(*%r)"
            % (HERE, ROOT, fn, args))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout[-2000:])


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


def _reference(tape, dt, nn, dx, s, ev_src, ev_rows, rcv, ds):
    """the restatement on the fields the device holds: (dtt in rcv order, (n_events, n_cols) field tangents)"""
    fields = [tape.field(e) for e in range(tape.n_events)]
    assert all(f.dtype == dt and f.size == int(np.prod(nn)) for f in fields)
    mus, dtts = TR.tangent(fields, np.asarray(s, dtype=dt), dx, nn, MN, ev_src, np.asarray(ds, dtype=dt), rcvs=[rcv[r] for r in ev_rows])
    dtt = np.zeros(rcv.shape[0], dtype=dt)
    for r, d in zip(ev_rows, dtts):
        dtt[r] = d
    return dtt, np.stack(mus)


def _check_jvp(tape, ref):
    """restatement == tiled == Jacobi == a second run, to the bit, receivers and fields; dtt alone is the same dtt"""
    ds, ref_dtt, ref_mu = ref
    assert np.all(np.isfinite(ref_mu)) and np.any(ref_mu != 0) and np.any(ref_dtt != 0)
    for schedule in ("tiled", "jacobi", "tiled"):
        dtt, mu = tape.jvp(ds, return_fields=True, schedule=schedule)
        assert tape.passes >= 1
        assert mu.shape == (tape.n_events, tape.n_cols)
        _bits_equal(dtt, ref_dtt)
        _bits_equal(mu, ref_mu)
        _bits_equal(tape.jvp(ds, schedule=schedule), ref_dtt)
    return dtt, mu


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
def test_jvp_bits_one_event(source, kind, dt):
    rng = np.random.default_rng(17)
    s = _model(NN, DX, kind)
    src = np.array(SOURCES[source])
    rcv = _receivers(rng)
    ds = (s * rng.standard_normal(s.size)).astype(dt)
    g = _grid(NN, DX, dt, s)
    tt, tape = g.raytrace_adjoint(src, rcv, aggregate_src=True)
    assert (tape.n_events, tape.n_data, tape.n_cols) == (1, rcv.shape[0], int(np.prod(NN)))
    ref = _reference(tape, dt, NN, DX, s, [src], [np.arange(rcv.shape[0])], rcv, ds)
    _check_jvp(tape, (ds,) + ref)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_jvp_bits_four_events_threads_and_device_lists(dt):
    rng = np.random.default_rng(23)
    nn, dx = (33, 29, 31), 0.5
    s = _model(nn, dx, "rough")
    src, rcv, ev_src, ev_rows = _events(4, nn, dx, rng)
    ds = (s * np.random.default_rng(99).standard_normal(s.size)).astype(dt)
    ref = None
    fields0 = None
    for kw in (dict(n_threads=1), dict(n_threads=4), dict(n_threads=4, device=[0]), dict(n_threads=4, device=[0, 0])):
        g = _grid(nn, dx, dt, s, **kw)
        tt, tape = g.raytrace_adjoint(src, rcv)
        assert tape.n_events == 4 and tape.device == 0
        fields = np.stack([tape.field(e) for e in range(4)])
        if ref is None:   # (the restatement is run once: every configuration holds the same fields, to the bit)
            fields0 = fields
            ref = _reference(tape, dt, nn, dx, s, ev_src, ev_rows, rcv, ds)
        _bits_equal(fields, fields0)
        _check_jvp(tape, (ds,) + ref)
    assert _grid(nn, dx, dt, s, n_threads=4, device=[0, 0]).n_devices == 2


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_gauss_newton_is_vjp_of_weighted_jvp(dt):
    rng = np.random.default_rng(31)
    nn, dx = (33, 29, 31), 0.5
    s = _model(nn, dx, "rough")
    src, rcv, ev_src, ev_rows = _events(4, nn, dx, rng)
    g = _grid(nn, dx, dt, s, n_threads=4)
    tt, tape = g.raytrace_adjoint(src, rcv)
    v = (s * rng.standard_normal(s.size)).astype(dt)
    rw = rng.uniform(0.5, 2.0, rcv.shape[0]).astype(dt)
    dtt = tape.jvp(v)
    assert dtt.dtype == dt
    for schedule in ("tiled", "jacobi"):
        gn = tape.gauss_newton(v, schedule=schedule)
        assert isinstance(tape.passes, tuple) and len(tape.passes) == 2 and min(tape.passes) >= 1
        _bits_equal(gn, tape.vjp(dtt))
        gw = tape.gauss_newton(v, rw, schedule=schedule)
        _bits_equal(gw, tape.vjp(rw * dtt))          # (the product in the grid dtype)
        assert (rw * dtt).dtype == dt
    f8 = lambda a: np.asarray(a, dtype=np.float64)   # noqa: E731
    lhs, rhs = f8(v) @ f8(gn), f8(dtt) @ f8(dtt)
    err = abs(lhs - rhs) / rhs
    print("<v, gauss_newton(v)> against |jvp(v)|^2, %s: %.2e (bound %.0e)" % (np.dtype(dt).name, err, DOT_TOL[np.dtype(dt)]))
    assert rhs > 0 and err <= DOT_TOL[np.dtype(dt)], (lhs, rhs, err)


# ---- against the oracle's finite differences (fp64, 21^3, eps 1e-15), fp32 against fp64, the dot-product identity
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


def _fd_setup(case):
    src, kind = FD_CASES[case]
    src = np.array(src)
    nn = (N, N, N)
    s = _model(nn, DX, kind)
    rng = np.random.default_rng(5)
    rcv = rng.uniform(0.6, (N - 1) * DX - 0.6, (30, 3))
    w = rng.standard_normal(30)
    gf = rng.standard_normal(N ** 3)
    ds = s * rng.standard_normal(s.size)
    return src, nn, s, rcv, w, gf, ds


@pytest.mark.parametrize("case", sorted(FD_CASES))
def test_fp64_jvp_against_oracle_finite_differences(case):
    src, nn, s, rcv, w, gf, ds = _fd_setup(case)
    g = _grid(nn, DX, np.float64, s, eps=1e-15, maxit=200)
    tt, tape = g.raytrace_adjoint(src, rcv, aggregate_src=True)
    o = _oracle(np.float64, s, src, rcv)
    _bits_equal(tape.field(0), o["tt"])
    op, om = _oracle(np.float64, s + STEP * ds, src, rcv), _oracle(np.float64, s - STEP * ds, src, rcv)
    fd_fld = (op["tt"] - om["tt"]) / (2 * STEP)
    fd_rcv = (op["tt_rcv"] - om["tt_rcv"]) / (2 * STEP)
    dtt, mu = tape.jvp(ds, return_fields=True)
    e_fld = np.linalg.norm(mu[0] - fd_fld) / np.linalg.norm(fd_fld)
    e_rcv = np.linalg.norm(dtt - fd_rcv) / np.linalg.norm(fd_rcv)
    print("device tangent vs oracle finite differences, %s: field %.2e, receivers %.2e (bound %.0e)" % (case, e_fld, e_rcv, TOL))
    assert e_fld <= TOL and e_rcv <= TOL, (e_fld, e_rcv)


@pytest.mark.parametrize("case", sorted(FD_CASES))
def test_fp32_jvp_against_fp64(case):
    """relative L2 difference of the fp32 and the fp64 dtt; bound: 10 x what the two CPU restatements (fp32 on the fp32 oracle field,
    fp64 on the fp64 one) give for this very case -- computed here, not taken from the device"""
    src, nn, s, rcv, w, gf, ds = _fd_setup(case)
    ref = {}
    dev = {}
    for dt in (np.float32, np.float64):
        from oracle import oracle as O

        o = O.solve3d(dt, (N - 1,) * 3, DX, MN, s.astype(dt), src.astype(dt), rcv=rcv.astype(dt), eps=1e-15, maxit=200)
        ref[dt] = TR.tangent([o["tt"]], s.astype(dt), DX, nn, MN, [src], ds.astype(dt), rcvs=[rcv])[1][0].astype(np.float64)
        g = _grid(nn, DX, dt, s, eps=1e-15, maxit=200)
        dev[dt] = g.raytrace_adjoint(src, rcv, aggregate_src=True)[1].jvp(ds.astype(dt)).astype(np.float64)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))   # noqa: E731
    bound = 10 * rel(ref[np.float32], ref[np.float64])
    got = rel(dev[np.float32], dev[np.float64])
    print("fp32 vs fp64 jvp, %s: device %.2e, restatements %.2e (bound %.2e)" % (case, got, bound / 10, bound))
    assert 0 < bound < 1e-3 and got <= bound, (got, bound)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", sorted(FD_CASES))
def test_dot_product_identity_on_the_device(case, dt):
    src, nn, s, rcv, w, gf, ds = _fd_setup(case)
    w, gf, ds = w.astype(dt), gf.astype(dt), ds.astype(dt)
    g = _grid(nn, DX, dt, s, eps=1e-15, maxit=200)
    tt, tape = g.raytrace_adjoint(src, rcv, aggregate_src=True)
    dtt, mu = tape.jvp(ds, return_fields=True)
    f8 = lambda a: np.asarray(a, dtype=np.float64)   # noqa: E731
    lhs_r, rhs_r = f8(w) @ f8(dtt), f8(tape.vjp(w)) @ f8(ds)
    lhs_f, rhs_f = f8(gf) @ f8(mu[0]), f8(tape.vjp(None, gf[None, :])) @ f8(ds)
    e_rcv = abs(lhs_r - rhs_r) / abs(rhs_r)
    e_fld = abs(lhs_f - rhs_f) / abs(rhs_f)
    bound = DOT_TOL[np.dtype(dt)]
    print("device <w, J v> against <J^T w, v>, %s, %s: receivers %.2e, field %.2e (bound %.0e)"
          % (case, np.dtype(dt).name, e_rcv, e_fld, bound))
    assert e_rcv <= bound and e_fld <= bound, (e_rcv, e_fld)


def test_memory_lifetime_and_refusals_of_the_tape():
    rng = np.random.default_rng(3)
    dt = np.float64
    s = _model(NN, DX, "rough")
    src = np.array(SOURCES["multi_point"])
    rcv = _receivers(rng)
    ds = s * rng.standard_normal(s.size)
    rw = rng.uniform(0.5, 2.0, rcv.shape[0])
    g = _grid(NN, DX, dt, s, n_threads=2)
    tt, ta = g.raytrace_adjoint(src, rcv, aggregate_src=True)
    before = ta.nbytes
    da = ta.jvp(ds)
    # what the first jvp allocates (include/ttcr_amd.h): 4 (n_rows + 1) + n_entries (8 + elem) + n_rows elem + 4 n_events n_tiles,
    # tiles of 8^3 nodes in fp64
    n_entries = sum(len(AR.stencil(dt, NN, DX, MN, p)[0]) for p in rcv)
    n_rows = rcv.shape[0]
    n_tiles = int(np.prod([-(-n // 8) for n in NN]))
    assert ta.nbytes >= before
    assert ta.nbytes - before in (0, 4 * (n_rows + 1) + n_entries * (8 + 8) + n_rows * 8 + 4 * n_tiles), (before, ta.nbytes, n_entries)
    after = ta.nbytes
    ga = ta.gauss_newton(ds, rw)
    assert ta.nbytes == after
    g.set_slowness((s * 1.3).reshape(NN, order="F"))
    _, tc = g.raytrace_adjoint(src, rcv, aggregate_src=True)
    assert not np.array_equal(tc.jvp(ds), da)
    del g
    gc.collect()
    _bits_equal(ta.jvp(ds), da)
    _bits_equal(ta.gauss_newton(ds, rw), ga)
    with pytest.raises(ValueError):
        ta.jvp(np.ones(3))                       # wrong length
    with pytest.raises(ValueError):
        ta.gauss_newton(np.ones(3))
    with pytest.raises(ValueError):
        ta.gauss_newton(ds, np.ones(3))
    with pytest.raises(ValueError):
        ta.jvp(ds, schedule="fastest")
    with pytest.raises(ValueError):
        ta.gauss_newton(ds, schedule="fastest")
    ta.free()
    ta.free()
    with pytest.raises(ValueError):
        ta.jvp(ds)
    with pytest.raises(ValueError):
        ta.gauss_newton(ds)


def test_refusals_of_the_grids():
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


# ---- torch.autograd.forward_ad through the operator (child processes)
def _torch_forward_ad(flat, return_fields):
    import torch
    import torch.autograd.forward_ad as fwAD

    import ttcr_amd.autograd as ag

    rng = np.random.default_rng(11)
    dt = np.float32
    nn, dx = (21, 23, 19), 0.5
    v = rng.uniform(1.0, 2.0, nn).astype(dt)
    tv = (v * rng.standard_normal(nn)).astype(dt)
    src, rcv, ev_src, ev_rows = _events(4, nn, dx, rng)
    g = _grid(nn, dx, dt, 1.0 / v.flatten("F"), n_threads=2)
    shape = (-1,) if flat else nn
    vel = torch.tensor(v.reshape(shape), device="cuda")
    tan = torch.tensor(tv.reshape(shape), device="cuda")
    with fwAD.dual_level():
        out = ag.raytrace_adjoint(g, fwAD.make_dual(vel, tan), src, rcv, return_fields=return_fields)
        outs = out if return_fields else (out,)
        pairs = [fwAD.unpack_dual(o) for o in outs]
        prim = [p.primal.detach().clone() for p in pairs]
        tang = [p.tangent.detach().clone() for p in pairs]
    assert all(t.is_cuda and t.dtype == torch.float32 for t in tang)
    g.set_velocity(v)
    tt_ref, tape = g.raytrace_adjoint(src, rcv)
    _bits_equal(prim[0].cpu().numpy(), tt_ref)
    ds = (-(tv / (v * v))).flatten("F")                                     # (nx, ny, nz) -> node order, x fastest
    assert ds.dtype == dt
    ref = tape.jvp(ds, return_fields=True)
    _bits_equal(tang[0].cpu().numpy(), ref[0])
    if return_fields:
        assert tang[1].shape == (4,) + nn
        _bits_equal(tang[1].cpu().numpy(), np.stack([m.reshape(nn, order="F") for m in ref[1]]))
    # device tensors in give device tensors out
    d_dev = tape.jvp(torch.from_numpy(ds).cuda())
    assert d_dev.is_cuda
    _bits_equal(d_dev.cpu().numpy(), ref[0])
    gn_dev = tape.gauss_newton(torch.from_numpy(ds).cuda())
    assert gn_dev.is_cuda
    _bits_equal(gn_dev.cpu().numpy(), tape.gauss_newton(ds))
    # forward mode and backward agree on <g, J tv> for a random cotangent
    cots = [torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(dt)).cuda() for t in tang]
    vel_r = vel.clone().requires_grad_(True)
    out = ag.raytrace_adjoint(g, vel_r, src, rcv, return_fields=return_fields)
    outs = out if return_fields else (out,)
    sum((c * o).sum() for c, o in zip(cots, outs)).backward()
    lhs = sum(float((c.double() * t.double()).sum()) for c, t in zip(cots, tang))
    rhs = float((vel_r.grad.double() * tan.double()).sum())
    err = abs(lhs - rhs) / abs(rhs)
    print("forward_ad against backward, flat=%s, return_fields=%s: %.12e, %.12e, relative %.2e (bound %.0e)"
          % (flat, return_fields, lhs, rhs, err, DOT_TOL[np.dtype(dt)]))
    assert err <= DOT_TOL[np.dtype(dt)], (lhs, rhs, err)


@pytest.mark.parametrize("return_fields", [False, True], ids=["tt", "tt and fields"])
@pytest.mark.parametrize("flat", [False, True], ids=["3-D", "flat C order"])
def test_torch_forward_ad_is_jvp_of_minus_tv_over_v_squared(flat, return_fields):
    _in_child("forward_ad", flat, return_fields)
