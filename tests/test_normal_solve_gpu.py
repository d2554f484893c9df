"""The normal equations of the field tape on the device (FieldTape.smooth, dot, solve_normal, release_solve and
inversion.gauss_newton_step).  Every comparison is to the bit, against the numpy restatements of tests/normal_reference.py;
the restated recurrence is driven by the device's own gauss_newton / newton, so that what is compared is the solver, not the product.
The grids are small: what can go wrong are tile seams, end rows and chunk boundaries."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import normal_reference as NR  # noqa: E402

DX = 0.5
DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
WRT = pytest.mark.parametrize("wrt", ["nodes", "cells"])


def _in_child(fn, *args):
    """Run _torch_<fn>(*args) of this module in a fresh process that initialises torch's device before the first grid (torch ships a
    HIP runtime of its own; a process whose first device user was the library may find no device through torch afterwards)."""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_normal_solve_gpu as t; t._torch_%s(*%r)"
            % (HERE, ROOT, fn, args))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    bad = np.nonzero(a.view(u) != b.view(u))[0]
    assert bad.size == 0, (bad.size, bad[:5], a[bad[:5]], b[bad[:5]])


def _tape(params, dt, wrt="nodes", n_events=1, n_rcv=2, seed=3):
    """a tape whose model vector has `params` parameters along x, y, z: (grid, tape, rcv)"""
    import ttcr_amd

    cell = wrt == "cells"
    nn = tuple(n + 1 for n in params) if cell else tuple(params)
    axes = [np.arange(n) * DX for n in nn]
    g = ttcr_amd.Grid3d(*axes, cell_slowness=1 if cell else 0, method="FSM", dtype=dt, weno=0, tt_from_rp=0)
    rng = np.random.default_rng(seed)
    g.set_slowness(rng.uniform(0.4, 0.7, params))
    hi = (np.array(nn) - 1.0) * DX
    pts = rng.uniform(0.2 * hi, 0.8 * hi, (n_events, 3))
    ids = np.repeat(np.arange(n_events), n_rcv)
    rcv = rng.uniform(0.05 * hi, 0.95 * hi, (ids.size, 3))
    perm = rng.permutation(ids.size)
    ids, rcv = ids[perm], rcv[perm]
    src = np.column_stack([ids, np.zeros(ids.size), pts[ids]])
    tt, tape = g.raytrace_adjoint(src, rcv, wrt=wrt)
    assert tape.n_cols == int(np.prod(params)) and tape.n_events == n_events and tape.n_data == ids.size and tape.wrt == wrt
    return g, tape, rcv


def _wide(rng, n, dt):
    """magnitudes spread over 2^-12 .. 2^12"""
    return (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 13, n)).astype(dt)


# ---- 1. smooth
def _edge(dt):
    from ttcr_amd import _lib

    lib = _lib.load()
    return lib.ttcr_fsm_normal_tile_edge(_lib.TTCR_F32 if np.dtype(dt) == np.float32 else _lib.TTCR_F64)


def _smooth_bits(axis, wrt, dt, on_device):
    """smooth against the restatement on the axis lengths of the issue; on_device: the input is a CUDA tensor, else a numpy array"""
    edge = _edge(dt)
    assert edge >= 6
    rng = np.random.default_rng(41 + axis)
    for n in (3, 4, 5, edge - 1, edge, edge + 1, 2 * edge + 1):
        params = [4, 5, 3]
        params[axis] = n
        params = tuple(params)
        g, tape, rcv = _tape(params, dt, wrt)
        assert tape.smooth_tile_edge == edge
        v = _wide(rng, tape.n_cols, dt)
        for weights in ((1.0, 1.0, 1.0), (2.0, 0.0, 0.75)):
            ref = NR.smooth(v, params, DX, weights, dtype=dt)
            assert np.all(np.isfinite(ref)) and np.any(ref != 0)
            if on_device:
                import torch

                out = tape.smooth(torch.as_tensor(v, device="cuda"), weights)
                assert out.is_cuda
                out = out.cpu().numpy()
            else:
                out = tape.smooth(v, weights)
                assert isinstance(out, np.ndarray)
            _bits_equal(out, ref)
        tape.free()


@DTYPES
@WRT
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_smooth_bits(axis, wrt, dt):
    _smooth_bits(axis, wrt, dt, False)


def _torch_smooth(dtname):
    for wrt in ("nodes", "cells"):
        for axis in (0, 1, 2):
            _smooth_bits(axis, wrt, np.dtype(dtname).type, True)


@DTYPES
def test_smooth_bits_of_device_tensors(dt):
    _in_child("smooth", np.dtype(dt).name)


@DTYPES
def test_smooth_two_tiles_on_every_axis_and_short_axes(dt):
    edge = _edge(dt)
    params = (edge + 3, 2 * edge + 1, edge + 1)
    g, tape, rcv = _tape(params, dt)
    v = _wide(np.random.default_rng(43), tape.n_cols, dt)
    _bits_equal(tape.smooth(v, (0.5, 1.5, 1.0)), NR.smooth(v, params, DX, (0.5, 1.5, 1.0), dtype=dt))
    g2, cells, _ = _tape((2, 4, 3), dt, "cells")      # 3 x 5 x 4 nodes: two cells along x
    with pytest.raises(ValueError, match="at least 3"):
        cells.smooth(np.zeros(cells.n_cols, dtype=dt))
    with pytest.raises(ValueError, match="at least 3"):
        cells.solve_normal(np.ones(cells.n_cols, dtype=dt), smooth=1.0)
    x, info = cells.solve_normal(np.ones(cells.n_cols, dtype=dt), damp=1.0, maxiter=2, return_info=True)   # (no smoothing: allowed)
    assert info["iterations"] >= 1


# ---- 2. dot
DOT_SHAPES = [(3, 11, 31), (8, 8, 16), (5, 5, 41), (64, 64, 64), (65, 37, 109)]


def _dot_bits(nn, dt, on_device):
    g, tape, rcv = _tape(nn, dt)
    assert tape.n_cols in (1023, 1024, 1025, 262144, 262145)
    rng = np.random.default_rng(tape.n_cols)
    a, b = _wide(rng, tape.n_cols, dt), _wide(rng, tape.n_cols, dt)
    for u, v in ((a, b), (a, a)):
        ref = NR.dot(u, v)
        if on_device:
            import torch

            tu, tv = torch.as_tensor(u, device="cuda"), torch.as_tensor(v, device="cuda")
            assert tape.dot(tu, tv) == ref and tape.dot(tu, v) == ref and tape.dot(tu, tu) == NR.dot(u, u)
        else:
            got = tape.dot(u, v)
            assert isinstance(got, float) and got == ref and np.isfinite(ref) and ref != 0, (got, ref)


@DTYPES
@pytest.mark.parametrize("nn", DOT_SHAPES, ids=lambda nn: str(int(np.prod(nn))))
def test_dot_bits(nn, dt):
    _dot_bits(nn, dt, False)


def _torch_dot(dtname):
    for nn in DOT_SHAPES:
        _dot_bits(nn, np.dtype(dtname).type, True)


@DTYPES
def test_dot_bits_of_device_tensors(dt):
    _in_child("dot", np.dtype(dt).name)


# ---- 3. solve_normal
SOLVE_NN = (17, 14, 19)
REG = {"both": (2e-2, 1e-1), "smooth": (2e-2, 0.0), "damp": (0.0, 1e-1), "none": (0.0, 0.0)}
WEIGHTS = (1.0, 0.5, 2.0)


def _solve_params(wrt):
    return tuple(n - 1 for n in SOLVE_NN) if wrt == "cells" else SOLVE_NN


def _reference(tape, params, dt, rhs, rw, smooth, damp, x0, maxiter, rtol=1e-6, product="gauss_newton", schedule="tiled"):
    H = getattr(tape, product)
    return NR.cg(lambda p: H(p, rw, schedule=schedule), rhs, dt, smooth_op=lambda p: NR.smooth(p, params, DX, WEIGHTS, dtype=dt),
                 smooth=smooth, damp=damp, x0=x0, maxiter=maxiter, rtol=rtol)


def _same(got, ref):
    x, info = got
    xr, inf_r = ref
    _bits_equal(x, xr)
    assert info["status"] == inf_r["status"] and info["iterations"] == inf_r["iterations"], (info, inf_r)
    assert info["rho"] == inf_r["rho"] and info["pq"] == inf_r["pq"], (info, inf_r)
    assert len(info["passes"]) == len(info["pq"]) and all(min(p) >= 1 for p in info["passes"])


@DTYPES
@WRT
@pytest.mark.parametrize("reg", sorted(REG))
def test_solve_normal_bits(reg, wrt, dt):
    params = _solve_params(wrt)
    g, tape, rcv = _tape(params, dt, wrt, n_events=2, n_rcv=20, seed=7)
    rng = np.random.default_rng(59)
    smooth, damp = REG[reg]
    rhs = rng.standard_normal(tape.n_cols).astype(dt)
    start = (0.1 * rng.standard_normal(tape.n_cols)).astype(dt)
    weight = rng.uniform(0.5, 2.0, tape.n_data).astype(dt)
    kw = dict(smooth=smooth, smooth_weights=WEIGHTS, damp=damp, return_info=True)
    for x0 in (None, start):
        for rw in (None, weight):
            for maxiter in (1, 2, 3, 4, 5):
                ref = _reference(tape, params, dt, rhs, rw, smooth, damp, x0, maxiter)
                got = tape.solve_normal(rhs, row_weight=rw, x0=x0, maxiter=maxiter, **kw)
                _same(got, ref)
                assert got[1]["status"] == 1 and got[1]["iterations"] == maxiter and (got[1]["passes_x0"] is None) == (x0 is None)
            _same(tape.solve_normal(rhs, row_weight=rw, x0=x0, maxiter=5, schedule="jacobi", **kw), ref)
            _bits_equal(tape.solve_normal(rhs, row_weight=rw, x0=x0, maxiter=5, smooth=smooth, smooth_weights=WEIGHTS, damp=damp), ref[0])


@DTYPES
def test_solve_normal_converges_and_breaks_down(dt):
    params = SOLVE_NN
    g, tape, rcv = _tape(params, dt, n_events=2, n_rcv=20, seed=7)
    rng = np.random.default_rng(61)
    rhs = rng.standard_normal(tape.n_cols).astype(dt)
    # heavy damping: the residual test is met within a few iterations
    kw = dict(smooth=1e-3, smooth_weights=WEIGHTS, damp=50.0, maxiter=30, rtol=1e-4)
    x, info = tape.solve_normal(rhs, return_info=True, **kw)
    ref = _reference(tape, params, dt, rhs, None, 1e-3, 50.0, None, 30, rtol=1e-4)
    _same((x, info), ref)
    assert info["status"] == 0 and 1 <= info["iterations"] < 30 and info["rho"][-1] <= 1e-8 * info["rho"][0]
    # row_weight = 0 and no regularisation: <p, A p> = 0, no update, x stays x0
    zero = np.zeros(tape.n_data, dtype=dt)
    x0 = rng.standard_normal(tape.n_cols).astype(dt)
    for start in (None, x0):
        x, info = tape.solve_normal(rhs, row_weight=zero, x0=start, maxiter=4, return_info=True)
        assert info["status"] == 2 and info["iterations"] == 0 and info["pq"] == [0.0] and len(info["rho"]) == 2
        _bits_equal(x, np.zeros(tape.n_cols, dtype=dt) if start is None else start)
        _same((x, info), _reference(tape, params, dt, rhs, zero, 0.0, 0.0, start, 4))


@DTYPES
def test_solve_normal_across_a_chunk_boundary(dt):
    params = (5, 5, 41)   # 1025 parameters: one full chunk and a remainder of one element
    g, tape, rcv = _tape(params, dt, n_events=2, n_rcv=6, seed=11)
    rng = np.random.default_rng(67)
    rhs = _wide(rng, tape.n_cols, dt)
    rw = rng.uniform(0.5, 2.0, tape.n_data).astype(dt)
    smooth, damp = REG["both"]
    for maxiter in (1, 4):
        got = tape.solve_normal(rhs, row_weight=rw, smooth=smooth, smooth_weights=WEIGHTS, damp=damp, maxiter=maxiter, return_info=True)
        _same(got, _reference(tape, params, dt, rhs, rw, smooth, damp, None, maxiter))


def _torch_solve(dtname):
    import torch

    dt = np.dtype(dtname).type
    params = SOLVE_NN
    g, tape, rcv = _tape(params, dt, n_events=2, n_rcv=20, seed=7)
    rng = np.random.default_rng(71)
    rhs = rng.standard_normal(tape.n_cols).astype(dt)
    x0 = (0.1 * rng.standard_normal(tape.n_cols)).astype(dt)
    rw = rng.uniform(0.5, 2.0, tape.n_data).astype(dt)
    smooth, damp = REG["both"]
    kw = dict(smooth=smooth, smooth_weights=WEIGHTS, damp=damp, maxiter=3, return_info=True)
    ref = tape.solve_normal(rhs, row_weight=rw, x0=x0, **kw)
    dev = lambda a: torch.as_tensor(a, device="cuda")   # noqa: E731
    t_rhs, t_x0 = dev(rhs), dev(x0)
    x, info = tape.solve_normal(t_rhs, row_weight=dev(rw), x0=t_x0, **kw)
    assert x.is_cuda and info == ref[1]
    _bits_equal(x.cpu().numpy(), ref[0])
    _bits_equal(t_rhs.cpu().numpy(), rhs)     # (the arguments are read, not used as work arrays)
    _bits_equal(t_x0.cpu().numpy(), x0)
    x, info = tape.solve_normal(rhs, row_weight=dev(rw), x0=x0, **kw)   # mixed: the result lives with the first tensor
    assert x.is_cuda and info == ref[1]
    _bits_equal(x.cpu().numpy(), ref[0])


@DTYPES
def test_solve_normal_with_device_tensors(dt):
    _in_child("solve", np.dtype(dt).name)


# ---- 4. the Newton product
@DTYPES
def test_solve_normal_with_the_newton_product(dt):
    params = SOLVE_NN
    g, tape, rcv = _tape(params, dt, n_events=2, n_rcv=20, seed=7)
    rng = np.random.default_rng(73)
    rhs = rng.standard_normal(tape.n_cols).astype(dt)
    rw = rng.uniform(0.5, 2.0, tape.n_data).astype(dt)
    smooth, damp = 2e-2, 5.0
    kw = dict(row_weight=rw, smooth=smooth, smooth_weights=WEIGHTS, damp=damp, maxiter=3, hessian="newton", return_info=True)
    with pytest.raises(ValueError, match="holds no cotangent"):
        tape.solve_normal(rhs, **kw)
    with pytest.raises(ValueError, match="holds no cotangent"):
        tape.newton(rhs, rw)
    tape.hold((1e-2 * rng.standard_normal(tape.n_data)).astype(dt))
    got = tape.solve_normal(rhs, **kw)
    _same(got, _reference(tape, params, dt, rhs, rw, smooth, damp, None, 3, product="newton"))
    gn = tape.solve_normal(rhs, **{**kw, "hessian": "gauss_newton"})
    assert not np.array_equal(gn[0], got[0])
    tape.release()
    with pytest.raises(ValueError, match="holds no cotangent"):
        tape.solve_normal(rhs, **kw)


# ---- 5. memory
@DTYPES
@WRT
def test_release_solve(wrt, dt):
    params = _solve_params(wrt)
    g, tape, rcv = _tape(params, dt, wrt, n_events=2, n_rcv=20, seed=7)
    rng = np.random.default_rng(79)
    rhs = rng.standard_normal(tape.n_cols).astype(dt)
    v = rng.standard_normal(tape.n_cols).astype(dt)
    tape.gauss_newton(v)                      # (what the first product allocates is not the solver's)
    before = tape.nbytes
    kw = dict(smooth=2e-2, damp=1e-1, maxiter=3, return_info=True)
    x, info = tape.solve_normal(rhs, **kw)
    elem = np.dtype(dt).itemsize
    chunks = -(-tape.n_cols // 1024)
    assert tape.nbytes == before + 5 * tape.n_cols * elem + 8 * chunks + 48
    tape.release_solve()
    assert tape.nbytes == before
    tape.release_solve()                      # (a second release is a no-op)
    assert tape.nbytes == before
    x2, info2 = tape.solve_normal(rhs, **kw)
    _bits_equal(x2, x)
    assert info2 == info
    tape.release_solve()
    d = tape.dot(v, v)                        # dot and smooth allocate the same arrays
    assert tape.nbytes == before + 5 * tape.n_cols * elem + 8 * chunks + 48 and d == NR.dot(v, v)
    tape.release_solve()
    assert tape.nbytes == before


# ---- 6. the step helper
@DTYPES
def test_gauss_newton_step(dt):
    from ttcr_amd.inversion import gauss_newton_step

    params = SOLVE_NN
    g, tape, rcv = _tape(params, dt, n_events=2, n_rcv=20, seed=7)
    rng = np.random.default_rng(83)
    residual = (1e-2 * rng.standard_normal(tape.n_data)).astype(dt)
    model = rng.uniform(0.4, 0.7, tape.n_cols).astype(dt)
    rw = rng.uniform(0.5, 2.0, tape.n_data).astype(dt)
    smooth, damp = dt(2e-2), dt(1e-1)
    for weight in (None, rw):
        b = tape.vjp(residual if weight is None else weight * residual) - smooth * tape.smooth(model, WEIGHTS)
        assert b.dtype == dt
        want = tape.solve_normal(b, row_weight=weight, smooth=smooth, smooth_weights=WEIGHTS, damp=damp, maxiter=4, return_info=True)
        got = gauss_newton_step(tape, residual, model, row_weight=weight, smooth=smooth, damp=damp, smooth_weights=WEIGHTS, maxiter=4,
                                return_info=True)
        _bits_equal(got[0], want[0])
        assert got[1] == want[1] and got[1]["iterations"] == 4
    b0 = tape.vjp(residual)
    _bits_equal(gauss_newton_step(tape, residual, model, damp=damp, maxiter=2), tape.solve_normal(b0, damp=damp, maxiter=2))
