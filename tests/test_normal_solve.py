"""The normal equations of the field tape without a device: the numpy restatements of tests/normal_reference.py -- what the
device is compared with bit for bit in tests/test_normal_solve_gpu.py -- against independent definitions (compute_K's sparse matrices,
math.fsum of exact products, a dense solve), the degenerate systems, and every argument error of the Python layer and of the C entries
before any device call."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adjoint_reference as AR  # noqa: E402,F401  (tangent_reference imports it)
import normal_reference as NR  # noqa: E402
import tangent_reference as TR  # noqa: E402

DX = 0.3
LENGTHS = (3, 4, 5, 6, 9)
WEIGHTS = [(1.0, 1.0, 1.0), (2.0, 0.5, 1.25), (1.0, 0.0, 3.0)]


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


# ---- 1. the restated smoothing operator against compute_K's matrices
def _to_k_order(v, shape):
    """tape order (x fastest) -> compute_K's order (C order of shape: z fastest)"""
    mx, my, mz = shape
    return np.asarray(v).reshape(mz, my, mx).transpose(2, 1, 0).ravel()


def _smooth_shapes():
    out = []
    for pos in range(3):
        for n in LENGTHS:
            shape = [4, 5, 6]
            shape[pos] = n
            out.append(tuple(shape))
    return out


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("kind", ["nodes", "cells"])
@pytest.mark.parametrize("shape", _smooth_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_restated_smooth_against_compute_K(shape, kind, dt):
    from ttcr_amd import inversion

    # the parameters of a node grid of `shape` nodes, or the cells of the node grid one node larger along every axis: `shape` either way
    nn = shape if kind == "nodes" else tuple(n + 1 for n in shape)
    params = nn if kind == "nodes" else tuple(n - 1 for n in nn)
    assert params == shape
    K = inversion.smoothing_matrices(params, (DX, DX, DX), order=2)
    rng = np.random.default_rng(sum(shape) + (0 if kind == "nodes" else 100))
    n = int(np.prod(params))
    v = (rng.standard_normal(n) * 2.0 ** rng.integers(-3, 4, n)).astype(dt)
    vk = _to_k_order(v, params).astype(np.float64)
    eps = float(np.finfo(dt).eps)
    for a in WEIGHTS:
        got = _to_k_order(NR.smooth(v, params, DX, a, dtype=dt), params).astype(np.float64)
        want = sum(a[d] * (K[d].T @ (K[d] @ vk)) for d in range(3))
        bound = 64 * eps * sum(a[d] * (abs(K[d]).T @ (abs(K[d]) @ np.abs(vk))) for d in range(3))
        err = np.abs(got - want)
        print("smooth %s %s %s weights %s: max error / bound %.3f" % (shape, kind, np.dtype(dt).name, a, float(np.max(err / np.maximum(bound, 1e-300)))))
        assert np.all(err <= bound)
    assert np.any(want != 0)


def test_restated_smooth_refuses_short_axes():
    for shape in ((2, 4, 5), (4, 2, 5), (4, 5, 2)):
        with pytest.raises(ValueError, match="at least 3"):
            NR.smooth(np.zeros(int(np.prod(shape))), shape, DX, dtype=np.float64)


# ---- 2. the restated inner product against math.fsum of the exact products
def _two_prod(a, b):
    """a * b = p + e exactly (Dekker), float64 arrays of moderate magnitude"""
    def split(x):
        c = 134217729.0 * x
        hi = c - (c - x)
        return hi, x - hi
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025, 262144, 262145])
def test_restated_dot_against_fsum(n, dt):
    rng = np.random.default_rng(n)
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 13, n)).astype(dt)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 13, n)).astype(dt)
    got = NR.dot(a, b)
    p, e = _two_prod(a.astype(np.float64), b.astype(np.float64))
    if dt == np.float32:
        assert not np.any(e)   # (24-bit factors: the double products are exact)
    want = math.fsum(np.concatenate([p, e]).tolist())
    moduli = math.fsum(np.abs(p).tolist())
    bound = n * float(np.finfo(np.float64).eps) * moduli
    print("dot n = %d %s: error %.3e, bound %.3e" % (n, np.dtype(dt).name, abs(got - want), bound))
    assert isinstance(got, float) and abs(got - want) <= bound
    assert NR.dot(b, a) == got


def test_restated_dot_pairing():
    """the order itself: one large element per thread slot cancels only under the pairing of the definition"""
    e = np.zeros(2048, dtype=np.float64)
    e[0], e[256], e[512] = 1e300, -1e300, 1.0        # thread 0 of chunk 0: ((1e300 - 1e300) + 1) + 0 = 1
    e[1024 + 3], e[1024 + 3 + 128] = 3.0, 4.0        # chunk 1: threads 3 and 131 meet at stride 128
    assert NR.dot(e, np.ones_like(e)) == 8.0
    e[0], e[256], e[512] = 1e300, 1.0, -1e300        # (1e300 + 1) - 1e300 = 0: the 1 is lost
    assert NR.dot(e, np.ones_like(e)) == 7.0


# ---- 3. the restated recurrence on a dense system
NN = (6, 5, 7)
CG_DX = 0.5


@pytest.fixture(scope="module")
def dense():
    """J of two events on the 6 x 5 x 7 node grid from the tangent restatement (fp64, fields from the oracle), R from compute_K"""
    from oracle import oracle as O
    from ttcr_amd import inversion

    n = int(np.prod(NN))
    rng = np.random.default_rng(17)
    X, Y, Z = np.meshgrid(*[np.arange(k) * CG_DX for k in NN], indexing="ij")
    s = (0.5 + 0.02 * X + 0.015 * Y + 0.03 * Z + 0.05 * np.sin(0.9 * X) * np.cos(0.7 * Y + 0.3 * Z)).flatten("F")
    hi = (np.array(NN) - 1) * CG_DX
    srcs = [np.array([[0.7, 0.9, 1.1]]), np.array([[1.9, 1.3, 2.6]])]
    rcvs = [rng.uniform(0.2, hi - 0.2, (10, 3)) for _ in srcs]
    fields = []
    for src, rcv in zip(srcs, rcvs):
        o = O.solve3d(np.float64, tuple(k - 1 for k in NN), CG_DX, (0.0, 0.0, 0.0), s, src, rcv=rcv, eps=1e-15, maxit=200)
        assert o["niter"] < 200 and o["change"][-1] == 0
        fields.append(o["tt"])
    J = np.zeros((20, n))
    for j in range(n):
        unit = np.zeros(n)
        unit[j] = 1.0
        _, dtts = TR.tangent(fields, s, CG_DX, NN, (0.0, 0.0, 0.0), srcs, unit, rcvs=rcvs)
        J[:, j] = np.concatenate(dtts)
    K = inversion.smoothing_matrices(NN, (CG_DX,) * 3, order=2)
    perm = _to_k_order(np.arange(n), NN)     # perm[k] = the tape index of compute_K's parameter k
    Rk = sum((Kd.T @ Kd).toarray() for Kd in K)
    R = np.zeros((n, n))
    R[np.ix_(perm, perm)] = Rk
    return dict(J=J, R=R, n=n, rng=rng)


def _system(dense, rw, smooth, damp):
    H = dense["J"].T @ (rw[:, None] * dense["J"])
    A = H + smooth * dense["R"] + damp * np.eye(dense["n"])
    return H, A


def test_restated_cg_on_a_dense_system(dense):
    n, rng = dense["n"], np.random.default_rng(23)
    rtol = 1e-6
    rw = rng.uniform(0.5, 2.0, 20)
    smooth, damp = 1e-3, 1e-1
    H, A = _system(dense, rw, smooth, damp)
    cond = np.linalg.cond(A)
    assert cond * np.finfo(np.float64).eps < 0.01 * rtol, cond
    b = rng.standard_normal(n)
    x, info = NR.cg(lambda p: H @ p, b, np.float64, smooth_op=lambda p: NR.smooth(p, NN, CG_DX), smooth=smooth, damp=damp, maxiter=n,
                    rtol=rtol)
    true = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print("cg: cond %.3e, %d iterations, recurrence residual %.3e, true residual %.3e"
          % (cond, info["iterations"], math.sqrt(info["rho"][-1] / info["rho"][0]), true))
    assert info["status"] == 0 and 1 <= info["iterations"] < n
    assert len(info["rho"]) == info["iterations"] + 2 and len(info["pq"]) == info["iterations"]
    assert info["rho"][-1] <= rtol * rtol * info["rho"][0] < info["rho"][-2]
    assert true <= 2 * rtol
    # a start at the solution: the test is met before the first product; a start elsewhere reaches the same solution
    x2, info2 = NR.cg(lambda p: H @ p, b, np.float64, smooth_op=lambda p: NR.smooth(p, NN, CG_DX), smooth=smooth, damp=damp, x0=x,
                      maxiter=n, rtol=2 * rtol)
    assert info2["status"] == 0 and info2["iterations"] == 0 and np.array_equal(x2, x) and info2["pq"] == []
    x3, info3 = NR.cg(lambda p: H @ p, b, np.float64, smooth_op=lambda p: NR.smooth(p, NN, CG_DX), smooth=smooth, damp=damp,
                      x0=rng.standard_normal(n), maxiter=n, rtol=rtol)
    assert info3["status"] == 0 and np.linalg.norm(b - A @ x3) / np.linalg.norm(b) <= 2 * rtol


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_every_intermediate_is_in_the_dtype(dense, dt):
    """the restatement in fp32 is not the fp64 one rounded: it solves the system to fp32 accuracy with fp32 vectors"""
    n, rng = dense["n"], np.random.default_rng(29)
    H, A = _system(dense, np.ones(20), 1e-3, 1.0)
    b = rng.standard_normal(n).astype(dt)
    Hd = H.astype(dt)
    x, info = NR.cg(lambda p: Hd @ p, b, dt, smooth_op=lambda p: NR.smooth(p, NN, CG_DX, dtype=dt), smooth=1e-3, damp=1.0, maxiter=n,
                    rtol=1e-3)
    assert x.dtype == dt and info["status"] == 0
    assert np.linalg.norm(b - A @ x.astype(np.float64)) / np.linalg.norm(b) <= 1e-2


# ---- 4. degenerate systems
def test_degenerate_systems(dense):
    n, rng = dense["n"], np.random.default_rng(31)
    J = dense["J"]
    b = rng.standard_normal(n)
    x0 = rng.standard_normal(n)
    zero = np.zeros(20)
    for start in (None, x0):
        x, info = NR.cg(lambda p: J.T @ (zero * (J @ p)), b, np.float64, x0=start, maxiter=7)
        assert info["status"] == 2 and info["iterations"] == 0 and info["pq"] == [0.0] and len(info["rho"]) == 2
        assert np.array_equal(x, np.zeros(n) if start is None else start)
    H, A = _system(dense, np.ones(20), 0.0, 1e-1)
    x, info = NR.cg(lambda p: H @ p, b, np.float64, damp=1e-1, maxiter=1)
    assert info["status"] == 1 and info["iterations"] == 1 and len(info["rho"]) == 3 and len(info["pq"]) == 1 and np.any(x != 0)
    # rhs = 0: the test is met at once
    x, info = NR.cg(lambda p: H @ p, np.zeros(n), np.float64, damp=1e-1, maxiter=3)
    assert info["status"] == 0 and info["iterations"] == 0 and not np.any(x)


# ---- 5. argument errors, before anything is launched
class _NoLibrary:
    """stands in for the C library of a tape that has no device: reaching it is the failure"""
    def __getattr__(self, name):
        if name == "ttcr_fsm_adjoint_free":
            return lambda h: 0
        raise AssertionError("the call reached the library (%s)" % name)


@pytest.fixture()
def fake_tape():
    from ttcr_amd.rgrid import FieldTape

    t = object.__new__(FieldTape)
    t._lib, t._h = _NoLibrary(), C.c_void_p(1)
    t.dtype, t.n_cols, t.n_data, t._per, t.device = np.dtype(np.float32), 60, 7, "node", 0
    t._rows = np.arange(7)
    yield t
    t._h = C.c_void_p()


def test_python_argument_errors(fake_tape):
    t = fake_tape
    b, rw = np.zeros(60, dtype=np.float32), np.ones(7, dtype=np.float32)
    bad = [
        (dict(smooth=-1.0), "smooth"), (dict(smooth=float("nan")), "smooth"), (dict(damp=-1e-3), "damp"), (dict(damp=float("inf")), "damp"),
        (dict(maxiter=0), "maxiter"), (dict(maxiter=-2), "maxiter"), (dict(maxiter=2.5), "maxiter"), (dict(rtol=-1e-6), "rtol"),
        (dict(hessian="full"), "hessian"), (dict(hessian=None), "hessian"), (dict(schedule="fast"), "schedule"),
        (dict(smooth_weights=(1.0, 1.0)), "smooth_weights"), (dict(smooth_weights=(1.0, -1.0, 1.0)), "smooth_weights"),
        (dict(row_weight=np.ones(6)), "row_weight"), (dict(row_weight=np.ones((7, 1))), "row_weight"), (dict(x0=np.zeros(59)), "x0"),
    ]
    for kw, name in bad:
        with pytest.raises(ValueError, match=name):
            t.solve_normal(b, **{"row_weight": rw, **kw})
    with pytest.raises(ValueError, match="rhs"):
        t.solve_normal(np.zeros(61, dtype=np.float32))
    with pytest.raises(ValueError, match="v should hold 60"):
        t.smooth(np.zeros(59))
    with pytest.raises(ValueError, match="weights"):
        t.smooth(b, weights=(1.0, 2.0, float("nan")))
    with pytest.raises(ValueError, match="a should hold 60"):
        t.dot(np.zeros(3), b)
    with pytest.raises(ValueError, match="b should hold 60"):
        t.dot(b, np.zeros(61))
    with pytest.raises(AssertionError, match="reached the library"):   # (and a good call does get there)
        t.solve_normal(b, row_weight=rw, smooth=1.0, damp=1.0)


def _err(lib, status, *words):
    from ttcr_amd import _lib

    assert status == _lib.ERR_VALUE, status
    msg = _lib.last_error()
    assert msg and all(w in msg for w in words), msg


def test_c_argument_errors_come_before_the_device(lib):
    from ttcr_amd import _lib

    names = ("ttcr_fsm_normal_tile_edge", "ttcr_fsm_normal_smooth", "ttcr_fsm_normal_dot", "ttcr_fsm_normal_solve", "ttcr_fsm_normal_release")
    for n in names:
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None
    assert lib.ttcr_fsm_normal_tile_edge(_lib.TTCR_F32) == 16 and lib.ttcr_fsm_normal_tile_edge(_lib.TTCR_F64) == 12
    a = np.zeros(8, dtype=np.float32)
    p = a.ctypes.data_as(C.c_void_p)
    w3 = (C.c_double * 3)(1.0, 1.0, 1.0)
    neg = (C.c_double * 3)(1.0, -1.0, 1.0)
    st, it = C.c_int(-7), C.c_int(-7)
    rho, pq = (C.c_double * 8)(), (C.c_double * 8)()
    out = C.c_double(-7.0)

    def solve(**kw):
        v = dict(t=None, rhs=p, rw=None, smooth=1.0, w=w3, damp=1.0, x0=None, maxiter=3, rtol=1e-6, newton=0, schedule=0, x=p, st=C.byref(st),
                 it=C.byref(it), rho=rho, pq=pq)
        v.update(kw)
        return lib.ttcr_fsm_normal_solve(v["t"], v["rhs"], 0, v["rw"], 0, v["smooth"], v["w"], v["damp"], v["x0"], 0, v["maxiter"], v["rtol"],
                                         v["newton"], v["schedule"], v["x"], 0, v["st"], v["it"], v["rho"], v["pq"], None)

    _err(lib, solve(smooth=-1.0), "smooth")
    _err(lib, solve(smooth=float("nan")), "smooth")
    _err(lib, solve(damp=-0.5), "damp")
    _err(lib, solve(maxiter=0), "maxiter")
    _err(lib, solve(rtol=-1.0), "rtol")
    _err(lib, solve(newton=2), "hessian")
    _err(lib, solve(w=None), "null smooth_weights")
    _err(lib, solve(w=neg), "smooth_weights")
    _err(lib, solve(schedule=2), "schedule")
    _err(lib, solve(rhs=None), "null rhs")
    _err(lib, solve(x=None), "null x")
    _err(lib, solve(st=None), "null status")
    _err(lib, solve(), "null tape")
    _err(lib, solve(newton=1), "null tape")
    _err(lib, lib.ttcr_fsm_normal_smooth(None, p, 0, None, p, 0), "null weights")
    _err(lib, lib.ttcr_fsm_normal_smooth(None, p, 0, neg, p, 0), "weights")
    _err(lib, lib.ttcr_fsm_normal_smooth(None, None, 0, w3, p, 0), "null v")
    _err(lib, lib.ttcr_fsm_normal_smooth(None, p, 0, w3, None, 0), "null out")
    _err(lib, lib.ttcr_fsm_normal_smooth(None, p, 0, w3, p, 0), "null tape")
    _err(lib, lib.ttcr_fsm_normal_dot(None, None, 0, p, 0, C.byref(out)), "null a")
    _err(lib, lib.ttcr_fsm_normal_dot(None, p, 0, None, 0, C.byref(out)), "null b")
    _err(lib, lib.ttcr_fsm_normal_dot(None, p, 0, p, 0, None), "null result")
    _err(lib, lib.ttcr_fsm_normal_dot(None, p, 0, p, 0, C.byref(out)), "null tape")
    _err(lib, lib.ttcr_fsm_normal_release(None), "null tape")
    assert st.value == -7 and it.value == -7 and out.value == -7.0 and not np.any(a)   # (no call got as far as its outputs)


def test_python_layer_has_the_methods_without_torch():
    import subprocess

    code = ("import sys, ttcr_amd; from ttcr_amd.rgrid import FieldTape; from ttcr_amd.inversion import gauss_newton_step; "
            "assert all(callable(getattr(FieldTape, a, None)) for a in ('smooth', 'dot', 'solve_normal', 'release_solve')); "
            "assert 'torch' not in sys.modules")
    subprocess.check_call([sys.executable, "-c", code], cwd=os.path.dirname(HERE))
