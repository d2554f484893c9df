"""The coarse model grid of a field tape without a device, on the restatement tests/model_reference.py that the device is
compared with bit for bit: P and P^T with m = n are the identity; P reproduces a linear function exactly where the weights are dyadic;
P^T e_n is row n of P, unit vector by unit vector (support ranges, the last-node clamp); the dot-product identity within a bound derived
from the roundings; the gradient P^T (node gradient of tests/adjoint_reference.py) is the derivative of what the oracle computes for
s = P m (central finite differences, the project's 1e-6 relative); the per-axis smoothing operator equals tests/normal_reference.py for
m = n and leaves out the axes it has to; and the Python layer and the C entries refuse bad arguments before any device call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_reference as AR  # noqa: E402
import model_reference as MR  # noqa: E402
import normal_reference as NR  # noqa: E402

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
MODEL_SYMBOLS = ["ttcr_fsm_model_raytrace_multi_adjoint", "ttcr_fsm_model_shape", "ttcr_fsm_model_tape_prolong",
                 "ttcr_fsm_model_tape_restrict", "ttcr_fsm_model_device", "ttcr_fsm_model_prolong", "ttcr_fsm_model_restrict"]


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- identity
@DTYPES
@pytest.mark.parametrize("n", [(5, 7, 4), (2, 2, 2), (9, 1, 3)], ids=_ids)
def test_identity_bit_for_bit(dt, n):
    rng = np.random.default_rng(11)
    v = rng.standard_normal(int(np.prod(n))).astype(dt)
    v[:3] = [-0.0, np.finfo(dt).tiny / 4, np.finfo(dt).max]   # (a signed zero, a subnormal and the largest value go through unchanged)
    assert same_bits(MR.prolong(v, n, n, dt), v)
    assert same_bits(MR.restrict(v, n, n, dt), v)


# ---- linear reproduction
@DTYPES
def test_linear_function_is_reproduced_exactly(dt):
    n, m = (9, 9, 9), (3, 5, 9)
    a, b, c, d = 1.5, 0.25, -0.75, 2.0   # dyadic rationals; coordinates are the fine indices
    mc = [np.arange(m[k]) * ((n[k] - 1) // (m[k] - 1)) for k in range(3)]
    Zm, Ym, Xm = np.meshgrid(mc[2], mc[1], mc[0], indexing="ij")
    v = (a + b * Xm + c * Ym + d * Zm).astype(dt).ravel()
    Z, Y, X = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    want = (a + b * X + c * Y + d * Z).astype(dt).ravel()
    assert same_bits(MR.prolong(v, n, m, dt), want)


# ---- transpose rows
@DTYPES
@pytest.mark.parametrize("n,m", [((5, 7, 4), (2, 3, 2)), ((6, 1, 5), (3, 1, 1))], ids=_ids)
def test_transpose_rows_on_unit_vectors(dt, n, m):
    """Both directions against W, the products w_x w_y w_z of the rounded per-axis weights: the same entries are non-zero, and every
    entry is W's within the two roundings of its two products (P multiplies x first, P^T z first, so the two are not each other's bits):
    3 u_T relative, which leaves room for W itself being formed in fp64."""
    nn, nm = int(np.prod(n)), int(np.prod(m))
    P = np.zeros((nn, nm), dtype=dt)
    for c in range(nm):
        e = np.zeros(nm, dtype=dt)
        e[c] = 1
        P[:, c] = MR.prolong(e, n, m, dt)
    W = MR.weight_matrix(n, m, dt)
    tol = 3 * (np.finfo(dt).eps / 2)
    assert np.array_equal(P != 0, W != 0) and np.all(np.abs(P.astype(np.float64) - W) <= tol * W)
    assert np.all(np.abs(W.sum(axis=1) - 1) <= 8 * tol)   # (the weights of a fine node sum to one)
    for k in range(nn):
        e = np.zeros(nn, dtype=dt)
        e[k] = 1
        row = MR.restrict(e, n, m, dt)
        assert row.dtype == np.dtype(dt) and np.array_equal(row != 0, W[k] != 0), (k, row, W[k])
        assert np.all(np.abs(row.astype(np.float64) - W[k]) <= tol * W[k]), (k, row, W[k])


# ---- dot test
DOT_CASES = [((17, 9, 11), (4, 3, 5)), ((13, 13, 13), (1, 1, 4)), ((5, 7, 4), (5, 7, 4)), ((37, 35, 41), (5, 4, 6))]


@DTYPES
@pytest.mark.parametrize("n,m", DOT_CASES, ids=_ids)
def test_dot_product_identity_within_the_rounding_bound(dt, n, m):
    """|<P v, u> - <v, P^T u>| <= 4 (L_x + L_y + L_z + 9) u_T S: one rounding per weight and per product and L - 1 additions per stage
    give (L_x + L_y + L_z + 9) u_T S per side to first order; the bar is twice the two sides.  The inner products are taken in fp64."""
    rng = np.random.default_rng(23 + n[0])
    v = rng.standard_normal(int(np.prod(m))).astype(dt)
    u = rng.standard_normal(int(np.prod(n))).astype(dt)
    Pv, Ptu = MR.prolong(v, n, m, dt), MR.restrict(u, n, m, dt)
    lhs, rhs = Pv.astype(np.float64) @ u.astype(np.float64), v.astype(np.float64) @ Ptu.astype(np.float64)
    W = MR.weight_matrix(n, m, dt)
    S = float(np.abs(u.astype(np.float64)) @ (np.abs(W) @ np.abs(v.astype(np.float64))))
    L = MR.stage_lengths(n, m)
    uT = np.finfo(dt).eps / 2
    bound = 4 * (sum(L) + 9) * uT * S
    print("dot test %s / %s %s: |lhs - rhs| = %.3e, bound %.3e (L = %s, S = %.3e)" % (_ids(n), _ids(m), np.dtype(dt).name, abs(lhs - rhs), bound, L, S))
    assert abs(lhs - rhs) <= bound


# ---- finite differences of the oracle on s = P m (fp64, eps = 1e-15: the field is a fixed point of the sweeps)
DX = 0.5
MN = (0.0, 0.0, 0.0)
TOL = 1e-6
STEP = 1e-6
FD_CASES = {
    "21x21x21_5x5x5": ((21, 21, 21), (5, 5, 5), [[6.6, 8.2, 11.4]]),
    "12x9x14_1x1x5_two_points": ((12, 9, 14), (1, 1, 5), [[3.3, 4.1, 5.7], [3.6, 4.2, 5.4]]),
}


def _rough_model(m, rng):
    """a smooth trend times 1 +- 30 % noise, one value per model node, flat, x fastest"""
    ax = [np.linspace(0.0, 5.0, k) if k > 1 else np.array([2.5]) for k in m]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    s = 0.5 + 0.04 * X + 0.03 * Y + 0.06 * Z + 0.05 * np.sin(0.9 * X) * np.cos(0.7 * Y + 0.3 * Z)
    return (s * (1.0 + 0.30 * rng.uniform(-1, 1, s.shape))).flatten("F")


def _solve(n, s, src, rcv):
    from oracle import oracle as O

    o = O.solve3d(np.float64, tuple(k - 1 for k in n), DX, MN, s, src, rcv=rcv, eps=1e-15, maxit=200)
    assert o["niter"] < 200 and o["change"][-1] <= 1e-13, (o["niter"], o["change"][-3:])
    return o


@pytest.mark.parametrize("case", sorted(FD_CASES))
def test_model_gradient_is_the_derivative_of_the_oracle(case):
    n, m, src = FD_CASES[case]
    src = np.array(src) * DX
    rng = np.random.default_rng(5)
    mv = _rough_model(m, rng)
    hi = (np.array(n) - 1) * DX
    rcv = rng.uniform(0.1 * hi, 0.9 * hi, (30, 3))
    w = rng.standard_normal(30)
    gfield = rng.standard_normal(int(np.prod(n)))
    dm = mv * rng.standard_normal(mv.size)
    s = MR.prolong(mv, n, m, np.float64)
    o = _solve(n, s, src, rcv)
    g_rcv = MR.restrict(AR.adjoint([o["tt"]], s, DX, n, MN, [src], rcvs=[rcv], ws=[w]), n, m, np.float64)
    g_fld = MR.restrict(AR.adjoint([o["tt"]], s, DX, n, MN, [src], field_cot=[gfield]), n, m, np.float64)
    op = _solve(n, MR.prolong(mv + STEP * dm, n, m, np.float64), src, rcv)
    om = _solve(n, MR.prolong(mv - STEP * dm, n, m, np.float64), src, rcv)
    fd_rcv = (w @ op["tt_rcv"] - w @ om["tt_rcv"]) / (2 * STEP)
    fd_fld = (gfield @ op["tt"] - gfield @ om["tt"]) / (2 * STEP)
    e_rcv = abs(g_rcv @ dm - fd_rcv) / abs(fd_rcv)
    e_fld = abs(g_fld @ dm - fd_fld) / abs(fd_fld)
    print("model gradient vs oracle finite differences, %s: receivers %.2e, field %.2e (bound %.0e)" % (case, e_rcv, e_fld, TOL))
    assert e_rcv <= TOL and e_fld <= TOL, (e_rcv, e_fld)


# ---- smoothing
@DTYPES
def test_smoothing_with_m_equal_n_is_the_node_operator(dt):
    n = (6, 5, 7)
    rng = np.random.default_rng(3)
    v = rng.standard_normal(int(np.prod(n))).astype(dt)
    for dx, weights in ((0.5, (1.0, 1.0, 1.0)), (0.3, (0.5, 0.0, 2.0))):
        assert same_bits(MR.smooth(v, n, n, dx, weights, dt), NR.smooth(v, n, dx, weights, dt))


@DTYPES
def test_smoothing_uses_the_model_spacing_and_leaves_out_short_axes(dt):
    T = np.dtype(dt).type
    n, m, dx = (13, 13, 13), (1, 2, 4), 0.5
    rng = np.random.default_rng(4)
    v = rng.standard_normal(int(np.prod(m))).astype(dt)
    out = MR.smooth(v, n, m, dx, (0.0, 0.0, 1.5), dt)
    h = dx * 12 / 3
    ih2 = T(1.0 / (h * h))
    want = T(1.5) * NR._axis(v.reshape(m[2], m[1], m[0]), 0, ih2, T(-2) * ih2)   # the z axis alone: no zero terms of x and y in the sum
    assert same_bits(out, want.ravel())
    for weights in ((1.0, 0.0, 1.0), (0.0, 0.5, 1.0)):
        with pytest.raises(ValueError, match="weight 0"):
            MR.smooth(v, n, m, dx, weights, dt)
    assert same_bits(MR.smooth(v[:2], n, (1, 2, 1), dx, (0.0, 0.0, 0.0), dt), np.zeros(2, dtype=dt))
    assert MR.spacings(n, (3, 5, 13), dx) == (3.0, 1.5, 0.5)


# ---- arguments, before any device call
@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def test_model_symbols_exported_and_declared(lib):
    import re

    from ttcr_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ttcr_amd.h")).read()
    pxd = open(os.path.join(ROOT, "integration", "ttcr_amd.pxd")).read()
    for name in MODEL_SYMBOLS:
        assert len(re.findall(r"^int %s\(" % name, hdr, re.M)) == 1 and len(re.findall(r"^    int %s\(" % name, pxd, re.M)) == 1, name
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert not name.startswith(("ttcr_fsm_adjoint_", "ttcr_fsm_normal_", "ttcr_fsm_joint_", "ttcr_fsm_rjoint_", "ttcr_fsm_rcv_"))


def test_c_entries_refuse_null_arguments_before_the_device(lib):
    from ttcr_amd import _lib

    fake = C.c_void_p(1234)   # never dereferenced: the argument checks come first
    shape = (C.c_int * 3)(2, 2, 2)
    h = C.c_void_p(1234)
    assert lib.ttcr_fsm_model_raytrace_multi_adjoint(None, 0, None, None, None, None, None, None, None, shape) == _lib.ERR_VALUE
    assert "tape" in _lib.last_error()
    assert lib.ttcr_fsm_model_raytrace_multi_adjoint(fake, -1, None, None, None, None, None, None, C.byref(h), shape) == _lib.ERR_VALUE
    assert "model_raytrace_multi_adjoint" in _lib.last_error() and h.value is None
    h = C.c_void_p(1234)
    assert lib.ttcr_fsm_model_raytrace_multi_adjoint(None, 0, None, None, None, None, None, None, C.byref(h), shape) == _lib.ERR_VALUE
    assert "null grid" in _lib.last_error() and h.value is None
    d = C.c_int(0)
    assert lib.ttcr_fsm_model_shape(None, C.byref(d), shape) == _lib.ERR_VALUE and "null" in _lib.last_error()
    assert lib.ttcr_fsm_model_shape(fake, None, shape) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_model_shape(fake, C.byref(d), None) == _lib.ERR_VALUE
    buf = (C.c_double * 8)()
    assert lib.ttcr_fsm_model_device(None, C.byref(d)) == _lib.ERR_VALUE and _lib.last_error() == "null grid handle"
    assert lib.ttcr_fsm_model_device(fake, None) == _lib.ERR_VALUE and _lib.last_error() == "null device"
    for entry in (lib.ttcr_fsm_model_tape_prolong, lib.ttcr_fsm_model_tape_restrict):
        assert entry(fake, None, 0, buf, 0) == _lib.ERR_VALUE and _lib.last_error() == "null in"
        assert entry(fake, buf, 0, None, 0) == _lib.ERR_VALUE and _lib.last_error() == "null out"
        assert entry(None, buf, 0, buf, 0) == _lib.ERR_VALUE and _lib.last_error() == "null tape"
    for entry in (lib.ttcr_fsm_model_prolong, lib.ttcr_fsm_model_restrict):
        assert entry(fake, shape, None, 0, buf, 0) == _lib.ERR_VALUE and _lib.last_error() == "null in"
        assert entry(fake, shape, buf, 0, None, 0) == _lib.ERR_VALUE and _lib.last_error() == "null out"
        assert entry(None, shape, buf, 0, buf, 0) == _lib.ERR_VALUE and _lib.last_error() == "null grid handle"


def _stub_grid(cell_slowness=False, ndim=3, n=(5, 7, 4)):
    """a grid object without a handle: what the Python layer checks before it calls the library"""
    from ttcr_amd.rgrid import Grid3d_f

    g = object.__new__(Grid3d_f)
    g._h, g._lib = C.c_void_p(), None
    g._ndim = ndim
    g.cell_slowness = cell_slowness
    g._x, g._y, g._z = (np.arange(k, dtype=np.float32) for k in n)
    return g


def test_python_layer_refuses_bad_arguments_before_the_device():
    import inspect

    from ttcr_amd import inversion
    from ttcr_amd.rgrid import FieldTape, _Grid3d, _model_shape_arg

    assert inspect.signature(_Grid3d.raytrace_adjoint).parameters["model_shape"].default is None
    src, rcv = np.zeros((1, 3)), np.zeros((2, 3))
    g = _stub_grid()
    for kw, word in [(dict(wrt="nodes", model_shape=(2, 2, 2)), "model_shape goes with wrt='model'"),
                     (dict(wrt="cells", model_shape=(2, 2, 2)), "model_shape goes with wrt='model'"),
                     (dict(wrt="model"), "needs model_shape"),
                     (dict(wrt="model", model_shape=(2, 2)), "model_shape should be three integers"),
                     (dict(wrt="model", model_shape=(0, 2, 2)), "model_shape should be three integers"),
                     (dict(wrt="model", model_shape=(6, 2, 2)), "model_shape should be three integers"),
                     (dict(wrt="model", model_shape=(2, 2.5, 2)), "model_shape should be three integers"),
                     (dict(wrt="model", model_shape="abc"), "model_shape should be three integers"),
                     (dict(wrt="nothing"), "wrt should be 'nodes' or 'cells', got 'nothing' .*'model'")]:
        with pytest.raises(ValueError, match=word):
            g.raytrace_adjoint(src, rcv, **kw)
    with pytest.raises(ValueError, match="slowness defined at the nodes"):
        _stub_grid(cell_slowness=True).raytrace_adjoint(src, rcv, wrt="model", model_shape=(2, 2, 2))
    for fn in (g.prolong, g.restrict):
        with pytest.raises(ValueError, match="model_shape should be three integers"):
            fn(np.zeros(8), (2, 2, 9))
    with pytest.raises(ValueError, match="v should hold 12 values"):
        g.prolong(np.zeros(11), (2, 3, 2))
    with pytest.raises(ValueError, match="g should hold 140 values"):
        g.restrict(np.zeros(12), (2, 3, 2))
    with pytest.raises(ValueError, match="slowness defined at the nodes"):
        _stub_grid(cell_slowness=True).prolong(np.zeros(8), (2, 2, 2))
    assert _model_shape_arg(np.array([1, 7, 4]), (5, 7, 4)) == (1, 7, 4)
    for name in ("prolong", "restrict", "model_coordinates"):
        assert hasattr(FieldTape, name)
    assert hasattr(inversion, "apply_model_update")


def test_update_helper_adds_the_prolonged_step():
    from ttcr_amd import inversion

    class Tape:
        def prolong(self, dm):
            return MR.prolong(dm, (5, 7, 4), (2, 3, 2), np.float64)

    rng = np.random.default_rng(9)
    s, dm = rng.uniform(0.2, 1.0, 140), rng.standard_normal(12)
    assert same_bits(inversion.apply_model_update(Tape(), s, dm), s + MR.prolong(dm, (5, 7, 4), (2, 3, 2), np.float64))
