"""The joint hypocentre-velocity system of the field tape without a device: the numpy restatement of
tests/joint_reference.py -- what the device is compared with bit for bit in tests/test_joint_solve_gpu.py -- against the restated
separate calls (jvp plus jvp_source), against central finite differences of the oracle along a joint direction, against the restated
reverse mode (dot-product identity) and, for the recurrence, on a dense joint system; every argument error of the Python layer and of the
C entries before any device call."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import joint_reference as JR  # noqa: E402
import normal_reference as NR  # noqa: E402
import source_reference as SR  # noqa: E402
import tangent_reference as TR  # noqa: E402
from test_tangent import DOT_TOL, DX, MN, N, NN3, STEP, TOL, model  # noqa: E402  (grid, model, step and bounds of 6c / 6d)

JOINT_SYMBOLS = ["ttcr_fsm_joint_jvp", "ttcr_fsm_joint_gn", "ttcr_fsm_joint_solve", "ttcr_fsm_joint_release"]
CASES = {
    "off_node": ([[3.3, 4.1, 5.7]], "smooth"),
    "two_points": ([[3.3, 4.1, 5.7], [3.6, 4.2, 5.4]], "smooth"),   # the boxes overlap: the last writer wins
    "rough": ([[6.2, 2.9, 4.4]], "rough"),
}


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def _solve(s, src, t0, rcv, dt=np.float64):
    from oracle import oracle as O

    o = O.solve3d(dt, (N - 1,) * 3, DX, MN, s, src, t0=t0, rcv=rcv, eps=1e-15, maxit=200)
    assert o["niter"] < 200 and o["change"][-1] == 0, (o["niter"], o["change"][-3:])
    return o


def _setup(case):
    src, kind = CASES[case]
    src = np.array(src)
    s = model(kind)
    rng = np.random.default_rng(5)
    rcv = rng.uniform(0.6, (N - 1) * DX - 0.6, (30, 3))
    w = rng.standard_normal(30)
    t0 = rng.uniform(0, 0.5, src.shape[0]).round(3)
    ds = s * rng.standard_normal(s.size)
    dsrc = rng.standard_normal((src.shape[0], 4))
    return src, t0, s, rcv, w, ds, dsrc


_FIELDS = {}


def _field(case, dt):
    """the oracle's field of a case in a dtype, solved once and shared (never written to)"""
    key = (case, np.dtype(dt).name)
    if key not in _FIELDS:
        src, t0, s, rcv, w, ds, dsrc = _setup(case)
        _FIELDS[key] = _solve(s.astype(dt), src.astype(dt), t0.astype(dt), rcv.astype(dt), dt)["tt"]
        _FIELDS[key].setflags(write=False)
    return _FIELDS[key]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- 1. the joint tangent against the separate calls
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_joint_tangent_against_the_separate_calls(case, dt):
    src, t0, s, rcv, w, ds, dsrc = _setup(case)
    T = _field(case, dt)
    s, ds, dsrc = s.astype(dt), ds.astype(dt), dsrc.astype(dt)
    args = ([T], s, DX, NN3, MN, [src])
    mu_j, dtt_j = JR.joint_tangent(*args, ds, dsrc, rcvs=[rcv])
    mu_s, dtt_s = TR.tangent(*args, ds, rcvs=[rcv])
    mu_e, dtt_e = SR.source_tangent(*args, dsrc, rcvs=[rcv])
    f8 = lambda a: np.asarray(a, dtype=np.float64)   # noqa: E731
    e_fld = _rel(mu_j[0], f8(mu_s[0]) + f8(mu_e[0]))
    e_rcv = _rel(dtt_j[0], f8(dtt_s[0]) + f8(dtt_e[0]))
    print("joint tangent vs jvp + jvp_source, %s, %s: field %.2e, receivers %.2e (bound %.0e)"
          % (case, np.dtype(dt).name, e_fld, e_rcv, DOT_TOL[dt]))
    assert e_fld <= DOT_TOL[dt] and e_rcv <= DOT_TOL[dt]
    assert mu_j[0].dtype == dt and dtt_j[0].dtype == dt
    # each operand alone: the values of the separate call (== : the sign of a zero may differ)
    mu_a, dtt_a = JR.joint_tangent(*args, ds, np.zeros_like(dsrc), rcvs=[rcv])
    assert np.array_equal(mu_a[0], mu_s[0]) and np.array_equal(dtt_a[0], dtt_s[0])
    mu_b, dtt_b = JR.joint_tangent(*args, np.zeros_like(ds), dsrc, rcvs=[rcv])
    assert np.array_equal(mu_b[0], mu_e[0]) and np.array_equal(dtt_b[0], dtt_e[0])
    assert np.any(dtt_s[0] != 0) and np.any(dtt_e[0] != 0)


# ---- 2. central finite differences of the oracle along one joint direction
@pytest.mark.parametrize("case", sorted(CASES))
def test_joint_tangent_is_the_directional_derivative_of_the_oracle(case):
    src, t0, s, rcv, w, ds, dsrc = _setup(case)
    T = _field(case, np.float64)
    mus, dtts = JR.joint_tangent([T], s, DX, NN3, MN, [src], ds, dsrc, rcvs=[rcv])
    cell = np.floor(src / DX)
    for sign in (1, -1):   # no point moves across a cell face
        assert np.array_equal(np.floor((src + sign * STEP * dsrc[:, 1:]) / DX), cell)
    op = _solve(s + STEP * ds, src + STEP * dsrc[:, 1:], t0 + STEP * dsrc[:, 0], rcv)
    om = _solve(s - STEP * ds, src - STEP * dsrc[:, 1:], t0 - STEP * dsrc[:, 0], rcv)
    e_fld = _rel(mus[0], (op["tt"] - om["tt"]) / (2 * STEP))
    e_rcv = _rel(dtts[0], (op["tt_rcv"] - om["tt_rcv"]) / (2 * STEP))
    print("joint tangent vs oracle finite differences, %s: field %.2e, receivers %.2e (bound %.0e)" % (case, e_fld, e_rcv, TOL))
    assert e_fld <= TOL and e_rcv <= TOL, (e_fld, e_rcv)


# ---- 3. forward against reverse
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_dot_product_identity_of_the_joint_tangent(case, dt):
    src, t0, s, rcv, w, ds, dsrc = _setup(case)
    T = _field(case, dt)
    s, ds, dsrc, w = s.astype(dt), ds.astype(dt), dsrc.astype(dt), w.astype(dt)
    _, dtts = JR.joint_tangent([T], s, DX, NN3, MN, [src], ds, dsrc, rcvs=[rcv])
    g_s, g_e = SR.source_adjoint([T], s, DX, NN3, MN, [src], rcvs=[rcv], ws=[w])
    f8 = lambda a: np.asarray(a, dtype=np.float64).ravel()   # noqa: E731
    lhs = f8(w) @ f8(dtts[0])
    rhs = f8(g_s) @ f8(ds) + f8(g_e) @ f8(dsrc)
    err = abs(lhs - rhs) / abs(rhs)
    print("<w, J [v_s; v_e]> against <J^T w, [v_s; v_e]>, %s, %s: %.2e (bound %.0e)" % (case, np.dtype(dt).name, err, DOT_TOL[dt]))
    assert err <= DOT_TOL[dt], (lhs, rhs, err)


# ---- 4. the restated recurrence on a dense joint system
NN = (6, 5, 7)
CG_DX = 0.5
SCALE = np.array([1.0, 0.05, 0.05, 0.05])
SDAMP = np.array([1e-2, 1e-1, 1e-1, 1e-1])


@pytest.fixture(scope="module")
def dense():
    """[J_s J_e] of two events on the 6 x 5 x 7 node grid from the joint tangent restatement (fp64, fields from the oracle), R from
    compute_K"""
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
    J = np.zeros((20, n + 8))
    for j in range(n + 8):
        unit = np.zeros(n + 8)
        unit[j] = 1.0
        _, dtts = JR.joint_tangent(fields, s, CG_DX, NN, (0.0, 0.0, 0.0), srcs, unit[:n], unit[n:].reshape(2, 4), rcvs=rcvs)
        J[:, j] = np.concatenate(dtts)
    K = inversion.smoothing_matrices(NN, (CG_DX,) * 3, order=2)
    perm = np.arange(n).reshape(NN[2], NN[1], NN[0]).transpose(2, 1, 0).ravel()   # perm[k] = the tape index of compute_K's parameter k
    Rk = sum((Kd.T @ Kd).toarray() for Kd in K)
    R = np.zeros((n, n))
    R[np.ix_(perm, perm)] = Rk
    return dict(J=J, R=R, n=n)


def _product(dense, rw, scale):
    J, n = dense["J"], dense["n"]

    def product(ps, pe):
        ve = JR.scale_block(scale, pe, np.float64)
        g = J.T @ (rw * (J @ np.concatenate([ps, ve.ravel()])))
        return g[:n], JR.scale_block(scale, g[n:], np.float64)
    return product


@pytest.mark.parametrize("scaled", [True, False], ids=["scale_and_damp", "plain"])
def test_restated_joint_cg_on_a_dense_system(dense, scaled):
    n, J, rng = dense["n"], dense["J"], np.random.default_rng(23)
    rtol = 1e-6
    rw = rng.uniform(0.5, 2.0, 20)
    smooth, damp = 1e-3, 1e-1
    scale = np.tile(SCALE, (2, 1)) if scaled else None
    sdamp = np.tile(SDAMP, (2, 1)) if scaled else None
    S = np.concatenate([np.ones(n), scale.ravel() if scaled else np.ones(8)])
    A = S[:, None] * (J.T @ (rw[:, None] * J)) * S[None, :]
    A[:n, :n] += smooth * dense["R"] + damp * np.eye(n)
    if scaled:
        A[n:, n:] += np.diag(sdamp.ravel())
    cond = np.linalg.cond(A)
    assert cond * np.finfo(np.float64).eps < 0.01 * rtol, cond
    b_s, b_e = rng.standard_normal(n), rng.standard_normal((2, 4))
    x_s, x_e, info = JR.cg(_product(dense, rw, scale), b_s, b_e, np.float64, smooth_op=lambda p: NR.smooth(p, NN, CG_DX), smooth=smooth,
                           damp=damp, source_damp=sdamp, source_scale=scale, maxiter=n + 8, rtol=rtol)
    b = np.concatenate([b_s, S[n:] * b_e.ravel()])
    z = np.concatenate([x_s, x_e.ravel() / S[n:]])
    true = np.linalg.norm(b - A @ z) / np.linalg.norm(b)
    print("joint cg (%s): cond %.3e, %d iterations, recurrence residual %.3e, true residual %.3e"
          % ("scaled" if scaled else "plain", cond, info["iterations"], math.sqrt(info["rho"][-1] / info["rho"][0]), true))
    assert info["status"] == 0 and 1 <= info["iterations"] < n + 8
    assert len(info["rho"]) == info["iterations"] + 2 and len(info["pq"]) == info["iterations"]
    assert info["rho"][-1] <= rtol * rtol * info["rho"][0] < info["rho"][-2]
    assert true <= 2 * rtol
    assert np.any(x_e != 0)


def test_all_zero_scale_is_solve_normal(dense):
    n, J, rng = dense["n"], dense["J"], np.random.default_rng(29)
    rw = rng.uniform(0.5, 2.0, 20)
    smooth, damp = 1e-3, 1e-1
    b_s, b_e = rng.standard_normal(n), rng.standard_normal((2, 4))
    H = J[:, :n].T @ (rw[:, None] * J[:, :n])
    kw = dict(smooth_op=lambda p: NR.smooth(p, NN, CG_DX), smooth=smooth, damp=damp, maxiter=6, rtol=1e-6)
    x_ref, info_ref = NR.cg(lambda p: H @ p, b_s, np.float64, **kw)
    # the joint product with the source columns scaled to zero: the slowness block of the dense product, formed from the same H
    def product(ps, pe):
        assert not np.any(JR.scale_block(np.zeros(4), pe, np.float64))
        return H @ ps, JR.scale_block(np.zeros(4), J[:, n:].T @ (rw * (J[:, :n] @ ps)), np.float64)
    for sdamp in (None, np.tile(SDAMP, (2, 1))):
        x_s, x_e, info = JR.cg(product, b_s, b_e, np.float64, source_damp=sdamp, source_scale=np.zeros(4), **kw)
        assert not np.any(x_e) and x_e.shape == (2, 4)
        assert np.array_equal(x_s, x_ref)
        assert info["rho"] == info_ref["rho"] and info["pq"] == info_ref["pq"] and info["iterations"] == info_ref["iterations"] == 6


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
    t.n_points, t.n_rows, t.n_events, t.n_nodes = 3, 7, 2, 60
    t._rows = np.arange(7)
    yield t
    t._h = C.c_void_p()


def test_python_argument_errors(fake_tape):
    t = fake_tape
    v, e, rw = np.zeros(60, dtype=np.float32), np.zeros((3, 4), dtype=np.float32), np.ones(7, dtype=np.float32)
    bad = [
        (dict(smooth=-1.0), "smooth"), (dict(smooth=float("nan")), "smooth"), (dict(damp=-1e-3), "damp"), (dict(damp=float("inf")), "damp"),
        (dict(maxiter=0), "maxiter"), (dict(maxiter=2.5), "maxiter"), (dict(rtol=-1e-6), "rtol"), (dict(rtol=float("nan")), "rtol"),
        (dict(hessian="newton"), "hessian"), (dict(schedule="fast"), "schedule"),
        (dict(smooth_weights=(1.0, 1.0)), "smooth_weights"), (dict(smooth_weights=(1.0, -1.0, 1.0)), "smooth_weights"),
        (dict(row_weight=np.ones(6)), "row_weight"), (dict(row_weight=np.ones((7, 1))), "row_weight"),
        (dict(source_damp=-1.0), "source_damp"), (dict(source_damp=float("nan")), "source_damp"), (dict(source_damp=np.ones(3)), "source_damp"),
        (dict(source_damp=np.ones((2, 4))), "source_damp"), (dict(source_damp=None), "source_damp"),
        (dict(source_scale=(1.0, 1.0, -1.0, 1.0)), "source_scale"), (dict(source_scale=(1.0, 1.0, float("inf"), 1.0)), "source_scale"),
        (dict(source_scale=2.0), "source_scale"), (dict(source_scale=np.ones((3, 3))), "source_scale"),
    ]
    for kw, name in bad:
        with pytest.raises(ValueError, match=name):
            t.solve_joint(v, e, **{"row_weight": rw, **kw})
    with pytest.raises(ValueError, match="rhs should hold 60"):
        t.solve_joint(np.zeros(61, dtype=np.float32), e)
    for wrong in (np.zeros((4, 3)), np.zeros(12), np.zeros((2, 4))):
        with pytest.raises(ValueError, match="rhs_src"):
            t.solve_joint(v, wrong)
        with pytest.raises(ValueError, match="v_src"):
            t.gauss_newton_joint(v, wrong)
        with pytest.raises(ValueError, match="dsrc"):
            t.jvp_joint(v, wrong)
    with pytest.raises(ValueError, match="v should hold 60"):
        t.gauss_newton_joint(np.zeros(59), e)
    with pytest.raises(ValueError, match="row_weight"):
        t.gauss_newton_joint(v, e, row_weight=np.ones(8))
    with pytest.raises(ValueError, match="source_scale"):
        t.gauss_newton_joint(v, e, source_scale=(1.0, -2.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="source_scale"):
        t.gauss_newton_joint(v, e, source_scale=np.ones((4, 4)))
    with pytest.raises(ValueError, match="schedule"):
        t.gauss_newton_joint(v, e, schedule="fast")
    with pytest.raises(ValueError, match="ds should hold 60"):
        t.jvp_joint(np.zeros(61), e)
    with pytest.raises(ValueError, match="schedule"):
        t.jvp_joint(v, e, schedule=0)
    for good in (lambda: t.solve_joint(v, e, row_weight=rw, smooth=1.0, damp=1.0, source_damp=(1.0, 2.0, 2.0, 2.0), source_scale=np.ones((3, 4))),
                 lambda: t.gauss_newton_joint(v, e, rw, source_scale=(1.0, 0.0, 0.1, 0.1)), lambda: t.jvp_joint(v, e)):
        with pytest.raises(AssertionError, match="reached the library"):   # (and a good call does get there)
            good()


def _err(lib, status, *words):
    from ttcr_amd import _lib

    assert status == _lib.ERR_VALUE, status
    msg = _lib.last_error()
    assert msg and all(w in msg for w in words), msg


def test_c_argument_errors_come_before_the_device(lib):
    from ttcr_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ttcr_amd.h")).read()
    pxd = open(os.path.join(ROOT, "integration", "ttcr_amd.pxd")).read()
    for name in JOINT_SYMBOLS:
        assert name + "(" in hdr and name + "(" in pxd and name in _lib.SYMBOLS and getattr(lib, name) is not None, name
    a = np.zeros(8, dtype=np.float32)
    p = a.ctypes.data_as(C.c_void_p)
    w3 = (C.c_double * 3)(1.0, 1.0, 1.0)
    neg = (C.c_double * 3)(1.0, -1.0, 1.0)
    st, it = C.c_int(-7), C.c_int(-7)
    rho, pq = (C.c_double * 8)(), (C.c_double * 8)()

    def solve(**kw):
        v = dict(t=None, rhs=p, rs=p, rw=None, smooth=1.0, w=w3, damp=1.0, sd=None, sc=None, maxiter=3, rtol=1e-6, schedule=0, x=p, xs=p,
                 st=C.byref(st), it=C.byref(it), rho=rho, pq=pq)
        v.update(kw)
        return lib.ttcr_fsm_joint_solve(v["t"], v["rhs"], 0, v["rs"], 0, v["rw"], 0, v["smooth"], v["w"], v["damp"], v["sd"], v["sc"],
                                        v["maxiter"], v["rtol"], v["schedule"], v["x"], 0, v["xs"], 0, v["st"], v["it"], v["rho"], v["pq"], None)

    _err(lib, solve(smooth=-1.0), "smooth")
    _err(lib, solve(smooth=float("nan")), "smooth")
    _err(lib, solve(damp=-0.5), "damp")
    _err(lib, solve(maxiter=0), "maxiter")
    _err(lib, solve(rtol=-1.0), "rtol")
    _err(lib, solve(w=None), "null smooth_weights")
    _err(lib, solve(w=neg), "smooth_weights")
    _err(lib, solve(schedule=2), "schedule")
    _err(lib, solve(rhs=None), "null rhs")
    _err(lib, solve(rs=None), "null rhs_src")
    _err(lib, solve(x=None), "null x")
    _err(lib, solve(xs=None), "null x_src")
    _err(lib, solve(st=None), "null status")
    _err(lib, solve(), "null tape")
    jvp, gn = lib.ttcr_fsm_joint_jvp, lib.ttcr_fsm_joint_gn
    fake = C.c_void_p(1234)   # never dereferenced: the argument checks come first
    _err(lib, jvp(fake, None, 0, p, 0, p, 0, None, 0, 0, None), "null ds")
    _err(lib, jvp(fake, p, 0, None, 0, p, 0, None, 0, 0, None), "null dsrc")
    _err(lib, jvp(None, p, 0, p, 0, p, 0, None, 0, 0, None), "null tape")
    _err(lib, jvp(fake, p, 0, p, 0, None, 0, None, 0, 0, None), "both")
    _err(lib, jvp(fake, p, 0, p, 0, p, 0, None, 0, 2, None), "schedule")
    _err(lib, gn(fake, None, 0, p, 0, None, 0, None, p, 0, p, 0, 0, None, None), "null v")
    _err(lib, gn(fake, p, 0, None, 0, None, 0, None, p, 0, p, 0, 0, None, None), "null v_src")
    _err(lib, gn(fake, p, 0, p, 0, None, 0, None, None, 0, p, 0, 0, None, None), "null out")
    _err(lib, gn(fake, p, 0, p, 0, None, 0, None, p, 0, None, 0, 0, None, None), "null out_src")
    _err(lib, gn(None, p, 0, p, 0, None, 0, None, p, 0, p, 0, 0, None, None), "null tape")
    _err(lib, lib.ttcr_fsm_joint_release(None), "null tape")
    assert st.value == -7 and it.value == -7 and not np.any(a)   # (no call got as far as its outputs)


def test_python_layer_has_the_methods_without_torch():
    code = ("import sys, ttcr_amd; from ttcr_amd.rgrid import FieldTape; from ttcr_amd.inversion import joint_gauss_newton_step; "
            "assert all(callable(getattr(FieldTape, a, None)) for a in ('jvp_joint', 'gauss_newton_joint', 'solve_joint', 'release_joint')); "
            "assert 'torch' not in sys.modules")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)
