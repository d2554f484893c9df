"""The receiver-point derivatives and the receiver joint system of the field tape without a device: the numpy restatement
of tests/receiver_reference.py -- what the device is compared with bit for bit in tests/test_receiver_derivative_gpu.py -- against central
finite differences of the oracle's interpolated receiver traveltimes in the receiver position, the receiver joint tangent against a
finite difference along a joint direction, forward against reverse, the recurrence on a dense system, the all-zero scale against
solve_normal's restatement, the receiver-point map, and every argument error of the Python layer and of the C entries before any device
call."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import adjoint_reference as AR  # noqa: E402
import normal_reference as NR  # noqa: E402
import receiver_reference as RR  # noqa: E402
import tangent_reference as TR  # noqa: E402
from test_tangent import DOT_TOL, DX, MN, N, NN3, STEP, TOL, model, solve  # noqa: E402  (grid, model, step and bounds of 6c / 6d)

RCV_SYMBOLS = ["ttcr_fsm_rcv_eval", "ttcr_fsm_rcv_points", "ttcr_fsm_rcv_jvp", "ttcr_fsm_rcv_vjp",
               "ttcr_fsm_rjoint_jvp", "ttcr_fsm_rjoint_gn", "ttcr_fsm_rjoint_solve", "ttcr_fsm_rcv_release"]
SRC = np.array([[3.3, 4.1, 5.7]])
SRC_OF = {"smooth": SRC, "rough": np.array([[6.2, 2.9, 4.4]])}   # (the sources of test_tangent's cases for the two models)
HI = (N - 1) * DX
# receivers of the finite-difference test and the axes each lies on a grid plane of (those get no step: the code's value does not depend
# on them there).  No receiver lies within 0.02 dx of a face other than the planes it is on.
FD_RCV = [
    ([6.23, 2.91, 4.38], ()),                          # generic interior
    ([1.12, 8.77, 7.31], ()),
    ([HI - 0.21, HI - 0.13, HI - 0.34], ()),           # the last cell of the far corner
    ([4.0, 2.63, 7.19], (0,)),                         # on one plane, each axis in turn
    ([3.37, 6.5, 1.88], (1,)),
    ([8.14, 5.29, 2.0], (2,)),
    ([4.5, 7.0, 3.27], (0, 1)),                        # on two planes
    ([2.0, 6.81, 9.0], (0, 2)),
    ([5.61, 1.5, 8.5], (1, 2)),
    ([7.0, 3.5, 6.0], (0, 1, 2)),                      # on a node
    ([HI, 4.33, HI], (0, 2)),                          # on the far faces
]


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_fd_receivers_keep_their_distance_from_the_faces():
    for p, on in FD_RCV:
        for a in range(3):
            off = (p[a] / DX) % 1.0
            dist = min(off, 1.0 - off) * DX
            if a in on:
                assert dist < 1e-12, (p, a)
            else:
                assert dist > 0.02 * DX, (p, a, dist)


# ---- 1. the restatement against central finite differences of the oracle in the receiver position
@pytest.mark.parametrize("kind", ["smooth", "rough"])
def test_restatement_is_the_derivative_of_the_oracle_in_the_receiver_position(kind):
    s = model(kind)
    rcv = np.array([p for p, _ in FD_RCV])
    rng = np.random.default_rng(41)
    d = rng.standard_normal(rcv.shape)
    for i, (_, on) in enumerate(FD_RCV):
        d[i, list(on)] = 0.0
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)
    o = solve(s, SRC_OF[kind], rcv)
    tt, G = RR.evaluate_points([o["tt"]], NN3, DX, MN, rcv, np.zeros(len(rcv), dtype=int))
    assert np.array_equal(tt, o["tt_rcv"])          # the restated interpolation has the oracle's bits
    for i, (_, on) in enumerate(FD_RCV):
        for a in range(3):
            if a in on:
                assert G[i, a] == 0 and not np.signbit(G[i, a]), (i, a)   # exactly +0 on the axes of its planes
            else:
                assert G[i, a] != 0, (i, a)
    op, om = solve(s, SRC_OF[kind], rcv + STEP * d), solve(s, SRC_OF[kind], rcv - STEP * d)
    assert np.array_equal(op["tt"], o["tt"]) and np.array_equal(om["tt"], o["tt"])   # (the field does not see the receivers)
    fd = (op["tt_rcv"] - om["tt_rcv"]) / (2 * STEP)
    mine = np.einsum("ra,ra->r", G, d)
    off_node = [i for i, (_, on) in enumerate(FD_RCV) if len(on) < 3]
    assert fd[9] == 0 and mine[9] == 0              # the point on a node: no free axis
    err = _rel(mine[off_node], fd[off_node])
    worst = max(abs(mine[i] - fd[i]) / abs(fd[i]) for i in off_node)
    print("receiver gradient vs oracle finite differences, %s: relative L2 %.2e, worst row %.2e (bound %.0e)" % (kind, err, worst, TOL))
    assert err <= TOL, err


# ---- 2. the receiver joint tangent along one joint direction
def _joint_setup(dt=np.float64):
    rng = np.random.default_rng(43)
    s = model("smooth")
    rcv = rng.uniform(0.6, HI - 0.6, (12, 3))
    off = (rcv / DX) % 1.0
    rcv = np.where(np.minimum(off, 1 - off) < 0.05, rcv + 0.1 * DX, rcv)
    por = np.arange(12)
    ds = s * rng.standard_normal(s.size)
    drcv = rng.standard_normal((12, 4))
    w = rng.standard_normal(12)
    return s, rcv, por, ds, drcv, w


def test_receiver_joint_tangent_is_the_directional_derivative_of_the_oracle():
    s, rcv, por, ds, drcv, w = _joint_setup()
    o = solve(s, SRC, rcv)
    _, G = RR.evaluate_points([o["tt"]], NN3, DX, MN, rcv, np.zeros(12, dtype=int))
    _, dtts = TR.tangent([o["tt"]], s, DX, NN3, MN, [SRC], ds, rcvs=[rcv])
    dtt = RR.joint_tangent(dtts[0], G, por, drcv)
    for sign in (1, -1):   # no receiver moves across a cell face
        assert np.array_equal(np.floor((rcv + sign * STEP * drcv[:, 1:]) / DX), np.floor(rcv / DX))
    op = solve(s + STEP * ds, SRC, rcv + STEP * drcv[:, 1:])
    om = solve(s - STEP * ds, SRC, rcv - STEP * drcv[:, 1:])
    fd = (op["tt_rcv"] - om["tt_rcv"]) / (2 * STEP) + drcv[:, 0]   # (t0 of a receiver point adds to its rows)
    err = _rel(dtt, fd)
    print("receiver joint tangent vs oracle finite differences: %.2e (bound %.0e)" % (err, TOL))
    assert err <= TOL, err
    assert np.array_equal(RR.joint_tangent(dtts[0], G, por, np.zeros_like(drcv)), dtts[0])
    assert np.array_equal(RR.joint_tangent(np.zeros(12), G, por, drcv), RR.forward(G, por, drcv))


# ---- 3. forward against reverse
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_dot_product_identities(dt):
    s, rcv, _, ds, _, w = _joint_setup()
    rng = np.random.default_rng(47)
    o = solve(s.astype(dt), SRC.astype(dt), rcv.astype(dt), dt)
    por = np.array([0, 1, 2, 3, 0, 1, 2, 3, 4, 4, 6, 6])   # shared points (their G differ: the identity does not care), point 5 empty
    n_points = 8
    drcv = rng.standard_normal((n_points, 4)).astype(dt)
    s, ds, w = s.astype(dt), ds.astype(dt), w.astype(dt)
    _, G = RR.evaluate_points([o["tt"]], NN3, DX, MN, rcv.astype(dt), np.zeros(12, dtype=int))
    assert G.dtype == dt
    f8 = lambda a: np.asarray(a, dtype=np.float64).ravel()   # noqa: E731
    fwd, rev = RR.forward(G, por, drcv), RR.reverse(G, por, n_points, w)
    assert fwd.dtype == dt and rev.dtype == dt and not np.any(rev[5]) and not np.any(rev[7]) and not np.any(np.signbit(rev[5]))
    lhs, rhs = f8(w) @ f8(fwd), f8(rev) @ f8(drcv)
    e_rcv = abs(lhs - rhs) / abs(rhs)
    _, dtts = TR.tangent([o["tt"]], s, DX, NN3, MN, [SRC], ds, rcvs=[rcv.astype(dt)])
    g = AR.adjoint([o["tt"]], s, DX, NN3, MN, [SRC], rcvs=[rcv.astype(dt)], ws=[w])
    lhs = f8(w) @ f8(RR.joint_tangent(dtts[0], G, por, drcv))
    rhs = f8(g) @ f8(ds) + f8(rev) @ f8(drcv)
    e_joint = abs(lhs - rhs) / abs(rhs)
    print("<w, dtt_rcv> against <grcv, drcv>, %s: %.2e; the joint identity: %.2e (bound %.0e)"
          % (np.dtype(dt).name, e_rcv, e_joint, DOT_TOL[dt]))
    assert e_rcv <= DOT_TOL[dt] and e_joint <= DOT_TOL[dt], (e_rcv, e_joint)


# ---- 4. the restated recurrence on a dense receiver joint system
NN = (6, 5, 7)
CG_DX = 0.5
SCALE = np.array([1.0, 0.05, 0.05, 0.05])
RDAMP = np.array([1e-2, 1e-1, 1e-1, 1e-1])
POR = np.array([0, 1, 2, 0, 1, 2])   # the reciprocal layout: both events see the three receiver points


@pytest.fixture(scope="module")
def dense():
    """[J_s J_rcv] of two events and three receiver points on the 6 x 5 x 7 node grid (fp64, fields from the oracle), R from compute_K"""
    from oracle import oracle as O
    from ttcr_amd import inversion

    n = int(np.prod(NN))
    X, Y, Z = np.meshgrid(*[np.arange(k) * CG_DX for k in NN], indexing="ij")
    s = (0.5 + 0.02 * X + 0.015 * Y + 0.03 * Z + 0.05 * np.sin(0.9 * X) * np.cos(0.7 * Y + 0.3 * Z)).flatten("F")
    srcs = [np.array([[0.7, 0.9, 1.1]]), np.array([[1.9, 1.3, 2.6]])]
    pts = np.array([[1.63, 0.41, 2.37], [0.38, 1.71, 0.62], [2.21, 1.12, 1.34]])
    fields = []
    for src in srcs:
        o = O.solve3d(np.float64, tuple(k - 1 for k in NN), CG_DX, (0.0, 0.0, 0.0), s, src, rcv=pts, eps=1e-15, maxit=200)
        assert o["niter"] < 200 and o["change"][-1] == 0
        fields.append(o["tt"])
    rcv_rows = np.concatenate([pts, pts])
    _, G = RR.evaluate_points(fields, NN, CG_DX, (0.0, 0.0, 0.0), rcv_rows, [0, 0, 0, 1, 1, 1])
    J = np.zeros((6, n + 12))
    for r in range(6):   # a row of J_s is the adjoint of the row's unit cotangent
        e, k = divmod(r, 3)
        unit = np.zeros(3)
        unit[k] = 1.0
        J[r, :n] = AR.adjoint([fields[e]], s, CG_DX, NN, (0.0, 0.0, 0.0), [srcs[e]], rcvs=[pts], ws=[unit])
    for j in range(12):
        unit = np.zeros(12)
        unit[j] = 1.0
        J[:, n + j] = RR.forward(G, POR, unit.reshape(3, 4))
    K = inversion.smoothing_matrices(NN, (CG_DX,) * 3, order=2)
    perm = np.arange(n).reshape(NN[2], NN[1], NN[0]).transpose(2, 1, 0).ravel()   # perm[k] = the tape index of compute_K's parameter k
    Rk = sum((Kd.T @ Kd).toarray() for Kd in K)
    R = np.zeros((n, n))
    R[np.ix_(perm, perm)] = Rk
    return dict(J=J, R=R, n=n, G=G)


def _product(dense, rw, scale):
    J, n, G = dense["J"], dense["n"], dense["G"]
    return lambda p, pe: RR.joint_product(lambda v: J[:, :n] @ v, lambda w: J[:, :n].T @ w, G, POR, 3, p, pe, row_weight=rw, rcv_scale=scale)


def test_dense_product_is_the_dense_matrix(dense):
    J, n, rng = dense["J"], dense["n"], np.random.default_rng(31)
    rw, v, ve = rng.uniform(0.5, 2.0, 6), rng.standard_normal(n), rng.standard_normal((3, 4))
    g, ge = _product(dense, rw, None)(v, ve)
    ref = J.T @ (rw * (J @ np.concatenate([v, ve.ravel()])))
    assert _rel(np.concatenate([g, ge.ravel()]), ref) < 1e-13


@pytest.mark.parametrize("scaled", [True, False], ids=["scale_and_damp", "plain"])
def test_restated_receiver_joint_cg_on_a_dense_system(dense, scaled):
    """Six rows see twelve receiver parameters, so without rcv_damp the receiver block of A is singular; the right-hand side is a
    Gauss-Newton gradient J^T W res as reciprocal_gauss_newton_step forms it, which lies in the range of A, and conjugate gradients from
    zero converge on it all the same."""
    n, J, rng = dense["n"], dense["J"], np.random.default_rng(23)
    rtol = 1e-6
    rw = rng.uniform(0.5, 2.0, 6)
    smooth, damp = 1e-3, 1e-1
    scale = np.tile(SCALE, (3, 1)) if scaled else None
    rdamp = np.tile(RDAMP, (3, 1)) if scaled else None
    S = np.concatenate([np.ones(n), scale.ravel() if scaled else np.ones(12)])
    A = S[:, None] * (J.T @ (rw[:, None] * J)) * S[None, :]
    A[:n, :n] += smooth * dense["R"] + damp * np.eye(n)
    if scaled:
        A[n:, n:] += np.diag(rdamp.ravel())
        cond = np.linalg.cond(A)
        assert cond * np.finfo(np.float64).eps < 0.01 * rtol, cond
    grad = J.T @ (rw * rng.standard_normal(6))
    b_s, b_e = grad[:n], grad[n:].reshape(3, 4)
    x_s, x_e, info = RR.cg(_product(dense, rw, scale), b_s, b_e, np.float64, smooth_op=lambda p: NR.smooth(p, NN, CG_DX), smooth=smooth,
                           damp=damp, rcv_damp=rdamp, rcv_scale=scale, maxiter=n + 12, rtol=rtol)
    b = np.concatenate([b_s, S[n:] * b_e.ravel()])
    z = np.concatenate([x_s, x_e.ravel() / S[n:]])
    true = np.linalg.norm(b - A @ z) / np.linalg.norm(b)
    print("receiver joint cg (%s): %d iterations, recurrence residual %.3e, true residual %.3e"
          % ("scaled" if scaled else "plain", info["iterations"], math.sqrt(info["rho"][-1] / info["rho"][0]), true))
    assert info["status"] == 0 and 1 <= info["iterations"] < n + 12
    assert len(info["rho"]) == info["iterations"] + 2 and len(info["pq"]) == info["iterations"]
    assert info["rho"][-1] <= rtol * rtol * info["rho"][0] < info["rho"][-2]
    assert true <= 2 * rtol
    assert np.any(x_e != 0)


def test_all_zero_scale_is_solve_normal(dense):
    n, J, rng = dense["n"], dense["J"], np.random.default_rng(29)
    rw = rng.uniform(0.5, 2.0, 6)
    smooth, damp = 1e-3, 1e-1
    b_s, b_e = rng.standard_normal(n), rng.standard_normal((3, 4))
    Js = J[:, :n]
    kw = dict(smooth_op=lambda p: NR.smooth(p, NN, CG_DX), smooth=smooth, damp=damp, maxiter=6, rtol=1e-6)
    x_ref, info_ref = NR.cg(lambda p: Js.T @ (rw * (Js @ p)), b_s, np.float64, **kw)
    for rdamp in (None, np.tile(RDAMP, (3, 1))):
        x_s, x_e, info = RR.cg(_product(dense, rw, np.zeros(4)), b_s, b_e, np.float64, rcv_damp=rdamp, rcv_scale=np.zeros(4), **kw)
        assert not np.any(x_e) and x_e.shape == (3, 4)
        assert np.array_equal(x_s, x_ref)
        assert info["rho"] == info_ref["rho"] and info["pq"] == info_ref["pq"] and info["iterations"] == info_ref["iterations"] == 6


# ---- 5. receiver points
def test_receiver_points_restated():
    rcv = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]], dtype=np.float32)
    assert RR.check_points(rcv, [0, 1, 0, 1, 2]) == 3                 # points shared across events
    assert RR.check_points(rcv, [0, 1, 0, 1, 3], n_points=6) == 6     # points without rows
    with pytest.raises(ValueError, match="rows 1 and 2"):
        RR.check_points(rcv, [0, 1, 1, 0, 2])
    with pytest.raises(ValueError, match="rows 0 and 2"):             # -0 and +0 are different points
        RR.check_points(np.array([[0.0, 1, 1], [2, 2, 2], [-0.0, 1, 1]], dtype=np.float32), [0, 1, 0])
    with pytest.raises(ValueError):
        RR.check_points(rcv, [0, 1, 0, 1, 2], n_points=2)
    G = np.arange(15, dtype=np.float32).reshape(5, 3)
    g = RR.reverse(G, [0, 1, 0, 1, 3], 5, np.ones(5, dtype=np.float32))
    assert np.array_equal(g[0], [2, 0 + 6, 1 + 7, 2 + 8]) and not np.any(g[2]) and not np.any(g[4]) and not np.any(np.signbit(g))


# ---- 6. argument errors, before anything is launched
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
    t.n_points, t.n_rows, t.n_events, t.n_nodes = 2, 7, 2, 60
    t.n_rcv_points = 3
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
        (dict(rcv_damp=-1.0), "rcv_damp"), (dict(rcv_damp=float("nan")), "rcv_damp"), (dict(rcv_damp=np.ones(3)), "rcv_damp"),
        (dict(rcv_damp=np.ones((2, 4))), "rcv_damp"), (dict(rcv_damp=None), "rcv_damp"),
        (dict(rcv_scale=(1.0, 1.0, -1.0, 1.0)), "rcv_scale"), (dict(rcv_scale=(1.0, 1.0, float("inf"), 1.0)), "rcv_scale"),
        (dict(rcv_scale=2.0), "rcv_scale"), (dict(rcv_scale=np.ones((3, 3))), "rcv_scale"),
    ]
    for kw, name in bad:
        with pytest.raises(ValueError, match=name):
            t.solve_receiver_joint(v, e, **{"row_weight": rw, **kw})
    with pytest.raises(ValueError, match="rhs should hold 60"):
        t.solve_receiver_joint(np.zeros(61, dtype=np.float32), e)
    for wrong in (np.zeros((4, 3)), np.zeros(12), np.zeros((2, 4))):
        with pytest.raises(ValueError, match="rhs_rcv"):
            t.solve_receiver_joint(v, wrong)
        with pytest.raises(ValueError, match="v_rcv"):
            t.gauss_newton_receiver_joint(v, wrong)
        with pytest.raises(ValueError, match="drcv"):
            t.jvp_joint_receiver(v, wrong)
        with pytest.raises(ValueError, match="drcv.*receiver point"):
            t.jvp_receiver(wrong)
    with pytest.raises(ValueError, match="v should hold 60"):
        t.gauss_newton_receiver_joint(np.zeros(59), e)
    with pytest.raises(ValueError, match="row_weight"):
        t.gauss_newton_receiver_joint(v, e, row_weight=np.ones(8))
    with pytest.raises(ValueError, match="rcv_scale"):
        t.gauss_newton_receiver_joint(v, e, rcv_scale=(1.0, -2.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="rcv_scale"):
        t.gauss_newton_receiver_joint(v, e, rcv_scale=np.ones((4, 4)))
    with pytest.raises(ValueError, match="schedule"):
        t.gauss_newton_receiver_joint(v, e, schedule="fast")
    with pytest.raises(ValueError, match="ds should hold 60"):
        t.jvp_joint_receiver(np.zeros(61), e)
    with pytest.raises(ValueError, match="schedule"):
        t.jvp_joint_receiver(v, e, schedule=0)
    # receiver_eval: shapes, integer events, their range
    pts = np.zeros((5, 3), dtype=np.float32)
    for wrong in (np.zeros((5, 2)), np.zeros(15), np.zeros((1, 5, 3))):
        with pytest.raises(ValueError, match="pts"):
            t.receiver_eval(wrong, np.zeros(5, dtype=int))
    for wrong in (np.zeros(4, dtype=int), np.zeros((5, 1), dtype=int), np.zeros(5), [0, 0, 0, 0, 2], [0, -1, 0, 0, 0]):
        with pytest.raises(ValueError, match="event_of_pt"):
            t.receiver_eval(pts, wrong)
    # set_receiver_points: one integer per data row, >= 0, n_points above the largest index
    for wrong in (np.zeros(6, dtype=int), np.zeros((7, 1), dtype=int), np.zeros(7), [0, 1, 2, 3, 4, 5, -1]):
        with pytest.raises(ValueError, match="point_of_row"):
            t.set_receiver_points(wrong)
    for wrong in (2, 2.5, -1):
        with pytest.raises(ValueError, match="n_points"):
            t.set_receiver_points([0, 1, 2, 0, 1, 2, 0], n_points=wrong)
    # vjp with the receiver gradient: the checks of vjp
    with pytest.raises(ValueError, match="nothing to back-propagate"):
        t.vjp(return_receiver_grad=True)
    with pytest.raises(ValueError, match="w should hold 7"):
        t.vjp(np.ones(6), return_receiver_grad=True)
    good = [lambda: t.solve_receiver_joint(v, e, row_weight=rw, smooth=1.0, damp=1.0, rcv_damp=(1.0, 2.0, 2.0, 2.0), rcv_scale=np.ones((3, 4))),
            lambda: t.gauss_newton_receiver_joint(v, e, rw, rcv_scale=(1.0, 0.0, 0.1, 0.1)), lambda: t.jvp_joint_receiver(v, e),
            lambda: t.jvp_receiver(e), lambda: t.receiver_eval(pts, [0, 1, 0, 1, 1]), lambda: t.receiver_jacobian(),
            lambda: t.set_receiver_points([0, 1, 2, 0, 1, 2, 0], n_points=5), lambda: t.release_receiver(),
            lambda: t.vjp(rw, return_receiver_grad=True)]
    for call in good:
        with pytest.raises(AssertionError, match="reached the library"):   # (and a good call does get there)
            call()


def _err(lib, status, *words):
    from ttcr_amd import _lib

    assert status == _lib.ERR_VALUE, status
    msg = _lib.last_error()
    assert msg and all(w in msg for w in words), msg


def test_c_argument_errors_come_before_the_device(lib):
    from ttcr_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ttcr_amd.h")).read()
    pxd = open(os.path.join(ROOT, "integration", "ttcr_amd.pxd")).read()
    for name in RCV_SYMBOLS:
        assert name + "(" in hdr and name + "(" in pxd and name in _lib.SYMBOLS and getattr(lib, name) is not None, name
    a = np.zeros(8, dtype=np.float32)
    p = a.ctypes.data_as(C.c_void_p)
    ev = (C.c_int * 2)(0, 0)
    w3 = (C.c_double * 3)(1.0, 1.0, 1.0)
    neg = (C.c_double * 3)(1.0, -1.0, 1.0)
    st, it = C.c_int(-7), C.c_int(-7)
    rho, pq = (C.c_double * 8)(), (C.c_double * 8)()

    def solve(**kw):
        v = dict(t=None, rhs=p, rs=p, rw=None, smooth=1.0, w=w3, damp=1.0, sd=None, sc=None, maxiter=3, rtol=1e-6, schedule=0, x=p, xs=p,
                 st=C.byref(st), it=C.byref(it), rho=rho, pq=pq)
        v.update(kw)
        return lib.ttcr_fsm_rjoint_solve(v["t"], v["rhs"], 0, v["rs"], 0, v["rw"], 0, v["smooth"], v["w"], v["damp"], v["sd"], v["sc"],
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
    _err(lib, solve(rs=None), "null rhs_rcv")
    _err(lib, solve(x=None), "null x")
    _err(lib, solve(xs=None), "null x_rcv")
    _err(lib, solve(st=None), "null status")
    _err(lib, solve(), "null tape")
    fake = C.c_void_p(1234)   # never dereferenced: the argument checks come first
    jvp, gn = lib.ttcr_fsm_rjoint_jvp, lib.ttcr_fsm_rjoint_gn
    _err(lib, jvp(fake, None, 0, p, 0, p, 0, None, 0, 0, None), "null ds")
    _err(lib, jvp(fake, p, 0, None, 0, p, 0, None, 0, 0, None), "null drcv")
    _err(lib, jvp(None, p, 0, p, 0, p, 0, None, 0, 0, None), "null tape")
    _err(lib, jvp(fake, p, 0, p, 0, None, 0, None, 0, 0, None), "both")
    _err(lib, jvp(fake, p, 0, p, 0, p, 0, None, 0, 2, None), "schedule")
    _err(lib, gn(fake, None, 0, p, 0, None, 0, None, p, 0, p, 0, 0, None, None), "null v")
    _err(lib, gn(fake, p, 0, None, 0, None, 0, None, p, 0, p, 0, 0, None, None), "null v_rcv")
    _err(lib, gn(fake, p, 0, p, 0, None, 0, None, None, 0, p, 0, 0, None, None), "null out")
    _err(lib, gn(fake, p, 0, p, 0, None, 0, None, p, 0, None, 0, 0, None, None), "null out_rcv")
    _err(lib, gn(None, p, 0, p, 0, None, 0, None, p, 0, p, 0, 0, None, None), "null tape")
    _err(lib, gn(fake, p, 0, p, 0, None, 0, None, p, 0, p, 0, 3, None, None), "schedule")
    ev_ = lib.ttcr_fsm_rcv_eval
    _err(lib, ev_(fake, 2, p, 0, ev, None, 0, None, 0), "both null")
    _err(lib, ev_(fake, 2, p, 0, None, p, 0, None, 0), "null event_of_pt")
    _err(lib, ev_(None, 2, p, 0, ev, p, 0, p, 0), "null tape")
    _err(lib, ev_(None, 0, None, 0, None, None, 0, p, 0), "null tape")
    _err(lib, lib.ttcr_fsm_rcv_points(None, None, 0, None, None, None), "null tape")
    _err(lib, lib.ttcr_fsm_rcv_jvp(fake, None, 0, p, 0), "null drcv")
    _err(lib, lib.ttcr_fsm_rcv_jvp(fake, p, 0, None, 0), "null dtt")
    _err(lib, lib.ttcr_fsm_rcv_jvp(None, p, 0, p, 0), "null tape")
    _err(lib, lib.ttcr_fsm_rcv_vjp(fake, None, 0, p, 0), "null w")
    _err(lib, lib.ttcr_fsm_rcv_vjp(fake, p, 0, None, 0), "null grcv")
    _err(lib, lib.ttcr_fsm_rcv_vjp(None, p, 0, p, 0), "null tape")
    _err(lib, lib.ttcr_fsm_rcv_release(None), "null tape")
    assert st.value == -7 and it.value == -7 and not np.any(a)   # (no call got as far as its outputs)
