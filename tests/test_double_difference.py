"""The double-difference rows of the field tape without a device: the numpy restatement of tests/dd_reference.py -- what the
device is compared with bit for bit in tests/test_double_difference_gpu.py -- against a dense diag(rw) + Q^T diag(pw) Q, its three
consequences (empty pair list, constant rows, symmetry), the three restated CG systems with pairs on 6k's dense case, every argument
error of the Python layer and of the C entries before any device call, the symbols, and double_difference_step on a stand-in tape."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import adjoint_reference as AR  # noqa: E402,F401
import dd_reference as DD  # noqa: E402
import joint_reference as JR  # noqa: E402
import normal_reference as NR  # noqa: E402
import receiver_reference as RR  # noqa: E402
from test_receiver_derivative import CG_DX, NN, POR, RDAMP, SCALE, dense  # noqa: E402,F401  (6k's dense case and its settings)

DD_SYMBOLS = ["ttcr_fsm_dd_pairs", "ttcr_fsm_dd_apply", "ttcr_fsm_dd_gn", "ttcr_fsm_dd_solve", "ttcr_fsm_dd_release"]
DTYPES = pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def random_pairs(rng, n_rows=40, n_pairs=300):
    """300 pairs on 40 rows with duplicates, rows 7, 19 and 33 in no pair, and a fifth of the weights zero"""
    used = np.array([r for r in range(n_rows) if r not in (7, 19, 33)])
    a = rng.choice(used, n_pairs)
    b = rng.choice(used, n_pairs)
    b = np.where(a == b, used[(np.searchsorted(used, a) + 1) % used.size], b)
    a[100:120], b[100:120] = a[0:20], b[0:20]       # duplicates, and the same rows the other way round
    a[120:130], b[120:130] = b[20:30].copy(), a[20:30].copy()
    pw = rng.uniform(0.1, 3.0, n_pairs)
    pw[rng.choice(n_pairs, n_pairs // 5, replace=False)] = 0.0
    rw = rng.uniform(0.0, 2.0, n_rows)
    rw[[3, 7, 21]] = 0.0
    return a, b, rw, pw


# ---- 1. the restated B against the dense matrix
@DTYPES
@pytest.mark.parametrize("with_rw", [True, False], ids=["row_weight", "identity"])
def test_row_operator_against_the_dense_matrix(dt, with_rw):
    rng = np.random.default_rng(61)
    a, b, rw, pw = random_pairs(rng)
    assert len(set(zip(a.tolist(), b.tolist()))) < 300 and not np.any(a == b)
    rw, pw = rw.astype(dt), pw.astype(dt)
    x, y = rng.standard_normal(40).astype(dt), rng.standard_normal(40).astype(dt)
    rwa = rw if with_rw else None
    # the dense fp64 matrix, applied in extended precision so that the reference's own error is far below the bound in fp64 too
    B = DD.dense_operator(40, a, b, rwa, pw)
    assert np.array_equal(B, B.T)
    ref = lambda v: (B.astype(np.longdouble) @ v.astype(np.longdouble))   # noqa: E731
    Bx, By = DD.row_operator(x, a, b, rwa, pw), DD.row_operator(y, a, b, rwa, pw)
    assert Bx.dtype == dt
    for v, Bv in ((x, Bx), (y, By)):
        err = np.abs(Bv.astype(np.longdouble) - ref(v)).astype(np.float64)
        bound = DD.row_bound(v, a, b, rwa, pw)
        print("B x, %s: worst row error / bound %.3f" % (np.dtype(dt).name, float(np.max(err / np.maximum(bound, 1e-300)))))
        assert np.all(err <= bound)
    # rows without entries: the start term alone
    for r in (7, 19, 33):
        assert Bx[r] == (dt(rw[r] * x[r]) if with_rw else x[r])
    # symmetry, <x, B y> = <B x, y>, held by the same per-row bound
    f8 = lambda v: np.asarray(v, dtype=np.float64)   # noqa: E731
    lhs, rhs = f8(x) @ f8(By), f8(Bx) @ f8(y)
    sym_bound = np.abs(f8(x)) @ DD.row_bound(y, a, b, rwa, pw) + np.abs(f8(y)) @ DD.row_bound(x, a, b, rwa, pw)
    # (and the two fp64 inner products of 40 terms of the test itself: gamma_40 = 20 eps each)
    sym_bound += 20 * np.finfo(np.float64).eps * (np.abs(f8(x)) @ np.abs(f8(By)) + np.abs(f8(Bx)) @ np.abs(f8(y)))
    print("symmetry, %s: |<x, B y> - <B x, y>| = %.3e (bound %.3e)" % (np.dtype(dt).name, abs(lhs - rhs), sym_bound))
    assert abs(lhs - rhs) <= sym_bound


@DTYPES
def test_pair_adjoint_is_the_transpose_of_pair_difference(dt):
    rng = np.random.default_rng(67)
    a, b, _, _ = random_pairs(rng)
    Q = np.stack([DD.pair_difference(np.eye(40, dtype=dt)[r], a, b) for r in range(40)], axis=1)       # (n_pairs, n_rows)
    Qt = np.stack([DD.pair_adjoint(np.eye(300, dtype=dt)[p], 40, a, b) for p in range(300)], axis=1)   # (n_rows, n_pairs)
    assert Q.dtype == dt and Qt.dtype == dt and np.array_equal(Q.T, Qt)
    assert np.array_equal(np.abs(Q).sum(axis=1), np.full(300, 2)) and not np.any(Q.sum(axis=1))
    assert not np.any(Qt[[7, 19, 33]]) and not np.any(np.signbit(Qt[[7, 19, 33]]))
    off, ent = DD.csr(40, a, b)
    assert off[-1] == 600 and all(np.all(np.diff(ent[off[r]:off[r + 1]] // 2) >= 0) for r in range(40))


# ---- 2. the three consequences
@DTYPES
def test_empty_pair_list(dt):
    rng = np.random.default_rng(71)
    x, rw = rng.standard_normal(9).astype(dt), rng.uniform(0, 2, 9).astype(dt)
    x[4] = -0.0
    e = np.zeros(0, dtype=np.int64)
    assert DD.row_operator(x, e, e, rw, np.zeros(0, dtype=dt)).tobytes() == (rw * x).astype(dt).tobytes()
    assert DD.row_operator(x, e, e, None, np.zeros(0, dtype=dt)).tobytes() == x.tobytes()
    assert DD.pair_difference(x, e, e).shape == (0,) and not np.any(DD.pair_adjoint(np.zeros(0, dtype=dt), 9, e, e))


@DTYPES
def test_constant_rows_and_the_common_origin_time_shift(dt, dense):   # noqa: F811
    rng = np.random.default_rng(73)
    a, b, _, pw = random_pairs(rng)
    for c in (1.25, -3.0e-7, 0.0):
        d = DD.pair_difference(np.full(40, c, dtype=dt), a, b)
        assert not np.any(d) and not np.any(np.signbit(d))
    # the receiver joint system of 6k's dense case: all-zero row_weight, v = 0, one common dt0 on every receiver point
    n, J, G = dense["n"], dense["J"], dense["G"].astype(dt)
    Js = J[:, :n].astype(dt)
    pa, pb = np.array([0, 1, 2, 3, 0]), np.array([3, 4, 5, 1, 5])
    ppw = np.array([1.5, 0.0, 2.0, 0.7, 1.0], dtype=dt)
    v_rcv = np.zeros((3, 4), dtype=dt)
    v_rcv[:, 0] = dt(0.3712)
    dtt = RR.joint_tangent((Js @ np.zeros(n, dtype=dt)).astype(dt), G, POR, v_rcv)
    assert np.array_equal(dtt, np.full(6, dt(0.3712), dtype=dt))
    g, g_rcv = DD.receiver_joint_product(lambda v: (Js @ v).astype(dt), lambda w: (Js.T @ w).astype(dt), G, POR, 3, np.zeros(n, dtype=dt),
                                         v_rcv, pa, pb, row_weight=np.zeros(6, dtype=dt), pair_weight=ppw)
    assert not np.any(DD.row_operator(dtt, pa, pb, np.zeros(6, dtype=dt), ppw))
    assert g.shape == (n,) and g_rcv.shape == (3, 4) and not np.any(g) and not np.any(g_rcv)


# ---- 3. the three restated CG systems with pairs, on 6k's dense case
PAIR_A, PAIR_B = np.array([0, 1, 2]), np.array([3, 4, 5])   # the two events' rows at each of the three shared receiver points
SDAMP = np.array([1e-2, 1e-1, 1e-1, 1e-1])                   # (6j's)
CG_RTOL = 1e-6
CG_SMOOTH, CG_DAMP = 1e-3, 1e-1


@pytest.fixture(scope="module")
def dense_src(dense):   # noqa: F811
    """6k's dense case with the source block of its two events added: J_src (6 x 8) from the joint tangent restatement"""
    from oracle import oracle as O

    n = dense["n"]
    X, Y, Z = np.meshgrid(*[np.arange(k) * CG_DX for k in NN], indexing="ij")
    s = (0.5 + 0.02 * X + 0.015 * Y + 0.03 * Z + 0.05 * np.sin(0.9 * X) * np.cos(0.7 * Y + 0.3 * Z)).flatten("F")
    srcs = [np.array([[0.7, 0.9, 1.1]]), np.array([[1.9, 1.3, 2.6]])]
    pts = np.array([[1.63, 0.41, 2.37], [0.38, 1.71, 0.62], [2.21, 1.12, 1.34]])
    fields = []
    for src in srcs:
        o = O.solve3d(np.float64, tuple(k - 1 for k in NN), CG_DX, (0.0, 0.0, 0.0), s, src, rcv=pts, eps=1e-15, maxit=200)
        fields.append(o["tt"])
    Jsrc = np.zeros((6, 8))
    for j in range(8):
        unit = np.zeros(8)
        unit[j] = 1.0
        _, dtts = JR.joint_tangent(fields, s, CG_DX, NN, (0.0, 0.0, 0.0), srcs, np.zeros(n), unit.reshape(2, 4), rcvs=[pts, pts])
        Jsrc[:, j] = np.concatenate(dtts)
    # (the slowness half of that tangent is 6k's J_s: one column as a check)
    unit = np.zeros(n)
    unit[n // 2] = 1.0
    _, dtts = JR.joint_tangent(fields, s, CG_DX, NN, (0.0, 0.0, 0.0), srcs, unit, np.zeros((2, 4)), rcvs=[pts, pts])
    assert np.allclose(np.concatenate(dtts), dense["J"][:, n // 2], rtol=1e-12, atol=1e-15)
    return dict(dense, Jsrc=Jsrc)


def _weights(kind, rng):
    """pure double-difference weights (all-zero row_weight) or mixed ones, with a zero among each"""
    pw = rng.uniform(0.5, 2.0, 3)
    rw = np.zeros(6) if kind == "pure" else rng.uniform(0.5, 2.0, 6)
    if kind == "mixed":
        rw[4] = 0.0
    return rw, pw


@pytest.mark.parametrize("kind", ["pure", "mixed"])
@pytest.mark.parametrize("system", ["model", "joint", "receiver_joint"])
def test_restated_cg_with_pairs_on_a_dense_system(dense_src, system, kind):
    """The right-hand side is a Gauss-Newton gradient J^T B r as double_difference_step forms it.  With pure double-difference weights a
    common origin-time shift is in the null space of B J: the block damping (rcv_damp / source_damp > 0) is what makes the system
    definite, and the recurrence converges on it."""
    n, rng = dense_src["n"], np.random.default_rng({"model": 83, "joint": 89, "receiver_joint": 97}[system] + (kind == "mixed"))
    Js, G = dense_src["J"][:, :n], dense_src["G"]
    rw, pw = _weights(kind, rng)
    B = DD.dense_operator(6, PAIR_A, PAIR_B, rw, pw)
    res = rng.standard_normal(6)
    smooth_op = lambda p: NR.smooth(p, NN, CG_DX)   # noqa: E731
    if system == "model":
        J, nb, S = Js, 0, np.ones(n)
        A = J.T @ B @ J
        A += CG_SMOOTH * dense_src["R"] + CG_DAMP * np.eye(n)
        b = J.T @ (B @ res)
        x, info = NR.cg(lambda p: DD.gauss_newton(lambda v: Js @ v, lambda w: Js.T @ w, p, PAIR_A, PAIR_B, rw, pw), b, np.float64,
                        smooth_op=smooth_op, smooth=CG_SMOOTH, damp=CG_DAMP, maxiter=n, rtol=CG_RTOL)
        z, bz = x, b
    else:
        Jb = dense_src["Jsrc"] if system == "joint" else dense_src["J"][:, n:]
        npt = Jb.shape[1] // 4
        J, nb = np.concatenate([Js, Jb], axis=1), Jb.shape[1]
        scale, bdamp = np.tile(SCALE, (npt, 1)), np.tile(SDAMP if system == "joint" else RDAMP, (npt, 1))
        S = np.concatenate([np.ones(n), scale.ravel()])
        A = S[:, None] * (J.T @ B @ J) * S[None, :]
        A[:n, :n] += CG_SMOOTH * dense_src["R"] + CG_DAMP * np.eye(n)
        A[n:, n:] += np.diag(bdamp.ravel())
        grad = J.T @ (B @ res)
        b_s, b_e = grad[:n], grad[n:].reshape(npt, 4)
        if system == "joint":
            def product(p, pe):
                return DD.joint_product(lambda v, ve: Js @ v + Jb @ np.asarray(ve).ravel(),
                                        lambda w: (Js.T @ w, (Jb.T @ w).reshape(npt, 4)), p, pe, PAIR_A, PAIR_B, np.float64, rw, pw, scale)
            x_s, x_e, info = JR.cg(product, b_s, b_e, np.float64, smooth_op=smooth_op, smooth=CG_SMOOTH, damp=CG_DAMP, source_damp=bdamp,
                                   source_scale=scale, maxiter=n + nb, rtol=CG_RTOL)
        else:
            def product(p, pe):
                return DD.receiver_joint_product(lambda v: Js @ v, lambda w: Js.T @ w, G, POR, 3, p, pe, PAIR_A, PAIR_B, rw, pw, scale)
            x_s, x_e, info = RR.cg(product, b_s, b_e, np.float64, smooth_op=smooth_op, smooth=CG_SMOOTH, damp=CG_DAMP, rcv_damp=bdamp,
                                   rcv_scale=scale, maxiter=n + nb, rtol=CG_RTOL)
        assert np.any(x_e != 0)
        bz = np.concatenate([b_s, S[n:] * b_e.ravel()])
        z = np.concatenate([x_s, x_e.ravel() / S[n:]])
    assert np.linalg.cond(A) * np.finfo(np.float64).eps < 0.01 * CG_RTOL
    if kind == "pure" and system != "model":   # without the block damping the common origin-time shift is a null vector of the block
        shift = np.zeros(n + nb)
        shift[n::4] = 1.0
        A0 = A.copy()
        A0[n:, n:] -= np.diag(bdamp.ravel())
        assert np.linalg.norm(A0 @ shift) <= 1e-12 * np.linalg.norm(A0) and np.linalg.norm(A @ shift) > 1e-3
    true = np.linalg.norm(bz - A @ z) / np.linalg.norm(bz)
    print("dd cg, %s system, %s weights: %d iterations, recurrence residual %.3e, true residual %.3e"
          % (system, kind, info["iterations"], math.sqrt(info["rho"][-1] / info["rho"][0]), true))
    assert info["status"] == 0 and 1 <= info["iterations"] < n + nb
    assert info["rho"][-1] <= CG_RTOL * CG_RTOL * info["rho"][0] < info["rho"][-2]
    assert true <= 2 * CG_RTOL


def test_restated_products_are_the_dense_matrices(dense_src):
    n, rng = dense_src["n"], np.random.default_rng(101)
    Js, Jr, Jq, G = dense_src["J"][:, :n], dense_src["J"][:, n:], dense_src["Jsrc"], dense_src["G"]
    rw, pw = _weights("mixed", rng)
    B = DD.dense_operator(6, PAIR_A, PAIR_B, rw, pw)
    v, vr, vq = rng.standard_normal(n), rng.standard_normal((3, 4)), rng.standard_normal((2, 4))
    rel = lambda x, y: np.linalg.norm(x - y) / np.linalg.norm(y)   # noqa: E731
    g = DD.gauss_newton(lambda p: Js @ p, lambda w: Js.T @ w, v, PAIR_A, PAIR_B, rw, pw)
    assert rel(g, Js.T @ B @ Js @ v) < 1e-13
    g, ge = DD.receiver_joint_product(lambda p: Js @ p, lambda w: Js.T @ w, G, POR, 3, v, vr, PAIR_A, PAIR_B, rw, pw)
    J = np.concatenate([Js, Jr], axis=1)
    assert rel(np.concatenate([g, ge.ravel()]), J.T @ B @ J @ np.concatenate([v, vr.ravel()])) < 1e-13
    g, ge = DD.joint_product(lambda p, pe: Js @ p + Jq @ np.asarray(pe).ravel(), lambda w: (Js.T @ w, (Jq.T @ w).reshape(2, 4)), v, vq,
                             PAIR_A, PAIR_B, np.float64, rw, pw)
    J = np.concatenate([Js, Jq], axis=1)
    assert rel(np.concatenate([g, ge.ravel()]), J.T @ B @ J @ np.concatenate([v, vq.ravel()])) < 1e-13


# ---- 4. argument errors, before anything is launched
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
    t.dtype, t.n_cols, t.n_data, t._per, t.device = np.dtype(np.float32), 60, 9, "node", 0
    t.n_points, t.n_rows, t.n_events, t.n_nodes = 2, 7, 2, 60
    t.n_rcv_points = 3
    t._rows = np.array([0, 1, 2, 4, 5, 6, 8])   # data rows 3 and 7 are not on the tape
    yield t
    t._h = C.c_void_p()


def _products_and_solves(t, **kw):
    v, es, er = np.zeros(60, dtype=np.float32), np.zeros((2, 4), dtype=np.float32), np.zeros((3, 4), dtype=np.float32)
    return [lambda: t.gauss_newton(v, **kw), lambda: t.newton(v, **kw), lambda: t.gauss_newton_joint(v, es, **kw),
            lambda: t.gauss_newton_receiver_joint(v, er, **kw), lambda: t.solve_normal(v, **kw), lambda: t.solve_joint(v, es, **kw),
            lambda: t.solve_receiver_joint(v, er, **kw)]


def test_python_argument_errors(fake_tape):
    t = fake_tape
    assert t.n_pairs == 0 and t.row_pairs.shape == (0, 2)
    # pair_weight without pairs, on all seven methods; None stays today's call
    for call in _products_and_solves(t, pair_weight=np.zeros(0, dtype=np.float32)):
        with pytest.raises(ValueError, match="no row pairs"):
            call()
    for call in _products_and_solves(t, pair_weight=None):
        with pytest.raises(AssertionError, match="reached the library"):
            call()
    for call in (lambda: t.pair_difference(np.zeros(9)), lambda: t.pair_adjoint(np.zeros(0)), lambda: t.row_operator(np.zeros(9))):
        with pytest.raises(ValueError, match="no row pairs"):
            call()
    # set_row_pairs: shapes and dtypes, a == b, rows that are not on the tape, all before the library
    for wrong_a, wrong_b in (([0, 1], [1]), ([[0, 1]], [[1, 2]]), ([0.0, 1.0], [1, 2]), (["a"], ["b"])):
        with pytest.raises(ValueError, match="row_a|row_b"):
            t.set_row_pairs(wrong_a, wrong_b)
    with pytest.raises(ValueError, match=r"pair 2 \(data rows 4, 4\) joins a row to itself"):
        t.set_row_pairs([0, 1, 4, 3], [1, 2, 4, 0])
    with pytest.raises(ValueError, match=r"pair 1 \(data rows 1, 3\).*not on the tape"):
        t.set_row_pairs([0, 1, 2], [1, 3, 7])
    for outside in (9, -1):
        with pytest.raises(ValueError, match=r"pair 0 \(data rows 0, %d\).*not on the tape" % outside):
            t.set_row_pairs([0], [outside])
    with pytest.raises(AssertionError, match="reached the library"):   # (a good list, an empty one too, does get there)
        t.set_row_pairs([0, 8, 0], [8, 2, 8])
    with pytest.raises(AssertionError, match="reached the library"):
        t.set_row_pairs([], [])
    # with pairs set: the shape and the values of pair_weight, x and y
    t._pairs_set, t.n_pairs = True, 4
    good = np.array([1.0, 0.0, 2.0, 0.5], dtype=np.float32)
    for wrong in (np.ones(3), np.ones(5), np.ones((4, 1)), 1.0, np.array([1, 1, -1e-9, 1]), np.array([1, np.nan, 1, 1]),
                  np.array([1, 1, 1, np.inf])):
        for call in _products_and_solves(t, pair_weight=wrong) + [lambda: t.row_operator(np.zeros(9), None, wrong)]:
            with pytest.raises(ValueError, match="pair_weight"):
                call()
    for call in _products_and_solves(t, pair_weight=good) + [lambda: t.row_operator(np.zeros(9), np.ones(9), good),
                                                             lambda: t.row_operator(np.zeros(9)), lambda: t.pair_difference(np.zeros(9)),
                                                             lambda: t.pair_adjoint(good), lambda: t.release_pairs()]:
        with pytest.raises(AssertionError, match="reached the library"):
            call()
    with pytest.raises(ValueError, match="x should hold 9"):
        t.pair_difference(np.zeros(7))
    with pytest.raises(ValueError, match="x should hold 9"):
        t.row_operator(np.zeros(4), None, good)
    with pytest.raises(ValueError, match="row_weight should hold 9"):
        t.row_operator(np.zeros(9), np.ones(7), good)
    with pytest.raises(ValueError, match="y should hold 4"):
        t.pair_adjoint(np.zeros(9))
    # the other checks of the seven methods still come first or alongside
    with pytest.raises(ValueError, match="hessian"):
        t.solve_joint(np.zeros(60), np.zeros((2, 4)), pair_weight=good, hessian="newton")
    with pytest.raises(ValueError, match="schedule"):
        t.gauss_newton(np.zeros(60), pair_weight=good, schedule="fast")
    with pytest.raises(ValueError, match="v should hold 60"):
        t.newton(np.zeros(61), pair_weight=good)


def _err(lib, status, *words):
    from ttcr_amd import _lib

    assert status == _lib.ERR_VALUE, status
    msg = _lib.last_error()
    assert msg and all(w in msg for w in words), msg


def test_symbols_and_c_argument_errors_come_before_the_device(lib):
    from ttcr_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ttcr_amd.h")).read()
    pxd = open(os.path.join(ROOT, "integration", "ttcr_amd.pxd")).read()
    for name in DD_SYMBOLS:
        assert name + "(" in hdr and name + "(" in pxd and name in _lib.SYMBOLS and getattr(lib, name) is not None, name
    a = np.zeros(8, dtype=np.float32)
    p = a.ctypes.data_as(C.c_void_p)
    ia = (C.c_int * 2)(0, 1)
    w3 = (C.c_double * 3)(1.0, 1.0, 1.0)
    st, it = C.c_int(-7), C.c_int(-7)
    rho, pq = (C.c_double * 8)(), (C.c_double * 8)()
    bad_pair = C.c_longlong(5)
    fake = C.c_void_p(1234)   # never dereferenced: the argument checks come first
    pairs, apply_, gn = lib.ttcr_fsm_dd_pairs, lib.ttcr_fsm_dd_apply, lib.ttcr_fsm_dd_gn
    _err(lib, pairs(None, None, None, 0, None, None, None, C.byref(bad_pair)), "null tape")
    assert bad_pair.value == -1
    _err(lib, pairs(None, ia, ia, 2, None, None, None, None), "null tape")
    _err(lib, pairs(fake, ia, None, 2, None, None, None, None), "null set_row_b")
    _err(lib, pairs(fake, None, ia, 2, None, None, None, None), "null set_row_a")
    _err(lib, pairs(fake, ia, ia, 2 ** 30, None, None, None, None), "2^30 - 1")
    _err(lib, apply_(fake, 3, p, 0, None, 0, None, 0, p, 0), "mode")
    _err(lib, apply_(fake, -1, p, 0, None, 0, None, 0, p, 0), "mode")
    _err(lib, apply_(fake, 0, None, 0, None, 0, None, 0, p, 0), "null x")
    _err(lib, apply_(fake, 1, p, 0, None, 0, None, 0, None, 0), "null out")
    _err(lib, apply_(fake, 0, p, 0, p, 0, None, 0, p, 0), "mode 2")
    _err(lib, apply_(fake, 1, p, 0, None, 0, p, 0, p, 0), "mode 2")
    _err(lib, apply_(None, 2, p, 0, p, 0, p, 0, p, 0), "null tape")

    def gn_(**kw):
        v = dict(t=fake, system=0, newton=0, v=p, vb=p, pw=p, out=p, ob=p, schedule=0)
        v.update(kw)
        return gn(v["t"], v["system"], v["newton"], v["v"], 0, v["vb"], 0, None, 0, v["pw"], 0, None, v["out"], 0, v["ob"], 0, v["schedule"],
                  None, None)

    _err(lib, gn_(system=3), "system")
    _err(lib, gn_(system=-1), "system")
    _err(lib, gn_(newton=2), "newton")
    _err(lib, gn_(system=1, newton=1), "newton", "model system")
    _err(lib, gn_(system=2, newton=1), "newton", "model system")
    _err(lib, gn_(pw=None), "null pair_weight")
    _err(lib, gn_(t=None), "null tape")
    _err(lib, gn_(v=None), "null v")
    _err(lib, gn_(out=None), "null out")
    _err(lib, gn_(system=1, vb=None), "null v_src")
    _err(lib, gn_(system=2, vb=None), "null v_rcv")
    _err(lib, gn_(system=1, ob=None), "null out_src")
    _err(lib, gn_(system=2, t=None), "null tape")
    _err(lib, gn_(system=2, schedule=3, t=None), "null tape")

    def solve(**kw):
        v = dict(t=None, system=0, rhs=p, rb=p, pw=p, smooth=1.0, w=w3, damp=1.0, x0=None, maxiter=3, rtol=1e-6, newton=0, schedule=0, x=p,
                 xb=p, st=C.byref(st))
        v.update(kw)
        return lib.ttcr_fsm_dd_solve(v["t"], v["system"], v["rhs"], 0, v["rb"], 0, None, 0, v["pw"], 0, v["smooth"], v["w"], v["damp"], None,
                                     None, v["x0"], 0, v["maxiter"], v["rtol"], v["newton"], v["schedule"], v["x"], 0, v["xb"], 0, v["st"],
                                     C.byref(it), rho, pq, None)

    _err(lib, solve(system=4), "system")
    _err(lib, solve(newton=-1), "newton")
    _err(lib, solve(system=1, newton=1), "newton", "model system")
    _err(lib, solve(system=2, x0=p), "x0", "model system")
    _err(lib, solve(pw=None), "null pair_weight")
    _err(lib, solve(smooth=-1.0), "smooth")
    _err(lib, solve(damp=float("nan")), "damp")
    _err(lib, solve(maxiter=0), "maxiter")
    _err(lib, solve(rtol=-1.0), "rtol")
    _err(lib, solve(w=None), "null smooth_weights")
    _err(lib, solve(schedule=2), "schedule")
    _err(lib, solve(rhs=None), "null rhs")
    _err(lib, solve(system=1, rb=None), "null rhs_src")
    _err(lib, solve(system=2, rb=None), "null rhs_rcv")
    _err(lib, solve(x=None), "null x")
    _err(lib, solve(system=2, xb=None), "null x_rcv")
    _err(lib, solve(st=None), "null status")
    for system in (0, 1, 2):
        _err(lib, solve(system=system), "null tape")
    _err(lib, lib.ttcr_fsm_dd_release(None), "null tape")
    assert st.value == -7 and it.value == -7 and not np.any(a)   # (no call got as far as its outputs)


# ---- 5. double_difference_step on a stand-in tape that records the calls it receives
class _Recorder:
    dtype = np.dtype(np.float64)
    n_pairs = 3

    def __init__(self):
        self.calls = []

    def pair_adjoint(self, y):
        self.calls.append(("pair_adjoint", np.array(y)))
        return np.array([y[0], y[1], y[2], -y[0], -y[1], -y[2]])

    def vjp(self, w, **kw):
        self.calls.append(("vjp", np.array(w), kw))
        g = np.full(5, w.sum() + 1.0)
        return (g, np.full((2, 4), 7.0)) if kw else g

    def smooth(self, model, weights):
        self.calls.append(("smooth", np.array(model), tuple(weights)))
        return 2.0 * np.asarray(model)

    def _solve(self, name, *args, **kw):
        self.calls.append((name, args, kw))
        return name

    def solve_normal(self, *args, **kw):
        return self._solve("solve_normal", *args, **kw)

    def solve_joint(self, *args, **kw):
        return self._solve("solve_joint", *args, **kw)

    def solve_receiver_joint(self, *args, **kw):
        return self._solve("solve_receiver_joint", *args, **kw)


def test_double_difference_step_on_a_stand_in_tape():
    from ttcr_amd import inversion

    res, pres = np.arange(6.0), np.array([0.5, -1.0, 2.0])
    rw, pw, model = np.array([1.0, 2.0, 0.0, 1.0, 1.0, 3.0]), np.array([2.0, 0.0, 1.0]), np.arange(5.0)
    # the model system with mixed weights and smoothing
    t = _Recorder()
    out = inversion.double_difference_step(t, res, pres, model, row_weight=rw, pair_weight=pw, smooth=0.5, damp=0.1, maxiter=7,
                                           smooth_weights=(1.0, 2.0, 3.0))
    assert out == "solve_normal" and [c[0] for c in t.calls] == ["pair_adjoint", "vjp", "smooth", "solve_normal"]
    assert np.array_equal(t.calls[0][1], pw * pres)
    w = rw * res + np.array([1.0, 0.0, 2.0, -1.0, 0.0, -2.0])
    assert np.array_equal(t.calls[1][1], w) and t.calls[1][2] == {}
    assert np.array_equal(t.calls[2][1], model) and t.calls[2][2] == (1.0, 2.0, 3.0)
    (b,), kw = t.calls[3][1], t.calls[3][2]
    assert np.array_equal(b, np.full(5, w.sum() + 1.0) - 0.5 * 2.0 * model)
    assert kw["row_weight"] is rw and kw["pair_weight"] is pw and kw["smooth"] == 0.5 and kw["damp"] == 0.1 and kw["maxiter"] == 7
    assert kw["smooth_weights"] == (1.0, 2.0, 3.0)
    # pure double-difference data on the two joint systems: no residual, pair_weight None means ones, row_weight all zero
    for system, solve, grad, setting in (("joint", "solve_joint", "return_source_grad", "source"),
                                         ("receiver_joint", "solve_receiver_joint", "return_receiver_grad", "rcv")):
        t = _Recorder()
        out = inversion.double_difference_step(t, None, pres, model, system=system, block_damp=(1e-2, 0, 0, 0), block_scale=(1, 0.1, 0.1, 0.1))
        assert out == solve and [c[0] for c in t.calls] == ["pair_adjoint", "vjp", solve]
        assert np.array_equal(t.calls[0][1], pres)
        assert np.array_equal(t.calls[1][1], [0.5, -1.0, 2.0, -0.5, 1.0, -2.0]) and t.calls[1][2] == {grad: True}
        (b, b_blk), kw = t.calls[2][1], t.calls[2][2]
        assert np.array_equal(b, np.full(5, 1.0)) and np.array_equal(b_blk, np.full((2, 4), 7.0))
        assert np.array_equal(kw["row_weight"], np.zeros(6)) and np.array_equal(kw["pair_weight"], np.ones(3))
        assert kw[setting + "_damp"] == (1e-2, 0, 0, 0) and kw[setting + "_scale"] == (1, 0.1, 0.1, 0.1) and kw["smooth"] == 0 and kw["damp"] == 0
    with pytest.raises(ValueError, match="system"):
        inversion.double_difference_step(_Recorder(), res, pres, model, system="source")


def test_python_layer_documents_the_null_vector():
    from ttcr_amd.rgrid import FieldTape

    for name in ("solve_joint", "solve_receiver_joint", "gauss_newton_receiver_joint"):
        doc = " ".join(getattr(FieldTape, name).__doc__.split())
        assert "pair_weight" in doc and ("origin-time shift" in doc or "common dt0" in doc), name
