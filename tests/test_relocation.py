"""Moving the receiver points of the field tape and the relocation-only system, without a device: the numpy restatement
of tests/relocation_reference.py against dense matrices, numpy.linalg.solve and its own invariants, the recovery of a cluster of
hypocentres by the restated relocation loop, inversion.relocate on a stand-in tape against that loop (to the bit), and the argument errors
of the new methods and C entries.  Fields come from the oracle, the receiver arithmetic from tests/receiver_reference.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import relocation_reference as LR  # noqa: E402

RELOC_SYMBOLS = ["ttcr_fsm_reloc_move", "ttcr_fsm_reloc_get_points", "ttcr_fsm_reloc_gn", "ttcr_fsm_reloc_solve"]

# ---- the recovery case: 21^3 nodes, dx 1, slowness falling linearly with depth index; six stations on nodes of the top and the sides
# solve, five hypocentres in a cluster are the receiver points of every station
NN, DX, ORIGIN = (21, 21, 21), 1.0, (0.0, 0.0, 0.0)
STATIONS = np.array([[2., 3., 0.], [17., 2., 0.], [10., 18., 0.], [3., 16., 1.], [18., 17., 2.], [0., 9., 6.]])
TRUE = np.array([[9.3, 10.4, 11.2], [10.6, 9.7, 12.3], [11.2, 11.4, 10.6], [8.7, 11.6, 12.7], [10.3, 8.6, 11.7]])
# (at most 0.4 dx per axis; no start coordinate on a grid plane: G is zero along an axis on whose plane a point lies, so a
# Gauss-Newton step never leaves that plane)
OFFSET = 0.4 * np.array([[1., -0.75, 0.5], [-0.75, 1., -1.], [0.5, 0.25, 0.75], [-1., -0.5, -0.25], [0.9, 0.8, -0.7]])
T0_TRUE = np.array([0.3, -0.2, 0.1, 0.0, 0.25])
# the location error max |xyz - TRUE| the restated loop ends with, as measured here (both 10 iterations, rcv_damp 1e-3)
MEASURED = {"absolute": 9.5e-9, "pairs": 2.3e-9}


def gradient_model():
    k = np.arange(NN[2], dtype=np.float64)
    s = np.broadcast_to((0.5 - 0.01 * k)[None, None, :], NN)
    return s.flatten("F")


@pytest.fixture(scope="module")
def fields():
    from oracle import oracle as O

    O.build(with_ref=False)
    s = gradient_model()
    nc = tuple(n - 1 for n in NN)
    return [O.solve3d(np.float64, nc, DX, ORIGIN, s, st[None, :])["tt"] for st in STATIONS]


def layout_of(fields, pairs=False, dtype=np.float64):
    E, P = len(STATIONS), len(TRUE)
    ev, pt = np.repeat(np.arange(E), P), np.tile(np.arange(P), E)
    pr = None
    if pairs:   # neighbouring hypocentres at one station, and the first against the last
        a = [e * P + q for e in range(E) for q in range(P - 1)] + [e * P for e in range(E)]
        b = [e * P + q + 1 for e in range(E) for q in range(P - 1)] + [e * P + P - 1 for e in range(E)]
        pr = (a, b)
    return LR.Layout([np.asarray(f, dtype=dtype) for f in fields], NN, DX, ORIGIN, ev, pt, P, pairs=pr)


def data_of(layout):
    tt, _, _ = LR.move(layout, TRUE)
    t_obs = tt + T0_TRUE[layout.point_of_row]
    pair_dt = None
    if layout.pairs is not None:
        a, b = layout.pairs
        pair_dt = t_obs[a] - t_obs[b]
    return t_obs, pair_dt


def weights(layout, seed=3):
    rng = np.random.default_rng(seed)
    rw = rng.uniform(0.5, 2.0, len(layout.point_of_row))
    pw = rng.uniform(0.2, 3.0, len(layout.pairs[0])) if layout.pairs is not None else None
    return rw, pw


# ---- 1. the product and the CG against dense matrices
@pytest.mark.parametrize("with_pairs", [False, True], ids=["rows", "pairs"])
def test_product_against_the_dense_matrices(fields, with_pairs):
    lay = layout_of(fields, with_pairs)
    _, G, _ = LR.move(lay, TRUE + OFFSET)
    rw, pw = weights(lay)
    scale = np.array([1.0, 0.5, 2.0, 0.25])
    A, Gm, B = LR.dense(lay, G, rw, scale, pw)
    assert np.allclose(A, A.T, rtol=0, atol=1e-13 * np.abs(A).max())
    rng = np.random.default_rng(5)
    for _ in range(3):
        v = rng.standard_normal((lay.n_points, 4))
        got = LR.product(lay, G, v, rw, scale, pw)
        want = (A @ v.ravel()).reshape(-1, 4)
        # fp64, sums of at most n_rows + pairs terms: a forward error of a few hundred roundings of the largest term
        assert np.max(np.abs(got - want)) <= 1e-12 * np.abs(want).max()
    u, v = rng.standard_normal((2, lay.n_points, 4))
    uAv = float(np.sum(u * LR.product(lay, G, v, rw, scale, pw)))
    vAu = float(np.sum(v * LR.product(lay, G, u, rw, scale, pw)))
    assert abs(uAv - vAu) <= 1e-12 * max(abs(uAv), abs(vAu))
    assert not np.any(LR.product(lay, G, v, rw, np.zeros(4), pw))            # rcv_scale all zeros: zeros


def test_cg_against_linalg_solve(fields):
    lay = layout_of(fields, True)
    _, G, _ = LR.move(lay, TRUE + OFFSET)
    rw, pw = weights(lay)
    scale = np.array([1.0, 0.5, 0.5, 0.5])
    damp = np.array([0.5, 2.0, 2.0, 2.0])      # well damped: the condition number stays below 1e3
    A, _, _ = LR.dense(lay, G, rw, scale, pw)
    rhs = np.random.default_rng(9).standard_normal((lay.n_points, 4))
    c = np.broadcast_to(scale, rhs.shape).ravel()
    M = A + np.diag(np.broadcast_to(damp, rhs.shape).ravel())
    assert np.linalg.cond(M) < 1e3
    z = np.linalg.solve(M, c * rhs.ravel())
    x, info = LR.cg(lambda p: LR.product(lay, G, p, rw, scale, pw), rhs, np.float64, rcv_damp=damp, rcv_scale=scale, maxiter=200, rtol=1e-13)
    assert info["status"] == 0 and info["iterations"] <= 4 * lay.n_points
    # |r| <= 1e-13 |b| at a condition number below 1e3: a relative error below 1e-10
    assert np.max(np.abs(x.ravel() - c * z)) <= 1e-10 * np.abs(c * z).max()


def test_common_origin_time_shift_is_a_null_vector_of_pure_pair_data(fields):
    lay = layout_of(fields, True)
    _, G, _ = LR.move(lay, TRUE + OFFSET)
    _, pw = weights(lay)
    shift = np.zeros((lay.n_points, 4))
    shift[:, 0] = 0.75
    out = LR.product(lay, G, shift, np.zeros(len(G)), None, pw)
    assert not np.any(out) and not np.any(np.signbit(out))
    assert np.any(LR.product(lay, G, shift, None, None, pw))                 # with absolute rows it is not


# ---- 2. recovery by the restated loop, and inversion.relocate on a stand-in tape against it
@pytest.mark.parametrize("mode", ["absolute", "pairs"])
def test_relocate_recovers_the_cluster(fields, mode):
    from ttcr_amd import inversion

    lay = layout_of(fields, mode == "pairs")
    t_obs, pair_dt = data_of(lay)
    start, t0 = TRUE + OFFSET, np.zeros(len(TRUE))
    assert np.max(np.abs(OFFSET)) <= 0.4 * DX
    kw = dict(pair_dt=pair_dt, n_iter=10, rcv_damp=1e-3)
    t0r, xyz, hist, info = LR.relocate(lay, start, t_obs, t0, **kw)
    err = float(np.max(np.abs(xyz - TRUE)))
    print("relocate[%s]: %d iterations, halvings %s, misfit %.3e -> %.3e, location error %.3e dx, t0 error %.3e"
          % (mode, info["iterations"], info["halvings"], hist[0], hist[-1], err / DX, float(np.max(np.abs(t0r - T0_TRUE)))))
    assert all(b <= a for a, b in zip(hist, hist[1:])) and len(hist) == info["iterations"] + 1
    assert hist[-1] < 1e-3 * hist[0]
    assert err <= 10 * MEASURED[mode]
    # the host glue on a stand-in tape: the same points, times and misfits, to the bit
    tape = LR.StandInTape(lay, start)
    t0g, xyzg, histg, infog = inversion.relocate(tape, t_obs, t0, **kw)
    assert np.array_equal(t0g, t0r) and np.array_equal(xyzg, xyz) and histg == hist
    assert infog["halvings"] == info["halvings"] and [c["rho"] for c in infog["cg"]] == [c["rho"] for c in info["cg"]]
    assert np.array_equal(tape.receiver_points(), xyz)                       # the tape is left at the returned points


def test_relocation_step_is_the_restated_step(fields):
    from ttcr_amd import inversion

    lay = layout_of(fields, True)
    t_obs, pair_dt = data_of(lay)
    tape = LR.StandInTape(lay, TRUE + OFFSET)
    tt, G, _ = LR.move(lay, TRUE + OFFSET)
    rw, pw = weights(lay)
    r = t_obs - tt
    rp = pair_dt - (tt[lay.pairs[0]] - tt[lay.pairs[1]])
    for kw in (dict(), dict(row_weight=rw), dict(pair_residual=rp, pair_weight=pw), dict(row_weight=rw, pair_residual=rp)):
        got = inversion.relocation_step(tape, r, rcv_damp=1e-2, rcv_scale=(1., 0.5, 0.5, 0.5), maxiter=7, **kw)
        want, _ = LR.step(lay, G, r, kw.get("pair_residual"), kw.get("row_weight"), kw.get("pair_weight"), 1e-2, (1., 0.5, 0.5, 0.5), 7)
        assert np.array_equal(got, want)
    only_pairs = inversion.relocation_step(tape, None, pair_residual=rp, rcv_damp=1e-2)
    want, _ = LR.step(lay, G, np.zeros_like(r), rp, np.zeros_like(r), None, 1e-2)
    assert np.array_equal(only_pairs, want)
    with pytest.raises(ValueError, match="no data"):
        inversion.relocation_step(tape, None)


# ---- 3. argument errors, none of which reaches the device
def test_move_check():
    from ttcr_amd.rgrid import FieldTape

    geo = ((5, 4, 6), 25.0, np.array([-37.25, 1200.5, -3.125]))
    good = np.array([[-37.25, 1200.5, -3.125], [62.75, 1275.5, 121.875], [0.0, 1250.0, 50.0]])
    for dt in (np.float32, np.float64):
        assert FieldTape.move_check(3, geo, dt, good) is not None
        assert FieldTape.move_check(3, geo, dt, good.tolist()) is not None
        assert FieldTape.move_check(0, geo, dt, np.zeros((0, 3))) is not None
        for bad in (good[:2], good.ravel(), good[:, :2], good[None]):
            with pytest.raises(ValueError, match="xyz should be \\(3, 3\\)"):
                FieldTape.move_check(3, geo, dt, bad)
        with pytest.raises(ValueError, match="real numbers"):
            FieldTape.move_check(3, geo, dt, good.astype(np.complex128))
        with pytest.raises(ValueError, match="real numbers"):
            FieldTape.move_check(3, geo, dt, good.astype(str))
        for v in (np.nan, np.inf, -np.inf):
            bad = good.copy()
            bad[1, 2] = v
            with pytest.raises(ValueError, match="finite"):
                FieldTape.move_check(3, geo, dt, bad)
        for q, a, v in ((0, 0, -37.5), (1, 0, 62.76), (2, 1, 1200.0), (2, 1, 1275.6), (0, 2, -3.2), (1, 2, 122.0)):
            bad = good.copy()
            bad[q, a] = v
            with pytest.raises(ValueError, match="^Receiver outside grid$"):
                FieldTape.move_check(3, geo, dt, bad)


class _NoDevice:
    """stands where the library would: any entry that is reached fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the call reached the library entry " + name)


def _tape_without_device(dt=np.float32):
    from ttcr_amd.rgrid import FieldTape

    t = object.__new__(FieldTape)
    t._lib, t._h, t.dtype = _NoDevice(), C.c_void_p(1), np.dtype(dt)
    t.n_rcv_points, t.n_data, t.n_rows, t.n_events, t.n_nodes, t.n_cols = 3, 6, 6, 2, 8, 8
    t._rows = np.arange(6)
    t.device = 0
    return t


def test_python_argument_errors_come_before_the_device():
    t = _tape_without_device()
    v, w = np.zeros((3, 4), dtype=np.float32), np.zeros(6, dtype=np.float32)
    with pytest.raises(ValueError, match="v_rcv should be \\(3, 4\\)"):
        t.gauss_newton_receiver(v[:2])
    with pytest.raises(ValueError, match="row_weight should hold 6 values"):
        t.gauss_newton_receiver(v, row_weight=w[:5])
    with pytest.raises(ValueError, match="no row pairs"):
        t.gauss_newton_receiver(v, pair_weight=w[:2])
    with pytest.raises(ValueError, match="rcv_scale"):
        t.gauss_newton_receiver(v, rcv_scale=(1., 2., 3.))
    with pytest.raises(ValueError, match="rcv_scale"):
        t.gauss_newton_receiver(v, rcv_scale=(1., -2., 3., 1.))
    with pytest.raises(ValueError, match="rhs_rcv should be \\(3, 4\\)"):
        t.solve_receiver(v.ravel())
    with pytest.raises(ValueError, match="maxiter"):
        t.solve_receiver(v, maxiter=0)
    with pytest.raises(ValueError, match="rtol"):
        t.solve_receiver(v, rtol=-1.0)
    with pytest.raises(ValueError, match="rcv_damp"):
        t.solve_receiver(v, rcv_damp=float("nan"))
    with pytest.raises(ValueError, match="rcv_damp"):
        t.solve_receiver(v, rcv_damp=(1., 2.))
    with pytest.raises(ValueError, match="no row pairs"):
        t.solve_receiver(v, pair_weight=w[:2])
    with pytest.raises(ValueError, match="w should hold 6 values"):
        t.vjp_receiver(w[:3])
    t._h = C.c_void_p()
    for call in (lambda: t.move_receiver_points(np.zeros((3, 3))), t.receiver_points, lambda: t.vjp_receiver(w),
                 lambda: t.gauss_newton_receiver(v), lambda: t.solve_receiver(v)):
        with pytest.raises(ValueError, match="freed"):
            call()


def _err(lib, status, *words):
    from ttcr_amd import _lib

    assert status == _lib.ERR_VALUE, status
    msg = _lib.last_error()
    assert msg and all(w in msg for w in words), msg


def test_c_entries_are_declared_and_check_their_arguments():
    from ttcr_amd import build, _lib

    build.build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ttcr_amd.h")).read()
    pxd = open(os.path.join(ROOT, "integration", "ttcr_amd.pxd")).read()
    for name in RELOC_SYMBOLS:
        assert name + "(" in hdr and name + "(" in pxd and name in _lib.SYMBOLS and getattr(lib, name) is not None, name
    a = np.zeros(16, dtype=np.float32)
    p = a.ctypes.data_as(C.c_void_p)
    d4 = (C.c_double * 16)()
    st, it = C.c_int(-7), C.c_int(-7)
    rho, pq = (C.c_double * 8)(), (C.c_double * 8)()
    fake = C.c_void_p(1234)   # never dereferenced: the argument checks come first
    _err(lib, lib.ttcr_fsm_reloc_move(fake, None, 0, p, 0), "null pts")
    _err(lib, lib.ttcr_fsm_reloc_move(None, p, 0, p, 0), "null tape")
    _err(lib, lib.ttcr_fsm_reloc_get_points(None, d4), "null tape")
    _err(lib, lib.ttcr_fsm_reloc_get_points(fake, None), "null pts")
    gn = lib.ttcr_fsm_reloc_gn
    _err(lib, gn(fake, None, 0, None, 0, None, 0, None, p, 0), "null v_rcv")
    _err(lib, gn(fake, p, 0, None, 0, None, 0, None, None, 0), "null out_rcv")
    _err(lib, gn(None, p, 0, None, 0, None, 0, None, p, 0), "null tape")

    def solve(**kw):
        v = dict(t=None, rhs=p, maxiter=3, rtol=1e-6, x=p, st=C.byref(st))
        v.update(kw)
        return lib.ttcr_fsm_reloc_solve(v["t"], v["rhs"], 0, None, 0, None, 0, None, None, v["maxiter"], v["rtol"], v["x"], 0, v["st"],
                                        C.byref(it), rho, pq)

    _err(lib, solve(maxiter=0), "maxiter")
    _err(lib, solve(rtol=-1.0), "rtol")
    _err(lib, solve(rtol=float("nan")), "rtol")
    _err(lib, solve(rhs=None), "null rhs_rcv")
    _err(lib, solve(x=None), "null x_rcv")
    _err(lib, solve(st=None), "null status")
    _err(lib, solve(), "null tape")
    assert st.value == -7 and it.value == -7 and not np.any(a)   # (no call got as far as its outputs)
