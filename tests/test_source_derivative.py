"""The field tape's derivatives with respect to the source points (origin time and position) without a device: the definition
(tests/source_reference.py, the numpy restatement the device is compared with bit for bit) is the directional derivative of what the
reference's scheme computes -- central finite differences of the oracle in all four parameters of every point agree with it to 1e-6
relative, over the whole field and at the receivers --, its origin-time column is exactly 1 everywhere, and its reverse mode is the
transpose of its forward mode (dot-product identity, to rounding); the three C entry points are exported and declared, refuse bad
arguments before any device call, and the Python layer has the methods without importing torch.

No finite difference is taken across a cell face or the 1e-4 on-node tolerance: the map has a kink there."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import source_reference as SR  # noqa: E402
from test_tangent import DOT_TOL, DX, MN, N, NN3, STEP, TOL, model  # noqa: E402  (grid, model, step and bounds of the tangent's tests)

SRC_SYMBOLS = ["ttcr_fsm_adjoint_points", "ttcr_fsm_adjoint_jvp_source", "ttcr_fsm_adjoint_vjp_source"]


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


# ---- (c) interface
def test_source_symbols_exported_and_declared(lib):
    from ttcr_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ttcr_amd.h")).read()
    pxd = open(os.path.join(ROOT, "integration", "ttcr_amd.pxd")).read()
    for name in SRC_SYMBOLS:
        assert name + "(" in hdr, name
        assert name + "(" in pxd, name
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name) is not None


def test_bad_arguments_are_value_errors_before_the_device(lib):
    from ttcr_amd import _lib

    buf = (C.c_double * 16)()
    n = C.c_size_t(0)
    fake = C.c_void_p(1234)   # never dereferenced: the argument checks come first
    assert lib.ttcr_fsm_adjoint_points(None, C.byref(n), None) == _lib.ERR_VALUE
    assert "null tape" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_points(fake, None, None) == _lib.ERR_VALUE
    assert "null n_points" in _lib.last_error()
    jvp = lib.ttcr_fsm_adjoint_jvp_source
    assert jvp(None, buf, 0, 1, buf, 0, None, 0, 0, None) == _lib.ERR_VALUE
    assert "null tape" in _lib.last_error()
    assert jvp(fake, None, 0, 1, buf, 0, None, 0, 0, None) == _lib.ERR_VALUE
    assert "null dsrc" in _lib.last_error()
    assert jvp(fake, buf, 0, 1, None, 0, None, 0, 0, None) == _lib.ERR_VALUE   # dtt and dfields both NULL
    assert "both" in _lib.last_error()
    for bad in (0, 5, -1):
        assert jvp(fake, buf, 0, bad, buf, 0, None, 0, 0, None) == _lib.ERR_VALUE
        assert "n_cols" in _lib.last_error()
    assert jvp(fake, buf, 0, 4, buf, 0, None, 0, 2, None) == _lib.ERR_VALUE    # unknown schedule
    assert "schedule" in _lib.last_error()
    vjp = lib.ttcr_fsm_adjoint_vjp_source
    assert vjp(None, buf, 0, None, 0, buf, 0, buf, 0, 0, None) == _lib.ERR_VALUE
    assert "null tape" in _lib.last_error()
    assert vjp(fake, buf, 0, None, 0, None, 0, None, 0, 0, None) == _lib.ERR_VALUE
    assert "null gsrc" in _lib.last_error()
    assert vjp(fake, None, 0, None, 0, None, 0, buf, 0, 0, None) == _lib.ERR_VALUE   # w and field_cot both NULL
    assert "both" in _lib.last_error()
    assert vjp(fake, buf, 0, None, 0, None, 0, buf, 0, -1, None) == _lib.ERR_VALUE
    assert "schedule" in _lib.last_error()


def test_python_layer_without_a_device():
    code = ("import sys, inspect, ttcr_amd; assert 'torch' not in sys.modules; "
            "import ttcr_amd.autograd as ag; assert 'torch' not in sys.modules; "
            "assert callable(ag.raytrace_events) and callable(ag.raytrace_adjoint); "
            "from ttcr_amd.rgrid import FieldTape; "
            "assert all(callable(getattr(FieldTape, a, None)) for a in ('jvp_source', 'source_jacobian', 'vjp', 'jvp')); "
            "assert 'return_source_grad' in inspect.signature(FieldTape.vjp).parameters; "
            "assert inspect.signature(FieldTape.vjp).parameters['return_source_grad'].default is False; "
            "assert 'torch' not in sys.modules")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ---- (a), (b) the definition against the oracle
CASES = {
    "off_node": ([[3.3, 4.1, 5.7]], "smooth"),
    "two_points": ([[3.3, 4.1, 5.7], [3.6, 4.2, 5.4]], "smooth"),   # the boxes overlap: the last writer wins
    "rough": ([[6.2, 2.9, 4.4]], "rough"),
    "near_face": ([[3.02, 4.1, 5.7]], "smooth"),                    # 0.02 from a cell face
    "on_node": ([[4.0, 5.5, 3.0]], "smooth"),
}


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
    gfield = rng.standard_normal(N ** 3)
    t0 = rng.uniform(0, 0.5, src.shape[0]).round(3)
    dsrc = rng.standard_normal((src.shape[0], 4))
    return src, t0, s, rcv, w, gfield, dsrc


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_is_the_directional_derivative_of_the_oracle(case):
    src, t0, s, rcv, w, gfield, dsrc = _setup(case)
    o = _solve(s, src, t0, rcv)
    mus, dtts = SR.source_tangent([o["tt"]], s, DX, NN3, MN, [src], dsrc, rcvs=[rcv])
    op = _solve(s, src + STEP * dsrc[:, 1:], t0 + STEP * dsrc[:, 0], rcv)
    om = _solve(s, src - STEP * dsrc[:, 1:], t0 - STEP * dsrc[:, 0], rcv)
    fd_fld = (op["tt"] - om["tt"]) / (2 * STEP)
    fd_rcv = (op["tt_rcv"] - om["tt_rcv"]) / (2 * STEP)
    e_fld = np.linalg.norm(mus[0] - fd_fld) / np.linalg.norm(fd_fld)
    e_rcv = np.linalg.norm(dtts[0] - fd_rcv) / np.linalg.norm(fd_rcv)
    print("source tangent vs oracle finite differences, %s: field %.2e, receivers %.2e (bound %.0e)" % (case, e_fld, e_rcv, TOL))
    assert e_fld <= TOL and e_rcv <= TOL, (e_fld, e_rcv)
    # the origin-time column alone: every node moves with t0, exactly
    only_t0 = np.zeros_like(dsrc)
    only_t0[:, 0] = 1
    mu1 = SR.source_tangent([o["tt"]], s, DX, NN3, MN, [src], only_t0)[0][0]
    assert np.array_equal(mu1, np.ones_like(mu1))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", list(CASES))
def test_dot_product_identity_of_forward_and_reverse(case, dt):
    src, t0, s, rcv, w, gfield, dsrc = _setup(case)
    o = _solve(s.astype(dt), src.astype(dt), t0.astype(dt), rcv.astype(dt), dt)
    s, dsrc, w, gfield = s.astype(dt), dsrc.astype(dt), w.astype(dt), gfield.astype(dt)
    mus, dtts = SR.source_tangent([o["tt"]], s, DX, NN3, MN, [src], dsrc, rcvs=[rcv])
    grad, gsrc = SR.source_adjoint([o["tt"]], s, DX, NN3, MN, [src], rcvs=[rcv], ws=[w], field_cot=[gfield])
    assert gsrc.shape == dsrc.shape and gsrc.dtype == dt
    f8 = lambda a: np.asarray(a, dtype=np.float64).ravel()   # noqa: E731
    lhs = f8(w) @ f8(dtts[0]) + f8(gfield) @ f8(mus[0])
    rhs = f8(gsrc) @ f8(dsrc)
    err = abs(lhs - rhs) / abs(rhs)
    print("<w, J_src v> + <gfield, mu> against <J_src^T (w, gfield), v>, %s, %s: %.2e (bound %.0e)"
          % (case, np.dtype(dt).name, err, DOT_TOL[dt]))
    assert err <= DOT_TOL[dt], (lhs, rhs, err)
