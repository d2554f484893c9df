"""The forward mode of the field tape without a device: the definition (tests/tangent_reference.py, the numpy restatement the device is
compared with bit for bit) is the directional derivative of what the reference's scheme computes -- central finite differences of the
oracle agree with it to 1e-6 relative, over the whole field and at the receivers -- and it is the transpose of the adjoint restatement
(dot-product identity, to rounding); the two C entry points are exported and declared, refuse bad arguments before any device call, and
the Python layer has the methods without importing torch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_reference as AR  # noqa: E402
import tangent_reference as TR  # noqa: E402

TAN_SYMBOLS = ["ttcr_fsm_adjoint_jvp", "ttcr_fsm_adjoint_gn"]


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def test_tangent_symbols_exported_and_declared(lib):
    from ttcr_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ttcr_amd.h")).read()
    pxd = open(os.path.join(ROOT, "integration", "ttcr_amd.pxd")).read()
    for name in TAN_SYMBOLS:
        assert name + "(" in hdr, name
        assert name + "(" in pxd, name
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name) is not None


def test_null_arguments_are_value_errors_before_the_device(lib):
    from ttcr_amd import _lib

    buf = (C.c_double * 4)()
    fake = C.c_void_p(1234)   # never dereferenced: the argument checks come first
    assert lib.ttcr_fsm_adjoint_jvp(None, buf, 0, buf, 0, None, 0, 0, None) == _lib.ERR_VALUE
    assert "null tape" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_jvp(fake, None, 0, buf, 0, None, 0, 0, None) == _lib.ERR_VALUE
    assert "null ds" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_jvp(fake, buf, 0, None, 0, None, 0, 0, None) == _lib.ERR_VALUE   # dtt and dfields both NULL
    assert "both" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_jvp(fake, buf, 0, buf, 0, None, 0, 2, None) == _lib.ERR_VALUE    # unknown schedule
    assert "schedule" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_gn(None, buf, 0, None, 0, buf, 0, 0, None, None) == _lib.ERR_VALUE
    assert "null tape" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_gn(fake, None, 0, None, 0, buf, 0, 0, None, None) == _lib.ERR_VALUE
    assert "null" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_gn(fake, buf, 0, None, 0, None, 0, 0, None, None) == _lib.ERR_VALUE
    assert "null" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_gn(fake, buf, 0, None, 0, buf, 0, -1, None, None) == _lib.ERR_VALUE
    assert "schedule" in _lib.last_error()


def test_python_layer_without_a_device():
    code = ("import sys, ttcr_amd; assert 'torch' not in sys.modules; "
            "import ttcr_amd.autograd as ag; assert 'torch' not in sys.modules; "
            "from ttcr_amd.rgrid import FieldTape; "
            "assert all(callable(getattr(FieldTape, a, None)) for a in ('jvp', 'gauss_newton', 'vjp')); "
            "assert 'torch' not in sys.modules")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ---- the definition against the oracle: model, cases, grid and step of tests/test_adjoint.py, restated
N = 21
DX = 0.5
NN3 = (N, N, N)
MN = (0.0, 0.0, 0.0)
TOL = 1e-6    # the project's bound for finite differences; the prototype measured <= 3.2e-9, a wrong coupling shows as 1e-3 or more
STEP = 1e-6
DOT_TOL = {np.float64: 1e-12, np.float32: 5e-5}   # set by the issue (measured on the CPU: 2.4e-14 and 4.8e-6)


def model(kind):
    x = np.arange(N) * DX
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    s = 0.5 + 0.02 * X + 0.015 * Y + 0.03 * Z + 0.05 * np.sin(0.9 * X) * np.cos(0.7 * Y + 0.3 * Z)
    if kind == "rough":
        s = s * (1.0 + 0.15 * np.random.default_rng(11).uniform(-1, 1, s.shape))
    return s.flatten("F")


def solve(s, src, rcv, dt=np.float64):
    from oracle import oracle as O

    o = O.solve3d(dt, (N - 1,) * 3, DX, MN, s, src, rcv=rcv, eps=1e-15, maxit=200)
    assert o["niter"] < 200 and o["change"][-1] == 0, (o["niter"], o["change"][-3:])
    return o


CASES = {
    "off_node": ([[3.3, 4.1, 5.7]], "smooth"),
    "on_node": ([[4.0, 5.5, 3.0]], "smooth"),
    "two_points": ([[3.3, 4.1, 5.7], [3.6, 4.2, 5.4]], "smooth"),
    "rough": ([[6.2, 2.9, 4.4]], "rough"),
}


def _setup(case):
    src, kind = CASES[case]
    src = np.array(src)
    s = model(kind)
    rng = np.random.default_rng(5)
    rcv = rng.uniform(0.6, (N - 1) * DX - 0.6, (30, 3))
    w = rng.standard_normal(30)
    gfield = rng.standard_normal(N ** 3)
    ds = s * rng.standard_normal(s.size)
    return src, s, rcv, w, gfield, ds


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_is_the_directional_derivative_of_the_oracle(case):
    src, s, rcv, w, gfield, ds = _setup(case)
    o = solve(s, src, rcv)
    mus, dtts = TR.tangent([o["tt"]], s, DX, NN3, MN, [src], ds, rcvs=[rcv])
    op, om = solve(s + STEP * ds, src, rcv), solve(s - STEP * ds, src, rcv)
    fd_fld = (op["tt"] - om["tt"]) / (2 * STEP)
    fd_rcv = (op["tt_rcv"] - om["tt_rcv"]) / (2 * STEP)
    e_fld = np.linalg.norm(mus[0] - fd_fld) / np.linalg.norm(fd_fld)
    e_rcv = np.linalg.norm(dtts[0] - fd_rcv) / np.linalg.norm(fd_rcv)
    print("tangent vs oracle finite differences, %s: field %.2e, receivers %.2e (bound %.0e)" % (case, e_fld, e_rcv, TOL))
    assert e_fld <= TOL and e_rcv <= TOL, (e_fld, e_rcv)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_dot_product_identity_with_the_adjoint_restatement(case, dt):
    src, s, rcv, w, gfield, ds = _setup(case)
    o = solve(s.astype(dt), src.astype(dt), rcv.astype(dt), dt)
    s, ds, w, gfield = s.astype(dt), ds.astype(dt), w.astype(dt), gfield.astype(dt)
    mus, dtts = TR.tangent([o["tt"]], s, DX, NN3, MN, [src], ds, rcvs=[rcv])
    g_rcv = AR.adjoint([o["tt"]], s, DX, NN3, MN, [src], rcvs=[rcv], ws=[w])
    g_fld = AR.adjoint([o["tt"]], s, DX, NN3, MN, [src], field_cot=[gfield])
    f8 = lambda a: np.asarray(a, dtype=np.float64)   # noqa: E731
    lhs_r, rhs_r = f8(w) @ f8(dtts[0]), f8(g_rcv) @ f8(ds)
    lhs_f, rhs_f = f8(gfield) @ f8(mus[0]), f8(g_fld) @ f8(ds)
    e_rcv = abs(lhs_r - rhs_r) / abs(rhs_r)
    e_fld = abs(lhs_f - rhs_f) / abs(rhs_f)
    print("<w, J v> against <J^T w, v>, %s, %s: receivers %.2e, field %.2e (bound %.0e)"
          % (case, np.dtype(dt).name, e_rcv, e_fld, DOT_TOL[dt]))
    assert e_rcv <= DOT_TOL[dt] and e_fld <= DOT_TOL[dt], (e_rcv, e_fld)
