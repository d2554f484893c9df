"""The adjoint-state gradient without a device: the C ABI of ttcr_fsm_raytrace_multi_adjoint and its companions is exported and
declared, argument errors come back before any device call, the Python layer is importable without torch -- and the definition itself
(tests/adjoint_reference.py, the numpy restatement the device is compared with bit for bit) is the derivative of what the reference's
scheme computes: central finite differences of the oracle agree with it to 1e-6 relative."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_reference as AR  # noqa: E402

ADJ_SYMBOLS = ["ttcr_fsm_raytrace_multi_adjoint", "ttcr_fsm_adjoint_size", "ttcr_fsm_adjoint_bytes", "ttcr_fsm_adjoint_device",
               "ttcr_fsm_adjoint_get_field", "ttcr_fsm_adjoint_vjp", "ttcr_fsm_adjoint_free"]


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def test_adjoint_symbols_exported_and_declared(lib):
    from ttcr_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ttcr_amd.h")).read()
    assert "typedef struct ttcr_fsm_adjoint ttcr_fsm_adjoint;" in hdr
    pxd = open(os.path.join(ROOT, "integration", "ttcr_amd.pxd")).read()
    for name in ADJ_SYMBOLS:
        assert name + "(" in hdr, name
        assert name + "(" in pxd, name
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name) is not None


def test_null_arguments_are_value_errors_before_the_device(lib):
    from ttcr_amd import _lib

    n = C.c_size_t(0)
    d = C.c_int(0)
    buf = (C.c_double * 4)()
    fake = C.c_void_p(1234)   # never dereferenced: the argument checks come first
    assert lib.ttcr_fsm_adjoint_vjp(None, buf, 0, None, 0, buf, 0, 0, None) == _lib.ERR_VALUE
    assert "null" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_vjp(fake, None, 0, None, 0, buf, 0, 0, None) == _lib.ERR_VALUE   # w and field_cot both NULL
    assert "both" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_vjp(fake, buf, 0, None, 0, None, 0, 0, None) == _lib.ERR_VALUE   # no grad
    assert lib.ttcr_fsm_adjoint_vjp(fake, buf, 0, None, 0, buf, 0, 2, None) == _lib.ERR_VALUE    # unknown schedule
    assert "schedule" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_size(None, C.byref(n), C.byref(n), C.byref(n)) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_adjoint_size(fake, None, C.byref(n), C.byref(n)) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_adjoint_bytes(None, C.byref(n)) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_adjoint_device(None, C.byref(d)) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_adjoint_get_field(None, 0, buf) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_adjoint_get_field(fake, 0, None) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_adjoint_free(None) == _lib.OK
    assert lib.ttcr_fsm_raytrace_multi_adjoint(None, 0, None, None, None, None, None, None, None) == _lib.ERR_VALUE
    assert "tape" in _lib.last_error()
    h = C.c_void_p(1234)
    assert lib.ttcr_fsm_raytrace_multi_adjoint(None, 0, None, None, None, None, None, None, C.byref(h)) == _lib.ERR_VALUE
    assert h.value is None   # (*tape is cleared first)


def test_python_layer_without_a_device():
    code = ("import sys, ttcr_amd; assert 'torch' not in sys.modules; "
            "import ttcr_amd.autograd as ag; assert 'torch' not in sys.modules; "
            "from ttcr_amd.rgrid import FieldTape, _Grid3d; assert callable(ag.raytrace_adjoint) and hasattr(_Grid3d, 'raytrace_adjoint'); "
            "assert all(hasattr(FieldTape, a) for a in ('vjp', 'field', 'free'))")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ---- the definition against the oracle (fp64, 21^3 nodes, eps = 1e-15: the field is a fixed point of the sweeps)
N = 21
DX = 0.5
NN3 = (N, N, N)
MN = (0.0, 0.0, 0.0)
TOL = 1e-6    # set by the issue: the prototype measured <= 1.8e-8 for this step; a wrong coupling shows as 1e-3 or more
STEP = 1e-6


def model(kind):
    x = np.arange(N) * DX
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    s = 0.5 + 0.02 * X + 0.015 * Y + 0.03 * Z + 0.05 * np.sin(0.9 * X) * np.cos(0.7 * Y + 0.3 * Z)
    if kind == "rough":
        s = s * (1.0 + 0.15 * np.random.default_rng(11).uniform(-1, 1, s.shape))
    return s.flatten("F")


def solve(s, src, rcv):
    from oracle import oracle as O

    o = O.solve3d(np.float64, (N - 1,) * 3, DX, MN, s, src, rcv=rcv, eps=1e-15, maxit=200)
    assert o["niter"] < 200 and o["change"][-1] == 0, (o["niter"], o["change"][-3:])
    return o


CASES = {
    "off_node": ([[3.3, 4.1, 5.7]], "smooth"),
    "on_node": ([[4.0, 5.5, 3.0]], "smooth"),
    "two_points": ([[3.3, 4.1, 5.7], [3.6, 4.2, 5.4]], "smooth"),
    "rough": ([[6.2, 2.9, 4.4]], "rough"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_is_the_derivative_of_the_oracle(case):
    src, kind = CASES[case]
    src = np.array(src)
    s = model(kind)
    rng = np.random.default_rng(5)
    rcv = rng.uniform(0.6, (N - 1) * DX - 0.6, (30, 3))
    w = rng.standard_normal(30)
    gfield = rng.standard_normal(N ** 3)
    ds = s * rng.standard_normal(s.size)
    o = solve(s, src, rcv)
    # the frozen-node rule reproduces the oracle's frozen values
    for m, d in AR.frozen_nodes(np.float64, NN3, DX, MN, src).items():
        assert o["tt"][m] == d * s[m], (m, o["tt"][m], d * s[m])
    # the stencil reproduces the interpolated traveltimes (an 8-term sum re-associated)
    for r in range(len(rcv)):
        nodes, wts = AR.stencil(np.float64, NN3, DX, MN, rcv[r])
        assert abs(sum(wt * o["tt"][m] for m, wt in zip(nodes, wts)) - o["tt_rcv"][r]) <= 16 * np.spacing(o["tt_rcv"][r])
    g_rcv = AR.adjoint([o["tt"]], s, DX, NN3, MN, [src], rcvs=[rcv], ws=[w])
    g_fld = AR.adjoint([o["tt"]], s, DX, NN3, MN, [src], field_cot=[gfield])
    op, om = solve(s + STEP * ds, src, rcv), solve(s - STEP * ds, src, rcv)
    fd_rcv = (w @ op["tt_rcv"] - w @ om["tt_rcv"]) / (2 * STEP)
    fd_fld = (gfield @ op["tt"] - gfield @ om["tt"]) / (2 * STEP)
    e_rcv = abs(g_rcv @ ds - fd_rcv) / abs(fd_rcv)
    e_fld = abs(g_fld @ ds - fd_fld) / abs(fd_fld)
    print("adjoint vs oracle finite differences, %s: receivers %.2e, field %.2e (bound %.0e)" % (case, e_rcv, e_fld, TOL))
    assert e_rcv <= TOL and e_fld <= TOL, (e_rcv, e_fld)
