"""The second-order products of the field tape without a device: the definition (tests/hessian_reference.py, the numpy restatement the
device is compared with bit for bit) is the directional derivative of the adjoint-state gradient -- central finite differences of
tests/adjoint_reference.py on oracle fields converge to it as the step shrinks --, it is symmetric (<u, H v> = <v, H u> to rounding),
and the Newton product is the composition it is defined as; the four C entry points are exported and declared, refuse bad arguments
before any device call, and the Python layer has the methods without importing torch."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_reference as AR  # noqa: E402
import hessian_reference as HR  # noqa: E402
import tangent_reference as TR  # noqa: E402

HESS_SYMBOLS = ["ttcr_fsm_adjoint_hold", "ttcr_fsm_adjoint_release", "ttcr_fsm_adjoint_hvp", "ttcr_fsm_adjoint_newton"]


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def test_hessian_symbols_exported_and_declared(lib):
    from ttcr_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ttcr_amd.h")).read()
    pxd = open(os.path.join(ROOT, "integration", "ttcr_amd.pxd")).read()
    for name in HESS_SYMBOLS:
        assert name + "(" in hdr, name
        assert name + "(" in pxd, name
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name) is not None


def test_null_and_misuse_arguments_are_value_errors_before_the_device(lib):
    from ttcr_amd import _lib

    buf = (C.c_double * 4)()
    fake = C.c_void_p(1234)   # never dereferenced: the argument checks come first
    assert lib.ttcr_fsm_adjoint_hold(None, buf, 0, None, 0, None, 0, 0, None) == _lib.ERR_VALUE
    assert "null tape" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_hold(fake, None, 0, None, 0, None, 0, 0, None) == _lib.ERR_VALUE   # w and field_cot both NULL
    assert "both" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_hold(fake, buf, 0, None, 0, None, 0, 2, None) == _lib.ERR_VALUE    # unknown schedule
    assert "schedule" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_release(None) == _lib.ERR_VALUE
    assert "null tape" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_hvp(None, buf, 0, buf, 0, 0, None, None) == _lib.ERR_VALUE
    assert "null tape" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_hvp(fake, None, 0, buf, 0, 0, None, None) == _lib.ERR_VALUE
    assert "null v" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_hvp(fake, buf, 0, None, 0, 0, None, None) == _lib.ERR_VALUE
    assert "null out" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_hvp(fake, buf, 0, buf, 0, 3, None, None) == _lib.ERR_VALUE
    assert "schedule" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_newton(None, buf, 0, None, 0, buf, 0, 0, None, None) == _lib.ERR_VALUE
    assert "null tape" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_newton(fake, None, 0, None, 0, buf, 0, 0, None, None) == _lib.ERR_VALUE
    assert "null v" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_newton(fake, buf, 0, None, 0, None, 0, 0, None, None) == _lib.ERR_VALUE
    assert "null out" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_newton(fake, buf, 0, None, 0, buf, 0, -1, None, None) == _lib.ERR_VALUE
    assert "schedule" in _lib.last_error()


def test_python_layer_without_a_device():
    code = ("import sys, ttcr_amd; assert 'torch' not in sys.modules; "
            "import ttcr_amd.autograd as ag; assert 'torch' not in sys.modules; "
            "from ttcr_amd.rgrid import FieldTape; "
            "assert all(callable(getattr(FieldTape, a, None)) for a in ('hold', 'release', 'hvp', 'newton')); "
            "assert 'torch' not in sys.modules")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ---- the definition against finite differences of the restated gradient on oracle fields: model, cases, grid of tests/test_adjoint.py
N = 21
DX = 0.5
NN3 = (N, N, N)
MN = (0.0, 0.0, 0.0)
STEPS = (1e-5, 1e-6)
# Bounds at step 1e-6: ten times the worst figure the restatement measures over the four cases and the two losses (a wrong coupling
# shows as 1e-3 or more; rounding in the differenced gradients moves the figure severalfold between cases).
FD_MEASURED = 1.84e-9     # worst relative L2 error of H v at step 1e-6 (on_node, field loss); 6.1e-10 to 1.84e-9 over the eight
FD_TOL = 10 * FD_MEASURED
SYM_MEASURED = 1.44e-14   # worst relative |<u, H v> - <v, H u>| (two_points, receiver loss); the other seven are below 1e-15
SYM_TOL = 10 * SYM_MEASURED


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
LOSSES = ("receivers", "field")


@functools.lru_cache(maxsize=None)
def _setup(case):
    """inputs and the oracle field of a case, computed once and shared (read-only) by the tests"""
    src, kind = CASES[case]
    src = np.array(src)
    s = model(kind)
    rng = np.random.default_rng(5)
    rcv = rng.uniform(0.6, (N - 1) * DX - 0.6, (30, 3))
    w = rng.standard_normal(30)
    gfield = rng.standard_normal(N ** 3)
    v = s * rng.standard_normal(s.size)
    u = s * rng.standard_normal(s.size)
    T = solve(s, src, rcv)["tt"]
    for a in (s, rcv, w, gfield, v, u, T):
        a.setflags(write=False)
    return src, s, rcv, w, gfield, v, u, T


def _cot(loss, rcv, w, gfield):
    return dict(rcvs=[rcv], ws=[w]) if loss == "receivers" else dict(field_cot=[gfield])


def _gradient(s, src, rcv, cot):
    return AR.adjoint([solve(s, src, rcv)["tt"]], s, DX, NN3, MN, [src], **cot)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_is_the_directional_derivative_of_the_restated_gradient(case, loss):
    src, s, rcv, w, gfield, v, u, T = _setup(case)
    cot = _cot(loss, rcv, w, gfield)
    hv = HR.hvp([T], s, DX, NN3, MN, [src], v, **cot)
    grad = AR.adjoint([T], s, DX, NN3, MN, [src], **cot)
    errs = []
    for h in STEPS:
        fd = (_gradient(s + h * v, src, rcv, cot) - _gradient(s - h * v, src, rcv, cot)) / (2 * h)
        errs.append(np.linalg.norm(hv - fd) / np.linalg.norm(fd))
    print("H v vs finite differences of the restated gradient, %s, %s loss: %.2e at step %.0e, %.2e at step %.0e (bound %.1e); "
          "|H v| / |grad| = %.2f" % (case, loss, errs[0], STEPS[0], errs[1], STEPS[1], FD_TOL,
                                     np.linalg.norm(hv) / np.linalg.norm(grad)))
    assert errs[1] < errs[0], errs        # the error falls with the step: H v is the derivative, not something near it
    assert errs[1] <= FD_TOL, errs


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_is_symmetric(case, loss):
    src, s, rcv, w, gfield, v, u, T = _setup(case)
    cot = _cot(loss, rcv, w, gfield)
    hv = HR.hvp([T], s, DX, NN3, MN, [src], v, **cot)
    hu = HR.hvp([T], s, DX, NN3, MN, [src], u, **cot)
    a, b = float(u @ hv), float(v @ hu)
    e = abs(a - b) / max(abs(a), abs(b))
    print("<u, H v> against <v, H u>, %s, %s loss: %.2e (bound %.1e)" % (case, loss, e, SYM_TOL))
    assert e <= SYM_TOL, (a, b)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", ["off_node", "two_points"])
def test_newton_is_the_composition(case, dt):
    """newton(v, W) == adjoint(seeds: q as the field cotangent, rows W . J v) + r, bit for bit, and differs from hvp(v) by the
    Gauss-Newton product to rounding"""
    src, s, rcv, w, gfield, v, u, T = _setup(case)
    dt = np.dtype(dt)
    s, w, v, T = s.astype(dt), w.astype(dt), v.astype(dt), T.astype(dt)
    W = np.random.default_rng(7).uniform(0.5, 2.0, rcv.shape[0]).astype(dt)
    fr = AR.frozen_nodes(dt, NN3, DX, MN, src)
    nt = HR.newton([T], s, DX, NN3, MN, [src], v, [rcv], ws=[w], row_weights=[W])
    out_h, lam, q, r, _ = HR.product_event(T, s, DX, NN3, MN, fr, rcv, w, None, v)
    mu = TR.tangent_event(T, s, DX, NN3, fr, v)
    rows = (W * TR.rows(dt, NN3, DX, MN, rcv, mu)).astype(dt)
    comp = AR.adjoint_event(T, s, DX, NN3, fr, AR.seeds(dt, NN3, DX, MN, rcv, rows, q))[1]
    fz = np.zeros(T.size, dtype=bool)
    fz[list(fr)] = True
    comp[~fz] = (comp[~fz] + r[~fz]).astype(dt)
    assert np.array_equal(nt.view(np.uint8), comp.view(np.uint8))
    gn = AR.adjoint_event(T, s, DX, NN3, fr, AR.seeds(dt, NN3, DX, MN, rcv, rows))[1]
    f8 = lambda a: np.asarray(a, dtype=np.float64)   # noqa: E731
    e = np.linalg.norm(f8(nt) - (f8(gn) + f8(out_h))) / np.linalg.norm(f8(nt))
    assert e <= (1e-12 if dt == np.float64 else 1e-4), e   # (linearity of the relaxation in its seeds, to the rounding of the dtype)
