"""The M tape without a device: the C ABI of ttcr_fsm_raytrace_multi_tape and its companions is exported and declared, argument errors
come back before any device call, and the Python layer (Grid3d.raytrace_tape, ttcr_amd.autograd) is importable without torch being
loaded by `import ttcr_amd`."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPE_SYMBOLS = ["ttcr_fsm_raytrace_multi_tape", "ttcr_fsm_tape_size", "ttcr_fsm_tape_bytes", "ttcr_fsm_tape_device",
                "ttcr_fsm_tape_get_csr", "ttcr_fsm_tape_vjp", "ttcr_fsm_tape_free"]


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def test_tape_symbols_exported_and_declared(lib):
    from ttcr_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ttcr_amd.h")).read()
    assert "typedef struct ttcr_fsm_tape ttcr_fsm_tape;" in hdr
    for name in TAPE_SYMBOLS:
        assert name + "(" in hdr, name
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name) is not None


def test_null_tape_is_a_value_error_before_the_device(lib):
    from ttcr_amd import _lib

    n = C.c_size_t(0)
    d = C.c_int(0)
    buf = (C.c_double * 4)()
    assert lib.ttcr_fsm_tape_vjp(None, buf, 0, buf, 0) == _lib.ERR_VALUE
    assert "null" in _lib.last_error()
    assert lib.ttcr_fsm_tape_size(None, C.byref(n), C.byref(n), C.byref(n)) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_tape_get_csr(None, buf, buf, buf) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_tape_bytes(None, C.byref(n)) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_tape_device(None, C.byref(d)) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_tape_free(None) == _lib.OK
    # no place for the tape: refused before the grid (here a null handle) is looked at
    assert lib.ttcr_fsm_raytrace_multi_tape(None, 0, None, None, None, None, None, None, None) == _lib.ERR_VALUE
    assert "tape" in _lib.last_error()
    h = C.c_void_p(1234)
    assert lib.ttcr_fsm_raytrace_multi_tape(None, 0, None, None, None, None, None, None, C.byref(h)) == _lib.ERR_VALUE
    assert h.value is None   # (*tape is cleared first)


def test_python_layer_without_a_device():
    code = ("import sys, ttcr_amd; assert 'torch' not in sys.modules; "
            "import ttcr_amd.autograd as ag; assert 'torch' not in sys.modules; "
            "from ttcr_amd.rgrid import MTape, _Grid3d; assert callable(ag.raytrace) and hasattr(_Grid3d, 'raytrace_tape'); "
            "assert hasattr(MTape, 'vjp') and hasattr(MTape, 'to_csr') and hasattr(MTape, 'free')")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)
