"""The block products of the field tape without a device: the four entries of the C ABI resolve, and every argument error
that can be told without a live tape returns TTCR_ERR_VALUE with a message of its own before any device call.  The entries check what
needs no tape first and the tape last, so with a NULL tape each error is reached by making everything checked before it valid."""
import ctypes as C

import numpy as np
import pytest

NAMES = ("ttcr_fsm_adjoint_jvp_block", "ttcr_fsm_adjoint_vjp_block", "ttcr_fsm_adjoint_gn_block", "ttcr_fsm_adjoint_block_release")


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def test_the_four_symbols_resolve(lib):
    from ttcr_amd import _lib

    for n in NAMES:
        assert n in _lib.SYMBOLS and getattr(lib, n) is not None


def _err(lib, status, *words):
    from ttcr_amd import _lib

    assert status == _lib.ERR_VALUE, status
    msg = _lib.last_error()
    assert msg and all(w in msg for w in words), msg


def test_argument_errors_come_before_the_device(lib):
    a = np.zeros(8, dtype=np.float32)
    p = a.ctypes.data_as(C.c_void_p)
    np_ = C.c_int(-7)
    jvp, vjp, gn = lib.ttcr_fsm_adjoint_jvp_block, lib.ttcr_fsm_adjoint_vjp_block, lib.ttcr_fsm_adjoint_gn_block
    # n_cols < 1
    for k in (0, -3):
        _err(lib, jvp(None, k, p, 0, p, 0, None, 0, 0, C.byref(np_)), "n_cols")
        _err(lib, vjp(None, k, p, 0, p, 0, 0, C.byref(np_)), "n_cols")
        _err(lib, gn(None, k, p, 0, None, 0, 0, p, 0, 0, None, None), "n_cols")
    # unknown schedule
    for sch in (2, -1):
        _err(lib, jvp(None, 2, p, 0, p, 0, None, 0, sch, C.byref(np_)), "schedule")
        _err(lib, vjp(None, 2, p, 0, p, 0, sch, C.byref(np_)), "schedule")
        _err(lib, gn(None, 2, p, 0, None, 0, 0, p, 0, sch, None, None), "schedule")
    # NULL input
    _err(lib, jvp(None, 2, None, 0, p, 0, None, 0, 0, C.byref(np_)), "null ds")
    _err(lib, vjp(None, 2, None, 0, p, 0, 0, C.byref(np_)), "null w")
    _err(lib, gn(None, 2, None, 0, None, 0, 0, p, 0, 0, None, None), "null v")
    # no output
    _err(lib, jvp(None, 2, p, 0, None, 0, None, 0, 0, C.byref(np_)), "dtt and dfields are both null")
    _err(lib, vjp(None, 2, p, 0, None, 0, 0, C.byref(np_)), "null grad")
    _err(lib, gn(None, 2, p, 0, None, 0, 0, None, 0, 0, None, None), "null out")
    # rw_cols not in {0, 1, n_cols}; a NULL row_weight that rw_cols says is there
    for rw_cols in (-1, 2, 4):
        _err(lib, gn(None, 3, p, 0, p, rw_cols, 0, p, 0, 0, None, None), "rw_cols")
    for rw_cols in (1, 3):
        _err(lib, gn(None, 3, p, 0, None, rw_cols, 0, p, 0, 0, None, None), "null row_weight")
    # NULL tape, everything else in order (rw_cols 0, 1 and n_cols)
    _err(lib, jvp(None, 2, p, 0, p, 0, None, 0, 0, C.byref(np_)), "null tape")
    _err(lib, jvp(None, 5, p, 0, None, 0, p, 0, 1, C.byref(np_)), "null tape")
    _err(lib, vjp(None, 2, p, 0, p, 0, 1, C.byref(np_)), "null tape")
    for rw, rw_cols in ((None, 0), (p, 1), (p, 3)):
        _err(lib, gn(None, 3, p, 0, rw, rw_cols, 0, p, 0, 0, None, None), "null tape")
    _err(lib, lib.ttcr_fsm_adjoint_block_release(None), "null tape")
    assert np_.value == -7   # (no call got as far as its outputs)
