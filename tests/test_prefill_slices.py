"""The slices of the spare traveltime fields that the units of a sweep launch fill (ttcr_fsm_prefill_slice,
ttcr_amd/csrc/fsm_prefill_slices.h; option "prefill_inline"), on the CPU.

Every unit of the call's first sweep launch sets slice `ticket` of the spare field set to max() as it draws its ticket.  Every ticket of a
launch is drawn exactly once whatever the number of resident workgroups, so the set is initialised completely if and only if the slices of
tickets 0 .. n_tickets - 1 tile [0, n_el) -- which nothing on a device checks node by node but the far-apart sources of
tests/test_inline_prefill_gpu.py.  Checked here for the C entry, which calls the functions the kernel calls:
  * the slices follow each other in ticket order from 0 to n_el without gap or overlap (the tail included: the last non-empty slice ends
    at n_el whether or not n_el is a multiple of n_tickets x vector);
  * every slice starts on a 16-byte boundary (4 fp32 / 2 fp64 elements) and only the one that ends at n_el may hold a partial vector;
  * tickets at or beyond the unit count -- the draws that tell a workgroup the launch is over -- cover nothing.
"""
import ctypes as C

import numpy as np
import pytest

import few_workgroups_cases as fw

F32, F64 = 0, 1
VEC = {F32: 4, F64: 2}
# the grids of tests/test_inline_prefill_gpu.py: nodes per field, and the fields of a set as the library pads them -- 3 slots in the pair
# layout take 4 fields, a lone slot one
NODES = [int(np.prod(s)) for s in (fw.SHAPES[0], fw.SHAPES[2], fw.SHAPES[3])] + [70 * 45, 21 ** 3]
PADDED = sorted({n * f for n in NODES for f in (1, 3, 4)})
COUNTS = [1, 7, 4096] + PADDED
TICKETS = [8, 72, 1024]


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def slices(lib, dtype, n_el, n_tickets, tickets):
    from ttcr_amd import _lib

    out = []
    ln, b, e = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    for t in tickets:
        st = lib.ttcr_fsm_prefill_slice(dtype, n_el, n_tickets, t, C.byref(ln), C.byref(b), C.byref(e))
        assert st == _lib.OK, _lib.last_error()
        out.append((ln.value, b.value, e.value))
    return out


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n_tickets", TICKETS)
@pytest.mark.parametrize("n_el", COUNTS)
def test_slices_tile_the_element_range(lib, dtype, n_tickets, n_el):
    vec = VEC[dtype]
    sl = slices(lib, dtype, n_el, n_tickets, range(n_tickets))
    length = sl[0][0]
    assert length > 0 and length % vec == 0 and all(s[0] == length for s in sl)
    assert length * n_tickets >= n_el and (length - vec) * n_tickets < n_el   # (the smallest whole-vector slice that reaches)
    pos = 0
    for t, (_, b, e) in enumerate(sl):
        assert b == pos and b <= e <= n_el, (t, b, e, pos)
        assert (b % vec == 0 or b == e) and e - b <= length, (t, b, e)   # (an empty slice sits at n_el)
        assert (e - b) % vec == 0 or e == n_el, (t, b, e)
        assert e - b == length or e == n_el, (t, b, e)   # (short only where the range ends)
        pos = e
    assert pos == n_el
    # marked element by element where that is cheap: each exactly once
    if n_el <= 1 << 16:
        hits = np.zeros(n_el, dtype=np.int32)
        for _, b, e in sl:
            hits[b:e] += 1
        assert np.all(hits == 1)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n_tickets", TICKETS)
def test_tickets_beyond_the_unit_count_cover_nothing(lib, dtype, n_tickets):
    for n_el in (1, 7, 4096, PADDED[-1]):
        beyond = [n_tickets, n_tickets + 1, n_tickets + 2047, 2 * n_tickets + 5, 2 ** 31 - 1, 2 ** 32 - 1]
        for _, b, e in slices(lib, dtype, n_el, n_tickets, beyond):
            assert b == e == n_el


def test_a_large_set_and_bad_arguments(lib):
    """64 fields of 512^3 nodes over the 262 144 units of their launch: 128 KiB per unit, the products beyond 2^32 hold"""
    from ttcr_amd import _lib

    n_el, n_tickets = 64 * 512 ** 3, 1024 * 8 * 32
    (ln, b0, e0), (_, b1, e1), (_, b2, e2) = slices(lib, F32, n_el, n_tickets, [0, n_tickets - 1, n_tickets])
    assert ln == 32768 and (b0, e0) == (0, ln) and (b1, e1) == (n_el - ln, n_el) and b2 == e2 == n_el
    n_el += 3   # (not a multiple of the vector)
    ln = slices(lib, F32, n_el, n_tickets, [0])[0][0]
    last = (n_el - 1) // ln   # (whole vectors per slice: the range ends a little before the last ticket)
    (_, b1, e1), (_, b2, e2), (_, b3, e3) = slices(lib, F32, n_el, n_tickets, [last, last + 1, n_tickets - 1])
    assert ln == 32772 and last < n_tickets and (b1, e1) == (last * ln, n_el) and b2 == e2 == n_el and b3 == e3 == n_el
    assert lib.ttcr_fsm_prefill_slice(7, 16, 8, 0, None, None, None) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_prefill_slice(F32, 16, 0, 0, None, None, None) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_prefill_slice(F32, 16, 8, 0, None, None, None) == _lib.OK
