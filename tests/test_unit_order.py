"""The ticket order of the whole-iteration sweep launch (ttcr_fsm_unit_order, ttcr_amd/csrc/fsm_unit_order.h), on the CPU.

The first-order 3-D kernels launch at most `persist_wgs` workgroups, and each takes work units (sweep direction d, patch) in ticket order
until none is left.  A workgroup spins on the progress words of the units its unit needs; with few resident workgroups that only ends if
every one of those units has a LOWER ticket -- it is then running or done.  The order promises exactly that, and nothing on a device
checks it: with one fresh workgroup per unit, all resident, any order works.

The dependency relation below is restated from what the KERNEL waits for (fsm_sweep_unit, ttcr_amd/csrc/fsm_kernels.h), not from the
function that builds the order:
  * up_j / up_k: the patches (TJ - 1, TK) and (TJ, TK - 1) of the same sweep (2-D: up_j only);
  * prev_sweep_counter (and the chasing units of the 2-D kernels, which follow the same patches): for d > 0 the patches of sweep d - 1,
    in ITS oriented partition, that own a column within 2 H of the unit's own columns -- the window clamped to the grid, and mirrored
    along an axis whose orientation differs between the two sweeps (3-D: J bit 1, K bit 2 of d; 2-D: J reversed for d = 1 and d = 2).
Every batch entry z draws the units in the same order (ticket = position * batch + z) and waits only for units of its own z, so the
positions of the list are all that matters.

Patch sizes are restated here as well: 3-D 16 x 16 columns (fp32), 16 x 8 (fp64); 2-D 64 x 1.
"""
import ctypes as C
import os

import numpy as np
import pytest

import few_workgroups_cases as fw

F32, F64 = 0, 1
PATCH = {(3, F32): (16, 16), (3, F64): (16, 8), (2, F32): (64, 1), (2, F64): (64, 1)}

# 3-D shapes, NODES (nx, ny, nz): x is the level axis, the patches tile (y, z)
SHAPES_3D = (
    [(5, 16, 8), (2, 16, 10)]                                   # one patch (fp64: (2, 16, 10) has two along z)
    + [(2, 40, 40), (40, 2, 40), (40, 40, 2), (16, 2, 10), (10, 16, 2), (2, 2, 2)]   # two nodes along each axis in turn
    + [s for s in fw.SHAPES if s != (2, 16, 10)]                # the shapes of tests/test_few_workgroups_gpu.py
    + [(9, 33, 17), (9, 31, 31), (9, 47, 23), (33, 17, 33)]      # remainders of 1 and of PJ - 1 / PK - 1 columns (15; 15 and 7)
    + [(20, 48, 32), (16, 16, 16)]                              # exact multiples
    + [(7, 64, 64), (7, 80, 80), (7, 64, 40), (7, 80, 32)]       # 4 and 5 patches along an axis (fp64: 8 / 10 / 5 / 4 along z)
    + [(512, 512, 512)]                                         # 32 x 32 patches, fp64 32 x 64
    + [(9, 32, 640), (9, 32, 320), (9, 640, 32)]                # long and thin: 2 x 40 (fp64: 2 x 80, 2 x 40), 40 x 2
    + [(17, 33, 34), (17, 34, 33), (41, 18, 5), (9, 49, 17)]    # the shapes of tests/test_weno_2d_gpu.py: last patches of 1 and 2 columns under H = 2
)
# 2-D shapes, NODES (nx, nz): z is the level axis, the patches tile x -- 1, 1, 2, 2, 3 and 65 patches; then the other 2-D shapes of
# tests/test_weno_2d_gpu.py: 3 patches (the last of 2 columns) and 2
SHAPES_2D = [(64, 30), (2, 40), (40, 2), (65, 130), (128, 9), (150, 70), (4097, 33), (130, 65), (66, 37)]


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def unit_order(lib, dim, dtype, stage, by_time, shape):
    from ttcr_amd import _lib

    nnx, nny, nnz = shape if dim == 3 else (shape[0], 0, shape[1])
    n = C.c_size_t(0)
    st = lib.ttcr_fsm_unit_order(dim, dtype, stage, by_time, nnx, nny, nnz, None, 0, C.byref(n))
    assert st == _lib.OK, _lib.last_error()
    out = np.full(n.value, 0xffffffff, dtype=np.uint32)
    st = lib.ttcr_fsm_unit_order(dim, dtype, stage, by_time, nnx, nny, nnz, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(n))
    assert st == _lib.OK and n.value == out.size, _lib.last_error()
    return out


def geometry(dim, dtype, shape):
    """(NJ, NK, PJ, PK, npj, npk, ndir) of the patch grid"""
    PJ, PK = PATCH[(dim, dtype)]
    NJ, NK = (shape[1], shape[2]) if dim == 3 else (shape[0], 1)
    return NJ, NK, PJ, PK, -(-NJ // PJ), -(-NK // PK), 8 if dim == 3 else 4


def flips(dim, d):
    """(J reversed, K reversed) in sweep d"""
    return ((d >> 1) & 1, (d >> 2) & 1) if dim == 3 else (int(d == 1) | int(d == 2), 0)


def _windows(N, P, H, mirrored):
    """per patch index along one axis: first and last patch index of the previous sweep that owns a column within 2 H of its columns"""
    t = np.arange(-(-N // P))
    lo, hi = t * P, np.minimum(t * P + P, N) - 1
    a, b = np.maximum(lo - 2 * H, 0), np.minimum(hi + 2 * H, N - 1)
    if mirrored:
        a, b = N - 1 - b, N - 1 - a
    return a // P, b // P


def violations(words, dim, dtype, stage, shape):
    """Everything wrong with a ticket order, as a list of strings (empty: the order is a permutation of all units in which every unit comes
    after the units the kernel makes it wait for)."""
    NJ, NK, PJ, PK, npj, npk, ndir = geometry(dim, dtype, shape)
    H = 1 if stage == 0 else 2
    words = np.asarray(words, dtype=np.uint32)
    TJ, TK, D = (words & 0x3fff).astype(np.int64), ((words >> 14) & 0x3fff).astype(np.int64), (words >> 28).astype(np.int64)
    bad = []
    if words.size != ndir * npj * npk:
        return ["%d words for %d units" % (words.size, ndir * npj * npk)]
    if np.any(TJ >= npj) or np.any(TK >= npk) or np.any(D >= ndir):
        return ["a word names a unit outside the launch"]
    pos = np.full((ndir, npk, npj), -1, dtype=np.int64)
    pos[D, TK, TJ] = np.arange(words.size)
    if np.any(pos < 0):
        return ["not a permutation: %d units never drawn" % int((pos < 0).sum())]

    def report(what, d, mask, dep_pos):
        for tk, tj in np.argwhere(mask)[:3]:
            bad.append("unit (d %d, TJ %d, TK %d) at %d waits for %s at %d" % (d, tj, tk, pos[d, tk, tj], what, dep_pos[tk, tj]))

    for d in range(ndir):
        me = pos[d]
        if npj > 1:   # up_j
            dep = np.full_like(me, -1)
            dep[:, 1:] = me[:, :-1]
            report("its upwind patch along J", d, dep > me, dep)
        if npk > 1:   # up_k
            dep = np.full_like(me, -1)
            dep[1:, :] = me[:-1, :]
            report("its upwind patch along K", d, dep > me, dep)
        if d == 0:
            continue
        (rj, rk), (prj, prk) = flips(dim, d), flips(dim, d - 1)
        ja, jb = _windows(NJ, PJ, H, rj != prj)
        ka, kb = _windows(NK, PK, H, rk != prk)
        assert np.all(jb - ja <= 3) and np.all(kb - ka <= 3)   # (the kernel has 4 x 4 lanes for them)
        prev = pos[d - 1]
        kk, jj = np.meshgrid(np.arange(npk), np.arange(npj), indexing="ij")
        for ib in range(int((kb - ka).max()) + 1):
            for ia in range(int((jb - ja).max()) + 1):
                tk, tj = ka[kk] + ib, ja[jj] + ia
                ok = (tk <= kb[kk]) & (tj <= jb[jj])
                dep = np.where(ok, prev[np.minimum(tk, npk - 1), np.minimum(tj, npj - 1)], -1)
                report("a patch of sweep %d" % (d - 1), d, dep > me, dep)
    return bad


CASES = [(3, s) for s in SHAPES_3D] + [(2, s) for s in SHAPES_2D]


@pytest.mark.parametrize("dim,shape", CASES, ids=["x".join(map(str, s)) for _, s in CASES])
def test_every_unit_comes_after_the_units_it_waits_for(lib, dim, shape):
    for dtype in (F32, F64):
        for stage in (0, 1):        # H = 1, H = 2
            for by_time in (0, 1):
                words = unit_order(lib, dim, dtype, stage, by_time, shape)
                bad = violations(words, dim, dtype, stage, shape)
                assert not bad, (shape, "fp64" if dtype else "fp32", "stage", stage, "by_time", by_time, bad[:5])


def test_patch_counts_are_the_ones_the_shapes_were_chosen_for(lib):
    counts = lambda dtype, s: geometry(3, dtype, s)[4:6]
    assert counts(F32, (37, 35, 41)) == (3, 3) and counts(F64, (37, 35, 41)) == (3, 6)
    assert counts(F32, (19, 50, 36)) == (4, 3) and counts(F64, (19, 50, 36)) == (4, 5)
    assert counts(F32, (70, 17, 9)) == (2, 1) and counts(F32, (2, 16, 10)) == (1, 1) and counts(F32, (5, 16, 8)) == counts(F64, (5, 16, 8)) == (1, 1)
    assert counts(F32, (512, 512, 512)) == (32, 32) and counts(F64, (512, 512, 512)) == (32, 64)
    assert counts(F32, (9, 32, 640)) == (2, 40) and counts(F64, (9, 32, 320)) == (2, 40)
    assert [geometry(2, F32, s)[4] for s in SHAPES_2D] == [1, 1, 1, 2, 2, 3, 65, 3, 2]
    assert counts(F32, (17, 33, 34)) == (3, 3) and counts(F64, (17, 33, 34)) == (3, 5) and counts(F64, (17, 34, 33)) == (3, 5)
    assert counts(F32, (41, 18, 5)) == counts(F64, (41, 18, 5)) == (2, 1) and counts(F32, (9, 49, 17)) == (4, 2) and counts(F64, (9, 49, 17)) == (4, 3)
    for dtype in (F32, F64):   # the list has one word per unit, whatever the order
        assert unit_order(lib, 3, dtype, 0, 1, (37, 35, 41)).size == 8 * int(np.prod(counts(dtype, (37, 35, 41))))
    assert unit_order(lib, 2, F32, 0, 1, (4097, 33)).size == 4 * 65


def test_sweep_by_sweep_order_is_direction_major(lib):
    """by_time = 0: all of sweep d before any of sweep d + 1, anti-diagonals TJ + TK ascending inside a sweep"""
    w = unit_order(lib, 3, F32, 0, 0, (19, 50, 36))
    d, m = (w >> 28).astype(int), ((w & 0x3fff) + ((w >> 14) & 0x3fff)).astype(int)
    assert np.all(np.diff(d) >= 0)
    assert all(np.all(np.diff(m[d == q]) >= 0) for q in range(8))
    # by start time the sweeps overlap: some unit of sweep d + 1 is drawn before the last one of sweep d
    assert np.any(np.diff((unit_order(lib, 3, F32, 0, 1, (19, 50, 36)) >> 28).astype(int)) < 0)


@pytest.mark.parametrize("dim,dtype,stage,shape", [(3, F32, 0, (37, 35, 41)), (3, F64, 1, (37, 35, 41)), (2, F32, 0, (150, 70))])
def test_the_checker_rejects_an_order_with_two_dependent_units_swapped(lib, dim, dtype, stage, shape):
    """negative control: exchange a unit with one it waits for -- its upwind patch, then a patch of the previous sweep"""
    NJ, NK, PJ, PK, npj, npk, ndir = geometry(dim, dtype, shape)
    for by_time in (0, 1):
        words = unit_order(lib, dim, dtype, stage, by_time, shape)
        assert not violations(words, dim, dtype, stage, shape)
        word = lambda d, tj, tk: np.uint32(tj | (tk << 14) | (d << 28))
        tk = 1 if dim == 3 else 0
        # the interior patch and its upwind neighbour along J; the interior patch of sweep 3 and the same patch of sweep 2
        # (it owns the columns themselves, whichever way the partition is mirrored: 3 x 3 patches, 2-D 3 patches)
        for a, b in ((word(2, 1, tk), word(2, 0, tk)), (word(3, 1, tk), word(2, 1, tk))):
            w = words.copy()
            ia, ib = int(np.flatnonzero(w == a)[0]), int(np.flatnonzero(w == b)[0])
            assert ib < ia
            w[ia], w[ib] = w[ib], w[ia]
            bad = violations(w, dim, dtype, stage, shape)
            assert bad and any("waits for" in v for v in bad), (by_time, a, b)
        # a unit drawn twice (and another never) is no permutation
        w = words.copy()
        w[3] = w[4]
        assert any("not a permutation" in v for v in violations(w, dim, dtype, stage, shape))
        assert violations(words[:-1], dim, dtype, stage, shape)


def test_the_order_is_the_parents(lib):
    """the words GridT::xs_order produced before its arithmetic moved into fsm_unit_order.h (tests/golden/unit_order_parent.npz: written
    by the parent's code for a few shapes, both precisions, both stages, both orders)"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unit_order_parent.npz"))
    assert len(g.files) >= 40
    for key in g.files:
        dim, dtype, stage, by_time, *shape = (int(v) for v in key.split("_"))
        np.testing.assert_array_equal(unit_order(lib, dim, dtype, stage, by_time, tuple(shape)), g[key], err_msg=key)


def test_arguments_are_validated_and_no_device_is_needed(lib):
    from ttcr_amd import _lib

    n = C.c_size_t(0)
    buf = (C.c_uint32 * 8)()
    call = lambda *a: lib.ttcr_fsm_unit_order(*a)
    assert call(4, F32, 0, 1, 37, 35, 41, None, 0, C.byref(n)) == _lib.ERR_VALUE
    assert call(3, 2, 0, 1, 37, 35, 41, None, 0, C.byref(n)) == _lib.ERR_VALUE
    assert call(3, F32, 2, 1, 37, 35, 41, None, 0, C.byref(n)) == _lib.ERR_VALUE
    assert call(3, F32, 0, 1, 37, 1, 41, None, 0, C.byref(n)) == _lib.ERR_VALUE
    assert call(3, F32, 0, 1, 37, 35, 41, None, 0, None) == _lib.ERR_VALUE
    assert call(3, F32, 0, 1, 37, 16 << 14, 41, None, 0, C.byref(n)) == _lib.ERR_VALUE and "too large" in _lib.last_error()
    # too small a buffer: an error, and nothing written
    assert call(3, F32, 0, 1, 37, 35, 41, buf, 8, C.byref(n)) == _lib.ERR_VALUE and n.value == 72
    assert list(buf) == [0] * 8
    # (2-D: the y count is ignored)
    assert call(2, F64, 1, 0, 150, 0, 70, None, 0, C.byref(n)) == _lib.OK and n.value == 12
