"""The dirty bits a changed node sets for the next sweep (ttcr_fsm_chunk_dirty_marks, ttcr_amd/csrc/fsm_chunk_dirty.h), on the CPU.

The first-order 3-D sweep kernels with exact skipping evaluate a chunk (C levels of one unit's patch) only if it may hold a node with a
neighbour that changed since the node's last visit.  Changes of the sweep before arrive as bits, one per (unit, chunk) of the sweep that
reads them, set by the thread that changed the node with the function this entry calls.  Exactness needs one thing of that function: for
every node M and each of its six axis neighbours N, the bits of M hold the chunk of N's unit -- in the NEXT sweep's oriented partition
and chunk grid -- that evaluates N.  The reader's side is restated here from the kernel (fsm_sweep_unit, ttcr_amd/csrc/fsm_kernels.h):
  * direction dn has bits (F, J, K) = (dn & 1, dn >> 1 & 1, dn >> 2 & 1): an axis with its bit set is walked from its last index down;
  * unit (TJ, TK) owns the oriented columns j' in [TJ PJ, TJ PJ + PJ), k' in [TK PK, TK PK + PK);
  * its chunks start at lcf + ci C with lcf = Ls - ((Ls - (TJ + TK)) mod C), Ls = TJ PJ + TK PK, and node (i', j', k') sits at level
    i' + j' + k'.
Patch sizes: 16 x 16 columns (fp32), 16 x 8 (fp64).
"""
import ctypes as C

import numpy as np
import pytest

F32, F64 = 0, 1
PATCH = {F32: (16, 16), F64: (16, 8)}
# NODES (nx, ny, nz): x is the level axis, the patches tile (y, z).  (70, 53, 41): J and K no multiples of the patch, so the partitions
# of two sweeps that walk an axis in opposite directions differ.  (600, 35, 19) and (300, 20, 18): marks with chunk indices >= 32, on chunks
# of 8 and of 16 / of 8 (tests/long_axis_cases.py)
SHAPES = [(37, 35, 41), (70, 53, 41), (2, 16, 10), (17, 33, 34), (600, 35, 19), (300, 20, 18)]


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def marks(lib, dtype, chunk, d, edge_rule, shape):
    from ttcr_amd import _lib

    nnx, nny, nnz = shape
    out = np.full((nnz, nny, nnx, 3, 4), -7, dtype=np.int32)
    st = lib.ttcr_fsm_chunk_dirty_marks(dtype, chunk, d, edge_rule, nnx, nny, nnz, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size)
    assert st == _lib.OK, _lib.last_error()
    return out


def readers(dtype, chunk, dn, shape):
    """(TJ, TK, ci) of the unit and chunk of sweep dn that evaluates each node, arrays [k][j][i] in natural indices"""
    NF, NJ, NK = shape
    PJ, PK = PATCH[dtype]
    k, j, i = np.meshgrid(np.arange(NK), np.arange(NJ), np.arange(NF), indexing="ij")
    i2 = NF - 1 - i if dn & 1 else i
    j2 = NJ - 1 - j if (dn >> 1) & 1 else j
    k2 = NK - 1 - k if (dn >> 2) & 1 else k
    TJ, TK = j2 // PJ, k2 // PK
    Ls = TJ * PJ + TK * PK
    lcf = Ls - (Ls - (TJ + TK)) % chunk
    return TJ, TK, (i2 + j2 + k2 - lcf) // chunk


def missing(m, TJ, TK, ci):
    """per neighbour offset: nodes M (as a mask over the grid) whose marks lack the chunk that evaluates the neighbour M + offset"""
    out = []
    for ax in range(3):
        for step in (-1, 1):
            src = [slice(None)] * 3   # M
            dst = [slice(None)] * 3   # N = M + step along ax
            src[ax] = slice(1, None) if step < 0 else slice(None, -1)
            dst[ax] = slice(None, -1) if step < 0 else slice(1, None)
            src, dst = tuple(src), tuple(dst)
            mm = m[src]
            tj, tk, c = TJ[dst][..., None], TK[dst][..., None], ci[dst][..., None]
            hit = (mm[..., 0] == tj) & (mm[..., 1] == tk) & (mm[..., 2] <= c) & (c <= mm[..., 3])
            out.append(~hit.any(axis=-1))
    return out


@pytest.mark.parametrize("chunk", [8, 16])
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_reader_of_a_changed_node_is_marked(lib, shape, dtype, chunk):
    for d in range(8):   # 7 -> 0 included
        dn = (d + 1) % 8
        m = marks(lib, dtype, chunk, d, 1, shape)
        assert not np.any(m == -7), "every word of the output is written"
        TJ, TK, ci = readers(dtype, chunk, dn, shape)
        for q, miss in enumerate(missing(m, TJ, TK, ci)):
            assert not miss.any(), (shape, dtype, chunk, d, q, np.argwhere(miss)[:4])
        # a node's own unit comes first, and one node reaches at most two chunks of a unit (levels l - 1 .. l + 1)
        assert np.array_equal(m[..., 0, 0], TJ) and np.array_equal(m[..., 0, 1], TK)
        used = m[..., 0] >= 0
        assert np.all((m[..., 2] <= m[..., 3])[used]) and np.all((m[..., 3] - m[..., 2])[used] <= 1)
        assert np.all(m[..., 2][used] >= 0)
        # the marked chunks exist: a unit has nodes at levels Ls .. Le
        NF, NJ, NK = shape
        PJ, PK = PATCH[dtype]
        tj, tk = m[..., 0][used], m[..., 1][used]
        Ls = tj * PJ + tk * PK
        Le = np.minimum(tj * PJ + PJ, NJ) - 1 + np.minimum(tk * PK + PK, NK) - 1 + NF - 1
        lcf = Ls - (Ls - (tj + tk)) % chunk
        assert np.all(tj * PJ < NJ) and np.all(tk * PK < NK) and np.all(lcf + m[..., 3][used] * chunk <= Le)


@pytest.mark.parametrize("shape,dtype", [((37, 35, 41), F32), ((70, 53, 41), F32), ((2, 16, 10), F64), ((17, 33, 34), F64)])
def test_without_the_edge_columns_a_reader_is_missed(lib, shape, dtype):
    """negative control: the check above notices marks that stop at the patch edge -- exactly at the columns beside an edge"""
    PJ, PK = PATCH[dtype]
    for chunk in (8, 16):
        for d in range(8):
            dn = (d + 1) % 8
            TJ, TK, ci = readers(dtype, chunk, dn, shape)
            miss = missing(marks(lib, dtype, chunk, d, 0, shape), TJ, TK, ci)
            assert not miss[4].any() and not miss[5].any()   # F neighbours share the column
            n_bad = 0
            for ax, q in ((1, 2), (1, 3), (0, 0), (0, 1)):   # J steps, K steps
                T = TJ if ax == 1 else TK
                step = -1 if q % 2 == 0 else 1
                src = [slice(None)] * 3
                dst = [slice(None)] * 3
                src[ax] = slice(1, None) if step < 0 else slice(None, -1)
                dst[ax] = slice(None, -1) if step < 0 else slice(1, None)
                crosses = T[tuple(src)] != T[tuple(dst)]
                assert np.array_equal(miss[q], crosses), (shape, dtype, chunk, d, q)
                n_bad += int(crosses.sum())
            assert n_bad > 0


def test_argument_errors(lib):
    from ttcr_amd import _lib

    out = np.zeros(12 * 8, dtype=np.int32)
    p = out.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.ttcr_fsm_chunk_dirty_marks(F32, 8, 0, 1, 2, 2, 2, p, out.size) == _lib.OK
    for args in [(2, 8, 0, 1, 2, 2, 2, p, out.size), (F32, 4, 0, 1, 2, 2, 2, p, out.size), (F32, 8, 8, 1, 2, 2, 2, p, out.size),
                 (F32, 8, 0, 1, 1, 2, 2, p, out.size), (F32, 8, 0, 1, 2, 2, 2, None, out.size), (F32, 8, 0, 1, 2, 2, 2, p, out.size - 1)]:
        assert lib.ttcr_fsm_chunk_dirty_marks(*args) != _lib.OK
