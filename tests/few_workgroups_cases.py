"""Inputs of tests/test_few_workgroups_gpu.py (the looped sweep kernels with 1 and 3 resident workgroups), shared with
tests/test_few_workgroups_cases.py (CPU: what the GPU tests rely on) and tests/test_unit_order.py (the ticket order on the same shapes).

Node grids, weno = 0, dx = 0.5, origin 0, slowness uniform in [0.25, 1) node by node (seed 101), rounded to the grid's dtype.  The 3-D
patches are 16 x 16 columns (y, z) in fp32 and 16 x 8 in fp64, marched along x in chunks of 8 or 16 levels:

    (37, 35, 41)   fp32 3 x 3 patches (remainders 3 and 9: an interior patch with both upwind neighbours and a full 3 x 3 neighbourhood in the
                   previous sweep), fp64 3 x 6 (z remainder 1); 9 / 5 chunks along x
    (19, 50, 36)   fp32 4 x 3, fp64 4 x 5
    (70, 17, 9)    fp32 2 x 1, thin, many chunks per unit
    (2, 16, 10)    one patch (fp64: two along z): a lone workgroup runs the directional units of an iteration back to back
"""
import numpy as np

import arith_cases as ac

SHAPES = [(37, 35, 41), (19, 50, 36), (70, 17, 9), (2, 16, 10)]
LARGER = SHAPES[:3]
DX = 0.5
SEED = 101
FRACTIONS = [(0.31, 0.62, 0.22), (0.5, 0.5, 0.5), (0.93, 0.08, 0.77), (0.12, 0.9, 0.41)]
N_SRC = len(FRACTIONS)
DTYPES = [np.float32, np.float64]
# (70, 17, 9) with option "pair_sources" = 0 and four slots: the pairs are (first, second) and (third, fourth) source of the call --
# in this order each pair holds a source that needs 4 iterations and one that needs 5
PAIR_ORDER_70 = [0, 2, 1, 3]


def axes(shape):
    return [np.arange(m) * DX for m in shape]


def slowness(shape, dtype):
    """(nx, ny, nz) node slowness in the grid's dtype"""
    return np.ascontiguousarray(np.random.default_rng(SEED).uniform(0.25, 1.0, shape), dtype=dtype)


def sources(shape):
    """the four source points, (4, 3)"""
    ext = np.array([(m - 1) * DX for m in shape])
    return np.array(FRACTIONS) * ext


def receivers(shape):
    """corners, faces, nodes, a few ulp inside the last planes, off everything (arith_cases.receivers)"""
    return ac.receivers(dict(n=shape, dx=DX, dim=3))


_REFS = {}


def reference(oracle, shape, dtype, k):
    """oracle solve of source k: dict(tt, niter, change, tt_rcv).  Computed once per (shape, dtype, source) and shared: do not modify."""
    key = (tuple(shape), np.dtype(dtype).name, k)
    if key not in _REFS:
        s = slowness(shape, dtype)
        _REFS[key] = oracle.solve3d(dtype, tuple(m - 1 for m in shape), DX, (0.0, 0.0, 0.0), s.flatten("F"), sources(shape)[k:k + 1],
                                    rcv=receivers(shape))
    return _REFS[key]


def held(order, n_threads):
    """slot -> source whose field the slot holds after a call with the sources in `order`: block distribution (get_blk_size,
    ttcr/Grid3D.h:451-465) -- slot b takes blk[b] consecutive sources, one per round, and keeps the last.  Also the rounds: lists of the
    sources solved together."""
    n = len(order)
    n_blk = min(n_threads, n)
    blk = [0] * n_blk
    for q in range(n):
        blk[q % n_blk] += 1
    start = [sum(blk[:b]) for b in range(n_blk)]
    rounds = [[order[start[b] + r] for b in range(n_blk) if r < blk[b]] for r in range(max(blk))]
    return {b: order[start[b] + blk[b] - 1] for b in range(n_blk)}, rounds
