"""Inputs of tests/test_long_axis_gpu.py (the sweep kernels with exact skipping where a unit's bit sets pass their first 32-bit word),
shared with tests/test_long_axis_cases.py (CPU: what the GPU tests rely on).  Device-free.

The skip kernels (fsm_sweep_unit, ttcr_amd/csrc/fsm_kernels.h) keep per-unit bit sets indexed along the level axis F (x in 3-D, z in
2-D): chunk dirty bits and change maps (one bit per chunk of C levels), slab mask and brick stamps (one bit per F brick of 16 nodes).
A chunk index reaches 32 from 32 C levels on, a brick index from 513 nodes on: long thin grids get there with 1e5 - 1e6 nodes.

Node grids, dx = 0.5, origin 0.  The 3-D patches are 16 x 16 columns (y, z) in fp32 and 16 x 8 in fp64; the 2-D patches are 64 columns (x).

    LONG        (600, 35, 19)    fp32 3 x 2 patches with remainders 3 and 3, fp64 3 x 3; 81 chunks of 8 and 40 of 16 per unit, 38 F bricks
    LONGER      (2100, 17, 9)    dirty-bit words up to index 8, slab / stamp word 4
    LONG_WENO   (600, 18, 9)     fp32 2 x 1, fp64 2 x 2: the WENO pair kernel's chunks of 4 reach word 4
    LONG_2D     (130, 600) and (66, 1100) as (nx, nz)
    LIMIT       (16384, 17, 2) and (16385, 17, 2): the last NF with exact skipping (1024 F bricks = 32 words of 32 bits) and the first
                without

Models: "gradient" 1 / (1 + 0.1 z); "block16" / "block64" / "block256": uniform random slowness in [0.25, 1) per block of 16 / 64 / 256
nodes along F and 16 along the other axes, seed 5 ("block16" is the model of tests/test_chunk_dirty_gpu.py); "smooth": the WENO model
of tests/weno_2d_cases.py.

Sources of the first-order 3-D tests: the four off-node fractions of test_chunk_dirty_gpu.OFF and two on nodes, (250, 3, 3) and
(506, 3, 3), whose frozen boxes straddle level 256 (chunk 32 of unit (0, 0) on chunks of 8) and level 512 (chunk 32 on chunks of 16) in
direction 0.  The WENO-stage, 2-D and limit tests use four (three) of them: the instantiation table of tests/test_weno_2d_gpu.py is
built for calls of four sources.
"""
import numpy as np

import weno_2d_cases as wc

DX = 0.5
SEED = 5
OFF = [(0.31, 0.62, 0.22), (0.93, 0.08, 0.77), (0.12, 0.9, 0.41), (0.55, 0.45, 0.6)]   # == test_chunk_dirty_gpu.OFF (test_long_axis_cases.py)
ON_NODES = [(250, 3, 3), (506, 3, 3)]
DTYPES = [np.float32, np.float64]
BRICK = 16
MAXIT = 50


def _case(n):
    n = tuple(n)
    return dict(name="x".join(map(str, n)), dim=len(n), n=n, d=(DX,) * len(n), cell=False)


LONG = _case((600, 35, 19))
LONGER = _case((2100, 17, 9))
LONG_WENO = _case((600, 18, 9))
LONG_2D = [_case((130, 600)), _case((66, 1100))]
LIMIT = [_case((16384, 17, 2)), _case((16385, 17, 2))]
CASES = [LONG, LONGER, LONG_WENO] + LONG_2D + LIMIT

BLOCKS = {"block16": 16, "block64": 64, "block256": 256}
# models that take the oracle several iterations, per case (the gradient converges with the first sweeps)
ITERATING = {LONG["name"]: "block16", LONGER["name"]: "block64", LONG_WENO["name"]: "block16", LONG_2D[0]["name"]: "block16",
             LONG_2D[1]["name"]: "block16", LIMIT[0]["name"]: "block256", LIMIT[1]["name"]: "block256"}


def f_axis(c):
    """the level axis: x in 3-D, z in 2-D"""
    return 0 if c["dim"] == 3 else 1


def slowness(c, model, dtype):
    """(nx, ny, nz) / (nx, nz) node slowness in the grid's dtype"""
    shape = c["n"]
    if model == "gradient":
        z = np.arange(shape[-1]) * DX
        s = np.broadcast_to((1.0 / (1.0 + 0.1 * z))[(None,) * (len(shape) - 1)], shape)
    elif model in BLOCKS:
        edge = [16] * len(shape)
        edge[f_axis(c)] = BLOCKS[model]
        b = np.random.default_rng(SEED).uniform(0.25, 1.0, [(m + e - 1) // e for m, e in zip(shape, edge)])
        for a, e in enumerate(edge):
            b = np.repeat(b, e, axis=a)
        s = b[tuple(slice(0, m) for m in shape)]
    else:
        return wc.slowness(c, model, dtype)
    return np.ascontiguousarray(s, dtype=dtype)


def maxit(c, model):
    return wc.maxit(c, model) if model in wc.MODELS else MAXIT


def sources(c):
    """(n, dim) source points of a case"""
    ext = np.array([(m - 1) * DX for m in c["n"]])
    off = np.array(OFF) * ext[None, :] if c["dim"] == 3 else np.array(OFF)[:, :2] * ext[None, :]
    if c in LIMIT:
        return off[:3]
    if c["dim"] == 2:
        return off
    node = np.array(ON_NODES, dtype=np.float64) * DX
    if c is LONG_WENO:
        return np.vstack([off[0], node[0], off[2], node[1]])
    return np.vstack([off, node])


def n_src(c):
    return len(sources(c))


def receivers(c):
    """few_workgroups_cases.receivers(shape), and the same rule in 2-D"""
    return wc.receivers(c)


_REFS = {}


def reference(oracle, c, model, dtype, k, weno=False, maxit_=None):
    """oracle solve of source k: dict(tt, niter, niterw, change, changew, tt_rcv).  Computed once and shared: read-only."""
    mi = maxit(c, model) if maxit_ is None else maxit_
    key = (c["name"], model, np.dtype(dtype).name, int(k), bool(weno), mi)
    if key not in _REFS:
        s = wc.flat(c, slowness(c, model, dtype))
        nc = tuple(m - 1 for m in c["n"])
        kw = dict(eps=wc.EPS, maxit=mi, rcv=receivers(c), weno=weno)
        src = sources(c)[k:k + 1]
        if c["dim"] == 3:
            o = oracle.solve3d(dtype, nc, DX, (0.0, 0.0, 0.0), s, src, **kw)
        else:
            o = oracle.solve2d(dtype, nc, DX, DX, (0.0, 0.0), s, src, **kw)
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        _REFS[key] = o
    return _REFS[key]


def field(c, tt):
    """a flat field of the solver as an array with the case's shape"""
    return tt.reshape(c["n"], order="F") if c["dim"] == 3 else tt.reshape(c["n"])
