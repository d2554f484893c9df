"""Inputs and references of tests/test_weno_2d_gpu.py (every WENO-stage and every 2-D instantiation of fsm_sweep_persistent by name),
shared with tests/test_weno_2d_cases.py (CPU: what the GPU tests rely on) and tests/test_unit_order.py (the ticket order on the same
shapes).  Device-free.

Origin 0, four sources at the fractions of few_workgroups_cases.FRACTIONS (2-D: their first two components), receivers from
arith_cases.receivers.  The 3-D patches are PJ x PK columns (y, z) marched along x in chunks of 4, 8 or 16 levels; the 2-D patches are one
wave of 64 columns (x) marched along z in chunks of 16 levels.  The WENO stage (H = 2) exchanges a halo of two columns between patches.

    3-D, dx = 0.5
    (37, 35, 41)   the shape of the looped suite: 3 x 3 patches fp32, 3 x 6 fp64, an interior patch with a full neighbourhood
    (17, 33, 34)   last patch of 1 column in J (33 = 2 16 + 1) and of 2 in K (fp32 34 = 2 16 + 2, fp64 34 = 4 8 + 2): narrower than
                   and equal to the halo it serves; 17 levels: one more than a chunk of 16
    (17, 34, 33)   the same with J and K exchanged: a K patch of 1 column in both precisions
    (41, 18, 5)    5 nodes along K, barely wider than the 2 H = 4 columns the two halos take; many chunks per unit
    (9, 49, 17)    a short march axis under four J patches (49 = 3 16 + 1), K remainder 1
    (17, 33, 34)c  the cell grid of 16 x 32 x 33 cells on those nodes
    2-D (J = x)
    (65, 130)      dx = 0.2, dz = 0.3 (the fp32 values, in both precisions): a patch of 64 and one of 1; update2_xz
    (130, 65)      dx = dz = 0.25: 64 + 64 + 2
    (66, 37)       dx = dz = 0.25: 64 + 2
    (66, 37)c      the cell grid of 65 x 36 cells on those nodes

Models: "rough" -- uniform(0.25, 1) node by node (seed 211), rounded to the grid's dtype, maxit = 15: the WENO stage does not converge and
leaves at the cap, every chunk stays dirty; "smooth" -- the gradient with a ripple of stopping_sums_cases.slowness, maxit 50 (2-D: 80):
the stage converges, exact skipping really skips, the sources of a batch finish apart.
"""
import numpy as np

import arith_cases as ac
import few_workgroups_cases as fw
import stopping_sums_cases as sc

# columns of a patch (PJ, PK): TileCfg<T, DIM> in ttcr_amd/csrc/fsm_capi.hip
TILE = {(3, "float32"): (16, 16), (3, "float64"): (16, 8), (2, "float32"): (64, 1), (2, "float64"): (64, 1)}
HALO = 2                 # columns a WENO patch reads beyond its own, each side
DTYPES = fw.DTYPES
N_SRC = fw.N_SRC
SEED = 211
EPS = 1e-5               # the default of the grid classes
# 0.2 and 0.3 as fp32 has them: both precisions work on the same spacings, and arith_cases.receivers keeps the last planes inside
DX2, DZ2 = float(np.float32(0.2)), float(np.float32(0.3))
MODELS = ("rough", "smooth")


def _case(n, d, cell=False):
    n = tuple(n)
    return dict(name="x".join(map(str, n)) + ("c" if cell else ""), dim=len(n), n=n, d=tuple(d), cell=cell)


MAIN_3D = _case((37, 35, 41), (0.5,) * 3)
OTHER_3D = [_case((17, 33, 34), (0.5,) * 3), _case((17, 34, 33), (0.5,) * 3), _case((41, 18, 5), (0.5,) * 3), _case((9, 49, 17), (0.5,) * 3)]
XZ_2D = _case((65, 130), (DX2, DZ2))
MAIN_2D = _case((130, 65), (0.25, 0.25))
OTHER_2D = [_case((66, 37), (0.25, 0.25))]
CELLS_3D = _case((17, 33, 34), (0.5,) * 3, cell=True)
CELLS_2D = _case((66, 37), (0.25, 0.25), cell=True)
NODE_CASES = [MAIN_3D] + OTHER_3D + [XZ_2D, MAIN_2D] + OTHER_2D
CELL_CASES = [CELLS_3D, CELLS_2D]
CASES = NODE_CASES + CELL_CASES
BY_NAME = {c["name"]: c for c in CASES}

# the order of the four sources in which, with option "pair_sources" = 0 and four slots, each pair -- (first, second) and (third, fourth)
# source of the call -- holds two different WENO iteration counts on the smooth model, in both precisions and in the reversed call
# (tests/test_weno_2d_cases.py)
PAIR_ORDER = {"37x35x41": [0, 2, 1, 3], "130x65": [0, 1, 2, 3]}


def rows():
    """(case, model) of every reference: both models on the node grids, the smooth one on the cell grids"""
    return [(c, m) for c in NODE_CASES for m in MODELS] + [(c, "smooth") for c in CELL_CASES]


def maxit(c, model):
    return 15 if model == "rough" else (50 if c["dim"] == 3 else 80)


def axes(c):
    return [np.arange(m) * h for m, h in zip(c["n"], c["d"])]


def slowness(c, model, dtype):
    """(nx, ny, nz) / (nx, nz) array of node slowness (cell grid: of cell slowness) in the grid's dtype"""
    shape = tuple(m - 1 for m in c["n"]) if c["cell"] else c["n"]
    if model == "rough":
        s = np.random.default_rng(SEED).uniform(0.25, 1.0, shape)
    else:
        s = sc.slowness(dict(nodes=c["n"], dim=c["dim"], cell=c["cell"], smooth=True, dx=c["d"][0], dz=c["d"][-1], seed=0))
    assert s.shape == shape
    return np.ascontiguousarray(s, dtype=dtype)


def flat(c, a):
    """the solver's flat order: 3-D x fastest, 2-D z fastest"""
    return a.flatten("F") if c["dim"] == 3 else a.ravel()


def sources(c):
    """the four source points, (4, dim)"""
    ext = np.array([(m - 1) * h for m, h in zip(c["n"], c["d"])])
    return np.array(fw.FRACTIONS)[:, :c["dim"]] * ext


def receivers(c):
    """arith_cases.receivers, axis by axis: every coordinate of a row depends on its own axis and spacing alone"""
    cols = [ac.receivers(dict(n=c["n"], dx=h, dim=c["dim"]))[:, a] for a, h in enumerate(c["d"])]
    return np.column_stack(cols)


def threshold(c, dtype):
    """epsilon *= N in the grid's precision: what a stage's change is held against"""
    t = np.dtype(dtype).type
    return float(t(EPS) * t(int(np.prod(c["n"]))))


def _solve(oracle, c, model, dtype, k, weno, ref):
    s = flat(c, slowness(c, model, dtype))
    nc = tuple(m - 1 for m in c["n"])
    kw = dict(eps=EPS, maxit=maxit(c, model), cell_slowness=c["cell"], rcv=receivers(c), weno=weno)
    src = sources(c)[k:k + 1]
    if c["dim"] == 3:
        f = oracle.ref_solve3d if ref else oracle.solve3d
        return f(dtype, nc, c["d"][0], (0.0, 0.0, 0.0), s, src, **kw)
    f = oracle.ref_solve2d if ref else oracle.solve2d
    return f(dtype, nc, c["d"][0], c["d"][1], (0.0, 0.0), s, src, **kw)


_REFS = {}


def reference(oracle, c, model, dtype, k, weno=True, ref=False):
    """oracle solve of source k: dict(tt, niter, niterw, change, changew, tt_rcv); ref: the compiled reference instead (no histories).
    Computed once per (case, model, dtype, source, weno) and shared: read-only."""
    key = (c["name"], model, np.dtype(dtype).name, int(k), bool(weno), bool(ref))
    if key not in _REFS:
        o = _solve(oracle, c, model, dtype, k, weno, ref)
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        _REFS[key] = o
    return _REFS[key]


def patches(c, dtype):
    """per patch axis (3-D: J = y, K = z; 2-D: J = x): (number of patches, columns of the last one)"""
    t = TILE[(c["dim"], np.dtype(dtype).name)]
    cols = c["n"][1:] if c["dim"] == 3 else c["n"][:1]
    return [(-(-m // p), m - (-(-m // p) - 1) * p) for m, p in zip(cols, t)]
