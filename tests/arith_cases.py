"""The small grids of the tolerance-mode tests (option "arith" = 1), shared by tests/test_arith_reference.py (CPU: the numpy restatement
against both oracles) and tests/test_arith_small_gpu.py (the kernels against both oracles).  All fp32, weno = 0, origin 0.

A case: name, dim, n = NODE counts (for a cell grid: of the node grid the solver works on), cell, dx, model, seed, src (points), t0,
smooth (iteration counts are asserted on smooth models only).  The 3-D patches of the sweep kernels are 16 x 16 columns (y, z) marched
along x in chunks of 16 or 8 levels; the 2-D patches are one wave of 64 columns (x) marched along z.
"""
import numpy as np

f32 = np.float32


def _case(name, n, dx, model, src, t0=None, cell=False, seed=1, smooth=False):
    src = np.atleast_2d(np.asarray(src, dtype=np.float64))
    return dict(name=name, dim=len(n), n=tuple(n), dx=dx, model=model, seed=seed, cell=cell, src=src,
                t0=np.zeros(src.shape[0]) if t0 is None else np.asarray(t0, dtype=np.float64), smooth=smooth)


def _off(n, dx, frac):
    """a point off every node: frac of the way through the grid, then 0.37 / 0.21 / 0.43 of a cell further"""
    return [min((int(f * (m - 1)) + o), m - 1 - 1e-3) * dx for f, m, o in zip(frac, n, (0.37, 0.21, 0.43))]


N3 = (33, 31, 35)   # remainders of 1, 15 and 3 columns / levels against the 16 x 16 patches and the chunks
CASES = [
    _case("grad-33x31x35", N3, 0.5, "gradient", _off(N3, 0.5, (0.3, 0.6, 0.2)), smooth=True),
    _case("rand-33x31x35", N3, 0.5, "random", _off(N3, 0.5, (0.3, 0.6, 0.2))),
    _case("two-33x31x35", N3, 0.5, "two", _off(N3, 0.5, (0.3, 0.6, 0.2))),
    _case("rand-33x31x35-on-node", N3, 0.5, "random", [[8.0, 7.5, 3.0]]),
    _case("rand-33x31x35-corner-cell", N3, 0.5, "random", [[16.0 - 0.15, 15.0 - 0.1, 17.0 - 0.2]]),
    # three points, two of them within one cell of each other
    _case("rand-33x31x35-3pts", N3, 0.5, "random", [[4.2, 9.1, 3.3], [4.45, 9.3, 3.1], [12.0, 2.6, 14.7]], t0=[0.0, 0.05, 0.3]),
    _case("rand-70x17x9", (70, 17, 9), 0.5, "random", _off((70, 17, 9), 0.5, (0.4, 0.5, 0.5)), seed=2),
    _case("thin-2x16x10", (2, 16, 10), 0.5, "random", [[0.2, 3.3, 2.1]], seed=3),
    _case("thin-16x2x10", (16, 2, 10), 0.5, "random", [[3.3, 0.2, 2.1]], seed=4),
    _case("thin-10x16x2", (10, 16, 2), 0.5, "random", [[2.1, 3.3, 0.2]], seed=5),
    _case("rand-4x4x4", (4, 4, 4), 0.5, "random", [[0.7, 0.6, 0.9]], seed=6),
    _case("rand-20x18x17-dx2.3", (20, 18, 17), 2.3, "random", _off((20, 18, 17), 2.3, (0.3, 0.6, 0.2)), seed=7),
    _case("cells-32x30x34", N3, 0.5, "random", _off(N3, 0.5, (0.6, 0.3, 0.7)), cell=True, seed=8),
    _case("grad2d-150x70", (150, 70), 0.5, "gradient", _off((150, 70), 0.5, (0.3, 0.6)), smooth=True),
    _case("rand2d-150x70", (150, 70), 0.5, "random", _off((150, 70), 0.5, (0.3, 0.6)), seed=9),
    _case("rand2d-65x130", (65, 130), 0.5, "random", _off((65, 130), 0.5, (0.7, 0.2)), seed=10),
    _case("thin2d-2x40", (2, 40), 0.5, "random", [[0.2, 7.3]], seed=11),
    _case("thin2d-40x2", (40, 2), 0.5, "random", [[7.3, 0.2]], seed=12),
    _case("cells2d-60x44", (61, 45), 0.5, "random", _off((61, 45), 0.5, (0.5, 0.4)), cell=True, seed=13),
]
BY_NAME = {c["name"]: c for c in CASES}


# single-point sources on the random 33 x 31 x 35 model for the batch tests: off the nodes, on a node, near faces and corners
BATCH_SRC = [[4.685, 9.105, 3.215], [8.0, 7.5, 3.0], [15.85, 14.9, 16.8], [0.2, 0.1, 0.3], [12.3, 2.6, 14.7], [7.1, 13.3, 9.9]]


def batch_cases(n):
    """the first n sources of BATCH_SRC as cases of their own on the model of rand-33x31x35"""
    base = BY_NAME["rand-33x31x35"]
    return [dict(base, name="rand-33x31x35-batch%d" % k, src=np.array([BATCH_SRC[k]]), t0=np.zeros(1)) for k in range(n)]


def grid_dx(c):
    """the cell size an fp32 grid of this case works with: x[1] - x[0] of its fp32 axes (origin 0)"""
    return float(f32(c["dx"]))


def axes(c):
    return [np.arange(m) * c["dx"] for m in c["n"]]


def slowness(c, model=None):
    """fp32 slowness in the shape the grid classes take it: (nx, ny, nz) / (nx, nz) of nodes, or of cells for a cell grid"""
    shape = tuple(m - 1 for m in c["n"]) if c["cell"] else c["n"]
    rng = np.random.default_rng(c["seed"])
    model = model or c["model"]
    if model == "gradient":      # 1 / (1 + 0.1 z) with a smooth bump, depth along the last axis
        g = np.meshgrid(*[np.arange(m) * c["dx"] for m in shape], indexing="ij")
        r2 = sum((gi - 0.4 * gi.max()) ** 2 for gi in g)
        s = (1.0 + 0.2 * np.exp(-r2 / 20.0)) / (1.0 + 0.1 * g[-1])
    elif model == "random":      # uniform 0.25 ... 1, node by node
        s = rng.uniform(0.25, 1.0, shape)
    elif model == "two":         # 0.2 or 5.0 in blocks of 4 nodes: contrasts of 25 across faces that cut the patches
        b = rng.integers(0, 2, [m // 4 + 1 for m in shape])
        for a in range(len(shape)):
            b = np.repeat(b, 4, axis=a)
        s = np.where(b[tuple(slice(0, m) for m in shape)] == 1, 5.0, 0.2)
    else:
        raise ValueError(model)
    return np.ascontiguousarray(s, dtype=f32)


def flat(c, s):
    """the solver's flat order: 3-D x fastest, 2-D z fastest"""
    return s.flatten("F") if c["dim"] == 3 else s.ravel()


def _last_plane(m, dx):
    """the last plane of an axis of m nodes as the fp32 axis has it and as the fp32 and the fp64 solver compute it (xmin + nx * dx, dx the fp32
    cell size): whichever is furthest in, as an fp32 value"""
    v = min(f32((m - 1) * dx), f32(f32(m - 1) * f32(dx)))
    while float(v) > (m - 1) * float(f32(dx)):
        v = np.nextafter(v, f32(0))
    return float(v)


def receivers(c):
    """on nodes, on faces, at both corners, a few ulp (fp32) inside the last planes, and off everything"""
    ax = axes(c)
    hi = [_last_plane(a.size, c["dx"]) for a in ax]
    inside = []
    for v in hi:
        w = f32(v)
        for _ in range(3):
            w = np.nextafter(w, f32(0))
        inside.append(float(w))
    mid = [float(a[a.size // 2]) for a in ax]
    off = [float(a[(a.size - 1) // 3] + 0.3 * c["dx"]) for a in ax]
    rows = [[0.0] * c["dim"], hi, inside, mid, off]
    for a in range(c["dim"]):
        face = list(off); face[a] = hi[a]; rows.append(face)             # on the last face of an axis
        face = list(off); face[a] = 0.0; rows.append(face)               # on the first
        edge = list(off); edge[a] = inside[a]; rows.append(edge)         # a few ulp inside the last plane
        node = list(mid); node[a] = float(ax[a][1]); rows.append(node)   # another node
    return np.array(rows)


def source_array(c):
    """(t0, x, y, z) rows, the points of ONE event (raytrace(..., aggregate_src=True))"""
    return np.hstack([c["t0"][:, None], c["src"]])


_REFS = {}


def references(oracle, c, eps, maxit, rotated=False):
    """fp32 and fp64 oracle on the same fp32-rounded node slowness (a cell grid: the fp32 cell-to-node average), and the field after the
    source initialisation.  Computed once per (case, eps, maxit) -- the key holds everything of the case that the result depends on -- and shared: do not modify."""
    key = (c["name"], c["n"], c["cell"], c["dx"], c["model"], c["seed"], c["src"].tobytes(), c["t0"].tobytes(), eps, maxit, rotated)
    if key in _REFS:
        return _REFS[key]
    nc = tuple(m - 1 for m in c["n"])
    dx = grid_dx(c)
    s = flat(c, slowness(c))
    rcv = receivers(c)
    org = (0.0,) * c["dim"]
    if c["dim"] == 3:
        solve = lambda dt, sl, cell, **kw: oracle.solve3d(dt, nc, dx, org, sl, c["src"], c["t0"], cell_slowness=cell, rcv=rcv, **kw)
    else:
        kr = dict(rotated=True) if rotated else {}
        solve = lambda dt, sl, cell, **kw: oracle.solve2d(dt, nc, dx, dx, org, sl, c["src"], c["t0"], cell_slowness=cell, rcv=rcv, **kr, **kw)
    r32 = solve(np.float32, s, c["cell"], eps=eps, maxit=maxit)
    sn = r32["node_slowness"]
    r64 = solve(np.float64, sn.astype(np.float64), False, eps=eps, maxit=maxit)
    init = solve(np.float32, s, c["cell"], eps=eps, maxit=0)
    assert init["niter"] == 0
    out = dict(ref32=r32, ref64=r64, T0=init["tt"], sn=sn, rcv=rcv)
    _REFS[key] = out
    return out


def errors(a, b):
    """(max, rms) of a - b over the nodes, in float64"""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(d))), float(np.sqrt(np.mean(d * d)))


# ---- the seeded sweep of tests/test_arith_small_gpu.py: random small configurations, fp32, weno = 0, square cells

SWEEP_SEEDS = [21, 22]
N_CONFIGS = 12   # per seed: 24 configurations in all


def draw_configuration(rng):
    """one random configuration: 3-D or 2-D, node or cell grid, 2 - 40 (2 - 140) cells per axis, 1 - 2 source points per event with or
    without origin times, 1 - 4 slots, skipping on / off, pairs on / off in 3-D.  A few points fall outside the grid: the oracle rejects
    those configurations (tests/test_arith_reference.py checks that the seeds in use lose at most a quarter that way)."""
    dim = 3 if rng.random() < 0.6 else 2
    cell = bool(rng.random() < 0.4)
    nc = tuple(int(v) for v in rng.integers(2, 41 if dim == 3 else 141, dim))
    dx = float(rng.choice([0.25, 0.5, 1.0, 0.7]))
    n = tuple(v + 1 for v in nc)
    hi = [v * float(f32(dx)) for v in nc]
    n_threads = int(rng.integers(1, 5))
    npt = int(rng.integers(1, 3))
    n_ev = 1 if npt == 2 else int(rng.integers(1, n_threads + 1))   # several events: one point each, one slot each
    pts = np.column_stack([rng.uniform(-0.005 * h, 1.005 * h, npt * n_ev) for h in hi])
    if rng.random() < 0.3:      # the first point on a node (not of the last planes: their fp32 coordinate may round outwards)
        pts[0] = [float(f32(int(rng.integers(0, m - 1)) * dx)) for m in n]
    if npt == 2 and rng.random() < 0.4:   # the second point within a cell of the first
        pts[1] = np.clip(pts[0] + rng.uniform(-0.6, 0.6, dim) * dx, 0.0, hi)
    t0 = np.round(rng.uniform(0, 0.5, npt * n_ev), 3) if rng.random() < 0.5 else np.zeros(npt * n_ev)
    return dict(name="sweep", dim=dim, cell=cell, n=n, dx=dx, model="random", seed=int(rng.integers(1 << 30)), n_threads=n_threads,
                npt=npt, n_ev=n_ev, pts=pts, t0=t0, skip=int(rng.integers(0, 2)), pair=bool(dim == 3 and rng.random() < 0.5), smooth=False)


def sweep_events(q, seed, n_cfg):
    """the events of a drawn configuration as cases of their own (same grid and model)"""
    k = q["npt"]
    return [dict(q, name="sweep-%d-%d-%d" % (seed, n_cfg, e), src=q["pts"][e * k:(e + 1) * k], t0=q["t0"][e * k:(e + 1) * k]) for e in range(q["n_ev"])]
