"""Case table of tests/test_stopping_sums_gpu.py and the CPU side of its construction: solves whose LAST iteration of a chosen stage
is decided by the reference's sequential T1 sum itself (ttcr/Grid3Drnfs.h:141-152), so that the sum the device computed for that
iteration can be compared with the oracle's `change` bit for bit.

The construction (oracle only, no device):
  1. solve at eps = 1e-9 and read the history of the stage (`change` first-order, `changew` WENO);
  2. a target is an iteration k whose change c[k] is finite and > 0 (first-order: k >= 1, the first iteration has no snapshot);
  3. eps = m c[k] / N with m = 1.5 (fp32: c[k] / thr = 0.67 inside the [1/2, 16] window) or 1 + 5e-7 (fp64: inside 1 +- 1e-6);
  4. thr = T(eps) T(N) (epsilon *= N in T1, ttcr/Grid3Drnfs.h:49);
  5. solve again with that eps: this second solve is the reference of the device run.
aim() asserts the precondition on the oracle's numbers alone: the stage of the second solve ends at k + 1 iterations, its last change is
below thr and inside the window, every earlier one is at or above thr."""
import numpy as np

WINDOW = {np.dtype(np.float32): (0.5, 16.0), np.dtype(np.float64): (1.0 - 1e-6, 1.0 + 1e-6)}
MARGIN = {np.dtype(np.float32): 1.5, np.dtype(np.float64): 1.0 + 5e-7}

# fractions of the grid's extent: off-node sources (source 0 sets eps; the others fill the slots of the multi-source layouts)
SOURCES = np.array([[0.3137, 0.4721, 0.2309], [0.7213, 0.2817, 0.6619], [0.1523, 0.8109, 0.5231]])


def _case(name, nodes, cell=False, weno=False, smooth=False, dx=0.25, dz=None, seed=0, pick="all", dtypes=(np.float32, np.float64)):
    return dict(name=name, nodes=tuple(nodes), dim=len(nodes), cell=cell, weno=weno, smooth=smooth, dx=dx, dz=dx if dz is None else dz,
                seed=seed, pick=pick, dtypes=tuple(np.dtype(d) for d in dtypes))


# pick: "all" qualifying iterations, or indices into the list of qualifying ones
CASES = [
    _case("odd_37x29x45", (37, 29, 45), seed=31),                      # N odd: one element per lane; partial blocks, partial bricks
    _case("vec_36x29x45", (36, 29, 45), seed=32),                      # NF % 4 == 0: vectors and brick stamps together
    _case("vec_34x30x46", (34, 30, 46), seed=33),                      # NF % 4 == 2: fp32, one field per slot falls back to whole fields
    _case("n4r2_38x29x45", (38, 29, 45), seed=34),                     # N % 4 == 2
    _case("cells_21x20x24", (21, 20, 24), cell=True, seed=35, pick=(0, 1)),
    _case("n2d_151x71", (151, 71), dx=0.2, dz=0.3, seed=36, pick=(0, 1, 2, 3, 4, 5)),
    _case("weno_25x27x23", (25, 27, 23), weno=True, smooth=True, dx=0.5, pick=(0, "mid", -1)),
    _case("weno_cells2d_131x67", (131, 67), cell=True, weno=True, smooth=True, dx=0.25, dz=0.25, pick=(0, "mid", -1)),
    _case("big_97x83x91", (97, 83, 91), seed=37, pick=(0, -1), dtypes=(np.float32,)),   # 732 641 nodes, 179 blocks
]
BY_NAME = {c["name"]: c for c in CASES}
FIRST_ORDER_3D = [c["name"] for c in CASES if c["dim"] == 3 and not c["weno"]]


def n_nodes(c):
    return int(np.prod(c["nodes"]))


def axes(c, dt):
    """node coordinates in the grid's dtype, and the spacings the wrapper derives from them (x[1] - x[0] in that dtype)"""
    dt = np.dtype(dt)
    d = [c["dx"]] * c["dim"] if c["dim"] == 3 else [c["dx"], c["dz"]]
    ax = [(np.arange(n) * h).astype(dt) for n, h in zip(c["nodes"], d)]
    return ax, [float(a[1] - a[0]) for a in ax]


def slowness(c):
    """(nx, ny, nz) / (nx, nz) array of node or cell slowness: uniform(0.3, 1.0), or a smooth gradient with a gentle lateral ripple"""
    shape = tuple(n - 1 for n in c["nodes"]) if c["cell"] else c["nodes"]
    if not c["smooth"]:
        return np.random.default_rng(c["seed"]).uniform(0.3, 1.0, shape)
    d = [c["dx"]] * c["dim"] if c["dim"] == 3 else [c["dx"], c["dz"]]
    g = np.meshgrid(*[(np.arange(n) + (0.5 if c["cell"] else 0.0)) * h for n, h in zip(shape, d)], indexing="ij")
    s = 1.0 / (1.0 + 0.08 * g[-1])
    return s * (1.0 + 0.2 * np.sin(0.4 * g[0])) if c["dim"] == 2 else s * (1.0 + 0.2 * np.sin(0.4 * g[0]) * np.cos(0.3 * g[1]))


def sources(c, n_src=1):
    ext = np.array([(n - 1) * h for n, h in zip(c["nodes"], [c["dx"]] * 3 if c["dim"] == 3 else [c["dx"], c["dz"]])])
    return SOURCES[:n_src, :c["dim"]] * ext


def flat(c, a):
    """an (nx, ny, nz) array in the solver's flat order (3-D: x fastest, 2-D: z fastest)"""
    return a.flatten("F") if c["dim"] == 3 else a.ravel()


_SOLVED = {}   # (case, dtype, source, eps) -> the oracle's solve: the layouts of a case share their references


def solve(O, c, dt, i_src, eps):
    """the oracle's solve of source i_src of a case (kept: callers read it, none writes to it)"""
    dt = np.dtype(dt)
    key = (c["name"], dt.name, int(i_src), float(eps))
    if key not in _SOLVED:
        _, d = axes(c, dt)
        nc = tuple(n - 1 for n in c["nodes"])
        s = flat(c, slowness(c))
        src = sources(c, i_src + 1)[i_src:i_src + 1]
        if c["dim"] == 3:
            o = O.solve3d(dt, nc, d[0], (0, 0, 0), s, src, eps=eps, cell_slowness=c["cell"], weno=c["weno"])
        else:
            o = O.solve2d(dt, nc, d[0], d[1], (0, 0), s, src, eps=eps, cell_slowness=c["cell"], weno=c["weno"])
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        _SOLVED[key] = o
    return _SOLVED[key]


def history(c, o):
    return np.asarray(o["changew"] if c["weno"] else o["change"])


def threshold(c, dt, eps):
    t = np.dtype(dt).type
    return t(eps) * t(n_nodes(c))


def targets(O, c, dt):
    """the iterations of the probing solve (eps = 1e-9, source 0) that qualify, restricted to the case's pick"""
    h = history(c, solve(O, c, dt, 0, 1e-9)).astype(np.float64)
    m = MARGIN[np.dtype(dt)]
    ok = [k for k in range(0 if c["weno"] else 1, h.size) if np.isfinite(h[k]) and h[k] > 0 and np.all(h[:k] >= m * h[k] * (1 + 1e-6))]
    if c["pick"] == "all":
        return ok
    out = []
    for p in c["pick"]:
        k = ok[len(ok) // 2] if p == "mid" else ok[p]
        if k not in out:
            out.append(k)
    return out


def aim(O, c, dt, k):
    """eps that makes iteration k (0-based) of the case's stage the one the reference's sum decides, thr, and the oracle's solve with
    that eps; asserts the CPU precondition"""
    dt = np.dtype(dt)
    h = history(c, solve(O, c, dt, 0, 1e-9)).astype(np.float64)
    eps = MARGIN[dt] * h[k] / n_nodes(c)
    thr = threshold(c, dt, eps)
    o2 = solve(O, c, dt, 0, eps)
    h2 = history(c, o2)
    lo, hi = WINDOW[dt]
    assert h2.size == k + 1, (c["name"], dt.name, k, h, h2)
    assert h2[k] < thr and lo <= float(h2[k]) / float(thr) <= hi, (c["name"], dt.name, k, h2[k], thr)
    assert np.all(h2[:k] >= thr), (c["name"], dt.name, k, h2, thr)
    if c["weno"]:
        assert len(o2["change"]) >= 1
    return eps, thr, o2
