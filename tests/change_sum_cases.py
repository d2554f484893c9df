"""Case table of tests/test_change_sum_gpu.py and its CPU side (tests/test_change_sum_cases.py): the EXACT decrease of every iteration of
a first-order solve, which the fp64 sum the sweep kernels hand over (`change`, get_changes()) is held to.

Every sweep kernel adds the decreases c - t of the nodes it lowers; first-order sweeps only lower a node, so over an iteration the
decreases of a node telescope to F_{k-1}[n] - F_k[n], F_k the field after k iterations.  The fields are the oracle's (which the device
reproduces bit for bit): one solve per k with maxit = k.  E_k = exact_decrease(F_{k-1}, F_k), k >= 2; iteration 1 starts from max() and
is never compared.

bar() restates the host's own claim about that sum (decide_go_on, ttcr_amd/csrc/fsm_capi.hip): m = 2 (NF + NJ + NK + 64) u + 1e-6, and for
fp64 the window 1 +- 1e-6 within which the reference's sequential sum is asked for -- 1e-6 less that sum's own gamma = N u / (1 - N u).
Nothing here is measured on the code under test.

The shapes, models and sources are those of tests/few_workgroups_cases.py (four sources) and tests/stopping_sums_cases.py (cell and 2-D
grids), plus two 2-D node grids (dx != dz and dx = dz; 64 x 1 patches with remainders 1 and 2) and the rotated template (sweep45 after the axis
sweeps) on a grid that crosses a strip boundary of the strip kernel and on three elongated ones.  On the rough model the rotated
template does not converge within maxit = 50 on the elongated grids, so the rotated grids are made with maxit = K_ROT and all K_ROT
iterations are compared."""
import math

import numpy as np

import few_workgroups_cases as fw
import stopping_sums_cases as sc

K_ROT = 6
MAXIT = 50
EPS = 1e-5


def _fw(shape):
    return dict(name="fw_" + "x".join(map(str, shape)), kind="fw", nodes=tuple(shape), dim=3, cell=False, rotated=False, maxit=MAXIT, n_src=fw.N_SRC,
                dtypes=tuple(np.dtype(d) for d in fw.DTYPES))


def _sc(c, n_src):
    assert not c["weno"]
    return dict(c, kind="sc", rotated=False, maxit=MAXIT, n_src=n_src)


def _rot(nodes, n_src, seed, z0=0.0, dtypes=(np.float32,)):
    c = sc._case("rot_" + "x".join(map(str, nodes)), nodes, dx=0.25, seed=seed, dtypes=dtypes)
    return dict(c, kind="sc", rotated=True, maxit=K_ROT, n_src=n_src, z0=z0)


# 2-D patches are 64 columns along x (one wavefront), marched along z
N2D_XZ = sc._case("n2d_65x130", (65, 130), dx=0.2, dz=0.3, seed=41)      # dx != dz: update2_xz; 65 columns: a patch of 64 and one of 1
N2D_REM = sc._case("n2d_130x65", (130, 65), dx=0.25, seed=42)            # dx = dz: update2; 130 columns: 64 + 64 + 2
CELLS2D = dict(sc.BY_NAME["weno_cells2d_131x67"], name="cells2d_131x67", weno=False, smooth=False, seed=43)   # the 2-D cell grid, first order

CASES = [_fw(s) for s in fw.SHAPES]
CASES += [_sc(sc.BY_NAME["cells_21x20x24"], 2), _sc(CELLS2D, 2), _sc(sc.BY_NAME["n2d_151x71"], 2), _sc(N2D_XZ, 2), _sc(N2D_REM, 2)]
CASES += [
    _rot((1201, 150), 2, 77, z0=1.0, dtypes=(np.float32, np.float64)),   # two strips of the strip kernel (1022 / 510 columns)
    _rot((8192, 64), 1, 78),
    _rot((64, 8192), 1, 79),
    _rot((2051, 40), 2, 80),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
ROWS = [(c["name"], dt) for c in CASES for dt in c["dtypes"]]
ROW_IDS = ["%s-%s" % (n, dt.name) for n, dt in ROWS]


def n_nodes(c):
    return int(np.prod(c["nodes"]))


def axes(c, dt):
    """node coordinates handed to Grid3d / Grid2d"""
    if c["kind"] == "fw":
        return fw.axes(c["nodes"])
    ax, _ = sc.axes(c, dt)
    if c["rotated"]:
        ax[1] = (c["z0"] + np.arange(c["nodes"][1]) * c["dz"]).astype(np.dtype(dt))
    return ax


def origin(c):
    return (0.0, c["z0"]) if c["rotated"] else (0.0,) * c["dim"]


def slowness(c, dt):
    """(nx, ny, nz) / (nx, nz) node or cell slowness as handed to set_slowness"""
    if c["kind"] == "fw":
        return fw.slowness(c["nodes"], dt)
    if c["rotated"]:
        return np.random.default_rng(c["seed"]).uniform(0.25, 1.0, c["nodes"])
    return sc.slowness(c)


def sources(c):
    """(n_src, dim) source points, off the nodes"""
    if c["kind"] == "fw":
        return fw.sources(c["nodes"])
    return sc.sources(c, c["n_src"]) + np.array(origin(c))


def flat(c, a):
    """an (nx, ny, nz) / (nx, nz) array in the solver's flat order"""
    return a.flatten("F") if c["dim"] == 3 else a.ravel()


def solve(oracle, c, dt, source, maxit):
    """the oracle's solve of one source with at most maxit iterations (eps = 1e-5, the grids' default)"""
    dt = np.dtype(dt)
    nc = tuple(n - 1 for n in c["nodes"])
    s = flat(c, slowness(c, dt))
    src = sources(c)[source:source + 1]
    if c["kind"] == "fw":
        return oracle.solve3d(dt, nc, fw.DX, origin(c), s, src, eps=EPS, maxit=maxit)
    _, d = sc.axes(c, dt)
    if c["dim"] == 3:
        return oracle.solve3d(dt, nc, d[0], origin(c), s, src, eps=EPS, maxit=maxit, cell_slowness=c["cell"])
    return oracle.solve2d(dt, nc, d[0], d[1], origin(c), s, src, eps=EPS, maxit=maxit, cell_slowness=c["cell"], rotated=c["rotated"])


def exact_decrease(prev, cur):
    """the exact value of sum_n (prev[n] - cur[n]), correctly rounded to a float: the differences in long double (asserted exact), added
    with math.fsum.  Asserts prev >= cur everywhere: first-order sweeps only lower a node."""
    prev, cur = np.asarray(prev), np.asarray(cur)
    assert prev.shape == cur.shape and prev.dtype == cur.dtype
    assert np.all(np.isfinite(prev)) and np.all(np.isfinite(cur))
    assert np.all(prev >= cur), "a node went up"
    a, b = prev.astype(np.longdouble), -cur.astype(np.longdouble)
    d = a + b
    # exact terms: the rounding error of the long-double difference (Knuth's TwoSum) is zero, and the difference survives the way
    # through float64 unchanged, so fsum sees the true differences
    a1 = d - b
    b1 = d - a1
    assert not np.any((a - a1) + (b - b1)), "a long-double difference was rounded"
    d64 = d.astype(np.float64)
    assert np.array_equal(d64.astype(np.longdouble), d), "a difference does not fit a float64"
    return math.fsum(d64.tolist())


_FIELDS = {}


def fields(oracle, c, dt, source):
    """dict(F, E, niter, change, tt): F[k] the oracle's field after k iterations (k = 1 ... K = niter of the plain solve; F[0] is None),
    E[k] = exact_decrease(F[k-1], F[k]) for k >= 2 (NaN below), and the plain solve's niter, change history and field.  Computed once
    per (case, dtype, source) and shared: do not modify."""
    dt = np.dtype(dt)
    key = (c["name"], dt.name, int(source))
    if key in _FIELDS:
        return _FIELDS[key]
    plain = fw.reference(oracle, c["nodes"], dt, source) if c["kind"] == "fw" else solve(oracle, c, dt, source, c["maxit"])
    K = plain["niter"]
    assert 1 <= K <= c["maxit"]
    F, E = [None], [math.nan, math.nan]
    for k in range(1, K + 1):
        o = solve(oracle, c, dt, source, k)
        assert o["niter"] == k, (key, k, o["niter"])
        assert np.array_equal(o["change"], plain["change"][:k]), (key, k)
        o["tt"].flags.writeable = False
        F.append(o["tt"])
        if k >= 2:
            E.append(exact_decrease(F[k - 1], F[k]))
    # the plain solve needed K iterations: its field is the one after K
    assert np.array_equal(F[K], plain["tt"]), key
    out = dict(F=F, E=E, niter=K, change=np.asarray(plain["change"]), tt=plain["tt"])
    _FIELDS[key] = out
    return out


def unit_roundoff(dt):
    return 0.5 * float(np.finfo(np.dtype(dt)).eps)


def gamma(dt, n):
    """bound on the relative error of a sequential sum of n non-negative terms in dt"""
    nu = n * unit_roundoff(dt)
    return nu / (1.0 - nu)


def geom(shape):
    """NF, NJ, NK as the host's constructor sets them (GridT::GridT, fsm_capi.hip): 3-D (nx, ny, nz); 2-D F = z, J = x, NK = 1"""
    return tuple(shape) if len(shape) == 3 else (shape[1], shape[0], 1)


def bar(dt, shape):
    """the relative distance from the exact decrease that the host allows the fp64 sum of the sweep kernels: m of decide_go_on; fp64: also
    what the window 1 +- 1e-6 leaves once the reference's own sum has taken gamma(N) of it -- the smaller of the two"""
    dt = np.dtype(dt)
    m = 2.0 * (sum(geom(shape)) + 64) * unit_roundoff(dt) + 1e-6
    if dt == np.float64:
        return min(m, 1e-6 - gamma(dt, int(np.prod(shape))))
    return m
