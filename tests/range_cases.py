"""Case table of tests/test_range_cases.py (CPU: oracle against the compiled reference, and the preconditions that make each case the
case it claims to be) and tests/test_range_gpu.py (device against the oracle): the sweep kernels away from numbers of order one.

Every other sweep test feeds slowness 0.2 ... 1.5, dx 0.1 ... 2.3 and traveltimes below 50.  The hand-written arithmetic of
ttcr_amd/csrc/fsm_kernels.h states range assumptions (sqrt_disc without range scaling, the fp32 "clearly 3-D" test of update3, the
2^73 bound of weno_axes, div_h2 without an infinity fix-up, fp32 products of update2_xz) that those numbers never approach.  Here:

  a  unit systems that are no powers of two: metres and s/m with UTM origins, ground-penetrating radar in s/m and in ns/m, ultrasound,
     planetary scale;
  b  slowness times 2^k: around the fp32 underflow (k <= -58) and overflow (k >= 58) of fh^2, u^2, v^2 in update3, and k = 34, 37, 40
     with the WENO second differences on both sides of 2^36.5 (spans on both sides of 2^73); each k with eps = 1e-5 (the stopping rule
     then fires at another iteration than at k = 0) and with eps = 1e-5 2^k;
  c  dx times 2^m with the slowness fixed (source initialisation distances, interpolation weights, h2 and r2 of div_h2);
  d  contrasts and zeros: blocks of 1e12, of 1e-12, of exact 0.0 (ties), of the smallest fp32 subnormal, and an all-zero model;
  e  finite inputs whose fp32 candidates overflow (k = 100, 122: nodes stay at the unreached sentinel) and subnormal models
     (k = -120, -140 with eps = 0: all 50 iterations on subnormal fields).  Node grids only.

Non-finite and negative slowness are outside the kernels' precondition (include/ttcr_amd.h, ttcr_fsm_set_slowness) and not here.

Grids: two patches and a remainder along every patched axis.  Points are given in node-index units (like field_tape_cases.at) so that
they follow dx and the origin.  Rows on which the oracle cannot judge are listed in DISAGREE.  Pure numpy; reads nothing outside the
repository."""
import time

import numpy as np

GRIDS = {
    # name: (node counts, cell slowness, dx, dz)
    "n3": ((19, 21, 35), False, 1.0, 1.0),
    "c3": ((19, 21, 35), True, 1.0, 1.0),       # 18 x 20 x 34 cells
    "n2": ((70, 45), False, 1.0, 1.0),
    "x2": ((70, 45), False, 1.0, 0.4),          # dx != dz, ratio 2.5: update2_xz
    "c2": ((70, 45), True, 1.0, 1.0),           # 69 x 44 cells
}
SOURCES = {   # node-index units; the second point of "two" fires 0.3 s dx later
    3: {"off": [[6.6, 8.2, 11.4]], "node": [[8, 11, 6]], "two": [[3.3, 4.4, 5.5], [3.9, 4.1, 6.2]]},
    2: {"off": [[23.3, 17.9]], "node": [[20, 30]], "two": [[10.3, 8.4], [10.9, 8.1]]},
}
KINDS = ("off", "node", "two")
BLOCK = {3: (slice(5, 12), slice(6, 15), slice(9, 24)), 2: (slice(20, 45), slice(12, 30))}
# a slot inside the block, one node thick, that keeps the model's values: its nodes lie between two block nodes -- of equal traveltime
# when the block is 0.0, so that the upwind choice there is made by the tie rule alone (cell grids: the block only)
SLOT = {3: (8, slice(8, 13), slice(12, 21)), 2: (30, slice(15, 27))}
TINY32 = float(np.finfo(np.float32).smallest_subnormal)
K_B = (-40, -60, -62, -66, -72, 34, 37, 40, 58, 62, 64)
K_B_XZ = (-40, -60, 40, 55)
K_WENO_SPAN = (34, 37, 40)
K_OVER = (65, 66, 80)

DTYPES = [np.dtype(np.float32), np.dtype(np.float64)]
CASES = []


def _add(name, cls, grid, model="rough", scale=1.0, dx_scale=1.0, dx=None, dz=None, origin=None, translate=False, eps=1e-5, block=None,
         k=None, eps_scaled=None):
    nodes, cell, gdx, gdz = GRIDS[grid]
    dim = len(nodes)
    dx = gdx * dx_scale if dx is None else dx
    dz = (gdz * dx_scale if dz is None else dz) if dim == 2 else dx
    c = dict(name=name, cls=cls, grid=grid, dim=dim, nodes=nodes, cell=cell, model=model, scale=float(scale), dx=float(dx), dz=float(dz),
             origin=tuple(float(v) for v in (origin or (0.0,) * dim)), translate=bool(translate), eps=float(eps), maxit=50, block=block,
             k=k, eps_scaled=eps_scaled, kind=KINDS[len(CASES) % 3], alt=KINDS[(len(CASES) + 1) % 3])
    assert name not in [q["name"] for q in CASES], name
    CASES.append(c)


# ---- a. unit systems ------------------------------------------------------------------------------------------------------------------
UNITS = [("metric_utm", 25.0, 6e-4, 1e-5, 10.0), ("gpr_s_per_m", 0.05, 1e-8, 1e-15, 0.02), ("gpr_ns_per_m", 0.05, 10.0, 1e-5, None),
         ("ultrasound", 2e-4, 7e-4, 1e-12, 1e-4), ("planet", 100.0, 0.2, 1e-5, None)]
for _i, (_n, _dx, _s, _eps, _dz) in enumerate(UNITS):
    for _g in ("n3", "c3", "n2", "c2"):
        _o = None
        if _n == "metric_utm":
            _o = (500000.0, 4000000.0, -1000.0) if _g.endswith("3") else (500000.0, -1000.0)
        _add("%s-%s" % (_n, _g), "a", _g, model=("rough", "smooth")[_i % 2], scale=_s, dx=_dx, dz=_dx, origin=_o, eps=_eps)
    if _n == "metric_utm":
        _add("metric_utm_translated-n3", "a", "n3", model="smooth", scale=_s, dx=_dx, origin=(500000.0, 4000000.0, -1000.0), translate=True,
             eps=_eps)
    if _dz is not None:
        _add("%s-x2" % _n, "a", "x2", scale=_s, dx=_dx, dz=_dz, origin=(500000.0, -1000.0) if _n == "metric_utm" else None, eps=_eps)

# ---- b. powers of two on slowness -----------------------------------------------------------------------------------------------------
for _g, _ks in (("n3", K_B), ("n2", K_B), ("x2", K_B_XZ), ("c3", (-66, 37, 62)), ("c2", (-66, 37, 62))):
    for _k in _ks:
        for _sc in ((False, True) if _g in ("n3", "n2", "x2") else (True,)):
            _add("k%+d-%s-%s" % (_k, "eps_scaled" if _sc else "eps_fixed", _g), "b", _g, model="smooth" if _k == 37 and _g == "n2" else "rough",
                 scale=2.0 ** _k, eps=1e-5 * 2.0 ** _k if _sc else 1e-5, k=_k, eps_scaled=_sc)

# ---- c. powers of two on dx -----------------------------------------------------------------------------------------------------------
for _g in ("n3", "c3", "n2", "x2"):
    for _m in (-40, 40):
        _add("dx%+d-%s" % (_m, _g), "c", _g, model=("rough", "smooth")[_m > 0], dx_scale=2.0 ** _m, eps=1e-5 * 2.0 ** _m, k=_m)

# ---- d. contrasts and zeros -----------------------------------------------------------------------------------------------------------
for _g in ("n3", "n2"):
    _add("block_1e12-" + _g, "d", _g, block=1e12)
    _add("block_1e-12-" + _g, "d", _g, block=1e-12)
    _add("block_zero-" + _g, "d", _g, block=0.0)
    _add("all_zero-" + _g, "d", _g, scale=0.0)
    _add("block_subnormal-" + _g, "d", _g, block=TINY32)
_add("block_zero-c3", "d", "c3", block=0.0)
_add("block_zero-x2", "d", "x2", block=0.0)
_add("block_1e12-c2", "d", "c2", block=1e12)

# ---- e. overflowing candidates, subnormal models: node grids --------------------------------------------------------------------------
for _g in ("n3", "n2"):
    for _k in (100, 122):
        _add("k%+d-%s" % (_k, _g), "e", _g, scale=2.0 ** _k, eps=1e-5 * 2.0 ** _k, k=_k)
    for _k in (-120, -140):
        _add("k%+d-eps0-%s" % (_k, _g), "e", _g, scale=2.0 ** _k, eps=0.0, k=_k)

# ---- b, continued: fh^2 itself overflows fp32 (s dx >= 2^64): at some nodes (k = 65), at all; the reference then leaves nodes unreached ---
for _k in K_OVER:
    _add("k%+d-eps_scaled-n3" % _k, "b", "n3", scale=2.0 ** _k, eps=1e-5 * 2.0 ** _k, k=_k, eps_scaled=True)

BY_NAME = {c["name"]: c for c in CASES}

# Rows (case, dtype, order) on which the oracle and the compiled reference DISAGREE (tests/test_range_cases.py found them): the oracle
# cannot judge the device there, so they are no rows of either test.  All are fp32 WENO runs of 2-D grids that do not converge (50 WENO
# iterations, traveltimes driven negative), in which squares or products leave the fp32 range.
DISAGREE = {(n, "float32", True): why for n, why in [
    ("k+62-eps_fixed-n2", "99 % of the nodes differ after 50 WENO iterations"), ("k+62-eps_scaled-n2", "99 % of the nodes differ"),
    ("k+64-eps_fixed-n2", "49 % of the nodes differ"), ("k+64-eps_scaled-n2", "99 % of the nodes differ"),
    ("dx-40-x2", "dx^2 dx^2 underflows: nodes differ from the first WENO iteration on"), ("dx+40-x2", "two nodes differ"),
    ("block_zero-x2", "nodes differ from the first WENO iteration on"), ("k+100-n2", "two nodes differ"), ("k+122-n2", "two nodes differ")]}
# ... and one RECEIVER: with dx = 0.05 in fp32 the last node coordinate, 0.9f, lies 7e-7 cells below the last plane as the grid computes
# it (18 * 0.05f), further than the reference's absolute 1e-8 "on the plane" test allows: the reference takes the last node as the lower
# index and reads one node past the row (oracle/fsm_oracle_impl.h, fsm_interp3d: oracle and kernel clamp).  No result is defined there;
# the two gpr systems do without that receiver.
NO_FAR_X_RECEIVER = ("gpr_s_per_m", "gpr_ns_per_m")


def rows(cases=None):
    """(case, dtype, weno) rows of the two tests"""
    return [(c, dt, w) for c in (CASES if cases is None else cases) for dt in DTYPES for w in (False, True) if (c["name"], dt.name, w) not in DISAGREE]

WALK_CASE = "metric_utm_translated-n3"   # the raypath calls: a smooth model


def rot_ok(c):
    """sweep45 exists for 2-D square cells"""
    return c["dim"] == 2 and c["dx"] == c["dz"]


def n_cells(c):
    return tuple(n - 1 for n in c["nodes"])


def axes(c, dt):
    """node coordinates as the wrapper keeps them (cast to the grid's dtype), and the steps it derives from them"""
    dt = np.dtype(dt)
    d = [c["dx"]] * 3 if c["dim"] == 3 else [c["dx"], c["dz"]]
    ax = [(o + np.arange(n) * h).astype(dt) for o, n, h in zip(c["origin"], c["nodes"], d)]
    return ax, [float(a[1] - a[0]) for a in ax]


def _base(c):
    """the two models on the case's slowness points, values 0.25 ... 1.0, as an array of the grid's shape"""
    shape = n_cells(c) if c["cell"] else c["nodes"]
    if c["model"] == "rough":
        return np.random.default_rng(1000 + sorted(GRIDS).index(c["grid"])).uniform(0.25, 1.0, shape)
    g = np.meshgrid(*[0.5 * (np.arange(n) + (0.5 if c["cell"] else 0.0)) for n in shape], indexing="ij")
    s = 0.3 + 0.65 / (1.0 + 0.12 * g[-1])
    ripple = np.sin(0.4 * g[0]) * (np.cos(0.3 * g[1]) if c["dim"] == 3 else 1.0)
    return np.clip(s * (1.0 + 0.05 * ripple), 0.25, 1.0)


def slowness_array(c):
    """float64 array of shape (nx, ny, nz) / (nx, nz) (cells: one less along every axis), as Grid3d / Grid2d take it"""
    s = _base(c) * c["scale"]
    if c["block"] is not None:
        keep = s[SLOT[c["dim"]]].copy()
        s[BLOCK[c["dim"]]] = c["block"]
        if not c["cell"]:
            s[SLOT[c["dim"]]] = keep
    return s


def flat(c, a):
    """an array of the grid's shape in the solver's flat order (3-D: x fastest, 2-D: z fastest)"""
    return a.flatten("F") if c["dim"] == 3 else a.ravel()


def at(dx, origin, idx):
    """coordinates of points given in node-index units (fractions allowed), as field_tape_cases.at gives them"""
    return np.asarray(origin, dtype=np.float64) + np.asarray(idx, dtype=np.float64) * dx


def _inside(c, dt, idx):
    """points given in node-index units, never beyond the last planes as the grid computes them (xmin + ncx dx in the grid's dtype)"""
    dt = np.dtype(dt)
    ax, d = axes(c, dt)
    p = at(np.array([c["dx"]] * 3 if c["dim"] == 3 else [c["dx"], c["dz"]]), c["origin"], idx)
    lo = np.array([float(a[0]) for a in ax])
    hi = np.array([float(dt.type(a[0]) + dt.type(n - 1) * dt.type(h)) for a, n, h in zip(ax, c["nodes"], d)])
    hi = np.minimum(hi, [float(a[-1]) for a in ax])
    return np.clip(p.astype(dt).astype(np.float64), lo, hi)


def source(c, dt, kind=None):
    """(points, origin times) of the case's source, or of its source of another kind"""
    kind = c["kind"] if kind is None else kind
    pts = _inside(c, dt, SOURCES[c["dim"]][kind])
    t0 = np.zeros(len(pts))
    if len(pts) > 1:
        t0[1] = 0.3 * c["scale"] * c["dx"]
    return pts, t0


def source_rows(c, dt, kind=None):
    """ttcrpy-style rows (t0, x, y, z) of one event"""
    pts, t0 = source(c, dt, kind)
    return np.hstack([t0[:, None], pts])


def receivers(c, dt):
    """on a node, inside a cell, on the far faces, in the first corner"""
    hi = [n - 1 for n in c["nodes"]]
    if c["dim"] == 3:
        idx = [[5, 7, 11], [6.4, 8.3, 20.6], [hi[0], 3.3, 9.7], [4.2, hi[1], hi[2]], [0, 0, 0]]
    else:
        idx = [[31, 12], [40.4, 20.6], [hi[0], 9.7], [14.2, hi[1]], [0, 0]]
    if c["name"].split("-")[0] in NO_FAR_X_RECEIVER:
        del idx[2]
    return _inside(c, dt, idx)


_SOLVED = {}


def solve(O, c, dt, weno, rotated=False, kind=None, ref=False, maxit=None, **kw):
    """the oracle's (ref: the compiled reference's) solve of the case; kept, and read-only"""
    dt = np.dtype(dt)
    maxit = c["maxit"] if maxit is None else maxit
    key = (c["name"], dt.name, bool(weno), bool(rotated), kind, bool(ref), maxit, tuple(sorted(kw.items())))
    if key in _SOLVED:
        return _SOLVED[key]
    _, d = axes(c, dt)
    pts, t0 = source(c, dt, kind)
    args = dict(slowness=flat(c, slowness_array(c)), src=pts, t0=t0, eps=c["eps"], maxit=maxit, cell_slowness=c["cell"],
                rcv=receivers(c, dt), weno=bool(weno), **kw)
    t = time.perf_counter()
    if c["dim"] == 3:
        f = O.ref_solve3d if ref else O.solve3d
        o = f(dt, n_cells(c), d[0], c["origin"], translate=c["translate"], **args)
    else:
        f = O.ref_solve2d if ref else O.solve2d
        o = f(dt, n_cells(c), d[0], d[1], c["origin"], rotated=bool(rotated), **args)
    o["seconds"] = time.perf_counter() - t
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    _SOLVED[key] = o
    return o


# ---- what the preconditions of tests/test_range_cases.py count --------------------------------------------------------------------------
def node_field(c, a):
    """a flat node array as (nx, ny, nz) / (nx, nz)"""
    return np.asarray(a).reshape(c["nodes"], order="F" if c["dim"] == 3 else "C")


def fh32(c, o):
    """fp32 s dx of every node (3-D and square 2-D cells: the fh of update3 / update2)"""
    return (np.asarray(o["node_slowness"], dtype=np.float32) * np.float32(axes(c, np.float32)[1][0])).astype(np.float32)


def upwind_spread(c, T):
    """u = a3 - a1 of update3 on a converged fp32 field: the axis minima of every node (one-sided on the faces), their largest minus their
    smallest"""
    T = node_field(c, np.asarray(T, dtype=np.float32))
    big = np.float32(np.finfo(np.float32).max)
    mins = []
    for a in range(T.ndim):
        pad = [(1, 1) if b == a else (0, 0) for b in range(T.ndim)]
        P = np.pad(T, pad, constant_values=big)
        n = T.shape[a]
        mins.append(np.minimum(np.take(P, range(0, n), axis=a), np.take(P, range(2, n + 2), axis=a)))
    m = np.stack(mins)
    with np.errstate(over="ignore"):
        return (m.max(axis=0) - m.min(axis=0)).astype(np.float32)


def weno_spans(c, T):
    """eps + den^2 of weno_pre (fsm_kernels.h) on a fp32 field: den = (p1 - 2 c) + m1 in double, rounded to fp32, squared in fp32; the
    largest over the axes, interior nodes of every axis"""
    T = node_field(c, np.asarray(T, dtype=np.float32)).astype(np.float64)
    eps = np.float32(1.1920928955078125e-07)
    out = None
    for a in range(T.ndim):
        n = T.shape[a]
        m1, cc, p1 = (np.take(T, range(o, n - 2 + o), axis=a) for o in (0, 1, 2))
        den = ((p1 - 2.0 * cc) + m1).astype(np.float32)
        with np.errstate(over="ignore"):
            B = (eps + den * den).astype(np.float32)
        B = B[tuple(slice(None) if b == a else slice(1, -1) for b in range(T.ndim))]
        out = B if out is None else np.maximum(out, B)
    return out


def exact_decreases(O, c, dt):
    """E[k], k = 2 ... niter: the exact decrease of iteration k of the case's first-order solve (change_sum_cases.exact_decrease of the
    oracle's fields after k - 1 and after k iterations); E[0] = E[1] = NaN, and NaN for every later iteration in which a node left the
    unreached value max(): like iteration 1, such an iteration is outside what the host's bound covers (tests/test_change_sum_gpu.py)"""
    from change_sum_cases import exact_decrease

    K = solve(O, c, dt, False)["niter"]
    F = [None] + [solve(O, c, dt, False, maxit=k)["tt"] for k in range(1, K + 1)]
    assert np.array_equal(F[K], solve(O, c, dt, False)["tt"])
    big = np.finfo(np.dtype(dt)).max
    return [np.nan, np.nan] + [np.nan if np.any((F[k - 1] == big) & (F[k] != big)) else exact_decrease(F[k - 1], F[k]) for k in range(2, K + 1)]
