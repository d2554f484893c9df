"""Inputs of the field tape's edge tests (tests/test_field_tape_edges.py on the CPU, tests/test_field_tape_edges_gpu.py on the device): grid
shapes against the tile edges of ttcr_amd/csrc/fsm_adjoint.hip, fields with exact ties between the two neighbours of a node, translated
origins and metric units, receivers that share nodes, long relaxations and more events than slots.  One table per class, a model builder,
receiver builders, the tie count and the checks both files share.  The definitions themselves are tests/adjoint_reference.py and
tests/tangent_reference.py; the comparison and the bounds are those of tests/test_tangent_gpu.py.

A case is a Case tuple: nodes per axis, spacing, origin, node slowness (flat, x fastest, float64) and its events -- each a dict with the
source points `pts` (k, 3), the origin time `t0` and the receivers `rcv` (n, 3).
"""
import collections

import numpy as np

import adjoint_reference as AR
import tangent_reference as TR
from test_tangent_gpu import DOT_TOL, STEP, TOL, _bits_equal  # noqa: F401  (the project's comparison and bounds, not restated)

ADJ_RING = 8                                                     # rows of the flag ring of relax_to_fixed_point
ADJ_EDGE = {np.dtype(np.float32): 14, np.dtype(np.float64): 10}   # interior edge of a relaxation tile of the adjoint
TAN_EDGE = {np.dtype(np.float32): 10, np.dtype(np.float64): 8}    # ... and of the tangent

Case = collections.namedtuple("Case", "name nn dx origin s events")

NN, DX = (21, 17, 25), 0.5   # the grid of the existing one-event tests: x 0..10, y 0..8, z 0..12
ZERO = (0.0, 0.0, 0.0)


def model(nn, dx, origin, kind, scale=1.0):
    """Node slowness, flat, x fastest.  `smooth` is the function of the existing field-tape tests evaluated at 0.5 * (node index) -- the
    same values at the same nodes whatever dx and origin are --, `rough` that times 1 +- 15 % noise, `homogeneous` 0.5 everywhere,
    `two_layers` 0.5 below the node plane k = nnz // 2 and 0.25 on and above it; all times `scale`."""
    ax = [0.5 * np.arange(n) for n in nn]   # (x - origin) / dx / 2, exactly
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    if kind in ("smooth", "rough"):
        s = 0.5 + 0.02 * X + 0.015 * Y + 0.03 * Z + 0.05 * np.sin(0.9 * X) * np.cos(0.7 * Y + 0.3 * Z)
        if kind == "rough":
            s = s * (1.0 + 0.15 * np.random.default_rng(11).uniform(-1, 1, s.shape))
    elif kind == "homogeneous":
        s = np.full(X.shape, 0.5)
    elif kind == "two_layers":
        s = np.where(Z < 0.5 * (nn[2] // 2), 0.5, 0.25)
    else:
        raise ValueError(kind)
    return (scale * s).flatten("F")


def at(nn, dx, origin, idx):
    """coordinates of points given in node-index units (fractions allowed)"""
    return np.asarray(origin, dtype=np.float64) + np.asarray(idx, dtype=np.float64) * dx


def special_receivers(nn, dx, origin):
    """receivers on a node, on a plane, on an edge, on the last planes, in the last corner and in the first one (SPECIAL_RCV of the
    existing tests, for any grid)"""
    hi = [n - 1 for n in nn]
    c = [h // 3 for h in hi]
    f = [min(c[a] + 0.6, hi[a] - 0.4) for a in range(3)]
    idx = [[c[0], c[1], c[2]], [c[0], f[1], f[2]], [c[0], c[1], f[2]], [hi[0], f[1], f[2]], [f[0], hi[1], hi[2]], hi, [0, 0, 0]]
    return at(nn, dx, origin, idx)


def random_receivers(nn, dx, origin, rng, n):
    hi = np.array(nn) - 1.0
    return at(nn, dx, origin, rng.uniform(0.3, hi - 0.3, (n, 3)))


def tile_receivers(nn, dx, origin, rng, edge=8, per_tile=2):
    """`per_tile` receivers inside every tile of `edge` nodes per axis (the smallest tile edge: every workgroup of every relaxation kernel
    then has receivers of its own); a tile that holds one node plane only gets its receivers on that plane"""
    out = []
    for tz in range(0, nn[2], edge):
        for ty in range(0, nn[1], edge):
            for tx in range(0, nn[0], edge):
                lo = np.array([tx, ty, tz], dtype=np.float64)
                hi = np.minimum(lo + edge - 1, np.array(nn) - 1.0)
                out.append(rng.uniform(lo, hi, (per_tile, 3)))
    return at(nn, dx, origin, np.vstack(out))


def receivers(nn, dx, origin, rng, n=6):
    return np.vstack([random_receivers(nn, dx, origin, rng, n), special_receivers(nn, dx, origin)])


def count_ties(T, nn):
    """(decisive, all): node triples along an axis whose two outer values are equal to the bit -- `all` of them, and the `decisive` ones,
    where the equal pair is also smaller than the node between: there the upwind choice is made by the tie rule alone"""
    T3 = np.asarray(T).reshape(nn[2], nn[1], nn[0])
    decisive = total = 0
    for a in range(3):
        n = T3.shape[a]
        if n < 3:
            continue
        lo, mid, hi = (np.take(T3, range(o, n - 2 + o), axis=a) for o in (0, 1, 2))
        eq = lo == hi
        total += int(np.sum(eq))
        decisive += int(np.sum(eq & (lo < mid)))
    return decisive, total


def _event(pts, rcv, t0=0.0):
    return dict(pts=np.asarray(pts, dtype=np.float64).reshape(-1, 3), t0=float(t0), rcv=np.asarray(rcv, dtype=np.float64).reshape(-1, 3))


# ---- a. grid shapes against the tile edges 8, 10 (twice) and 14: every edge meets tile - 1, tile, tile + 1, 2 tile and 2 tile + 1 on some
# axis, every axis is the short one at least once
SHAPES = [(2, 2, 2), (3, 40, 2), (2, 3, 57), (7, 9, 13), (8, 10, 14), (9, 11, 15), (16, 20, 28), (17, 21, 29), (29, 41, 31), (40, 2, 3)]


def shape_case(nn):
    """rough model, origin 0; event 0: an off-node source, event 1: a source in the last cell of the far corner; two receivers per 8^3
    tile and the special ones for each"""
    rng = np.random.default_rng(1000 + nn[0] * 10000 + nn[1] * 100 + nn[2])
    src0 = [np.floor(0.4 * (nn[a] - 1)) + (0.3, 0.6, 0.2)[a] for a in range(3)]
    src1 = [nn[a] - 1 - (0.7, 0.4, 0.8)[a] for a in range(3)]
    ev = [_event(at(nn, DX, ZERO, [p]), np.vstack([tile_receivers(nn, DX, ZERO, rng), special_receivers(nn, DX, ZERO)]), t0)
          for p, t0 in ((src0, 0.125), (src1, 0.0))]
    return Case("x".join(map(str, nn)), nn, DX, ZERO, model(nn, DX, ZERO, "rough"), ev)


# ---- b. ties: fields that are mirror images of themselves about node planes
# receivers on nodes of the symmetry planes x = 5, y = 4, z = 6 (node planes 10, 8, 12), on the line where two of them meet, and an
# off-node point of the plane x = 5
PLANE_RCV = [[10, 3, 5], [4, 8, 20], [7, 2, 12], [10, 8, 20], [10, 2.6, 15.4]]
TIES = {
    "centre_node": ("homogeneous", [[10, 8, 12]]),
    "face_node": ("homogeneous", [[0, 8, 12]]),
    "two_layers": ("two_layers", [[10, 8, 4]]),                                       # (the interface is the node plane k = 12)
    "symmetric_points": ("homogeneous", [[8.375, 8.25, 12.625], [11.625, 8.25, 12.625], [10, 4.75, 6.25]]),   # mirror plane i = 10
    "mirrored_nodes": ("homogeneous", [[6, 8, 12], [14, 8, 12]]),                      # mirror planes i = 10, j = 8, k = 12
}
# A tie decides something only where the equal pair is smaller than the node between (count_ties' first figure).  About a single point
# source the equal pairs straddle the symmetry planes, whose nodes are the EARLIER ones: those ties are inactive axes.  Where the fronts of
# two mirrored sources meet, the pair is the upwind one and the rule "the lower index wins" picks the neighbour.
DECISIVE_TIES = ("symmetric_points", "mirrored_nodes")


def tie_case(name):
    kind, src = TIES[name]
    rng = np.random.default_rng(41)
    rcv = np.vstack([receivers(NN, DX, ZERO, rng), at(NN, DX, ZERO, PLANE_RCV)])
    return Case(name, NN, DX, ZERO, model(NN, DX, ZERO, kind), [_event(at(NN, DX, ZERO, src), rcv)])


# ---- c. origin and units
ORIGINS = {
    "translated": ((-37.25, 1200.5, -3.125), 0.5, 1.0),
    "metric": ((1000.0, 2000.0, -500.0), 25.0, 1.0e-3),
}
ORIGIN_SOURCES = {"off_node": [6.6, 8.2, 11.4], "on_node": [8, 11, 6]}   # node-index units: SOURCES of the existing tests
ORIGIN_CASES = ["%s-%s" % (o, s) for o in sorted(ORIGINS) for s in sorted(ORIGIN_SOURCES)]


def origin_case(name):
    o, srcname = name.split("-")
    origin, dx, scale = ORIGINS[o]
    rng = np.random.default_rng(43)
    return Case(name, NN, dx, origin, model(NN, dx, origin, "smooth", scale),
                [_event(at(NN, dx, origin, [ORIGIN_SOURCES[srcname]]), receivers(NN, dx, origin, rng, 20))])


# ---- d. receivers that share nodes
def _dense_receivers(src):
    surf = [[i, j, 0] for i in range(NN[0]) for j in range(NN[1])]                    # all 357 nodes of the z-min plane
    dup = [[4.4, 6.6, 9.4]] * 50                                                      # 50 copies of one off-node point
    cell = 8 + np.random.default_rng(1).uniform(0.02, 0.98, (40, 3))                  # 40 points inside one cell
    return np.vstack([at(NN, DX, ZERO, surf), at(NN, DX, ZERO, dup), at(NN, DX, ZERO, cell), at(NN, DX, ZERO, [src]),
                      at(NN, DX, ZERO, [np.ceil(src)])])                               # ... one at the source, one on a frozen node


def shared_case(name):
    src = [6.6, 8.2, 11.4]
    s = model(NN, DX, ZERO, "rough")
    dense = _dense_receivers(src)
    assert dense.shape[0] == 357 + 50 + 40 + 2
    if name == "one_event":
        return Case(name, NN, DX, ZERO, s, [_event(at(NN, DX, ZERO, [src]), dense)])
    # three events with interleaved rows: the dense set dealt at random to events 0 and 1, event 1 with an on-node source, event 2 with
    # a single receiver
    pick = np.random.default_rng(2).integers(0, 2, dense.shape[0]).astype(bool)
    return Case(name, NN, DX, ZERO, s, [_event(at(NN, DX, ZERO, [src]), dense[pick], 0.25),
                                        _event(at(NN, DX, ZERO, [[16, 4, 19]]), dense[~pick], 0.0),
                                        _event(at(NN, DX, ZERO, [[12.4, 5.8, 8.8]]), at(NN, DX, ZERO, [[10.2, 10.4, 10.6]]), 0.5)])


SHARED_CASES = ["one_event", "three_events"]


def wide_weights(rng, n, dt):
    """random values times powers of two spanning 2^-12 .. 2^12: a chain summed in another order has other bits"""
    return (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 13, n)).astype(dt)


# ---- e. long runs: three events that finish at very different passes (a source in a corner cell, one at the centre, one on the far face)
LONG = {np.dtype(np.float32): (113, 97, 129), np.dtype(np.float64): (61, 53, 71)}   # no extent a multiple of 14, 10 or 8


def long_case(dt):
    nn = LONG[np.dtype(dt)]
    rng = np.random.default_rng(47)
    hi = [n - 1 for n in nn]
    srcs = [[0.4, 0.6, 0.2], [hi[0] // 2 + 0.3, hi[1] // 2 + 0.6, hi[2] // 2 + 0.2], [hi[0], 0.3 * hi[1] + 0.1, hi[2]]]
    return Case("long", nn, DX, ZERO, model(nn, DX, ZERO, "rough"),
                [_event(at(nn, DX, ZERO, [p]), receivers(nn, DX, ZERO, rng, 8), t0) for p, t0 in zip(srcs, (0.0, 0.25, 0.5))])


# ---- f. more events than slots
def slots_case():
    nn = (25, 27, 29)
    rng = np.random.default_rng(53)
    hi = np.array(nn) - 1.0
    return Case("slots", nn, DX, ZERO, model(nn, DX, ZERO, "rough"),
                [_event(at(nn, DX, ZERO, [rng.uniform(1.5, hi - 1.5)]), random_receivers(nn, DX, ZERO, rng, int(rng.integers(3, 8))),
                        round(float(rng.uniform(0, 0.5)), 3)) for _ in range(11)])


# ---- what the two test files share
def call_arrays(case, rng):
    """(source, rcv, aggregate_src, rows): the arrays of one raytrace_adjoint call for the events of a case.  One event: (t0, x, y, z)
    rows, its points aggregated.  Several: 5-column rows (event id, t0, x, y, z) with the events' receiver rows interleaved; rows[e] are
    the rows of rcv that belong to event e, in rcv order (the order of the tape's rows within an event)."""
    ev = case.events
    if len(ev) == 1:
        e = ev[0]
        src = np.column_stack([np.full(e["pts"].shape[0], e["t0"]), e["pts"]])
        return src, e["rcv"], True, [np.arange(e["rcv"].shape[0])]
    assert all(e["pts"].shape[0] == 1 for e in ev)
    ids = np.concatenate([np.full(e["rcv"].shape[0], k) for k, e in enumerate(ev)])
    rcv = np.vstack([e["rcv"] for e in ev])
    perm = rng.permutation(ids.size)
    ids, rcv = ids[perm], rcv[perm]
    src = np.column_stack([ids, np.array([e["t0"] for e in ev])[ids], np.vstack([e["pts"] for e in ev])[ids]])
    rows = [np.nonzero(ids == k)[0] for k in range(len(ev))]
    return src, rcv, False, rows


def reference_vjp(fields, case, dt, rcv, rows, w, fc):
    """AR.adjoint on given fields; w in rcv order (or None), fc (n_events, n_nodes) (or None)"""
    return AR.adjoint(fields, np.asarray(case.s, dtype=dt), case.dx, case.nn, case.origin, [e["pts"] for e in case.events],
                      rcvs=[rcv[r] for r in rows], ws=None if w is None else [w[r] for r in rows], field_cot=fc)


def reference_jvp(fields, case, dt, rcv, rows, ds):
    """TR.tangent on given fields: (dtt in rcv order, (n_events, n_nodes) field tangents)"""
    mus, dtts = TR.tangent(fields, np.asarray(case.s, dtype=dt), case.dx, case.nn, case.origin, [e["pts"] for e in case.events],
                           np.asarray(ds, dtype=dt), rcvs=[rcv[r] for r in rows])
    dtt = np.zeros(rcv.shape[0], dtype=dt)
    for r, d in zip(rows, dtts):
        dtt[r] = d
    return dtt, np.stack(mus)


def dot_errors(w, dtt, g_rcv, fc, mu, g_fld, ds):
    """relative |<w, J v> - <J^T w, v>|, receivers and field, in float64 arithmetic"""
    f8 = lambda a: np.asarray(a, dtype=np.float64).ravel()   # noqa: E731
    lhs_r, rhs_r = f8(w) @ f8(dtt), f8(g_rcv) @ f8(ds)
    lhs_f, rhs_f = f8(fc) @ f8(mu), f8(g_fld) @ f8(ds)
    return abs(lhs_r - rhs_r) / abs(rhs_r), abs(lhs_f - rhs_f) / abs(rhs_f)
