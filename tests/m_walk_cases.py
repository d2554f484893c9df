"""Inputs of the edge tests of the recording ray walks and of the M tape's merge (tests/test_m_walk_edges.py on the CPU, proving the tables
against the oracle; tests/test_m_walk_edges_gpu.py on the device): receiver rows without records, walks along the far faces, sources of
many points in one cell, receivers that share nodes, thin grids and moved origins -- and the two things only a buffer size can reach on a
small grid: a walk longer than its row, which is walked again alone (status 3), and a call whose receivers do not fit one launch (the
seams between chunks).  Option "walk_records" (include/ttcr_amd.h) sets that size; no result may depend on it.

A case is a field_tape_cases.Case; model, receiver builders and weights are that module's.  An event's `t0` is a number, or one value per
source point.  The reference of every check is the oracle: `reference(oracle, ...)` keeps the receivers whose walk the oracle finishes
(the reference throws, or never returns, for the others) and returns its results for them, computed once per case and dtype.
"""
import collections

import numpy as np

import field_tape_cases as FC
from field_tape_cases import DX, NN, ZERO, Case, at, model, special_receivers, wide_weights  # noqa: F401  (reused, not restated)

SRC = [6.6, 8.2, 11.4]                     # the off-node source of the existing one-event tests, node-index units
HI = tuple(n - 1 for n in NN)
WALK_STEP_LIMIT = 1000000                 # GridBase::walk_step_limit, the largest walk_records


def _event(pts, rcv, t0=0.0):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    t0 = float(t0) if np.ndim(t0) == 0 else np.asarray(t0, dtype=np.float64)
    return dict(pts=pts, t0=t0, rcv=np.asarray(rcv, dtype=np.float64).reshape(-1, 3))


def event_t0(ev):
    """one origin time per source point"""
    return np.broadcast_to(np.asarray(ev["t0"], dtype=np.float64), (ev["pts"].shape[0],)).copy()


# ---- a. receiver rows without records: a receiver exactly on the source point has no entries and tt = 0
def _with_empty_rows(src, rcv):
    """the source point first, last and three times in a row in the middle of the receivers; (receivers, indices of the empty rows)"""
    h = rcv.shape[0] // 2
    out = np.vstack([src, rcv[:h], src, src, src, rcv[h:], src])
    return out, [0, h + 1, h + 2, h + 3, out.shape[0] - 1]


def empty_case(name):
    """(case, empty rows per event)"""
    rng = np.random.default_rng(83)
    s = model(NN, DX, ZERO, "rough")
    src = at(NN, DX, ZERO, [SRC, [15.3, 4.4, 19.7], [3.2, 12.6, 5.1]])
    if name == "first_middle_last":
        rcv, empty = _with_empty_rows(src[:1], FC.random_receivers(NN, DX, ZERO, rng, 8))
        return Case(name, NN, DX, ZERO, s, [_event(src[0], rcv, 0.125)]), [empty]
    if name == "empty_event_between":
        r0, e0 = _with_empty_rows(src[:1], FC.random_receivers(NN, DX, ZERO, rng, 6))
        r2, e2 = _with_empty_rows(src[2:], FC.random_receivers(NN, DX, ZERO, rng, 4))
        return Case(name, NN, DX, ZERO, s, [_event(src[0], r0, 0.25), _event(src[1], np.repeat(src[1:2], 4, axis=0), 0.5),
                                            _event(src[2], r2, 0.0)]), [e0, [0, 1, 2, 3], e2]
    if name == "nothing_but_empty":
        return Case(name, NN, DX, ZERO, s, [_event(src[0], np.repeat(src[:1], 4, axis=0), 0.25)]), [[0, 1, 2, 3]]
    raise ValueError(name)


EMPTY_CASES = ["first_middle_last", "empty_event_between", "nothing_but_empty"]

# ---- b. far faces: receivers on the last planes, their edges, the far corner, on nodes of those planes and inside the last cells; an
# interior source, a source on a node of the x-max face and one in the last cell
FAR_RCV = [[HI[0], 5.3, 7.6], [HI[0], 11.5, 18.2], [6.4, HI[1], 9.7], [13.6, HI[1], 20.3], [4.7, 8.2, HI[2]], [15.1, 3.9, HI[2]],
           [HI[0], HI[1], 11.4], [HI[0], 7.7, HI[2]], [9.2, HI[1], HI[2]], list(HI),
           [HI[0], 8, 12], [10, HI[1], 12], [10, 8, HI[2]], [HI[0], HI[1], 12], [HI[0], 8, HI[2]],
           [19.3, 15.6, 23.2], [19.9, 15.1, 23.8], [19.5, 15.5, 23.5], [19.6, 4.4, 10.2], [7.3, 15.7, 3.3], [12.2, 9.1, 23.4]]
LAST_CELL_RCV = [[19.3, 15.6, 23.2], [19.9, 15.1, 23.8], [19.5, 15.5, 23.5], [19.1, 15.9, 23.9], [19.8, 15.8, 23.1], [19.2, 15.2, 23.7],
                 [19.7, 15.4, HI[2]], [HI[0], 15.3, 23.4], [19.6, HI[1], 23.3], list(HI)]
FAR_SOURCES = [(SRC, 0.0), ([HI[0], 9, 13], 0.25), ([19.4, 15.3, 23.6], 0.5)]


def far_case():
    """event 0: the interior source with every receiver of FAR_RCV; event 1: a source on a node of the x-max face with those that do not
    lie next to that face themselves (a walk along the face of its source leaves the grid, see e.); event 2: a source in the last cell
    with receivers in that cell and on its far faces -- their walks touch the last planes, where the node index runs past the grid"""
    rcv = at(NN, DX, ZERO, FAR_RCV)
    off_face = at(NN, DX, ZERO, [p for p in FAR_RCV if p[0] < HI[0] - 1])
    return Case("far_faces", NN, DX, ZERO, model(NN, DX, ZERO, "rough"),
                [_event(at(NN, DX, ZERO, [p]), r, t0) for (p, t0), r in zip(FAR_SOURCES, (rcv, off_face, at(NN, DX, ZERO, LAST_CELL_RCV)))])


# ---- c. one source of 12 points inside one cell, distinct origin times: the end game of a walk serves several points, their terms meet
# at the same eight nodes
N_POINTS = 12


def points_case():
    rng = np.random.default_rng(89)
    pts = np.floor(SRC) + rng.uniform(0.05, 0.95, (N_POINTS, 3))
    t0 = np.round(rng.uniform(0.0, 0.5, N_POINTS), 3) + 0.001 * np.arange(N_POINTS)
    assert np.unique(t0).size == N_POINTS
    return Case("points_in_one_cell", NN, DX, ZERO, model(NN, DX, ZERO, "rough"),
                [_event(at(NN, DX, ZERO, pts), FC.random_receivers(NN, DX, ZERO, rng, 20), t0)])


# ---- d. receivers that share nodes: field_tape_cases' dense set (a whole node plane, 50 copies of one point, 40 points in one cell)
SHARED_CASES = FC.SHARED_CASES
shared_case = FC.shared_case

# ---- e. shapes, origins, the WENO stage
# The walk of the reference follows the gradient of the field cell by cell and has no rule for a face of the grid: along a grid one or two
# cells thick, and from or towards a source next to a far face, most walks end with "going outside grid" after a few cells.  So the thin
# grids get their receivers within 2.5 cells of the source (walks of 3 to 6 records, and the thin extents are what they are there for), and
# the ordinary shape gets two interior sources with receivers in every 8^3 tile and the special ones.
THIN = [(2, 2, 2), (3, 40, 2), (2, 3, 57), (40, 2, 3)]
SHAPES = THIN + [NN]
ORIGIN_CASES = ["translated-off_node", "metric-off_node"]
THIN_REACH, THIN_RCV = 2.5, 16


def shape_case(nn):
    """rough model, origin 0, two events.  Thin grids: sources at 0.4 and 0.7 of the extents, THIN_RCV receivers within THIN_REACH cells
    of each and one on it; the ordinary shape: two interior sources, field_tape_cases' tile and special receivers for each."""
    rng = np.random.default_rng(2000 + nn[0] * 10000 + nn[1] * 100 + nn[2])
    hi = np.array(nn) - 1.0
    if tuple(nn) == NN:
        srcs = [SRC, [13.3, 4.6, 17.2]]
        rcvs = [np.vstack([FC.tile_receivers(nn, DX, ZERO, rng), special_receivers(nn, DX, ZERO)]) for _ in srcs]
    else:
        srcs = [[np.floor(f * hi[a]) + (0.3, 0.6, 0.2)[a] for a in range(3)] for f in (0.4, 0.7)]
        rcvs = [np.vstack([at(nn, DX, ZERO, rng.uniform(np.maximum(np.array(p) - THIN_REACH, 0.0), np.minimum(np.array(p) + THIN_REACH, hi),
                                                        (THIN_RCV, 3))), at(nn, DX, ZERO, [p])]) for p in srcs]
    return Case("x".join(map(str, nn)), nn, DX, ZERO, model(nn, DX, ZERO, "rough"),
                [_event(at(nn, DX, ZERO, [p]), r, t0) for p, r, t0 in zip(srcs, rcvs, (0.125, 0.0))])


# every case of a - e: name -> (builder of the case, weno)
CASES = collections.OrderedDict(
    [("empty-" + n, (lambda n=n: empty_case(n)[0], 0)) for n in EMPTY_CASES] +
    [("far_faces", (far_case, 0)), ("points_in_one_cell", (points_case, 0))] +
    [("shared-" + n, (lambda n=n: shared_case(n), 0)) for n in SHARED_CASES] +
    [("shape-" + "x".join(map(str, nn)), (lambda nn=nn: shape_case(nn), 0)) for nn in SHAPES] +
    [("shape-" + "x".join(map(str, NN)) + "-weno", (lambda: shape_case(NN), 1))] +
    [("origin-" + n, (lambda n=n: FC.origin_case(n), 0)) for n in ORIGIN_CASES])


# ---- f. seams and retraces: three events of 5, 17 and 9 receivers
SEAM_COUNTS = (5, 17, 9)
M_CHUNK = {np.dtype(np.float32): 13, np.dtype(np.float64): 6}      # receivers per launch of the M walks at walk_records = 1 000 000:
L_CHUNK = {np.dtype(np.float32): 16, np.dtype(np.float64): 8}      # 256 MiB / (sizeof(T) * 5 (L: 4) * (1 000 000 + 3 (L: 4)))
RAYS_CHUNK = {np.dtype(np.float32): 357, np.dtype(np.float64): 178}   # 4 GiB / (sizeof(T) * 3 * 1 000 003)


def seam_case():
    rng = np.random.default_rng(97)
    srcs = [SRC, [15.3, 4.4, 19.7], [3.2, 12.6, 5.1]]
    return Case("seams", NN, DX, ZERO, model(NN, DX, ZERO, "rough"),
                [_event(at(NN, DX, ZERO, [p]), FC.random_receivers(NN, DX, ZERO, rng, n), t0)
                 for p, n, t0 in zip(srcs, SEAM_COUNTS, (0.0, 0.25, 0.5))])


def rays_seam_case():
    """400 receivers in two events of one batch: at 357 rows per launch the seam falls inside the second event"""
    rng = np.random.default_rng(101)
    srcs = [SRC, [15.3, 4.4, 19.7]]
    return Case("rays_seam", NN, DX, ZERO, model(NN, DX, ZERO, "rough"),
                [_event(at(NN, DX, ZERO, [p]), FC.random_receivers(NN, DX, ZERO, rng, n), t0) for p, n, t0 in zip(srcs, (150, 250), (0.0, 0.25))])


def seams(counts, chunk):
    """rows of the call (events one after the other) at which a launch of the per-event walks ends inside an event"""
    out, base = [], 0
    for n in counts:
        out += [base + c for c in range(chunk, n, chunk)]
        base += n
    return out


def records(ray):
    """records of a walk whose ray has these points: one per point after the receiver (a receiver on the source: none)"""
    return max(len(ray) - 1, 0)


def m_retraced(rays, walk_records, n_tx=1):
    """walks of compute_M / the M tape that do not fit a row of walk_records + 2 n_tx + 1 records"""
    return [q for q, r in enumerate(rays) if records(r) > walk_records + 2 * n_tx + 1]


def rays_retraced(rays, walk_records):
    """rays that do not fit a row of walk_records + 3 points"""
    return [q for q, r in enumerate(rays) if len(r) > walk_records + 3]


def median_records(rays):
    return int(np.median([records(r) for r in rays]))


# ---- the 2-D cell grid of tests/test_parity_gpu.py (receivers next to its last planes) for compute_L
L_NN, L_DX, L_DZ, L_SRC = (12, 10), 2.3, 3.1, np.array([[3.0, 4.0]])
L_CORNER = 17   # row of the receiver 1.7e-4 inside the far corner among l_case's candidates


def l_case(dt):
    """(cell slowness (ncx, ncz), candidate receivers): on the far planes, 1 .. 500 representable numbers inside them, and 1.7e-4 inside
    the far corner -- the receiver whose ray has tens of thousands of points"""
    dt = np.dtype(dt).type
    x2, z2 = np.arange(L_NN[0]) * L_DX, np.arange(L_NN[1]) * L_DZ
    hi2 = np.minimum(np.array([dt(0) + dt(L_NN[0] - 1) * dt(L_DX), dt(0) + dt(L_NN[1] - 1) * dt(L_DZ)], dtype=dt),
                     np.array([dt(x2[-1]), dt(z2[-1])], dtype=dt))
    pts = [hi2.copy()]
    for ax in range(2):
        for back in (1, 3, 60, 500):
            p = hi2.copy()
            for _ in range(back):
                p[ax] = np.nextafter(p[ax], dt(0))
            pts.append(p.copy())
            q = p.copy()
            q[1 - ax] = dt(0.41 * hi2[1 - ax])
            pts.append(q)
    assert len(pts) == L_CORNER
    pts.append(hi2 - dt(1.7e-4))
    rng = np.random.default_rng(103)
    inner = rng.uniform([0.5, 0.5], [(L_NN[0] - 1) * L_DX - 0.5, (L_NN[1] - 1) * L_DZ - 0.5], (12, 2))
    sc = 1.0 / (1.0 + 0.05 * np.arange(L_NN[1] - 1))
    return np.ascontiguousarray(np.broadcast_to(sc[None, :], (L_NN[0] - 1, L_NN[1] - 1))), np.vstack([np.array(pts, dtype=np.float64), inner])


# ---- the arrays of a call
def call_arrays(case, seed=61):
    """field_tape_cases.call_arrays and, per event, `pick`: row i of rows[e] (the event's rows in call order, which is the order of the
    tape's rows within the event) is receiver pick[e][i] of the event -- the oracle's results are in the event's own order"""
    src, rcv, agg, rows = FC.call_arrays(case, np.random.default_rng(seed))
    if len(case.events) == 1:
        return src, rcv, agg, rows, [np.arange(rcv.shape[0])]
    stacked = np.vstack([e["rcv"] for e in case.events])
    perm = np.random.default_rng(seed).permutation(stacked.shape[0])   # (the shuffle FC.call_arrays draws first)
    assert np.array_equal(rcv, stacked[perm])
    base = np.concatenate([[0], np.cumsum([e["rcv"].shape[0] for e in case.events])])
    return src, rcv, agg, rows, [perm[rows[e]] - base[e] for e in range(len(case.events))]


# ---- the oracle's side
def finished(solve, rcv):
    """indices of the receivers whose walk the oracle finishes.  solve(rcv) raises for a call that holds a walk which leaves the grid or
    never reaches the source, like the reference: the call is halved until those stand alone."""
    def part(idx):
        try:
            solve(rcv[idx])
            return list(idx)
        except RuntimeError as e:
            assert "going outside grid" in str(e) or "did not reach the source" in str(e), e
            if len(idx) == 1:
                return []
            h = len(idx) // 2
            return part(idx[:h]) + part(idx[h:])
    return part(np.arange(rcv.shape[0]))


_REFERENCE = {}


def reference(oracle, name, case, dt, weno=0, rays=False):
    """(case with the receivers the oracle finishes, oracle results per event, candidates per event) -- computed once per (name, dtype,
    weno, rays) and shared: nobody changes them.  rays: the overloads with r_data as well (keys rm: r_data + m_data, r: r_data alone)."""
    key = (name, np.dtype(dt).name, int(weno), bool(rays))
    if key not in _REFERENCE:
        nc = tuple(n - 1 for n in case.nn)
        events, results, candidates = [], [], []
        for ev in case.events:
            def solve(rcv, **kw):
                return oracle.solve3d(dt, nc, case.dx, case.origin, case.s, ev["pts"], t0=event_t0(ev), rcv=rcv, weno=bool(weno), **kw)
            keep = finished(lambda r: solve(r, compute_m=True), ev["rcv"])
            kept = dict(ev, rcv=ev["rcv"][keep])
            o = dict(m=solve(kept["rcv"], compute_m=True))
            if rays:
                o["rm"] = solve(kept["rcv"], compute_m=True, return_rays=True)
                o["r"] = solve(kept["rcv"], return_rays=True)
            events.append(kept)
            results.append(o)
            candidates.append(ev["rcv"].shape[0])
        _REFERENCE[key] = (case._replace(events=events), results, candidates)
    return _REFERENCE[key]


def oracle_rows(o, n_nodes):
    """the rows of an oracle result as compute_M's Python layer keeps them: (columns, values) per receiver, entries past the grid dropped,
    columns ascending, the entries of a column in push order (there is one: the walk merges by node)"""
    out = []
    for j, v in o["m"]:
        keep = j < n_nodes
        order = np.argsort(j[keep], kind="stable")
        out.append((j[keep][order], v[keep][order]))
    return out


def stacked_csr(rows, n_nodes):
    """scipy CSR (float64 values, like compute_M's matrices) of a list of (columns, values) rows"""
    import scipy.sparse as sp

    indptr = np.concatenate([[0], np.cumsum([len(j) for j, _ in rows])]).astype(np.int64)
    ind = np.concatenate([j for j, _ in rows]) if rows else np.zeros(0, dtype=np.int64)
    val = np.concatenate([v.astype(np.float64) for _, v in rows]) if rows else np.zeros(0)
    return sp.csr_matrix((val, ind.astype(np.int64), indptr), shape=(len(rows), n_nodes))


def reference_vjp(Ms, w_rows, dt):
    """M^T w as the tape defines it: per node the entries in ascending row order, fl(v * w[row]) added one by one from +0 in dt"""
    g = np.zeros(Ms.shape[1], dt)
    rows = np.repeat(np.arange(Ms.shape[0]), np.diff(Ms.indptr))
    np.add.at(g, Ms.indices, Ms.data.astype(dt) * np.asarray(w_rows, dt)[rows])
    return g
