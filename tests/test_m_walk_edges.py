"""The tables of tests/m_walk_cases.py test what they claim, proved with the oracle alone (no device): every kept receiver's walk ends, no
case loses more than a quarter of its candidates, the rows without records are where the table says and have tt = 0 exactly, the far-face
case has entries one past the grid, the many-point source has merged rows, the order of the vjp chain is observable on the dense
receivers, and the median of the retrace case splits its walks.  tests/test_m_walk_edges_gpu.py compares the device with the same oracle
results on the same inputs, bit for bit; the figures printed here (walks walked again per walk_records value, rows of the seams) say which
paths those runs take."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import m_walk_cases as MC  # noqa: E402

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])


def _reference(oracle, name, dt, rays=False):
    build, weno = MC.CASES[name]
    return MC.reference(oracle, name, build(), dt, weno, rays=rays)


@DTYPES
@pytest.mark.parametrize("name", list(MC.CASES))
def test_kept_walks_end_and_few_are_dropped(oracle, name, dt):
    case, res, candidates = _reference(oracle, name, dt)
    kept = [ev["rcv"].shape[0] for ev in case.events]
    print("%s, %s: receivers kept per event %s of %s" % (name, np.dtype(dt).name, kept, candidates))
    assert 4 * sum(kept) >= 3 * sum(candidates) and all(k >= 1 for k in kept), (kept, candidates)
    for ev, o in zip(case.events, res):   # (the oracle raises for a walk that does not end: these did, one row each)
        assert len(o["m"]["m"]) == ev["rcv"].shape[0] == o["m"]["tt_rcv"].size and np.all(np.isfinite(o["m"]["tt_rcv"]))


@DTYPES
@pytest.mark.parametrize("name", MC.EMPTY_CASES)
def test_empty_rows_are_where_the_table_says(oracle, name, dt):
    case, res, candidates = _reference(oracle, "empty-" + name, dt)
    _, empty = MC.empty_case(name)
    assert [ev["rcv"].shape[0] for ev in case.events] == candidates   # (nothing dropped: the row numbers of the table hold)
    for ev, o, rows in zip(case.events, res, empty):
        lens = np.array([len(j) for j, _ in o["m"]["m"]])
        assert sorted(np.nonzero(lens == 0)[0]) == sorted(rows), (lens, rows)
        tt = o["m"]["tt_rcv"][rows]
        assert np.all(tt == 0) and not np.any(np.signbit(tt))
    if name == "first_middle_last":
        e = empty[0]
        assert e[0] == 0 and e[-1] == case.events[0]["rcv"].shape[0] - 1 and e[1:4] == [e[1], e[1] + 1, e[1] + 2] and 0 < e[1] < e[-1] - 3
    if name == "empty_event_between":
        assert len(case.events) == 3 and len(empty[1]) == case.events[1]["rcv"].shape[0] and 0 in empty[0] and 0 in empty[2]
    if name == "nothing_but_empty":
        assert len(case.events) == 1 and sum(len(j) for j, _ in res[0]["m"]["m"]) == 0


@DTYPES
def test_far_faces_have_entries_past_the_grid(oracle, dt):
    case, res, _ = _reference(oracle, "far_faces", dt)
    n_nodes = int(np.prod(case.nn))
    past = [int(sum(np.sum(j >= n_nodes) for j, _ in o["m"]["m"])) for o in res]
    print("far_faces, %s: entries with a node index past the grid, per event: %s" % (np.dtype(dt).name, past))
    assert sum(past) >= 1
    hi = np.array(MC.HI) * case.dx
    kept = np.vstack([ev["rcv"] for ev in case.events])
    for a in range(3):   # receivers on every far plane survive, and the far corner
        assert np.any(kept[:, a] == hi[a]), a
    assert np.any(np.all(kept == hi, axis=1))
    assert case.events[1]["pts"][0, 0] == hi[0]   # (the source on a node of the x-max face)


@DTYPES
def test_many_points_rows_are_merged(oracle, dt):
    case, res, _ = _reference(oracle, "points_in_one_cell", dt, rays=True)
    ev = case.events[0]
    assert ev["pts"].shape[0] == MC.N_POINTS and ev["rcv"].shape[0] == 20
    cell = np.floor(ev["pts"] / case.dx)
    assert np.all(cell == cell[0]) and np.unique(MC.event_t0(ev)).size == MC.N_POINTS
    nz = np.array([np.count_nonzero(v) for _, v in res[0]["m"]["m"]])
    # the points a ray's end game served: those that appear among its last points
    pts = ev["pts"].astype(dt)
    served = np.array([sum(any(np.array_equal(q, p) for q in ray) for p in pts) for ray in res[0]["rm"]["rays"]])
    print("points_in_one_cell, %s: non-zero entries per row %s, source points served per ray %s" % (np.dtype(dt).name, nz.tolist(), served.tolist()))
    assert np.any(nz < 8 * MC.N_POINTS)
    assert np.any(served >= 2) and np.any(nz < 8 * served)   # (several points per ray, and their terms met at shared nodes)


@DTYPES
@pytest.mark.parametrize("name", MC.SHARED_CASES)
def test_vjp_order_is_observable_on_the_dense_receivers(oracle, name, dt):
    case, res, _ = _reference(oracle, "shared-" + name, dt)
    n_nodes = int(np.prod(case.nn))
    rows = [r for o in res for r in MC.oracle_rows(o["m"], n_nodes)]
    Ms = MC.stacked_csr(rows, n_nodes)
    w = MC.wide_weights(np.random.default_rng(71), Ms.shape[0], dt)
    g = MC.reference_vjp(Ms, w, dt)
    back = MC.stacked_csr(rows[::-1], n_nodes)
    g_back = MC.reference_vjp(back, w[::-1], dt)
    differ = int(np.sum(g.view(np.uint8).reshape(n_nodes, -1) != g_back.view(np.uint8).reshape(n_nodes, -1)) > 0)
    per_node = np.bincount(Ms.indices, minlength=n_nodes)
    print("shared-%s, %s: %d rows, %d entries, longest node chain %d, rows reversed: other bits at %d nodes"
          % (name, np.dtype(dt).name, Ms.shape[0], Ms.nnz, per_node.max(), int(np.sum(g != g_back))))
    assert differ and np.sum(g != g_back) >= 1
    assert per_node.max() >= 50   # (the 50 copies of one point: a long chain at each of their nodes)


@DTYPES
def test_seam_case_medians_split_the_walks(oracle, dt):
    case, res, candidates = MC.reference(oracle, "seams", MC.seam_case(), dt, rays=True)
    assert tuple(ev["rcv"].shape[0] for ev in case.events) == MC.SEAM_COUNTS == tuple(candidates)
    rays = [r for o in res for r in o["rm"]["rays"]]
    for o in res:   # (the overloads with r_data walk the same path: one length per receiver)
        assert [len(r) for r in o["rm"]["rays"]] == [len(r) for r in o["r"]["rays"]]
    n = len(rays)
    med = MC.median_records(rays)
    rec = np.array([MC.records(r) for r in rays])
    print("seams, %s: records per walk %s, median %d" % (np.dtype(dt).name, rec.tolist(), med))
    assert 4 * np.sum(rec > med) >= n and 4 * np.sum(rec < med) >= n
    for wr in (1, 4, med, MC.WALK_STEP_LIMIT):
        m, r = MC.m_retraced(rays, wr), MC.rays_retraced(rays, wr)
        print("  walk_records %7d: M walks walked again %2d of %d (rows %s), rays %2d" % (wr, len(m), n, m, len(r)))
    for wr in (1, 4):   # (nearly every walk; one that ends within the additive part of a row fits even then)
        assert 4 * len(MC.m_retraced(rays, wr)) >= 3 * n and 4 * len(MC.rays_retraced(rays, wr)) >= 3 * n
    assert 4 * len(MC.m_retraced(rays, med)) >= n and 4 * (n - len(MC.m_retraced(rays, med))) >= n
    assert MC.m_retraced(rays, MC.WALK_STEP_LIMIT) == []
    sm = MC.seams(MC.SEAM_COUNTS, MC.M_CHUNK[np.dtype(dt)])
    print("  walk_records %d: launches of the M walks end inside an event at rows %s (and at the event bounds %s)"
          % (MC.WALK_STEP_LIMIT, sm, np.cumsum(MC.SEAM_COUNTS)[:-1].tolist()))
    assert len(sm) >= 1


@DTYPES
def test_l_case_receivers_and_the_corner_ray(oracle, dt):
    """compute_L's table: enough receivers for a seam, rays longer than a row of walk_records = 4.  The receiver 1.7e-4 inside the far corner
    is a candidate, but the oracle's l_data walk leaves the grid from there (both dtypes); its r_data walk ends in fp64, after more than
    200 default rows of points -- the long ray the rays recorder meets without any option."""
    sc, cand = MC.l_case(dt)
    nc = (MC.L_NN[0] - 1, MC.L_NN[1] - 1)

    def solve(rcv, **kw):
        return oracle.solve2d(dt, nc, MC.L_DX, MC.L_DZ, (0, 0), sc.ravel(), MC.L_SRC, rcv=rcv, cell_slowness=True, **kw)

    keep = MC.finished(lambda r: (solve(r, compute_L=True, return_rays=True), solve(r, compute_L=True)), cand)
    o = solve(cand[keep], compute_L=True, return_rays=True)
    lens = [len(r) for r in o["rays"]]
    print("compute_L on the %s grid, %s: %d of %d receivers kept, points per ray %s" % (MC.L_NN, np.dtype(dt).name, len(keep), len(cand), lens))
    assert 4 * len(keep) >= 3 * len(cand) and len(keep) > MC.L_CHUNK[np.dtype(dt)] and max(lens) > 4 + 4
    assert MC.L_CORNER not in keep
    if dt == np.float64:
        n = len(solve(cand[MC.L_CORNER:MC.L_CORNER + 1], return_rays=True)["rays"][0])
        print("  the r_data walk from the corner receiver: %d points" % n)
        assert n > 200 * (8 * (nc[0] + nc[1] + 3) + 3)
