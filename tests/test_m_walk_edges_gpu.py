"""The recording ray walks and the M tape's merge on the device at the inputs of tests/m_walk_cases.py, against the oracle, bit for bit
(signed zeros are entries): rows without records and a tape without entries, walks that touch the last planes (node indices one past the
grid), sources of many points in one cell, receivers that share nodes, thin grids, moved origins, the WENO stage -- and, through option
"walk_records", walks longer than their row (walked again alone) and calls whose receivers take several launches, for compute_M with and
without the rays, return_rays alone, the M tape (one device and two replicas) and compute_L.  No result may depend on the option.
tests/test_m_walk_edges.py proves on the CPU that the tables hold these edges and prints which walks are walked again and where the
seams fall."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import m_walk_cases as MC  # noqa: E402
from test_l_matrix import _same_up_to_ties  # noqa: E402
from test_m_tape_gpu import _bits_equal, _same_csr  # noqa: E402  (the project's comparisons, not restated)

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
LAYOUTS = [(1, 0), (4, 0), (4, [0, 0])]   # (n_threads, device): one slot, four slots, four slots on two replicas of one device


def _grid(case, dt, weno=0, n_threads=2, device=0, walk_records=0):
    import ttcr_amd

    axes = [case.origin[a] + np.arange(case.nn[a]) * case.dx for a in range(3)]
    g = ttcr_amd.Grid3d(*axes, n_threads=n_threads, cell_slowness=0, method="FSM", tt_from_rp=0, weno=weno, dtype=dt, device=device)
    g.set_slowness(case.s.reshape(case.nn, order="F"))
    g.set_option("walk_records", walk_records)
    return g


def _expected(case, res, key, call, dt):
    """the oracle's results of one overload in the order of the call: tt per rcv row, per event the (columns, values) rows of M in call
    order (None for the overload without m_data), the ray of every rcv row (None without r_data)"""
    src, rcv, agg, rows, pick = call
    n_nodes = int(np.prod(case.nn))
    tt = np.zeros(rcv.shape[0], dtype=dt)
    ev_rows, rays = [], [None] * rcv.shape[0]
    for e, o in enumerate(res):
        tt[rows[e]] = o[key]["tt_rcv"][pick[e]]
        if "m" in o[key]:
            r = MC.oracle_rows(o[key], n_nodes)
            ev_rows.append([r[i] for i in pick[e]])
        if "rays" in o[key]:
            for row, i in zip(rows[e], pick[e]):
                rays[row] = o[key]["rays"][i].astype(np.float64)
    return tt, (ev_rows or None), (rays if "rays" in res[0][key] else None)


def _check_m(out, case, exp):
    """raytrace(..., compute_M=True[, return_rays=True]) against the oracle: tt, rays, every event's matrix entry for entry"""
    tt_ref, ev_rows, rays_ref = exp
    n_nodes = int(np.prod(case.nn))
    tt, M = out[0], out[-1]
    _bits_equal(tt, tt_ref)
    assert len(M) == len(ev_rows)
    for m, r in zip(M, ev_rows):
        assert m.shape == (len(r), n_nodes)
        _same_csr(m, MC.stacked_csr(r, n_nodes))
    if rays_ref is not None:
        _check_rays(out[1], rays_ref)


def _check_rays(rays, rays_ref):
    assert len(rays) == len(rays_ref)
    for a, b in zip(rays, rays_ref):
        _bits_equal(np.asarray(a, dtype=np.float64), b)


def _check_tape(tt, tape, case, exp, call, dt):
    """raytrace_tape against the oracle: tt, the CSR, the sizes, M^T w; returns (CSR, gradient)"""
    src, rcv, agg, rows, pick = call
    tt_ref, ev_rows, _ = exp
    n_nodes = int(np.prod(case.nn))
    _bits_equal(tt, tt_ref)
    Ms = MC.stacked_csr([r for ev in ev_rows for r in ev], n_nodes)
    A = tape.to_csr()
    _same_csr(A, Ms)
    el = np.dtype(dt).itemsize
    assert tape.nnz == Ms.nnz and tape.shape == A.shape == Ms.shape == (rcv.shape[0], n_nodes) and tape.n_data == rcv.shape[0]
    assert tape.nbytes == 8 * (tape.n_rows + 1 + n_nodes + 1) + 2 * tape.nnz * (4 + el) + (tape.n_rows + n_nodes) * el   # (include/ttcr_amd.h)
    w = MC.wide_weights(np.random.default_rng(73), rcv.shape[0], dt)
    grad = tape.vjp(w)
    _bits_equal(grad, MC.reference_vjp(Ms, w[np.concatenate(rows)], dt))   # (no entries: +0 everywhere)
    return A, grad


def _check_case(g, case, res, call, dt):
    src, rcv, agg, rows, pick = call
    exp = _expected(case, res, "m", call, dt)
    _check_m(g.raytrace(src, rcv, compute_M=True, aggregate_src=agg), case, exp)
    tt, tape = g.raytrace_tape(src, rcv, aggregate_src=agg)
    return _check_tape(tt, tape, case, exp, call, dt)


@DTYPES
@pytest.mark.parametrize("name", list(MC.CASES))
def test_compute_m_and_tape_match_the_oracle(oracle, name, dt):
    build, weno = MC.CASES[name]
    case, res, _ = MC.reference(oracle, name, build(), dt, weno)
    A, grad = _check_case(_grid(case, dt, weno), case, res, MC.call_arrays(case), dt)
    if name == "empty-nothing_but_empty":
        assert A.nnz == 0 and not np.any(grad) and not np.any(np.signbit(grad))
    else:
        assert A.nnz > 0 and np.any(grad != 0)


@DTYPES
@pytest.mark.parametrize("name", MC.SHARED_CASES)
def test_shared_nodes_whatever_the_slots_and_replicas(oracle, name, dt):
    case, res, _ = MC.reference(oracle, "shared-" + name, MC.shared_case(name), dt)
    call = MC.call_arrays(case)
    outs = []
    for n_threads, device in LAYOUTS:
        g = _grid(case, dt, n_threads=n_threads, device=device)
        assert g.n_devices == (2 if isinstance(device, list) else 1)
        outs.append(_check_case(g, case, res, call, dt))
    for A, grad in outs[1:]:   # (each equals the oracle; and so one another)
        _same_csr(A, outs[0][0])
        _bits_equal(grad, outs[0][1])


# ---- f. seams and retraces
def _seam_reference(oracle, dt):
    case, res, _ = MC.reference(oracle, "seams", MC.seam_case(), dt, rays=True)
    assert tuple(ev["rcv"].shape[0] for ev in case.events) == MC.SEAM_COUNTS
    return case, res, [r for o in res for r in o["rm"]["rays"]]


def _run_all(g, case, res, call, dt):
    """every recording call on one grid, each against the oracle; what they returned"""
    src, rcv, agg, rows, pick = call
    out = {}
    out["m"] = g.raytrace(src, rcv, compute_M=True)
    _check_m(out["m"], case, _expected(case, res, "m", call, dt))
    out["rm"] = g.raytrace(src, rcv, compute_M=True, return_rays=True)
    _check_m(out["rm"], case, _expected(case, res, "rm", call, dt))
    out["r"] = g.raytrace(src, rcv, return_rays=True)
    tt_ref, _, rays_ref = _expected(case, res, "r", call, dt)
    _bits_equal(out["r"][0], tt_ref)
    _check_rays(out["r"][1], rays_ref)
    tt, tape = g.raytrace_tape(src, rcv)
    out["tape"] = (tt,) + _check_tape(tt, tape, case, _expected(case, res, "m", call, dt), call, dt)
    return out


def _same_outputs(a, b):
    for key in ("m", "rm"):
        _bits_equal(a[key][0], b[key][0])
        for x, y in zip(a[key][-1], b[key][-1]):
            _same_csr(x, y)
    for key in ("rm", "r"):
        _check_rays(a[key][1], [np.asarray(r, dtype=np.float64) for r in b[key][1]])
    _bits_equal(a["r"][0], b["r"][0])
    _bits_equal(a["tape"][0], b["tape"][0])
    _same_csr(a["tape"][1], b["tape"][1])
    _bits_equal(a["tape"][2], b["tape"][2])


_DEFAULT_RUN = {}


def _default_run(oracle, dt):
    """the outputs at walk_records = 0 (two slots, one device), once per dtype"""
    key = np.dtype(dt).name
    if key not in _DEFAULT_RUN:
        case, res, _ = _seam_reference(oracle, dt)
        _DEFAULT_RUN[key] = _run_all(_grid(case, dt), case, res, MC.call_arrays(case), dt)
    return _DEFAULT_RUN[key]


@DTYPES
@pytest.mark.parametrize("walk_records", [MC.WALK_STEP_LIMIT, 1, 4, "median"])
def test_seams_and_retraces_change_nothing(oracle, walk_records, dt):
    """walk_records = 1 000 000: 13 (fp32) / 6 (fp64) receivers per launch of the M walks, seams inside and between the events of 5, 17
    and 9 receivers; 1, 4 and the median record count: nearly all, nearly all and about four in ten of the 31 walks are walked again
    (tests/test_m_walk_edges.py prints which).  Every output is the oracle's and that of the default."""
    case, res, rays = _seam_reference(oracle, dt)
    wr = MC.median_records(rays) if walk_records == "median" else walk_records
    call = MC.call_arrays(case)
    default = _default_run(oracle, dt)
    for n_threads, device in LAYOUTS:
        g = _grid(case, dt, n_threads=n_threads, device=device, walk_records=wr)
        _same_outputs(_run_all(g, case, res, call, dt), default)


def test_rays_seam_inside_an_event(oracle):
    """400 receivers, fp32, walk_records = 1 000 000: 357 rays per launch, the second launch starts inside the second event of the batch"""
    dt = np.float32
    case, res, _ = MC.reference(oracle, "rays_seam", MC.rays_seam_case(), dt, rays=True)
    counts = [ev["rcv"].shape[0] for ev in case.events]
    assert sum(counts) == 400 and counts[0] < MC.RAYS_CHUNK[np.dtype(dt)] < sum(counts)
    call = MC.call_arrays(case)
    src, rcv = call[0], call[1]
    tt_ref, _, rays_ref = _expected(case, res, "r", call, dt)
    outs = []
    for wr in (MC.WALK_STEP_LIMIT, 0):
        g = _grid(case, dt, n_threads=2, walk_records=wr)
        tt, rays = g.raytrace(src, rcv, return_rays=True)
        _bits_equal(tt, tt_ref)
        _check_rays(rays, rays_ref)
        outs.append((tt, rays))
        del g
    _bits_equal(outs[0][0], outs[1][0])


def _grid2d(sc, dt, walk_records, **kw):
    import ttcr_amd

    x, z = np.arange(MC.L_NN[0]) * MC.L_DX, np.arange(MC.L_NN[1]) * MC.L_DZ
    g = ttcr_amd.Grid2d(x, z, n_threads=1, cell_slowness=1, method="FSM", weno=0, dtype=dt, **kw)
    g.set_slowness(sc)
    g.set_option("walk_records", walk_records)
    return g


@DTYPES
def test_compute_l_seams_and_retraces(oracle, dt):
    """compute_L on the 2-D cell grid of tests/test_parity_gpu.py, receivers next to its last planes: walk_records = 4 sends every chunk
    round again with the room its longest ray asked for, 1 000 000 leaves 16 (fp32) / 8 (fp64) receivers per launch.  The receiver
    1.7e-4 inside the far corner is a candidate; the oracle's l_data walk leaves the grid from there, so it is not among the kept."""
    sc, cand = MC.l_case(dt)
    nc = (MC.L_NN[0] - 1, MC.L_NN[1] - 1)

    def solve(rcv, rays):
        return oracle.solve2d(dt, nc, MC.L_DX, MC.L_DZ, (0, 0), sc.ravel(), MC.L_SRC, rcv=rcv, cell_slowness=True, compute_L=True, return_rays=rays)

    rcv = cand[MC.finished(lambda r: (solve(r, True), solve(r, False)), cand)]
    n = rcv.shape[0]
    assert 4 * n >= 3 * cand.shape[0] and n > MC.L_CHUNK[np.dtype(dt)]   # (more than one launch at walk_records = 1 000 000)
    o0, o1 = solve(rcv, False), solve(rcv, True)
    assert max(len(r) for r in o1["rays"]) > 4 + 4   # (rays longer than a row of walk_records = 4)
    srows = np.repeat(MC.L_SRC, n, axis=0)
    first = None
    for wr in (0, 4, MC.WALK_STEP_LIMIT):
        g = _grid2d(sc, dt, wr)
        tt, Lm = g.raytrace(srows, rcv, compute_L=True)
        tt2, rays, L2 = g.raytrace(srows, rcv, compute_L=True, return_rays=True)
        _bits_equal(tt, o0["tt_rcv"])
        _bits_equal(tt2, o1["tt_rcv"])
        assert Lm.shape == L2.shape == (n, nc[0] * nc[1])
        for q in range(n):
            for mat, o in ((Lm, o0), (L2, o1)):
                row = mat.getrow(q)
                _same_up_to_ties(row.indices.astype(np.int64), row.data.astype(dt), o["l"][q][0].astype(np.int64), o["l"][q][1])
        _check_rays(rays, [r.astype(np.float64) for r in o1["rays"]])
        if first is None:
            first = (Lm, L2)
        else:   # (and the default's, entry for entry in its order)
            _same_csr(Lm.tocsr(), first[0].tocsr())
            _same_csr(L2.tocsr(), first[1].tocsr())


def test_long_2d_ray_is_walked_again_without_the_option(oracle):
    """fp64, return_rays on the same 2-D grid: the ray from 1.7e-4 inside the far corner has 41 512 points, more than 200 times the default
    row -- the second walk of the rays recorder with no option set; with walk_records = 1 000 000 it fits its row.  The same rays."""
    dt = np.float64
    sc, cand = MC.l_case(dt)
    nc = (MC.L_NN[0] - 1, MC.L_NN[1] - 1)
    rcv = np.vstack([cand[-3:-1], cand[MC.L_CORNER], cand[-1:]])
    o = oracle.solve2d(dt, nc, MC.L_DX, MC.L_DZ, (0, 0), sc.ravel(), MC.L_SRC, rcv=rcv, cell_slowness=True, return_rays=True)
    lens = [len(r) for r in o["rays"]]
    assert lens[2] > 200 * (8 * (nc[0] + nc[1] + 3) + 3) and max(lens[:2] + lens[3:]) < 100, lens
    for wr in (0, MC.WALK_STEP_LIMIT):
        g = _grid2d(sc, dt, wr, tt_from_rp=1)
        tt, rays = g.raytrace(np.repeat(MC.L_SRC, rcv.shape[0], axis=0), rcv, return_rays=True)
        _bits_equal(tt, o["tt_rcv"])
        _check_rays(rays, [r.astype(np.float64) for r in o["rays"]])


def test_walk_records_values_and_reset(oracle):
    import ttcr_amd

    dt = np.float32
    case, res, _ = _seam_reference(oracle, dt)
    call = MC.call_arrays(case)
    src, rcv = call[0], call[1]
    x = np.arange(5) * 1.0
    grids = [_grid(case, dt), _grid(case, dt, n_threads=4, device=[0, 0]),
             ttcr_amd.Grid2d(x, x, cell_slowness=1, method="FSM", weno=0, dtype=np.float64)]
    for g in grids:
        for bad in (-1, 1.5, MC.WALK_STEP_LIMIT + 1, float("nan")):
            with pytest.raises(ValueError):
                g.set_option("walk_records", bad)
        for good in (1, MC.WALK_STEP_LIMIT, 0):
            g.set_option("walk_records", good)
    # set and set back: the default's outputs again (a refused value has changed nothing either)
    g = grids[0]
    runs = []
    for wr in (0, 4, 0):
        g.set_option("walk_records", wr)
        with pytest.raises(ValueError):
            g.set_option("walk_records", -1)
        tt, tape = g.raytrace_tape(src, rcv)
        runs.append((tt, tape.to_csr(), g.raytrace(src, rcv, return_rays=True)))
    for tt, A, (tt_r, rays) in runs[1:]:
        _bits_equal(tt, runs[0][0])
        _same_csr(A, runs[0][1])
        _bits_equal(tt_r, runs[0][2][0])
        _check_rays(rays, [np.asarray(r, dtype=np.float64) for r in runs[0][2][1]])
