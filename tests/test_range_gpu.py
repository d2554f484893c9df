"""The sweep kernels across the float range (-m gpu): every case of tests/range_cases.py -- unit systems that are no powers of two,
slowness and dx times powers of two up to the fp32 underflow and overflow of the squares in update3, WENO second differences on both
sides of the 2^73 bound of weno_axes, blocks of 1e12 / 1e-12 / 0.0 / the smallest subnormal, models whose candidates overflow or whose
fields are subnormal -- in fp32 and fp64, first order and WENO, against the CPU oracle, which tests/test_range_cases.py holds to the
compiled reference on the same cases.

The bar is bit for bit: grid traveltimes, interpolated receiver traveltimes, get_niter, get_niterw, and the sums of
get_reference_changes wherever the device took a decision with one.  The get_changes history is held to the host's own bound
(change_sum_cases.bar, as in tests/test_change_sum_gpu.py) on one case and more per class: the exact decreases take one oracle solve
per iteration.

Launches: a lone source with whole-iteration launches (TTCR_FSM_MODE = 2) with TTCR_FSM_SKIP = 0 and 1 on every case; two sources in
the pair layout (TTCR_FSM_PAIR = 1) on every 3-D case, each slot against its own oracle solve; TTCR_FSM_MODE = 0 and 1 on one case and
more per class; the raypath calls on the smooth model in metres with a translated UTM origin."""
import numpy as np
import pytest

import change_sum_cases as cs
import range_cases as rc
from test_stopping_sums_gpu import _check_history

pytestmark = pytest.mark.gpu

ENV_KEYS = ("TTCR_FSM_WGS", "TTCR_FSM_PAIR", "TTCR_FSM_PAIR_UNITS", "TTCR_FSM_PRE_MIN", "TTCR_FSM_MODE", "TTCR_FSM_SKIP", "TTCR_FSM_ARITH",
            "TTCR_FSM_LONE_CHUNK", "TTCR_FSM_RS_FIELDS", "TTCR_FSM_SWEEP45", "TTCR_FSM_WENO_C16_BELOW", "TTCR_FSM_TIME_ORDER_BELOW")
ORDER = {False: "first", True: "weno"}
ROWS = rc.rows()
ROW_IDS = ["%s-%s-%s" % (c["name"], dt.name, ORDER[w]) for c, dt, w in ROWS]


def _env(monkeypatch, **env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("TTCR_FSM_" + k, str(v))


def _grid(c, dt, weno, n_threads=1, rotated=0, tt_from_rp=0):
    import ttcr_amd

    ax, d = rc.axes(c, dt)
    if c["dim"] == 3:
        g = ttcr_amd.Grid3d(*ax, n_threads=n_threads, cell_slowness=int(c["cell"]), method="FSM", tt_from_rp=tt_from_rp, weno=int(weno),
                            eps=c["eps"], maxit=c["maxit"], translate_grid=c["translate"], dtype=dt.type)
        assert g.dx == d[0]
    else:
        g = ttcr_amd.Grid2d(*ax, n_threads=n_threads, cell_slowness=int(c["cell"]), method="FSM", weno=int(weno), eps=c["eps"], maxit=c["maxit"],
                            rotated_template=rotated, tt_from_rp=tt_from_rp, dtype=dt.type)
        assert (g.dx, g.dz) == (d[0], d[1])
    g.set_slowness(rc.slowness_array(c))
    return g


def _check_slot(g, slot, c, dt, o, tag):
    """field, both iteration counts and the reference's sums of one slot against the oracle's solve o"""
    T = rc.flat(c, g.get_grid_traveltimes(slot))
    assert T.dtype == dt
    bad = np.flatnonzero(T != o["tt"])
    assert bad.size == 0, (tag, "nodes that differ", bad.size, "first", int(bad[0]), T[bad[0]], o["tt"][bad[0]], g.last_kernel())
    assert (g.get_niter(slot), g.get_niterw(slot)) == (o["niter"], o["niterw"]), (tag, g.get_niter(slot), g.get_niterw(slot), o["niter"], o["niterw"])
    thr = float(dt.type(c["eps"]) * dt.type(T.size))
    first, weno = g.get_reference_changes(slot)
    _check_history(first, o["change"], thr, tag + ("reference sums, first order",))
    _check_history(weno, o["changew"], thr, tag + ("reference sums, weno",))


def _lone(monkeypatch, c, dt, weno, rotated=0, **env):
    _env(monkeypatch, **env)
    g = _grid(c, dt, weno, rotated=rotated)
    tt = g.raytrace(rc.source_rows(c, dt), rc.receivers(c, dt), aggregate_src=True)
    o = rc.solve(oracle_module(), c, dt, weno, rotated=bool(rotated))
    tag = (c["name"], dt.name, ORDER[weno], "rotated" if rotated else "", tuple(sorted(env.items())))
    _check_slot(g, 0, c, dt, o, tag)
    assert tt.dtype == dt
    np.testing.assert_array_equal(tt, o["tt_rcv"], err_msg=str(tag))
    return g


def oracle_module():
    from oracle import oracle as O

    O.lib()
    return O


@pytest.mark.parametrize("c,dt,weno", ROWS, ids=ROW_IDS)
def test_lone_source_whole_iteration_launches(monkeypatch, c, dt, weno):
    for skip in (0, 1):
        g = _lone(monkeypatch, c, dt, weno, MODE=2, SKIP=skip)
        f = g.last_kernel().split(",")
        assert f[0] == "fsm_sweep_persistent<" + ("float" if dt == np.float32 else "double"), g.last_kernel()
        assert f[5] == ("true" if skip else "false"), g.last_kernel()
        if c["dim"] == 3 and not weno:
            assert f[3] == "16" and f[7] == "1", g.last_kernel()   # a lone source: chunks of 16 levels, one field per workgroup


ROT = [(c, dt) for c in rc.CASES if rc.rot_ok(c) for dt in rc.DTYPES]


@pytest.mark.parametrize("c,dt", ROT, ids=["%s-%s" % (c["name"], dt.name) for c, dt in ROT])
def test_rotated_template(monkeypatch, c, dt):
    _lone(monkeypatch, c, dt, False, rotated=1, MODE=2)


PAIRS = [(c, dt) for c in rc.CASES if c["dim"] == 3 for dt in rc.DTYPES]


@pytest.mark.parametrize("c,dt", PAIRS, ids=["%s-%s" % (c["name"], dt.name) for c, dt in PAIRS])
def test_two_sources_in_the_pair_layout(oracle, monkeypatch, c, dt):
    """first order: the WENO stage keeps one field per workgroup"""
    _env(monkeypatch, MODE=2, PAIR=1)
    kinds = ("off", "node")
    g = _grid(c, dt, False, n_threads=2)
    rcv = rc.receivers(c, dt)
    rows = np.vstack([np.repeat(rc.source_rows(c, dt, k), len(rcv), axis=0) for k in kinds])
    tt = g.raytrace(rows, np.tile(rcv, (2, 1))).reshape(2, -1)
    assert ",2," in g.last_kernel(), g.last_kernel()
    for slot, k in enumerate(kinds):
        o = rc.solve(oracle, c, dt, False, kind=k)
        tag = (c["name"], dt.name, "pair", "slot", slot, k)
        _check_slot(g, slot, c, dt, o, tag)
        np.testing.assert_array_equal(tt[slot], o["tt_rcv"], err_msg=str(tag))


# one case and more per class for the launch modes that are not the default and for the get_changes history
SOME = ["metric_utm-n3", "gpr_s_per_m-n2", "ultrasound-x2", "k-66-eps_scaled-n3", "k+37-eps_scaled-n3", "k+64-eps_scaled-n3", "k+55-eps_scaled-x2",
        "k-66-eps_scaled-c2", "dx-40-c3", "dx+40-n2", "block_zero-n3", "block_subnormal-n2", "k+122-n3", "k-140-eps0-n2"]
assert {rc.BY_NAME[n]["cls"] for n in SOME} == {"a", "b", "c", "d", "e"}
SOME_ROWS = rc.rows([rc.BY_NAME[n] for n in SOME])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c,dt,weno", SOME_ROWS, ids=["%s-%s-%s" % (c["name"], dt.name, ORDER[w]) for c, dt, w in SOME_ROWS])
def test_one_launch_per_tile_wavefront_and_per_sweep(monkeypatch, c, dt, weno, mode):
    g = _lone(monkeypatch, c, dt, weno, MODE=mode)
    if mode == 0:
        assert g.last_kernel().startswith("fsm_sweep_tile<") or weno, g.last_kernel()


CHANGE_ROWS = [(rc.BY_NAME[n], dt) for n in SOME for dt in rc.DTYPES]


@pytest.mark.parametrize("c,dt", CHANGE_ROWS, ids=["%s-%s" % (c["name"], dt.name) for c, dt in CHANGE_ROWS])
def test_change_history_within_the_hosts_bound(oracle, monkeypatch, capsys, c, dt):
    """|c_k / E_k - 1| <= change_sum_cases.bar for every first-order iteration k >= 2, c_k == 0.0 exactly where E_k == 0.  Iterations in
    which a node leaves max() are not compared, like iteration 1 (k = 122: one more): the kernels add such decreases up to inf."""
    E = rc.exact_decreases(oracle, c, dt)
    b = cs.bar(dt, c["nodes"])
    worst = 0.0
    assert sum(1 for e in E if not np.isnan(e)) >= 1
    for skip in (0, 1):
        g = _lone(monkeypatch, c, dt, False, MODE=2, SKIP=skip)
        ch = g.get_changes(0)[0]
        assert ch.size == len(E) - 1, (c["name"], ch, E)
        for k in range(2, len(E)):
            cv = float(ch[k - 1])
            if np.isnan(E[k]):
                assert cv > 0.0, (c["name"], dt.name, "skip", skip, "iteration", k, cv)
            elif E[k] == 0:
                assert cv == 0.0, (c["name"], dt.name, "skip", skip, "iteration", k, cv)
            else:
                r = abs(cv / E[k] - 1.0) / b
                worst = max(worst, r)
                assert r <= 1.0, (c["name"], dt.name, "skip", skip, "iteration", k, cv, E[k], r)
    with capsys.disabled():
        print("\n[range] %-28s %s worst |c / E - 1| / bar %.3e over %d iterations" % (c["name"], dt.name, worst, len(E) - 2), end="")


@pytest.mark.parametrize("dt", rc.DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("weno", [False, True], ids=["first", "weno"])
def test_raypath_calls_in_metres_with_a_translated_origin(oracle, monkeypatch, dt, weno):
    """traveltimes integrated along the ray (tt_from_rp = 1) and the rays themselves (return_rays) against the oracle's walk"""
    _env(monkeypatch, MODE=2)
    c = rc.BY_NAME[rc.WALK_CASE]
    src, rcv = rc.source_rows(c, dt), rc.receivers(c, dt)
    g = _grid(c, dt, weno, tt_from_rp=1)
    o = rc.solve(oracle, c, dt, weno, tt_from_rp=True)
    np.testing.assert_array_equal(g.raytrace(src, rcv, aggregate_src=True), o["tt_rcv"])
    _check_slot(g, 0, c, dt, o, (c["name"], dt.name, ORDER[weno], "tt_from_rp"))
    g = _grid(c, dt, weno)
    o = rc.solve(oracle, c, dt, weno, return_rays=True)
    tt, rays = g.raytrace(src, rcv, aggregate_src=True, return_rays=True)
    np.testing.assert_array_equal(tt, o["tt_rcv"])
    assert len(rays) == len(o["rays"]) == len(rcv)
    for a, b in zip(rays, o["rays"]):
        np.testing.assert_array_equal(np.asarray(a, dtype=dt), b)
