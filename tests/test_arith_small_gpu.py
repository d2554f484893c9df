"""Tolerance-grade arithmetic (option "arith" = 1 / 2) on SMALL grids, node by node (-m gpu).

tests/test_arith_mode_gpu.py holds the mode to the contract (1e-5 s RMS) at the full size of the workloads; an RMS over 1e8 nodes cannot
see a wrong halo column, chunk seam, upwind branch or thin axis.  Here every grid has 30 - 70 nodes per 3-D axis (up to 150 in 2-D), every
fault of that kind moves a node by a fraction of s dx (0.05 - 1 s), and the bar is per node:

    max |T - ref64| <= 2 K_CPU max |ref32 - ref64|      and the same for the RMS over the nodes

ref32 / ref64: the CPU oracle in fp32 / fp64 on the same fp32-rounded node slowness, all three run to a fixed point (eps = EPS_FIXED).
K_CPU (tests/arith_reference.py) is the worst ratio of the numpy restatement of the mode over the same cases, measured on the CPU against
the reference alone (tests/test_arith_reference.py); the factor 2 is for the two 1-ulp hardware operations (v_rcp_f32, v_sqrt_f32), which
act on the increment t - a1 <= s dx.  So: the mode may be about as far from the fp64 solution as the reference's own fp32 run is -- a few
ulp of the largest traveltime -- at every node.  Every case prints its ratio; measured worst on an MI355X 1.29 (max) / 1.19 (rms), receivers
1.24 of max |ref32 - ref64| (every figure: DESIGN.md section 0 item 12).

What runs: the case list of tests/arith_cases.py (patch remainders, several chunks, thin axes, the smallest grid, cell grids, sources on a
node / in the far corner cell / of three points with origin times), batches (one slot, a slot solved twice, pairs), each of the 18 AR = 1
instantiations of ttcr_amd/csrc/fsm_fast.hip once (by name), the exact properties the code promises (dx != dz, fp64 and weno grids stay
bit-identical under arith = 1; results scale exactly with the units) and a seeded sweep over random small configurations.
"""
import numpy as np
import pytest

import arith_cases as ac
import arith_reference as ar

pytestmark = pytest.mark.gpu
TOL = 1e-5                 # seconds RMS against the fp32 reference, BASELINE.json north_star
K_GPU = 2.0 * ar.K_CPU     # per-node bar, see above


def _grid(c, n_threads=1, eps=ar.EPS_FIXED, maxit=ar.MAXIT_FIXED, weno=0, dtype=np.float32, rotated=0, steps=None):
    import ttcr_amd

    ax = ac.axes(c) if steps is None else [np.arange(m) * h for m, h in zip(c["n"], steps)]
    if c["dim"] == 3:
        return ttcr_amd.Grid3d(*ax, n_threads=n_threads, cell_slowness=int(c["cell"]), method="FSM", tt_from_rp=0, weno=weno, eps=eps,
                               maxit=maxit, dtype=dtype)
    return ttcr_amd.Grid2d(*ax, n_threads=n_threads, cell_slowness=int(c["cell"]), method="FSM", weno=weno, eps=eps, maxit=maxit,
                           rotated_template=rotated, dtype=dtype)


def _field(g, slot=0):
    return g._flat_tt(slot)


def _check_bar(capsys, what, T, r, kernel, niter=None):
    """the per-node bar and the contract for one field; prints the ratios"""
    ref_max, ref_rms = ac.errors(r["ref32"]["tt"], r["ref64"]["tt"])
    got_max, got_rms = ac.errors(T, r["ref64"]["tt"])
    d32_max, d32_rms = ac.errors(T, r["ref32"]["tt"])
    with capsys.disabled():
        print(f"\n[arith small] {what:34s} ref32-ref64 {ref_max:.1e} / {ref_rms:.1e}  T-ref64 {got_max:.1e} / {got_rms:.1e}  T-ref32 {d32_max:.1e} / "
              f"{d32_rms:.1e}  ratio {got_max / max(ref_max, 1e-300):.2f} / {got_rms / max(ref_rms, 1e-300):.2f} (bar {K_GPU:.1f})  niter {niter} / {r['ref32']['niter']}  [{kernel}]")
    worst = int(np.argmax(np.abs(T.astype(np.float64) - r["ref64"]["tt"])))
    assert got_max <= K_GPU * ref_max, (what, "node", worst, got_max, ref_max)
    assert got_rms <= K_GPU * ref_rms, (what, got_rms, ref_rms)
    assert d32_rms <= TOL, (what, d32_rms)
    return ref_max


def _check_rcv(capsys, what, tt, r, ref_max):
    """receiver traveltimes within the per-node bar of the fp32 oracle's: kernel and oracle interpolate their fields with the same convex
    weights, so a receiver differs by no more than the nodes around it do"""
    ref = r["ref32"]["tt_rcv"]
    d = float(np.max(np.abs(tt.astype(np.float64) - ref.astype(np.float64))))
    with capsys.disabled():
        print(f"[arith small] {what:34s} receivers: max |tt - tt32| {d:.1e}, {d / max(ref_max, 1e-300):.2f} of max |ref32 - ref64| (bar {K_GPU:.1f})")
    assert d <= K_GPU * ref_max, (what, d, ref_max)


@pytest.mark.parametrize("c", ac.CASES, ids=[c["name"] for c in ac.CASES])
def test_small_grid_per_node(oracle, capsys, c):
    r = ac.references(oracle, c, ar.EPS_FIXED, ar.MAXIT_FIXED)
    g = _grid(c)
    s = ac.slowness(c)
    src, rcv = ac.source_array(c), r["rcv"]
    g.set_option("arith", 1)
    tt = g.raytrace(src, rcv, slowness=s, aggregate_src=True)
    assert g.last_kernel().endswith(",1>"), g.last_kernel()
    assert g.get_niter(0) < ar.MAXIT_FIXED
    ref_max = _check_bar(capsys, c["name"], _field(g), r, g.last_kernel(), g.get_niter(0))
    _check_rcv(capsys, c["name"], tt, r, ref_max)
    # the same grid in the default mode: the fp32 oracle bit for bit (the mode leaves nothing behind)
    g.set_option("arith", 0)
    tt0 = g.raytrace(src, rcv, aggregate_src=True)
    assert not g.last_kernel().endswith(",1>")
    np.testing.assert_array_equal(_field(g), r["ref32"]["tt"])
    assert g.get_niter(0) == r["ref32"]["niter"]
    np.testing.assert_array_equal(tt0, r["ref32"]["tt_rcv"])
    # the stopping rule as callers use it (eps = 1e-5): iteration counts are the fp32 oracle's on smooth models, reported on rough ones
    d = ac.references(oracle, c, 1e-5, 50)
    g5 = _grid(c, eps=1e-5, maxit=50)
    g5.set_option("arith", 1)
    g5.raytrace(src, rcv, slowness=s, aggregate_src=True)
    with capsys.disabled():
        print(f"[arith small] {c['name']:34s} eps 1e-5: niter {g5.get_niter(0)} / oracle {d['ref32']['niter']}")
    if c["smooth"]:
        assert g5.get_niter(0) == d["ref32"]["niter"]


@pytest.mark.parametrize("n_threads,n_src,pair", [(1, 1, None), (4, 5, None), (6, 6, "1")], ids=["1-slot", "4-slots-5-sources", "6-slots-pairs"])
def test_batches_per_node(oracle, capsys, monkeypatch, n_threads, n_src, pair):
    """n_threads 4 with five sources: the sources are block-distributed, slot 0 is solved twice (sources 0 and 1) and ends holding source 1"""
    if pair is not None:
        monkeypatch.setenv("TTCR_FSM_PAIR", pair)
    cs = ac.batch_cases(n_src)
    refs = [ac.references(oracle, c, ar.EPS_FIXED, ar.MAXIT_FIXED) for c in cs]
    rcv = refs[0]["rcv"]
    g = _grid(cs[0], n_threads=n_threads)
    g.set_option("arith", 1)
    src_rows = np.repeat(np.vstack([c["src"] for c in cs]), rcv.shape[0], axis=0)
    tt = g.raytrace(src_rows, np.tile(rcv, (n_src, 1)), slowness=ac.slowness(cs[0])).reshape(n_src, -1)
    k = g.last_kernel()
    assert k.endswith(",1>") and ((",2,true," in k) == (pair is not None)), k
    # slot -> the source whose field it holds at the end: block distribution (get_blk_size, ttcr/Grid3D.h:451-465) -- slot b takes
    # blk[b] = ceil((n_src - b) / n_blk) consecutive sources, one per round, and keeps the last
    n_blk = min(n_threads, n_src)
    blk = [(n_src - b + n_blk - 1) // n_blk for b in range(n_blk)]
    held = {b: sum(blk[:b + 1]) - 1 for b in range(n_blk)}
    ref_max = {}
    for slot, i in held.items():
        ref_max[i] = _check_bar(capsys, f"{cs[i]['name']} ({n_threads} slots)", _field(g, slot), refs[i], k, g.get_niter(slot))
    for i in range(n_src):
        rm = ref_max.get(i, ac.errors(refs[i]["ref32"]["tt"], refs[i]["ref64"]["tt"])[0])
        _check_rcv(capsys, cs[i]["name"], tt[i], refs[i], rm)
    g.set_option("arith", 0)
    tt0 = g.raytrace(src_rows, np.tile(rcv, (n_src, 1))).reshape(n_src, -1)
    for slot, i in held.items():
        np.testing.assert_array_equal(_field(g, slot), refs[i]["ref32"]["tt"])
        assert g.get_niter(slot) == refs[i]["ref32"]["niter"]
    for i in range(n_src):
        np.testing.assert_array_equal(tt0[i], refs[i]["ref32"]["tt_rcv"])


# ---- every AR = 1 instantiation of fsm_fast.hip once ---------------------------------------------------------------------------------------
# (stage, dim, fields per workgroup, chunk, skip, PRE) -> how the host is brought to launch it (fsm_sweep_plan.h, fsm_sweep_plan):
#   first order 3-D, one field: any grid with one slot group layout NS = 1; chunks of 16 whatever the batch, PRE compiled out (NO_PRE)
#   first order 3-D, pairs:     TTCR_FSM_PAIR = 1 and n_threads >= 2; chunks of 8; PRE = batch >= TTCR_FSM_PRE_MIN (2 slot groups here)
#   2-D:                        chunks of 16, PRE always on
#   WENO 3-D (arith = 2):       one field per workgroup; chunks of 16 while batch < TTCR_FSM_WENO_C16_BELOW, else 8; PRE = batch >= PRE_MIN
# UNREACHABLE by the host's rules, and absent from fsm_fast.hip accordingly: first-order 3-D one field with PRE (NO_PRE), pairs in the WENO
# stage (the stage keeps the exact kernels there: SweepPlan::AR), 2-D without PRE (pre = DIM == 2 || ...).
def _inst(stage, dim, ns, chunk, skip, pre):
    env, n_threads = {}, 1
    if dim == 3 and stage == 1 and ns == 2:
        env, n_threads = {"TTCR_FSM_PAIR": "1", "TTCR_FSM_PRE_MIN": "2" if pre else "100"}, 4
    if dim == 3 and stage == 2:
        env = {"TTCR_FSM_WENO_C16_BELOW": "3" if chunk == 16 else "0", "TTCR_FSM_PRE_MIN": "1" if pre else "100"}
    b = lambda v: "true" if v else "false"
    name = f"fsm_sweep_persistent<float,{'16,16' if dim == 3 else '64,1'},{chunk},{b(dim == 3)},{b(skip)},{stage},{ns},true,{b(pre)},1>"
    tag = f"{'first' if stage == 1 else 'weno'}-{dim}d-ns{ns}-c{chunk}-skip{int(skip)}-pre{int(pre)}"
    return pytest.param(stage, dim, skip, env, n_threads, name, id=tag)


INSTANTIATIONS = (
    [_inst(1, 3, 1, 16, sk, False) for sk in (0, 1)]
    + [_inst(1, 3, 2, 8, sk, pre) for sk in (0, 1) for pre in (0, 1)]
    + [_inst(1, 2, 1, 16, sk, True) for sk in (0, 1)]
    + [_inst(2, 3, 1, 16, sk, pre) for sk in (0, 1) for pre in (0, 1)]
    + [_inst(2, 3, 1, 8, sk, pre) for sk in (0, 1) for pre in (0, 1)]
    + [_inst(2, 2, 1, 16, sk, True) for sk in (0, 1)]
)
assert len(INSTANTIATIONS) == 18   # every launch_one<...> of fsm_fast.hip: 2 + 4 + 2 first-order, 4 + 4 + 2 WENO


@pytest.mark.parametrize("stage,dim,skip,env,n_threads,name", INSTANTIATIONS)
def test_every_instantiation_once(oracle, capsys, monkeypatch, stage, dim, skip, env, n_threads, name):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if stage == 1:
        # first-order kernels: the per-node bar on the random model (pairs: four sources, two slot groups)
        cs = ac.batch_cases(n_threads) if dim == 3 else [ac.BY_NAME["rand2d-150x70"]]
        refs = [ac.references(oracle, c, ar.EPS_FIXED, ar.MAXIT_FIXED) for c in cs]
        rcv = refs[0]["rcv"]
        g = _grid(cs[0], n_threads=n_threads)
        g.set_option("arith", 1)
        g.set_option("skip", skip)
        src_rows = np.repeat(np.vstack([c["src"] for c in cs]), rcv.shape[0], axis=0)
        g.raytrace(src_rows, np.tile(rcv, (len(cs), 1)), slowness=ac.slowness(cs[0]))
        assert g.last_kernel() == name
        for i, (c, r) in enumerate(zip(cs, refs)):
            _check_bar(capsys, c["name"], _field(g, i), r, g.last_kernel(), g.get_niter(i))
        return
    # WENO kernels (arith = 2): the stage amplifies an ulp of its input to 1e-3 s (profiles/r06/weno_sensitivity.txt) -- the smooth model
    # only, against the default mode on the same grid, with the bars of tests/test_arith_mode_gpu.py
    c = ac.BY_NAME["grad-33x31x35" if dim == 3 else "grad2d-150x70"]
    g = _grid(c, weno=1, eps=1e-5, maxit=50)
    g.set_option("skip", skip)
    src, rcv = ac.source_array(c), ac.receivers(c)
    g.raytrace(src, rcv, slowness=ac.slowness(c), aggregate_src=True)
    assert not g.last_kernel().endswith(",1>")
    ref, it = _field(g).copy(), (g.get_niter(0), g.get_niterw(0))
    g.set_option("arith", 2)
    g.raytrace(src, rcv, aggregate_src=True)
    assert g.last_kernel() == name
    worst, rms = ac.errors(_field(g), ref)
    with capsys.disabled():
        print(f"\n[arith = 2] {c['name']}: rms {rms:.3e} s, max {worst:.3e} s vs the default mode; niter {g.get_niter(0)} + {g.get_niterw(0)} / "
              f"{it[0]} + {it[1]}  [{g.last_kernel()}]")
    assert rms <= 2e-4 and worst <= 2e-2
    assert g.get_niter(0) == it[0] and abs(g.get_niterw(0) - it[1]) <= 2


# ---- exact properties ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", [False, True], ids=["nodes", "cells"])
def test_2d_rectangular_cells_keep_the_reference_arithmetic(oracle, cell):
    """dx != dz under arith = 1: update2_xz, the reference's arithmetic (fsm_march_levels.inc) -- bit-identical"""
    c = dict(ac.BY_NAME["rand2d-150x70"], cell=cell)
    dx, dz = 0.25, 0.4
    s = ac.slowness(c)
    src = np.array([[0.0, 11.3, 16.7], [0.02, 11.5, 16.9]])
    rcv = np.array([[0.0, 0.0], [149 * dx, 69 * dz], [3.3, 9.1], [10.0, 8.0], [149 * dx, 2.2]])
    g = _grid(c, eps=1e-5, maxit=50, steps=(dx, dz))
    g.set_option("arith", 1)
    tt = g.raytrace(src, rcv, slowness=s, aggregate_src=True)
    o = oracle.solve2d(np.float32, (149, 69), g.dx, g.dz, (0.0, 0.0), s.ravel(), src[:, 1:], src[:, 0], cell_slowness=cell, rcv=rcv)
    assert g.last_kernel().endswith(",1>")   # the AR = 1 kernel runs, with the reference's local solver
    np.testing.assert_array_equal(_field(g), o["tt"])
    assert g.get_niter(0) == o["niter"]
    np.testing.assert_array_equal(tt, o["tt_rcv"])


@pytest.mark.parametrize("name", ["rand-33x31x35", "rand2d-150x70"])
@pytest.mark.parametrize("kind", ["fp64", "weno"])
def test_fp64_and_weno_grids_stay_bit_identical_under_arith_1(oracle, name, kind):
    c = ac.BY_NAME[name]
    dt, weno = (np.float64, 0) if kind == "fp64" else (np.float32, 1)
    s = ac.slowness(c)
    rcv = ac.receivers(c)
    g = _grid(c, eps=1e-5, maxit=50, weno=weno, dtype=dt)
    g.set_option("arith", 1)
    tt = g.raytrace(ac.source_array(c), rcv, slowness=s, aggregate_src=True)
    assert ",1>" not in g.last_kernel(), g.last_kernel()
    nc = tuple(m - 1 for m in c["n"])
    if c["dim"] == 3:
        o = oracle.solve3d(dt, nc, g.dx, (0, 0, 0), ac.flat(c, s), c["src"], c["t0"], rcv=rcv, weno=bool(weno))
    else:
        o = oracle.solve2d(dt, nc, g.dx, g.dz, (0, 0), ac.flat(c, s), c["src"], c["t0"], rcv=rcv, weno=bool(weno))
    np.testing.assert_array_equal(_field(g), o["tt"])
    assert (g.get_niter(0), g.get_niterw(0)) == (o["niter"], o["niterw"])
    np.testing.assert_array_equal(tt, o["tt_rcv"])


def test_rotated_template_per_node(oracle, capsys):
    """rotated_template = 1 on square cells: sweep45 keeps the reference's arithmetic, the axis sweeps do not -- the per-node bar against
    the oracle with the rotated template, not equality"""
    c = ac.BY_NAME["rand2d-150x70"]
    r = ac.references(oracle, c, ar.EPS_FIXED, ar.MAXIT_FIXED, rotated=True)
    g = _grid(c, rotated=1)
    g.set_option("arith", 1)
    tt = g.raytrace(ac.source_array(c), r["rcv"], slowness=ac.slowness(c), aggregate_src=True)
    assert g.last_kernel().endswith(",1>")
    ref_max = _check_bar(capsys, c["name"] + " rotated", _field(g), r, g.last_kernel(), g.get_niter(0))
    _check_rcv(capsys, c["name"], tt, r, ref_max)


@pytest.mark.parametrize("name,arith", [("rand-33x31x35", 1), ("rand2d-150x70", 1), ("rand-33x31x35", 0)],
                         ids=["3d-arith1", "2d-arith1", "3d-default"])
def test_results_scale_exactly_with_the_units(oracle, name, arith):
    """slowness and eps times 2^k: every operation of update3_fast / update2_fast (and of the reference's chain) scales exactly by a power of
    two, and so does the source initialisation s d -- the field times 2^k bit for bit, with the same iteration count.  3-D: also k = -70
    and + 60, where fh^2 underflows / comes within 2^8 of overflowing fp32 (update3_fast never forms it).  2-D stays inside +- 40:
    update2_fast forms fh^2 in fp32.
    The reference's chain (arith = 0) squares a1 - a2 in fp32 (ttcr/Grid3Drn.h:2943): from s dx 2^-60 down that square is subnormal and the
    compiled reference itself stops scaling (this model: 591 nodes off at k = -60, 35 777 of 35 805 at k = -70, one iteration fewer).  At
    k = -70 the default mode is therefore held to what it promises, the oracle's field at k = -70 bit for bit, not to 2^-70 times its own
    field at k = 0."""
    c = ac.BY_NAME[name]
    s = ac.slowness(c)
    src, rcv = ac.source_array(c), ac.receivers(c)
    out = {}
    ks = (-10, 10, -40, 40) + ((-70, 60) if c["dim"] == 3 else ())
    for k in (0,) + ks:
        g = _grid(c, eps=ar.EPS_FIXED * 2.0 ** k)
        g.set_option("arith", arith)
        sk = (s * np.float32(2.0 ** k)).astype(np.float32)
        tt = g.raytrace(src, rcv, slowness=sk, aggregate_src=True)
        assert g.last_kernel().endswith(",1>") == (arith == 1)
        out[k] = (_field(g).copy(), g.get_niter(0), tt)
        if arith == 0 and k == -70:
            assert not np.any(c["t0"])
            o = oracle.solve3d(np.float32, tuple(m - 1 for m in c["n"]), g.dx, (0, 0, 0), ac.flat(c, sk), c["src"], c["t0"], rcv=rcv,
                               eps=ar.EPS_FIXED * 2.0 ** k, maxit=ar.MAXIT_FIXED)
            np.testing.assert_array_equal(out[k][0], o["tt"], err_msg=f"{name} k = {k} against the oracle")
            assert out[k][1] == o["niter"]
            np.testing.assert_array_equal(tt, o["tt_rcv"])
            assert np.any(o["tt"] != out[0][0] * np.float32(2.0 ** k))   # (the reference does not scale here)
    for k in ks:
        if arith == 0 and k == -70:
            continue
        np.testing.assert_array_equal(out[k][0], out[0][0] * np.float32(2.0 ** k), err_msg=f"{name} k = {k}")
        assert out[k][1] == out[0][1]
        np.testing.assert_array_equal(out[k][2], out[0][2] * np.float32(2.0 ** k), err_msg=f"{name} k = {k} (receivers)")


# ---- a seeded sweep over random small configurations ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", ac.SWEEP_SEEDS)
def test_seeded_sweep_per_node(oracle, capsys, monkeypatch, seed):
    rng = np.random.default_rng(seed)
    done = 0
    for n_cfg in range(ac.N_CONFIGS):
        q = ac.draw_configuration(rng)
        events = ac.sweep_events(q, seed, n_cfg)
        try:
            refs = [ac.references(oracle, ev, ar.EPS_FIXED, ar.MAXIT_FIXED) for ev in events]
        except RuntimeError as e:
            assert "Point outside grid" in str(e), e   # the only rejection that drops a draw
            continue
        if q["pair"]:
            monkeypatch.setenv("TTCR_FSM_PAIR", "1")
        else:
            monkeypatch.delenv("TTCR_FSM_PAIR", raising=False)
        g = _grid(events[0], n_threads=q["n_threads"])
        g.set_option("arith", 1)
        g.set_option("skip", q["skip"])
        rcv = refs[0]["rcv"]
        s = ac.slowness(events[0])
        if q["n_ev"] == 1:
            tt = g.raytrace(ac.source_array(events[0]), rcv, slowness=s, aggregate_src=True).reshape(1, -1)
        else:
            rows = np.repeat(np.vstack([ac.source_array(ev) for ev in events]), rcv.shape[0], axis=0)
            tt = g.raytrace(rows, np.tile(rcv, (q["n_ev"], 1)), slowness=s).reshape(q["n_ev"], -1)
        assert g.last_kernel().endswith(",1>")
        tag = f"seed {seed} #{n_cfg} {'x'.join(map(str, q['n']))}{' cells' if q['cell'] else ''} dx {q['dx']} slots {q['n_threads']} ev {q['n_ev']} pts {q['npt']} skip {q['skip']} pair {int(q['pair'])}"
        for e, r in enumerate(refs):
            ref_max = _check_bar(capsys, tag + f" ev{e}", _field(g, e), r, g.last_kernel(), g.get_niter(e))
            _check_rcv(capsys, tag, tt[e], r, ref_max)
        done += 1
    assert done >= ac.N_CONFIGS - ac.N_CONFIGS // 4, done   # at most a quarter dropped, and only because the oracle rejects the input
