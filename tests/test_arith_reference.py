"""The numpy restatement of a whole tolerance-mode solve (tests/arith_reference.py) against the fp32 and the fp64 oracle on the small grids of
tests/arith_cases.py, run to a fixed point.  No device: this calibrates the per-node bar of tests/test_arith_small_gpu.py against the
reference alone -- K_CPU is the worst ratio measured HERE, not anything a kernel produced (the table is in arith_reference's docstring)."""
import numpy as np
import pytest

import arith_cases as ac
import arith_reference as ar

TOL = 1e-5   # seconds RMS against the fp32 reference, BASELINE.json north_star


@pytest.mark.parametrize("c", ac.CASES, ids=[c["name"] for c in ac.CASES])
def test_restated_solve_is_as_close_to_fp64_as_the_fp32_reference(oracle, capsys, c):
    r = ac.references(oracle, c, ar.EPS_FIXED, ar.MAXIT_FIXED)
    assert r["ref32"]["niter"] < ar.MAXIT_FIXED and r["ref64"]["niter"] < ar.MAXIT_FIXED
    solve = ar.solve3d_fast if c["dim"] == 3 else ar.solve2d_fast
    fast, niter = solve(c["n"], ac.grid_dx(c), r["sn"], r["T0"], maxit=ar.MAXIT_FIXED, eps=ar.EPS_FIXED)
    assert niter < ar.MAXIT_FIXED
    # the smallest non-zero traveltime is far enough above eps * N for the run to have reached its fixed point
    assert ar.EPS_FIXED * fast.size < np.spacing(np.float32(np.min(fast[fast > 0])))
    ref_max, ref_rms = ac.errors(r["ref32"]["tt"], r["ref64"]["tt"])
    got_max, got_rms = ac.errors(fast, r["ref64"]["tt"])
    d32_max, d32_rms = ac.errors(fast, r["ref32"]["tt"])
    with capsys.disabled():
        print(f"\n[restated arith = 1] {c['name']:28s} ref32-ref64 {ref_max:.1e} / {ref_rms:.1e}  fast-ref64 {got_max:.1e} / {got_rms:.1e}  "
              f"fast-ref32 {d32_max:.1e} / {d32_rms:.1e}  ratio {got_max / ref_max:.2f} / {got_rms / ref_rms:.2f}  niter {niter} / {r['ref32']['niter']}")
    assert got_max <= ar.K_CPU * ref_max, (got_max, ref_max)          # (a) per node
    assert got_rms <= ar.K_CPU * ref_rms, (got_rms, ref_rms)
    assert d32_rms <= TOL, d32_rms                                    # (b) the contract


def test_level_order_is_the_lexicographic_sweep(oracle):
    """the restated driver with the REFERENCE's 2-D local solver (its float evaluation, as tests/test_arith_formulas.py writes it) reproduces
    the fp32 oracle bit for bit, field and iteration count: the sweep order, the frozen nodes, the border and the stopping rule of the
    restatement are the reference's, so what the calibration measures is the local solver alone"""
    def update2_ref(a, b, s, dx):
        fh = (s * dx).astype(np.float32)
        d = (a - b).astype(np.float32)
        d2 = (d * d).astype(np.float32)
        disc = 2.0 * fh.astype(np.float64) ** 2 - d2.astype(np.float64)
        t2 = (0.5 * ((a + b).astype(np.float32).astype(np.float64) + np.sqrt(np.maximum(disc, 0)))).astype(np.float32)
        return np.where(np.abs(d) >= fh, (np.minimum(a, b) + fh).astype(np.float32), t2)

    for name in ("rand2d-150x70", "rand2d-65x130", "thin2d-2x40", "cells2d-60x44"):
        c = ac.BY_NAME[name]
        nc = tuple(m - 1 for m in c["n"])
        s = ac.flat(c, ac.slowness(c))
        o = oracle.solve2d(np.float32, nc, ac.grid_dx(c), ac.grid_dx(c), (0.0, 0.0), s, c["src"], c["t0"], cell_slowness=c["cell"])
        init = oracle.solve2d(np.float32, nc, ac.grid_dx(c), ac.grid_dx(c), (0.0, 0.0), s, c["src"], c["t0"], cell_slowness=c["cell"], maxit=0)
        nnx, nnz = c["n"]
        flips = [(rj, ri) for ri, rj in zip((0, 1, 1, 0), (0, 0, 1, 1))]
        got, niter = ar._solve_fast((nnz, nnx), flips, ac.grid_dx(c), o["node_slowness"], init["tt"], 1e-5, 50, update2_ref)
        np.testing.assert_array_equal(got, o["tt"], err_msg=name)
        assert niter == o["niter"], name


def test_level_order_is_the_lexicographic_sweep_3d(oracle):
    """the same in 3-D: the restated driver (eight directions, border, frozen nodes, stopping rule) with the reference's local solver
    (ttcr/Grid3Drn.h:2936-2956: float sums and differences, the quadratics in double, one rounding) is the fp32 oracle bit for bit"""
    f32, f64 = np.float32, np.float64

    def update3_ref(ax, ay, az, s, dx):
        a = np.sort(np.stack([ax, ay, az]), axis=0)
        a1, a2, a3 = a[0], a[1], a[2]
        fh = (s * dx).astype(f32)
        d1, d2, d3, fh64 = a1.astype(f64), a2.astype(f64), a3.astype(f64), fh.astype(f64)
        t1 = (a1 + fh).astype(f32)
        d12 = (a1 - a2).astype(f32)
        t2 = (0.5 * ((a1 + a2).astype(f32).astype(f64) + np.sqrt(np.maximum(2.0 * fh64 * fh64 - (d12 * d12).astype(f32).astype(f64), 0)))).astype(f32)
        disc = -2.0 * d1 * d1 + 2.0 * d1 * d2 - 2.0 * d2 * d2 + 2.0 * d1 * d3 + 2.0 * d2 * d3 - 2.0 * d3 * d3 + 3.0 * fh64 * fh64
        t3 = (1.0 / 3.0 * (((a1 + a2).astype(f32) + a3).astype(f32).astype(f64) + np.sqrt(np.maximum(disc, 0)))).astype(f32)
        return np.where(t1 > a2, np.where(t2 > a3, t3, t2), t1)

    flips = [((d & 1), (d >> 1) & 1, (d >> 2) & 1) for d in range(8)]
    for name in ("rand-33x31x35", "rand-33x31x35-3pts", "rand-70x17x9", "thin-16x2x10", "cells-32x30x34"):
        c = ac.BY_NAME[name]
        nc = tuple(m - 1 for m in c["n"])
        s = ac.flat(c, ac.slowness(c))
        kw = dict(cell_slowness=c["cell"])
        o = oracle.solve3d(np.float32, nc, ac.grid_dx(c), (0.0, 0.0, 0.0), s, c["src"], c["t0"], **kw)
        init = oracle.solve3d(np.float32, nc, ac.grid_dx(c), (0.0, 0.0, 0.0), s, c["src"], c["t0"], maxit=0, **kw)
        got, niter = ar._solve_fast(c["n"], flips, ac.grid_dx(c), o["node_slowness"], init["tt"], 1e-5, 50, update3_ref)
        np.testing.assert_array_equal(got, o["tt"], err_msg=name)
        assert niter == o["niter"], name


@pytest.mark.parametrize("seed", ac.SWEEP_SEEDS)
def test_the_oracle_accepts_enough_of_the_seeded_sweep(oracle, seed):
    """tests/test_arith_small_gpu.py drops a drawn configuration only when the oracle rejects it (a point outside the grid): at most a
    quarter of each seed's draws, checked here with the oracle alone"""
    rng = np.random.default_rng(seed)
    kept = 0
    for n_cfg in range(ac.N_CONFIGS):
        q = ac.draw_configuration(rng)
        try:
            for ev in ac.sweep_events(q, seed, n_cfg):
                r = ac.references(oracle, ev, ar.EPS_FIXED, ar.MAXIT_FIXED)
                assert r["ref32"]["niter"] < ar.MAXIT_FIXED
        except RuntimeError as e:
            assert "Point outside grid" in str(e), e
            continue
        kept += 1
    assert kept >= ac.N_CONFIGS - ac.N_CONFIGS // 4, kept
