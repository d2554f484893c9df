"""Tolerance-grade arithmetic (option "arith" = 1, update3_fast / update2_fast in ttcr_amd/csrc/fsm_kernels.h) against the CPU oracle (-m gpu).

north_star's contract for the traveltimes is "within 1e-5 s RMS of the reference CPU Grid3Drnfs output".  The default mode (arith = 0) is
bit-identical to the oracle at the full size of every BASELINE.json configuration (tests/test_baseline_configs_gpu.py); this file holds the
opt-in mode to the contract, at the same sizes:

  C2  Grid3d 256^3 nodes gradient, 1 source, fp32                          vs the oracle
  C3  Grid3d 512^3 nodes gradient: one source                              vs the oracle
      ... and the 64 sources of the headline batch                         vs the default mode on the same grid (= the oracle, see above),
                                                                           four of the 64 fields vs the oracle as well
  C4  Grid3d 256^3 cells layers model (cell -> node path), 8 sources       vs the oracle
  C5  Grid2d 4096^2 nodes gradient, 16 sources                             vs the oracle
  +   the rough 512^3 model (16^3-node blocks), one source, to convergence vs the default mode (= the oracle)

RMS over ALL nodes of a field, in float64; the tolerance is TOL = 1e-5 s as the contract states it.  Iteration counts are reported next to the
oracle's and must agree on these models (the stopping rule sees changes of ~1e-7 relative).  The mode must also leave the default path alone:
switching it off again gives the bit-identical default fields.

An RMS over 1e8 nodes cannot see a local fault (a halo column, a chunk seam, a thin axis), and these sizes launch only half of the AR = 1
kernels: tests/test_arith_small_gpu.py holds the mode to a PER-NODE bar on grids of 30 - 70 nodes per axis (patch remainders, thin grids,
cell grids, batches, dx != dz, units), launches every instantiation of fsm_fast.hip once and runs a seeded sweep; the bar is calibrated on
the CPU by tests/test_arith_reference.py (tests/arith_reference.py restates a whole tolerance-mode solve in numpy).
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
TOL = 1e-5   # seconds RMS, BASELINE.json north_star


def _rms(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float(np.sqrt(np.mean(d * d))), float(np.max(np.abs(d)))


def _gradient_nodes_f32(n):
    dx = 20.0 / (n - 1)
    sz = (1.0 / (1.0 + 0.1 * (np.arange(n, dtype=np.float64) * dx))).astype(np.float32)
    return dx, sz


def _report(capsys, what, rms, worst, it_tol, it_ref, kernel):
    with capsys.disabled():
        print(f"\n[arith = 1] {what}: rms {rms:.3e} s, max {worst:.3e} s (tolerance {TOL:g} s rms); niter {it_tol} / oracle {it_ref}  [{kernel}]")


def test_c2_gradient_256(oracle, capsys):
    import ttcr_amd

    n = 256
    dx, sz = _gradient_nodes_f32(n)
    x = np.arange(n) * dx
    src = cases.mt_sources(1)
    rcv = cases.rcv_lattice3d()
    g = ttcr_amd.Grid3d(x, x, x, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, dtype=np.float32)
    g.set_slowness(np.ascontiguousarray(np.broadcast_to(sz[None, None, :], (n, n, n))))
    g.set_option("arith", 1)
    tt = g.raytrace(src, rcv)
    assert g.last_kernel().endswith(",1>")   # the tolerance-grade instantiation ran
    o = oracle.solve3d(np.float32, (n - 1,) * 3, dx, (0, 0, 0), np.repeat(sz, n * n), src, rcv=rcv)
    rms, worst = _rms(g._flat_tt(0), o["tt"])
    _report(capsys, "C2 256^3 gradient, 1 source", rms, worst, g.get_niter(0), o["niter"], g.last_kernel())
    assert rms <= TOL and g.get_niter(0) == o["niter"]
    assert _rms(tt, o["tt_rcv"])[0] <= TOL
    # back to the default: bit-identical to the oracle again (the mode leaves nothing behind)
    g.set_option("arith", 0)
    g.raytrace(src, rcv)
    assert np.array_equal(g._flat_tt(0), o["tt"])


def test_c3_gradient_512_single_and_64_sources(oracle, capsys):
    import ttcr_amd

    n, S = 512, 64
    dx, sz = _gradient_nodes_f32(n)
    x = np.arange(n, dtype=np.float64) * dx
    srcs = cases.mt_sources(S)
    rcv1 = cases.rcv_lattice3d()
    flat = np.repeat(sz, n * n)
    # one source
    g1 = ttcr_amd.Grid3d(x, x, x, n_threads=1, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, dtype=np.float32)
    g1.set_slowness(flat.reshape((n, n, n), order="F"))
    g1.set_option("arith", 1)
    g1.raytrace(srcs[:1], rcv1[:1])
    f_single = g1._flat_tt(0).copy()
    k_single, it_single = g1.last_kernel(), g1.get_niter(0)
    del g1
    # the batch, both modes on one grid
    g = ttcr_amd.Grid3d(x, x, x, n_threads=S, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, dtype=np.float32)
    g.set_slowness(flat.reshape((n, n, n), order="F"))
    src_rows, rcv_rows = np.repeat(srcs, rcv1.shape[0], axis=0), np.tile(rcv1, (S, 1))
    g.set_option("arith", 1)
    tt_tol = g.raytrace(src_rows, rcv_rows)
    k_batch = g.last_kernel()
    assert k_batch.endswith(",1>")
    it_tol = [g.get_niter(i) for i in range(S)]
    # the oracle for source 0 and three more (thread pool), compared while the fields are still the tolerance mode's
    pick = [0, 21, 42, 63]
    with ThreadPoolExecutor(max_workers=4) as ex:
        orc = list(ex.map(lambda i: oracle.solve3d(np.float32, (n - 1,) * 3, dx, (0, 0, 0), flat, srcs[i:i + 1], rcv=rcv1), pick))
    for i, o in zip(pick, orc):
        rms, worst = _rms(g._flat_tt(i), o["tt"])
        _report(capsys, f"C3 512^3 x 64, source {i} vs the oracle", rms, worst, it_tol[i], o["niter"], k_batch)
        assert rms <= TOL and it_tol[i] == o["niter"]
    rms, worst = _rms(f_single, orc[0]["tt"])
    _report(capsys, "C3 512^3, ONE source vs the oracle", rms, worst, it_single, orc[0]["niter"], k_single)
    assert rms <= TOL and it_single == orc[0]["niter"]
    # all 64 against the default mode (bit-identical to the oracle: test_baseline_configs_gpu.py).  64 fields of 512 MiB do not fit the
    # host twice: four whole fields and a strided sample (every 4099th node) of every field are kept across the default-mode solve
    keep = {i: g._flat_tt(i).copy() for i in (7, 28, 35, 56)}
    sample = [g._flat_tt(i)[::4099].copy() for i in range(S)]
    g.set_option("arith", 0)
    tt_def = g.raytrace(src_rows, rcv_rows)
    it_def = [g.get_niter(i) for i in range(S)]
    assert it_tol == it_def, (it_tol, it_def)
    worst_rms = 0.0
    for i in range(S):
        f = g._flat_tt(i)
        worst_rms = max(worst_rms, _rms(sample[i], f[::4099])[0])
        if i in keep:
            rms, _ = _rms(keep[i], f)
            assert rms <= TOL, (i, rms)
            worst_rms = max(worst_rms, rms)
    _report(capsys, "C3 512^3 x 64 vs the default mode: four whole fields + a strided sample of all 64 (worst)", worst_rms, float("nan"), it_tol[0], it_def[0], k_batch)
    assert worst_rms <= TOL
    assert _rms(tt_tol, tt_def)[0] <= TOL


def test_c4_layers_256_cells_8_sources(oracle, capsys):
    import ttcr_amd

    nc, S = 256, 8
    dx = 20.0 / nc
    x = np.arange(nc + 1, dtype=np.float64) * dx
    sc_z = (1.0 / (cases.A + cases.B * (np.floor(np.arange(nc) * dx) + 0.5)))
    srcs = cases.mt_sources(S)
    rcv1 = cases.rcv_lattice3d()
    g = ttcr_amd.Grid3d(x, x, x, n_threads=S, cell_slowness=1, method="FSM", tt_from_rp=0, weno=0, dtype=np.float32)
    g.set_option("arith", 1)
    g.raytrace(np.repeat(srcs, rcv1.shape[0], axis=0), np.tile(rcv1, (S, 1)),
               slowness=np.ascontiguousarray(np.broadcast_to(sc_z[None, None, :], (nc, nc, nc))))
    assert g.last_kernel().endswith(",1>")
    flat = np.repeat(sc_z, nc * nc)
    with ThreadPoolExecutor(max_workers=min(8, (os.cpu_count() or 2))) as ex:
        orc = list(ex.map(lambda i: oracle.solve3d(np.float32, (nc,) * 3, dx, (0, 0, 0), flat, srcs[i:i + 1], rcv=rcv1, cell_slowness=True), range(S)))
    worst_rms = 0.0
    for i, o in enumerate(orc):
        rms, worst = _rms(g._flat_tt(i), o["tt"])
        worst_rms = max(worst_rms, rms)
        assert rms <= TOL and g.get_niter(i) == o["niter"], (i, rms, g.get_niter(i), o["niter"])
    _report(capsys, "C4 256^3 cells x 8 (worst source)", worst_rms, float("nan"), g.get_niter(0), orc[0]["niter"], g.last_kernel())


def test_c5_gradient2d_4096_16_sources(oracle, capsys):
    import ttcr_amd

    n, S = 4096, 16
    dx, sz = _gradient_nodes_f32(n)
    x = np.arange(n, dtype=np.float64) * dx
    srcs = cases.mt_sources(S, ndim=2)
    rcv1 = np.array([[0.0, 0.0], [20.0, 20.0], [3.21, 7.77]])
    g = ttcr_amd.Grid2d(x, x, n_threads=S, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, dtype=np.float32)
    g.set_option("arith", 1)
    g.raytrace(np.repeat(srcs, rcv1.shape[0], axis=0), np.tile(rcv1, (S, 1)), slowness=np.ascontiguousarray(np.broadcast_to(sz[None, :], (n, n))))
    assert g.last_kernel().endswith(",1>")
    flat = np.tile(sz, n)
    with ThreadPoolExecutor(max_workers=min(8, (os.cpu_count() or 2))) as ex:
        orc = list(ex.map(lambda i: oracle.solve2d(np.float32, (n - 1, n - 1), dx, dx, (0, 0), flat, srcs[i:i + 1], rcv=rcv1), range(S)))
    worst_rms = 0.0
    for i, o in enumerate(orc):
        rms, worst = _rms(g._flat_tt(i), o["tt"])
        worst_rms = max(worst_rms, rms)
        assert rms <= TOL and g.get_niter(i) == o["niter"], (i, rms, g.get_niter(i), o["niter"])
    _report(capsys, "C5 4096^2 x 16 (worst source)", worst_rms, float("nan"), g.get_niter(0), orc[0]["niter"], g.last_kernel())


def test_rough_512_model_to_convergence(capsys):
    """the model on which the stopping rule decides (tests/test_baseline_configs_gpu.py pins the default mode to the oracle on it)"""
    import ttcr_amd

    n = 512
    dx = 20.0 / (n - 1)
    x = np.arange(n) * dx
    rng = np.random.default_rng(5)
    c = rng.uniform(0.4, 1.0, (n // 16 + 2,) * 3)
    s = np.repeat(np.repeat(np.repeat(c, 16, 0), 16, 1), 16, 2)[:n, :n, :n].astype(np.float32).copy()
    src = cases.mt_sources(1)
    rcv = cases.rcv_lattice3d()
    g = ttcr_amd.Grid3d(x, x, x, n_threads=1, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, dtype=np.float32)
    g.set_slowness(s)
    g.set_option("arith", 1)
    tt1 = g.raytrace(np.repeat(src, rcv.shape[0], axis=0), rcv)
    f1, it1, k1 = g._flat_tt(0).copy(), g.get_niter(0), g.last_kernel()
    g.set_option("arith", 0)
    tt0 = g.raytrace(np.repeat(src, rcv.shape[0], axis=0), rcv)
    rms, worst = _rms(f1, g._flat_tt(0))
    _report(capsys, "rough 512^3 model, 1 source, to convergence (vs the default mode = the oracle)", rms, worst, it1, g.get_niter(0), k1)
    assert rms <= TOL and it1 == g.get_niter(0) and it1 >= 4
    assert _rms(tt1, tt0)[0] <= TOL


def test_weno_grids_keep_the_reference_arithmetic_under_arith_1_and_arith_2_is_the_opt_in(capsys):
    """The WENO stage (weno = True, the ttcrpy default) amplifies differences of an ulp in its input to 1e-3 s: under arith = 1 a grid with the
    WENO stage stays bit-identical in both stages; arith = 2 switches both stages to the tolerance-grade arithmetic, outside the 1e-5 s bound
    (profiles/r06/weno_sensitivity.txt).  The default mode is the oracle bit for bit here as everywhere (tests/test_parity_gpu.py,
    tests/test_fullsize_gpu.py), so it serves as the reference."""
    import ttcr_amd

    n, n_src = 128, 3
    dx, sz = _gradient_nodes_f32(n)
    x = np.arange(n) * dx
    srcs = cases.mt_sources(64)[:n_src]
    rcv = np.zeros((n_src, 3))
    g = ttcr_amd.Grid3d(x, x, x, n_threads=n_src, cell_slowness=0, method="FSM", tt_from_rp=0, weno=1, dtype=np.float32)
    g.set_slowness(np.ascontiguousarray(np.broadcast_to(sz[None, None, :], (n, n, n))))
    g.raytrace(srcs, rcv)
    ref = [g._flat_tt(i).copy() for i in range(n_src)]
    it = [(g.get_niter(i), g.get_niterw(i)) for i in range(n_src)]
    g.set_option("arith", 1)
    g.raytrace(srcs, rcv)
    assert not g.last_kernel().endswith(",1>")
    assert all(np.array_equal(g._flat_tt(i), ref[i]) for i in range(n_src)) and it == [(g.get_niter(i), g.get_niterw(i)) for i in range(n_src)]
    g.set_option("arith", 2)
    g.raytrace(srcs, rcv)
    assert g.last_kernel().endswith(",1>")
    for i in range(n_src):
        rms, worst = _rms(g._flat_tt(i), ref[i])
        with capsys.disabled():
            print(f"\n[arith = 2] WENO 128^3, source {i}: rms {rms:.3e} s, max {worst:.3e} s vs the default mode; niter {g.get_niter(i)} + {g.get_niterw(i)} / {it[i][0]} + {it[i][1]}")
        assert rms <= 2e-4 and worst <= 2e-2
        assert g.get_niter(i) == it[i][0] and abs(g.get_niterw(i) - it[i][1]) <= 2
    # 2-D with the WENO stage
    n2 = 1024
    dx2, sz2 = _gradient_nodes_f32(n2)
    x2 = np.arange(n2, dtype=np.float64) * dx2
    src2 = cases.mt_sources(1, ndim=2)
    g2 = ttcr_amd.Grid2d(x2, x2, n_threads=1, cell_slowness=0, method="FSM", tt_from_rp=0, weno=1, dtype=np.float32)
    g2.set_slowness(np.ascontiguousarray(np.broadcast_to(sz2[None, :], (n2, n2))))
    g2.raytrace(src2, np.zeros((1, 2)))
    ref2 = g2._flat_tt(0).copy()
    g2.set_option("arith", 2)
    g2.raytrace(src2, np.zeros((1, 2)))
    rms, worst = _rms(g2._flat_tt(0), ref2)
    with capsys.disabled():
        print(f"\n[arith = 2] WENO 2-D 1024^2: rms {rms:.3e} s, max {worst:.3e} s vs the default mode  [{g2.last_kernel()}]")
    assert g2.last_kernel().endswith(",1>") and rms <= 2e-4


def test_mode_needs_whole_iteration_launches():
    import ttcr_amd

    x = np.arange(33) * 0.5
    g = ttcr_amd.Grid3d(x, x, x, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, dtype=np.float32)
    g.set_slowness(np.full((33, 33, 33), 0.5, dtype=np.float32))
    g.set_option("arith", 1)
    g.set_option("mode", 1)
    with pytest.raises(ValueError):
        g.raytrace(np.array([[1.0, 2.0, 3.0]]), np.array([[0.0, 0.0, 0.0]]))
    with pytest.raises(ValueError):
        g.set_option("arith", 3)
    # fp64 grids keep the reference's arithmetic whatever the option says
    g64 = ttcr_amd.Grid3d(x, x, x, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0)
    g64.set_slowness(np.full((33, 33, 33), 0.5))
    g64.raytrace(np.array([[1.0, 2.0, 3.0]]), np.array([[0.0, 0.0, 0.0]]))
    ref = g64._flat_tt(0).copy()
    g64.set_option("arith", 1)
    g64.raytrace(np.array([[1.0, 2.0, 3.0]]), np.array([[0.0, 0.0, 0.0]]))
    assert np.array_equal(ref, g64._flat_tt(0)) and not g64.last_kernel().endswith(",1>")
