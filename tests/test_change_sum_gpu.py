"""The fp64 sum of decreases of every sweep kernel (`change`: a.change / d_change, read back as h_change, handed out by get_changes())
against the EXACT decrease of the iteration (-m gpu).

That sum decides when a solve stops (decide_go_on, ttcr_amd/csrc/fsm_capi.hip): outside the window around eps N by itself, inside it
wherever c (1 +- m)(1 +- g) lies on one side of eps N (option stopping_shortcuts, bit 2).  A kernel that loses the decrease of a node at a
patch remainder, of a pair's second source, of a unit taken on a second trip through the unit loop, of a chunk the skip scheduler stepped
over, keeps every field and nearly every iteration count -- and breaks the bound m the host relies on.  Here, for every launch and every
slot of the call:

    field and niter equal the oracle's (so the exact decreases E_k of tests/change_sum_cases.py belong to the run),
    |c_k / E_k - 1| <= bar for every iteration k >= 2 of the slot's solve, c_k == 0.0 exactly where E_k == 0,
    the history ends where the oracle's does (a source of a pair that converged is no longer summed),

bar = change_sum_cases.bar(): the host's own m (fp64: what the window 1 +- 1e-6 leaves), no other tolerance.  Iteration 1 is not compared
(its old values are max()).  Every test prints its worst |c / E - 1| / bar (the table of DESIGN.md section 5).

Out of scope: the WENO stage's `changew`.  A node may move up and down within an iteration there, so the sum of the changes of the single
updates is not the net change of the iteration, and bit 2 of stopping_shortcuts applies to stage 0 only.
"""
import numpy as np
import pytest

import change_sum_cases as cs
import few_workgroups_cases as fw
import test_few_workgroups_gpu as fwg

pytestmark = pytest.mark.gpu

ENV_KEYS = fwg.ENV_KEYS + ("TTCR_FSM_SWEEP45", "TTCR_FSM_RS_FIELDS")
MAIN = cs.BY_NAME["fw_37x35x41"]
assert MAIN["nodes"] == fw.SHAPES[0]


class Worst:
    """collects |c / E - 1| / bar of a test; report() prints the worst and then asserts every one"""

    def __init__(self):
        self.rows = []

    def add(self, ratio, what):
        self.rows.append((ratio, what))

    def report(self, capsys, title):
        assert self.rows, title
        w = max(self.rows, key=lambda r: r[0])
        with capsys.disabled():
            print("\n[change sum] %-58s worst |c / E - 1| / bar %.3e over %d sums  %s" % (title, w[0], len(self.rows), w[1]), end="")
        bad = [r for r in self.rows if not r[0] <= 1.0]
        assert not bad, (title, bad[:8])


def _clean_env(monkeypatch, env=None):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _check_slot(g, slot, c, dt, f, worst, tag):
    """slot holds the solve whose oracle fields are f (change_sum_cases.fields)"""
    K = f["niter"]
    np.testing.assert_array_equal(cs.flat(c, g.get_grid_traveltimes(slot)), f["tt"], err_msg=str(tag))
    assert g.get_niter(slot) == K, tag
    ch = g.get_changes(slot)[0]
    assert ch.size == K, (tag, ch)                       # (the history ends where the oracle's does)
    b = cs.bar(dt, c["nodes"])
    for k in range(2, K + 1):
        E, cv = f["E"][k], float(ch[k - 1])
        if E == 0:
            assert cv == 0.0, (tag, "iteration", k, cv)
        else:
            worst.add(abs(cv / E - 1.0) / b, "%s slot %d iteration %d: c %.17g E %.17g c - E %.3e" % (tag, slot, k, cv, E, cv - E))


def _rows(c, n):
    """raytrace arguments: source q with one receiver (the first node), q = 0 ... n - 1"""
    src = cs.sources(c)[:n]
    rcv = np.array([[a[0] for a in cs.axes(c, np.float64)]] * n, dtype=np.float64)
    return src, rcv


# ------------------------------------------------------------------------------------------------- the looped 3-D instantiations
def _run_inst(oracle, monkeypatch, capsys, inst, c, wgs, order=None, extra_opts=None):
    order = list(range(fw.N_SRC)) if order is None else order
    dt = np.dtype(inst.dtype)
    g = fwg._grid(monkeypatch, inst, c["nodes"], wgs, extra_opts=extra_opts)
    src, rcv = fw.sources(c["nodes"]), fw.receivers(c["nodes"])
    g.raytrace(np.repeat(src[order], len(rcv), axis=0), np.tile(rcv, (len(order), 1)))
    assert g.last_kernel() == inst.name, (g.last_kernel(), inst.name)
    slots, _ = fw.held(order, inst.n_threads)
    assert len(slots) == inst.n_threads
    worst = Worst()
    for slot, q in slots.items():
        _check_slot(g, slot, c, dt, cs.fields(oracle, c, dt, q), worst, "%s source %d" % (inst.id, q))
    worst.report(capsys, "%s %s WGS %s" % (c["name"], inst.id, "unset" if wgs is None else wgs))


@pytest.mark.parametrize("inst", fwg.INSTANTIATIONS, ids=[i.id for i in fwg.INSTANTIATIONS])
def test_every_looped_instantiation(oracle, monkeypatch, capsys, inst):
    """(37, 35, 41), four sources per call, the workgroup count the library picks"""
    _run_inst(oracle, monkeypatch, capsys, inst, MAIN, None)


@pytest.mark.parametrize("inst", fwg.REDUCED, ids=[i.id for i in fwg.REDUCED])
def test_one_workgroup_takes_every_unit(oracle, monkeypatch, capsys, inst):
    """TTCR_FSM_WGS=1: the sum is handed over once per unit, and a workgroup that loops must start each unit from zero"""
    _run_inst(oracle, monkeypatch, capsys, inst, MAIN, 1)


@pytest.mark.parametrize("wgs", [None, 1], ids=["wgs-unset", "wgs-1"])
@pytest.mark.parametrize("inst", fwg.REDUCED, ids=[i.id for i in fwg.REDUCED])
def test_pair_with_a_source_that_converges_first(oracle, monkeypatch, capsys, inst, wgs):
    """(70, 17, 9), pair_sources = 0, PAIR_ORDER_70: each pair holds a source that converges one iteration before its partner
    (tests/test_few_workgroups_cases.py).  The partner's later sums must not contain the finished source's nodes, and the finished source's
    history ends where the oracle's does.  (The instantiations with one field per workgroup run the same call.)"""
    c = cs.BY_NAME["fw_70x17x9"]
    _run_inst(oracle, monkeypatch, capsys, inst, c, wgs, order=fw.PAIR_ORDER_70, extra_opts={"pair_sources": 0})


# ------------------------------------------------------------------------------------------------- grids of the other tables
def _grid(c, dt, n_threads):
    import ttcr_amd

    dt = np.dtype(dt)
    ax = cs.axes(c, dt)
    if c["dim"] == 3:
        g = ttcr_amd.Grid3d(*ax, n_threads=n_threads, cell_slowness=int(c["cell"]), method="FSM", tt_from_rp=0, weno=0, eps=cs.EPS, maxit=c["maxit"],
                            dtype=dt.type)
    else:
        g = ttcr_amd.Grid2d(*ax, n_threads=n_threads, cell_slowness=int(c["cell"]), method="FSM", weno=0, eps=cs.EPS, maxit=c["maxit"],
                            rotated_template=int(c["rotated"]), dtype=dt.type)
    g.set_slowness(cs.slowness(c, dt))
    return g


def _run_case(oracle, capsys, c, dt, opts, title, n_src=None):
    """one call with the case's sources, one per slot; returns the kernel's name"""
    dt = np.dtype(dt)
    n = c["n_src"] if n_src is None else n_src
    g = _grid(c, dt, n)
    for k, v in opts.items():
        g.set_option(k, v)
    g.raytrace(*_rows(c, n))
    worst = Worst()
    for q in range(n):
        _check_slot(g, q, c, dt, cs.fields(oracle, c, dt, q), worst, "%s %s source %d" % (c["name"], dt.name, q))
    kern = g.last_kernel()
    worst.report(capsys, "%s %s %s [%s]" % (c["name"], dt.name, title, kern))
    return kern


DT = [np.dtype(np.float32), np.dtype(np.float64)]
DT_IDS = ["fp32", "fp64"]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("name", ["fw_37x35x41", "n2d_65x130"])
def test_one_launch_per_tile_wavefront_and_per_sweep(oracle, monkeypatch, capsys, name, dt, mode):
    """mode = 0: fsm_sweep_tile, a sum per tile of BL levels; mode = 1: the persistent kernel, one launch per sweep"""
    _clean_env(monkeypatch)
    c = cs.BY_NAME[name]
    kern = _run_case(oracle, capsys, c, dt, {"mode": mode}, "mode %d" % mode, n_src=2)
    if mode == 0:
        assert kern.startswith("fsm_sweep_tile<" + ("float" if dt == np.float32 else "double")), kern
    else:
        assert kern.startswith("fsm_sweep_persistent<") and kern.endswith(",false,false>"), kern


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("name", ["n2d_65x130", "n2d_130x65", "n2d_151x71"])
def test_2d_persistent_kernels(oracle, monkeypatch, capsys, name, dt, skip):
    """one-wave patches of 64 columns: dx != dz (update2_xz), patch remainders of 1 and 2 columns, two sources, with and without skipping"""
    _clean_env(monkeypatch)
    kern = _run_case(oracle, capsys, cs.BY_NAME[name], dt, {"skip": skip}, "skip %d" % skip)
    f = kern.split(",")
    assert f[0] == "fsm_sweep_persistent<" + ("float" if dt == np.float32 else "double") and f[4] == "false", kern
    assert f[5] == ("true" if skip else "false") and f[6] == "1" and f[8] == "true", kern


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("name", ["cells_21x20x24", "cells2d_131x67"])
def test_cell_grids(oracle, monkeypatch, capsys, name, dt):
    _clean_env(monkeypatch)
    kern = _run_case(oracle, capsys, cs.BY_NAME[name], dt, {}, "cells")
    assert kern.startswith("fsm_sweep_persistent<"), kern


# ------------------------------------------------------------------------------------------------- rotated template
def _sweep45_kernel(c, dt, env):
    """the kernel launch_sweep45 (fsm_capi.hip) takes: rows while four rows of nnz + 2 values fit 156 KiB of LDS, unless strips are forced"""
    rows = 4 * (c["nodes"][1] + 2) * np.dtype(dt).itemsize <= 156 * 1024 and env != "strips"
    return "fsm_sweep45_rows" if rows else "fsm_sweep45"


ROT = [("rot_1201x150", np.float32, "rows"), ("rot_1201x150", np.float32, "strips"), ("rot_1201x150", np.float64, "rows"),
       ("rot_1201x150", np.float64, "strips"), ("rot_2051x40", np.float32, "rows"), ("rot_8192x64", np.float32, None), ("rot_64x8192", np.float32, None)]


@pytest.mark.parametrize("name,dt,kernel", ROT, ids=["%s-%s-%s" % (n, np.dtype(d).name, k or "library") for n, d, k in ROT])
def test_rotated_template(oracle, monkeypatch, capsys, name, dt, kernel):
    """sweep45 after the axis sweeps: the compared sums are the whole iteration's, as the host sees them.  All K_ROT iterations of a grid
    made with maxit = K_ROT (the rough model does not converge on the elongated grids).  A thread of fsm_sweep45_rows meets
    4 nnx ceil(nnz / blockDim) nodes per iteration, one of fsm_sweep45 4 ceil(nnx / S) nnz: 32 768 on 8192 x 64, four times what m allows
    a thread to add in T -- the decreases are added in double."""
    _clean_env(monkeypatch, {} if kernel is None else {"TTCR_FSM_SWEEP45": kernel})
    c = cs.BY_NAME[name]
    assert np.dtype(dt) in c["dtypes"]
    k45 = _sweep45_kernel(c, dt, kernel)
    kern = _run_case(oracle, capsys, c, dt, {}, "TTCR_FSM_SWEEP45 %s -> %s" % (kernel or "unset", k45))
    assert kern.startswith("fsm_sweep_persistent<") and kern.split(",")[5] == "false", kern   # (no skipping next to sweep45)


# ------------------------------------------------------------------------------------------------- tolerance-grade arithmetic
@pytest.mark.parametrize("name", ["fw_37x35x41", "n2d_130x65"])
def test_tolerance_grade_arithmetic(monkeypatch, capsys, name):
    """arith = 1: the fields are not the oracle's, so F_k comes from the device itself -- a second grid object with option fixed_iters = k
    (k = 1 ... niter).  The same bar applies, because the shortcut applies to these launches too."""
    _clean_env(monkeypatch)
    c, dt, n = cs.BY_NAME[name], np.dtype(np.float32), 2
    g = _grid(c, dt, n)
    g.set_option("arith", 1)
    g.raytrace(*_rows(c, n))
    assert g.last_kernel().endswith(",1>"), g.last_kernel()
    niter = [g.get_niter(q) for q in range(n)]
    assert min(niter) >= 3 and max(niter) < cs.MAXIT, niter
    g2 = _grid(c, dt, n)
    g2.set_option("arith", 1)
    F = [None]
    for k in range(1, max(niter) + 1):
        g2.set_option("fixed_iters", k)
        g2.raytrace(*_rows(c, n))
        assert g2.last_kernel() == g.last_kernel()
        F.append([cs.flat(c, g2.get_grid_traveltimes(q)).copy() for q in range(n)])
    worst = Worst()
    b = cs.bar(dt, c["nodes"])
    for q in range(n):
        K = niter[q]
        np.testing.assert_array_equal(cs.flat(c, g.get_grid_traveltimes(q)), F[K][q])
        ch = g.get_changes(q)[0]
        assert ch.size == K
        for k in range(2, K + 1):
            E, cv = cs.exact_decrease(F[k - 1][q], F[k][q]), float(ch[k - 1])
            if E == 0:
                assert cv == 0.0, (name, q, k, cv)
            else:
                worst.add(abs(cv / E - 1.0) / b, "%s source %d iteration %d: c %.17g E %.17g" % (name, q, k, cv, E))
    worst.report(capsys, "%s fp32 arith 1 [%s]" % (name, g.last_kernel()))
