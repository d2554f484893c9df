"""Every WENO-stage (H = 2) and every 2-D instantiation of fsm_sweep_persistent, launched under its own name and held to the CPU oracle bit
for bit (-m gpu).

tests/test_few_workgroups_gpu.py and tests/test_arith_small_gpu.py do this for the first-order 3-D kernels.  This is the other half of the
table the host picks from (fsm_sweep_plan, ttcr_amd/csrc/fsm_sweep_plan.h): the 3-D WENO stage with one field per workgroup on
chunks of 16 and of 8 levels and with pairs (TTCR_FSM_PAIR=1) on chunks of 8 and of 4, and both stages of the 2-D solver -- each with and
without exact skipping, as a whole-iteration launch with and without the upwind counters sampled ahead (PRE), and as one launch per
sweep (option "mode" = 1): 22 + 16 names per precision, 76 in all.  Here the patches exchange a halo of two columns, the whole-iteration
launch follows the second ticket order, and a solve changes stage on progress words, change maps and brick stamps that are never reset.

Every grid object makes three calls with the four sources of tests/weno_2d_cases.py (in order, reversed, in order again: with fewer slots
than sources several rounds per call, and six or more changes of stage on one set of ticket counters, launch epochs, change maps, stamps
and sweep tallies).  After every call last_kernel() is the instantiation's name, and every slot that holds a field equals the oracle's solve
of its source: field, both iteration counts, the receivers of every source of the call, and the reference's own sums wherever the device
decided with them (test_stopping_sums_gpu._check_history).  The WENO iteration amplifies an ulp of difference in its input to 1e-3 s
(profiles/r06/weno_sensitivity.txt): equality of a converged WENO field is the sharpest detector there is.  Evaluated counts are printed,
never compared between runs: skipping decisions move with timing.
"""
import time

import numpy as np
import pytest

import few_workgroups_cases as fw
import weno_2d_cases as wc
from test_stopping_sums_gpu import _check_history

pytestmark = pytest.mark.gpu

ENV_KEYS = ("TTCR_FSM_WGS", "TTCR_FSM_PAIR", "TTCR_FSM_PRE_MIN", "TTCR_FSM_TIME_ORDER_BELOW", "TTCR_FSM_MODE", "TTCR_FSM_SKIP",
            "TTCR_FSM_LONE_CHUNK", "TTCR_FSM_ARITH", "TTCR_FSM_PAIR_UNITS", "TTCR_FSM_WENO_CH4_MIN", "TTCR_FSM_WENO_C16_BELOW",
            "TTCR_FSM_F64_C16_BELOW", "TTCR_FSM_XS_LDS", "TTCR_FSM_XS_LDS_BELOW", "TTCR_FSM_RS_FIELDS", "TTCR_FSM_SKIP_UNITS",
            "TTCR_FSM_SKIP_PROBE_UNITS", "TTCR_FSM_PREFILL", "TTCR_FSM_SKIP_ALL_DIRTY", "TTCR_FSM_NO_SW")


def _b(v):
    return "true" if v else "false"


class Inst:
    """one instantiation fsm_sweep_persistent<T,PJ,PK,CH,IS3D,SKIP,H,NS,XS,PRE> and how the host is brought to launch it
    (fsm_sweep_plan, ttcr_amd/csrc/fsm_sweep_plan.h; tests/test_sweep_plan.py checks every row on the CPU).  The name is that of the LAST launch of a call: the WENO stage of the last
    round (weno = 0: its first-order stage), so every row is built for the batch size of its last round."""

    def __init__(self, dtype, dim, h, ns, ch, xs, skip, pre):
        self.dtype, self.dim, self.h, self.ns, self.ch, self.xs, self.skip, self.pre = dtype, dim, h, ns, ch, xs, skip, pre
        f64 = np.dtype(dtype) == np.float64
        pj, pk = wc.TILE[(dim, np.dtype(dtype).name)]
        self.name = "fsm_sweep_persistent<%s,%d,%d,%d,%s,%s,%d,%d,%s,%s>" % ("double" if f64 else "float", pj, pk, ch, _b(dim == 3), _b(skip),
                                                                             h, ns, _b(xs), _b(pre))
        self.id = "%s-%dd-h%d-ns%d-c%d-%s-skip%d-pre%d" % ("fp64" if f64 else "fp32", dim, h, ns, ch, "xs" if xs else "mode1", skip, pre)
        self.weno = int(h == 2)
        self.env, self.opts = {}, {"skip": skip}
        if not xs:
            assert not pre
            self.opts["mode"] = 1          # one launch per sweep (the name carries XS = PRE = false)
        if ns == 2:
            # pairs: four slots, two slot groups in every launch
            self.env["TTCR_FSM_PAIR"] = "1"
            self.n_threads = 4
            if dim == 3:
                assert h == 2 and ch in (4, 8)
                self.env["TTCR_FSM_WENO_CH4_MIN"] = "2" if ch == 4 else "100"
                if xs:
                    self.env["TTCR_FSM_PRE_MIN"] = "2" if pre else "100"
        elif dim == 2:
            self.n_threads = 3             # a batch of three, then a lone source
        elif ch == 16:
            # one field per workgroup on chunks of 16 levels: batches below weno_c16_below = 3, whole-iteration launches only.  PRE from
            # pre_min = 2 entries on (no dynamic LDS in the WENO stage): two batches of two, or four lone sources -- the default path of a
            # lone source on a WENO grid
            assert xs and h == 2
            self.n_threads = 2 if pre else 1
        elif xs:
            # chunks of 8 below three entries as well: option lone_chunk.  PRE on: a batch of three, then a lone source that still samples
            # ahead; PRE off: two batches of two
            self.opts["lone_chunk"] = 8
            self.n_threads = 3 if pre else 2
            self.env["TTCR_FSM_PRE_MIN"] = "1" if pre else "100"
        else:
            self.n_threads = 3             # (launches per sweep never use chunks of 16)
        if dim == 2:
            assert ch == 16 and pre == xs   # mode 2 always samples ahead in 2-D


def instantiations(dtype):
    out = [Inst(dtype, 3, 2, 1, 16, True, sk, pre) for sk in (0, 1) for pre in (0, 1)]
    for ns, chs in ((1, (8,)), (2, (8, 4))):
        for ch in chs:
            out += [Inst(dtype, 3, 2, ns, ch, True, sk, pre) for sk in (0, 1) for pre in (0, 1)]
            out += [Inst(dtype, 3, 2, ns, ch, False, sk, 0) for sk in (0, 1)]
    out += [Inst(dtype, 2, h, ns, 16, xs, sk, xs) for h in (1, 2) for ns in (1, 2) for sk in (0, 1) for xs in (True, False)]
    return out


INSTANTIATIONS = [i for dt in wc.DTYPES for i in instantiations(dt)]
assert len(INSTANTIATIONS) == 76 and len({i.name for i in INSTANTIATIONS}) == 76 and not any(i.name.endswith(",1>") for i in INSTANTIATIONS)
INST_3D = [i for i in INSTANTIATIONS if i.dim == 3]
INST_2D = [i for i in INSTANTIATIONS if i.dim == 2]
assert len(INST_3D) == 44 and len(INST_2D) == 32


def _grid(monkeypatch, inst, c, model, extra_env=None, extra_opts=None):
    import ttcr_amd

    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(inst.env, **(extra_env or {})).items():
        monkeypatch.setenv(k, v)
    kw = dict(n_threads=inst.n_threads, cell_slowness=int(c["cell"]), method="FSM", weno=inst.weno, eps=wc.EPS, maxit=wc.maxit(c, model),
              dtype=inst.dtype)
    ax = [a.astype(inst.dtype) for a in wc.axes(c)]
    g = ttcr_amd.Grid3d(*ax, tt_from_rp=0, **kw) if c["dim"] == 3 else ttcr_amd.Grid2d(*ax, **kw)
    for k, v in dict(inst.opts, **(extra_opts or {})).items():
        g.set_option(k, v)
    g.set_slowness(wc.slowness(c, model, inst.dtype))
    return g


def _three_calls(oracle, g, inst, c, model, first, tag):
    """three raytrace calls on one grid object; every slot against the oracle after every call"""
    src, rcv = wc.sources(c), wc.receivers(c)
    refs = [wc.reference(oracle, c, model, inst.dtype, k, weno=bool(inst.weno)) for k in range(wc.N_SRC)]
    thr = wc.threshold(c, inst.dtype)
    for call, order in enumerate((first, first[::-1], first)):
        tt = g.raytrace(np.repeat(src[order], len(rcv), axis=0), np.tile(rcv, (len(order), 1))).reshape(len(order), -1)
        what = tag + ("call", call, "order", order)
        assert g.last_kernel() == inst.name, what
        for q, k in enumerate(order):   # receivers of every source of the call
            np.testing.assert_array_equal(tt[q], refs[k]["tt_rcv"], err_msg=str(what + ("receivers of source", k)))
        slots, _ = fw.held(list(order), inst.n_threads)
        assert len(slots) == inst.n_threads
        for slot, k in slots.items():
            w = what + ("slot", slot, "source", k)
            np.testing.assert_array_equal(wc.flat(c, g.get_grid_traveltimes(slot)), refs[k]["tt"], err_msg=str(w))
            assert (g.get_niter(slot), g.get_niterw(slot)) == (refs[k]["niter"], refs[k]["niterw"]), w
            if inst.weno:
                assert g.get_niterw(slot) >= 2, w           # (the name above is the WENO stage's)
            rc = g.get_reference_changes(slot)
            _check_history(rc[0], refs[k]["change"], thr, w + ("first-order",))
            _check_history(rc[1], refs[k]["changew"], thr, w + ("weno",))
        t = g.timing()
        assert t["node_updates"] > 0, what
        if inst.skip:
            assert t["evaluated_updates"] <= t["node_updates"], (what, t)
    return t


def _run(oracle, monkeypatch, capsys, inst, c, model, first=None, extra_env=None, extra_opts=None):
    first = list(range(wc.N_SRC)) if first is None else first
    for k in range(wc.N_SRC):   # (computed once per case and shared; the oracle's time is not the device's)
        wc.reference(oracle, c, model, inst.dtype, k, weno=bool(inst.weno))
    t0 = time.perf_counter()
    g = _grid(monkeypatch, inst, c, model, extra_env, extra_opts)
    tag = (inst.id, c["name"], model)
    t = _three_calls(oracle, g, inst, c, model, first, tag)
    with capsys.disabled():
        print("\n[weno / 2-D] %-9s %-6s %s  three calls bit-equal to the oracle, %.0f %% of the node updates evaluated in the last, %.2f s"
              % (c["name"], model, g.last_kernel(), 100.0 * t["evaluated_updates"] / t["node_updates"], time.perf_counter() - t0), end="")
    del g


_ids = lambda insts: [i.id for i in insts]


@pytest.mark.parametrize("model", wc.MODELS)
@pytest.mark.parametrize("inst", INST_3D, ids=_ids(INST_3D))
def test_every_3d_weno_instantiation(oracle, monkeypatch, capsys, inst, model):
    _run(oracle, monkeypatch, capsys, inst, wc.MAIN_3D, model)


@pytest.mark.parametrize("model", wc.MODELS)
@pytest.mark.parametrize("c", [wc.MAIN_2D, wc.XZ_2D], ids=lambda c: c["name"])
@pytest.mark.parametrize("inst", INST_2D, ids=_ids(INST_2D))
def test_every_2d_instantiation(oracle, monkeypatch, capsys, inst, c, model):
    """(130, 65): three patches, the last of two columns, dx = dz; (65, 130): a patch of one column, dx != dz -- `variant` is a runtime
    argument, the same names take the other local solver"""
    _run(oracle, monkeypatch, capsys, inst, c, model)


# the other shapes: the skip-on kernels of one field on chunks of 16 (lone sources), one field with a launch per sweep, pairs on chunks of 4
# with PRE, pairs with a launch per sweep; 2-D: one field and pairs in one launch, one field with a launch per sweep
REDUCED_3D = [i for i in INST_3D if i.skip and (i.ns, i.ch, i.xs, i.pre) in ((1, 16, True, 0), (1, 8, False, 0), (2, 4, True, 1), (2, 8, False, 0))]
REDUCED_2D = [i for i in INST_2D if i.skip and i.h == 2 and (i.ns, i.xs) in ((1, True), (2, True), (1, False))]
assert len(REDUCED_3D) == 8 and len(REDUCED_2D) == 6


@pytest.mark.parametrize("model", wc.MODELS)
@pytest.mark.parametrize("c", wc.OTHER_3D, ids=lambda c: c["name"])
@pytest.mark.parametrize("inst", REDUCED_3D, ids=_ids(REDUCED_3D))
def test_other_3d_shapes(oracle, monkeypatch, capsys, inst, c, model):
    """last patches of one and of two columns (narrower than, and as wide as, the halo they serve), a K axis of five nodes, a short march"""
    _run(oracle, monkeypatch, capsys, inst, c, model)


@pytest.mark.parametrize("model", wc.MODELS)
@pytest.mark.parametrize("c", wc.OTHER_2D, ids=lambda c: c["name"])
@pytest.mark.parametrize("inst", REDUCED_2D, ids=_ids(REDUCED_2D))
def test_other_2d_shapes(oracle, monkeypatch, capsys, inst, c, model):
    _run(oracle, monkeypatch, capsys, inst, c, model)


APART = [i for i in INSTANTIATIONS if i.skip and i.ns == 2 and i.h == 2 and (i.pre or not i.xs)]
assert len(APART) == 12


@pytest.mark.parametrize("inst", APART, ids=_ids(APART))
def test_pairs_whose_sources_converge_apart(oracle, monkeypatch, capsys, inst):
    """option pair_sources = 0: the pairs are the (first, second) and (third, fourth) source of the call, and in the order of
    weno_2d_cases.PAIR_ORDER each pair holds two different WENO iteration counts (tests/test_weno_2d_cases.py): the kernel marches a group
    with one live and one finished source (lmask) through the WENO stage"""
    c = wc.MAIN_3D if inst.dim == 3 else wc.MAIN_2D
    _run(oracle, monkeypatch, capsys, inst, c, "smooth", first=wc.PAIR_ORDER[c["name"]], extra_opts={"pair_sources": 0})


SWEEP_BY_SWEEP = [i for i in INSTANTIATIONS if i.skip and i.xs]
assert len(SWEEP_BY_SWEEP) == 24


@pytest.mark.parametrize("model", wc.MODELS)
@pytest.mark.parametrize("inst", SWEEP_BY_SWEEP, ids=_ids(SWEEP_BY_SWEEP))
def test_sweep_by_sweep_ticket_order(oracle, monkeypatch, capsys, inst, model):
    """TTCR_FSM_TIME_ORDER_BELOW=0: no batch is small enough for the start-time order, every launch hands its units out sweep by sweep"""
    _run(oracle, monkeypatch, capsys, inst, wc.MAIN_3D if inst.dim == 3 else wc.MAIN_2D, model, extra_env={"TTCR_FSM_TIME_ORDER_BELOW": "0"})


CELLS = [i for i in INSTANTIATIONS if i.skip and i.xs and i.h == 2 and i.pre and i.ch in (8, 16) and not (i.dim == 3 and i.ns == 1 and i.ch == 16)]
assert len(CELLS) == 8 and {(i.dim, i.ns) for i in CELLS} == {(3, 1), (3, 2), (2, 1), (2, 2)}


@pytest.mark.parametrize("inst", CELLS, ids=_ids(CELLS))
def test_cell_grids(oracle, monkeypatch, capsys, inst):
    """fsm_cells_to_nodes* feeds both stages"""
    _run(oracle, monkeypatch, capsys, inst, wc.CELLS_3D if inst.dim == 3 else wc.CELLS_2D, "smooth")


@pytest.mark.parametrize("dtype", wc.DTYPES, ids=["fp32", "fp64"])
def test_weno_grid_under_mode_0_takes_the_launch_per_sweep_kernel(oracle, monkeypatch, capsys, dtype):
    """fsm_persistent(): stage 1 goes to the persistent kernel whatever the mode -- under mode 0 (first-order stage: fsm_sweep_tile) the WENO
    stage is the launch-per-sweep instantiation, skipping by default"""
    inst = Inst(dtype, 3, 2, 1, 8, False, 1, 0)   # (a row of its own: the table's keeps "mode" = 1 and forces "skip")
    inst.opts = {"mode": 0}
    _run(oracle, monkeypatch, capsys, inst, wc.MAIN_3D, "smooth")
