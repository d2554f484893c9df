"""The looped sweep kernels with few resident workgroups: the unit loop and the ticket order on the device (-m gpu).

The first-order 3-D kernels (fsm_looped, ttcr_amd/csrc/fsm_kernels.h) launch at most 2 048 workgroups, and each takes work units until none
is left.  A workgroup that comes back for a second unit reuses what the first left in LDS (the tile, the scheduler state of the SKIP
kernels, the cached change-map words, s_u[], s_ticket, s_abort) and reads its arguments again through the kernel argument segment.  On a
small grid a launch has fewer units than workgroups, so that second pass is never taken -- unless TTCR_FSM_WGS (read when the grid is
created) caps the workgroups:

    TTCR_FSM_WGS=1    one workgroup evaluates every unit of the launch in ticket order: every carry-over from unit to unit, and an order
                      that names a unit before one it waits for ends in the kernel's time-out (tests/test_unit_order.py checks the order
                      itself on the CPU);
    TTCR_FSM_WGS=3    dozens of units per workgroup with real waiting between them;
    TTCR_FSM_WGS=0    one workgroup per unit;      unset: the control, min(units, 2 048) workgroups.

Every looped default-mode instantiation -- 14 per precision -- runs by name on (37, 35, 41) nodes under all four settings, a reduced set on
the other shapes of tests/few_workgroups_cases.py under 1 and 3, and the XS skip kernels once more sweep by sweep
(TTCR_FSM_TIME_ORDER_BELOW=0).  Every grid object makes three calls (the sources, reversed, the first order again: 12 or more launches on
one set of ticket counters, progress-word epochs, change maps and brick stamps); after every call every slot is held to the CPU oracle bit
for bit -- field, iteration count, receivers, the reference's own sums -- and the fp64 change sums to the control run (atomics: rtol 1e-6,
the bar of tests/test_lone_chunk_gpu.py).  Evaluated counts are not compared between settings: skipping decisions move with timing.
"""
import numpy as np
import pytest

import few_workgroups_cases as fw

pytestmark = pytest.mark.gpu

MAIN = fw.SHAPES[0]
ENV_KEYS = ("TTCR_FSM_WGS", "TTCR_FSM_PAIR", "TTCR_FSM_PRE_MIN", "TTCR_FSM_TIME_ORDER_BELOW", "TTCR_FSM_MODE", "TTCR_FSM_SKIP",
            "TTCR_FSM_LONE_CHUNK", "TTCR_FSM_ARITH", "TTCR_FSM_PAIR_UNITS")


def _b(v):
    return "true" if v else "false"


class Inst:
    """one instantiation fsm_sweep_persistent<T,PJ,PK,CH,true,SKIP,1,NS,XS,PRE> and how the host is brought to launch it
    (fsm_sweep_plan, ttcr_amd/csrc/fsm_sweep_plan.h; tests/test_sweep_plan.py checks every row on the CPU)"""

    def __init__(self, dtype, ns, ch, xs, skip, pre):
        self.dtype, self.ns, self.ch, self.xs, self.skip, self.pre = dtype, ns, ch, xs, skip, pre
        f64 = np.dtype(dtype) == np.float64
        self.name = "fsm_sweep_persistent<%s,16,%d,%d,true,%s,1,%d,%s,%s>" % ("double" if f64 else "float", 8 if f64 else 16, ch, _b(skip), ns,
                                                                             _b(xs), _b(pre))
        self.id = "%s-ns%d-c%d-%s-skip%d-pre%d" % ("fp64" if f64 else "fp32", ns, ch, "xs" if xs else "mode1", skip, pre)
        self.env, self.opts = {}, {"skip": skip}
        if ns == 2:
            # pairs: four slots, two slot groups in every launch; PRE from TTCR_FSM_PRE_MIN groups on
            self.env["TTCR_FSM_PAIR"] = "1"
            self.n_threads = 4
            if xs:
                self.env["TTCR_FSM_PRE_MIN"] = "2" if pre else "100"
        elif ch == 16:
            # one field per workgroup, chunks of 16 (PRE compiled out): a batch of three and a lone source (fp64: batches below five)
            assert xs and not pre
            self.n_threads = 3
        elif xs:
            # chunks of 8.  PRE on: a batch of three (>= the default pre_min of 2), then a lone source (dynamic LDS); PRE off: two batches
            # of two, never a lone source
            self.opts["lone_chunk"] = 8
            self.n_threads = 3 if pre else 2
            if not pre:
                self.env["TTCR_FSM_PRE_MIN"] = "100"
        else:
            self.n_threads = 3
        if not xs:
            assert ch == 8 and not pre
            self.opts["mode"] = 1   # one launch per sweep (the name carries PRE = false)


def instantiations(dtype):
    out = [Inst(dtype, 1, 16, True, sk, False) for sk in (0, 1)]
    out += [Inst(dtype, 1, 8, True, sk, pre) for sk in (0, 1) for pre in (0, 1)]
    out += [Inst(dtype, 2, 8, True, sk, pre) for sk in (0, 1) for pre in (0, 1)]
    out += [Inst(dtype, ns, 8, False, sk, False) for ns in (1, 2) for sk in (0, 1)]
    return out


INSTANTIATIONS = [i for dt in fw.DTYPES for i in instantiations(dt)]
assert len(INSTANTIATIONS) == 28 and len({i.name for i in INSTANTIATIONS}) == 28 and not any(i.name.endswith(",1>") for i in INSTANTIATIONS)


def _grid(monkeypatch, inst, shape, wgs, extra_env=None, extra_opts=None):
    import ttcr_amd

    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    env = dict(inst.env, **(extra_env or {}))
    if wgs is not None:
        env["TTCR_FSM_WGS"] = str(wgs)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = ttcr_amd.Grid3d(*fw.axes(shape), n_threads=inst.n_threads, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, dtype=inst.dtype)
    for k, v in dict(inst.opts, **(extra_opts or {})).items():
        g.set_option(k, v)
    g.set_slowness(fw.slowness(shape, inst.dtype))
    return g


def _three_calls(oracle, g, inst, shape, first, tag, control=None):
    """three raytrace calls on one grid object; every slot against the oracle after every call.  Returns the fp64 change sums
    [call][slot] (compared with `control`, the same list of the control run, when given)."""
    src, rcv = fw.sources(shape), fw.receivers(shape)
    refs = [fw.reference(oracle, shape, inst.dtype, k) for k in range(fw.N_SRC)]
    changes = []
    for call, order in enumerate((first, first[::-1], first)):
        tt = g.raytrace(np.repeat(src[order], len(rcv), axis=0), np.tile(rcv, (len(order), 1))).reshape(len(order), -1)
        what = (tag, "call", call, "order", order)
        assert g.last_kernel() == inst.name, what
        for q, k in enumerate(order):   # receivers of every source of the call
            np.testing.assert_array_equal(tt[q], refs[k]["tt_rcv"], err_msg=str(what + ("receivers of source", k)))
        slots, _ = fw.held(list(order), inst.n_threads)
        assert len(slots) == inst.n_threads
        changes.append({})
        for slot, k in slots.items():
            w = str(what + ("slot", slot, "source", k))
            np.testing.assert_array_equal(g.get_grid_traveltimes(slot).flatten("F"), refs[k]["tt"], err_msg=w)
            assert g.get_niter(slot) == refs[k]["niter"], w
            rc = g.get_reference_changes(slot)[0]
            m = ~np.isnan(rc)
            np.testing.assert_array_equal(rc[m], refs[k]["change"].astype(np.float64)[m], err_msg=w)
            ch = g.get_changes(slot)[0]
            assert ch.size == refs[k]["niter"], w
            changes[-1][slot] = ch
            if control is not None:
                np.testing.assert_allclose(ch, control[call][slot], rtol=1e-6, err_msg=w)
        t = g.timing()
        assert t["node_updates"] > 0, what
        if inst.skip:
            assert t["evaluated_updates"] <= t["node_updates"], (what, t)
    return changes


def _run(oracle, monkeypatch, capsys, inst, shape, settings, first=None, extra_env=None, extra_opts=None):
    first = list(range(fw.N_SRC)) if first is None else first
    control = None
    for wgs in settings:   # (None first: the control)
        g = _grid(monkeypatch, inst, shape, wgs, extra_env, extra_opts)
        tag = (inst.id, "x".join(map(str, shape)), "TTCR_FSM_WGS", "unset" if wgs is None else wgs)
        ch = _three_calls(oracle, g, inst, shape, first, tag, control)
        if wgs is None:
            control = ch
        t = g.timing()
        with capsys.disabled():
            print("\n[few workgroups] %-12s WGS %-5s %s  three calls bit-equal to the oracle, %.0f %% of the node updates evaluated in the last"
                  % (tag[1], tag[3], g.last_kernel(), 100.0 * t["evaluated_updates"] / t["node_updates"]), end="")
        del g


@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=[i.id for i in INSTANTIATIONS])
def test_every_looped_instantiation_with_few_workgroups(oracle, monkeypatch, capsys, inst):
    _run(oracle, monkeypatch, capsys, inst, MAIN, (None, 1, 3, 0))


# the other shapes: pairs + skip + PRE, one field + skip on chunks of 16, pairs with one launch per sweep
REDUCED = [i for i in INSTANTIATIONS if i.skip and ((i.ns, i.ch, i.xs, i.pre) in ((2, 8, True, 1), (1, 16, True, 0), (2, 8, False, 0)))]
assert len(REDUCED) == 6


@pytest.mark.parametrize("shape", fw.SHAPES[1:], ids=["x".join(map(str, s)) for s in fw.SHAPES[1:]])
@pytest.mark.parametrize("inst", REDUCED, ids=[i.id for i in REDUCED])
def test_other_shapes_with_few_workgroups(oracle, monkeypatch, capsys, inst, shape):
    if shape == (70, 17, 9) and inst.ns == 2:
        # every pair holds a source that converges an iteration before the other (tests/test_few_workgroups_cases.py)
        _run(oracle, monkeypatch, capsys, inst, shape, (None, 1, 3), first=fw.PAIR_ORDER_70, extra_opts={"pair_sources": 0})
    else:
        _run(oracle, monkeypatch, capsys, inst, shape, (None, 1, 3))


SWEEP_BY_SWEEP = [i for i in INSTANTIATIONS if i.skip and i.xs and ((i.ns, i.ch, i.pre) in ((2, 8, 1), (1, 16, 0)))]
assert len(SWEEP_BY_SWEEP) == 4


@pytest.mark.parametrize("inst", SWEEP_BY_SWEEP, ids=[i.id for i in SWEEP_BY_SWEEP])
def test_sweep_by_sweep_ticket_order_with_few_workgroups(oracle, monkeypatch, capsys, inst):
    """TTCR_FSM_TIME_ORDER_BELOW=0: no batch is small enough for the start-time order, every launch hands its units out sweep by sweep"""
    _run(oracle, monkeypatch, capsys, inst, MAIN, (None, 1, 3), extra_env={"TTCR_FSM_TIME_ORDER_BELOW": "0"})

