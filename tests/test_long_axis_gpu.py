"""Every sweep kernel with exact skipping where a unit's bit sets pass their first 32-bit word, by name and bit for bit (-m gpu).

fsm_sweep_unit (ttcr_amd/csrc/fsm_kernels.h) keeps four per-unit bit sets indexed along the level axis F: the chunk dirty bits of the
first-order 3-D kernels (reader, first-sweep seed from the frozen boxes, writer with its one-word / two-word split, the scatter into the
next direction's words, the "whole unit clean" loop), the change maps and their upwind lookup, the slab mask of the WENO-stage and 2-D
kernels, and the stamped bricks of every skip kernel.  The other by-name tests (test_chunk_dirty_gpu, test_few_workgroups_gpu,
test_arith_small_gpu, test_weno_2d_gpu) stay below 21 chunks and 9 F bricks per unit: word 0 of each.  The grids here are long and thin
(tests/long_axis_cases.py; tests/test_long_axis_cases.py checks on the CPU that they reach the high words in every direction and that the
oracle still changes nodes there after the first iteration):

  first-order 3-D    the five rows of test_chunk_dirty_gpu.KERNELS on (600, 35, 19) with the 16^3-block model and the gradient;
                     pairs + skip + PRE and the fp64 pair kernel on (2100, 17, 9) (blocks of 64 x 16 x 16) as well; TTCR_FSM_WGS unset
                     and 3; six sources (four slots: a batch of four and one of two; the one-field kernel's three: two of three), two of
                     them on nodes whose frozen boxes straddle chunk 32 on chunks of 8 and of 16.  Option arith = 1 has no bit-exact
                     CPU restatement: held, as in test_chunk_dirty_gpu, to the same arithmetic with every chunk evaluated (skip = 0)
  WENO stage 3-D     the skip = 1 rows of test_weno_2d_gpu.instantiations, both precisions, on (600, 18, 9), 16^3-block model
  2-D                both stages, skip = 1, both precisions, on (130, 600) and (66, 1100) (F = z): the first-order stage on the
                     16^2-block model (6 - 16 iterations), the WENO stage on the smooth model of tests/weno_2d_cases.py.  On grids
                     this long its WENO stage converges for some sources only (39 - 78 iterations) and leaves at maxit = 80 for the
                     others (one of four on (130, 600), three of four on (66, 1100)): there the fields after 80 WENO iterations
                     are compared, bit for bit all the same
  the limit          fsm_skip() (ttcr_amd/csrc/fsm_sweep_plan.h) lets a grid skip up to 32 FSM_SLAB_WORDS = 1024 F bricks: (16384, 17, 2)
                     must run the SKIP = true kernel with the top bit of the top word live, (16385, 17, 2) the SKIP = false one -- with
                     one field per workgroup on chunks of 16 and with pairs on chunks of 8; no other limit of the library rejects
                     these shapes

Each grid object makes three calls: the sources in order, reversed, in order again.  After every call last_kernel() is the expected
name, and for every slot that holds a field: the field, the iteration counts of both stages, the receivers of every source of the call
and the reference's own sums wherever the device formed one equal the oracle's.  evaluated_updates / node_updates is printed;
0 < evaluated <= node_updates, strictly less on the gradient.
"""
import time

import numpy as np
import pytest

import few_workgroups_cases as fw
import long_axis_cases as la
import weno_2d_cases as wc
from test_chunk_dirty_gpu import KERNELS
from test_stopping_sums_gpu import _check_history
from test_weno_2d_gpu import ENV_KEYS, Inst, instantiations

pytestmark = pytest.mark.gpu

ids = lambda c: c["name"]


def _make(monkeypatch, c, model, dtype, n_threads, weno, env, opts):
    import ttcr_amd

    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(n_threads=n_threads, cell_slowness=0, method="FSM", weno=int(weno), eps=wc.EPS, maxit=la.maxit(c, model), dtype=dtype)
    ax = [a.astype(dtype) for a in wc.axes(c)]
    g = ttcr_amd.Grid3d(*ax, tt_from_rp=0, **kw) if c["dim"] == 3 else ttcr_amd.Grid2d(*ax, **kw)
    for k, v in opts.items():
        g.set_option(k, v)
    g.set_slowness(la.slowness(c, model, dtype))
    return g


def _orders(c):
    first = list(range(la.n_src(c)))
    return [first, first[::-1], first]


def _raytrace(g, c, order):
    src, rcv = la.sources(c), la.receivers(c)
    return g.raytrace(np.repeat(src[order], len(rcv), axis=0), np.tile(rcv, (len(order), 1))).reshape(len(order), -1)


def _three_calls(oracle, g, c, model, dtype, weno, n_threads, name, tag, exact_sums, after_call=None):
    """three raytrace calls on one grid object; every slot against the oracle after every call"""
    refs = [la.reference(oracle, c, model, dtype, k, weno=weno) for k in range(la.n_src(c))]
    thr = wc.threshold(c, dtype)
    t = None
    for call, order in enumerate(_orders(c)):
        tt = _raytrace(g, c, order)
        what = tag + ("call", call)
        assert g.last_kernel() == name, (what, g.last_kernel())
        for q, k in enumerate(order):
            np.testing.assert_array_equal(tt[q], refs[k]["tt_rcv"], err_msg=str(what + ("receivers of source", k)))
        slots, _ = fw.held(list(order), n_threads)
        assert len(slots) == n_threads
        for slot, k in slots.items():
            w = what + ("slot", slot, "source", k)
            np.testing.assert_array_equal(wc.flat(c, g.get_grid_traveltimes(slot)), refs[k]["tt"], err_msg=str(w))
            assert (g.get_niter(slot), g.get_niterw(slot)) == (refs[k]["niter"], refs[k]["niterw"]), w
            rc = g.get_reference_changes(slot)
            if exact_sums:   # first-order 3-D: every sum the device formed is the whole sum
                m = ~np.isnan(rc[0])
                np.testing.assert_array_equal(rc[0][m], refs[k]["change"].astype(np.float64)[m], err_msg=str(w))
            else:
                _check_history(rc[0], refs[k]["change"], thr, w + ("first-order",))
                _check_history(rc[1], refs[k]["changew"], thr, w + ("weno",))
            if weno:
                assert g.get_niterw(slot) >= 2, w           # (the name above is the WENO stage's)
        t = g.timing()
        assert 0 < t["evaluated_updates"] <= t["node_updates"], (what, t)
        if after_call:
            after_call(call, t, what)
    return t


# ------------------------------------------------------------------------------------------------------------ first-order 3-D
FIRST_ORDER = [(kern, la.LONG, m) for kern in KERNELS if kern != "arith1-pairs" for m in ("block16", "gradient")]
FIRST_ORDER += [(kern, la.LONGER, m) for kern in ("pairs-skip-pre", "fp64-pairs") for m in ("block64", "gradient")]
assert len(KERNELS) == 5 and len(FIRST_ORDER) == 12


def _print_fraction(capsys, kern, c, model, wgs, how):
    def f(call, t, what):
        with capsys.disabled():
            print("\n[long axis] %-14s %-10s %-8s WGS %-5s call %d: bit-equal to %s, %.1f %% of the node updates evaluated"
                  % (kern, c["name"], model, "unset" if wgs is None else wgs, call, how, 100.0 * t["evaluated_updates"] / t["node_updates"]), end="")
        if model == "gradient":
            assert t["evaluated_updates"] < t["node_updates"], (what, t)
    return f


@pytest.mark.parametrize("wgs", [None, 3], ids=["wgs-unset", "wgs-3"])
@pytest.mark.parametrize("kern,c,model", FIRST_ORDER, ids=["%s-%s-%s" % (k, c["name"], m) for k, c, m in FIRST_ORDER])
def test_first_order_3d_bit_equal_to_the_oracle(oracle, monkeypatch, capsys, kern, c, model, wgs):
    dtype, slots, env, opts, name = KERNELS[kern]
    if wgs is not None:
        env = dict(env, TTCR_FSM_WGS=str(wgs))
    g = _make(monkeypatch, c, model, dtype, slots, False, env, opts)
    _three_calls(oracle, g, c, model, dtype, False, slots, name, (kern, c["name"], model, "TTCR_FSM_WGS", wgs), True,
                 _print_fraction(capsys, kern, c, model, wgs, "the oracle"))
    del g


@pytest.mark.parametrize("model", ["block16", "gradient"])
def test_arith_1_pairs_bit_equal_to_every_chunk_evaluated(monkeypatch, capsys, model):
    kern, c = "arith1-pairs", la.LONG
    dtype, slots, env, opts, name = KERNELS[kern]
    full = _make(monkeypatch, c, model, dtype, slots, False, env, dict(opts, skip=0))   # the same arithmetic, no skipping
    want = []
    for order in _orders(c)[:2]:   # (the third call repeats the first)
        tt = _raytrace(full, c, order)
        assert full.last_kernel() == name.replace("true,true,1,2", "true,false,1,2"), full.last_kernel()
        held, _ = fw.held(list(order), slots)
        want.append((tt.copy(), {s: (full.get_grid_traveltimes(s).flatten("F").copy(), full.get_niter(s), full.get_reference_changes(s)[0].copy())
                                 for s in held}))
        t = full.timing()
        assert t["evaluated_updates"] == t["node_updates"]
    del full
    want.append(want[0])
    for wgs in (None, 3):
        g = _make(monkeypatch, c, model, dtype, slots, False, env if wgs is None else dict(env, TTCR_FSM_WGS=str(wgs)), opts)
        show = _print_fraction(capsys, kern, c, model, wgs, "every chunk evaluated")
        for call, order in enumerate(_orders(c)):
            tt = _raytrace(g, c, order)
            what = (kern, c["name"], model, "TTCR_FSM_WGS", wgs, "call", call)
            assert g.last_kernel() == name, what
            np.testing.assert_array_equal(tt, want[call][0], err_msg=str(what + ("receivers",)))
            for slot, (field, niter, rc_full) in want[call][1].items():
                np.testing.assert_array_equal(g.get_grid_traveltimes(slot).flatten("F"), field, err_msg=str(what + ("slot", slot)))
                assert g.get_niter(slot) == niter, what
                # the reference's own sums, wherever both solves were decided with one (which iterations are depends on the stamps)
                rc = g.get_reference_changes(slot)[0]
                m = ~np.isnan(rc) & ~np.isnan(rc_full)
                np.testing.assert_array_equal(rc[m], rc_full[m], err_msg=str(what + ("reference sums, slot", slot)))
            t = g.timing()
            assert 0 < t["evaluated_updates"] <= t["node_updates"], (what, t)
            show(call, t, what)
        del g


# ------------------------------------------------------------------------------------------------- WENO stage 3-D, both stages 2-D
def _run_inst(oracle, monkeypatch, capsys, inst, c, model):
    for k in range(la.n_src(c)):   # (computed once per module and shared; the oracle's time is not the device's)
        la.reference(oracle, c, model, inst.dtype, k, weno=bool(inst.weno))
    t0 = time.perf_counter()
    g = _make(monkeypatch, c, model, inst.dtype, inst.n_threads, inst.weno, inst.env, inst.opts)
    t = _three_calls(oracle, g, c, model, inst.dtype, bool(inst.weno), inst.n_threads, inst.name, (inst.id, c["name"], model), False)
    with capsys.disabled():
        print("\n[long axis] %-9s %-8s %s  three calls bit-equal to the oracle, %.0f %% of the node updates evaluated in the last, %.2f s"
              % (c["name"], model, g.last_kernel(), 100.0 * t["evaluated_updates"] / t["node_updates"], time.perf_counter() - t0), end="")
    del g


SKIP_3D = [i for dt in la.DTYPES for i in instantiations(dt) if i.dim == 3 and i.skip]
SKIP_2D = [i for dt in la.DTYPES for i in instantiations(dt) if i.dim == 2 and i.skip]
assert len(SKIP_3D) == 22 and len(SKIP_2D) == 16 and {i.h for i in SKIP_3D} == {2} and {i.h for i in SKIP_2D} == {1, 2}
assert {(i.ns, i.ch) for i in SKIP_3D} == {(1, 16), (1, 8), (2, 8), (2, 4)}


@pytest.mark.parametrize("inst", SKIP_3D, ids=[i.id for i in SKIP_3D])
def test_weno_stage_3d(oracle, monkeypatch, capsys, inst):
    assert la.n_src(la.LONG_WENO) == wc.N_SRC   # (the rows are built for the batch sizes of a call of four sources)
    _run_inst(oracle, monkeypatch, capsys, inst, la.LONG_WENO, "block16")


@pytest.mark.parametrize("c", la.LONG_2D, ids=ids)
@pytest.mark.parametrize("inst", SKIP_2D, ids=[i.id for i in SKIP_2D])
def test_2d(oracle, monkeypatch, capsys, inst, c):
    assert la.n_src(c) == wc.N_SRC
    _run_inst(oracle, monkeypatch, capsys, inst, c, "smooth" if inst.weno else "block16")


# ---------------------------------------------------------------------------------------------------------------- the limit
@pytest.mark.parametrize("model", ["block256", "gradient"])
@pytest.mark.parametrize("pair", [None, "1"], ids=["one-field", "pairs"])
@pytest.mark.parametrize("dtype", la.DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("c,skip", [(la.LIMIT[0], "true"), (la.LIMIT[1], "false")], ids=[c["name"] for c in la.LIMIT])
def test_the_limit(oracle, monkeypatch, capsys, c, skip, dtype, pair, model):
    """option skip = 1, two slots, three sources (a batch of two and a lone source): 1024 F bricks skip, 1025 do not.  With the
    environment unset two slots take the kernel of one field per workgroup on chunks of 16 (chunk indices up to 1024: dirty-bit word
    32); TTCR_FSM_PAIR=1 takes the pair kernel on chunks of 8 (up to 2049: word 64, the last of the 65 the host gives a unit)."""
    g = _make(monkeypatch, c, model, dtype, 2, False, {} if pair is None else {"TTCR_FSM_PAIR": pair}, {"skip": 1})
    _raytrace(g, c, [0])
    name = g.last_kernel()
    f = name.split(",")
    assert name.startswith("fsm_sweep_persistent<") and f[4] == "true" and f[5] == skip and f[6] == "1", name
    assert (f[3], f[7]) == (("16", "1") if pair is None else ("8", "2")), name

    def show(call, t, what):
        with capsys.disabled():
            print("\n[long axis] limit %-11s %-8s %s call %d: bit-equal to the oracle, %.1f %% of the node updates evaluated"
                  % (c["name"], model, g.last_kernel(), call, 100.0 * t["evaluated_updates"] / t["node_updates"]), end="")
        if skip == "false":
            assert t["evaluated_updates"] == t["node_updates"], (what, t)

    _three_calls(oracle, g, c, model, dtype, False, 2, name, ("limit", c["name"], model, np.dtype(dtype).name), True, show)
    del g
