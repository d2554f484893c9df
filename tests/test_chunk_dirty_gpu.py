"""Exact skipping from chunk-shaped dirty bits, on the device (-m gpu).

The first-order 3-D sweep kernels with exact skipping decide per chunk whether it can change a node.  What the sweep before changed
arrives as one bit per (unit, chunk), set by the threads that changed the nodes (ttcr_amd/csrc/fsm_chunk_dirty.h; the arithmetic itself:
tests/test_chunk_dirty_marks.py, CPU) and written out before the unit's final progress value; the reader loads its words after the wait
for the previous sweep and leaves them zero.  DESIGN.md section 4a argues that no evaluation that could change a node is left out; here
the kernels are held to the CPU oracle bit for bit:

  shapes (nodes)   (70, 53, 41), (97, 33, 49), (129, 65, 33): three or more patches per axis (fp32 16 x 16 columns, fp64 16 x 8), remainder
                   patches -- so the partitions of two sweeps that walk an axis in opposite directions differ --, several chunks per unit
  models           gradient 1 / (1 + 0.1 z), uniform, and uniform random slowness in [0.25, 1) per 16^3 block
  sources          five: four off every node (two per pair of the pair kernels), one on a node; four slots, so a call is a batch of four
                   and a lone source (three slots for the kernel with one field per workgroup: batches of three and two)
  kernels          by name (last_kernel): pairs + skip + PRE; one field + skip on chunks of 16; the fp64 pair kernel; pairs with option
                   arith = 1; pairs with one launch per sweep (option mode = 1)
  workgroups       TTCR_FSM_WGS unset and 3 (a workgroup takes dozens of units: the bits of one sweep are read by the same few workgroups
                   that wrote them, and LDS carries over from unit to unit)
  calls            three per grid object: the sources, reversed, the first order again -- the bits, like the stamps, live across the calls

After every call field, iteration count, receivers and the reference's own sums are bit-equal to the oracle.  The tolerance-grade
arithmetic (arith = 1) has no bit-exact CPU restatement (its two 1-ulp hardware operations): exact skipping is held there to what it
promises, the bits of the SAME arithmetic with every chunk evaluated (option skip = 0 on a second grid object): field, iteration count,
receivers, and the reference's sums wherever both solves formed one.  On the gradient model
evaluated_updates < node_updates: the rule is really exercised (the fraction is printed).
"""
import numpy as np
import pytest

import few_workgroups_cases as fw

pytestmark = pytest.mark.gpu

SHAPES = [(70, 53, 41), (97, 33, 49), (129, 65, 33)]
MODELS = ["gradient", "uniform", "block16"]
DX = 0.5
OFF = [(0.31, 0.62, 0.22), (0.93, 0.08, 0.77), (0.12, 0.9, 0.41), (0.55, 0.45, 0.6)]
ENV_KEYS = ("TTCR_FSM_WGS", "TTCR_FSM_PAIR", "TTCR_FSM_PRE_MIN", "TTCR_FSM_TIME_ORDER_BELOW", "TTCR_FSM_MODE", "TTCR_FSM_SKIP",
            "TTCR_FSM_LONE_CHUNK", "TTCR_FSM_ARITH", "TTCR_FSM_PAIR_UNITS", "TTCR_FSM_SKIP_ALL_DIRTY", "TTCR_FSM_NO_SW")

# name -> (dtype, slots, environment, options, kernel the host must launch)
KERNELS = {
    "pairs-skip-pre": (np.float32, 4, {"TTCR_FSM_PAIR": "1", "TTCR_FSM_PRE_MIN": "2"}, {"skip": 1},
                       "fsm_sweep_persistent<float,16,16,8,true,true,1,2,true,true>"),
    "one-field-c16": (np.float32, 3, {}, {"skip": 1}, "fsm_sweep_persistent<float,16,16,16,true,true,1,1,true,false>"),
    "fp64-pairs": (np.float64, 4, {"TTCR_FSM_PAIR": "1", "TTCR_FSM_PRE_MIN": "2"}, {"skip": 1},
                   "fsm_sweep_persistent<double,16,8,8,true,true,1,2,true,true>"),
    "arith1-pairs": (np.float32, 4, {"TTCR_FSM_PAIR": "1", "TTCR_FSM_PRE_MIN": "2"}, {"skip": 1, "arith": 1},
                     "fsm_sweep_persistent<float,16,16,8,true,true,1,2,true,true,1>"),
    "mode1-pairs": (np.float32, 4, {"TTCR_FSM_PAIR": "1"}, {"skip": 1, "mode": 1},
                    "fsm_sweep_persistent<float,16,16,8,true,true,1,2,false,false>"),
}


def axes(shape):
    return [np.arange(m) * DX for m in shape]


def slowness(shape, model, dtype):
    if model == "gradient":
        z = np.arange(shape[2]) * DX
        s = np.broadcast_to(1.0 / (1.0 + 0.1 * z)[None, None, :], shape)
    elif model == "uniform":
        s = np.full(shape, 0.5)
    else:
        b = np.random.default_rng(5).uniform(0.25, 1.0, [(m + 15) // 16 for m in shape])
        for a in range(3):
            b = np.repeat(b, 16, axis=a)
        s = b[tuple(slice(0, m) for m in shape)]
    return np.ascontiguousarray(s, dtype=dtype)


def sources(shape):
    ext = np.array([(m - 1) * DX for m in shape])
    node = np.array([(m // 3) * DX for m in shape])
    return np.vstack([np.array(OFF) * ext, node])


N_SRC = len(OFF) + 1
_REFS = {}


def reference(oracle, shape, model, dtype, k):
    """oracle solve of source k: dict(tt, niter, change, tt_rcv).  Computed once and shared: do not modify."""
    key = (shape, model, np.dtype(dtype).name, k)
    if key not in _REFS:
        _REFS[key] = oracle.solve3d(dtype, tuple(m - 1 for m in shape), DX, (0.0, 0.0, 0.0), slowness(shape, model, dtype).flatten("F"),
                                    sources(shape)[k:k + 1], rcv=fw.receivers(shape))
    return _REFS[key]


def _grid(monkeypatch, kern, shape, model, wgs, opts=None):
    import ttcr_amd

    dtype, slots, env, kopts, _ = KERNELS[kern]
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if wgs is not None:
        monkeypatch.setenv("TTCR_FSM_WGS", str(wgs))
    g = ttcr_amd.Grid3d(*axes(shape), n_threads=slots, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, dtype=dtype)
    for k, v in dict(kopts, **(opts or {})).items():
        g.set_option(k, v)
    g.set_slowness(slowness(shape, model, dtype))
    return g


def _call(g, shape, order):
    src, rcv = sources(shape), fw.receivers(shape)
    return g.raytrace(np.repeat(src[order], len(rcv), axis=0), np.tile(rcv, (len(order), 1))).reshape(len(order), -1)


ORDERS = [list(range(N_SRC)), list(range(N_SRC))[::-1], list(range(N_SRC))]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("kern", [k for k in KERNELS if k != "arith1-pairs"])
def test_bit_equal_to_the_oracle(oracle, monkeypatch, capsys, kern, shape, model):
    dtype, slots, _, _, name = KERNELS[kern]
    refs = [reference(oracle, shape, model, dtype, k) for k in range(N_SRC)]
    for wgs in (None, 3):
        g = _grid(monkeypatch, kern, shape, model, wgs)
        for call, order in enumerate(ORDERS):
            tt = _call(g, shape, order)
            what = (kern, shape, model, "TTCR_FSM_WGS", wgs, "call", call)
            assert g.last_kernel() == name, what
            for q, k in enumerate(order):
                np.testing.assert_array_equal(tt[q], refs[k]["tt_rcv"], err_msg=str(what + ("receivers of source", k)))
            held, _ = fw.held(list(order), slots)
            for slot, k in held.items():
                w = str(what + ("slot", slot, "source", k))
                np.testing.assert_array_equal(g.get_grid_traveltimes(slot).flatten("F"), refs[k]["tt"], err_msg=w)
                assert g.get_niter(slot) == refs[k]["niter"], w
                rc = g.get_reference_changes(slot)[0]
                m = ~np.isnan(rc)
                np.testing.assert_array_equal(rc[m], refs[k]["change"].astype(np.float64)[m], err_msg=w)
            t = g.timing()
            frac = t["evaluated_updates"] / t["node_updates"]
            with capsys.disabled():
                print("\n[chunk dirty] %-14s %-10s %-8s WGS %-5s call %d: bit-equal to the oracle, %.1f %% of the node updates evaluated"
                      % (kern, "x".join(map(str, shape)), model, "unset" if wgs is None else wgs, call, 100.0 * frac), end="")
            assert 0 < t["evaluated_updates"] <= t["node_updates"], (what, t)
            if model == "gradient":
                assert t["evaluated_updates"] < t["node_updates"], (what, t)
        del g


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_arith_1_pairs_bit_equal_to_every_chunk_evaluated(monkeypatch, capsys, shape, model):
    kern = "arith1-pairs"
    _, slots, _, _, name = KERNELS[kern]
    full = _grid(monkeypatch, kern, shape, model, None, {"skip": 0})   # the same arithmetic, no skipping
    want = []
    for order in ORDERS[:2]:   # (the third call repeats the first)
        tt = _call(full, shape, order)
        assert full.last_kernel() == name.replace("true,true,1,2", "true,false,1,2"), full.last_kernel()
        held, _ = fw.held(list(order), slots)
        want.append((tt.copy(), {s: (full.get_grid_traveltimes(s).flatten("F").copy(), full.get_niter(s), full.get_reference_changes(s)[0].copy())
                                 for s in held}))
        t = full.timing()
        assert t["evaluated_updates"] == t["node_updates"]
    del full
    want.append(want[0])
    for wgs in (None, 3):
        g = _grid(monkeypatch, kern, shape, model, wgs)
        for call, order in enumerate(ORDERS):
            tt = _call(g, shape, order)
            what = (kern, shape, model, "TTCR_FSM_WGS", wgs, "call", call)
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
            frac = t["evaluated_updates"] / t["node_updates"]
            with capsys.disabled():
                print("\n[chunk dirty] %-14s %-10s %-8s WGS %-5s call %d: bit-equal to every chunk evaluated, %.1f %% of the node updates evaluated"
                      % (kern, "x".join(map(str, shape)), model, "unset" if wgs is None else wgs, call, 100.0 * frac), end="")
            assert 0 < t["evaluated_updates"] <= t["node_updates"], (what, t)
            if model == "gradient":
                assert t["evaluated_updates"] < t["node_updates"], (what, t)
        del g
