"""What tests/test_weno_2d_gpu.py relies on, checked on the CPU so that it cannot silently stop holding (tests/weno_2d_cases.py): the oracle
is the compiled reference on every new case -- the shapes are thinner than anything it had been pinned on under WENO --, every solve
reaches the WENO stage and stays in it for at least two iterations (last_kernel() then names the WENO kernel), the rough model leaves at
the cap and the smooth one converges with the sources of a batch finishing apart, and every shape has the patch remainder it was chosen
for."""
import numpy as np
import pytest

import few_workgroups_cases as fw
import weno_2d_cases as wc
from test_oracle_vs_reference import HAVE_REF, needs_ref

ROWS = wc.rows()
IDS = ["%s-%s" % (c["name"], m) for c, m in ROWS]

# WENO iterations of the four sources on the smooth model (measured with the oracle; fp64 in brackets where it differs)
NITERW = {"37x35x41": [9, 8, 11, 11], "17x33x34": [7, 6, 9, 9], "17x34x33": [7, 6, 8, 9], "41x18x5": [7, 5, 7, 8], "9x49x17": [7, 6, 7, 9],
          "65x130": [29, 23, 17, 41], "130x65": [20, 21, 27, 24], "66x37": [12, 13, 21, 15], "17x33x34c": [7, 6, 9, 9],
          "66x37c": [12, 13, 21, 16]}
NITERW_F64 = {"65x130": [29, 23, 17, 40]}


@pytest.fixture(scope="module")
def O(oracle):
    if HAVE_REF:
        oracle.build(with_ref=True)
    return oracle


def _stages(c):
    """the WENO solve, and for the 2-D node grids the first-order solve of the H = 1 rows as well"""
    return (True, False) if c["dim"] == 2 and not c["cell"] else (True,)


@needs_ref
@pytest.mark.parametrize("c,model", ROWS, ids=IDS)
def test_oracle_is_the_reference(O, c, model):
    """field, both iteration counts and receivers (the compiled reference hands out no histories: the oracle's are held by the iteration
    counts, which follow from them, and by numpy below)"""
    for dt in wc.DTYPES:
        for weno in _stages(c):
            for k in range(wc.N_SRC):
                a, b = wc.reference(O, c, model, dt, k, weno), wc.reference(O, c, model, dt, k, weno, ref=True)
                tag = (c["name"], model, np.dtype(dt).name, "weno", weno, "source", k)
                assert (a["niter"], a["niterw"]) == (b["niter"], b["niterw"]), (tag, a["niter"], a["niterw"], b["niter"], b["niterw"])
                np.testing.assert_array_equal(a["tt"], b["tt"], err_msg=str(tag))
                np.testing.assert_array_equal(a["tt_rcv"], b["tt_rcv"], err_msg=str(tag))


@needs_ref
@pytest.mark.parametrize("c", [wc.OTHER_3D[0], wc.XZ_2D], ids=lambda c: c["name"])
def test_oracle_histories_are_the_references_sums(O, c):
    """The reference run with maxit = j stops after j iterations of a stage: the sequential sum of abs(field after j - 1 - field after j) in the
    grid's precision (numpy's accumulate: the same chain of additions) is the `change` of iteration j.  First-order stage: every iteration;
    WENO stage: from iteration niter + 1 on (a smaller maxit cuts the first-order stage short as well)."""
    nc = tuple(m - 1 for m in c["n"])
    for dt in wc.DTYPES:
        o = wc.reference(O, c, "smooth", dt, 0, True)
        s = wc.flat(c, wc.slowness(c, "smooth", dt))
        src = wc.sources(c)[:1]

        def field(j, weno):
            kw = dict(eps=wc.EPS, maxit=j, weno=weno)
            if c["dim"] == 3:
                return O.ref_solve3d(dt, nc, c["d"][0], (0.0, 0.0, 0.0), s, src, **kw)["tt"]
            return O.ref_solve2d(dt, nc, c["d"][0], c["d"][1], (0.0, 0.0), s, src, **kw)["tt"]

        def seq(a, b):
            with np.errstate(over="ignore"):
                return np.add.accumulate(np.abs(a - b))[-1]

        # (a grid without the WENO stage freezes a smaller box around the source: its first-order fields are its own)
        o1 = wc.reference(O, c, "smooth", dt, 0, False)
        T = [field(j, False) for j in range(1, o1["niter"] + 1)]
        assert len(T) >= 2
        for j in range(1, len(T)):
            assert seq(T[j - 1], T[j]) == o1["change"][j], (c["name"], dt, "first-order iteration", j + 1)
        n1, nw = o["niter"], o["niterw"]
        assert nw >= n1 + 3
        W = {j: field(j, True) for j in range(n1, n1 + 3)}
        for j in range(n1 + 1, n1 + 3):
            assert seq(W[j - 1], W[j]) == o["changew"][j - 1], (c["name"], dt, "WENO iteration", j)


@pytest.mark.parametrize("c,model", ROWS, ids=IDS)
def test_iteration_counts(oracle, c, model):
    for dt in wc.DTYPES:
        o = [wc.reference(oracle, c, model, dt, k) for k in range(wc.N_SRC)]
        n, nw = [a["niter"] for a in o], [a["niterw"] for a in o]
        tag = (c["name"], model, np.dtype(dt).name, n, nw)
        assert min(n) >= 2 and min(nw) >= 2, tag
        assert all(a["change"].size == a["niter"] and a["changew"].size == a["niterw"] for a in o), tag
        if model == "rough":
            assert nw == [wc.maxit(c, model)] * wc.N_SRC == [15] * wc.N_SRC, tag          # the WENO stage leaves at the cap
            assert max(n) < 15, tag                                                        # (the first-order stage does not)
        else:
            assert max(n) < wc.maxit(c, model) and max(nw) < wc.maxit(c, model), tag       # the stopping rule ended both stages
            assert len(set(nw)) >= 2, tag
            want = NITERW_F64.get(c["name"], NITERW[c["name"]]) if np.dtype(dt) == np.float64 else NITERW[c["name"]]
            assert nw == want, tag
        for weno in _stages(c)[1:]:   # the H = 1 rows of the 2-D table: weno = 0 grids
            o1 = [wc.reference(oracle, c, model, dt, k, weno) for k in range(wc.N_SRC)]
            assert min(a["niter"] for a in o1) >= 2 and all(a["niterw"] == 0 for a in o1), tag
            assert max(a["niter"] for a in o1) < wc.maxit(c, model), tag


@pytest.mark.parametrize("dt", wc.DTYPES, ids=["fp32", "fp64"])
def test_batches_hold_sources_that_converge_at_different_weno_iterations(oracle, dt):
    """smooth model: the rounds of three and of four slots hold different WENO iteration counts -- the kernels meet converged batch
    entries (grp < 0) in the WENO stage"""
    for c in wc.CASES:
        nw = [wc.reference(oracle, c, "smooth", dt, k)["niterw"] for k in range(wc.N_SRC)]
        for order in (list(range(wc.N_SRC)), list(range(wc.N_SRC))[::-1]):
            for n_threads in (2, 3, 4):
                _, rounds = fw.held(order, n_threads)
                assert any(len({nw[k] for k in r}) > 1 for r in rounds), (c["name"], n_threads, nw)


@pytest.mark.parametrize("dt", wc.DTYPES, ids=["fp32", "fp64"])
def test_the_pair_order_puts_different_weno_counts_in_each_pair(oracle, dt):
    """four slots, option pair_sources = 0: the pairs are the (first, second) and (third, fourth) source of the call"""
    assert set(wc.PAIR_ORDER) == {wc.MAIN_3D["name"], wc.MAIN_2D["name"]}
    for name, first in wc.PAIR_ORDER.items():
        assert sorted(first) == list(range(wc.N_SRC))
        nw = [wc.reference(oracle, wc.BY_NAME[name], "smooth", dt, k)["niterw"] for k in range(wc.N_SRC)]
        for order in (first, first[::-1]):
            assert fw.held(order, 4)[0] == dict(enumerate(order))
            assert nw[order[0]] != nw[order[1]] and nw[order[2]] != nw[order[3]], (name, order, nw)


def test_patch_remainders():
    """(number of patches, columns of the last one) along J and K: what each shape was chosen for"""
    f32, f64 = np.float32, np.float64
    assert wc.TILE == {(3, "float32"): (16, 16), (3, "float64"): (16, 8), (2, "float32"): (64, 1), (2, "float64"): (64, 1)} and wc.HALO == 2
    p = lambda name, dt: wc.patches(wc.BY_NAME[name], dt)
    assert p("37x35x41", f32) == [(3, 3), (3, 9)] and p("37x35x41", f64) == [(3, 3), (6, 1)]
    # narrower than the halo (1 column) in J, as wide as the halo (2) in K, in both precisions
    assert p("17x33x34", f32) == [(3, 1), (3, 2)] and p("17x33x34", f64) == [(3, 1), (5, 2)]
    # ... and the other way round: a K patch of one column in both precisions
    assert p("17x34x33", f32) == [(3, 2), (3, 1)] and p("17x34x33", f64) == [(3, 2), (5, 1)]
    assert p("17x33x34c", f32) == p("17x33x34", f32) and p("17x33x34c", f64) == p("17x33x34", f64)
    assert wc.BY_NAME["17x33x34"]["n"][0] == 16 + 1                      # one more level than a chunk of 16
    # a K axis barely wider than the 2 H columns the two halos take
    assert p("41x18x5", f32) == [(2, 2), (1, 5)] and p("41x18x5", f64) == [(2, 2), (1, 5)] and 5 == 2 * wc.HALO + 1
    assert p("9x49x17", f32) == [(4, 1), (2, 1)] and p("9x49x17", f64) == [(4, 1), (3, 1)]
    for dt in (f32, f64):
        assert p("65x130", dt) == [(2, 1)] and p("130x65", dt) == [(3, 2)] and p("66x37", dt) == p("66x37c", dt) == [(2, 2)]
    # the largest patch grid is 3 x 6 (3-D) and 3 (2-D): all inside what tests/test_unit_order.py checks the H = 2 order on
    assert max(n for c in wc.CASES if c["dim"] == 3 for dt in (f32, f64) for n, _ in wc.patches(c, dt)) == 6
    assert sorted({wc.patches(c, f32)[0][0] for c in wc.CASES if c["dim"] == 2}) == [2, 3]


def test_unit_order_checks_these_shapes():
    import test_unit_order as tu

    for c in wc.CASES:
        assert c["n"] in (tu.SHAPES_3D if c["dim"] == 3 else tu.SHAPES_2D), c["name"]


def test_inputs():
    for c in wc.CASES:
        hi = np.array([(m - 1) * h for m, h in zip(c["n"], c["d"])])
        src, rcv = wc.sources(c), wc.receivers(c)
        assert src.shape == (4, c["dim"]) and np.all(src > 0) and np.all(src < hi)
        assert np.all(rcv >= 0) and np.all(rcv <= hi) and len(rcv) >= 5
        # corners, and a point off every node plane
        assert np.any(np.all(rcv == 0, axis=1)) and np.any(np.all(np.abs(rcv / c["d"] - np.round(rcv / c["d"])) > 0.1, axis=1))
        # the last planes: at most a few fp32 ulp inside
        assert np.all(rcv.max(axis=0) >= hi * (1 - 1e-6))
        for dt in wc.DTYPES:
            # both precisions work on the same spacings: the axes' first step, in the grid's dtype, is the case's
            assert all(float(a.astype(dt)[1] - a.astype(dt)[0]) == h for a, h in zip(wc.axes(c), c["d"])), c["name"]
            for m in ([] if c["cell"] else ["rough"]) + ["smooth"]:
                s = wc.slowness(c, m, dt)
                assert s.dtype == dt and s.shape == (tuple(v - 1 for v in c["n"]) if c["cell"] else c["n"]) and s.min() > 0.05 and s.max() <= 1.25
    r = wc.slowness(wc.MAIN_3D, "rough", np.float64)
    assert 0.25 <= r.min() and r.max() < 1.0
    assert wc.XZ_2D["d"][0] != wc.XZ_2D["d"][1] and wc.MAIN_2D["d"][0] == wc.MAIN_2D["d"][1]
    assert np.float32(wc.DX2) == np.float32(0.2) and np.float32(wc.DZ2) == np.float32(0.3)


def test_instantiation_table():
    """the table of tests/test_weno_2d_gpu.py (its count and the uniqueness of its names are asserted when it is imported)"""
    import test_weno_2d_gpu as tg

    names = [i.name for i in tg.INSTANTIATIONS]
    assert len(names) == len(set(names)) == 76 and not any(n.endswith(",1>") for n in names)
    f = [n[len("fsm_sweep_persistent<"):-1].split(",") for n in names]
    # T, PJ, PK, CH, IS3D, SKIP, H, NS, XS, PRE
    assert all(len(q) == 10 for q in f)
    assert sum(q[4] == "true" for q in f) == 44 and all(q[6] == "2" for q in f if q[4] == "true")
    assert sum(q[4] == "false" and q[6] == "1" for q in f) == sum(q[4] == "false" and q[6] == "2" for q in f) == 16
    assert not any(q[8] == "false" and q[9] == "true" for q in f)                        # PRE only in the whole-iteration launch
    assert all((q[1], q[2]) == ("64", "1") and q[3] == "16" and q[8] == q[9] for q in f if q[4] == "false")
    assert {(q[7], q[3]) for q in f if q[4] == "true"} == {("1", "16"), ("1", "8"), ("2", "8"), ("2", "4")}
    for i in tg.INSTANTIATIONS:
        # the batch of the last round decides the name: lone sources where the table says so, whole batches elsewhere
        _, rounds = fw.held(list(range(wc.N_SRC)), i.n_threads)
        last = len(rounds[-1]) if i.ns == 1 else (len(rounds[-1]) + 1) // 2
        if i.dim == 3 and i.ch == 16:
            assert last < 3 and i.xs
        if i.dim == 3 and i.xs:
            assert bool(i.pre) == (last >= int(i.env.get("TTCR_FSM_PRE_MIN", 2))), i.id
        if i.dim == 3 and i.ns == 2:
            assert (i.ch == 4) == (last >= int(i.env["TTCR_FSM_WENO_CH4_MIN"])), i.id
