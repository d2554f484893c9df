"""The sums of the default stopping rule (stopping_rule = 1: the reference's sequential T1 sum of abs(times[n] - T[n]), computed in
parallel, fsm_refsum_* in fsm_kernels.h) at the shapes, layouts, stages and precisions where a wrong sum would not change an iteration
count:
  A. solves built so that a chosen iteration is DECIDED by that sum (tests/stopping_sums_cases.py): the sum the device took the decision
     with is the oracle's `change` of that iteration, bit for bit -- odd node counts (one element per lane), partial blocks and bricks,
     every vector layout of the term pass, brick stamps and the fallback to whole fields, pair layout with a lone source, strided
     fields and small batches, 3-D cell grids, 2-D grids, the WENO stage, fp64;
  B. reference_change() -- the parallel form and the one-chain kernel -- against numpy's sequential sum (np.add.accumulate of a
     contiguous array is the same chain of additions in the array's dtype) at sizes around the head, the first window and the tile,
     with empty heads, subnormal sums, overflow to infinity, binade crossings on tile and chunk seams, and the largest window."""
import numpy as np
import pytest

import stopping_sums_cases as sc

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------- A
# layout -> (TTCR_FSM_PAIR, slots = sources, TTCR_FSM_RS_FIELDS)
LAYOUTS = {
    "single": ("0", 1, None),            # one field per slot
    "pair2": ("1", 2, None),             # two fields per workgroup, interleaved
    "pair3": ("1", 3, None),             # ... the second group holds one source: its other term array is null
    "single-strided": ("0", 3, "0"),     # no room for compact term arrays: the sums go by the strided fields
    "single-batch2": ("0", 3, "2"),      # batches of two fields
    "pair-strided": ("1", 3, "0"),
    "pair-batch2": ("1", 3, "2"),
}


def _grid(c, dt, n_src, eps):
    import ttcr_amd

    ax, _ = sc.axes(c, dt)
    if c["dim"] == 3:
        return ttcr_amd.Grid3d(*ax, n_threads=n_src, cell_slowness=int(c["cell"]), method="FSM", tt_from_rp=0, weno=int(c["weno"]), eps=eps, dtype=dt.type)
    return ttcr_amd.Grid2d(*ax, n_threads=n_src, cell_slowness=int(c["cell"]), method="FSM", weno=int(c["weno"]), eps=eps, dtype=dt.type)


def _solve(c, dt, n_src, eps, opts):
    g = _grid(c, dt, n_src, eps)
    g.set_slowness(sc.slowness(c))
    for k, v in opts.items():
        g.set_option(k, v)
    g.raytrace(sc.sources(c, n_src), np.zeros((n_src, c["dim"])))
    out = [dict(niter=g.get_niter(i), niterw=g.get_niterw(i), ref=g.get_reference_changes(i), tt=sc.flat(c, g.get_grid_traveltimes(i)))
           for i in range(n_src)]
    return out, g.stopping_stats(), g.last_kernel()


def _check_history(got, ref, thr, tag):
    """sums handed out by get_reference_changes against the oracle's of the same iterations: a value below the threshold is the whole sum,
    bit for bit; one at or above it may have been cut short there (a sequential sum of non-negative terms only grows).  Returns the
    number of whole sums."""
    ref = np.asarray(ref, dtype=np.float64)
    assert got.size == ref.size, (tag, got, ref)
    m = ~np.isnan(got)
    below = m & (ref < thr)
    assert np.array_equal(got[below], ref[below]), (tag, got, ref, thr)
    cut = m & ~below
    assert np.all((got[cut] >= thr) & (got[cut] <= ref[cut])), (tag, got, ref, thr)
    return int(below.sum())


def _decided_by_the_reference_sum(oracle, c, dt, layout, monkeypatch):
    pair, n_src, rs = LAYOUTS[layout]
    monkeypatch.setenv("TTCR_FSM_PAIR", pair)
    if rs is not None:
        monkeypatch.setenv("TTCR_FSM_RS_FIELDS", rs)
    else:
        monkeypatch.delenv("TTCR_FSM_RS_FIELDS", raising=False)
    one_asked_in_a_group = False
    first_order_3d = c["dim"] == 3 and not c["weno"]
    ks = sc.targets(oracle, c, dt)
    assert ks
    for k in ks:
        eps, thr, o2 = sc.aim(oracle, c, dt, k)            # (asserts the CPU precondition)
        thr = float(thr)
        refs = [o2] + [sc.solve(oracle, c, dt, i, eps) for i in range(1, n_src)]
        for v in (0, 1):
            opts = {"stopping_shortcuts": v}
            if first_order_3d:
                opts["skip"] = 1                            # (exact skipping keeps the brick stamps)
            out, st, kern = _solve(c, dt, n_src, eps, opts)
            tag = (c["name"], dt.name, layout, "k", k, "shortcuts", v)
            print(tag, kern, st, "eps", eps, "thr", thr)
            if first_order_3d:
                f = kern.split(",")
                assert f[7] == ("2" if pair == "1" and n_src >= 2 else "1") and f[5] == "true", kern
            assert st["reference_sums_missed"] == 0 and st["reference_sums"] > 0, (tag, st)
            whole = [0] * n_src
            for i in range(n_src):
                o, r = refs[i], out[i]
                print("  source", i, "device", r["ref"], "oracle", o["change"], o["changew"])
                assert (r["niter"], r["niterw"]) == (o["niter"], o["niterw"]), (tag, i, r["niter"], r["niterw"], o["niter"], o["niterw"])
                assert np.array_equal(r["tt"], o["tt"]), (tag, i)
                whole[i] += _check_history(r["ref"][0], o["change"], thr, tag + (i, "first-order"))
                whole[i] += _check_history(r["ref"][1], o["changew"], thr, tag + (i, "weno"))
            assert whole[0] >= 1, (tag, whole)
            # three sources lie in two slot groups, two and one: an iteration in which one or all three were asked had a group of
            # which one source was asked -- the term pass then runs with the other term array null
            for j in range(max(r["ref"][0].size for r in out)):
                asked = sum(1 for r in out if j < r["ref"][0].size and not np.isnan(r["ref"][0][j]))
                one_asked_in_a_group = one_asked_in_a_group or asked % 2 == 1
            got = out[0]["ref"][1 if c["weno"] else 0]
            want = sc.history(c, o2)
            # the decision of the targeted iteration was taken with the reference's sum itself: a whole sum, not NaN, bit for bit
            assert got.size == k + 1 and not np.isnan(got[k]), (tag, got, want)
            assert got[k] == float(want[k]) and dt.type(got[k]) == want[k] and got[k] < thr, (tag, got, want, thr)
    if layout == "pair3":
        assert one_asked_in_a_group, "no term pass of this row ran with one term array null"


ROWS_3D = [(n, dt, lay) for n in sc.FIRST_ORDER_3D for dt in sc.BY_NAME[n]["dtypes"] for lay in LAYOUTS]


@pytest.mark.parametrize("name,dt,layout", ROWS_3D, ids=[f"{n}-{dt.name}-{lay}" for n, dt, lay in ROWS_3D])
def test_first_order_3d_sum_that_decides_is_the_oracles(oracle, monkeypatch, name, dt, layout):
    """3-D first-order solves, node and cell grids, in every layout of the fields and of the term arrays"""
    _decided_by_the_reference_sum(oracle, sc.BY_NAME[name], dt, layout, monkeypatch)


ROWS_OTHER = [(c["name"], dt) for c in sc.CASES if c["name"] not in sc.FIRST_ORDER_3D for dt in c["dtypes"]]


@pytest.mark.parametrize("name,dt", ROWS_OTHER, ids=[f"{n}-{dt.name}" for n, dt in ROWS_OTHER])
def test_2d_and_weno_sum_that_decides_is_the_oracles(oracle, monkeypatch, name, dt):
    """2-D first-order solves and the WENO stage (3-D node grid, 2-D cell grid): real absolute values, a snapshot before the first
    WENO iteration"""
    monkeypatch.delenv("TTCR_FSM_PAIR", raising=False)
    monkeypatch.delenv("TTCR_FSM_RS_FIELDS", raising=False)
    c = sc.BY_NAME[name]
    ks = sc.targets(oracle, c, dt)
    assert ks
    for k in ks:
        eps, thr, o2 = sc.aim(oracle, c, dt, k)
        thr = float(thr)
        for v in (0, 1):
            out, st, kern = _solve(c, dt, 1, eps, {"stopping_shortcuts": v})
            tag = (name, dt.name, "k", k, "shortcuts", v)
            r = out[0]
            print(tag, kern, st, "eps", eps, "thr", thr, "device", r["ref"], "oracle", o2["change"], o2["changew"])
            assert st["reference_sums_missed"] == 0 and st["reference_sums"] > 0, (tag, st)
            assert (r["niter"], r["niterw"]) == (o2["niter"], o2["niterw"]), (tag, r["niter"], r["niterw"], o2["niter"], o2["niterw"])
            assert np.array_equal(r["tt"], o2["tt"]), tag
            whole = _check_history(r["ref"][0], o2["change"], thr, tag + ("first-order",))
            whole += _check_history(r["ref"][1], o2["changew"], thr, tag + ("weno",))
            assert whole >= 1, (tag, whole)
            got, want = r["ref"][1 if c["weno"] else 0], sc.history(c, o2)
            assert got.size == k + 1 and not np.isnan(got[k]), (tag, got, want)
            assert got[k] == float(want[k]) and dt.type(got[k]) == want[k] and got[k] < thr, (tag, got, want, thr)


def test_brick_passes_above_the_always_snapshot_size_odd_shape(monkeypatch):
    """(257, 259, 253) nodes: 16 840 439, above 2^24, odd, no edge a multiple of 16 -- snapshots on prediction only, one element per
    lane in the pair layout's term pass, partial bricks on every far face.  The oracle is too slow here: the default path against the
    one-chain sum over whole strided fields with whole-field snapshots (stopping_rule = 2, stopping_shortcuts = 0)."""
    import ttcr_amd

    nn, n_src, eps, dx = (257, 259, 253), 2, 1e-5, 0.25
    N = nn[0] * nn[1] * nn[2]
    assert N > 1 << 24 and N % 2 == 1 and all(v % 16 for v in nn)
    thr = float(np.float32(eps) * np.float32(N))
    b = np.random.default_rng(24).uniform(0.25, 1.0, tuple((v + 7) // 8 for v in nn))
    s = np.repeat(np.repeat(np.repeat(b, 8, 0), 8, 1), 8, 2)[:nn[0], :nn[1], :nn[2]].copy()
    src = np.array([[0.31, 0.47, 0.23], [0.72, 0.28, 0.66]]) * (np.array(nn) - 1) * dx
    monkeypatch.setenv("TTCR_FSM_PAIR", "1")
    monkeypatch.delenv("TTCR_FSM_RS_FIELDS", raising=False)

    def solve(opts):
        g = ttcr_amd.Grid3d(*[np.arange(v) * dx for v in nn], n_threads=n_src, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, eps=eps,
                            dtype=np.float32)
        g.set_slowness(s)
        for k, v in opts.items():
            g.set_option(k, v)
        g.raytrace(src, np.zeros((n_src, 3)))
        return [(g.get_niter(i), g.get_reference_changes(i)[0], g.get_grid_traveltimes(i)) for i in range(n_src)], g.stopping_stats(), g.last_kernel()

    a, st_a, kern = solve({"skip": 1, "stopping_shortcuts": 1})
    b_, st_b, _ = solve({"skip": 1, "stopping_rule": 2, "stopping_shortcuts": 0})
    d, st_d, _ = solve({"skip": 1})
    print(kern, st_a, st_b, st_d, [q[0] for q in a], [q[1] for q in a], [q[1] for q in b_])
    assert kern.split(",")[7] == "2" and kern.split(",")[5] == "true", kern
    assert [q[0] for q in d] == [q[0] for q in b_] and all(np.array_equal(d[i][2], b_[i][2]) for i in range(n_src))
    assert st_a["reference_sums"] == st_b["reference_sums"] > 0 and st_a["reference_sums_missed"] == st_b["reference_sums_missed"] == 0
    for i in range(n_src):
        assert a[i][0] == b_[i][0] and np.array_equal(a[i][2], b_[i][2])
        ga, gb = a[i][1], b_[i][1]
        m = ~np.isnan(gb)
        assert np.array_equal(m, ~np.isnan(ga)), (i, ga, gb)
        whole = m & (gb < thr)
        assert np.array_equal(ga[whole], gb[whole]) and np.all(ga[m & ~whole] >= thr), (i, ga, gb, thr)


# ---------------------------------------------------------------------------------------------------------------------------- B
HEAD, WMIN, TILE = 4096, 65536, 4096      # FSM_REFSUM_HEAD, FSM_REFSUM_WMIN, FSM_REFSUM_TILE (fsm_kernels.h)
# exact node counts of 2-D grids: the head +- 1, the head plus the first window +- 1, seven window doublings
SIZES = {4095: (63, 65), 4096: (64, 64), 4097: (17, 241), 69631: (179, 389), 69632: (256, 272), 69633: (27, 2579), 4198397: (2051, 2047)}


def _seq(x):
    """the reference's sum: one chain of additions in the array's dtype, in order"""
    with np.errstate(over="ignore"):
        return np.add.accumulate(np.ascontiguousarray(x))[-1]


def _same(a, b):
    return (np.isinf(a) and np.isinf(b)) or a == b


def _contents(dt, N, rng):
    """(name, old, base) with terms abs(old - base) in dt: the kinds of test_parallel_form_of_the_sequential_sum, then the edges"""
    P = 24 if dt == np.float32 else 53
    tiny = np.finfo(dt).smallest_subnormal
    big = np.finfo(dt).max
    base = rng.uniform(1.0, 2.0, N).astype(dt)
    zero = np.zeros(N, dtype=dt)
    u, w, e = rng.uniform(0, 1, N), rng.uniform(0, 1, N), rng.integers(-40, 3, N)   # (drawn once: the kinds below share them)
    small = u * 1e-3

    def on_base(d):
        return (base + d.astype(dt)).astype(dt), base

    def exact(d):                                  # the terms themselves (field 0: nothing is rounded away)
        return np.ascontiguousarray(d, dtype=dt), zero

    yield ("uniform", *on_base(small))
    yield ("sparse", *on_base(u * (w < 0.01)))
    yield ("powers of two", *on_base(2.0 ** e.astype(np.float64)))
    yield ("half ulps", *on_base((e & 3) * 2.0 ** (-24 if dt == np.float32 else -53) + (w < 1e-4) * 1.0))
    yield ("many binades", *on_base(-np.log1p(-u) * 10.0 ** ((e + 40) % 15 - 12).astype(np.float64)))
    yield ("constant", *on_base(np.full(N, 2.0 ** -20)))
    yield ("all zero", base.copy(), base)
    d = np.zeros(N); d[-1] = 0.37
    yield ("one term, last node", *on_base(d))
    d = small.copy(); d[:HEAD] = 0
    yield ("empty head", *on_base(d))
    d[min(HEAD, N - 1) + 1:] = 0; d[min(HEAD, N - 1)] = 0.37e-3
    yield ("empty head, one term behind it", *on_base(d))
    yield ("subnormal terms, subnormal sum", *exact((e & 1).astype(dt) * tiny))
    yield ("subnormal terms, sum reaches the normal range", *exact(np.floor(w * 2.0 ** (P - 1)).astype(dt) * tiny))
    for name, first in (("inside the head", 100), ("beyond the head", HEAD + (N - HEAD) // 3)):
        if first + 300 >= N:
            continue
        old, _ = on_base(small)
        old[first:first + 300] = big               # (nodes still at max(): the sum reaches infinity, as in every first iteration)
        yield ("max() " + name, old, base)
    # a constant background and one term equal to the running sum: the sum leaves its binade exactly there
    bg = dt(2.0 ** (-20 if dt == np.float32 else -40))
    t = 2
    spots = [TILE * t - 1, TILE * t, TILE * t + 1, TILE * t + 16 * 37 - 1, TILE * t + 16 * 37, TILE * t + 16 * 37 + 1, HEAD + WMIN - 1, HEAD + WMIN,
             HEAD - 1, HEAD, N - 1]
    if N > 1 << 20:                                # (a far tile, where the window has doubled several times; the seams near the head are
        t = 700                                    # the smaller sizes' business)
        spots = [TILE * t - 1, TILE * t, TILE * t + 1, TILE * t + 16 * 37 - 1, TILE * t + 16 * 37, TILE * t + 16 * 37 + 1, HEAD + WMIN, N - 1]
    d = np.full(N, bg, dtype=dt)
    for p in sorted(set(q for q in spots if 0 < q < N)):
        d[p] = dt(p) * bg                          # (p bg is exact: p < 2^24)
        yield ("crossing at %d" % p, *exact(d))
        d[p] = bg
    # one term of 2^(P+2) units of the running sum in the middle, then terms far below a unit of the new sum
    d = small.copy()
    mid = N // 2
    s_mid = float(_seq(d[:mid].astype(dt)))
    d[mid] = s_mid * 2.0 ** (P + 2)
    d[mid + 1:] = d[mid] * 2.0 ** -(P + 40) * (0.5 + 0.5 * w[mid + 1:])
    yield ("one term beyond the cap, then terms below 2^-32 units", *exact(d))


@pytest.mark.parametrize("N", list(SIZES))
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_reference_change_is_numpys_sequential_sum(dt, N):
    import ttcr_amd

    nx, nz = SIZES[N]
    assert nx * nz == N
    g = ttcr_amd.Grid2d(np.arange(nx) * 0.5, np.arange(nz) * 0.5, n_threads=1, cell_slowness=0, method="FSM", weno=0, dtype=dt)
    assert g.get_number_of_nodes() == N
    rng = np.random.default_rng(N % 1000 + (0 if dt == np.float32 else 1))
    seen = []
    for name, old, base in _contents(dt, N, rng):
        terms = np.abs(old - base)
        assert terms.dtype == dt and not np.isnan(terms).any()
        want = _seq(terms)
        a = g.reference_change(old, base, parallel=True)
        b = g.reference_change(old, base, parallel=False)
        print(N, np.dtype(dt).name, name, "numpy", want, "parallel", a, "one chain", b)
        assert a.dtype == dt and _same(a, want) and _same(b, want), (N, name, want, a, b)
        seen.append((name, want))
    sums = dict(seen)
    tiny_normal = np.finfo(dt).smallest_normal
    assert sums["all zero"] == 0 and 0 < sums["subnormal terms, subnormal sum"] < tiny_normal
    assert tiny_normal <= sums["subnormal terms, sum reaches the normal range"] < 1e-20
    assert np.isinf(sums["max() inside the head"]) and (N < HEAD + 1000 or np.isinf(sums["max() beyond the head"]))
    print(np.dtype(dt).name, N, g.stopping_stats())


def test_reference_change_with_the_largest_window():
    """FSM_REFSUM_WMAX: one large first term, then 6.7e7 terms that leave the sum in its binade -- quarter units (add nothing), ties
    (half a unit: to even) and three quarters (one unit).  Every partial sum lies in [1, 2) (the sum only grows and ends there), so no
    round meets a binade crossing and each one doubles the window: 2^16 ... 2^24 cover 4096 + 2^25 - 2^16 terms, the next window is the
    clamped one of 2^25, and terms are left for one more round behind it.  The window is not visible from outside (stopping_stats counts
    rounds in bunches of 16 and 8): that the clamp is reached follows from these sizes, asserted below, not from a measurement."""
    import ttcr_amd

    dt = np.float32
    n = 8200
    N = n * n
    WMAX = 1 << 25                                # FSM_REFSUM_WMAX
    assert WMIN * 2 ** 9 == WMAX and N > HEAD + (WMAX - WMIN) + WMAX
    g = ttcr_amd.Grid2d(np.arange(n) * 0.5, np.arange(n) * 0.5, n_threads=1, cell_slowness=0, method="FSM", weno=0, dtype=dt)
    rng = np.random.default_rng(5)
    u = rng.integers(0, 40, N, dtype=np.uint8)
    d = np.full(N, 2.0 ** -25, dtype=dt)         # a quarter of the unit of sums in [1, 2): 2^-23
    d[u == 0] = dt(2.0 ** -24)                    # half a unit
    d[u == 1] = dt(3 * 2.0 ** -25)                # three quarters
    d[0] = 1.0
    zero = np.zeros(N, dtype=dt)
    want = _seq(d)
    assert 1.0 < want < 2.0
    st0 = g.stopping_stats()["rounds"]
    a = g.reference_change(d, zero, parallel=True)
    rounds = g.stopping_stats()["rounds"] - st0
    b = g.reference_change(d, zero, parallel=False)
    print("largest window: numpy", want, "parallel", a, "one chain", b, "rounds", rounds)
    assert a == want and b == want
