"""What tests/test_long_axis_gpu.py relies on, checked on the CPU so that it cannot silently stop holding (tests/long_axis_cases.py).  These
are conditions on the inputs, not on the kernels; the partition and chunk grid are restated from the docstring of
tests/test_chunk_dirty_marks.py, nothing is taken from the library:
  * direction dn has bits (F, J, K) = (dn & 1, dn >> 1 & 1, dn >> 2 & 1): an axis with its bit set is walked from its last index down;
  * unit (TJ, TK) owns the oriented columns j' in [TJ PJ, TJ PJ + PJ), k' in [TK PK, TK PK + PK);
  * its chunks start at lcf + ci C with lcf = Ls - ((Ls - (TJ + TK)) mod C), Ls = TJ PJ + TK PK; node (i', j', k') sits at level i' + j' + k';
  * an F brick holds 16 nodes; bit b of word b >> 5.
Every grid reaches chunk and brick indices beyond the first word in every direction, the iterating models still change nodes after the first
iteration on both sides of brick 32 (so the high words carry news when the low ones do), the frozen boxes of the two on-node sources
straddle chunk 32, and the limit shapes sit on either side of 32 x 32 F bricks."""
import numpy as np
import pytest

import few_workgroups_cases as fw
import long_axis_cases as la
import weno_2d_cases as wc

PATCH = {(3, "float32"): (16, 16), (3, "float64"): (16, 8), (2, "float32"): (64, 1), (2, "float64"): (64, 1)}
# chunk lengths the GPU tests run on each case: first-order 3-D pairs and fp64 8, one field 16; the WENO stage 4, 8 and 16; 2-D 16;
# two slots at the limit: 8 or 16
CHUNKS = {la.LONG["name"]: (8, 16), la.LONGER["name"]: (8,), la.LONG_WENO["name"]: (4, 8, 16), la.LONG_2D[0]["name"]: (16,),
          la.LONG_2D[1]["name"]: (16,), la.LIMIT[0]["name"]: (8, 16), la.LIMIT[1]["name"]: (8, 16)}
ids = lambda c: c["name"]


def fjk(c):
    """(NF, NJ, NK) of a case"""
    return c["n"] if c["dim"] == 3 else (c["n"][1], c["n"][0], 1)


def chunk_of_last_plane(c, dtype, chunk, dn):
    """(TJ, TK, ci) of the unit and chunk of sweep dn that evaluates each node of the natural plane the sweep reaches last, arrays [k][j]"""
    NF, NJ, NK = fjk(c)
    PJ, PK = PATCH[(c["dim"], np.dtype(dtype).name)]
    k, j = np.meshgrid(np.arange(NK), np.arange(NJ), indexing="ij")
    i = np.full_like(j, 0 if dn & 1 else NF - 1)
    i2 = NF - 1 - i if dn & 1 else i
    j2 = NJ - 1 - j if (dn >> 1) & 1 else j
    k2 = NK - 1 - k if (dn >> 2) & 1 else k
    TJ, TK = j2 // PJ, k2 // PK
    Ls = TJ * PJ + TK * PK
    lcf = Ls - (Ls - (TJ + TK)) % chunk
    return TJ, TK, (i2 + j2 + k2 - lcf) // chunk


@pytest.mark.parametrize("c", la.CASES, ids=ids)
def test_chunk_and_brick_indices_pass_the_first_word(c):
    NF = fjk(c)[0]
    nbf = (NF + la.BRICK - 1) // la.BRICK
    assert nbf > 32, (c["name"], nbf)
    want = 256 if c is la.LONGER else 34
    for dt in la.DTYPES:
        for chunk in CHUNKS[c["name"]]:
            for dn in range(8 if c["dim"] == 3 else 4):
                _, _, ci = chunk_of_last_plane(c, dt, chunk, dn)
                assert ci.max() >= want, (c["name"], dt, chunk, dn, ci.max())
                # the host sizes a unit's dirty bits for chunks of 8 or more: ((NF + 2 (PJ + PK)) / 8 + 4) / 32 + 1 words hold every index
                PJ, PK = PATCH[(c["dim"], np.dtype(dt).name)]
                if chunk >= 8:
                    assert ci.max() < 32 * (((NF + 2 * (PJ + PK)) // 8 + 4) // 32 + 1)
    if c is la.LONGER:
        assert (NF - 1) // 8 >> 5 == 8 and (nbf - 1) >> 5 == 4      # dirty-bit word 8, slab word 4
    if c is la.LONG_WENO:
        assert (NF - 1) // 4 >> 5 == 4


def test_the_limit():
    """skip_now (ttcr_amd/csrc/fsm_capi.hip): exact skipping needs nbf <= 32 FSM_SLAB_WORDS = 1024 F bricks, NF <= 16384; there the top
    bit of the top word of the slab mask and of the stamped bricks is live, and 65 words of dirty bits are in use"""
    nbf = [(c["n"][0] + la.BRICK - 1) // la.BRICK for c in la.LIMIT]
    assert nbf == [1024, 1025]
    assert (nbf[0] - 1) >> 5 == 31 and (nbf[0] - 1) & 31 == 31 and (nbf[1] - 1) >> 5 == 32
    for dt in la.DTYPES:
        PJ, PK = PATCH[(3, np.dtype(dt).name)]
        assert ((la.LIMIT[0]["n"][0] + 2 * (PJ + PK)) // 8 + 4) // 32 + 1 <= 65 <= 68


def test_patches():
    p = lambda c, dt: wc.patches(c, dt)
    f32, f64 = np.float32, np.float64
    assert p(la.LONG, f32) == [(3, 3), (2, 3)] and p(la.LONG, f64) == [(3, 3), (3, 3)]
    assert p(la.LONG_WENO, f32) == [(2, 2), (1, 9)] and p(la.LONG_WENO, f64) == [(2, 2), (2, 1)]
    assert p(la.LONGER, f32) == [(2, 1), (1, 9)] and p(la.LONGER, f64) == [(2, 1), (2, 1)]
    assert p(la.LONG_2D[0], f32) == [(3, 2)] and p(la.LONG_2D[1], f32) == [(2, 2)]
    assert [int(np.prod(c["n"])) for c in (la.LONG, la.LONGER)] == [399000, 321300]
    assert max(int(np.prod(c["n"])) for c in la.CASES) < 1e6


ITER_ROWS = [(c, w) for c in la.CASES for w in ((True,) if c is la.LONG_WENO else (False,))]


@pytest.mark.parametrize("dt", la.DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("c,weno", ITER_ROWS, ids=[c["name"] for c, _ in ITER_ROWS])
def test_the_iterating_model_changes_nodes_late_on_both_sides_of_brick_32(oracle, c, weno, dt):
    model = la.ITERATING[c["name"]]
    ax = la.f_axis(c)
    other = tuple(a for a in range(c["dim"]) if a != ax)
    for k in range(la.n_src(c)):
        o = la.reference(oracle, c, model, dt, k, weno=weno)
        tag = (c["name"], model, np.dtype(dt).name, "source", k, o["niter"], o["niterw"])
        assert 3 <= o["niter"] < la.maxit(c, model), tag
        if weno:
            assert 2 <= o["niterw"] < la.maxit(c, model), tag
        first = la.reference(oracle, c, model, dt, k, weno=False, maxit_=1)
        assert first["niter"] == 1
        late = np.any(la.field(c, o["tt"]) != la.field(c, first["tt"]), axis=other)        # per F index
        bricks = np.unique(np.nonzero(late)[0] // la.BRICK)
        assert bricks.size and bricks.min() < 32 and bricks.max() >= 32, (tag, bricks)


@pytest.mark.parametrize("dt", la.DTYPES, ids=["fp32", "fp64"])
def test_long_block16_changes_nodes_late_over_the_whole_f_range(oracle, dt):
    late = np.zeros(la.LONG["n"][0], dtype=bool)
    for k in range(la.n_src(la.LONG)):
        o = la.reference(oracle, la.LONG, "block16", dt, k)
        first = la.reference(oracle, la.LONG, "block16", dt, k, maxit_=1)
        late |= np.any(la.field(la.LONG, o["tt"]) != la.field(la.LONG, first["tt"]), axis=(1, 2))
    assert late[0] and late[-1] and late.mean() > 0.95, np.nonzero(~late)[0]


@pytest.mark.parametrize("c", [la.LONG, la.LONGER], ids=ids)
@pytest.mark.parametrize("dt", la.DTYPES, ids=["fp32", "fp64"])
def test_frozen_boxes_of_the_on_node_sources_straddle_chunk_32(oracle, c, dt):
    """unit (0, 0) of direction 0: the first sweep of a solve seeds its dirty bits from the F range of the frozen box widened by one
    (levels b0 - 1 + j0 + k0 .. b1 + 1 + jmax + kmax of the unit); the box is the oracle's: the nodes it has set before the first sweep"""
    NF, NJ, NK = c["n"]
    PJ, PK = PATCH[(3, np.dtype(dt).name)]
    jmax, kmax = min(PJ, NJ) - 1, min(PK, NK) - 1
    src = la.sources(c)
    for node, chunk in zip(la.ON_NODES, (8, 16)):
        k = int(np.nonzero(np.all(src == np.array(node) * la.DX, axis=1))[0][0])
        init = la.reference(oracle, c, "gradient", dt, k, maxit_=0)
        assert init["niter"] == 0
        set_ = np.nonzero(la.field(c, init["tt"]) < np.finfo(dt).max)
        lo, hi = [int(a.min()) for a in set_], [int(a.max()) for a in set_]
        assert (lo, hi) == ([v - 1 for v in node], [v + 1 for v in node])          # on a node: one node either side
        assert hi[1] <= jmax and hi[2] <= kmax                                        # inside unit (0, 0)
        ca, cb = (lo[0] - 1) // chunk, (hi[0] + 1 + jmax + kmax) // chunk              # lcf = 0
        assert ca < 32 <= cb, (node, chunk, ca, cb)
    # ... and on chunks of 8 the second one straddles the seam of words 1 and 2 (chunk 63 | 64)
    assert (505 - 1) // 8 == 63 and (507 + 1 + jmax + kmax) // 8 >= 64


def test_inputs():
    import test_chunk_dirty_gpu as cd

    assert la.OFF == cd.OFF and la.DX == cd.DX == fw.DX
    for dt in la.DTYPES:
        for m in ("block16", "gradient"):
            assert np.array_equal(la.slowness(la.LONG, m, dt), cd.slowness(la.LONG["n"], m, dt))
        b = la.slowness(la.LONGER, "block64", dt)
        assert np.all(b[:64, :16, :] == b[0, 0, 0]) and len(np.unique(b)) == 33 * 2 and 0.25 <= b.min() and b.max() < 1.0
        b = la.slowness(la.LIMIT[1], "block256", dt)
        assert np.all(b[16128:16384, :16, :] == b[16128, 0, 0]) and len(np.unique(b)) == 65 * 2
        b = la.slowness(la.LONG_2D[0], "block16", dt)
        assert b.shape == (130, 600) and np.all(b[:16, :16] == b[0, 0]) and len(np.unique(b)) == 9 * 38
    for c in la.CASES:
        hi = np.array([(m - 1) * la.DX for m in c["n"]])
        src, rcv = la.sources(c), la.receivers(c)
        assert src.shape == (la.n_src(c), c["dim"]) and np.all(src > 0) and np.all(src < hi)
        assert np.all(rcv >= 0) and np.all(rcv <= hi) and len(rcv) >= 5
        if c["dim"] == 3:
            assert np.array_equal(rcv, fw.receivers(c["n"]))
    assert la.n_src(la.LONG) == la.n_src(la.LONGER) == 6 and la.n_src(la.LONG_WENO) == 4 == wc.N_SRC and la.n_src(la.LIMIT[0]) == 3
    # six sources: a batch of four and one of two with four slots, two batches of three with the one-field kernel's three slots
    assert [len(r) for r in fw.held(list(range(6)), 4)[1]] == [4, 2] and [len(r) for r in fw.held(list(range(6)), 3)[1]] == [3, 3]
