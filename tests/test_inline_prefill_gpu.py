"""The spare traveltime fields re-initialised from inside the first sweep launch of a call (option "prefill_inline",
ttcr_amd/csrc/fsm_kernels.h: fsm_sweep_unit at ticket draw; GridT::solve_batch), on the device (-m gpu).
Replaces the same reference code as the fill it stands in for -- `reinit` of every node, ttcr/Grid3Drnfs.h:92-94, Node3Dn.h:103-105.

A grid with options prefill = 1, prefill_inline = 1 makes three back-to-back calls that restart every slot.  The first fills in place and
leaves the spare set to the side stream; from the second on the call swaps the sets and its first whole-iteration launch stores max() into
the set it swapped out -- the RESULTS of the call before -- slice by slice, one slice per ticket (tests/test_prefill_slices.py: the
slices tile the set).  The sources of consecutive calls lie in opposite corners of the grid: a node of the spare set that kept its old,
finite time holds, two calls later, a value below the true time of the new source wherever the old source was nearer; the sweeps only
ever lower a value, so it stays, and the field differs from the oracle's.

Bar, after every call and for every slot: field, iteration count(s), receiver times and the reference's own change sums equal to the CPU
oracle bit for bit; the fp64 change sums (atomic adds, order not fixed) equal in count to the oracle's iterations and within rtol 1e-6 --
the bar of tests/test_few_workgroups_gpu.py -- of the same grid with prefill_inline = 0, whose results are held to the same oracle.
ttcr_fsm_prefill_swaps counts one swap per call from the second call on.

Shapes: those of tests/few_workgroups_cases.py -- (37, 35, 41), (70, 17, 9) and (2, 16, 10) (one fp32 patch: 8 tickets per slot) -- in fp32
and fp64 with 3 slots (odd: padded to 4 fields in the pair layout) and 4, one field per workgroup and pairs; one resident workgroup
(TTCR_FSM_WGS = 1: every ticket, hence every slice, by one workgroup in turn); maxit = 1 (the fill is complete after the only launch); a
2-D grid and a weno = 1 grid (one workgroup per unit); a grid in the layout window whose layout changes between the calls.
"""
import numpy as np
import pytest

import few_workgroups_cases as fw

pytestmark = pytest.mark.gpu

ENV_KEYS = ("TTCR_FSM_WGS", "TTCR_FSM_PAIR", "TTCR_FSM_PAIR_UNITS", "TTCR_FSM_MODE", "TTCR_FSM_SKIP", "TTCR_FSM_PREFILL", "TTCR_FSM_ARITH")
# per call and slot: where the source lies, as a fraction of the extent -- consecutive calls in opposite corners
CORNERS = [(0.08, 0.11, 0.07), (0.93, 0.9, 0.94), (0.06, 0.92, 0.09)]
SPREAD = [(0.0, 0.0, 0.0), (0.03, -0.02, 0.02), (-0.02, 0.03, -0.03), (0.02, 0.02, 0.04)]


def sources(extent, call, n):
    """(n, dim) source points of a call"""
    dim = len(extent)
    f = np.array([np.clip(np.array(CORNERS[call][:dim]) + np.array(SPREAD[q][:dim]), 0.02, 0.98) for q in range(n)])
    return f * np.array(extent)


_REFS = {}


def reference(oracle, key, solve):
    """oracle solve, computed once per key and shared: do not modify"""
    if key not in _REFS:
        _REFS[key] = solve()
    return _REFS[key]


def _clean_env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _check_calls(oracle, grids, n_slots, n_calls, srcs_of, rcv, solve_one, field_of, weno=False, opts_between=None):
    """grids[0]: prefill_inline = 1, grids[1]: prefill_inline = 0.  Every call restarts every slot."""
    for call in range(n_calls):
        srcs = srcs_of(call)
        refs = [solve_one(call, q, srcs[q:q + 1]) for q in range(n_slots)]
        source, rc = np.repeat(srcs, len(rcv), axis=0), np.tile(rcv, (n_slots, 1))
        changes = []
        for gi, g in enumerate(grids):
            if opts_between:
                for k, v in opts_between(call).items():
                    g.set_option(k, v)
            tt = g.raytrace(source, rc).reshape(n_slots, -1)
            changes.append([])
            for q in range(n_slots):
                w = "prefill_inline %d call %d slot %d [%s]" % (1 - gi, call, q, g.last_kernel())
                np.testing.assert_array_equal(tt[q], refs[q]["tt_rcv"], err_msg=w)
                np.testing.assert_array_equal(field_of(g, q), refs[q]["tt"], err_msg=w)
                assert g.get_niter(q) == refs[q]["niter"], w
                if weno:
                    assert g.get_niterw(q) == refs[q]["niterw"], w
                for stage, name in ((0, "change"), (1, "changew")) if weno else ((0, "change"),):
                    rch = g.get_reference_changes(q)[stage]
                    m = ~np.isnan(rch)
                    np.testing.assert_array_equal(rch[m], refs[q][name].astype(np.float64)[m], err_msg=w)
                ch = g.get_changes(q)
                assert ch[0].size == refs[q]["niter"], w
                changes[-1].append(np.concatenate(ch))
        for q in range(n_slots):
            np.testing.assert_allclose(changes[0][q], changes[1][q], rtol=1e-6, err_msg="call %d slot %d" % (call, q))
    assert grids[0].prefill_swaps() == n_calls - 1 and grids[1].prefill_swaps() == n_calls - 1
    # (the first launch of every call but the first carried the fill -- and none of the other grid's)
    assert grids[0].prefill_inline_fills() == n_calls - 1 and grids[1].prefill_inline_fills() == 0


def _grids3d(shape, dt, n_slots, weno=0, maxit=50, opts=None):
    import ttcr_amd

    out = []
    for inline in (1, 0):
        g = ttcr_amd.Grid3d(*fw.axes(shape), n_threads=n_slots, cell_slowness=0, method="FSM", tt_from_rp=0, weno=weno, maxit=maxit, dtype=dt)
        for k, v in dict({"prefill": 1, "prefill_inline": inline}, **(opts or {})).items():
            g.set_option(k, v)
        g.set_slowness(fw.slowness(shape, dt))
        out.append(g)
    return out


def _run3d(oracle, shape, dt, n_slots, weno=0, maxit=50, opts=None, opts_between=None, n_calls=3):
    ext = [(m - 1) * fw.DX for m in shape]
    rcv = fw.receivers(shape)
    s = fw.slowness(shape, dt).flatten("F")

    def solve_one(call, q, p):
        key = (tuple(shape), np.dtype(dt).name, weno, maxit, call, q)
        return reference(oracle, key, lambda: oracle.solve3d(dt, tuple(m - 1 for m in shape), fw.DX, (0.0, 0.0, 0.0), s, p, rcv=rcv,
                                                             weno=bool(weno), maxit=maxit))

    _check_calls(oracle, _grids3d(shape, dt, n_slots, weno, maxit, opts), n_slots, n_calls, lambda call: sources(ext, call, n_slots), rcv,
                 solve_one, lambda g, q: g.get_grid_traveltimes(q).flatten("F"), weno=bool(weno), opts_between=opts_between)


SHAPES = [fw.SHAPES[0], fw.SHAPES[2], fw.SHAPES[3]]


@pytest.mark.parametrize("pair", [0, 1], ids=["one-field", "pairs"])
@pytest.mark.parametrize("n_slots", [3, 4])
@pytest.mark.parametrize("dt", fw.DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_three_calls_with_far_apart_sources(oracle, monkeypatch, shape, dt, n_slots, pair):
    _clean_env(monkeypatch, {"TTCR_FSM_PAIR": str(pair)})
    _run3d(oracle, shape, dt, n_slots)


@pytest.mark.parametrize("pair", [0, 1], ids=["one-field", "pairs"])
@pytest.mark.parametrize("dt", fw.DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_one_resident_workgroup(oracle, monkeypatch, shape, dt, pair):
    """every ticket of the launch drawn by the same workgroup, one after the other: 3 slots"""
    _clean_env(monkeypatch, {"TTCR_FSM_PAIR": str(pair), "TTCR_FSM_WGS": "1"})
    _run3d(oracle, shape, dt, 3)


@pytest.mark.parametrize("pair", [0, 1], ids=["one-field", "pairs"])
@pytest.mark.parametrize("dt", fw.DTYPES, ids=["fp32", "fp64"])
def test_one_iteration_per_call(oracle, monkeypatch, dt, pair):
    """maxit = 1: the only launch of the call carries the whole fill"""
    _clean_env(monkeypatch, {"TTCR_FSM_PAIR": str(pair)})
    _run3d(oracle, fw.SHAPES[0], dt, 3, maxit=1)


@pytest.mark.parametrize("dt", fw.DTYPES, ids=["fp32", "fp64"])
def test_layout_changes_between_calls(oracle, monkeypatch, dt):
    """3 slots x 9 (fp64: 18) patches with the pairing threshold at 24 (window: up to 60): a grid that may change its layout, padded to 4
    fields; pairs in calls 0 and 1, one field per workgroup in call 2 -- the armed launch fills the whole set whatever the layout"""
    _clean_env(monkeypatch, {"TTCR_FSM_PAIR_UNITS": "24"})
    _run3d(oracle, fw.SHAPES[0], dt, 3, opts={"pair_layout": 1}, opts_between=lambda call: {"pair_layout": 0 if call == 2 else 1})


@pytest.mark.parametrize("dt", fw.DTYPES, ids=["fp32", "fp64"])
def test_weno_grid(oracle, monkeypatch, dt):
    """weno = 1: the first launch is the first-order stage's; one workgroup per unit in the WENO stage"""
    _clean_env(monkeypatch, {})
    _run3d(oracle, (21, 21, 21), dt, 3, weno=1)


@pytest.mark.parametrize("dt", fw.DTYPES, ids=["fp32", "fp64"])
def test_2d_grid(oracle, monkeypatch, dt):
    """2-D: one workgroup per unit, one-wave patches of 64 columns (two along x, the second with 6)"""
    import ttcr_amd

    _clean_env(monkeypatch, {})
    nx, nz, dx, S = 70, 45, 0.5, 3
    x, z = np.arange(nx) * dx, np.arange(nz) * dx
    s = np.ascontiguousarray(np.random.default_rng(2).uniform(0.3, 1.0, (nx, nz)), dtype=dt)
    rcv = np.array([[0.0, 0.0], [3.0, 2.0], [20.0, 11.0], [x[-1], z[-1]], [x[-1], 0.0]])
    grids = []
    for inline in (1, 0):
        g = ttcr_amd.Grid2d(x, z, n_threads=S, cell_slowness=0, method="FSM", weno=0, dtype=dt)
        g.set_option("prefill", 1)
        g.set_option("prefill_inline", inline)
        g.set_slowness(s)
        grids.append(g)

    def solve_one(call, q, p):
        return reference(oracle, ("2d", np.dtype(dt).name, call, q), lambda: oracle.solve2d(dt, (nx - 1, nz - 1), dx, dx, (0, 0), s.ravel(), p, rcv=rcv))

    _check_calls(oracle, grids, S, 3, lambda call: sources([x[-1], z[-1]], call, S), rcv, solve_one, lambda g, q: g.get_grid_traveltimes(q).ravel())


def test_call_that_restarts_some_slots(oracle, monkeypatch):
    """calls 0, 1, 3: every slot (the swap, the fill inside the launch); call 2: one source in a named slot -- filled in place, the other
    slots keep their fields, the spare set filled during call 1 stays as it is and call 3 takes it"""
    import ttcr_amd

    _clean_env(monkeypatch, {})
    shape, dt, S = fw.SHAPES[0], np.float32, 3
    ext = [(m - 1) * fw.DX for m in shape]
    rcv = fw.receivers(shape)
    s = fw.slowness(shape, dt).flatten("F")
    g = _grids3d(shape, dt, S)[0]

    def solve(p):
        return oracle.solve3d(dt, tuple(m - 1 for m in shape), fw.DX, (0.0, 0.0, 0.0), s, p, rcv=rcv)

    held = [None] * S
    for call in range(4):
        srcs = sources(ext, call % 3, S)
        if call == 2:
            srcs = srcs[1:2]
            tt = g.raytrace(np.repeat(srcs, len(rcv), axis=0), rcv, thread_no=1).reshape(1, -1)
            held[1] = solve(srcs)
            np.testing.assert_array_equal(tt[0], held[1]["tt_rcv"])
        else:
            tt = g.raytrace(np.repeat(srcs, len(rcv), axis=0), np.tile(rcv, (S, 1))).reshape(S, -1)
            for q in range(S):
                held[q] = solve(srcs[q:q + 1])
                np.testing.assert_array_equal(tt[q], held[q]["tt_rcv"], err_msg="call %d slot %d" % (call, q))
        for q in range(S):
            w = "call %d slot %d" % (call, q)
            np.testing.assert_array_equal(g.get_grid_traveltimes(q).flatten("F"), held[q]["tt"], err_msg=w)
            assert g.get_niter(q) == held[q]["niter"], w
    assert g.prefill_swaps() == 2 and g.prefill_inline_fills() == 2   # (swaps: calls 1 and 3; fills inside the launch: the same two)
