"""The field tape's definition on the input classes of tests/field_tape_cases.py, without a device: on the oracle's fp64 and fp32 fields the
frozen-node rule and the receiver stencil of tests/adjoint_reference.py reproduce what the oracle computes, the tangent and the adjoint
restatements are transposes of each other to rounding, and -- where the map is differentiable: translated origins, metric units, dense
receivers, small non-cubic grids -- both are the derivative of the oracle by central finite differences.  The tie classes get no finite
differences (the map has a kink there); they assert that their fields do have ties.  tests/test_field_tape_edges_gpu.py compares the
device with the same restatements on the same inputs, bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_reference as AR  # noqa: E402
import field_tape_cases as FC  # noqa: E402
from field_tape_cases import DOT_TOL, STEP, TOL  # noqa: E402

SMALL_SHAPES = [(2, 2, 2), (3, 40, 2), (2, 3, 57), (7, 9, 13), (9, 11, 15), (40, 2, 3)]
CASES = dict([("ties-" + n, lambda n=n: FC.tie_case(n)) for n in sorted(FC.TIES)] +
             [("origin-" + n, lambda n=n: FC.origin_case(n)) for n in FC.ORIGIN_CASES] +
             [("shared-one_event", lambda: FC.shared_case("one_event"))] +
             [("shape-" + "x".join(map(str, nn)), lambda nn=nn: FC.shape_case(nn)) for nn in SMALL_SHAPES])
# the map is differentiable at these (generic sources, smooth or noisy models); (2, 2, 2) is one cell whose 8 nodes are all frozen
FD_CASES = [n for n in CASES if n.startswith(("origin-", "shared-"))] + ["shape-3x40x2", "shape-7x9x13", "shape-9x11x15"]


def test_shape_table_meets_every_tile_edge():
    """every tile edge of the two tiled kernels (fp32 and fp64) meets tile - 1, tile, tile + 1, 2 tile and 2 tile + 1 on some axis of
    some grid, and every axis is the single shortest one of some grid"""
    extents = {n for nn in FC.SHAPES for n in nn}
    for edge in sorted(set(FC.ADJ_EDGE.values()) | set(FC.TAN_EDGE.values())):
        assert {edge - 1, edge, edge + 1, 2 * edge, 2 * edge + 1} <= extents, edge
    assert {nn.index(min(nn)) for nn in FC.SHAPES if sorted(nn)[0] < sorted(nn)[1]} == {0, 1, 2}


def _solve(case, dt, s, e):
    """the oracle's field and receiver traveltimes of event e, origin time 0, run to the end of its changes"""
    from oracle import oracle as O

    ev = case.events[e]
    o = O.solve3d(dt, tuple(n - 1 for n in case.nn), case.dx, case.origin, np.asarray(s, dtype=dt), ev["pts"].astype(dt),
                  rcv=ev["rcv"].astype(dt), eps=1e-15, maxit=400)
    assert o["niter"] < 400, o["change"][-3:]
    return o


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_definition_on_the_oracle_fields(name, dt):
    case = CASES[name]()
    dtype = np.dtype(dt)
    rng = np.random.default_rng(7)
    s = case.s.astype(dt)
    ds = (case.s * rng.standard_normal(s.size)).astype(dt)
    for e, ev in enumerate(case.events):
        o = _solve(case, dt, s, e)
        T = o["tt"]
        # the frozen-node rule reproduces the oracle's frozen values, exactly
        frozen = AR.frozen_nodes(dt, case.nn, case.dx, case.origin, ev["pts"])
        for m, d in frozen.items():
            assert T[m] == dtype.type(dtype.type(d) * s[m]), (m, T[m], d, s[m])
        # the stencil reproduces the interpolated traveltimes (an 8-term sum re-associated)
        worst = 0.0
        for r, p in enumerate(ev["rcv"]):
            nodes, wts = AR.stencil(dt, case.nn, case.dx, case.origin, p)
            v = sum(np.float64(wt) * np.float64(T[m]) for m, wt in zip(nodes, wts))
            sp = np.spacing(dtype.type(o["tt_rcv"][r]))
            assert abs(v - np.float64(o["tt_rcv"][r])) <= 16 * sp, (r, p, v, o["tt_rcv"][r])
            worst = max(worst, abs(v - np.float64(o["tt_rcv"][r])) / sp)
        # <w, J v> = <J^T w, v>
        one = FC.Case(case.name, case.nn, case.dx, case.origin, case.s, [ev])
        rows = [np.arange(ev["rcv"].shape[0])]
        w = FC.wide_weights(rng, ev["rcv"].shape[0], dt)
        fc = rng.standard_normal((1, s.size)).astype(dt)
        dtt, mu = FC.reference_jvp([T], one, dt, ev["rcv"], rows, ds)
        g_rcv = FC.reference_vjp([T], one, dt, ev["rcv"], rows, w, None)
        g_fld = FC.reference_vjp([T], one, dt, ev["rcv"], rows, None, fc)
        assert np.all(np.isfinite(mu)) and np.all(np.isfinite(g_rcv)) and np.all(np.isfinite(g_fld))
        e_rcv, e_fld = FC.dot_errors(w, dtt, g_rcv, fc, mu, g_fld, ds)
        ties = FC.count_ties(T, case.nn)
        print("%s, %s, event %d: %d frozen nodes exact, stencil within %.1f ulp, <w, J v> against <J^T w, v>: receivers %.2e, field %.2e "
              "(bound %.0e); ties %d decisive of %d" % (name, dtype.name, e, len(frozen), worst, e_rcv, e_fld, DOT_TOL[dtype], ties[0], ties[1]))
        assert e_rcv <= DOT_TOL[dtype] and e_fld <= DOT_TOL[dtype], (e_rcv, e_fld)
        if name.startswith("ties-"):
            assert ties[1] > 0, ties   # (without ties the case has lost its point)
            assert ties[0] > 0 or case.name not in FC.DECISIVE_TIES, ties


@pytest.mark.parametrize("name", FD_CASES)
def test_fp64_restatements_against_oracle_finite_differences(name):
    case = CASES[name]()
    dt = np.float64
    rng = np.random.default_rng(9)
    ds = case.s * rng.standard_normal(case.s.size)
    for e, ev in enumerate(case.events):
        one = FC.Case(case.name, case.nn, case.dx, case.origin, case.s, [ev])
        rows = [np.arange(ev["rcv"].shape[0])]
        w = FC.wide_weights(rng, ev["rcv"].shape[0], dt)
        fc = rng.standard_normal((1, case.s.size))
        o = _solve(case, dt, case.s, e)
        op, om = _solve(case, dt, case.s + STEP * ds, e), _solve(case, dt, case.s - STEP * ds, e)
        fd_fld = (op["tt"] - om["tt"]) / (2 * STEP)
        fd_rcv = (op["tt_rcv"] - om["tt_rcv"]) / (2 * STEP)
        dtt, mu = FC.reference_jvp([o["tt"]], one, dt, ev["rcv"], rows, ds)
        j_fld = np.linalg.norm(mu[0] - fd_fld) / np.linalg.norm(fd_fld)
        j_rcv = np.linalg.norm(dtt - fd_rcv) / np.linalg.norm(fd_rcv)
        g_rcv = FC.reference_vjp([o["tt"]], one, dt, ev["rcv"], rows, w, None)
        g_fld = FC.reference_vjp([o["tt"]], one, dt, ev["rcv"], rows, None, fc)
        v_rcv = abs(g_rcv @ ds - w @ fd_rcv) / abs(w @ fd_rcv)
        v_fld = abs(g_fld @ ds - fc[0] @ fd_fld) / abs(fc[0] @ fd_fld)
        print("%s, event %d, against oracle finite differences: jvp field %.2e, receivers %.2e; vjp receivers %.2e, field %.2e (bound %.0e)"
              % (name, e, j_fld, j_rcv, v_rcv, v_fld, TOL))
        assert max(j_fld, j_rcv, v_rcv, v_fld) <= TOL, (j_fld, j_rcv, v_rcv, v_fld)
