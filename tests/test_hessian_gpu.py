"""The second-order products of the field tape on the device (FieldTape.hold / release / hvp / newton, DESIGN.md 6f, and the double
backward of ttcr_amd.autograd.raytrace_adjoint).  hvp and newton are bit-equal to the numpy restatement (tests/hessian_reference.py) run
on the device's own fields, under both schedules, in fp32 and fp64, on one-event grids, on the tile-edge shapes, on fields with decisive
ties and on a translated origin; the bits do not depend on slots or device lists; hold returns vjp's gradient, newton is the composition
it is defined as, a new hold replaces the cotangent, release returns the memory; the cell tape is the node tape between A and A^T; the
fp64 hvp is the derivative of the device's own vjp (finite differences, the bound of tests/test_hessian.py); torch's double backward
through raytrace_adjoint is the full second derivative, and raises through raytrace_events."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import adjoint_reference as AR  # noqa: E402
import field_tape_cases as FC  # noqa: E402
import hessian_reference as HR  # noqa: E402
from field_tape_cases import DX, ZERO, _bits_equal  # noqa: E402

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
SCHEDULES = ("tiled", "jacobi")


def _in_child(fn, *args):
    """Run _torch_<fn>(*args) of this module in a fresh process that initialises torch's device before the first grid"""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_hessian_gpu as t; t._torch_%s(*%r)"
            % (HERE, ROOT, fn, args))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout[-2000:])


def _grid(case, dt, **kw):
    import ttcr_amd

    axes = [case.origin[a] + np.arange(case.nn[a]) * case.dx for a in range(3)]
    g = ttcr_amd.Grid3d(*axes, cell_slowness=0, method="FSM", dtype=dt, weno=0, tt_from_rp=0, **kw)
    g.set_slowness(case.s.reshape(case.nn, order="F"))
    return g


def _tape(case, dt, **kw):
    src, rcv, agg, rows = FC.call_arrays(case, np.random.default_rng(61))
    g = _grid(case, dt, **kw)
    tt, tape = g.raytrace_adjoint(src, rcv, aggregate_src=agg)
    fields = [tape.field(e) for e in range(tape.n_events)]
    return tape, rcv, rows, fields


def _inputs(case, dt, rcv):
    """the held cotangent (w per receiver row, fc per event and node), the direction v and the row weights rw"""
    rng = np.random.default_rng(67)
    n_nodes = int(np.prod(case.nn))
    w = rng.standard_normal(rcv.shape[0]).astype(dt)
    fc = rng.standard_normal((len(case.events), n_nodes)).astype(dt)
    v = (case.s * rng.standard_normal(n_nodes)).astype(dt)
    rw = rng.uniform(0.5, 2.0, rcv.shape[0]).astype(dt)
    return w, fc, v, rw


def _reference(case, dt, fields, rcv, rows, w, fc, v, rw):
    """(hvp, newton) of the restatement on given fields; w, rw in rcv order (w or fc may be None)"""
    kw = dict(rcvs=[rcv[r] for r in rows], ws=None if w is None else [w[r] for r in rows], field_cot=fc)
    args = (fields, np.asarray(case.s, dtype=dt), case.dx, case.nn, case.origin, [e["pts"] for e in case.events], v)
    return HR.hvp(*args, **kw), HR.newton(*args, row_weights=[rw[r] for r in rows], **kw)


def _check_products(case, dt, label, **kw):
    """restatement == tiled == Jacobi, to the bit, for hvp and newton with the cotangent (w, fc) held"""
    tape, rcv, rows, fields = _tape(case, dt, **kw)
    w, fc, v, rw = _inputs(case, dt, rcv)
    ref_h, ref_n = _reference(case, dt, fields, rcv, rows, w, fc, v, rw)
    assert all(np.all(np.isfinite(a)) and np.any(a != 0) for a in (ref_h, ref_n)) and not np.array_equal(ref_h, ref_n)
    tape.hold(w, fc)
    for schedule in SCHEDULES:
        hv = tape.hvp(v, schedule=schedule)
        assert isinstance(tape.passes, tuple) and len(tape.passes) == 2 and min(tape.passes) >= 1
        assert hv.dtype == dt and hv.shape == (tape.n_cols,)
        _bits_equal(hv, ref_h)
        _bits_equal(tape.newton(v, rw, schedule=schedule), ref_n)
    print("%s, %s: %d events; |H v| = %.3e, |newton| = %.3e" % (label, np.dtype(dt).name, tape.n_events, np.linalg.norm(ref_h),
                                                               np.linalg.norm(ref_n)))
    return tape, rcv, rows, fields


# ---- 1. bit equality with the restatement
ONE_NN = (13, 11, 17)
ONE_SOURCES = {   # node-index units
    "off_node": [[4.6, 3.2, 7.4]],
    "on_node": [[5, 4, 9]],
    "two_points": [[4.6, 3.2, 7.4], [5.2, 3.4, 6.8]],
}


def one_event_case(source, kind):
    rng = np.random.default_rng(29)
    return FC.Case("%s-%s" % (source, kind), ONE_NN, DX, ZERO, FC.model(ONE_NN, DX, ZERO, kind),
                   [FC._event(FC.at(ONE_NN, DX, ZERO, ONE_SOURCES[source]), FC.receivers(ONE_NN, DX, ZERO, rng))])


@DTYPES
@pytest.mark.parametrize("kind", ["smooth", "rough"])
@pytest.mark.parametrize("source", sorted(ONE_SOURCES))
def test_bits_one_event(source, kind, dt):
    _check_products(one_event_case(source, kind), dt, "one event " + source + " " + kind)


EDGE_SHAPES = [(7, 9, 13), (8, 10, 14), (9, 11, 15), (17, 21, 29), (2, 3, 57), (40, 2, 3)]
assert set(EDGE_SHAPES) <= set(FC.SHAPES)


@DTYPES
@pytest.mark.parametrize("nn", EDGE_SHAPES, ids=lambda nn: "x".join(map(str, nn)))
def test_bits_on_the_tile_edge_shapes(nn, dt):
    case = FC.shape_case(nn)
    assert len(case.events) == 2
    _check_products(case, dt, "shape " + case.name)


@DTYPES
@pytest.mark.parametrize("name", FC.DECISIVE_TIES)
def test_bits_on_fields_with_decisive_ties(name, dt):
    case = FC.tie_case(name)
    tape, rcv, rows, fields = _check_products(case, dt, "ties " + name)
    decisive, total = FC.count_ties(fields[0], case.nn)
    assert decisive > 0, (decisive, total)   # (without them the case has lost its point)


@DTYPES
def test_bits_on_a_translated_origin(dt):
    _check_products(FC.origin_case("translated-off_node"), dt, "origin translated-off_node")


# ---- 2. schedule and device independence
def four_event_case():
    nn = (17, 13, 15)
    rng = np.random.default_rng(53)
    hi = np.array(nn) - 1.0
    return FC.Case("four", nn, DX, ZERO, FC.model(nn, DX, ZERO, "rough"),
                   [FC._event(FC.at(nn, DX, ZERO, [rng.uniform(1.5, hi - 1.5)]), FC.random_receivers(nn, DX, ZERO, rng, 5),
                              round(float(rng.uniform(0, 0.5)), 3)) for _ in range(4)])


@DTYPES
def test_bits_do_not_depend_on_slots_or_device_lists(dt):
    case = four_event_case()
    first = None
    for kw in (dict(n_threads=1), dict(n_threads=4), dict(n_threads=4, device=[0]), dict(n_threads=4, device=[0, 0])):
        tape, rcv, rows, fields = _tape(case, dt, **kw)
        assert tape.n_events == 4
        w, fc, v, rw = _inputs(case, dt, rcv)
        tape.hold(w, fc)
        got = [tape.hvp(v), tape.hvp(v, schedule="jacobi"), tape.newton(v, rw), tape.newton(v, rw, schedule="jacobi")]
        _bits_equal(got[0], got[1])
        _bits_equal(got[2], got[3])
        if first is None:   # (the restatement is run once: every configuration holds the same fields, to the bit)
            first = (fields,) + _reference(case, dt, fields, rcv, rows, w, fc, v, rw)
        for a, b in zip(fields, first[0]):
            _bits_equal(a, b)
        _bits_equal(got[0], first[1])
        _bits_equal(got[2], first[2])


# ---- 3. the held cotangent
@DTYPES
def test_held_cotangent_behaviour(dt):
    case = one_event_case("two_points", "rough")
    tape, rcv, rows, fields = _tape(case, dt)
    w, fc, v, rw = _inputs(case, dt, rcv)
    elem = np.dtype(dt).itemsize
    dtt = tape.jvp(v)                       # (the first jvp allocates its lists: taken before the byte counts below)
    before = tape.nbytes
    for call in (lambda: tape.hvp(v), lambda: tape.newton(v, rw)):
        with pytest.raises(ValueError, match="hold"):
            call()
    # hold returns vjp's gradient, with and without a field cotangent, and adds lam and the work array
    for ww, ff in ((w, None), (None, fc), (w, fc)):
        for schedule in SCHEDULES:
            _bits_equal(tape.hold(ww, ff, return_grad=True, schedule=schedule), tape.vjp(ww, ff, schedule=schedule))
    assert tape.hold(w) is None
    assert tape.nbytes == before + 2 * tape.n_events * tape.n_nodes * elem, (before, tape.nbytes)
    # newton(v, W) == vjp(W . jvp(v), field_cotangent=q) with r added at the nodes that are not frozen (one event: the sums over the
    # events have one term); q and r from the restatement on the device's field
    s = np.asarray(case.s, dtype=dt)
    fr = AR.frozen_nodes(dt, case.nn, case.dx, case.origin, case.events[0]["pts"])
    _, lam, q, r, _ = HR.product_event(fields[0], s, case.dx, case.nn, case.origin, fr, rcv, w, None, v)
    fz = np.zeros(s.size, dtype=bool)
    fz[list(fr)] = True
    assert (rw * dtt).dtype == dt and np.any(q != 0) and np.any(r != 0)
    for schedule in SCHEDULES:
        comp = tape.vjp(rw * dtt, q[None, :], schedule=schedule)
        comp[~fz] = (comp[~fz] + r[~fz]).astype(dt)
        _bits_equal(tape.newton(v, rw, schedule=schedule), comp)
        comp = tape.vjp(None, q[None, :], schedule=schedule)
        comp[~fz] = (comp[~fz] + r[~fz]).astype(dt)
        _bits_equal(tape.hvp(v, schedule=schedule), comp)
    # another cotangent: the products follow it
    h1 = tape.hvp(v)
    w2 = np.random.default_rng(71).standard_normal(rcv.shape[0]).astype(dt)
    tape.hold(w2)
    assert tape.nbytes == before + 2 * tape.n_events * tape.n_nodes * elem
    ref_h2, ref_n2 = _reference(case, dt, fields, rcv, rows, w2, None, v, rw)
    h2 = tape.hvp(v)
    _bits_equal(h2, ref_h2)
    _bits_equal(tape.newton(v, rw), ref_n2)
    assert not np.array_equal(h1, h2)
    # a jvp or a vjp in between does not disturb the held cotangent
    tape.vjp(w)
    tape.jvp(v)
    tape.gauss_newton(v, rw)
    _bits_equal(tape.hvp(v), ref_h2)
    # release returns the memory; the products raise again; a new hold works
    tape.release()
    assert tape.nbytes == before
    tape.release()
    with pytest.raises(ValueError, match="hold"):
        tape.hvp(v)
    tape.hold(w2)
    _bits_equal(tape.hvp(v), ref_h2)
    with pytest.raises(ValueError):
        tape.hvp(np.ones(3))
    with pytest.raises(ValueError):
        tape.newton(v, np.ones(3))
    with pytest.raises(ValueError):
        tape.hvp(v, schedule="fastest")
    with pytest.raises(ValueError):
        tape.hold()
    tape.free()
    with pytest.raises(ValueError):
        tape.hvp(v)


# ---- 4. cell tapes
@DTYPES
def test_cell_tape_is_the_node_tape_between_a_and_a_transposed(dt):
    from test_cell_tape_gpu import Pair, cell_model, shape_events

    nn = (9, 11, 15)
    p = Pair(shape_events(nn), dt, cell_model(nn, "rough"), oracle_fields=False)
    v = p.ds
    p.cell.hold(p.w, p.fc)
    p.node.hold(p.w, p.fc)
    for schedule in SCHEDULES:
        hv = p.cell.hvp(v, schedule=schedule)
        assert hv.shape == (p.n_cells,) and hv.dtype == dt and np.any(hv != 0)
        _bits_equal(hv, p.At(p.node.hvp(p.A(v), schedule=schedule)))
        _bits_equal(p.cell.newton(v, p.rw, schedule=schedule), p.At(p.node.newton(p.A(v), p.rw, schedule=schedule)))
        _bits_equal(p.cell.newton(v, schedule=schedule), p.At(p.node.newton(p.A(v), schedule=schedule)))
    _bits_equal(p.cell.hold(p.w, p.fc, return_grad=True), p.cell.vjp(p.w, p.fc))


# ---- 5. fp64: the device hvp against finite differences of the device's own vjp, fresh grids at s +- h v
@pytest.mark.parametrize("loss", ["receivers", "field"])
@pytest.mark.parametrize("case", ["off_node", "on_node", "rough", "two_points"])
def test_fp64_hvp_against_finite_differences_of_the_device_vjp(case, loss):
    import test_hessian as TH

    src, kind = TH.CASES[case]
    src = np.array(src)
    s = TH.model(kind)
    rng = np.random.default_rng(5)
    rcv = rng.uniform(0.6, (TH.N - 1) * TH.DX - 0.6, (30, 3))
    w = rng.standard_normal(30)
    gfield = rng.standard_normal((1, TH.N ** 3))
    v = s * rng.standard_normal(s.size)
    cot = (w, None) if loss == "receivers" else (None, gfield)
    h = TH.STEPS[1]

    def tape_at(sl):
        c = FC.Case(case, TH.NN3, TH.DX, TH.MN, sl, None)
        return _grid(c, np.float64, eps=1e-15, maxit=200).raytrace_adjoint(src, rcv, aggregate_src=True)[1]

    t0 = tape_at(s)
    t0.hold(*cot)
    hv = t0.hvp(v)
    fd = (tape_at(s + h * v).vjp(*cot) - tape_at(s - h * v).vjp(*cot)) / (2 * h)
    err = np.linalg.norm(hv - fd) / np.linalg.norm(fd)
    print("device H v vs finite differences of the device vjp, %s, %s loss, step %.0e: %.2e (bound %.1e)" % (case, loss, h, err, TH.FD_TOL))
    assert err <= TH.FD_TOL, err


# ---- 6. torch: double backward (child processes)
def _torch_double_backward(wrt, return_fields):
    import torch

    import ttcr_amd
    import ttcr_amd.autograd as ag

    rng = np.random.default_rng(83)
    dt = np.float64
    nn = (9, 11, 13)
    mm = tuple(n - 1 for n in nn) if wrt == "cells" else nn
    axes = [np.arange(n) * DX for n in nn]
    g = ttcr_amd.Grid3d(*axes, cell_slowness=1 if wrt == "cells" else 0, method="FSM", dtype=dt, weno=0, tt_from_rp=0)
    v = rng.uniform(1.0, 2.0, mm)
    x = v * rng.standard_normal(mm)
    hi = (np.array(nn) - 1) * DX
    ev_src = rng.uniform(1.5 * DX, hi - 1.5 * DX, (2, 3))
    ids = np.array([0, 1, 1, 0, 0, 1, 0])
    src = np.column_stack([ids, np.array([0.0, 0.125])[ids], ev_src[ids]])
    rcv = rng.uniform(0.7 * DX, hi - 0.7 * DX, (ids.size, 3))
    t_obs = torch.from_numpy(rng.uniform(1.0, 4.0, ids.size)).cuda()
    f_obs = torch.from_numpy(rng.uniform(1.0, 4.0, (2,) + nn)).cuda()
    xt = torch.from_numpy(x).cuda()

    def loss(vel):
        out = ag.raytrace_adjoint(g, vel, src, rcv, return_fields=return_fields, wrt=wrt)
        if not return_fields:
            return 0.5 * ((out - t_obs) ** 2).sum()
        return 0.5 * ((out[0] - t_obs) ** 2).sum() + 0.5 * ((out[1] - f_obs) ** 2).sum()

    vel = torch.from_numpy(v).cuda().requires_grad_(True)
    (grad,) = torch.autograd.grad(loss(vel), vel, create_graph=True)
    assert grad.requires_grad
    (hx,) = torch.autograd.grad((grad * xt).sum(), vel)
    hx = hx.cpu().numpy()
    # the composition through the tape: model order x fastest <-> (mx, my, mz) in C order is Fortran flattening
    g.set_velocity(v)
    tt, tape = g.raytrace_adjoint(src, rcv, wrt=wrt)
    res = tt - t_obs.cpu().numpy()
    resf = None
    if return_fields:
        fld = np.stack([tape.field(e) for e in range(2)])
        resf = fld - np.stack([f.flatten("F") for f in f_obs.cpu().numpy()])
    vm, xm = v.flatten("F"), x.flatten("F")
    ds = -(xm / (vm * vm))
    h = tape.hold(res, resf, return_grad=True)
    _bits_equal(h, tape.vjp(res, resf))
    _bits_equal(grad.detach().cpu().numpy().flatten("F"), -h / (vm * vm))            # the first derivative, as before
    dtt, df = tape.jvp(ds, return_fields=True)
    part_a = -tape.vjp(dtt, df if return_fields else None) / (vm * vm)               # through the cotangent: Gauss-Newton
    part_b = -tape.hvp(ds) / (vm * vm)                                               # through the model: the second-order term
    part_c = 2 * h * xm / (vm * vm * vm)                                             # the factor -1 / v^2
    want = (part_a + (part_b + part_c)).reshape(mm, order="F")
    f8 = np.linalg.norm
    e_comp = f8(hx - want) / f8(want)
    # torch.autograd.functional.hvp of the same loss (a forward of its own)
    _, hx2 = torch.autograd.functional.hvp(loss, torch.from_numpy(v).cuda(), xt)
    e_func = f8(hx2.cpu().numpy() - want) / f8(want)
    print("double backward, wrt=%s, return_fields=%s: against the composition %.2e, functional.hvp against it %.2e (bound 1e-12); "
          "parts |A| %.3e |B| %.3e |C| %.3e" % (wrt, return_fields, e_comp, e_func, f8(part_a), f8(part_b), f8(part_c)))
    # the same kernels on the same inputs, three fp64 terms added in another order at most: a few ulp of the largest term
    assert e_comp <= 1e-12 and e_func <= 1e-12, (e_comp, e_func)
    assert f8(part_b) > 1e-3 * f8(want) and f8(part_a) > 1e-3 * f8(want)             # (neither term is negligible here)
    # a third derivative raises
    vel3 = torch.from_numpy(v).cuda().requires_grad_(True)
    (g1,) = torch.autograd.grad(loss(vel3), vel3, create_graph=True)
    (g2,) = torch.autograd.grad((g1 * xt).sum(), vel3, create_graph=True)
    _bits_equal(g2.detach().cpu().numpy(), hx)
    try:
        torch.autograd.grad((g2 * xt).sum(), vel3)
    except RuntimeError as e:
        assert "third derivatives are not implemented" in str(e), e
    else:
        raise AssertionError("a third derivative did not raise")


def _torch_refusals():
    import torch

    import ttcr_amd
    import ttcr_amd.autograd as ag

    rng = np.random.default_rng(89)
    nn = (9, 11, 13)
    axes = [np.arange(n) * DX for n in nn]
    g = ttcr_amd.Grid3d(*axes, cell_slowness=0, method="FSM", dtype=np.float64, weno=0, tt_from_rp=0)
    hi = (np.array(nn) - 1) * DX
    rcv = rng.uniform(0.7 * DX, hi - 0.7 * DX, (5, 3))
    eor = np.array([0, 1, 1, 0, 1])
    x = torch.from_numpy(rng.standard_normal(nn)).cuda()
    ev = np.column_stack([[0.0, 0.1], rng.uniform(1.5 * DX, hi - 1.5 * DX, (2, 3))])   # (t0, x, y, z) of two events
    for name in ("events", "m_tape"):
        vel = torch.from_numpy(rng.uniform(1.0, 2.0, nn)).cuda().requires_grad_(True)
        if name == "events":
            tt = ag.raytrace_events(g, vel, torch.from_numpy(ev).cuda().requires_grad_(True), eor, rcv)
        else:
            tt = ag.raytrace(g, vel, np.column_stack([eor, ev[eor]]), rcv)
        (g1,) = torch.autograd.grad(0.5 * (tt ** 2).sum(), vel, create_graph=True)   # the first derivative still works
        assert torch.isfinite(g1).all() and bool((g1 != 0).any())
        assert g1.requires_grad
        # once_differentiable cuts g1 off from vel behind a node that raises when the engine reaches it (backward()); asked for the
        # gradient with respect to vel alone, torch.autograd.grad finds vel unreachable and raises before that.  Neither returns a part.
        try:
            (g1 * x).sum().backward()
        except RuntimeError as e:
            assert "once_differentiable" in str(e), e
        else:
            raise AssertionError("a second derivative through %s did not raise" % name)
        (g1,) = torch.autograd.grad(0.5 * (tt ** 2).sum(), vel, create_graph=True)
        try:
            torch.autograd.grad((g1 * x).sum(), vel)
        except RuntimeError:
            pass
        else:
            raise AssertionError("torch.autograd.grad of a second derivative through %s did not raise" % name)


@pytest.mark.parametrize("return_fields", [False, True], ids=["tt", "tt and fields"])
@pytest.mark.parametrize("wrt", ["nodes", "cells"])
def test_torch_double_backward_is_the_full_second_derivative(wrt, return_fields):
    _in_child("double_backward", wrt, return_fields)


def test_torch_second_derivative_through_events_and_the_m_tape_raises():
    _in_child("refusals")
