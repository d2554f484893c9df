"""The field tape's derivatives with respect to the source points on the device (FieldTape.jvp_source, FieldTape.source_jacobian,
FieldTape.vjp(..., return_source_grad=True), ttcr_amd.autograd.raytrace_events): bit-equal to the numpy restatement of the definition
(tests/source_reference.py) run on the device's own fields, whatever the schedule (tiled or global Jacobi), the number of columns of a
call, n_threads or the grid shape; the slowness gradient of such a vjp has the bits of the plain vjp; forward and reverse are transposes
of each other to rounding; the torch operator returns these values in its layouts and its fp64 derivative is the central difference of
its own forward."""
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
import source_reference as SR  # noqa: E402
from field_tape_cases import DOT_TOL, STEP, TOL, _bits_equal  # noqa: E402

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
SCHEDULES = ("tiled", "jacobi")


def _in_child(fn, *args):
    """Run _torch_<fn>(*args) of this module in a fresh process that initialises torch's device before the first grid (as
    tests/test_tangent_gpu.py does)."""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_source_derivative_gpu as t; t._torch_%s(*%r)"
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


class Run:
    """one raytrace_adjoint call for the events of a case, with the device's fields and the inputs of the checks"""

    def __init__(self, case, dt, **kw):
        self.case, self.dt = case, dt
        self.src, self.rcv, agg, self.rows = FC.call_arrays(case, np.random.default_rng(61))
        self.grid = _grid(case, dt, **kw)
        self.tt, self.tape = self.grid.raytrace_adjoint(self.src, self.rcv, aggregate_src=agg)
        self.sources = [e["pts"] for e in case.events]
        self.n_points = sum(p.shape[0] for p in self.sources)
        assert self.tape.n_points == self.n_points and self.tape.n_events == len(case.events)
        assert np.array_equal(self.tape.point_event, np.concatenate([np.full(p.shape[0], e) for e, p in enumerate(self.sources)]))
        self.fields = [self.tape.field(e) for e in range(self.tape.n_events)]
        rng = np.random.default_rng(71)
        n_nodes = int(np.prod(case.nn))
        self.dsrc = rng.standard_normal((4, self.n_points, 4)).astype(dt)
        self.w = rng.standard_normal(self.rcv.shape[0]).astype(dt)
        self.fc = rng.standard_normal((len(case.events), n_nodes)).astype(dt)
        self.s = np.asarray(case.s, dtype=dt)

    def ref_jvp(self, dsrc):
        """the restatement: (dtt in rcv order, (n_events, n_nodes) field tangents)"""
        c = self.case
        mus, dtts = SR.source_tangent(self.fields, self.s, c.dx, c.nn, c.origin, self.sources, dsrc, rcvs=[self.rcv[r] for r in self.rows])
        dtt = np.zeros(self.rcv.shape[0], dtype=self.dt)
        for r, d in zip(self.rows, dtts):
            dtt[r] = d
        return dtt, np.stack(mus)

    def ref_vjp(self, w, fc):
        c = self.case
        return SR.source_adjoint(self.fields, self.s, c.dx, c.nn, c.origin, self.sources, rcvs=[self.rcv[r] for r in self.rows],
                                 ws=None if w is None else [w[r] for r in self.rows], field_cot=fc)


def _check_against_the_restatement(run, kinds=("receivers", "field", "both")):
    """jvp_source with its fields and vjp with the source gradient: restatement == tiled == Jacobi, to the bit; the slowness gradient of
    that vjp == the plain vjp's"""
    tape = run.tape
    ref_dtt, ref_mu = run.ref_jvp(run.dsrc[0])
    assert np.all(np.isfinite(ref_mu)) and np.any(ref_mu != 0) and np.any(ref_dtt != 0)
    for schedule in SCHEDULES:
        dtt, mu = tape.jvp_source(run.dsrc[0], return_fields=True, schedule=schedule)
        assert tape.passes >= 1 and mu.shape == (tape.n_events, tape.n_cols) and dtt.dtype == run.dt
        _bits_equal(dtt, ref_dtt)
        _bits_equal(mu, ref_mu)
        _bits_equal(tape.jvp_source(run.dsrc[0], schedule=schedule), ref_dtt)
    for kind in kinds:
        w, fc = {"receivers": (run.w, None), "field": (None, run.fc), "both": (run.w, run.fc)}[kind]
        ref_grad, ref_gsrc = run.ref_vjp(w, fc)
        assert ref_gsrc.shape == (run.n_points, 4) and np.all(np.isfinite(ref_gsrc)) and np.any(ref_gsrc != 0)
        for schedule in SCHEDULES:
            grad, gsrc = tape.vjp(w, fc, schedule=schedule, return_source_grad=True)
            assert tape.passes >= 1
            _bits_equal(gsrc, ref_gsrc)
            _bits_equal(grad, ref_grad)
            _bits_equal(grad, tape.vjp(w, fc, schedule=schedule))
    return ref_dtt, ref_mu


def _dot_error(run):
    """relative |<w, J_src v> + <fc, mu> - <gsrc, v>| on the device with the moduli of the inputs, in float64 arithmetic"""
    wp, fcp, dsp = np.abs(run.w), np.abs(run.fc), np.abs(run.dsrc[0])
    dtt, mu = run.tape.jvp_source(dsp, return_fields=True)
    grad, gsrc = run.tape.vjp(wp, fcp, return_source_grad=True)
    f8 = lambda a: np.asarray(a, dtype=np.float64).ravel()   # noqa: E731
    lhs, rhs = f8(wp) @ f8(dtt) + f8(fcp) @ f8(mu), f8(gsrc) @ f8(dsp)
    return abs(lhs - rhs) / abs(rhs)


# ---- the five cases of tests/test_source_derivative.py on their 21^3 grid
N = 21
NN3 = (N, N, N)
CASES = {
    "off_node": ([[3.3, 4.1, 5.7]], "smooth"),
    "two_points": ([[3.3, 4.1, 5.7], [3.6, 4.2, 5.4]], "smooth"),
    "rough": ([[6.2, 2.9, 4.4]], "rough"),
    "near_face": ([[3.02, 4.1, 5.7]], "smooth"),
    "on_node": ([[4.0, 5.5, 3.0]], "smooth"),
}


def _case21(name):
    src, kind = CASES[name]
    rng = np.random.default_rng(5)
    rcv = rng.uniform(0.6, (N - 1) * FC.DX - 0.6, (30, 3))
    return FC.Case(name, NN3, FC.DX, FC.ZERO, FC.model(NN3, FC.DX, FC.ZERO, kind), [FC._event(src, rcv, 0.125)])


@DTYPES
@pytest.mark.parametrize("name", list(CASES))
def test_bits_of_the_five_cases_and_the_device_identity(name, dt):
    run = Run(_case21(name), dt)
    _check_against_the_restatement(run)
    err = _dot_error(run)
    bound = DOT_TOL[np.dtype(dt)]
    print("device <w, J_src v> against <J_src^T w, v>, %s, %s: %.2e (bound %.0e)" % (name, np.dtype(dt).name, err, bound))
    assert err <= bound, err


# ---- grid shapes: 2 x 2 x 2, and on every axis an extent of the forward tile + 1 (11 in fp32, 9 in fp64); two events each, the second
# source in the last cell of the far corner (FC.shape_case)
SHAPES = [(2, 2, 2), (9, 11, 15), (11, 3, 9), (3, 9, 11)]
assert SHAPES[0] in FC.SHAPES and SHAPES[1] in FC.SHAPES
assert all(any(nn[a] == FC.TAN_EDGE[np.dtype(d)] + 1 for nn in SHAPES) for a in range(3) for d in (np.float32, np.float64))


@DTYPES
@pytest.mark.parametrize("nn", SHAPES, ids=lambda nn: "x".join(map(str, nn)))
def test_shapes_against_the_tile_edge(nn, dt):
    case = FC.shape_case(nn)
    assert len(case.events) == 2 and all(case.events[1]["pts"][0, a] > (nn[a] - 2) * case.dx for a in range(3))
    _check_against_the_restatement(Run(case, dt), kinds=("both",))


@DTYPES
def test_translated_origin(dt):
    _check_against_the_restatement(Run(FC.origin_case("translated-off_node"), dt), kinds=("both",))


# ---- K columns at once
def _five_events():
    c = FC.slots_case()
    return FC.Case("five", c.nn, c.dx, c.origin, c.s, c.events[:5])


@DTYPES
def test_four_columns_have_the_bits_of_four_calls(dt):
    run = Run(_five_events(), dt, n_threads=4)
    tape = run.tape
    before = tape.nbytes
    one = [tape.jvp_source(run.dsrc[k], return_fields=True) for k in range(4)]
    grown = tape.nbytes
    assert grown > before
    _bits_equal(one[0][0], run.ref_jvp(run.dsrc[0])[0])
    for schedule in SCHEDULES:
        for K in (4, 3, 2, 1):
            dtt, mu = tape.jvp_source(run.dsrc[:K], return_fields=True, schedule=schedule)
            assert dtt.shape == (K, run.rcv.shape[0]) and mu.shape == (K, tape.n_events, tape.n_cols) and tape.passes >= 1
            for k in range(K):
                _bits_equal(dtt[k], one[k][0])
                _bits_equal(mu[k], one[k][1])
            _bits_equal(tape.jvp_source(run.dsrc[:K], schedule=schedule), dtt)
    # the four-column work arrays: one per schedule, 4 n_events n_nodes elements each, reported from the first call that needs them
    assert tape.nbytes - grown == 2 * 4 * tape.n_events * tape.n_cols * np.dtype(dt).itemsize, (grown, tape.nbytes)
    for bad in (np.zeros((5, run.n_points, 4)), np.zeros((run.n_points, 3)), np.zeros((run.n_points + 1, 4)), np.zeros(4)):
        with pytest.raises(ValueError):
            tape.jvp_source(bad.astype(dt))
    with pytest.raises(ValueError):
        tape.jvp_source(run.dsrc[0], schedule="fastest")


@DTYPES
def test_source_jacobian(dt):
    run = Run(_five_events(), dt, n_threads=4)
    tape, case = run.tape, run.case
    for schedule in SCHEDULES:
        J = tape.source_jacobian(schedule=schedule)
        assert J.shape == (run.rcv.shape[0], 4) and J.dtype == dt
        for k in range(4):
            unit = np.zeros((run.n_points, 4), dtype=dt)
            unit[:, k] = 1
            _bits_equal(J[:, k], tape.jvp_source(unit, schedule=schedule))
    # d tt / d t0: every node moves with t0, so a row is the sum of its stencil weights, taken in stencil order from +0
    sums = np.zeros(run.rcv.shape[0], dtype=dt)
    for r, p in enumerate(run.rcv):
        acc = dt(0)
        for wt in AR.stencil(dt, case.nn, case.dx, case.origin, p)[1]:
            acc = dt(acc + dt(wt * dt(1)))
        sums[r] = acc
    _bits_equal(J[:, 0], sums)
    assert np.all(np.abs(J[:, 0] - 1) < 1e-5) and np.any(J[:, 1:] != 0)
    two = Run(_case21("two_points"), dt)
    with pytest.raises(ValueError, match="jvp_source"):
        two.tape.source_jacobian()


@DTYPES
def test_five_events_on_one_slot_and_on_four(dt):
    a, b = Run(_five_events(), dt, n_threads=1), Run(_five_events(), dt, n_threads=4)
    _bits_equal(np.stack(a.fields), np.stack(b.fields))
    for schedule in SCHEDULES:
        da, db = (r.tape.jvp_source(r.dsrc, return_fields=True, schedule=schedule) for r in (a, b))
        _bits_equal(da[0], db[0])
        _bits_equal(da[1], db[1])
        ga, gb = (r.tape.vjp(r.w, r.fc, schedule=schedule, return_source_grad=True) for r in (a, b))
        _bits_equal(ga[0], gb[0])
        _bits_equal(ga[1], gb[1])
    assert np.any(ga[1] != 0) and np.any(da[0] != 0)
    err = _dot_error(b)
    print("device identity, five events, %s: %.2e (bound %.0e)" % (np.dtype(dt).name, err, DOT_TOL[np.dtype(dt)]))
    assert err <= DOT_TOL[np.dtype(dt)], err


# ---- the torch operator (child processes)
def _torch_setup(dt, nn, n_ev, n_rcv, seed, **kw):
    import ttcr_amd

    rng = np.random.default_rng(seed)
    dx = 0.5
    hi = (np.array(nn) - 1) * dx
    v = rng.uniform(1.0, 2.0, nn).astype(dt)
    ev = np.column_stack([rng.uniform(0, 0.5, n_ev).round(3), (np.floor(rng.uniform(2, np.array(nn) - 3, (n_ev, 3))) + rng.uniform(0.2, 0.8, (n_ev, 3))) * dx])
    eor = np.concatenate([np.arange(n_ev), rng.integers(0, n_ev, n_rcv - n_ev)])[rng.permutation(n_rcv)]
    rcv = rng.uniform(0.7 * dx, hi - 0.7 * dx, (n_rcv, 3))
    axes = [np.arange(n) * dx for n in nn]
    g = ttcr_amd.Grid3d(*axes, cell_slowness=0, method="FSM", dtype=dt, weno=0, tt_from_rp=0, **kw)
    return rng, g, v, ev.astype(dt), eor, rcv


def _torch_events_operator():
    import torch
    import torch.autograd.forward_ad as fwAD

    import ttcr_amd.autograd as ag

    dt = np.float32
    nn = (13, 15, 11)
    rng, g, v, ev, eor, rcv = _torch_setup(dt, nn, 3, 12, 13, n_threads=2)
    vel = torch.tensor(v, device="cuda", requires_grad=True)
    evt = torch.tensor(ev, device="cuda", requires_grad=True)
    tt, fields = ag.raytrace_events(g, vel, evt, eor, rcv, return_fields=True)
    assert tt.is_cuda and fields.shape == (3,) + nn
    c_tt = rng.standard_normal(12).astype(dt)
    c_f = rng.standard_normal((3,) + nn).astype(dt)
    ((torch.from_numpy(c_tt).cuda() * tt).sum() + (torch.from_numpy(c_f).cuda() * fields).sum()).backward()
    # the same call by hand
    g.set_velocity(v)
    tt_ref, tape = g.raytrace_adjoint(np.column_stack([eor, ev[eor]]), rcv)
    assert tape.n_points == 3 and np.array_equal(tape.point_event, np.arange(3))
    _bits_equal(tt.detach().cpu().numpy(), tt_ref)
    fc = np.ascontiguousarray(c_f.transpose(0, 3, 2, 1)).reshape(3, -1)     # (n_events, nx, ny, nz) -> node order, x fastest
    grad, gsrc = tape.vjp(c_tt, fc, return_source_grad=True)
    _bits_equal(evt.grad.cpu().numpy(), gsrc)
    gv = torch.from_numpy(grad).cuda().reshape(nn[2], nn[1], nn[0]).permute(2, 1, 0).contiguous()
    _bits_equal(vel.grad.cpu().numpy(), (-gv / (vel.detach() * vel.detach())).cpu().numpy())
    _bits_equal(grad, tape.vjp(c_tt, fc))
    # device tensors in give device tensors out
    gd = tape.vjp(torch.from_numpy(c_tt).cuda(), torch.from_numpy(fc).cuda(), return_source_grad=True)
    assert gd[0].is_cuda and gd[1].is_cuda
    _bits_equal(gd[1].cpu().numpy(), gsrc)
    # forward mode: jvp + jvp_source
    tv = (v * rng.standard_normal(nn)).astype(dt)
    te = rng.standard_normal((3, 4)).astype(dt)
    with fwAD.dual_level():
        out = ag.raytrace_events(g, fwAD.make_dual(vel.detach(), torch.from_numpy(tv).cuda()),
                                 fwAD.make_dual(evt.detach(), torch.from_numpy(te).cuda()), eor, rcv, return_fields=True)
        tang = [fwAD.unpack_dual(o).tangent.detach().clone() for o in out]
        only = fwAD.unpack_dual(ag.raytrace_events(g, vel.detach(), fwAD.make_dual(evt.detach(), torch.from_numpy(te).cuda()), eor,
                                                   rcv)).tangent.detach().clone()
    ds = (-(tv / (v * v))).flatten("F")
    a, b = tape.jvp(ds, return_fields=True), tape.jvp_source(te, return_fields=True)
    _bits_equal(tang[0].cpu().numpy(), a[0] + b[0])
    _bits_equal(tang[1].cpu().numpy(), np.stack([m.reshape(nn, order="F") for m in a[1] + b[1]]))
    _bits_equal(only.cpu().numpy(), b[0])
    d_dev = tape.jvp_source(torch.from_numpy(te).cuda())
    assert d_dev.is_cuda
    _bits_equal(d_dev.cpu().numpy(), b[0])
    # forward and backward agree on the events' part
    lhs = float(c_tt.astype(np.float64) @ b[0].astype(np.float64) + c_f.astype(np.float64).ravel() @
                np.stack([m.reshape(nn, order="F") for m in b[1]]).astype(np.float64).ravel())
    rhs = float(gsrc.astype(np.float64).ravel() @ te.astype(np.float64).ravel())
    err = abs(lhs - rhs) / abs(rhs)
    print("raytrace_events, forward against backward: %.2e (bound %.0e)" % (err, DOT_TOL[np.dtype(dt)]))
    assert err <= DOT_TOL[np.dtype(dt)], (lhs, rhs)
    for bad in (np.array([0, 1, 1] * 4), np.zeros(12)):   # (an event without a row; no integers)
        try:
            ag.raytrace_events(g, vel, evt, bad, rcv)
        except ValueError:
            continue
        raise AssertionError("no ValueError")


def _torch_events_central_differences():
    import torch
    import torch.autograd.forward_ad as fwAD

    import ttcr_amd.autograd as ag

    dt = np.float64
    nn = (11, 11, 11)
    rng, g, v, ev, eor, rcv = _torch_setup(dt, nn, 1, 10, 19, eps=1e-15, maxit=200)
    vel = torch.tensor(v, device="cuda")

    def forward(e):
        return ag.raytrace_events(g, vel, torch.tensor(e, device="cuda"), eor, rcv).cpu().numpy()

    evt = torch.tensor(ev, device="cuda", requires_grad=True)
    c = rng.standard_normal(10)
    (torch.from_numpy(c).cuda() * ag.raytrace_events(g, vel, evt, eor, rcv)).sum().backward()
    J = np.zeros((10, 4))
    worst = 0.0
    for k in range(4):
        te = np.zeros((1, 4))
        te[0, k] = 1
        with fwAD.dual_level():
            J[:, k] = fwAD.unpack_dual(ag.raytrace_events(g, vel, fwAD.make_dual(evt.detach(), torch.from_numpy(te).cuda()), eor,
                                                          rcv)).tangent.cpu().numpy()
        fd = (forward(ev + STEP * te) - forward(ev - STEP * te)) / (2 * STEP)
        err = np.linalg.norm(J[:, k] - fd) / np.linalg.norm(fd)
        worst = max(worst, err)
        print("raytrace_events, d tt / d %s against central differences: %.2e (bound %.0e)" % ("t0 x y z".split()[k], err, TOL))
    assert worst <= TOL, worst
    back = evt.grad.cpu().numpy().ravel()
    err = np.linalg.norm(back - J.T @ c) / np.linalg.norm(J.T @ c)
    print("raytrace_events, backward against the forward-mode Jacobian: %.2e" % err)
    assert err <= 1e-12, err


def test_torch_raytrace_events_backward_and_forward_ad():
    _in_child("events_operator")


def test_torch_raytrace_events_against_central_differences():
    _in_child("events_central_differences")
