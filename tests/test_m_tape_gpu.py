"""The M tape on the device (Grid3d.raytrace_tape, ttcr_fsm_raytrace_multi_tape): its rows are compute_M's matrices stacked, entry for
entry and sign bit for sign bit; tape.vjp(w) is M^T w summed per node in ascending row order from +0 in the grid dtype -- bit-equal to
np.add.at over the stacked CSR -- whatever n_threads, the device list or the number of runs; the torch operator's backward is that
product in velocity's layout."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _in_child(fn, *args):
    """Run _torch_<fn>(*args) of this module in a fresh process that initialises torch's device before the first grid (torch ships a
    HIP runtime of its own; a process whose first device user was the library finds no device through torch afterwards)."""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_m_tape_gpu as t; t._torch_%s(*%r)"
            % (HERE, ROOT, fn, args))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
CASES = ["m_grad", "m_rough", "m_translate", "m_weno", "m_two_points", "m_close_points"]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))


def _stacked(M):
    import scipy.sparse as sp

    return sp.vstack(M).tocsr()


def _same_csr(A, B):
    np.testing.assert_array_equal(A.indptr, B.indptr)
    np.testing.assert_array_equal(A.indices, B.indices)
    _bits_equal(A.data, B.data)   # (-0.0 and +0.0 are different entries)


def _ref_vjp(Ms, w_t, T):
    g = np.zeros(Ms.shape[1], T)
    rows = np.repeat(np.arange(Ms.shape[0]), np.diff(Ms.indptr))
    np.add.at(g, Ms.indices, Ms.data.astype(T) * np.asarray(w_t, T)[rows])
    return g


def _events(n_ev, nn, dx, rng, n_rcv=(2, 7)):
    """5-column rows (event id, t0, x, y, z) with the events' receiver rows interleaved; tape rows = events ascending, rcv order within"""
    hi = (np.array(nn) - 1) * dx
    ev_src = rng.uniform(1.5 * dx, hi - 1.5 * dx, (n_ev, 3))
    ev_t0 = rng.uniform(0, 0.5, n_ev).round(3)
    ids = np.concatenate([np.full(int(k), e) for e, k in enumerate(rng.integers(n_rcv[0], n_rcv[1], n_ev))])
    ids = ids[rng.permutation(ids.size)]
    src = np.column_stack([ids, ev_t0[ids], ev_src[ids]])
    rcv = rng.uniform(0.7 * dx, hi - 0.7 * dx, (ids.size, 3))
    order = np.concatenate([np.nonzero(ids == e)[0] for e in range(n_ev)])
    return src, rcv, order


def _grid(nn, dx, dt, s, **kw):
    import ttcr_amd

    axes = [np.arange(n) * dx for n in nn]
    kw.setdefault("weno", 0)
    g = ttcr_amd.Grid3d(*axes, cell_slowness=0, method="FSM", tt_from_rp=0, dtype=dt, **kw)
    g.set_slowness(s.reshape(nn, order="F"))
    return g


@pytest.fixture(scope="module")
def mg():
    return np.load(os.path.join(HERE, "golden", "m_golden.npz"))


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_tape_csr_is_compute_m(mg, name, dt):
    import ttcr_amd

    m = mg[name + "/meta"]
    nc, dx, org, translate, weno = tuple(int(v) for v in m[:3]), float(m[3]), tuple(float(v) for v in m[4:7]), bool(m[7]), bool(m[8])
    nn = tuple(v + 1 for v in nc)
    axes = [org[a] + np.arange(nn[a]) * dx for a in range(3)]
    g = ttcr_amd.Grid3d(*axes, n_threads=2, cell_slowness=0, method="FSM", tt_from_rp=0, weno=int(weno), dtype=dt, translate_grid=translate)
    g.set_slowness(mg[name + "/slowness"].reshape(nn, order="F"))
    src = np.column_stack([mg[name + "/t0"], mg[name + "/src"]])
    rcv = mg[name + "/rcv"]
    multi = src.shape[0] > 1
    srows = src if multi else np.repeat(src, rcv.shape[0], axis=0)
    tt, M = g.raytrace(srows, rcv, compute_M=True, aggregate_src=multi)
    tt2, tape = g.raytrace_tape(srows, rcv, aggregate_src=multi)
    _bits_equal(tt2, tt)
    Ms = _stacked(M)
    A = tape.to_csr()
    assert A.dtype == np.float64 and A.shape == Ms.shape == (rcv.shape[0], nn[0] * nn[1] * nn[2])
    _same_csr(A, Ms)
    w = np.random.default_rng(5).standard_normal(rcv.shape[0]).astype(dt)
    _bits_equal(tape.vjp(w), _ref_vjp(Ms, w, dt))


@pytest.mark.parametrize("n_threads", [1, 3, 5])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_tape_vjp_several_events(n_threads, dt):
    rng = np.random.default_rng(21)
    nn, dx = (41, 37, 33), 0.5
    s = rng.uniform(0.5, 1.0, int(np.prod(nn)))
    src, rcv, order = _events(7, nn, dx, rng)
    g = _grid(nn, dx, dt, s, n_threads=n_threads)
    tt, M = g.raytrace(src, rcv, compute_M=True)
    tt2, tape = g.raytrace_tape(src, rcv)
    _bits_equal(tt2, tt)
    Ms = _stacked(M)
    _same_csr(tape.to_csr(), Ms)
    w = rng.standard_normal(rcv.shape[0]).astype(dt)
    ref = _ref_vjp(Ms, w[order], dt)
    _bits_equal(tape.vjp(w), ref)


def _torch_device_w(n_threads, dt_name):
    import torch

    dt = np.dtype(dt_name).type
    rng = np.random.default_rng(21)
    nn, dx = (41, 37, 33), 0.5
    s = rng.uniform(0.5, 1.0, int(np.prod(nn)))
    src, rcv, order = _events(7, nn, dx, rng)
    g = _grid(nn, dx, dt, s, n_threads=n_threads)
    _, M = g.raytrace(src, rcv, compute_M=True)
    _, tape = g.raytrace_tape(src, rcv)
    w = rng.standard_normal(rcv.shape[0]).astype(dt)
    ref = _ref_vjp(_stacked(M), w[order], dt)
    gd = tape.vjp(torch.from_numpy(w).cuda())          # w on the device: no host copy, the result stays there
    assert gd.is_cuda and gd.dtype == (torch.float32 if dt == np.float32 else torch.float64)
    _bits_equal(gd.cpu().numpy(), ref)
    gh = tape.vjp(torch.from_numpy(w))                   # a host tensor gives a host tensor
    assert not gh.is_cuda
    _bits_equal(gh.numpy(), ref)
    with pytest.raises(ValueError):
        tape.vjp(torch.ones(1, device="cuda"))


@pytest.mark.parametrize("n_threads,dt", [(3, "float32"), (5, "float64")])
def test_tape_vjp_of_a_device_tensor(n_threads, dt):
    _in_child("device_w", n_threads, dt)


def test_tape_aggregate_src_and_device_list():
    rng = np.random.default_rng(8)
    dt = np.float32
    nn, dx = (33, 29, 31), 0.5
    s = rng.uniform(0.5, 1.0, int(np.prod(nn)))
    hi = (np.array(nn) - 1) * dx
    # aggregate_src: the distinct source rows are the points of ONE source, every receiver belongs to it
    pts = np.array([[5.1, 6.2, 7.3], [5.4, 6.0, 7.1], [9.0, 4.0, 3.0]])
    rcv = rng.uniform(0.7 * dx, hi - 0.7 * dx, (3, 3))
    for agg in (True, False):
        g = _grid(nn, dx, dt, s, n_threads=2)
        tt, M = g.raytrace(pts, rcv, compute_M=True, aggregate_src=agg)
        tt2, tape = g.raytrace_tape(pts, rcv, aggregate_src=agg)
        _bits_equal(tt2, tt)
        Ms = _stacked(M)
        _same_csr(tape.to_csr(), Ms)
        w = rng.standard_normal(rcv.shape[0]).astype(dt)
        _bits_equal(tape.vjp(w), _ref_vjp(Ms, w, dt))   # (one row per receiver either way: every event here has one receiver or all)
    # two replicas of the grid on one device against the one-device grid: the same tape, the same gradient bits
    src, rcv, order = _events(6, nn, dx, rng)
    w = rng.standard_normal(rcv.shape[0]).astype(dt)
    g1 = _grid(nn, dx, dt, s, n_threads=4, device=0)
    g2 = _grid(nn, dx, dt, s, n_threads=4, device=[0, 0])
    assert g2.n_devices == 2
    tt1, t1 = g1.raytrace_tape(src, rcv)
    tt2, t2 = g2.raytrace_tape(src, rcv)
    _bits_equal(tt2, tt1)
    _same_csr(t2.to_csr(), t1.to_csr())
    _bits_equal(t2.vjp(w), t1.vjp(w))
    _bits_equal(t1.vjp(w), _ref_vjp(_stacked(g1.raytrace(src, rcv, compute_M=True)[1]), w[order], dt))


def test_tape_128_cube():
    rng = np.random.default_rng(128)
    dt = np.float32
    nn, dx = (128, 128, 128), 1.0
    z = np.arange(nn[2]) * dx
    s = (np.repeat(1.0 / (1.5 + 0.02 * z), nn[0] * nn[1]) * rng.uniform(0.95, 1.05, int(np.prod(nn)))).astype(dt)
    src, rcv, order = _events(4, nn, dx, rng, n_rcv=(8, 17))
    g = _grid(nn, dx, dt, s, n_threads=2)
    tt, M = g.raytrace(src, rcv, compute_M=True)
    tt2, tape = g.raytrace_tape(src, rcv)
    _bits_equal(tt2, tt)
    Ms = _stacked(M)
    _same_csr(tape.to_csr(), Ms)
    w = rng.standard_normal(rcv.shape[0]).astype(dt)
    _bits_equal(tape.vjp(w), _ref_vjp(Ms, w[order], dt))
    assert tape.nbytes > 0 and tape.shape == Ms.shape


def test_tape_repeatable_and_independent_of_the_grid():
    rng = np.random.default_rng(3)
    dt = np.float64
    nn, dx = (25, 27, 29), 0.5
    s = rng.uniform(0.5, 1.0, int(np.prod(nn)))
    src, rcv, order = _events(4, nn, dx, rng)
    w = rng.standard_normal(rcv.shape[0])
    g = _grid(nn, dx, dt, s, n_threads=2)
    tt_a, ta = g.raytrace_tape(src, rcv)
    tt_b, tb = g.raytrace_tape(src, rcv)
    _bits_equal(tt_a, tt_b)
    ga = ta.vjp(w)
    _bits_equal(tb.vjp(w), ga)
    _bits_equal(ta.vjp(w), ga)
    csr_a = ta.to_csr()
    # another model, another call: the first tape keeps its own matrix; so it does after the grid is gone
    g.set_slowness((s * 1.3).reshape(nn, order="F"))
    _, tc = g.raytrace_tape(src, rcv)
    g.raytrace(src, rcv, compute_M=True)
    assert not np.array_equal(tc.vjp(w), ga)
    del g
    import gc

    gc.collect()
    _bits_equal(ta.vjp(w), ga)
    _same_csr(ta.to_csr(), csr_a)
    ta.free()
    ta.free()
    with pytest.raises(ValueError):
        ta.vjp(w)


@pytest.mark.parametrize("flat", [False, True], ids=["3-D", "flat C order"])
def test_torch_op_backward_is_m_transpose(flat):
    _in_child("op", flat)


def _torch_op(flat):
    import torch

    import ttcr_amd.autograd as ag

    rng = np.random.default_rng(11)
    dt = np.float32
    nn, dx = (21, 23, 19), 0.5
    v = rng.uniform(1.0, 2.0, nn).astype(dt)
    src, rcv, order = _events(4, nn, dx, rng)
    g = _grid(nn, dx, dt, 1.0 / v.flatten("F"), n_threads=2)
    vel = torch.tensor(v.reshape(-1) if flat else v, device="cuda", requires_grad=True)
    d = torch.from_numpy(rng.uniform(0.5, 4.0, rcv.shape[0]).astype(dt)).cuda()
    tt = ag.raytrace(g, vel, src, rcv)
    assert tt.is_cuda and tt.dtype == torch.float32
    g.set_velocity(v)
    tt_ref, M = g.raytrace(src, rcv, compute_M=True)
    _bits_equal(tt.detach().cpu().numpy(), tt_ref)
    loss = ((tt - d) ** 2).sum()
    loss.backward(retain_graph=True)
    w = (2 * (tt - d)).detach().cpu().numpy()
    ref = _ref_vjp(_stacked(M), w[order], dt)                              # node order, x fastest
    ref_v = ref.reshape(nn, order="F")                                     # -> (nx, ny, nz)
    ref_v = ref_v.reshape(-1) if flat else ref_v
    assert vel.grad.shape == vel.shape
    _bits_equal(vel.grad.cpu().numpy(), ref_v)
    first = vel.grad.clone()
    vel.grad = None
    loss.backward()                                                        # (the graph was retained: the tape is still there)
    _bits_equal(vel.grad.cpu().numpy(), first.cpu().numpy())
    # forward and backward once more from scratch: the same bits
    vel.grad = None
    ((ag.raytrace(g, vel, src, rcv) - d) ** 2).sum().backward()
    _bits_equal(vel.grad.cpu().numpy(), first.cpu().numpy())


def test_tape_refusals():
    import ttcr_amd

    x = np.arange(9) * 1.0
    gc = ttcr_amd.Grid3d(x, x, x, cell_slowness=1, method="FSM", tt_from_rp=0, weno=0, dtype=np.float32)
    src = np.array([[3.1, 3.2, 3.3]])
    rcv = np.array([[1.0, 1.0, 1.0], [6.5, 6.0, 5.0]])
    with pytest.raises(NotImplementedError):
        gc.raytrace_tape(src, rcv)
    g2 = ttcr_amd.Grid2d(x, x, cell_slowness=0, method="FSM", dtype=np.float32)
    with pytest.raises(NotImplementedError):
        g2.raytrace_tape(np.array([[3.1, 3.3]]), np.array([[1.0, 1.0], [6.5, 5.0]]))
    g = _grid((9, 9, 9), 1.0, np.float32, np.ones(729))
    _, tape = g.raytrace_tape(src, rcv)
    with pytest.raises(ValueError):
        tape.vjp(np.ones(3, np.float32))
