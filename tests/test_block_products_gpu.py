"""The block products of the field tape (FieldTape.jvp_block, vjp_block, gauss_newton_block) on the device, at the inputs of
tests/field_tape_cases.py.  Every comparison is to the bit and has three parts: jvp_block (receiver rows and fields) against tape.jvp of
each column on the same tape and against tests/tangent_reference.py; vjp_block against tape.vjp of each column and against
tests/adjoint_reference.py; gauss_newton_block against tape.gauss_newton of each column.  Neither the one-column kernels nor the numpy
restatements were written with the block kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import field_tape_cases as FC  # noqa: E402
import test_field_tape_edges_gpu as EG  # noqa: E402  (the grid and tape builders of the edge tests)
from field_tape_cases import _bits_equal  # noqa: E402

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
BLOCK_EDGE = {np.dtype(np.float32): 10, np.dtype(np.float64): 8}   # interior edge of a tile of the K-column relaxations: the tangent's
GROUP = 4                                                          # columns per relaxation


def _columns(rng, n, dt, scale, K=5):
    """K columns of n values: random; all +0; random with -0.0 and negative entries; wide-range; a copy of column 0; then random ones"""
    cols = [(scale * rng.standard_normal(n)).astype(dt) for _ in range(K)]
    if K > 1:
        cols[1] = np.zeros(n, dtype=dt)
    if K > 2:
        c = -np.abs(cols[2])
        c[rng.random(n) < 0.3] = -0.0
        c[rng.random(n) < 0.2] *= -1
        assert np.any(np.signbit(c) & (c == 0)) and np.any(c < 0)
        cols[2] = c.astype(dt)
    if K > 3:
        cols[3] = FC.wide_weights(rng, n, dt) * np.asarray(scale, dtype=dt)
    if K > 4:
        cols[4] = cols[0].copy()
    return np.stack(cols)


def _inputs(case, dt, rcv, K=5, seed=71):
    rng = np.random.default_rng(seed)
    n_nodes = int(np.prod(case.nn))
    ds = _columns(rng, n_nodes, dt, case.s, K)
    w = _columns(rng, rcv.shape[0], dt, 1.0, K)
    rw = rng.uniform(0.5, 2.0, (K, rcv.shape[0])).astype(dt)
    return ds, w, rw


def _check_block(tape, ds, w, rw, schedule="tiled", reference=None):
    """the three comparisons for the K columns of ds, w and rw (rw: (K, n_data), (n_data,) or None); reference = (case, dt, rcv, rows,
    fields) adds the numpy restatements.  Returns what the block calls gave."""
    K = ds.shape[0]
    dtt, mu = tape.jvp_block(ds, return_fields=True, schedule=schedule)
    pj = tape.passes
    assert dtt.shape == (K, tape.n_data) and mu.shape == (K, tape.n_events, tape.n_nodes) and dtt.dtype == tape.dtype
    _bits_equal(tape.jvp_block(ds, schedule=schedule), dtt)
    grad = tape.vjp_block(w, schedule=schedule)
    pv = tape.passes
    assert grad.shape == (K, tape.n_cols) and pj >= 1 and pv >= 1
    gn = tape.gauss_newton_block(ds, rw, schedule=schedule)
    assert gn.shape == (K, tape.n_cols) and isinstance(tape.passes, tuple) and min(tape.passes) >= 1
    for k in range(K):
        d1, m1 = tape.jvp(ds[k], return_fields=True, schedule=schedule)
        _bits_equal(dtt[k], d1)
        _bits_equal(mu[k], m1)
        _bits_equal(grad[k], tape.vjp(w[k], schedule=schedule))
        rwk = None if rw is None else (rw if rw.ndim == 1 else rw[k])
        _bits_equal(gn[k], tape.gauss_newton(ds[k], rwk, schedule=schedule))
        if reference is not None:
            case, dt, rcv, rows, fields = reference
            rd, rm = FC.reference_jvp(fields, case, dt, rcv, rows, ds[k])
            _bits_equal(dtt[k], rd)
            _bits_equal(mu[k], rm)
            _bits_equal(grad[k], FC.reference_vjp(fields, case, dt, rcv, rows, w[k], None))
    return dict(dtt=dtt, mu=mu, grad=grad, gn=gn, passes=(pj, pv))


def _check_copy_of_column_0(out):
    """column 4 repeats column 0 and sits alone in the second group: the bits of the first group's column 0"""
    for name in ("dtt", "mu", "grad"):
        _bits_equal(out[name][4], out[name][0])
    assert np.any(out["dtt"][0] != 0) and np.any(out["grad"][0] != 0)
    assert not np.any(out["dtt"][1]) and not np.any(out["mu"][1]) and not np.any(out["grad"][1])   # (the +0 columns)


# ---- 1. grid shapes against the tile edges
def test_the_shapes_meet_the_block_tile_edges():
    assert BLOCK_EDGE == FC.TAN_EDGE
    extents = {n for nn in FC.SHAPES for n in nn}
    for edge in BLOCK_EDGE.values():
        assert {edge - 1, edge, edge + 1, 2 * edge, 2 * edge + 1} <= extents, (edge, sorted(extents))


@DTYPES
@pytest.mark.parametrize("nn", FC.SHAPES, ids=lambda nn: "x".join(map(str, nn)))
def test_shapes_against_the_tile_edges(nn, dt):
    case = FC.shape_case(nn)
    assert len(case.events) == 2
    g, tape, rcv, rows, fields = EG._tape(case, dt)
    ds, w, rw = _inputs(case, dt, rcv, K=GROUP + 1)
    out = _check_block(tape, ds, w, rw, reference=(case, dt, rcv, rows, fields))
    _check_copy_of_column_0(out)
    rw[4] = rw[0]
    _bits_equal(tape.gauss_newton_block(ds, rw)[4], out["gn"][0])


# ---- 2. ties
@DTYPES
@pytest.mark.parametrize("name", FC.DECISIVE_TIES)
def test_fields_with_decisive_ties(name, dt):
    case = FC.tie_case(name)
    g, tape, rcv, rows, fields = EG._tape(case, dt)
    decisive, total = FC.count_ties(fields[0], case.nn)
    assert decisive > 0, (decisive, total)
    ds, w, rw = _inputs(case, dt, rcv)
    _check_copy_of_column_0(_check_block(tape, ds, w, rw, reference=(case, dt, rcv, rows, fields)))


# ---- 3. receivers that share nodes
@DTYPES
@pytest.mark.parametrize("name", FC.SHARED_CASES)
def test_receivers_that_share_nodes(name, dt):
    case = FC.shared_case(name)
    g, tape, rcv, rows, fields = EG._tape(case, dt, n_threads=1 if name == "one_event" else 2)
    ds, w, rw = _inputs(case, dt, rcv)
    rng = np.random.default_rng(73)
    for k in (0, 2, 3):   # cotangents over 2^-12 .. 2^12: a seed chain summed in another order has other bits
        w[k] = FC.wide_weights(rng, rcv.shape[0], dt)
    w[4] = w[0]
    _check_copy_of_column_0(_check_block(tape, ds, w, rw, reference=(case, dt, rcv, rows, fields)))


# ---- 4. group remainders
@DTYPES
def test_group_remainders(dt):
    case = FC.shape_case((17, 21, 29))
    g, tape, rcv, rows, fields = EG._tape(case, dt)
    ds, w, rw = _inputs(case, dt, rcv, K=9)
    nine = _check_block(tape, ds, w, rw)   # two full groups and a remainder of one, against the one-column calls
    for K in (1, 2, 3, 4, 8):
        dtt, mu = tape.jvp_block(ds[:K], return_fields=True)
        _bits_equal(dtt, nine["dtt"][:K])
        _bits_equal(mu, nine["mu"][:K])
        _bits_equal(tape.vjp_block(w[:K]), nine["grad"][:K])
        if K == 2:     # one set of row weights shared by the columns
            gn = tape.gauss_newton_block(ds[:K], rw[0])
            for k in range(K):
                _bits_equal(gn[k], tape.gauss_newton(ds[k], rw[0]))
        elif K == 3:   # none
            gn = tape.gauss_newton_block(ds[:K])
            for k in range(K):
                _bits_equal(gn[k], tape.gauss_newton(ds[k]))
        else:
            _bits_equal(tape.gauss_newton_block(ds[:K], rw[:K]), nine["gn"][:K])
    with pytest.raises(ValueError):
        tape.jvp_block(np.zeros((0, tape.n_cols), dtype=dt))
    with pytest.raises(ValueError):
        tape.gauss_newton_block(np.zeros((0, tape.n_cols), dtype=dt))
    with pytest.raises(ValueError):
        tape.vjp_block(np.zeros((0, tape.n_data), dtype=dt))


# ---- 5. cell tape
@DTYPES
def test_cell_tape(dt):
    import ttcr_amd

    nc = (9, 11, 8)
    nn = tuple(n + 1 for n in nc)
    rng = np.random.default_rng(79)
    axes = [np.arange(n) * FC.DX for n in nn]
    g = ttcr_amd.Grid3d(*axes, cell_slowness=1, method="FSM", dtype=dt, weno=0, tt_from_rp=0, n_threads=2)
    sc = 0.5 * (1.0 + 0.3 * rng.uniform(-1, 1, nc))
    g.set_slowness(sc)
    src = np.array([[0, 0.125, 3.3, 4.6, 2.2], [1, 0.0, 1.2, 0.7, 3.4]])
    rcv = FC.receivers(nn, FC.DX, FC.ZERO, rng, 10)
    src = src[rng.integers(0, 2, rcv.shape[0])]
    tt, tape = g.raytrace_adjoint(src, rcv, wrt="cells")
    n_cells = int(np.prod(nc))
    assert (tape.wrt, tape.n_cols, tape.n_events, tape.n_nodes) == ("cells", n_cells, 2, int(np.prod(nn)))
    ds = _columns(rng, n_cells, dt, sc.flatten("F"))
    w = _columns(rng, rcv.shape[0], dt, 1.0)
    rw = rng.uniform(0.5, 2.0, (5, rcv.shape[0])).astype(dt)
    for schedule in ("tiled", "jacobi"):
        _check_copy_of_column_0(_check_block(tape, ds, w, rw, schedule=schedule))


# ---- 6. slots and devices
@DTYPES
def test_slots_and_devices(dt):
    case = FC.slots_case()
    first = None
    for kw in (dict(n_threads=1), dict(n_threads=4), dict(n_threads=16), dict(n_threads=4, device=[0, 0])):
        g, tape, rcv, rows, fields = EG._tape(case, dt, **kw)
        assert g.n_devices == len(kw.get("device", [0]))
        ds, w, rw = _inputs(case, dt, rcv)
        if first is None:
            first = _check_block(tape, ds, w, rw)
            continue
        dtt, mu = tape.jvp_block(ds, return_fields=True)
        _bits_equal(dtt, first["dtt"])
        _bits_equal(mu, first["mu"])
        _bits_equal(tape.vjp_block(w), first["grad"])
        _bits_equal(tape.gauss_newton_block(ds, rw), first["gn"])


# ---- 7. long run
def test_long_run():
    dt = np.float32
    case = FC.long_case(dt)
    g, tape, rcv, rows, fields = EG._tape(case, dt, n_threads=3)
    ds, w, rw = _inputs(case, dt, rcv, K=GROUP)
    dtt, mu = tape.jvp_block(ds, return_fields=True)
    pj = tape.passes
    grad = tape.vjp_block(w)
    pv = tape.passes
    gn = tape.gauss_newton_block(ds, rw[0])
    print("long run, %s nodes, 3 events, 4 columns: passes of the block jvp %d, of the block vjp %d" % ("x".join(map(str, case.nn)), pj, pv))
    assert pj > FC.ADJ_RING and pv > FC.ADJ_RING, (pj, pv)
    for k in range(GROUP):
        d1, m1 = tape.jvp(ds[k], return_fields=True)
        _bits_equal(dtt[k], d1)
        _bits_equal(mu[k], m1)
        _bits_equal(grad[k], tape.vjp(w[k]))
    _bits_equal(gn[3], tape.gauss_newton(ds[3], rw[0]))


# ---- 8. neighbours keep their state
@DTYPES
def test_neighbours_keep_their_state(dt):
    case = FC.shape_case((17, 21, 29))
    g, tape, rcv, rows, fields = EG._tape(case, dt)
    ds, w, rw = _inputs(case, dt, rcv)
    rng = np.random.default_rng(83)
    dsrc = rng.standard_normal((4, tape.n_points, 4)).astype(dt)
    a = tape.jvp_source(dsrc, return_fields=True)
    tape.jvp_block(ds)
    tape.vjp_block(w)
    b = tape.jvp_source(dsrc, return_fields=True)
    _bits_equal(a[0], b[0])
    _bits_equal(a[1], b[1])
    tape.hold(w[0])
    h0 = tape.hvp(ds[0])
    grad = tape.vjp_block(w[2:])
    h1 = tape.hvp(ds[0])
    _bits_equal(h0, h1)
    tape.release_block()
    _bits_equal(tape.hvp(ds[0]), h0)   # (release_block leaves the held cotangent alone)
    _bits_equal(tape.vjp_block(w[2:]), grad)
    tape.release()
    _bits_equal(tape.vjp_block(w[2:]), grad)   # (... and release the block arrays)
    _bits_equal(tape.jvp_source(dsrc), a[0])


# ---- 9. memory and interface
def _block_bytes(tape, with_mu4):
    """what the header says the first block call adds (after a jvp): seeds of four columns, lam / mu of four columns unless jvp_source
    allocated them, and the staging of a group"""
    el = tape.dtype.itemsize
    en = tape.n_events * tape.n_nodes
    return (2 if with_mu4 else 1) * 4 * en * el + (4 * tape.n_cols + 8 * tape.n_rows) * el + (4 * tape.n_nodes * el if tape.wrt == "cells" else 0)


@DTYPES
def test_memory(dt):
    case = FC.shape_case((9, 11, 15))
    g, tape, rcv, rows, fields = EG._tape(case, dt)
    ds, w, rw = _inputs(case, dt, rcv)
    tape.jvp(ds[0])   # (the first jvp's arrays are not the block's)
    n0 = tape.nbytes
    grad = tape.vjp_block(w)
    assert tape.nbytes - n0 == _block_bytes(tape, True), (tape.nbytes - n0, _block_bytes(tape, True))
    tape.jvp_block(ds)
    tape.gauss_newton_block(ds, rw)
    assert tape.nbytes - n0 == _block_bytes(tape, True)
    tape.release_block()
    assert tape.nbytes == n0
    tape.release_block()
    assert tape.nbytes == n0
    # after a four-column jvp_source the lam / mu array is there already, and stays when the block arrays go
    tape.jvp_source(np.ones((2, tape.n_points, 4), dtype=dt))
    n1 = tape.nbytes
    _bits_equal(tape.vjp_block(w), grad)
    assert tape.nbytes - n1 == _block_bytes(tape, False)
    tape.release_block()
    assert tape.nbytes == n1
    # a tape whose first forward-mode call is a block call
    g, tape2, rcv, rows, fields = EG._tape(case, dt)
    _bits_equal(tape2.vjp_block(w), grad)
    assert tape2.nbytes == n0 + _block_bytes(tape2, True)


@DTYPES
def test_jacobi_has_the_bits_of_tiled(dt):
    case = FC.shape_case((16, 20, 28))
    g, tape, rcv, rows, fields = EG._tape(case, dt)
    ds, w, rw = _inputs(case, dt, rcv)
    t = _check_block(tape, ds, w, rw, schedule="tiled")
    dtt, mu = tape.jvp_block(ds, return_fields=True, schedule="jacobi")
    _bits_equal(dtt, t["dtt"])
    _bits_equal(mu, t["mu"])
    _bits_equal(tape.vjp_block(w, schedule="jacobi"), t["grad"])
    _bits_equal(tape.gauss_newton_block(ds, rw, schedule="jacobi"), t["gn"])
    with pytest.raises(ValueError):
        tape.jvp_block(ds, schedule="sweep")
    for bad in (ds[0], ds[:, :-1], ds[None]):
        with pytest.raises(ValueError):
            tape.jvp_block(bad)
    with pytest.raises(ValueError):
        tape.vjp_block(w[:, :-1])
    with pytest.raises(ValueError):
        tape.gauss_newton_block(ds, rw[:3])


def _torch_device_tensors(flat):
    import torch

    dt = np.float32 if flat == "fp32" else np.float64
    case = FC.shape_case((9, 11, 15))
    g, tape, rcv, rows, fields = EG._tape(case, dt)
    ds, w, rw = _inputs(case, dt, rcv)
    dev = torch.device("cuda", tape.device)
    tds, tw, trw = (torch.from_numpy(a).to(dev) for a in (ds, w, rw))
    dtt, mu = tape.jvp_block(ds, return_fields=True)
    tdtt, tmu = tape.jvp_block(tds, return_fields=True)
    assert tdtt.device == dev and tmu.device == dev and tmu.shape == (5, tape.n_events, tape.n_nodes)
    _bits_equal(tdtt.cpu().numpy(), dtt)
    _bits_equal(tmu.cpu().numpy(), mu)
    _bits_equal(tape.jvp_block(tds).cpu().numpy(), dtt)
    tg = tape.vjp_block(tw)
    assert tg.device == dev
    _bits_equal(tg.cpu().numpy(), tape.vjp_block(w))
    for a, b in ((trw, rw), (trw[0], rw[0]), (None, None)):
        tgn = tape.gauss_newton_block(tds, a)
        assert tgn.device == dev
        _bits_equal(tgn.cpu().numpy(), tape.gauss_newton_block(ds, b))
    # tensors on the host come back on the host
    hg = tape.vjp_block(torch.from_numpy(w))
    assert hg.device.type == "cpu"
    _bits_equal(hg.numpy(), tape.vjp_block(w))


@pytest.mark.parametrize("flat", ["fp32", "fp64"])
def test_torch_device_tensors(flat):
    """in a fresh process that initialises torch's device before the first grid (torch ships a HIP runtime of its own)"""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_block_products_gpu as t; "
            "t._torch_device_tensors(%r)" % (HERE, ROOT, flat))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
