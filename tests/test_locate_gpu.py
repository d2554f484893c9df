"""The grid-search hypocentre location of the field tape on the device (FieldTape.locate_grid, geometry, node_coordinates,
release_locate, inversion.locate).  Every comparison is to the bit, against the numpy restatement of
tests/locate_reference.py run on the device's own fields, for fp32 and fp64 tapes.  The grids are small: what can go wrong are the seams
between node tiles and between the nodes of one lane, the last partial tile, the chunks of hypocentres, the three staging shapes and the
path without staging, the order of a hypocentre's picks, and the tie rule.  tests/test_locate.py asserts on oracle fields that the cases
decide what they are meant to decide."""
import ctypes as C
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
import locate_cases as LC  # noqa: E402
import locate_reference as LR  # noqa: E402

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
ORIGIN = (-37.25, 1200.5, -3.125)
THIN = (1025, 3, 2)                 # a grid on which boxes of tile - 1, tile, tile + 1 and 2 tile + 1 nodes exist for tiles of 256 .. 1024
SMALL = (7, 6, 8)                   # 336 nodes: more than the 256 lanes of a workgroup, so every tile shape has a seam inside it
FIELD_COUNTS = (7, 13, 25, 49)      # fields per tape: 4, 2 and 1 nodes per lane and the path without staging, in fp32 and in fp64


class Tape:
    """one raytrace_adjoint call in the reciprocal layout: every event is a station, with one receiver each"""

    def __init__(self, nn, dt, stations, kind="gradient", wrt="nodes", origin=LC.ZERO, translate=False, n_threads=1, dx=LC.DX):
        import ttcr_amd

        self.nn, self.dt, self.dx, self.origin = nn, dt, dx, origin
        rng = np.random.default_rng(sum(nn) + len(stations))
        pts = LC.station_points(stations, dx, origin)
        events = [FC._event(p[None, :], FC.random_receivers(nn, dx, origin, rng, 1)) for p in pts]
        s = LC.model(nn, kind)
        case = FC.Case("stations", nn, dx, origin, s, events)
        src, rcv, agg, rows = FC.call_arrays(case, np.random.default_rng(61))
        axes = [origin[a] + np.arange(nn[a]) * dx for a in range(3)]
        cells = wrt == "cells"
        self.grid = ttcr_amd.Grid3d(*axes, n_threads=n_threads, cell_slowness=1 if cells else 0, method="FSM", dtype=dt, weno=0,
                                    tt_from_rp=0, translate_grid=translate, eps=1e-15, maxit=200)   # (converged fields)
        if cells:
            nc = tuple(n - 1 for n in nn)
            self.grid.set_slowness(np.random.default_rng(67).uniform(0.4, 0.7, int(np.prod(nc))).astype(dt).reshape(nc, order="F"))
        else:
            self.grid.set_slowness(np.asarray(s, dtype=dt).reshape(nn, order="F"))
        self.rcv = rcv
        self.tt, self.tape = self.grid.raytrace_adjoint(src, rcv, aggregate_src=agg, wrt=wrt)
        assert self.tape.n_events == len(stations)
        self.T = np.stack([self.tape.field(e) for e in range(len(stations))])
        assert self.T.dtype == dt and np.all(np.isfinite(self.T))

    def check(self, picks, n_hypo=None, box=None, volume=True):
        """locate_grid against the restatement on the device's fields, to the bit; returns the reference (node, t0, misfit, volume)"""
        ref = LR.grid_search(self.T, self.nn, LR.csr_of(*picks, n_hypo=n_hypo), box)
        got = self.tape.locate_grid(*picks, n_hypo=n_hypo, box=box, return_misfit=volume)
        assert got[0].dtype == np.int64 and np.array_equal(got[0], ref[0]), (got[0], ref[0])
        assert LC.same_bits(got[1], ref[1]) and LC.same_bits(got[2], ref[2]), (got[1:3], ref[1:3])
        if volume:
            assert got[3].shape == ref[3].shape and got[3].dtype == np.float64
            assert LC.same_bits(got[3], ref[3]), np.argwhere(got[3].view(np.int64) != ref[3].view(np.int64))[:5]
        return ref


def random_picks(T, n_hypo, rng, t_origin=0.0, noise=0.02):
    """n_hypo hypocentres at random nodes, each seen by a random subset (at least two) of the fields in random order, with noise on the
    times and random weights; the picks of the hypocentres interleaved"""
    nf, n = T.shape
    ps = []
    for q in range(n_hypo):
        f = rng.permutation(nf)[:int(rng.integers(2, nf + 1))]
        p = LC.picks_at(T, int(rng.integers(0, n)), fields=f, t_origin=t_origin, weights=rng.uniform(0.5, 2.0, f.size), hypo=q)
        ps.append((p[0], p[1], p[2] + noise * rng.standard_normal(f.size), p[3]))
    return LC.join(*ps)


def many_stations(nn, n, rng):
    hi = np.array(nn) - 1.0
    return [list(p) for p in rng.uniform(0.2, hi - 0.2, (n, 3))]


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["fp32", "fp64"])
def base(request):
    return Tape(LC.NN, request.param, LC.STATIONS)


def test_base_case_nodes_origin_times_misfits_and_every_node_of_the_volume(base):
    picks = LC.base_picks(base.T)
    node, t0, mis, vol = base.check(picks)
    # (what test_locate.py asserts on oracle fields holds on the device's fields too: the case decides)
    assert list(node) == list(LC.TRUE_NODES) * 2 + [0]
    assert np.all(mis == 0) and np.all(t0[:4] == 0) and np.all(t0[4:8] == LC.T_ORIGIN)
    assert np.all(vol[8] == 0) and all((vol[q] == 0).sum() == 1 for q in range(8))
    assert base.tape.geometry[0] == LC.NN and base.tape.geometry[1] == LC.DX and np.array_equal(base.tape.geometry[2], [0, 0, 0])


@pytest.mark.parametrize("count", ["chunk-1", "chunk", "chunk+1"])
def test_hypocentre_counts_around_the_chunk(base, count):
    chunk = base.tape.locate_shape[1]
    nq = chunk + {"chunk-1": -1, "chunk": 0, "chunk+1": 1}[count]
    base.check(random_picks(base.T, nq, np.random.default_rng(nq)), volume=count == "chunk+1")


def test_boxes_one_node_x_extent_one_and_the_numbering(base):
    picks = random_picks(base.T, 5, np.random.default_rng(7))
    whole = base.check(picks)
    for box in [((3, 4), (2, 3), (5, 6)), ((4, 5), (0, 8), (0, 10)), ((2, 7), (1, 6), (3, 9)), ((0, 9), (7, 8), (0, 10)), ((8, 9), (7, 8), (9, 10))]:
        ref = base.check(picks, box=box)
        sl = tuple(slice(*box[a]) for a in (2, 1, 0))
        assert LC.same_bits(ref[3], whole[3][(slice(None),) + sl])            # the volume of a box is the whole volume's slice
    assert list(base.check(picks, box=((3, 4), (2, 3), (5, 6)))[0]) == [LC.node_of(LC.NN, 3, 2, 5)] * 5


@DTYPES
def test_boxes_around_the_node_tile(dt):
    run = Tape(THIN, dt, [[0.3, 0.4, 0.0], [1000.6, 1.7, 1.0]], kind="smooth")
    tile, chunk, staged = run.tape.locate_shape
    assert staged and tile % 256 == 0
    picks = random_picks(run.T, 3, np.random.default_rng(11))
    for n in (tile - 1, tile, tile + 1, 2 * tile + 1):
        ext = next((a, b, c) for c in (1, 2) for b in (1, 2, 3) for a in range(1, THIN[0] + 1) if a * b * c == n)
        box = ((THIN[0] - ext[0], THIN[0]), (THIN[1] - ext[1], THIN[1]), (0, ext[2]))
        run.check(picks, box=box)
    run.check(picks)   # and the whole grid: several tiles, the last one partial


@DTYPES
@pytest.mark.parametrize("n_fields", FIELD_COUNTS)
def test_field_counts_through_every_staging_shape_and_pick_layouts(dt, n_fields):
    rng = np.random.default_rng(100 + n_fields)
    run = Tape(SMALL, dt, many_stations(SMALL, n_fields, rng))
    tile, chunk, staged = run.tape.locate_shape
    # the shapes the counts are chosen for: 48 KiB of LDS hold the values of 256 * sub nodes of every field, sub = 4, 2, 1; else no staging
    sub = next((s for s in (4, 2, 1) if n_fields * np.dtype(dt).itemsize * 256 * s <= 48 * 1024), 0)
    assert (tile, staged) == (256 * max(sub, 1), sub > 0)
    T, n = run.T, run.T.shape[1]
    every = np.arange(n_fields)
    ps = [LC.picks_at(T, 200, fields=np.concatenate([every, every[::-1], every[:3]]), weights=rng.uniform(0.5, 2, 2 * n_fields + 3), hypo=0),
          LC.picks_at(T, 17, fields=every[1::2], hypo=1),                                       # a strict subset
          LC.picks_at(T, 300, fields=every, weights=np.zeros(n_fields), hypo=3),                # all weights zero (2: no picks at all)
          LC.picks_at(T, 255, fields=every, weights=np.where(every % 3 == 1, 0.0, 1.5), hypo=4),   # zero weights among others
          LC.picks_at(T, 256, fields=every[::-1], hypo=5)]
    ps = [(p[0], p[1], p[2] + 0.01 * rng.standard_normal(p[2].size), p[3]) for p in ps]         # (noise: the order of the sums shows)
    node, t0, mis, vol = run.check(LC.join(*ps), n_hypo=7)
    assert node[2] == node[3] == node[6] == -1 and np.all(vol[[2, 3, 6]] == 0) and np.all(np.signbit(vol[[2, 3, 6]]) == 0)
    assert np.all(node[[0, 1, 4, 5]] >= 0)
    run.check(random_picks(T, 9, rng), box=((1, 7), (0, 6), (1, 8)))


@DTYPES
def test_mirror_tie_takes_the_lower_node(dt):
    run = Tape(LC.NN, dt, LC.MIRROR_STATIONS, kind="homogeneous")
    i, j, k = LC.MIRROR_TRUE
    true, mirror = LC.node_of(LC.NN, i, j, k), LC.node_of(LC.NN, i, j, 2 * LC.MIRROR_PLANE - k)
    assert LC.same_bits(run.T[:, true], run.T[:, mirror])             # the device's fields are mirror-symmetric to the bit, as the oracle's
    node, t0, mis, vol = run.check(LC.picks_at(run.T, true))
    assert mirror < true and list(node) == [mirror] and mis[0] == 0 and (vol[0] == 0).sum() == 2


def test_epoch_seconds_are_held_in_float64(base):
    epoch = 1.7e9
    ps = [LC.picks_at(base.T, m, t_origin=epoch, hypo=q) for q, m in enumerate(LC.TRUE_NODES)]
    node, t0, mis, vol = base.check(LC.join(*ps))
    # the precondition: at this magnitude a time is held to 2.4e-7 s, and the fields still decide
    assert list(node) == list(LC.TRUE_NODES) and np.all(np.abs(t0 - epoch) < 1e-6)
    runner_up = np.array([np.sort(v.ravel())[1] for v in vol])
    assert np.all(mis < 1e-12) and np.all(runner_up > 1e-4), (mis, runner_up)


@DTYPES
@pytest.mark.parametrize("variant", ["translated", "origin", "cells", "threads4"])
def test_grid_and_tape_variants(dt, variant):
    kw = dict(translated=dict(origin=ORIGIN, translate=True), origin=dict(origin=ORIGIN), cells=dict(wrt="cells"), threads4=dict(n_threads=4))
    run = Tape(LC.NN, dt, LC.STATIONS, **kw[variant])
    t = run.tape
    assert t.wrt == ("cells" if variant == "cells" else "nodes")
    node = run.check(random_picks(run.T, 6, np.random.default_rng(23)))[0]
    nn3, dx, origin = t.geometry
    assert nn3 == LC.NN and dx == LC.DX and np.array_equal(origin, run.origin)
    # the returned node as a point: receiver_eval there reads the field value itself
    xyz = t.node_coordinates(np.concatenate([node, [-1]]))
    assert np.all(np.isnan(xyz[-1])) and np.all(np.isfinite(xyz[:-1]))
    for f in range(t.n_events):
        tt = t.receiver_eval(xyz[:-1], np.full(node.size, f), return_grad=False)
        assert LC.same_bits(tt, run.T[f, node])


def test_nbytes_and_the_other_calls_are_left_alone(base):
    t = base.tape
    t.release_locate()
    w = np.random.default_rng(5).standard_normal(base.rcv.shape[0]).astype(base.dt)
    g0, before = t.vjp(w), t.nbytes
    picks = random_picks(base.T, 70, np.random.default_rng(29))
    t.locate_grid(*picks)
    small = t.nbytes
    assert small > before
    t.locate_grid(*picks, return_misfit=True)
    with_volume = t.nbytes
    assert with_volume >= small + 70 * 720 * 8                  # the host volume is formed in a buffer of the tape
    t.locate_grid(*random_picks(base.T, 3, np.random.default_rng(31)), return_misfit=True)
    assert t.nbytes == with_volume                              # the buffers grow to the largest call and stay
    assert LC.same_bits(t.vjp(w), g0) and t.nbytes == with_volume
    t.release_locate()
    assert t.nbytes == before
    t.release_locate()
    assert t.nbytes == before and LC.same_bits(t.vjp(w), g0)


def test_c_entry_refuses_what_needs_the_tape_to_tell(base):
    from ttcr_amd import _lib

    lib, h = _lib.load(), base.tape._h
    off, tm = (C.c_longlong * 2)(0, 1), (C.c_double * 1)(1.0)
    node, t0, mis = (C.c_longlong * 1)(), (C.c_double * 1)(), (C.c_double * 1)()

    def call(field, box):
        st = lib.ttcr_fsm_loc_grid(h, 1, off, (C.c_int * 1)(field), tm, None, None if box is None else (C.c_int * 6)(*box), node, t0, mis, None, 0)
        return st, _lib.last_error()
    assert call(0, None)[0] == 0
    for field, box, word in [(5, None, "pick_field"), (-1, None, "pick_field"), (0, (0, 10, 0, 8, 0, 10), "box"), (0, (-1, 9, 0, 8, 0, 10), "box"),
                             (0, (0, 9, 0, 8, 10, 11), "box"), (0, (3, 3, 0, 8, 0, 10), "box"), (0, (0, 9, 5, 4, 0, 10), "box")]:
        st, msg = call(field, box)
        assert st == 1 and msg.startswith(word), (field, box, st, msg)
    with pytest.raises(ValueError, match="pick_field"):
        base.tape.locate_grid([0], [5], [1.0])
    with pytest.raises(ValueError, match="box"):
        base.tape.locate_grid([0], [0], [1.0], box=((0, 10), (0, 8), (0, 10)))


def _noise_free_picks(stand_in, true, t_origin):
    nf = stand_in.n_events
    hyp = np.repeat(np.arange(len(true)), nf)
    fld = np.tile(np.arange(nf), len(true))
    tt = stand_in.receiver_eval(np.repeat(true, nf, axis=0), fld, return_grad=False).astype(np.float64)
    return hyp, fld, t_origin + tt, 1.0 + 0.5 * (fld % 3)


@DTYPES
def test_inversion_locate_equals_the_stand_in_element_for_element(dt):
    from ttcr_amd import inversion

    run = Tape(LC.NN, dt, LC.STATIONS, kind="smooth", origin=ORIGIN)
    stand_in = LR.StandInTape(list(run.T), LC.NN, LC.DX, origin=ORIGIN)
    rng = np.random.default_rng(37)
    true = np.asarray(ORIGIN) + rng.uniform(0.6, np.array(LC.NN) - 1.6, (7, 3)) * LC.DX
    picks = _noise_free_picks(stand_in, true, 3.0)
    for refine in (0, 10):
        got = inversion.locate(run.tape, *picks, n_hypo=8, refine=refine)
        ref = inversion.locate(stand_in, *picks, n_hypo=8, refine=refine)
        for a, b in zip(got[:3], ref[:3]):
            assert a.dtype == np.float64 and LC.same_bits(a, b), (a, b)
        assert set(got[3]) == set(ref[3])
        for key in ref[3]:
            assert LC.same_bits(np.asarray(got[3][key]), np.asarray(ref[3][key])), key
        assert got[3]["node"][7] == -1 and np.all(np.isnan(got[1][7]))
    assert np.max(np.linalg.norm(got[1][:7] - true, axis=1)) < 1e-3 * LC.DX and np.all(got[3]["iterations"][:7] > 0)


def _torch_device_volume(fp64):
    import torch

    dt = np.float64 if fp64 else np.float32
    run = Tape(LC.NN, dt, LC.STATIONS)
    picks = random_picks(run.T, 5, np.random.default_rng(41))
    ref = LR.grid_search(run.T, LC.NN, LR.csr_of(*picks), ((1, 8), (0, 8), (2, 9)))
    dev = torch.device("cuda", run.tape.device)
    tens = [torch.as_tensor(p, device=dev) for p in picks]
    before = run.tape.nbytes
    node, t0, mis, vol = run.tape.locate_grid(*tens, box=((1, 8), (0, 8), (2, 9)), return_misfit=True)
    assert isinstance(vol, torch.Tensor) and vol.device == dev and vol.dtype == torch.float64 and tuple(vol.shape) == ref[3].shape
    assert isinstance(node, np.ndarray) and np.array_equal(node, ref[0]) and LC.same_bits(t0, ref[1]) and LC.same_bits(mis, ref[2])
    assert LC.same_bits(vol.cpu().numpy(), ref[3])
    assert run.tape.nbytes - before < 5 * 7 * 8 * 7 * 8                  # a volume on the device is the caller's: the tape holds none


@DTYPES
def test_device_tensors_in_and_the_volume_out_on_the_device(dt):
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_locate_gpu as t; t._torch_device_volume(%r)"
            % (HERE, ROOT, dt == np.float64))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
