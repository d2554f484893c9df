"""Where the arguments of the field tape's products live (FieldTape): every product gives the same bytes and the same pass
counts whether its arguments are numpy arrays, CPU tensors, CUDA tensors or one of each, returns its result where the documented argument
lives, and leaves the tape with the same nbytes.  A host argument is staged in a work array of the tape (the table above stage_in in
ttcr_amd/csrc/fsm_capi.hip); the last test runs products back to back on one tape, host and device arguments alternating, against the same
products on fresh tapes: a staging array that is not idle when the table says so shows there.

One grid of 13 x 11 x 9 nodes (more than one relaxation tile along x for the tile edges of both dtypes, the last tile ragged), velocity
linear in z plus noise, three events -- the second with two source points --, seven receivers each with one position repeated, the data
rows of the events interleaved and two data rows that belong to no event.  fp32 and fp64, node tape and cell tape, both schedules.
What the products compute is held by the other field-tape tests; here only residency varies."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from field_tape_cases import _bits_equal  # noqa: E402

NN, DX = (13, 11, 9), 0.5
K_BLOCK = 5   # two groups of the block products, the last one padded
SCHEDULES = ("tiled", "jacobi")
MODES = ("cpu", "cuda", "numpy+cuda", "cuda+numpy")   # each against "numpy"


def _in_child(fn, *args):
    """Run _torch_<fn>(*args) of this module in a fresh process that initialises torch's device before the first grid (torch ships a HIP
    runtime of its own)"""
    code = ("import sys, torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; import test_field_tape_residency_gpu as t; t._torch_%s(*%r)"
            % (HERE, ROOT, fn, args))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


class Setup:
    """the grid, the events and the arguments of every product for one dtype and one kind of tape; tape() makes a fresh tape"""

    def __init__(self, flat, wrt):
        import ttcr_amd

        self.dt = dt = np.float32 if flat == "fp32" else np.float64
        self.wrt = wrt
        cells = wrt == "cells"
        rng = np.random.default_rng(97)
        shape = tuple(n - 1 for n in NN) if cells else NN
        z = DX * (np.arange(shape[2]) + (0.5 if cells else 0.0))
        vel = (1.5 + 0.25 * z)[None, None, :] * np.ones(shape) + 0.1 * rng.uniform(-1, 1, shape)
        self.grid = ttcr_amd.Grid3d(*[np.arange(n) * DX for n in NN], cell_slowness=int(cells), method="FSM", dtype=dt, weno=0,
                                    tt_from_rp=0, n_threads=2)
        self.grid.set_slowness(1.0 / vel)
        hi = (np.array(NN) - 1) * DX
        self.pts = [np.array([[1.3, 2.1, 0.7]]), np.array([[4.9, 0.4, 3.1], [5.3, 4.2, 1.0]]), np.array([[2.0, 3.5, 3.0]])]
        self.t0 = [np.array([0.125]), np.array([0.0, 0.25]), np.array([0.5])]
        rcv = []
        for e in range(3):
            r = rng.uniform(0.1, hi - 0.1, (7, 3))
            r[6] = r[2]   # (one position twice)
            rcv.append(r)
        self.rcv = rcv
        self.n_data = 23
        rows = rng.permutation(self.n_data)
        self.rows = [np.sort(rows[7 * e:7 * e + 7]) for e in range(3)]   # rows 21, 22 of the permutation: on no event
        n_model = int(np.prod(shape))
        n_nodes = int(np.prod(NN))
        s = (1.0 / vel).flatten("F")
        self.w = rng.standard_normal(self.n_data).astype(dt)
        self.fc = rng.standard_normal((3, n_nodes)).astype(dt)
        self.ds = (s * rng.standard_normal(n_model)).astype(dt)
        self.rw = rng.uniform(0.5, 2.0, self.n_data).astype(dt)
        self.dsrc = rng.standard_normal((3, 4, 4)).astype(dt)   # (K = 3 perturbations of the 4 points)
        self.ds_k = (s * rng.standard_normal((K_BLOCK, n_model))).astype(dt)
        self.w_k = rng.standard_normal((K_BLOCK, self.n_data)).astype(dt)
        self.rw_k = rng.uniform(0.5, 2.0, (K_BLOCK, self.n_data)).astype(dt)

    def tape(self):
        import ctypes as C

        from ttcr_amd import _lib
        from ttcr_amd.rgrid import FieldTape, _ptr

        g = self.grid
        tx_off, tx, t0, rx_off, rx, out = g._event_arrays(self.pts, self.t0, self.rcv)
        h = C.c_void_p()
        entry = g._lib.ttcr_fsm_raytrace_multi_adjoint_cells if self.wrt == "cells" else g._lib.ttcr_fsm_raytrace_multi_adjoint
        _lib.check(entry(g._h, 3, _ptr(tx_off), _ptr(tx), _ptr(t0), _ptr(rx_off), _ptr(rx), _ptr(out), C.byref(h)))
        tape = FieldTape(g._lib, h, self.dt, np.concatenate(self.rows).astype(np.int64), self.n_data)
        assert (tape.n_events, tape.n_rows, tape.n_data, tape.n_points, tape.wrt) == (3, 21, 23, 4, self.wrt)
        assert tape.n_nodes == int(np.prod(NN)) and tape.n_cols == self.ds.size
        return tape


def _place(a, where, device):
    import torch

    if a is None or where == "numpy":
        return a
    t = torch.from_numpy(a.copy())
    return t.to(device) if where == "cuda" else t


def _products(s):
    """(name, method, arguments by name, keywords, which argument the result lives with: 'first' or 'first tensor') of every product, in
    the order they run on a tape; hvp and newton follow the hold"""
    out = []
    for sch in SCHEDULES:
        kw = dict(schedule=sch)
        out += [
            ("vjp w", "vjp", [s.w, None], kw, "first tensor"),
            ("vjp fc", "vjp", [None, s.fc], kw, "first tensor"),
            ("vjp w fc", "vjp", [s.w, s.fc], kw, "first tensor"),
            ("vjp w fc gsrc", "vjp", [s.w, s.fc], dict(kw, return_source_grad=True), "first tensor"),
            ("jvp", "jvp", [s.ds], kw, "first"),
            ("jvp fields", "jvp", [s.ds], dict(kw, return_fields=True), "first"),
            ("jvp_source", "jvp_source", [s.dsrc[0]], dict(kw, return_fields=True), "first"),
            ("jvp_source K", "jvp_source", [s.dsrc], dict(kw, return_fields=True), "first"),
            ("gauss_newton", "gauss_newton", [s.ds, None], kw, "first tensor"),
            ("gauss_newton rw", "gauss_newton", [s.ds, s.rw], kw, "first tensor"),
            ("hold", "hold", [s.w, s.fc], dict(kw, return_grad=True), "first"),
            ("hvp", "hvp", [s.ds], kw, "first"),
            ("newton", "newton", [s.ds, s.rw], kw, "first"),
            ("jvp_block", "jvp_block", [s.ds_k], dict(kw, return_fields=True), "first"),
            ("vjp_block", "vjp_block", [s.w_k], kw, "first"),
            ("gauss_newton_block", "gauss_newton_block", [s.ds_k, None], kw, "first"),
            ("gauss_newton_block rw", "gauss_newton_block", [s.ds_k, s.rw], kw, "first"),
            ("gauss_newton_block rw K", "gauss_newton_block", [s.ds_k, s.rw_k], kw, "first"),
        ]
    return [(("%s [%s]" % (p[0], p[3]["schedule"]),) + p[1:]) for p in out]


def _run(tape, s, mode, device):
    """every product on `tape` with its arguments placed by `mode`: [(name, results as numpy arrays, passes)], the containers checked"""
    import torch

    where = mode.split("+") if "+" in mode else [mode, mode]
    done = []
    for name, method, args, kw, lives in _products(s):
        given = [k for k, a in enumerate(args) if a is not None]
        placed = list(args)
        for n, k in enumerate(given):   # (the first argument given and the second; a lone argument goes where the first would)
            placed[k] = _place(args[k], where[min(n, 1)], device)
        res = getattr(tape, method)(*placed, **kw)
        res = res if isinstance(res, tuple) else (res,)
        tensors = [placed[k] for k in given if isinstance(placed[k], torch.Tensor)]
        like = placed[given[0]] if lives == "first" or not tensors else tensors[0]
        for r in res:
            if isinstance(like, torch.Tensor):
                assert isinstance(r, torch.Tensor) and r.device == like.device, (name, mode, type(r), getattr(r, "device", None))
            else:
                assert isinstance(r, np.ndarray), (name, mode, type(r))
        done.append((name, [r.cpu().numpy() if isinstance(r, torch.Tensor) else r for r in res], tape.passes))
    return done


def _torch_residency(flat, wrt):
    import torch

    s = Setup(flat, wrt)
    tape = s.tape()
    device = torch.device("cuda", tape.device)
    base = _run(tape, s, "numpy", device)
    nbytes = tape.nbytes
    for name, res, passes in base:
        assert all(r.dtype == s.dt and np.all(np.isfinite(r)) and np.any(r != 0) for r in res), name
        assert passes >= 1 if isinstance(passes, int) else min(passes) >= 1, (name, passes)
    for mode in MODES:
        tape = s.tape()
        got = _run(tape, s, mode, device)
        assert [g[0] for g in got] == [b[0] for b in base]
        for (name, res, passes), (_, res0, passes0) in zip(got, base):
            assert passes == passes0 and type(passes) is type(passes0), (name, mode, passes, passes0)
            assert len(res) == len(res0), (name, mode)
            for r, r0 in zip(res, res0):
                _bits_equal(r, r0)
        assert tape.nbytes == nbytes, (mode, tape.nbytes, nbytes)


def _torch_call_order(flat):
    """one tape, products back to back, host and device arguments alternating; each result against the same product on a fresh tape"""
    import torch

    s = Setup(flat, "nodes")
    tape = s.tape()
    device = torch.device("cuda", tape.device)
    cuda = lambda a: _place(a, "cuda", device)   # noqa: E731
    steps = [
        ("hold", [cuda(s.w), None], dict(return_grad=True)),                        # device
        ("vjp", [None, s.fc], {}),                                                   # host field cotangent (lam2)
        ("gauss_newton", [cuda(s.ds), cuda(s.rw)], {}),                              # device
        ("gauss_newton", [s.ds, s.rw], {}),                                          # host v (model_tmp), host row_weight (rw_tmp)
        ("jvp", [cuda(s.ds)], dict(return_fields=True, schedule="jacobi")),          # device
        ("jvp", [s.ds], dict(return_fields=True, schedule="jacobi")),                # host fields (lam / lam2 by parity)
        ("newton", [s.ds, cuda(s.rw)], {}),                                          # v numpy (model_tmp, in and out)
        ("vjp_block", [cuda(s.w_k)], {}),                                            # device
        ("vjp_block", [s.w_k], {}),                                                  # host (blk_rows, blk_model)
        ("vjp", [s.w, s.fc], {}),                                                    # host again, after the block arrays came
    ]
    for n, (method, args, kw) in enumerate(steps):
        res = getattr(tape, method)(*args, **kw)
        passes = tape.passes
        fresh = s.tape()
        if method == "newton":
            fresh.hold(s.w)
        ref = getattr(fresh, method)(*args, **kw)
        assert passes == fresh.passes, (n, method, passes, fresh.passes)
        res, ref = (r if isinstance(r, tuple) else (r,) for r in (res, ref))
        for r, r0 in zip(res, ref):
            assert type(r) is type(r0), (n, method)
            r, r0 = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (r, r0))
            assert np.any(r != 0), (n, method)
            _bits_equal(r, r0)


@pytest.mark.parametrize("wrt", ["nodes", "cells"])
@pytest.mark.parametrize("flat", ["fp32", "fp64"])
def test_results_do_not_depend_on_where_the_arguments_live(flat, wrt):
    _in_child("residency", flat, wrt)


@pytest.mark.parametrize("flat", ["fp32", "fp64"])
def test_products_back_to_back_on_one_tape(flat):
    _in_child("call_order", flat)
