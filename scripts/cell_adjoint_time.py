"""Wall time of the field tape of a 3-D CELL grid beside the node tape of the same node count.

For n^3 cells (fp32, weno=0), events at depth, a 21 x 21 surface array of receivers per event:
  raytrace_adjoint(wrt='cells')                    (the solves; fields, frozen nodes and stencils taped, coupling pass)
  tape.vjp(w), tape.jvp(ds), tape.gauss_newton(v)  (tiled schedule; w, ds and v torch tensors on the device; ds and v one value per cell)
and, in the same run, the same four on a NODE grid of (n + 1)^3 nodes whose slowness is the cell model averaged onto the nodes (the
fields of the two grids are the same): the difference is the cost of A (fsm_cells_to_nodes3d) and A^T (one thread per cell) per product.
Medians of --reps runs after one warm-up; one JSON line per grid.

    python scripts/cell_adjoint_time.py [--sizes 128,256] [--events 16,8] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def case(n, n_ev, reps):
    import torch

    torch.cuda.init()   # (before the first grid: torch ships a HIP runtime of its own)
    import ttcr_amd

    dt = np.float32
    dx = 1.0
    x = np.arange(n + 1) * dx                                  # n cells, n + 1 nodes per axis
    zc = (np.arange(n) + 0.5) * dx
    vc = ((1.5 + 0.02 * zc)[None, None, :] * np.ones((n, n, n))).astype(dt)
    rng = np.random.default_rng(1)
    hi = n * dx
    ev = np.column_stack([rng.uniform(0.2 * hi, 0.8 * hi, (n_ev, 2)), rng.uniform(0.5 * hi, 0.9 * hi, n_ev)])
    a = np.linspace(0.05 * hi, 0.95 * hi, 21)
    arr = np.array([[p, q, 0.0] for p in a for q in a])
    src = np.column_stack([np.repeat(np.arange(n_ev), arr.shape[0]), np.zeros(n_ev * arr.shape[0]), np.repeat(ev, arr.shape[0], axis=0)])
    rcv = np.tile(arr, (n_ev, 1))
    wd = torch.from_numpy(rng.standard_normal(rcv.shape[0]).astype(dt)).cuda()

    def timed(f):
        f()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    def products(g, wrt):
        keep = {}

        def adjoint_path():
            keep["a"] = None   # (the previous tape is released first: two tapes of 256^3 x 8 need not fit side by side)
            keep["a"] = g.raytrace_adjoint(src, rcv, wrt=wrt)[1]

        t_adj = timed(adjoint_path)
        tape = keep["a"]
        v = torch.from_numpy(rng.standard_normal(tape.n_cols).astype(dt)).cuda()
        res = {}

        def call(name, f):
            def run():
                f()
                torch.cuda.synchronize()
                res[name + "_passes"] = tape.passes
            return timed(run)

        out = dict(raytrace_adjoint_ms=round(t_adj, 2), vjp_ms=round(call("vjp", lambda: tape.vjp(wd)), 2),
                   jvp_ms=round(call("jvp", lambda: tape.jvp(v)), 2), gauss_newton_ms=round(call("gn", lambda: tape.gauss_newton(v)), 2),
                   vjp_passes=res["vjp_passes"], jvp_passes=res["jvp_passes"], model_values=tape.n_cols, field_tape_bytes=tape.nbytes)
        keep["a"] = tape = None
        return out

    gc = ttcr_amd.Grid3d(x, x, x, n_threads=8, cell_slowness=1, method="FSM", tt_from_rp=0, weno=0, dtype=dt)
    gc.set_velocity(vc)
    cells = products(gc, "cells")
    sn = gc.get_slowness()   # the node slowness the cell grid solved with, (nx, ny, nz)
    del gc
    gn = ttcr_amd.Grid3d(x, x, x, n_threads=8, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, dtype=dt)
    gn.set_slowness(sn)
    nodes = products(gn, "nodes")
    return dict(cells=f"{n}^3", nodes=f"{n + 1}^3", dtype="float32", events=n_ev, receivers_per_event=int(arr.shape[0]), cell_tape=cells,
                node_tape=nodes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--events", default="16,8")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for n, e in zip([int(s) for s in a.sizes.split(",")], [int(s) for s in a.events.split(",")]):
        print(json.dumps(case(n, e, a.reps)), flush=True)


if __name__ == "__main__":
    main()
