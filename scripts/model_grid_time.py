"""Wall time of the field tape of a coarse MODEL grid beside the node tape of the same grid.

For n^3 nodes (fp32, weno=0), events at depth, a 21 x 21 surface array of receivers per event (441 per event), per model shape:
  tape.vjp(w), tape.jvp(v), tape.gauss_newton(v)   (tiled schedule; w and v torch tensors on the device; v one value per model node)
  ten iterations of tape.solve_normal               (damped, smoothed on the axes with three model nodes or more; the relaxation
                                                    passes of its ten products are recorded beside the time)
  tape.prolong(v), tape.restrict(g)                 (P and P^T alone)
and, in the same run, the same products and the same solve on the NODE tape of the same call: the difference is the cost of P and P^T per
product, and what the solver's vectors cost at n^3 values instead of mx my mz.  Medians of --reps runs after one warm-up; one JSON line
per grid.

--only-node measures the node tape's gauss_newton alone and needs nothing of the model grid, so the same script runs against another
checkout of the package (--package-root), e.g. the parent commit before and after:

    python scripts/model_grid_time.py [--sizes 128,256] [--events 16,8] [--models 33x33x33,1x1x33] [--reps 3]
    python scripts/model_grid_time.py --only-node --package-root <checkout>
"""
import argparse
import json
import os
import sys
import time

import numpy as np


def case(n, n_ev, models, reps, only_node):
    import torch

    torch.cuda.init()   # (before the first grid: torch ships a HIP runtime of its own)
    import ttcr_amd

    dt = np.float32
    dx = 1.0
    x = np.arange(n) * dx
    s = (1.0 / (1.5 + 0.02 * x))[None, None, :] * np.ones((n, n, n))
    rng = np.random.default_rng(1)
    hi = (n - 1) * dx
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
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return dict(median_ms=round(float(np.median(ts)) * 1e3, 3), min_ms=round(min(ts) * 1e3, 3), max_ms=round(max(ts) * 1e3, 3))

    def products(tape, weights, with_maps):
        v = torch.from_numpy(rng.standard_normal(tape.n_cols).astype(dt)).cuda()
        out = dict(model_values=tape.n_cols)
        out["gauss_newton"] = timed(lambda: tape.gauss_newton(v))
        out["gauss_newton_passes"] = list(tape.passes)
        if only_node:
            return out
        out["vjp"] = timed(lambda: tape.vjp(wd))
        out["jvp"] = timed(lambda: tape.jvp(v))
        rhs = tape.vjp(wd)
        kw = dict(smooth=1e-2, smooth_weights=weights, damp=1e-1, maxiter=10, rtol=0.0)
        out["solve_normal_10"] = timed(lambda: tape.solve_normal(rhs, **kw))
        info = tape.solve_normal(rhs, return_info=True, **kw)[1]
        out["solve_passes"] = [int(sum(p[0] for p in info["passes"])), int(sum(p[1] for p in info["passes"]))]   # (jvp, vjp), summed
        if with_maps:
            g = torch.from_numpy(rng.standard_normal(tape.n_nodes).astype(dt)).cuda()
            out["prolong"] = timed(lambda: tape.prolong(v))
            out["restrict"] = timed(lambda: tape.restrict(g))
        out["field_tape_bytes"] = tape.nbytes
        tape.release_solve()
        return out

    g = ttcr_amd.Grid3d(x, x, x, n_threads=8, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, dtype=dt)
    g.set_slowness(s)
    res = dict(nodes=f"{n}^3", dtype="float32", events=n_ev, receivers_per_event=int(arr.shape[0]), only_node=only_node)
    tape = g.raytrace_adjoint(src, rcv)[1]
    res["node_tape"] = products(tape, (1., 1., 1.), False)
    tape.free()
    for m in ([] if only_node else models):
        tape = g.raytrace_adjoint(src, rcv, wrt="model", model_shape=m)[1]
        res["model_%dx%dx%d" % m] = products(tape, tuple(1.0 if k >= 3 else 0.0 for k in m), True)
        tape.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--events", default="16,8")
    ap.add_argument("--models", default="33x33x33,1x1x33")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only-node", action="store_true")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    models = [tuple(int(k) for k in m.split("x")) for m in a.models.split(",")]
    for n, e in zip([int(s) for s in a.sizes.split(",")], [int(s) for s in a.events.split(",")]):
        print(json.dumps(case(n, e, models, a.reps, a.only_node)), flush=True)


if __name__ == "__main__":
    main()
