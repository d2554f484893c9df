"""Wall time of FieldTape.solve_normal beside the Gauss-Newton products it is made of and beside the same loop written
with torch operations around tape.gauss_newton.

For a 3-D node grid (fp32, weno=0), events at depth, a 21 x 21 surface array of receivers per event, on one field tape, device tensors,
--iters iterations of conjugate gradients on (J^T W J + smooth R + damp I) x = b with smooth > 0 and damp > 0, rtol = 0 (no early stop):
  solve          one call of tape.solve_normal(b, row_weight, smooth, damp, maxiter=iters, rtol=0)
  products       iters calls of tape.gauss_newton(v, row_weight) in a row: what the solve cannot avoid
  torch_loop     the loop a user would otherwise write: tape.gauss_newton and tape.smooth for the operator, torch for the vector
                 updates and the inner products (torch.dot, .item() for every scalar)
The cost the solver adds per iteration is (solve - products) / iters, a difference of two numbers measured in the same run.  Per figure:
--warmup calls that are not timed, then the median of --reps (at least 5) timed calls and their spread (max - min), in ms.  The solve and
the torch loop sum in different orders, so their iterates differ in the last bits; the relative difference of the two results is
printed, not asserted.  One JSON line per grid.

    python scripts/normal_solve_time.py [--sizes 128,256] [--events 16,8] [--iters 10] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case(n, n_ev, iters, reps, warmup):
    import torch

    torch.cuda.init()   # (before the first grid: torch ships a HIP runtime of its own)
    import ttcr_amd

    dt = np.float32
    dx = 1.0
    x = np.arange(n) * dx
    v = (1.5 + 0.02 * x)[None, None, :] * np.ones((n, n, n))
    g = ttcr_amd.Grid3d(x, x, x, n_threads=8, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, dtype=dt)
    g.set_velocity(v.astype(dt))
    rng = np.random.default_rng(1)
    hi = (n - 1) * dx
    ev = np.column_stack([rng.uniform(0.2 * hi, 0.8 * hi, (n_ev, 2)), rng.uniform(0.5 * hi, 0.9 * hi, n_ev)])
    a = np.linspace(0.05 * hi, 0.95 * hi, 21)
    arr = np.array([[p, q, 0.0] for p in a for q in a])
    src = np.column_stack([np.repeat(np.arange(n_ev), arr.shape[0]), np.zeros(n_ev * arr.shape[0]), np.repeat(ev, arr.shape[0], axis=0)])
    rcv = np.tile(arr, (n_ev, 1))
    tape = g.raytrace_adjoint(src, rcv)[1]
    rw = torch.from_numpy(rng.uniform(0.5, 2.0, rcv.shape[0]).astype(dt)).cuda()
    b = tape.vjp(torch.from_numpy(rng.standard_normal(rcv.shape[0]).astype(dt)).cuda())
    smooth, damp = 1e-2, 1e-1

    def timed(f):
        for _ in range(warmup):
            f()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return dict(median_ms=round(float(np.median(ts)), 2), spread_ms=round(float(max(ts) - min(ts)), 2))

    def solve():
        return tape.solve_normal(b, row_weight=rw, smooth=smooth, damp=damp, maxiter=iters, rtol=0.0, return_info=True)

    def products():
        for _ in range(iters):
            tape.gauss_newton(b, rw)

    def torch_loop():
        x_ = torch.zeros_like(b)
        r = b.clone()
        p = r.clone()
        rho = torch.dot(r, r).item()
        for _ in range(iters):
            q = tape.gauss_newton(p, rw) + smooth * tape.smooth(p) + damp * p
            alpha = rho / torch.dot(p, q).item()
            x_ += alpha * p
            r -= alpha * q
            rho_new = torch.dot(r, r).item()
            p = r + (rho_new / rho) * p
            rho = rho_new
        return x_

    res = dict(nodes=f"{n}^3", dtype="float32", events=n_ev, receivers_per_event=int(arr.shape[0]), iterations=iters, smooth=smooth,
               damp=damp, reps=reps, warmup=warmup, build_id=ttcr_amd._lib.build_id())
    # alternating order: products, solve, torch loop, then products again
    res["products_before"] = timed(products)
    res["solve"] = timed(solve)
    res["torch_loop"] = timed(torch_loop)
    res["products_after"] = timed(products)
    xs, info = solve()
    xt = torch_loop()
    res["solve_status"], res["solve_iterations"] = info["status"], info["iterations"]
    res["passes_per_iteration"] = info["passes"]
    res["residual_reduction"] = float(np.sqrt(info["rho"][-1] / info["rho"][0]))
    res["solve_vs_torch_loop_rel_diff"] = float((torch.linalg.norm((xs - xt).double()) / torch.linalg.norm(xt.double())).item())
    prod = 0.5 * (res["products_before"]["median_ms"] + res["products_after"]["median_ms"])
    res["added_per_iteration_ms"] = dict(solve=round((res["solve"]["median_ms"] - prod) / iters, 3),
                                         torch_loop=round((res["torch_loop"]["median_ms"] - prod) / iters, 3))
    res["field_tape_bytes_with_solver_arrays"] = tape.nbytes
    tape.release_solve()
    res["field_tape_bytes"] = tape.nbytes
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--events", default="16,8")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    sys.path.insert(0, HERE)
    for n, e in zip([int(s) for s in a.sizes.split(",")], [int(s) for s in a.events.split(",")]):
        print(json.dumps(case(n, e, a.iters, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
