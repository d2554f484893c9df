"""Wall time of the field tape's receiver-point calls beside the calls they extend, in the reciprocal layout.

For a 3-D node grid (fp32, weno=0): n_fields stations near the surface are the sources of the call, 441 hypocentres at depth are its
receivers -- every field sees all of them, so the 441 n_fields rows are grouped into 441 receiver points --, on one field tape, device
tensors:
  gn                  one tape.gauss_newton(v, row_weight): what the receiver block is added to; timed before and after gn_receiver_joint
  gn_receiver_joint   one tape.gauss_newton_receiver_joint(v, v_rcv, row_weight, rcv_scale)
  solve               one tape.solve_receiver_joint(..., maxiter=iters, rtol=0)
  products            iters calls of tape.gauss_newton_receiver_joint in a row: what the solve cannot avoid; timed before and after it
  receiver_eval       tape.receiver_eval of 10^5 points inside the grid, events dealt in turn (traveltime and gradient)
  solve_joint         one tape.solve_joint(..., maxiter=iters, rtol=0) of the same tape (the sources are the stations here): an existing
                      entry, timed with gn to show that the existing entries did not move
On a build without the receiver calls only gn and solve_joint are timed (the same script at the parent commit).  What is to be read off:
what the receiver block adds to gauss_newton, and whether that is resolved above the spreads.  Per figure: --warmup calls that are not
timed, then the median of --reps (at least 5) timed calls and their spread (max - min), in ms.  One JSON line per grid.

    python scripts/receiver_time.py [--sizes 128,256] [--fields 16,8] [--iters 10] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case(n, n_fields, iters, reps, warmup):
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
    stations = np.column_stack([rng.uniform(0.05 * hi, 0.95 * hi, (n_fields, 2)), rng.uniform(0.0, 0.02 * hi, n_fields)])
    hyp = np.column_stack([rng.uniform(0.2 * hi, 0.8 * hi, (441, 2)), rng.uniform(0.5 * hi, 0.9 * hi, 441)]).astype(dt).astype(np.float64)
    src = np.column_stack([np.repeat(np.arange(n_fields), 441), np.zeros(n_fields * 441), np.repeat(stations, 441, axis=0)])
    rcv = np.tile(hyp, (n_fields, 1))
    tape = g.raytrace_adjoint(src, rcv)[1]
    dev = lambda h: torch.from_numpy(np.ascontiguousarray(h, dtype=dt)).cuda()   # noqa: E731
    rw = dev(rng.uniform(0.5, 2.0, rcv.shape[0]))
    w = dev(rng.standard_normal(rcv.shape[0]))
    scale = (1.0, 0.05, 0.05, 0.05)
    rdamp = (1e-2, 1e-1, 1e-1, 1e-1)
    smooth, damp = 1e-2, 1e-1
    have = hasattr(tape, "gauss_newton_receiver_joint")

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

    res = dict(nodes=f"{n}^3", dtype="float32", fields=n_fields, rows_per_field=441, iterations=iters, smooth=smooth, damp=damp,
               reps=reps, warmup=warmup, build_id=ttcr_amd._lib.build_id(), receiver_calls=have)
    b, b_src = tape.vjp(w, return_source_grad=True)

    def gn():
        return tape.gauss_newton(b, rw)

    def solve_joint():
        return tape.solve_joint(b, b_src, row_weight=rw, smooth=smooth, damp=damp, source_damp=rdamp, source_scale=scale, maxiter=iters,
                                rtol=0.0, return_info=True)

    res["gn_before"] = timed(gn)
    if have:
        tape.set_receiver_points(np.tile(np.arange(441), n_fields))
        res["receiver_points"] = tape.n_rcv_points
        b_rcv = tape.vjp(w, return_receiver_grad=True)[1]

        def gn_rj():
            return tape.gauss_newton_receiver_joint(b, b_rcv, rw, scale)

        def products():
            for _ in range(iters):
                gn_rj()

        def solve():
            return tape.solve_receiver_joint(b, b_rcv, row_weight=rw, smooth=smooth, damp=damp, rcv_damp=rdamp, rcv_scale=scale,
                                             maxiter=iters, rtol=0.0, return_info=True)

        pts = dev(np.column_stack([rng.uniform(0.0, hi, (100000, 2)), rng.uniform(0.0, hi, 100000)]))
        ev = np.arange(100000) % n_fields
        res["gn_receiver_joint"] = timed(gn_rj)
        res["gn_after"] = timed(gn)
        res["products_before"] = timed(products)
        res["solve"] = timed(solve)
        res["products_after"] = timed(products)
        res["receiver_eval_1e5"] = timed(lambda: tape.receiver_eval(pts, ev))
        info = solve()[2]
        res["solve_status"], res["solve_iterations"] = info["status"], info["iterations"]
        res["residual_reduction"] = float(np.sqrt(info["rho"][-1] / info["rho"][0]))
        gn_ms = 0.5 * (res["gn_before"]["median_ms"] + res["gn_after"]["median_ms"])
        prod = 0.5 * (res["products_before"]["median_ms"] + res["products_after"]["median_ms"])
        res["receiver_block_adds_ms"] = round(res["gn_receiver_joint"]["median_ms"] - gn_ms, 2)
        res["solve_adds_per_iteration_ms"] = round((res["solve"]["median_ms"] - prod) / iters, 3)
        res["field_tape_bytes_with_receiver_arrays"] = tape.nbytes
        tape.release_receiver()
    else:
        res["gn_after"] = timed(gn)
    res["solve_joint"] = timed(solve_joint)
    tape.release_joint()
    res["field_tape_bytes"] = tape.nbytes
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--fields", default="16,8")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    sys.path.insert(0, HERE)
    for n, e in zip([int(s) for s in a.sizes.split(",")], [int(s) for s in a.fields.split(",")]):
        print(json.dumps(case(n, e, a.iters, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
