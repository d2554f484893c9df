"""Wall time of the gradient of a traveltime misfit, M^T w, through compute_M on the host against the M tape on the device.

For a 3-D node grid (fp32), events at depth, a 21 x 21 surface array of receivers per event:
  (a) raytrace(compute_M=True) + scipy M.T @ w   (host assembly of M, host product)
  (b) raytrace_tape                               (the same solves and walks, M merged and indexed on the device)
  (c) tape.vjp(w) with w a torch tensor on the device
  plain raytrace (no M) for scale, and the device memory the tape holds (tape.nbytes).
Medians of --reps runs after one warm-up; one JSON line per grid.

    python scripts/tape_time.py [--sizes 128,256] [--events 16,8] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def case(n, n_ev, reps):
    import scipy.sparse as sp
    import torch

    import ttcr_amd

    dt = np.float32
    dx = 1.0
    x = np.arange(n) * dx
    z = x
    v = (1.5 + 0.02 * z)[None, None, :] * np.ones((n, n, n))
    g = ttcr_amd.Grid3d(x, x, x, n_threads=8, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, dtype=dt)
    g.set_velocity(v.astype(dt))
    rng = np.random.default_rng(1)
    hi = (n - 1) * dx
    ev = np.column_stack([rng.uniform(0.2 * hi, 0.8 * hi, (n_ev, 2)), rng.uniform(0.5 * hi, 0.9 * hi, n_ev)])
    a = np.linspace(0.05 * hi, 0.95 * hi, 21)
    arr = np.array([[p, q, 0.0] for p in a for q in a])
    src = np.column_stack([np.repeat(np.arange(n_ev), arr.shape[0]), np.zeros(n_ev * arr.shape[0]), np.repeat(ev, arr.shape[0], axis=0)])
    rcv = np.tile(arr, (n_ev, 1))
    w = rng.standard_normal(rcv.shape[0]).astype(dt)
    wd = torch.from_numpy(w).cuda()

    def timed(f):
        f()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    def host_path():
        _, M = g.raytrace(src, rcv, compute_M=True)
        Ms = sp.vstack(M).tocsr()
        return Ms.T @ w

    t_plain = timed(lambda: g.raytrace(src, rcv))
    t_a = timed(host_path)
    keep = {}

    def tape_path():
        keep["t"] = g.raytrace_tape(src, rcv)[1]

    t_b = timed(tape_path)
    tape = keep["t"]

    def vjp():
        tape.vjp(wd)
        torch.cuda.synchronize()

    t_c = timed(vjp)
    ref = np.asarray(host_path(), dtype=np.float64)
    got = tape.vjp(wd).cpu().numpy().astype(np.float64)
    return dict(nodes=f"{n}^3", dtype="float32", events=n_ev, receivers_per_event=int(arr.shape[0]), rows=tape.n_rows, nnz=tape.nnz,
                plain_raytrace_ms=round(t_plain, 2), a_compute_M_plus_scipy_MTw_ms=round(t_a, 2), b_raytrace_tape_ms=round(t_b, 2),
                c_tape_vjp_device_ms=round(t_c, 4), tape_bytes=tape.nbytes,
                max_abs_diff_vs_scipy_fp64_product=float(np.max(np.abs(ref - got))) if ref.size else 0.0)


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
