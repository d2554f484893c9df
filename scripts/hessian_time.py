"""Wall time of the second-order products of the field tape beside the Gauss-Newton product.

For a 3-D node grid (fp32, weno=0), events at depth, a 21 x 21 surface array of receivers per event, on one field tape, in one run:
  tape.hold(w)                         (one adjoint relaxation; lam stays on the tape)
  tape.hvp(v)                          (tangent relaxation, dD and q, adjoint relaxation, gradient with the direct term)
  tape.newton(v, row_weight)           (J^T W J v + hvp(v) from one adjoint relaxation)
  tape.gauss_newton(v, row_weight)     (J^T W J v: the figure newton is compared with)
with their pass counts, whether hvp is bit-equal under the two schedules, and the bytes hold adds.  v, w and row_weight are torch
tensors on the device.  Medians of --reps runs after one warm-up; one JSON line per grid.

    python scripts/hessian_time.py [--sizes 128,256] [--events 16,8] [--reps 3]
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
    wd = torch.from_numpy(rng.standard_normal(rcv.shape[0]).astype(dt)).cuda()
    rwd = torch.from_numpy(rng.uniform(0.5, 2.0, rcv.shape[0]).astype(dt)).cuda()
    vd = torch.from_numpy((rng.standard_normal(n ** 3) / v.flatten("F") ** 2).astype(dt)).cuda()

    def timed(f):
        f()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    tape = g.raytrace_adjoint(src, rcv)[1]
    out = {}

    def hold():
        tape.hold(wd)
        torch.cuda.synchronize()
        out["hold_passes"] = tape.passes

    def hvp(schedule):
        def f():
            out["hvp_" + schedule] = tape.hvp(vd, schedule=schedule)
            torch.cuda.synchronize()
            out["hvp_" + schedule + "_passes"] = tape.passes
        return f

    def newton():
        out["newton"] = tape.newton(vd, rwd)
        torch.cuda.synchronize()
        out["newton_passes"] = tape.passes

    def gn():
        out["gn"] = tape.gauss_newton(vd, rwd)
        torch.cuda.synchronize()
        out["gn_passes"] = tape.passes

    tape.jvp(vd)   # (the lists of the forward mode are allocated once, outside the timings and the byte counts)
    before = tape.nbytes
    t_hold = timed(hold)
    held = tape.nbytes - before
    t_gn = timed(gn)
    t_hvp = timed(hvp("tiled"))
    t_newton = timed(newton)
    t_gn2 = timed(gn)
    hvp("jacobi")()
    same = bool(torch.equal(out["hvp_jacobi"].view(torch.int32), out["hvp_tiled"].view(torch.int32)))
    return dict(nodes=f"{n}^3", dtype="float32", events=n_ev, receivers_per_event=int(arr.shape[0]), hold_ms=round(t_hold, 2),
                hold_passes=out["hold_passes"], hvp_ms=round(t_hvp, 2), hvp_passes=list(out["hvp_tiled_passes"]),
                newton_ms=round(t_newton, 2), newton_passes=list(out["newton_passes"]),
                gauss_newton_ms=[round(t_gn, 2), round(t_gn2, 2)], gauss_newton_passes=list(out["gn_passes"]),
                hvp_tiled_bit_equal_to_jacobi=same, held_bytes=held, field_tape_bytes=tape.nbytes)


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
