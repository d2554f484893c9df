"""Wall time of the forward mode of the field tape (J v and the Gauss-Newton product).

For a 3-D node grid (fp32, weno=0), events at depth, a 21 x 21 surface array of receivers per event, on one field tape:
  tape.vjp(w) with the tiled relaxation            (J^T w: the orientation figure, J and J^T do the same amount of arithmetic)
  tape.jvp(v) with the global Jacobi baseline and with the tiled relaxation, with their pass counts, and whether the two are bit-equal
  tape.gauss_newton(v, row_weight)                 (J^T W J v: jvp, row scaling and vjp on the tape's stream)
v, w and row_weight are torch tensors on the device.  Medians of --reps runs after one warm-up; one JSON line per grid.

    python scripts/tangent_time.py [--sizes 128,256] [--events 16,8] [--reps 3]
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

    def vjp():
        out["vjp"] = tape.vjp(wd)
        torch.cuda.synchronize()
        out["vjp_passes"] = tape.passes

    def jvp(schedule):
        def f():
            out[schedule] = tape.jvp(vd, schedule=schedule)
            torch.cuda.synchronize()
            out[schedule + "_passes"] = tape.passes
        return f

    def gn():
        out["gn"] = tape.gauss_newton(vd, rwd)
        torch.cuda.synchronize()
        out["gn_passes"] = tape.passes

    t_vjp = timed(vjp)
    t_jac = timed(jvp("jacobi"))
    t_til = timed(jvp("tiled"))
    t_gn = timed(gn)
    same = bool(torch.equal(out["jacobi"].view(torch.int32), out["tiled"].view(torch.int32)))
    gn_same = bool(torch.equal(out["gn"].view(torch.int32), tape.vjp(rwd * out["tiled"]).view(torch.int32)))
    return dict(nodes=f"{n}^3", dtype="float32", events=n_ev, receivers_per_event=int(arr.shape[0]), vjp_tiled_ms=round(t_vjp, 2),
                vjp_tiled_passes=out["vjp_passes"], jvp_jacobi_ms=round(t_jac, 2), jvp_jacobi_passes=out["jacobi_passes"],
                jvp_tiled_ms=round(t_til, 2), jvp_tiled_passes=out["tiled_passes"], jvp_tiled_bit_equal_to_jacobi=same,
                gauss_newton_ms=round(t_gn, 2), gauss_newton_passes=list(out["gn_passes"]),
                gauss_newton_bit_equal_to_vjp_of_jvp=gn_same, field_tape_bytes=tape.nbytes)


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
