"""Wall time of the field tape's derivatives with respect to the source points.

For a 3-D node grid (fp32, weno=0), events at depth, a 21 x 21 surface array of receivers per event, on one field tape:
  tape.source_jacobian()                           (one K = 4 relaxation) with the tiled relaxation and with the global Jacobi baseline,
                                                   with their pass counts, and whether the two are bit-equal
  four tape.jvp_source calls of one column each    (four K = 1 relaxations: what the K = 4 kernel is to beat), and whether the columns
                                                   are bit-equal to those of the K = 4 call
  tape.jvp(v) and tape.vjp(w)                      (the orientation figures: one relaxation each)
  tape.vjp(w, return_source_grad=True)             (the same relaxation and the source-gradient kernel)
Inputs are torch tensors on the device where the call takes them.  Medians of --reps runs after one warm-up; one JSON line per grid.

    python scripts/source_time.py [--sizes 128,256] [--events 16,8] [--reps 3]
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
    units = torch.zeros((4, tape.n_points, 4), dtype=torch.float32, device="cuda")
    for k in range(4):
        units[k, :, k] = 1
    out = {}

    def jac(schedule):
        def f():
            out[schedule] = tape.source_jacobian(schedule=schedule)
            out[schedule + "_passes"] = tape.passes
        return f

    def four():
        out["four"] = torch.stack([tape.jvp_source(units[k]) for k in range(4)], dim=1)
        torch.cuda.synchronize()
        out["four_passes"] = tape.passes

    def jvp():
        out["jvp"] = tape.jvp(vd)
        torch.cuda.synchronize()

    def vjp(source_grad):
        def f():
            out["vjp%d" % source_grad] = tape.vjp(wd, return_source_grad=source_grad)
            torch.cuda.synchronize()
        return f

    t_til = timed(jac("tiled"))
    t_jac = timed(jac("jacobi"))
    t_four = timed(four)
    t_jvp = timed(jvp)
    t_vjp = timed(vjp(False))
    t_vjps = timed(vjp(True))
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)   # noqa: E731
    same = bool(np.array_equal(bits(out["tiled"]), bits(out["jacobi"])))
    same4 = bool(np.array_equal(bits(out["tiled"]), bits(out["four"].cpu().numpy())))
    grad_same = bool(torch.equal(out["vjp0"].view(torch.int32), out["vjp1"][0].view(torch.int32)))
    return dict(nodes=f"{n}^3", dtype="float32", events=n_ev, receivers_per_event=int(arr.shape[0]),
                source_jacobian_tiled_ms=round(t_til, 2), source_jacobian_tiled_passes=out["tiled_passes"],
                source_jacobian_jacobi_ms=round(t_jac, 2), source_jacobian_jacobi_passes=out["jacobi_passes"],
                source_jacobian_tiled_bit_equal_to_jacobi=same, four_jvp_source_ms=round(t_four, 2),
                four_jvp_source_passes_of_the_last=out["four_passes"], four_columns_bit_equal_to_four_calls=same4,
                jvp_tiled_ms=round(t_jvp, 2), vjp_tiled_ms=round(t_vjp, 2), vjp_with_source_grad_ms=round(t_vjps, 2),
                vjp_grad_bit_equal=grad_same, field_tape_bytes=tape.nbytes)


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
