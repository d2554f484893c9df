"""Wall time of the adjoint-state gradient (the exact discrete adjoint of the first-order solver).

For a 3-D node grid (fp32, weno=0), events at depth, a 21 x 21 surface array of receivers per event:
  plain raytrace                                   (the solves and the receiver interpolation, no derivative)
  raytrace_adjoint                                 (the same solves; fields, frozen nodes and stencils taped, coupling pass)
  tape.vjp(w) with the global Jacobi baseline and with the tiled relaxation, w a torch tensor on the device, with their pass counts
  raytrace_tape + MTape.vjp                        (the ray-frozen derivative of compute_M: a different derivative, for orientation)
and the device memory the field tape holds.  Medians of --reps runs after one warm-up; one JSON line per grid.

    python scripts/adjoint_time.py [--sizes 128,256] [--events 16,8] [--reps 3]
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

    t_plain = timed(lambda: g.raytrace(src, rcv))
    keep = {}

    def adjoint_path():
        keep["a"] = None   # (the previous tape is released first: two tapes of 256^3 x 8 need not fit side by side)
        keep["a"] = g.raytrace_adjoint(src, rcv)[1]

    t_adj = timed(adjoint_path)
    tape = keep["a"]
    out = {}

    def vjp(schedule):
        def f():
            out[schedule] = tape.vjp(wd, schedule=schedule)
            torch.cuda.synchronize()
            out[schedule + "_passes"] = tape.passes
        return f

    t_jac = timed(vjp("jacobi"))
    t_til = timed(vjp("tiled"))
    same = bool(torch.equal(out["jacobi"].view(torch.int32), out["tiled"].view(torch.int32)))
    nbytes = tape.nbytes
    keep["a"] = tape = None
    out.pop("jacobi"), out.pop("tiled")

    def mtape_path():
        keep["m"] = None
        keep["m"] = g.raytrace_tape(src, rcv)[1]

    t_mtape = timed(mtape_path)
    mt = keep["m"]

    def mvjp():
        mt.vjp(wd)
        torch.cuda.synchronize()

    t_mvjp = timed(mvjp)
    return dict(nodes=f"{n}^3", dtype="float32", events=n_ev, receivers_per_event=int(arr.shape[0]), plain_raytrace_ms=round(t_plain, 2),
                raytrace_adjoint_ms=round(t_adj, 2), vjp_jacobi_ms=round(t_jac, 2), jacobi_passes=out["jacobi_passes"],
                vjp_tiled_ms=round(t_til, 2), tiled_passes=out["tiled_passes"], tiled_bit_equal_to_jacobi=same, field_tape_bytes=nbytes,
                raytrace_tape_ms=round(t_mtape, 2), m_tape_vjp_ms=round(t_mvjp, 4))


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
