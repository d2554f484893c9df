"""Wall time of the block products of the field tape (jvp_block, vjp_block, gauss_newton_block) beside the one-column
products they replace.

For a 3-D node grid (fp32, weno=0), events at depth, a 21 x 21 surface array of receivers per event, on one field tape, device tensors:
  one call of tape.jvp / tape.vjp / tape.gauss_newton                              (the one-column products)
  for K in --cols: K such calls in a row, and one call of tape.jvp_block / vjp_block / gauss_newton_block on the same K columns,
  with whether every column of the block result has the bits of its one-column call.
Per figure: --warmup calls that are not timed, then the median of --reps (at least 5) timed calls and their spread (max - min), in ms.
The yardstick for a block product is K times the one-column time of the build it is compared with: --one-column-only times the one-column
products alone, and --root names another checkout (the parent commit's, built) whose package is measured instead of this one.
One JSON line per grid.

    python scripts/block_time.py [--sizes 128,256] [--events 16,8] [--cols 4,8] [--reps 5] [--warmup 2] [--one-column-only] [--root DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case(n, n_ev, cols, reps, warmup, one_column_only):
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
    kmax = max(cols)
    wd = torch.from_numpy(rng.standard_normal((kmax, rcv.shape[0])).astype(dt)).cuda()
    rwd = torch.from_numpy(rng.uniform(0.5, 2.0, rcv.shape[0]).astype(dt)).cuda()
    vd = torch.from_numpy((rng.standard_normal((kmax, n ** 3)) / v.flatten("F") ** 2).astype(dt)).cuda()

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

    tape = g.raytrace_adjoint(src, rcv)[1]
    one = {"jvp": lambda k: tape.jvp(vd[k]), "vjp": lambda k: tape.vjp(wd[k]), "gauss_newton": lambda k: tape.gauss_newton(vd[k], rwd)}
    res = dict(nodes=f"{n}^3", dtype="float32", events=n_ev, receivers_per_event=int(arr.shape[0]), reps=reps, warmup=warmup,
               build_id=ttcr_amd._lib.build_id(), package=os.path.dirname(os.path.abspath(ttcr_amd.__file__)), one_column={})
    for name, f in one.items():
        res["one_column"][name] = timed(lambda: f(0))
        res["one_column"][name]["passes"] = tape.passes
    if not one_column_only:
        block = {"jvp": lambda K: tape.jvp_block(vd[:K]), "vjp": lambda K: tape.vjp_block(wd[:K]),
                 "gauss_newton": lambda K: tape.gauss_newton_block(vd[:K], rwd)}
        for K in cols:
            r = res["K=%d" % K] = {}
            for name in one:
                r[name] = dict(one_column_calls=timed(lambda: [one[name](k) for k in range(K)]), block=timed(lambda: block[name](K)))
                r[name]["block"]["passes"] = tape.passes
                out = block[name](K)
                r[name]["block_bit_equal_to_one_column"] = all(
                    bool(torch.equal(out[k].view(torch.int32), one[name](k).view(torch.int32))) for k in range(K))
                r[name]["block_over_K_one_column"] = round(r[name]["block"]["median_ms"] / (K * res["one_column"][name]["median_ms"]), 3)
        res["field_tape_bytes_with_block_arrays"] = tape.nbytes
        tape.release_block()
    res["field_tape_bytes"] = tape.nbytes
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--events", default="16,8")
    ap.add_argument("--cols", default="4,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--one-column-only", action="store_true")
    ap.add_argument("--root", default=HERE, help="the checkout whose ttcr_amd package is measured (default: this one)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    sys.path.insert(0, os.path.abspath(a.root))
    cols = [int(s) for s in a.cols.split(",")]
    for n, e in zip([int(s) for s in a.sizes.split(",")], [int(s) for s in a.events.split(",")]):
        print(json.dumps(case(n, e, cols, a.reps, a.warmup, a.one_column_only)), flush=True)


if __name__ == "__main__":
    main()
