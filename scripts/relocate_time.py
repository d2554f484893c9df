"""Wall time of moving a field tape's receiver points and of the relocation-only system beside what they replace, in the
reciprocal layout.

For a 3-D node grid (fp32, weno=0): n_fields stations near the surface are the sources of the call, 1 000 hypocentres at depth are its
receivers -- every field sees all of them, so the 1 000 n_fields rows are grouped into 1 000 receiver points.  Pairs join every row with
its --neighbours nearest points within its field.  On one field tape, device tensors, in one run:
  gn, solve_rj          one tape.gauss_newton(v, row_weight) and one tape.solve_receiver_joint(..., maxiter=iters, rtol=0): existing entries,
                        timed first and last (they must stay within the run's spread)
  fresh                 grid.raytrace_adjoint with the moved rcv, set_receiver_points and set_row_pairs: what the parent commit offers to
                        get products at new points (the solves of n_fields fields, a new tape, the coupling pass, the host lists)
  move                  tape.move_receiver_points(xyz), alternating between two sets of points (the first move's allocation is in the warm-up)
  solve_r, solve_r_pairs   one tape.solve_receiver(..., maxiter=iters, rtol=0) without and with pair_weight
  solve_rj_pairs        one tape.solve_receiver_joint(..., pair_weight, maxiter=iters, rtol=0)
  relocate              one inversion.relocate(..., n_iter=iters) with pairs from points 0.3 dx off the true ones (device tensors)
On a build without the new calls only gn, solve_rj and fresh are timed (the same script at the parent commit).  Per figure: --warmup
calls that are not timed, then the median of --reps (at least 5) timed calls and their spread (max - min), in ms.  One JSON line per grid.

    python scripts/relocate_time.py [--sizes 128,256] [--fields 16,8] [--neighbours 20] [--iters 10] [--reps 5] [--warmup 2] [--root DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_HYP = 1000


def case(n, n_fields, neighbours, iters, reps, warmup):
    import torch

    torch.cuda.init()   # (before the first grid: torch ships a HIP runtime of its own)
    import ttcr_amd
    from ttcr_amd import inversion

    dt = np.float32
    dx = 1.0
    x = np.arange(n) * dx
    v = (1.5 + 0.02 * x)[None, None, :] * np.ones((n, n, n))
    g = ttcr_amd.Grid3d(x, x, x, n_threads=8, cell_slowness=0, method="FSM", tt_from_rp=0, weno=0, dtype=dt)
    g.set_velocity(v.astype(dt))
    rng = np.random.default_rng(1)
    hi = (n - 1) * dx
    stations = np.column_stack([rng.uniform(0.05 * hi, 0.95 * hi, (n_fields, 2)), rng.uniform(0.0, 0.02 * hi, n_fields)])
    true = np.column_stack([rng.uniform(0.2 * hi, 0.8 * hi, (N_HYP, 2)), rng.uniform(0.5 * hi, 0.9 * hi, N_HYP)])
    true = (np.floor(true) + rng.uniform(0.35, 0.65, true.shape)).astype(dt).astype(np.float64)   # well inside their cells
    moved = (true + rng.uniform(-0.3, 0.3, true.shape) * dx).astype(dt).astype(np.float64)
    src = np.column_stack([np.repeat(np.arange(n_fields), N_HYP), np.zeros(n_fields * N_HYP), np.repeat(stations, N_HYP, axis=0)])
    por = np.tile(np.arange(N_HYP), n_fields)
    d2 = ((true[:, None, :] - true[None, :, :]) ** 2).sum(axis=2)
    near = np.argsort(d2, axis=1)[:, 1:neighbours // 2 + 1]
    off = N_HYP * np.arange(n_fields)[:, None]
    pa = (np.repeat(np.arange(N_HYP), near.shape[1])[None, :] + off).ravel()
    pb = (near.ravel()[None, :] + off).ravel()

    def fresh(xyz):
        tt, tape = g.raytrace_adjoint(src, np.tile(xyz, (n_fields, 1)))
        if hasattr(tape, "set_receiver_points"):
            tape.set_receiver_points(por)
        if hasattr(tape, "set_row_pairs"):
            tape.set_row_pairs(pa, pb)
        return tt, tape

    t_true, tape = fresh(true)
    dev = lambda h: torch.from_numpy(np.ascontiguousarray(h, dtype=dt)).cuda()   # noqa: E731
    n_rows = src.shape[0]
    rw = dev(rng.uniform(0.5, 2.0, n_rows))
    w = dev(rng.standard_normal(n_rows))
    pw = dev(rng.uniform(0.5, 2.0, pa.size))
    scale = (1.0, 0.05, 0.05, 0.05)
    rdamp = (1e-2, 1e-1, 1e-1, 1e-1)
    smooth, damp = 1e-2, 1e-1
    have = hasattr(tape, "move_receiver_points")

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
        return dict(median_ms=round(float(np.median(ts)), 3), spread_ms=round(float(max(ts) - min(ts)), 3))

    res = dict(nodes=f"{n}^3", dtype="float32", fields=n_fields, hypocentres=N_HYP, rows=n_rows, pairs=int(pa.size), iterations=iters,
               reps=reps, warmup=warmup, build_id=ttcr_amd._lib.build_id(), relocation_calls=have)
    b, b_rcv = tape.vjp(w, return_receiver_grad=True)

    def gn():
        return tape.gauss_newton(b, rw)

    def solve_rj(pair_weight=None):
        return tape.solve_receiver_joint(b, b_rcv, row_weight=rw, smooth=smooth, damp=damp, rcv_damp=rdamp, rcv_scale=scale, maxiter=iters,
                                         rtol=0.0, return_info=True, pair_weight=pair_weight)

    res["gn_before"] = timed(gn)
    res["solve_rj_before"] = timed(solve_rj)
    flip = [0]

    def fresh_call():
        flip[0] ^= 1
        fresh(moved if flip[0] else true)[1].free()

    res["fresh"] = timed(fresh_call)
    if have:
        pts = [dev(true), dev(moved)]

        def move():
            flip[0] ^= 1
            return tape.move_receiver_points(pts[flip[0]])

        before = tape.nbytes
        res["move"] = timed(move)
        res["move_adds_bytes"] = tape.nbytes - before
        res["fresh_over_move"] = round(res["fresh"]["median_ms"] / res["move"]["median_ms"], 1)
        tape.move_receiver_points(pts[0])
        res["solve_r"] = timed(lambda: tape.solve_receiver(b_rcv, row_weight=rw, rcv_damp=rdamp, rcv_scale=scale, maxiter=iters, rtol=0.0,
                                                           return_info=True))
        res["solve_r_pairs"] = timed(lambda: tape.solve_receiver(b_rcv, row_weight=rw, rcv_damp=rdamp, rcv_scale=scale, maxiter=iters,
                                                                 rtol=0.0, return_info=True, pair_weight=pw))
        res["solve_rj_pairs"] = timed(lambda: solve_rj(pw))
        t_obs = dev(t_true)
        pair_dt = t_obs[torch.from_numpy(pa).cuda()] - t_obs[torch.from_numpy(pb).cuda()]
        t0 = torch.zeros(N_HYP, dtype=torch.float32, device="cuda")
        out = {}

        def relocate():
            tape.move_receiver_points(pts[1])
            out["r"] = inversion.relocate(tape, t_obs, t0, pair_dt=pair_dt, n_iter=iters, rcv_damp=1e-3)

        res["relocate"] = timed(relocate)
        _, xyz, hist, info = out["r"]
        err = (xyz.cpu().numpy().astype(np.float64) - true)
        res["relocate_iterations"] = info["iterations"]
        res["relocate_misfit"] = [hist[0], hist[-1]]
        res["relocate_error_dx"] = dict(start=round(float(np.abs(moved - true).max() / dx), 4), median=float(np.median(np.abs(err).max(axis=1)) / dx),
                                        max=float(np.abs(err).max() / dx))
        tape.move_receiver_points(pts[0])
    res["gn_after"] = timed(gn)
    res["solve_rj_after"] = timed(solve_rj)
    res["field_tape_bytes"] = tape.nbytes
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--fields", default="16,8")
    ap.add_argument("--neighbours", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--root", default=HERE, help="the tree whose ttcr_amd package is timed (default: this one)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    sys.path.insert(0, os.path.abspath(a.root))
    for n, e in zip([int(s) for s in a.sizes.split(",")], [int(s) for s in a.fields.split(",")]):
        print(json.dumps(case(n, e, a.neighbours, a.iters, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
