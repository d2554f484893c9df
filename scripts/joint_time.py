"""Wall time of the field tape's joint hypocentre-velocity calls beside the calls they replace.

For a 3-D node grid (fp32, weno=0), events at depth, a 21 x 21 surface array of receivers per event, on one field tape, device tensors:
  gn_joint            one tape.gauss_newton_joint(v, v_src, row_weight, source_scale)
  composition         what it replaces: tape.jvp(v) + tape.jvp_source(scale * v_src) (K = 1), then tape.vjp(row_weight * sum,
                      return_source_grad=True) and scale * gsrc -- two tangent relaxations and one adjoint relaxation; timed before and
                      after gn_joint
  jvp_joint, jvp, jvp_source      the three tangents alone, with their passes
  solve               one tape.solve_joint(..., maxiter=iters, rtol=0)
  products            iters calls of tape.gauss_newton_joint in a row: what the solve cannot avoid; timed before and after the other two
  torch_loop          the same recurrence written with torch operations around the composition (three tape calls per iteration)
The claim to confirm or refute: gn_joint costs about one tangent relaxation less than the composition.  Both differences are taken from
figures of the same run and are to be read against their spreads.  Per figure: --warmup calls that are not timed, then the median of
--reps (at least 5) timed calls and their spread (max - min), in ms.  The solve and the torch loop sum in different orders, so their
iterates differ in the last bits; the relative difference of the results is printed, not asserted.  One JSON line per grid.

    python scripts/joint_time.py [--sizes 128,256] [--events 16,8] [--iters 10] [--reps 5] [--warmup 2]
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
    dev = lambda h: torch.from_numpy(np.ascontiguousarray(h, dtype=dt)).cuda()   # noqa: E731
    rw = dev(rng.uniform(0.5, 2.0, rcv.shape[0]))
    b, b_e = tape.vjp(dev(rng.standard_normal(rcv.shape[0])), return_source_grad=True)
    scale_h = np.array([1.0, 0.05, 0.05, 0.05])
    scale = dev(np.tile(scale_h, (tape.n_points, 1)))
    sdamp = (1e-2, 1e-1, 1e-1, 1e-1)
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

    def gn_joint(p=b, pe=b_e):
        return tape.gauss_newton_joint(p, pe, rw, scale_h)

    def composition(p=b, pe=b_e):
        dtt = tape.jvp(p) + tape.jvp_source(scale * pe)
        g_s, g_e = tape.vjp(rw * dtt, return_source_grad=True)
        return g_s, scale * g_e

    def solve():
        return tape.solve_joint(b, b_e, row_weight=rw, smooth=smooth, damp=damp, source_damp=sdamp, source_scale=scale_h, maxiter=iters,
                                rtol=0.0, return_info=True)

    def products():
        for _ in range(iters):
            gn_joint()

    delta = dev(np.tile(sdamp, (tape.n_points, 1)))

    def torch_loop():
        dot = lambda u, w: (torch.dot(u[0], w[0]) + torch.dot(u[1].ravel(), w[1].ravel())).item()   # noqa: E731
        r = (b.clone(), scale * b_e)
        x_ = (torch.zeros_like(b), torch.zeros_like(b_e))
        p = (r[0].clone(), r[1].clone())
        rho = dot(r, r)
        for _ in range(iters):
            g_s, g_e = composition(p[0], p[1])
            q = (g_s + smooth * tape.smooth(p[0]) + damp * p[0], g_e + delta * p[1])
            alpha = rho / dot(p, q)
            x_ = (x_[0] + alpha * p[0], x_[1] + alpha * p[1])
            r = (r[0] - alpha * q[0], r[1] - alpha * q[1])
            rho_new = dot(r, r)
            p = (r[0] + (rho_new / rho) * p[0], r[1] + (rho_new / rho) * p[1])
            rho = rho_new
        return x_[0], scale * x_[1]

    res = dict(nodes=f"{n}^3", dtype="float32", events=n_ev, receivers_per_event=int(arr.shape[0]), iterations=iters, smooth=smooth,
               damp=damp, source_damp=list(sdamp), source_scale=list(scale_h), reps=reps, warmup=warmup, build_id=ttcr_amd._lib.build_id())
    # 1. the product: composition, joint, composition again
    res["composition_before"] = timed(composition)
    res["gn_joint"] = timed(gn_joint)
    res["composition_after"] = timed(composition)
    gn_joint()
    res["gn_joint_passes"] = list(tape.passes)
    # 2. the tangents alone
    for name, f in (("jvp_joint", lambda: tape.jvp_joint(b, b_e)), ("jvp", lambda: tape.jvp(b)), ("jvp_source", lambda: tape.jvp_source(b_e))):
        res[name] = timed(f)
        res[name]["passes"] = tape.passes
    # 3. the solve: products, solve, torch loop, products again
    res["products_before"] = timed(products)
    res["solve"] = timed(solve)
    res["torch_loop"] = timed(torch_loop)
    res["products_after"] = timed(products)
    xs, xe, info = solve()
    ts, te = torch_loop()
    res["solve_status"], res["solve_iterations"] = info["status"], info["iterations"]
    res["passes_per_iteration"] = info["passes"]
    res["residual_reduction"] = float(np.sqrt(info["rho"][-1] / info["rho"][0]))
    rel = lambda u, w: float((torch.linalg.norm((u - w).double()) / torch.linalg.norm(w.double())).item())   # noqa: E731
    res["solve_vs_torch_loop_rel_diff"] = dict(model=rel(xs, ts), sources=rel(xe, te))
    comp = 0.5 * (res["composition_before"]["median_ms"] + res["composition_after"]["median_ms"])
    prod = 0.5 * (res["products_before"]["median_ms"] + res["products_after"]["median_ms"])
    res["composition_minus_gn_joint_ms"] = round(comp - res["gn_joint"]["median_ms"], 2)
    res["added_per_iteration_ms"] = dict(solve=round((res["solve"]["median_ms"] - prod) / iters, 3),
                                         torch_loop=round((res["torch_loop"]["median_ms"] - prod) / iters, 3))
    res["field_tape_bytes_with_joint_arrays"] = tape.nbytes
    tape.release_joint()
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
