"""Wall time of the field tape's double-difference products and solve beside the calls they extend, in the reciprocal layout.

For a 3-D node grid (fp32, weno=0): n_fields stations near the surface are the sources of the call, 441 hypocentres at depth are its
receivers -- every field sees all of them, so the 441 n_fields rows are grouped into 441 receiver points.  Pairs join the rows of
neighbouring points within each field: once every row with its --neighbours nearest points (each pair once, about that many entries
per row: `near`), once every pair of a field's rows (`all`: 440 entries per row).  On one field tape, device tensors:
  gn                    one tape.gauss_newton(v, row_weight): an existing entry, timed first and last
  solve_joint           one tape.solve_joint(..., maxiter=iters, rtol=0): an existing entry, timed first and last
  gn_rj                 one tape.gauss_newton_receiver_joint(v, v_rcv, row_weight, rcv_scale) without pair_weight
and per pair list
  gn_rj_pairs           the same call with pair_weight
  row_operator          one tape.row_operator(x, row_weight, pair_weight): the two pair kernels and the entry around them (the tape's
                        stream is the tape's own, so this is the wall time of the call with device tensors in and out, an upper bound
                        of the two kernels)
  torch_composed        the same product composed in torch in the same run: jvp_joint_receiver, index_select / index_add_, vjp
  products, solve       iters calls of gn_rj_pairs in a row (before and after), one tape.solve_receiver_joint(..., pair_weight,
                        maxiter=iters, rtol=0)
On a build without the pair calls only gn and solve_joint are timed (the same script at the parent commit).  Per figure: --warmup calls
that are not timed, then the median of --reps (at least 5) timed calls and their spread (max - min), in ms.  One JSON line per grid.

    python scripts/dd_time.py [--sizes 128,256] [--fields 16,8] [--neighbours 20] [--iters 10] [--reps 5] [--warmup 2] [--root DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pair_lists(hyp, n_fields, neighbours):
    """{name: (row_a, row_b)} in data rows; the rows of field f are 441 f .. 441 f + 440, row k of a field is point k"""
    n = hyp.shape[0]
    d2 = ((hyp[:, None, :] - hyp[None, :, :]) ** 2).sum(axis=2)
    near = np.argsort(d2, axis=1)[:, 1:neighbours // 2 + 1]            # each pair once: about `neighbours` entries per row
    a = np.repeat(np.arange(n), near.shape[1])
    b = near.ravel()
    iu = np.triu_indices(n, 1)
    out = {}
    for name, (pa, pb) in (("near", (a, b)), ("all", iu)):
        off = 441 * np.arange(n_fields)[:, None]
        out[name] = ((pa[None, :] + off).ravel(), (pb[None, :] + off).ravel())
    return out


def case(n, n_fields, neighbours, iters, reps, warmup):
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
    have = hasattr(tape, "set_row_pairs")

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

    res = dict(nodes=f"{n}^3", dtype="float32", fields=n_fields, rows_per_field=441, iterations=iters, smooth=smooth, damp=damp,
               reps=reps, warmup=warmup, build_id=ttcr_amd._lib.build_id(), pair_calls=have)
    b, b_src = tape.vjp(w, return_source_grad=True)

    def gn():
        return tape.gauss_newton(b, rw)

    def solve_joint():
        return tape.solve_joint(b, b_src, row_weight=rw, smooth=smooth, damp=damp, source_damp=rdamp, source_scale=scale, maxiter=iters,
                                rtol=0.0, return_info=True)

    res["gn_before"] = timed(gn)
    res["solve_joint_before"] = timed(solve_joint)
    if have:
        tape.set_receiver_points(np.tile(np.arange(441), n_fields))
        b_rcv = tape.vjp(w, return_receiver_grad=True)[1]
        res["gn_rj"] = timed(lambda: tape.gauss_newton_receiver_joint(b, b_rcv, rw, scale))
        c = dev(np.broadcast_to(np.array(scale), (441, 4)))
        for name, (pa, pb) in pair_lists(hyp, n_fields, neighbours).items():
            tape.set_row_pairs(pa, pb)
            pw = dev(rng.uniform(0.5, 2.0, pa.size))
            ia, ib = torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda()

            def gn_rj_pairs():
                return tape.gauss_newton_receiver_joint(b, b_rcv, rw, scale, pair_weight=pw)

            def torch_composed():
                dtt = tape.jvp_joint_receiver(b, c * b_rcv)
                u = pw * (dtt.index_select(0, ia) - dtt.index_select(0, ib))
                rows = (rw * dtt).index_add_(0, ia, u).index_add_(0, ib, -u)
                gs, ge = tape.vjp(rows, return_receiver_grad=True)
                return gs, c * ge

            def products():
                for _ in range(iters):
                    gn_rj_pairs()

            def solve():
                return tape.solve_receiver_joint(b, b_rcv, row_weight=rw, pair_weight=pw, smooth=smooth, damp=damp, rcv_damp=rdamp,
                                                 rcv_scale=scale, maxiter=iters, rtol=0.0, return_info=True)

            r = dict(pairs=int(pa.size), entries_per_row=round(2 * pa.size / rcv.shape[0], 1))
            r["gn_rj_pairs"] = timed(gn_rj_pairs)
            r["row_operator"] = timed(lambda: tape.row_operator(w, rw, pw))
            r["torch_composed"] = timed(torch_composed)
            got, ref = gn_rj_pairs(), torch_composed()
            r["torch_composed_rel_diff"] = float((got[0] - ref[0]).norm() / ref[0].norm())
            r["products_before"] = timed(products)
            r["solve"] = timed(solve)
            r["products_after"] = timed(products)
            prod = 0.5 * (r["products_before"]["median_ms"] + r["products_after"]["median_ms"])
            r["solve_adds_per_iteration_ms"] = round((r["solve"]["median_ms"] - prod) / iters, 3)
            r["pairs_add_ms"] = round(r["gn_rj_pairs"]["median_ms"] - res["gn_rj"]["median_ms"], 3)
            r["field_tape_bytes_with_pair_arrays"] = tape.nbytes
            tape.release_pairs()
            res[name] = r
        tape.release_receiver()
    res["gn_after"] = timed(gn)
    res["solve_joint_after"] = timed(solve_joint)
    tape.release_joint()
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
