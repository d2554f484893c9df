"""Wall time of the field tape's grid-search location beside the same search written in torch, in the reciprocal layout.

For a 3-D node grid (fp32, weno=0): n_fields stations near the surface are the sources of the call, on one field tape.  --hypos
hypocentres at depth with --picks picks each (fields dealt in turn, times from the fields at a node plus noise, random weights):
  locate_grid         one tape.locate_grid of all hypocentres (numpy picks in, numpy results out)
  locate_grid_subset  the same for the first --baseline-hypos hypocentres: what the baseline is compared with
  torch_subset        the baseline: the same search in torch on the same fields on the tape's device (float64, one (chunk, n_nodes)
                      intermediate per operation, chunked over the hypocentres so that it fits), for those first hypocentres; its nodes,
                      origin times and misfits are compared with the kernel's
  locate_grid_volume  locate_grid of the first 16 hypocentres with return_misfit=True, the volume left on the device (tensor picks)
  locate_grid_16      ... and without the volume
  locate              one inversion.locate(..., refine=10) of all hypocentres
  gn                  one tape.gauss_newton(v, row_weight), an existing entry: timed before and after the locate calls, and the only
                      figure on a build without locate_grid (the same script at the parent commit)
field_read_GBps: n_hypo * picks * 2 passes * n_nodes field values of the tape's dtype read (from LDS) per locate_grid call, over its time;
volume_GBps: the same against the bytes of the field volume (n_fields * n_nodes values), the figure of a search that read it once.
Per figure: --warmup calls that are not timed, then the median of --reps (at least 5) timed calls and their spread (max - min), in ms.
One JSON line per grid.

    python scripts/locate_time.py [--sizes 128,256] [--fields 16,8] [--hypos 1000] [--picks 12] [--baseline-hypos 100] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_search(torch, T64, hyp_field, hyp_time, hyp_weight, budget_bytes=2 << 30):
    """the baseline: T64 (n_fields, n_nodes) float64 on the device; hyp_* (n_hypo, K) tensors there.  The definition's operations in its
    order, a (chunk, n_nodes) intermediate each."""
    nq, K = hyp_field.shape
    n = T64.shape[1]
    chunk = max(1, int(budget_bytes // (8 * n * 6)))
    node, t0, mis = [], [], []
    for q0 in range(0, nq, chunk):
        f, t, w = hyp_field[q0:q0 + chunk], hyp_time[q0:q0 + chunk], hyp_weight[q0:q0 + chunk]
        sw = torch.zeros(f.shape[0], dtype=torch.float64, device=T64.device)
        for k in range(K):
            sw = sw + w[:, k]
        a = torch.zeros((f.shape[0], n), dtype=torch.float64, device=T64.device)
        for k in range(K):
            a = a + w[:, k, None] * (t[:, k, None] - T64[f[:, k]])
        t0n = a / sw[:, None]
        del a
        phi = torch.zeros((f.shape[0], n), dtype=torch.float64, device=T64.device)
        for k in range(K):
            d = (t[:, k, None] - T64[f[:, k]]) - t0n
            phi = phi + w[:, k, None] * (d * d)
        m, i = torch.min(phi, dim=1)
        # (the lowest index among equal minima, as the definition has it: torch.min does not promise one)
        i = torch.argmax((phi == m[:, None]).to(torch.uint8), dim=1)
        node.append(i)
        mis.append(m)
        t0.append(t0n.gather(1, i[:, None])[:, 0])
    return torch.cat(node), torch.cat(t0), torch.cat(mis)


def case(n, n_fields, n_hypo, n_picks, n_base, reps, warmup):
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
    rcv = np.column_stack([rng.uniform(0.2 * hi, 0.8 * hi, (64, 2)), rng.uniform(0.5 * hi, 0.9 * hi, 64)])
    src = np.column_stack([np.repeat(np.arange(n_fields), 64), np.zeros(n_fields * 64), np.repeat(stations, 64, axis=0)])
    tape = g.raytrace_adjoint(src, np.tile(rcv, (n_fields, 1)))[1]
    dev = lambda h: torch.from_numpy(np.ascontiguousarray(h, dtype=dt)).cuda()   # noqa: E731
    rw = dev(rng.uniform(0.5, 2.0, n_fields * 64))
    b = tape.vjp(dev(rng.standard_normal(n_fields * 64)))
    have = hasattr(tape, "locate_grid")

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

    res = dict(nodes=f"{n}^3", dtype="float32", fields=n_fields, hypocentres=n_hypo, picks_per_hypocentre=n_picks, reps=reps, warmup=warmup,
               build_id=ttcr_amd._lib.build_id(), locate_calls=have)
    res["gn_before"] = timed(lambda: tape.gauss_newton(b, rw))
    if have:
        res["locate_shape"] = tape.locate_shape
        T = np.stack([tape.field(e) for e in range(n_fields)])
        nodes = rng.integers(0, n ** 3, n_hypo)
        fld = (np.arange(n_picks)[None, :] + rng.integers(0, n_fields, n_hypo)[:, None]) % n_fields
        tm = 100.0 + T[fld, nodes[:, None]].astype(np.float64) + 0.05 * rng.standard_normal((n_hypo, n_picks))
        wt = rng.uniform(0.5, 2.0, (n_hypo, n_picks))
        hyp = np.repeat(np.arange(n_hypo), n_picks)
        picks = (hyp, fld.ravel(), tm.ravel(), wt.ravel())
        sub = tuple(p[:n_base * n_picks] for p in picks)
        p16 = tuple(torch.as_tensor(p[:16 * n_picks]).cuda() for p in picks)
        res["locate_grid"] = timed(lambda: tape.locate_grid(*picks))
        res["locate_grid_subset"] = timed(lambda: tape.locate_grid(*sub))
        T64 = torch.from_numpy(T).cuda().to(torch.float64)
        tf, tt, tw = (torch.as_tensor(a[:n_base]).cuda() for a in (fld, tm, wt))
        res["torch_subset"] = timed(lambda: torch_search(torch, T64, tf, tt, tw))
        got = tape.locate_grid(*sub)
        ref = [a.cpu().numpy() for a in torch_search(torch, T64, tf, tt, tw)]
        res["baseline_hypocentres"] = n_base
        res["baseline_equal"] = [bool(np.array_equal(got[i], ref[i])) for i in range(3)]
        del T64
        torch.cuda.empty_cache()
        res["locate_grid_16"] = timed(lambda: tape.locate_grid(*p16))
        res["locate_grid_volume_16"] = timed(lambda: tape.locate_grid(*p16, return_misfit=True))
        res["locate_refine10"] = timed(lambda: inversion.locate(tape, *picks, refine=10))
        info = inversion.locate(tape, *picks, refine=10)[3]
        res["locate_iterations_mean"] = float(np.mean(info["iterations"]))
        res["locate_misfit_start_final_median"] = [float(np.median(info["start_misfit"])), float(np.median(info["misfit"]))]
        ms = res["locate_grid"]["median_ms"]
        res["field_read_GBps"] = round(n_hypo * n_picks * 2 * n ** 3 * 4 / (ms * 1e-3) / 1e9, 1)
        res["volume_GBps"] = round(n_fields * n ** 3 * 4 / (ms * 1e-3) / 1e9, 3)
        res["speedup_over_torch"] = round(res["torch_subset"]["median_ms"] / res["locate_grid_subset"]["median_ms"], 1)
        res["field_tape_bytes_with_locate_arrays"] = tape.nbytes
        tape.release_locate()
    res["gn_after"] = timed(lambda: tape.gauss_newton(b, rw))
    res["field_tape_bytes"] = tape.nbytes
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--fields", default="16,8")
    ap.add_argument("--hypos", type=int, default=1000)
    ap.add_argument("--picks", type=int, default=12)
    ap.add_argument("--baseline-hypos", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    sys.path.insert(0, HERE)
    for n, e in zip([int(s) for s in a.sizes.split(",")], [int(s) for s in a.fields.split(",")]):
        print(json.dumps(case(n, e, a.hypos, a.picks, min(a.baseline_hypos, a.hypos), a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
