"""DTW alignment (sonar_amd.alignment) on one MI355X: one JSON line, also written to profiles/alignment_bench.json.

  (a) 4096 document pairs of 32..128 sentences, one call;  (b) one 8192 x 8192 pair, full matrix;  (c) the same pair at
  radius = 256.  d = 1024 fp16 embeddings.  Every y document is its x document with planted 1-1, 1-2 (a sentence repeated)
  and 2-1 (two sentences merged into their mean) beads plus noise, and the run checks that every planted path is recovered.
  Times the whole call from embeddings (smi_dtw_align), the call from given costs (smi_dtw_align_cost: layout + DP +
  backtrack) and, from a torch.profiler kernel trace of one call, the cost kernel, the DP kernel and the backtrack kernel
  separately (null when the profiler is not available).  cells/s counts nx * ny cells of the full matrices (for the band:
  the admissible cells as well).  The CPU figure is the literal restatement (tests/alignment_ref.py, numpy fp32 scalars in a
  Python loop) on a 256 x 256 matrix on the host of the same box: context, not a competitor.
    python tools/bench_alignment.py [--pairs 4096] [--big 8192] [--radius 256] [--d 1024] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("dtw_cost_kernel", "dtw_skew_kernel", "dtw_dp_kernel", "dtw_backtrack_kernel")


def planted(sizes, rng):
    """-> (source rows a, b of every y row (y = mean of x[a], x[b]), x offsets, y offsets, planted paths)."""
    a, b, xo, yo, paths = [], [], [0], [0], []
    for nx in sizes:
        op = rng.choice(3, nx, p=[0.8, 0.1, 0.1])   # 0: 1-1, 1: the sentence twice, 2: merged with the next one
        path, i, j = [], 0, 0
        while i < nx:
            if op[i] == 2 and i + 1 < nx:
                a.append(xo[-1] + i)
                b.append(xo[-1] + i + 1)
                path += [(i, j), (i + 1, j)]
                i, j = i + 2, j + 1
                continue
            for _ in range(2 if op[i] == 1 else 1):
                a.append(xo[-1] + i)
                b.append(xo[-1] + i)
                path.append((i, j))
                j += 1
            i += 1
        xo.append(xo[-1] + nx)
        yo.append(yo[-1] + j)
        paths.append(path)
    return np.array(a), np.array(b), xo, yo, paths


def make(sizes, d, seed):
    rng = np.random.default_rng(seed)
    a, b, xo, yo, paths = planted(sizes, rng)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(xo[-1], d, generator=g, device="cuda")
    y = 0.5 * (x[torch.from_numpy(a).cuda()] + x[torch.from_numpy(b).cuda()])
    y += 0.05 * torch.randn(y.shape, generator=g, device="cuda")
    return x.half(), y.half(), xo, yo, paths


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def kernel_times(fn):
    """Device time of every dtw kernel in one call, in ms, from a torch.profiler trace; None where that is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            for k in KERNELS:
                if k in ev.name and ev.device_time > 0:
                    out[k] = out.get(k, 0.0) + ev.device_time / 1e3
        return {k: round(v, 4) for k, v in out.items()} or None
    except Exception as e:  # noqa: BLE001  (a measurement aid: the timed figures above do not depend on it)
        return {"unavailable": repr(e)[:200]}


def run_case(name, sizes, d, radius, reps, seed):
    from sonar_amd.alignment import DtwPlan
    from sonar_amd.xsim import normalize_rows
    from tests import alignment_ref

    x, y, xo, yo, paths = make(sizes, d, seed)
    xn, yn = normalize_rows(x), normalize_rows(y)
    plan = DtwPlan(xo, yo, x.device)
    t_align = timed(lambda: plan.run(xn, yn, radius), reps)
    got = plan.results()
    cost = plan.costs().clone()
    kt = kernel_times(lambda: plan.run(xn, yn, radius))
    t_cost = timed(lambda: plan.run_cost(cost, radius), reps)
    again = plan.results()
    recovered = sum([tuple(p) for p in g[0].tolist()] == want for g, want in zip(got, paths))
    same = all(torch.equal(p[0], q[0]) and p[1] == q[1] for p, q in zip(got, again))
    cells = sum((xo[b + 1] - xo[b]) * (yo[b + 1] - yo[b]) for b in range(len(sizes)))
    res = {"pairs": len(sizes), "cells": cells, "radius": radius, "align_ms": round(t_align * 1e3, 3),
           "align_cost_ms": round(t_cost * 1e3, 3), "cells_per_s_align": round(cells / t_align, 1),
           "cells_per_s_align_cost": round(cells / t_cost, 1), "kernel_ms": kt, "planted_recovered": recovered,
           "every_planted_path_recovered": recovered == len(sizes), "align_cost_equals_align": same,
           "workspace_bytes": plan.ws_bytes}
    if radius and len(sizes) == 1:
        res["admissible_cells"] = int(alignment_ref.admissible_matrix(xo[1], yo[1], radius).sum())
    if kt and "dtw_dp_kernel" in kt:
        res["cells_per_s_dp_kernel"] = round(res.get("admissible_cells", cells) / (kt["dtw_dp_kernel"] * 1e-3), 1)
    return name, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--big", type=int, default=8192)
    ap.add_argument("--radius", type=int, default=256)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alignment_bench.json"))
    args = ap.parse_args()
    from tests import alignment_ref

    rng = np.random.default_rng(0)
    out = {"metric": "alignment_batch_ms", "config": f"d = {args.d} fp16; {args.pairs} pairs of 32..128 sentences; "
           f"one {args.big} x ~{args.big} pair full and at radius {args.radius}"}
    cases = [("batch", rng.integers(32, 129, args.pairs).tolist(), 0), ("big_full", [args.big], 0),
             ("big_band", [args.big], args.radius)]
    for n, (name, sizes, radius) in enumerate(cases):
        key, res = run_case(name, sizes, args.d, radius, args.reps, seed=n + 1)
        out[key] = res
    c = np.random.default_rng(1).random((256, 256)).astype(np.float32)
    t0 = time.perf_counter()
    alignment_ref.dtw(c)
    out["cpu_restatement_cells_per_s"] = round(c.size / (time.perf_counter() - t0), 1)
    out["cpu_restatement"] = "tests/alignment_ref.py (Python loop over numpy fp32 scalars), 256 x 256, host of the same box"
    out["value"] = out["batch"]["align_ms"]
    ok = all(out[k]["every_planted_path_recovered"] and out[k]["align_cost_equals_align"] for k, _, _ in cases)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
