"""IVF-Flat index (sonar_amd.index) on one MI355X: one JSON line, also written to profiles/ivf_bench.json.

  Data: n = 1 M rows x 1024 fp16 with planted clusters (tools/bench_kmeans.py's generator: K unit Gaussian directions, row i
  belongs to cluster i % K), K = 1024 and K = 16 384 lists; 262 144 queries, query j a noisy copy of a random corpus row
  (normalise(x + 0.1 g / sqrt(d))); k = 4; nprobe in {1, 4, 8}.  The quantiser is SphericalKMeans fitted on the corpus
  (2 rounds from the first member of each cluster).
  Per K: the build (smi_ivf_build) and, per nprobe, the probe (smi_xsim_topk against the centroids), the list search
  (smi_ivf_search: bucketing of the probe table + scan + merge), the merge alone (smi_xsim_merge_topk on arrays of the same
  shape) and the whole `IVFFlatIndex.search` (normalise + probe + list search), each in event windows of `--launches`
  back-to-back calls, median / min / max over `--reps` windows; the kernels of one list search from a torch.profiler trace.
  In the same run, on the same data: brute-force xsim.topk_normalized (k = 4), and recall@1 / recall@4 of every search
  against it.  The run checks itself: every planted neighbour must be found at nprobe = 1.
  Derived expectation, to read next to the measurement: the scan scores sum over the (query, probe) pairs of the probed
  list's size ~ nq nprobe n / K pairs, nprobe / K of brute force's; it will not reach the mining kernel's share of the MFMA
  peak, because its query operand is gathered per work unit and its tiles are 64 x 64.  The build's gather is a copy:
  2 n d 2 bytes, reported next to the device-to-device copy rate measured in the same run.
    python tools/bench_ivf.py [--rows 1000000] [--queries 262144] [--reps 5] [--launches 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_kmeans import planted, windows_ms  # noqa: E402

PEAK_FP16 = 2.5e15  # dense fp16 MFMA, flop/s


def kernel_trace(fn):
    """Device time in us of every kernel of one call, from a torch.profiler trace; a note where that is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            if ev.device_time > 0:
                name = next((s for s in ("ivf_scan_lists", "bucket_hist", "ivf_scan_kernel", "bucket_scatter", "ivf_gather",
                                         "ivf_fill", "topk_merge", "Memset", "memset") if s in ev.name), None)
                if name:
                    out[name] = round(out.get(name, 0.0) + ev.device_time, 2)
        return out or None
    except Exception as e:  # noqa: BLE001  (a measurement aid: the timed figures do not depend on it)
        return {"unavailable": repr(e)[:200]}


def queries(x, nq, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n, d = x.shape
    target = torch.randint(0, n, (nq,), device="cuda", generator=g)
    q = x[target].float() + 0.1 / d ** 0.5 * torch.randn(nq, d, device="cuda", generator=g)
    return torch.nn.functional.normalize(q, dim=1).half(), target.int()


def run(x, q, target, k_lists, k, nprobes, bf, reps, launches, copy_ms):
    from sonar_amd import clustering, index, xsim

    n, d = x.shape
    nq = q.shape[0]
    xn, qn = xsim.normalize_rows(x), xsim.normalize_rows(q)
    km = clustering.SphericalKMeans(k_lists, n_iter=2).fit_normalized(xn, n, init=x[:k_lists])
    ix = index.IVFFlatIndex(km).add(x)
    torch.cuda.synchronize()
    labels = km.labels
    used, bound = int(ix.list_offsets[-1]), int(ix._ids.shape[0])
    sizes = ix.list_sizes
    res = {"n": n, "d": d, "K": k_lists, "nq": nq, "k": k, "ntotal": ix.ntotal,
           "list_size_min_mean_max": [int(sizes.min()), round(float(sizes.float().mean()), 1), int(sizes.max())],
           "slots_used": used, "slots_allocated": bound, "padding_overhead_used": round(used / n - 1, 4),
           "padding_overhead_allocated": round(bound / n - 1, 4)}
    res["build_ms"] = windows_ms(lambda: index.build_lists(xn, labels, k_lists), reps, launches)
    res["build_kernel_trace_us"] = kernel_trace(lambda: index.build_lists(xn, labels, k_lists))
    res["build_gather_bytes"] = 2 * used * d * 2
    res["copy_of_the_corpus_ms"] = copy_ms
    bf_s, bf_i = bf
    for nprobe in nprobes:
        r = {}
        probes = ix.probe(q, nprobe)
        r["probe_ms"] = windows_ms(lambda: xsim.topk_normalized(qn, nq, ix._c16, k_lists, nprobe), reps, launches)
        search = lambda: index.search_lists(qn, probes, ix._rows, ix._ids, ix._offsets, k)  # noqa: E731
        r["list_search_ms"] = windows_ms(search, reps, launches)
        r["list_search_kernel_trace_us"] = kernel_trace(search)
        ps = torch.randn(nprobe, nq, k, device="cuda").sort(dim=2, descending=True)[0].contiguous()
        pi = torch.randint(0, n, (nprobe, nq, k), device="cuda", dtype=torch.int32)
        r["merge_ms"] = windows_ms(lambda: xsim.merge_topk(ps, pi), reps, launches)
        r["search_ms"] = windows_ms(lambda: ix.search(q, k=k, nprobe=nprobe), reps, launches)
        score, idx = ix.search(q, k=k, nprobe=nprobe)
        pairs = int(sizes[probes.long().clamp(0, k_lists - 1)].long().sum())
        r["scored_pairs"] = pairs
        r["share_of_brute_force_pairs"] = round(pairs / (nq * n), 6)
        scan_us = (r["list_search_kernel_trace_us"] or {}).get("ivf_scan_lists")
        scan_ms = scan_us / 1e3 if scan_us else r["list_search_ms"]["median"]
        r["scan_ms_used_for_rates"] = round(scan_ms, 4)
        r["scan_pairs_per_s"] = round(pairs / (scan_ms * 1e-3), 1)
        r["scan_share_of_fp16_peak"] = round(pairs * 2 * d / (scan_ms * 1e-3) / PEAK_FP16, 4)
        r["recall_at_1"] = round(float((idx[:, 0] == bf_i[:, 0]).float().mean()), 6)
        r["recall_at_k"] = round(float((idx[:, :, None] == bf_i[:, None, :]).any(dim=2).float().mean()), 6)
        r["planted_found"] = int((idx[:, 0] == target).sum())
        r["top1_score_equals_brute_force"] = int((score[:, 0] == bf_s[:, 0]).sum())
        res[f"nprobe{nprobe}"] = r
    res["all_planted_found_at_nprobe_1"] = res[f"nprobe{nprobes[0]}"]["planted_found"] == nq
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--lists", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivf needs an MI355X: there is no CPU path")
    from sonar_amd import xsim

    n, d, nq = args.rows, args.dim, args.queries
    assert args.nprobe[0] == 1, "the self-check is stated at nprobe = 1"
    out = {"metric": "ivf_search_ms", "config": f"{n} x {d} fp16 planted clusters, {nq} queries, k = {args.k}, one MI355X",
           "expectation": "the scan scores about nprobe / K of brute force's pairs, below the mining kernel's share of the "
                          "MFMA peak (gathered query operand, 64 x 64 tiles); the build's gather is a copy of the corpus"}
    src = torch.empty(n, d, dtype=torch.float16, device="cuda").normal_()
    dst = torch.empty_like(src)
    cp = windows_ms(lambda: dst.copy_(src), args.reps, args.launches)
    out["copy_read_plus_write_TBps"] = round(2 * n * d * 2 / (cp["median"] * 1e-3) / 1e12, 3)
    del src, dst
    for k_lists in args.lists:
        x, _ = planted(n, k_lists, d, seed=k_lists)
        q, target = queries(x, nq, seed=k_lists + 1)
        xn, qn = xsim.normalize_rows(x), xsim.normalize_rows(q)
        bf = xsim.topk_normalized(qn, nq, xn, n, args.k)
        bf_ms = windows_ms(lambda: xsim.topk_normalized(qn, nq, xn, n, args.k), min(args.reps, 3), 1)
        del xn, qn
        res = run(x, q, target, k_lists, args.k, args.nprobe, bf, args.reps, args.launches, cp)
        res["brute_force_ms"] = bf_ms
        res["brute_force_pairs_per_s"] = round(nq * n / (bf_ms["median"] * 1e-3), 1)
        res["brute_force_share_of_fp16_peak"] = round(nq * n * 2 * d / (bf_ms["median"] * 1e-3) / PEAK_FP16, 4)
        res["brute_force_top1_is_planted"] = int((bf[1][:, 0] == target).sum())
        for p in args.nprobe:
            res[f"nprobe{p}"]["speedup_over_brute_force"] = round(bf_ms["median"] / res[f"nprobe{p}"]["search_ms"]["median"], 2)
        out[f"K{k_lists}"] = res
        del x, q, target, bf
        torch.cuda.empty_cache()
    out["value"] = out[f"K{args.lists[0]}"][f"nprobe{args.nprobe[0]}"]["search_ms"]["median"]
    out["all_planted_found_at_nprobe_1"] = all(out[f"K{k}"]["all_planted_found_at_nprobe_1"] for k in args.lists)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not out["all_planted_found_at_nprobe_1"]:
        raise SystemExit("a planted neighbour was not found at nprobe = 1")


if __name__ == "__main__":
    main()
