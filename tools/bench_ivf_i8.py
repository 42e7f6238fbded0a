"""Int8 IVF index against the flat one (sonar_amd.index) on one MI355X, in ONE run on the same data: one JSON line, also
written to profiles/ivf_i8_bench.json.

  Data and shapes: tools/bench_ivf.py's -- n = 1 M rows x 1024 fp16 with planted clusters, K = 1024 and K = 16 384 lists,
  262 144 queries (noisy copies of corpus rows), k = 4, nprobe in {1, 4, 8}; the quantiser is SphericalKMeans fitted on the
  corpus, shared by both indexes.
  Per K: both builds (smi_ivf_build, smi_ivf_i8_build) and the bytes both keep; per nprobe, for both indexes, the list
  search (bucketing of the probe table + scan + merge; the int8 one encodes the queries first) and, from a torch.profiler
  trace of one call, its scan kernel and the query encoding; the refine step (`index.refine_candidates`: pair cosines + two
  stable sorts) on the int8 candidates; the whole `search` of the flat index, of the int8 index raw and refined.  Event
  windows of `--launches` back-to-back calls, median / min / max over `--reps` windows.  Recall@1 / recall@k of the int8
  index, raw and refined, and of the flat index against brute-force xsim.topk_normalized of the same run.
  The yardstick for the int8 scan is the flat scan of this run.  The run checks itself: every planted neighbour must be
  found at nprobe = 1 by the int8 index, raw and refined.
  Derived expectation, to read next to the measurement: the flat scan is bound by the bytes its K slices bring from L2
  (profiles/ivf_experiments.txt, item 1); int8 operands halve those bytes and v_mfma_i32_16x16x64_i8 has twice the fp16
  rate, so the scan can gain up to 2x; the fold, the bucketing and the merge are unchanged and the query encoding is added.
    python tools/bench_ivf_i8.py [--rows 1000000] [--queries 262144] [--reps 5] [--launches 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ivf import PEAK_FP16, queries  # noqa: E402
from bench_kmeans import planted, windows_ms  # noqa: E402

PEAK_I8 = 2 * PEAK_FP16  # dense int8 MFMA, op/s: twice the fp16 rate
KERNELS = ("ivf_i8_scan_lists", "ivf_scan_lists", "ivf_i8_encode", "ivf_i8_gather", "ivf_gather", "bucket_hist",
           "ivf_scan_kernel", "bucket_scatter", "ivf_fill", "topk_merge", "Memset", "memset")


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
                name = next((s for s in KERNELS if s in ev.name), None)
                if name:
                    out[name] = round(out.get(name, 0.0) + ev.device_time, 2)
        return out or None
    except Exception as e:  # noqa: BLE001  (a measurement aid: the timed figures do not depend on it)
        return {"unavailable": repr(e)[:200]}


def recalls(idx, bf_i, target):
    return {"recall_at_1": round(float((idx[:, 0] == bf_i[:, 0]).float().mean()), 6),
            "recall_at_k": round(float((idx[:, :, None] == bf_i[:, None, :]).any(dim=2).float().mean()), 6),
            "planted_found": int((idx[:, 0] == target).sum())}


def run(x, q, target, k_lists, k, nprobes, bf_i, reps, launches):
    from sonar_amd import clustering, index, xsim

    n, d = x.shape
    nq = q.shape[0]
    xn, qn = xsim.normalize_rows(x), xsim.normalize_rows(q)
    km = clustering.SphericalKMeans(k_lists, n_iter=2).fit_normalized(xn, n, init=x[:k_lists])
    labels = km.labels
    flat, i8 = index.IVFFlatIndex(km).add(x, labels=labels), index.IVFInt8Index(km).add(x, labels=labels)
    torch.cuda.synchronize()
    used, bound = int(flat.list_offsets[-1]), int(flat._ids.shape[0])
    sizes = flat.list_sizes
    res = {"n": n, "d": d, "K": k_lists, "nq": nq, "k": k, "ntotal": i8.ntotal, "slots_used": used, "slots_allocated": bound,
           "list_size_min_mean_max": [int(sizes.min()), round(float(sizes.float().mean()), 1), int(sizes.max())],
           "storage_bytes_used": {"flat": used * (2 * d + 4), "int8": used * (d + 4 + 4)},
           "storage_bytes_allocated": {"flat": bound * (2 * d + 4), "int8": bound * (d + 4 + 4)}}
    res["storage_ratio_int8_over_flat"] = round(res["storage_bytes_used"]["int8"] / res["storage_bytes_used"]["flat"], 4)
    res["flat_build_ms"] = windows_ms(lambda: index.build_lists(xn, labels, k_lists), reps, launches)
    res["int8_build_ms"] = windows_ms(lambda: index.build_lists_int8(xn, labels, k_lists), reps, launches)
    res["flat_build_kernel_trace_us"] = kernel_trace(lambda: index.build_lists(xn, labels, k_lists))
    res["int8_build_kernel_trace_us"] = kernel_trace(lambda: index.build_lists_int8(xn, labels, k_lists))
    res["corpus_encode_ms"] = windows_ms(lambda: index.encode_rows_int8(xn, n), reps, launches)
    for nprobe in nprobes:
        r = {}
        probes = flat.probe(q, nprobe)
        pairs = int(sizes[probes.long().clamp(0, k_lists - 1)].long().sum())
        r["scored_pairs"] = pairs
        searches = {"flat": lambda: index.search_lists(qn, probes, flat._rows, flat._ids, flat._offsets, k),
                    "int8": lambda: index.search_lists_int8(qn, probes, i8._rows, i8._scales, i8._ids, i8._offsets, k)}
        for name, fn in searches.items():
            r[f"{name}_list_search_ms"] = windows_ms(fn, reps, launches)
            r[f"{name}_list_search_kernel_trace_us"] = trace = kernel_trace(fn)
            scan_us = (trace or {}).get("ivf_i8_scan_lists" if name == "int8" else "ivf_scan_lists")
            if scan_us:
                r[f"{name}_scan_ms"] = round(scan_us / 1e3, 4)
                r[f"{name}_scan_pairs_per_s"] = round(pairs / (scan_us * 1e-6), 1)
                r[f"{name}_scan_share_of_its_mfma_peak"] = round(
                    pairs * 2 * d / (scan_us * 1e-6) / (PEAK_I8 if name == "int8" else PEAK_FP16), 4)
        if "flat_scan_ms" in r and "int8_scan_ms" in r:
            r["scan_speedup_int8_over_flat"] = round(r["flat_scan_ms"] / r["int8_scan_ms"], 3)
        r["list_search_speedup_int8_over_flat"] = round(
            r["flat_list_search_ms"]["median"] / r["int8_list_search_ms"]["median"], 3)
        r["query_encode_ms"] = round(((r["int8_list_search_kernel_trace_us"] or {}).get("ivf_i8_encode") or 0.0) / 1e3, 4)
        raw_s, raw_i = searches["int8"]()
        r["refine_ms"] = windows_ms(lambda: index.refine_candidates(qn, nq, xn, raw_i), reps, launches)
        r["flat_search_ms"] = windows_ms(lambda: flat.search(q, k=k, nprobe=nprobe), reps, launches)
        r["int8_search_ms"] = windows_ms(lambda: i8.search(q, k=k, nprobe=nprobe), reps, launches)
        r["int8_refined_search_ms"] = windows_ms(lambda: i8.search(q, k=k, nprobe=nprobe, refine=xn), reps, launches)
        flat_s, flat_i = flat.search(q, k=k, nprobe=nprobe)
        ref_s, ref_i = i8.search(q, k=k, nprobe=nprobe, refine=xn)
        r["flat"], r["int8_raw"], r["int8_refined"] = (recalls(i, bf_i, target) for i in (flat_i, raw_i, ref_i))
        r["int8_raw_top1_equals_flat_top1"] = int((raw_i[:, 0] == flat_i[:, 0]).sum())
        r["int8_refined_top1_score_equals_flat"] = int((ref_s[:, 0] == flat_s[:, 0]).sum())
        r["max_abs_raw_score_minus_flat_score_at_top1"] = float(
            (raw_s[:, 0] - flat_s[:, 0])[raw_i[:, 0] == flat_i[:, 0]].abs().max())
        res[f"nprobe{nprobe}"] = r
    first = res[f"nprobe{nprobes[0]}"]
    res["all_planted_found_at_nprobe_1"] = first["int8_raw"]["planted_found"] == nq == first["int8_refined"]["planted_found"]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_i8_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivf_i8 needs an MI355X: there is no CPU path")
    from sonar_amd import xsim

    n, d, nq = args.rows, args.dim, args.queries
    assert args.nprobe[0] == 1, "the self-check is stated at nprobe = 1"
    out = {"metric": "ivf_i8_list_search_ms",
           "config": f"{n} x {d} fp16 planted clusters, {nq} queries, k = {args.k}, one MI355X; flat and int8 in one run",
           "expectation": "int8 halves the bytes a K slice brings from L2 and doubles the MFMA rate: up to 2x on the scan; "
                          "the bucketing, fold and merge are unchanged and the query encoding is added"}
    for k_lists in args.lists:
        x, _ = planted(n, k_lists, d, seed=k_lists)
        q, target = queries(x, nq, seed=k_lists + 1)
        xn, qn = xsim.normalize_rows(x), xsim.normalize_rows(q)
        bf_i = xsim.topk_normalized(qn, nq, xn, n, args.k)[1]
        del xn, qn
        res = run(x, q, target, k_lists, args.k, args.nprobe, bf_i, args.reps, args.launches)
        res["brute_force_top1_is_planted"] = int((bf_i[:, 0] == target).sum())
        out[f"K{k_lists}"] = res
        del x, q, target, bf_i
        torch.cuda.empty_cache()
    out["value"] = out[f"K{args.lists[0]}"][f"nprobe{args.nprobe[0]}"]["int8_list_search_ms"]["median"]
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
