"""IVF-PQ index against the flat one (sonar_amd.index) on one MI355X, in ONE run on the same data: one JSON line, also written
to profiles/ivf_pq_bench.json.

  Data and shapes: tools/bench_ivf.py's -- n = 1 M rows x 1024 fp16 with planted clusters, K = 1024 and K = 16 384 lists,
  262 144 queries (noisy copies of corpus rows), k = 4, nprobe in {1, 4, 8}; the coarse quantiser is SphericalKMeans fitted on
  the corpus, shared by both indexes; dsub in {8, 16}, `--pq-iter` Lloyd rounds from `clustering.init_rows(n, 256, 0)`.
  Per K and dsub: training (smi_pq_train), the corpus encoding (smi_pq_encode), the build (smi_ivf_pq_build) and the bytes
  kept, next to the flat build and bytes; per nprobe, for both indexes, the list search (bucketing of the probe table + scan +
  merge) and, from a torch.profiler trace of one call, its scan kernel; the refine step on the PQ candidates; the whole
  `search` of the flat index and of the PQ index raw and refined.  Event windows of `--launches` back-to-back calls, median /
  min / max over `--reps` windows.  Recall@1 / recall@k of the PQ index, raw and refined, and of the flat index against
  brute-force xsim.topk_normalized of the same run, and whether every planted neighbour is found.
  The yardstick for the PQ scan is the flat scan of this run: `scan_ratio_pq_over_flat` per (K, nprobe, dsub).
  Derived, to read next to the measurement: the code bytes are d / dsub per row against 2 d (1/16 at dsub = 8, 1/32 at 16);
  per tile and K slice the scan brings the same 2 * B * 128 bytes out of L2 as the flat scan, the list half now as scattered
  16-byte pieces of a 512 KB table, so "about the flat scan's time" is the expectation and nothing more is derived.
  The planted data's noise part is isotropic and does not compress: the recall figures say nothing about real SONAR rows.
    python tools/bench_ivf_pq.py [--rows 1000000] [--queries 262144] [--dsub 8 16] [--reps 5] [--launches 5]
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
from bench_ivf_i8 import recalls  # noqa: E402
from bench_kmeans import planted, windows_ms  # noqa: E402

KERNELS = ("ivf_pq_scan_lists", "ivf_scan_lists", "ivf_pq_gather", "ivf_gather", "pq_encode", "pq_accumulate", "pq_finalize",
           "pq_init", "bucket_hist", "ivf_scan_kernel", "bucket_scatter", "ivf_fill", "topk_merge", "Memset", "memset")


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


def run(x, q, target, k_lists, k, nprobes, dsubs, pq_iter, bf_i, reps, launches):
    from sonar_amd import clustering, index, xsim

    n, d = x.shape
    nq = q.shape[0]
    xn, qn = xsim.normalize_rows(x), xsim.normalize_rows(q)
    km = clustering.SphericalKMeans(k_lists, n_iter=2).fit_normalized(xn, n, init=x[:k_lists])
    labels = km.labels
    flat = index.IVFFlatIndex(km).add(x, labels=labels)
    torch.cuda.synchronize()
    used, bound = int(flat.list_offsets[-1]), int(flat._ids.shape[0])
    sizes = flat.list_sizes
    res = {"n": n, "d": d, "K": k_lists, "nq": nq, "k": k, "ntotal": flat.ntotal, "slots_used": used, "slots_allocated": bound,
           "list_size_min_mean_max": [int(sizes.min()), round(float(sizes.float().mean()), 1), int(sizes.max())],
           "flat_storage_bytes_used": {"rows": used * 2 * d, "ids": used * 4},
           "flat_build_ms": windows_ms(lambda: index.build_lists(xn, labels, k_lists), reps, launches)}
    init = clustering.init_rows(n, index.PQ_CODEWORDS, 0).to(device=x.device, dtype=torch.int32)
    flat_runs = {}
    for nprobe in nprobes:
        probes = flat.probe(q, nprobe)
        fn = lambda: index.search_lists(qn, probes, flat._rows, flat._ids, flat._offsets, k)  # noqa: E731
        r = {"scored_pairs": int(sizes[probes.long().clamp(0, k_lists - 1)].long().sum()),
             "flat_list_search_ms": windows_ms(fn, reps, launches), "flat_list_search_kernel_trace_us": kernel_trace(fn),
             "flat_search_ms": windows_ms(lambda: flat.search(q, k=k, nprobe=nprobe), reps, launches)}
        scan_us = (r["flat_list_search_kernel_trace_us"] or {}).get("ivf_scan_lists")
        if scan_us:
            r["flat_scan_ms"] = round(scan_us / 1e3, 4)
            r["flat_scan_share_of_mfma_peak"] = round(r["scored_pairs"] * 2 * d / (scan_us * 1e-6) / PEAK_FP16, 4)
        flat_i = flat.search(q, k=k, nprobe=nprobe)[1]
        r["flat"] = recalls(flat_i, bf_i, target)
        flat_runs[nprobe] = (r, probes, flat_i)
    for dsub in dsubs:
        m = d // dsub
        p = {"dsub": dsub, "code_bytes_per_row": m,
             "train_ms": windows_ms(lambda: index.pq_train(xn, dsub, init, pq_iter, n), max(1, reps // 2), 1),
             "train_kernel_trace_us": kernel_trace(lambda: index.pq_train(xn, dsub, init, pq_iter, n))}
        codebooks = index.pq_train(xn, dsub, init, pq_iter, n)
        p["corpus_encode_ms"] = windows_ms(lambda: index.pq_encode(xn, codebooks, n), max(1, reps // 2), 1)
        p["build_ms"] = windows_ms(lambda: index.build_lists_pq(xn, labels, k_lists, codebooks), max(1, reps // 2), 1)
        pq = index.IVFPQIndex(km, codebooks).add(x, labels=labels)
        torch.cuda.synchronize()
        assert int(pq.list_offsets[-1]) == used
        p["storage_bytes_used"] = {"codes": used * m, "ids": used * 4, "codebooks": 256 * d * 2}
        p["code_bytes_over_flat_row_bytes"] = round(used * m / (used * 2 * d), 6)
        recon = index.pq_decode(index.pq_encode(xn, codebooks, n), codebooks).float() - xn[:n].float()
        p["quantisation_error_mean_sq"] = round(float((recon * recon).sum(dim=1).mean()), 5)
        del recon
        for nprobe in nprobes:
            base, probes, flat_i = flat_runs[nprobe]
            r = dict(base)
            fn = lambda: index.search_lists_pq(qn, probes, pq._rows, pq._codebooks, pq._ids, pq._offsets, k)  # noqa: E731
            r["pq_list_search_ms"] = windows_ms(fn, reps, launches)
            r["pq_list_search_kernel_trace_us"] = trace = kernel_trace(fn)
            scan_us = (trace or {}).get("ivf_pq_scan_lists")
            if scan_us:
                r["pq_scan_ms"] = round(scan_us / 1e3, 4)
                r["pq_scan_share_of_mfma_peak"] = round(r["scored_pairs"] * 2 * d / (scan_us * 1e-6) / PEAK_FP16, 4)
                if "flat_scan_ms" in r:
                    r["scan_ratio_pq_over_flat"] = round(r["pq_scan_ms"] / r["flat_scan_ms"], 3)
            r["list_search_ratio_pq_over_flat"] = round(r["pq_list_search_ms"]["median"] / r["flat_list_search_ms"]["median"], 3)
            raw_s, raw_i = fn()
            r["refine_ms"] = windows_ms(lambda: index.refine_candidates(qn, nq, xn, raw_i), reps, launches)
            r["pq_search_ms"] = windows_ms(lambda: pq.search(q, k=k, nprobe=nprobe), reps, launches)
            r["pq_refined_search_ms"] = windows_ms(lambda: pq.search(q, k=k, nprobe=nprobe, refine=xn), reps, launches)
            ref_i = pq.search(q, k=k, nprobe=nprobe, refine=xn)[1]
            r["pq_raw"], r["pq_refined"] = recalls(raw_i, bf_i, target), recalls(ref_i, bf_i, target)
            r["pq_refined_top1_equals_flat_top1"] = int((ref_i[:, 0] == flat_i[:, 0]).sum())
            p[f"nprobe{nprobe}"] = r
        first = p[f"nprobe{nprobes[0]}"]
        p["all_planted_found_at_nprobe_1"] = {"raw": first["pq_raw"]["planted_found"] == nq,
                                              "refined": first["pq_refined"]["planted_found"] == nq}
        res[f"dsub{dsub}"] = p
        del pq, codebooks
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--lists", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--dsub", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--pq-iter", type=int, default=4)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_pq_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivf_pq needs an MI355X: there is no CPU path")
    from sonar_amd import xsim

    n, d, nq = args.rows, args.dim, args.queries
    out = {"metric": "ivf_pq_list_search_ms",
           "config": f"{n} x {d} fp16 planted clusters, {nq} queries, k = {args.k}, {args.pq_iter} PQ rounds, one MI355X; flat "
                     "and PQ in one run",
           "expectation": "code bytes d / dsub per row against 2 d; the scan brings the flat scan's bytes out of L2 per slice, "
                          "the list half as scattered 16-byte pieces of the codebooks: about the flat scan's time"}
    for k_lists in args.lists:
        x, _ = planted(n, k_lists, d, seed=k_lists)
        q, target = queries(x, nq, seed=k_lists + 1)
        xn, qn = xsim.normalize_rows(x), xsim.normalize_rows(q)
        bf_i = xsim.topk_normalized(qn, nq, xn, n, args.k)[1]
        del xn, qn
        res = run(x, q, target, k_lists, args.k, args.nprobe, args.dsub, args.pq_iter, bf_i, args.reps, args.launches)
        res["brute_force_top1_is_planted"] = int((bf_i[:, 0] == target).sum())
        out[f"K{k_lists}"] = res
        del x, q, target, bf_i
        torch.cuda.empty_cache()
    out["value"] = out[f"K{args.lists[0]}"][f"dsub{args.dsub[0]}"][f"nprobe{args.nprobe[0]}"]["pq_list_search_ms"]["median"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
