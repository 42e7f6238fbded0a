"""IVF-PQ with residual encoding against the plain IVF-PQ index and the flat one (sonar_amd.index) on one MI355X,
in ONE run on the same data: one JSON line, also written to profiles/ivf_pq_residual_bench.json.

  Data and shapes: tools/bench_ivf_pq.py's -- n = 1 M rows x 1024 fp16 with planted clusters, K = 1024 and K = 16 384 lists,
  262 144 queries, k = 4, nprobe in {1, 4, 8}, dsub in {8, 16}, `--pq-iter` Lloyd rounds from `clustering.init_rows(n, 256, 0)`;
  one SphericalKMeans per K, shared by the three indexes.
  Per K and dsub, plain next to residual: training, the corpus encoding, the build and the quantisation error (the mean squared
  distance of what is encoded -- the row, or its residual -- from its reconstruction; the residual's is also the distance of
  the row from centroid + reconstruction, up to the residual's fp16 rounding).  Per nprobe: the flat list search and scan, and
  for both PQ indexes the list search (bucketing + scan + merge), its scan kernel from a torch.profiler trace of one call, the
  whole `search` raw and refined, and recall@1 of the planted neighbour and recall@k against brute-force xsim.topk_normalized
  of the same run, raw and refined; and each scan kernel once on the OTHER index's codes, which tells a difference of the kernels
  from a difference of the codes they gather by.  Event windows of `--launches` back-to-back calls, median / min / max over `--reps`.
  Derived, to read next to the measurement: the residual scan adds one LDS read and one fp32 add per score that reaches the fold
  and 4 bytes of global traffic per pair -- within noise of the plain scan; the fused encoders read one more 2 KB centroid row
  per encoded row, L2-resident at K = 1024 -- within a few per cent; the error should fall well below the plain quantiser's,
  whose codewords spend themselves on the list centres.  The planted noise is isotropic: nothing here speaks for real SONAR rows.
    python tools/bench_ivf_pq_residual.py [--rows 1000000] [--queries 262144] [--dsub 8 16] [--reps 5] [--launches 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ivf import queries  # noqa: E402
from bench_ivf_i8 import recalls  # noqa: E402
from bench_ivf_pq import kernel_trace  # noqa: E402
from bench_kmeans import planted, windows_ms  # noqa: E402


def sq_error(rows, n, codes, codebooks):
    """The mean squared distance of the first n fp16 rows from the reconstruction of their codes."""
    from sonar_amd import index

    diff = index.pq_decode(codes, codebooks).float() - rows[:n].float()
    return round(float((diff * diff).sum(dim=1).mean()), 5)


def timed_search(fn, scan_name, reps, launches):
    out = {"list_search_ms": windows_ms(fn, reps, launches), "kernel_trace_us": kernel_trace(fn)}
    scan_us = (out["kernel_trace_us"] or {}).get(scan_name)
    if scan_us:
        out["scan_ms"] = round(scan_us / 1e3, 4)
    return out


def run(x, q, target, k_lists, k, nprobes, dsubs, pq_iter, bf_i, reps, launches):
    from sonar_amd import clustering, index, xsim

    n, d = x.shape
    nq = q.shape[0]
    few = max(1, reps // 2)
    xn, qn = xsim.normalize_rows(x), xsim.normalize_rows(q)
    km = clustering.SphericalKMeans(k_lists, n_iter=2).fit_normalized(xn, n, init=x[:k_lists])
    labels, c16 = km.labels, km.centroids_normalized.contiguous()
    flat = index.IVFFlatIndex(km).add(x, labels=labels)
    torch.cuda.synchronize()
    sizes = flat.list_sizes
    res = {"n": n, "d": d, "K": k_lists, "nq": nq, "k": k, "ntotal": flat.ntotal,
           "list_size_min_mean_max": [int(sizes.min()), round(float(sizes.float().mean()), 1), int(sizes.max())]}
    init = clustering.init_rows(n, index.PQ_CODEWORDS, 0).to(device=x.device, dtype=torch.int32)
    flat_runs = {}
    for nprobe in nprobes:
        coarse, probes = xsim.topk_normalized(qn, nq, flat._c16, k_lists, nprobe)
        r = timed_search(lambda: index.search_lists(qn, probes, flat._rows, flat._ids, flat._offsets, k), "ivf_scan_lists", reps,
                         launches)
        r["search_ms"] = windows_ms(lambda: flat.search(q, k=k, nprobe=nprobe), reps, launches)
        r["recall"] = recalls(flat.search(q, k=k, nprobe=nprobe)[1], bf_i, target)
        flat_runs[nprobe] = (r, probes, coarse)
    for dsub in dsubs:
        p = {"dsub": dsub, "code_bytes_per_row": d // dsub}
        trainers = {"plain": lambda: index.pq_train(xn, dsub, init, pq_iter, n),
                    "residual": lambda: index.pq_train_residual(xn, labels, c16, dsub, init, pq_iter)}
        for kind, train in trainers.items():
            t = {"train_ms": windows_ms(train, few, 1)}
            cb = train()
            if kind == "plain":
                encode = lambda: index.pq_encode(xn, cb, n)  # noqa: E731
                build = lambda: index.build_lists_pq(xn, labels, k_lists, cb)  # noqa: E731
                t["quantisation_error_mean_sq"] = sq_error(xn, n, encode(), cb)
                ix = index.IVFPQIndex(km, cb).add(x, labels=labels)
            else:
                encode = lambda: index.pq_encode_residual(xn, labels, c16, cb)  # noqa: E731
                build = lambda: index.build_lists_pq_residual(xn, labels, c16, cb)  # noqa: E731
                resid = index.pq_residuals(xn, labels, c16)
                t["quantisation_error_mean_sq"] = sq_error(resid, n, encode(), cb)
                t["residual_energy_mean_sq"] = round(float((resid.float() ** 2).sum(dim=1).mean()), 5)
                del resid
                ix = index.IVFPQResidualIndex(km, cb).add(x, labels=labels)
            t["corpus_encode_ms"] = windows_ms(encode, few, 1)
            t["build_ms"] = windows_ms(build, few, 1)
            torch.cuda.synchronize()
            for nprobe in nprobes:
                flat_r, probes, coarse = flat_runs[nprobe]
                if kind == "plain":
                    fn = lambda: index.search_lists_pq(qn, probes, ix._rows, ix._codebooks, ix._ids, ix._offsets, k)  # noqa: E731
                else:
                    fn = lambda: index.search_lists_pq_residual(qn, probes, coarse, ix._rows, ix._codebooks, ix._ids,  # noqa: E731
                                                                ix._offsets, k)
                r = timed_search(fn, "ivf_pq_scan_lists", reps, launches)
                # the OTHER scan kernel on these codes (its scores mean nothing): is a difference the kernel's or the codes'?
                if kind == "plain":
                    other = lambda: index.search_lists_pq_residual(qn, probes, coarse, ix._rows, ix._codebooks, ix._ids,  # noqa: E731
                                                                   ix._offsets, k)
                else:
                    other = lambda: index.search_lists_pq(qn, probes, ix._rows, ix._codebooks, ix._ids, ix._offsets, k)  # noqa: E731
                other_us = (kernel_trace(other) or {}).get("ivf_pq_scan_lists")
                if other_us:
                    r["other_scan_kernel_on_these_codes_ms"] = round(other_us / 1e3, 4)
                r["search_ms"] = windows_ms(lambda: ix.search(q, k=k, nprobe=nprobe), reps, launches)
                r["refined_search_ms"] = windows_ms(lambda: ix.search(q, k=k, nprobe=nprobe, refine=xn), reps, launches)
                r["raw"] = recalls(ix.search(q, k=k, nprobe=nprobe)[1], bf_i, target)
                r["refined"] = recalls(ix.search(q, k=k, nprobe=nprobe, refine=xn)[1], bf_i, target)
                t[f"nprobe{nprobe}"] = r
            p[kind] = t
            del ix, cb
            torch.cuda.empty_cache()
        ratios = {"train": p["residual"]["train_ms"]["median"] / p["plain"]["train_ms"]["median"],
                  "build": p["residual"]["build_ms"]["median"] / p["plain"]["build_ms"]["median"],
                  "error": p["residual"]["quantisation_error_mean_sq"] / p["plain"]["quantisation_error_mean_sq"]}
        for nprobe in nprobes:
            a, b = p["residual"][f"nprobe{nprobe}"], p["plain"][f"nprobe{nprobe}"]
            if "scan_ms" in a and "scan_ms" in b:
                ratios[f"scan_nprobe{nprobe}"] = a["scan_ms"] / b["scan_ms"]
            ratios[f"search_nprobe{nprobe}"] = a["search_ms"]["median"] / b["search_ms"]["median"]
        p["residual_over_plain"] = {name: round(v, 4) for name, v in ratios.items()}
        res[f"dsub{dsub}"] = p
    res["flat"] = {f"nprobe{nprobe}": flat_runs[nprobe][0] for nprobe in nprobes}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_pq_residual_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivf_pq_residual needs an MI355X: there is no CPU path")
    from sonar_amd import xsim

    n, d, nq = args.rows, args.dim, args.queries
    out = {"metric": "ivf_pq_residual_list_search_ms",
           "config": f"{n} x {d} fp16 planted clusters, {nq} queries, k = {args.k}, {args.pq_iter} PQ rounds, one MI355X; flat, "
                     "plain PQ and residual PQ in one run",
           "expectation": "scan within noise of plain PQ (one LDS read and one add per score at the fold); build and training "
                          "within a few per cent (one more centroid row per encoded row); error well below plain PQ's"}
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
    out["value"] = out[f"K{args.lists[0]}"][f"dsub{args.dsub[0]}"]["residual"][f"nprobe{args.nprobe[0]}"]["list_search_ms"]["median"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
