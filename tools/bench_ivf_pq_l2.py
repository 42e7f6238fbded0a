"""The L2 product-quantised indexes against their cosine counterparts on one MI355X, in ONE run: one JSON
line, also written to profiles/ivf_pq_l2_bench.json.

  Data: tools/bench_l2.py's -- n = 1 M rows x 1024 fp16 with planted clusters, every row scaled by a factor from 0.5 .. 2
  (lengths differ: the L2 order is not the cosine order); 262 144 queries, query j a noisy copy of a random corpus row, its
  planted L2 neighbour.  K = 1024 and 16 384 lists by one Euclidean KMeans per K, dsub 8 and 16, k = 4, nprobe 1 / 4 / 8.
  Per K and dsub, for IVFPQL2Index and IVFPQResidualL2Index:
  (a) the kernel: smi_l2_pq_search against smi_ivf_pq_search, and smi_l2_pq_search_residual against
      smi_ivf_pq_search_residual, over the SAME codes, lists, probes (and coarse terms) -- what the bias costs the scan;
  (b) the bias kernel over the slots against the composition it replaces, prepare_rows(pq_decode(codes))[1].neg(), and the
      bytes that composition allocates and the kernel does not;
  (c) the whole `search`, raw and refined, and how often the planted neighbour comes first, raw and refined;
  (d) the list sizes (min / mean / max): the end-to-end time inherits the Euclidean quantiser's imbalance, which is a
      property of the lists, not of the scan.
  Event windows of `--launches` calls, median / min / max over `--reps`.
  Derived expectation: the flat L2 scan's -- one 16-byte load of four biases per four slots beside the ids, one add per score
  that reaches the fold (two with the coarse term, which the cosine residual scan adds as well): a little above 1 x
  (DESIGN.md 3.28 measured 1.12 / 0.98 / 0.97 for the flat pair).  The planted noise is isotropic and does not compress: nothing
  here speaks for real SONAR rows.
  The run checks itself: distances are non-decreasing everywhere and the refined search finds the planted neighbour first at
  least as often as the raw one.
    python tools/bench_ivf_pq_l2.py [--rows 1000000] [--queries 262144] [--lists 1024 16384] [--dsub 8 16] [--reps 3] [--launches 1]
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
from bench_l2 import queries, ratio, scaled  # noqa: E402


def run(x, q, target, prepared, k_lists, dsubs, pq_iter, reps, launches):
    from sonar_amd import clustering, index

    (x16, hx), (q16, hq) = prepared
    n, d = x.shape
    nq = q.shape[0]
    km = clustering.KMeans(k_lists, n_iter=2).fit_prepared(x16, hx, n, init=x[:k_lists])
    init = clustering.init_rows(n, 256, 0).to(device=x.device, dtype=torch.int32)
    labels = index.IVFFlatL2Index(km).probe(x, 1)[:, 0].contiguous()
    cent = km._c16[:k_lists]
    out = {"K": k_lists}
    ok = True
    for dsub in dsubs:
        per = {"code_bytes_per_row": d // dsub}
        for kind in ("plain", "residual"):
            res = {}
            if kind == "plain":
                cb = index.pq_train(x16, dsub, init, pq_iter, n)
                ix = index.IVFPQL2Index(km, cb).add(x, labels=labels)
            else:
                cb = index.pq_train_residual(x16, labels, cent, dsub, init, pq_iter)
                ix = index.IVFPQResidualL2Index(km, cb).add(x, labels=labels)
            sizes = ix.list_sizes
            res["list_size_min_mean_max"] = [int(sizes.min()), round(float(sizes.float().mean()), 1), int(sizes.max())]
            codes, bias, ids, off = ix._rows, ix._bias, ix._ids, ix._offsets
            slots = codes.shape[0]
            # (b) the bias of every slot: the kernel against decode + prepare
            if kind == "plain":
                res["bias_kernel_ms"] = windows_ms(lambda: index.pq_l2_bias(codes, cb, ids=ids), reps, launches)
                res["decode_prepare_ms"] = windows_ms(lambda: index.prepare_rows(index.pq_decode(codes, cb))[1].neg(), reps, launches)
                res["bias_kernel_over_decode_prepare"] = ratio(res, "bias_kernel_ms", "decode_prepare_ms")
                pad = (slots + 255) // 256 * 256
                res["bytes_not_allocated"] = slots * d * 2 + pad * d * 2 + pad * 4  # the decoded rows, their padded copy, its norms
            else:
                res["bias_kernel_ms"] = windows_ms(lambda: index.pq_l2_bias(codes, cb, None, cent, ids=ids, offsets=off), reps, launches)
            for nprobe in (1, 4, 8):
                coarse, probes = ix._nearest_lists(q16, nq, nprobe)
                if kind == "plain":
                    l2 = lambda: index.search_lists_pq_l2(q16, probes, codes, cb, bias, ids, off, 4)  # noqa: E731
                    cos = lambda: index.search_lists_pq(q16, probes, codes, cb, ids, off, 4)  # noqa: E731
                else:
                    l2 = lambda: index.search_lists_pq_l2(q16, probes, codes, cb, bias, ids, off, 4, coarse)  # noqa: E731
                    cos = lambda: index.search_lists_pq_residual(q16, probes, coarse, codes, cb, ids, off, 4)  # noqa: E731
                cell = {"l2_list_search_ms": windows_ms(l2, reps, launches), "cosine_list_search_ms": windows_ms(cos, reps, launches)}
                cell["l2_list_search_again_ms"] = windows_ms(l2, reps, launches)  # the pair's own drift
                cell["l2_over_cosine"] = ratio(cell, "l2_list_search_ms", "cosine_list_search_ms")
                cell["search_ms"] = windows_ms(lambda: ix.search(q, 4, nprobe), reps, launches)
                cell["refined_search_ms"] = windows_ms(lambda: ix.search(q, 4, nprobe, refine=(x16, hx)), reps, launches)
                dist, idx = ix.search(q, 4, nprobe)
                rdist, ridx = ix.search(q, 4, nprobe, refine=(x16, hx))
                cell["planted_first_raw"] = int((idx[:, 0] == target).sum())
                cell["planted_first_refined"] = int((ridx[:, 0] == target).sum())
                cell["planted_among_candidates"] = int((idx == target[:, None]).any(dim=1).sum())
                ok &= bool((dist[:, :-1] <= dist[:, 1:]).all()) and bool((rdist[:, :-1] <= rdist[:, 1:]).all())
                ok &= cell["planted_first_refined"] >= cell["planted_first_raw"]
                res[f"nprobe{nprobe}"] = cell
            per[kind] = res
            del ix
        out[f"dsub{dsub}"] = per
    return out, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--lists", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--dsub", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--pq-iter", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_pq_l2_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivf_pq_l2 needs an MI355X: there is no CPU path")
    from sonar_amd import xsim

    n, d, nq = args.rows, args.dim, args.queries
    out = {"metric": "l2_pq_list_search_over_cosine_pq_list_search",
           "config": f"{n} x {d} fp16 planted clusters with row lengths 0.5 .. 2, {nq} queries, k = 4, {args.pq_iter} PQ rounds, one MI355X",
           "expectation": "one 16-byte load of four biases per four slots and one add per score at the fold: a little above 1 x",
           "data_caveat": "synthetic planted rows with isotropic noise; real SONAR rows are unmeasured"}
    x = scaled(planted(n, 1024, d, seed=1024)[0], seed=1026)
    q, target = queries(x, nq, seed=1025)
    prepared = (xsim.prepare_rows(x), xsim.prepare_rows(q))
    ok = True
    for k_lists in args.lists:
        out[f"K{k_lists}"], good = run(x, q, target, prepared, k_lists, args.dsub, args.pq_iter, args.reps, args.launches)
        ok &= good
    ratios = [cell["l2_over_cosine"] for key, part in out.items() if key.startswith("K") for ds, per in part.items() if ds.startswith("dsub")
              for kind in ("plain", "residual") for name, cell in per[kind].items() if name.startswith("nprobe")]
    out["l2_over_cosine_min_median_max"] = [min(ratios), sorted(ratios)[len(ratios) // 2], max(ratios)]
    out["value"] = out["l2_over_cosine_min_median_max"][1]
    out["self_check"] = bool(ok)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not ok:
        raise SystemExit("the self-check failed: distances decrease, or refining lost planted neighbours")


if __name__ == "__main__":
    main()
