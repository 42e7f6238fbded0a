"""Paged top-k on one MI355X: one JSON line, also written to profiles/topk_wide_bench.json.

  Data: tools/bench_ivf.py's -- n = 1 M rows x 1024 fp16 with planted clusters, 262 144 queries, query j a noisy copy of a
  random corpus row.  Everything is timed in ONE run, in event windows of `--launches` calls, median / min / max over `--reps`:
  (a) brute force, queries x corpus: the k = 8 pass (smi_xsim_topk, the yardstick: boxes differ by +-4 %), a page of 16 without
      and with a ceiling (smi_xsim_topk_page), and topk_wide_normalized at k = 32 and 64 (2 and 4 pages).
      Derived expectation: the MFMA work of a page is the k = 8 pass's; only the cascade is longer and the insertions are about
      16 (1 + ln(n / 16)) per row and chunk: a page within a few percent of the k = 8 pass, k = 64 four pages.
  (b) the index, K = 1024 and 16 384 lists: search(8, 8), and search_wide at (k, nprobe) = (16, 8), (16, 16), (16, 64),
      (64, 16) with the probe (topk_wide_normalized against the centroids) and the scan (the pages of search_lists_page) timed
      separately; the recall of search_wide(k = 16) against topk_wide(k = 16) at nprobe = 8, 16, 32, 64 over the 15
      neighbours behind the planted one (the bulk rows).
      Expectation: the scan scales with nprobe as it does between 4 and 8; at K = 16 384 the paged probe costs at most four
      of today's probes.
  The run checks itself: the planted neighbour comes first in every result, and every page is in order (scores
  non-increasing, ids ascending inside a tie, no id twice, across the page boundaries).
    python tools/bench_topk_wide.py [--rows 1000000] [--queries 262144] [--reps 3] [--launches 1]
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
from bench_kmeans import planted, windows_ms  # noqa: E402


def in_order(score, idx):
    """Every row best first in the total order, fill behind the candidates, no id twice."""
    s0, s1, i0, i1 = score[:, :-1], score[:, 1:], idx[:, :-1].long(), idx[:, 1:].long()
    fill = i1 < 0
    ok = (s1 < s0) | ((s1 == s0) & (i1 > i0)) | (fill & torch.isneginf(s1))
    ok &= ~((i0 < 0) & ~fill)  # nothing behind a fill entry
    return bool(ok.all())


def brute_force(xn, n, qn, nq, reps, launches):
    from sonar_amd import xsim

    res = {}
    res["k8_pass_ms"] = windows_ms(lambda: xsim.topk_normalized(qn, nq, xn, n, 8), reps, launches)
    res["page16_ms"] = windows_ms(lambda: xsim.topk_page_normalized(qn, nq, xn, n, 16), reps, launches)
    first = xsim.topk_page_normalized(qn, nq, xn, n, 16)
    below = xsim.last_entry(*first)
    res["page16_with_ceiling_ms"] = windows_ms(lambda: xsim.topk_page_normalized(qn, nq, xn, n, 16, 0, below), reps, launches)
    res["k32_ms"] = windows_ms(lambda: xsim.topk_wide_normalized(qn, nq, xn, n, 32), reps, launches)
    res["k64_ms"] = windows_ms(lambda: xsim.topk_wide_normalized(qn, nq, xn, n, 64), reps, launches)
    base = res["k8_pass_ms"]["median"]
    for name in ("page16_ms", "page16_with_ceiling_ms", "k32_ms", "k64_ms"):
        res[name.replace("_ms", "_over_k8_pass")] = round(res[name]["median"] / base, 4)
    # the k = 8 pass again, behind everything: what the yardstick itself moved by inside this run
    res["k8_pass_again_ms"] = windows_ms(lambda: xsim.topk_normalized(qn, nq, xn, n, 8), reps, launches)
    return res


def index_part(x, q, target, k_lists, bf16, reps, launches):
    from sonar_amd import clustering, index, xsim

    n, nq = x.shape[0], q.shape[0]
    xn, qn = xsim.normalize_rows(x), xsim.normalize_rows(q)
    km = clustering.SphericalKMeans(k_lists, n_iter=2).fit_normalized(xn, n, init=x[:k_lists])
    ix = index.IVFFlatIndex(km).add(x)
    del xn
    torch.cuda.synchronize()
    res = {"K": k_lists}
    probes8 = ix.probe(q, 8)
    res["search_k8_nprobe8"] = {
        "probe_ms": windows_ms(lambda: xsim.topk_normalized(qn, nq, ix._c16, k_lists, 8), reps, launches),
        "scan_ms": windows_ms(lambda: index.search_lists(qn, probes8, ix._rows, ix._ids, ix._offsets, 8), reps, launches),
        "search_ms": windows_ms(lambda: ix.search(q, 8, 8), reps, launches)}
    ok = True
    for k, nprobe in ((16, 8), (16, 16), (16, 64), (64, 16)):
        probes = ix.probe_wide(q, nprobe)

        def scan():
            pages, below = [], None
            for kp in xsim.page_sizes(k):
                pages.append(index.search_lists_page(qn, probes, ix._rows, ix._ids, ix._offsets, kp, below))
                below = xsim.last_entry(*pages[-1])
            return pages

        r = {"probe_ms": windows_ms(lambda: xsim.topk_wide_normalized(qn, nq, ix._c16, k_lists, nprobe), reps, launches),
             "scan_ms": windows_ms(scan, reps, launches),
             "search_wide_ms": windows_ms(lambda: ix.search_wide(q, k, nprobe), reps, launches)}
        score, idx = ix.search_wide(q, k, nprobe)
        r["planted_first"] = int((idx[:, 0] == target).sum())
        r["in_order"] = in_order(score, idx)
        ok &= r["planted_first"] == nq and r["in_order"]
        res[f"search_wide_k{k}_nprobe{nprobe}"] = r
    bulk = bf16[1][:, 1:]
    recall = {}
    for nprobe in (8, 16, 32, 64):
        idx = ix.search_wide(q, 16, nprobe)[1]
        recall[f"nprobe{nprobe}"] = round(float((bulk[:, :, None] == idx[:, None, :]).any(dim=2).float().mean()), 6)
    res["recall_at_16_of_the_bulk_neighbours"] = recall
    res["self_check"] = ok
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--lists", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_wide_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk_wide needs an MI355X: there is no CPU path")
    from sonar_amd import xsim

    n, d, nq = args.rows, args.dim, args.queries
    out = {"metric": "topk_page_over_k8_pass", "config": f"{n} x {d} fp16 planted clusters, {nq} queries, one MI355X",
           "expectation": "a page costs the k = 8 pass within a few percent (the same MFMA work, a longer cascade), k = 64 four "
                          "pages; the scan scales with nprobe; the paged probe at K = 16 384 costs at most four probes"}
    ok = True
    for n_lists in args.lists:
        x, _ = planted(n, n_lists, d, seed=n_lists)
        q, target = queries(x, nq, seed=n_lists + 1)
        xn, qn = xsim.normalize_rows(x), xsim.normalize_rows(q)
        bf16 = xsim.topk_wide_normalized(qn, nq, xn, n, 16)
        if n_lists == args.lists[0]:
            out["brute_force"] = brute_force(xn, n, qn, nq, args.reps, args.launches)
            s64, i64 = xsim.topk_wide_normalized(qn, nq, xn, n, 64)
            s8, i8 = xsim.topk_normalized(qn, nq, xn, n, 8)
            check = {"planted_first": int((i64[:, 0] == target).sum()), "in_order": in_order(s64, i64),
                     "first_8_equal_the_k8_pass": bool(torch.equal(i64[:, :8], i8) and torch.equal(s64[:, :8], s8)),
                     "first_16_equal_one_page": bool(torch.equal(i64[:, :16], bf16[1]) and torch.equal(s64[:, :16], bf16[0]))}
            out["brute_force"]["self_check"] = check
            ok &= check["planted_first"] == nq and all(v for k, v in check.items() if k != "planted_first")
            del s64, i64, s8, i8
        del xn, qn
        res = index_part(x, q, target, n_lists, bf16, args.reps, args.launches)
        ok &= res["self_check"]
        out[f"K{n_lists}"] = res
        del x, q, target, bf16
        torch.cuda.empty_cache()
    out["value"] = out["brute_force"]["page16_over_k8_pass"]
    out["self_check"] = bool(ok)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not ok:
        raise SystemExit("the self-check failed: a planted neighbour is not first, or a page is out of order")


if __name__ == "__main__":
    main()
