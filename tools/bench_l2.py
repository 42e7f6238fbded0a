"""L2 entries against their cosine counterparts on one MI355X: one JSON line, also written to
profiles/l2_bench.json.

  Data: tools/bench_kmeans.py's planted clusters, n = 1 M rows x 1024 fp16 over 1024 centres, every row scaled by a factor
  drawn uniformly from 0.5 .. 2 (rows of different lengths: the L2, the inner-product and the cosine order differ); 262 144
  queries, query j a noisy copy of a random corpus row, which is its planted L2 neighbour.  The cosine entries run on the
  normalised copies of the same rows.  Everything is timed in ONE run, in event windows of `--launches` calls, median / min /
  max over `--reps`:
  (a) brute force, queries x corpus, k = 1 and 4: smi_l2_topk against smi_xsim_topk (both on prepared / normalised rows);
  (b) one k-means round (update -> finalise -> assign) at K = 1024: KMeans.step against SphericalKMeans.step;
  (c) the index, K = 1024 lists, k = 4, nprobe = 1, 4, 8: the L2 scan against the cosine scan over the SAME lists and probes
      (what the bias costs the kernel), and IVFFlatL2Index.search against IVFFlatIndex.search, each with its own quantiser
      (the lists differ: Euclidean clusters of rows of different lengths are not the cosine clusters; sizes recorded).
  Derived expectation: the bias costs 16 adds and four LDS reads per lane and y tile in a fold that is ~12 % of the stream, and
  one 16-byte load per four slots in the scan: every ratio a little above 1.
  The run checks itself: the planted L2 neighbour is first in every row of the brute-force results (the exact search), the
  distances are non-decreasing everywhere, and the index -- an approximate search: a query at a cluster boundary may not probe
  its neighbour's list -- finds it first in at least 0.999 of the rows at nprobe = 8 (the count is recorded).
    python tools/bench_l2.py [--rows 1000000] [--queries 262144] [--reps 3] [--launches 1]
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


def scaled(x, seed):
    """The rows of x times a per-row factor from 0.5 .. 2, in slabs."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty_like(x)
    for r0 in range(0, x.shape[0], 131072):
        m = min(131072, x.shape[0] - r0)
        out[r0:r0 + m] = (x[r0:r0 + m].float() * (0.5 + 1.5 * torch.rand(m, 1, device="cuda", generator=g))).half()
    return out


def queries(x, nq, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n, d = x.shape
    target = torch.randint(0, n, (nq,), device="cuda", generator=g)
    q = x[target].float() + 0.1 / d ** 0.5 * torch.randn(nq, d, device="cuda", generator=g)
    return q.half(), target.int()


def ratio(res, a, b):
    return round(res[a]["median"] / res[b]["median"], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--lists", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l2_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_l2 needs an MI355X: there is no CPU path")
    from sonar_amd import clustering, index, xsim

    n, d, nq, K, reps, launches = args.rows, args.dim, args.queries, args.lists, args.reps, args.launches
    out = {"metric": "l2_topk_over_cosine_topk", "config": f"{n} x {d} fp16 planted clusters with row lengths 0.5 .. 2, {nq} queries, one MI355X",
           "expectation": "16 adds and four LDS reads per lane and tile, one 16-byte load per four slots: a little above 1 x"}
    x = scaled(planted(n, K, d, seed=K)[0], seed=K + 2)
    q, target = queries(x, nq, seed=K + 1)
    (x16, hx), (q16, hq) = xsim.prepare_rows(x), xsim.prepare_rows(q)
    xn, qn = xsim.normalize_rows(x), xsim.normalize_rows(q)
    bias = hx.neg()
    ok = True

    # (a) brute force
    bf = {}
    for k in (1, 4):
        bf[f"cosine_k{k}_ms"] = windows_ms(lambda: xsim.topk_normalized(qn, nq, xn, n, k), reps, launches)
        bf[f"l2_k{k}_ms"] = windows_ms(lambda: xsim.topk_bias_prepared(q16, nq, x16, n, bias, k), reps, launches)
        bf[f"l2_over_cosine_k{k}"] = ratio(bf, f"l2_k{k}_ms", f"cosine_k{k}_ms")
        dist, idx, _ = xsim.topk_l2_prepared(q16, nq, hq, x16, n, hx, k)
        first = int((idx[:, 0] == target).sum())
        ordered = bool((dist[:, :-1] <= dist[:, 1:]).all())
        bf[f"self_check_k{k}"] = {"planted_first": first, "non_decreasing": ordered}
        ok &= first == nq and ordered
    bf["cosine_k1_again_ms"] = windows_ms(lambda: xsim.topk_normalized(qn, nq, xn, n, 1), reps, launches)  # the yardstick's own drift
    bf["prepare_rows_ms"] = windows_ms(lambda: xsim.prepare_rows(x), reps, launches)
    bf["normalize_rows_ms"] = windows_ms(lambda: xsim.normalize_rows(x), reps, launches)
    out["brute_force"] = bf

    # (b) one k-means round
    km_l2 = clustering.KMeans(K, n_iter=1).fit_prepared(x16, hx, n, init=x[:K])
    km_cos = clustering.SphericalKMeans(K, n_iter=1).fit_normalized(xn, n, init=x[:K])
    km = {"K": K, "l2_round_ms": windows_ms(km_l2.step, reps, launches), "cosine_round_ms": windows_ms(km_cos.step, reps, launches)}
    km["l2_over_cosine"] = ratio(km, "l2_round_ms", "cosine_round_ms")
    km["l2_history"] = {key: v[:4] for key, v in km_l2.history.items()}
    out["kmeans"] = km

    # (c) the index.  The kernels are compared on the SAME lists and the SAME probes (the cosine quantiser's: the units of the
    # two scans are then the same); the searches end to end each with its own quantiser, whose lists differ -- Euclidean
    # clusters of rows of different lengths are not the cosine clusters, and their sizes are recorded.
    def sizes(ix):
        s = ix.list_sizes
        return [int(s.min()), round(float(s.float().mean()), 1), int(s.max())]

    ix_cos = index.IVFFlatIndex(km_cos).add(x)
    ix_same = index.IVFFlatL2Index(km_l2).add(x, labels=km_cos.labels)
    ix_l2 = index.IVFFlatL2Index(km_l2).add(x)
    res = {"K": K, "k": 4, "list_size_min_mean_max": {"cosine": sizes(ix_cos), "l2": sizes(ix_l2)}}
    for nprobe in (1, 4, 8):
        probes = ix_cos.probe(q, nprobe)
        res[f"l2_scan_nprobe{nprobe}_ms"] = windows_ms(
            lambda: index.search_lists_l2(q16, probes, ix_same._rows, ix_same._bias, ix_same._ids, ix_same._offsets, 4), reps, launches)
        res[f"cosine_scan_nprobe{nprobe}_ms"] = windows_ms(
            lambda: index.search_lists(qn, probes, ix_cos._rows, ix_cos._ids, ix_cos._offsets, 4), reps, launches)
        res[f"l2_scan_over_cosine_scan_nprobe{nprobe}"] = ratio(res, f"l2_scan_nprobe{nprobe}_ms", f"cosine_scan_nprobe{nprobe}_ms")
        dist, idx = ix_same.search(q, 4, probes=probes)
        res[f"same_lists_planted_first_nprobe{nprobe}"] = int((idx[:, 0] == target).sum())
        ok &= bool((dist[:, :-1] <= dist[:, 1:]).all())
        res[f"l2_search_nprobe{nprobe}_ms"] = windows_ms(lambda: ix_l2.search(q, 4, nprobe), reps, launches)
        res[f"cosine_search_nprobe{nprobe}_ms"] = windows_ms(lambda: ix_cos.search(q, 4, nprobe), reps, launches)
        res[f"l2_search_over_cosine_search_nprobe{nprobe}"] = ratio(res, f"l2_search_nprobe{nprobe}_ms", f"cosine_search_nprobe{nprobe}_ms")
        dist, idx = ix_l2.search(q, 4, nprobe)
        res[f"planted_first_nprobe{nprobe}"] = int((idx[:, 0] == target).sum())
        ok &= bool((dist[:, :-1] <= dist[:, 1:]).all())
    ok &= res["planted_first_nprobe8"] >= 0.999 * nq and res["same_lists_planted_first_nprobe8"] >= 0.999 * nq
    out["index"] = res

    out["value"] = bf["l2_over_cosine_k1"]
    out["self_check"] = bool(ok)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not ok:
        raise SystemExit("the self-check failed: a planted L2 neighbour is not first, or distances decrease")


if __name__ == "__main__":
    main()
