"""Range search over the IVF-Flat lists (sonar_amd.index) on one MI355X: one JSON line, also written to
profiles/ivf_range_bench.json.

  Data: tools/bench_ivf.py's -- n = 1 M rows x 1024 fp16 with planted clusters, K = 1024 and K = 16 384 lists, 262 144
  queries, query j a noisy copy of a random corpus row; nprobe in {1, 4, 8}.  A query scores ~0.995 against its planted
  neighbour, ~0.73 against the other rows of that row's cluster and ~0 +- 0.1 against the rest, so
    leg "neighbour": threshold 0.9 isolates the planted neighbour, one hit per query, all `--queries` queries;
    leg "cluster":   threshold 0.45 returns the whole cluster of the neighbour (~n / K rows), the first `--cluster-queries`.
  Per K, leg and nprobe, each in event windows of `--launches` back-to-back calls, median / min / max over `--reps` windows:
  the count pass (smi_range_search_count: inversion of the probe table + the counting walk), the emit pass
  (smi_range_search_emit: the writing walk), the sort of the segments (three stable torch sorts), the whole
  `IVFFlatIndex.range_search` (normalise + probe + both passes + cumsum + read-back + sort), and -- the yardstick, in the same
  run on the same data -- the flat `search_lists(k = 8)`; the walking kernels of one call of each (ivf_range_lists in its two
  modes, ivf_scan_lists) from a torch.profiler trace.  The run checks itself: in the "neighbour" leg every query must
  return exactly its planted neighbour, in the "cluster" leg exactly the rows of the neighbour's list, the neighbour first.
  Derived expectation, to read next to the measurement: a pass runs the flat scan's loop with a lighter fold (a compare per
  sum and, on most tiles, nothing else, against the insertion into a sorted key list), so each pass costs about one flat
  scan or less; the "cluster" leg pays one LDS fetch-add and two scattered 4-byte stores per hit on top.
    python tools/bench_ivf_range.py [--rows 1000000] [--queries 262144] [--cluster-queries 16384] [--reps 5] [--launches 5]
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

NEIGHBOUR, CLUSTER = 0.9, 0.45
WALKS = ("ivf_range_lists", "ivf_scan_lists")


def walk_trace(fn):
    """Device time in us of the list-walking kernels of one call, from a torch.profiler trace; a note where that is not
    available."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            name = next((s for s in WALKS if s in ev.name), None)
            if ev.device_time > 0 and name:
                out[name] = round(out.get(name, 0.0) + ev.device_time, 2)
        return out or None
    except Exception as e:  # noqa: BLE001  (a measurement aid: the timed figures do not depend on it)
        return {"unavailable": repr(e)[:200]}


def leg(ix, q, qn, target, nprobe, threshold, want_hits, reps, launches):
    """One (threshold, nprobe) cell on the queries q: the timings and the self-check."""
    from sonar_amd import _lib, index

    lib = _lib.load()
    nq, d, k_lists = q.shape[0], q.shape[1], ix.n_lists
    probes = ix.probe(q, nprobe).contiguous()
    thr = torch.full((nq,), threshold, dtype=torch.float32, device="cuda")
    ws_bytes = int(lib.smi_range_search_ws_bytes(nq, k_lists, nprobe, d))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    counts = torch.empty(nq * nprobe, dtype=torch.int32, device="cuda")
    inputs = (qn.data_ptr(), nq, d, probes.data_ptr(), nprobe, thr.data_ptr(), ix._rows.data_ptr(), ix._ids.data_ptr(),
              ix._offsets.data_ptr(), k_lists)
    stream = _lib.current_stream_ptr()

    def count():
        _lib.check(lib.smi_range_search_count(*inputs, counts.data_ptr(), ws.data_ptr(), ws_bytes, stream))

    r = {"count_ms": windows_ms(count, reps, launches), "count_walk_trace_us": walk_trace(count)}
    base = torch.zeros(nq * nprobe + 1, dtype=torch.int64, device="cuda")
    base[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(base[-1].item())
    score = torch.empty(total, dtype=torch.float32, device="cuda")
    idx = torch.empty(total, dtype=torch.int32, device="cuda")

    def emit():  # on the workspace the last count left
        _lib.check(lib.smi_range_search_emit(*inputs, base.data_ptr(), total, score.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                                             ws_bytes, stream))

    r["hits"] = total
    r["emit_ms"] = windows_ms(emit, reps, launches)
    r["emit_walk_trace_us"] = walk_trace(emit)
    lims = base[::nprobe].contiguous()
    r["sort_ms"] = windows_ms(lambda: index._sort_segments(lims, score, idx), reps, launches)
    r["range_search_ms"] = windows_ms(lambda: ix.range_search(q, threshold, nprobe=nprobe), reps, launches)
    flat = lambda: index.search_lists(qn, probes, ix._rows, ix._ids, ix._offsets, 8)  # noqa: E731
    r["flat_list_search_k8_ms"] = windows_ms(flat, reps, launches)
    r["flat_walk_trace_us"] = walk_trace(flat)
    r["flat_search_k8_ms"] = windows_ms(lambda: ix.search(q, k=8, nprobe=nprobe), reps, launches)
    scan = (r["flat_walk_trace_us"] or {}).get("ivf_scan_lists")
    for name in ("count", "emit"):
        walk = (r[f"{name}_walk_trace_us"] or {}).get("ivf_range_lists")
        r[f"{name}_walk_over_flat_scan"] = round(walk / scan, 4) if walk and scan else None
    res = ix.range_search(q, threshold, nprobe=nprobe)
    first = res.ids[res.lims[:-1].clamp(max=max(total - 1, 0))] if total else res.ids
    r["queries_with_the_wanted_count"] = int((res.counts == want_hits).sum())  # (want_hits: an int, or one per query)
    r["queries_whose_best_hit_is_planted"] = int((first == target).sum()) if total else 0
    r["ok"] = r["queries_with_the_wanted_count"] == nq and r["queries_whose_best_hit_is_planted"] == nq
    return r


def run(x, q, target, k_lists, nprobes, cluster_queries, reps, launches):
    from sonar_amd import clustering, index, xsim

    n, d = x.shape
    xn, qn = xsim.normalize_rows(x), xsim.normalize_rows(q)
    km = clustering.SphericalKMeans(k_lists, n_iter=2).fit_normalized(xn, n, init=x[:k_lists])
    ix = index.IVFFlatIndex(km).add(x)
    torch.cuda.synchronize()
    del xn
    sizes = ix.list_sizes
    res = {"n": n, "d": d, "K": k_lists, "nq": q.shape[0], "cluster_queries": cluster_queries,
           "list_size_min_mean_max": [int(sizes.min()), round(float(sizes.float().mean()), 1), int(sizes.max())]}
    truth = target.long() % k_lists  # the planted cluster of row i is i % K, and the fit keeps cluster c in list c
    qc = q[:cluster_queries].contiguous()
    qcn = xsim.normalize_rows(qc)
    for nprobe in nprobes:
        res[f"nprobe{nprobe}"] = {
            "neighbour": leg(ix, q, qn, target, nprobe, NEIGHBOUR, 1, reps, launches),
            "cluster": leg(ix, qc, qcn, target[:cluster_queries], nprobe, CLUSTER, sizes[truth[:cluster_queries]].long(), reps,
                           launches)}
    res["ok"] = all(res[f"nprobe{p}"][name]["ok"] for p in nprobes for name in ("neighbour", "cluster"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=262144)
    ap.add_argument("--cluster-queries", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--lists", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_range_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivf_range needs an MI355X: there is no CPU path")
    n, d, nq = args.rows, args.dim, args.queries
    out = {"metric": "ivf_range_search_ms",
           "config": f"{n} x {d} fp16 planted clusters, {nq} queries at threshold {NEIGHBOUR} (the planted neighbour alone), "
                     f"{args.cluster_queries} at {CLUSTER} (its whole cluster), one MI355X",
           "expectation": "each pass runs the flat scan's loop with a lighter fold: about one flat scan (ivf_scan_lists, k = 8, "
                          "the same run) or less; the cluster leg adds one LDS fetch-add and two 4-byte stores per hit"}
    for k_lists in args.lists:
        x, _ = planted(n, k_lists, d, seed=k_lists)
        q, target = queries(x, nq, seed=k_lists + 1)
        out[f"K{k_lists}"] = run(x, q, target, k_lists, args.nprobe, min(args.cluster_queries, nq), args.reps, args.launches)
        del x, q, target
        torch.cuda.empty_cache()
    out["value"] = out[f"K{args.lists[0]}"][f"nprobe{args.nprobe[0]}"]["neighbour"]["range_search_ms"]["median"]
    out["ok"] = all(out[f"K{k}"]["ok"] for k in args.lists)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not out["ok"]:
        raise SystemExit("a query did not return exactly its planted neighbour / its neighbour's cluster")


if __name__ == "__main__":
    main()
