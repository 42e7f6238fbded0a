"""extend / remove / merge_from of the IVF indexes (sonar_amd.index) on one MI355X: one JSON line, also
written to profiles/ivf_extend_bench.json.

  Data: n = 1 M rows x 1024 fp16 with planted clusters (tools/bench_kmeans.py's generator), K = 1024 and K = 16 384 lists in
  one run; 4096 queries, query j a noisy copy of a random corpus row (tools/bench_ivf.py's).  The quantiser is SphericalKMeans
  fitted on the corpus (2 rounds from the first member of each cluster); every variant is given its labels, so what is timed
  is normalise + encode + the storage work, not the assignment.
  Per K, on `IVFFlatIndex`, each in event windows of `--launches` back-to-back calls, median / min / max over `--reps`:
    add of all rows;  extend by the last 10 % of an index that holds the first 90 %;  ten chunks of 10 % (one add, nine
    extends);  remove of 10 % of the rows;  merge_from of two halves;  and, at list level, smi_ivf_build of the union and
    smi_lists_regroup of 90 % + 10 % with the kernels of one call from a torch.profiler trace -- the move kernel with its bytes
    read and written over its time, next to the build's ivf_gather_kernel and a device-to-device copy of the same bytes.
  Once each, at the first K: the same add / extend on `IVFInt8Index` and on `IVFPQIndex` at dsub = 16.
  The run checks itself: after every variant `search(k = 4, nprobe = 1)` must find every planted neighbour that is still in
  the index (flat and int8; on the PQ index the count is reported and the result must equal the one-shot index's).
  Derived expectation, unmeasured, to read next to the measurement: an extend copies (old + new) bytes at about the rate of
  the build's gather and buckets (old slots + new rows) keys where the build buckets n labels: roughly one build of the
  union per call.  There is no pass mark; the ratios against smi_ivf_build of the union in the same run are in the JSON.
    python tools/bench_ivf_extend.py [--rows 1000000] [--reps 5] [--launches 3]
"""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ivf import queries  # noqa: E402
from bench_kmeans import planted, windows_ms  # noqa: E402

KERNELS = ("ivf_regroup_move", "ivf_regroup_keys", "ivf_regroup_scatter", "bucket_hist", "ivf_scan_kernel", "bucket_scatter",
           "ivf_gather", "Memset", "memset")


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


def found(ix, q, target, gone=None):
    """(queries whose planted neighbour is still in the index, those of them whose search returns it first, whether a removed
    row came back)."""
    _, idx = ix.search(q, k=4, nprobe=1)
    live = torch.ones_like(target, dtype=torch.bool) if gone is None else ~gone[target.long()]
    ghost = False if gone is None else bool(gone[idx.clamp_min(0).long()][idx >= 0].any())
    return int(live.sum()), int((idx[:, 0] == target)[live].sum()), ghost


def variants(make, x, labels, q, target, reps, launches, chunks=10):
    """The timed variants of one index class; make(): an empty index."""
    n = x.shape[0]
    cut, half, step = n - n // chunks, n // 2, n // chunks
    res, checks = {}, {}

    def check(name, ix, gone=None):
        live, hit, ghost = found(ix, q, target, gone)
        checks[name] = {"planted_in_index": live, "planted_found": hit, "removed_row_returned": ghost}
        return ix

    whole = check("add_all", make().add(x, labels))
    res["add_all_ms"] = windows_ms(lambda: make().add(x, labels), reps, launches)
    head = make().add(x[:cut], labels[:cut])
    check("add_90_extend_10", copy.copy(head).extend(x[cut:], labels[cut:]))
    res["extend_10_of_90_ms"] = windows_ms(lambda: copy.copy(head).extend(x[cut:], labels[cut:]), reps, launches)

    def in_chunks():
        ix = make().add(x[:step], labels[:step])
        for r0 in range(step, n, step):
            ix.extend(x[r0: r0 + step], labels[r0: r0 + step])
        return ix

    check("ten_chunks", in_chunks())
    res["ten_chunks_ms"] = windows_ms(in_chunks, max(2, reps // 2), 1)
    gone = torch.zeros(n, dtype=torch.bool, device=x.device)
    gone[torch.randperm(n, device=x.device, generator=torch.Generator(device=x.device).manual_seed(7))[: n // 10]] = True
    check("remove_10", copy.copy(whole).remove(mask=gone), gone)
    res["remove_10_ms"] = windows_ms(lambda: copy.copy(whole).remove(mask=gone), reps, launches)
    a, b = make().add(x[:half], labels[:half]), make().add(x[half:], labels[half:])
    check("merge_halves", copy.copy(a).merge_from(b))
    res["merge_halves_ms"] = windows_ms(lambda: copy.copy(a).merge_from(b), reps, launches)
    res["self_check"] = checks
    return res, whole, head


def run(x, labels, q, target, k_lists, reps, launches, copy_tbps, quantised):
    from sonar_amd import clustering, index, xsim

    n, d = x.shape
    xn = xsim.normalize_rows(x)
    km = clustering.SphericalKMeans(k_lists, n_iter=2).fit_normalized(xn, n, init=x[:k_lists])
    labels = km.labels.contiguous()
    res, whole, head = variants(lambda: index.IVFFlatIndex(km), x, labels, q, target, reps, launches)
    res = {"n": n, "d": d, "K": k_lists, **res}
    # list level: the build of the union against the regroup of 90 % + 10 %, and their kernels
    cut = head._next_id
    build = lambda: index.build_lists(xn, labels, k_lists)  # noqa: E731
    old = (head._rows, None, head._ids, head._offsets)
    new = (xn[cut:], None, labels[cut:], None)
    regroup = lambda: index.regroup_lists(k_lists, old, new, cut, cut)  # noqa: E731
    res["build_of_the_union_ms"] = windows_ms(build, reps, launches)
    res["regroup_90_plus_10_ms"] = windows_ms(regroup, reps, launches)
    res["build_kernel_trace_us"] = kernel_trace(build)
    res["regroup_kernel_trace_us"] = kernel_trace(regroup)
    used = int(whole.list_offsets[-1])
    moved = 2 * used * (d * 2 + 4)  # every slot in use read and written once: its row and its id
    res["slots_used"], res["move_bytes_read_plus_written"] = used, moved
    for name, trace, kernel in (("move_kernel", res["regroup_kernel_trace_us"], "ivf_regroup_move"),
                                ("build_gather_kernel", res["build_kernel_trace_us"], "ivf_gather")):
        us = (trace or {}).get(kernel)
        res[name + "_TBps"] = round(moved / (us * 1e-6) / 1e12, 3) if us else None
    res["copy_read_plus_write_TBps"] = copy_tbps
    union = res["build_of_the_union_ms"]["median"]
    res["ratio_to_build_of_the_union"] = {
        key[:-3]: round(res[key]["median"] / union, 3)
        for key in ("add_all_ms", "extend_10_of_90_ms", "ten_chunks_ms", "remove_10_ms", "merge_halves_ms", "regroup_90_plus_10_ms")}
    res["ratio_to_add_all"] = {key[:-3]: round(res[key]["median"] / res["add_all_ms"]["median"], 3)
                               for key in ("extend_10_of_90_ms", "ten_chunks_ms", "remove_10_ms", "merge_halves_ms")}
    ok = all(c["planted_found"] == c["planted_in_index"] and not c["removed_row_returned"] for c in res["self_check"].values())
    if quantised:
        cent = km.centroids_normalized
        pq = index.ProductQuantizer.train(x[:131072], dsub=16, n_iter=4)
        for name, make, exact in (("int8", lambda: index.IVFInt8Index(cent), True), ("pq_dsub16", lambda: index.IVFPQIndex(cent, pq), False)):
            cut = n - n // 10
            one = make().add(x, labels)
            two = make().add(x[:cut], labels[:cut]).extend(x[cut:], labels[cut:])
            r = {"add_all_ms": windows_ms(lambda: make().add(x, labels), reps, launches)}
            part = make().add(x[:cut], labels[:cut])
            r["extend_10_of_90_ms"] = windows_ms(lambda: copy.copy(part).extend(x[cut:], labels[cut:]), reps, launches)
            r["ratio_extend_to_add_all"] = round(r["extend_10_of_90_ms"]["median"] / r["add_all_ms"]["median"], 3)
            live, hit, _ = found(two, q, target)
            r["planted_in_index"], r["planted_found"] = live, hit
            r["search_equals_the_one_shot_index"] = all(torch.equal(s, t) for s, t in zip(two.search(q, k=4, nprobe=1),
                                                                                         one.search(q, k=4, nprobe=1)))
            ok = ok and r["search_equals_the_one_shot_index"] and (hit == live or not exact)
            res[name] = r
            del one, two, part
            torch.cuda.empty_cache()
    res["self_check_passed"] = ok
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--lists", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_extend_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivf_extend needs an MI355X: there is no CPU path")
    n, d = args.rows, args.dim
    out = {"metric": "ivf_extend_ms", "config": f"{n} x {d} fp16 planted clusters, labels given, one MI355X",
           "expectation": "derived, unmeasured: an extend copies (old + new) bytes at about the rate of the build's gather and "
                          "buckets (old slots + new rows) keys: roughly one build of the union per call; no pass mark"}
    src = torch.empty(n, d, dtype=torch.float16, device="cuda").normal_()
    dst = torch.empty_like(src)
    cp = windows_ms(lambda: dst.copy_(src), args.reps, args.launches)
    copy_tbps = round(2 * n * d * 2 / (cp["median"] * 1e-3) / 1e12, 3)
    del src, dst
    for j, k_lists in enumerate(args.lists):
        x, labels = planted(n, k_lists, d, seed=k_lists)
        q, target = queries(x, args.queries, seed=k_lists + 1)
        out[f"K{k_lists}"] = run(x, labels, q, target, k_lists, args.reps, args.launches, copy_tbps, quantised=j == 0)
        del x, q, target
        torch.cuda.empty_cache()
    first = out[f"K{args.lists[0]}"]
    out["value"] = first["extend_10_of_90_ms"]["median"]
    out["self_check_passed"] = all(out[f"K{k}"]["self_check_passed"] for k in args.lists)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not out["self_check_passed"]:
        raise SystemExit("a planted neighbour was not found after one of the variants")


if __name__ == "__main__":
    main()
