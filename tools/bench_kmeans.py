"""Spherical k-means (sonar_amd.clustering) on one MI355X: one JSON line, also written to profiles/kmeans_bench.json.

  Data: n = 1 M rows x 1024 fp16 with planted clusters (K unit Gaussian directions, row i belongs to cluster i % K and is
  normalise(centre + 0.6 g / sqrt(d)); the initial centroids are the first member of each cluster), K = 1024 and
  K = 16 384, 10 rounds.  The run checks itself: every planted label must be recovered.
  Per K: the whole `fit` between two HIP events (everything is enqueued, nothing is read back), and one round split into
  assign (smi_xsim_topk, k = 1), update (smi_kmeans_update) and finalise (smi_kmeans_finalize), each in event windows of
  `--launches` back-to-back launches, median / min / max over `--reps` windows.
  Derived expectation, to read next to the measurement: assign costs n K pairs at the mining rate (5.8-6.4e11 pairs/s:
  ~1.7 ms at K = 1024, ~27 ms at K = 16 384); update reads the 2 GB matrix once, so it is reported as bytes / time next
  to the chip's copy rate measured in the same run (a device-to-device copy of the same matrix, read + write bytes), and
  as a share of the K = 1024 round.
    python tools/bench_kmeans.py [--rows 1000000] [--rounds 10] [--reps 5] [--launches 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows_ms(fn, reps, launches):
    """Per-launch time in ms of `fn` (asynchronous launches only) -> (median, min, max) over `reps` event windows."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = []
    for _ in range(reps):
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) / launches)
    t.sort()
    return {"median": round(t[len(t) // 2], 4), "min": round(t[0], 4), "max": round(t[-1], 4)}


def kernel_trace(fn):
    """Device time in us of every kernel of one call, from a torch.profiler trace; a note where that is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            if ev.device_time > 0 and any(s in ev.name for s in ("km_", "bucket_", "xsim", "l2norm", "pack", "Memset", "memset")):
                name = ev.name.split("(")[0][-48:]
                out[name] = round(out.get(name, 0.0) + ev.device_time, 2)
        return out or None
    except Exception as e:  # noqa: BLE001  (a measurement aid: the timed figures do not depend on it)
        return {"unavailable": repr(e)[:200]}


def planted(n, k, d, seed):
    """(x fp16 [n, d] on the device, planted labels int32 [n]); generated in slabs, a multiple of k rows each."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn(k, d, device="cuda", generator=g), dim=1)
    x = torch.empty(n, d, dtype=torch.float16, device="cuda")
    slab = max(k, 131072 // k * k)
    for r0 in range(0, n, slab):
        m = min(slab, n - r0)
        lab = torch.arange(r0, r0 + m, device="cuda") % k
        v = centres[lab] + 0.6 / d ** 0.5 * torch.randn(m, d, device="cuda", generator=g)
        x[r0:r0 + m] = torch.nn.functional.normalize(v, dim=1).half()
    return x, (torch.arange(n, device="cuda") % k).int()


def run(x, truth, k, rounds, reps, launches):
    from sonar_amd import _lib, clustering, xsim

    lib = _lib.load()
    n, d = x.shape
    xn = xsim.normalize_rows(x)
    init = x[:k]
    km = clustering.SphericalKMeans(k, n_iter=1).fit_normalized(xn, n, init=init)  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    km = clustering.SphericalKMeans(k, n_iter=rounds)
    a.record()
    km.fit_normalized(xn, n, init=init)
    b.record()
    torch.cuda.synchronize()
    fit_ms = a.elapsed_time(b)
    recovered = int((km.labels == truth).sum())
    hist = km.history
    res = {"n": n, "d": d, "K": k, "rounds": rounds, "fit_ms": round(fit_ms, 3),
           "round_ms_from_fit": round(fit_ms / (rounds + 1), 4),  # rounds + 1 assignments, `rounds` updates
           "planted_labels_recovered": recovered, "all_recovered": recovered == n,
           "objective_first_last": [hist["objective"][0], hist["objective"][-1]], "moved": hist["moved"],
           "empty": hist["empty"]}
    # one round, piece by piece, on the fitted state
    st = _lib.current_stream_ptr()
    c16 = km._c16
    res["assign_ms"] = windows_ms(lambda: xsim.topk_normalized(xn, n, c16, k, 1), reps, launches)
    ws_bytes = int(lib.smi_kmeans_workspace_bytes(n, k, d))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    sums = torch.empty((k, d), dtype=torch.int64, device="cuda")
    counts = torch.empty((k,), dtype=torch.int32, device="cuda")
    labels = km.labels
    res["update_ms"] = windows_ms(lambda: _lib.check(lib.smi_kmeans_update(
        xn.data_ptr(), labels.data_ptr(), n, d, k, sums.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws_bytes, st)),
        reps, launches)
    assert torch.equal(sums, km.sums) and torch.equal(counts, km.counts)
    res["update_kernel_trace_us"] = kernel_trace(lambda: _lib.check(lib.smi_kmeans_update(
        xn.data_ptr(), labels.data_ptr(), n, d, k, sums.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws_bytes, st)))
    res["assign_kernel_trace_us"] = kernel_trace(lambda: xsim.topk_normalized(xn, n, c16, k, 1))
    c32, c16b, empty = km.centroids.clone(), c16.clone(), torch.empty(1, dtype=torch.int32, device="cuda")
    res["finalize_ms"] = windows_ms(lambda: _lib.check(lib.smi_kmeans_finalize(
        sums.data_ptr(), counts.data_ptr(), k, d, c32.data_ptr(), c16b.data_ptr(), empty.data_ptr(), ws.data_ptr(), ws_bytes,
        st)), reps, launches)
    # all one cluster: the same bytes, one destination
    one = torch.zeros_like(labels)
    res["update_one_cluster_ms"] = windows_ms(lambda: _lib.check(lib.smi_kmeans_update(
        xn.data_ptr(), one.data_ptr(), n, d, k, sums.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws_bytes, st)),
        reps, launches)
    x_bytes = n * d * 2
    res["update_read_TBps"] = round(x_bytes / (res["update_ms"]["median"] * 1e-3) / 1e12, 3)
    piece_sum = res["assign_ms"]["median"] + res["update_ms"]["median"] + res["finalize_ms"]["median"]
    res["update_share_of_round"] = round(res["update_ms"]["median"] / piece_sum, 3)
    res["assign_pairs_per_s"] = round(n * k / (res["assign_ms"]["median"] * 1e-3), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--clusters", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_bench.json"))
    args = ap.parse_args()
    n, d = args.rows, args.dim
    out = {"metric": "kmeans_round_ms", "config": f"{n} x {d} fp16 planted clusters, {args.rounds} rounds, one MI355X",
           "expectation": "assign = n K pairs at the mining rate 5.8-6.4e11 pairs/s (1.7 ms at K = 1024, 27 ms at "
                          "K = 16384); update = one read of the n x d fp16 matrix"}
    src = torch.empty(n, d, dtype=torch.float16, device="cuda").normal_()
    dst = torch.empty_like(src)
    cp = windows_ms(lambda: dst.copy_(src), args.reps, args.launches)
    out["copy_ms"] = cp
    out["copy_read_plus_write_TBps"] = round(2 * n * d * 2 / (cp["median"] * 1e-3) / 1e12, 3)
    del src, dst
    for k in args.clusters:
        x, truth = planted(n, k, d, seed=k)
        out[f"K{k}"] = run(x, truth, k, args.rounds, args.reps, args.launches)
        del x, truth
        torch.cuda.empty_cache()
    first = out[f"K{args.clusters[0]}"]
    out["value"] = first["round_ms_from_fit"]
    out["all_recovered"] = all(out[f"K{k}"]["all_recovered"] for k in args.clusters)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not out["all_recovered"]:
        raise SystemExit("planted labels were not recovered")


if __name__ == "__main__":
    main()
