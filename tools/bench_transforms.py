"""PCA / OPQ transforms (sonar_amd.transforms) on one MI355X: one JSON line, also written to
profiles/transforms_bench.json.

  Data: n = 1 M rows x 1024 fp16, anisotropic -- a spectrum falling geometrically from 1 to 0.05, mixed by a random
  orthogonal matrix, rows normalised (tests/transforms_ref.py `planted`, generated on the device in slabs).
  Timed, each in event windows of `--launches` back-to-back calls, median / min / max over `--reps` windows:
    gram        the symmetric form gram(x) and the cross form gram(x, y) at n x d (x d): the call (both kernels) and, as the median
                over the launches of one torch.profiler trace, gram_kernel and gram_reduce_kernel alone; TFLOP/s of the call from 2 n d1 d2
                (the symmetric form computes (T + 1) / 2T of that, T = d / 128 tiles a side, and is rated on what it computes)
    apply       LinearTransform.apply of the d x d rotation on the n rows
    one OPQ round split into its parts: apply / pq_train (`--pq-iter` Lloyd rounds) / pq_encode / pq_decode / gram(xn, xhat) /
                the host SVD of the d x d fp64 matrix (wall clock, the read-back included)
    PCA.fit     whole, wall clock (it synchronises), and its host eigh alone
  Derived expectation, unmeasured when written: 2 n d^2 = 2.2 TFLOP for the cross form, 1.1 for the symmetric one; at the
  458-596 TFLOP/s the head trainer's backward kernel reaches (the same loop), 2-5 ms; the host SVD of a 1024^2 fp64 matrix
  dominates an OPQ round.
  The run checks itself on the planted-data criterion of tests/test_gpu_transforms.py at its full size (4096 x 128, dsub 16,
  two rounds of 8 Lloyd rounds: OPQ error <= 0.6 x plain PQ's), and records the same two errors at n x d.
    python tools/bench_transforms.py [--rows 1000000] [--dim 1024] [--dsub 16] [--pq-iter 4] [--reps 5] [--launches 5]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_kmeans import windows_ms  # noqa: E402


def planted(n, d, seed, lo=0.05):
    """fp16 [n, d] on the device: tests/transforms_ref.py's planted rows, generated in slabs."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = lo ** (torch.arange(d, device="cuda", dtype=torch.float32) / (d - 1))
    mix = torch.linalg.qr(torch.randn(d, d, device="cuda", generator=g))[0]
    x = torch.empty(n, d, dtype=torch.float16, device="cuda")
    for r0 in range(0, n, 65536):
        m = min(65536, n - r0)
        v = (torch.randn(m, d, device="cuda", generator=g) * scale) @ mix
        x[r0:r0 + m] = torch.nn.functional.normalize(v, dim=1).half()
    return x


def gram_trace(fn, calls):
    """Device time in us of the two kernels of a gram call: the median over `calls` calls inside one torch.profiler trace; a
    note where that is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        seen = {}
        for ev in prof.events():
            name = next((s for s in ("gram_reduce_kernel", "gram_kernel") if s in ev.name), None)
            if ev.device_time > 0 and name:
                seen.setdefault(name, []).append(ev.device_time)
        out = {name: round(sorted(t)[len(t) // 2], 2) for name, t in seen.items()}
        out["launches"] = {name: len(t) for name, t in seen.items()}
        return out if seen else None
    except Exception as e:  # noqa: BLE001  (a measurement aid: the timed figures do not depend on it)
        return {"unavailable": repr(e)[:200]}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, round((time.perf_counter() - t0) * 1e3, 3)


def gram_leg(x, y, reps, launches):
    from sonar_amd import _lib

    lib = _lib.load()
    n, d1 = x.shape
    d2 = d1 if y is None else y.shape[1]
    ws_bytes = int(lib.smi_gram_ws_bytes(n, d1, d2))
    t = (d1 + 127) // 128
    if y is None:  # the upper triangle's tile slots
        ws_bytes = ws_bytes // (t * t) * (t * (t + 1) // 2)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(d1, d2, dtype=torch.float64, device="cuda")
    stream = _lib.current_stream_ptr()

    def call():
        _lib.check(lib.smi_gram(x.data_ptr(), None if y is None else y.data_ptr(), n, d1, d2, out.data_ptr(), ws.data_ptr(),
                                ws_bytes, stream))

    r = {"call_ms": windows_ms(call, reps, launches), "kernel_trace_us": gram_trace(call, reps * launches),
         "workspace_bytes": ws_bytes}
    flop = 2.0 * n * d1 * d2 * ((t + 1) / (2 * t) if y is None else 1.0)
    r["tflop_computed"] = round(flop / 1e12, 4)
    r["call_tflops"] = round(flop / (r["call_ms"]["median"] * 1e-3) / 1e12, 1)
    k_us = (r["kernel_trace_us"] or {}).get("gram_kernel")
    r["kernel_tflops"] = round(flop / (k_us * 1e-6) / 1e12, 1) if k_us else None
    return r


def opq_round(x, dsub, pq_iter, reps, launches):
    """One OPQ round at the size of x, split into its parts, and the errors under the start rotation and without any."""
    from sonar_amd import index, transforms, xsim
    from sonar_amd.clustering import init_rows

    n, d = x.shape
    xn = xsim.normalize_rows(x)
    init = init_rows(n, index.PQ_CODEWORDS, 0).to(device="cuda", dtype=torch.int32)
    (w, v), eigh_ms = wall_ms(lambda: transforms._eigh_descending(transforms.gram(xn, n=n).cpu()))
    order = [i for b in transforms.balanced_bins(w.tolist(), d // dsub) for i in b]
    t = transforms.LinearTransform(v[:, order].t().contiguous().cuda())
    r = {"gram_readback_eigh_wall_ms": eigh_ms}
    r["apply_ms"] = windows_ms(lambda: t.apply(xn[:n]), reps, launches)
    xr = t.apply(xn[:n])
    r["pq_train_ms"] = windows_ms(lambda: index.pq_train(xr, dsub, init, pq_iter, n), max(reps // 2, 1), 1)
    cb = index.pq_train(xr, dsub, init, pq_iter, n)
    r["pq_encode_ms"] = windows_ms(lambda: index.pq_encode(xr, cb, n), reps, 1)
    codes = index.pq_encode(xr, cb, n)
    r["pq_decode_ms"] = windows_ms(lambda: index.pq_decode(codes, cb), reps, launches)
    xhat = index.pq_decode(codes, cb)
    r["gram_cross_ms"] = windows_ms(lambda: transforms.gram(xn, xhat, n), reps, launches)
    m = transforms.gram(xn, xhat, n)
    _, r["readback_svd_wall_ms"] = wall_ms(lambda: torch.linalg.svd(m.cpu()))
    mh = m.cpu()
    t0 = time.perf_counter()
    torch.linalg.svd(mh)
    r["host_svd_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    device_ms = sum(r[k]["median"] for k in ("apply_ms", "pq_train_ms", "pq_encode_ms", "pq_decode_ms", "gram_cross_ms"))
    r["device_parts_ms"] = round(device_ms, 3)
    r["host_svd_share_of_round"] = round(r["host_svd_ms"] / (device_ms + r["host_svd_ms"]), 3)
    r["error_opq_start"] = round(transforms._relative_error(xr, xhat, n), 5)
    cb0 = index.pq_train(xn, dsub, init, pq_iter, n)
    r["error_plain_pq"] = round(transforms._relative_error(xn, index.pq_decode(index.pq_encode(xn, cb0, n), cb0), n), 5)
    r["error_ratio"] = round(r["error_opq_start"] / r["error_plain_pq"], 4)
    return r


def criterion():
    """tests/test_gpu_transforms.py's planted-data criterion."""
    from sonar_amd import transforms, xsim
    from sonar_amd.index import ProductQuantizer

    x = planted(4096, 128, 0)
    opq, fit_ms = wall_ms(lambda: transforms.OPQ.fit(x, 16, n_iter=2, pq_iter=8, seed=0))
    pq = ProductQuantizer.train(x, dsub=16, n_iter=16, seed=0)
    plain = transforms._relative_error(xsim.normalize_rows(x), pq.decode(pq.encode(x)), 4096)
    return {"n": 4096, "d": 128, "dsub": 16, "opq_fit_wall_ms": fit_ms, "error_plain_pq": round(plain, 5),
            "opq_history": [round(h, 5) for h in opq.history], "ratio": round(opq.history[-1] / plain, 4),
            "ok": opq.history[-1] <= 0.6 * plain}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--dsub", type=int, default=16)
    ap.add_argument("--pq-iter", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transforms_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_transforms needs an MI355X: there is no CPU path")
    from sonar_amd import transforms

    n, d = args.rows, args.dim
    out = {"metric": "gram_symmetric_call_ms",
           "config": f"{n} x {d} fp16 anisotropic rows (spectrum 1 .. 0.05), dsub {args.dsub}, {args.pq_iter} Lloyd rounds, one MI355X",
           "expectation": "2 n d^2 = 2.2 TFLOP cross / 1.1 symmetric at 1 M x 1024: 2-5 ms at the 458-596 TFLOP/s of "
                          "head_bwd_gemm_kernel (the same loop); the host SVD of a 1024^2 fp64 matrix dominates an OPQ round",
           "chunk_rows": transforms.GRAM_CHUNK_ROWS}
    out["criterion"] = criterion()
    x = planted(n, d, 1)
    y = planted(n, d, 2)
    out["gram_symmetric"] = gram_leg(x, None, args.reps, args.launches)
    out["gram_cross"] = gram_leg(x, y, args.reps, args.launches)
    del y
    torch.cuda.empty_cache()
    out["opq_round"] = opq_round(x, args.dsub, args.pq_iter, args.reps, args.launches)
    d_out = max(d // 2 // 128 * 128, 128)
    pca, out["pca_fit_wall_ms"] = wall_ms(lambda: transforms.PCA.fit(x, d_out))
    out["pca_d_out"] = d_out
    c = (transforms.gram(x) / (n - 1)).cpu()
    out["pca_explained_variance_share"] = round(float(pca.explained_variance.sum() / torch.trace(c)), 4)  # (uncentred trace)
    t0 = time.perf_counter()
    torch.linalg.eigh(c)
    out["host_eigh_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["value"] = out["gram_symmetric"]["call_ms"]["median"]
    out["ok"] = bool(out["criterion"]["ok"])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not out["ok"]:
        raise SystemExit("the OPQ error on the planted data is above 0.6 x plain PQ's")


if __name__ == "__main__":
    main()
