"""Head training (sonar_amd.head_training) on one MI355X: one JSON line, also written to profiles/head_training_bench.json.

  Heads, all at batch 512 (the notebook's 64 x 8 GPUs): the fine-tuning notebook's classifier [1024 -> 8192 -> 2] (tanh,
  cross-entropy, dropout 0.1), MuTox [1024 -> 512 -> 128 -> 1] (ReLU, BCE, input dropout 0.01) and BLASER basic_ref
  [6144 -> 3072 -> 1536 -> 1] (tanh, MSE, dropout 0.1), on random fp32 embeddings with planted labels.
  steps/s is a whole `fit` (enqueue of every step + the one read-back of the losses) over its step count.  Kernel times:
  the backward MFMA kernel at every hidden layer's two products (smi_head_bwd_gemm), 200 back-to-back launches between two
  HIP events, median / min / max over `--reps` such windows (the operands stay in cache from launch to launch, which a
  training step does not offer); and, where torch.profiler is available, the device time of every kernel of one training
  step from a kernel trace -- the only figures for the small kernels and AdamW.
  Derived expectation for the notebook head, to read next to the measurement: the step is bound by optimizer traffic,
  8.4 M parameters x ~30 B (p, m, v read and written, g read, shadow written) = ~250 MB, about 50 us at the achievable
  copy rate; the backward GEMMs are ~9 GFLOP (2 x 512 x 8192 x 1024 each way would be 17; the input layer needs no dA);
  so a step is on the order of 100 us.
    python tools/bench_head_training.py [--rows 4096] [--batch 512] [--epochs 8] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADS = {
    "notebook_classifier": dict(dims=[1024, 8192, 2], activation="TANH", loss="ce", p_in=0.0, p_hidden=0.1),
    "mutox": dict(dims=[1024, 512, 128, 1], activation="RELU", loss="bce", p_in=0.01, p_hidden=0.0),
    "blaser_basic_ref": dict(dims=[6144, 3072, 1536, 1], activation="TANH", loss="mse", p_in=0.1, p_hidden=0.1),
}


LAUNCHES = 200   # per event pair: a window of milliseconds, not of one 20 us launch


def event_us(fn, reps):
    """Per-launch time in us of `fn` (asynchronous launches only): `reps` windows of LAUNCHES back-to-back launches between
    two HIP events each -> (median, min, max) over the windows."""
    for _ in range(LAUNCHES):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = []
    for _ in range(reps):
        a.record()
        for _ in range(LAUNCHES):
            fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1e3 / LAUNCHES)
    t.sort()
    return t[len(t) // 2], t[0], t[-1]


def kernel_trace(fn):
    """Device time in us of every kernel of one call, from a torch.profiler trace; a note where that is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            if ev.device_time > 0 and ("smi" in ev.name or "kernel" in ev.name):
                name = ev.name.split("(")[0][-60:]
                out[name] = round(out.get(name, 0.0) + ev.device_time, 2)
        return out or None
    except Exception as e:  # noqa: BLE001  (a measurement aid: the timed figures do not depend on it)
        return {"unavailable": repr(e)[:200]}


def run_head(name, spec, rows, batch, epochs, reps):
    from sonar_amd import _lib
    from sonar_amd.head_training import HeadTrainer

    L, lib = _lib, _lib.load()
    dims = spec["dims"]
    g = torch.Generator().manual_seed(1)
    X = (0.5 * torch.randn(rows, dims[0], generator=g)).cuda()
    s = X @ (torch.randn(dims[0], generator=g) / dims[0] ** 0.5).cuda()
    y = {"ce": (s > 0).long(), "bce": (s > 0).float()[:, None], "mse": torch.tanh(2 * s)[:, None]}[spec["loss"]]
    tr = HeadTrainer(dims[0], dims[1:-1], dims[-1], activation=spec["activation"], loss=spec["loss"], p_in=spec["p_in"],
                     p_hidden=spec["p_hidden"], lr=1e-4, weight_decay=1e-3, warmup_steps=4, max_grad_norm=1.0, seed=1,
                     device="cuda:0", max_batch=batch)
    tr.fit(X, y, 1, batch)  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = tr.fit(X, y, epochs, batch)
    dt = time.perf_counter() - t0
    steps = len(losses)
    res = {"dims": dims, "batch": batch, "steps": steps, "steps_per_s": round(steps / dt, 1),
           "step_us": round(dt / steps * 1e6, 1), "rows_per_s": round(steps * batch / dt, 1),
           "first_loss": round(float(losses[0]), 5), "last_loss": round(float(losses[-1]), 5)}
    stream = L.current_stream_ptr()
    ker = {}
    for l in range(len(dims) - 2):
        i, o = dims[l], dims[l + 1]
        dz = torch.randn(batch, o, device="cuda").bfloat16()
        A = torch.randn(batch, i, device="cuda").half()
        W = torch.randn(o, i, device="cuda").half()
        gw = torch.empty(o, i, device="cuda")
        med, lo, hi = event_us(lambda: lib.smi_head_bwd_gemm(0, dz.data_ptr(), L.SMI_BF16, A.data_ptr(), L.SMI_F16, batch, o,
                                                             i, gw.data_ptr(), stream), reps)
        ker[f"gW{l}_{o}x{i}_us"] = {"median": round(med, 2), "min": round(lo, 2), "max": round(hi, 2)}
        ker[f"gW{l}_tflops"] = round(2.0 * batch * o * i / (med * 1e-6) / 1e12, 1)
        if l > 0:
            dA = torch.empty(batch, i, device="cuda")
            med, lo, hi = event_us(lambda: lib.smi_head_bwd_gemm(1, dz.data_ptr(), L.SMI_BF16, W.data_ptr(), L.SMI_F16, batch,
                                                                 o, i, dA.data_ptr(), stream), reps)
            ker[f"dA{l}_{batch}x{i}_us"] = {"median": round(med, 2), "min": round(lo, 2), "max": round(hi, 2)}
            ker[f"dA{l}_tflops"] = round(2.0 * batch * o * i / (med * 1e-6) / 1e12, 1)
    n = sum(a * b + b for a, b in zip(dims[:-1], dims[1:]))
    res["parameters"] = n
    res["kernels_alone"] = ker
    xb, yb = X[:batch], y[:batch]
    res["step_kernel_trace_us"] = kernel_trace(lambda: tr.step(xb, yb))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_training_bench.json"))
    args = ap.parse_args()
    out = {"metric": "head_training_steps_per_s",
           "config": f"batch {args.batch}, {args.rows} rows of fp32 embeddings, {args.epochs} epochs, AdamW + clip 1.0",
           "expectation_notebook_head": "optimizer traffic 8.4 M parameters x ~30 B = ~250 MB = ~50 us; backward GEMMs "
                                        "~9 GFLOP; a step on the order of 100 us"}
    for name, spec in HEADS.items():
        out[name] = run_head(name, spec, args.rows, args.batch, args.epochs, args.reps)
    out["value"] = out["notebook_classifier"]["steps_per_s"]
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
