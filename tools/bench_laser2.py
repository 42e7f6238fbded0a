"""LASER2 BiLSTM encoder (arch `laser2`: 5 layers x 2 directions, H = 512, embed 320) on one MI355X: one JSON line.

  sentences/s at 1024 x 128 tokens and at 1024 ragged sentences of 8..64 tokens (seeded); latency of a batch of 5; us per
  recurrent step; TFLOP/s and the fraction of the 2.5 PF dense fp16 peak; a CPU fp32 torch.nn.LSTM baseline on the first 32
  rows of the 1024 x 128 batch with its max |delta| and 1 - cos against the engine's rows.
Synthetic weights (uniform in +-1/sqrt(H), the nn.LSTM init range); vocabulary cut to 8000 rows (the table is not read
per token beyond the gather).   python tools/bench_laser2.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 2500.0


def flops(cfg, tokens):
    """Multiply-adds x 2 of the input projections and the recurrence (gate math not counted)."""
    nd = 2 if cfg.bidirectional else 1
    H, per_tok = cfg.hidden_size, 0
    for k in range(cfg.num_layers):
        in_dim = cfg.model_dim if k == 0 else nd * H
        per_tok += nd * 2 * 4 * H * (in_dim + H)
    return per_tok * tokens


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-rows", type=int, default=32)
    args = ap.parse_args()
    from sonar_amd.laser2 import Laser2Model, get_laser2_config, _lstm_keys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_laser2 import cpu_laser2

    cfg = get_laser2_config("laser2")
    cfg.vocabulary_size = 8000
    g = torch.Generator().manual_seed(0)
    lim = cfg.hidden_size ** -0.5
    sd = {"embed_tokens.weight": torch.randn(cfg.vocabulary_size, cfg.model_dim, generator=g) * 0.5}
    for group in _lstm_keys(cfg):
        for k, shape in group:
            sd[k] = (torch.rand(shape, generator=g) * 2 - 1) * lim
    dev = "cuda:0"
    model = Laser2Model(cfg, sd, device=dev)
    out = {"metric": "laser2_sentences_per_s", "config": "laser2 5x2x512, embed 320"}

    x = torch.randint(3, cfg.vocabulary_size, (1024, 128), generator=g)
    lens = torch.full((1024,), 128, dtype=torch.int32)
    xd = x.to(dev)
    dt = timed(lambda: model(xd, lens), args.reps)
    steps = cfg.num_layers * 128
    fl = flops(cfg, 1024 * 128)
    out["full_1024x128"] = {"ms": round(dt * 1e3, 3), "sentences_per_s": round(1024 / dt, 1),
                            "tflops": round(fl / dt / 1e12, 1), "fraction_of_peak": round(fl / dt / 1e12 / PEAK_TFLOPS, 4),
                            "us_per_recurrent_step_incl_projection": round(dt * 1e6 / steps, 2)}
    out["value"] = out["full_1024x128"]["sentences_per_s"]

    rl = torch.randint(8, 65, (1024,), generator=g, dtype=torch.int32)
    rl[0] = 64
    xr = torch.randint(3, cfg.vocabulary_size, (1024, 64), generator=g)
    for i, l in enumerate(rl.tolist()):
        xr[i, l:] = cfg.pad_idx
    xrd = xr.to(dev)
    dt = timed(lambda: model(xrd, rl), args.reps)
    fl = flops(cfg, int(rl.sum()))
    out["ragged_1024x8_64"] = {"ms": round(dt * 1e3, 3), "sentences_per_s": round(1024 / dt, 1),
                               "tokens": int(rl.sum()), "tflops": round(fl / dt / 1e12, 1)}

    x5, l5 = x[:5, :30].contiguous().to(dev), torch.full((5,), 30, dtype=torch.int32)
    dt = timed(lambda: model(x5, l5), args.reps * 4)
    out["batch5_30tok"] = {"ms": round(dt * 1e3, 3), "us_per_recurrent_step": round(dt * 1e6 / (cfg.num_layers * 30), 2)}

    emb = model(xd, lens).cpu()
    n = args.cpu_rows
    t0 = time.perf_counter()
    ref = cpu_laser2(cfg, sd, x[:n], lens[:n])
    tc = time.perf_counter() - t0
    out["cpu_baseline"] = {"kind": "torch.nn.LSTM fp32", "rows": n, "sentences_per_s": round(n / tc, 2),
                           "threads": torch.get_num_threads(),
                           "max_abs_delta": float((emb[:n] - ref).abs().max()),
                           "max_1_minus_cos": float((1 - F.cosine_similarity(emb[:n].double(), ref.double(), dim=-1)).max())}
    out["device_bytes"] = model.device_bytes()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
