"""Teacher-forced scoring (TextDecoderEngine.score) on one MI355X: one JSON line.

  basic synthetic fp16 decoder (24 x 1024, vocab 256206): 256 sentences x 64 tokens and 256 ragged sentences of 8..128
  tokens.  For each: call ms, scored tokens/s, TFLOP/s and the fraction of the 2.5 PF dense fp16 peak (FLOPs from the
  shapes: 24 x 2 (4 d^2 + 2 d f) + 2 d V per scored row, the padding the call computes not counted), and the old route --
  logits() + log_softmax + gather -- on the same sentences, with the speed-up of the new one.
    python tools/bench_score.py [--reps 3]
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

PEAK_TFLOPS = 2500.0


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def old_route(eng, emb, toks, lens, chunk=32):
    """logits() + log_softmax + gather (in sentence chunks: the fp32 [n, t, V] logits of a whole call do not fit)."""
    n, t = toks.shape
    out = torch.zeros(n, t - 1, device=toks.device)
    for s0 in range(0, n, chunk):
        lg = eng.logits(emb[s0:s0 + chunk], toks[s0:s0 + chunk, :t - 1])
        out[s0:s0 + chunk] = torch.log_softmax(lg, dim=-1).gather(-1, toks[s0:s0 + chunk, 1:, None]).squeeze(-1)
        del lg
    mask = torch.arange(t - 1, device=toks.device)[None, :] < (torch.as_tensor(lens, device=toks.device)[:, None] - 1)
    return out * mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--old-reps", type=int, default=1)
    args = ap.parse_args()
    import synth
    from sonar_amd.text_decoder import TextDecoderEngine, get_text_decoder_config

    cfg = get_text_decoder_config("basic")
    d, f, V = cfg.model_dim, cfg.ffn_inner_dim, cfg.vocab_info.size
    per_row = cfg.num_decoder_layers * 2 * (4 * d * d + 2 * d * f) + 2 * d * V
    eng = TextDecoderEngine(cfg, synth.text_decoder_state_dict("cuda:0"), device="cuda:0", dtype=torch.float16)
    g = torch.Generator().manual_seed(0)
    out = {"metric": "score_tokens_per_s", "config": "basic synthetic fp16, 24 x 1024, vocab 256206",
           "gflop_per_scored_row": round(per_row / 1e9, 3)}
    cases = {"uniform_256x64": torch.full((256,), 64, dtype=torch.int32),
             "ragged_256x8_128": torch.randint(8, 129, (256,), generator=g, dtype=torch.int32)}
    for name, lens in cases.items():
        t = int(lens.max())
        toks = torch.randint(4, V, (256, t), generator=g)
        toks[:, 0] = 3
        toks = toks.cuda()
        emb = (torch.randn(256, d, generator=g) * 0.3).half().cuda()
        scored = int((lens - 1).sum())
        dt = timed(lambda: eng.score(emb, toks, lens), args.reps)
        fl = per_row * scored
        new = eng.score(emb, toks, lens)
        dt_old = timed(lambda: old_route(eng, emb, toks, lens), args.old_reps)
        ref = old_route(eng, emb, toks, lens)
        out[name] = {"ms": round(dt * 1e3, 3), "scored_tokens": scored, "tokens_per_s": round(scored / dt, 1),
                     "tflops": round(fl / dt / 1e12, 1), "fraction_of_peak": round(fl / dt / 1e12 / PEAK_TFLOPS, 4),
                     "old_route_ms": round(dt_old * 1e3, 3), "old_route_tokens_per_s": round(scored / dt_old, 1),
                     "speedup_vs_old_route": round(dt_old / dt, 2),
                     "max_abs_delta_vs_old_route": float((new - ref).abs().max())}
    out["value"] = out["uniform_256x64"]["tokens_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
