"""Per-sentence prompts of the beam search (TextDecoderEngine.generate with one prompt per row) on one MI355X: one JSON
line, also written to profiles/decoder_prompts_bench.json.

  basic synthetic fp16 decoder (24 x 1024, vocab 256206), beam 5, 64 generated tokens (min_gen_len = the cap, so every call
  runs all its steps):
    fan_out     250 rows = 5 embeddings x 50 target languages as ONE call with per-sentence prompts, against 50 calls of 5
                rows with one language each through the one-prompt generate() -- the route a caller had before, timed in the
                same process.  (Token identity of the two is not checked: the row counts differ)
    all_equal   256 rows, 256 copies of one prompt through the per-sentence entry against the one-prompt generate(),
                alternating; generate() against itself gives the run-to-run spread "no slower" is read against.
    ragged      256 rows with prompts of 2..6 tokens (forced prefixes), ms per step.
    python tools/bench_prompts.py [--reps 5] [--steps 64]
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


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_prompts_bench.json"))
    args = ap.parse_args()
    import synth
    from sonar_amd.text_decoder import TextDecoderEngine, get_text_decoder_config

    cfg = get_text_decoder_config("basic")
    d, V = cfg.model_dim, cfg.vocab_info.size
    eng = TextDecoderEngine(cfg, synth.text_decoder_state_dict("cuda:0"), device="cuda:0", dtype=torch.float16)
    g = torch.Generator().manual_seed(0)
    steps = args.steps
    kw = dict(beam_size=5, min_gen_len=steps, max_gen_len=(0, steps))
    out = {"metric": "decoder_prompts_fan_out_speedup", "config": "basic synthetic fp16, 24 x 1024, vocab 256206, beam 5",
           "generated_tokens": steps, "reps": args.reps}

    # ---- 5 embeddings x 50 languages: one call of 250 rows against 50 calls of 5
    langs = [256001 + i for i in range(50)]
    emb5 = (torch.randn(5, d, generator=g) * 0.3).half().cuda()
    emb250 = emb5.repeat(50, 1)                                  # rows 5 k .. 5 k + 4: language k
    prompts250 = [[3, langs[r // 5]] for r in range(250)]

    def mixed():
        eng.generate(emb250, prompts250, **kw)

    def per_language():
        for lang in langs:
            eng.generate(emb5, [3, lang], **kw)

    mixed(), per_language()
    m_ms, p_ms = [], []
    for _ in range(args.reps):
        m_ms.append(once(mixed))
        p_ms.append(once(per_language))
    positions = steps + 2 - 1                                    # decoder steps of a call: prompt + generated tokens - 1
    m, p = stats(m_ms), stats(p_ms)
    out["fan_out"] = {"rows": 250, "mixed_call": m, "fifty_calls_of_5": p,
                      "mixed_ms_per_step": round(m["median_ms"] / positions, 3),
                      "fifty_calls_ms_per_step": round(p["median_ms"] / positions, 3),
                      "one_call_of_5_ms_per_step": round(p["median_ms"] / 50 / positions, 3),
                      "speedup": round(p["median_ms"] / m["median_ms"], 2)}

    # ---- 256 rows, all-equal prompts: the per-sentence entry against generate(), alternating
    emb256 = (torch.randn(256, d, generator=g) * 0.3).half().cuda()
    one = [3, 256047]
    same256 = [one] * 256

    def gen():
        eng.generate(emb256, one, **kw)

    def gen_rows():
        eng.generate(emb256, same256, **kw)

    gen(), gen_rows()
    a_ms, b_ms, c_ms = [], [], []
    for _ in range(args.reps):
        a_ms.append(once(gen))
        b_ms.append(once(gen_rows))
        c_ms.append(once(gen))
    a, b, c = stats(a_ms), stats(b_ms), stats(c_ms)
    base = stats(a_ms + c_ms)
    out["all_equal"] = {"rows": 256, "generate": base, "generate_first_of_each_round": a, "generate_last_of_each_round": c,
                        "per_sentence_entry": b,
                        "generate_ms_per_step": round(base["median_ms"] / positions, 3),
                        "per_sentence_entry_ms_per_step": round(b["median_ms"] / positions, 3),
                        "generate_spread_percent": round(100 * (base["max_ms"] - base["min_ms"]) / base["median_ms"], 2),
                        "entry_vs_generate_percent": round(100 * (b["median_ms"] / base["median_ms"] - 1), 2)}

    # ---- 256 rows, ragged prompts of 2..6 tokens, and the same lengths' worth of languages only (2 tokens, 50 languages)
    ragged = [[3, langs[r % 50]] + [int(t) for t in torch.randint(4, 256000, (r % 5,), generator=g)] for r in range(256)]
    lang256 = [[3, langs[r % 50]] for r in range(256)]

    def gen_ragged():
        eng.generate(emb256, ragged, **kw)

    def gen_langs():
        eng.generate(emb256, lang256, **kw)

    gen_ragged(), gen_langs()
    r_ms, l_ms = [], []
    for _ in range(args.reps):
        r_ms.append(once(gen_ragged))
        l_ms.append(once(gen_langs))
    r, l = stats(r_ms), stats(l_ms)
    out["ragged"] = {"rows": 256, "prompt_lens": "2..6", "call": r, "steps": steps + 6 - 1,
                     "ms_per_step": round(r["median_ms"] / (steps + 6 - 1), 3)}
    out["fifty_languages_256_rows"] = {"rows": 256, "call": l, "ms_per_step": round(l["median_ms"] / positions, 3)}
    out["value"] = out["fan_out"]["speedup"]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
