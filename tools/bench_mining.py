"""Bitext mining (sonar_amd.mining) on one MI355X: one JSON line.

  262 144 x 262 144 x 1024 fp16 rows, k = 4, `ratio` margin, `max` retrieval: x is a noisy permutation of y, so every row
  has one planted partner.  Times the two top-k passes (x -> y, y -> x) and, separately, everything after them -- margin
  select in both directions, smi_xsim_mine (the rounds, with their host reads, and the compaction) and the final sort --
  and checks that every planted pair is mined.  The number of rounds is counted by the CPU restatement
  (tests/mining_ref.py) on the candidates the device produced.
    python tools/bench_mining.py [--n 262144] [--d 1024] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--noise", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from sonar_amd import mining, xsim
    from tests import mining_ref

    n, d, k = args.n, args.d, args.k
    g = torch.Generator(device="cuda").manual_seed(2)
    y = torch.nn.functional.normalize(torch.randn(n, d, generator=g, device="cuda"), dim=-1)
    perm = torch.randperm(n, generator=g, device="cuda")
    x = (y[perm] + args.noise * torch.randn(n, d, generator=g, device="cuda") / d ** 0.5).half()
    y = y.half()
    xn, yn = xsim.normalize_rows(x), xsim.normalize_rows(y)
    del x, y

    t_fwd, (fs, fi) = timed(lambda: xsim.topk_normalized(xn, n, yn, n, k), args.reps)
    t_bwd, (bs, bi) = timed(lambda: xsim.topk_normalized(yn, n, xn, n, k), args.reps)

    def after_topk():
        fwd_best, fwd_score = xsim.margin_select(fs, fi, bs, "ratio")
        bwd_best, bwd_score = xsim.margin_select(bs, bi, fs, "ratio")
        return (fwd_best, fwd_score, bwd_best, bwd_score), mining.mine_candidates(fwd_best, fwd_score, bwd_best, bwd_score,
                                                                                  n, n, "max")

    t_post, (cands, (src, trg, score)) = timed(after_topk, args.reps)
    t_mine, _ = timed(lambda: mining.mine_candidates(*cands, n, n, "max", sort=False), args.reps)

    found = torch.zeros(n, dtype=torch.bool, device="cuda")
    found[src] = trg == perm[src]
    mined_all = bool(found.all())
    _, rounds, live = mining_ref.parallel_rounds(mining_ref.candidates(*(t.cpu().numpy() for t in cands)), n, n)
    out = {"metric": "mining_post_topk_ms", "config": f"{n} x {n} x {d} fp16, k = {k}, ratio, max",
           "topk_fwd_ms": round(t_fwd * 1e3, 3), "topk_bwd_ms": round(t_bwd * 1e3, 3),
           "post_topk_ms": round(t_post * 1e3, 3), "mine_call_ms": round(t_mine * 1e3, 3),
           "post_topk_fraction_of_topk": round(t_post / (t_fwd + t_bwd), 5),
           "pairs": int(src.shape[0]), "planted_pairs_mined": int(found.sum()), "every_planted_pair_mined": mined_all,
           "sorted_descending": bool((score.diff() <= 0).all()), "rounds": rounds, "live_per_round": live,
           "value": round(t_post * 1e3, 3)}
    print(json.dumps(out))
    if not mined_all:
        sys.exit(1)


if __name__ == "__main__":
    main()
