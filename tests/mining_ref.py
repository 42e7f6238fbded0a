"""CPU restatement of LASER's bitext mining (facebookresearch/LASER source/mine_bitexts.py; LASER is not vendored and
cannot run here, the published algorithm is restated) as the engine states it in include/sonar_mi355.h: the loops are
written literally, in numpy, over explicit candidate lists.  Where the original leaves the result open it is fixed the way
the engine fixes it: candidates are walked by (score descending, candidate number ascending) -- numpy's stable argsort
over the negated scores, which also makes -0 and +0 equal -- and a candidate with a NaN score or an index outside its
side is excluded altogether.  `threshold` (None = none) is strict and applies to every retrieval.  Also here: a brute-force
statement of the same greedy matching, a simulation of the engine's parallel rounds that counts them, and the whole path
(k-NN both ways, margins, best candidates) in fp64.  Not collected by pytest."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

Pairs = List[Tuple[int, int, float]]


def candidates(fwd_best, fwd_score, bwd_best, bwd_score) -> List[Tuple[int, int, float]]:
    """Candidate c < nx: (c, fwd_best[c], fwd_score[c]); candidate c >= nx: (bwd_best[c - nx], c - nx, bwd_score[c - nx])."""
    out = [(i, int(j), float(s)) for i, (j, s) in enumerate(zip(fwd_best, fwd_score))]
    out += [(int(i), j, float(s)) for j, (i, s) in enumerate(zip(bwd_best, bwd_score))]
    return out


def excluded(cand, nx: int, ny: int) -> bool:
    s, t, v = cand
    return v != v or not 0 <= s < nx or not 0 <= t < ny


def _above(v: float, threshold: Optional[float]) -> bool:
    return threshold is None or v > threshold


def walk_order(cands, nx: int, ny: int) -> List[int]:
    """The candidate numbers of the non-excluded candidates, score descending, candidate number ascending."""
    live = [c for c, cand in enumerate(cands) if not excluded(cand, nx, ny)]
    scores = np.array([cands[c][2] for c in live], dtype=np.float32)
    return [live[i] for i in np.argsort(-scores, kind="stable")]


def max_accepted(cands, nx: int, ny: int) -> List[int]:
    """LASER's `max` loop: walk the sorted candidates, accept one iff its source and its target are both unseen.
    Returns the accepted candidate numbers in the order of the walk."""
    seen_src, seen_trg, out = set(), set(), []
    for c in walk_order(cands, nx, ny):
        src_ind, trg_ind, _ = cands[c]
        if src_ind not in seen_src and trg_ind not in seen_trg:
            seen_src.add(src_ind)
            seen_trg.add(trg_ind)
            out.append(c)
    return out


def max_accepted_bruteforce(cands, nx: int, ny: int) -> List[int]:
    """The same matching stated without a sort: again and again take the best remaining candidate (highest score, then
    lowest number) among those whose source and target are both free."""
    free = [c for c, cand in enumerate(cands) if not excluded(cand, nx, ny)]
    out = []
    while free:
        best = free[0]
        for c in free[1:]:
            if cands[c][2] > cands[best][2]:  # strict: an equal score keeps the lower number (-0 == +0 in this compare)
                best = c
        out.append(best)
        s, t, _ = cands[best]
        free = [c for c in free if cands[c][0] != s and cands[c][1] != t]
    return out


def parallel_rounds(cands, nx: int, ny: int) -> Tuple[List[int], int, List[int]]:
    """The engine's scheme: per round every live candidate bids (score, -number) for its source and its target; one that
    holds both maxima is accepted; one whose source or target is then taken dies.  Returns (accepted candidate numbers
    ascending, number of rounds, live candidates at the start of every round)."""
    live = [c for c, cand in enumerate(cands) if not excluded(cand, nx, ny)]
    key = {c: (np.float32(cands[c][2]) + np.float32(0), -c) for c in live}
    accepted, rounds, history = [], 0, []
    src_taken, trg_taken = set(), set()
    while live:
        rounds += 1
        history.append(len(live))
        src_best, trg_best = {}, {}
        for c in live:
            s, t, _ = cands[c]
            if s not in src_best or key[c] > key[src_best[s]]:
                src_best[s] = c
            if t not in trg_best or key[c] > key[trg_best[t]]:
                trg_best[t] = c
        won = [c for c in live if src_best[cands[c][0]] == c and trg_best[cands[c][1]] == c]
        for c in won:
            src_taken.add(cands[c][0])
            trg_taken.add(cands[c][1])
        accepted += won
        won = set(won)
        live = [c for c in live if c not in won and cands[c][0] not in src_taken and cands[c][1] not in trg_taken]
    return sorted(accepted), rounds, history


def mine(fwd_best, fwd_score, bwd_best, bwd_score, nx: int, ny: int, retrieval: str,
         threshold: Optional[float] = None) -> Pairs:
    """The (src, trg, score) pairs of one retrieval in CANDIDATE order (what smi_xsim_mine writes)."""
    cands = candidates(fwd_best, fwd_score, bwd_best, bwd_score)
    if retrieval == "fwd":
        keep = [c for c in range(nx) if not excluded(cands[c], nx, ny)]
    elif retrieval == "bwd":
        keep = [c for c in range(nx, nx + ny) if not excluded(cands[c], nx, ny)]
    elif retrieval == "intersect":
        keep = [c for c in range(nx) if not excluded(cands[c], nx, ny) and int(bwd_best[cands[c][1]]) == c]
    elif retrieval == "max":
        keep = sorted(max_accepted(cands, nx, ny))
    else:
        raise ValueError(retrieval)
    return [cands[c] for c in keep if _above(cands[c][2], threshold)]


def final_order(pairs: Pairs, retrieval: str) -> Pairs:
    """What mine_bitexts returns: `max` by score descending, equal scores in candidate order; the others as they are."""
    if retrieval != "max":
        return list(pairs)
    scores = np.array([p[2] for p in pairs], dtype=np.float32)
    return [pairs[i] for i in np.argsort(-scores, kind="stable")]


def contested_share(fwd_best, fwd_score, bwd_best, bwd_score, nx: int, ny: int) -> float:
    """Share of the accepted `max` pairs that had a competitor with an EQUAL score sharing their source or target (another
    pair, not the same pair listed from the other side): where the tie order decides."""
    cands = candidates(fwd_best, fwd_score, bwd_best, bwd_score)
    by_src, by_trg = {}, {}
    for c, cand in enumerate(cands):
        if not excluded(cand, nx, ny):
            by_src.setdefault(cand[0], []).append(c)
            by_trg.setdefault(cand[1], []).append(c)
    acc = max_accepted(cands, nx, ny)
    hit = 0
    for c in acc:
        s, t, v = cands[c]
        rivals = [o for o in by_src[s] + by_trg[t] if o != c and cands[o][:2] != (s, t)]
        hit += any(cands[o][2] == v for o in rivals)
    return hit / max(1, len(acc))


# ------------------------------------------------------------------------------------------ the whole path
def knn(a: np.ndarray, b: np.ndarray, k: int):
    """k best rows of b for every row of a by dot product: (scores [na, k], indices [na, k]), score descending, index
    ascending (the engine's total order)."""
    sim = a.astype(np.float64) @ b.astype(np.float64).T
    idx = np.argsort(-sim, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(sim, idx, axis=1), idx


def margin_fn(margin: str):
    return {"ratio": lambda a, b: a / b, "distance": lambda a, b: a - b, "cosine": lambda a, b: a, "absolute": lambda a, b: a}[margin]


def best_candidates(sim_k, idx_k, other_mean, margin: str):
    """LASER's score_candidates + argmax: per row, the candidate with the best margin score (first on ties)."""
    own_mean = sim_k.mean(axis=1)
    scores = margin_fn(margin)(sim_k, (own_mean[:, None] + other_mean[idx_k]) / 2)
    j = scores.argmax(axis=1)
    rows = np.arange(sim_k.shape[0])
    return idx_k[rows, j], scores[rows, j]


def pipeline(xn: np.ndarray, yn: np.ndarray, k: int, margin: str):
    """(fwd_best, fwd_score, bwd_best, bwd_score, x2y_mean, y2x_mean) over rows that are used as they are (normalise
    first for cosines), in fp64."""
    fs, fi = knn(xn, yn, min(k, yn.shape[0]))
    bs, bi = knn(yn, xn, min(k, xn.shape[0]))
    x_mean, y_mean = fs.mean(axis=1), bs.mean(axis=1)
    fwd_best, fwd_score = best_candidates(fs, fi, y_mean, margin)
    bwd_best, bwd_score = best_candidates(bs, bi, x_mean, margin)
    return fwd_best, fwd_score, bwd_best, bwd_score, x_mean, y_mean


def score_pairs(xn: np.ndarray, yn: np.ndarray, src, trg, x_mean, y_mean, margin: str) -> np.ndarray:
    """LASER's --mode score: margin(x_s . y_t, (mean_s + mean_t) / 2) in fp64 (the means are not read for "cosine")."""
    src, trg = np.asarray(src), np.asarray(trg)
    a = (xn[src].astype(np.float64) * yn[trg].astype(np.float64)).sum(axis=1)
    if margin in ("cosine", "absolute"):
        return a
    return margin_fn(margin)(a, (x_mean[src] + y_mean[trg]) / 2)
