"""The paged top-k restated in numpy: the contract smi_xsim_topk_page / smi_ivf_search_page and the wide calls
of sonar_amd.xsim / .index are tested against.

A candidate is (score, id).  The total order is score descending, ties to the lower id.  A PAGE returns, for a row, the k <= 16
best candidates strictly AFTER the row's exclusive ceiling (cs, ci): s < cs, or s == cs and i > ci.  No ceiling: the best k.  A
ceiling whose id is negative: the row is exhausted, only fill.  Fill is (-inf, -1).  A ceiling need not be a candidate.  The last
entry of a page is the ceiling of the next; the pages concatenated are the first k of the full sort.
"""
import numpy as np

PAGE = 16
WIDE_MAX = 64


def page_sizes(k: int):
    """16, 16, ..., and what is left."""
    return [min(PAGE, k - done) for done in range(0, k, PAGE)]


def after(scores, ids, ceiling):
    """Boolean [m]: which candidates come strictly after the ceiling (None: all; id < 0: none)."""
    scores, ids = np.asarray(scores, dtype=np.float64), np.asarray(ids, dtype=np.int64)
    if ceiling is None:
        return np.ones(len(ids), dtype=bool)
    cs, ci = float(ceiling[0]), int(ceiling[1])
    if ci < 0:
        return np.zeros(len(ids), dtype=bool)
    return (scores < cs) | ((scores == cs) & (ids > ci))


def page(scores, ids, k: int, ceiling=None):
    """One row: (scores float64 [k], ids int64 [k]) of the k best candidates after the ceiling, by a stable sort on
    (-score, id)."""
    scores, ids = np.asarray(scores, dtype=np.float64), np.asarray(ids, dtype=np.int64)
    keep = after(scores, ids, ceiling)
    s, i = scores[keep], ids[keep]
    order = np.lexsort((i, -s))[:k]  # last key first: score descending, then id ascending; lexsort is stable
    out_s, out_i = np.full(k, -np.inf), np.full(k, -1, dtype=np.int64)
    out_s[: len(order)], out_i[: len(order)] = s[order], i[order]
    return out_s, out_i


def page_loop(scores, ids, k: int, ceiling=None):
    """`page` as a plain double loop: k times, the best candidate not yet taken that comes after the ceiling."""
    out_s, out_i, taken = [], [], set()
    for _ in range(k):
        best = None
        for m in range(len(ids)):
            s, i = float(scores[m]), int(ids[m])
            if m in taken:
                continue
            if ceiling is not None:
                cs, ci = float(ceiling[0]), int(ceiling[1])
                if ci < 0 or not (s < cs or (s == cs and i > ci)):
                    continue
            if best is None or s > float(scores[best]) or (s == float(scores[best]) and i < int(ids[best])):
                best = m
        if best is None:
            out_s.append(-np.inf)
            out_i.append(-1)
        else:
            taken.add(best)
            out_s.append(float(scores[best]))
            out_i.append(int(ids[best]))
    return np.array(out_s), np.array(out_i, dtype=np.int64)


def wide(scores, ids, k: int):
    """One row, the way the wide calls compute it: the pages of page_sizes(k), each under the last entry of the one before."""
    out_s, out_i, ceiling = [], [], None
    for kp in page_sizes(k):
        s, i = page(scores, ids, kp, ceiling)
        out_s.append(s)
        out_i.append(i)
        ceiling = (s[-1], i[-1])
    return np.concatenate(out_s), np.concatenate(out_i)


def full_sort(scores, ids, k: int):
    """One row: the first k of the full stable sort, (-inf, -1) behind the candidates."""
    return page(scores, ids, k, None)


def brute_force(s, k: int, offset: int = 0, ceilings=None):
    """All rows of a score matrix s [nx, ny] (ids = column numbers + offset): (scores float64 [nx, k], ids int64 [nx, k]) of
    one page; ceilings: None or (scores [nx], ids [nx])."""
    s = np.asarray(s, dtype=np.float64)
    ids = np.arange(s.shape[1], dtype=np.int64) + offset
    out_s, out_i = np.empty((s.shape[0], k)), np.empty((s.shape[0], k), dtype=np.int64)
    for r in range(s.shape[0]):
        out_s[r], out_i[r] = page(s[r], ids, k, None if ceilings is None else (ceilings[0][r], ceilings[1][r]))
    return out_s, out_i


def first_k(s, k: int, offset: int = 0):
    """The first k columns of the stable descending sort of every row of s [nx, ny], vectorised: what a wide call must return
    (equal to chaining `brute_force` pages: tests/test_topk_wide_cpu.py)."""
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[1]
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    out_s = np.full((s.shape[0], k), -np.inf)
    out_i = np.full((s.shape[0], k), -1, dtype=np.int64)
    out_s[:, : min(k, n)] = np.take_along_axis(s, order, axis=1)
    out_i[:, : min(k, n)] = order + offset
    return out_s, out_i


def search(s, labels, n_lists: int, probes, k: int, ceilings=None, visible=None):
    """A page of the index search.  s: scores float64 [nq, n] of the queries against the corpus (row number = id); labels [n];
    probes [nq, nprobe] (an entry outside [0, n_lists) names no list); ceilings: None or (scores [nq], ids [nq]), one per
    QUERY over all its lists; visible: None or bool [n], the row mask."""
    labels = np.asarray(labels).astype(np.int64)
    probes = np.asarray(probes).astype(np.int64)
    members = [np.flatnonzero((labels == c) & (True if visible is None else np.asarray(visible))) for c in range(n_lists)]
    out_s, out_i = np.empty((len(probes), k)), np.empty((len(probes), k), dtype=np.int64)
    for r, row in enumerate(probes):
        cand = [members[c] for c in row if 0 <= c < n_lists]
        cand = np.concatenate(cand) if cand else np.zeros(0, dtype=np.int64)
        out_s[r], out_i[r] = page(s[r, cand], cand, k, None if ceilings is None else (ceilings[0][r], ceilings[1][r]))
    return out_s, out_i


def search_wide(s, labels, n_lists: int, probes, k: int, visible=None):
    """The pages of `search` chained, as IVFFlatIndex.search_wide does."""
    out_s, out_i, ceilings = [], [], None
    for kp in page_sizes(k):
        ps, pi = search(s, labels, n_lists, probes, kp, ceilings, visible)
        out_s.append(ps)
        out_i.append(pi)
        ceilings = (ps[:, -1], pi[:, -1])
    return np.concatenate(out_s, axis=1), np.concatenate(out_i, axis=1)
