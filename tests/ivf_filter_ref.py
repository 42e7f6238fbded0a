"""Filtered search over the IVF lists restated in numpy, on top of the restatements of the unfiltered
entries: the contract `search(..., rows=, query_keys=, match=)`, `range_search` and smi_*_keyed are tested against.

A candidate (query q, row i) counts iff the row is visible (mask[i]; rows beyond the end of mask or of row_keys are not) and
the pair passes the key predicate: bit cmp + 1 of `accept` is set, cmp = the sign of (row_keys[i] - query_keys[q]) as signed
integers -- bit 0 less, bit 1 equal, bit 2 greater.  THE RULE: a query's filtered result is the unfiltered result over an
index that holds only the rows this query may see.  So, for every distinct query key, the labels of the rows that do not
count are set to -1 (a label outside [0, K) leaves a row out of every list; labels are membership only in every
restatement) and the EXISTING restatement answers the queries with that key.
"""
import numpy as np

ACCEPT = {"==": 2, "!=": 5, "<": 1, "<=": 3, ">": 4, ">=": 6}


def passes(row_keys, query_key, accept: int):
    """bool [n]: the key predicate of every row against one query key."""
    rk = np.asarray(row_keys).astype(np.int64)
    cmp = np.sign(rk - int(query_key)).astype(np.int64)
    return ((int(accept) >> (cmp + 1)) & 1).astype(bool)


def allowed(n: int, row_keys, mask, query_key, accept):
    """bool [n]: the rows that count for a query with this key.  row_keys / mask may be None (no predicate / all visible) or
    shorter than n (the uncovered rows do not count); query_key None: the mask alone."""
    ok = np.ones(n, dtype=bool)
    if mask is not None:
        m = np.asarray(mask).astype(bool)
        ok[: len(m)] &= m[:n]
        ok[len(m):] = False
    if row_keys is not None:
        ok[len(row_keys):] = False
        if query_key is not None:
            r = min(n, len(row_keys))
            ok[:r] &= passes(np.asarray(row_keys)[:r], query_key, accept)
    return ok


def masked_labels(labels, ok):
    return np.where(ok, np.asarray(labels).astype(np.int64), -1)


def groups(query_keys, nq: int):
    """[(key or None, the queries with it)]: one group per distinct query key; without keys, all queries."""
    if query_keys is None:
        return [(None, np.arange(nq))]
    qk = np.asarray(query_keys).astype(np.int64)
    return [(int(key), np.flatnonzero(qk == key)) for key in np.unique(qk)]


def search(base, nq: int, n: int, labels, row_keys, mask, query_keys, accept, call):
    """(scores [nq, k], ids [nq, k]).  call(sel, labels_for_them) = the existing restatement's `search` on the queries sel
    (an index array) with the labels given; `base` is unused documentation of which one (a module)."""
    out_s = out_i = None
    for key, sel in groups(query_keys, nq):
        s, i = call(sel, masked_labels(labels, allowed(n, row_keys, mask, key, accept)))
        if out_s is None:
            out_s, out_i = np.empty((nq, s.shape[1]), dtype=s.dtype), np.empty((nq, i.shape[1]), dtype=i.dtype)
        out_s[sel], out_i[sel] = s, i
    return out_s, out_i


def flat_search(q, x, labels, k_lists: int, probes, k: int, row_keys=None, mask=None, query_keys=None, accept: int = 7, s=None):
    """`ivf_ref.search` under the rule.  s: precomputed scores [nq, n] (float64)."""
    from tests import ivf_ref as R

    q, probes = np.asarray(q), np.asarray(probes)
    s = R.scores64(q, x) if s is None else s
    return search(R, len(probes), len(x), labels, row_keys, mask, query_keys, accept,
                  lambda sel, lab: R.search(q[sel], x, lab, k_lists, probes[sel], k, s=s[sel]))


def range_search(q, x, labels, k_lists: int, probes, thresholds, row_keys=None, mask=None, query_keys=None, accept: int = 7,
                 s=None):
    """`ivf_range_ref.range_search` under the rule: (lims int64 [nq + 1], scores, ids)."""
    from tests import ivf_range_ref as G
    from tests import ivf_ref as R

    q, probes, thr = np.asarray(q), np.asarray(probes), np.asarray(thresholds, dtype=np.float32)
    nq = len(probes)
    s = R.scores64(q, x) if s is None else s
    seg_s, seg_i = [None] * nq, [None] * nq
    for key, sel in groups(query_keys, nq):
        lab = masked_labels(labels, allowed(len(x), row_keys, mask, key, accept))
        lims, sc, ids = G.range_search(q[sel], x, lab, k_lists, probes[sel], thr[sel], s=s[sel])
        for j, r in enumerate(sel):
            seg_s[r], seg_i[r] = sc[lims[j]: lims[j + 1]], ids[lims[j]: lims[j + 1]]
    lims = np.concatenate([[0], np.cumsum([len(a) for a in seg_i])]).astype(np.int64)
    return lims, np.concatenate(seg_s).astype(np.float64), np.concatenate(seg_i).astype(np.int64)


def flat_search_loop(q, x, labels, k_lists: int, probes, k: int, row_keys=None, mask=None, query_keys=None, accept: int = 7):
    """`flat_search` as a plain double loop over (query, row): what the restatement is checked against."""
    q64, x64 = np.asarray(q, dtype=np.float64), np.asarray(x, dtype=np.float64)
    out_s, out_i = np.full((len(probes), k), -np.inf), np.full((len(probes), k), -1, dtype=np.int64)
    for r in range(len(probes)):
        best = []  # (score, id), best first
        for c in probes[r]:
            c = int(c)
            if not 0 <= c < k_lists:
                continue
            for i in range(len(x64)):
                if int(labels[i]) != c:
                    continue
                if mask is not None and (i >= len(mask) or not mask[i]):
                    continue
                if row_keys is not None:
                    if i >= len(row_keys):
                        continue
                    if query_keys is not None:
                        rk, qk = int(row_keys[i]), int(query_keys[r])
                        bit = 0 if rk < qk else 1 if rk == qk else 2
                        if not accept >> bit & 1:
                            continue
                sc = float((x64[i] * q64[r]).sum())
                at = 0
                while at < len(best) and (best[at][0] > sc or (best[at][0] == sc and best[at][1] <= i)):
                    at += 1
                best.insert(at, (sc, i))
        for j, (sc, i) in enumerate(best[:k]):
            out_s[r, j], out_i[r, j] = sc, i
    return out_s, out_i
