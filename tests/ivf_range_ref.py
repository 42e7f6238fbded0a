"""The range search over the IVF-Flat lists restated in numpy, on top of tests/ivf_ref.py: the contract
sonar_amd.index.range_search_lists / smi_range_search_* are tested against.

The candidates of a query are those of `ivf_ref.search`: the rows of the lists its probe row names (an entry outside [0, K)
names none; a list named twice contributes twice).  A candidate is a hit iff float32(score) >= float32(threshold of the
query): an fp32 compare, so a NaN threshold hits nothing and -inf everything probed.  The hits of query q are the entries
lims[q] .. lims[q + 1] of (scores, ids), ordered score descending and ties to the lower id.  Scores are float64 here, as in
ivf_ref: exact on integer-valued operands.
"""
import numpy as np

from tests import ivf_ref as R


def range_search(q, x, labels, k_lists: int, probes, thresholds, s=None):
    """(lims int64 [nq + 1], scores float64 [total], ids int64 [total]).  x: the corpus rows [n, d] (row number = id),
    labels [n], probes [nq, nprobe], thresholds [nq]; s: precomputed ivf_ref.scores64(q, x)."""
    labels = np.asarray(labels).astype(np.int64)
    probes = np.asarray(probes).astype(np.int64)
    thr = np.asarray(thresholds, dtype=np.float32)
    s = R.scores64(q, x) if s is None else s
    members = [np.flatnonzero(labels == c) for c in range(k_lists)]
    lims, out_s, out_i = [0], [], []
    for r, row in enumerate(probes):
        cand = [members[c] for c in row if 0 <= c < k_lists]
        cand = np.concatenate(cand) if cand else np.zeros(0, dtype=np.int64)
        sc = s[r, cand]
        with np.errstate(invalid="ignore"):
            hit = sc.astype(np.float32) >= thr[r]
        cand, sc = cand[hit], sc[hit]
        order = np.lexsort((cand, -sc))  # last key first: score, then id
        out_s.append(sc[order])
        out_i.append(cand[order])
        lims.append(lims[-1] + len(order))
    return (np.array(lims, dtype=np.int64), np.concatenate(out_s).astype(np.float64) if out_s else np.zeros(0),
            np.concatenate(out_i).astype(np.int64) if out_i else np.zeros(0, dtype=np.int64))


def range_search_loop(q, x, labels, k_lists: int, probes, thresholds):
    """`range_search` as plain loops over queries, probe slots and rows, with an insertion into the ordered segment."""
    q64, x64 = np.asarray(q, dtype=np.float64), np.asarray(x, dtype=np.float64)
    lims, out_s, out_i = [0], [], []
    for r in range(len(probes)):
        seg = []  # (score, id), best first
        t = np.float32(thresholds[r])
        for c in probes[r]:
            c = int(c)
            if not 0 <= c < k_lists:
                continue
            for i in range(len(x64)):
                if int(labels[i]) != c:
                    continue
                sc = float((x64[i] * q64[r]).sum())
                if not np.float32(sc) >= t:  # (NaN: never a hit)
                    continue
                at = 0
                while at < len(seg) and (seg[at][0] > sc or (seg[at][0] == sc and seg[at][1] <= i)):
                    at += 1
                seg.insert(at, (sc, i))
        out_s += [e[0] for e in seg]
        out_i += [e[1] for e in seg]
        lims.append(len(out_i))
    return np.array(lims, dtype=np.int64), np.array(out_s, dtype=np.float64), np.array(out_i, dtype=np.int64)
