"""Semantic de-duplication restated in numpy: the contract sonar_amd.dedup / smi_ivf_dedup are tested against.

Input: the corpus rows x [n, d] (row number = id) and the flat list storage of tests/ivf_ref.py (ids [slots] with -1 in the
pad slots, offsets [K + 1]); priority None (all equal) or [n] by original row number.  Row j PRECEDES row i iff both are in
the same list and (priority[j] > priority[i] or (priority[j] == priority[i] and j < i)).  Output, by original row number:
max_sim[i] = the best score of row i against the rows that precede it (-inf if none does, or if i is in no list) and
nearest[i] = that row's id (-1), "best" in the total order of the mining kernels: score descending, ties to the lower id.
Scores are float64 here (tests/ivf_ref.scores64): exact on integer-valued rows, and what the device's fp32 accumulation is
bounded against otherwise.  keep = ~(max_sim > threshold), strict.
"""
import numpy as np

from tests import ivf_ref as R


def members_of(ids, offsets):
    """The ids of every list, pad slots dropped, in slot order."""
    ids, offsets = np.asarray(ids).astype(np.int64), np.asarray(offsets).astype(np.int64)
    out = []
    for c in range(len(offsets) - 1):
        seg = ids[offsets[c]: offsets[c + 1]]
        out.append(seg[seg >= 0])
    return out


def precedes(pj, j, pi, i):
    return pj > pi or (pj == pi and j < i)


def self_join(x, ids, offsets, n: int, priority=None, s=None):
    """(max_sim float64 [n], nearest int64 [n]).  s: precomputed scores of all pairs [n, n] (R.scores64(x, x), or any exact
    product on integer-valued rows)."""
    p = np.zeros(n) if priority is None else np.asarray(priority, dtype=np.float64)
    max_sim, nearest = np.full(n, -np.inf), np.full(n, -1, dtype=np.int64)
    for m in members_of(ids, offsets):
        if len(m) < 2:
            continue
        sm = R.scores64(x[m], x[m]) if s is None else s[np.ix_(m, m)]
        pm = p[m]
        before = (pm[None, :] > pm[:, None]) | ((pm[None, :] == pm[:, None]) & (m[None, :] < m[:, None]))  # [own, candidate]
        masked = np.where(before, sm, -np.inf)
        best = masked.max(axis=1)
        # ties to the lower id: the lowest id among the preceding rows that reach the best score
        winner = np.where(before & (masked == best[:, None]), m[None, :], np.iinfo(np.int64).max).min(axis=1)
        have = before.any(axis=1)
        max_sim[m[have]], nearest[m[have]] = best[have], winner[have]
    return max_sim, nearest


def self_join_loop(x, ids, offsets, n: int, priority=None):
    """`self_join` as a plain double loop over all pairs of a list."""
    x64 = np.asarray(x, dtype=np.float64)
    p = [0.0] * n if priority is None else [float(v) for v in priority]
    max_sim, nearest = np.full(n, -np.inf), np.full(n, -1, dtype=np.int64)
    for m in members_of(ids, offsets):
        for i in m:
            for j in m:
                if not precedes(p[j], j, p[i], i):
                    continue
                s = float((x64[j] * x64[i]).sum())
                if nearest[i] < 0 or s > max_sim[i] or (s == max_sim[i] and j < nearest[i]):
                    max_sim[i], nearest[i] = s, j
    return max_sim, nearest


def semdedup_recipe(x, members, priority):
    """The literal SemDeDup step for ONE cluster with unique priorities: sort the cluster by priority (descending), take the
    similarity matrix, its strict upper triangle, the column max.  Returns (ids in sorted order, max_sim in that order)."""
    members = np.asarray(members)
    order = np.argsort(-np.asarray(priority, dtype=np.float64)[members], kind="stable")
    m = members[order]
    x64 = np.asarray(x, dtype=np.float64)[m]
    sim = np.stack([(x64 * r).sum(axis=1) for r in x64], axis=0)
    tri = np.where(np.triu(np.ones_like(sim, dtype=bool), k=1), sim, -np.inf)  # [earlier, later]
    return m, tri.max(axis=0)


def keep_mask(max_sim, threshold: float):
    return ~(np.asarray(max_sim) > threshold)


def planted_groups(n_groups: int, group_size: int, k: int, d: int, seed: int = 0, noise: float = 0.1):
    """Planted near-duplicate groups: every group is a random unit base row plus group_size - 1 members base + noise * (a
    random unit row), all normalised and rounded to fp16; the rows are shuffled; the label of a row is its group % k, so a
    group lies in one list.  Returns (x fp16 [n, d], labels int32 [n], group int64 [n])."""
    rng = np.random.default_rng(seed)
    base = R.normalize64(rng.standard_normal((n_groups, d)))
    rows = [base[:, None, :]]
    if group_size > 1:
        dirs = R.normalize64(rng.standard_normal((n_groups * (group_size - 1), d))).reshape(n_groups, group_size - 1, d)
        rows.append(base[:, None, :] + noise * dirs)
    x = np.concatenate(rows, axis=1).reshape(n_groups * group_size, d)
    group = np.repeat(np.arange(n_groups), group_size)
    perm = rng.permutation(len(x))
    x, group = R.normalize64(x[perm]).astype(np.float16), group[perm]
    return x, (group % k).astype(np.int32), group.astype(np.int64)


def refusal_cases(lib):
    """{name: return code} of calls smi_ivf_dedup must refuse on its arguments alone (no pointer is dereferenced)."""
    p, big = 0x1000, 1 << 40
    f = lib.smi_ivf_dedup
    need = lib.smi_ivf_dedup_workspace_bytes(160, 100, 7, 64)
    return {
        "null rows": f(None, p, p, 7, 160, 64, p, 100, p, p, p, big, None),
        "null ids": f(p, None, p, 7, 160, 64, p, 100, p, p, p, big, None),
        "null offsets": f(p, p, None, 7, 160, 64, p, 100, p, p, p, big, None),
        "null max_sim": f(p, p, p, 7, 160, 64, p, 100, None, p, p, big, None),
        "null nearest": f(p, p, p, 7, 160, 64, None, 100, p, None, p, big, None),
        "null ws": f(p, p, p, 7, 160, 64, None, 100, p, p, None, big, None),
        "d": f(p, p, p, 7, 160, 96, p, 100, p, p, p, big, None),
        "d 0": f(p, p, p, 7, 160, 0, p, 100, p, p, p, big, None),
        "n": f(p, p, p, 7, 160, 64, p, 0, p, p, p, big, None),
        "K": f(p, p, p, 0, 160, 64, p, 100, p, p, p, big, None),
        "slots": f(p, p, p, 7, 0, 64, p, 100, p, p, p, big, None),
        "big n": f(p, p, p, 7, 160, 64, p, 1 << 31, p, p, p, big, None),
        "big K": f(p, p, p, 1 << 31, 160, 64, p, 100, p, p, p, big, None),
        "big slots": f(p, p, p, 7, 1 << 31, 64, p, 100, p, p, p, big, None),
        "slots % 16": f(p, p, p, 7, 150, 64, p, 100, p, p, p, big, None),
        "short ws": f(p, p, p, 7, 160, 64, p, 100, p, p, p, need - 1, None),
        "misaligned ws": f(p, p, p, 7, 160, 64, p, 100, p, p, p + 8, big, None),
    }
