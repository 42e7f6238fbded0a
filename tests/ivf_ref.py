"""The IVF-Flat index restated in numpy: the contract sonar_amd.index / smi_ivf_* are tested against.

Build: row i goes to list labels[i]; a label outside [0, K) leaves it out.  Every list starts at a multiple of ALIGN slots
and is padded to one with zero rows of id -1.  Search: the candidates of a query are the rows of the lists its probe row
names (an entry outside [0, K) names none; a list named twice contributes twice); the result is the k best in the total
order (score descending, ties to the lower original row number), (-inf, -1) where fewer exist.  Scores are float64 here:
exact on integer-valued operands, and what the device's fp32 accumulation is bounded against otherwise.
"""
import numpy as np

ALIGN = 16  # SMI_IVF_LIST_ALIGN


def round_up(c, a=ALIGN):
    return (np.asarray(c, dtype=np.int64) + a - 1) // a * a


def slots_bound(n: int, k: int, a: int = ALIGN) -> int:
    """The most slots any labelling of n rows over k lists can need: min(n, k) lists take one row each (a whole block per
    row), the remaining rows fill whole blocks of one of them."""
    m = min(n, k)
    return m * a + (n - m) // a * a


def build(labels, k: int, a: int = ALIGN):
    """(offsets int64 [k + 1], sizes int64 [k], ids int64 [offsets[k]] with -1 in the pad slots); the rows of a list in
    ascending row number (the engine's order inside a list is unspecified)."""
    labels = np.asarray(labels).astype(np.int64)
    ok = (labels >= 0) & (labels < k)
    sizes = np.bincount(labels[ok], minlength=k).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(round_up(sizes, a))]).astype(np.int64)
    ids = np.full(int(offsets[k]), -1, dtype=np.int64)
    order = np.argsort(np.where(ok, labels, k), kind="stable")[: int(ok.sum())]
    fill = np.concatenate([offsets[c] + np.arange(sizes[c]) for c in range(k)]) if k else np.zeros(0, dtype=np.int64)
    ids[fill.astype(np.int64)] = order
    return offsets, sizes, ids


def build_loop(labels, k: int, a: int = ALIGN):
    """`build` as a plain loop over the rows."""
    lists = [[] for _ in range(k)]
    for i, c in enumerate(labels):
        if 0 <= int(c) < k:
            lists[int(c)].append(i)
    offsets, ids = [0], []
    for members in lists:
        pad = (-len(members)) % a
        ids += members + [-1] * pad
        offsets.append(len(ids))
    return np.array(offsets, dtype=np.int64), np.array([len(m) for m in lists], dtype=np.int64), np.array(ids, dtype=np.int64)


def scores64(q, x):
    """float64 dot products [nq, n], each one a sum over a fresh array of products: equal rows get equal scores."""
    q64, x64 = np.asarray(q, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return np.stack([(x64 * r).sum(axis=1) for r in q64], axis=0)


def topk_total_order(scores, ids, k: int):
    """The k best of the candidates (scores [m], ids [m]) by (score descending, id ascending): (scores [k], ids [k])."""
    out_s, out_i = np.full(k, -np.inf), np.full(k, -1, dtype=np.int64)
    if len(ids):
        order = np.lexsort((ids, -np.asarray(scores, dtype=np.float64)))[:k]  # last key first: score, then id
        out_s[: len(order)], out_i[: len(order)] = np.asarray(scores)[order], np.asarray(ids)[order]
    return out_s, out_i


def search(q, x, labels, k_lists: int, probes, k: int, s=None):
    """(scores float64 [nq, k], ids int64 [nq, k]).  x: the corpus rows [n, d] (row number = id), labels [n], probes
    [nq, nprobe]; s: precomputed scores64(q, x)."""
    labels = np.asarray(labels).astype(np.int64)
    probes = np.asarray(probes).astype(np.int64)
    s = scores64(q, x) if s is None else s
    members = [np.flatnonzero(labels == c) for c in range(k_lists)]
    out_s, out_i = np.empty((len(probes), k)), np.empty((len(probes), k), dtype=np.int64)
    for r, row in enumerate(probes):
        cand = [members[c] for c in row if 0 <= c < k_lists]
        cand = np.concatenate(cand) if cand else np.zeros(0, dtype=np.int64)
        out_s[r], out_i[r] = topk_total_order(s[r, cand], cand, k)
    return out_s, out_i


def brute_force(q, x, k: int, s=None):
    """The k best of ALL rows by a stable sort of the float64 scores, descending (stable = ties to the lower row)."""
    s = scores64(q, x) if s is None else s
    n = s.shape[1]
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    out_s = np.full((s.shape[0], k), -np.inf)
    out_i = np.full((s.shape[0], k), -1, dtype=np.int64)
    out_s[:, : min(k, n)] = np.take_along_axis(s, order, axis=1)
    out_i[:, : min(k, n)] = order
    return out_s, out_i


def integer_rows(rng, n: int, d: int):
    """fp16 rows with entries from {-1, 0, 1}, half of them zeroed at d = 1024 (tests/test_gpu_xsim_kernels.py): every
    partial sum is a small integer, so a score is exact in any summation order."""
    x = rng.integers(-1, 2, (n, d)).astype(np.float16)
    if d >= 1024:
        x *= rng.integers(0, 2, (n, d)).astype(np.float16)
    return x


def normalize64(c):
    c = np.asarray(c, dtype=np.float64)
    return c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-12)


def planted(n: int, k: int, d: int, nq: int, seed: int = 0, noise: float = 0.6, qnoise: float = 0.1):
    """Planted clusters (tests/kmeans_ref.planted: row i in cluster i % k) and nq queries, query j a noisy copy of corpus row
    target[j].  Returns (x fp16 [n, d], labels int32 [n], centres float64 [k, d], q fp16 [nq, d], target int64 [nq])."""
    rng = np.random.default_rng(seed)
    centres = normalize64(rng.standard_normal((k, d)))
    labels = (np.arange(n) % k).astype(np.int32)
    x = normalize64(centres[labels] + noise * rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float16)
    target = rng.permutation(n)[:nq] if nq <= n else rng.integers(0, n, nq)
    q = normalize64(x[target].astype(np.float64) + qnoise * rng.standard_normal((nq, d)) / np.sqrt(d)).astype(np.float16)
    return x, labels, centres, q, target.astype(np.int64)


# (n, K) crosses of the alignment rule and the slot bound
BOUND_CROSSES = [(n, k) for n in (1, ALIGN - 1, ALIGN, ALIGN + 1, 300, 4099) for k in (1, 3, 300, 5000)]
