"""Squared-Euclidean / inner-product search and Euclidean k-means restated in numpy: the contract that
smi_l2_prepare, smi_l2_topk, smi_l2_kmeans_* and sonar_amd.xsim.topk_l2 / clustering.KMeans are tested against.

A score is fl32(acc + bias[j]), acc the fp32 sum the fp16 mining tile produces for rows x_i and y_j.  That sum is restated
here as fl32 of the float64 dot product: exact, hence equal to the device's bits, whenever the dot product is a multiple of
some 2^-e below 2^(24 - e) (`int_rows`: small integers); on other rows it is what the device is BOUNDED against.

Half norms.  h[r] = fl32(S_r / 2), S_r the sum of the squares of the fp16 row, each square exact in float64, added in float64
in the order the header states, which depends on d alone: the row is d / 8 chunks of 8 consecutive columns; for l = 0 .. 63,
p[l] = the sum, from 0, of the squares of chunks l, l + 64, l + 128, ... in that order, the 8 columns of a chunk in ascending
order; then six steps off = 32, 16, 8, 4, 2, 1, each replacing every p[l] by p[l] + p[l ^ off] at once; S_r = p[0].

Top-k: stable sort of the float32 scores, descending (stable = ties to the lower row), (-inf, -1) where y has fewer than k
rows, y_index_offset added to the ids that exist.  Squared distances: clamp_min(2 (h_x - score), 0) in float32, fill +inf.

Euclidean k-means: the update is tests/kmeans_ref.update (exact int64 sums in units of 2^-24).  Finalise, for a cluster with
members: centroid_f32 = fl32(fl64(sum) * 2^-24 / fl64(count)) (int64 -> float64 by round to nearest even), the fp16 row its
round to nearest even, h_c the half norm of that fp16 row; a cluster without members keeps all three.  Assignment: the top-1
of the scores against bias -h_c.  The recorded objective is the float64 sum of the float32 scores in `objective_sum`'s order.
"""
import numpy as np

from tests import kmeans_ref as KR


def pad256(n: int) -> int:
    return (n + 255) // 256 * 256


# ---------------------------------------------------------------------------------------------------------- half norms
def half_norms(x16: np.ndarray) -> np.ndarray:
    """float32 [rows]: the half norms of fp16 rows (d a multiple of 8) in the header's order."""
    assert x16.dtype == np.float16 and x16.ndim == 2 and x16.shape[1] % 8 == 0
    rows, d = x16.shape
    sq = x16.astype(np.float64) ** 2  # exact: 22 significant bits
    nc = d // 8
    p = np.zeros((rows, 64), dtype=np.float64)
    for c0 in range(0, nc, 64):                       # chunks l, l + 64, ... of lane l, in that order
        lanes = min(64, nc - c0)
        for e in range(8):                            # the 8 columns of a chunk in ascending order
            p[:, :lanes] = p[:, :lanes] + sq[:, (c0 * 8 + e):(c0 + lanes) * 8:8]
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lane ^ off]
    return (0.5 * p[:, 0]).astype(np.float32)


def prepare(x):
    """What smi_l2_prepare writes for fp16 / fp32 rows: (fp16 [padded rows, d] with zero pad rows, float32 [padded rows])."""
    x16 = np.asarray(x).astype(np.float16)  # round to nearest even from float32
    out = np.zeros((pad256(len(x16)), x16.shape[1]), dtype=np.float16)
    out[: len(x16)] = x16
    h = np.zeros(len(out), dtype=np.float32)
    h[: len(x16)] = half_norms(x16)
    return out, h


# -------------------------------------------------------------------------------------------------------------- scores
def dots64(x16, y16) -> np.ndarray:
    """float64 [nx, ny] dot products, products then a row sum per y row (equal y rows get equal sums)."""
    x64, y64 = np.asarray(x16).astype(np.float64), np.asarray(y16).astype(np.float64)
    return np.stack([(x64 * y).sum(axis=1) for y in y64], axis=1) if len(y64) else np.zeros((len(x64), 0))


def scores(x16, y16, bias) -> np.ndarray:
    """float32 [nx, ny]: fl32(fl32(x . y) + bias[j]); bias: at least ny entries (the padded vector is fine)."""
    acc = dots64(x16, y16).astype(np.float32)
    b = np.asarray(bias, dtype=np.float32)[: len(y16)]
    return (acc + b[None, :]).astype(np.float32) + np.float32(0.0)  # a zero score is +0


def topk_of(s, k: int, y_index_offset: int = 0):
    """(scores float32 [nx, k], ids int64 [nx, k]) of a float32 score matrix: stable sort, descending."""
    s = np.asarray(s, dtype=np.float32)
    nx, ny = s.shape
    order = np.argsort(-s.astype(np.float64), axis=1, kind="stable")[:, :k]
    out_s = np.full((nx, k), -np.inf, dtype=np.float32)
    out_i = np.full((nx, k), -1, dtype=np.int64)
    out_s[:, : min(k, ny)] = np.take_along_axis(s, order, axis=1)
    out_i[:, : min(k, ny)] = order + y_index_offset
    return out_s, out_i


def topk(x16, y16, bias, k: int, y_index_offset: int = 0, s=None):
    return topk_of(scores(x16, y16, bias) if s is None else s, k, y_index_offset)


def topk_loop(x16, y16, bias, k: int, y_index_offset: int = 0):
    """`topk` as a plain float64 double loop and Python's stable sort (for rows whose scores are exact in float32)."""
    x16, y16 = np.asarray(x16), np.asarray(y16)
    out_s = np.full((len(x16), k), -np.inf, dtype=np.float32)
    out_i = np.full((len(x16), k), -1, dtype=np.int64)
    for m in range(len(x16)):
        cand = []
        for n in range(len(y16)):
            acc = 0.0
            for a, b in zip(x16[m].tolist(), y16[n].tolist()):
                acc += a * b
            cand.append((acc + float(bias[n]), n))
        cand.sort(key=lambda t: -t[0])  # stable
        for j, (v, n) in enumerate(cand[:k]):
            out_s[m, j], out_i[m, j] = v + 0.0, n + y_index_offset
    return out_s, out_i


def sq_dist(hx, score) -> np.ndarray:
    """float32: clamp_min(2 (h_x[:, None] - score), 0); a fill score of -inf gives +inf."""
    hx = np.asarray(hx, dtype=np.float32)[: len(score), None]
    with np.errstate(invalid="ignore"):
        return np.maximum((np.float32(2.0) * (hx - np.asarray(score, dtype=np.float32))).astype(np.float32), np.float32(0.0))


def topk_l2(x16, y16, k: int, y_index_offset: int = 0):
    """(sq_dist float32 [nx, k] ascending, ids int64, raw scores) between fp16 rows."""
    hx, hy = half_norms(np.asarray(x16)), half_norms(np.asarray(y16))
    s, i = topk(x16, y16, -hy, k, y_index_offset)
    return sq_dist(hx, s), i, s


def score_bound(x16, y16, s64, h):
    """The bound of a real-valued score against float64: d 2^-23 sum_c |x_c| |y_c| for the fp32 accumulation in any order,
    2^-24 (|s| + h) for the last add and the rounding of the half norm."""
    ax, ay = np.abs(np.asarray(x16).astype(np.float64)), np.abs(np.asarray(y16).astype(np.float64))
    d = ax.shape[1]
    return d * 2.0 ** -23 * (ax @ ay.T) + 2.0 ** -24 * (np.abs(s64) + np.asarray(h, dtype=np.float64)[None, : len(ay)])


# ---------------------------------------------------------------------------------------------------------------- data
def int_rows(rng, n: int, d: int) -> np.ndarray:
    """x side of the exact cases: entries uniform in {-3 .. 3}."""
    return rng.integers(-3, 4, (n, d)).astype(np.float16)


def sparse_int_rows(rng, n: int, d: int) -> np.ndarray:
    """y side: entries uniform in {-3 .. 3}, each kept with a per-row probability drawn uniformly from 0.2 .. 1.0 -- rows of
    very different lengths, so that the nearest row, the row of the largest inner product and the row of the largest cosine
    differ."""
    keep = rng.random((n, d)) < rng.uniform(0.2, 1.0, (n, 1))
    return (rng.integers(-3, 4, (n, d)) * keep).astype(np.float16)


EXACT_SHAPES = [(300, 513, 64), (257, 256, 128), (513, 2305, 64), (300, 2305, 1024)]


def data_conditions(x16, y16):
    """What the GPU tests rely on, measured on the restatement: (share of rows whose L2 top-1 differs from the inner-product
    top-1, ... from the cosine top-1, share of rows whose 8 best hold a tie between two adjacent positions k | k + 1 -- a
    decision only the tie-break makes --, that share for every k = 1 .. 7 apart, all scores and half norms multiples of 1/2
    below 2^24 and equal to their float64 values)."""
    hy = half_norms(y16)
    dots = dots64(x16, y16)
    s = scores(x16, y16, -hy)
    l2 = topk_of(s, 8)
    ip = np.argsort(-dots, axis=1, kind="stable")[:, 0]
    norm = np.sqrt(2.0 * hy.astype(np.float64))
    cos = np.argsort(-(dots / np.maximum(norm, 1e-30)[None, :]), axis=1, kind="stable")[:, 0]
    tie = l2[0][:, :-1] == l2[0][:, 1:]
    exact = bool((np.abs(s) < 2 ** 24).all() and (s * 2 == np.round(s * 2)).all() and (hy * 2 == np.round(hy * 2)).all()
                 and np.array_equal(s.astype(np.float64), dots - hy.astype(np.float64)[None, :]))
    return (float((l2[1][:, 0] != ip).mean()), float((l2[1][:, 0] != cos).mean()), float(tie.any(axis=1).mean()),
            tie.mean(axis=0).tolist(), exact)


def planted(seed: int = 0, groups: int = 75, d: int = 64, k: int = 4):
    """Real-valued rows with a designed nearest set: y holds `groups` far-apart centres times k members at distances 0.1, 0.2,
    .. from their centre (scaled Gaussian directions), x one row per group next to the centre, both shuffled.  Returns (x fp16
    [groups, d], y fp16 [groups * k, d], truth int64 [groups, k]: the members of x's group, nearest first)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((groups, d))
    unit = rng.standard_normal((groups, k, d))
    unit /= np.linalg.norm(unit, axis=2, keepdims=True)
    y = centres[:, None, :] + unit * (0.1 * np.arange(1, k + 1))[None, :, None]
    perm = rng.permutation(groups * k)
    y16 = y.reshape(groups * k, d)[perm].astype(np.float16)
    where = np.argsort(perm).reshape(groups, k)  # row (g, m) of the unshuffled y sits at where[g, m]
    x16 = (centres + 0.01 * rng.standard_normal((groups, d))).astype(np.float16)
    order = rng.permutation(groups)
    return x16[order], y16, where[order]


def planted_gap(x16, y16, truth):
    """(the smallest float64 gap between consecutive scores among a row's k + 1 best, the largest bound of a score): the
    planted order is decided above the arithmetic when gap > 2 bound."""
    hy = half_norms(y16)
    s64 = dots64(x16, y16) - hy.astype(np.float64)[None, :]
    k = truth.shape[1]
    order = np.argsort(-s64, axis=1, kind="stable")[:, : k + 1]
    assert np.array_equal(order[:, :k], truth)
    top = np.take_along_axis(s64, order, axis=1)
    return float((top[:, :-1] - top[:, 1:]).min()), float(score_bound(x16, y16, s64, hy).max())


# ------------------------------------------------------------------------------------------------------------- k-means
def finalize(sums: np.ndarray, counts: np.ndarray, prev32: np.ndarray, prev16: np.ndarray, prev_h: np.ndarray):
    """(centroids float32 [K, d], fp16 [K, d], half norms float32 [K], number of clusters without members)."""
    has = counts > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        new32 = (sums.astype(np.float64) * 2.0 ** -24 / counts.astype(np.float64)[:, None]).astype(np.float32)
    c32 = np.where(has[:, None], new32, prev32.astype(np.float32))
    with np.errstate(over="ignore"):
        c16 = np.where(has[:, None], c32.astype(np.float16), prev16[: len(counts)])
    h = np.where(has, half_norms(np.ascontiguousarray(c16)), np.asarray(prev_h, dtype=np.float32)[: len(counts)])
    return c32, c16, h.astype(np.float32), int((~has).sum())


def assign(x16, c16, h):
    """(labels int32, scores float32) = the top-1 against bias -h, ties to the lower index."""
    s, i = topk(x16, c16, -np.asarray(h, dtype=np.float32), 1)
    return i[:, 0].astype(np.int32), s[:, 0]


def objective_sum(scores32: np.ndarray) -> float:
    """The float64 sum of the scores in the device's order (km_round_part_kernel / km_round_sum_kernel): 256 partitions of
    ceil(n / 256) consecutive rows; in a partition thread t of 256 adds rows lo + t, lo + t + 256, ... in that order from 0; the
    256 thread sums, and then the 256 partition sums, are joined by the tree w = 128, 64, .., 1: v[t] += v[t + w], t < w."""
    s = np.asarray(scores32, dtype=np.float32).astype(np.float64)
    n = len(s)
    per = (n + 255) // 256

    def tree(v):
        v = v.copy()
        w = 128
        while w:
            v[:w] = v[:w] + v[w:2 * w]
            w //= 2
        return v[0]

    parts = np.zeros(256)
    for b in range(256):
        seg = s[b * per:min(n, (b + 1) * per)]
        th = np.zeros(256)
        for j in range(0, len(seg), 256):
            piece = seg[j:j + 256]
            th[: len(piece)] = th[: len(piece)] + piece
        parts[b] = tree(th)
    return float(tree(parts))


def fit(x16, init, n_iter: int):
    """The round loop: prepare the initial centroids, assign, then n_iter x (update -> finalise -> assign).  Returns n_iter + 1
    records {labels, scores, c32, c16, h, sums, counts, objective, moved, empty}."""
    k = len(init)
    c32 = np.asarray(init).astype(np.float32)
    c16 = c32.astype(np.float16)
    h = half_norms(c16)
    labels = np.full(len(x16), -1, dtype=np.int32)
    rounds, sums, counts, empty = [], None, None, None
    for t in range(n_iter + 1):
        if t:
            sums, counts = KR.update(x16, labels, k)
            c32, c16, h, empty = finalize(sums, counts, c32, c16, h)
        new, sc = assign(x16, c16, h)
        rounds.append(dict(labels=new, scores=sc, c32=c32, c16=c16, h=h, sums=sums, counts=counts,
                           objective=objective_sum(sc), moved=int((new != labels).sum()), empty=empty))
        labels = new
    return rounds


def search(x16, y16, labels, probes, k: int, visible=None):
    """The L2 flat index restated: for query q the candidates are the rows y_j with labels[j] among probes[q] (an entry outside
    the lists names none) and visible[j]; (sq_dist float32 [nq, k] ascending, ids int64, raw scores), fill (+inf, -1, -inf)."""
    hx, hy = half_norms(np.asarray(x16)), half_norms(np.asarray(y16))
    s = scores(x16, y16, -hy)
    labels, probes = np.asarray(labels), np.asarray(probes)
    cand = (labels[None, None, :] == probes[:, :, None]).any(axis=1)
    if visible is not None:
        cand &= np.asarray(visible, dtype=bool)[None, :]
    sc, ids = topk_of(np.where(cand, s, -np.inf), k)
    ids = np.where(np.isneginf(sc), -1, ids)
    return sq_dist(hx, sc), ids, sc


def inertia(hx, objective: float, n: int) -> float:
    """sum_i ||x_i - c(i)||^2 = 2 (sum_i h_x[i] - objective), the half norms added in float64."""
    return 2.0 * (float(np.asarray(hx[:n], dtype=np.float64).sum()) - objective)


def ray_clusters(seed: int = 0, n: int = 400, d: int = 64):
    """Two clusters on ONE ray, at distances 1 and 3 from the origin, with isotropic noise of norm ~0.24: (x fp16 [n, d],
    planted labels int32 [n] = i % 2, init fp16 [2, d] = the first member of each).  The clusters differ in length, not in
    direction."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(d)
    u /= np.linalg.norm(u)
    truth = (np.arange(n) % 2).astype(np.int32)
    x = np.where(truth == 0, 1.0, 3.0)[:, None] * u[None, :] + 0.03 * rng.standard_normal((n, d))
    x16 = x.astype(np.float16)
    return x16, truth, x16[:2].copy()
