"""Spherical k-means restated in numpy: the contract sonar_amd.clustering is tested against.

The update is exact integer arithmetic: every finite fp16 is an integer multiple of 2^-24, so a row sum is an int64 in units
of 2^-24 whatever the order.  Finalise is one round to nearest even (int64 -> float32) and an exact scale; normalisation and
scoring are float64 here, which is what the device's fp32 arithmetic is bounded against.
"""
import numpy as np

SCALE_BITS = 24


def fixed(x16: np.ndarray) -> np.ndarray:
    """fp16 array -> int64 array of x * 2^24; Inf / NaN -> 0."""
    assert x16.dtype == np.float16
    v = x16.astype(np.float64)
    v = np.where(np.isfinite(v), v, 0.0) * float(1 << SCALE_BITS)
    q = v.astype(np.int64)
    assert np.array_equal(q.astype(np.float64), v), "not an integer multiple of 2^-24"
    return q


def update(xn16: np.ndarray, labels: np.ndarray, k: int):
    """(sums int64 [k, d], counts int32 [k]); rows with a label outside [0, k) are skipped."""
    q = fixed(xn16)
    n, d = q.shape
    labels = np.asarray(labels).astype(np.int64)
    assert labels.shape == (n,)
    ok = (labels >= 0) & (labels < k)
    sums = np.zeros((k, d), dtype=np.int64)
    np.add.at(sums, labels[ok], q[ok])
    counts = np.bincount(labels[ok], minlength=k).astype(np.int32)
    return sums, counts


def live_clusters(sums: np.ndarray, counts: np.ndarray) -> np.ndarray:
    return (counts > 0) & (sums != 0).any(axis=1)


def finalize(sums: np.ndarray, counts: np.ndarray, prev32: np.ndarray):
    """(centroids float32 [k, d], number of clusters that kept their previous row)."""
    live = live_clusters(sums, counts)
    new = sums.astype(np.float32) * np.float32(2.0 ** -SCALE_BITS)  # astype: round to nearest even; the scale is exact
    out = np.where(live[:, None], new, prev32.astype(np.float32))
    return out, int((~live).sum())


def normalize64(c: np.ndarray) -> np.ndarray:
    c = c.astype(np.float64)
    return c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-12)


def assign(xn16: np.ndarray, cn: np.ndarray):
    """float64 cosines of the rows against unit centroids cn -> (labels, best score, top-1 minus top-2 margin); ties to
    the lower index."""
    x64, c64 = xn16.astype(np.float64), cn.astype(np.float64)
    # products then a row sum over a fresh array, per centroid: equal centroids get equal scores (a BLAS product's last
    # bit can depend on where a centroid sits in the block or in memory)
    s = np.stack([(x64 * c).sum(axis=1) for c in c64], axis=1)
    labels = s.argmax(axis=1)
    best = s[np.arange(s.shape[0]), labels]
    if s.shape[1] > 1:
        rest = s.copy()
        rest[np.arange(s.shape[0]), labels] = -np.inf
        margin = best - rest.max(axis=1)
    else:
        margin = np.full(s.shape[0], np.inf)
    return labels.astype(np.int32), best, margin


def fit(xn16: np.ndarray, init: np.ndarray, n_iter: int):
    """The round loop: assign, then n_iter x (update -> finalise -> assign).  Returns a list of n_iter + 1 records
    {labels, scores, margin, centroids (float32, the ones the labels were assigned against), empty}."""
    k = init.shape[0]
    c32 = init.astype(np.float32)
    rounds = []
    labels, best, margin = assign(xn16, normalize64(c32))
    rounds.append(dict(labels=labels, scores=best, margin=margin, centroids=c32, empty=None))
    for _ in range(n_iter):
        sums, counts = update(xn16, labels, k)
        c32, empty = finalize(sums, counts, c32)
        labels, best, margin = assign(xn16, normalize64(c32))
        rounds.append(dict(labels=labels, scores=best, margin=margin, centroids=c32, empty=empty))
    return rounds


def planted(n: int, k: int, d: int, seed: int = 0, noise: float = 0.6):
    """k unit Gaussian directions; row i belongs to cluster i % k and is normalise(centre + noise * g / sqrt(d)) in fp16.
    Returns (x fp16 [n, d], planted labels int32 [n], init fp16 [k, d] = the first member of each cluster)."""
    rng = np.random.default_rng(seed)
    centres = normalize64(rng.standard_normal((k, d)))
    labels = (np.arange(n) % k).astype(np.int32)
    x = normalize64(centres[labels] + noise * rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float16)
    assert n >= k
    return x, labels, x[:k].copy()


PLANTED_SHAPES = [(1000, 7, 1024), (4099, 16, 1024), (777, 300, 1024), (600, 5, 64)]
