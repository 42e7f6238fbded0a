"""L2 search over the product-quantised lists, plain and residual, restated in numpy: the contract
sonar_amd.index.IVFPQL2Index / IVFPQResidualL2Index, pq_l2_bias, search_lists_pq_l2 and smi_l2_pq_* are tested against.  The
product quantiser is tests/ivf_pq_ref.py's, the residual tests/ivf_pq_residual_ref.py's, the half norm, the fp32 score of two
rows, the distance and the data tests/l2_ref.py's, the total order tests/ivf_ref.py's: called, not restated.  New are the bias
of a slot and the two score expressions.

The row a slot stands for.  Plain: y^ = decode(codes).  Residual: y^ = c + r^, c the fp16 centroid of the row's list, r^ =
decode(codes of the residual).  The nearest row has the largest q . y^ - 1/2 ||y^||^2, and

    q . y^ - 1/2 ||y^||^2 = (q . c - 1/2 ||c||^2) + q . r^ - (c . r^ + 1/2 ||r^||^2).

Bias (`ordered_sum`: the float64 sum of exact products in the half norm's order, which depends on d alone -- the row is d / 8
chunks of 8 consecutive columns; p[l], l = 0 .. 63, is the sum from 0 of the terms of chunks l, l + 64, ... in that order, a
chunk's 8 columns ascending; then six steps off = 32, 16, 8, 4, 2, 1, each replacing every p[l] by p[l] + p[l ^ off]; p[0]):
    plain     bias = -fl32(0.5 * ordered_sum(y^ y^))                      = -l2_ref.half_norms(y^)
    residual  bias = -fl32(S1 + S2),  S1 = ordered_sum(c r^),  S2 = 0.5 * ordered_sum(r^ r^), one float64 add, one rounding;
              a label outside [0, K) names no centroid: c = 0.
Score, acc = fl32 of the dot product of the query and the decoded codes (l2_ref.scores' sum: exact on integer operands):
    plain     score = fl32(acc + bias)
    residual  score = fl32(fl32(acc + bias) + coarse),  coarse = fl32(fl32(q . c) - h_c): the L2 probe's own score (`coarse`)
    a zero score is +0.
Search: the candidates of query q are the rows whose label is among probes[q] (an entry outside [0, K) names none; its coarse
entry is not read) and that are visible; the k best by (score descending, id ascending), fill (-inf, -1); the distance is
l2_ref.sq_dist(h_q, score), fill +inf.

The bound of a real-valued residual score against float64 (`residual_score_bound`), derived as l2_ref.score_bound is.  The
float64 value is s = q . (c + r^) - 1/2 ||c + r^||^2 on the fp16 operands.  The device's value differs from it by
    d 2^-23 sum |q_j| |r^_j|         the fp32 accumulation of q . r^, in any order;
    2^-24 |S1 + S2|                  the one rounding of the bias (its float64 sums are exact to 2^-50 of that);
    2^-24 |q . r^ - (S1 + S2)|       the add of the bias;
    d 2^-23 sum |q_j| |c_j| + 2^-24 (|q . c - h_c| + h_c)     the coarse term, l2_ref.score_bound of the probe;
    2^-24 |s|                        the add of the coarse term;
each rounding taken at the exact value of what it rounds; the computed values differ from those by the errors above, which
enlarges every 2^-24 term by at most 2^-22 of the bound itself: the sum is multiplied by 1 + 2^-20.
"""
import numpy as np

from tests import ivf_pq_ref as P
from tests import ivf_pq_residual_ref as PR
from tests import ivf_ref as R
from tests import l2_ref as L


# ---------------------------------------------------------------------------------------------------------------- bias
def ordered_sum(terms64: np.ndarray) -> np.ndarray:
    """float64 [rows]: the sum of every row of terms64 (float64 [rows, d], d a multiple of 8) in the half norm's order."""
    t = np.asarray(terms64, dtype=np.float64)
    rows, d = t.shape
    assert d % 8 == 0
    nc = d // 8
    p = np.zeros((rows, 64), dtype=np.float64)
    for c0 in range(0, nc, 64):
        lanes = min(64, nc - c0)
        for e in range(8):
            p[:, :lanes] = p[:, :lanes] + t[:, (c0 * 8 + e):(c0 + lanes) * 8:8]
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lane ^ off]
    return p[:, 0]


def bias_plain(codes, cb16) -> np.ndarray:
    """float32 [n]: -fl32(1/2 ||y^||^2)."""
    y = P.decode(codes, cb16).astype(np.float64)
    return -((0.5 * ordered_sum(y * y)).astype(np.float32))


def list_centroids(labels, c16) -> np.ndarray:
    """fp16 [n, d]: the centroid row of every label, zeros for a label outside [0, K)."""
    c16 = np.asarray(c16, dtype=np.float16)
    labels = np.asarray(labels).astype(np.int64)
    ok = (labels >= 0) & (labels < len(c16))
    out = np.zeros((len(labels), c16.shape[1]), dtype=np.float16)
    out[ok] = c16[labels[ok]]
    return out


def bias_residual(codes, cb16, labels, c16) -> np.ndarray:
    """float32 [n]: -fl32(S1 + S2)."""
    r = P.decode(codes, cb16).astype(np.float64)
    c = list_centroids(labels, c16).astype(np.float64)
    return -((ordered_sum(c * r) + 0.5 * ordered_sum(r * r)).astype(np.float32))


def slot_bias(bias, slot_ids) -> np.ndarray:
    """The bias vector of a storage: bias[id] per slot, +0 where the slot holds no row."""
    slot_ids = np.asarray(slot_ids).astype(np.int64)
    return np.where(slot_ids >= 0, np.asarray(bias, dtype=np.float32)[np.maximum(slot_ids, 0)], np.float32(0.0)).astype(np.float32)


def reconstruct(codes, cb16, labels=None, c16=None) -> np.ndarray:
    """float64 [n, d]: y^ (plain), or c + r^ with labels and c16 (exact: both are fp16)."""
    y = P.decode(codes, cb16).astype(np.float64)
    return y if c16 is None else y + list_centroids(labels, c16).astype(np.float64)


# -------------------------------------------------------------------------------------------------------------- scores
def coarse(q16, c16, probes) -> np.ndarray:
    """float32 [nq, nprobe]: the biased probe score fl32(fl32(q . c) - h_c) of every probed list (an entry outside [0, K) is
    clamped into range: its value is not read)."""
    c16 = np.asarray(c16, dtype=np.float16)
    s = L.scores(q16, c16, -L.half_norms(c16))
    return np.take_along_axis(s, np.clip(np.asarray(probes).astype(np.int64), 0, len(c16) - 1), axis=1)


def scores_plain(q16, codes, cb16) -> np.ndarray:
    """float32 [nq, n]: fl32(acc + bias), a zero +0."""
    return L.scores(q16, P.decode(codes, cb16), bias_plain(codes, cb16))


def _search(q16, pre, labels, k_lists: int, probes, coarse32, k: int, visible):
    """pre: float32 [nq, n], fl32(acc + bias) of every row; coarse32 None (plain) or float32 [nq, nprobe]."""
    labels = np.asarray(labels).astype(np.int64)
    probes = np.asarray(probes).astype(np.int64)
    vis = np.ones(len(labels), dtype=bool) if visible is None else np.asarray(visible, dtype=bool)
    members = [np.flatnonzero((labels == c) & vis) for c in range(k_lists)]
    out_s = np.full((len(probes), k), -np.inf, dtype=np.float32)
    out_i = np.full((len(probes), k), -1, dtype=np.int64)
    for r, row in enumerate(probes):
        cs, ci = [], []
        for p, c in enumerate(row):
            if 0 <= c < k_lists:
                s = pre[r, members[c]]
                if coarse32 is not None:
                    s = (s + np.float32(coarse32[r, p])).astype(np.float32) + np.float32(0.0)
                cs.append(s)
                ci.append(members[c])
        if ci:
            top_s, top_i = R.topk_total_order(np.concatenate(cs), np.concatenate(ci), k)
            out_s[r], out_i[r] = top_s.astype(np.float32), top_i
    return L.sq_dist(L.half_norms(np.asarray(q16, dtype=np.float16)), out_s), out_i, out_s


def search_plain(q16, codes, cb16, labels, k_lists: int, probes, k: int, visible=None):
    """(sq_dist float32 [nq, k] ascending, ids int64, raw scores float32).  codes: of ALL rows, row number = id."""
    return _search(q16, scores_plain(q16, codes, cb16), labels, k_lists, probes, None, k, visible)


def search_residual(q16, codes, cb16, labels, c16, probes, coarse32, k: int, visible=None):
    """The same for residual codes; coarse32 float32 [nq, nprobe] (None: `coarse`, the probe's own)."""
    pre = L.scores(q16, P.decode(codes, cb16), bias_residual(codes, cb16, labels, c16))
    coarse32 = coarse(q16, c16, probes) if coarse32 is None else np.asarray(coarse32, dtype=np.float32)
    return _search(q16, pre, labels, len(c16), probes, coarse32, k, visible)


def exact_sq_dist(q16, y64) -> np.ndarray:
    """int64 [nq, n]: ||q - y||^2 of integer-valued rows."""
    q = np.asarray(q16).astype(np.int64)
    y = np.asarray(y64).astype(np.int64)
    assert np.array_equal(y, np.asarray(y64, dtype=np.float64))
    return ((q[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)


def residual_score_bound(q16, codes, cb16, labels, c16):
    """(s64 float64 [nq, n], bound float64 [nq, n]): the float64 score of every query against every reconstructed row, with
    the coarse term of the row's own list, and the bound of the device's score against it (the module text)."""
    q = np.asarray(q16).astype(np.float64)
    r = P.decode(codes, cb16).astype(np.float64)
    c16r = list_centroids(labels, c16)
    c = c16r.astype(np.float64)
    d = q.shape[1]
    y = c + r
    s64 = q @ y.T - 0.5 * (y * y).sum(axis=1)[None, :]
    big_b = ((c * r).sum(axis=1) + 0.5 * (r * r).sum(axis=1))[None, :]
    qr, qc = q @ r.T, q @ c.T
    hc = L.half_norms(np.ascontiguousarray(c16r)).astype(np.float64)[None, :]
    bound = (d * 2.0 ** -23 * (np.abs(q) @ np.abs(r).T + np.abs(q) @ np.abs(c).T)
             + 2.0 ** -24 * (np.abs(big_b) + np.abs(qr - big_b) + np.abs(qc - hc) + hc + np.abs(s64)))
    return s64, bound * (1.0 + 2.0 ** -20)


# ---------------------------------------------------------------------------------------------------------------- data
def scaled_integer_codebooks(rng, d: int, dsub: int) -> np.ndarray:
    """ivf_pq_ref.integer_codebooks with every codeword multiplied by an integer from {0, 1, 2, 3}: integer codewords of very
    different lengths, so that among reconstructed rows the nearest one and the one of the largest inner product differ."""
    cb = P.integer_codebooks(rng, d, dsub)
    return (cb * rng.integers(0, 4, cb.shape[:2])[:, :, None].astype(np.float16)).astype(np.float16)


def int_case(n: int, nq: int, d: int, n_lists: int, dsub: int = 8, seed: int = 0):
    """The integer data of the exact tests: (rows y fp16 [n, d] from l2_ref.sparse_int_rows, queries q fp16 [nq, d] from
    l2_ref.int_rows, centroids fp16 [n_lists, d] from l2_ref.int_rows, labels int32 [n] = the Euclidean nearest centroid,
    codebooks fp16 [M, 256, dsub] from `scaled_integer_codebooks`)."""
    rng = np.random.default_rng(seed + n + nq + d + n_lists + dsub)
    y, q = L.sparse_int_rows(rng, n, d), L.int_rows(rng, nq, d)
    centroids = L.int_rows(rng, n_lists, d)
    labels = L.assign(y, centroids, L.half_norms(centroids))[0]
    cb = scaled_integer_codebooks(rng, d, dsub)
    return y, q, centroids, labels, cb


def data_conditions(q16, y64, bias, total):
    """What the GPU tests rely on: (the share of queries whose nearest reconstructed row differs from the row of the largest
    inner product; every bias and every total score a multiple of 1/2 below 2^24 and equal to its float64 value).
    y64: the reconstructed rows, total: float32 [nq, n] scores with the coarse term of every row's own list."""
    q = np.asarray(q16).astype(np.float64)
    dots = q @ np.asarray(y64, dtype=np.float64).T
    s64 = dots - 0.5 * (np.asarray(y64, dtype=np.float64) ** 2).sum(axis=1)[None, :]
    l2_best = np.argsort(-s64, axis=1, kind="stable")[:, 0]
    ip_best = np.argsort(-dots, axis=1, kind="stable")[:, 0]
    bias, total = np.asarray(bias, dtype=np.float64), np.asarray(total, dtype=np.float64)
    exact = bool((np.abs(total) < 2 ** 24).all() and (total * 2 == np.round(total * 2)).all()
                 and (bias * 2 == np.round(bias * 2)).all() and np.array_equal(total, s64))
    return float((l2_best != ip_best).mean()), exact
