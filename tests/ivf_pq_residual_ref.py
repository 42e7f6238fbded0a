"""Residual encoding against the list centroid for the IVF-PQ index, restated in numpy: the contract
sonar_amd.index.IVFPQResidualIndex and smi_pq_*_residual / smi_ivf_pq_*_residual are tested against.  The product quantiser
is tests/ivf_pq_ref.py's and the list layout and total order tests/ivf_ref.py's; they are called, not restated.  New are the
residual of a row and the score of a search.

Residual of row i with label l in [0, K), c16 the fp16 centroid table [K, d]:
  r_i[j] = fp16_rn(fp32_rn((float)x_i[j] - (float)c16[l][j])), two roundings to nearest even: numpy's
  (x.astype(f32) - c.astype(f32)).astype(f16).  A label outside [0, K) addresses nothing: the residual is the row itself.
Training, encoding, decoding: tests/ivf_pq_ref.py on the residuals.
Search: per probe column the top-k of that list on the decoded residuals, `coarse` (float32 [nq, nprobe]) added to the scores
  of that column, then the columns merged by (score descending, id ascending).  Nothing is added to an empty entry, and the
  coarse entry of a probe that names no list is not read.  The scores are float64 here (the sum of the float64 residual score
  and the float32 coarse value): exact on integer-valued operands; on real-valued ones the device's fl32(acc + coarse) lies
  within (d + 2) * 2^-23 of it -- d * 2^-23 for the fp32 accumulation (tests/test_gpu_ivf.py), and one more rounding of a
  sum below 4 in magnitude, half an ulp of at most 2^-22: 2^-23 of the 2 * 2^-23 the bound adds.
"""
import numpy as np

from tests import ivf_pq_ref as P
from tests import ivf_ref as R


def residuals(x16, labels, c16):
    """fp16 [n, d]."""
    x = np.asarray(x16, dtype=np.float16)
    c = np.asarray(c16, dtype=np.float16)
    labels = np.asarray(labels).astype(np.int64)
    ok = (labels >= 0) & (labels < len(c))
    out = x.copy()
    out[ok] = (x[ok].astype(np.float32) - c[labels[ok]].astype(np.float32)).astype(np.float16)
    return out


def train(x16, labels, c16, init, dsub: int, n_iter: int):
    """tests/ivf_pq_ref.train on the residuals: the codebooks after every round, the start (the residuals of the rows init
    names) first."""
    return P.train(residuals(x16, labels, c16), init, dsub, n_iter)


def encode(x16, labels, c16, cb16):
    """uint8 [n, M]: the codes of the residuals."""
    return P.encode(residuals(x16, labels, c16), cb16)


def merge(col_scores, col_ids, k: int):
    """The k best of the columns' lists in the total order.  col_scores / col_ids: [nprobe][nq, k], -1 ids = no entry."""
    s = np.concatenate([np.asarray(c) for c in col_scores], axis=1)
    i = np.concatenate([np.asarray(c) for c in col_ids], axis=1).astype(np.int64)
    out_s, out_i = np.full((len(s), k), -np.inf, dtype=s.dtype), np.full((len(s), k), -1, dtype=np.int64)
    for r in range(len(s)):
        have = i[r] >= 0
        top_s, top_i = R.topk_total_order(s[r, have], i[r, have], k)
        out_s[r], out_i[r] = top_s.astype(s.dtype), top_i
    return out_s, out_i


def add_coarse(scores, ids, coarse_col):
    """scores [nq, k] + coarse_col [nq] where there is an entry (id >= 0), in the dtype of scores; -inf elsewhere."""
    scores = np.asarray(scores)
    with np.errstate(invalid="ignore", over="ignore"):
        total = scores + np.asarray(coarse_col)[:, None].astype(scores.dtype)
    return np.where(np.asarray(ids) >= 0, total, -np.inf).astype(scores.dtype)


def search(q16, codes, cb16, labels, k_lists: int, probes, coarse, k: int, s=None):
    """(scores float64 [nq, k], ids int64 [nq, k]).  codes: the residual codes of ALL rows, in row order (row number = id);
    coarse float32 [nq, nprobe]; s: precomputed R.scores64(q16, P.decode(codes, cb16))."""
    probes = np.asarray(probes).astype(np.int64)
    coarse = np.asarray(coarse, dtype=np.float32)
    assert coarse.shape == probes.shape
    x = P.decode(codes, cb16)
    s = R.scores64(q16, x) if s is None else s
    cols = [R.search(q16, x, labels, k_lists, probes[:, p: p + 1], k, s=s) for p in range(probes.shape[1])]
    return merge([add_coarse(cs, ci, coarse[:, p]) for p, (cs, ci) in enumerate(cols)], [ci for _, ci in cols], k)
