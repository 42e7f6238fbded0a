"""The int8 scalar-quantised IVF index restated in numpy: the contract sonar_amd.index.IVFInt8Index and
smi_ivf_i8_* are tested against, bit for bit.  The list layout, the candidate rule and the total order are tests/ivf_ref.py's
and are called, not restated; what is new is the encoding of a row and the arithmetic of a score.

Encoding of one fp16 row x (`encode`): amax = max |x_j|; inv = 127 / amax and scale = amax / 127 in float32 (numpy's
float32 division is correctly rounded, as the device's is); code_j = clip(rint(float32(x_j * inv)), -127, 127), ties to even.
A zero row has all codes 0 and scale 0.  Non-finite elements are outside the contract.

Score (`scores`): acc = the integer dot product of the two code rows (exact; |acc| <= 127^2 d < 2^31 for d <= MAX_DIM);
score = float32(float32(float32(acc) * scale_x) * scale_q), the conversion to nearest even.  No summation order appears: the
bits depend on the two fp16 rows alone.

Error bound (`bound`): with t_j = 127 x_j / amax the device rounds rint(t_j (1 + e)) with |e| <= 2^-23 (the division
and the product), so code_j = t_j + r_j with |r_j| <= 1/2 + 127 * 2^-23, and x_j = S (code_j - r_j) with S = amax / 127.  Then
  x . q = S_x S_q (acc - sum cq_j rx_j - sum cx_j rq_j + sum rx_j rq_j),
  |x . q - S_x S_q acc| <= S_x S_q (1/2 sum |cq| + 1/2 sum |cx| + 1/4 d) (1 + 2^-14),
and the returned score differs from S_x S_q acc by the roundings of the two scales, of the conversion and of the two
products: five factors (1 + e), |e| <= 2^-24, at most 6 * 2^-24 |score| in all.
"""
import numpy as np

from tests import ivf_ref as R

ALIGN = R.ALIGN
MAX_DIM = 131072  # SMI_IVF_I8_MAX_DIM
assert 127 * 127 * MAX_DIM < 2 ** 31


def encode(x16):
    """(codes int8 [n, d], scales float32 [n]) of fp16 rows [n, d]."""
    x = np.asarray(x16, dtype=np.float16).astype(np.float32)
    amax = np.abs(x).max(axis=1)
    with np.errstate(divide="ignore"):
        inv = np.where(amax > 0, np.float32(127) / amax, np.float32(0)).astype(np.float32)
    codes = np.clip(np.rint(x * inv[:, None]), -127, 127).astype(np.int8)
    return codes, (amax / np.float32(127)).astype(np.float32)


def int_dots(cq, cx):
    """int64 [nq, n]: the exact dot products of code rows.  Through float64, where every product and partial sum of at most
    127^2 * MAX_DIM < 2^53 is exact in any order."""
    acc = np.asarray(cq, dtype=np.float64) @ np.asarray(cx, dtype=np.float64).T
    assert np.array_equal(acc, np.rint(acc)) and np.abs(acc).max(initial=0) < 2 ** 31
    return acc.astype(np.int64)


def scores_from_codes(cq, sq, cx, sx):
    acc = int_dots(cq, cx).astype(np.float32)  # int -> float32, to nearest even
    return (acc * np.asarray(sx, dtype=np.float32)[None, :]) * np.asarray(sq, dtype=np.float32)[:, None]


def scores(q16, x16):
    """float32 [nq, n]: the score of every query row against every corpus row."""
    return scores_from_codes(*encode(q16), *encode(x16))


def search(q16, x16, labels, k_lists: int, probes, k: int, s=None):
    """tests/ivf_ref.search on the quantised scores: (scores float64 [nq, k] holding float32 values, ids int64 [nq, k])."""
    s = scores(q16, x16) if s is None else s
    return R.search(q16, x16, labels, k_lists, probes, k, s=np.asarray(s, dtype=np.float64))


def l1(codes):
    return np.abs(np.asarray(codes, dtype=np.float64)).sum(axis=-1)


def bound(l1q, sq, l1x, sx, d: int, score):
    """The derived bound on |score - the float64 dot product of the two fp16 rows|; l1q / sq of the query row, l1x / sx of the
    corpus row and score = the returned score, arrays that broadcast against each other."""
    quant = np.asarray(sq, dtype=np.float64) * np.asarray(sx, dtype=np.float64) * (0.5 * l1q + 0.5 * l1x + 0.25 * d)
    return quant * (1 + 2.0 ** -14) + 6 * 2.0 ** -24 * np.abs(np.asarray(score, dtype=np.float64))


def half_tie_rows(d: int):
    """Rows on which inv is exactly 128 and every x_j * inv an exact half: amax = 127 * 2^-7 and elements (m + 1/2) * 2^-7,
    m = -127 .. 126 in turn, so rint must go to the even neighbour.  fp16 [2, d]; the second row has no element at amax but
    one at -amax."""
    m = (np.arange(d) % 254) - 127
    a = ((m + 0.5) * 2.0 ** -7).astype(np.float16)
    assert np.array_equal(a.astype(np.float64), (m + 0.5) * 2.0 ** -7)
    b = a.copy()
    a[0], b[0] = 127 * 2.0 ** -7, -127 * 2.0 ** -7
    return np.stack([a, b])


def edge_rows(rng, d: int):
    """fp16 [9, d]: a zero row, a one-hot row, rows of +-amax only, the exact-half rows, a row at fp16's largest finite value,
    a row of subnormals, a row with -0 in it, a constant row."""
    z = np.zeros(d, dtype=np.float16)
    hot = z.copy()
    hot[d // 3] = -0.37
    sat = (rng.choice([-1.0, 1.0], d) * 0.0313).astype(np.float16)
    big = rng.standard_normal(d).astype(np.float16)
    big[1], big[2] = 65504.0, -65504.0
    sub = (rng.integers(-1023, 1024, d) * 2.0 ** -24).astype(np.float16)
    neg0 = rng.standard_normal(d).astype(np.float16)
    neg0[::2] = -0.0
    one = np.full(d, 3.0, dtype=np.float16)
    return np.stack([z, hot, sat, *half_tie_rows(d), big, sub, neg0, one])
