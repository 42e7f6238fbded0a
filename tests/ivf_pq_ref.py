"""The product quantiser and the IVF-PQ index restated in numpy: the contract sonar_amd.index.ProductQuantizer,
IVFPQIndex and smi_pq_* / smi_ivf_pq_* are tested against.  The list layout, the candidate rule and the total order are
tests/ivf_ref.py's and are called, not restated; new are the encoding of a row, the training round and the decoded row.

Shape: d = M * dsub, dsub in DSUBS, always CW = 256 codewords: codebooks fp16 [M, 256, dsub], a code row uint8 [M].

Encoding of subvector x_m against codeword c (`keys`, `encode`), all in float32:
  n2 = ((0 + c_0 c_0) + c_1 c_1) + ... ascending;  bias = -0.5 n2 (exact);
  key = fmaf(x_{dsub-1}, c_{dsub-1}, ... fmaf(x_0, c_0, bias)), one chain ascending in j;  code_m = argmax_c key, ties to
  the lower code (numpy's argmax takes the first).  A product of two fp16 values is exact in float32 (22 significant bits,
  magnitude in [2^-48, 2^32) or zero), so numpy's `acc + x * c` in float32 rounds once, like the fmaf: the chain's bits.
  tests/test_ivf_pq_cpu.py proves that with exact rationals.  Non-finite input is outside the contract.

Training round (`train_round`): encode all rows; S[m][c][j] = sum over the members of x_j * 2^24 as int64 (tests/kmeans_ref.
fixed: exact in any order; needs n * max|x| * 2^24 < 2^63, always true for normalised rows), count[m][c]; then
  c_j = fp16_rn(float32(S) / float32(count) * 2^-24): the int64 -> float32 conversion, the division and the fp16 conversion
  are each correctly rounded to nearest even, the scaling is exact.  A codeword with no member keeps its value.
`train`: codeword c of every sub-quantiser starts as that subvector of row init[c]; n_iter rounds.

Decode (`decode`): the concatenation of the M codewords.  Search (`search`): tests/ivf_ref.search on the decoded rows; its
scores are float64, exact on integer-valued operands.  On real-valued rows the engine's bits are those of the flat index on
the decoded rows (compared on the device) and lie within d * 2^-23 of the float64 score (tests/test_gpu_ivf.py).
"""
import numpy as np

from tests import ivf_ref as R
from tests import kmeans_ref as KR

ALIGN = R.ALIGN
CW = 256
DSUBS = (8, 16, 32, 64)


def split(x16, dsub: int):
    """fp16 [n, d] -> float32 [n, M, dsub]."""
    x = np.asarray(x16, dtype=np.float16)
    n, d = x.shape
    assert dsub in DSUBS and d % dsub == 0
    return x.astype(np.float32).reshape(n, d // dsub, dsub)


def biases(cb16):
    """float32 [M, 256]: -0.5 * (the ascending float32 sum of squares of every codeword)."""
    c = np.asarray(cb16, dtype=np.float16).astype(np.float32)
    n2 = np.zeros(c.shape[:2], dtype=np.float32)
    for j in range(c.shape[2]):
        n2 = n2 + c[:, :, j] * c[:, :, j]
    return np.float32(-0.5) * n2


def keys(x16, cb16):
    """float32 [n, M, 256]: the key of every subvector against every codeword of its sub-quantiser."""
    c = np.asarray(cb16, dtype=np.float16).astype(np.float32)
    x = split(x16, c.shape[2])
    assert c.shape[:2] == (x.shape[1], CW)
    key = np.broadcast_to(biases(cb16)[None], (len(x), x.shape[1], CW)).astype(np.float32)
    for j in range(c.shape[2]):
        key = key + x[:, :, None, j] * c[None, :, :, j]
    assert key.dtype == np.float32
    return key


def encode(x16, cb16, chunk: int = 256):
    """uint8 [n, M]."""
    x16 = np.asarray(x16, dtype=np.float16)
    out = [np.argmax(keys(x16[i: i + chunk], cb16), axis=2) for i in range(0, len(x16), chunk)]
    return np.concatenate(out).astype(np.uint8)


def decode(codes, cb16):
    """fp16 [n, d]: row r = the codewords codes[r] names, side by side."""
    cb16 = np.asarray(cb16, dtype=np.float16)
    codes = np.asarray(codes).astype(np.int64)
    m = cb16.shape[0]
    assert codes.shape[1] == m
    return cb16[np.arange(m)[None, :], codes].reshape(len(codes), -1)


def sums_counts(x16, codes, dsub: int):
    """(S int64 [M, 256, dsub] in units of 2^-24, counts int64 [M, 256])."""
    q = KR.fixed(np.asarray(x16, dtype=np.float16))
    n, d = q.shape
    m = d // dsub
    q = q.reshape(n, m, dsub)
    sums = np.zeros((m, CW, dsub), dtype=np.int64)
    counts = np.zeros((m, CW), dtype=np.int64)
    codes = np.asarray(codes).astype(np.int64)
    for s in range(m):
        np.add.at(sums[s], codes[:, s], q[:, s])
        counts[s] = np.bincount(codes[:, s], minlength=CW)
    return sums, counts


def finalize(sums, counts, prev16):
    """fp16 [M, 256, dsub]: fp16_rn(float32(S) / float32(count) * 2^-24), or the previous value where count = 0."""
    s32 = np.asarray(sums, dtype=np.int64).astype(np.float32)
    c32 = np.asarray(counts, dtype=np.int64).astype(np.float32)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        new = ((s32 / c32) * np.float32(2.0 ** -24)).astype(np.float16)
    return np.where(np.asarray(counts)[..., None] > 0, new, np.asarray(prev16, dtype=np.float16))


def train_round(x16, cb16):
    """(the next codebooks, the codes this round's encoding gave)."""
    cb16 = np.asarray(cb16, dtype=np.float16)
    codes = encode(x16, cb16)
    return finalize(*sums_counts(x16, codes, cb16.shape[2]), cb16), codes


def init_codebooks(x16, init, dsub: int):
    x16 = np.asarray(x16, dtype=np.float16)
    init = np.asarray(init).astype(np.int64)
    assert init.shape == (CW,) and init.min() >= 0 and init.max() < len(x16)
    n, d = x16.shape
    return np.ascontiguousarray(x16[init].reshape(CW, d // dsub, dsub).transpose(1, 0, 2))


def train(x16, init, dsub: int, n_iter: int):
    """The codebooks after every round: a list of n_iter + 1 arrays, the start first."""
    out = [init_codebooks(x16, init, dsub)]
    for _ in range(n_iter):
        out.append(train_round(x16, out[-1])[0])
    return out


def quantisation_error(x16, cb16, codes=None):
    """The mean squared distance of the rows from their reconstruction, float64."""
    codes = encode(x16, cb16) if codes is None else codes
    diff = np.asarray(x16, dtype=np.float64) - decode(codes, cb16).astype(np.float64)
    return float((diff * diff).sum(axis=1).mean())


def search(q16, codes, cb16, labels, k_lists: int, probes, k: int, s=None):
    """tests/ivf_ref.search on the decoded rows: (scores float64 [nq, k], ids int64 [nq, k]).  codes: of ALL rows, in row
    order (row number = id); s: precomputed R.scores64(q16, decode(codes, cb16))."""
    x = decode(codes, cb16)
    return R.search(q16, x, labels, k_lists, probes, k, s=R.scores64(q16, x) if s is None else s)


def integer_codebooks(rng, d: int, dsub: int):
    """fp16 [M, 256, dsub] with entries from {-1, 0, 1} (tests/ivf_ref.integer_rows): scores against integer queries are
    exact in any order."""
    return np.ascontiguousarray(R.integer_rows(rng, CW, d).reshape(CW, d // dsub, dsub).transpose(1, 0, 2))


def random_codebooks(rng, d: int, dsub: int, scale: float = 1.0):
    return (rng.standard_normal((d // dsub, CW, dsub)) * scale / np.sqrt(d)).astype(np.float16)
