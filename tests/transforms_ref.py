"""numpy fp64 restatement of sonar_amd/transforms.py and of smi_gram's contract (sonar_amd/csrc/gram.hip):
the chunked Gram matrix (an exact integer path in int64, and the any-order fp32 error bound for real values), the PCA with
its sign rule, the balanced allocation of eigenvalues, the orthogonal Procrustes step, a plain Lloyd product quantiser, the
OPQ loop over them, and the planted anisotropic data the quality criterion is stated on."""
import math

import numpy as np

CHUNK_ROWS = 2048  # SMI_GRAM_CHUNK_ROWS
CODEWORDS = 256


# ------------------------------------------------------------------------------------------------------------ Gram
def gram_int(x, y=None, chunk=CHUNK_ROWS):
    """x^T y for integer-valued operands, by the contract's chunks: every chunk's sums must be exact in fp32 (below 2^24 in
    magnitude, asserted on the sums of the magnitudes), and the chunks are added as integers.  int64 [d1, d2].  A chunk's
    product is formed in fp64, where integers of this size are exact, so that BLAS does the work."""
    xf = np.asarray(x, dtype=np.float64)
    yf = xf if y is None else np.asarray(y, dtype=np.float64)
    assert np.array_equal(xf, np.rint(xf)) and np.array_equal(yf, np.rint(yf)), "integer-valued operands"
    out = np.zeros((xf.shape[1], yf.shape[1]), dtype=np.int64)
    for lo in range(0, xf.shape[0], chunk):
        assert (np.abs(xf[lo:lo + chunk]).T @ np.abs(yf[lo:lo + chunk])).max() < 2 ** 24, \
            "a chunk sum leaves the exact range of fp32"
        out += (xf[lo:lo + chunk].T @ yf[lo:lo + chunk]).astype(np.int64)
    return out


def gram64(x, y=None):
    x = np.asarray(x, dtype=np.float64)
    return x.T @ (x if y is None else np.asarray(y, dtype=np.float64))


def gram_bound(x, y=None, chunk=CHUNK_ROWS):
    """The elementwise bound on |smi_gram - gram64| for finite operands: the products are exact, a chunk adds at most
    `chunk` of them in fp32 in some order (error <= (chunk - 1) 2^-24 sum |products| to first order, for any order), and the
    fp64 adds are far below that."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    y = x if y is None else np.abs(np.asarray(y, dtype=np.float64))
    return (chunk - 1) * 2.0 ** -24 * (x.T @ y)


# ------------------------------------------------------------------------------------------------------------ PCA
def fix_signs(v):
    """Columns of v with their largest-magnitude component positive, ties to the lower index."""
    v = np.array(v, dtype=np.float64)
    for j in range(v.shape[1]):
        a = np.abs(v[:, j])
        first = int(np.flatnonzero(a == a.max())[0])
        if v[first, j] < 0:
            v[:, j] = -v[:, j]
    return v


def eigh_descending(c):
    w, v = np.linalg.eigh(c)
    return w[::-1].copy(), fix_signs(v[:, ::-1])


def covariance(x, center=True):
    """(C, mu): C = (x^T x - n mu mu^T) / (n - 1), or x^T x / (n - 1) and mu = 0 without centring."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mu = x.sum(axis=0) / n if center else np.zeros(x.shape[1])
    return (x.T @ x - n * np.outer(mu, mu)) / (n - 1), mu


def pca(x, d_out=None, center=True):
    """(matrix [d_out, d], bias [d_out] or None, explained_variance [d_out], mu)."""
    c, mu = covariance(x, center)
    w, v = eigh_descending(c)
    d_out = c.shape[0] if d_out is None else d_out
    m = v[:, :d_out].T.copy()
    return m, (-(m @ mu) if center else None), w[:d_out], mu


# ------------------------------------------------------------------------------------------------------------ OPQ
def balanced_bins(eigenvalues, n_bins):
    """Descending eigenvalues, each to the bin with the smallest running sum of log-eigenvalues that has room; ties to the
    lower bin.  An eigenvalue below 2^-52 of the largest counts as that."""
    ev = [float(e) for e in eigenvalues]
    assert len(ev) % n_bins == 0
    cap = len(ev) // n_bins
    floor = max(max(ev), 5e-324) * 2.0 ** -52
    bins, acc = [[] for _ in range(n_bins)], [0.0] * n_bins
    for i, e in enumerate(ev):
        best = None
        for b in range(n_bins):
            if len(bins[b]) < cap and (best is None or acc[b] < acc[best]):
                best = b
        bins[best].append(i)
        acc[best] += math.log(max(e, floor))
    return bins


def procrustes(x, xhat):
    """The orthogonal R that minimises ||x R - xhat||_F: U V^T of x^T xhat = U S V^T."""
    u, _, vt = np.linalg.svd(gram64(x, xhat))
    return u @ vt


def pq_encode(x, codebooks):
    """codes [n, M]: per sub-space the Euclidean nearest codeword, ties to the lower code."""
    m, _, dsub = codebooks.shape
    codes = np.empty((x.shape[0], m), dtype=np.int64)
    for j in range(m):
        s, c = x[:, j * dsub:(j + 1) * dsub], codebooks[j]
        dist = (s * s).sum(1)[:, None] - 2.0 * (s @ c.T) + (c * c).sum(1)[None, :]
        codes[:, j] = dist.argmin(axis=1)
    return codes


def pq_decode(codes, codebooks):
    return np.concatenate([codebooks[j][codes[:, j]] for j in range(codebooks.shape[0])], axis=1)


def pq_train(x, dsub, init_rows, n_iter):
    """Plain Lloyd rounds per sub-space, started from the sub-vectors of the rows init_rows names; an empty codeword keeps
    its value.  codebooks fp64 [M, 256, dsub]."""
    x = np.asarray(x, dtype=np.float64)
    m = x.shape[1] // dsub
    codebooks = np.stack([x[init_rows, j * dsub:(j + 1) * dsub] for j in range(m)]).copy()
    for _ in range(n_iter):
        codes = pq_encode(x, codebooks)
        for j in range(m):
            s = x[:, j * dsub:(j + 1) * dsub]
            counts = np.bincount(codes[:, j], minlength=codebooks.shape[1])
            sums = np.zeros_like(codebooks[j])
            np.add.at(sums, codes[:, j], s)
            have = counts > 0
            codebooks[j][have] = sums[have] / counts[have, None]
    return codebooks


def pq_error(x, dsub, init_rows, n_iter):
    """(relative quantisation error sum ||x - xhat||^2 / sum ||x||^2, xhat) of a product quantiser trained on x itself."""
    x = np.asarray(x, dtype=np.float64)
    codebooks = pq_train(x, dsub, init_rows, n_iter)
    xhat = pq_decode(pq_encode(x, codebooks), codebooks)
    return float(((x - xhat) ** 2).sum() / (x ** 2).sum()), xhat


def opq(x, dsub, n_iter, pq_iter, init_rows):
    """(R [d, d] with xr = x R, history): the start rotation from the eigenvectors of x^T x dealt by `balanced_bins`, then
    n_iter Procrustes rounds; history[t] = the error of the product quantiser trained under the rotation after t rounds."""
    x = np.asarray(x, dtype=np.float64)
    w, v = eigh_descending(gram64(x))
    order = [i for b in balanced_bins(w, x.shape[1] // dsub) for i in b]
    r = v[:, order]
    history = []
    for it in range(n_iter + 1):
        err, xhat = pq_error(x @ r, dsub, init_rows, pq_iter)
        history.append(err)
        if it < n_iter:
            r = procrustes(x, xhat)
    return r, history


# ------------------------------------------------------------------------------------------------------------ data
def planted(seed, n=4096, d=128, lo=0.05):
    """Anisotropic rows: a spectrum falling geometrically from 1 to `lo`, mixed by a random orthogonal matrix, rows
    normalised and rounded to fp16.  float16 [n, d]."""
    rng = np.random.default_rng(seed)
    scale = lo ** (np.arange(d) / (d - 1))
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    x = (rng.standard_normal((n, d)) * scale) @ q
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float16)
