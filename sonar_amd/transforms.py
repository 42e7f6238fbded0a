"""Learned linear transforms in front of the indexes: PCA and OPQ on the MI355X engine.

A PCA cuts 1024-d SONAR rows to 256 or 512 dimensions before they are stored; an OPQ rotation (Ge et al., "Optimized Product
Quantization"; FAISS's `OPQMatrix`) turns the rows so that the sub-spaces of a product quantiser carry equal shares of the
variance and are as uncorrelated as a rotation can make them, which is what real, anisotropic embeddings need -- the index
strings of the LASER / NLLB mining recipes begin with `OPQ64,` or `PCA...,` for that reason.

What runs where.  The one product that is too long for anything else here, C = X^T Y contracted over the n rows of a corpus,
is `gram` (smi_gram: fp16 operands, exact products, fp32 MFMA sums inside chunks of `GRAM_CHUNK_ROWS` rows, fp64 across them,
one fixed order: the same bits on every run and grid).  The mean is an exact int64 column sum (`column_sums`,
smi_kmeans_update with one cluster).  Applying a transform is smi_gemm_tn on the pinned 128 x 128 engine.  The PQ rounds
inside OPQ are `index.pq_train` / `pq_encode` / `pq_decode`.  The d x d eigen- and singular-value decompositions run on the
HOST in fp64 (`torch.linalg.eigh` / `svd`) after one read-back of the matrix: fitting synchronises with the host and cannot be
captured in a graph; `apply` reads nothing back.  There is no CPU path.

`sonar_amd.index.PreTransformIndex` puts a transform in front of an index (FAISS's `IndexPreTransform`).

Not here: whitening (FAISS's `eigen_power`), random rotations, an OPQ with d_out < d_in, transforms inside the
`state_dict` of the bare index classes.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

from . import _lib
from .clustering import init_rows, update
from .index import PQ_CODEWORDS, _check_device_tensor, _check_dsub, _check_matrix, _check_rows16, pq_decode, pq_encode, pq_train
from .xsim import normalize_rows

GRAM_CHUNK_ROWS = 2048  # SMI_GRAM_CHUNK_ROWS: the rows whose products one fp32 accumulator takes before it is widened to fp64
GRAM_MAX_DIM = 8192     # d1, d2 of smi_gram
_ENGINE_128 = 1 << 8    # smi_gemm_tn's engine selector 1: the 128 x 128 tiles, whatever the row count


def gram(x: torch.Tensor, y: Optional[torch.Tensor] = None, n: Optional[int] = None) -> torch.Tensor:
    """smi_gram: fp64 [d1, d2] on the device, out[i, j] = sum over the first n rows (default: all of x) of x[r, i] * y[r, j].
    x contiguous fp16 [>= n, d1], y contiguous fp16 [>= n, d2] or None (y = x: only the upper triangle is computed and the
    result is bitwise symmetric); d1, d2 multiples of 64, at most 8192.  The numerics are the contract of
    include/sonar_mi355.h: exact for integer-valued rows whose chunk sums stay below 2^24, the same bits on every run.
    Enqueued on the current stream; nothing is read back."""
    n = _check_rows16(x, "x", n)
    d1 = d2 = x.shape[1]
    if y is not None:
        _check_rows16(y, "y", n)
        if y.device != x.device:
            raise ValueError("x and y must be on the same device")
        d2 = y.shape[1]
    if max(d1, d2) > GRAM_MAX_DIM:
        raise ValueError(f"dim = {max(d1, d2)} exceeds {GRAM_MAX_DIM}")
    lib = _lib.load()
    ws_bytes = int(lib.smi_gram_ws_bytes(n, d1, d2))
    if ws_bytes < 1:
        raise ValueError(f"{n} rows of dims {d1}, {d2}: too large for one call")
    if y is None:  # the upper triangle's tile slots only (include/sonar_mi355.h)
        t = (d1 + 127) // 128
        ws_bytes = ws_bytes // (t * t) * (t * (t + 1) // 2)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    out = torch.empty((d1, d2), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.smi_gram(x.data_ptr(), None if y is None else y.data_ptr(), n, d1, d2, out.data_ptr(), ws.data_ptr(),
                                ws_bytes, _lib.current_stream_ptr()))
    return out


def column_sums(x: torch.Tensor, n: Optional[int] = None) -> torch.Tensor:
    """int64 [d] on the device: the sums of the columns of the first n rows (default: all) of x (contiguous fp16 [>= n, d])
    in units of 2^-24, EXACT (smi_kmeans_update with one cluster and every label 0; an Inf or NaN element counts as 0).
    mean = sums * 2^-24 / n in fp64."""
    n = _check_rows16(x, "x", n)
    labels = torch.zeros((n,), dtype=torch.int32, device=x.device)
    return update(x, labels, 1)[0][0]


def _rows16(x, name: str, d: int) -> torch.Tensor:
    """x (fp16 / fp32 [n, d] on the device) as a contiguous fp16 matrix; fp32 is converted by smi_cast."""
    _check_matrix(x, name)
    if x.shape[1] != d:
        raise ValueError(f"{name} has dim {x.shape[1]}, the transform takes {d}")
    if x.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"{name} must be fp16 or fp32, got {x.dtype}")
    return _lib.cast(x.contiguous(), torch.float16)


def _fix_signs(v: torch.Tensor) -> torch.Tensor:
    """The columns of v (host fp64 [d, m]) with the sign that makes their largest-magnitude component positive, ties to the
    lower index."""
    a = v.abs()
    first = (a == a.max(dim=0, keepdim=True)[0]).to(torch.int8).argmax(dim=0)  # the first row that attains the maximum
    lead = v[first, torch.arange(v.shape[1])]
    return v * torch.where(lead < 0, -1.0, 1.0).to(v.dtype)


def _eigh_descending(c: torch.Tensor):
    """(eigenvalues descending, eigenvectors as sign-fixed columns) of a symmetric host fp64 matrix."""
    w, v = torch.linalg.eigh(c)
    return w.flip(0).contiguous(), _fix_signs(v.flip(1).contiguous())


def balanced_bins(eigenvalues, n_bins: int) -> List[List[int]]:
    """FAISS's balanced allocation (Ge et al.'s parametric solution): take the eigenvalues in the order given (descending) and
    give each to the bin with the smallest running sum of log-eigenvalues that still has room (len / n_bins places), ties to
    the lower bin.  An eigenvalue below 2^-52 of the largest counts as that.  Returns the indices of every bin, in the order
    they arrived."""
    ev = [float(e) for e in eigenvalues]
    if n_bins < 1 or len(ev) % n_bins:
        raise ValueError(f"{len(ev)} eigenvalues over {n_bins} bins")
    cap = len(ev) // n_bins
    floor = max(max(ev), 5e-324) * 2.0 ** -52
    bins: List[List[int]] = [[] for _ in range(n_bins)]
    acc = [0.0] * n_bins
    for i, e in enumerate(ev):
        best = min((b for b in range(n_bins) if len(bins[b]) < cap), key=lambda b: (acc[b], b))
        bins[best].append(i)
        acc[best] += math.log(max(e, floor))
    return bins


class LinearTransform:
    """y = f16(x . matrix^T + bias), applied on the device.

    matrix: [d_out, d_in] on the device (any float dtype; kept in fp64 as `matrix64` and, rounded, in fp16 as `matrix`, the
    W[n, k] of smi_gemm_tn), d_in a multiple of 64, d_out a multiple of 128; bias: [d_out] or None (kept in fp32)."""

    def __init__(self, matrix: torch.Tensor, bias: Optional[torch.Tensor] = None):
        _check_device_tensor(matrix, "matrix")
        if matrix.dim() != 2 or not matrix.is_floating_point():
            raise ValueError(f"matrix must be a floating-point [d_out, d_in] matrix, got {matrix.dtype} {list(matrix.shape)}")
        d_out, d_in = matrix.shape
        if d_in < 64 or d_in % 64:
            raise ValueError(f"d_in = {d_in} must be a multiple of 64")
        if d_out < 128 or d_out % 128:
            raise ValueError(f"d_out = {d_out} must be a multiple of 128")
        if bias is not None:
            _check_device_tensor(bias, "bias")
            if tuple(bias.shape) != (d_out,) or not bias.is_floating_point():
                raise ValueError(f"bias must be a floating-point [{d_out}] vector, got {bias.dtype} {list(bias.shape)}")
        self._m64 = matrix.detach().to(torch.float64).contiguous().clone()
        self._w = self._m64.to(torch.float32).to(torch.float16).contiguous()
        self._has_bias = bias is not None
        self._bias = (torch.zeros((d_out,), dtype=torch.float32, device=matrix.device) if bias is None
                      else bias.detach().to(torch.float32).contiguous().clone())

    # ------------------------------------------------------------------------------------------------ properties
    @property
    def d_in(self) -> int:
        return self._w.shape[1]

    @property
    def d_out(self) -> int:
        return self._w.shape[0]

    @property
    def matrix(self) -> torch.Tensor:
        """fp16 [d_out, d_in]: what `apply` multiplies by."""
        return self._w

    @property
    def matrix64(self) -> torch.Tensor:
        """fp64 [d_out, d_in]: what the transform was made from."""
        return self._m64

    @property
    def bias(self) -> Optional[torch.Tensor]:
        """fp32 [d_out], or None."""
        return self._bias if self._has_bias else None

    # ------------------------------------------------------------------------------------------------ apply
    def apply(self, x: torch.Tensor) -> torch.Tensor:
        """fp16 [n, d_out] = f16(x . matrix^T + bias) for x fp16 / fp32 [n, d_in] on the device (fp32 is rounded to fp16
        first, by smi_cast).  smi_gemm_tn with the 128 x 128 engine pinned, so the bits of a row do not depend on the rows
        around it or on their number.  The full 128-row blocks are multiplied where they lie; only the last n % 128 rows go
        through a zero-padded 128-row copy.  Enqueued on the current stream, nothing is read back."""
        x16 = _rows16(x, "x", self.d_in)
        n, d_in, d_out = x16.shape[0], self.d_in, self.d_out
        if x16.device != self._w.device:
            raise ValueError(f"x is on {x16.device}, the transform on {self._w.device}")
        out = torch.empty((n, d_out), dtype=torch.float16, device=x16.device)
        full = n // 128 * 128
        if full >= 2 ** 31:
            raise ValueError(f"{n} rows: row numbers must fit int32")
        lib = _lib.load()
        with torch.cuda.device(x16.device):
            if full:
                _lib.check(lib.smi_gemm_tn(_ENGINE_128, x16.data_ptr(), self._w.data_ptr(), self._bias.data_ptr(),
                                           out.data_ptr(), full, d_out, d_in, d_out, _lib.current_stream_ptr()))
            if n > full:
                tail = torch.zeros((128, d_in), dtype=torch.float16, device=x16.device)
                tail[: n - full] = x16[full:]
                tail_out = torch.empty((128, d_out), dtype=torch.float16, device=x16.device)
                _lib.check(lib.smi_gemm_tn(_ENGINE_128, tail.data_ptr(), self._w.data_ptr(), self._bias.data_ptr(),
                                           tail_out.data_ptr(), 128, d_out, d_in, d_out, _lib.current_stream_ptr()))
                out[full:] = tail_out[: n - full]
        return out

    __call__ = apply

    # ------------------------------------------------------------------------------------------------ persistence
    def state_dict(self) -> Dict[str, torch.Tensor]:
        """matrix (fp16), matrix64 (fp64) and, where there is one, bias (fp32)."""
        state = {"matrix": self._w.clone(), "matrix64": self._m64.clone()}
        if self._has_bias:
            state["bias"] = self._bias.clone()
        return state

    @classmethod
    def from_state_dict(cls, state: Dict[str, torch.Tensor]) -> "LinearTransform":
        """A plain `LinearTransform` with the bits of `apply` of the one that was saved (whatever class that was)."""
        if "matrix" not in state:
            raise ValueError("state lacks ['matrix']")
        t = LinearTransform(state.get("matrix64", state["matrix"]), state.get("bias"))
        w = state["matrix"]
        if not w.is_cuda or w.dtype != torch.float16 or tuple(w.shape) != tuple(t._w.shape):
            raise ValueError(f"matrix must be fp16 {list(t._w.shape)} on the device")
        t._w = w.contiguous().clone()
        return t


def _check_fit_rows(x, name: str):
    _check_matrix(x, name)
    if x.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"{name} must be fp16 or fp32, got {x.dtype}")
    if x.shape[1] > GRAM_MAX_DIM:
        raise ValueError(f"{name}: dim = {x.shape[1]} exceeds {GRAM_MAX_DIM}")


class PCA(LinearTransform):
    """A `LinearTransform` onto the leading principal axes (`fit`).  `explained_variance`: fp64 [d_out] on the host, the
    eigenvalues of the covariance matrix that belong to the rows of `matrix`, descending; `mean`: fp64 [d_in] on the device
    (zeros without centring)."""

    explained_variance: torch.Tensor
    mean: torch.Tensor

    @classmethod
    def fit(cls, x: torch.Tensor, d_out: Optional[int] = None, center: bool = True) -> "PCA":
        """The PCA of the rows of x (fp16 / fp32 [n, d] on the device, n >= 2; fp32 is rounded to fp16 first: the statistics
        are those of the fp16 rows).  d_out: the axes kept (default d), a multiple of 128.

        C = (gram(x) - n mu mu^T) / (n - 1) in fp64 on the device, mu from the exact `column_sums` (center=False: C =
        gram(x) / (n - 1), mu = 0).  C is READ BACK once and decomposed on the host (`torch.linalg.eigh`, fp64): the call
        synchronises with the host.  The eigenvectors come in descending order of their eigenvalues, each with the sign that
        makes its largest-magnitude component positive (ties to the lower index).  matrix = V[:, :d_out]^T, bias = -matrix mu
        (none with center=False)."""
        _check_fit_rows(x, "x")
        n, d = x.shape
        d_out = d if d_out is None else d_out
        if isinstance(d_out, bool) or not isinstance(d_out, int) or d_out < 128 or d_out % 128 or d_out > d:
            raise ValueError(f"d_out = {d_out!r}: a multiple of 128, at most dim = {d}")
        if n < 2:
            raise ValueError("a covariance needs at least 2 rows")
        x16 = _rows16(x, "x", d)
        c = gram(x16)
        mu = torch.zeros((d,), dtype=torch.float64, device=x.device)
        if center:
            mu = column_sums(x16).to(torch.float64) * (2.0 ** -24 / n)
            c = c - n * torch.outer(mu, mu)
        c = c / (n - 1)
        w, v = _eigh_descending(c.cpu())  # the read-back
        m64 = v[:, :d_out].t().contiguous().to(x.device)
        t = cls(m64, -(m64 @ mu) if center else None)
        t.explained_variance = w[:d_out].clone()
        t.mean = mu
        return t


def _relative_error(xr: torch.Tensor, xhat: torch.Tensor, n: int) -> float:
    """sum ||xr - xhat||^2 / sum ||xr||^2 over the first n rows, in blocks on the device (fp32 differences, fp64 sums)."""
    num = torch.zeros((), dtype=torch.float64, device=xr.device)
    den = torch.zeros((), dtype=torch.float64, device=xr.device)
    for lo in range(0, n, 1 << 16):
        a, b = xr[lo:min(n, lo + (1 << 16))].float(), xhat[lo:min(n, lo + (1 << 16))].float()
        num += ((a - b) ** 2).sum(dtype=torch.float64)
        den += (a ** 2).sum(dtype=torch.float64)
    return float((num / den).item())


class OPQ(LinearTransform):
    """A square `LinearTransform` without bias: the rotation of an optimised product quantiser (`fit`).  `dsub`; `history`:
    the relative quantisation error sum ||xr - decode(encode(xr))||^2 / sum ||xr||^2 of every round, n_iter numbers, entry t
    under the rotation that round t began with (entry 0: the start rotation); `codebooks` (fp16 [d / dsub, 256, dsub]): those
    of the last round, trained one Procrustes step before `matrix`, for `IVFPQIndex` to start from (None with n_iter = 0)."""

    dsub: int
    codebooks: Optional[torch.Tensor]
    history: List[float]

    @classmethod
    def fit(cls, x: torch.Tensor, dsub: int, n_iter: int = 4, pq_iter: int = 4, seed: int = 0,
            n_train: Optional[int] = None) -> "OPQ":
        """Fit on the first n_train rows (default: all, at least 256) of `normalize_rows(x)`, what the indexes store (x fp16 /
        fp32 [n, d] on the device, d a multiple of 128 and of dsub, dsub in {8, 16, 32, 64}).

        Start: the eigenvectors of gram(xn) (no centring), dealt to the d / dsub sub-spaces by `balanced_bins`.  Then n_iter
        rounds: xr = apply(xn); codebooks = pq_train(xr, dsub, rows of `init_rows(n, 256, seed)`, pq_iter); xhat =
        pq_decode(pq_encode(xr)); M = gram(xn, xhat); M = U S V^T on the host; R = U V^T, the orthogonal matrix that
        minimises ||xn R - xhat||_F; matrix = R^T.  Every decomposition READS a d x d matrix BACK: the call synchronises with
        the host n_iter + 1 times and more (the errors of `history` are read back too)."""
        _check_fit_rows(x, "x")
        n, d = x.shape
        _check_dsub(dsub, d)
        if d % 128:
            raise ValueError(f"dim = {d} must be a multiple of 128 (the rotation is a square LinearTransform)")
        for v, name in ((n_iter, "n_iter"), (pq_iter, "pq_iter")):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"{name} = {v!r}: a non-negative integer")
        n = n if n_train is None else n_train
        if isinstance(n, bool) or not isinstance(n, int) or not PQ_CODEWORDS <= n <= x.shape[0]:
            raise ValueError(f"n_train = {n!r}: between {PQ_CODEWORDS} and the {x.shape[0]} rows of x")
        xn = normalize_rows(x)
        init = init_rows(n, PQ_CODEWORDS, seed).to(device=x.device, dtype=torch.int32)
        w, v = _eigh_descending(gram(xn, n=n).cpu())  # read-back
        order = [i for b in balanced_bins(w.tolist(), d // dsub) for i in b]
        t = cls(v[:, order].t().contiguous().to(x.device))
        codebooks, history = None, []
        for _ in range(n_iter):
            xr = t.apply(xn[:n])
            codebooks = pq_train(xr, dsub, init, pq_iter, n)
            xhat = pq_decode(pq_encode(xr, codebooks, n), codebooks)
            history.append(_relative_error(xr, xhat, n))
            u, _, vh = torch.linalg.svd(gram(xn, xhat, n).cpu())  # read-back
            t = cls((u @ vh).t().contiguous().to(x.device))
        t.dsub, t.codebooks, t.history = dsub, codebooks, history
        return t
