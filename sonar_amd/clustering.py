"""Spherical k-means over sentence embeddings on the MI355X engine.

Similarity is cosine, as everywhere SONAR embeddings are compared here: a row belongs to the nearest of K unit centroids and
a centroid is the normalised sum of its members.  The assignment is `smi_xsim_topk` with k = 1 against the normalised
centroids (the mining kernel, unchanged); the centroid update is `smi_kmeans_update`, an exact int64 scatter-reduce of the
fp16 rows, so one seed gives one run bit for bit.  `smi_kmeans_fit` enqueues every round on the current stream and reads
nothing back; the per-round record is copied to the host only when `history` is read.  There is no CPU path.

Used for semantic de-duplication, as the coarse quantiser of the IVF index (`sonar_amd.index.IVFFlatIndex`, DESIGN.md 3.18;
`predict(x, k)` is its probe) and for codebooks over SONAR space.  Not here: k-means++ initialisation, splitting of large clusters to refill empty ones (an empty
cluster keeps its centroid), multi-GPU.

`KMeans` is ordinary (Euclidean) k-means on the rows as they are: the same update, a finalise that divides
by the member count, and the assignment as the biased top-1 `argmax_c (x . c - ||c||^2 / 2) = argmin_c ||x - c||^2`
(`smi_l2_kmeans_fit`).  SONAR embeddings are not unit vectors, and a product quantiser is an L2 object.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .xsim import (WIDE_MAX, check_count, normalize_rows, prepare_rows, topk_l2_prepared, topk_normalized,
                   topk_wide_normalized)

UNIT_ROWS = 64  # SMI_KMEANS_UNIT_ROWS: members one work unit of the update sums in registers


def init_rows(n: int, n_clusters: int, seed: int) -> torch.Tensor:
    """The row numbers of the initial centroids: K distinct rows from a seeded CPU permutation (int64 [K], on the host)."""
    if n_clusters > n:
        raise ValueError(f"n_clusters = {n_clusters} exceeds the {n} rows to initialise from; pass init= or fewer clusters")
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return torch.randperm(n, generator=g)[:n_clusters]


def _check_matrix(t, name: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: k-means runs on a HIP device only (no CPU path); move the embeddings to cuda")
    if t.dim() != 2:
        raise ValueError(f"{name} must be [rows, dim], got {t.dim()} dimension(s)")
    if t.shape[0] < 1:
        raise ValueError(f"{name} is empty")
    if t.shape[1] % 64:
        raise ValueError(f"{name}: dim = {t.shape[1]} must be a multiple of 64")


def _check_padded16(t, name: str, n, source: str) -> None:
    """The contiguous fp16 matrix `source` returns, whose first n rows are the data."""
    _check_matrix(t, name)
    if t.dtype != torch.float16 or not t.is_contiguous():
        raise ValueError(f"{name} must be the contiguous fp16 matrix {source} returns")
    if isinstance(n, bool) or not isinstance(n, int) or n < 1 or (n + 255) // 256 * 256 != t.shape[0]:
        raise ValueError(f"n = {n!r} does not match the {t.shape[0]} padded rows of {name}")


def _fit_workspace_bytes(lib, n: int, k: int, d: int) -> int:
    up16 = lambda b: (int(b) + 15) // 16 * 16  # noqa: E731
    return (up16(lib.smi_kmeans_workspace_bytes(n, k, d)) + up16(lib.smi_xsim_workspace_bytes(n, k, 1, d)) + up16(4 * n)
            + 3072)


class SphericalKMeans:
    """fit / step / predict; see the module text.  Attributes after `fit`: centroids (fp32 [K, d], the un-normalised
    means' direction: sum of the members), centroids_normalized (fp16 [K, d]), labels (int32 [n]), scores (fp32 [n], the
    cosine to the own centroid), counts (int32 [K], members at the last update), history."""

    def __init__(self, n_clusters: int, n_iter: int = 20, seed: int = 0):
        if isinstance(n_clusters, bool) or not isinstance(n_clusters, int) or n_clusters < 1:
            raise ValueError(f"n_clusters = {n_clusters!r}: at least one cluster")
        if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 0:
            raise ValueError(f"n_iter = {n_iter!r}: a non-negative number of rounds")
        self.n_clusters = n_clusters
        self.n_iter = n_iter
        self.seed = int(seed)
        self._fitted = False

    # ------------------------------------------------------------------------------------------------ fitting
    def fit(self, x: torch.Tensor, init: Optional[torch.Tensor] = None) -> "SphericalKMeans":
        """x: fp16 / fp32 [n, d] on the device.  init: None (K distinct rows of x by `init_rows(n, K, seed)`) or [K, d]."""
        _check_matrix(x, "x")
        self._check_init(init, x.shape[0], x.shape[1])
        start = init if init is not None else x[init_rows(x.shape[0], self.n_clusters, self.seed).to(x.device)]
        return self._fit(normalize_rows(x), x.shape[0], start)

    def fit_normalized(self, xn: torch.Tensor, n: int, init: Optional[torch.Tensor] = None) -> "SphericalKMeans":
        """As `fit`, on a matrix from `xsim.normalize_rows` (fp16, padded) whose first n rows are the data."""
        _check_padded16(xn, "xn", n, "normalize_rows")
        self._check_init(init, n, xn.shape[1])
        start = init if init is not None else xn[init_rows(n, self.n_clusters, self.seed).to(xn.device)]
        return self._fit(xn, n, start)

    def _check_init(self, init, n: int, d: int) -> None:
        if init is None:
            if self.n_clusters > n:
                init_rows(n, self.n_clusters, self.seed)  # raises
            return
        _check_matrix(init, "init")
        if tuple(init.shape) != (self.n_clusters, d):
            raise ValueError(f"init must be [{self.n_clusters}, {d}], got {list(init.shape)}")

    def _fit(self, xn: torch.Tensor, n: int, start: torch.Tensor) -> "SphericalKMeans":
        lib = _lib.load()
        dev, d, k = xn.device, xn.shape[1], self.n_clusters
        self._xn, self._n, self._d = xn, n, d
        self._c32 = start.to(device=dev, dtype=torch.float32).contiguous().clone()
        self._c16 = torch.empty((int(lib.smi_xsim_padded_rows(k)), d), dtype=torch.float16, device=dev)
        self.labels = torch.empty((n,), dtype=torch.int32, device=dev)
        self.scores = torch.empty((n,), dtype=torch.float32, device=dev)
        self._sums = torch.zeros((k, d), dtype=torch.int64, device=dev)
        self.counts = torch.zeros((k,), dtype=torch.int32, device=dev)
        self._ws = torch.empty(self._fit_ws_bytes(lib, n, k, d), dtype=torch.uint8, device=dev)
        cap = self.n_iter + 1
        self._objective = torch.zeros((cap,), dtype=torch.float64, device=dev)
        self._moved = torch.zeros((cap,), dtype=torch.int32, device=dev)
        self._empty = torch.zeros((cap,), dtype=torch.int32, device=dev)
        self._rounds = 0
        self._run(self.n_iter, resume=False)
        self._fitted = True
        return self

    _FIT = "smi_kmeans_fit"
    _fit_ws_bytes = staticmethod(_fit_workspace_bytes)

    def _fit_extra(self) -> tuple:
        """What the entry `_FIT` takes between the fp16 centroids and the labels."""
        return ()

    def _run(self, n_iter: int, resume: bool) -> None:
        lib = _lib.load()
        # records of this call start at: objective / moved [assignments so far], empty [rounds so far]
        a0 = self._rounds + 1 if resume else 0
        need = a0 + n_iter + (0 if resume else 1)
        if need > self._objective.shape[0]:
            grow = max(need, 2 * self._objective.shape[0]) - self._objective.shape[0]
            self._objective = torch.cat([self._objective, self._objective.new_zeros(grow)])
            self._moved = torch.cat([self._moved, self._moved.new_zeros(grow)])
            self._empty = torch.cat([self._empty, self._empty.new_zeros(grow)])
        with torch.cuda.device(self._xn.device):
            _lib.check(getattr(lib, self._FIT)(
                self._xn.data_ptr(), self._n, self._d, self.n_clusters, n_iter, int(resume), self._c32.data_ptr(),
                self._c16.data_ptr(), *self._fit_extra(), self.labels.data_ptr(), self.scores.data_ptr(),
                self._sums.data_ptr(), self.counts.data_ptr(), self._objective.data_ptr() + 8 * a0,
                self._moved.data_ptr() + 4 * a0, self._empty.data_ptr() + 4 * self._rounds, self._ws.data_ptr(),
                self._ws.numel(), _lib.current_stream_ptr()))
        self._rounds += n_iter

    def step(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """One more round on the fitted data: update -> finalise -> assign.  Returns that round's (labels, scores), the
        tensors `labels` / `scores` themselves.  `fit` with n_iter = T is `fit` with n_iter = 0 and T steps, bit for bit."""
        self._need_fit("step")
        self._run(1, resume=True)
        return self.labels, self.scores

    # ---------------------------------------------------------------------------------------------- after fit
    def _need_fit(self, what: str) -> None:
        if not self._fitted:
            raise RuntimeError(f"{what} before fit: there are no centroids yet")

    @property
    def centroids(self) -> torch.Tensor:
        self._need_fit("centroids")
        return self._c32

    @property
    def centroids_normalized(self) -> torch.Tensor:
        self._need_fit("centroids_normalized")
        return self._c16[: self.n_clusters]

    @property
    def sums(self) -> torch.Tensor:
        """int64 [K, d]: the exact member sums of the last update, in units of 2^-24."""
        self._need_fit("sums")
        return self._sums

    @property
    def history(self) -> Dict[str, List]:
        """objective (sum of the rows' cosines to their centroids) and moved (rows whose label changed; n at first) per
        assignment, rounds + 1 entries; empty (clusters that kept their centroid) per round.  Read back on access."""
        self._need_fit("history")
        r = self._rounds
        return {"objective": self._objective[: r + 1].tolist(), "moved": self._moved[: r + 1].tolist(),
                "empty": self._empty[:r].tolist()}

    def _check_predict(self, what: str, x, k, most: int = 8) -> None:
        check_count(k, "k", most)
        self._need_fit(what)
        _check_matrix(x, "x")
        if x.shape[1] != self._d:
            raise ValueError(f"x has dim {x.shape[1]}, the centroids {self._d}")

    def predict(self, x: torch.Tensor, k: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """The k (<= 8) nearest centroids of every row of x, best first: (labels int32, cosines fp32), [n] for k = 1 and
        [n, k] otherwise.  k > 1 is the probe of an IVF index."""
        self._check_predict("predict", x, k)
        score, idx = topk_normalized(normalize_rows(x), x.shape[0], self._c16, self.n_clusters, k)
        return (idx[:, 0], score[:, 0]) if k == 1 else (idx, score)

    def predict_wide(self, x: torch.Tensor, k: int = 16) -> Tuple[torch.Tensor, torch.Tensor]:
        """`predict` for k up to 64, always [n, k]: the paged top-k (`xsim.topk_wide_normalized`), one pass
        over the centroids per 16 results.  (labels -1, cosines -inf) where k exceeds the number of centroids."""
        self._check_predict("predict_wide", x, k, WIDE_MAX)
        score, idx = topk_wide_normalized(normalize_rows(x), x.shape[0], self._c16, self.n_clusters, k)
        return idx, score


class KMeans(SphericalKMeans):
    """Euclidean k-means with `SphericalKMeans`'s surface: fit / step / predict / centroids / history.  Attributes after
    `fit`: centroids (fp32 [K, d], the means of the members), centroids_f16 (their fp16 roundings, what rows are assigned
    against), centroid_half_norms (fp32 [K], ||c||^2 / 2 of the fp16 rows), labels (int32 [n]), scores (fp32 [n]: x . c - h_c
    against the own centroid, so ||x - c||^2 = 2 (h_x - score)), counts, history (with `inertia`)."""

    def fit(self, x: torch.Tensor, init: Optional[torch.Tensor] = None) -> "KMeans":
        """x: fp16 / fp32 [n, d] on the device, taken as it is (rounded to fp16, not normalised).  init: None (K distinct rows
        of x by `init_rows(n, K, seed)`) or [K, d]."""
        _check_matrix(x, "x")
        self._check_init(init, x.shape[0], x.shape[1])
        start = init if init is not None else x[init_rows(x.shape[0], self.n_clusters, self.seed).to(x.device)]
        x16, hx = prepare_rows(x)
        return self._fit_l2(x16, hx, x.shape[0], start)

    def fit_prepared(self, x16: torch.Tensor, half_norms: torch.Tensor, n: int, init: Optional[torch.Tensor] = None) -> "KMeans":
        """As `fit`, on what `xsim.prepare_rows` returned (fp16 rows padded to a multiple of 256, their half norms) for n rows."""
        _check_padded16(x16, "x16", n, "prepare_rows")
        if (not isinstance(half_norms, torch.Tensor) or half_norms.dtype != torch.float32 or half_norms.device != x16.device
                or tuple(half_norms.shape) != (x16.shape[0],)):
            raise ValueError(f"half_norms must be the fp32 [{x16.shape[0]}] vector prepare_rows returns, on the device of x16")
        self._check_init(init, n, x16.shape[1])
        start = init if init is not None else x16[init_rows(n, self.n_clusters, self.seed).to(x16.device)]
        return self._fit_l2(x16, half_norms, n, start)

    def fit_normalized(self, *args, **kwargs):
        raise TypeError("KMeans clusters rows as they are: use fit, or fit_prepared on what xsim.prepare_rows returns")

    def _fit_l2(self, x16: torch.Tensor, hx: torch.Tensor, n: int, start: torch.Tensor) -> "KMeans":
        lib = _lib.load()
        dev, d, k = x16.device, x16.shape[1], self.n_clusters
        self._hx = hx
        self._ch = torch.empty((int(lib.smi_xsim_padded_rows(k)),), dtype=torch.float32, device=dev)
        return self._fit(x16, n, start)  # the buffers, the records and the call of the spherical fit, on the entry below

    _FIT = "smi_l2_kmeans_fit"

    @staticmethod
    def _fit_ws_bytes(lib, n: int, k: int, d: int) -> int:
        return int(lib.smi_l2_kmeans_fit_ws_bytes(n, k, d))

    def _fit_extra(self) -> tuple:
        return (self._ch.data_ptr(),)

    @property
    def centroids_f16(self) -> torch.Tensor:
        self._need_fit("centroids_f16")
        return self._c16[: self.n_clusters]

    @property
    def centroid_half_norms(self) -> torch.Tensor:
        self._need_fit("centroid_half_norms")
        return self._ch[: self.n_clusters]

    @property
    def centroids_normalized(self) -> torch.Tensor:
        raise TypeError("KMeans keeps its centroids as they are: centroids (fp32) or centroids_f16")

    @property
    def history(self) -> Dict[str, List]:
        """`SphericalKMeans.history`, objective being the sum of the scores x . c - h_c, and inertia = the sum of the squared
        distances of the rows to their centroids, 2 (sum of the rows' half norms - objective), per assignment."""
        h = SphericalKMeans.history.fget(self)
        hx = float(self._hx[: self._n].double().sum().item())
        h["inertia"] = [2.0 * (hx - o) for o in h["objective"]]
        return h

    def predict(self, x: torch.Tensor, k: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """The k (<= 8) nearest centroids of every row of x, nearest first: (labels int32, squared distances fp32), [n] for
        k = 1 and [n, k] otherwise."""
        self._check_predict("predict", x, k)
        x16, hx = prepare_rows(x)
        dist, idx, _ = topk_l2_prepared(x16, x.shape[0], hx, self._c16, self.n_clusters, self._ch, k)
        return (idx[:, 0], dist[:, 0]) if k == 1 else (idx, dist)

    def predict_wide(self, *args, **kwargs):
        raise TypeError("predict_wide is the paged cosine top-k; KMeans.predict takes k <= 8")


def update(xn: torch.Tensor, labels: torch.Tensor, n_clusters: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """smi_kmeans_update: (sums int64 [K, d] in units of 2^-24, counts int32 [K]) of the rows of xn (fp16 [>= n, d]) under
    labels (int32 [n]); a row with a label outside [0, K) is skipped."""
    _check_matrix(xn, "xn")
    if xn.dtype != torch.float16 or not xn.is_contiguous():
        raise ValueError("xn must be a contiguous fp16 matrix")
    if not labels.is_cuda or labels.dtype != torch.int32 or labels.dim() != 1 or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous int32 vector on the device")
    n, d = labels.shape[0], xn.shape[1]
    if not 1 <= n <= xn.shape[0]:
        raise ValueError(f"{n} labels for {xn.shape[0]} rows")
    if isinstance(n_clusters, bool) or not isinstance(n_clusters, int) or n_clusters < 1:
        raise ValueError(f"n_clusters = {n_clusters!r}: at least one cluster")
    lib = _lib.load()
    ws_bytes = int(lib.smi_kmeans_workspace_bytes(n, n_clusters, d))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=xn.device)
    sums = torch.empty((n_clusters, d), dtype=torch.int64, device=xn.device)
    counts = torch.empty((n_clusters,), dtype=torch.int32, device=xn.device)
    with torch.cuda.device(xn.device):
        _lib.check(lib.smi_kmeans_update(xn.data_ptr(), labels.data_ptr(), n, d, n_clusters, sums.data_ptr(),
                                         counts.data_ptr(), ws.data_ptr(), ws_bytes, _lib.current_stream_ptr()))
    return sums, counts


def finalize(sums: torch.Tensor, counts: torch.Tensor, centroids: torch.Tensor,
             centroids_normalized: torch.Tensor) -> torch.Tensor:
    """smi_kmeans_finalize, in place: centroids (fp32 [K, d]) and centroids_normalized (fp16 [padded K, d]) take the rows of
    the clusters with members and a non-zero sum, the others keep theirs.  Returns the device int32 [1] count of those."""
    k, d = sums.shape
    pad = (k + 255) // 256 * 256
    if sums.dtype != torch.int64 or counts.dtype != torch.int32 or tuple(counts.shape) != (k,):
        raise ValueError("sums int64 [K, d] and counts int32 [K] as smi_kmeans_update returns them")
    if centroids.dtype != torch.float32 or tuple(centroids.shape) != (k, d) or not centroids.is_contiguous():
        raise ValueError(f"centroids must be contiguous fp32 [{k}, {d}]")
    if (centroids_normalized.dtype != torch.float16 or tuple(centroids_normalized.shape) != (pad, d)
            or not centroids_normalized.is_contiguous()):
        raise ValueError(f"centroids_normalized must be contiguous fp16 [{pad}, {d}]")
    lib = _lib.load()
    ws_bytes = int(lib.smi_kmeans_workspace_bytes(1, k, d))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=sums.device)
    empty = torch.empty((1,), dtype=torch.int32, device=sums.device)
    with torch.cuda.device(sums.device):
        _lib.check(lib.smi_kmeans_finalize(sums.contiguous().data_ptr(), counts.contiguous().data_ptr(), k, d,
                                           centroids.data_ptr(), centroids_normalized.data_ptr(), empty.data_ptr(),
                                           ws.data_ptr(), ws_bytes, _lib.current_stream_ptr()))
    return empty
