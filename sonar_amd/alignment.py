"""Monotonic alignment of two documents that are translations of each other: dynamic time warping over the cosine
distances of their sentence embeddings, on the MI355X engine.

This is the application of the reference's `examples/bilingual_document.ipynb`, which embeds a novel and its translation
and runs `fastdtw(eng_embeddings, spa_embeddings, dist=cosine)`, because nearest-neighbour matching "does not maintain
monotonicity".  Mining (`sonar_amd.mining`) ignores order on purpose; this module keeps it.  Cost, DP, backtrack and path
output run in the library's kernels (`smi_dtw_align`, `smi_dtw_align_cost`) for a ragged batch of
document pairs in one call; there is no CPU path.

The result is fixed where fastdtw leaves it to its implementation: all arithmetic is fp32 with one rounding per cell,
`D[i][j] = min(D[i-1][j], D[i][j-1], D[i-1][j-1]) + c[i][j]`, and a tie goes to the first of up, left, diagonal.  This
is exact DTW (fastdtw's multiresolution approximation is not reproduced); `radius` is a Sakoe-Chiba band around the
diagonal instead.  The tie order is the one fastdtw's pure-Python `__dtw` is believed to use; it is NOT pinned to
fastdtw's output (tests/alignment_ref.py restates the contract, not the package).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from .xsim import normalize_rows

MAX_PAIRS = 65535   # per call of the library (smi_dtw_align); longer batches are cut into calls of this size


def _check_radius(radius) -> int:
    if radius is None:
        return 0
    if isinstance(radius, bool) or not isinstance(radius, int):
        raise ValueError(f"radius = {radius!r}: None / 0 for the full matrix or an integer >= 1")
    if radius < 0:
        raise ValueError(f"radius = {radius}: a band cannot be negative")
    return radius


def _check_offsets(offsets, rows: int, name: str) -> List[int]:
    offs = [int(v) for v in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
    if len(offs) < 2:
        raise ValueError(f"{name}: offsets are [n_pairs + 1] row numbers, got {len(offs)} entries")
    if offs[0] < 0 or any(b < a for a, b in zip(offs, offs[1:])):
        raise ValueError(f"{name}: offsets must be non-negative and non-decreasing")
    if offs[-1] > rows:
        raise ValueError(f"{name}: offsets end at row {offs[-1]} of {rows}")
    return offs


class DtwPlan:
    """Offsets, workspace and outputs of one batch of pairs; `run` / `run_cost` only launch (stream-ordered, no host
    read-back: they can be captured into a graph), `results` synchronises and cuts the outputs into per-pair results."""

    def __init__(self, x_offsets: Sequence[int], y_offsets: Sequence[int], device):
        if len(x_offsets) != len(y_offsets):
            raise ValueError("x_offsets and y_offsets must describe the same number of pairs")
        self.n = len(x_offsets) - 1
        if not 1 <= self.n <= MAX_PAIRS:
            raise ValueError(f"{self.n} pairs: one plan takes 1..{MAX_PAIRS}")
        self.xo, self.yo = list(x_offsets), list(y_offsets)
        lib = _lib.load()
        self.xo_host = (C.c_int64 * (self.n + 1))(*self.xo)
        self.yo_host = (C.c_int64 * (self.n + 1))(*self.yo)
        self.ws_bytes = int(lib.smi_dtw_workspace_bytes(self.n, self.xo_host, self.yo_host))
        if self.ws_bytes <= 0:   # the offsets are in order (checked by the callers): what is left is a pair's size
            raise ValueError("a pair is beyond what one workgroup takes: at most 2^31 - 1 cells and 2^30 rows a side")
        sizes = [(self.xo[b + 1] - self.xo[b], self.yo[b + 1] - self.yo[b]) for b in range(self.n)]
        self.path_offsets = [0]
        for nx, ny in sizes:
            self.path_offsets.append(self.path_offsets[-1] + (nx + ny - 1 if nx > 0 and ny > 0 else 0))
        self.cells = sum(nx * ny for nx, ny in sizes)
        self.device = device
        self.xo_dev = torch.tensor(self.xo, dtype=torch.int64, device=device)
        self.yo_dev = torch.tensor(self.yo, dtype=torch.int64, device=device)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.path = torch.zeros((max(self.path_offsets[-1], 1), 2), dtype=torch.int32, device=device)
        self.path_len = torch.zeros(self.n, dtype=torch.int32, device=device)
        self.distance = torch.zeros(self.n, dtype=torch.float32, device=device)

    def run_cost(self, cost: torch.Tensor, radius: int = 0) -> None:
        """cost: device fp32, the pairs' row-major [nx, ny] blocks one after the other."""
        if cost.dtype != torch.float32 or not cost.is_contiguous() or cost.numel() != self.cells:
            raise ValueError(f"cost must be {self.cells} contiguous fp32 values")
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().smi_dtw_align_cost(
                cost.data_ptr() if self.cells else self.ws.data_ptr(), self.n, self.xo_host, self.yo_host,
                self.xo_dev.data_ptr(), self.yo_dev.data_ptr(), radius, self.path.data_ptr(), self.path_len.data_ptr(),
                self.distance.data_ptr(), self.ws.data_ptr(), self.ws_bytes, _lib.current_stream_ptr()))

    def run(self, xn: torch.Tensor, yn: torch.Tensor, radius: int = 0) -> None:
        """xn / yn: matrices from normalize_rows that the offsets index."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().smi_dtw_align(
                xn.data_ptr(), yn.data_ptr(), xn.shape[1], self.n, self.xo_host, self.yo_host, self.xo_dev.data_ptr(),
                self.yo_dev.data_ptr(), radius, self.path.data_ptr(), self.path_len.data_ptr(), self.distance.data_ptr(),
                self.ws.data_ptr(), self.ws_bytes, _lib.current_stream_ptr()))

    def costs(self) -> torch.Tensor:
        """After `run`: the fp32 costs it computed, the pairs' row-major [nx, ny] blocks one after the other (a view of the
        workspace's last section)."""
        return self.ws[self.ws_bytes - 4 * self.cells:].view(torch.float32)

    def results(self) -> List[Tuple[torch.Tensor, float]]:
        lens, dist = self.path_len.tolist(), self.distance.tolist()
        path = self.path.long()
        return [(path[o:o + n].clone(), d) for o, n, d in zip(self.path_offsets, lens, dist)]


def _run_chunks(x_offsets: List[int], y_offsets: List[int], device, launch) -> List[Tuple[torch.Tensor, float]]:
    """launch(plan, number of its first pair) for every MAX_PAIRS pairs of the batch -> the results of all of them."""
    out = []
    for lo in range(0, len(x_offsets) - 1, MAX_PAIRS):
        hi = min(lo + MAX_PAIRS, len(x_offsets) - 1)
        plan = DtwPlan(x_offsets[lo:hi + 1], y_offsets[lo:hi + 1], device)
        launch(plan, lo)
        out += plan.results()
    return out


def dtw_from_cost(cost, radius: Optional[int] = None):
    """DTW over given cost matrices (smi_dtw_align_cost).  cost: one device tensor [nx, ny] -> (path int64 [L, 2],
    distance); a list of them -> a list of such results, computed in one call.  +inf marks a forbidden cell; a matrix with
    an empty side gives an empty path and distance +inf."""
    r = _check_radius(radius)
    single = isinstance(cost, torch.Tensor)
    costs = [cost] if single else list(cost)
    if not costs:
        raise ValueError("no cost matrix")
    for c in costs:
        if not isinstance(c, torch.Tensor) or c.dim() != 2:
            raise ValueError("a cost matrix is a 2-D tensor [nx, ny]")
    for c in costs:
        if not c.is_cuda:
            raise RuntimeError("alignment runs on a HIP device only (no CPU path); move the costs to cuda")
    xo, yo = [0], [0]
    for c in costs:
        xo.append(xo[-1] + c.shape[0])
        yo.append(yo[-1] + c.shape[1])
    dev = costs[0].device
    flat = [c.to(torch.float32).reshape(-1) for c in costs]

    def launch(plan, first):
        part = flat[first:first + plan.n]
        plan.run_cost(torch.cat(part) if len(part) > 1 else part[0].contiguous(), r)

    res = _run_chunks(xo, yo, dev, launch)
    return res[0] if single else res


def dtw_align(x: torch.Tensor, y: torch.Tensor, x_offsets=None, y_offsets=None, radius: Optional[int] = None):
    """Align the rows of x [N, d] with the rows of y [M, d] (sentence embeddings of a document and of its translation, fp16 /
    fp32 on the device) under c[i][j] = 1 - cos(x_i, y_j); a zero row costs 1 against everything.

    Without offsets: one pair -> (path int64 [L, 2] from (0, 0) to (N-1, M-1), distance).  With x_offsets / y_offsets
    ([n_pairs + 1] row numbers): pair b is x[x_offsets[b]:x_offsets[b+1]] against y[y_offsets[b]:y_offsets[b+1]] -> a list
    of such results with pair-local indices; a pair with an empty side gives an empty path and distance +inf.
    radius: None / 0 = exact DTW over the full matrix; r >= 1 = only cells with |i (ny-1) - j (nx-1)| <= r max(nx-1, ny-1, 1).
    """
    r = _check_radius(radius)
    if x.dim() != 2 or y.dim() != 2:
        raise ValueError("embeddings must be [rows, dim]")
    if x.shape[1] != y.shape[1]:
        raise ValueError("x and y must have the same dimension")
    if (x_offsets is None) != (y_offsets is None):
        raise ValueError("give both x_offsets and y_offsets, or neither")
    single = x_offsets is None
    xo = [0, x.shape[0]] if single else _check_offsets(x_offsets, x.shape[0], "x_offsets")
    yo = [0, y.shape[0]] if single else _check_offsets(y_offsets, y.shape[0], "y_offsets")
    if len(xo) != len(yo):
        raise ValueError("x_offsets and y_offsets must describe the same number of pairs")
    if not x.is_cuda or not y.is_cuda:
        raise RuntimeError("alignment runs on a HIP device only (no CPU path); move the embeddings to cuda")
    if x.shape[0] == 0 or y.shape[0] == 0:   # nothing to normalise: every pair has an empty side
        res = [(torch.empty((0, 2), dtype=torch.int64, device=x.device), math.inf) for _ in range(len(xo) - 1)]
        return res[0] if single else res
    xn, yn = normalize_rows(x), normalize_rows(y)
    res = _run_chunks(xo, yo, x.device, lambda plan, first: plan.run(xn, yn, r))
    return res[0] if single else res


def beads(path) -> List[Tuple[List[int], List[int]]]:
    """A path as the side-by-side table of the notebook: runs of (source indices, target indices) that belong together,
    1-1, 1-n (one source sentence against several target sentences) and n-1; a staircase through both gives an n-m run.
    A new run starts at every diagonal step."""
    cells = path.tolist() if isinstance(path, torch.Tensor) else [tuple(p) for p in path]
    out: List[Tuple[List[int], List[int]]] = []
    for i, j in cells:
        if out and (out[-1][0][-1] == i or out[-1][1][-1] == j):
            if out[-1][0][-1] != i:
                out[-1][0].append(i)
            if out[-1][1][-1] != j:
                out[-1][1].append(j)
        else:
            out.append(([i], [j]))
    return out
