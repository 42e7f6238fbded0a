"""Semantic de-duplication of sentence embeddings on the MI355X engine: SemDeDup (Abbas et al. 2023) over
the lists of an `IVFFlatIndex`.

`self_join` is the kernel's entry: for every row, the best cosine against the rows of its own list that precede it in a keep
order (higher priority first, ties to the lower row number), and the id of that row.  It keeps no threshold: SemDeDup sweeps
eps over one stored `max_sim`, and so does `DedupResult.keep_at`.  `semdedup` is the recipe around it: cluster (or take a
filled index), order the rows of a cluster, self-join, threshold.  `keep = ~(max_sim > threshold)` is a strict comparison,
like mining's `threshold`.  Nothing here synchronises with the host or reads anything back.  There is no CPU path.

A row is compared with its own list only (as in SemDeDup): duplicates that the quantiser separates are not found.  A dropped
row still drops the rows it precedes (one pass, not greedy or transitive).  `IVFInt8Index` is refused.  The contract is
restated in numpy in tests/dedup_ref.py.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple, Union

import torch

from . import _lib
from .index import IVFFlatIndex, IVFInt8Index, LIST_ALIGN, _check_matrix, _check_table
from .xsim import normalize_rows, topk_normalized

PRIORITY_MODES = ("centroid", "-centroid")


def _check_priority(priority, n: int) -> None:
    if not isinstance(priority, torch.Tensor):
        raise TypeError("priority must be a torch.Tensor or None")
    if not priority.is_cuda:
        raise RuntimeError("priority: de-duplication runs on a HIP device only (no CPU path)")
    if priority.dtype != torch.float32 or tuple(priority.shape) != (n,):
        raise ValueError(f"priority must be float32 [{n}], got {priority.dtype} {list(priority.shape)}")


def self_join(rows: torch.Tensor, ids: torch.Tensor, offsets: torch.Tensor, n: int,
              priority: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """smi_ivf_dedup over the storage `index.build_lists` returned (rows fp16 [slots, d], ids int32 [slots], offsets int32
    [K + 1]); n = the number of original rows (ids lie in [0, n)); priority = None or device fp32 [n] by original row number.

    Returns (max_sim fp32 [n], nearest int32 [n]): the best score of row i against the rows of its list that precede it
    (priority higher, or equal and id lower) and that row's id; (-inf, -1) where none does or the row is in no list."""
    _check_matrix(rows, "rows")
    if rows.dtype != torch.float16 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous fp16 matrix")
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"n = {n!r}: at least one row")
    slots, d = rows.shape
    if slots % LIST_ALIGN:
        raise ValueError(f"rows has {slots} slots: a multiple of {LIST_ALIGN} is expected (the storage build_lists returns)")
    _check_table(ids, "ids", slots, None)
    if isinstance(offsets, torch.Tensor) and (offsets.dim() != 1 or offsets.shape[0] < 2):
        raise ValueError(f"offsets must be int32 [K + 1], got {list(offsets.shape)}")
    _check_table(offsets, "offsets", offsets.shape[0] if isinstance(offsets, torch.Tensor) else -1, None)
    if priority is not None:
        _check_priority(priority, n)
        priority = priority.contiguous()
    lib = _lib.load()
    n_lists, dev = offsets.shape[0] - 1, rows.device
    ws_bytes = int(lib.smi_ivf_dedup_workspace_bytes(slots, n, n_lists, d))
    if ws_bytes < 1:
        raise ValueError(f"{slots} slots, {n} rows, {n_lists} lists: slot, row and list numbers must fit int32")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    max_sim = torch.empty((n,), dtype=torch.float32, device=dev)
    nearest = torch.empty((n,), dtype=torch.int32, device=dev)
    ids, offsets = ids.contiguous(), offsets.contiguous()
    with torch.cuda.device(dev):
        _lib.check(lib.smi_ivf_dedup(rows.data_ptr(), ids.data_ptr(), offsets.data_ptr(), n_lists, slots, d,
                                     priority.data_ptr() if priority is not None else None, n, max_sim.data_ptr(),
                                     nearest.data_ptr(), ws.data_ptr(), ws_bytes, _lib.current_stream_ptr()))
    return max_sim, nearest


class DedupResult(NamedTuple):
    """keep bool [n] (False = a near-duplicate of a preceding row of its cluster), max_sim fp32 [n], nearest int32 [n] (what
    `self_join` returns), labels int32 [n] (the list of every row, -1 = in none)."""

    keep: torch.Tensor
    max_sim: torch.Tensor
    nearest: torch.Tensor
    labels: torch.Tensor

    def keep_at(self, threshold: float) -> torch.Tensor:
        """`keep` at another threshold, from the stored `max_sim`: no second scan."""
        return keep_mask(self.max_sim, threshold)


def keep_mask(max_sim: torch.Tensor, threshold: float) -> torch.Tensor:
    """~(max_sim > threshold): a row whose best preceding neighbour scores exactly the threshold is kept."""
    return ~(max_sim > threshold)


def _threshold(threshold, eps) -> float:
    if (threshold is None) == (eps is None):
        raise ValueError("give exactly one of threshold and eps (threshold = 1 - eps)")
    v = threshold if eps is None else eps
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{'threshold' if eps is None else 'eps'} = {v!r}: a number")
    return float(threshold) if eps is None else 1.0 - float(eps)


def _list_of_rows(index: IVFFlatIndex, n: int) -> torch.Tensor:
    """int32 [n]: the list every row is in (-1: in none), from the index's own ids and offsets; no read-back."""
    ids, offsets = index._ids, index._offsets
    slot = torch.arange(ids.shape[0], dtype=torch.int32, device=ids.device)
    lst = torch.searchsorted(offsets[1:].contiguous(), slot, right=True).to(torch.int32)
    labels = torch.full((n + 1,), -1, dtype=torch.int32, device=ids.device)
    where = torch.where((ids >= 0) & (ids < n), ids, torch.full_like(ids, n)).to(torch.int64)
    labels.scatter_(0, where, lst)  # pad and unused slots (id -1) land on the extra entry
    return labels[:n]


def semdedup(x: torch.Tensor, *, index: Optional[IVFFlatIndex] = None, n_lists: Optional[int] = None,
             threshold: Optional[float] = None, eps: Optional[float] = None,
             priority: Union[None, str, torch.Tensor] = None, n_iter: int = 10, seed: int = 0) -> DedupResult:
    """SemDeDup of the rows of x (fp16 / fp32 [n, d] on the device).

    index: a fitted and filled `IVFFlatIndex` whose ids are the row numbers of x; or None, and one is trained on x with
    `n_lists` clusters (`n_iter`, `seed`: the k-means) and filled.  Exactly one of `threshold` and `eps` (threshold =
    1 - eps).  priority: None (keep the first occurrence), an fp32 [n] tensor (higher is kept), "centroid" (SemDeDup's order:
    the cosine of a row to its nearest centroid, higher first) or "-centroid" (its negation: keep the hard examples)."""
    thr = _threshold(threshold, eps)
    if isinstance(priority, str) and priority not in PRIORITY_MODES:
        raise ValueError(f"priority = {priority!r}: one of {PRIORITY_MODES}, a tensor or None")
    if (index is None) == (n_lists is None):
        raise ValueError("give exactly one of index (a filled IVFFlatIndex) and n_lists (train one on x)")
    if isinstance(index, IVFInt8Index):
        raise TypeError("semdedup needs the fp16 lists of an IVFFlatIndex; an IVFInt8Index holds int8 codes")
    if index is not None and not isinstance(index, IVFFlatIndex):
        raise TypeError("index must be an IVFFlatIndex")
    _check_matrix(x, "x")
    n = x.shape[0]
    if priority is not None and not isinstance(priority, str):
        _check_priority(priority, n)
    if index is not None:
        index._need_add("semdedup")
        if x.shape[1] != index.dim:
            raise ValueError(f"x has dim {x.shape[1]}, the index {index.dim}")
    centroid_score = None
    if index is None:
        index = IVFFlatIndex.train(x, n_lists, n_iter=n_iter, seed=seed)
        score, label = topk_normalized(normalize_rows(x), n, index._c16, index._k, 1)
        index.add(x, labels=label[:, 0].contiguous())
        centroid_score = score[:, 0]
    elif isinstance(priority, str):
        centroid_score = topk_normalized(normalize_rows(x), n, index._c16, index._k, 1)[0][:, 0]
    if isinstance(priority, str):
        priority = (centroid_score if priority == "centroid" else -centroid_score).contiguous()
    max_sim, nearest = self_join(index._rows, index._ids, index._offsets, n, priority)
    return DedupResult(keep_mask(max_sim, thr), max_sim, nearest, _list_of_rows(index, n))
