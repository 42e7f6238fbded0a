"""IVF indexes over sentence embeddings on the MI355X engine: flat fp16 lists, int8 scalar-quantised
lists and product-quantised lists, plain or of residuals, under the cosine
or, for the flat and the product-quantised lists, the squared Euclidean distance.

Brute-force `xsim.topk` scores every query against every row.  An inverted-file index scores a query against the rows of the
`nprobe` nearest of K clusters only, about nprobe / K of the work, which is what repeated search of one corpus (LASER-style
mining, semantic de-duplication) wants.  The coarse quantiser is `clustering.SphericalKMeans`; the probe is `xsim.topk`
against its centroids (the mining kernel, unchanged); the lists are fp16 copies of the normalised rows, uncompressed
("flat"), so a returned score is the cosine `xsim.topk` would return, within the rounding of one fp32 accumulation.

`search` returns what `xsim.topk` returns -- (scores fp32 [nq, k], ids int32 [nq, k]), best first, score descending and
ties to the lower row number, (-inf, -1) where the probed lists hold fewer than k rows -- so `xsim.margin_select` and
`mining` consume it unchanged.  Its bits do not depend on the company of a query, on the order of the corpus or on the run.
There is no CPU path.

`IVFInt8Index` is the same index with one signed byte per element and one fp32 scale per row (per-row symmetric, amax / 127):
half the bytes, scanned with an integer MFMA whose sums are exact, so a score is specified down to its bits for any data
(tests/ivf_i8_ref.py).  Its raw scores are the quantised rows' dot products, within a derived bound of the cosine but not
the cosine; `search(..., refine=xn)` re-scores the k candidates against the fp16 corpus with `mining.pair_scores` and
re-orders them, which is what margin mining wants.  The quality was measured on synthetic planted data only; real SONAR
embeddings may have heavier-tailed rows, where a per-row scale loses more.

`IVFFlatIndex.self_join` and `sonar_amd.dedup` are the de-duplication over the flat lists.
`IVFFlatIndex.range_search` returns every row of the probed lists at or above a per-query threshold, not the k <= 8 best
(FAISS's `range_search`).

`ProductQuantizer` and `IVFPQIndex` are the same index over product-quantised rows: d / dsub bytes per row,
one byte per sub-quantiser of 256 codewords, 1/16 (dsub = 8) to 1/128 (dsub = 64) of the fp16 rows.  The scan decodes a
tile's codes into the flat scan's fp16 image once per tile, so a raw score is bit for bit the flat index's score against the
reconstructed row (tests/ivf_pq_ref.py); `search(..., refine=xn)` re-scores the candidates like the int8 index.  The quality
was measured on synthetic planted data only, whose noise is isotropic and does not compress; real SONAR rows are unmeasured.

`IVFPQResidualIndex` is `IVFPQIndex` with every row encoded as its residual against the centroid of its list (DESIGN.md 3.22,
FAISS's `by_residual`): the same bytes, a lower quantisation error, and one fp32 add per score -- the query's score against
the list's centroid, which the probe has already computed (tests/ivf_pq_residual_ref.py).

Filtered search (FAISS's `IDSelector`): `index.row_filter(keys=, mask=)` gives a `RowFilter`, and
`search(..., rows=, query_keys=, match=)` of all four classes and `IVFFlatIndex.range_search` count a candidate (query q, row i)
only where the row is visible (`mask[i]`, shared by all queries) and `keys[i] match query_keys[q]` holds, `match` one of
== != < <= > >= over signed int32 keys.  It happens inside the scan, so k results come back wherever k rows qualify: a
query's filtered result is, bit for bit, its unfiltered result over an index that holds only the rows it may see.  Recipes:
  a language-restricted search     keys = the rows' language numbers, query_keys = the wanted language, match "=="
  excluding the query itself       keys = arange(n), query_keys = the queries' own row numbers, match "!="  (k-NN of a corpus
                                   against its own index, where every query finds itself first)
  excluding the query's document   keys = document numbers, match "!="
  a cut-off date                   keys = dates, query_keys = the query's cut-off, match "<"
  rows to be ignored               mask = False for them: they stay in the lists and are scanned; `remove` takes them out

`PreTransformIndex` puts a learned linear transform (`sonar_amd.transforms`: a PCA that cuts the dimension, an OPQ rotation in
front of the sub-quantisers) in front of any of the four classes, FAISS's `IndexPreTransform`.

Wide search: `probe_wide` (every class) and `IVFFlatIndex.search_wide` take nprobe and k up to 64 --
the range real corpora are probed at -- as pages of 16 results: `search_page(..., below=)` returns the k <= 16 best rows of
the probed lists strictly after a per-query exclusive ceiling, and `search_wide` chains ceil(k / 16) of them, each page's
last entry the next one's ceiling.  The pages concatenated are the top-k bit for bit.  `search`, `probe` and every other
entry keep their limit of 8.

`IVFFlatL2Index` is the flat index under the squared Euclidean distance, on the rows as they are: the
quantiser is `clustering.KMeans`, every slot carries the bias -||row||^2 / 2 beside its id, and `search` returns (squared
distances ascending, ids).  SONAR embeddings are not unit vectors; this is FAISS's `METRIC_L2`.

`IVFPQL2Index` and `IVFPQResidualL2Index` are the product-quantised indexes under the squared Euclidean distance (DESIGN.md
3.30; FAISS's `IVFx,PQy` with `METRIC_L2`, the second with `by_residual`): a Euclidean `KMeans`, codebooks trained on the rows
as they are, and one fp32 bias per slot -- -1/2 ||y^||^2 of the decoded row, or -(c . r^ + 1/2 ||r^||^2) of the decoded residual
against its list's centroid (`pq_l2_bias`) -- that the scan adds to the PQ scan's sum (`search_lists_pq_l2`).  `search` returns
squared distances to the RECONSTRUCTED rows, ascending; `refine=prepare_rows(x)` re-scores the candidates against the fp16 rows.

The storage life-cycle, on every class: `add` fills an empty index once; `extend(x)` takes further rows
(`add(x1).extend(x2)` is the index `add(cat(x1, x2))` builds), `remove(ids= | mask=)` takes rows out, bytes and scan cost
included, and `merge_from(other)` takes over the rows of an index of the same class over the same quantiser.  All three run
one device operation, `regroup_lists` (smi_lists_regroup): the surviving slots and the new, already-encoded rows are regrouped
into fresh list-contiguous storage, so a call costs about one build of the union -- feed chunks, not rows.  A `RowFilter`
belongs to the storage it was made from: after any of the three, make a new one (an old one is refused).

Not here: L2 on the int8 lists (a scale AND a bias per slot) and in the wide, keyed and range searches, an OPQ fitted on rows that are not normalised, a look-up-table scan for a handful of queries, codes of fewer than 8 bits, lists of more than 16
results in one pass, k above 64, nprobe or k above 8 on the int8 / PQ / residual indexes, in `range_search` and in `mining`,
the key predicate on the wide search, de-duplication or range search over quantised lists, in-place growth with spare capacity per list (an `extend` that costs
O(new rows), not O(all rows), bytes), 64-bit ids, splitting of long lists, multi-GPU sharding; of filtering: skipping whole tiles or lists by key, per-query bitmaps or id lists, keys wider than
32 bits, more than one key per row, a filter on the coarse probe.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional, Tuple, Union

import torch

from . import _lib
from .clustering import KMeans, SphericalKMeans, init_rows
from .mining import pair_scores
from .xsim import (PAGE, WIDE_MAX, check_below, check_count, concat_pages, normalize_rows, prepare_rows, topk_bias_prepared,
                   topk_normalized, topk_wide_normalized)

LIST_ALIGN = 16    # SMI_IVF_LIST_ALIGN: every list starts at a multiple of this many slots and is padded to it
UNIT_QUERIES = 64  # SMI_IVF_UNIT_QUERIES: queries of one list that one work unit of the scan takes (128 when nq nprobe >= 256 K)
INT8_MAX_DIM = 131072  # SMI_IVF_I8_MAX_DIM: above it the int32 sum of int8 products could overflow
PQ_CODEWORDS = 256  # codewords of every sub-quantiser: a code is one byte
PQ_DSUBS = (8, 16, 32, 64)  # dimensions per sub-quantiser
# the relations of a key predicate as the C ABI's `accept`: a 3-bit mask over the outcome of one signed compare of the row's key
# with the query's, bit 0 less, bit 1 equal, bit 2 greater (0: nothing passes, 7: everything)
MATCH_ACCEPT = {"==": 2, "!=": 5, "<": 1, "<=": 3, ">": 4, ">=": 6}
ID_MAX = 0x7FFFFF00  # 2^31 - 256: the largest row count, and so one more than the largest row id, of every entry


def _check_device_tensor(t, name: str, hint: str = "") -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the index runs on a HIP device only (no CPU path){hint}")


def _check_matrix(t, name: str) -> None:
    _check_device_tensor(t, name, "; move the embeddings to cuda")
    if t.dim() != 2:
        raise ValueError(f"{name} must be [rows, dim], got {t.dim()} dimension(s)")
    if t.shape[0] < 1:
        raise ValueError(f"{name} is empty")
    if t.shape[1] % 64:
        raise ValueError(f"{name}: dim = {t.shape[1]} must be a multiple of 64")


def _check_table(t, name: str, rows: int, cols: Optional[int]) -> None:
    """A device int32 vector [rows] (cols None) or matrix [rows, cols]."""
    _check_device_tensor(t, name)
    shape = (rows,) if cols is None else (rows, cols)
    if t.dtype != torch.int32 or tuple(t.shape) != shape:
        raise ValueError(f"{name} must be int32 {list(shape)}, got {t.dtype} {list(t.shape)}")


def _check_small(v, name: str) -> None:
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 8:
        raise ValueError(f"{name} = {v!r}: an integer in [1, 8]")


def _check_rows16(xn, name: str, n=None) -> int:
    """A contiguous fp16 device matrix; returns n, the rows of it a call takes (None: all)."""
    _check_matrix(xn, name)
    if xn.dtype != torch.float16 or not xn.is_contiguous():
        raise ValueError(f"{name} must be a contiguous fp16 matrix")
    n = xn.shape[0] if n is None else n
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= xn.shape[0]:
        raise ValueError(f"n = {n!r}: between 1 and the {xn.shape[0]} rows of {name}")
    return n


def _check_build_args(xn, labels, n_lists) -> None:
    _check_rows16(xn, "xn")
    if isinstance(n_lists, bool) or not isinstance(n_lists, int) or n_lists < 1:
        raise ValueError(f"n_lists = {n_lists!r}: at least one list")
    if isinstance(labels, torch.Tensor) and labels.dim() == 1 and not 1 <= labels.shape[0] <= xn.shape[0]:
        raise ValueError(f"{labels.shape[0]} labels for {xn.shape[0]} rows")
    _check_table(labels, "labels", labels.shape[0] if isinstance(labels, torch.Tensor) and labels.dim() == 1 else -1, None)


def _check_int8_dim(d: int) -> None:
    if d > INT8_MAX_DIM:
        raise ValueError(f"dim = {d} exceeds {INT8_MAX_DIM}: the int32 sum of int8 products could overflow")


def _build(entry: str, sizing: str, xn, labels, n_lists: int, extras, storage, dsub=()):
    """A build entry of the C ABI and its sizing call, both by name; the arguments were checked by the caller.  The four
    signatures are `head + extras + storage + tail`: extras are the kind's own arguments behind the list count, storage names
    the row tensors it fills as (dtype, trailing shape); dsub: what the sizing call takes behind d.  Returns (row storage ...,
    ids, offsets, sizes)."""
    lib = _lib.load()
    n, d, dev = labels.shape[0], xn.shape[1], xn.device
    cap = int(lib.smi_ivf_slots_bound(n, n_lists))
    if cap < 1:
        raise ValueError(f"{n} rows over {n_lists} lists: slot numbers must fit int32")
    rows = [torch.empty((cap, *shape), dtype=dtype, device=dev) for dtype, shape in storage]
    ids = torch.empty((cap,), dtype=torch.int32, device=dev)
    offsets = torch.empty((n_lists + 1,), dtype=torch.int32, device=dev)
    sizes = torch.empty((n_lists,), dtype=torch.int32, device=dev)
    ws_bytes = int(getattr(lib, sizing)(n, n_lists, d, *dsub))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    labels = labels.contiguous()
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, entry)(xn.data_ptr(), labels.data_ptr(), n, d, n_lists, *extras, *(t.data_ptr() for t in rows),
                                       ids.data_ptr(), cap, offsets.data_ptr(), sizes.data_ptr(), ws.data_ptr(), ws_bytes,
                                       _lib.current_stream_ptr()))
    return (*rows, ids, offsets, sizes)


def _check_search_args(qn, probes, k) -> None:
    _check_small(k, "k")
    _check_rows16(qn, "qn")
    if isinstance(probes, torch.Tensor) and (probes.dim() != 2 or not 1 <= probes.shape[1] <= 8
                                             or not 1 <= probes.shape[0] <= qn.shape[0]):
        raise ValueError(f"probes must be [nq, 1..8] with nq <= {qn.shape[0]} rows, got {list(probes.shape)}")
    _check_table(probes, "probes", *(probes.shape if isinstance(probes, torch.Tensor) else (-1, 1)))


class RowFilter(NamedTuple):
    """Which rows of an index's lists count, in slot order (`row_filter`): ids int32 [slots], the row of every
    slot or -1 where it is masked out (or holds none), and keys int32 [slots] or None, the rows' keys.  Reusable across calls;
    not part of `state_dict`; tied to the storage it was made from by its length and by `generation`, the number of
    `extend` / `remove` / `merge_from` calls the index had seen when `row_filter` made it (0: none)."""

    ids: torch.Tensor
    keys: Optional[torch.Tensor]
    generation: int = 0


def slot_filter(ids: torch.Tensor, offsets: torch.Tensor, keys: Optional[torch.Tensor] = None,
                mask: Optional[torch.Tensor] = None) -> RowFilter:
    """smi_slot_filter: the row filter of the storage (ids int32 [slots], offsets int32 [K + 1]) a `build_lists*` returned.
    keys: device int32 [n], one key per row, or None; mask: device bool [n], True = visible, or None; at least one of them.
    A row whose id is not below the length of a given tensor (the shorter, where both are given) is left out.  One small
    gather kernel, enqueued; nothing is read back."""
    if keys is None and mask is None:
        raise ValueError("row_filter: give keys, mask or both")
    for t, name, dtype in ((keys, "keys", torch.int32), (mask, "mask", torch.bool)):
        if t is not None:
            _check_device_tensor(t, name)
            if t.dtype != dtype or t.dim() != 1 or t.shape[0] < 1:
                raise ValueError(f"{name} must be {str(dtype).replace('torch.', '')} [n], got {t.dtype} {list(t.shape)}")
    n = min(t.shape[0] for t in (keys, mask) if t is not None)
    lib = _lib.load()
    slots = ids.shape[0]
    out_ids = torch.empty((slots,), dtype=torch.int32, device=ids.device)
    out_keys = None if keys is None else torch.empty((slots,), dtype=torch.int32, device=ids.device)
    keys = None if keys is None else keys.contiguous()
    mask = None if mask is None else mask.contiguous()
    with torch.cuda.device(ids.device):
        _lib.check(lib.smi_slot_filter(ids.data_ptr(), offsets.data_ptr(), offsets.shape[0] - 1,
                                       None if keys is None else keys.data_ptr(), None if mask is None else mask.data_ptr(), n,
                                       out_ids.data_ptr(), None if out_keys is None else out_keys.data_ptr(), slots,
                                       _lib.current_stream_ptr()))
    return RowFilter(out_ids, out_keys)


def _check_keyed(slot_keys, query_keys, accept, slots: int, nq: int):
    """The optional trailing arguments of the list functions: () without them, else the three a `_keyed` entry takes behind
    its twin's (the tensors themselves, to be held until the call is enqueued)."""
    if slot_keys is None and query_keys is None and accept is None:
        return ()
    if slot_keys is None or query_keys is None or accept is None:
        raise ValueError("slot_keys, query_keys and accept go together: all three, or none")
    if isinstance(accept, bool) or not isinstance(accept, int) or not 0 <= accept <= 7:
        raise ValueError(f"accept = {accept!r}: a 3-bit mask in [0, 7] (bit 0 less, bit 1 equal, bit 2 greater)")
    _check_table(slot_keys, "slot_keys", slots, None)
    _check_table(query_keys, "query_keys", nq, None)
    return (slot_keys.contiguous(), query_keys.contiguous(), accept)


def _keyed_args(keyed):
    return (keyed[0].data_ptr(), keyed[1].data_ptr(), keyed[2]) if keyed else ()


def _search(entry: str, sizing: str, qn, probes, k: int, extras, storage, ids, offsets, dsub=(), keyed=(), last=()):
    """A search entry of the C ABI and its sizing call, as in `_build`: `head + extras + nprobe + storage + tail`, storage the
    arguments that describe the lists (pointers of tensors the caller holds).  keyed: `_check_keyed`'s result; with it the
    entry is its `_keyed` twin.  last: what the entry takes behind the stream (the ceilings of a page).  Returns (scores,
    ids)."""
    lib = _lib.load()
    (nq, nprobe), d, n_lists = probes.shape, qn.shape[1], offsets.shape[0] - 1
    if keyed:
        entry += "_keyed"
    ws_bytes = int(getattr(lib, sizing)(nq, n_lists, nprobe, k, d, *dsub))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=qn.device)
    idx = torch.empty((nq, k), dtype=torch.int32, device=qn.device)
    score = torch.empty((nq, k), dtype=torch.float32, device=qn.device)
    probes = probes.contiguous()
    with torch.cuda.device(qn.device):
        _lib.check(getattr(lib, entry)(qn.data_ptr(), nq, d, probes.data_ptr(), *extras, nprobe, *storage, ids.data_ptr(),
                                       offsets.data_ptr(), n_lists, k, idx.data_ptr(), score.data_ptr(), ws.data_ptr(), ws_bytes,
                                       _lib.current_stream_ptr(), *_keyed_args(keyed), *last))
    return score, idx


def _check_lists_dim(qn, rows) -> None:
    if rows.shape[1] != qn.shape[1]:
        raise ValueError(f"qn has dim {qn.shape[1]}, the lists {rows.shape[1]}")


def build_lists(xn: torch.Tensor, labels: torch.Tensor, n_lists: int):
    """smi_ivf_build: the inverted lists of the first len(labels) rows of xn (contiguous fp16 [>= n, d]) under labels (device
    int32 [n]; a label outside [0, n_lists) leaves the row out).  Returns (rows fp16 [slots, d], ids int32 [slots], offsets
    int32 [n_lists + 1], sizes int32 [n_lists]) with slots = smi_ivf_slots_bound(n, n_lists): the host has not seen the
    labels, so the storage is sized for any labelling.  Slots from offsets[n_lists] on are unused (ids -1, rows unwritten)."""
    _check_build_args(xn, labels, n_lists)
    return _build("smi_ivf_build", "smi_ivf_build_workspace_bytes", xn, labels, n_lists, (), [(torch.float16, xn.shape[1:])])


def _check_regroup_side(side, name: str, rows_like, want_aux):
    """One side of `regroup_lists`: (rows, aux, third, fourth) -> the four tensors, contiguous; rows_like / want_aux: the rows
    and whether there is an aux vector on the side checked before (None: this is the first)."""
    if not isinstance(side, (tuple, list)) or len(side) != 4:
        raise TypeError(f"{name} must be None or a tuple of four: rows, aux or None, and its two int32 vectors")
    rows, aux = side[0], side[1]
    _check_device_tensor(rows, f"{name} rows")
    if rows.dim() != 2 or rows.shape[1] < 1 or not rows.is_contiguous():
        raise ValueError(f"{name} rows must be a contiguous [slots, width] matrix, got {list(rows.shape)}")
    if rows_like is not None and (rows.dtype != rows_like.dtype or rows.shape[1] != rows_like.shape[1]
                                  or rows.device != rows_like.device):
        raise ValueError(f"{name} rows are {rows.dtype} [., {rows.shape[1]}] on {rows.device}, the old rows "
                         f"{rows_like.dtype} [., {rows_like.shape[1]}] on {rows_like.device}")
    if want_aux is not None and (aux is not None) != want_aux:
        raise ValueError("aux goes with both sides or with neither: the storage holds one value per slot, or none")
    if aux is not None:
        _check_device_tensor(aux, f"{name} aux")
        if aux.dtype != torch.float32 or aux.dim() != 1 or not aux.is_contiguous():
            raise ValueError(f"{name} aux must be contiguous fp32 [slots], got {aux.dtype} {list(aux.shape)}")
    return rows, aux, side[2], side[3]


def regroup_lists(n_lists: int, old=None, new=None, old_rows_bound: Optional[int] = None, new_id_base: int = 0,
                  capacity: Optional[int] = None):
    """smi_lists_regroup: fresh list-contiguous storage from the surviving slots of a filled storage and a set
    of new rows that are already encoded.  What `extend`, `remove` and `merge_from` of every index class run on.

    old: None, or (rows [slots, w], aux fp32 [slots] or None, ids int32 [slots], offsets int32 [n_lists + 1]) as a
         `build_lists*` or an earlier regroup returned them; a slot survives iff its id is >= 0, so ids may be a `RowFilter`'s.
    new: None, or (rows [>= n, w], aux fp32 [>= n] or None, labels int32 [n], ids int32 [n] or None): row i goes to list
         labels[i] (outside [0, n_lists): left out) with the id ids[i] (below 0: left out), or new_id_base + i without ids.
    rows are of any dtype, the same on both sides: fp16 rows, int8 or uint8 codes.  old_rows_bound: an upper bound on the
    survivors (default: the old slots).  capacity: the slots of the result, at least (and by default)
    smi_ivf_slots_bound(old_rows_bound + n, n_lists).  Returns (rows, aux or None, ids, offsets, sizes) in `build_lists`'s
    layout: pad slots are zero with aux 0 and id -1.  Enqueued on the current stream; nothing is read back."""
    if isinstance(n_lists, bool) or not isinstance(n_lists, int) or n_lists < 1:
        raise ValueError(f"n_lists = {n_lists!r}: at least one list")
    if old is None and new is None:
        raise ValueError("regroup_lists: give old, new or both")
    rows_like = want_aux = None
    old_slots = n_new = 0
    o_rows = o_aux = o_ids = o_off = n_rows = n_aux = n_labels = n_ids = None
    if old is not None:
        o_rows, o_aux, o_ids, o_off = _check_regroup_side(old, "old", None, None)
        old_slots = o_rows.shape[0]
        _check_table(o_ids, "old ids", old_slots, None)
        _check_table(o_off, "old offsets", n_lists + 1, None)
        if o_aux is not None and o_aux.shape[0] != old_slots:
            raise ValueError(f"old aux has {o_aux.shape[0]} entries for {old_slots} slots")
        o_ids, o_off = o_ids.contiguous(), o_off.contiguous()
        rows_like, want_aux = o_rows, o_aux is not None
    if new is not None:
        n_rows, n_aux, n_labels, n_ids = _check_regroup_side(new, "new", rows_like, want_aux)
        _check_table(n_labels, "labels", n_labels.shape[0] if isinstance(n_labels, torch.Tensor) and n_labels.dim() == 1 else -1,
                     None)
        n_new = n_labels.shape[0]
        if n_new > n_rows.shape[0] or (n_aux is not None and n_new > n_aux.shape[0]):
            raise ValueError(f"{n_new} labels for {n_rows.shape[0]} new rows")
        if n_ids is not None:
            _check_table(n_ids, "new ids", n_new, None)
            n_ids = n_ids.contiguous()
        n_labels = n_labels.contiguous()
        rows_like, want_aux = n_rows, n_aux is not None
    if old_slots + n_new < 1:
        raise ValueError("regroup_lists: no old slots and no new rows")
    if old_rows_bound is None:
        old_rows_bound = old_slots
    if isinstance(old_rows_bound, bool) or not isinstance(old_rows_bound, int) or not 0 <= old_rows_bound <= old_slots:
        raise ValueError(f"old_rows_bound = {old_rows_bound!r}: between 0 and the {old_slots} old slots")
    if isinstance(new_id_base, bool) or not isinstance(new_id_base, int) or new_id_base < 0 or new_id_base + n_new > ID_MAX:
        raise ValueError(f"new_id_base = {new_id_base!r} with {n_new} new rows: row ids must lie in [0, {ID_MAX}]")
    lib = _lib.load()
    need = int(lib.smi_ivf_slots_bound(old_rows_bound + n_new, n_lists)) if old_rows_bound + n_new else 0
    ws_bytes = int(lib.smi_lists_regroup_ws_bytes(old_slots, n_new, n_lists))
    if (old_rows_bound + n_new and need < 1) or ws_bytes < 1:
        raise ValueError(f"{old_slots} slots and {n_new} rows over {n_lists} lists: slot numbers must fit int32")
    if capacity is None:
        capacity = max(need, LIST_ALIGN)
    if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < max(need, 1):
        raise ValueError(f"capacity = {capacity!r}: at least smi_ivf_slots_bound({old_rows_bound + n_new}, {n_lists}) = {need}")
    dev, width = rows_like.device, rows_like.shape[1]
    rows = torch.empty((capacity, width), dtype=rows_like.dtype, device=dev)
    aux = torch.empty((capacity,), dtype=torch.float32, device=dev) if want_aux else None
    ids = torch.empty((capacity,), dtype=torch.int32, device=dev)
    offsets = torch.empty((n_lists + 1,), dtype=torch.int32, device=dev)
    sizes = torch.empty((n_lists,), dtype=torch.int32, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(lib.smi_lists_regroup(ptr(o_rows), ptr(o_aux), ptr(o_ids), ptr(o_off), old_slots, old_rows_bound, ptr(n_rows),
                                       ptr(n_aux), ptr(n_labels), ptr(n_ids), new_id_base, n_new, width * rows_like.element_size(),
                                       n_lists, rows.data_ptr(), ptr(aux), ids.data_ptr(), capacity, offsets.data_ptr(),
                                       sizes.data_ptr(), ws.data_ptr(), ws_bytes, _lib.current_stream_ptr()))
    return rows, aux, ids, offsets, sizes


def search_lists(qn: torch.Tensor, probes: torch.Tensor, rows: torch.Tensor, ids: torch.Tensor, offsets: torch.Tensor,
                 k: int = 1, slot_keys: Optional[torch.Tensor] = None, query_keys: Optional[torch.Tensor] = None,
                 accept: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """smi_ivf_search: the k best rows of the lists probes (device int32 [nq, 1..8]) names, for the first nq rows of qn
    (contiguous fp16 [>= nq, d]) against the storage `build_lists` returned: (scores fp32 [nq, k], ids int32 [nq, k]).

    slot_keys (device int32 [slots]), query_keys (device int32 [nq]) and accept (`MATCH_ACCEPT`, or any mask in [0, 7]), all
    three or none: smi_ivf_search_keyed, where a row counts only if its key passes against the query's.
    ids may be a `RowFilter`'s: a slot whose id is -1 never counts.  The other `search_lists_*` take the same three."""
    _check_search_args(qn, probes, k)
    _check_lists_dim(qn, rows)
    keyed = _check_keyed(slot_keys, query_keys, accept, ids.shape[0], probes.shape[0])
    return _search("smi_ivf_search", "smi_ivf_search_workspace_bytes", qn, probes, k, (), (rows.data_ptr(),), ids, offsets,
                   keyed=keyed)


def slot_bias(ids: torch.Tensor, half_norms: torch.Tensor) -> torch.Tensor:
    """smi_l2_slot_bias: fp32 [slots], -half_norms[id] for the row every slot holds and 0 where it holds none.
    ids: int32 [slots] from `build_lists`; half_norms: fp32 [>= n] from `xsim.prepare_rows` (row number = id)."""
    _check_table(ids, "ids", ids.shape[0] if isinstance(ids, torch.Tensor) and ids.dim() == 1 else -1, None)
    _check_device_tensor(half_norms, "half_norms")
    if half_norms.dtype != torch.float32 or half_norms.dim() != 1 or half_norms.device != ids.device:
        raise ValueError(f"half_norms must be fp32 [n] on the device of ids, got {half_norms.dtype} {list(half_norms.shape)}")
    lib = _lib.load()
    out = torch.empty((ids.shape[0],), dtype=torch.float32, device=ids.device)
    ids, half_norms = ids.contiguous(), half_norms.contiguous()
    with torch.cuda.device(ids.device):
        _lib.check(lib.smi_l2_slot_bias(ids.data_ptr(), ids.shape[0], half_norms.data_ptr(), out.data_ptr(),
                                        _lib.current_stream_ptr()))
    return out


def search_lists_l2(q16: torch.Tensor, probes: torch.Tensor, rows: torch.Tensor, bias: torch.Tensor, ids: torch.Tensor,
                    offsets: torch.Tensor, k: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """smi_l2_flat_search: `search_lists` with score = sum + bias[slot] (bias: `slot_bias` of the storage, fp32 [slots]) over
    prepared rows (`xsim.prepare_rows`): (scores fp32 [nq, k] best first, ids int32 [nq, k]).  With the bias of `slot_bias`,
    ||q - row||^2 = 2 (h_q - score).  ids may be a `RowFilter`'s."""
    _check_search_args(q16, probes, k)
    _check_lists_dim(q16, rows)
    _check_device_tensor(bias, "bias")
    if bias.dtype != torch.float32 or tuple(bias.shape) != (ids.shape[0],) or not bias.is_contiguous():
        raise ValueError(f"bias must be contiguous fp32 [{ids.shape[0]}], got {bias.dtype} {list(bias.shape)}")
    return _search("smi_l2_flat_search", "smi_l2_flat_search_ws_bytes", q16, probes, k, (), (rows.data_ptr(), bias.data_ptr()),
                   ids, offsets)


def search_lists_page(qn: torch.Tensor, probes: torch.Tensor, rows: torch.Tensor, ids: torch.Tensor, offsets: torch.Tensor,
                      k: int = PAGE, below=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """smi_ivf_search_page: `search_lists` for k <= 16 and probes int32 [nq, 1..64], and with below =
    (scores fp32 [nq], ids int32 [nq]) the k best rows of the probed lists strictly AFTER each query's exclusive ceiling
    in the total order (score descending, ties to the lower id) -- one ceiling per query, over all its lists.  A query
    whose ceiling id is negative is exhausted: only fill.  ids may be a `RowFilter`'s.  Nothing is read back."""
    check_count(k, "k", PAGE)
    _check_rows16(qn, "qn")
    if isinstance(probes, torch.Tensor) and (probes.dim() != 2 or not 1 <= probes.shape[1] <= WIDE_MAX
                                             or not 1 <= probes.shape[0] <= qn.shape[0]):
        raise ValueError(f"probes must be [nq, 1..{WIDE_MAX}] with nq <= {qn.shape[0]} rows, got {list(probes.shape)}")
    _check_table(probes, "probes", *(probes.shape if isinstance(probes, torch.Tensor) else (-1, 1)))
    _check_lists_dim(qn, rows)
    below = check_below(below, probes.shape[0], qn)
    ceil = (C.cast(below[0].data_ptr(), C.POINTER(C.c_float)), C.cast(below[1].data_ptr(), C.POINTER(C.c_int32))) \
        if below else (None, None)
    return _search("smi_ivf_search_page", "smi_ivf_search_page_ws_bytes", qn, probes, k, (), (rows.data_ptr(),), ids, offsets,
                   last=ceil)


class RangeResult(NamedTuple):
    """What a range search returns, in FAISS's layout: the hits of query q are the entries lims[q] .. lims[q + 1] of scores
    and ids.  lims int64 [nq + 1], scores fp32 [total], ids int32 [total], all on the device."""

    lims: torch.Tensor
    scores: torch.Tensor
    ids: torch.Tensor

    @property
    def counts(self) -> torch.Tensor:
        """int64 [nq]: the hits of every query."""
        return self.lims[1:] - self.lims[:-1]


def _check_thresholds(threshold, nq: int, like: torch.Tensor) -> torch.Tensor:
    """The thresholds of a range search as a device fp32 [nq] tensor: a Python float (NaN refused) for every query, or such
    a tensor."""
    if isinstance(threshold, (int, float)) and not isinstance(threshold, bool):
        if threshold != threshold:
            raise ValueError("threshold is NaN: no score compares to it")
        return torch.full((nq,), float(threshold), dtype=torch.float32, device=like.device)
    _check_device_tensor(threshold, "threshold")
    if threshold.dtype != torch.float32 or tuple(threshold.shape) != (nq,):
        raise ValueError(f"threshold must be a float or fp32 [{nq}], got {threshold.dtype} {list(threshold.shape)}")
    return threshold.contiguous()


def _check_max_total(max_total) -> None:
    if max_total is not None and (isinstance(max_total, bool) or not isinstance(max_total, int) or max_total < 0):
        raise ValueError(f"max_total = {max_total!r}: None or a non-negative integer")


def range_search_lists(qn: torch.Tensor, probes: torch.Tensor, thresholds: Union[float, torch.Tensor], rows: torch.Tensor,
                       ids: torch.Tensor, offsets: torch.Tensor, sort: bool = True, max_total: Optional[int] = None,
                       slot_keys: Optional[torch.Tensor] = None, query_keys: Optional[torch.Tensor] = None,
                       accept: Optional[int] = None) -> RangeResult:
    """smi_range_search_count / smi_range_search_emit: every row of the lists probes (device int32 [nq, 1..8]) names whose
    score against query q is >= thresholds[q] (device fp32 [nq], or one Python float for all; an fp32 compare, so NaN hits
    nothing and -inf everything probed), for the first nq rows of qn against the storage `build_lists` returned.  A score
    has the bits `search_lists` returns for the same two rows.

    Two walks of the lists, count and emit, with `torch.cumsum` of the pair counts between them and ONE READ-BACK, of the
    total, to size the output: the call synchronises with the host and cannot be captured in a graph.  max_total: raise
    (ValueError, the total named) instead of allocating more than this many hits.

    sort: every query's segment in `xsim.topk`'s total order, score descending and ties to the lower id (three stable
    `torch.sort`s); the result then has the same bits whatever the batch or the run.  sort=False leaves the order inside a
    segment unspecified (it differs from run to run).

    slot_keys, query_keys, accept: as for `search_lists`; the `_keyed` twins of both entries."""
    _check_search_args(qn, probes, 1)
    _check_lists_dim(qn, rows)
    _check_max_total(max_total)
    keyed = _check_keyed(slot_keys, query_keys, accept, ids.shape[0], probes.shape[0])
    (nq, nprobe), d, n_lists, dev = probes.shape, qn.shape[1], offsets.shape[0] - 1, qn.device
    thresholds = _check_thresholds(thresholds, nq, qn)
    lib = _lib.load()
    ws_bytes = int(lib.smi_range_search_ws_bytes(nq, n_lists, nprobe, d))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    pair_counts = torch.empty((nq * nprobe,), dtype=torch.int32, device=dev)
    probes = probes.contiguous()
    inputs = (qn.data_ptr(), nq, d, probes.data_ptr(), nprobe, thresholds.data_ptr(), rows.data_ptr(), ids.data_ptr(),
              offsets.data_ptr(), n_lists)
    count, emit = (getattr(lib, name + ("_keyed" if keyed else "")) for name in ("smi_range_search_count", "smi_range_search_emit"))
    keys = _keyed_args(keyed)
    with torch.cuda.device(dev):
        _lib.check(count(*inputs, pair_counts.data_ptr(), ws.data_ptr(), ws_bytes, _lib.current_stream_ptr(), *keys))
        base = torch.zeros((nq * nprobe + 1,), dtype=torch.int64, device=dev)
        torch.cumsum(pair_counts, 0, dtype=torch.int64, out=base[1:])
        total = int(base[-1].item())  # the read-back
        if max_total is not None and total > max_total:
            raise ValueError(f"the range search has {total} hits, max_total = {max_total}")
        score = torch.empty((total,), dtype=torch.float32, device=dev)
        idx = torch.empty((total,), dtype=torch.int32, device=dev)
        if total:
            _lib.check(emit(*inputs, base.data_ptr(), total, score.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws_bytes,
                            _lib.current_stream_ptr(), *keys))
    lims = base[::nprobe].contiguous()
    if sort and total:
        score, idx = _sort_segments(lims, score, idx)
    return RangeResult(lims, score, idx)


def _sort_segments(lims: torch.Tensor, score: torch.Tensor, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Every segment lims[q] .. lims[q + 1] of (score, idx) in the total order: stable sorts by id, by score descending, by
    query, the last key first (`refine_candidates`' way)."""
    nq, total = lims.shape[0] - 1, score.shape[0]
    query = torch.repeat_interleave(torch.arange(nq, device=lims.device), lims[1:] - lims[:-1], output_size=total)
    order = torch.sort(idx, stable=True)[1]
    order = order[torch.sort(score[order], descending=True, stable=True)[1]]
    order = order[torch.sort(query[order], stable=True)[1]]
    return score[order], idx[order]


def encode_rows_int8(xn: torch.Tensor, n: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """smi_ivf_i8_encode: (codes int8 [n, d], scales fp32 [n]) of the first n rows (default: all) of xn (contiguous fp16
    [>= n, d]): scale = amax / 127, code = rint(x * (127 / amax)), a zero row all zeros (tests/ivf_i8_ref.py)."""
    n = _check_rows16(xn, "xn", n)
    _check_int8_dim(xn.shape[1])
    lib = _lib.load()
    codes = torch.empty((n, xn.shape[1]), dtype=torch.int8, device=xn.device)
    scales = torch.empty((n,), dtype=torch.float32, device=xn.device)
    with torch.cuda.device(xn.device):
        _lib.check(lib.smi_ivf_i8_encode(xn.data_ptr(), n, xn.shape[1], codes.data_ptr(), scales.data_ptr(),
                                         _lib.current_stream_ptr()))
    return codes, scales


def build_lists_int8(xn: torch.Tensor, labels: torch.Tensor, n_lists: int):
    """smi_ivf_i8_build: `build_lists` with encoded rows.  Returns (codes int8 [slots, d], scales fp32 [slots], ids, offsets,
    sizes); a pad slot has zero codes, scale 0 and id -1."""
    _check_build_args(xn, labels, n_lists)
    _check_int8_dim(xn.shape[1])
    return _build("smi_ivf_i8_build", "smi_ivf_i8_build_workspace_bytes", xn, labels, n_lists, (),
                  [(torch.int8, xn.shape[1:]), (torch.float32, ())])


def search_lists_int8(qn: torch.Tensor, probes: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, ids: torch.Tensor,
                      offsets: torch.Tensor, k: int = 1, slot_keys: Optional[torch.Tensor] = None,
                      query_keys: Optional[torch.Tensor] = None, accept: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """smi_ivf_i8_search: `search_lists` against the storage `build_lists_int8` returned; the queries are encoded like the
    rows.  score = fl32(fl32((float)(integer dot product) * scale_row) * scale_query)."""
    _check_device_tensor(scales, "scales")
    _check_search_args(qn, probes, k)
    _check_int8_dim(qn.shape[1])
    _check_lists_dim(qn, codes)
    keyed = _check_keyed(slot_keys, query_keys, accept, ids.shape[0], probes.shape[0])
    return _search("smi_ivf_i8_search", "smi_ivf_i8_search_workspace_bytes", qn, probes, k, (),
                   (codes.data_ptr(), scales.data_ptr()), ids, offsets, keyed=keyed)


def _check_codebooks(codebooks, d: Optional[int] = None) -> Tuple[int, int]:
    """(M, dsub) of fp16 codebooks [M, 256, dsub] on the device; d: the row width they must add up to."""
    _check_device_tensor(codebooks, "codebooks")
    if (codebooks.dtype != torch.float16 or codebooks.dim() != 3 or codebooks.shape[1] != PQ_CODEWORDS
            or codebooks.shape[2] not in PQ_DSUBS or codebooks.shape[0] < 1 or not codebooks.is_contiguous()):
        raise ValueError(f"codebooks must be contiguous fp16 [M, {PQ_CODEWORDS}, dsub] with dsub in {PQ_DSUBS}, got "
                         f"{codebooks.dtype} {list(codebooks.shape)}")
    m, dsub = codebooks.shape[0], codebooks.shape[2]
    if (m * dsub) % 64:
        raise ValueError(f"codebooks: dim = {m} * {dsub} must be a multiple of 64")
    if d is not None and m * dsub != d:
        raise ValueError(f"codebooks cover dim {m} * {dsub} = {m * dsub}, the rows have {d}")
    return m, dsub


def _check_dsub(dsub, d: int) -> None:
    if isinstance(dsub, bool) or not isinstance(dsub, int) or dsub not in PQ_DSUBS:
        raise ValueError(f"dsub = {dsub!r}: one of {PQ_DSUBS}")
    if d % dsub:
        raise ValueError(f"dsub = {dsub} does not divide dim = {d}")


def _check_codes(codes, name: str, m: int) -> None:
    _check_device_tensor(codes, name)
    if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[0] < 1 or codes.shape[1] != m or not codes.is_contiguous():
        raise ValueError(f"{name} must be contiguous uint8 [rows, {m}], got {codes.dtype} {list(codes.shape)}")


def _pq_train(xn, n: int, dsub, init, n_iter, residual=None) -> torch.Tensor:
    """smi_pq_train on the first n rows of xn, or smi_pq_train_residual with residual = (labels, centroids, K)."""
    d = xn.shape[1]
    _check_dsub(dsub, d)
    if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 0:
        raise ValueError(f"n_iter = {n_iter!r}: a non-negative integer")
    _check_table(init, "init", PQ_CODEWORDS, None)
    lib = _lib.load()
    ws_bytes = int(lib.smi_pq_train_workspace_bytes(n, d, dsub))
    if ws_bytes < 1:
        raise ValueError(f"{n} rows of dim {d}: too large for one training call")
    codebooks = torch.empty((d // dsub, PQ_CODEWORDS, dsub), dtype=torch.float16, device=xn.device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=xn.device)
    init = init.contiguous()
    tail = (dsub, init.data_ptr(), n_iter, codebooks.data_ptr(), ws.data_ptr(), ws_bytes, _lib.current_stream_ptr())
    with torch.cuda.device(xn.device):
        if residual is None:
            _lib.check(lib.smi_pq_train(xn.data_ptr(), n, d, *tail))
        else:
            labels, centroids, k = residual
            _lib.check(lib.smi_pq_train_residual(xn.data_ptr(), labels.data_ptr(), n, d, centroids.data_ptr(), k, *tail))
    return codebooks


def pq_train(xn: torch.Tensor, dsub: int, init: torch.Tensor, n_iter: int = 10, n: Optional[int] = None) -> torch.Tensor:
    """smi_pq_train: codebooks fp16 [d / dsub, 256, dsub] after n_iter Lloyd rounds on the first n rows (default: all) of xn
    (contiguous fp16 [>= n, d]: rows of `normalize_rows`, or of `prepare_rows` for the L2 classes -- the quantiser is
    Euclidean and never needed unit rows), started from the subvectors of the rows init names (device int32 [256], values in
    [0, n): not checked here).  No read-back; one init gives one result bit for bit."""
    return _pq_train(xn, _check_rows16(xn, "xn", n), dsub, init, n_iter)


def pq_encode(xn: torch.Tensor, codebooks: torch.Tensor, n: Optional[int] = None) -> torch.Tensor:
    """smi_pq_encode: codes uint8 [n, M] of the first n rows (default: all) of xn (contiguous fp16 [>= n, d]) against
    codebooks (fp16 [M, 256, dsub]): per sub-quantiser the Euclidean nearest codeword by the fp32 chain of
    tests/ivf_pq_ref.py, ties to the lower code."""
    n = _check_rows16(xn, "xn", n)
    m, dsub = _check_codebooks(codebooks, xn.shape[1])
    lib = _lib.load()
    codes = torch.empty((n, m), dtype=torch.uint8, device=xn.device)
    with torch.cuda.device(xn.device):
        _lib.check(lib.smi_pq_encode(xn.data_ptr(), n, xn.shape[1], dsub, codebooks.data_ptr(), codes.data_ptr(),
                                     _lib.current_stream_ptr()))
    return codes


def pq_decode(codes: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    """smi_pq_decode: rows fp16 [n, d], row r the concatenation of the codewords codes[r] (uint8 [n, M]) names."""
    m, dsub = _check_codebooks(codebooks)
    _check_codes(codes, "codes", m)
    lib = _lib.load()
    rows = torch.empty((codes.shape[0], m * dsub), dtype=torch.float16, device=codes.device)
    with torch.cuda.device(codes.device):
        _lib.check(lib.smi_pq_decode(codes.data_ptr(), codes.shape[0], m * dsub, dsub, codebooks.data_ptr(), rows.data_ptr(),
                                     _lib.current_stream_ptr()))
    return rows


def _build_pq(xn, labels, n_lists: int, codebooks, centroids=None):
    """smi_ivf_pq_build, or smi_ivf_pq_build_residual against centroids (fp16 [n_lists, d])."""
    m, dsub = _check_codebooks(codebooks, xn.shape[1])
    entry, cent = ("smi_ivf_pq_build", ()) if centroids is None else ("smi_ivf_pq_build_residual", (centroids.data_ptr(),))
    return _build(entry, "smi_ivf_pq_build_workspace_bytes", xn, labels, n_lists, (*cent, dsub, codebooks.data_ptr()),
                  [(torch.uint8, (m,))], (dsub,))


def build_lists_pq(xn: torch.Tensor, labels: torch.Tensor, n_lists: int, codebooks: torch.Tensor):
    """smi_ivf_pq_build: `build_lists` with every row encoded against codebooks (fp16 [M, 256, dsub]).  Returns (codes uint8
    [slots, M], ids, offsets, sizes); a pad slot has zero codes and id -1."""
    _check_build_args(xn, labels, n_lists)
    return _build_pq(xn, labels, n_lists, codebooks)


def _check_coarse(coarse, shape) -> None:
    """The coarse term of a residual search: device fp32 of the probe table's shape."""
    _check_device_tensor(coarse, "coarse")
    if coarse.dtype != torch.float32 or tuple(coarse.shape) != tuple(shape):
        raise ValueError(f"coarse must be fp32 {list(shape)}, got {coarse.dtype} {list(coarse.shape)}")


def _search_pq(qn, probes, codes, codebooks, ids, offsets, k: int, coarse=None, keys=(None, None, None)):
    """smi_ivf_pq_search, or smi_ivf_pq_search_residual with coarse (fp32, the shape of probes); keys: (slot_keys,
    query_keys, accept) of `search_lists`."""
    _check_search_args(qn, probes, k)
    keyed = _check_keyed(*keys, ids.shape[0], probes.shape[0])
    if coarse is not None:
        _check_coarse(coarse, probes.shape)
    m, dsub = _check_codebooks(codebooks, qn.shape[1])
    _check_codes(codes, "codes", m)
    entry, extra = "smi_ivf_pq_search", ()
    if coarse is not None:
        coarse = coarse.contiguous()  # (held until the call is enqueued)
        entry, extra = "smi_ivf_pq_search_residual", (coarse.data_ptr(),)
    return _search(entry, "smi_ivf_pq_search_workspace_bytes", qn, probes, k, extra, (codes.data_ptr(), dsub, codebooks.data_ptr()),
                   ids, offsets, (dsub,), keyed)


def search_lists_pq(qn: torch.Tensor, probes: torch.Tensor, codes: torch.Tensor, codebooks: torch.Tensor, ids: torch.Tensor,
                    offsets: torch.Tensor, k: int = 1, slot_keys: Optional[torch.Tensor] = None,
                    query_keys: Optional[torch.Tensor] = None, accept: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """smi_ivf_pq_search: `search_lists` against the storage `build_lists_pq` returned.  A score has the bits `search_lists`
    returns for the query against `pq_decode` of the row."""
    return _search_pq(qn, probes, codes, codebooks, ids, offsets, k, None, (slot_keys, query_keys, accept))


def _check_centroids(centroids, d: int) -> int:
    """K of the fp16 centroid table [>= K, d] a residual function is given: K = its rows."""
    _check_matrix(centroids, "centroids")
    if centroids.dtype != torch.float16 or not centroids.is_contiguous() or centroids.shape[1] != d:
        raise ValueError(f"centroids must be a contiguous fp16 [K, {d}] matrix, got {centroids.dtype} {list(centroids.shape)}")
    return centroids.shape[0]


def _check_residual_args(xn, labels, centroids) -> Tuple[int, int]:
    """(n, K): the rows labels covers and the rows of centroids."""
    _check_matrix(xn, "xn")
    k = _check_centroids(centroids, xn.shape[1])
    _check_build_args(xn, labels, k)
    return labels.shape[0], k


def pq_residuals(xn: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
    """smi_pq_residuals: fp16 [n, d], row i = fp16(fp32(xn[i]) - fp32(centroids[labels[i]])) for the first n = len(labels) rows of
    xn (contiguous fp16 [>= n, d]); labels device int32 [n], centroids contiguous fp16 [K, d].  A label outside [0, K) leaves
    the row as it is.  The other residual functions form these elements inside their kernels."""
    n, k = _check_residual_args(xn, labels, centroids)
    lib = _lib.load()
    out = torch.empty((n, xn.shape[1]), dtype=torch.float16, device=xn.device)
    labels = labels.contiguous()
    with torch.cuda.device(xn.device):
        _lib.check(lib.smi_pq_residuals(xn.data_ptr(), labels.data_ptr(), n, xn.shape[1], centroids.data_ptr(), k,
                                        out.data_ptr(), _lib.current_stream_ptr()))
    return out


def pq_encode_residual(xn: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    """smi_pq_encode_residual: `pq_encode(pq_residuals(xn, labels, centroids), codebooks)` without the residual matrix."""
    n, k = _check_residual_args(xn, labels, centroids)
    m, dsub = _check_codebooks(codebooks, xn.shape[1])
    lib = _lib.load()
    codes = torch.empty((n, m), dtype=torch.uint8, device=xn.device)
    labels = labels.contiguous()
    with torch.cuda.device(xn.device):
        _lib.check(lib.smi_pq_encode_residual(xn.data_ptr(), labels.data_ptr(), n, xn.shape[1], centroids.data_ptr(), k, dsub,
                                              codebooks.data_ptr(), codes.data_ptr(), _lib.current_stream_ptr()))
    return codes


def pq_train_residual(xn: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor, dsub: int, init: torch.Tensor,
                      n_iter: int = 10) -> torch.Tensor:
    """smi_pq_train_residual: `pq_train(pq_residuals(xn, labels, centroids), dsub, init, n_iter)` without the residual
    matrix: the codebooks start from the residuals of the rows init names."""
    n, k = _check_residual_args(xn, labels, centroids)
    return _pq_train(xn, n, dsub, init, n_iter, (labels.contiguous(), centroids, k))


def build_lists_pq_residual(xn: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor, codebooks: torch.Tensor):
    """smi_ivf_pq_build_residual: `build_lists_pq` over the n_lists = len(centroids) lists with every row encoded as its
    residual against the centroid of its list.  Returns (codes uint8 [slots, M], ids, offsets, sizes): `build_lists_pq`'s
    storage, byte for byte."""
    _, n_lists = _check_residual_args(xn, labels, centroids)
    return _build_pq(xn, labels, n_lists, codebooks, centroids)


def search_lists_pq_residual(qn: torch.Tensor, probes: torch.Tensor, coarse: torch.Tensor, codes: torch.Tensor,
                             codebooks: torch.Tensor, ids: torch.Tensor, offsets: torch.Tensor, k: int = 1,
                             slot_keys: Optional[torch.Tensor] = None, query_keys: Optional[torch.Tensor] = None,
                             accept: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """smi_ivf_pq_search_residual: `search_lists_pq` against the storage `build_lists_pq_residual` returned, with
    coarse (device fp32 [nq, nprobe]: the score of query q against the centroid of the list probes[q, p]) added to every score
    of that pair in fp32.  The entry of a probe that names no list is not read."""
    if coarse is None:
        raise TypeError("coarse must be a torch.Tensor")
    return _search_pq(qn, probes, codes, codebooks, ids, offsets, k, coarse, (slot_keys, query_keys, accept))


def pq_l2_bias(codes: torch.Tensor, codebooks: torch.Tensor, labels: Optional[torch.Tensor] = None,
               centroids: Optional[torch.Tensor] = None, *, ids: Optional[torch.Tensor] = None,
               offsets: Optional[torch.Tensor] = None) -> torch.Tensor:
    """smi_l2_pq_bias: fp32 [n], the L2 bias of every row of codes (uint8 [n, M]) against codebooks (fp16
    [M, 256, dsub]); one wave per row, nothing of size n x d is allocated.

    Plain (centroids None): -fl32(1/2 ||y^||^2) of the decoded row y^, the bits of `prepare_rows(pq_decode(codes,
    codebooks))[1].neg()`.  Residual (centroids: contiguous fp16 [K, d], the lists' Euclidean centroids): -fl32(sum c r^ +
    1/2 sum r^ r^) against the centroid c of the row's list, r^ the decoded residual -- two fp64 sums in `prepare_rows`' order,
    one fp64 add, one rounding.  The list of row i is labels[i] (device int32 [n]; the form `extend` encodes new rows with),
    or, over the slots of a storage, the list whose range of offsets (int32 [K + 1]) holds slot i: exactly one of the two.
    ids (int32 [n]): the rows are slots, and one whose id is below 0 (a pad, an unused slot) gets 0.  Both forms run one
    device function: the bias of a row does not depend on the form."""
    m, dsub = _check_codebooks(codebooks)
    _check_codes(codes, "codes", m)
    n, d = codes.shape[0], m * dsub
    if ids is not None:
        _check_table(ids, "ids", n, None)
    k = 0
    if centroids is None:
        if labels is not None or offsets is not None:
            raise ValueError("labels and offsets name the lists of centroids: give centroids, or neither")
    else:
        k = _check_centroids(centroids, d)
        if (labels is None) == (offsets is None):
            raise ValueError("with centroids, give labels or offsets: one of the two")
        if labels is not None:
            _check_table(labels, "labels", n, None)
        else:
            if ids is None:
                raise ValueError("offsets describe slots: give ids with them")
            _check_table(offsets, "offsets", k + 1, None)
    lib = _lib.load()
    out = torch.empty((n,), dtype=torch.float32, device=codes.device)
    held = [None if t is None else t.contiguous() for t in (ids, offsets, labels)]  # (until the call is enqueued)
    with torch.cuda.device(codes.device):
        _lib.check(lib.smi_l2_pq_bias(codes.data_ptr(), n, d, dsub, codebooks.data_ptr(), *(None if t is None else t.data_ptr() for t in held),
                                      None if centroids is None else centroids.data_ptr(), k, out.data_ptr(),
                                      _lib.current_stream_ptr()))
    return out


def search_lists_pq_l2(q16: torch.Tensor, probes: torch.Tensor, codes: torch.Tensor, codebooks: torch.Tensor, bias: torch.Tensor,
                       ids: torch.Tensor, offsets: torch.Tensor, k: int = 1,
                       coarse: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """smi_l2_pq_search, or with coarse smi_l2_pq_search_residual: `search_lists_pq` on prepared queries
    (`xsim.prepare_rows`) with score = fl32(sum + bias[slot]), bias fp32 [slots] from `pq_l2_bias`; with coarse (device fp32,
    the shape of probes: the biased score of query q against the centroid of the list probes[q, p], `topk_bias_prepared`'s)
    over residual codes, score = fl32(fl32(sum + bias[slot]) + coarse[q, p]).  (scores fp32 [nq, k] best first, ids int32
    [nq, k]); ||q - row||^2 = 2 (h_q - score) for the reconstructed row.  ids may be a `RowFilter`'s.  No keyed form."""
    _check_search_args(q16, probes, k)
    if coarse is not None:
        _check_coarse(coarse, probes.shape)
    m, dsub = _check_codebooks(codebooks, q16.shape[1])
    _check_codes(codes, "codes", m)
    _check_device_tensor(bias, "bias")
    if bias.dtype != torch.float32 or tuple(bias.shape) != (ids.shape[0],) or not bias.is_contiguous():
        raise ValueError(f"bias must be contiguous fp32 [{ids.shape[0]}], got {bias.dtype} {list(bias.shape)}")
    entry, extra = "smi_l2_pq_search", ()
    if coarse is not None:
        coarse = coarse.contiguous()  # (held until the call is enqueued)
        entry, extra = "smi_l2_pq_search_residual", (coarse.data_ptr(),)
    return _search(entry, "smi_l2_pq_search_ws_bytes", q16, probes, k, extra,
                   (codes.data_ptr(), dsub, codebooks.data_ptr(), bias.data_ptr()), ids, offsets, (dsub,))


class ProductQuantizer:
    """M = d / dsub sub-quantisers of 256 codewords each over rows of `normalize_rows`.  `train` and `encode`
    normalise; the L2 classes train their codebooks on the rows as they are (`pq_train`) and hand them over.

    codebooks: fp16 [M, 256, dsub] on the device, dsub in {8, 16, 32, 64}, M * dsub a multiple of 64 (copied)."""

    def __init__(self, codebooks: torch.Tensor):
        self._m, self._dsub = _check_codebooks(codebooks)
        self._codebooks = codebooks.clone()

    @classmethod
    def train(cls, x: torch.Tensor, dsub: int = 16, n_iter: int = 10, seed: int = 0, init: Optional[torch.Tensor] = None):
        """Lloyd rounds on `normalize_rows(x)` (x fp16 / fp32 [n, d] on the device).  init: None (256 distinct rows from
        `clustering.init_rows(n, 256, seed)`, so n >= 256) or 256 row numbers (a host or device integer tensor); a row named
        twice gives twin codewords, of which the higher code never gets a member and keeps its value."""
        _check_matrix(x, "x")
        n, d = x.shape
        _check_dsub(dsub, d)
        if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 0:
            raise ValueError(f"n_iter = {n_iter!r}: a non-negative integer")
        if init is None:
            init = init_rows(n, PQ_CODEWORDS, seed)
        else:
            if not isinstance(init, torch.Tensor) or init.dtype not in (torch.int32, torch.int64) or tuple(init.shape) != (PQ_CODEWORDS,):
                raise ValueError(f"init must be an integer tensor of {PQ_CODEWORDS} row numbers")
            if init.device.type != "meta" and not bool(((init >= 0) & (init < n)).all()):
                raise ValueError(f"init names rows outside [0, {n})")
        xn = normalize_rows(x)
        return cls(pq_train(xn, dsub, init.to(device=x.device, dtype=torch.int32), n_iter, n))

    @property
    def codebooks(self) -> torch.Tensor:
        return self._codebooks

    @property
    def dim(self) -> int:
        return self._m * self._dsub

    @property
    def dsub(self) -> int:
        return self._dsub

    @property
    def n_subquantizers(self) -> int:
        return self._m

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        """codes uint8 [n, M] of `normalize_rows(x)` (x fp16 / fp32 [n, d] on the device)."""
        _check_matrix(x, "x")
        if x.shape[1] != self.dim:
            raise ValueError(f"x has dim {x.shape[1]}, the codebooks {self.dim}")
        return pq_encode(normalize_rows(x), self._codebooks, x.shape[0])

    def decode(self, codes: torch.Tensor) -> torch.Tensor:
        """fp16 [n, d]: the reconstructed rows of codes (uint8 [n, M])."""
        return pq_decode(codes, self._codebooks)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"codebooks": self._codebooks.clone()}

    @classmethod
    def from_state_dict(cls, state: Dict[str, torch.Tensor]):
        if "codebooks" not in state:
            raise ValueError("state lacks ['codebooks']")
        return cls(state["codebooks"])


def _check_refine(refine, d: int) -> None:
    """`refine` of a quantised index's search: None, or the normalised fp16 corpus."""
    if refine is not None:
        _check_matrix(refine, "refine")
        if refine.dtype != torch.float16 or not refine.is_contiguous() or refine.shape[1] != d:
            raise ValueError(f"refine must be the contiguous fp16 [rows, {d}] matrix normalize_rows returned")


class _IVFIndex:
    """What the IVF indexes share: the quantiser, the probe, `search` with its argument checks, and the persistence.  A
    subclass names its storage (`_ROWS_DTYPE`, `_ROWS_NAME`; `_STORAGE`: the attributes `add` fills, in the order of its build
    entry; `_SLOT_VECTORS`: those of them that hold one value per slot beside `rows`, as (attribute, dtype, its name);
    `_EXTRA`: further tensors of its state, checked by `_check_extra`), says what it `_HOLDS` and gives `_build_lists` and
    `_search_lists`."""

    _ROWS_DTYPE = torch.float16
    _ROWS_NAME = "fp16"
    _STORAGE = ("_rows", "_ids", "_offsets", "_sizes")
    _SLOT_VECTORS = ()
    _EXTRA = ()
    _HOLDS = None  # the sentence that ends the refusal of `self_join`
    # the storage life-cycle, as class defaults so that an index made any way has them
    _generation = 0  # the `extend` / `remove` / `merge_from` calls so far: a `RowFilter` of another generation is refused
    _next_id = None  # the running id, one more than any id handed out; None: not known (a loaded state), read back on demand
    _rows_bound = None  # an upper bound on the rows the storage holds, known without a read-back

    def _check_extra(self, state, d: int, fresh: bool):
        """load_state_dict: (the columns `rows` must have, the attributes to take over from the `_EXTRA` entries)."""
        if "metric_l2" in state:
            raise ValueError("the state is that of an IVFFlatL2Index: its rows are not normalised and its scores carry a bias")
        return d, {}

    def __init__(self, quantizer: Union[SphericalKMeans, torch.Tensor]):
        if isinstance(quantizer, SphericalKMeans):
            c16 = quantizer.centroids_normalized  # raises before fit
            self._c16 = quantizer._c16.clone()  # a later step() of the quantiser must not move the lists' centroids
            self._k, self._d = quantizer.n_clusters, c16.shape[1]
        else:
            _check_matrix(quantizer, "quantizer")
            self._k, self._d = quantizer.shape
            self._c16 = normalize_rows(quantizer)
        self._added = False

    @classmethod
    def train(cls, x: torch.Tensor, n_lists: int, n_iter: int = 10, seed: int = 0):
        """Fit the coarse quantiser: spherical k-means with `n_lists` clusters on x (fp16 / fp32 [n, d] on the device)."""
        return cls(SphericalKMeans(n_lists, n_iter=n_iter, seed=seed).fit(x))

    # ------------------------------------------------------------------------------------------------ properties
    @property
    def n_lists(self) -> int:
        return self._k

    @property
    def dim(self) -> int:
        return self._d

    @property
    def centroids_normalized(self) -> torch.Tensor:
        return self._c16[: self._k]

    def _need_add(self, what: str) -> None:
        if not self._added:
            raise RuntimeError(f"{what} before add: the index holds no rows yet")

    @property
    def list_sizes(self) -> torch.Tensor:
        """int32 [K] on the device: the rows of every list."""
        self._need_add("list_sizes")
        return self._sizes

    @property
    def list_offsets(self) -> torch.Tensor:
        """int32 [K + 1] on the device: list c is the slots [offsets[c], offsets[c + 1]); offsets[K] = the slots in use."""
        self._need_add("list_offsets")
        return self._offsets

    @property
    def ntotal(self) -> int:
        """The rows in the index (those whose label named a list).  Reads the list sizes back."""
        self._need_add("ntotal")
        return int(self._sizes.sum().item())

    # ------------------------------------------------------------------------------------------------ the metric
    def _prepare_rows(self, x) -> tuple:
        """What the metric makes of rows, of the corpus and of queries alike: first the padded fp16 matrix that the nearest
        lists are found for and that the lists hold, then what `_build_lists` takes beside it."""
        return (normalize_rows(x),)

    def _nearest_lists(self, x16, n: int, nprobe: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(scores fp32, lists int32) [n, nprobe]: the nearest centroids of the first n prepared rows, nearest first."""
        return topk_normalized(x16, n, self._c16, self._k, nprobe)

    def _check_query(self, q) -> int:
        """The queries of a probe or a search: a device matrix of the index's dimension; returns nq."""
        _check_matrix(q, "q")
        if q.shape[1] != self._d:
            raise ValueError(f"q has dim {q.shape[1]}, the index {self._d}")
        return q.shape[0]

    # ------------------------------------------------------------------------------------------------ add
    def add(self, x: torch.Tensor, labels: Optional[torch.Tensor] = None):
        """Index the rows of x (fp16 / fp32 [n, d] on the device); ids are the row numbers.  Once per index.

        labels: None (the nearest centroid, the quantiser's top-1) or device int32 [n]; a label outside [0, K) leaves the
        row out.  Enqueued on the current stream with no read-back: instead of one synchronisation to size the storage from
        the list counts, the storage is sized for any labelling, `smi_ivf_slots_bound(n, K)` slots, at most
        (LIST_ALIGN - 1) * min(n, K) more than n; `state_dict` cuts it to the slots in use."""
        if self._added:
            raise RuntimeError("add was already called: `add` fills an empty index once; `extend` takes further rows")
        _check_matrix(x, "x")
        if x.shape[1] != self._d:
            raise ValueError(f"x has dim {x.shape[1]}, the centroids {self._d}")
        n = x.shape[0]
        if labels is not None:
            _check_table(labels, "labels", n, None)
        prepared = self._prepare_rows(x)
        if labels is None:
            labels = self._nearest_lists(prepared[0], n, 1)[1][:, 0]
        for name, t in zip(self._STORAGE, self._build_lists(*prepared, labels)):
            setattr(self, name, t)
        self._added = True
        self._next_id = self._rows_bound = n
        return self

    # ------------------------------------------------------------------------------------------------ extend, remove, merge
    def _encode_rows(self, prepared: tuple, labels: torch.Tensor, n: int):
        """(rows, aux or None) of the first n prepared rows as the lists hold them: what the build's gather writes for a
        row, by the class's stand-alone encoder."""
        return prepared[0], None

    @property
    def _aux_name(self) -> Optional[str]:
        """The attribute of the one value per slot the class keeps beside its rows (`_scales`, `_bias`), or None."""
        return self._SLOT_VECTORS[0][0] if self._SLOT_VECTORS else None

    def _running_id(self) -> int:
        """One more than the largest id handed out.  After `load_state_dict` it is max(ids) + 1: one read-back, once."""
        if self._next_id is None:
            self._next_id = int(self._ids.max().item()) + 1 if self._ids.shape[0] else 0
        return self._next_id

    def _old_storage(self, ids: Optional[torch.Tensor] = None):
        """This index's storage as the `old` of `regroup_lists` (ids: effective ids in place of its own), None if it has no
        slot."""
        if not self._ids.shape[0]:
            return None
        aux = self._aux_name
        return (self._rows, getattr(self, aux) if aux else None, self._ids if ids is None else ids, self._offsets)

    def _take_regrouped(self, old, new, n_new_bound: int, id_base: int = 0) -> None:
        """Run the regroup and take its storage over; n_new_bound: the most rows `new` adds."""
        slots = self._ids.shape[0]
        bound = slots if self._rows_bound is None else min(self._rows_bound, slots)
        rows, aux, ids, offsets, sizes = regroup_lists(self._k, old, new, bound if old is not None else None, id_base)
        self._rows, self._ids, self._offsets, self._sizes = rows, ids, offsets, sizes
        if self._aux_name:
            setattr(self, self._aux_name, aux)
        self._rows_bound = bound + n_new_bound
        self._generation += 1

    def _check_id_range(self, first: int, count: int, what: str) -> None:
        if first + count > ID_MAX:
            raise ValueError(f"{what}: ids {first} .. {first + count} exceed {ID_MAX} (row ids are int32)")

    def extend(self, x: torch.Tensor, labels: Optional[torch.Tensor] = None, first_id: Optional[int] = None):
        """Add the rows of x (fp16 / fp32 [n, d] on the device) to a filled index: `add(x1).extend(x2)` is the
        index `add(cat(x1, x2))` builds -- the same lists, ids, rows or codes and aux values, hence the same search results
        bit for bit.  The order of the slots inside a list is unspecified, as after `add`.

        labels: as for `add`.  first_id: the id of x[0] (the ids are first_id .. first_id + n); None continues at the running
        id, the number of rows handed to `add` / `extend` so far -- after `load_state_dict`, max(ids) + 1, read back once.
        The rows are encoded by the class's stand-alone encoder and regrouped with the old storage into fresh storage of
        `smi_ivf_slots_bound(rows so far + n, K)` slots (`regroup_lists`): one call costs about one build of the union, so
        feed chunks, not single rows.  Enqueued on the current stream, no read-back.  A `RowFilter` made before is refused
        afterwards: make a new one."""
        self._need_add("extend")
        _check_matrix(x, "x")
        if x.shape[1] != self._d:
            raise ValueError(f"x has dim {x.shape[1]}, the centroids {self._d}")
        if x.dtype not in (torch.float16, torch.float32):
            raise ValueError(f"x must be fp16 or fp32, got {x.dtype}")
        if x.device != self._ids.device:
            raise ValueError(f"x is on {x.device}, the index on {self._ids.device}")
        n = x.shape[0]
        if labels is not None:
            _check_table(labels, "labels", n, None)
        if first_id is not None and (isinstance(first_id, bool) or not isinstance(first_id, int) or first_id < 0):
            raise ValueError(f"first_id = {first_id!r}: None or a non-negative integer")
        base = self._running_id() if first_id is None else first_id
        self._check_id_range(base, n, "extend")
        prepared = self._prepare_rows(x)
        if labels is None:
            labels = self._nearest_lists(prepared[0], n, 1)[1][:, 0]
        labels = labels.contiguous()
        rows, aux = self._encode_rows(prepared, labels, n)
        self._take_regrouped(self._old_storage(), (rows, aux, labels, None), n, base)
        if self._next_id is not None:  # (unknown after load_state_dict and a first_id: max(ids) + 1 will cover these rows)
            self._next_id = max(self._next_id, base + n)
        return self

    def remove(self, ids: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
        """Drop rows from the index: their bytes and their scan cost go, where a `RowFilter` mask only hides
        them.  Exactly one of
          ids   a 1-D device int32 / int64 tensor of row ids (an id the index does not hold is ignored);
          mask  a device bool tensor, True = the row leaves, covering every id handed out so far.
        The rows that stay keep their ids.  The index is compacted into fresh storage on the effective ids `slot_filter`
        makes from the complement; the storage keeps its bound (`from_state_dict(state_dict())` cuts it to the slots in
        use).  Enqueued, no read-back (after `load_state_dict`: the one of the running id).  A `RowFilter` made before is
        refused afterwards."""
        self._need_add("remove")
        if (ids is None) == (mask is None):
            raise ValueError("remove: give ids or mask, one of the two")
        total = self._running_id()
        if mask is not None:
            _check_device_tensor(mask, "mask")
            if mask.dtype != torch.bool or mask.dim() != 1:
                raise ValueError(f"mask must be bool [n], got {mask.dtype} {list(mask.shape)}")
            if mask.shape[0] < max(total, 1):
                raise ValueError(f"mask has {mask.shape[0]} entries, the ids handed out so far go up to {total}")
            keep = mask.logical_not()
        else:
            _check_device_tensor(ids, "ids")
            if ids.dtype not in (torch.int32, torch.int64) or ids.dim() != 1:
                raise ValueError(f"ids must be int32 or int64 [m], got {ids.dtype} {list(ids.shape)}")
            # an id outside [0, total) lands in the spare entry: nothing is indexed out of range, nothing is read back
            keep = torch.ones((total + 1,), dtype=torch.bool, device=self._ids.device)
            if ids.shape[0]:
                inside = (ids >= 0) & (ids < total)
                keep[torch.where(inside, ids, torch.full_like(ids, total)).long()] = False
            keep = keep[: max(total, 1)]
        if keep.device != self._ids.device:
            raise ValueError(f"the rows to remove are named on {keep.device}, the index is on {self._ids.device}")
        old = self._old_storage()
        if old is None:
            return self  # no slots: nothing to remove
        effective = slot_filter(self._ids, self._offsets, mask=keep).ids
        self._take_regrouped(self._old_storage(effective), None, 0)
        return self

    def _check_same_lists(self, other) -> None:
        """merge_from: the two indexes must quantise alike, bit for bit (`torch.equal` reads back)."""
        if type(other) is not type(self):
            raise TypeError(f"merge_from: a {type(self).__name__} takes a {type(self).__name__}, got {type(other).__name__}")
        if other is self:
            raise ValueError("merge_from: an index cannot be merged into itself")
        other._need_add("merge_from (the other index)")
        if (other._k, other._d) != (self._k, self._d) or other._ids.device != self._ids.device:
            raise ValueError(f"merge_from: the other index has {other._k} lists of dim {other._d} on {other._ids.device}, this "
                             f"one {self._k} of dim {self._d} on {self._ids.device}")
        for name in ("_c16", *self._EXTRA):
            a, b = getattr(self, name), getattr(other, name)
            if name == "_c16":
                a, b = a[: self._k], b[: self._k]
            if a.shape != b.shape or not torch.equal(a, b):
                raise ValueError(f"merge_from: the other index has other {name[1:].replace('c16', 'centroids')}; merged lists "
                                 "need the same quantiser, bit for bit")

    def merge_from(self, other, add_id: Optional[int] = None):
        """Take over the rows of `other`, an index of the same class over the same centroids (and codebooks), bitwise
        (DESIGN.md 3.29): shards embedded separately become one index.  `other`'s slots are the new rows of a regroup, their
        labels their list numbers and their ids shifted by add_id (default: this index's running id, so that
        `a.add(x1); b.add(x2); a.merge_from(b)` is `add(cat(x1, x2))`).  `other` is left as it is.  The comparison of the
        quantisers reads back; the merge itself is enqueued."""
        self._need_add("merge_from")
        if not isinstance(other, _IVFIndex):
            raise TypeError(f"merge_from: a {type(self).__name__} takes a {type(self).__name__}, got {type(other).__name__}")
        self._check_same_lists(other)
        if add_id is not None and (isinstance(add_id, bool) or not isinstance(add_id, int) or add_id < 0):
            raise ValueError(f"add_id = {add_id!r}: None or a non-negative integer")
        shift = self._running_id() if add_id is None else add_id
        self._check_id_range(shift, other._running_id(), "merge_from")
        new = other._old_storage()
        if new is not None:
            slots = other._ids.shape[0]
            # the list of every slot from the offsets, without a read-back: the offsets at or below the slot, less one
            # (slots from offsets[K] on get K, which names no list)
            labels = torch.searchsorted(other._offsets[1:].contiguous(), torch.arange(slots, dtype=torch.int32, device=other._ids.device),
                                        right=True).to(torch.int32)
            ids = torch.where(other._ids >= 0, other._ids + shift, other._ids)
            self._take_regrouped(self._old_storage(), (new[0], new[1], labels, ids), min(other._rows_bound, slots))
        self._next_id = max(self._running_id(), shift + other._running_id())
        return self

    # ------------------------------------------------------------------------------------------------ search
    def probe(self, q: torch.Tensor, nprobe: int = 1) -> torch.Tensor:
        """int32 [nq, nprobe]: the nprobe nearest lists of every query, nearest first."""
        _check_small(nprobe, "nprobe")
        nq = self._check_query(q)
        if nprobe > self._k:
            raise ValueError(f"nprobe = {nprobe} exceeds the {self._k} lists")
        return self._nearest_lists(self._prepare_rows(q)[0], nq, nprobe)[1]

    def probe_wide(self, q: torch.Tensor, nprobe: int = PAGE) -> torch.Tensor:
        """`probe` for nprobe up to 64: the paged top-k against the centroids (`xsim.topk_wide_normalized`),
        one pass over them per 16 lists.  Like `probe`, it refuses an nprobe above the number of lists."""
        return self._probe_wide(q, nprobe)[1]

    def _probe_wide(self, q, nprobe, qn=None):
        """(coarse scores, probes) of `probe_wide`; qn: the normalised q, where the caller has it."""
        check_count(nprobe, "nprobe", WIDE_MAX)
        nq = self._check_query(q)
        if nprobe > self._k:
            raise ValueError(f"nprobe = {nprobe} exceeds the {self._k} lists")
        qn = normalize_rows(q) if qn is None else qn
        return topk_wide_normalized(qn, nq, self._c16, self._k, nprobe)

    def row_filter(self, keys: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> RowFilter:
        """The `RowFilter` of `search(..., rows=)`.  keys: device int32 [n], the key of every row `add` was
        given (row number = id), for `query_keys=` / `match=`; mask: device bool [n], False = the row does not exist for any
        query.  At least one of them.  A row beyond the end of a given tensor is left out.  Enqueued, no read-back; make it
        once and reuse it."""
        self._need_add("row_filter")
        return slot_filter(self._ids, self._offsets, keys, mask)._replace(generation=self._generation)

    def _filter(self, rows, query_keys, match, nq: int):
        """The filter arguments of `search` / `range_search`: (the ids the scan runs on, None for the index's own,
        (slot_keys, query_keys, accept) of the list function or three Nones)."""
        if match not in MATCH_ACCEPT:
            raise ValueError(f"match = {match!r}: one of {' '.join(MATCH_ACCEPT)}")
        if rows is None:
            if query_keys is not None:
                raise ValueError("query_keys needs rows=, a RowFilter that index.row_filter(keys=...) built")
            return None, (None, None, None)
        if not isinstance(rows, RowFilter):
            raise TypeError("rows must be a RowFilter (index.row_filter)")
        _check_device_tensor(rows.ids, "rows.ids")
        if rows.ids.dtype != torch.int32 or tuple(rows.ids.shape) != tuple(self._ids.shape):
            raise ValueError(f"rows: a RowFilter of {list(rows.ids.shape)} slots, this index has {list(self._ids.shape)} "
                             "(it belongs to another index, or to this one before load_state_dict)")
        if rows.generation != self._generation:
            raise ValueError(f"rows: a RowFilter of generation {rows.generation}, this index is at {self._generation}: extend, "
                             "remove and merge_from regroup the slots, so make a new one with index.row_filter")
        if query_keys is None:
            return rows.ids, (None, None, None)  # the mask alone: the existing scan on the filter's ids
        if rows.keys is None:
            raise ValueError("query_keys needs a RowFilter built with keys: index.row_filter(keys=...)")
        _check_table(query_keys, "query_keys", nq, None)
        return rows.ids, (rows.keys, query_keys, MATCH_ACCEPT[match])

    def _checked_search(self, q, k, nprobe, probes, refine=None, coarse=None, rows=None, query_keys=None, match="=="):
        """`search` of every kind: the argument checks, the probe, the subclass's scan and, with refine, the re-scoring.
        coarse: the scores that belong to probes (`IVFPQResidualIndex` alone passes them on); where the index probes by
        itself they are the probe's own, so `_search_lists` is handed them either way.  rows, query_keys, match: the filter
        (`IVFFlatIndex.search`)."""
        _check_refine(refine, self._d)
        nq = self._check_search(q, k, nprobe, probes)
        ids, keys = self._filter(rows, query_keys, match, nq)
        if coarse is not None:
            if probes is None:
                raise ValueError("coarse belongs to probes: give both, or neither")
            _check_coarse(coarse, probes.shape)
        qn = normalize_rows(q)
        if probes is None:
            coarse, probes = topk_normalized(qn, nq, self._c16, self._k, nprobe)
        score, idx = self._search_lists(qn, probes, k, coarse, ids, keys)
        return (score, idx) if refine is None else refine_candidates(qn, nq, refine, idx)

    def self_join(self, *args, **kwargs):
        raise TypeError(f"self_join and semdedup need the fp16 lists of an IVFFlatIndex; {self._HOLDS}")

    def range_search(self, *args, **kwargs):
        raise TypeError(f"range_search needs the fp16 lists of an IVFFlatIndex; {self._HOLDS}")

    def _check_search(self, q, k, nprobe, probes, what: str = "search", most_k: int = 8, most_probes: int = 8) -> int:
        """The argument checks of `search` (of `range_search`, with k = 1; of the paged searches, with their limits); returns
        nq."""
        check_count(k, "k", most_k)
        check_count(nprobe, "nprobe", most_probes)
        self._need_add(what)
        nq = self._check_query(q)
        if probes is not None:
            if isinstance(probes, torch.Tensor) and (probes.dim() != 2 or not 1 <= probes.shape[1] <= most_probes):
                raise ValueError(f"probes must be [nq, 1..{most_probes}], got {list(probes.shape)}")
            _check_table(probes, "probes", nq, probes.shape[1] if isinstance(probes, torch.Tensor) else 1)
        elif nprobe > self._k:
            raise ValueError(f"nprobe = {nprobe} exceeds the {self._k} lists")
        return nq

    # ------------------------------------------------------------------------------------------------ persistence
    def state_dict(self) -> Dict[str, torch.Tensor]:
        """centroids (fp16 [K, d], normalised), offsets, sizes, ids and rows (and scales, where the rows are int8 codes, or
        codebooks, where they are product-quantiser codes); the storage is cut to the slots in use (one read-back)."""
        self._need_add("state_dict")
        used = int(self._offsets[self._k].item())
        state = {"centroids": self._c16[: self._k].clone(), "offsets": self._offsets.clone(), "sizes": self._sizes.clone()}
        for name in self._STORAGE[:-2]:
            state[name[1:]] = getattr(self, name)[:used].clone()
        for name in self._EXTRA:
            state[name[1:]] = getattr(self, name).clone()
        return state

    @classmethod
    def from_state_dict(cls, state: Dict[str, torch.Tensor]):
        index = cls.__new__(cls)
        index._added = False
        index.load_state_dict(state, _fresh=True)
        return index

    def load_state_dict(self, state: Dict[str, torch.Tensor], _fresh: bool = False):
        """Take over a `state_dict()` (tensors on the device).  The centroids must have this index's shape."""
        missing = {"centroids", "offsets", "sizes", *(name[1:] for name in self._STORAGE[:-2] + self._EXTRA)} - set(state)
        if missing:
            raise ValueError(f"state lacks {sorted(missing)}")
        c = state["centroids"]
        _check_matrix(c, "centroids")
        k, d = c.shape
        if not _fresh and (k, d) != (self._k, self._d):
            raise ValueError(f"centroids are [{k}, {d}], this index has [{self._k}, {self._d}]")
        if c.dtype != torch.float16:
            raise ValueError("centroids must be the fp16 rows state_dict returns")
        _check_table(state["offsets"], "offsets", k + 1, None)
        _check_table(state["sizes"], "sizes", k, None)
        rows, ids = state["rows"], state["ids"]
        _check_table(ids, "ids", rows.shape[0] if isinstance(rows, torch.Tensor) else -1, None)
        width, extra = self._check_extra(state, d, _fresh)
        if not rows.is_cuda or rows.dtype != self._ROWS_DTYPE or rows.dim() != 2 or rows.shape[1] != width:
            raise ValueError(f"rows must be {self._ROWS_NAME} [slots, {width}] on the device")
        for attr, dtype, name in self._SLOT_VECTORS:
            t = state[attr[1:]]
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or tuple(t.shape) != (rows.shape[0],):
                raise ValueError(f"{attr[1:]} must be {name} [{rows.shape[0]}] on the device")
            extra[attr] = t.contiguous().clone()
        used = int(state["offsets"][k].item())
        if used != rows.shape[0] or used % LIST_ALIGN:
            raise ValueError(f"offsets end at slot {used}, rows has {rows.shape[0]} (a multiple of {LIST_ALIGN} is expected)")
        self._k, self._d = k, d
        pad = (k + 255) // 256 * 256
        self._c16 = torch.zeros((pad, d), dtype=torch.float16, device=c.device)
        self._c16[:k] = c
        self._offsets, self._sizes = state["offsets"].contiguous().clone(), state["sizes"].contiguous().clone()
        self._ids, self._rows = ids.contiguous().clone(), rows.contiguous().clone()
        for name, t in extra.items():
            setattr(self, name, t)
        self._added = True
        self._next_id, self._rows_bound = None, rows.shape[0]  # the running id: max(ids) + 1, read back when first needed
        return self


class IVFFlatIndex(_IVFIndex):
    """train / add / search over fp16 copies of the rows; see the module text.

    quantizer: a fitted `SphericalKMeans`, or an [K, d] tensor of centroids (normalised with `normalize_rows`)."""

    def _build_lists(self, xn, labels):
        return build_lists(xn, labels, self._k)

    def _search_lists(self, qn, probes, k, coarse, ids, keys):
        return search_lists(qn, probes, self._rows, self._ids if ids is None else ids, self._offsets, k, *keys)

    def search(self, q: torch.Tensor, k: int = 1, nprobe: int = 1, probes: Optional[torch.Tensor] = None, *,
               rows: Optional[RowFilter] = None, query_keys: Optional[torch.Tensor] = None,
               match: str = "==") -> Tuple[torch.Tensor, torch.Tensor]:
        """The k best rows of the probed lists for every row of q (fp16 / fp32 [nq, d] on the device): (scores fp32
        [nq, k], ids int32 [nq, k]), the layout and order of `xsim.topk`.

        probes: None (the nprobe nearest lists by the quantiser) or device int32 [nq, 1..8]; an entry outside [0, K) names
        no list.  A row of probes that names a list twice may return that list's rows twice.

        Filtering (the recipes are in the module text), on every index class alike.  rows: a `RowFilter` of
        this index (`row_filter`): only its visible rows count.  query_keys: device int32 [nq], with a filter built with
        keys: row i counts for query j only if `keys[i] match query_keys[j]`, match one of == != < <= > >= (signed).  The
        result is what `search` would return over an index of the rows that count for the query: k results wherever k of the
        probed rows qualify, (-inf, -1) behind them, the same bits alone and in any batch.  Nothing more is read back; the
        call stays capturable."""
        return self._checked_search(q, k, nprobe, probes, rows=rows, query_keys=query_keys, match=match)

    def _check_search_wide(self, q, k, most_k, nprobe, probes, rows, what: str):
        """The argument checks of `search_page` / `search_wide`; returns (nq, the ids the scan runs on)."""
        nq = self._check_search(q, k, nprobe, probes, what, most_k, WIDE_MAX)
        ids = self._filter(rows, None, "==", nq)[0]
        return nq, self._ids if ids is None else ids

    def search_page(self, q: torch.Tensor, k: int = PAGE, nprobe: int = 1, probes: Optional[torch.Tensor] = None, *,
                    rows: Optional[RowFilter] = None, below=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """One page of a wide search: `search` for k <= 16 and nprobe <= 64, and with below = (scores fp32
        [nq], ids int32 [nq]) the k best rows of the probed lists strictly AFTER each query's exclusive ceiling in the total
        order -- hand it the last entry of the page before.  A query whose ceiling id is negative (a fill entry) is
        exhausted.  probes: None or device int32 [nq, 1..64]; give the SAME probes to every page of one search (the probe is
        then computed once).  rows: the mask of a `RowFilter`, as for `search`; the key predicate is not available here."""
        nq, ids = self._check_search_wide(q, k, PAGE, nprobe, probes, rows, "search_page")
        below = check_below(below, nq, q)
        qn = normalize_rows(q)
        if probes is None:
            probes = self._probe_wide(q, nprobe, qn)[1]
        return search_lists_page(qn, probes, self._rows, ids, self._offsets, k, below)

    def search_wide(self, q: torch.Tensor, k: int = PAGE, nprobe: int = PAGE, probes: Optional[torch.Tensor] = None, *,
                    rows: Optional[RowFilter] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """`search` for k and nprobe up to 64: one probe (`probe_wide`), then ceil(k / 16) pages of the
        scan (`search_page`), each with the last entry of the one before as its ceiling, the last asking only for what is
        left, concatenated on the device.  The result is the top-k of the probed lists in `search`'s order and layout, bit
        for bit the same however it is split, alone or in any batch.  rows: the mask of a `RowFilter`.  No read-back."""
        nq, ids = self._check_search_wide(q, k, WIDE_MAX, nprobe, probes, rows, "search_wide")
        qn = normalize_rows(q)
        if probes is None:
            probes = self._probe_wide(q, nprobe, qn)[1]
        return concat_pages(lambda kp, below: search_lists_page(qn, probes, self._rows, ids, self._offsets, kp, below), k)

    def range_search(self, q: torch.Tensor, threshold: Union[float, torch.Tensor], nprobe: int = 1,
                     probes: Optional[torch.Tensor] = None, sort: bool = True, max_total: Optional[int] = None, *,
                     rows: Optional[RowFilter] = None, query_keys: Optional[torch.Tensor] = None,
                     match: str = "==") -> RangeResult:
        """EVERY row of the probed lists whose score is >= threshold, for every row of q (fp16 / fp32 [nq, d] on the device):
        `RangeResult(lims int64 [nq + 1], scores fp32 [total], ids int32 [total])`, FAISS's layout -- the hits of query i are
        the entries lims[i] .. lims[i + 1].  A score has the bits `search` returns for the same two rows.

        threshold: a Python float for every query (NaN is refused), or device fp32 [nq], one per query (an fp32 compare:
        a NaN entry hits nothing, -inf every row of the probed lists).  probes: as for `search`; a list named twice returns
        its hits twice.  sort: every segment best first, in `search`'s total order (score descending, ties to the lower
        id); with sort=False the order inside a segment is unspecified.  max_total: raise ValueError, the total named, where
        more hits than this would be allocated.

        rows, query_keys, match: the filter of `search`; only the rows that count for a query can be its hits.

        The lists are walked twice, to count and to write, and the total is READ BACK once in between to size the result:
        the call synchronises with the host and is not capturable."""
        nq = self._check_search(q, 1, nprobe, probes, "range_search")
        _check_max_total(max_total)
        threshold = _check_thresholds(threshold, nq, q)
        ids, keys = self._filter(rows, query_keys, match, nq)
        qn = normalize_rows(q)
        if probes is None:
            probes = topk_normalized(qn, nq, self._c16, self._k, nprobe)[1]
        return range_search_lists(qn, probes, threshold, self._rows, self._ids if ids is None else ids, self._offsets, sort,
                                  max_total, *keys)

    def self_join(self, priority: Optional[torch.Tensor] = None, n: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """`dedup.self_join` over this index's own lists: (max_sim fp32 [n], nearest int32 [n]), for every
        row its best score against the rows of its list that precede it (priority higher, or equal and id lower), and that
        row's id.  n: the number of rows `add` was given (ids lie in [0, n)); None takes the length of `priority`."""
        from . import dedup

        self._need_add("self_join")
        if n is None:
            if not isinstance(priority, torch.Tensor):
                raise ValueError("give n, the number of rows the index was filled from, or a priority tensor of that length")
            n = priority.shape[0] if priority.dim() == 1 else -1
        return dedup.self_join(self._rows, self._ids, self._offsets, n, priority)


class IVFFlatL2Index(_IVFIndex):
    """`IVFFlatIndex` under the squared Euclidean distance, on the rows as they are: train / add / probe /
    search, `state_dict` / `load_state_dict`.  The lists hold fp16 copies of the rows (rounded, not normalised) and one fp32
    bias per slot, -||row||^2 / 2; the probe is the biased top-k against the centroids and the scan adds the slot's bias to
    the flat scan's sum, so the best score is the nearest row.  `state_dict` adds `bias` and the marker `metric_l2`, so that
    neither this class nor `IVFFlatIndex` loads the other's state.

    quantizer: a fitted `clustering.KMeans`, or an [K, d] tensor of centroids (taken as they are, rounded to fp16)."""

    _STORAGE = ("_rows", "_bias", "_ids", "_offsets", "_sizes")
    _SLOT_VECTORS = (("_bias", torch.float32, "fp32"),)
    _HOLDS = "an IVFFlatL2Index holds rows that are not normalised"

    def __init__(self, quantizer: Union[KMeans, torch.Tensor]):
        if isinstance(quantizer, KMeans):
            c16 = quantizer.centroids_f16  # raises before fit
            self._c16, self._ch = quantizer._c16.clone(), quantizer._ch.clone()
            self._k, self._d = quantizer.n_clusters, c16.shape[1]
        elif isinstance(quantizer, SphericalKMeans):
            raise TypeError("an IVFFlatL2Index needs Euclidean centroids: a fitted clustering.KMeans, or a tensor")
        else:
            _check_matrix(quantizer, "quantizer")
            self._k, self._d = quantizer.shape
            self._c16, self._ch = prepare_rows(quantizer)
        self._added = False

    @classmethod
    def train(cls, x: torch.Tensor, n_lists: int, n_iter: int = 10, seed: int = 0):
        """Fit the coarse quantiser: Euclidean k-means with `n_lists` clusters on x (fp16 / fp32 [n, d] on the device)."""
        return cls(KMeans(n_lists, n_iter=n_iter, seed=seed).fit(x))

    @property
    def centroids_f16(self) -> torch.Tensor:
        return self._c16[: self._k]

    @property
    def centroids_normalized(self) -> torch.Tensor:
        raise TypeError("an IVFFlatL2Index keeps its centroids as they are: centroids_f16")

    # the metric: the rows as they are with their half norms, the nearest centroid in the Euclidean sense (the biased top-k)
    _prepare_rows = staticmethod(prepare_rows)

    def _nearest_lists(self, x16, n: int, nprobe: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return topk_bias_prepared(x16, n, self._c16, self._k, self._ch.neg(), nprobe)

    def _build_lists(self, x16, half_norms, labels):
        rows, ids, offsets, sizes = build_lists(x16, labels, self._k)
        return rows, slot_bias(ids, half_norms), ids, offsets, sizes

    def _encode_rows(self, prepared, labels, n):
        return prepared[0], prepared[1][:n].neg()  # `slot_bias`'s value for the row

    def search(self, q: torch.Tensor, k: int = 1, nprobe: int = 1, probes: Optional[torch.Tensor] = None, *,
               rows: Optional[RowFilter] = None, query_keys=None, refine=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The k nearest rows of the probed lists for every row of q (fp16 / fp32 [nq, d] on the device): (squared distances
        fp32 [nq, k] ascending, ids int32 [nq, k]), ties to the lower row number, (+inf, -1) where the probed lists hold fewer
        than k rows.  sq_dist = clamp_min(2 (h_q - score), 0), as `xsim.topk_l2`; over all lists it IS `xsim.topk_l2` over the
        corpus.  probes: as for `IVFFlatIndex.search`.  rows: a `RowFilter` of this index built with a mask."""
        if query_keys is not None:
            raise TypeError("query_keys: the keyed scan has no L2 twin (DESIGN.md 7); filter with rows=index.row_filter(mask=...)")
        if refine is not None:
            raise TypeError("refine re-scores quantised candidates with fp16 cosines; an IVFFlatL2Index already scores the fp16 rows")
        nq = self._check_search(q, k, nprobe, probes)
        ids = self._filter(rows, None, "==", nq)[0]
        q16, hq = prepare_rows(q)
        if probes is None:
            probes = self._nearest_lists(q16, nq, nprobe)[1]
        score, idx = search_lists_l2(q16, probes, self._rows, self._bias, self._ids if ids is None else ids, self._offsets, k)
        return (2.0 * (hq[:nq, None] - score)).clamp_min(0.0), idx

    def range_search(self, *args, **kwargs):
        raise TypeError("range_search thresholds cosines; it has no L2 variant (DESIGN.md 7)")

    def probe_wide(self, *args, **kwargs):
        raise TypeError("probe_wide is the paged cosine top-k; an IVFFlatL2Index probes at most 8 lists (DESIGN.md 7)")

    def search_wide(self, *args, **kwargs):
        raise TypeError("search_wide is the paged cosine search; an IVFFlatL2Index returns at most 8 rows (DESIGN.md 7)")

    def self_join(self, *args, **kwargs):
        raise TypeError("self_join and semdedup score cosines; they have no L2 variant (DESIGN.md 7)")

    def _check_extra(self, state, d: int, fresh: bool):
        if "metric_l2" not in state:
            raise ValueError("state lacks ['metric_l2']: the state is that of an IVFFlatIndex, whose rows are normalised")
        return d, {}

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """`IVFFlatIndex.state_dict` with the centroids as they are, `bias` (fp32 [slots]) and the marker `metric_l2`."""
        state = super().state_dict()
        state["metric_l2"] = torch.ones(1, dtype=torch.uint8, device=self._rows.device)
        return state

    def load_state_dict(self, state: Dict[str, torch.Tensor], _fresh: bool = False):
        super().load_state_dict(state, _fresh)
        self._ch = prepare_rows(self._c16[: self._k])[1]  # the half norms of the fp16 centroids: the same bits
        return self


class IVFInt8Index(_IVFIndex):
    """`IVFFlatIndex` over int8 codes and one fp32 scale per row: half the storage, exact integer scan.
    `state_dict` adds `scales`, and its `rows` are the int8 codes."""

    _ROWS_DTYPE = torch.int8
    _ROWS_NAME = "int8"
    _STORAGE = ("_rows", "_scales", "_ids", "_offsets", "_sizes")
    _SLOT_VECTORS = (("_scales", torch.float32, "fp32"),)
    _HOLDS = "an IVFInt8Index holds int8 codes"

    def __init__(self, quantizer: Union[SphericalKMeans, torch.Tensor]):
        super().__init__(quantizer)
        _check_int8_dim(self._d)

    def _build_lists(self, xn, labels):
        return build_lists_int8(xn, labels, self._k)

    def _encode_rows(self, prepared, labels, n):
        return encode_rows_int8(prepared[0], n)

    def _search_lists(self, qn, probes, k, coarse, ids, keys):
        return search_lists_int8(qn, probes, self._rows, self._scales, self._ids if ids is None else ids, self._offsets, k, *keys)

    def search(self, q: torch.Tensor, k: int = 1, nprobe: int = 1, probes: Optional[torch.Tensor] = None,
               refine: Optional[torch.Tensor] = None, *, rows: Optional[RowFilter] = None,
               query_keys: Optional[torch.Tensor] = None, match: str = "==") -> Tuple[torch.Tensor, torch.Tensor]:
        """`IVFFlatIndex.search` on the quantised rows: the scores are the quantised dot products of tests/ivf_i8_ref.py.

        refine: None, or the normalised fp16 corpus the index was built from (`normalize_rows(x)`, row number = id).  The k
        candidates of every query are then re-scored with their fp16 cosines (`mining.pair_scores`, cosine mode) and each
        row is re-ordered into the same total order; (-inf, -1) entries stay what they are.  No host synchronisation.
        rows, query_keys, match: the filter of `IVFFlatIndex.search`; refine re-scores the filtered candidates."""
        return self._checked_search(q, k, nprobe, probes, refine, rows=rows, query_keys=query_keys, match=match)


class IVFPQIndex(_IVFIndex):
    """`IVFFlatIndex` over product-quantised rows: d / dsub bytes per row.  A raw score is the flat index's
    score against the reconstructed row, bit for bit.  `state_dict` adds `codebooks`, and its `rows` are the uint8 codes.

    quantizer: as for `IVFFlatIndex`; pq: a `ProductQuantizer` of the same dim, or its fp16 [M, 256, dsub] codebooks."""

    _ROWS_DTYPE = torch.uint8
    _ROWS_NAME = "uint8"
    _EXTRA = ("_codebooks",)
    _HOLDS = "an IVFPQIndex holds product-quantiser codes"

    def __init__(self, quantizer: Union[SphericalKMeans, torch.Tensor], pq: Union[ProductQuantizer, torch.Tensor]):
        super().__init__(quantizer)
        if not isinstance(pq, ProductQuantizer):
            pq = ProductQuantizer(pq)
        if pq.dim != self._d:
            raise ValueError(f"the product quantiser has dim {pq.dim}, the centroids {self._d}")
        self._codebooks = pq.codebooks.clone()

    @classmethod
    def train(cls, x: torch.Tensor, n_lists: int, dsub: int = 16, n_iter: int = 10, pq_iter: int = 8, seed: int = 0):
        """Fit the coarse quantiser (spherical k-means, `n_lists` clusters, n_iter rounds) and the product quantiser (dsub
        dimensions per sub-quantiser, pq_iter Lloyd rounds) on x (fp16 / fp32 [n, d] on the device, n >= 256)."""
        _check_matrix(x, "x")
        _check_dsub(dsub, x.shape[1])
        return cls(SphericalKMeans(n_lists, n_iter=n_iter, seed=seed).fit(x),
                   ProductQuantizer.train(x, dsub=dsub, n_iter=pq_iter, seed=seed))

    @property
    def codebooks(self) -> torch.Tensor:
        return self._codebooks

    @property
    def dsub(self) -> int:
        return self._codebooks.shape[2]

    def _build_lists(self, xn, labels):
        return build_lists_pq(xn, labels, self._k, self._codebooks)

    def _encode_rows(self, prepared, labels, n):
        return pq_encode(prepared[0], self._codebooks, n), None

    def _search_lists(self, qn, probes, k, coarse, ids, keys):
        return search_lists_pq(qn, probes, self._rows, self._codebooks, self._ids if ids is None else ids, self._offsets, k, *keys)

    _BY_RESIDUAL = False  # the codes are of the rows themselves; `IVFPQResidualIndex`: of their residuals

    def _check_extra(self, state, d: int, fresh: bool):
        if "metric_l2" in state:
            raise ValueError("the state is that of an IVFPQL2Index or IVFPQResidualL2Index: its codes are of rows that are not "
                             "normalised and its scores carry a bias")
        if ("by_residual" in state) != self._BY_RESIDUAL:
            raise ValueError("the state is that of an IVFPQResidualIndex: its codes are residuals against the list centroids"
                             if "by_residual" in state else
                             "state lacks ['by_residual']: the state is that of a plain IVFPQIndex")
        codebooks = state["codebooks"]
        m, _ = _check_codebooks(codebooks, d)
        return m, {"_codebooks": codebooks.clone()}

    def search(self, q: torch.Tensor, k: int = 1, nprobe: int = 1, probes: Optional[torch.Tensor] = None,
               refine: Optional[torch.Tensor] = None, *, rows: Optional[RowFilter] = None,
               query_keys: Optional[torch.Tensor] = None, match: str = "==") -> Tuple[torch.Tensor, torch.Tensor]:
        """`IVFFlatIndex.search` on the reconstructed rows.  refine: as for `IVFInt8Index.search`, the normalised fp16 corpus
        the index was built from; the k candidates are re-scored with their fp16 cosines and re-ordered.  rows, query_keys,
        match: the filter of `IVFFlatIndex.search`."""
        return self._checked_search(q, k, nprobe, probes, refine, rows=rows, query_keys=query_keys, match=match)


class IVFPQResidualIndex(IVFPQIndex):
    """`IVFPQIndex` with every row encoded as its residual against the centroid of its list (FAISS's
    `by_residual`): the same storage, byte for byte, and the codewords describe only what the coarse quantiser has not
    already said.  A raw score is fl32(the plain scan's score against the decoded residual + the query's score against the
    list's centroid), the second term one fp32 per (query, probed list).  `state_dict` adds the marker `by_residual`, so that
    neither class loads the other's state.

    The codes hang on the bits of the centroids: a tensor given as `quantizer` is normalised (once more, if it already was),
    so a second index over the same lists is built from the fitted `SphericalKMeans` or from a state dict."""

    _BY_RESIDUAL = True
    _HOLDS = "an IVFPQResidualIndex holds product-quantiser codes of residuals"

    @classmethod
    def train(cls, x: torch.Tensor, n_lists: int, dsub: int = 16, n_iter: int = 10, pq_iter: int = 8, seed: int = 0):
        """Fit the coarse quantiser (spherical k-means, `n_lists` clusters, n_iter rounds), label the rows with their nearest
        centroid as `add` will, and fit the product quantiser on the residuals (dsub dimensions per sub-quantiser, pq_iter
        Lloyd rounds, started from the residuals of `clustering.init_rows(n, 256, seed)`); x fp16 / fp32 [n, d] on the
        device, n >= 256."""
        _check_matrix(x, "x")
        n, d = x.shape
        _check_dsub(dsub, d)
        init = init_rows(n, PQ_CODEWORDS, seed)
        km = SphericalKMeans(n_lists, n_iter=n_iter, seed=seed).fit(x)
        c16 = km._c16[:n_lists]
        xn = normalize_rows(x)
        labels = topk_normalized(xn, n, km._c16, n_lists, 1)[1][:, 0].contiguous()
        return cls(km, pq_train_residual(xn, labels, c16, dsub, init.to(device=x.device, dtype=torch.int32), pq_iter))

    def _build_lists(self, xn, labels):
        return build_lists_pq_residual(xn, labels, self._c16[: self._k], self._codebooks)

    def _encode_rows(self, prepared, labels, n):
        return pq_encode_residual(prepared[0], labels, self._c16[: self._k], self._codebooks), None

    def _search_lists(self, qn, probes, k, coarse, ids, keys):
        if coarse is None:
            coarse = self.coarse_scores(qn, probes.shape[0], probes)
        return search_lists_pq_residual(qn, probes, coarse, self._rows, self._codebooks, self._ids if ids is None else ids,
                                        self._offsets, k, *keys)

    def coarse_scores(self, qn: torch.Tensor, nq: int, probes: torch.Tensor) -> torch.Tensor:
        """fp32 [nq, nprobe]: the cosines of the first nq rows of qn (`normalize_rows`) against the centroids probes names,
        by `mining.pair_scores` in cosine mode; an entry outside [0, K) is clamped into range first (the scan does not read
        its value).  The probe's own scores (`xsim.topk_normalized`) are the tiled mining kernel's and may differ from these
        in the last place."""
        src = torch.arange(nq, device=probes.device).repeat_interleave(probes.shape[1])
        trg = probes.clamp(0, self._k - 1).reshape(-1)
        return pair_scores(qn, nq, self._c16, self._k, src, trg, None, None, "cosine").reshape(nq, probes.shape[1])

    def search(self, q: torch.Tensor, k: int = 1, nprobe: int = 1, probes: Optional[torch.Tensor] = None,
               coarse: Optional[torch.Tensor] = None, refine: Optional[torch.Tensor] = None, *,
               rows: Optional[RowFilter] = None, query_keys: Optional[torch.Tensor] = None,
               match: str = "==") -> Tuple[torch.Tensor, torch.Tensor]:
        """`IVFPQIndex.search`.  With probes None the index probes by itself and the coarse term is the score
        `xsim.topk_normalized` returns beside every list number: no extra work.  With probes given, coarse is None (computed
        by `coarse_scores`; its bits may differ from the probe's own in the last place) or device fp32 [nq, nprobe], the
        query's score against the centroid of every probed list.  refine: re-scores against the original rows, unchanged.
        rows, query_keys, match: the filter of `IVFFlatIndex.search`."""
        return self._checked_search(q, k, nprobe, probes, refine, coarse, rows, query_keys, match)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        state = super().state_dict()
        state["by_residual"] = torch.ones(1, dtype=torch.uint8, device=self._rows.device)
        return state


def _check_refine_l2(refine, d: int) -> None:
    """`refine` of an L2 quantised index's search: None, or (x16, h) as `prepare_rows` of the original corpus returns it."""
    if refine is None:
        return
    if not isinstance(refine, (tuple, list)) or len(refine) != 2:
        raise TypeError("refine must be None or the pair (rows fp16, half norms fp32) prepare_rows returned for the corpus")
    x16, h = refine
    _check_matrix(x16, "refine")
    if x16.dtype != torch.float16 or not x16.is_contiguous() or x16.shape[1] != d:
        raise ValueError(f"refine must hold the contiguous fp16 [rows, {d}] matrix prepare_rows returned")
    _check_device_tensor(h, "refine half norms")
    if h.dtype != torch.float32 or tuple(h.shape) != (x16.shape[0],) or h.device != x16.device:
        raise ValueError(f"refine must hold the fp32 [{x16.shape[0]}] half norms prepare_rows returned beside the rows")


class IVFPQL2Index(IVFFlatL2Index):
    """`IVFPQIndex` under the squared Euclidean distance, on the rows as they are (FAISS's `IVFx,PQy` with
    `METRIC_L2`): the quantiser, the probe and the results are `IVFFlatL2Index`'s, the lists hold product-quantiser codes and
    one fp32 bias per slot, -1/2 ||decoded row||^2 (`pq_l2_bias`).  A score is the flat L2 index's score against the
    reconstructed row, bit for bit, so a distance is the squared distance to that row.  `state_dict` holds `bias`,
    `codebooks` and the marker `metric_l2`; each of the four PQ classes refuses the states of the other three.

    quantizer: a fitted `clustering.KMeans`, or an [K, d] tensor of centroids (rounded to fp16, not normalised); pq: a
    `ProductQuantizer` of the same dim, or its fp16 [M, 256, dsub] codebooks (trained on rows that are not normalised)."""

    _ROWS_DTYPE = torch.uint8
    _ROWS_NAME = "uint8"
    _EXTRA = ("_codebooks",)
    _HOLDS = "an IVFPQL2Index holds product-quantiser codes of rows that are not normalised"
    _BY_RESIDUAL = False

    def __init__(self, quantizer: Union[KMeans, torch.Tensor], pq: Union[ProductQuantizer, torch.Tensor]):
        if isinstance(quantizer, SphericalKMeans) and not isinstance(quantizer, KMeans):
            raise TypeError(f"an {type(self).__name__} needs Euclidean centroids: a fitted clustering.KMeans, or a tensor")
        super().__init__(quantizer)
        if not isinstance(pq, ProductQuantizer):
            pq = ProductQuantizer(pq)
        if pq.dim != self._d:
            raise ValueError(f"the product quantiser has dim {pq.dim}, the centroids {self._d}")
        self._codebooks = pq.codebooks.clone()

    @classmethod
    def _train_codebooks(cls, x16, n: int, km: KMeans, dsub: int, init: torch.Tensor, pq_iter: int) -> torch.Tensor:
        return pq_train(x16, dsub, init, pq_iter, n)

    @classmethod
    def train(cls, x: torch.Tensor, n_lists: int, dsub: int = 16, n_iter: int = 10, pq_iter: int = 8, seed: int = 0):
        """Fit the coarse quantiser (Euclidean k-means, `n_lists` clusters, n_iter rounds) and the product quantiser (dsub
        dimensions per sub-quantiser, pq_iter Lloyd rounds from the rows `clustering.init_rows(n, 256, seed)` names) on the
        rows of x as they are (fp16 / fp32 [n, d] on the device, n >= 256).  The residual class labels the rows with their
        Euclidean nearest centroid, as `add` will, and fits the codebooks on the residuals."""
        _check_matrix(x, "x")
        n, d = x.shape
        _check_dsub(dsub, d)
        init = init_rows(n, PQ_CODEWORDS, seed).to(device=x.device, dtype=torch.int32)
        km = KMeans(n_lists, n_iter=n_iter, seed=seed).fit(x)
        return cls(km, cls._train_codebooks(prepare_rows(x)[0], n, km, dsub, init, pq_iter))

    @property
    def codebooks(self) -> torch.Tensor:
        return self._codebooks

    @property
    def dsub(self) -> int:
        return self._codebooks.shape[2]

    def _list_centroids(self) -> Optional[torch.Tensor]:
        """The centroids the codes are residuals against; None: the codes are of the rows themselves."""
        return None

    def _build_lists(self, x16, half_norms, labels):
        cent = self._list_centroids()
        codes, ids, offsets, sizes = (build_lists_pq(x16, labels, self._k, self._codebooks) if cent is None else
                                      build_lists_pq_residual(x16, labels, cent, self._codebooks))
        bias = pq_l2_bias(codes, self._codebooks, None, cent, ids=ids, offsets=None if cent is None else offsets)
        return codes, bias, ids, offsets, sizes

    def _encode_rows(self, prepared, labels, n):
        cent = self._list_centroids()
        if cent is None:
            codes = pq_encode(prepared[0], self._codebooks, n)
            return codes, pq_l2_bias(codes, self._codebooks)
        codes = pq_encode_residual(prepared[0], labels, cent, self._codebooks)
        return codes, pq_l2_bias(codes, self._codebooks, labels, cent)

    def _scan(self, q16, nq: int, probes, k: int, coarse, ids):
        return search_lists_pq_l2(q16, probes, self._rows, self._codebooks, self._bias, self._ids if ids is None else ids,
                                  self._offsets, k)

    def _search_l2(self, q, k, nprobe, probes, coarse, rows, query_keys, refine):
        if query_keys is not None:
            raise TypeError("query_keys: the keyed scan has no L2 twin (DESIGN.md 7); filter with rows=index.row_filter(mask=...)")
        _check_refine_l2(refine, self._d)
        nq = self._check_search(q, k, nprobe, probes)
        ids = self._filter(rows, None, "==", nq)[0]
        if coarse is not None:
            if probes is None:
                raise ValueError("coarse belongs to probes: give both, or neither")
            _check_coarse(coarse, probes.shape)
        q16, hq = prepare_rows(q)
        if probes is None:
            coarse, probes = self._nearest_lists(q16, nq, nprobe)
        score, idx = self._scan(q16, nq, probes, k, coarse, ids)
        if refine is not None:
            score, idx = refine_candidates_l2(q16, nq, refine[0], refine[1], idx)
        return (2.0 * (hq[:nq, None] - score)).clamp_min(0.0), idx

    def search(self, q: torch.Tensor, k: int = 1, nprobe: int = 1, probes: Optional[torch.Tensor] = None, refine=None, *,
               rows: Optional[RowFilter] = None, query_keys=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """`IVFFlatL2Index.search` on the reconstructed rows: (squared distances fp32 [nq, k] ascending, ids int32 [nq, k]),
        ties to the lower row number, (+inf, -1) where the probed lists hold fewer than k rows; sq_dist = clamp_min(2 (h_q -
        score), 0), score the flat L2 scan's against the decoded row, bit for bit.  k, nprobe <= 8; probes and rows (a
        `RowFilter` built with a mask) as there.

        refine: None, or `prepare_rows(x)` of the corpus the index was built from -- the pair (rows fp16, half norms fp32),
        row number = id.  The k candidates are re-scored as fl32(q . x[id] - h[id]) (`mining.pair_scores` in cosine mode,
        which on prepared rows is a plain dot product) and re-ordered by the two stable sorts of `refine_candidates`; the
        distances returned are then those to the fp16 rows.  No kernel of its own, no host synchronisation."""
        return self._search_l2(q, k, nprobe, probes, None, rows, query_keys, refine)

    @property
    def centroids_normalized(self) -> torch.Tensor:
        raise TypeError(f"an {type(self).__name__} keeps its centroids as they are: centroids_f16")

    def range_search(self, *args, **kwargs):
        raise TypeError(f"range_search needs the fp16 lists of an IVFFlatIndex; {self._HOLDS}")

    def probe_wide(self, *args, **kwargs):
        raise TypeError(f"probe_wide is the paged cosine top-k; an {type(self).__name__} probes at most 8 lists (DESIGN.md 7)")

    def search_wide(self, *args, **kwargs):
        raise TypeError(f"search_wide needs the fp16 lists of an IVFFlatIndex; {self._HOLDS}")

    def self_join(self, *args, **kwargs):
        raise TypeError(f"self_join and semdedup need the fp16 lists of an IVFFlatIndex; {self._HOLDS}")

    def _check_extra(self, state, d: int, fresh: bool):
        if "metric_l2" not in state:
            raise ValueError("state lacks ['metric_l2']: the state is that of an IVFPQIndex or IVFPQResidualIndex, whose rows "
                             "are normalised")
        if ("by_residual" in state) != self._BY_RESIDUAL:
            raise ValueError("the state is that of an IVFPQResidualL2Index: its codes are residuals against the list centroids"
                             if "by_residual" in state else
                             "state lacks ['by_residual']: the state is that of a plain IVFPQL2Index")
        codebooks = state["codebooks"]
        m, _ = _check_codebooks(codebooks, d)
        return m, {"_codebooks": codebooks.clone()}

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """`IVFPQIndex.state_dict` (rows: the uint8 codes; codebooks) with the centroids as they are, `bias` (fp32 [slots]),
        the marker `metric_l2` and, for the residual class, the marker `by_residual`."""
        state = super().state_dict()
        if self._BY_RESIDUAL:
            state["by_residual"] = torch.ones(1, dtype=torch.uint8, device=self._rows.device)
        return state


class IVFPQResidualL2Index(IVFPQL2Index):
    """`IVFPQL2Index` with every row encoded as its residual against the Euclidean centroid of its list (DESIGN.md 3.30;
    FAISS's `IVFx,PQy` with `METRIC_L2` and `by_residual`, its default): the row a slot stands for is c + r^, the slot's bias
    is -(c . r^ + 1/2 ||r^||^2), and a score is fl32(fl32(sum + bias) + coarse), coarse the biased score of the query against
    the list's centroid that the L2 probe has already computed.  The same storage as the plain class, byte for byte in its
    layout.  The codes and the bias hang on the bits of the fp16 centroids."""

    _BY_RESIDUAL = True
    _HOLDS = "an IVFPQResidualL2Index holds product-quantiser codes of residuals of rows that are not normalised"

    @classmethod
    def _train_codebooks(cls, x16, n: int, km: KMeans, dsub: int, init: torch.Tensor, pq_iter: int) -> torch.Tensor:
        k = km.n_clusters
        labels = topk_bias_prepared(x16, n, km._c16, k, km._ch.neg(), 1)[1][:, 0].contiguous()
        return pq_train_residual(x16, labels, km._c16[:k], dsub, init, pq_iter)

    def _list_centroids(self) -> torch.Tensor:
        return self._c16[: self._k]

    def coarse_scores(self, q16: torch.Tensor, nq: int, probes: torch.Tensor) -> torch.Tensor:
        """fp32 [nq, nprobe]: fl32(q . c - h_c) of the first nq rows of q16 (`prepare_rows`) against the centroids probes
        names, the dot products by `mining.pair_scores` in cosine mode; an entry outside [0, K) is clamped into range first
        (the scan does not read its value).  The probe's own scores (`xsim.topk_bias_prepared`) are the tiled kernel's and
        may differ from these in the last place."""
        src = torch.arange(nq, device=probes.device).repeat_interleave(probes.shape[1])
        trg = probes.clamp(0, self._k - 1).reshape(-1)
        dots = pair_scores(q16, nq, self._c16, self._k, src, trg, None, None, "cosine")
        return (dots - self._ch[trg.long()]).reshape(nq, probes.shape[1])

    def _scan(self, q16, nq: int, probes, k: int, coarse, ids):
        if coarse is None:
            coarse = self.coarse_scores(q16, nq, probes)
        return search_lists_pq_l2(q16, probes, self._rows, self._codebooks, self._bias, self._ids if ids is None else ids,
                                  self._offsets, k, coarse)

    def search(self, q: torch.Tensor, k: int = 1, nprobe: int = 1, probes: Optional[torch.Tensor] = None,
               coarse: Optional[torch.Tensor] = None, refine=None, *, rows: Optional[RowFilter] = None,
               query_keys=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """`IVFPQL2Index.search`; a distance is the squared distance to c + r^.  With probes None the index probes by itself
        and the coarse term is the biased score `xsim.topk_bias_prepared` returns beside every list number: no extra work.
        With probes given, coarse is None (computed by `coarse_scores`; its bits may differ from the probe's own in the last
        place) or device fp32 [nq, nprobe], fl32(q . c - h_c) for the centroid of every probed list."""
        return self._search_l2(q, k, nprobe, probes, coarse, rows, query_keys, refine)


def refine_candidates(qn: torch.Tensor, nq: int, xn: torch.Tensor, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The candidates idx (int32 [nq, k], -1 = none) of the first nq rows of qn re-scored with their fp16 cosines against the
    rows of xn (both from `normalize_rows`) and every row re-ordered into the total order: (scores fp32 [nq, k], ids int32
    [nq, k]).  `mining.pair_scores` in cosine mode and two stable sorts; an empty entry never reaches the kernel's NaN path
    (it scores row 0 and is overwritten with -inf)."""
    k = idx.shape[1]
    have = idx >= 0
    src = torch.arange(nq, device=idx.device).repeat_interleave(k)
    trg = torch.where(have, idx, torch.zeros_like(idx)).reshape(-1)
    cos = pair_scores(qn, nq, xn, xn.shape[0], src, trg, None, None, "cosine").reshape(nq, k)
    return _total_order(torch.where(have, cos, torch.full_like(cos, float("-inf"))), idx)


def _total_order(score: torch.Tensor, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Every row of (score, idx) [nq, k] in the total order, score descending and ties to the lower id: two stable sorts."""
    by_id = torch.sort(idx, dim=1, stable=True)[1]  # then a stable sort by score: ties go to the lower id
    score, idx = torch.gather(score, 1, by_id), torch.gather(idx, 1, by_id)
    order = torch.sort(score, dim=1, descending=True, stable=True)[1]
    return torch.gather(score, 1, order), torch.gather(idx, 1, order)


def refine_candidates_l2(q16: torch.Tensor, nq: int, x16: torch.Tensor, half_norms: torch.Tensor,
                         idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """`refine_candidates` under L2: the candidates idx (int32 [nq, k], -1 = none) of the first nq rows of q16
    re-scored as fl32(q . x[id] - half_norms[id]) against the prepared corpus (x16, half_norms of `prepare_rows`) and every
    row re-ordered into the total order: (scores fp32 [nq, k], ids int32 [nq, k]); ||q - x||^2 = 2 (h_q - score).  The dot
    product is `mining.pair_scores` in cosine mode, which on prepared rows divides by nothing."""
    k = idx.shape[1]
    have = idx >= 0
    src = torch.arange(nq, device=idx.device).repeat_interleave(k)
    trg = torch.where(have, idx, torch.zeros_like(idx)).reshape(-1)
    dot = pair_scores(q16, nq, x16, x16.shape[0], src, trg, None, None, "cosine").reshape(nq, k)
    score = dot - half_norms[trg.long()].reshape(nq, k)
    return _total_order(torch.where(have, score, torch.full_like(score, float("-inf"))), idx)


class PreTransformIndex:
    """An index behind a linear transform (FAISS's `IndexPreTransform`): `add` stores
    `transform.apply(x)`, every query is transformed once, and the wrapped index does the rest, unchanged -- a wrapped search
    equals `index.search(transform.apply(q), ...)` bit for bit, and every argument of the wrapped class passes through.

    transform: a `sonar_amd.transforms.LinearTransform` (`PCA`, `OPQ`) whose d_out is the index's dim; index: one of the four
    IVF classes or of their L2 counterparts, before or after its `add`."""

    def __init__(self, transform, index: _IVFIndex):
        from .transforms import LinearTransform

        if not isinstance(transform, LinearTransform):
            raise TypeError("transform must be a sonar_amd.transforms.LinearTransform")
        if not isinstance(index, _IVFIndex):
            raise TypeError("index must be an IVFFlatIndex, IVFInt8Index, IVFPQIndex or IVFPQResidualIndex")
        if transform.d_out != index.dim:
            raise ValueError(f"the transform gives dim {transform.d_out}, the index takes {index.dim}")
        self.transform, self.index = transform, index

    @property
    def dim(self) -> int:
        """The dimension of the rows and queries this index takes: the transform's d_in."""
        return self.transform.d_in

    @property
    def n_lists(self) -> int:
        return self.index.n_lists

    @property
    def ntotal(self) -> int:
        return self.index.ntotal

    @property
    def list_sizes(self) -> torch.Tensor:
        return self.index.list_sizes

    @property
    def list_offsets(self) -> torch.Tensor:
        return self.index.list_offsets

    def add(self, x: torch.Tensor, labels: Optional[torch.Tensor] = None):
        """`index.add(transform.apply(x), labels)`; x fp16 / fp32 [n, d_in] on the device."""
        self.index.add(self.transform.apply(x), labels)
        return self

    def extend(self, x: torch.Tensor, labels: Optional[torch.Tensor] = None, first_id: Optional[int] = None):
        """`index.extend(transform.apply(x), labels, first_id)`."""
        self.index.extend(self.transform.apply(x), labels, first_id)
        return self

    def remove(self, ids: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
        self.index.remove(ids, mask)
        return self

    def merge_from(self, other, add_id: Optional[int] = None):
        """`index.merge_from(other.index, add_id)`; other: a `PreTransformIndex` with the same transform matrix and offset,
        bit for bit (`torch.equal` reads back)."""
        if not isinstance(other, PreTransformIndex):
            raise TypeError(f"merge_from: a PreTransformIndex takes a PreTransformIndex, got {type(other).__name__}")
        if other is self:
            raise ValueError("merge_from: an index cannot be merged into itself")
        mine, theirs = self.transform.state_dict(), other.transform.state_dict()
        if set(mine) != set(theirs) or any(mine[k].shape != theirs[k].shape or not torch.equal(mine[k], theirs[k]) for k in mine):
            raise ValueError("merge_from: the other index has another transform; merged lists need the same one, bit for bit")
        self.index.merge_from(other.index, add_id)
        return self

    def probe(self, q: torch.Tensor, nprobe: int = 1) -> torch.Tensor:
        return self.index.probe(self.transform.apply(q), nprobe)

    def row_filter(self, keys: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> RowFilter:
        return self.index.row_filter(keys, mask)

    def search(self, q: torch.Tensor, k: int = 1, nprobe: int = 1, probes: Optional[torch.Tensor] = None, *,
               refine: Optional[torch.Tensor] = None, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """`index.search(transform.apply(q), k, nprobe, probes, **kwargs)`; q fp16 / fp32 [nq, d_in] on the device.  Whatever
        the wrapped class takes behind probes (coarse, rows, query_keys, match) goes by keyword.

        refine (by keyword, on every wrapped class): None, or the normalised fp16 corpus in the ORIGINAL space
        (`normalize_rows(x)` of the x `add` was given, [rows, d_in]): the candidates of the wrapped search are re-scored with
        the cosines of the untransformed q against those rows and re-ordered (`refine_candidates`), so the scores are what
        `xsim.topk` would return for the pair, whatever the transform lost.  The wrapped class's own `refine` (re-scoring in
        the transformed space, against the transformed corpus) is not reachable through the wrapper: call
        `index.search(transform.apply(q), ..., refine=)` for that."""
        if refine is not None:
            if isinstance(self.index, IVFFlatL2Index):
                raise TypeError("refine re-scores with cosines in the original space; the wrapped index scores squared "
                                "distances: call index.search(transform.apply(q), refine=prepare_rows(transform.apply(x)))")
            _check_refine(refine, self.dim)
        qt = self.transform.apply(q)
        score, idx = self.index.search(qt, k, nprobe, probes, **kwargs)
        return (score, idx) if refine is None else refine_candidates(normalize_rows(q), q.shape[0], refine, idx)

    def probe_wide(self, q: torch.Tensor, nprobe: int = PAGE) -> torch.Tensor:
        return self.index.probe_wide(self.transform.apply(q), nprobe)

    def search_wide(self, q: torch.Tensor, k: int = PAGE, nprobe: int = PAGE, probes: Optional[torch.Tensor] = None,
                    **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """`index.search_wide(transform.apply(q), k, nprobe, probes, **kwargs)`: the wrapped index must be an
        `IVFFlatIndex`."""
        if not hasattr(self.index, "search_wide"):
            raise TypeError("search_wide needs the fp16 lists of an IVFFlatIndex")
        return self.index.search_wide(self.transform.apply(q), k, nprobe, probes, **kwargs)

    def range_search(self, q: torch.Tensor, *args, **kwargs) -> RangeResult:
        """`index.range_search(transform.apply(q), ...)`: the thresholds are cosines in the transformed space."""
        return self.index.range_search(self.transform.apply(q), *args, **kwargs)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The transform's state under `transform.*` and the index's under `index.*`."""
        return {**{"transform." + k: v for k, v in self.transform.state_dict().items()},
                **{"index." + k: v for k, v in self.index.state_dict().items()}}

    @classmethod
    def from_state_dict(cls, state: Dict[str, torch.Tensor], index_cls):
        """index_cls: the class of the wrapped index (its state does not name it).  The transform comes back as a plain
        `LinearTransform` with the same bits."""
        from .transforms import LinearTransform

        if not (isinstance(index_cls, type) and issubclass(index_cls, _IVFIndex)):
            raise TypeError("index_cls must be one of the IVF index classes")
        part = lambda prefix: {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}
        return cls(LinearTransform.from_state_dict(part("transform.")), index_cls.from_state_dict(part("index.")))
