"""xsim cosine / margin mining on the MI355X engine.

The reference names xsim as SONAR's evaluation (README.md:5) and computes
similarities as `F.normalize(x) @ F.normalize(y).T`
(tests/integration_tests/test_text_sonar.py:42-53, examples/sonar_text_demo.ipynb).
Here the similarity matrix is never materialised: `smi_xsim_topk` streams
256x256 score tiles out of the MFMA pipeline into a running top-k.
`topk_int8` / `topk_int8_normalized` run the same walk on int8 codes with one
scale per row (`smi_xsim_topk_i8`): the integer MFMA on half
the bytes, scores specified to their bits, optionally re-scored as fp16 cosines.
`topk_wide` / `topk_wide_normalized` return up to 64 neighbours as pages of 16
(`topk_page_normalized`, `smi_xsim_topk_page`): a page is the 16
best candidates strictly after a per-row exclusive ceiling in the total order, and
the pages concatenated are the top-k bit for bit; `topk` keeps its limit of 8.
`topk_l2` / `topk_ip` search rows AS THEY ARE (SONAR embeddings are not unit vectors): squared Euclidean
distance through one additive term per y row, -||y||^2 / 2, inside the same walk (`smi_l2_topk`), and maximum inner product
through the existing pass, which never needed unit rows.

Multi-GPU (sharded_topk): X rows are sharded over ranks, every rank's Y shard
is all-gathered once over RCCL/xGMI (2 GB for 1M x 1024 fp16 -- small next to
288 GB HBM), then each rank mines its X shard against all of Y with no further
exchange; margin scoring needs one more all-gather of the k-NN means.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib


def _prep(t: torch.Tensor) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError("xsim runs on a HIP device only (no CPU path); move the embeddings to cuda")
    if t.dim() != 2:
        raise ValueError("embeddings must be [rows, dim]")
    if t.dtype not in (torch.float16, torch.float32):
        t = t.float()
    return t.contiguous()


def normalize_rows(t: torch.Tensor) -> torch.Tensor:
    """fp16 L2-normalised copy, zero-padded to a multiple of 256 rows (engine layout)."""
    t = _prep(t)
    lib = _lib.load()
    rows, d = t.shape
    if rows == 0:
        raise ValueError("empty embedding matrix")
    pad = int(lib.smi_xsim_padded_rows(rows))
    out = torch.empty((pad, d), dtype=torch.float16, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(lib.smi_xsim_normalize(t.data_ptr(), _lib.SMI_F32 if t.dtype == torch.float32 else _lib.SMI_F16,
                                          rows, d, out.data_ptr(), _lib.current_stream_ptr()))
    return out


def _call_topk(entry: str, sizing: str, shape, dev, nx: int, k: int, *front, ws: Optional[torch.Tensor] = None):
    """A top-k entry of the C ABI on the current stream: `front`, its arguments up to the outputs, then idx int32 [nx, k],
    score fp32 [nx, k] and the workspace -- `ws`, or a fresh one of `sizing(*shape)` bytes.  Returns (score, idx)."""
    lib = _lib.load()
    if ws is None:
        ws = torch.empty(int(getattr(lib, sizing)(*shape)), dtype=torch.uint8, device=dev)
    idx = torch.empty((nx, k), dtype=torch.int32, device=dev)
    score = torch.empty((nx, k), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, entry)(*front, idx.data_ptr(), score.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _lib.current_stream_ptr()))
    return score, idx


def topk_normalized(xn: torch.Tensor, nx: int, yn: torch.Tensor, ny: int, k: int = 1,
                    y_index_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Mine on already normalised + padded matrices (see normalize_rows)."""
    d = xn.shape[1]
    if yn.shape[1] != d:
        raise ValueError("x and y must have the same dimension")
    if not 1 <= k <= 8:
        raise ValueError("k must be in [1, 8]")
    return _call_topk("smi_xsim_topk", "smi_xsim_workspace_bytes", (nx, ny, k, d), xn.device, nx, k,
                      xn.data_ptr(), nx, yn.data_ptr(), ny, d, k, y_index_offset)


def topk(x: torch.Tensor, y: torch.Tensor, k: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """For every row of x: (cosine scores [nx,k] fp32, indices into y [nx,k] int32), best first."""
    xn, yn = normalize_rows(x), normalize_rows(y)
    return topk_normalized(xn, x.shape[0], yn, y.shape[0], k)


# ---- squared-Euclidean and inner-product search on rows as they are ----

def prepare_rows(t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(fp16 copy zero-padded to a multiple of 256 rows, half norms fp32 [padded rows]): `normalize_rows` without the
    division, and h[r] = fl32(sum of the squares of the rounded row / 2), summed in fp64 in a fixed order (smi_l2_prepare);
    pad rows and their half norms are 0.  A value that is not finite in fp16 gives unspecified results."""
    t = _prep(t)
    rows, d = t.shape
    if rows == 0:
        raise ValueError("empty embedding matrix")
    if d % 8:
        raise ValueError(f"dim = {d} must be a multiple of 8")
    lib = _lib.load()
    pad = int(lib.smi_xsim_padded_rows(rows))
    out = torch.empty((pad, d), dtype=torch.float16, device=t.device)
    half_norms = torch.empty((pad,), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(lib.smi_l2_prepare(t.data_ptr(), _lib.SMI_F32 if t.dtype == torch.float32 else _lib.SMI_F16, rows, d,
                                      out.data_ptr(), half_norms.data_ptr(), _lib.current_stream_ptr()))
    return out, half_norms


def _check_prepared(rows16, n, name: str) -> int:
    """One side of a prepared call: the contiguous fp16 [padded n, dim] matrix on the device -> its padded row count."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"n{name} = {n!r}: at least one row")
    if not isinstance(rows16, torch.Tensor):
        raise TypeError(f"{name}16 must be a torch.Tensor")
    if not rows16.is_cuda:
        raise RuntimeError("xsim runs on a HIP device only (no CPU path); move the rows to cuda")
    pad = (n + 255) // 256 * 256
    if rows16.dim() != 2 or rows16.dtype != torch.float16 or not rows16.is_contiguous() or rows16.shape[0] != pad:
        raise ValueError(f"{name}16 must be the contiguous fp16 [{pad}, dim] matrix prepare_rows returns for {n} rows, got "
                         f"{rows16.dtype} {list(rows16.shape)}")
    return pad


def _check_per_row(v, pad: int, like: torch.Tensor, name: str) -> None:
    """A per-row fp32 vector of a prepared call (a bias, half norms): contiguous fp32 [pad] on the device of the rows."""
    if not isinstance(v, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not v.is_cuda:
        raise RuntimeError(f"xsim runs on a HIP device only (no CPU path); move {name} to cuda")
    if v.dtype != torch.float32 or tuple(v.shape) != (pad,) or not v.is_contiguous():
        raise ValueError(f"{name} must be contiguous fp32 [{pad}] (one per padded row), got {v.dtype} {list(v.shape)}")
    if v.device != like.device:
        raise ValueError(f"{name} ({v.device}) must be on the device of the rows ({like.device})")


def topk_bias_prepared(x16: torch.Tensor, nx: int, y16: torch.Tensor, ny: int, bias: torch.Tensor, k: int = 1,
                       y_index_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """`topk_normalized` with one additive fp32 term per y row (smi_l2_topk): score(i, j) = fl32(x_i . y_j + bias[j]) on
    fp16 rows in the padded layout, bias fp32 [padded ny] and finite; same order and fill, a zero score is +0."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 8:
        raise ValueError("k must be in [1, 8]")
    _check_prepared(x16, nx, "x")
    pad_y = _check_prepared(y16, ny, "y")
    d = x16.shape[1]
    if y16.shape[1] != d:
        raise ValueError("x and y must have the same dimension")
    if y16.device != x16.device:
        raise ValueError("x and y must be on the same device")
    if d % 64:
        raise ValueError(f"dim = {d} must be a multiple of 64")
    _check_per_row(bias, pad_y, x16, "bias")
    return _call_topk("smi_l2_topk", "smi_l2_topk_ws_bytes", (nx, ny, k, d), x16.device, nx, k,
                      x16.data_ptr(), nx, y16.data_ptr(), ny, d, k, y_index_offset, bias.data_ptr())


def topk_l2_prepared(x16: torch.Tensor, nx: int, x_half_norms: torch.Tensor, y16: torch.Tensor, ny: int,
                     y_half_norms: torch.Tensor, k: int = 1,
                     y_index_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Squared-Euclidean nearest neighbours on prepared sides (`prepare_rows`) -> (sq_dist fp32 [nx, k] ascending, idx int32
    [nx, k], the raw scores).  score(i, j) = fl32(x_i . y_j - h_y[j]) from `topk_bias_prepared`, so best first is nearest
    first (ties to the lower index), and sq_dist = clamp_min(2 (h_x[i] - score), 0) in fp32 torch ops; fill (+inf, -1)."""
    pad_x = _check_prepared(x16, nx, "x")
    _check_per_row(x_half_norms, pad_x, x16, "x_half_norms")
    _check_per_row(y_half_norms, _check_prepared(y16, ny, "y"), x16, "y_half_norms")
    score, idx = topk_bias_prepared(x16, nx, y16, ny, y_half_norms.neg(), k, y_index_offset)
    sq_dist = (2.0 * (x_half_norms[:nx, None] - score)).clamp_min(0.0)
    return sq_dist, idx, score


def topk_l2(x: torch.Tensor, y: torch.Tensor, k: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """For every row of x: (squared Euclidean distances [nx, k] fp32 ascending, indices into y [nx, k] int32), between the
    fp16 roundings of the rows as they are (`topk_l2_prepared`); fill (+inf, -1)."""
    (x16, hx), (y16, hy) = prepare_rows(x), prepare_rows(y)
    sq_dist, idx, _ = topk_l2_prepared(x16, x.shape[0], hx, y16, y.shape[0], hy, k)
    return sq_dist, idx


def topk_ip(x: torch.Tensor, y: torch.Tensor, k: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """Maximum inner product on rows as they are: (x_i . y_j [nx, k] fp32 best first, indices into y).  Prepared rows
    (`prepare_rows`) through the existing `topk_normalized`: that pass never needed unit rows -- its score is the fp32 sum
    of the fp16 products, whatever the rows' lengths -- so the zero-bias case takes no new kernel."""
    (x16, _), (y16, _) = prepare_rows(x), prepare_rows(y)
    return topk_normalized(x16, x.shape[0], y16, y.shape[0], k)


PAGE = 16      # results of one page: the list length of the paged pass
WIDE_MAX = 64  # the most a wide call returns: four pages


def check_count(v, name: str, most: int) -> None:
    """k or nprobe of a paged call: a Python int in [1, most]."""
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= most:
        raise ValueError(f"{name} = {v!r}: an integer in [1, {most}]")


def check_below(below, n: int, like: Optional[torch.Tensor] = None):
    """The ceilings of a page: None, or (scores fp32 [n], ids int32 [n]) on the device (of `like`) -> contiguous tensors."""
    if below is None:
        return None
    if not isinstance(below, (tuple, list)) or len(below) != 2 or not all(isinstance(t, torch.Tensor) for t in below):
        raise TypeError("below must be None or a (scores, ids) pair of tensors: one exclusive ceiling per row")
    cs, ci = below
    if cs.dtype != torch.float32 or tuple(cs.shape) != (n,):
        raise ValueError(f"below: scores must be fp32 [{n}], got {cs.dtype} {list(cs.shape)}")
    if ci.dtype != torch.int32 or tuple(ci.shape) != (n,):
        raise ValueError(f"below: ids must be int32 [{n}], got {ci.dtype} {list(ci.shape)}")
    if not cs.is_cuda or not ci.is_cuda:
        raise RuntimeError("below: the ceilings must be on the HIP device (no CPU path)")
    if cs.device != ci.device or (like is not None and cs.device != like.device):
        raise ValueError(f"below: scores ({cs.device}) and ids ({ci.device}) must be on the device of the rows"
                         + (f" ({like.device})" if like is not None else ""))
    return cs.contiguous(), ci.contiguous()


def page_sizes(k: int):
    """The pages of a wide call for k results: 16, 16, ..., and what is left."""
    return [min(PAGE, k - done) for done in range(0, k, PAGE)]


def last_entry(score: torch.Tensor, idx: torch.Tensor):
    """The ceiling of the next page: the last entry of every row of this one (a fill entry, id -1, exhausts the row)."""
    return score[:, -1].contiguous(), idx[:, -1].contiguous()


def topk_page_normalized(xn: torch.Tensor, nx: int, yn: torch.Tensor, ny: int, k: int = PAGE, y_index_offset: int = 0,
                         below=None, _ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One page of the top-k (smi_xsim_topk_page): `topk_normalized` for k <= 16, and with below =
    (scores fp32 [nx], ids int32 [nx]) the k best candidates strictly AFTER each row's exclusive ceiling in the total order
    (score descending, ties to the lower id; ids as returned, y_index_offset included).  A row whose ceiling id is negative
    is exhausted: only fill, (-inf, -1).  A ceiling need not be a candidate.  Nothing is read back."""
    check_count(k, "k", PAGE)
    below = check_below(below, nx, xn if isinstance(xn, torch.Tensor) and xn.is_cuda else None)
    d = xn.shape[1]
    if yn.shape[1] != d:
        raise ValueError("x and y must have the same dimension")
    return _call_topk("smi_xsim_topk_page", "smi_xsim_topk_page_ws_bytes", (nx, ny, k, d), xn.device, nx, k,
                      xn.data_ptr(), nx, yn.data_ptr(), ny, d, k, y_index_offset,
                      below[0].data_ptr() if below else None, below[1].data_ptr() if below else None, ws=_ws)


def concat_pages(page, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """A wide call for k results: page(kp, below) -> (score, idx) over `page_sizes(k)`, every page under the last entry of
    the one before as its ceiling (the first under None), concatenated on the device."""
    pages, below = [], None
    for kp in page_sizes(k):
        pages.append(page(kp, below))
        below = last_entry(*pages[-1])
    if len(pages) == 1:
        return pages[0]
    return torch.cat([p[0] for p in pages], 1), torch.cat([p[1] for p in pages], 1)


def topk_wide_normalized(xn: torch.Tensor, nx: int, yn: torch.Tensor, ny: int, k: int = PAGE,
                         y_index_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """`topk_normalized` for k up to 64, in ceil(k / 16) pages (`topk_page_normalized`): every page takes the last entry of
    the one before as its ceiling, the last page asks only for what is left, and the pages are concatenated on the device.
    The result is the top-k in the total order, bit for bit the same however it is split; one pass over y per page."""
    check_count(k, "k", WIDE_MAX)
    lib = _lib.load()
    ws = torch.empty(int(lib.smi_xsim_topk_page_ws_bytes(nx, ny, PAGE, xn.shape[1])), dtype=torch.uint8, device=xn.device)
    return concat_pages(lambda kp, below: topk_page_normalized(xn, nx, yn, ny, kp, y_index_offset, below, _ws=ws), k)


def topk_wide(x: torch.Tensor, y: torch.Tensor, k: int = PAGE) -> Tuple[torch.Tensor, torch.Tensor]:
    """`topk` for k up to 64 (`topk_wide_normalized`)."""
    check_count(k, "k", WIDE_MAX)
    xn, yn = normalize_rows(x), normalize_rows(y)
    return topk_wide_normalized(xn, x.shape[0], yn, y.shape[0], k)


PRECISIONS = ("fp16", "int8")


def check_precision(precision) -> None:
    if precision not in PRECISIONS:
        raise ValueError(f"precision {precision!r}: expected one of {PRECISIONS}")


def _check_int8_side(rows16, enc, n: int, name: str, need_rows: bool):
    """One side of topk_int8_normalized: the fp16 rows (None allowed where nothing reads them) and the optional
    (codes, scales) -> (padded row count, d, device); everything that can be refused without a kernel."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"n{name} = {n!r}: at least one row")
    pad = (n + 255) // 256 * 256
    ref = None
    if rows16 is not None:
        if not isinstance(rows16, torch.Tensor):
            raise TypeError(f"{name}n must be a torch.Tensor")
        if not rows16.is_cuda:
            raise RuntimeError("xsim runs on a HIP device only (no CPU path); move the embeddings to cuda")
        if rows16.dim() != 2 or rows16.dtype != torch.float16 or not rows16.is_contiguous() or rows16.shape[0] != pad:
            raise ValueError(f"{name}n must be the contiguous fp16 [{pad}, dim] matrix normalize_rows returns for {n} rows, got "
                             f"{rows16.dtype} {list(rows16.shape)}")
        ref = rows16
    elif need_rows or enc is None:
        raise ValueError(f"{name}n is needed: the fp16 rows are what is encoded and what refine re-scores")
    if enc is not None:
        if not isinstance(enc, (tuple, list)) or len(enc) != 2 or not all(isinstance(t, torch.Tensor) for t in enc):
            raise TypeError(f"{name}_enc must be the (codes, scales) pair index.encode_rows_int8 returns")
        codes, scales = enc
        if not codes.is_cuda or not scales.is_cuda:
            raise RuntimeError("xsim runs on a HIP device only (no CPU path); move the codes and scales to cuda")
        if codes.dtype != torch.int8 or codes.dim() != 2 or codes.shape[0] != pad or not codes.is_contiguous() or (
                ref is not None and codes.shape[1] != ref.shape[1]):
            raise ValueError(f"{name}_enc codes must be contiguous int8 [{pad}, dim] (the whole padded matrix encoded), got "
                             f"{codes.dtype} {list(codes.shape)}")
        if scales.dtype != torch.float32 or tuple(scales.shape) != (pad,) or not scales.is_contiguous():
            raise ValueError(f"{name}_enc scales must be contiguous fp32 [{pad}], got {scales.dtype} {list(scales.shape)}")
        ref = ref if ref is not None else codes
        if codes.device != ref.device or scales.device != ref.device:
            raise ValueError(f"{name}_enc codes ({codes.device}) and scales ({scales.device}) must be on the device of "
                             f"{name}'s rows ({ref.device})")
    d = ref.shape[1]
    if d % 64:
        raise ValueError(f"dim = {d} must be a multiple of 64")
    return d, ref.device


def topk_int8_normalized(xn: Optional[torch.Tensor], nx: int, yn: Optional[torch.Tensor], ny: int, k: int = 1, *,
                         refine: bool = True, candidates: int = 8, x_enc=None, y_enc=None,
                         y_index_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """topk_normalized on int8 rows (smi_xsim_topk_i8): both sides are encoded with one scale per row
    (index.encode_rows_int8 over the whole padded matrix; pass x_enc / y_enc = that pair to encode a corpus once) and scored
    as the int8 IVF index scores, fl32(fl32((float)(integer dot product) * scale_y) * scale_x) -- the same bits for the same
    two rows.  refine=True: the int8 pass returns `candidates` rows (k <= candidates <= 8), index.refine_candidates re-scores
    them with their fp16 cosines (mining.pair_scores) and re-orders them, and the first k are returned: scores are then the
    fp16 pair cosines in total order.  refine=False: the k best int8 scores (xn / yn may be None beside x_enc / y_enc)."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 8:
        raise ValueError("k must be in [1, 8]")
    if isinstance(candidates, bool) or not isinstance(candidates, int) or not k <= candidates <= 8:
        raise ValueError(f"candidates = {candidates!r}: an integer in [k, 8] = [{k}, 8]")
    d, dev = _check_int8_side(xn, x_enc, nx, "x", bool(refine))
    dy, devy = _check_int8_side(yn, y_enc, ny, "y", bool(refine))
    if dy != d:
        raise ValueError("x and y must have the same dimension")
    if devy != dev:
        raise ValueError("x and y must be on the same device")
    from . import index  # (index imports this module)

    index._check_int8_dim(d)
    xc, xs = x_enc if x_enc is not None else index.encode_rows_int8(xn)
    yc, ys = y_enc if y_enc is not None else index.encode_rows_int8(yn)
    kk = candidates if refine else k
    # (the workspace: int8 [rows, d] is fp16 [rows, d / 2] in bytes)
    score, idx = _call_topk("smi_xsim_topk_i8", "smi_xsim_workspace_bytes", (nx, ny, kk, d // 2), dev, nx, kk,
                            xc.data_ptr(), xs.data_ptr(), nx, yc.data_ptr(), ys.data_ptr(), ny, d, kk,
                            0 if refine else y_index_offset)
    if not refine:
        return score, idx
    score, idx = index.refine_candidates(xn, nx, yn, idx)
    score, idx = score[:, :k].contiguous(), idx[:, :k].contiguous()
    if y_index_offset:
        idx = torch.where(idx >= 0, idx + y_index_offset, idx)
    return score, idx


def topk_int8(x: torch.Tensor, y: torch.Tensor, k: int = 1, refine: bool = True,
              candidates: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
    """`topk` through the int8 pass (topk_int8_normalized): half the operand bytes and the integer MFMA; with refine the
    scores are the fp16 cosines of the returned rows."""
    xn, yn = normalize_rows(x), normalize_rows(y)
    return topk_int8_normalized(xn, x.shape[0], yn, y.shape[0], k, refine=refine, candidates=candidates)


def merge_topk(part_scores: torch.Tensor, part_idx: Optional[torch.Tensor] = None):
    """k-way merge of per-shard top-k lists [parts, n, k] (smi_xsim_merge_topk) -> (scores [n,k], idx [n,k] | None)."""
    lib = _lib.load()
    ps = part_scores.to(torch.float32).contiguous()
    parts, n, k = ps.shape
    pi = part_idx.to(torch.int32).contiguous() if part_idx is not None else None
    out_s = torch.empty((n, k), dtype=torch.float32, device=ps.device)
    out_i = torch.empty((n, k), dtype=torch.int32, device=ps.device) if pi is not None else None
    with torch.cuda.device(ps.device):
        _lib.check(lib.smi_xsim_merge_topk(ps.data_ptr(), pi.data_ptr() if pi is not None else None, parts, n, k,
                                           out_s.data_ptr(), out_i.data_ptr() if out_i is not None else None,
                                           _lib.current_stream_ptr()))
    return out_s, out_i


def margin_select(fwd_scores: torch.Tensor, fwd_idx: torch.Tensor, bwd_scores: Optional[torch.Tensor],
                  margin: str = "ratio", x_index_offset: int = 0, err_count: Optional[torch.Tensor] = None):
    """LASER margin re-scoring of the k-NN candidates on the device (smi_xsim_margin_select).
    Returns (predicted y index per x row int32 [nx], its margin score fp32 [nx]); `err_count` (device
    int32 [1]) is incremented by the number of rows whose prediction is not row index + x_index_offset."""
    if margin not in _lib.SMI_MARGIN:
        raise ValueError(margin)
    lib = _lib.load()
    fs = fwd_scores.to(torch.float32).contiguous()
    fi = fwd_idx.to(torch.int32).contiguous()
    nx, k = fs.shape
    bs = bwd_scores.to(torch.float32).contiguous() if bwd_scores is not None else None
    if bs is not None and bs.shape[1] != k:
        raise ValueError("forward and backward neighbour lists must have the same k")
    pred = torch.empty((nx,), dtype=torch.int32, device=fs.device)
    pm = torch.empty((nx,), dtype=torch.float32, device=fs.device)
    with torch.cuda.device(fs.device):
        _lib.check(lib.smi_xsim_margin_select(
            fs.data_ptr(), fi.data_ptr(), nx, k, bs.data_ptr() if bs is not None else None,
            bs.shape[0] if bs is not None else 0, _lib.SMI_MARGIN[margin], x_index_offset, pred.data_ptr(),
            pm.data_ptr(), err_count.data_ptr() if err_count is not None else None, _lib.current_stream_ptr()))
    return pred, pm


def xsim_error(x: torch.Tensor, y: torch.Tensor, margin: str = "cosine", k: int = 4,
               precision: str = "fp16") -> Tuple[float, torch.Tensor]:
    """xsim error rate for aligned x[i] <-> y[i] (LASER source/xsim.py); returns (error rate, predicted
    index per x row).  margin: "cosine" | "ratio" | "distance" (k nearest neighbours, LASER default 4).
    precision="int8": the neighbour passes run as topk_int8_normalized with 8 candidates, refined to fp16 cosines."""
    check_precision(precision)
    if x.shape[0] != y.shape[0]:
        raise ValueError("xsim expects aligned x and y")
    xn, yn = normalize_rows(x), normalize_rows(y)
    n = x.shape[0]
    errs = torch.zeros(1, dtype=torch.int32, device=xn.device)
    if precision == "int8":
        from . import index

        xe, ye = index.encode_rows_int8(xn), index.encode_rows_int8(yn)  # each side once, for both directions

        def fwd(kk):
            return topk_int8_normalized(xn, n, yn, n, kk, x_enc=xe, y_enc=ye)

        def bwd(kk):
            return topk_int8_normalized(yn, n, xn, n, kk, x_enc=ye, y_enc=xe)
    else:
        def fwd(kk):
            return topk_normalized(xn, n, yn, n, kk)

        def bwd(kk):
            return topk_normalized(yn, n, xn, n, kk)
    if margin == "cosine":
        fs, fi = fwd(1)
        pred, _ = margin_select(fs, fi, None, "cosine", 0, errs)
    else:
        kk = min(k, n)
        fs, fi = fwd(kk)
        bs, _ = bwd(kk)
        pred, _ = margin_select(fs, fi, bs, margin, 0, errs)
    return int(errs.item()) / n, pred.long()
