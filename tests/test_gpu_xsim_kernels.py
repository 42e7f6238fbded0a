"""GPU: the xsim mining kernels (sonar_amd/csrc/xsim.hip) against their ordering and masking contract.

`smi_xsim_topk` promises a TOTAL order (score descending, ties -> lower y index), `-1` / `-inf` where fewer
than k candidates exist and `y_index_offset` on valid indices only.  Most of this file checks that with exact
equality: on operands with small integer entries every product and every partial sum is an integer far below
2^24, so the fp32 score is exact in any accumulation order and the fp64 reference, stable-sorted, is the one
right answer -- scores AND indices, every row.  The two tolerances that remain are derived, not measured:
`d * 2^-23` for the fp32 accumulation of normalised rows, one fp16 ulp for `smi_xsim_normalize`."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


# ------------------------------------------------------------------------------------------------ helpers
def _pad256(t: torch.Tensor) -> torch.Tensor:
    """Zero rows up to a multiple of 256: the layout smi_xsim_topk reads (normalize_rows makes it otherwise)."""
    rows, d = t.shape
    out = torch.zeros(((rows + 255) // 256 * 256, d), dtype=t.dtype)
    out[:rows] = t
    return out


def _mine(x: torch.Tensor, y: torch.Tensor, k: int, offset: int = 0):
    """smi_xsim_topk on fp16 rows used as they are (it does not check that they are normalised)."""
    from sonar_amd import xsim

    s, i = xsim.topk_normalized(_pad256(x).cuda(), x.shape[0], _pad256(y).cuda(), y.shape[0], k, offset)
    torch.cuda.synchronize()
    return s.cpu(), i.cpu().long()


def _sorted_reference(x: torch.Tensor, y: torch.Tensor, keep: int = 9):
    """fp64 scores, stable-sorted descending (equal scores keep ascending index order): first `keep` columns."""
    vals, idx = torch.sort(x.double() @ y.double().T, dim=1, descending=True, stable=True)
    return vals[:, :keep].clone(), idx[:, :keep].clone()


def _first_k(vals: torch.Tensor, idx: torch.Tensor, k: int, offset: int = 0):
    """The expected output: the first k of the sorted reference, (-inf, -1) where y has fewer than k rows."""
    n, have = vals.shape[0], min(k, vals.shape[1])
    want_s = torch.full((n, k), NEG_INF, dtype=torch.float32)
    want_i = torch.full((n, k), -1, dtype=torch.int64)
    want_s[:, :have] = vals[:, :have].float()
    want_i[:, :have] = idx[:, :have] + offset
    assert torch.equal(want_s[:, :have].double(), vals[:, :have])  # integer scores: fp32 holds them exactly
    return want_s, want_i


def _assert_same(got: torch.Tensor, want: torch.Tensor, what: str):
    if not torch.equal(got, want):
        bad = (got != want).any(dim=1).nonzero().squeeze(1)
        r = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {got.shape[0]} rows differ, first row {r}: "
                             f"got {got[r].tolist()} want {want[r].tolist()}")


# ------------------------------------------------------------------ 1. exact total order, integer operands
# (nx, ny, d, ks, plant): d = 64 is the shortest slice stream (two slices a tile), 1024 the workload's.
#   1 x 1            the smallest launch
#   257 x 256        one y tile, two x tiles, the second with one valid row
#   300 x 513        three chunks of one tile, the last tile holds one valid row; every k: k_out < K in the merge
#   513 x 2305       10 y tiles: chunks of two tiles, three empty chunks
#   300 x 4352       17 tiles, no pad rows: chunks of 3, 3, 3, 3, 3, 2 and two empty
#   300 x 6100       24 tiles, three per chunk, none empty
#   600 x 4353       d = 1024: 32 slices a tile
#   2305 / 4353 rows of x: 10 and 18 x tiles (a raster group of 8 and a remainder group), grids of 40 and 54
_EXACT = [
    (1, 1, 64, (1, 8), False),
    (257, 256, 64, (1, 2), False),
    (300, 513, 128, (1, 2, 3, 4, 5, 6, 7, 8), True),
    (513, 2305, 128, (1, 2, 4, 8), True),
    (300, 4352, 64, (1, 3), False),
    (300, 6100, 64, (1, 3, 8), False),
    (600, 4353, 1024, (1, 5), False),
    (2305, 769, 64, (1, 4), False),
    (4353, 513, 64, (1, 4), False),
]
_EXACT_PARAMS = [(nx, ny, d, k, plant) for nx, ny, d, ks, plant in _EXACT for k in ks]
_ZERO_X_ROW, _TWIN_X_ROW, _TWIN_Y_SRC = 7, 11, 5
_TWIN_Y_ROWS = (5, 255, 256, 511)  # and ny - 1: ties across lanes, waves, tiles and chunks


@functools.lru_cache(maxsize=None)
def _exact_case(nx: int, ny: int, d: int, plant: bool):
    g = torch.Generator().manual_seed(1000003 * nx + 1009 * ny + d)
    x = torch.randint(-1, 2, (nx, d), generator=g).half()
    y = torch.randint(-1, 2, (ny, d), generator=g).half()
    if d >= 1024:
        # uniform draws from {-1, 0, 1} spread the scores of 1024 terms so far that the two best tie in under 10 %
        # of the rows: zero half of the entries (still {-1, 0, 1}, scores of about half the spread)
        x *= torch.randint(0, 2, (nx, d), generator=g)
        y *= torch.randint(0, 2, (ny, d), generator=g)
    if plant:
        x[_ZERO_X_ROW] = 0                       # every candidate ties at 0: the answer is 0, 1, 2, ...
        for r in _TWIN_Y_ROWS + (ny - 1,):
            y[r] = y[_TWIN_Y_SRC]
        x[_TWIN_X_ROW] = y[_TWIN_Y_SRC]          # its five copies tie at the top score
    vals, idx = _sorted_reference(x, y)
    return x, y, vals, idx


@pytest.mark.parametrize("nx,ny,d,k,plant", _EXACT_PARAMS)
def test_topk_exact_total_order(nx, ny, d, k, plant):
    """Scores and indices equal the stable-sorted fp64 reference exactly, every row."""
    x, y, vals, idx = _exact_case(nx, ny, d, plant)
    if ny > k:
        # a condition on the INPUTS (reference alone): the k-th and (k+1)-th scores tie in enough rows that the
        # tie-break decides what is kept.  (With ny <= k there is no (k+1)-th candidate to tie with.)
        share = (vals[:, k - 1] == vals[:, k]).double().mean().item()
        floor = 0.5 if d == 64 and k >= 3 else 0.1
        print(f"{nx} x {ny} x {d}, k = {k}: k-th / (k+1)-th tie in {share:.1%} of the rows")
        assert share >= floor, share
    if plant:
        assert idx[_ZERO_X_ROW, :min(9, ny)].tolist() == list(range(min(9, ny)))
        assert idx[_TWIN_X_ROW, :5].tolist() == sorted(_TWIN_Y_ROWS + (ny - 1,))
    s, i = _mine(x, y, k)
    want_s, want_i = _first_k(vals, idx, k)
    _assert_same(i, want_i, "indices")
    _assert_same(s, want_s, "scores")


# ------------------------------------------------------ 2. pad mask, missing candidates, offset, workspace
@functools.lru_cache(maxsize=None)
def _negative_case(ny: int):
    g = torch.Generator().manual_seed(77 + ny)
    x = torch.randint(1, 3, (300, 64), generator=g).half()
    y = -torch.randint(1, 3, (ny, 64), generator=g).half()
    return (x, y) + _sorted_reference(x, y)


@pytest.mark.parametrize("offset", [0, 1000])
@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("ny", [300, 2049])
def test_topk_pad_rows_never_win(ny, k, offset):
    """Every real score is negative, so a zero pad row of Y (score 0) would win if the fold let it in."""
    x, y, vals, idx = _negative_case(ny)
    assert vals.max().item() < 0
    s, i = _mine(x, y, k, offset)
    assert int(i.min()) >= offset and int(i.max()) < ny + offset
    want_s, want_i = _first_k(vals, idx, k, offset)
    _assert_same(i, want_i, "indices")
    _assert_same(s, want_s, "scores")


@pytest.mark.parametrize("offset", [0, 1000])
@pytest.mark.parametrize("ny", [1, 3, 5])
def test_topk_missing_candidates(ny, offset):
    """ny < k: positions >= ny hold (-inf, -1) -- with an offset too -- and positions < ny are exact."""
    g = torch.Generator().manual_seed(5 + ny)
    x = torch.randint(-1, 2, (70, 64), generator=g).half()
    y = torch.randint(-1, 2, (ny, 64), generator=g).half()
    vals, idx = _sorted_reference(x, y)
    s, i = _mine(x, y, 8, offset)
    assert (i[:, ny:] == -1).all() and (s[:, ny:] == NEG_INF).all()
    want_s, want_i = _first_k(vals, idx, 8, offset)
    _assert_same(i, want_i, "indices")
    _assert_same(s, want_s, "scores")


def test_topk_refuses_short_workspace():
    """One byte short of smi_xsim_workspace_bytes: an error before any launch, the outputs untouched."""
    from sonar_amd import _lib

    lib = _lib.load()
    nx, ny, d, k = 300, 513, 64, 4
    g = torch.Generator().manual_seed(3)
    xn = _pad256(torch.randint(-1, 2, (nx, d), generator=g).half()).cuda()
    yn = _pad256(torch.randint(-1, 2, (ny, d), generator=g).half()).cuda()
    need = int(lib.smi_xsim_workspace_bytes(nx, ny, k, d))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    idx = torch.full((nx, k), -77, dtype=torch.int32, device="cuda")
    score = torch.full((nx, k), 12345.0, dtype=torch.float32, device="cuda")

    def call(ws_bytes):
        return lib.smi_xsim_topk(xn.data_ptr(), nx, yn.data_ptr(), ny, d, k, 0, idx.data_ptr(), score.data_ptr(),
                                 ws.data_ptr(), ws_bytes, _lib.current_stream_ptr())

    with pytest.raises(_lib.SmiError):
        _lib.check(call(need - 1))
    torch.cuda.synchronize()
    assert (idx == -77).all() and (score == 12345.0).all()
    _lib.check(call(need))  # the exact size is accepted
    torch.cuda.synchronize()
    assert (idx >= 0).all() and (idx < ny).all()


# --------------------------------------------------------- 3. the real path: normalise, then mine, vs fp64
_REAL_NX, _REAL_NY = 300, 2305


@functools.lru_cache(maxsize=None)
def _real_case(d: int, src_dtype: torch.dtype):
    """Clustered rows, normalised ON THE DEVICE; the reference is the fp64 product of those fp16 rows, so all
    that separates it from the kernel is the fp32 accumulation."""
    from sonar_amd import xsim

    g = torch.Generator().manual_seed(4000 + d)
    y = torch.randn(_REAL_NY, d, generator=g)
    x = y[torch.randint(0, _REAL_NY, (_REAL_NX,), generator=g)] + 0.8 * torch.randn(_REAL_NX, d, generator=g)
    xn = xsim.normalize_rows(x.to(src_dtype).cuda())
    yn = xsim.normalize_rows(y.to(src_dtype).cuda())
    torch.cuda.synchronize()
    xn, yn = xn.cpu(), yn.cpu()
    full = xn[:_REAL_NX].double() @ yn[:_REAL_NY].double().T
    return xn, yn, full, torch.sort(full, dim=1, descending=True).values[:, :8].clone()


@pytest.mark.parametrize("k", [1, 4, 7])
@pytest.mark.parametrize("src_dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("d", [64, 320, 1024, 2048, 2560])
def test_topk_of_normalized_rows_vs_fp64(d, src_dtype, k):
    """tol = d * 2^-23: products of fp16 values are exact in fp32, accumulating d of them costs at most
    (d - 1) * 2^-24 * sum|x_i y_i| <= (d - 1) * 2^-24 * |x||y|, |x||y| ~ 1; the factor 2 covers second-order
    terms and the fp16 rounding of the norms."""
    from sonar_amd import xsim

    xn, yn, full, best = _real_case(d, src_dtype)
    tol = d * 2.0 ** -23
    s, i = xsim.topk_normalized(xn.cuda(), _REAL_NX, yn.cuda(), _REAL_NY, k)
    torch.cuda.synchronize()
    s, i = s.cpu().double(), i.cpu().long()
    assert int(i.min()) >= 0 and int(i.max()) < _REAL_NY
    assert (i.sort(dim=1).values.diff(dim=1) > 0).all()          # distinct
    assert (s.diff(dim=1) <= 0).all()                            # non-increasing
    err_picked = (s - full.gather(1, i)).abs().max().item()
    err_rank = (s - best[:, :k]).abs().max().item()
    print(f"d = {d}: |score - S64[idx]| <= {err_picked:.2e}, |score - j-th largest| <= {err_rank:.2e}, tol {tol:.2e}")
    assert err_picked <= tol
    assert err_rank <= tol


# ----------------------------------------------------------------- 4. smi_xsim_normalize, element by element
def _normalize_into(src: torch.Tensor, dst: torch.Tensor):
    from sonar_amd import _lib

    lib = _lib.load()
    rows, d = src.shape
    assert dst.shape == (int(lib.smi_xsim_padded_rows(rows)), d) and dst.dtype == torch.float16
    _lib.check(lib.smi_xsim_normalize(src.data_ptr(), _lib.SMI_F32 if src.dtype == torch.float32 else _lib.SMI_F16,
                                      rows, d, dst.data_ptr(), _lib.current_stream_ptr()))
    torch.cuda.synchronize()


def _ulp_fp16(r: torch.Tensor) -> torch.Tensor:
    """max(2^(floor(log2|r|) - 10), 2^-24): the spacing of fp16 values around r."""
    _, e = torch.frexp(r.abs())                                   # |r| = m * 2^e, m in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(r), e - 11)
    return torch.where(r == 0, torch.zeros_like(r), ulp).clamp_min(2.0 ** -24)


def _normalize_sources(rows: int, d: int, dtype: torch.dtype):
    """(source matrix, index of its all-zero row).  Special rows: all zero; scaled by 2^-14 (fp16 subnormals)
    and by 2^5; entries up to 6e4 (the fp32 sum of squares still fits: 2560 * 65504^2 ~ 1.1e13)."""
    g = torch.Generator().manual_seed(rows * 10007 + d)
    base = torch.randn(rows, d, generator=g)
    large = (torch.rand(d, generator=g) * 2 - 1) * 6e4
    if rows == 1:  # one row at a time
        return [(base.to(dtype), None), (torch.zeros(1, d).to(dtype), 0), ((base * 2.0 ** -14).to(dtype), None),
                ((base * 2.0 ** 5).to(dtype), None), (large[None].to(dtype), None)]
    base[3] = 0
    base[7] *= 2.0 ** -14
    base[11] *= 2.0 ** 5
    base[13] = large
    return [(base.to(dtype), 3)]


@pytest.mark.parametrize("src_dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("d", [64, 320, 512, 1024, 1536, 2048, 2560])
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_normalize_elementwise(rows, d, src_dtype):
    """Every element within one fp16 ulp of x / max(|x|, 1e-12) in fp64 (the adjacent fp16 value is allowed:
    the fp32 arithmetic in front of the rounding may flip a near-tie, nothing else may differ); pad rows
    exactly zero over a NaN prefill; an all-zero row stays zero.  d and the source type choose between the
    one-pass vector path (d % 512 == 0, d <= 2048 for fp16, <= 1024 for fp32) and the generic one."""
    for src, zero_row in _normalize_sources(rows, d, src_dtype):
        pad = (rows + 255) // 256 * 256
        dst = torch.full((pad, d), float("nan"), dtype=torch.float16, device="cuda")
        _normalize_into(src.cuda(), dst)
        out = dst.cpu()
        assert torch.isfinite(out[:rows]).all()
        assert (out[rows:] == 0).all()
        s64 = src.double()
        ref = s64 / s64.norm(dim=1, keepdim=True).clamp_min(1e-12)
        excess = ((out[:rows].double() - ref).abs() - _ulp_fp16(ref)).max().item()
        assert excess <= 0, f"an element is {excess:.3e} beyond one fp16 ulp"
        if zero_row is not None:
            assert (out[zero_row] == 0).all()


# ------------------------------------------------------------------------------- 5. small related checks
# dyadic values: every expected fp32 result below is exact
@pytest.mark.parametrize("margin", ["cosine", "distance"])
def test_margin_select_tie_takes_first_listed(margin):
    from sonar_amd import xsim

    # row 0: equal scores, equal neighbour means; row 1: different scores, the SAME margin
    # (0.75 - (0.625 + 1) / 2 = 0.5 - (0.625 + 0.5) / 2 = -0.0625); row 2: no tie, the second candidate wins
    fs = torch.tensor([[0.5, 0.5], [0.75, 0.5], [0.25, 0.5]])
    fi = torch.tensor([[9, 4], [6, 2], [9, 4]], dtype=torch.int32)
    bwd = torch.zeros(10, 2)
    bwd[9], bwd[4], bwd[6], bwd[2] = 0.25, 0.25, 1.0, 0.5
    pred, pm = xsim.margin_select(fs.cuda(), fi.cuda(), None if margin == "cosine" else bwd.cuda(), margin)
    if margin == "cosine":
        assert pred.cpu().tolist() == [9, 6, 4]
        assert pm.cpu().tolist() == [0.5, 0.75, 0.5]
    else:
        assert pred.cpu().tolist() == [9, 6, 4]
        assert pm.cpu().tolist() == [0.5 - (0.5 + 0.25) / 2, -0.0625, 0.5 - (0.375 + 0.25) / 2]


def test_margin_select_missing_candidate_reads_nothing():
    """A candidate index of -1 (or >= ny) has a neighbour mean of 0.  The backward scores are a window of a
    larger buffer whose rows just outside the window are huge: a read at row -1 or row ny would show."""
    from sonar_amd import xsim

    ny, k = 4, 2
    buf = torch.full((ny + 2, k), 2.0 ** 100).cuda()
    buf[1:ny + 1] = 1.0
    bwd = buf[1:ny + 1]
    fs = torch.tensor([[0.75, 0.25], [0.75, 0.25], [0.75, 0.25]]).cuda()
    fi = torch.tensor([[-1, 2], [ny, 2], [2, -1]], dtype=torch.int32).cuda()
    # forward mean 0.5; a missing candidate: b = 0.25; candidate 2: b = (0.5 + 1) / 2 = 0.75
    pred, pm = xsim.margin_select(fs, fi, bwd, "distance")
    assert pred.cpu().tolist() == [-1, ny, 2] and pm.cpu().tolist() == [0.5, 0.5, 0.0]
    pred, pm = xsim.margin_select(fs, fi, bwd, "ratio")
    assert pred.cpu().tolist() == [-1, ny, 2] and pm.cpu().tolist() == [3.0, 3.0, 1.0]


def test_margin_select_err_count_accumulates():
    from sonar_amd import xsim

    n = 600  # three blocks of 256 threads, the last one partly filled
    fs = torch.full((n, 1), 0.5).cuda()
    fi = torch.arange(n, dtype=torch.int32)[:, None].clone()
    fi[::7] = 0  # rows 7, 14, ... now point at y 0: wrong (row 0 itself stays right)
    wrong = int((fi[:, 0] != torch.arange(n)).sum())
    assert wrong == (n - 1) // 7
    errs = torch.zeros(1, dtype=torch.int32, device="cuda")
    xsim.margin_select(fs, fi.cuda(), None, "cosine", 0, errs)
    assert int(errs.item()) == wrong
    xsim.margin_select(fs, fi.cuda(), None, "cosine", 0, errs)
    assert int(errs.item()) == 2 * wrong


def test_merge_topk_keeps_missing_entries_last():
    """Part lists with (-inf, -1) tails, as smi_xsim_topk returns them for shards shorter than k."""
    from sonar_amd import xsim

    parts, n, k = 3, 300, 4
    g = torch.Generator().manual_seed(11)
    sc = torch.randint(-8, 9, (parts, n, k), generator=g).float() / 8   # dyadic, many ties across the shards
    idx = torch.stack([torch.stack([torch.randperm(50, generator=g)[:k] for _ in range(n)]) + 50 * p
                       for p in range(parts)])
    idx = idx.sort(dim=2).values                                        # every list: score descending, index ascending
    sc = torch.sort(sc, dim=2, descending=True, stable=True).values
    have = torch.randint(0, k + 1, (parts, n), generator=g)
    have[:, 0] = 0          # a row with no candidate at all
    have[:, 1] = 0
    have[1, 1] = 2          # a row with fewer than k candidates in all
    gone = torch.arange(k)[None, None, :] >= have[:, :, None]
    sc[gone], idx[gone] = NEG_INF, -1
    ms, mi = xsim.merge_topk(sc.cuda(), idx.int().cuda())
    ms, mi = ms.cpu(), mi.cpu().long()
    for r in range(n):
        cand = sorted((-float(sc[p, r, j]), int(idx[p, r, j])) for p in range(parts) for j in range(int(have[p, r])))[:k]
        want_s = [-c[0] for c in cand] + [NEG_INF] * (k - len(cand))
        want_i = [c[1] for c in cand] + [-1] * (k - len(cand))
        assert ms[r].tolist() == want_s and mi[r].tolist() == want_i, (r, ms[r], mi[r], want_s, want_i)
