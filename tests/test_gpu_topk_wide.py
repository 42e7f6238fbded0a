"""GPU: the paged brute-force top-k (smi_xsim_topk_page, xsim.topk_page_normalized / topk_wide_normalized)
against the restatement in tests/topk_wide_ref.py.

As in tests/test_gpu_xsim_kernels.py the operands of the exact tests have entries from {-1, 0, 1} (half of them zeroed at
d = 1024): every fp32 sum is an exact small integer, so the stable-sorted fp64 reference is the one right answer, scores AND
ids, on every row.  The one tolerance, d * 2^-23 for real normalised rows, is the derived bound of that file."""
import functools

import numpy as np
import pytest
import torch

from tests import topk_wide_ref as W

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


def _pad256(t: torch.Tensor) -> torch.Tensor:
    rows, d = t.shape
    out = torch.zeros(((rows + 255) // 256 * 256, d), dtype=t.dtype)
    out[:rows] = t
    return out


def _wide(x, y, k, offset=0):
    from sonar_amd import xsim

    s, i = xsim.topk_wide_normalized(_pad256(x).cuda(), x.shape[0], _pad256(y).cuda(), y.shape[0], k, offset)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy().astype(np.int64)


def _page(x, y, k, offset=0, below=None):
    from sonar_amd import xsim

    if below is not None:
        below = (torch.as_tensor(np.asarray(below[0], dtype=np.float32)).cuda(),
                 torch.as_tensor(np.asarray(below[1], dtype=np.int32)).cuda())
    s, i = xsim.topk_page_normalized(_pad256(x).cuda(), x.shape[0], _pad256(y).cuda(), y.shape[0], k, offset, below)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy().astype(np.int64)


def _assert_same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        r = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.shape[0]} rows differ, first row {r}: got {got[r].tolist()} "
                             f"want {want[r].tolist()}")


# ------------------------------------------------------------------ 1. exact total order over the pages, integer operands
_EXACT = [
    (1, 1, 64, (16, 64), False),
    (257, 256, 64, (9, 16, 17), False),              # one y tile, one valid row in the second x tile
    (300, 513, 128, (9, 12, 16, 17, 32, 33, 64), True),  # three chunks of one tile, one valid row in the last
    (513, 2305, 128, (16, 40, 64), False),           # chunks of two tiles, three of them empty
    (300, 6100, 64, (16, 64), False),                # three tiles per chunk
    (300, 2305, 1024, (16, 33), False),              # 32 slices a tile
]
_EXACT_PARAMS = [(nx, ny, d, k, plant) for nx, ny, d, ks, plant in _EXACT for k in ks]
_ZERO_X_ROW, _TWIN_X_ROW, _TWIN_Y_SRC = 7, 11, 5
_TWIN_Y_ROWS = (5, 255, 256, 511)  # and ny - 1: ties across lanes, waves, tiles and chunks


@functools.lru_cache(maxsize=None)
def _exact_case(nx: int, ny: int, d: int, plant: bool):
    """The seed recipe and the planted rows of tests/test_gpu_xsim_kernels.py; the reference once, 65 columns of it."""
    g = torch.Generator().manual_seed(1000003 * nx + 1009 * ny + d)
    x = torch.randint(-1, 2, (nx, d), generator=g).half()
    y = torch.randint(-1, 2, (ny, d), generator=g).half()
    if d >= 1024:
        x *= torch.randint(0, 2, (nx, d), generator=g)
        y *= torch.randint(0, 2, (ny, d), generator=g)
    if plant:
        x[_ZERO_X_ROW] = 0
        for r in _TWIN_Y_ROWS + (ny - 1,):
            y[r] = y[_TWIN_Y_SRC]
        x[_TWIN_X_ROW] = y[_TWIN_Y_SRC]
    s64 = (x.double() @ y.double().T).numpy()
    vals, idx = W.first_k(s64, 65)
    return x, y, vals, idx


def _tie_share(vals, a: int) -> float:
    """The share of the rows whose entries a and a + 1 (1-based) tie."""
    return float((vals[:, a - 1] == vals[:, a]).mean())


@pytest.mark.parametrize("nx,ny,d,k,plant", _EXACT_PARAMS)
def test_wide_topk_exact_total_order(nx, ny, d, k, plant):
    """Scores and ids of topk_wide_normalized equal the stable-sorted fp64 reference exactly, every row."""
    x, y, vals, idx = _exact_case(nx, ny, d, plant)
    # a condition on the INPUTS, asserted on the reference alone: the tie-break decides what is kept at k | k + 1 and at
    # every page boundary k passes
    for a in sorted({k} | {b for b in (16, 32, 48) if b <= k}):
        if ny > a:
            share = _tie_share(vals, a)
            print(f"{nx} x {ny} x {d}: entries {a} | {a + 1} tie in {share:.1%} of the rows")
            assert share >= 0.5, (a, share)
    if plant:
        assert idx[_ZERO_X_ROW, :64].tolist() == list(range(64))
        assert idx[_TWIN_X_ROW, :5].tolist() == sorted(_TWIN_Y_ROWS + (ny - 1,))
    s, i = _wide(x, y, k)
    assert s.shape == (nx, k) and i.shape == (nx, k)
    _assert_same(i, idx[:, :k], "ids")
    _assert_same(s, vals[:, :k], "scores")


# ------------------------------------------------------ 2. y runs out, offsets, pad rows, ceilings that are no candidate
@pytest.mark.parametrize("offset", [0, 1000])
@pytest.mark.parametrize("ny", [1, 15, 16, 17, 40])
def test_wide_fill_where_y_runs_out(ny, offset):
    g = torch.Generator().manual_seed(5 + ny)
    x = torch.randint(-1, 2, (70, 64), generator=g).half()
    y = torch.randint(-1, 2, (ny, 64), generator=g).half()
    s64 = (x.double() @ y.double().T).numpy()
    want_s, want_i = W.first_k(s64, 64, offset)
    s, i = _wide(x, y, 64, offset)
    assert (i[:, ny:] == -1).all() and np.isneginf(s[:, ny:]).all()
    _assert_same(i, want_i, "ids")
    _assert_same(s, want_s, "scores")
    # the page after an exhausted page is all fill; so is the page after a page that ended on the last candidate
    for kp in (16, 5):
        ps, pi = _page(x, y, kp, offset, below=(s[:, 63], i[:, 63]))
        assert (pi == -1).all() and np.isneginf(ps).all()
    last = (want_s[:, ny - 1], want_i[:, ny - 1])
    ps, pi = _page(x, y, 16, offset, below=last)
    assert (pi == -1).all() and np.isneginf(ps).all()


@functools.lru_cache(maxsize=None)
def _negative_case(ny: int):
    g = torch.Generator().manual_seed(77 + ny)
    x = torch.randint(1, 3, (300, 64), generator=g).half()
    y = -torch.randint(1, 3, (ny, 64), generator=g).half()
    return x, y, (x.double() @ y.double().T).numpy()


@pytest.mark.parametrize("k", [16, 48])
@pytest.mark.parametrize("ny", [300, 2049])
def test_wide_pad_rows_never_enter_on_any_page(ny, k):
    """Every real score is negative: a zero pad row of Y (score 0) would come first if a fold let it in."""
    x, y, s64 = _negative_case(ny)
    assert s64.max() < 0
    want_s, want_i = W.first_k(s64, k, 1000)
    s, i = _wide(x, y, k, 1000)
    assert i.min() >= 1000 and i.max() < ny + 1000
    _assert_same(i, want_i, "ids")
    _assert_same(s, want_s, "scores")


def test_page_with_ceilings_that_are_no_candidate():
    """topk_page_normalized directly: per-row ceilings between two scores, on a score with an id in front of, between and
    behind the rows that tie, an exhausted row, +-inf, and an id offset."""
    nx, ny, d, offset = 300, 513, 128, 1000
    x, y, _, _ = _exact_case(nx, ny, d, True)
    s64 = (x.double() @ y.double().T).numpy()
    rng = np.random.default_rng(1)
    cs = rng.integers(-6, 7, nx).astype(np.float64)
    cs[::3] += 0.5                                   # no integer score equals it
    ci = rng.integers(offset - 50, offset + ny + 50, nx).astype(np.int64)  # some in front of every id, some behind
    ci[::7] = offset
    ci[5::11] = -1                                   # exhausted
    cs[1], cs[2], cs[3] = np.inf, -np.inf, 0.0
    cs[_ZERO_X_ROW], ci[_ZERO_X_ROW] = 0.0, offset + 100   # every candidate ties: the id alone decides
    cs[13], ci[13] = -0.0, offset + 3                # a negative zero is the zero
    for k in (16, 5):
        want_s, want_i = W.brute_force(s64, k, offset, (cs, ci))
        s, i = _page(x, y, k, offset, below=(cs, ci))
        _assert_same(i, want_i, "ids")
        _assert_same(s, want_s, "scores")
    assert want_i[_ZERO_X_ROW].tolist() == list(range(offset + 101, offset + 101 + 5))
    assert (want_i[5::11] == -1).all()
    # no ceiling, k <= 16: the first page is topk_normalized's answer
    want_s, want_i = W.first_k(s64, 12, offset)
    s, i = _page(x, y, 12, offset)
    _assert_same(i, want_i, "ids")
    _assert_same(s, want_s, "scores")


# ------------------------------------------------------------------------------- 3. real rows: bits, bound, determinism
_REAL_NX, _REAL_NY, _REAL_D = 300, 2305, 1024


@functools.lru_cache(maxsize=None)
def _real_case():
    from sonar_amd import xsim

    g = torch.Generator().manual_seed(4000 + _REAL_D)
    y = torch.randn(_REAL_NY, _REAL_D, generator=g)
    x = y[torch.randint(0, _REAL_NY, (_REAL_NX,), generator=g)] + 0.8 * torch.randn(_REAL_NX, _REAL_D, generator=g)
    xn, yn = xsim.normalize_rows(x.cuda()), xsim.normalize_rows(y.cuda())
    s, i = xsim.topk_wide_normalized(xn, _REAL_NX, yn, _REAL_NY, 40)
    torch.cuda.synchronize()
    full = xn[:_REAL_NX].cpu().double() @ yn[:_REAL_NY].cpu().double().T
    return xn, yn, full, s.cpu(), i.cpu()


def test_first_columns_equal_the_k8_pass_bit_for_bit():
    """The same slice order, so the same sums: the first 8 columns of a page of 16 are topk_normalized(k = 8)'s bits."""
    from sonar_amd import xsim

    xn, yn, _, _, _ = _real_case()
    s16, i16 = xsim.topk_wide_normalized(xn, _REAL_NX, yn, _REAL_NY, 16)
    s8, i8 = xsim.topk_normalized(xn, _REAL_NX, yn, _REAL_NY, 8)
    torch.cuda.synchronize()
    assert torch.equal(i16[:, :8], i8)
    assert torch.equal(s16[:, :8].view(torch.int32), s8.view(torch.int32))


def test_wide_topk_of_normalized_rows_vs_fp64():
    """tol = d * 2^-23, the bound tests/test_gpu_xsim_kernels.py derives for the fp32 accumulation of normalised rows."""
    _, _, full, s, i = _real_case()
    tol = _REAL_D * 2.0 ** -23
    s, i = s.double(), i.long()
    assert int(i.min()) >= 0 and int(i.max()) < _REAL_NY
    assert (i.sort(dim=1).values.diff(dim=1) > 0).all()          # distinct across the pages
    assert (s.diff(dim=1) <= 0).all()                            # non-increasing across the page boundaries
    best = torch.sort(full, dim=1, descending=True).values[:, :40]
    err_picked = (s - full.gather(1, i)).abs().max().item()
    err_rank = (s - best).abs().max().item()
    print(f"|score - S64[idx]| <= {err_picked:.2e}, |score - j-th largest| <= {err_rank:.2e}, tol {tol:.2e}")
    assert err_picked <= tol and err_rank <= tol


def test_two_calls_and_a_subset_of_the_rows_agree_bit_for_bit():
    from sonar_amd import xsim

    xn, yn, _, s, i = _real_case()
    s2, i2 = xsim.topk_wide_normalized(xn, _REAL_NX, yn, _REAL_NY, 40)
    rows = torch.tensor([0, 3, 77, 255, 256, 299], device="cuda")
    sub = torch.zeros((256, _REAL_D), dtype=torch.float16, device="cuda")
    sub[: rows.numel()] = xn[rows]
    s3, i3 = xsim.topk_wide_normalized(sub, rows.numel(), yn, _REAL_NY, 40)
    torch.cuda.synchronize()
    assert torch.equal(i2.cpu(), i) and torch.equal(s2.cpu().view(torch.int32), s.view(torch.int32))
    assert torch.equal(i3.cpu(), i[rows.cpu()]) and torch.equal(s3.cpu().view(torch.int32), s[rows.cpu()].view(torch.int32))


def test_wide_topk_in_a_captured_graph_equals_the_eager_result():
    """Nothing is read back or allocated by the entry: one capture on a single stream, one replay."""
    from sonar_amd import xsim

    xn, yn, _, s, i = _real_case()
    xsim.topk_wide_normalized(xn, _REAL_NX, yn, _REAL_NY, 33)  # (the kernels' attributes are set outside the capture)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            gs, gi = xsim.topk_wide_normalized(xn, _REAL_NX, yn, _REAL_NY, 33)
    gs.zero_(), gi.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gi.cpu(), i[:, :33]) and torch.equal(gs.cpu().view(torch.int32), s[:, :33].contiguous().view(torch.int32))


def test_page_refuses_a_short_workspace():
    from sonar_amd import _lib

    lib = _lib.load()
    nx, ny, d, k = 300, 513, 64, 16
    g = torch.Generator().manual_seed(3)
    xn = _pad256(torch.randint(-1, 2, (nx, d), generator=g).half()).cuda()
    yn = _pad256(torch.randint(-1, 2, (ny, d), generator=g).half()).cuda()
    need = int(lib.smi_xsim_topk_page_ws_bytes(nx, ny, k, d))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    idx = torch.full((nx, k), -77, dtype=torch.int32, device="cuda")
    score = torch.full((nx, k), 12345.0, dtype=torch.float32, device="cuda")

    def call(ws_bytes):
        return lib.smi_xsim_topk_page(xn.data_ptr(), nx, yn.data_ptr(), ny, d, k, 0, None, None, idx.data_ptr(),
                                      score.data_ptr(), ws.data_ptr(), ws_bytes, _lib.current_stream_ptr())

    with pytest.raises(_lib.SmiError):
        _lib.check(call(need - 1))
    torch.cuda.synchronize()
    assert (idx == -77).all() and (score == 12345.0).all()
    _lib.check(call(need))
    torch.cuda.synchronize()
    assert (idx >= 0).all() and (idx < ny).all()


def test_predict_wide_extends_predict():
    """SphericalKMeans.predict_wide over 20 fitted centroids: its first 8 columns are predict(k = 8)'s bits, every centroid
    appears once, best first, and (-1, -inf) stands where k exceeds the centroids."""
    from sonar_amd.clustering import SphericalKMeans

    g = torch.Generator().manual_seed(21)
    x = torch.randn(400, 64, generator=g).cuda()
    km = SphericalKMeans(20, n_iter=1, seed=1).fit(x)
    l8, s8 = km.predict(x, 8)
    lw, sw = km.predict_wide(x, 64)
    torch.cuda.synchronize()
    assert lw.shape == (400, 64) and lw.dtype == torch.int32 and sw.dtype == torch.float32
    assert torch.equal(lw[:, :8], l8) and torch.equal(sw[:, :8].view(torch.int32), s8.view(torch.int32))
    assert torch.equal(lw[:, :20].long().sort(dim=1).values.cpu(), torch.arange(20).expand(400, 20))
    assert (sw[:, :20].diff(dim=1) <= 0).all()
    assert (lw[:, 20:] == -1).all() and torch.isneginf(sw[:, 20:]).all()
