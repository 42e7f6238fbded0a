"""GPU: the LayerNorm fold (GemmLnFold) kernel by kernel against plain torch in fp64, on the same fp16-rounded
inputs: the weight preparation, the first row statistics, the consumer and producer epilogues of both 256x256 GEMM engines, one
producer feeding one consumer, and what the router refuses.

The stream rows are built so that the fold's terms are material: row scales 0.25 / 1 / 4, |mean| / std of 0 / 0.5 / 4 with both
signs (a dropped "- mean * c1" moves the result by a few times the output scale), and all-zero padding rows (var = 0,
rstd = 1 / sqrt(eps)).  Every engine is asserted through smi_gemm_route before its launch; every output is pre-filled with NaN."""
import ctypes as C
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from tests.tile_major import from_tile_major, to_tile_major

pytestmark = pytest.mark.gpu

U = 2.0 ** -24      # unit roundoff of fp32
H = 2.0 ** -11      # ... of fp16
EPS = 1e-5
BIAS, RELU, SILU, GLU, RESID, RESID_HALF = 0, 1, 5, 6, 8, 9                  # epilogues (include/sonar_mi355.h: smi_gemm_tn)
FOLD_NONE, FOLD_PRODUCER_SUMS, FOLD_EXACT, FOLD_CENTRED = 0, 2, 3, 4         # fold_kind of smi_gemm_route
PP256, V2, V2_RESID = 4, 5, 6                                                # SMI_GEMM_ENGINE_*
ENGINES = {"8wave": dict(G2V2=0), "4wave": dict(G2V2=1, G2V2_MIN=1)}
UNSUPPORTED, INVALID_ARG = -2, -1


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib

    lib = _lib.load()
    _lib.check(lib.smi_init(0))
    return lib


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _route(lib, epi_sel, m, n, k, ldo, has_bias, fold, nparts):
    from sonar_amd import _lib

    info = _lib.GemmRouteInfo()
    _lib.check(lib.smi_gemm_route(epi_sel, m, n, k, ldo, int(has_bias), fold, nparts, 0, 0, _lib.SMI_F32, 0, C.byref(info)))
    return info


def _zero_rows(m):
    return sorted({3, m // 2 + 77, m - 2})   # different 16-row blocks, waves and (m > 256) row tiles


def _fold_stream(m, k, gen, zero_rows=True):
    """x[r] = half(randn * s_r + o_r * s_r), s_r cycling through 3 scales and o_r through 5 mean-to-std ratios (every
    combination occurs), some rows all zero"""
    r = torch.arange(m, device="cuda")
    s = torch.tensor([0.25, 1.0, 4.0], device="cuda")[r % 3]
    o = torch.tensor([0.0, 0.5, -0.5, 4.0, -4.0], device="cuda")[r % 5]
    x = (torch.randn(m, k, device="cuda", generator=gen) * s[:, None] + (o * s)[:, None]).half()
    if zero_rows:
        x[_zero_rows(m)] = 0
    return x


def _weights(n, k, gen):
    w = (torch.randn(n, k, device="cuda", generator=gen) * 0.05).half()
    g = 1 + 0.3 * torch.randn(k, device="cuda", generator=gen)
    b = 0.2 * torch.randn(k, device="cuda", generator=gen)
    bias = torch.randn(n, device="cuda", generator=gen)
    return w, g, b, bias


def _prep(lib, w, g, b, bias, centered):
    from sonar_amd import _lib

    n, k = w.shape
    wf, c1, c2 = _nan((n, k), torch.float16), _nan((n,)), _nan((n,))
    _lib.check(lib.smi_ln_fold_prep(w.data_ptr(), g.data_ptr(), b.data_ptr(), _ptr(bias), wf.data_ptr(), c1.data_ptr(),
                                    c2.data_ptr(), n, k, centered, _stream()))
    torch.cuda.synchronize()
    return wf, c1, c2


def _row_stats(lib, x_tm, m, d, nparts, extra=0):
    from sonar_amd import _lib

    part = _nan((nparts * m + extra, 2))
    _lib.check(lib.smi_row_stats_tm(x_tm.data_ptr(), part.data_ptr(), m, d, nparts, _stream()))
    torch.cuda.synchronize()
    return part


# ------------------------------------------------------------------------------------------------------------ a. preparation
PREP_SHAPES = [(130, 192), (768, 1024), (256, 256)]   # 130: not a multiple of the 4 rows per workgroup


def _prep_case(lib, n, k, centered, use_bias):
    gen = torch.Generator(device="cuda").manual_seed(n * 7 + k)
    w, g, b, bias = _weights(n, k, gen)
    return (w, g, b, bias) + _prep(lib, w, g, b, bias if use_bias else None, centered)


@pytest.mark.parametrize("use_bias", [True, False])
@pytest.mark.parametrize("centered", [0, 1])
@pytest.mark.parametrize("n,k", PREP_SHAPES)
def test_ln_fold_prep(lib, n, k, centered, use_bias):
    w, g, b, bias, wf, c1, c2 = _prep_case(lib, n, k, centered, use_bias)
    assert torch.isfinite(wf).all() and torch.isfinite(c1).all() and torch.isfinite(c2).all()   # every entry written
    wg = w.double() * g.double()                       # exact: 11 x 24 bits
    if centered:
        value = wg - wg.mean(dim=1, keepdim=True)
        assert ((wf.double() - value).abs() <= H * value.abs() + U).all()
        # centring is what makes c1 small: the rounding residue, not the row sum
        assert (c1.abs() <= k * H * wf.double().abs().max(dim=1).values).all()
    else:
        # bit for bit the fp32 product rounded to fp16 (a multiply fused with the conversion rounds once and differs from this
        # by an fp16 ulp in ~1e-4 of the entries)
        assert torch.equal(wf, (w.float() * g).half())
    # c1: the sum of the ROUNDED weights, which is what the GEMM multiplies
    assert ((c1.double() - wf.double().sum(1)).abs() <= k * U * wf.double().abs().sum(1)).all()
    bw = b.double() * w.double()
    want2 = bw.sum(1) + (bias.double() if use_bias else 0)
    assert ((c2.double() - want2).abs() <= k * U * (bw.abs().sum(1) + (bias.double().abs() if use_bias else 0))).all()


# ----------------------------------------------------------------------------------------------------------- b. row statistics
@pytest.mark.parametrize("nparts", [1, 4, 5])
@pytest.mark.parametrize("m,rows,d", [(512, 512, 256), (300, 512, 1024), (512, 512, 1280)])   # 300 rows of a 512-row image
def test_row_stats_tm(lib, m, rows, d, nparts):
    gen = torch.Generator(device="cuda").manual_seed(m + d)
    x = _fold_stream(rows, d, gen)
    extra = 64 if m < rows else 0
    part = _row_stats(lib, to_tile_major(x), m, d, nparts, extra)
    x64 = x[:m].double()
    got = part[:nparts * m].view(nparts, m, 2).double()
    assert ((got[0, :, 0] - x64.sum(1)).abs() <= d * U * x64.abs().sum(1)).all()
    assert ((got[0, :, 1] - (x64 * x64).sum(1)).abs() <= d * U * (x64 * x64).sum(1)).all()
    assert (got[0, _zero_rows(rows)[0]] == 0).all()
    assert (got[1:] == 0).all()                       # exactly zero: the consumers add every part
    assert torch.isnan(part[nparts * m:]).all()       # nothing past nparts * m entries


# ------------------------------------------------------------------------------------------------------------------ c. consumer
CONSUMER_EPIS = {   # engine -> variant -> (epilogue, tile-major output)
    "8wave": {"exact": [(BIAS, 1), (RELU, 1)], "centred": [(BIAS, 1), (RELU, 1), (SILU, 1), (BIAS, 0), (GLU, 0)]},
    "4wave": {"exact": [(BIAS, 1), (RELU, 1)], "centred": [(BIAS, 1), (RELU, 1), (SILU, 1), (GLU, 1)]},
}
SILU_LIPSCHITZ = 1.1   # max |silu'| = 1.0998


def _act64(epi, pre):
    if epi == RELU:
        return torch.relu(pre)
    if epi == SILU:
        return F.silu(pre)
    if epi == GLU:    # out[m][g * 32 + c] = a * sigmoid(b), a / b = columns g * 64 + c / g * 64 + 32 + c
        p = pre.view(pre.shape[0], -1, 2, 32)
        return (p[:, :, 0] * torch.sigmoid(p[:, :, 1])).reshape(pre.shape[0], -1)
    return pre


def _act_tol(epi, pre_ln, tol_pre):
    """bound of |act(p) - act(pre_ln)| over |p - pre_ln| <= tol_pre, through the activation's Lipschitz constant"""
    if epi == SILU:
        return SILU_LIPSCHITZ * tol_pre
    if epi == GLU:    # |a s(g) - a' s(g')| <= |a - a'| + |a'| |g - g'| / 4
        p, t = pre_ln.view(pre_ln.shape[0], -1, 2, 32), tol_pre.view(tol_pre.shape[0], -1, 2, 32)
        return (t[:, :, 0] + p[:, :, 0].abs() * t[:, :, 1] / 4).reshape(pre_ln.shape[0], -1)
    return tol_pre    # bias, relu: Lipschitz 1


class _FoldCase:
    """Inputs of one (m, n, k) and their fp64 references, computed once: `rows(variant, r0, r1)` gives, for a row range, the
    pre-activation of the fold identity with the kernel's own constants, that of the LayerNorm it replaces, and the bound on
    their difference that the fp16 rounding of the folded weights allows."""

    def __init__(self, lib, m, n, k, x=None):
        gen = torch.Generator(device="cuda").manual_seed(m * 3 + n * 5 + k)
        self.m, self.n, self.k = m, n, k
        self.x = _fold_stream(m, k, gen) if x is None else x
        self.w, self.g, self.b, self.bias = _weights(n, k, gen)
        self.x_tm = to_tile_major(self.x)
        self.nparts = k // 256
        self.part = _row_stats(lib, self.x_tm, m, k, self.nparts)
        x64 = self.x.double()
        self.mean = x64.mean(1, keepdim=True)
        self.rstd = 1 / torch.sqrt((x64 * x64).mean(1, keepdim=True) - self.mean ** 2 + EPS)   # fp64 from the fp16 stream
        self.wg = self.w.double() * self.g.double()            # the UNROUNDED scaled weights
        self.c2_ln = self.w.double() @ self.b.double() + self.bias.double()
        self.variants, self._rows = {}, {}
        for name, centered in (("exact", 0), ("centred", 1)):
            wf, c1, c2 = _prep(lib, self.w, self.g, self.b, self.bias, centered)
            shift = self.wg.mean(1, keepdim=True) if centered else torch.zeros(n, 1, device="cuda", dtype=torch.float64)
            self.variants[name] = types.SimpleNamespace(centered=centered, wf=wf, wf_tm=to_tile_major(wf), c1=c1, c2=c2,
                                                        dev=(self.wg - shift).abs())

    def rows(self, variant, r0, r1):
        if (variant, r0, r1) not in self._rows:
            self._rows[(variant, r0, r1)] = self._compute_rows(variant, r0, r1)
        return self._rows[(variant, r0, r1)]

    def _compute_rows(self, variant, r0, r1):
        v = self.variants[variant]
        x64, mean, rstd = self.x[r0:r1].double(), self.mean[r0:r1], self.rstd[r0:r1]
        acc = x64 @ v.wf.double().T
        if not v.centered:
            acc = acc - mean * v.c1.double()
        pre_kernel = rstd * acc + v.c2.double()
        pre_ln = rstd * ((x64 - mean) @ self.wg.T) + self.c2_ln          # = LN(x; g, b) . W^T + bias
        tol = H * rstd * ((x64 - mean).abs() @ v.dev.T)                 # worst-case fp16 rounding of Wf
        if v.centered:
            tol = tol + rstd * mean.abs() * v.c1.double().abs()          # the residue term the centred epilogue drops
        return pre_kernel, pre_ln, tol


@functools.lru_cache(maxsize=1)
def _fold_case(lib, m, n, k):
    return _FoldCase(lib, m, n, k)


def _launch_consumer(lib, engine, case, variant, epi, out_tm, part, reps=3):
    """`reps` launches from a NaN-filled output, bit-identical; the row-major [m][n or n / 2] result"""
    from sonar_amd import _lib

    m, n, k, v = case.m, case.n, case.k, case.variants[variant]
    no = n // 2 if epi == GLU else n
    epi_sel = epi | _lib.SMI_GEMM_IN_TM | (_lib.SMI_GEMM_OUT_TM if out_tm else 0)
    with _lib.tuning(**ENGINES[engine]):
        info = _route(lib, epi_sel, m, n, k, no, True, FOLD_CENTRED if v.centered else FOLD_EXACT, case.nparts)
        if engine == "8wave":
            assert (info.engine, info.layout) == (PP256, 2 if out_tm else 1), (info.engine, info.layout)
        else:
            assert (info.engine, info.flag) == (V2, 1), (info.engine, info.flag)
        outs = []
        for _ in range(reps):
            out = _nan((m * no,), torch.float16)
            _lib.check(lib.smi_gemm_tn_ln_fold(epi_sel, case.x_tm.data_ptr(), v.wf_tm.data_ptr(), v.c2.data_ptr(), out.data_ptr(),
                                               m, n, k, no, None, part.data_ptr(), v.c1.data_ptr(), case.nparts, EPS, v.centered,
                                               _stream()))
            torch.cuda.synchronize()
            outs.append(out)
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), (engine, variant, epi, out_tm)
    got = from_tile_major(outs[0], m, no) if out_tm else outs[0].view(m, no)
    assert torch.isfinite(got).all(), (engine, variant, epi, out_tm)
    return got, info


def _check_consumer_rows(case, variant, epi, got, r0, r1, tag):
    """assertions (i) and (ii) on rows [r0, r1) of `got`; returns the largest ratio of (ii)'s error to its bound"""
    pre_kernel, pre_ln, tol_pre = case.rows(variant, r0, r1)
    g64 = got[r0:r1].double()
    want = _act64(epi, pre_kernel)                       # (i) the kernel's arithmetic
    err = (g64 - want).abs()
    tol_i = 2e-3 * want.abs().clamp(min=1.0)
    assert (err <= tol_i).all(), (tag, "identity", (err / tol_i).max().item())
    want_ln = _act64(epi, pre_ln)                        # (ii) the fold as a LayerNorm
    bound = _act_tol(epi, pre_ln, tol_pre) + 2e-3 * want_ln.abs().clamp(min=1.0)
    ratio = ((g64 - want_ln).abs() / bound).max().item()
    assert ratio <= 1.0, (tag, "layernorm", ratio)
    return ratio


def _check_zero_rows(case, variant, epi, got, tag):
    """(iii) padding rows: act(c2) rounded to fp16, exactly"""
    c2 = case.variants[variant].c2.double()[None, :]
    want = _act64(epi, c2).half()
    for r in _zero_rows(case.m):
        bad = (got[r:r + 1] != want).sum().item()
        assert bad == 0, (tag, "zero row", r, bad)


@pytest.mark.parametrize("variant", ["exact", "centred"])
@pytest.mark.parametrize("engine", ["8wave", "4wave"])
@pytest.mark.parametrize("m,n,k", [(256, 256, 256), (256, 512, 768), (512, 768, 1024),   # nparts 1, 3, 4
                                   (4352, 4096, 512)])   # nparts 2; 272 tiles: more than one per persistent workgroup
def test_fold_consumer(lib, m, n, k, engine, variant):
    """Consumer epilogues of both engines: (i) the kernel's arithmetic against the fp64 identity with its own constants,
    (ii) the result against the fp64 LayerNorm + projection it replaces, within the worst-case rounding of the folded weights
    (SiLU and GLU: that bound taken through the activation's Lipschitz constant), (iii) zero rows exactly act(c2)."""
    case = _fold_case(lib, m, n, k)
    assert case.nparts == {256: 1, 512: 2, 768: 3, 1024: 4}[k]
    worst = 0.0
    for epi, out_tm in CONSUMER_EPIS[engine][variant]:
        tag = (engine, variant, epi, out_tm)
        got, _ = _launch_consumer(lib, engine, case, variant, epi, out_tm, case.part)
        worst = max(worst, _check_consumer_rows(case, variant, epi, got, 0, m, tag))
        _check_zero_rows(case, variant, epi, got, tag)
    # the same sums spread over all nparts partials, as a producer leaves them (one per 256 columns of the stream)
    t = case.x.double().view(m, case.nparts, 256)
    spread = torch.stack([t.sum(2), (t * t).sum(2)], dim=2).permute(1, 0, 2).float().contiguous()
    got, _ = _launch_consumer(lib, engine, case, variant, BIAS, 1, spread, reps=1)
    _check_consumer_rows(case, variant, BIAS, got, 0, m, (engine, variant, "spread partials"))
    print(f"fold consumer {engine} {variant} m={m} n={n} k={k}: largest error / bound of (ii) = {worst:.3f}")


@pytest.mark.parametrize("engine", ["8wave", "4wave"])
def test_fold_consumer_xcd_raster(lib, engine):
    """1024 tiles on the XCD-owned raster (four per workgroup), bias, centred weights; compared a row tile at a time"""
    m, n, k = 16384, 4096, 256
    case = _fold_case(lib, m, n, k)
    got, info = _launch_consumer(lib, engine, case, "centred", BIAS, 1, case.part)
    assert info.raster != 0 and info.grid_x == 256
    worst = 0.0
    for r0 in range(0, m, 256):
        worst = max(worst, _check_consumer_rows(case, "centred", BIAS, got, r0, r0 + 256, (engine, r0)))
    _check_zero_rows(case, "centred", BIAS, got, engine)
    print(f"fold consumer {engine} centred m={m} n={n} k={k}: largest error / bound of (ii) = {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ d. producer
@functools.lru_cache(maxsize=1)
def _producer_case(m, n, k):
    gen = torch.Generator(device="cuda").manual_seed(m + 3 * n + k)
    x = (torch.randn(m, k, device="cuda", generator=gen) * 0.5).half()
    w = (torch.randn(n, k, device="cuda", generator=gen) * 0.05).half()
    bias = torch.randn(n, device="cuda", generator=gen)
    resid = torch.randn(m, n, device="cuda", generator=gen).half()
    return types.SimpleNamespace(x_tm=to_tile_major(x), w_tm=to_tile_major(w), bias=bias, resid=resid,
                                 resid_tm=to_tile_major(resid), prod=x.double() @ w.double().T)


def _launch_producer(lib, engine, epi, x_tm, w_tm, bias, stream_tm, m, n, k, fold=True):
    """the residual epilogue on the tile-major stream (a copy of stream_tm), on the 256x256 engine `engine` names"""
    from sonar_amd import _lib

    epi_sel = epi | _lib.SMI_GEMM_IN_TM | _lib.SMI_GEMM_OUT_TM | (2 << 8)
    out, part = stream_tm.clone(), _nan((n // 256, m, 2))
    with _lib.tuning(**ENGINES[engine]):
        info = _route(lib, epi_sel, m, n, k, n, bias is not None, FOLD_PRODUCER_SUMS if fold else FOLD_NONE, 0)
        if engine == "8wave":
            assert (info.engine, info.layout) == (PP256, 3), (info.engine, info.layout)
        else:
            assert (info.engine, info.flag) == (V2_RESID, int(fold)), (info.engine, info.flag)
        if fold:
            _lib.check(lib.smi_gemm_tn_ln_fold(epi_sel, x_tm.data_ptr(), w_tm.data_ptr(), _ptr(bias), out.data_ptr(), m, n, k, n,
                                               part.data_ptr(), None, None, 0, 0.0, 0, _stream()))
        else:
            _lib.check(lib.smi_gemm_tn(epi_sel, x_tm.data_ptr(), w_tm.data_ptr(), _ptr(bias), out.data_ptr(), m, n, k, n, _stream()))
        torch.cuda.synchronize()
    return out, part


def _check_partials(part, stream, m, n):
    """every partial = fp64 (sum, sum of squares) of the ROUNDED fp16 values of its row over its 256 columns; the factor 2
    covers the accumulation inside the dot-product instruction"""
    assert torch.isfinite(part).all()
    t = stream.double().view(m, n // 256, 256)
    got = part.double().permute(1, 0, 2)               # [m][tile][2]
    assert ((got[:, :, 0] - t.sum(2)).abs() <= 2 * 256 * U * t.abs().sum(2)).all()
    assert ((got[:, :, 1] - (t * t).sum(2)).abs() <= 2 * 256 * U * (t * t).sum(2)).all()


@pytest.mark.parametrize("use_bias", [True, False])
@pytest.mark.parametrize("epi", [RESID, RESID_HALF])
@pytest.mark.parametrize("engine", ["8wave", "4wave"])
@pytest.mark.parametrize("m,n,k", [(256, 256, 1024), (512, 1024, 256), (16640, 1024, 256)])   # the last: 260 tiles
def test_fold_producer(lib, m, n, k, engine, epi, use_bias):
    c = _producer_case(m, n, k)
    bias = c.bias if use_bias else None
    plain, _ = _launch_producer(lib, engine, epi, c.x_tm, c.w_tm, bias, c.resid_tm, m, n, k, fold=False)
    out, part = _launch_producer(lib, engine, epi, c.x_tm, c.w_tm, bias, c.resid_tm, m, n, k)
    assert torch.equal(out, plain)                     # leaving the sums does not change the stream
    got = from_tile_major(out, m, n)
    want = c.resid.double() + (1.0 if epi == RESID else 0.5) * (c.prod + (c.bias.double() if use_bias else 0))
    assert (got.double() - want).abs().max().item() <= 2e-3 * max(want.abs().max().item(), 1.0)
    _check_partials(part, got, m, n)


# --------------------------------------------------------------------------------------------------------------------- e. chain
@pytest.mark.parametrize("engine", ["8wave", "4wave"])
@pytest.mark.parametrize("variant", ["exact", "centred"])
def test_fold_chain(lib, engine, variant):
    """One producer into one consumer at stream width 1024: the consumer reads the four partials per row the producer left"""
    m, d, kp, n = 512, 1024, 256, 768
    gen = torch.Generator(device="cuda").manual_seed(17)
    resid = _fold_stream(m, d, gen)
    r = torch.arange(m, device="cuda")
    s = torch.tensor([0.25, 1.0, 4.0], device="cuda")[r % 3]
    a = (torch.randn(m, kp, device="cuda", generator=gen) * 0.5 * s[:, None]).half()    # an update of the row's own scale
    a[_zero_rows(m)] = 0                                                                # ... that keeps the zero rows zero
    wp = (torch.randn(d, kp, device="cuda", generator=gen) * 0.05).half()
    stream_tm, part = _launch_producer(lib, engine, RESID, to_tile_major(a), to_tile_major(wp), None, to_tile_major(resid), m, d, kp)
    stream = from_tile_major(stream_tm, m, d)
    assert not torch.equal(stream, resid) and (stream[_zero_rows(m)] == 0).all()
    _check_partials(part, stream, m, d)
    case = _FoldCase(lib, m, n, d, x=stream)
    assert case.nparts == 4 and (part.view(4, m, 2)[1:, 5].abs().sum() > 0)             # four real partials
    got, _ = _launch_consumer(lib, engine, case, variant, BIAS, 1, part.view(-1, 2), reps=1)
    _check_consumer_rows(case, variant, BIAS, got, 0, m, (engine, variant, "chain"))
    _check_zero_rows(case, variant, BIAS, got, (engine, variant, "chain"))
    ref, _ = _launch_consumer(lib, engine, case, variant, BIAS, 1, case.part, reps=1)   # fed by smi_row_stats_tm instead
    assert (got.double() - ref.double()).abs().max().item() <= 2e-3 * max(ref.double().abs().max().item(), 1.0)


# ------------------------------------------------------------------------------------------------------------------ f. refusals
def test_fold_refusals(lib):
    """What no fold kernel computes is refused before anything is launched: the output keeps its sentinel"""
    from sonar_amd import _lib

    m = n = k = 256
    tm, otm = _lib.SMI_GEMM_IN_TM, _lib.SMI_GEMM_OUT_TM
    case = _fold_case(lib, m, n, k)
    v = case.variants["centred"]
    out = torch.full((m * n,), 1.5, device="cuda", dtype=torch.float16)
    part_out = torch.full((m, 2), 2.5, device="cuda")

    def call(epi_sel, ldo=n, x=case.x_tm, part_in=case.part, po=None, c1=v.c1, nparts=1, centered=1):
        return lib.smi_gemm_tn_ln_fold(epi_sel, x.data_ptr(), v.wf_tm.data_ptr(), v.c2.data_ptr(), out.data_ptr(), m, n, k, ldo,
                                       _ptr(po), _ptr(part_in), _ptr(c1), nparts, EPS, centered, _stream())

    both = [ENGINES["8wave"], ENGINES["4wave"]]
    cases = [("silu exact", both, dict(epi_sel=SILU | tm | otm, centered=0)),
             ("glu exact, tile-major out", both, dict(epi_sel=GLU | tm | otm, ldo=n // 2, centered=0)),
             ("glu exact, row-major out", both, dict(epi_sel=GLU | tm, ldo=n // 2, centered=0)),
             ("glu tile-major out on the 8-wave engine", both[:1], dict(epi_sel=GLU | tm | otm, ldo=n // 2)),
             ("relu row-major out", both, dict(epi_sel=RELU | tm)),
             ("nparts 0", both, dict(epi_sel=BIAS | tm | otm, nparts=0)),
             ("nparts 5", both, dict(epi_sel=BIAS | tm | otm, nparts=5)),
             ("c1 null", both, dict(epi_sel=BIAS | tm | otm, c1=None)),
             ("engine selector 1", both, dict(epi_sel=BIAS | tm | otm | (1 << 8))),
             ("row-major operands", both, dict(epi_sel=BIAS, x=case.x)),
             ("producer, row-major out", both, dict(epi_sel=RESID | tm, part_in=None, po=part_out, c1=None, nparts=0))]
    for name, tunings, kw in cases:
        for t in tunings:
            out.fill_(1.5)
            with _lib.tuning(**t):
                assert call(**kw) == UNSUPPORTED, (name, t)
            torch.cuda.synchronize()
            assert (out == 1.5).all() and (part_out == 2.5).all(), (name, t)
    assert call(BIAS | tm | otm, po=part_out) == INVALID_ARG       # a fold is a producer or a consumer
    torch.cuda.synchronize()
    assert (out == 1.5).all() and (part_out == 2.5).all()
    with _lib.tuning(**ENGINES["8wave"]):                          # the same call without the fault is taken
        assert call(BIAS | tm | otm) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not (out == 1.5).all()
