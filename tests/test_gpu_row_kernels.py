"""GPU: the conformer and decoder row kernels one at a time, through their C-ABI building blocks, against the float64
restatements of tests/row_kernels_ref.py on the same fp16 / fp32 inputs: stack_ln, ln2, dwconv_bn_silu, pool_attention
(csrc/speech.hip), sum_layernorm, dec_attention (csrc/decoder.hip) and the CAUSAL instantiation of csrc/attention.hip.

Rules of every test here:
 * outputs start as NaN; afterwards every element the kernel owns is finite and within tolerance and every other element is
   still NaN (rows past the last clip, padding rows of a tile-major image, rows >= rows); input rows that no clip owns are
   NaN too (rows after the last clip, KV-slab rows rows..rows_pad-1, the slab after position pos), so a read of one shows;
 * every kernel is called twice on the same inputs and the two results are bit-identical;
 * no element is left out of a comparison;
 * rule T for the fp32-arithmetic kernels, elementwise: |got - ref| <= ulp16(ref) + 2^-14 A.  The first term is one fp16
   ulp of the reference (half of it the output rounding): 2^-10 |ref|, and 2^-24 below 2^-14, where fp16 is subnormal
   (row_kernels_ref.py: the exact rounding of such a reference already misses 2^-10 |ref|).  A is the magnitude at which the
   fp32 arithmetic ran (per kernel in row_kernels_ref.py) and the second term allows for it at 1/8 of an fp16 half-ulp.  causal_attention rounds its
   probabilities to fp16 for the MFMAs like attention_kernel and takes test_attention's bound: 6e-3 absolute at qkv = randn * 1.5.
Each test prints its worst error / bound."""
import pytest
import torch

from tests import row_kernels_ref as R
from tests.tile_major import from_tile_major, to_tile_major

pytestmark = pytest.mark.gpu

EPS = 1e-5
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib

    lib = _lib.load()
    _lib.check(lib.smi_init(0))
    return lib


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _nan(shape, dtype):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), NAN, device="cuda", dtype=dtype)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _pad256(rows):
    return (rows + 255) // 256 * 256


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    """bit-identical, NaN poison included"""
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b) if x is not None)


def _cu(lens):
    return torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device="cuda")


def _ratio(got, ref, bound, what):
    """every element finite and within its bound; returns the worst error / bound"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    got = got.double()
    assert torch.isfinite(got).all(), (what, "not finite", (~torch.isfinite(got)).nonzero()[:4].tolist())
    err = (got - ref).abs()
    bad = err > bound
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    assert not bad.any(), (what, "error / bound", ratio, "at", bad.nonzero()[:4].tolist())
    return ratio


def _check_t(got, ref, mag, what, extra=None):
    bound = R.tolerance(ref, mag)
    return _ratio(got, ref, bound if extra is None else bound + extra, what)


def _untouched(t, what):
    assert torch.isnan(t).all(), (what, "rows the kernel does not own were written", (~torch.isnan(t)).nonzero()[:4].tolist())


def _ln_weights(d, g):
    return 1 + 0.3 * torch.randn(d, device="cuda", generator=g), 0.2 * torch.randn(d, device="cuda", generator=g)


def _rows_with_scales(rows, d, g):
    """randn * s_r + o_r * s_r, s_r cycling through 3 scales and o_r through 4 mean-to-std ratios"""
    r = torch.arange(rows, device="cuda")
    s = torch.tensor([0.25, 1.0, 4.0], device="cuda")[r % 3]
    o = torch.tensor([0.0, 0.5, -0.5, 0.25], device="cuda")[r % 4]
    return torch.randn(rows, d, device="cuda", generator=g) * s[:, None] + (o * s)[:, None]


# ---------------------------------------------------------------------------------------------------------------- stack_ln
@pytest.mark.parametrize("ldo", [192, 160])
def test_stack_ln(lib, ldo):
    """Frame stacking + LayerNorm(160): clips of 20, 1, 0, 7 and 13 stacked frames (a full grid row, a lone frame, an empty
    clip, waves past the clip's end inside a workgroup), max_len = 22 (the last workgroup of every clip is partly idle); the
    fbank frames no stacked frame owns are NaN; columns 160..ldo-1 exactly zero."""
    from sonar_amd import _lib

    n, t, nb, lens, max_len = 5, 40, 80, [20, 1, 0, 7, 13], 22
    g = _gen(ldo)
    fb = torch.randn(n, t, nb, device="cuda", generator=g) * 2 + 1
    fb *= torch.tensor([1.0, 0.1, 1.0, 8.0, 0.5], device="cuda")[:, None, None]
    for i, L in enumerate(lens):
        fb[i, 2 * L:] = NAN
    w, b = _ln_weights(2 * nb, g)
    rows = sum(lens)
    outs = []
    for rep in range(2):
        out = _nan((rows + 3, ldo), torch.float16)
        _lib.check(lib.smi_stack_ln(fb.data_ptr(), n, t, nb, _cu(lens).data_ptr(), max_len, w.data_ptr(), b.data_ptr(), EPS,
                                    out.data_ptr(), ldo, _stream()))
        torch.cuda.synchronize()
        outs.append(out)
    assert _same(outs[:1], outs[1:])
    ref, mag = R.stack_ln(fb, lens, w, b, EPS, ldo)
    ratio = _check_t(outs[0][:rows], ref, mag, "stack_ln")
    assert (outs[0][:rows, 2 * nb:] == 0).all()
    _untouched(outs[0][rows:], "stack_ln")
    print(f"stack_ln ldo={ldo}: worst err / tol = {ratio:.3f}")


# --------------------------------------------------------------------------------------------------------------------- ln2
@pytest.mark.parametrize("stream", ["f32", "f16"])
@pytest.mark.parametrize("d", [256, 512, 768, 1024, 2048])
def test_ln2(lib, d, stream):
    """x <- LN1(x) in place, h = f16(w2 ? LN2(x) : x): the fp32 path, the one-row-per-wave fp16 path (d = 256, 768) and the
    row-pair fp16 path (d = 512, 1024, 2048), each with h row-major / tile-major / absent, with and without the second
    LayerNorm and (fp16, d % 512 == 0) with the stream itself tile-major; rows = 1, 37 (an odd count: the second half of the
    last row pair is dead) and 264 (across a 256-row tile).  The returned x against the fp64 LN1 of the input, within T for an
    fp16 stream; h against the fp64 LN2 of the x the kernel RETURNED, within T.

    The fp32 stream: |x - ref| <= 2^-20 (A + |w| mean_i |x_i| rstd).  The second term is not in rule T's A.  The kernel forms
    mean = sum / d in fp32 (ln_core.hpp), off by a few ulp of mean_i |x_i|; that offset shifts EVERY centred value, and at an
    element with x ~ mean and b ~ 0 the plain A = |w| |x - mean| rstd + |b| is next to nothing while the shift is not: against
    2^-20 A alone the kernel measured 10.9 / 14.3 / 10.0 / 34.2 / 28.1 times the bound at d = 256 ... 2048, only at such
    elements (the rounding of any fp32 mean; no defect).  With the mean's magnitude in the bound the worst ratio is
    0.17 - 0.20, what torch's own fp32 layer_norm reaches on the same rows; both figures are printed below."""
    from sonar_amd import _lib

    f16 = stream == "f16"
    xdt = torch.float16 if f16 else torch.float32
    g = _gen(d + f16)
    w1, b1 = _ln_weights(d, g)
    w2, b2 = _ln_weights(d, g)
    worst_x = worst_h = plain_x = 0.0
    for rows in (1, 37, 264):
        pad = _pad256(rows)
        x0 = _rows_with_scales(rows, d, g).to(xdt)
        ref_x, mag_x = R.ln2_stream(x0, w1, b1, EPS)
        mean_x = R.layer_norm_mean_term(x0, w1, EPS)
        forms = [(h_tm, second, x_tm, True) for h_tm in (0, 1) for second in (True, False)
                 for x_tm in ((0, 1) if f16 and d % 512 == 0 else (0,))]
        forms += [(0, True, x_tm, False) for x_tm in ((0, 1) if f16 and d % 512 == 0 else (0,))]   # h = null: in place only
        for h_tm, second, x_tm, with_h in forms:
            what = ("ln2", d, stream, rows, "h_tm", h_tm, "ln2", second, "x_tm", x_tm, "h", with_h)
            runs = []
            for rep in range(2):
                xb = (to_tile_major(torch.cat([x0, _nan((pad - rows, d), xdt)])) if x_tm
                      else torch.cat([x0, _nan((3, d), xdt)]))
                h = None if not with_h else (_nan(pad * d, torch.float16) if h_tm else _nan((rows + 3, d), torch.float16))
                _lib.check(lib.smi_ln2(xb.data_ptr(), _lib.SMI_F16 if f16 else _lib.SMI_F32, w1.data_ptr(), b1.data_ptr(),
                                       _ptr(w2) if second else None, _ptr(b2) if second else None, EPS, _ptr(h), rows, d,
                                       h_tm | (x_tm << 1), _stream()))
                torch.cuda.synchronize()
                runs.append((xb, h))
            assert _same(runs[0], runs[1]), what
            xa = from_tile_major(runs[0][0], pad, d) if x_tm else runs[0][0]
            if f16:
                worst_x = max(worst_x, _check_t(xa[:rows], ref_x, mag_x, what))
            else:
                worst_x = max(worst_x, _ratio(xa[:rows], ref_x, 2.0 ** -20 * (mag_x + mean_x), what))
                plain_x = max(plain_x, ((xa[:rows].double() - ref_x).abs() / (2.0 ** -20 * mag_x)).max().item())
            _untouched(xa[rows:], what)
            if with_h:
                ha = from_tile_major(runs[0][1], pad, d) if h_tm else runs[0][1]
                ref_h, mag_h = R.ln2_out(xa[:rows], w2 if second else None, b2 if second else None, EPS)
                worst_h = max(worst_h, _check_t(ha[:rows], ref_h, mag_h, what))
                _untouched(ha[rows:], what)
    note = "" if f16 else f" ({plain_x:.2f} of 2^-20 A without the mean's term)"
    print(f"ln2 d={d} {stream} stream: worst err / bound of x = {worst_x:.3f}{note}, worst err / tol of h = {worst_h:.3f}")


# ---------------------------------------------------------------------------------------------------------- dwconv_bn_silu
DW_LENS = [1, 15, 16, 0, 31, 32, 33, 64, 65, 100]


@pytest.mark.parametrize("layout", [0, 1, 2, 3])
@pytest.mark.parametrize("d", [256, 512])
@pytest.mark.parametrize("ktaps", [7, 31])
def test_dwconv_bn_silu(lib, ktaps, d, layout):
    """Depthwise conv + BatchNorm + SiLU over packed clips shorter than the 15-frame halo, on and either side of the
    32-frame tile, over several tiles, and one empty clip; x and y row-major and tile-major.  The taps are NOT
    fp16-representable: within T of the reference with fp16-ROUNDED taps (the kernel's contract), and within T + 2^-11 A
    (one fp16 rounding of every tap) of the reference with the fp32 taps -- rounded to fp16, and no coarser."""
    from sonar_amd import _lib

    lens, max_len = DW_LENS, 100
    rows, pad = sum(lens), _pad256(sum(lens))
    g = _gen(ktaps * 1000 + d + layout)
    x = torch.randn(rows, d, device="cuda", generator=g).half()
    w = torch.randn(d, ktaps, device="cuda", generator=g) * 0.3
    assert (w.half().float() != w).float().mean().item() > 0.9
    scale = 1 + 0.3 * torch.randn(d, device="cuda", generator=g)
    shift = 0.2 * torch.randn(d, device="cuda", generator=g)
    xin = torch.cat([x, _nan((pad - rows, d), torch.float16)])
    if layout & 2:
        xin = to_tile_major(xin)
    cu = _cu(lens)
    outs = []
    for rep in range(2):
        y = _nan(pad * d, torch.float16)
        _lib.check(lib.smi_dwconv_bn_silu(xin.data_ptr(), cu.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                          y.data_ptr(), len(lens), max_len, d, ktaps, layout, _stream()))
        torch.cuda.synchronize()
        outs.append(y)
    assert _same(outs[:1], outs[1:])
    got = from_tile_major(outs[0], pad, d) if layout & 1 else outs[0].view(pad, d)
    ref16, mag16 = R.dwconv_bn_silu(x, lens, w, scale, shift, round_taps=True)
    ref32, mag32 = R.dwconv_bn_silu(x, lens, w, scale, shift, round_taps=False)
    r16 = _check_t(got[:rows], ref16, mag16, "fp16 taps")
    r32 = _check_t(got[:rows], ref32, mag32, "fp32 taps", extra=2.0 ** -11 * mag32)
    _untouched(got[rows:], "dwconv")
    off16 = ((got[:rows].double() - ref32).abs() / R.tolerance(ref32, mag32)).max().item()
    print(f"dwconv ktaps={ktaps} d={d} layout={layout}: worst err / tol = {r16:.3f} (fp16-tap reference), "
          f"{r32:.3f} of T + 2^-11 A (fp32-tap reference; {off16:.2f} of T alone)")


# ---------------------------------------------------------------------------------------------------------- pool_attention
@pytest.mark.parametrize("heads,d", [(1, 64), (4, 256), (16, 1024)])
def test_pool_attention(lib, heads, d):
    """One query per clip and head: clips of 1 row, either side of and on the 64-key round, several rounds, and an empty clip
    (context exactly zero); heads = 1: 7 waves, the last workgroup partly used."""
    from sonar_amd import _lib

    lens = [1, 63, 64, 65, 0, 129, 300]
    n, rows = len(lens), sum(lens)
    g = _gen(heads)
    q = torch.cat([torch.randn(n, d, device="cuda", generator=g).half(), _nan((1, d), torch.float16)])
    kv = torch.cat([torch.randn(rows, 2 * d, device="cuda", generator=g).half(), _nan((3, 2 * d), torch.float16)])
    cu = _cu(lens)
    outs = []
    for rep in range(2):
        ctx = _nan((n + 1, d), torch.float16)
        _lib.check(lib.smi_pool_attention(q.data_ptr(), kv.data_ptr(), cu.data_ptr(), ctx.data_ptr(), n, d, heads, _stream()))
        torch.cuda.synchronize()
        outs.append(ctx)
    assert _same(outs[:1], outs[1:])
    ref, mag = R.pool_attention(q[:n], kv[:rows], lens, heads)
    ratio = _check_t(outs[0][:n], ref, mag, "pool_attention")
    assert (outs[0][lens.index(0)] == 0).all()
    _untouched(outs[0][n:], "pool_attention")
    print(f"pool_attention heads={heads}: worst err / tol = {ratio:.3f}")


# ----------------------------------------------------------------------------------------------------------- sum_layernorm
SL_ROWS, SL_PAD = 37, 64


@pytest.mark.parametrize("slabs", ["f32", "f16"])
@pytest.mark.parametrize("stream", ["f32", "f16"])
@pytest.mark.parametrize("d", [256, 768, 1024, 2048])
def test_sum_layernorm(lib, d, stream, slabs):
    """x <- x + sum_z parts[z] (+ c[row / 5]); h = f16(LN(x)): the straight-line slab counts 0 / 1 / 2 / 4 / 8 and the looped
    ones (3, 11; 8 at d = 2048), fp32 and fp16 stream and slabs, with and without the constant, h row-major and tile-major.
    37 rows of 64-row slabs, the other rows NaN.  An fp32 stream is BIT-identical to the fp32 sum in the documented order
    (x, slabs ascending, constant); an fp16 stream is within T of the fp64 sum; h within T of the fp64 LN of the stored x."""
    from sonar_amd import _lib

    rows, pad_rows, group = SL_ROWS, SL_PAD, 5
    xdt = torch.float16 if stream == "f16" else torch.float32
    pdt = torch.float16 if slabs == "f16" else torch.float32
    xcode, pcode = (_lib.SMI_F16 if t == "f16" else _lib.SMI_F32 for t in (stream, slabs))
    g = _gen(d * 4 + (stream == "f16") * 2 + (slabs == "f16"))
    w, b = _ln_weights(d, g)
    x0 = torch.cat([_rows_with_scales(rows, d, g).to(xdt), _nan((pad_rows - rows, d), xdt)])
    parts_all = (torch.randn(11, pad_rows, d, device="cuda", generator=g) * 0.7).to(pdt)
    parts_all[:, rows:] = NAN
    c_all = torch.randn((rows + group - 1) // group, d, device="cuda", generator=g)
    worst_x = worst_h = 0.0
    for nparts in (0, 1, 2, 3, 4, 8, 11):
        parts = parts_all[:nparts].contiguous() if nparts else None
        for c in (None, c_all):
            for h_tm in (0, 1):
                what = ("sum_layernorm", d, stream, slabs, "nparts", nparts, "c", c is not None, "h_tm", h_tm)
                runs = []
                for rep in range(2):
                    x = x0.clone()
                    h = _nan(256 * d, torch.float16) if h_tm else _nan((pad_rows, d), torch.float16)
                    _lib.check(lib.smi_sum_layernorm(x.data_ptr(), xcode, _ptr(parts), pcode, nparts, pad_rows * d, _ptr(c),
                                                     group if c is not None else 1, w.data_ptr(), b.data_ptr(), EPS, h.data_ptr(), rows, d, h_tm, None, 0, _stream()))
                    torch.cuda.synchronize()
                    runs.append((x, h))
                assert _same(runs[0], runs[1]), what
                x, h = runs[0]
                if stream == "f32":
                    assert torch.equal(x[:rows], R.sum_stream_f32(x0[:rows], parts, c, group)), what
                else:
                    ref_x, mag_x = R.sum_stream(x0[:rows], parts, c, group)
                    worst_x = max(worst_x, _check_t(x[:rows], ref_x, mag_x, what))
                _untouched(x[rows:], what)
                ha = from_tile_major(h, 256, d) if h_tm else h
                ref_h, mag_h = R.layer_norm(x[:rows], w, b, EPS)
                worst_h = max(worst_h, _check_t(ha[:rows], ref_h, mag_h, what))
                _untouched(ha[rows:], what)
    xs = "bit-identical to the fp32 sum" if stream == "f32" else f"worst err / tol = {worst_x:.3f}"
    print(f"sum_layernorm d={d} {stream} stream, {slabs} slabs: x {xs}; h worst err / tol = {worst_h:.3f}")


@pytest.mark.parametrize("d", [256, 768, 1024, 2048])
def test_sum_layernorm_prefetch_changes_nothing(lib, d):
    """With a prefetch buffer and 37 rows (10 workgroups of row work) the launch carries surplus workgroups that stream the
    buffer through the cache: x and h are bit-identical to the call without it."""
    from sonar_amd import _lib

    rows, pad_rows = SL_ROWS, SL_PAD
    g = _gen(d)
    w, b = _ln_weights(d, g)
    x0 = torch.cat([_rows_with_scales(rows, d, g), _nan((pad_rows - rows, d), torch.float32)])
    parts = (torch.randn(2, pad_rows, d, device="cuda", generator=g) * 0.7).half()
    parts[:, rows:] = NAN
    pf = torch.randn(1 << 18, device="cuda", generator=g)   # 1 MiB
    pf0 = pf.clone()
    runs = []
    for prefetch in (None, pf, pf):
        x, h = x0.clone(), _nan((pad_rows, d), torch.float16)
        _lib.check(lib.smi_sum_layernorm(x.data_ptr(), _lib.SMI_F32, parts.data_ptr(), _lib.SMI_F16, 2, pad_rows * d, None, 1,
                                         w.data_ptr(), b.data_ptr(), EPS, h.data_ptr(), rows, d, 0, _ptr(prefetch),
                                         pf.numel() * 4 if prefetch is not None else 0, _stream()))
        torch.cuda.synchronize()
        runs.append((x, h))
    assert _same(runs[0], runs[1]) and _same(runs[1], runs[2])
    assert torch.equal(pf, pf0)
    assert torch.equal(runs[1][0][:rows], R.sum_stream_f32(x0[:rows], parts, None, 1))
    ref_h, mag_h = R.layer_norm(runs[1][0][:rows], w, b, EPS)
    ratio = _check_t(runs[1][1][:rows], ref_h, mag_h, "prefetch")
    _untouched(runs[1][1][rows:], "prefetch")
    print(f"sum_layernorm d={d} with a 1 MiB prefetch: bit-identical to the call without; h worst err / tol = {ratio:.3f}")


# ----------------------------------------------------------------------------------------------------------- dec_attention
# NG (8-position groups per pass) and passes of launch_dec_attention: pos 0, 7 -> NG 1; 8 -> 2; 16 -> 3; 24 -> 4; 32 -> 5; 40 -> 6;
# 48 -> 7; 63 -> 8 (one pass each); 64 -> 5 x 2 passes; 100, 127 -> 7 / 8 x 2; 128 -> 6 x 3; 200 -> 7 x 4; 511 -> 8 x 8
@pytest.mark.parametrize("heads,rows,pos", [(4, 37, p) for p in (0, 7, 8, 16, 24, 32, 40, 48, 63, 64, 100, 127, 128, 200, 511)]
                         + [(16, 5, 0), (16, 5, 70)])
def test_dec_attention(lib, heads, rows, pos):
    """Single-query attention over the position slabs with random ancestry: every chunk size with one pass, 2 / 3 / 4 / 8 passes,
    the last chunk partly masked in most cases.  Slab rows rows..rows_pad-1 and the slab after position pos are NaN."""
    from sonar_amd import _lib

    d, rows_pad = heads * 64, 64
    g = _gen(pos * 17 + heads)
    kv = _nan((pos + 2, rows_pad, 3 * d), torch.float16)
    kv[:pos + 1, :rows] = torch.randn(pos + 1, rows, 3 * d, device="cuda", generator=g).half()
    anc_stride = pos + 3
    anc = torch.randint(0, rows, (rows, anc_stride), device="cuda", generator=g, dtype=torch.int32)
    outs = []
    for rep in range(2):
        ctx = _nan((rows_pad, d), torch.float16)
        _lib.check(lib.smi_dec_attention(kv.data_ptr(), anc.data_ptr(), anc_stride, ctx.data_ptr(), rows, rows_pad, d, heads, pos,
                                         _stream()))
        torch.cuda.synchronize()
        outs.append(ctx)
    assert _same(outs[:1], outs[1:])
    ref, mag = R.dec_attention(kv, anc, rows, d, heads, pos)
    ratio = _check_t(outs[0][:rows], ref, mag, "dec_attention")
    _untouched(outs[0][rows:], "dec_attention")
    print(f"dec_attention heads={heads} rows={rows} pos={pos}: worst err / tol = {ratio:.3f}")


# -------------------------------------------------------------------------------------------------------- causal_attention
@pytest.mark.parametrize("seq", [1, 5, 64, 65, 128, 129, 200, 300])
@pytest.mark.parametrize("heads", [2, 16])
def test_causal_attention(lib, heads, seq):
    """Three sequences of `seq` rows, query i sees keys 0..i: the 64-key tile and the 128-query block on and either side of
    their boundaries.  The project's own attention bound (test_attention): 6e-3 absolute with qkv = randn * 1.5."""
    from sonar_amd import _lib

    nseq, d = 3, heads * 64
    rows = nseq * seq
    g = _gen(seq + heads)
    qkv = torch.cat([(torch.randn(rows, 3 * d, device="cuda", generator=g) * 1.5).half(), _nan((5, 3 * d), torch.float16)])
    cu = _cu([seq] * nseq)
    outs = []
    for rep in range(2):
        ctx = _nan((rows + 5, d), torch.float16)
        _lib.check(lib.smi_causal_attention(qkv.data_ptr(), cu.data_ptr(), ctx.data_ptr(), nseq, seq, d, heads, _stream()))
        torch.cuda.synchronize()
        outs.append(ctx)
    assert _same(outs[:1], outs[1:])
    ref, _ = R.causal_attention(qkv, nseq, seq, d, heads)
    ratio = _ratio(outs[0][:rows], ref, torch.full_like(ref, 6e-3), "causal_attention")
    _untouched(outs[0][rows:], "causal_attention")
    print(f"causal_attention heads={heads} seq={seq}: worst err / 6e-3 = {ratio:.3f}")
