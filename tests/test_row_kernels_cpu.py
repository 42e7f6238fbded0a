"""CPU: (a) the float64 references of tests/row_kernels_ref.py against independent torch formulations of the same operations, to
1e-12; (b) every refusal of the seven row-kernel building blocks (include/sonar_mi355.h) is decided before the device is asked
for, returns its code and leaves its text in smi_last_error."""
import pytest
import torch
import torch.nn.functional as F

from tests import row_kernels_ref as R

INVALID_ARG, UNSUPPORTED, NO_DEVICE = -1, -2, -3
EPS = 1e-5


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1.0), (a - b).abs().max().item()


# ------------------------------------------------------------------------------------------------- (a) reference self-checks
def test_layer_norm_refs_match_functional():
    g = torch.Generator().manual_seed(1)
    for d in (160, 256, 768):
        x = torch.randn(9, d, generator=g) * 3 + 0.7
        w, b = 1 + 0.3 * torch.randn(d, generator=g), 0.2 * torch.randn(d, generator=g)
        want = F.layer_norm(x.double(), (d,), w.double(), b.double(), EPS)
        y, mag = R.layer_norm(x, w, b, EPS)
        _close(y, want)
        assert (mag >= y.abs() - 1e-12).all()   # A bounds the result's magnitude
        _close(R.ln2_stream(x, w, b, EPS)[0], want)
        _close(R.ln2_out(x, w, b, EPS)[0], want)
        _close(R.ln2_out(x.half(), None, None, EPS)[0], x.half().double())
        std = torch.sqrt(x.double().var(-1, unbiased=False, keepdim=True) + EPS)
        _close(R.layer_norm_mean_term(x, w, EPS), w.double().abs() * x.double().abs().mean(-1, keepdim=True) / std)


def test_stack_ln_ref_matches_functional():
    g = torch.Generator().manual_seed(2)
    n, t, nb, lens = 3, 12, 80, [6, 0, 3]
    fb = torch.randn(n, t, nb, generator=g) * 2 + 1
    w, b = 1 + 0.3 * torch.randn(2 * nb, generator=g), 0.2 * torch.randn(2 * nb, generator=g)
    y, mag = R.stack_ln(fb, lens, w, b, EPS, 192)
    assert y.shape == (9, 192) and (y[:, 160:] == 0).all() and (mag[:, 160:] == 0).all()
    row = 0
    for i, L in enumerate(lens):
        for j in range(L):
            frame = torch.cat([fb[i, 2 * j], fb[i, 2 * j + 1]]).double()
            _close(y[row, :160], F.layer_norm(frame, (160,), w.double(), b.double(), EPS))
            row += 1
    assert R.stack_ln(fb, lens, w, b, EPS, 160)[0].shape == (9, 160)


@pytest.mark.parametrize("K", [7, 31])
def test_dwconv_ref_matches_conv1d(K):
    g = torch.Generator().manual_seed(K)
    C, lens = 16, [1, 15, 16, 0, 33, 40]
    x = torch.randn(sum(lens), C, generator=g).half()
    w = torch.randn(C, K, generator=g) * 0.3
    scale, shift = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    assert not torch.equal(w.half().float(), w)
    for rounded in (True, False):
        y, mag = R.dwconv_bn_silu(x, lens, w, scale, shift, round_taps=rounded)
        taps = (w.half() if rounded else w).double()
        o = 0
        for L in lens:
            if L:
                conv = F.conv1d(x[o:o + L].double().T[None], taps[:, None, :], groups=C, padding=(K - 1) // 2)[0].T
                _close(y[o:o + L], F.silu(scale.double() * conv + shift.double()))
                assert (mag[o:o + L] >= (scale.double() * conv + shift.double()).abs() - 1e-12).all()
            o += L
    assert (R.dwconv_bn_silu(x, lens, w, scale, shift, True)[0] - R.dwconv_bn_silu(x, lens, w, scale, shift, False)[0]).abs().max() > 1e-5


def test_pool_attention_ref_matches_sdpa():
    g = torch.Generator().manual_seed(3)
    heads, d, lens = 4, 256, [1, 5, 0, 70]
    q = torch.randn(len(lens), d, generator=g).half()
    kv = torch.randn(sum(lens), 2 * d, generator=g).half()
    ctx, mag = R.pool_attention(q, kv, lens, heads)
    o = 0
    for i, L in enumerate(lens):
        if L == 0:
            assert (ctx[i] == 0).all()
            continue
        k = kv[o:o + L, :d].double().view(L, heads, 64).transpose(0, 1)
        v = kv[o:o + L, d:].double().view(L, heads, 64).transpose(0, 1)
        want = F.scaled_dot_product_attention(q[i].double().view(heads, 1, 64), k, v)
        _close(ctx[i], want.reshape(d))
        assert (mag[i] >= ctx[i].abs() - 1e-12).all()
        o += L


def test_sum_refs():
    g = torch.Generator().manual_seed(4)
    rows, d = 7, 256
    x = torch.randn(rows, d, generator=g)
    parts = torch.randn(3, 10, d, generator=g).half()          # slab rows past `rows` are not the kernel's
    c = torch.randn(2, d, generator=g)
    want = x.double() + parts[:, :rows].double().sum(0) + c.double().repeat_interleave(5, 0)[:rows]
    _close(R.sum_stream(x, parts, c, 5)[0], want)
    _close(R.sum_stream_f32(x, parts, c, 5).double(), want, 1e-6)
    _close(R.sum_stream(x, None, None, 1)[0], x.double())
    assert torch.equal(R.sum_stream_f32(x, None, None, 1), x)
    assert torch.equal(R.sum_stream_f32(x, parts[:1], None, 1), x + parts[0, :rows].float())


@pytest.mark.parametrize("pos", [0, 1, 9])
def test_dec_attention_ref_matches_dense_attention_over_gathered_rows(pos):
    g = torch.Generator().manual_seed(pos)
    rows, rows_pad, heads = 5, 8, 2
    d = heads * 64
    kv = torch.randn(pos + 1, rows_pad, 3 * d, generator=g).half()
    anc = torch.randint(0, rows, (rows, pos + 2), generator=g, dtype=torch.int32)
    ctx, mag = R.dec_attention(kv, anc, rows, d, heads, pos)
    for r in range(rows):
        picked = torch.stack([kv[j, int(anc[r, j])] for j in range(pos)] + [kv[pos, r]]).double()   # [pos+1][3d]
        k = picked[:, d:2 * d].view(pos + 1, heads, 64).transpose(0, 1)
        v = picked[:, 2 * d:].view(pos + 1, heads, 64).transpose(0, 1)
        want = F.scaled_dot_product_attention(kv[pos, r, :d].double().view(heads, 1, 64), k, v)
        _close(ctx[r], want.reshape(d))
        _close(mag[r], v.abs().max(1).values.reshape(d))


@pytest.mark.parametrize("seq", [1, 5, 70])
def test_causal_attention_ref_matches_sdpa(seq):
    g = torch.Generator().manual_seed(seq)
    nseq, heads = 3, 2
    d = heads * 64
    qkv = (torch.randn(nseq * seq + 2, 3 * d, generator=g) * 1.5).half()
    ctx, mag = R.causal_attention(qkv, nseq, seq, d, heads)
    t = qkv[:nseq * seq].double().view(nseq, seq, 3, heads, 64)
    q, k, v = (t[:, :, i].transpose(1, 2) for i in range(3))
    want = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(nseq * seq, d)
    _close(ctx, want)
    assert (mag >= ctx.abs() - 1e-12).all()
    _close(mag.view(nseq, seq, d)[:, 0], qkv[:nseq * seq, 2 * d:].double().abs().view(nseq, seq, d)[:, 0])


def test_tolerance_rule():
    ref = torch.tensor([2.0, 2.0 ** -14, 1e-6, 0.0], dtype=torch.float64)
    mag = torch.tensor([4.0, 0.0, 1e-6, 1.0], dtype=torch.float64)
    want = [2.0 ** -9 + 2.0 ** -12, 2.0 ** -24, 2.0 ** -24 + 2.0 ** -14 * 1e-6, 2.0 ** -24 + 2.0 ** -14]
    assert torch.equal(R.tolerance(ref, mag), torch.tensor(want, dtype=torch.float64))
    # one fp16 ulp of the reference, the subnormal range included: the correct rounding of any value is within half of it
    v = torch.logspace(-9, 4, 20001, dtype=torch.float64).float()   # fp32 values: one rounding on the way to fp16
    v = torch.cat([v, -v]).double()
    assert ((v.float().half().double() - v).abs() <= 0.5 * R.tolerance(v, torch.zeros_like(v))).all()
    assert ((v.float().half().double() - v).abs() > 2.0 ** -10 * v.abs()).any()   # ... which 2^-10 |ref| alone does not grant


# ------------------------------------------------------------------------------------------------------------ (b) refusals
@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def test_refusals_need_no_device(lib):
    from sonar_amd import _lib

    if lib.smi_device_count() > 0:
        pytest.skip("a HIP device is visible: the made-up pointers must never reach a kernel")
    p, F32, F16 = 0x1000, _lib.SMI_F32, _lib.SMI_F16   # never dereferenced: every call below is refused
    good = {
        "smi_stack_ln": dict(fbank=p, n=5, t=40, nb=80, cu=p, max_len=22, w=p, b=p, eps=EPS, out=p, ldo=192, stream=None),
        "smi_ln2": dict(x=p, x_dtype=F16, w1=p, b1=p, w2=p, b2=p, eps=EPS, h=p, rows=37, d=512, layout=3, stream=None),
        "smi_dwconv_bn_silu": dict(x=p, cu=p, w=p, scale=p, shift=p, y=p, n=10, max_len=100, d=256, ktaps=31, layout=0, stream=None),
        "smi_pool_attention": dict(q=p, kv=p, cu=p, ctx=p, n=7, d=256, heads=4, stream=None),
        "smi_sum_layernorm": dict(x=p, x_dtype=F32, parts=p, parts_dtype=F16, nparts=3, part_stride=64 * 256, c=p, group=5, w=p, b=p,
                                  eps=EPS, h=p, rows=37, d=256, h_tm=0, prefetch=None, prefetch_bytes=0, stream=None),
        "smi_dec_attention": dict(kv=p, anc=p, anc_stride=10, ctx=p, rows=37, rows_pad=64, d=256, heads=4, pos=7, stream=None),
        "smi_causal_attention": dict(qkv=p, cu=p, ctx=p, nseq=3, seq=65, d=128, heads=2, stream=None),
    }
    A, U = INVALID_ARG, UNSUPPORTED
    cases = {
        "smi_stack_ln": [({k: None}, A, "null argument") for k in ("fbank", "cu", "w", "b", "out")] + [
            ({"n": 0}, A, "n=0"), ({"t": 0}, A, "t=0"), ({"max_len": 0}, A, "max_len=0"), ({"ldo": 159}, A, "ldo=159"),
            ({"nb": 97, "ldo": 194}, U, "2 nb <= ldo <= 192 (nb=97 ldo=194)"), ({"ldo": 193}, U, "2 nb <= ldo <= 192 (nb=80 ldo=193)"),
            ({"nb": 100, "ldo": 256}, U, "nb=100")],
        "smi_ln2": [({k: None}, A, "null argument") for k in ("x", "w1", "b1", "w2", "b2")] + [
            ({"x_dtype": 2}, A, "x_dtype=2"), ({"rows": 0}, A, "rows=0"), ({"layout": 4}, A, "layout=4"), ({"layout": -1}, A, "layout=-1"),
            ({"d": 0}, U, "d=0 unsupported"), ({"d": 384}, U, "d=384 unsupported"), ({"d": 1280}, U, "d=1280 unsupported"),
            ({"d": 4096}, U, "d=4096 unsupported"),
            ({"x_dtype": F32}, U, "tile-major stream is fp16"), ({"d": 768}, U, "d % 512 == 0 (x_dtype=1 d=768)"),
            ({"d": 256, "layout": 2}, U, "tile-major stream"), ({"x_dtype": F32, "layout": 2}, U, "x_dtype=0 d=512")],
        "smi_dwconv_bn_silu": [({k: None}, A, "null argument") for k in ("x", "cu", "w", "scale", "shift", "y")] + [
            ({"n": 0}, A, "n=0"), ({"max_len": 0}, A, "max_len=0"), ({"layout": 4}, A, "layout=4"),
            ({"d": 384}, U, "d=384 ktaps=31"), ({"d": 0}, U, "d=0"), ({"d": 64}, U, "d=64"),
            ({"ktaps": 15}, U, "ktaps=15"), ({"ktaps": 8}, U, "ktaps=8"), ({"ktaps": 0}, U, "ktaps=0")],
        "smi_pool_attention": [({k: None}, A, "null argument") for k in ("q", "kv", "cu", "ctx")] + [
            ({"n": 0}, A, "n=0"), ({"heads": 0}, U, "head_dim must be 64"), ({"d": 128}, U, "head_dim must be 64"),
            ({"heads": 8}, U, "head_dim must be 64")],
        "smi_sum_layernorm": [({k: None}, A, "null argument") for k in ("x", "w", "b", "h")] + [
            ({"x_dtype": 2}, A, "x_dtype=2"), ({"parts_dtype": 3}, A, "parts_dtype=3"), ({"rows": 0}, A, "rows=0"),
            ({"nparts": -1}, A, "nparts=-1"), ({"parts": None}, A, "parts null"), ({"group": 0}, A, "group=0"),
            ({"prefetch_bytes": -1}, A, "prefetch_bytes=-1"), ({"prefetch_bytes": 64}, A, "prefetch_bytes=64"),
            ({"part_stride": 37 * 256 - 1}, A, "overlap"),
            ({"d": 512 + 128}, U, "d=640 unsupported"), ({"d": 1536}, U, "d=1536 unsupported"), ({"d": 0}, U, "d=0 unsupported")],
        "smi_dec_attention": [({k: None}, A, "null argument") for k in ("kv", "anc", "ctx")] + [
            ({"d": 320}, U, "head_dim must be 64"), ({"heads": 0}, U, "head_dim must be 64"), ({"heads": 2}, U, "head_dim must be 64"),
            ({"pos": -1}, A, "pos=-1"), ({"rows": 0}, A, "rows=0"), ({"rows": 65}, A, "rows=65 rows_pad=64"),
            ({"anc_stride": 6}, A, "anc_stride=6")],
        "smi_causal_attention": [({k: None}, A, "null argument") for k in ("qkv", "cu", "ctx")] + [
            ({"nseq": 0}, A, "nseq=0"), ({"seq": 0}, A, "seq=0"), ({"d": 192}, U, "head_dim must be 64"),
            ({"heads": 0}, U, "head_dim must be 64")],
    }
    wrong = []
    for name, rows in cases.items():
        fn = getattr(lib, name)
        for change, code, text in rows:
            assert set(change) <= set(good[name]), (name, change)
            rc = fn(*{**good[name], **change}.values())
            err = lib.smi_last_error().decode()
            if rc != code or text not in err:
                wrong.append((name, change, code, text, rc, err))
        # the unchanged call passes every check and stops at the device
        rc = fn(*good[name].values())
        if rc != NO_DEVICE or "no HIP device visible" not in lib.smi_last_error().decode():
            wrong.append((name, "good", rc, lib.smi_last_error().decode()))
    assert not wrong, wrong
    # forms that are NOT refusals: no second LayerNorm, no output, no slabs, no constant, no ancestry at position 0
    for name, change in [("smi_ln2", {"w2": None, "b2": None}), ("smi_ln2", {"h": None}), ("smi_ln2", {"x_dtype": F32, "layout": 1}),
                         ("smi_sum_layernorm", {"parts": None, "nparts": 0}), ("smi_sum_layernorm", {"c": None, "group": 0}),
                         ("smi_sum_layernorm", {"nparts": 1, "part_stride": 0}), ("smi_dec_attention", {"anc": None, "pos": 0}),
                         ("smi_dwconv_bn_silu", {"ktaps": 7, "d": 1024, "layout": 3}), ("smi_stack_ln", {"ldo": 160})]:
        assert getattr(lib, name)(*{**good[name], **change}.values()) == NO_DEVICE, (name, change, lib.smi_last_error())
    assert lib.smi_abi_version() == 7   # the entry points are additions
