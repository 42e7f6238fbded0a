"""GPU: the four head_dim-64 MFMA attention kernels that share the online softmax of csrc/attn_core.hpp -- attention_kernel and its
CAUSAL instantiation (csrc/attention.hip), relpos_attention_kernel and relpos_attention_lds_kernel (csrc/relpos_attention.hip) --
through `smi_attention`, `smi_causal_attention` and `smi_relpos_attention`, against the float64 restatements of
tests/attention_ref.py on the same fp16 / fp32 inputs, on score patterns DESIGNED to move the lazy rescale to chosen places
(attention_ref.key_pattern; tests/test_attention_ref_cpu.py proves on a model of the schedule where each pattern rescales at
exactly these shapes) and on randn inputs, all under the derived elementwise bound attention_ref.bound.

Rules of every test here (those of tests/test_gpu_row_kernels.py):
 * outputs start as NaN; afterwards every element a clip owns is finite and within the bound and every other element is still
   NaN (rows after the last clip, the padding rows of a tile-major image);
 * qkv rows that no clip owns are NaN (rows after the last clip, the padding rows of a tile-major image): the kernels clamp
   their row index to len - 1 and must never read them -- a NaN key or value reaches the output through the MFMAs even with
   p = 0;
 * position-table rows that no (valid query, valid key) pair addresses after clamping hold a loud FINITE value, 1000, not NaN:
   both relpos kernels legitimately fetch whole aligned 32-row blocks of the table and form scores from them for keys and
   queries past the clip's end, which the tail mask and the store guard drop (attention_ref.poison_table);
 * every call runs twice on the same inputs and the two results are bit-identical;
 * no element is left out of a comparison;
 * |got - ref| <= ulp16(ref) + 2^-11 B + 2^-14 A elementwise, for the LDS-ring kernel on inexact position scores + 2 E B: derived
   in attention_ref.py, nothing fitted.
Each test prints its worst error / bound."""
import functools

import pytest
import torch

from tests import attention_ref as R
from tests.test_gpu_row_kernels import _cu, _nan, _pad256, _ratio, _same, _stream, _untouched, lib  # noqa: F401  (lib: the fixture)
from tests.tile_major import from_tile_major, to_tile_major

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(kind, args):
    """the case on the device and its float64 reference, computed once and shared by the tests (and variants) that use it"""
    build = {"attention": R.attention_case, "causal": R.causal_case, "relpos": R.relpos_case}[kind]
    case = R.to_device(build(*[list(a) if isinstance(a, tuple) else a for a in args]), "cuda")
    return case, R.reference(case)


def _frozen(args):
    return tuple(tuple(a) if isinstance(a, list) else a for a in args)


def _images(case, tm):
    """qkv as the kernel takes it, rows nobody owns NaN: row-major [pad][3d], or (tm & 2) the tile-major image of that"""
    t, d = case["qkv"].shape[0], case["d"]
    qkv = torch.cat([case["qkv"], _nan((_pad256(t) - t + 256, 3 * d), torch.float16)])
    return to_tile_major(qkv) if tm & 2 else qkv


def _twice(call, t, d, tm):
    """ctx [pad][d] row-major of two calls on NaN-filled outputs, bit-identical"""
    pad = _pad256(t) + 256
    outs = []
    for rep in range(2):
        ctx = _nan((pad, d), torch.float16)
        call(ctx)
        torch.cuda.synchronize()
        outs.append(ctx)
    assert _same(outs[:1], outs[1:]), "two runs differ"
    return from_tile_major(outs[0].view(-1), pad, d) if tm & 1 else outs[0]


def _verify(out, t, ref, bound, what):
    ratio = _ratio(out[:t], ref, bound, what)
    _untouched(out[t:], what)
    return ratio


def _attention(lib, case, tm):
    from sonar_amd import _lib

    lens, d = case["lens"], case["d"]
    qkv, cu = _images(case, tm), _cu(lens)
    return _twice(lambda ctx: _lib.check(lib.smi_attention(qkv.data_ptr(), cu.data_ptr(), ctx.data_ptr(), len(lens), max(lens), d,
                                                           case["heads"], tm, _stream())), sum(lens), d, tm)


# ------------------------------------------------------------------------------------------------------------- smi_attention
@pytest.mark.parametrize("tm", [0, 1, 2, 3])
@pytest.mark.parametrize("name", R.PATTERNS + ("random",))
def test_attention_patterns(lib, name, tm):
    """lens = [33, 97, 200, 514, 1, 32] in one call: 1 to 17 key blocks, tails of 1, 2 and 8 keys, no tail, two 128-query blocks
    per head for the longest; all four layouts (bit 0: ctx tile-major, bit 1: qkv tile-major)."""
    case, refs = _case("attention", _frozen((name, R.ATT_LENS, 2)))
    ratio = _verify(_attention(lib, case, tm), sum(R.ATT_LENS), refs[0], R.bound(*refs[:3]), f"attention {name} tm={tm}")
    print(f"attention {name} tm={tm}: worst err / bound = {ratio:.3f}")


@pytest.mark.parametrize("name", R.PATTERNS + ("random",))
def test_attention_non_temporal(lib, name):
    """max_len <= 128 under tile_major = 3: the instantiation that loads its K / V tiles non-temporally"""
    case, refs = _case("attention", _frozen((name, R.ATT_NT_LENS, 2)))
    ratio = _verify(_attention(lib, case, 3), sum(R.ATT_NT_LENS), refs[0], R.bound(*refs[:3]), f"attention nt {name}")
    print(f"attention non-temporal {name} lens={R.ATT_NT_LENS} tm=3: worst err / bound = {ratio:.3f}")


@pytest.mark.parametrize("order", [0, 1])
def test_attention_dispatch_order(lib, order):
    """ATT_ORDER: head-major (0) and sentence-major (1) dispatch of the same grid, on the over-threshold staircase"""
    from sonar_amd import _lib

    case, refs = _case("attention", _frozen(("stair_over", R.ATT_LENS, 2)))
    with _lib.tuning(ATT_ORDER=order):
        outs = [_attention(lib, case, tm) for tm in (0, 3)]
    for tm, out in zip((0, 3), outs):
        ratio = _verify(out, sum(R.ATT_LENS), refs[0], R.bound(*refs[:3]), f"attention ATT_ORDER={order} tm={tm}")
        print(f"attention stair_over ATT_ORDER={order} tm={tm}: worst err / bound = {ratio:.3f}")


def test_attention_16_heads(lib):
    """the text encoder's head count (d = 1024: other row strides, another block of the tile-major image per head pair)"""
    case, refs = _case("attention", _frozen(("stair_over", R.ATT_LENS, 16)))
    for tm in (0, 3):
        ratio = _verify(_attention(lib, case, tm), sum(R.ATT_LENS), refs[0], R.bound(*refs[:3]), f"attention heads=16 tm={tm}")
        print(f"attention stair_over heads=16 tm={tm}: worst err / bound = {ratio:.3f}")


def _g_rows(lens, heads, g):
    """[rows][heads] bool: the queries whose g of the cycle is `g`"""
    i = torch.cat([torch.arange(n) for n in lens])
    cyc = torch.tensor(R.G_CYCLE)
    return (cyc[(i[:, None] + torch.arange(heads)[None, :]) % 4] == g).cuda()


def test_attention_spike_returns_the_row(lib):
    """the closed form, without a reference: a g = 1 query of spike_last returns the last V row of its clip to an fp16 ulp
    (e^-40 of weight elsewhere), INT_COL = len - 1 exactly"""
    case, _ = _case("attention", _frozen(("spike_last", R.ATT_LENS, 2)))
    lens, d = case["lens"], case["d"]
    out = _attention(lib, case, 0)[:sum(lens)].double().view(-1, 2, 64)
    v = case["qkv"][:, 2 * d:].double().view(-1, 2, 64)
    last = torch.cat([torch.full((n,), o + n - 1) for o, n in zip(_cu(lens)[:-1].tolist(), lens)]).cuda()
    mine = _g_rows(lens, 2, 1.0)
    err = ((out - v[last]).abs() - 2.0 ** -10 * v[last].abs())[mine]
    assert (err <= 0).all(), err.max().item()
    assert torch.equal(out[:, :, R.INT_COL][mine], v[last][:, :, R.INT_COL][mine])


# ------------------------------------------------------------------------------------------------------ smi_causal_attention
@pytest.mark.parametrize("seq", R.CAUSAL_SEQS)
@pytest.mark.parametrize("name", R.PATTERNS + ("random",))
def test_causal_patterns(lib, name, seq):
    """three sequences of `seq` rows, query i sees keys 0..i: the rescale in the blocks that straddle the diagonal (the
    staircases, the ramp), the prefix means (uniform) and v_0 (spike_first, g = 1)"""
    from sonar_amd import _lib

    case, refs = _case("causal", (name, seq))
    n, d = R.CAUSAL_NSEQ, case["d"]
    qkv, cu = _images(case, 0), _cu(case["lens"])
    out = _twice(lambda ctx: _lib.check(lib.smi_causal_attention(qkv.data_ptr(), cu.data_ptr(), ctx.data_ptr(), n, seq, d, 2,
                                                                  _stream())), n * seq, d, 0)
    ratio = _verify(out, n * seq, refs[0], R.bound(*refs[:3]), f"causal {name} seq={seq}")
    if name == "spike_first":   # the closed form: v_0 of the sequence to an fp16 ulp for the g = 1 queries
        got = out[:n * seq].double().view(-1, 2, 64)
        v0 = case["qkv"][:, 2 * d:].double().view(n, seq, 2, 64)[:, :1].expand(n, seq, 2, 64).reshape(-1, 2, 64)
        mine = _g_rows(case["lens"], 2, 1.0)
        assert ((got - v0).abs() <= 2.0 ** -10 * v0.abs())[mine].all()
    print(f"causal {name} seq={seq}: worst err / bound = {ratio:.3f}")


# ------------------------------------------------------------------------------------------------------ smi_relpos_attention
@pytest.mark.parametrize("args", R.RELPOS_CASES, ids=R.case_id)
def test_relpos(lib, args):
    """Both kernels (SPEECH_RP_LDS 0: per-wave global loads, fp32 pad, layouts 0 and 1; 1: LDS ring, fp16 pad, layouts 0..3) on
    the patterns carried by q and k (rp = 0), the patterns carried by the position term (q = k = 0, v bias 8 e_0), the shifts
    (one hot position row: query i returns row i - delta0 of V, so an off-by-one in the pad addressing, the ring's slot
    rotation or the first block's second pad half returns the wrong integer in INT_COL), and randn inputs with non-zero u and v
    biases on the table layouts of attention_ref.TABLES: rp_zero != tmax - 1, one end or both ends of the table clamped."""
    from sonar_amd import _lib

    case, refs = _case("relpos", _frozen(args))
    lens, d, heads = case["lens"], case["d"], case["heads"]
    t, cu = sum(lens), _cu(lens)
    rp, u, v = case["rp"], case["u"], case["v"]
    for ring in (0, 1):
        bound = R.case_bound(case, refs, ring)
        for tm in ((0, 1, 2, 3) if ring else (0, 1)):
            qkv = _images(case, tm)
            with _lib.tuning(SPEECH_RP_LDS=ring):
                out = _twice(lambda ctx: _lib.check(lib.smi_relpos_attention(
                    qkv.data_ptr(), cu.data_ptr(), rp.data_ptr(), case["rp_zero"], rp.shape[0], u.data_ptr(), v.data_ptr(),
                    ctx.data_ptr(), len(lens), max(lens), d, heads, tm, _stream())), t, d, tm)
            what = f"relpos {R.case_id(args)} {'ring' if ring else 'global'} tm={tm}"
            ratio = _verify(out, t, refs[0], bound, what)
            if args[0] == "shift":
                want = R.shift_expected_rows(lens, args[1]).cuda()
                got = out[:t, R.INT_COL::64].double()
                assert torch.equal(got[want >= 0], want[want >= 0, None].double().expand(-1, heads)), what
            print(f"{what}: worst err / bound = {ratio:.3f}")
