"""CPU: tests/gemm_ref.py -- the designers' preconditions at every shape tests/test_gpu_gemm_engines.py launches, and the teeth of
its comparison rules: each rule must REJECT the expected output with one of the errors it is there for applied to it, several of
which the max-norm rule of tests/test_gpu_kernels.py accepts."""
import functools

import pytest
import torch

from tests import gemm_ref as R


@functools.lru_cache(maxsize=4)
def _dyadic(m, n, k):
    return R.dyadic_operands(m, n, k, R.seed_of(m, n, k))


# --------------------------------------------------------------------------------------------------------------- preconditions
@pytest.mark.parametrize("m,n,k", R.DYADIC_SHAPES)
def test_dyadic_preconditions(m, n, k):
    ops = R.dyadic_operands(m, n, k, R.seed_of(m, n, k))      # asserts exactness, granularity and the 2^15 range itself
    assert ops.inexact >= 0.01 and ops.ties > 0
    assert ops.scale == 0 or k < 256, (k, ops.scale)           # the plain ranges from K = 256 up
    assert ops.x.dtype == ops.w.dtype == ops.old16.dtype == torch.float16 and ops.bias.dtype == torch.float32
    assert ops.x.float().abs().max().item() <= 2 * 2 ** ops.scale and ops.w.float().abs().max().item() <= 0.25
    assert ops.bias.abs().max().item() <= 4 and ops.old16.float().abs().max().item() <= 4
    assert torch.equal(ops.old16.float(), ops.old32)
    if m * n <= 1 << 20:                                       # every linear epilogue: the fp64 reference is exact in fp32
        for epi in R.LINEAR:
            for use_bias in (True, False):
                want = R.dyadic_expected(ops, epi, use_bias)   # round_once asserts it
                assert want.dtype == (torch.float16 if R.out_is_f16(epi) else torch.float32)
    print(f"dyadic {m}x{n}x{k}: scale 2^{ops.scale}, max |x|.|w| {ops.max_abs_prod:.0f}, inexact {ops.inexact:.3f}, ties {ops.ties:.3f}")


def test_dyadic_figures_of_the_plain_ranges():
    """the unscaled operand ranges at K = 256 / 1024 / 8192: the reference is exact, max |x| . |w| ~ 44 / 157 / 1163, and 1.3 / 10 / 41 %
    of the outputs need a real fp16 rounding"""
    for (m, n, k), (lo, hi) in {(256, 256, 256): (0.005, 0.03), (256, 512, 1024): (0.07, 0.14), (256, 256, 8192): (0.35, 0.47)}.items():
        ops = _dyadic(m, n, k)
        assert ops.scale == 0 and lo <= ops.inexact <= hi and 0 < ops.ties <= ops.inexact, (k, ops.inexact, ops.ties)
        assert ops.max_abs_prod < 0.16 * k + 8 * k ** 0.5


@pytest.mark.parametrize("m,n,k,ksplit", R.INTEGER_SHAPES)
def test_integer_preconditions(m, n, k, ksplit):
    ops = R.integer_operands(m, n, k, R.seed_of(m, n, k))     # asserts the range of every K range of <= 1024 elements
    assert ops.x.float().abs().max().item() == 2 and ops.w.float().abs().max().item() == 1
    for parts in ([R.even_parts(k, ksplit)] if k % (64 * ksplit) == 0 else []) + [R.slice_parts(k, ksplit)]:
        assert parts[0][0] == 0 and parts[-1][1] == k and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        assert max(k1 - k0 for k0, k1 in parts) <= 1024
        slabs = R.splitk_ref(ops.x, ops.w, ops.bias, parts)
        assert slabs.abs().max().item() <= 2048 and (slabs.frac() == 0).all()
        assert torch.equal(slabs.half().double(), slabs)                                # exact even as fp16 slabs
        assert torch.equal(slabs.sum(0), R.preactivation(ops.x, ops.w, ops.bias))      # whatever the partition
    assert [b - a for a, b in R.slice_parts(1600, 3)] == [512, 544, 544]               # the 8-wave engine's unequal parts


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("m,n,k", R.SELECTOR_SHAPES)
def test_selector_covers_every_k_position(m, n, k, mirrored):
    """at every shape the GPU file runs selectors at (K = 64 .. 8192): the phases select every K position, and (the fp64 product
    is formed up to 2^20 outputs) the expected output is the product"""
    rows = n if mirrored else m
    seen = torch.zeros(k, dtype=torch.bool)
    for phase in range(R.selector_phases(rows, k)):
        ops = R.selector_operands(m, n, k, phase, mirrored, seed=R.seed_of(m, n, k))
        seen[ops.sel] = True
        assert ops.want.shape == (m, n) and ops.x.shape == (m, k) and ops.w.shape == (n, k)
        if m * n <= 1 << 20:
            want = R.gemm_tn_ref(R.BIAS, ops.x, ops.w)         # finite: no infinity or NaN among the patterns
            assert torch.equal(want, ops.want.double())        # one element, untouched by the zeros around it
        arb = ops.x if mirrored else ops.w
        assert (arb.float().abs() >= 2.0 ** -14).all() and torch.isfinite(arb.float()).all()
    assert seen.all()


def test_bounds_hold_for_an_fp32_product():
    """sanity of elementwise_bound and activation_ref_bound: a plain fp32 matmul rounded to fp16, and torch's fp32 activations,
    stay inside them (the GPU file measures the kernels' own margins)"""
    ops = R.scaled_operands(256, 384, 512, 3)
    ref = R.gemm_tn_ref(R.RESID16, ops.x, ops.w, ops.bias, ops.old16)
    got = (ops.old16.float() + (ops.x.float() @ ops.w.float().T + ops.bias)).half()
    assert R.check_bound(got, ref, R.elementwise_bound(ref, R.abs_sum(ops.x, ops.w, ops.bias, ops.old16), 512, True)) <= 1.0
    small = R.scaled_operands(256, 384, 512, 3)
    small.x[1::3] = 0                                           # rows of bias alone: the bound shrinks to their own size
    ref = R.gemm_tn_ref(R.BIAS, small.x, small.w, small.bias)
    bound = R.elementwise_bound(ref, R.abs_sum(small.x, small.w, small.bias), 512, True)
    assert (bound[1] <= 2.0 ** -10 * ref[1].abs() + 2.0 ** -24).all() and bound.max().item() > 1e-3
    d = _dyadic(256, 256, 256)
    pre = R.preactivation(d.x, d.w, d.bias)
    for epi, f in ((R.SILU, torch.nn.functional.silu), (R.TANH, torch.tanh)):
        ref, bound = R.activation_ref_bound(epi, pre)
        assert torch.equal(ref, R.epilogue_ref(epi, pre)) or (ref - R.epilogue_ref(epi, pre)).abs().max().item() < 1e-15
        assert R.check_bound(f(pre.float()).half(), ref, bound) <= 1.0
        assert (bound <= 2.0 ** -10 * ref.abs() + 2.0 ** -21).all()     # one fp16 rounding and a few fp32 ulps, no more
    ref, bound = R.activation_ref_bound(R.GLU, pre)
    a, g = R.glu_pair(pre.float())
    assert R.check_bound((a * torch.sigmoid(g)).half(), ref, bound) <= 1.0


# ----------------------------------------------------------------------------------------------------------------------- teeth
def _trunc16(ref):
    """fp64 -> fp16 rounded toward zero"""
    h = ref.float().half()
    away = h.double().abs() > ref.abs()
    return (h.view(torch.int16) - away.to(torch.int16)).view(torch.float16)     # one step towards zero in sign-magnitude


def _one_ulp(want, r, c):
    out = want.clone()
    out.view(torch.int16)[r, c] += 1
    return out


def _rejects(got, want):
    with pytest.raises(AssertionError, match="differ"):
        R.check_exact(got, want, "mutant")
    return True


@pytest.mark.parametrize("m,n,k", [(256, 512, 1024), (256, 256, 8192)])
def test_exact_rule_rejects_every_mutant(m, n, k):
    ops = _dyadic(m, n, k)
    want0, want8, want9 = (R.dyadic_expected(ops, e) for e in (R.BIAS, R.RESID16, R.RESID16_HALF))
    R.check_exact(want0.clone(), want0)
    pre = R.preactivation(ops.x, ops.w, ops.bias)

    def with_x(x, epi=R.BIAS):
        return R.round_once(R.gemm_tn_ref(epi, x, ops.w, ops.bias, ops.old16), True)

    # one K element dropped for one row
    r, kk = 37, int(torch.nonzero(ops.x[37].float().abs() == 0.125)[0])   # the smallest nonzero |x|: moves an output by <= 2^-5
    x = ops.x.clone()
    x[r, kk] = 0
    dropped = with_x(x)
    assert _rejects(dropped, want0) and torch.equal(dropped[:r], want0[:r]) and torch.equal(dropped[r + 1:], want0[r + 1:])
    # two 8-element K chunks swapped in x only
    x = ops.x.clone()
    x[:, 64:72], x[:, 136:144] = ops.x[:, 136:144], ops.x[:, 64:72]
    swapped = with_x(x)
    assert _rejects(swapped, want0)
    # truncation instead of round-to-nearest-even
    trunc = _trunc16(pre)
    assert _rejects(trunc, want0) and (trunc.double().abs() <= pre.abs()).all()
    # a second rounding: the fp16 residual epilogue through an fp16 intermediate, f16(old + f16(x . w^T + bias))
    twice8 = (ops.old16.double() + want0.double()).float().half()
    assert _rejects(twice8, want8)
    twice9 = (ops.old16.double() + (0.5 * pre).float().half().double()).float().half()
    assert _rejects(twice9, want9)
    # ... and fp32 -> a 12-bit significand -> fp16 (an intermediate with one more bit): differs from one rounding only where the
    # value has three bits below the fp16 spacing, |v| >= 32 on the 2^-8 grid
    if k == 8192:
        mant, e = torch.frexp(pre)
        mid = torch.ldexp(torch.round(mant * 4096), e - 12)          # torch.round: half to even
        assert _rejects(mid.float().half(), want0)
    assert _rejects(pre.float().bfloat16().half(), want0)            # ... and through the bf16 width
    # bias shifted by one column
    shifted = R.round_once(R.gemm_tn_ref(R.BIAS, ops.x, ops.w, ops.bias.roll(1)), True)
    assert _rejects(shifted, want0)
    # bias through an fp16 intermediate
    assert _rejects((R.preactivation(ops.x, ops.w).float().half().double() + ops.bias.double()).float().half(), want0)
    # epilogue 9 with factor 1
    assert _rejects(want8, want9)
    # one element off by one fp16 ulp
    ulp = _one_ulp(want0, m - 1, n - 3)
    assert _rejects(ulp, want0)
    # NaN left in the output
    nan = want0.clone()
    nan[5, 7] = float("nan")
    assert _rejects(nan, want0)
    # the gap this closes: the max-norm rule accepts the rounding mutants (and at K = 8192 a dropped K element)
    for name, mutant, w in (("truncation", trunc, want0), ("one ulp", ulp, want0), ("double rounding", twice8, want8)):
        assert R.legacy_maxnorm_accepts(mutant, w.double(), True), name
    assert R.legacy_maxnorm_accepts(want0, pre, True)
    if k == 8192:
        assert R.legacy_maxnorm_accepts(dropped, pre, True)


def test_selector_rule_names_the_position():
    ops = R.selector_operands(256, 384, 192, 0)
    R.check_selector(ops.want.clone(), ops)
    x = ops.x.clone()
    x[:, 64:72], x[:, 136:144] = ops.x[:, 136:144], ops.x[:, 64:72]           # two 8-element K chunks swapped in x only
    got = R.gemm_tn_ref(R.BIAS, x, ops.w).float().half()
    with pytest.raises(AssertionError, match=r"row \d+ column 0 \(K position (6[4-9]|7[01]|13[6-9]|14[0-3])\)"):
        R.check_selector(got, ops)
    bad_rows = (got != ops.want).any(1)
    assert int(bad_rows.sum()) == int(((ops.sel >= 64) & (ops.sel < 72) | (ops.sel >= 136) & (ops.sel < 144)).sum()) > 0
    with pytest.raises(AssertionError, match="K position"):
        R.check_selector(_one_ulp(ops.want, 9, 11), ops)
    assert R.legacy_maxnorm_accepts(_one_ulp(ops.want, 9, 11), ops.want, True)


def test_bound_rule_rejects_errors_in_small_rows_and_columns():
    """elementwise_bound judges a small row by its own size: an error of 2^-8 of the matrix maximum in a row of 1/16 of its scale is
    rejected, the max-norm rule accepts it; so is a wrong 0.5 on a small column and a dropped K element"""
    ops = R.scaled_operands(256, 384, 512, 5)
    ref = R.gemm_tn_ref(R.BIAS, ops.x, ops.w, ops.bias)
    bound = R.elementwise_bound(ref, R.abs_sum(ops.x, ops.w, ops.bias), 512, True)
    good = ref.float().half()
    assert R.check_bound(good, ref, bound) <= 1.0
    small_row = int(ref.abs().max(1).values.argmin())
    bad = good.clone()
    bad[small_row] = (ref[small_row] * (1 + 2.0 ** -8)).float().half()
    with pytest.raises(AssertionError, match=f"row {small_row} "):
        R.check_bound(bad, ref, bound)
    assert R.legacy_maxnorm_accepts(bad, ref, True)
    col = int(ref.abs().max(0).values.argmin())
    half = good.clone()
    half[:, col] = (0.5 * ref[:, col]).float().half()
    with pytest.raises(AssertionError, match=f"column {col}:"):
        R.check_bound(half, ref, bound)
    x = ops.x.clone()
    x[small_row, 100] = 0
    with pytest.raises(AssertionError, match=f"row {small_row} "):
        R.check_bound(R.gemm_tn_ref(R.BIAS, x, ops.w, ops.bias).float().half(), ref, bound)
    nan = good.clone()
    nan[3, 3] = float("nan")
    with pytest.raises(AssertionError):
        R.check_bound(nan, ref, bound)


def test_activation_rule_rejects_a_second_rounding_and_a_wrong_pairing():
    d = _dyadic(256, 512, 1024)
    pre = R.preactivation(d.x, d.w, d.bias) / 16          # still exact in fp32; moves the values into the activations' range
    ref, bound = R.activation_ref_bound(R.SILU, pre)
    with pytest.raises(AssertionError):                    # silu on the fp16-rounded pre-activation
        R.check_bound(torch.nn.functional.silu(pre.float().half().float()).half(), ref, bound)
    ref, bound = R.activation_ref_bound(R.GLU, pre)
    a, g = R.glu_pair(pre.float())
    with pytest.raises(AssertionError):                    # value and gate exchanged
        R.check_bound((g * torch.sigmoid(a)).half(), ref, bound)
    with pytest.raises(AssertionError):                    # halves of the row instead of 32-column groups
        R.check_bound((pre[:, :256].float() * torch.sigmoid(pre[:, 256:].float())).half(), ref, bound)
    ref, bound = R.activation_ref_bound(R.TANH, pre)
    with pytest.raises(AssertionError):
        R.check_bound(_trunc16(ref), ref, bound)
