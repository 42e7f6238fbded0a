"""fp64 restatement of smi_gemm_tn / smi_gemm_tn_splitk (include/sonar_mi355.h), the operand designers of the GEMM engine tests and
the rules their outputs are compared by.  torch only, importable without a GPU: tests/test_gemm_ref_cpu.py checks the designers'
preconditions and that every rule rejects the errors it is there for; tests/test_gpu_gemm_engines.py runs the engines.

Three kinds of operands make the expected output known TO THE BIT, whatever the engine's summation order:

  dyadic    x, w, bias and the old residual are small multiples of powers of two, so every product and every partial sum is an
            integer multiple of 2^-8 (2^-9 after the 0.5 of epilogues 4 / 9) below 2^15: exact in fp32 (24 bits) in ANY order.
            fp32 outputs equal the fp64 reference, fp16 outputs equal it rounded ONCE to nearest even.
  integer   x in {-2..2}, w in {-1, 0, 1}, integer bias: every partial sum over <= 1024 K elements is an integer of magnitude
            <= 2048, exact even as an fp16 split-K slab; the slabs sum to the reference for every K partition.
  selector  one operand is one-hot per row, the other holds arbitrary normal fp16 bit patterns: out[r][c] is ONE element of the
            other operand, bit for bit, and a wrong element names the K position, row and column that were mis-addressed.

Real-valued operands are judged element by element by `elementwise_bound`, the nonlinear epilogues by `activation_ref_bound`."""
import functools
import types

import torch

U = 2.0 ** -24      # unit roundoff of fp32
H = 2.0 ** -11      # ... of fp16
F16_TINY = 2.0 ** -25   # half the spacing of the fp16 subnormals: the absolute floor of one fp16 rounding

BIAS, RELU, RESID32, STORE32, RESID32_HALF, SILU, GLU, TANH, RESID16, RESID16_HALF = range(10)
LINEAR = (BIAS, RELU, RESID32, STORE32, RESID32_HALF, RESID16, RESID16_HALF)     # RELU: piecewise linear, exact on exact input
NONLINEAR = (SILU, GLU, TANH)
F32_OUT = (RESID32, STORE32, RESID32_HALF)
RMW = (RESID32, RESID32_HALF, RESID16, RESID16_HALF)                               # read-modify-write of `out`


def out_is_f16(epi):
    return epi not in F32_OUT


def out_cols(epi, n):
    return n // 2 if epi == GLU else n


# --------------------------------------------------------------------------------------------------------------- the reference
def glu_pair(pre):
    """GLU column pairing: output column g * 32 + c is (value, gate) = pre-activation columns g * 64 + c / g * 64 + 32 + c"""
    p = pre.view(pre.shape[0], -1, 2, 32)
    return p[:, :, 0].reshape(pre.shape[0], -1), p[:, :, 1].reshape(pre.shape[0], -1)


def preactivation(x, w, bias=None, k0=0, k1=None):
    """X[:, k0:k1] . W[:, k0:k1]^T + bias in fp64"""
    pre = x[:, k0:k1].double() @ w[:, k0:k1].double().T
    return pre if bias is None else pre + bias.double()[None, :]


def epilogue_ref(epi, pre, old=None):
    """the epilogue `epi` of smi_gemm_tn on an fp64 pre-activation, unrounded; old: the previous content of a read-modify-write
    output"""
    if epi in (BIAS, STORE32):
        return pre
    if epi == RELU:
        return torch.relu(pre)
    if epi in (RESID32, RESID16):
        return old.double() + pre
    if epi in (RESID32_HALF, RESID16_HALF):
        return old.double() + 0.5 * pre
    if epi == SILU:
        return pre * torch.sigmoid(pre)
    if epi == GLU:
        a, g = glu_pair(pre)
        return a * torch.sigmoid(g)
    if epi == TANH:
        return torch.tanh(pre)
    raise ValueError(epi)


def gemm_tn_ref(epi, x, w, bias=None, old=None):
    return epilogue_ref(epi, preactivation(x, w, bias), old)


def even_parts(k, ksplit):
    """K ranges of the 128x128 family and the lone units: K / ksplit each"""
    assert k % ksplit == 0
    return [(z * (k // ksplit), (z + 1) * (k // ksplit)) for z in range(ksplit)]


def slice_parts(k, ksplit):
    """K ranges of the 8-wave engine: part z covers the 32-wide slices [S z / ksplit, S (z + 1) / ksplit), S = K / 32"""
    s = k // 32
    return [(32 * (s * z // ksplit), 32 * (s * (z + 1) // ksplit)) for z in range(ksplit)]


def splitk_ref(x, w, bias, parts):
    """[len(parts)][m][n] fp64: the slabs of smi_gemm_tn_splitk, the bias in part 0"""
    return torch.stack([preactivation(x, w, bias if z == 0 else None, k0, k1) for z, (k0, k1) in enumerate(parts)])


def round_once(ref, f16):
    """the output format's round-to-nearest-even of an fp64 value that is exact in fp32 (so double -> float -> half rounds once)"""
    r32 = ref.float()
    assert torch.equal(r32.double(), ref), "reference is not exact in fp32: round_once would round twice"
    return r32.half() if f16 else r32


# ------------------------------------------------------------------------------------------------------------------- designers
def _randint(gen, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64)


def f16_inexact_and_ties(ref):
    """masks of the fp64 values that one fp16 rounding changes, and of those exactly half way between two fp16 numbers"""
    h = ref.float().half().double()
    _, e = torch.frexp(ref.abs().clamp(min=2.0 ** -14))          # |v| = f * 2^e, f in [0.5, 1): spacing 2^(e - 11)
    half_ulp = torch.ldexp(torch.ones_like(ref), e - 12)
    inexact = h != ref
    return inexact, inexact & ((h - ref).abs() == half_ulp)


def dyadic_operands(m, n, k, seed, device="cpu", min_inexact=0.01):
    """x: multiples of 2^-3 in [-2, 2] * 2^s, w: multiples of 2^-5 in [-1/4, 1/4], bias and the old residual: multiples of 2^-8 in
    [-4, 4]; s >= 0 is the smallest power that makes >= 1 % of the fp16 outputs of x . w^T + bias inexact with at least one exact
    tie among them (s = 0 from K = 256 up).  Asserts: x, w, old exact in fp16; every product a multiple of 2^-8;
    S = |x| . |w|^T + |bias| + |old| < 2^15, hence every partial sum, in any order, with bias / residual / 0.5 applied at any point, is
    a multiple of 2^-9 below 2^15 = at most 24 significant bits = exact in fp32; the fp64 reference is exact in fp32."""
    gen = torch.Generator().manual_seed(seed)
    xi = _randint(gen, -16, 16, (m, k))
    wi = _randint(gen, -8, 8, (n, k))
    bi = _randint(gen, -1024, 1024, (n,))
    oi = _randint(gen, -1024, 1024, (m, n))
    x0 = (xi.double() / 8).to(device)
    w = (wi.double() / 32).to(device)
    bias = (bi.double() / 256).to(device)
    old = (oi.double() / 256).to(device)
    prod0, aprod0 = x0 @ w.T, x0.abs() @ w.abs().T
    for s in range(0, 8):
        ref = prod0 * 2.0 ** s + bias
        inexact, ties = f16_inexact_and_ties(ref)
        if inexact.double().mean().item() >= min_inexact and ties.any():
            break
    else:
        raise AssertionError(f"no operand scale gives {min_inexact:.0%} inexact fp16 outputs and a tie at {(m, n, k)}")
    x = x0 * 2.0 ** s
    S = aprod0 * 2.0 ** s + bias.abs() + old.abs()
    assert S.max().item() < 2.0 ** 15, S.max().item()
    assert torch.equal(x.half().double(), x) and torch.equal(w.half().double(), w) and torch.equal(old.half().double(), old)
    assert ((x * 8).frac() == 0).all() and ((w * 32).frac() == 0).all()        # products: multiples of 2^-8
    assert ((bias * 256).frac() == 0).all() and ((old * 256).frac() == 0).all()
    assert torch.equal(ref.float().double(), ref)
    return types.SimpleNamespace(m=m, n=n, k=k, scale=s, x=x.half(), w=w.half(), bias=bias.float(), old16=old.half(), old32=old.float(),
                                 S=S, inexact=inexact.double().mean().item(), ties=ties.double().mean().item(),
                                 max_abs_prod=(aprod0 * 2.0 ** s).max().item())


def dyadic_expected(ops, epi, use_bias=True):
    """the bit-exact expected output of a LINEAR epilogue on dyadic operands"""
    assert epi in LINEAR
    old = ops.old16 if out_is_f16(epi) else ops.old32
    return round_once(gemm_tn_ref(epi, ops.x, ops.w, ops.bias if use_bias else None, old), out_is_f16(epi))


def integer_operands(m, n, k, seed, device="cpu", max_part=1024):
    """x in {-2..2}, w in {-1, 0, 1}, bias an integer in {-8..8}.  Asserts that sum |x_k| |w_k| over ANY K range of up to max_part
    elements, plus |bias|, is <= 2048: every slab of a split-K launch whose parts are no longer than that is an integer of
    magnitude <= 2048 = exact in fp16, and in fp32 along the way.  (The range sums are bounded through 64-wide blocks: any range of
    <= max_part elements lies inside max_part / 64 + 1 consecutive blocks.)"""
    gen = torch.Generator().manual_seed(seed)
    x = _randint(gen, -2, 2, (m, k)).double().to(device)
    w = _randint(gen, -1, 1, (n, k)).double().to(device)
    bias = _randint(gen, -8, 8, (n,)).double().to(device)
    nb, win = -(-k // 64), max_part // 64 + 1
    blocks = torch.stack([x[:, b * 64:(b + 1) * 64].abs() @ w[:, b * 64:(b + 1) * 64].abs().T for b in range(nb)])
    c = torch.cat([torch.zeros_like(blocks[:1]), blocks.cumsum(0)])
    worst = max((c[min(b + win, nb)] - c[b]).max().item() for b in range(nb))
    assert worst + bias.abs().max().item() <= 2048, worst
    return types.SimpleNamespace(m=m, n=n, k=k, x=x.half(), w=w.half(), bias=bias.float(), worst_range=worst)


SELECTOR_STRIDE = 17   # odd and coprime to every K of the tests (K = 2^a 3^b 5^c 7^d): k -> 17 k mod K is a bijection


def selector_phases(rows, k):
    return -(-k // rows)


def selector_k(rows, k, phase):
    """the K position row r of the one-hot operand selects: ((r + phase * rows) * 17) mod K.  Over phase < ceil(K / rows) the
    argument r + phase * rows runs over 0 .. >= K - 1 and the multiplication permutes the residues: every K position is selected."""
    import math

    assert math.gcd(SELECTOR_STRIDE, k) == 1
    return ((torch.arange(rows) + phase * rows) * SELECTOR_STRIDE) % k


@functools.lru_cache(maxsize=4)
def arbitrary_f16(shape, seed):
    """normal fp16 numbers with a random sign, exponent field (1..30) and mantissa: no zero, subnormal, infinity or NaN; +-65504 and
    2^-14 planted in the first row.  Cached (the phases of one shape share it): callers must not write into it."""
    gen = torch.Generator().manual_seed(seed)
    bits = (_randint(gen, 0, 1, shape) << 15) | (_randint(gen, 1, 30, shape) << 10) | _randint(gen, 0, 1023, shape)
    bits.view(-1)[:3] = torch.tensor([0x7BFF, 0xFBFF, 0x0400])
    a = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16).view(torch.float16)
    f = a.float()
    assert torch.isfinite(f).all() and (f.abs() >= 2.0 ** -14).all() and f.abs().max().item() == 65504 and f.abs().min().item() == 2.0 ** -14
    return a


def selector_operands(m, n, k, phase, mirrored=False, seed=0, device="cpu"):
    """mirrored False: X[r] one-hot (value 1) at selector_k(m, k, phase)[r], W arbitrary normal fp16: out[r][c] == W[c][k(r)].
    mirrored True: W[c] one-hot at selector_k(n, k, phase)[c], X arbitrary: out[r][c] == X[r][k(c)].  No bias (or a zero one):
    the one product that is not +-0 is 1 * v, the sum adds zeros to it, an fp16 or fp32 store of it is exact."""
    rows, other = (n, m) if mirrored else (m, n)
    sel = selector_k(rows, k, phase)
    hot = torch.zeros(rows, k, dtype=torch.float16)
    hot[torch.arange(rows), sel] = 1
    arb = arbitrary_f16((other, k), seed * 2 + int(mirrored))
    want = arb[:, sel]                                                  # [other][rows]
    x, w, want = (arb, hot, want) if mirrored else (hot, arb, want.T)
    assert want.shape == (m, n) and (hot.float().sum(1) == 1).all()
    return types.SimpleNamespace(m=m, n=n, k=k, x=x.to(device), w=w.to(device), want=want.contiguous().to(device), sel=sel,
                                 mirrored=mirrored)


def scaled_operands(m, n, k, seed, device="cpu"):
    """real-valued operands whose rows (x) and columns (w) have their own magnitudes: scales 0.25 / 1 / 4 with offsets, so that an
    error confined to small rows or columns is judged by their own size under `elementwise_bound`"""
    gen = torch.Generator().manual_seed(seed)
    r, c = torch.arange(m), torch.arange(n)
    sx, ox = torch.tensor([0.25, 1.0, 4.0])[r % 3], torch.tensor([0.0, 0.5, -0.5, 2.0, -2.0])[r % 5]
    sw, ow = torch.tensor([0.25, 1.0, 4.0])[c % 3] * 0.05, torch.tensor([0.0, 0.5, -0.5])[(c // 3) % 3]
    x = ((torch.randn(m, k, generator=gen) + ox[:, None]) * sx[:, None]).half()
    w = ((torch.randn(n, k, generator=gen) + ow[:, None]) * sw[:, None]).half()
    bias = torch.randn(n, generator=gen) * sw * 20
    old = (torch.randn(m, n, generator=gen) * sx[:, None]).half()
    return types.SimpleNamespace(m=m, n=n, k=k, x=x.to(device), w=w.to(device), bias=bias.to(device), old16=old.to(device),
                                 old32=old.float().to(device))


# ----------------------------------------------------------------------------------------------------------------------- rules
def abs_sum(x, w, bias=None, old=None):
    """S = |x| . |w|^T + |bias| + |old| in fp64"""
    s = x.double().abs() @ w.double().abs().T
    if bias is not None:
        s = s + bias.double().abs()[None, :]
    return s if old is None else s + old.double().abs()


def elementwise_bound(ref, S, k, out_f16):
    """Bound of |out - ref| per element for fp16 operands, fp32 accumulation in any order and one rounding of the output.

    The products of two fp16 numbers are exact in fp32 (22 bits), and the 0.5 of epilogues 4 / 9 is a power of two.  The result is
    a sum of k products, the bias and the old residual: k + 2 terms, k + 1 additions, so in ANY summation order a term passes
    through at most k + 1 roundings and the computed fp32 sum s satisfies (Higham, Accuracy and Stability of Numerical Algorithms,
    4.2)  |s - ref| <= gamma_(k+1) S,  gamma_j = j u / (1 - j u), u = 2^-24, S = |x| . |w|^T + |bias| + |old|.  An fp32 output is s.
    An fp16 output rounds s once, to nearest:  |out - s| <= 2^-11 |s| for a normal result and <= 2^-25 (half the spacing of the
    subnormals) below 2^-14, and |s| <= |ref| + gamma_(k+1) S.  The bound used is

        fp32 out:  gamma_(k+2) S        fp16 out:  2^-11 |ref| (1 + 2^-10) + 2^-25 + gamma_(k+2) S

    whose spare rounding (gamma_(k+2) - gamma_(k+1) >= u S) pays for the cross term 2^-11 gamma_(k+1) S while k + 2 <= 2^11; the
    cases judged by it have K <= 1024.  fp16 saturation is not modelled: |ref| + the bound must stay below 65504."""
    j = k + 2
    gamma = j * U / (1 - j * U)
    if not out_f16:
        return gamma * S
    assert (ref.abs() + gamma * S).max().item() < 65504 * (1 - H)
    return H * ref.abs() * (1 + 2.0 ** -10) + F16_TINY + gamma * S


def activation_ref_bound(epi, pre):
    """(fp64 reference, elementwise bound) of a NONLINEAR epilogue on a pre-activation that is EXACT in fp32 (dyadic operands), from
    the formulas of csrc/gemm_epi.hpp.  u = 2^-24; v_exp_f32 and v_rcp_f32 are 1 ulp = relative 2u; +, * round to nearest: u.

    sigmoid_f(v) = rcp(1 + exp2(c v)), c = fl(-log2 e):  c and the product c v carry u each, so the argument is
      -v log2(e) (1 + e1), |e1| <= 2u + u^2, and exp2 of it is e^-v (1 + eta), |eta| <= 2u + |v| (2u + u^2) to first order: the
      argument's RELATIVE error is an ABSOLUTE error |v| e1 ln-scaled in the exponent -- this is the term that grows with |v|.
      1 + E rounds (u), rcp 2u.  With s = sigmoid(v):  1 + E = (1 + e^-v)(1 + eta (1 - s)), so
      sigmoid_f = s (1 + d),  |d| <= [3 + (2 + 2|v|)(1 - s)] u =: sig(v) u.
    silu  a = b = v, GLU  a = value, b = gate:  out = fl(a * sigmoid_f(b)), one more u:  |err| <= |a| s(b) (sig(b) + 1) u.
    tanh_f(v) = 1 - 2 rcp(exp2(c2 v) + 1), c2 = fl(2 log2 e):  E = e^2v (1 + eta), |eta| <= (2 + 4|v|) u.  With q = 2 / (e^2v + 1)
      (tanh = 1 - q):  2 rcp(E + 1) = q (1 + rho), |rho| <= [3 + (2 + 4|v|)(1 - q / 2)] u; the subtraction (fused or not) adds u |tanh|:
      |err| <= q [3 + (2 + 4|v|)(1 - q / 2)] u + |tanh v| u -- near v = 0 (q = 1) this is an ABSOLUTE error of ~ 4 u = a few 2^-24
      however small tanh v is: inherent to the formula, it cancels 1 - q.
    Every first-order sum sigma of the (1 + delta) factors is widened to sigma / (1 - sigma) (Higham, lemma 3.1).  Where exp2
    overflows or underflows (|v| > 87) the formulas return the exact limits and the true values differ from them by < 2^-120, added as
    an absolute term, as is the flush of a subnormal intermediate.  The fp32 result is then rounded once to fp16:
    2^-11 (|ref| + err) + 2^-25."""
    assert epi in NONLINEAR
    assert torch.equal(pre.float().double(), pre)
    if epi == TANH:
        v = pre
        ref = torch.tanh(v)
        q = 2 / (torch.exp(2 * v) + 1)
        sigma = (q * (3 + (2 + 4 * v.abs()) * (1 - q / 2)) + ref.abs()) * U
        err = sigma / (1 - 8 * (1 + v.abs().max().item()) * U) + 2.0 ** -120
    else:
        a, b = (pre, pre) if epi == SILU else glu_pair(pre)
        s = torch.sigmoid(b)
        one_minus_s = torch.sigmoid(-b)                      # 1 - s without cancellation
        ref = a * s
        sigma = (4 + (2 + 2 * b.abs()) * one_minus_s) * U
        err = ref.abs() * sigma / (1 - sigma) + a.abs() * 2.0 ** -120
    return ref, err + H * (ref.abs() + err) + F16_TINY


def first_mismatch(bad):
    idx = torch.nonzero(bad)[0].tolist()
    return tuple(idx)


def check_exact(got, want, tag=""):
    """every element equal (NaN never is); the failure names the first (row, column), the two values and the count"""
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    bad = ~(got == want)
    if bad.any():
        r, c = first_mismatch(bad)
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} elements differ, first at row {r} column {c}: "
                             f"got {got[r, c].item()!r}, want {want[r, c].item()!r}")


def check_selector(got, ops, want=None, tag=""):
    """check_exact against the selected elements; the failure also names the K position that row / column should have read"""
    want = ops.want if want is None else want
    bad = ~(got == want)
    if bad.any():
        r, c = first_mismatch(bad)
        kpos = int(ops.sel[c if ops.mirrored else r])
        raise AssertionError(f"{tag}: {int(bad.sum())} elements differ, first at row {r} column {c} (K position {kpos}): "
                             f"got {got[r, c].item()!r}, want {want[r, c].item()!r}")


def check_bound(got, ref, bound, tag=""):
    """|got - ref| <= bound for every element; returns the largest error / bound"""
    ratio = (got.double() - ref).abs() / bound
    worst = ratio.max().item()                              # NaN in got: comparisons below are False
    if not (ratio <= 1.0).all():
        r, c = first_mismatch(~(ratio <= 1.0))
        raise AssertionError(f"{tag}: error / bound up to {worst:.3f}, first at row {r} column {c}: got {got[r, c].item()!r}, "
                             f"reference {ref[r, c].item()!r}, bound {bound[r, c].item():.3e}")
    return worst


def legacy_maxnorm_accepts(got, want, out_f16):
    """the rule of tests/test_gpu_kernels.py: max |got - want| <= (2e-3 | 2e-5) * max(max |want|, 1)"""
    got, want = got.double(), want.double()
    return bool(torch.isfinite(got).all()) and (got - want).abs().max().item() <= (2e-3 if out_f16 else 2e-5) * max(want.abs().max().item(), 1.0)


# ------------------------------------------------------------------------------------------- the shapes the GPU file launches
# (m, n, k) per engine group of tests/test_gpu_gemm_engines.py: test_gemm_ref_cpu.py checks the designers at each of them
RING4_SHAPES = [(256, 384, 64), (256, 384, 128), (256, 384, 192), (256, 384, 256), (256, 384, 1024)]   # 1, 2, 3, 4, 16 K tiles
RING4_TM_SHAPES = [(256, 512, 192), (256, 512, 1024)]
RING0_SHAPES = [(2176, 2048, 128)]                                        # 17 x 16 tiles of 128 x 128 > 256 CUs: two stages
LONE64_SHAPES = [(256, 384, 64), (256, 384, 320), (1024, 2048, 128)]     # 24 units; 512 units = two per CU
LONE64_TM_SHAPES = [(256, 512, 192)]
LONE16_SHAPES = [(256, 512, 256), (256, 512, 512), (256, 256, 1024)]     # 2, 4, 8 K blocks of 128 per unit
PP256_SHAPES = [(256, 512, 64), (256, 512, 192), (256, 512, 1024)]       # 2 slices: shorter than the pipeline lead
PP256_BIG = (4352, 4096, 64)                                              # 17 x 16 tiles of 256 x 256 > 256 CUs
V2_SHAPES = [(512, 512, 256), (512, 512, 384), (512, 512, 1024)]         # 8, 12, 32 slices
V2_STREAM = (16640, 1024, 256)                                            # 260 tiles: workgroups stream across a tile boundary
V2_RASTER = (14592, 4096, 256)                                            # 57 x 16 tiles: XCD-owned raster, skipped slots
LONG_K = (256, 256, 8192)                                                 # ring, lone64, 8-wave and 4-wave engine
# lone units of the 4-wave engine: the router takes the height that puts the most units on the chip without exceeding the CUs, so
# 160 / 192 rows need a launch whose 128-row units would not fit: 10 x 26 = 260 > 256 >= 8 x 26, 12 x 22 = 264 > 256 >= 8 x 22
V2_LONE_SHAPES = ([(512, 256, k) for k in (256, 320, 448, 1024)] +                        # 128 rows; 8, 10, 14, 32 slices per unit
                  [(m, n, k) for m, n in ((1280, 6656), (1536, 5632)) for k in (256, 320, 448)])   # 160 / 192 rows
V2_LONE_SLAB_SHAPES = ([(512, 256, k, 2) for k in (640, 896)] +                           # 10 and 14 slices per unit
                       [(m, 1024, k, 8) for m in (1280, 1536) for k in (2560, 3584)])     # 10 x 4 x 8 = 320 > 256 >= 8 x 4 x 8
SPLITK_SMALL = [(256, 256, 512, 2), (256, 384, 768, 3), (256, 256, 2048, 8)]              # ring, lone64 (row-major operands)
SPLITK_LONE16 = [(256, 256, 1024, 4), (256, 256, 2048, 2)]                                # 256 / 1024 per unit
SPLITK_PP256 = [(256, 256, 1600, 3), (256, 512, 2048, 4)]                                 # 50 slices in 3 parts: 16, 17, 17
STATS_SHAPES = [(256, 768, 256, 768 - 50), (512, 512, 1024, 512)]                         # masked last tile; every tile full

DYADIC_SHAPES = sorted(set(RING4_SHAPES + RING4_TM_SHAPES + RING0_SHAPES + LONE64_SHAPES + LONE64_TM_SHAPES + LONE16_SHAPES + PP256_SHAPES +
                           [PP256_BIG] + V2_SHAPES + [V2_STREAM, V2_RASTER, LONG_K] + V2_LONE_SHAPES + [s[:3] for s in STATS_SHAPES]))
SELECTOR_SHAPES = [s for s in DYADIC_SHAPES if s != V2_RASTER]             # a superset of the shapes the selectors run at
INTEGER_SHAPES = sorted(set(SPLITK_SMALL + SPLITK_LONE16 + SPLITK_PP256 + V2_LONE_SLAB_SHAPES))


def seed_of(m, n, k):
    return m * 7 + n * 3 + k
