"""Plain torch float64 restatements of the head_dim-64 MFMA attention kernels that share csrc/attn_core.hpp (attention_kernel
and its CAUSAL instantiation in csrc/attention.hip, relpos_attention_kernel and relpos_attention_lds_kernel in
csrc/relpos_attention.hip), the error bound their tests hold them to, and the builders of the inputs those tests use.  In the
style of tests/row_kernels_ref.py: the references take the kernel's own fp16 / fp32 tensors (on any device), widen them and
round only where the kernel's comments say it rounds -- q + u and q + v are formed in fp32 and rounded to fp16
(rp_query_frags), position rows clamp to [0, rp_rows - 1].

Every reference returns, elementwise in the output's shape, with a_j the softmax weights of the element's query and head:
  ref = sum_j a_j v_j,   B = sum_j a_j |v_j|,   A = max over the visible keys j of |v_j|
(relpos_attention also returns G = max_j |g_ij|, g_ij = (q_i + v) . rp[clamp(rp_zero + i - j)], the unscaled position score).

The bound (`bound`), elementwise, nothing in it fitted to a kernel's output:
  |got - ref| <= ulp16(ref) + 2^-11 B + 2^-14 A
 * ulp16(ref) as in row_kernels_ref.tolerance: 2^-10 |ref| with a floor of 2^-24, one fp16 ulp, half of it the output rounding;
 * 2^-11 B: each p_j = exp2(x_j - m) is rounded to nearest fp16 for the PV MFMA, a relative 2^-11 per p_j, while the denominator
   sums the unrounded fp32 p_j: the numerator moves by at most 2^-11 sum_j p_j |v_j|, the quotient by 2^-11 B;
 * 2^-14 A: the project's allowance for the fp32 arithmetic (row_kernels_ref.tolerance).  It also covers the p_j below the fp16
   normal range: m never exceeds the query's running maximum, so its largest p is >= 1 and a p_j that fp16 flushes or rounds
   coarsely is below 2^-14 of the denominator.
The LDS-ring kernel rounds g_ij to fp16 before it adds it to the content score (the header comment of
relpos_attention_lds_kernel).  That moves the logit x_ij = (c_ij + g_ij) / 8 by at most E_i = 2^-11 max_j |g_ij| / 8; softmax
weights whose logits move by at most E move by at most a factor e^(+-2E) (numerator e^(+-E), denominator e^(-+E)), to first
order a relative 2E, so its bound has one more term: 2 E_i B (`bound(..., gmax=G)`).

Designed scores (`designed_qkv`): q_i = 8 g_i e_0 and k_j = b_j e_0, every other coordinate zero, so the logit q.k / 8 is
exactly g_i b_j and every product is exact in fp16 and fp32.  In the log2 domain of attn_lazy_rescale the reference m moves
when a block maximum exceeds it by more than 8, i.e. by more than 8 ln 2 = 5.545 in logit units.  g_i cycles through
(1, -1, 0, 0.5) (started at the head's index), so within every 32-query wave some lanes rescale hard, some by alpha = 1, one
sees the mirrored pattern and one uniform scores.  v = randn * 1.5; the spike and shift inputs give v one column (INT_COL) of
the row's index in its clip, exact in fp16, so a wrong row is unmistakable.  The patterns b over the key index j
(block = j // 32) are in `key_pattern`.

Everything the builders make is made on the CPU from a seeded generator, so the CPU tests (the schedule model and the
emulation of tests/test_attention_ref_cpu.py) and the GPU tests see the same bits."""
import torch

from tests.row_kernels_ref import tolerance

G_CYCLE = (1.0, -1.0, 0.0, 0.5)
INT_COL = 5
POISON = 1000.0   # position-table rows that no (valid query, valid key) pair addresses

# the shapes of tests/test_gpu_attention_kernels.py, shared with the CPU tests that prove the inputs do what they claim
ATT_LENS = [33, 97, 200, 514, 1, 32]   # 1 to 17 key blocks, tails of 1 and 2 keys, no tail, two 128-query blocks
ATT_NT_LENS = [97, 128]                # max_len <= 128: the non-temporal instantiation under tile_major = 3
CAUSAL_SEQS = (97, 129, 200, 300)
CAUSAL_NSEQ = 3
RELPOS_LENS = [33, 97, 200, 300]       # 200 and 300 wrap the five-slot position-row ring
SHIFTS = (1, -1, 31, 32, -33)

PATTERNS = ("stair_under", "stair_hold", "stair_over", "stair_desc", "ramp", "spike_last", "spike_first", "uniform")
POSITION_PATTERNS = ("stair_under", "stair_hold", "stair_over", "stair_desc", "ramp")


def key_pattern(name, n):
    """b_j for j = 0 .. n-1, float64:
     stair_under  5.5 * block: one step is 7.93 < 8 in the log2 domain.  From block 0 to block 1 the reference holds and p
                  reaches e^5.5 = 245 < 256, the upper end of the lazy window; the second step is 15.9 above the reference and
                  moves it, so in longer clips the g = 1 lanes rescale at every other block with p at 245 in between;
     stair_hold   5.5 * (block & 1): the same step up and down again, so the reference NEVER moves after the first block and
                  p is 245 in every odd block, whatever the length;
     stair_over   5.625 * block: one step is 8.12 > 8, the g = 1 lanes rescale at every block;
     stair_desc   -6 * block: the g = -1 lanes rescale at every block;
     ramp         0.25 * j: 11.5 per block for g = 1, 5.8 for g = 0.5: the reference creeps, many small alpha;
     spike_last   40 at j = n - 1, else 0: the rescale lands in the last key block, the masked tail block when n % 32 != 0;
     spike_first  40 at j = 0, else 0;
     uniform      0: the output is the mean of V (the prefix mean under the causal mask)."""
    j = torch.arange(n, dtype=torch.float64)
    block = torch.div(j, 32, rounding_mode="floor")
    b = torch.zeros(n, dtype=torch.float64)
    if name == "stair_under":
        b = 5.5 * block
    elif name == "stair_hold":
        b = 5.5 * (block % 2)
    elif name == "stair_over":
        b = 5.625 * block
    elif name == "stair_desc":
        b = -6.0 * block
    elif name == "ramp":
        b = 0.25 * j
    elif name == "spike_last":
        b[n - 1] = 40.0
    elif name == "spike_first":
        b[0] = 40.0
    else:
        assert name == "uniform", name
    return b


def _values(lens, heads, gen, int_col):
    """v [t][heads][64] = randn * 1.5 (+ the row's index in its clip in column INT_COL)"""
    v = torch.randn(sum(lens), heads, 64, generator=gen) * 1.5
    if int_col:
        v[:, :, INT_COL] = torch.cat([torch.arange(n, dtype=torch.float32) for n in lens])[:, None]
    return v


def designed_qkv(name, lens, heads, seed, zero_q=False):
    """[sum(lens)][3 * heads * 64] fp16: q = 8 g_i e_0 (or 0), k = b_j e_0 with b = key_pattern(name) per clip, v random"""
    gen = torch.Generator().manual_seed(seed)
    t = sum(lens)
    qkv = torch.zeros(t, 3, heads, 64)
    qkv[:, 2] = _values(lens, heads, gen, name.startswith("spike") or name == "shift")
    if name == "shift":
        name = "uniform"
    cyc = torch.tensor(G_CYCLE)
    o = 0
    for n in lens:
        i = torch.arange(n)
        if not zero_q:
            for h in range(heads):
                qkv[o:o + n, 0, h, 0] = 8.0 * cyc[(i + h) % 4]
        qkv[o:o + n, 1, :, 0] = key_pattern(name, n).float()[:, None]
        o += n
    return qkv.half().view(t, 3 * heads * 64)


def random_qkv(lens, heads, seed, scale):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(sum(lens), 3 * heads * 64, generator=gen) * scale).half()


def attention_case(name, lens=ATT_LENS, heads=2, causal=False):
    """name: a pattern of PATTERNS or "random" (randn * 1.5, the existing tests' distribution)"""
    seed = 1000 * heads + sum(lens) + 7 * len(name)
    qkv = random_qkv(lens, heads, seed, 1.5) if name == "random" else designed_qkv(name, lens, heads, seed)
    return dict(kind="causal" if causal else "attention", name=name, qkv=qkv, lens=list(lens), heads=heads, d=heads * 64)


def causal_case(name, seq):
    return attention_case(name, [seq] * CAUSAL_NSEQ, 2, causal=True)


def addressed_rows(rp_rows, rp_zero, tmax):
    """the first and last position-table row that some (query, key) pair of a clip of tmax frames addresses after clamping"""
    return min(max(rp_zero - (tmax - 1), 0), rp_rows - 1), min(max(rp_zero + tmax - 1, 0), rp_rows - 1)


def poison_table(rp, rp_zero, tmax):
    """rows that no (valid query, valid key) pair addresses hold POISON, finite: both relpos kernels legitimately FETCH whole
    aligned 32-row blocks of the table (and form scores from them for keys and queries past the clip's end, which the tail mask
    and the `qi < len` store guard then drop), so NaN there would be a false alarm; 1000 in a score that counts is not missed."""
    lo, hi = addressed_rows(rp.shape[0], rp_zero, tmax)
    rp[:lo] = POISON
    rp[hi + 1:] = POISON
    return rp


TABLES = {   # name -> (rp_rows, rp_zero) for a longest clip of tmax frames
    "full": lambda tmax: ((2 * tmax - 1 + 127) // 128 * 128, tmax - 1),   # what the speech encoder passes
    "offset": lambda tmax: (2 * tmax + 100, tmax + 37),                   # rp_zero != tmax - 1, a table longer than needed
    "clamp_both": lambda tmax: (128, 64),                                 # both ends clamp for len 200 and 300
    "clamp_low": lambda tmax: (tmax + 20, 0),                             # every key after the query clamps to row 0
    "clamp_high": lambda tmax: (tmax + 20, tmax + 19),                    # every key before the query clamps to the last row
}


def relpos_case(mode, name, lens=RELPOS_LENS, table="full", heads=2):
    """mode "content": rp = 0, u = v = 0, the pattern `name` in q and k as in attention_case;
    mode "position": q = k = 0, the v bias is 8 e_0 and rp[rp_zero + delta][0] = f(delta) = b(tmax - 1 - delta), b =
        key_pattern(name, 2 tmax - 1): query i sees the logits b(j + tmax - 1 - i), the pattern shifted by its own index (the
        last query of the longest clip sees b(j) itself), all of it through the position MFMAs, the pad and its addressing;
    mode "shift": q = k = 0, v bias 8 e_0, rp[rp_zero + name][0] = 40 for the integer offset `name`, else 0: query i puts all
        its weight on key i - name where the clip has one, and uniform weight elsewhere;
    mode "random": qkv = randn * 1.2, rp = randn * 0.8, u and v = randn * 0.3 (the existing test's distribution).
    exact_g: every position score g_ij of the case is a number fp16 holds exactly (0, or 8 f(delta), an integer below 2048), so
    the LDS-ring kernel's fp16 pad rounds nothing and the kernel is held to the bound WITHOUT the ring term, which at
    max |g| = 810 would allow a tenth of B (tests/test_attention_ref_cpu.py checks the flag against the scores)."""
    d, tmax = heads * 64, max(lens)
    rp_rows, rp_zero = TABLES[table](tmax)
    seed = 2000 * heads + sum(lens) + 7 * len(str(name)) + 13 * len(mode) + rp_rows + rp_zero
    u, v = torch.zeros(d), torch.zeros(d)
    rp = torch.zeros(rp_rows, d)
    if mode == "content":
        qkv = designed_qkv(name, lens, heads, seed)
    elif mode == "random":
        gen = torch.Generator().manual_seed(seed + 1)
        qkv = random_qkv(lens, heads, seed, 1.2)
        rp = torch.randn(rp_rows, d, generator=gen) * 0.8
        u, v = torch.randn(d, generator=gen) * 0.3, torch.randn(d, generator=gen) * 0.3
    else:
        v[::64] = 8.0
        if mode == "shift":
            qkv = designed_qkv("shift", lens, heads, seed, zero_q=True)
            rp[rp_zero + name, ::64] = 40.0
        else:
            assert mode == "position", mode
            qkv = designed_qkv("uniform", lens, heads, seed, zero_q=True)
            delta = torch.arange(-(tmax - 1), tmax)
            rp[rp_zero + delta, ::64] = key_pattern(name, 2 * tmax - 1)[tmax - 1 - delta].float()[:, None]
    rp = poison_table(rp, rp_zero, tmax).half()
    return dict(kind="relpos", name=f"{mode}:{name}:{table}", qkv=qkv, lens=list(lens), heads=heads, d=d, rp=rp, rp_zero=rp_zero,
                u=u, v=v, exact_g=mode != "random")


# every (inputs, shape) the GPU tests run, as arguments of attention_case / causal_case / relpos_case
ATTENTION_CASES = ([(name, ATT_LENS, 2) for name in PATTERNS + ("random",)]
                   + [(name, ATT_NT_LENS, 2) for name in PATTERNS + ("random",)]
                   + [("stair_over", ATT_LENS, 16)])
CAUSAL_CASES = [(name, seq) for seq in CAUSAL_SEQS for name in PATTERNS + ("random",)]
RELPOS_CASES = ([("content", name, RELPOS_LENS, "full") for name in PATTERNS]
                + [("position", name, RELPOS_LENS, "full") for name in POSITION_PATTERNS]
                + [("position", "stair_over", RELPOS_LENS, "offset")]
                + [("shift", delta0, RELPOS_LENS, "full") for delta0 in SHIFTS]
                + [("shift", -33, RELPOS_LENS, "offset")]
                + [("random", "randn", RELPOS_LENS, table) for table in ("full", "offset", "clamp_low", "clamp_high")]
                + [("random", "randn", [200, 300], "clamp_both")])


def case_id(args):
    return "-".join("x".join(map(str, a)) if isinstance(a, list) else str(a) for a in args)


def shift_expected_rows(lens, delta0):
    """per packed row i of its clip: the clip's row i - delta0 that a shift case's query copies, or -1 where the clip has no
    such row (the query then returns the mean of V)"""
    out = []
    for n in lens:
        j = torch.arange(n) - delta0
        out.append(torch.where((j >= 0) & (j < n), j, torch.full_like(j, -1)))
    return torch.cat(out)


def to_device(case, device):
    return {k: v.to(device) if isinstance(v, torch.Tensor) else v for k, v in case.items()}


# ------------------------------------------------------------------------------------------------------------- references
def _clips(qkv, lens, d, heads):
    """per clip: q, k, v [heads][len][64] float64"""
    o = 0
    for n in lens:
        yield o, n, tuple(qkv[o:o + n, i * d:(i + 1) * d].double().view(n, heads, 64).transpose(0, 1) for i in range(3))
        o += n


def _weigh(s, v, causal, out, o, n):
    """softmax of the logits s [heads][n][n] over the visible keys, applied to v: fills rows o .. o + n of (ref, B, A)"""
    if causal:
        i = torch.arange(n, device=s.device)
        s = s.masked_fill(i[None, :] > i[:, None], float("-inf"))
    p = torch.exp(s - s.max(2, keepdim=True).values)
    a = p / p.sum(2, keepdim=True)
    va = v.abs()
    vmax = torch.cummax(va, 1).values if causal else va.max(1, keepdim=True).values.expand_as(va)
    for dst, val in zip(out, (a @ v, a @ va, vmax)):
        dst[o:o + n] = val.transpose(0, 1).reshape(n, -1)


def attention(qkv, lens, d, heads, causal=False):
    """qkv [sum(lens)][3d] packed clips: softmax(q . k / 8) v per clip and head over the clip's keys (causal: keys 0..i for
    query i).  Returns ref, B, A."""
    out = tuple(torch.zeros(sum(lens), d, dtype=torch.float64, device=qkv.device) for _ in range(3))
    for o, n, (q, k, v) in _clips(qkv, lens, d, heads):
        _weigh(q @ k.transpose(1, 2) * 0.125, v, causal, out, o, n)
    return out


def causal_attention(qkv, lens, d, heads):
    return attention(qkv, lens, d, heads, causal=True)


def position_scores(q, rp, rp_zero, v_bias, heads):
    """g [heads][n][n] float64: g_ij = f16(q_i + v) . rp[clamp(rp_zero + i - j, 0, rp_rows - 1)], q [heads][n][64] fp16-valued"""
    n = q.shape[1]
    qv = (q.float() + v_bias.float().view(heads, 1, 64)).half().double()
    i = torch.arange(n, device=q.device)
    idx = (rp_zero + i[:, None] - i[None, :]).clamp(0, rp.shape[0] - 1)
    g_all = qv @ rp.double().view(rp.shape[0], heads, 64).permute(1, 2, 0)          # [heads][n][rp_rows]
    return g_all.gather(2, idx[None].expand(heads, n, n))


def relpos_attention(qkv, lens, d, heads, rp, rp_zero, u, v):
    """scores[i][j] = (f16(q_i + u) . k_j + f16(q_i + v) . rp[clamp(rp_zero + i - j)]) / 8 per clip and head, softmax over the
    clip's frames, times v.  Returns ref, B, A, G (G = max_j |g_ij| of the element's query and head)."""
    out = tuple(torch.zeros(sum(lens), d, dtype=torch.float64, device=qkv.device) for _ in range(4))
    for o, n, (q, k, vv) in _clips(qkv, lens, d, heads):
        qu = (q.float() + u.float().view(heads, 1, 64)).half().double()
        g = position_scores(q, rp, rp_zero, v, heads)
        _weigh((qu @ k.transpose(1, 2) + g) * 0.125, vv, False, out[:3], o, n)
        out[3][o:o + n] = g.abs().max(2).values.transpose(0, 1).repeat_interleave(64, 1)
    return out


def reference(case):
    """(ref, B, A, G or None) of a case of attention_case / causal_case / relpos_case"""
    c = case
    if c["kind"] == "relpos":
        return relpos_attention(c["qkv"], c["lens"], c["d"], c["heads"], c["rp"], c["rp_zero"], c["u"], c["v"])
    return attention(c["qkv"], c["lens"], c["d"], c["heads"], causal=c["kind"] == "causal") + (None,)


def case_bound(case, refs, ring):
    """the bound of a case for the LDS-ring kernel (ring) or any other"""
    ref, B, A, G = refs
    return bound(ref, B, A, G if ring and not case["exact_g"] else None)


def bound(ref, B, A, gmax=None):
    """ulp16(ref) + 2^-11 B + 2^-14 A, and for the LDS-ring kernel (gmax = G) + 2 E B with E = 2^-11 G / 8: the module docstring"""
    t = tolerance(ref, A) + 2.0 ** -11 * B
    if gmax is not None:
        t = t + 2.0 * (2.0 ** -11 * gmax / 8.0) * B
    return t
