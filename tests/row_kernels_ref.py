"""Plain torch float64 restatements of the conformer and decoder row kernels (csrc/speech.hip, csrc/decoder.hip and the CAUSAL
instantiation of csrc/attention.hip), one function per kernel, each stating the contract written in the kernel's own comment.
They take the same fp16 / fp32 tensors the kernel takes (on any device) and widen them; nothing here rounds except where the
contract says the kernel does (the conv taps).

Every reference also returns A, the magnitude at which the kernel's fp32 arithmetic ran, elementwise in the output's shape:
the tests accept |got - ref| <= ulp16(ref) + 2^-14 A (`tolerance`): one fp16 ulp of the reference (half of it the output
rounding) plus an allowance for the fp32 arithmetic of 1/8 of an fp16 half-ulp of A.  ulp16(ref) = 2^-10 |ref|, and 2^-24 where
that is smaller: below 2^-14 fp16 is subnormal and its spacing is 2^-24 whatever the value, so the correctly ROUNDED fp16 of a
reference of 1e-6 is already 2.8e-8 = 29 x (2^-10 + 2^-14) |ref| away from it (measured on ln2's h = f16(x) of an fp32 stream,
where the kernel returns exactly that rounding)."""
import math

import torch


def tolerance(ref, mag):
    return (2.0 ** -10 * ref.abs()).clamp_min(2.0 ** -24) + 2.0 ** -14 * mag


def layer_norm(x, w, b, eps):
    """(x - mean) * rstd * w + b over the last dimension, biased variance; A = |w| |x - mean| rstd + |b|"""
    x, w, b = x.double(), w.double(), b.double()
    xc = x - x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    return xc * rstd * w + b, w.abs() * xc.abs() * rstd + b.abs()


def layer_norm_mean_term(x, w, eps):
    """|w| mean_i |x_i| rstd: the magnitude at which the row's MEAN was formed, carried to the output.  The fp32 mean
    (ln_core.hpp: sum / d) is off by a few ulp of mean_i |x_i|, and that offset reaches every centred value, the ones with
    x ~ mean included, where A of `layer_norm` is next to nothing.  Rule T's 2^-14 A hides it under the fp16 rounding; a bound
    at fp32 level (the fp32 stream that ln2 writes back) has to carry it."""
    x, w = x.double(), w.double()
    xc = x - x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    return w.abs() * x.abs().mean(-1, keepdim=True) * rstd


def stack_ln(fb, lens, w, b, eps, ldo):
    """fb [n][t][nb] fp32, lens: stacked frames per clip.  out[row(i, j)][0 : 2nb] = LN(fb[i][2j] | fb[i][2j+1]) * w + b, the
    columns 2nb .. ldo-1 are zero; rows packed in clip order."""
    n, t, nb = fb.shape
    rows = [fb[i, :2 * L].reshape(L, 2 * nb) for i, L in enumerate(lens)]
    y, mag = layer_norm(torch.cat(rows), w, b, eps)
    pad = torch.zeros(y.shape[0], ldo - 2 * nb, dtype=torch.float64, device=fb.device)
    return torch.cat([y, pad], 1), torch.cat([mag, pad], 1)


def ln2_stream(x, w1, b1, eps):
    """the first half of ln2: x <- LN1(x)"""
    return layer_norm(x, w1, b1, eps)


def ln2_out(x_stored, w2, b2, eps):
    """the second half: h = w2 ? LN2(x) : x, of the x the stream HOLDS after the first half (rounded for an fp16 stream)"""
    if w2 is None:
        return x_stored.double(), x_stored.double().abs()
    return layer_norm(x_stored, w2, b2, eps)


def silu(v):
    return v / (1.0 + torch.exp(-v))


def dwconv_bn_silu(x, lens, w, scale, shift, round_taps=True):
    """x [rows][C] fp16 packed clips, w [C][K] fp32 taps, K odd.  y[t][c] = silu(scale[c] * sum_k w16[c][k] x[t + k - (K-1)/2][c] +
    shift[c]) within each clip, frames outside the clip are zero; w16 = the taps rounded to fp16 (round_taps: the kernel's
    contract) or the fp32 taps as given.  A = |scale| sum_k |w x| + |shift|."""
    C, K = w.shape
    half = (K - 1) // 2
    taps = (w.half() if round_taps else w).double()
    scale, shift = scale.double(), shift.double()
    ys, mags = [], []
    o = 0
    for L in lens:
        clip = x[o:o + L].double()
        o += L
        padded = torch.cat([torch.zeros(half, C, dtype=torch.float64, device=x.device), clip,
                            torch.zeros(half, C, dtype=torch.float64, device=x.device)])
        acc = torch.zeros(L, C, dtype=torch.float64, device=x.device)
        mag = torch.zeros_like(acc)
        for k in range(K):
            term = taps[:, k] * padded[k:k + L]
            acc += term
            mag += term.abs()
        ys.append(silu(scale * acc + shift))
        mags.append(scale.abs() * mag + shift.abs())
    return torch.cat(ys), torch.cat(mags)


def pool_attention(q, kv, lens, heads):
    """q [n][d], kv [rows][2d] (k | v) packed clips: per clip and head softmax(q . k_j / 8) over the clip's rows, times v; a clip
    of length 0 yields zeros.  A = max_j |v_j| per output column."""
    n, d = q.shape
    ctx = torch.zeros(n, d, dtype=torch.float64, device=q.device)
    mag = torch.zeros_like(ctx)
    o = 0
    for i, L in enumerate(lens):
        if L == 0:
            continue
        k = kv[o:o + L, :d].double().view(L, heads, 64)
        v = kv[o:o + L, d:].double().view(L, heads, 64)
        o += L
        s = torch.einsum("hc,jhc->hj", q[i].double().view(heads, 64), k) * 0.125
        p = torch.exp(s - s.max(1, keepdim=True).values)
        p = p / p.sum(1, keepdim=True)
        ctx[i] = torch.einsum("hj,jhc->hc", p, v).reshape(d)
        mag[i] = v.abs().max(0).values.reshape(d)
    return ctx, mag


def sum_terms(x, parts, c, group):
    """the terms of the residual sum in the order the kernel documents: x, the slabs ascending, then the constant"""
    rows = x.shape[0]
    terms = [x] + [parts[z, :rows] for z in range(0 if parts is None else parts.shape[0])]
    if c is not None:
        terms.append(c[torch.arange(rows, device=x.device) // group])
    return terms


def sum_stream(x, parts, c, group):
    """x + sum_z parts[z] (+ c[row / group]); A = the sum of the terms' magnitudes"""
    terms = [t.double() for t in sum_terms(x, parts, c, group)]
    return sum(terms[1:], terms[0]), sum((t.abs() for t in terms[1:]), terms[0].abs())


def sum_stream_f32(x, parts, c, group):
    """the same sum formed in fp32 in the kernel's order: what an fp32 stream must hold bit for bit"""
    terms = [t.float() for t in sum_terms(x, parts, c, group)]
    v = terms[0]
    for t in terms[1:]:
        v = v + t
    return v


def dec_attention(kv, anc, rows, d, heads, pos):
    """kv [>= pos+1][rows_pad][3d] (q | k | v slabs), anc [rows][>= pos].  Query: q of slab pos, row r.  Key / value j < pos: row
    anc[r][j] of slab j; key / value pos: row r of slab pos.  softmax(q . k / 8) v per head.  A = max_j |v_j| per column."""
    r = torch.arange(rows, device=kv.device)
    src = torch.cat([anc[:rows, :pos].long(), r[:, None]], 1)                      # [rows][pos+1]
    g = kv[torch.arange(pos + 1, device=kv.device)[None, :], src].double()          # [rows][pos+1][3d]
    q = kv[pos, :rows, :d].double().view(rows, heads, 64)
    k = g[:, :, d:2 * d].reshape(rows, pos + 1, heads, 64)
    v = g[:, :, 2 * d:].reshape(rows, pos + 1, heads, 64)
    s = torch.einsum("rhc,rjhc->rhj", q, k) * 0.125
    p = torch.exp(s - s.max(2, keepdim=True).values)
    p = p / p.sum(2, keepdim=True)
    ctx = torch.einsum("rhj,rjhc->rhc", p, v).reshape(rows, d)
    return ctx, v.abs().max(1).values.reshape(rows, d)


def causal_attention(qkv, nseq, seq, d, heads):
    """qkv [nseq * seq][3d]: query i of a sequence sees its keys 0..i, scores / 8.  A = max_{j <= i} |v_j| per column."""
    t = qkv[:nseq * seq].double().view(nseq, seq, 3, heads, 64)
    q, k, v = (t[:, :, i].transpose(1, 2) for i in range(3))                        # [nseq][heads][seq][64]
    s = q @ k.transpose(2, 3) / math.sqrt(64.0)
    i = torch.arange(seq, device=qkv.device)
    s = s.masked_fill(i[None, :] > i[:, None], float("-inf"))
    p = torch.exp(s - s.max(3, keepdim=True).values)
    p = p / p.sum(3, keepdim=True)
    ctx = (p @ v).transpose(1, 2).reshape(nseq * seq, d)
    mag = torch.cummax(v.abs(), 2).values.transpose(1, 2).reshape(nseq * seq, d)
    return ctx, mag
