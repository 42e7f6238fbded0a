"""CPU: the inputs, the bound and the references of tests/attention_ref.py, before a GPU is involved.

(a) `emulate` is a model of the schedule of csrc/attn_core.hpp in the kernel's number formats: waves of 32 queries (rows past
    the clip's end are copies of its last query, as the kernels clamp them), key blocks of 32, the reference m of a query moves
    to max(m, block maximum) when ANY query of its wave has a block maximum above m + 8 in the log2 domain, p = exp2 in fp32,
    P rounded to fp16 for the PV product, fp32 PV and row sums, the tail mask, the causal mask.  (A causal 128-query block stops
    at key min(len, q0 + 128); the blocks behind that are wholly masked for its queries, where a block maximum of -inf moves
    nothing and every p is 0, so the model simply runs them.)  It records which (wave, key block) steps rescaled and the
    largest p, and with them the tests prove that each designed pattern does what attention_ref.key_pattern claims AT THE
    SHAPES THE GPU TESTS USE.
(b) The emulation's output stays under attention_ref.bound on every (inputs, shape) the GPU tests run, the LDS-ring variant
    (position scores rounded to fp16) under the ring bound: inputs and bound are compatible, with the margin printed.
(c) The float64 references against torch.softmax formulations, the closed forms of the designed inputs, and the position-table
    clamp against an unclamped reference on a table padded by repeating its end rows."""
import pytest
import torch

from tests import attention_ref as R

SL2E = torch.tensor(0.125, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)


def emulate(s, v, causal, keep_lsum=False):
    """s [heads][n][n] fp32 unscaled scores (q . k, + position term), v [heads][n][64] fp32 -> out [heads][n][64] fp16,
    fired [heads][waves][blocks] bool, the largest p of a valid query"""
    heads, n, _ = s.shape
    nw = (n + 31) // 32
    qi = torch.arange(nw * 32)
    key = torch.arange(nw * 32)
    sx = torch.full((heads, nw * 32, nw * 32), float("-inf"))
    sx[:, :, :n] = s[:, qi.clamp(max=n - 1)]                       # rows past the end: the last query; keys past it: masked
    if causal:
        sx = sx.masked_fill(key[None, :] > qi[:, None], float("-inf"))
    vx = v[:, key.clamp(max=n - 1)]
    m = torch.full((heads, nw * 32), -1e30)
    lsum = torch.zeros(heads, nw * 32)
    o = torch.zeros(heads, nw * 32, 64)
    fired = torch.zeros(heads, nw, nw, dtype=torch.bool)
    pmax = 0.0
    for kb in range(nw):
        sb = sx[:, :, kb * 32:(kb + 1) * 32]
        mx = sb.max(2).values * SL2E
        fire = (mx > m + 8.0).view(heads, nw, 32).any(2)
        fired[:, :, kb] = fire
        m_new = torch.where(fire.repeat_interleave(32, 1), torch.maximum(m, mx), m)
        alpha = torch.exp2(m - m_new)
        m = m_new
        lsum = lsum if keep_lsum else lsum * alpha   # keep_lsum: a deliberately wrong schedule, for the test of the bound
        o = o * alpha[:, :, None]
        p = torch.exp2((sb.double() * SL2E.double() - m.double()[:, :, None]).float())   # the fma rounds once
        lsum = lsum + p.sum(2)
        o = o + p.half().float() @ vx[:, kb * 32:(kb + 1) * 32]
        pmax = max(pmax, p[:, :n].max().item())
    return (o * (1.0 / lsum)[:, :, None]).half()[:, :n], fired, pmax


def run_emulation(case, ring=False, keep_lsum=False):
    """the emulation over a whole case: out [t][d] fp16, per clip (n, fired), the largest p"""
    c = case
    d, heads = c["d"], c["heads"]
    out = torch.zeros(sum(c["lens"]), d, dtype=torch.float16)
    clips, pmax = [], 0.0
    o = 0
    for n in c["lens"]:
        q, k, v = (c["qkv"][o:o + n, i * d:(i + 1) * d].view(n, heads, 64).transpose(0, 1) for i in range(3))
        if c["kind"] == "relpos":
            qu = (q.float() + c["u"].view(heads, 1, 64)).half().float()
            g = R.position_scores(q, c["rp"], c["rp_zero"], c["v"], heads).float()   # exact products, fp32 sums
            s = qu @ k.float().transpose(1, 2) + (g.half().float() if ring else g)
        else:
            s = q.float() @ k.float().transpose(1, 2)
        res, fired, pm = emulate(s, v.float(), c["kind"] == "causal", keep_lsum)
        out[o:o + n] = res.transpose(0, 1).reshape(n, d)
        clips.append((n, fired))
        pmax = max(pmax, pm)
        o += n
    return out, clips, pmax


def later(fired):
    """rescales after the first key block, per (head, wave)"""
    return fired[:, :, 1:].sum(2)


def full_waves(n):
    """the waves whose 32 queries hold all four g of the cycle (a clip's last wave may own a single query)"""
    return [w for w in range((n + 31) // 32) if n - 32 * w >= 4]


def worst_ratio(out, case, ring=False):
    refs = R.reference(case)
    return ((out.double() - refs[0]).abs() / R.case_bound(case, refs, ring)).max().item()


def check_claims(name, clips, pmax, causal):
    """what key_pattern promises of a pattern carried by q and k, at these clips"""
    tail = diag = 0
    for n, fired in clips:
        nb = (n + 31) // 32
        lat = later(fired)
        # (the ramp climbs 0.25 per key: the one-key tail block of a clip of 33 is 0.25 above block 0, it takes 23 keys to move m)
        if name in ("stair_over", "stair_desc", "ramp", "spike_last") and nb >= 2 and (name != "ramp" or n >= 64):
            # causal: wave w sees w + 1 blocks, wave 0 has no later block; the last-key spike is seen by the last query only
            waves = [w for w in full_waves(n) if not causal or (w >= 1 and name != "spike_last")]
            if name == "spike_last":
                waves = [w for w in waves if w == nb - 1] if causal else waves
            assert all((lat[:, w] >= 1).all() for w in waves), (name, n, lat.tolist())
        if name in ("stair_hold", "uniform", "spike_first") or (name == "stair_under" and nb <= 2):
            assert (lat == 0).all(), (name, n, lat.tolist())
        if name == "stair_under" and nb >= 3 and not causal:
            # g = 1: blocks 2, 4, ... move the reference, the odd ones hold it with p = e^5.5
            assert all((lat[:, w] >= (nb - 1) // 2).all() for w in full_waves(n)), (name, n, lat.tolist())
        if n % 32:
            tail += int(fired[:, :, nb - 1].sum()) if nb >= 2 else 0
        diag += sum(int(fired[:, w, w].sum()) for w in range(1, nb))
    if name in ("stair_under", "stair_hold") and max(n for n, _ in clips) > 32:
        assert 128.0 <= pmax < 256.0, (name, pmax)
    assert pmax <= 256.0, (name, pmax)
    # (not the ramp: the tails here are 1, 2, 8 and 12 keys long, at most 3 above the block before them)
    if name in ("stair_over", "stair_desc", "spike_last") and any(n % 32 and n > 32 for n, _ in clips):
        assert tail >= 1, (name, "no rescale in a tail block with masked keys")
    if causal and name in ("stair_over", "stair_desc", "ramp") and max(n for n, _ in clips) > 32:
        assert diag >= 1, (name, "no rescale in a block that straddles the diagonal")
    return tail, diag


def describe(clips):
    return " ".join(f"{n}:{int(later(f).sum())}/{f[:, :, 1:].numel()}" for n, f in clips)


# -------------------------------------------------------------------------------- (a) + (b): patterns, schedule, emulation
@pytest.mark.parametrize("args", R.ATTENTION_CASES, ids=R.case_id)
def test_attention_inputs(args):
    case = R.attention_case(*args)
    out, clips, pmax = run_emulation(case)
    tail, _ = check_claims(args[0], clips, pmax, False)
    ratio = worst_ratio(out, case)
    print(f"attention {R.case_id(args)}: later-block rescales / steps per clip {describe(clips)}, in masked tail blocks {tail}, "
          f"max p {pmax:.1f}, emulation worst err / bound {ratio:.3f}")
    assert ratio < 1.0


@pytest.mark.parametrize("args", R.CAUSAL_CASES, ids=R.case_id)
def test_causal_inputs(args):
    case = R.causal_case(*args)
    out, clips, pmax = run_emulation(case)
    tail, diag = check_claims(args[0], clips, pmax, True)
    ratio = worst_ratio(out, case)
    print(f"causal {R.case_id(args)}: later-block rescales / steps per clip {describe(clips)}, in masked tail blocks {tail}, "
          f"in blocks on the diagonal {diag}, max p {pmax:.1f}, emulation worst err / bound {ratio:.3f}")
    assert ratio < 1.0


@pytest.mark.parametrize("args", R.RELPOS_CASES, ids=R.case_id)
def test_relpos_inputs(args):
    mode, name = args[0], args[1]
    case = R.relpos_case(*args)
    ratios = []
    for ring in (False, True):
        out, clips, pmax = run_emulation(case, ring)
        if mode == "content":
            check_claims(name, clips, pmax, False)
        assert pmax <= 256.0
        total = sum(int(later(f).sum()) for _, f in clips)
        if mode == "position" and name == "stair_hold":
            assert total == 0 and 128.0 <= pmax < 256.0
        if mode == "position" and name in ("stair_under", "stair_over", "ramp"):
            assert all((later(f) >= 1).all() for n, f in clips if n > 64)   # q = 0: every query is a g = 1 lane
        if mode == "shift":
            assert total >= 1
        ratios.append(worst_ratio(out, case, ring))
    print(f"relpos {R.case_id(args)}: later-block rescales / steps per clip {describe(clips)}, max p {pmax:.1f}, emulation worst "
          f"err / bound {ratios[0]:.3f} (fp32 pad), {ratios[1]:.3f} (fp16 pad, its bound)")
    assert max(ratios) < 1.0


def test_a_missed_rescale_of_the_row_sum_breaks_the_bound():
    """the check of the checker: the emulation with the `lsum *= alpha` of attn_lazy_rescale left out misses the bound on every
    pattern that claims later-block rescales (on randn * 1.5 the same omission passes the flat 6e-3 on many seeds)"""
    for name in ("stair_under", "stair_over", "stair_desc", "ramp", "spike_last"):
        case = R.attention_case(name)
        out, _, _ = run_emulation(case, keep_lsum=True)
        ratio = worst_ratio(out, case)
        print(f"{name} without lsum *= alpha: emulation worst err / bound {ratio:.1f}")
        assert ratio > 1.0, name


# ------------------------------------------------------------------------------------------------ (c) reference cross-checks
def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1.0), (a - b).abs().max().item()


def _softmax_attention(q, k, v, extra=None, causal=False):
    s = q @ k.transpose(1, 2) / 8.0 + (0.0 if extra is None else extra / 8.0)
    if causal:
        n = s.shape[1]
        s = s + torch.full((n, n), float("-inf"), dtype=torch.float64).triu(1)
    return torch.softmax(s, 2) @ v


@pytest.mark.parametrize("causal", [False, True])
def test_attention_ref_matches_softmax(causal):
    lens, heads = [5, 1, 40], 3
    d = heads * 64
    qkv = R.random_qkv(lens, heads, 3, 1.5)
    ref, B, A = R.attention(qkv, lens, d, heads, causal)
    assert (B >= ref.abs() - 1e-12).all() and (A >= B - 1e-12).all()
    o = 0
    for n in lens:
        q, k, v = (qkv[o:o + n, i * d:(i + 1) * d].double().view(n, heads, 64).transpose(0, 1) for i in range(3))
        _close(ref[o:o + n], _softmax_attention(q, k, v, causal=causal).transpose(0, 1).reshape(n, d))
        vis = v.abs().cummax(1).values if causal else v.abs().max(1, keepdim=True).values.expand_as(v)
        _close(A[o:o + n], vis.transpose(0, 1).reshape(n, d))
        o += n
    if causal:
        _close(R.causal_attention(qkv, lens, d, heads)[0], ref)


def test_relpos_ref_matches_softmax_and_clamps():
    lens, heads = [7, 40], 2
    d, tmax = heads * 64, 40
    g = torch.Generator().manual_seed(4)
    qkv = R.random_qkv(lens, heads, 4, 1.2)
    u, vb = torch.randn(d, generator=g) * 0.3, torch.randn(d, generator=g) * 0.3
    for rp_rows, rp_zero in ((2 * tmax - 1, tmax - 1), (100, 50), (24, 10), (24, 0), (24, 23)):
        rp = (torch.randn(rp_rows, d, generator=g) * 0.8).half()
        ref, B, A, G = R.relpos_attention(qkv, lens, d, heads, rp, rp_zero, u, vb)
        # the same table padded by repeating its end rows needs no clamp
        padded = torch.cat([rp[:1].expand(tmax, d), rp, rp[-1:].expand(tmax, d)])
        o = 0
        for n in lens:
            q, k, v = (qkv[o:o + n, i * d:(i + 1) * d].view(n, heads, 64).transpose(0, 1) for i in range(3))
            qu = (q.float() + u.view(heads, 1, 64)).half().double()
            qv = (q.float() + vb.view(heads, 1, 64)).half().double()
            i = torch.arange(n)
            rows = padded.double().view(-1, heads, 64)[tmax + rp_zero + i[:, None] - i[None, :]]      # [n][n][heads][64]
            pos = torch.einsum("hid,ijhd->hij", qv, rows)
            want = _softmax_attention(qu, k.double(), v.double(), extra=pos)
            _close(ref[o:o + n], want.transpose(0, 1).reshape(n, d))
            _close(G[o:o + n], pos.abs().max(2).values.transpose(0, 1).repeat_interleave(64, 1))
            o += n
        assert (B >= ref.abs() - 1e-12).all() and (A >= B - 1e-12).all()


def test_designed_inputs_have_their_closed_forms():
    """uniform: the mean of V (causal: the prefix mean); a spike seen by a g = 1 query: that V row to far below an fp16 ulp; a
    shift: row i - delta0 of V where the clip has one, its mean elsewhere; the designed logits are exact in fp16."""
    lens, heads = [33, 97], 2
    d = heads * 64
    for causal in (False, True):
        c = R.attention_case("uniform", lens, heads, causal)
        ref = R.reference(c)[0]
        o = 0
        for n in lens:
            v = c["qkv"][o:o + n, 2 * d:].double()
            want = v.cumsum(0) / torch.arange(1, n + 1)[:, None] if causal else v.mean(0, keepdim=True).expand(n, d)
            _close(ref[o:o + n], want)
            o += n
    for name, causal in (("spike_last", False), ("spike_first", False), ("spike_first", True)):
        c = R.attention_case(name, lens, heads, causal)
        ref = R.reference(c)[0]
        o = 0
        for n in lens:
            v = c["qkv"][o:o + n, 2 * d:].double()
            row = v[n - 1] if name == "spike_last" else v[0]
            for h in range(heads):
                mine = [i for i in range(n) if R.G_CYCLE[(i + h) % 4] == 1.0]
                assert (ref[o:o + n][mine, h * 64:(h + 1) * 64] - row[h * 64:(h + 1) * 64]).abs().max() < 1e-12
            o += n
    for delta0 in R.SHIFTS:
        c = R.relpos_case("shift", delta0, lens, heads=heads)
        ref = R.reference(c)[0]
        want = R.shift_expected_rows(lens, delta0)
        col = ref[:, R.INT_COL::64]
        hit = want >= 0
        assert (col[hit] - want[hit, None]).abs().max() < 1e-9
        o = 0
        for n in lens:
            miss = ~hit[o:o + n]
            if miss.any():
                assert (col[o:o + n][miss] - (n - 1) / 2.0).abs().max() < 1e-9
            o += n
    for name in R.PATTERNS:
        b = R.key_pattern(name, 514)
        assert torch.equal(b.half().double(), b) and torch.equal((8 * b).half().double(), 8 * b)
    b = R.key_pattern("stair_over", 2 * 300 - 1)
    assert torch.equal((8 * b).half().double(), 8 * b)      # the position scores 8 f(delta) survive the ring's fp16 pad


def test_unaddressed_position_rows_are_poisoned():
    for args in R.RELPOS_CASES:
        c = R.relpos_case(*args)
        rows, tmax = c["rp"].shape[0], max(c["lens"])
        i = torch.arange(tmax)
        used = torch.zeros(rows, dtype=torch.bool)
        used[(c["rp_zero"] + i[:, None] - i[None, :]).clamp(0, rows - 1).unique()] = True
        assert (c["rp"][~used] == R.POISON).all() and (c["rp"][used].abs() < R.POISON).all(), args
        assert torch.isfinite(c["rp"]).all()
        if c["exact_g"]:   # what lets the ring kernel's bound go without its fp16-pad term
            o = 0
            for n in c["lens"]:
                q = c["qkv"][o:o + n, :c["d"]].view(n, c["heads"], 64).transpose(0, 1)
                g = R.position_scores(q, c["rp"], c["rp_zero"], c["v"], c["heads"])
                assert torch.equal(g.half().double(), g), args
                o += n
