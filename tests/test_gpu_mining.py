"""GPU: bitext mining (sonar_amd/csrc/mining.hip, sonar_amd/mining.py) against the CPU restatement of LASER's
mine_bitexts.py in tests/mining_ref.py.

Most of this file is exact equality.  `smi_xsim_mine` only moves and compares its inputs, so every (src, trg, score) list
must equal the reference's, element for element; the whole path is exact on integer-valued rows with the `distance`
margin and k in {1, 2, 4} (every cosine an integer, every mean and margin dyadic).  The tolerances that remain are
derived: `d * 2^-23` for the fp32 accumulation of a cosine of normalised rows (tests/test_gpu_xsim_kernels.py), and for
the ratio a / b of such a cosine over an exactly known b, `d * 2^-23 / |b| + 4 * 2^-24 * |a / b|` (the cosine's error
divided by |b|, plus four fp32 roundings -- two means, their half-sum, the quotient -- relative to the result)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import mining_ref as R

pytestmark = pytest.mark.gpu

RETRIEVALS = ("fwd", "bwd", "intersect", "max")
SENT_I, SENT_F = -77, 12345.0


# ------------------------------------------------------------------------------------------------ helpers
def _capacity(nx, ny, retrieval):
    return {"fwd": nx, "bwd": ny, "intersect": nx, "max": min(nx, ny)}[retrieval]


def _call_mine(fb, fs, bb, bs, nx, ny, retrieval, threshold=None, ws_short=0, guard=64):
    """smi_xsim_mine on device tensors, straight through ctypes: outputs prefilled with sentinels, the workspace a window
    of a larger buffer.  Returns (status, src, trg, score, count, workspace guards untouched)."""
    from sonar_amd import _lib

    lib = _lib.load()
    kind = _lib.SMI_MINE[retrieval]
    cap = _capacity(nx, ny, retrieval)
    need = int(lib.smi_xsim_mine_workspace_bytes(nx, ny, kind))
    assert need > 0
    big = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = big[guard:guard + need]
    src = torch.full((cap,), SENT_I, dtype=torch.int32, device="cuda")
    trg = torch.full((cap,), SENT_I, dtype=torch.int32, device="cuda")
    score = torch.full((cap,), SENT_F, dtype=torch.float32, device="cuda")
    count = torch.full((1,), SENT_I, dtype=torch.int32, device="cuda")
    status = lib.smi_xsim_mine(fb.data_ptr(), fs.data_ptr(), nx, bb.data_ptr(), bs.data_ptr(), ny, kind,
                               -math.inf if threshold is None else threshold, src.data_ptr(), trg.data_ptr(),
                               score.data_ptr(), count.data_ptr(), ws.data_ptr(), need - ws_short,
                               _lib.current_stream_ptr())
    torch.cuda.synchronize()
    guards_ok = bool((big[:guard] == 0xA5).all() and (big[guard + need:] == 0xA5).all())
    return status, src.cpu(), trg.cpu(), score.cpu(), int(count.item()), guards_ok


def _dev(fb, fs, bb, bs):
    return (torch.from_numpy(np.asarray(fb)).int().cuda(), torch.from_numpy(np.asarray(fs, dtype=np.float32)).cuda(),
            torch.from_numpy(np.asarray(bb)).int().cuda(), torch.from_numpy(np.asarray(bs, dtype=np.float32)).cuda())


def _columns(pairs):
    return (torch.tensor([p[0] for p in pairs], dtype=torch.int64), torch.tensor([p[1] for p in pairs], dtype=torch.int64),
            torch.tensor([p[2] for p in pairs], dtype=torch.float32))


def _assert_pairs(got, want_pairs, what):
    """got: (src, trg, score) tensors; want_pairs: the reference's list.  Exact, in order."""
    ws, wt, wv = _columns(want_pairs)
    gs, gt, gv = (t.cpu() for t in got)
    assert gs.shape[0] == len(want_pairs), f"{what}: {gs.shape[0]} pairs, the reference has {len(want_pairs)}"
    bad = ((gs.long() != ws) | (gt.long() != wt) | (gv != wv)).nonzero().squeeze(1)
    if bad.numel():
        r = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {len(want_pairs)} pairs differ, first at {r}: got "
                             f"({int(gs[r])}, {int(gt[r])}, {float(gv[r])}) want {want_pairs[r]}")


def _assert_mine_exact(fb, fs, bb, bs, nx, ny, retrieval, threshold=None):
    """The raw call: the pairs in candidate order, the count, nothing written past the count or outside the workspace."""
    want = R.mine(fb, fs, bb, bs, nx, ny, retrieval, threshold)
    status, src, trg, score, count, guards_ok = _call_mine(*_dev(fb, fs, bb, bs), nx, ny, retrieval, threshold)
    assert status == 0 and guards_ok
    assert count == len(want), (count, len(want))
    _assert_pairs((src[:count], trg[:count], score[:count]), want, f"{retrieval} {nx} x {ny}")
    assert (src[count:] == SENT_I).all() and (trg[count:] == SENT_I).all() and (score[count:] == SENT_F).all()
    return want


# ------------------------------------------------------------- 1. smi_xsim_mine in isolation, exact
#   1 x 1          one thread (max: two candidates)
#   1 x 300, 300 x 1   lopsided: every candidate of the long side competes for one row; one block and a bit
#   255 x 257      max: 512 candidates = two full blocks; fwd one partial block, bwd one block and one thread
#   600 x 513      several blocks, the last partial
#   2305 x 769     ten and four blocks; max: 3074 candidates
#   65536 x 1, 32768 x 32769   the block-count scan (one block of 256 threads, csrc/bucket.hpp) where a thread's run is one
#                  count: fwd 65 536 candidates = 256 blocks, every thread owns one; max 65 537 = 257 blocks, a run is two
#                  counts and half the threads own none -- once with one target for all, once as a matching of several rounds
_SHAPES = [(1, 1), (1, 300), (300, 1), (255, 257), (600, 513), (2305, 769), (65536, 1), (32768, 32769)]
_QUARTERS = np.arange(-4, 5, dtype=np.float32) / 4      # multiples of 1/4 in [-1, 1]


@functools.lru_cache(maxsize=None)
def _isolated_case(nx, ny):
    rng = np.random.default_rng(1000003 * nx + ny)
    fb, bb = rng.integers(0, ny, nx), rng.integers(0, nx, ny)
    fs, bs = rng.choice(_QUARTERS, nx), rng.choice(_QUARTERS, ny)
    return fb, fs, bb, bs


@pytest.mark.parametrize("retrieval", RETRIEVALS)
@pytest.mark.parametrize("nx,ny", _SHAPES)
def test_mine_isolated_exact(nx, ny, retrieval):
    from sonar_amd import mining

    fb, fs, bb, bs = _isolated_case(nx, ny)
    if retrieval == "max" and nx + ny > 255:
        # a condition on the INPUTS (reference alone): the tie order decides a good part of the matching
        share = R.contested_share(fb, fs, bb, bs, nx, ny)
        _, rounds, history = R.parallel_rounds(R.candidates(fb, fs, bb, bs), nx, ny)
        print(f"{nx} x {ny}: {share:.1%} of the accepted pairs had an equal-score competitor; {rounds} rounds, live {history}")
        assert share >= 0.10, share
    want = _assert_mine_exact(fb, fs, bb, bs, nx, ny, retrieval)
    # through the Python layer: the final order (max: score descending, equal scores in candidate order)
    got = mining.mine_candidates(*_dev(fb, fs, bb, bs), nx, ny, retrieval)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int64 and got[2].dtype == torch.float32
    _assert_pairs(got, R.final_order(want, retrieval), f"final order, {retrieval} {nx} x {ny}")
    # and with a threshold in the middle of the value set
    _assert_mine_exact(fb, fs, bb, bs, nx, ny, retrieval, threshold=0.25)


# ------------------------------------------------------------------------------------- 2. many rounds
def test_mine_max_monotone_chain_many_rounds():
    """Scores rise along x0 -> y0 -> x1 -> y1 -> ...: every candidate but the top one loses one of its slots to the next
    link, so a round accepts one pair."""
    n = 40
    fb, bb = np.arange(n), np.minimum(np.arange(n) + 1, n - 1)
    fs, bs = np.arange(n, dtype=np.float32) * 2, np.arange(n, dtype=np.float32) * 2 + 1
    _, rounds, _ = R.parallel_rounds(R.candidates(fb, fs, bb, bs), n, n)
    print(f"chain of {n} + {n} candidates: {rounds} rounds")
    assert rounds >= 20, rounds
    want = _assert_mine_exact(fb, fs, bb, bs, n, n, "max")
    assert len(want) == n


# ------------------------------------------------------------------------------------- 3. exclusions
def _exclusion_case():
    """nx = 6, ny = 5.  Excluded: x1 (no neighbour, -1), x2 (index = ny), x4 (NaN), y3 (index = nx), y4 (NaN).
    -0 / +0: x0 -> y0 scores -0 and y1 -> x0 scores +0: equal, so the lower candidate number (the forward one) goes first."""
    nan = float("nan")
    fb = np.array([0, -1, 5, 2, 2, 1])
    fs = np.array([-0.0, 0.75, 0.75, 0.5, nan, 0.0], dtype=np.float32)
    bb = np.array([3, 0, 3, 6, 0])
    bs = np.array([0.25, 0.0, 0.5, 0.75, nan], dtype=np.float32)
    return fb, fs, bb, bs, 6, 5


def test_reference_on_the_exclusion_case():
    fb, fs, bb, bs, nx, ny = _exclusion_case()
    assert R.mine(fb, fs, bb, bs, nx, ny, "fwd") == [(0, 0, -0.0), (3, 2, 0.5), (5, 1, 0.0)]
    assert R.mine(fb, fs, bb, bs, nx, ny, "bwd") == [(3, 0, 0.25), (0, 1, 0.0), (3, 2, 0.5)]
    assert R.mine(fb, fs, bb, bs, nx, ny, "intersect") == [(3, 2, 0.5)]
    # walk: (3,2,.5) fwd 3; (3,2,.5) bwd 2 blocked; (3,0,.25) blocked; then the zeros by number: fwd 0 (0,0) accepted,
    # fwd 5 (5,1) accepted, bwd 1 (0,1) blocked
    assert R.mine(fb, fs, bb, bs, nx, ny, "max") == [(0, 0, -0.0), (3, 2, 0.5), (5, 1, 0.0)]
    assert R.mine(fb, fs, bb, bs, nx, ny, "max", threshold=0.0) == [(3, 2, 0.5)]


@pytest.mark.parametrize("threshold", [None, 0.0, 0.5])
@pytest.mark.parametrize("retrieval", RETRIEVALS)
def test_mine_exclusions_threshold_and_untouched_tails(retrieval, threshold):
    """NaN scores, indices -1 and n, -0 against +0, a strict threshold; the candidate arrays are windows of larger buffers
    whose neighbours would show a read outside: scores of 2^100 (they would win `max`), and around bwd_best / fwd_best
    the very row numbers that would make a candidate with index -1 or n look mutual."""
    fb, fs, bb, bs, nx, ny = _exclusion_case()
    want = R.mine(fb, fs, bb, bs, nx, ny, retrieval, threshold)

    def window(values, before, after, dtype):
        buf = torch.tensor([before] + list(values) + [after], dtype=dtype).cuda()
        return buf[1:-1]

    # x1 has fwd_best = -1: bwd_best[-1] = 1 would make it mutual; x2 has fwd_best = ny: bwd_best[ny] = 2 likewise
    dfb = window(fb, 4, 4, torch.int32)           # fwd_best[-1] / fwd_best[nx]: y4 / y3 look there if they read at all
    dbb = window(bb, 1, 2, torch.int32)
    dfs = window(fs, 2.0 ** 100, 2.0 ** 100, torch.float32)
    dbs = window(bs, 2.0 ** 100, 2.0 ** 100, torch.float32)
    status, src, trg, score, count, guards_ok = _call_mine(dfb, dfs, dbb, dbs, nx, ny, retrieval, threshold)
    assert status == 0 and guards_ok
    assert count == len(want)
    _assert_pairs((src[:count], trg[:count], score[:count]), want, f"{retrieval}, threshold {threshold}")
    assert (src[count:] == SENT_I).all() and (trg[count:] == SENT_I).all() and (score[count:] == SENT_F).all()
    if threshold is not None:
        assert all(p[2] > threshold for p in want)
        cands = [c for c in R.candidates(fb, fs, bb, bs) if not R.excluded(c, nx, ny)]
        assert any(c[2] == threshold for c in cands)  # candidates score exactly the threshold: strictness is exercised


# --------------------------------------------------------------------------------- 4. short workspace
@pytest.mark.parametrize("retrieval", ["intersect", "max"])
def test_mine_refuses_short_workspace(retrieval):
    """One byte short of smi_xsim_mine_workspace_bytes: an error before any launch, outputs untouched; the exact size works."""
    from sonar_amd import _lib

    nx, ny = 600, 513
    fb, fs, bb, bs = _isolated_case(nx, ny)
    dev = _dev(fb, fs, bb, bs)
    status, src, trg, score, count, guards_ok = _call_mine(*dev, nx, ny, retrieval, ws_short=1)
    assert status == _lib.SMI_ERR_INVALID_ARG and b"smi_xsim_mine_workspace_bytes" in _lib.load().smi_last_error()
    assert guards_ok and count == SENT_I
    assert (src == SENT_I).all() and (trg == SENT_I).all() and (score == SENT_F).all()
    status, src, trg, score, count, guards_ok = _call_mine(*dev, nx, ny, retrieval)
    assert status == 0 and guards_ok and count == len(R.mine(fb, fs, bb, bs, nx, ny, retrieval))


# ------------------------------------------------------------------------------ 5. smi_xsim_pair_scores
_PNX, _PNY, _PM = 300, 257, 1000


@functools.lru_cache(maxsize=None)
def _pair_indices():
    g = torch.Generator().manual_seed(99)
    s = torch.randint(0, _PNX, (_PM,), generator=g)
    t = torch.randint(0, _PNY, (_PM,), generator=g)
    s[:4] = torch.tensor([0, _PNX - 1, 0, _PNX - 1])      # the corners
    t[:4] = torch.tensor([0, 0, _PNY - 1, _PNY - 1])
    bad = {10: (-1, 3), 11: (3, -1), 12: (_PNX, 3), 13: (3, _PNY), 14: (2 ** 40, 0), 15: (0, -2 ** 40)}
    for p, (a, b) in bad.items():
        s[p], t[p] = a, b
    return s, t, sorted(bad)


@functools.lru_cache(maxsize=None)
def _integer_rows(d):
    g = torch.Generator().manual_seed(31 + d)
    return torch.randint(-1, 2, (_PNX, d), generator=g).half(), torch.randint(-1, 2, (_PNY, d), generator=g).half()


def _check_nan_and_strip(out, bad):
    assert torch.isnan(out[bad]).all(), "a pair with an index out of range must score NaN"
    ok = torch.ones(out.shape[0], dtype=torch.bool)
    ok[bad] = False
    assert not torch.isnan(out[ok]).any()
    return ok


@pytest.mark.parametrize("d", [64, 1024])
def test_pair_scores_cosine_exact_on_integer_rows(d):
    """Entries in {-1, 0, 1}: every partial sum is an integer below 2^24, the fp32 dot product is exact in any order."""
    from sonar_amd import mining

    x, y = _integer_rows(d)
    s, t, bad = _pair_indices()
    out = mining.pair_scores(x.cuda(), _PNX, y.cuda(), _PNY, s.cuda(), t.cuda(), None, None, "cosine").cpu()
    ok = _check_nan_and_strip(out, bad)
    want = (x[s[ok]].double() * y[t[ok]].double()).sum(dim=1)
    assert torch.equal(out[ok].double(), want)


@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("d", [64, 1024])
def test_pair_scores_distance_exact_on_dyadic_lists(d, k):
    """Score lists in multiples of 1/8: sums of k of them, / k (a power of two), the half-sum and a - b are all exact."""
    from sonar_amd import mining

    x, y = _integer_rows(d)
    s, t, bad = _pair_indices()
    g = torch.Generator().manual_seed(5 * d + k)
    fs = torch.randint(-8, 9, (_PNX, k), generator=g).float() / 8
    bs = torch.randint(-8, 9, (_PNY, k), generator=g).float() / 8
    out = mining.pair_scores(x.cuda(), _PNX, y.cuda(), _PNY, s.cuda(), t.cuda(), fs.cuda(), bs.cuda(), "distance").cpu()
    ok = _check_nan_and_strip(out, bad)
    want = R.score_pairs(x.numpy(), y.numpy(), s[ok].numpy(), t[ok].numpy(), fs.double().mean(dim=1).numpy(),
                         bs.double().mean(dim=1).numpy(), "distance")
    assert torch.equal(out[ok].double(), torch.from_numpy(want))


@functools.lru_cache(maxsize=None)
def _normalized_case(d):
    """Clustered rows normalised ON THE DEVICE and their k = 4 neighbour lists from the device: the reference takes those
    fp16 rows and fp32 lists as given, so what separates it from the kernel is the kernel's own arithmetic."""
    from sonar_amd import xsim

    g = torch.Generator().manual_seed(700 + d)
    y = torch.randn(_PNY, d, generator=g)
    x = y[torch.randint(0, _PNY, (_PNX,), generator=g)] + 0.5 * torch.randn(_PNX, d, generator=g)
    xn, yn = xsim.normalize_rows(x.cuda()), xsim.normalize_rows(y.cuda())
    fs, _ = xsim.topk_normalized(xn, _PNX, yn, _PNY, 4)
    bs, _ = xsim.topk_normalized(yn, _PNY, xn, _PNX, 4)
    torch.cuda.synchronize()
    return xn, yn, fs, bs


@pytest.mark.parametrize("margin", ["cosine", "ratio"])
@pytest.mark.parametrize("d", [64, 320, 1024])
def test_pair_scores_of_normalized_rows_vs_fp64(d, margin):
    from sonar_amd import mining

    xn, yn, fs, bs = _normalized_case(d)
    s, t, bad = _pair_indices()
    out = mining.pair_scores(xn, _PNX, yn, _PNY, s.cuda(), t.cuda(), fs, bs, margin).cpu()
    ok = _check_nan_and_strip(out, bad)
    xh, yh = xn.cpu().numpy()[:_PNX], yn.cpu().numpy()[:_PNY]
    sn, tn = s[ok].numpy(), t[ok].numpy()
    a = R.score_pairs(xh, yh, sn, tn, None, None, "cosine")
    err = np.abs(out[ok].double().numpy() - a) if margin == "cosine" else None
    tol = np.full_like(a, d * 2.0 ** -23)
    if margin == "ratio":
        x_mean, y_mean = fs.cpu().double().mean(dim=1).numpy(), bs.cpu().double().mean(dim=1).numpy()
        b = (x_mean[sn] + y_mean[tn]) / 2
        assert np.abs(b).min() >= 0.1, np.abs(b).min()          # a condition on the inputs
        want = R.score_pairs(xh, yh, sn, tn, x_mean, y_mean, "ratio")
        err = np.abs(out[ok].double().numpy() - want)
        tol = d * 2.0 ** -23 / np.abs(b) + 4 * 2.0 ** -24 * np.abs(a / b)
    print(f"d = {d}, {margin}: max error {err.max():.2e}, smallest bound {tol.min():.2e}, max error / bound {(err / tol).max():.3f}")
    assert (err <= tol).all()


# --------------------------------------------------------------------------------- 6. the whole path, exact
def _pad256(t):
    out = torch.zeros(((t.shape[0] + 255) // 256 * 256, t.shape[1]), dtype=t.dtype)
    out[:t.shape[0]] = t
    return out


@functools.lru_cache(maxsize=None)
def _whole_case(nx, ny, d, k):
    g = torch.Generator().manual_seed(17 * nx + ny + d)
    x = torch.randint(-1, 2, (nx, d), generator=g).half()
    y = torch.randint(-1, 2, (ny, d), generator=g).half()
    ref = R.pipeline(x.numpy(), y.numpy(), k, "distance")
    return _pad256(x).cuda(), _pad256(y).cuda(), x, y, ref


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("nx,ny,d", [(300, 513, 128), (600, 257, 64)])
def test_whole_path_exact_on_integer_rows(nx, ny, d, k):
    """top-k both ways -> margin select both ways -> search / score / mine, fp16 rows used as they are: every cosine is
    an integer, every mean and every `distance` margin dyadic, so each stage must equal the fp64 reference exactly."""
    from sonar_amd import mining

    xd, yd, x, y, (fwd_best, fwd_score, bwd_best, bwd_score, x_mean, y_mean) = _whole_case(nx, ny, d, k)
    kw = dict(margin="distance", k=k)
    trg, sc = mining.mine_bitexts_normalized(xd, nx, yd, ny, mode="search", **kw)
    assert trg.dtype == torch.int64 and torch.equal(trg.cpu(), torch.from_numpy(fwd_best))
    assert torch.equal(sc.cpu().double(), torch.from_numpy(fwd_score))

    g = torch.Generator().manual_seed(k)
    ps, pt = torch.randint(0, nx, (500,), generator=g), torch.randint(0, ny, (500,), generator=g)
    ps[7], pt[9] = nx, -1
    got = mining.mine_bitexts_normalized(xd, nx, yd, ny, mode="score", pairs=(ps.cuda(), pt.cuda()), **kw).cpu()
    ok = _check_nan_and_strip(got, [7, 9])
    want = R.score_pairs(x.numpy(), y.numpy(), ps[ok].numpy(), pt[ok].numpy(), x_mean, y_mean, "distance")
    assert torch.equal(got[ok].double(), torch.from_numpy(want))

    for retrieval in RETRIEVALS:
        for threshold in (None, 0.0):
            want = R.final_order(R.mine(fwd_best, fwd_score, bwd_best, bwd_score, nx, ny, retrieval, threshold), retrieval)
            got = mining.mine_bitexts_normalized(xd, nx, yd, ny, retrieval=retrieval, threshold=threshold, **kw)
            _assert_pairs(got, want, f"{retrieval}, k = {k}, threshold {threshold}")
            assert threshold is not None or len(want) > 0


# ------------------------------------------------------------------------------------- 7. the real path
_RNX, _RNY, _RD = 1000, 750, 128


@functools.lru_cache(maxsize=None)
def _real_case(margin):
    """synthetic_pairs data (x = a noisy permutation of 1000 unit rows) rounded to fp16, y cut to its first 750 rows: a
    quarter of the x rows has no partner.  Reference: fp64 normalisation of the fp16 values, then the pipeline in fp64."""
    from oracle import xsim as OX

    x, y, _ = OX.synthetic_pairs(_RNX, d=_RD, noise=0.3, seed=5)
    x, y = x.half(), y[:_RNY].half()
    xn = x.double().numpy()
    yn = y.double().numpy()
    xn /= np.linalg.norm(xn, axis=1, keepdims=True)
    yn /= np.linalg.norm(yn, axis=1, keepdims=True)
    return x.cuda(), y.cuda(), R.pipeline(xn, yn, 4, margin)[:4]


@pytest.mark.parametrize("retrieval", RETRIEVALS)
@pytest.mark.parametrize("margin", ["ratio", "distance"])
def test_mine_bitexts_real_path_agrees_with_reference(margin, retrieval):
    """At least 99 % of the reference's pairs present, at most 1 % extra: the allowance
    test_margin_xsim_vs_laser_formula_golden grants for fp16 normalisation moving near-tied neighbours."""
    from sonar_amd import mining

    x, y, (fwd_best, fwd_score, bwd_best, bwd_score) = _real_case(margin)
    want = R.mine(fwd_best, fwd_score, bwd_best, bwd_score, _RNX, _RNY, retrieval)
    src, trg, score = mining.mine_bitexts(x, y, retrieval=retrieval, margin=margin, k=4)
    got = set(zip(src.cpu().tolist(), trg.cpu().tolist()))
    ref = {(p[0], p[1]) for p in want}
    assert len(got) == src.shape[0] and len(ref) == len(want)
    present, extra = len(ref & got) / len(ref), len(got - ref) / len(ref)
    by_pair = {(p[0], p[1]): p[2] for p in want}
    drift = max(abs(v - by_pair[p]) for p, v in zip(zip(src.cpu().tolist(), trg.cpu().tolist()), score.cpu().tolist())
                if p in by_pair)
    print(f"{margin} / {retrieval}: {len(ref)} reference pairs, {present:.2%} present, {extra:.2%} extra, "
          f"max |score - reference| on common pairs {drift:.2e}")
    assert present >= 0.99 and extra <= 0.01
    if retrieval == "max":
        assert (score.cpu().diff() <= 0).all()
