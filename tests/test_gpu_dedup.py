"""GPU: semantic de-duplication (sonar_amd/csrc/ivf.hip ivf_selfjoin_kernel, sonar_amd/dedup.py) against the numpy restatement
in tests/dedup_ref.py.

On operands with entries from {-1, 0, 1} every product and partial sum is a small integer, the fp32 score is exact in any order
and the float64 restatement is the one right answer: max_sim and nearest are compared for equality.  On real-valued rows the
tolerance is the one tests/test_gpu_xsim_kernels.py derives for the fp32 accumulation of normalised fp16 rows, d * 2^-23 per
score; the planted data keeps every decision 400 tolerances away from the threshold (asserted on the CPU,
tests/test_dedup_cpu.py), so `keep` is compared for equality there too.

The host picks the unit size (64 or 128 own rows = slots of a tile) from n and K alone.  `_join` runs every case three ways
-- as called, with the output one row longer than 256 K (units of 128), and with so many empty lists appended that n < 256 K
(units of 64) -- and asserts the same bits: no bit depends on the unit size or on what other lists exist."""
import functools

import numpy as np
import pytest
import torch

from tests import dedup_ref as D
from tests import ivf_ref as R
from tests.test_dedup_cpu import PLANTED, THRESHOLD
from tests.test_gpu_ivf import PATTERNS, _dev, _i32, _labels

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


def _exact_scores(x):
    """All pairs of integer-valued rows: exact in float64 in any order."""
    x64 = x.astype(np.float64)
    s = x64 @ x64.T
    assert np.array_equal(s, np.rint(s)) and np.abs(s).max() < 2 ** 11
    return s


def _join(rows, ids, off, n, priority=None):
    """dedup.self_join at both unit sizes: (max_sim, nearest) as numpy, after asserting that the three calls agree."""
    from sonar_amd import dedup

    k = off.shape[0] - 1
    pd = None if priority is None else _dev(np.asarray(priority, dtype=np.float32))
    got = dedup.self_join(rows, ids, off, n, pd)
    # units of 128: n' >= 256 K, the rows from n on are in no list
    n_big = max(n, 256 * k) + 1
    p_big = None if pd is None else torch.cat([pd, torch.zeros(n_big - n, dtype=torch.float32, device="cuda")])
    big = dedup.self_join(rows, ids, off, n_big, p_big)
    # units of 64: K' > n / 256, the lists from K on are empty
    k_small = max(k, n // 256 + 1) + 1
    off_small = torch.cat([off, off[-1:].expand(k_small - k)]).contiguous()
    small = dedup.self_join(rows, ids, off_small, n, pd)
    torch.cuda.synchronize()
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[0].shape == got[1].shape == (n,)
    assert torch.equal(big[0][:n].view(torch.int32), got[0].view(torch.int32)) and torch.equal(big[1][:n], got[1])
    assert (big[0][n:] == NEG_INF).all() and (big[1][n:] == -1).all()
    assert torch.equal(small[0].view(torch.int32), got[0].view(torch.int32)) and torch.equal(small[1], got[1])
    return got[0].cpu().numpy(), got[1].cpu().numpy()


def _check_exact(x, rows, ids, off, priority, s):
    n = len(x)
    got_s, got_i = _join(rows, ids, off, n, priority)
    want_s, want_i = D.self_join(x, ids.cpu().numpy(), off.cpu().numpy(), n, priority, s=s)
    bad = np.flatnonzero((got_i != want_i) | (got_s.astype(np.float64) != want_s))
    assert len(bad) == 0, (bad[:5], got_i[bad[:5]], want_i[bad[:5]], got_s[bad[:5]], want_s[bad[:5]])
    return got_s, got_i


def _storage(x, labels, k, slot_order=None):
    """The list storage built on the host (tests/ivf_ref.build), the members of a list in ascending id or, with slot_order
    (a permutation of the ids), in that order: full control over which tile a row is in."""
    off, _, ids = R.build(labels, k)
    if slot_order is not None:
        rank = np.empty(len(x), dtype=np.int64)
        rank[np.asarray(slot_order)] = np.arange(len(x))
        for c in range(k):
            seg = ids[off[c]: off[c + 1]]
            m = seg[seg >= 0]
            seg[: len(m)] = m[np.argsort(rank[m])]
    rows = np.where((ids >= 0)[:, None], x[np.maximum(ids, 0)], np.float16(0))
    return _dev(rows.astype(np.float16)), _i32(ids), _i32(off)


# ------------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("d", [64, 192, 1024])
@pytest.mark.parametrize("k", [1, 3, 300])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4099])
def test_integer_operands_equal_the_restatement(n, k, d):
    from sonar_amd import index

    rng = np.random.default_rng(n * 1000003 + k * 1009 + d)
    x = R.integer_rows(rng, n, d)
    if n > 16:
        x[rng.integers(0, n, n // 8)] = x[0]  # exact duplicates: score ties among the candidates
    s = _exact_scores(x)
    xd = _dev(x)
    priorities = (None, rng.standard_normal(n).astype(np.float32), rng.integers(0, 3, n).astype(np.float32))
    for pattern in PATTERNS:
        labels = _labels(rng, pattern, n, k)
        rows, ids, off, _ = index.build_lists(xd, _i32(labels), k)  # the device's own lists
        for priority in priorities:
            _check_exact(x, rows, ids, off, priority, s)


# ------------------------------------------------------------------------------------------------------ 2. edges
def test_list_sizes_across_both_tile_sizes_and_rows_left_out():
    rng = np.random.default_rng(21)
    sizes = [16, 17, 64, 65, 128, 129, 1, 0, 2]
    labels = np.concatenate([np.full(c, l) for l, c in enumerate(sizes)] + [np.full(7, -1), np.full(5, len(sizes))])
    labels = labels[rng.permutation(len(labels))]
    n, k = len(labels), len(sizes)
    x = R.integer_rows(rng, n, 128)
    s = _exact_scores(x)
    for order in (None, rng.permutation(n)):
        rows, ids, off = _storage(x, labels, k, order)
        assert np.diff(off.cpu().numpy()).tolist() == [16, 32, 64, 80, 128, 144, 16, 0, 16]  # all-pad tail blocks of a tile
        for priority in (None, rng.standard_normal(n).astype(np.float32), rng.integers(0, 2, n).astype(np.float32)):
            got_s, got_i = _check_exact(x, rows, ids, off, priority, s)
            out = np.flatnonzero((labels < 0) | (labels >= k))
            assert (got_i[out] == -1).all() and (got_s[out] == NEG_INF).all()  # rows left out of the index
            alone = np.flatnonzero(labels == 6)
            assert got_i[alone].tolist() == [-1] and got_s[alone].tolist() == [NEG_INF]  # a list with one row
            for c in (0, 1, 2, 3, 4, 5, 8):  # the first row of the keep order of every list has no predecessor
                m = np.flatnonzero(labels == c)
                p = np.zeros(n) if priority is None else priority
                top = m[np.lexsort((m, -p[m]))[0]]
                assert got_i[top] == -1 and got_s[top] == NEG_INF
                assert (got_i[np.setdiff1d(m, [top])] >= 0).all()


def test_exact_duplicates_drop_the_later_id():
    rng = np.random.default_rng(22)
    n = 200
    x = R.integer_rows(rng, n, 64)
    x[150], x[31], x[199] = x[30], x[30], x[30]
    labels = np.arange(n) % 2
    labels[[30, 31, 150, 199]] = 1
    self_score = float((x[30].astype(np.float64) ** 2).sum())
    assert (_exact_scores(x)[30, np.setdiff1d(np.arange(n), [30, 31, 150, 199])] < self_score).all()
    rows, ids, off = _storage(x, labels, 2, rng.permutation(n))
    got_s, got_i = _check_exact(x, rows, ids, off, None, _exact_scores(x))
    assert got_i[[31, 150, 199]].tolist() == [30, 30, 30] and (got_s[[31, 150, 199]] == self_score).all()
    assert got_s[30] < self_score
    keep = D.keep_mask(got_s, self_score - 0.5)
    assert keep[30] and not keep[[31, 150, 199]].any()  # the earlier id is kept, the later ones are dropped
    p = np.zeros(n, dtype=np.float32)
    p[150] = 1.0  # a priority turns it round: row 150 precedes its copies and is kept
    got_s, got_i = _check_exact(x, rows, ids, off, p, _exact_scores(x))
    # rows 31 and 199 come after 150 AND 30, which tie: the lower id is reported
    assert got_i[[30, 31, 199]].tolist() == [150, 30, 30] and (got_s[[30, 31, 199]] == self_score).all()
    assert got_s[150] < self_score


def test_nine_nearer_rows_follow_and_a_farther_one_precedes():
    """What a top-8 search cannot answer: the 9 nearest neighbours of row 10 all come after it."""
    from sonar_amd import index

    rng = np.random.default_rng(23)
    n, d = 40, 64
    x = np.zeros((n, d), dtype=np.float16)
    x[np.arange(n), np.arange(n)] = 1  # far from everything: score 0 or 1 against row 10
    x[10, :32] = 1
    for j in range(11, 20):  # nine rows at score 31 that follow row 10
        x[j] = x[10]
        x[j, j] = 0
    x[2, :20], x[2, 20:32] = 1, 0  # the one preceding row that is near: score 20
    labels = np.zeros(n, dtype=np.int64)
    s = _exact_scores(x)
    rows, ids, off = _storage(x, labels, 1, rng.permutation(n))
    got_s, got_i = _check_exact(x, rows, ids, off, None, s)
    assert got_i[10] == 2 and got_s[10] == 20
    score, idx = index.search_lists(_dev(x[10:11]), _i32([[0]]), rows, ids, off, 8)
    assert sorted(idx[0].tolist()) == [10, 11, 12, 13, 14, 15, 16, 17] and (score[0] >= 31).all()  # row 2 is not among them


def test_score_ties_between_preceding_rows_in_different_tiles():
    rng = np.random.default_rng(24)
    n, d = 300, 64
    x = R.integer_rows(rng, n, d)
    x[299] = 0
    x[299, :40] = 1
    copies = [3, 70, 140, 210, 280]
    for j in copies:  # equal rows: equal scores against row 299, and the best ones
        x[j] = 0
        x[j, :40] = 1
    labels = np.zeros(n, dtype=np.int64)
    s = _exact_scores(x)
    assert (s[299, np.setdiff1d(np.arange(299), copies)] < 40).all()
    # slot order: id 280 in the first tile of the walk, id 3 in the last, the others between, at either tile size
    rest = np.setdiff1d(np.arange(n), copies + [299])
    order = np.concatenate([[280], rest[:100], [210], rest[100:200], [140, 299], rest[200:], [70, 3]])
    assert sorted(order.tolist()) == list(range(n))
    rows, ids, off = _storage(x, labels, 1, order)
    got_s, got_i = _check_exact(x, rows, ids, off, None, s)
    assert got_i[299] == 3 and got_s[299] == 40  # the lower id wins, wherever it is met
    p = np.zeros(n, dtype=np.float32)
    p[[70, 210, 299]] = [2.0, 2.0, 1.0]  # only 70 and 210 precede row 299 now
    got_s, got_i = _check_exact(x, rows, ids, off, p, s)
    assert got_i[299] == 70 and got_s[299] == 40


# ------------------------------------------------------------------------------------------------------ 3. unit sizes
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("short", [0, 1])
def test_both_unit_sizes_at_the_threshold(k, short):
    """n = 256 K runs units of 128 own rows, n = 256 K - 1 units of 64 (csrc/ivf.hip, unit_pairs); `_join` forces the other
    size on the same data and compares the bits."""
    from sonar_amd import index

    n = 256 * k - short
    rng = np.random.default_rng(n)
    x = R.integer_rows(rng, n, 192)
    labels = rng.integers(0, k, n)
    labels[:5] = -1
    rows, ids, off, _ = index.build_lists(_dev(x), _i32(labels), k)
    s = _exact_scores(x)
    for priority in (None, rng.integers(0, 4, n).astype(np.float32)):
        _check_exact(x, rows, ids, off, priority, s)


# ------------------------------------------------------------------------------------------------------ 4. invariance
def test_bits_do_not_depend_on_run_order_company_and_equal_the_search_score():
    from sonar_amd import dedup, index, xsim

    rng = np.random.default_rng(41)
    n, d, k = 512, 1024, 3
    x = R.normalize64(rng.standard_normal((n, d)) + 2.0 * rng.standard_normal((1, d))).astype(np.float16)  # cosines ~ 0.8
    labels = rng.integers(0, k, n)
    labels[rng.random(n) < 0.1] = -1
    priority = rng.integers(0, 5, n).astype(np.float32)
    xn = xsim.normalize_rows(_dev(x))
    rows, ids, off, _ = index.build_lists(xn, _i32(labels), k)
    pd = _dev(priority)
    ms, nn = dedup.self_join(rows, ids, off, n, pd)
    again = dedup.self_join(rows, ids, off, n, pd)
    assert torch.equal(ms.view(torch.int32), again[0].view(torch.int32)) and torch.equal(nn, again[1])  # two runs
    _join(rows, ids, off, n, priority)  # both unit sizes, other (empty) lists
    # the corpus in another order, ids and priorities mapped through it: other slots, other tiles, the same bits
    perm = rng.permutation(n)  # new row r is old row perm[r]
    # precedence among equal priorities is by id, which the permutation changes: first a unique priority per row that
    # reproduces the keep order of the old corpus
    order_key = np.lexsort((np.arange(n), -priority))  # the keep order of the old corpus
    rank = np.empty(n, dtype=np.float32)
    rank[order_key] = -np.arange(n, dtype=np.float32)
    base = dedup.self_join(rows, ids, off, n, _dev(rank))
    assert torch.equal(base[0].view(torch.int32), ms.view(torch.int32)) and torch.equal(base[1], nn)  # the same order
    rows2, ids2, off2, _ = index.build_lists(xn[_dev(perm)].contiguous(), _i32(labels[perm]), k)
    ms2, nn2 = dedup.self_join(rows2, ids2, off2, n, _dev(rank[perm]))
    got_nn2 = nn2.cpu().numpy()
    assert torch.equal(ms2.view(torch.int32), ms[_dev(perm)].view(torch.int32))
    assert np.array_equal(np.where(got_nn2 >= 0, perm[np.maximum(got_nn2, 0)], -1), nn.cpu().numpy()[perm])
    # whatever other lists exist: list 1 alone
    only = np.where(labels == 1, 0, -1)
    rows3, ids3, off3, _ = index.build_lists(xn, _i32(only), 1)
    ms3, nn3 = dedup.self_join(rows3, ids3, off3, n, pd)
    in1 = _dev(labels == 1)
    assert torch.equal(ms3[in1].view(torch.int32), ms[in1].view(torch.int32)) and torch.equal(nn3[in1], nn[in1])
    assert (nn3[~in1] == -1).all() and (ms3[~in1] == NEG_INF).all()
    # max_sim[i] is the score the flat scan gives the pair (i, nearest[i]): every row in a list of its own, probed by i
    prows, pids, poff, _ = index.build_lists(xn, torch.arange(n, dtype=torch.int32, device="cuda"), n)
    have = nn >= 0
    probes = torch.where(have, nn, torch.full_like(nn, -1)).reshape(n, 1).contiguous()
    score, idx = index.search_lists(xn, probes, prows, pids, poff, 1)
    assert int(have.sum()) > n // 2 and torch.equal(idx[:, 0], nn)
    assert torch.equal(score[:, 0].view(torch.int32), ms.view(torch.int32))
    # and the score of (i, j) has the bits of the score of (j, i)
    back = torch.where(have, torch.arange(n, dtype=torch.int32, device="cuda"), torch.full_like(nn, -1))
    src = torch.where(have, nn, torch.zeros_like(nn)).long()
    score_t, _ = index.search_lists(xn[src].contiguous(), back.reshape(n, 1).contiguous(), prows, pids, poff, 1)
    assert torch.equal(score_t[:, 0].view(torch.int32), ms.view(torch.int32))


# ------------------------------------------------------------------------------------------------------ 5. real-valued
@functools.lru_cache(maxsize=None)
def _planted():
    """(x fp16, labels, group, xd on the device, xn64 = the engine's normalised rows in float64, s64 = their products)."""
    from sonar_amd import xsim

    x, labels, group = D.planted_groups(**PLANTED)
    xd = _dev(x)
    xn64 = xsim.normalize_rows(xd)[: len(x)].cpu().numpy().astype(np.float64)
    s64 = xn64 @ xn64.T
    for a in (x, group, xn64, s64):  # shared among the tests: left unchanged
        a.setflags(write=False)
    return x, labels, group, xd, xn64, s64


def _check_real(got_s, got_i, want_s, want_i, s64, labels, priority, d):
    """Decision by decision, on the device's own scores: every max_sim within d 2^-23 of float64, nearest precedes the row and
    is within twice that of the float64 best."""
    tol = d * 2.0 ** -23
    n = len(got_s)
    p = np.zeros(n) if priority is None else np.asarray(priority, dtype=np.float64)
    assert np.array_equal(got_i < 0, want_i < 0) and (got_s[got_i < 0] == NEG_INF).all()
    have = np.flatnonzero(got_i >= 0)
    j = got_i[have]
    assert np.array_equal(labels[j], labels[have])
    assert ((p[j] > p[have]) | ((p[j] == p[have]) & (j < have))).all()  # nearest precedes the row
    assert np.abs(got_s[have] - s64[have, j]).max() <= tol
    assert np.abs(got_s[have] - want_s[have]).max() <= tol
    assert (s64[have, j] >= want_s[have] - 2 * tol).all()


def test_planted_near_duplicates_decision_by_decision():
    from sonar_amd.index import IVFFlatIndex

    x, labels, group, xd, xn64, s64 = _planted()
    n, d, k = len(x), x.shape[1], PLANTED["k"]
    ix = IVFFlatIndex(xd[:k]).add(xd, labels=_i32(labels))
    ids, off = ix._ids.cpu().numpy(), ix.list_offsets.cpu().numpy()
    rng = np.random.default_rng(51)
    for priority in (None, rng.standard_normal(n).astype(np.float32)):
        ms, nn = ix.self_join(None if priority is None else _dev(priority), n=n)
        got_s, got_i = ms.cpu().numpy(), nn.cpu().numpy()
        want_s, want_i = D.self_join(xn64, ids, off, n, priority, s=s64)
        _check_real(got_s, got_i, want_s, want_i, s64, labels, priority, d)
        keep = D.keep_mask(got_s, THRESHOLD)
        assert np.array_equal(keep, D.keep_mask(want_s, THRESHOLD))  # the CPU-asserted gap: no decision near the threshold
        assert keep.sum() == PLANTED["n_groups"] and (np.bincount(group[keep]) == 1).all()  # exactly one row per group
        if priority is None:
            first = np.array([np.flatnonzero(group == g)[0] for g in range(PLANTED["n_groups"])])
            assert keep[first].all()


# ------------------------------------------------------------------------------------------------------ 6. semdedup
def _engine_priority(ix, xd, mode):
    from sonar_amd import xsim

    n = xd.shape[0]
    score = xsim.topk_normalized(xsim.normalize_rows(xd), n, ix._c16, ix.n_lists, 1)[0][:, 0]
    return (score if mode == "centroid" else -score).cpu().numpy()


def test_semdedup_end_to_end():
    from sonar_amd import dedup
    from sonar_amd.index import IVFFlatIndex

    x, _, group, xd, xn64, s64 = _planted()
    n, d = x.shape
    rng = np.random.default_rng(61)
    tensor_priority = rng.integers(0, 7, n).astype(np.float32)
    ix = IVFFlatIndex.train(xd, 8, n_iter=3, seed=1).add(xd)
    ids, off = ix._ids.cpu().numpy(), ix.list_offsets.cpu().numpy()
    labels = np.full(n, -1, dtype=np.int64)
    for c, m in enumerate(D.members_of(ids, off)):
        labels[m] = c
    assert (labels >= 0).all()
    for priority in (None, "centroid", "-centroid", tensor_priority):
        given = _dev(priority) if isinstance(priority, np.ndarray) else priority
        res = dedup.semdedup(xd, index=ix, threshold=THRESHOLD, priority=given)
        assert res.keep.dtype == torch.bool and np.array_equal(res.labels.cpu().numpy(), labels)
        p = _engine_priority(ix, xd, priority) if isinstance(priority, str) else priority
        got_s, got_i = res.max_sim.cpu().numpy(), res.nearest.cpu().numpy()
        want_s, want_i = D.self_join(xn64, ids, off, n, p, s=s64)
        _check_real(got_s, got_i, want_s, want_i, s64, labels, p, d)
        keep = res.keep.cpu().numpy()
        assert np.array_equal(keep, D.keep_mask(want_s, THRESHOLD))
        # a group the quantiser kept in one list loses all rows but one
        whole = np.array([len(set(labels[group == g])) == 1 for g in range(PLANTED["n_groups"])])
        assert whole.mean() > 0.9 and (np.bincount(group[keep], minlength=len(whole))[whole] == 1).all()
        for thr in (0.5, 0.99, 0.995):  # keep_at = a fresh call at that threshold
            fresh = dedup.semdedup(xd, index=ix, eps=1 - thr, priority=given)
            assert torch.equal(res.keep_at(1.0 - (1 - thr)), fresh.keep)
            assert torch.equal(fresh.max_sim.view(torch.int32), res.max_sim.view(torch.int32))
    # trains and fills an index of its own
    own = dedup.semdedup(xd, n_lists=8, threshold=THRESHOLD, priority="centroid", n_iter=3, seed=1)
    assert torch.equal(own.labels, res.labels)  # the same seed: the same quantiser
    ref = dedup.semdedup(xd, index=ix, threshold=THRESHOLD, priority="centroid")
    assert torch.equal(own.keep, ref.keep) and torch.equal(own.max_sim.view(torch.int32), ref.max_sim.view(torch.int32))
    assert torch.equal(own.nearest, ref.nearest)


def test_semdedup_is_capturable():
    from sonar_amd import dedup
    from sonar_amd.index import IVFFlatIndex

    x, labels, _, xd, _, _ = _planted()
    ix = IVFFlatIndex(xd[: PLANTED["k"]]).add(xd, labels=_i32(labels))
    want = dedup.semdedup(xd, index=ix, threshold=THRESHOLD, priority="centroid")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm up off the default stream, as torch's capture asks
        dedup.semdedup(xd, index=ix, threshold=THRESHOLD, priority="centroid")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = dedup.semdedup(xd, index=ix, threshold=THRESHOLD, priority="centroid")
    for _ in range(2):
        for t in got:
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got.max_sim.view(torch.int32), want.max_sim.view(torch.int32))
        assert torch.equal(got.nearest, want.nearest) and torch.equal(got.keep, want.keep)
        assert torch.equal(got.labels, want.labels)


# ------------------------------------------------------------------------------------------------------ 7. refusals
def test_c_level_refusals_launch_nothing():
    from sonar_amd import _lib

    lib = _lib.load()
    torch.cuda.synchronize()
    cases = D.refusal_cases(lib)  # every call is refused on its arguments: no pointer is dereferenced
    assert all(rc != 0 for rc in cases.values()), {k: v for k, v in cases.items() if v == 0}
    assert lib.smi_last_error()
    torch.cuda.synchronize()
    assert lib.smi_ivf_dedup_workspace_bytes(160, 100, 7, 96) == 0
