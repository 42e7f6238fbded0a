"""GPU: the IVF-Flat index (sonar_amd/csrc/ivf.hip, sonar_amd/index.py) against the numpy restatement in tests/ivf_ref.py.

The build is a permutation of rows, so it is compared for equality of bits.  The search is compared for equality of scores
AND ids on operands with entries from {-1, 0, 1}: every product and partial sum is a small integer, the fp32 score is exact in
any order and the float64 restatement is the one right answer.  On real-valued rows the tolerance is the one
tests/test_gpu_xsim_kernels.py derives for the fp32 accumulation of normalised fp16 rows, d * 2^-23 per score, so a row the
engine left out may beat the k-th returned one by at most twice that in float64 -- a condition on every row.  On planted
data the margins are asserted on the CPU (tests/test_ivf_cpu.py) to be orders of magnitude above it, so there the planted
neighbour itself must come first."""
import functools

import numpy as np
import pytest
import torch

from tests import ivf_ref as R

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
A = R.ALIGN


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i32(a):
    return _dev(np.asarray(a, dtype=np.int32))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy() if t.dtype == torch.float16 else t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------ 1. build
PATTERNS = ("random", "sorted", "reversed", "one", "empty lists", "skipped")


def _labels(rng, pattern, n, k):
    lab = rng.integers(0, k, n).astype(np.int64)
    if pattern == "sorted":
        lab.sort()
    elif pattern == "reversed":
        lab = np.sort(lab)[::-1].copy()
    elif pattern == "one":
        lab[:] = k - 1
    elif pattern == "empty lists":  # only every third list takes rows; with K = 1 no list does
        lab = np.where(lab % 3 == 1, lab, -1) if k == 1 else lab // 3 * 3
    elif pattern == "skipped":
        bad = rng.choice(np.array([-1, k, INT32_MAX]), n)
        lab = np.where(rng.random(n) < 0.3, bad, lab)
    return lab.astype(np.int32)


def _check_build(x16, labels, k):
    from sonar_amd import _lib, index

    n, d = x16.shape
    rows, ids, off, sizes = index.build_lists(_dev(x16), _i32(labels), k)
    torch.cuda.synchronize()
    rows, ids, off, sizes = _bits(rows), ids.cpu().numpy(), off.cpu().numpy(), sizes.cpu().numpy()
    r_off, r_sizes, r_ids = R.build(labels, k)
    assert len(ids) == _lib.load().smi_ivf_slots_bound(n, k) >= r_off[k]
    ok = (labels >= 0) & (labels < k)
    assert np.array_equal(sizes, np.bincount(labels[ok], minlength=k)) and np.array_equal(sizes, r_sizes)
    assert np.array_equal(off, r_off) and (off % A == 0).all()
    total = int(off[k])
    for c in range(k):
        seg, want = ids[off[c]: off[c + 1]], r_ids[r_off[c]: r_off[c + 1]]
        assert np.array_equal(np.sort(seg), np.sort(want)), c  # the members in any order, and the -1 of the pad slots
    real = ids[:total][ids[:total] >= 0]
    assert len(np.unique(real)) == len(real) == int(ok.sum())
    assert (ids[total:] == -1).all()
    want_rows = np.where((ids[:total] >= 0)[:, None], x16.view(np.int16)[np.maximum(ids[:total], 0)], 0)
    assert np.array_equal(rows[:total], want_rows)  # every slot its row, bit for bit; pad slots all-zero bits
    return off, sizes, ids


# k = 255 .. 513 (at n = 4099 only): a thread of the one-block scan (csrc/bucket.hpp) owns ceil(k / 256) lists -- one at 256,
# two at 257 with half the threads owning none, three at 513
BUILD_CASES = [(n, k) for n in (1, A - 1, A, A + 1, 4099) for k in (1, 3, 300)] + [(4099, k) for k in (255, 256, 257, 513)]


@pytest.mark.parametrize("d", [64, 192, 1024])
@pytest.mark.parametrize("n,k", BUILD_CASES)
def test_build_is_the_exact_list_layout(n, k, d):
    rng = np.random.default_rng(n * 1000003 + k * 1009 + d)
    x = rng.standard_normal((n, d)).astype(np.float16)
    x[0, :2] = [-0.0, 65504.0]  # bits travel, not values
    for pattern in PATTERNS:
        _check_build(x, _labels(rng, pattern, n, k), k)


# ------------------------------------------------------------------------------------------------------ 2. search, exact
def _check_search(x, labels, k_lists, q, probes, ks, storage=None):
    """Scores and ids of every row equal the restatement, for every k of ks.  x / q: integer-valued fp16."""
    from sonar_amd import index

    storage = storage or index.build_lists(_dev(x), _i32(labels), k_lists)
    rows, ids, off, _ = storage
    s64 = R.scores64(q, x)
    assert np.abs(s64).max() < 2 ** 11 and np.array_equal(s64, np.rint(s64))
    qd, pd = _dev(q), _i32(probes)
    for k in ks:
        score, idx = index.search_lists(qd, pd, rows, ids, off, k)
        torch.cuda.synchronize()
        want_s, want_i = R.search(q, x, labels, k_lists, probes, k, s=s64)
        got_s, got_i = score.cpu().numpy(), idx.cpu().numpy()
        assert got_s.dtype == np.float32 and got_i.dtype == np.int32 and got_s.shape == got_i.shape == (len(q), k)
        bad = np.flatnonzero((got_i != want_i).any(axis=1) | (got_s.astype(np.float64) != want_s).any(axis=1))
        assert len(bad) == 0, (k, bad[:5], got_i[bad[:2]], want_i[bad[:2]], got_s[bad[:2]], want_s[bad[:2]])
    return storage


def _distinct_probes(rng, nq, k_lists, nprobe):
    return np.stack([rng.permutation(k_lists)[:nprobe] for _ in range(nq)])


def test_search_one_row_one_list():
    rng = np.random.default_rng(1)
    x, q = R.integer_rows(rng, 1, 64), R.integer_rows(rng, 1, 64)
    _check_search(x, [0], 1, q, [[0]], (1, 8))


def test_search_every_k_and_nprobe():
    rng = np.random.default_rng(2)
    x, q = R.integer_rows(rng, 300, 128), R.integer_rows(rng, 65, 128)
    labels = rng.integers(0, 3, 300)
    storage = None
    for nprobe in (1, 2, 3):
        storage = _check_search(x, labels, 3, q, _distinct_probes(rng, 65, 3, nprobe), range(1, 9), storage)


def test_search_one_long_list_many_tiles_several_query_blocks():
    rng = np.random.default_rng(3)
    x, q = R.integer_rows(rng, 4099, 64), R.integer_rows(rng, 257, 64)
    _check_search(x, np.zeros(4099, dtype=np.int64), 1, q, np.zeros((257, 1), dtype=np.int64), (1, 4, 8))


# the list count also walks the boundaries of the inversion's one-block scan (csrc/bucket.hpp): a thread owns ceil(K / 256)
# lists -- one at 256, two at 257 with half the threads owning none, three at 513 -- in the pair offsets and the unit offsets
@pytest.mark.parametrize("k_lists", [300, 255, 256, 257, 513])
def test_search_lists_shorter_than_k_and_empty_lists(k_lists):
    rng = np.random.default_rng(4)
    x, q = R.integer_rows(rng, 4099, 64), R.integer_rows(rng, 300, 64)
    labels = rng.integers(0, k_lists, 4099)
    labels[labels % 5 == 0] += 1  # every fifth list stays empty (at 256 lists the rows of list 255 get no list at all)
    labels[:40] = np.arange(40) % 2 * 2 + 1  # two larger lists; most of the others hold ~17 rows, some fewer than 8
    probes = _distinct_probes(rng, 300, k_lists, 8)
    probes[:5] = np.arange(0, 40, 5).reshape(1, 8)  # rows that probe empty lists only: k x (-inf, -1)
    probes[5, :] = [0, 5, 10, 15, 20, 25, 30, 7]    # one short list among empty ones: a (-inf, -1) tail
    _check_search(x, labels, k_lists, q, probes, (8,))
    few = np.where(np.arange(4099) < 20, np.arange(4099) % 10, -1)  # lists of 2 rows, the others empty, most rows left out
    _check_search(x, few, k_lists, q, rng.integers(0, 12, (300, 8)), (8, 3))  # repeated lists in a row: rows returned twice


def test_search_d1024_nprobe4_k5():
    rng = np.random.default_rng(5)
    x, q = R.integer_rows(rng, 2000, 1024), R.integer_rows(rng, 130, 1024)
    _check_search(x, rng.integers(0, 16, 2000), 16, q, _distinct_probes(rng, 130, 16, 4), (5,))


def test_search_every_query_probes_the_same_list():
    rng = np.random.default_rng(6)
    x, q = R.integer_rows(rng, 1000, 64), R.integer_rows(rng, 200, 64)
    labels = rng.integers(0, 7, 1000)
    storage = _check_search(x, labels, 7, q, np.full((200, 1), 4), (1, 8))
    _check_search(x, labels, 7, q, np.tile([[4, 2, 6]], (200, 1)), (4,), storage)


def test_search_probe_entries_that_name_no_list():
    rng = np.random.default_rng(7)
    x, q = R.integer_rows(rng, 500, 64), R.integer_rows(rng, 70, 64)
    labels = rng.integers(0, 6, 500)
    probes = _distinct_probes(rng, 70, 6, 4)
    probes[rng.random(probes.shape) < 0.4] = -1
    probes[0], probes[69], probes[3, 1], probes[4, 0] = -1, -1, 6, INT32_MAX
    _check_search(x, labels, 6, q, probes, (1, 3, 8))
    _check_search(x, labels, 6, q, np.full((70, 2), -1), (2,))  # no pair at all: the scan has no unit


@pytest.mark.parametrize("nq", [66, 400])  # 3 nq pairs over 4 lists: units of 64 pairs, units of 128
def test_search_planted_ties_across_lists_and_tiles(nq):
    rng = np.random.default_rng(8)
    n, k_lists = 700, 4
    x, q = R.integer_rows(rng, n, 64), R.integer_rows(rng, nq, 64)
    q[0] = 0  # every candidate ties at 0: the lowest ids of the probed lists
    labels = rng.integers(1, k_lists, n)
    labels[np.arange(0, n, 3)] = 0  # list 0: 234 rows = 4 tiles of 64 slots, 2 of 128
    copies = {3: 0, 300: 0, 699: 0, 50: 1, 333: 1, 598: 2, 20: 3}  # id -> list: q[1] copied into different lists and tiles
    for i, c in copies.items():
        x[i], labels[i] = q[1], c
    probes = np.tile([[2, 0, 1]], (nq, 1))
    probes[2:] = _distinct_probes(rng, nq - 2, k_lists, 3)
    _check_search(x, labels, k_lists, q, probes, (1, 4, 6, 8))
    s, i = R.search(q[:2], x, labels, k_lists, probes[:2], 8)
    assert i[0].tolist() == sorted(np.flatnonzero(labels != 3)[:8].tolist()) and (s[0] == 0).all()
    assert i[1][:6].tolist() == [3, 50, 300, 333, 598, 699] and len(set(s[1][:6].tolist())) == 1 and s[1][6] < s[1][5]


def test_search_a_tile_that_holds_one_valid_row():
    rng = np.random.default_rng(9)
    x, q = R.integer_rows(rng, A + 1, 64), R.integer_rows(rng, 5, 64)
    _check_search(x, np.zeros(A + 1, dtype=np.int64), 1, q, np.zeros((5, 1), dtype=np.int64), (1, 8))
    x, q = R.integer_rows(rng, 65, 64), R.integer_rows(rng, 5, 64)  # one row in the second 64-slot tile
    _check_search(x, np.zeros(65, dtype=np.int64), 1, q, np.zeros((5, 1), dtype=np.int64), (2, 8))


@pytest.mark.parametrize("nq", [255, 256, 257])
def test_search_at_the_threshold_between_the_two_unit_sizes(nq):
    """A unit is 128 pairs x 128-slot tiles from nq * nprobe >= 256 K on, 64 x 64 below (csrc/ivf.hip, unit_pairs)."""
    rng = np.random.default_rng(nq)
    x, q = R.integer_rows(rng, 300, 128), R.integer_rows(rng, nq, 128)
    labels = np.zeros(300, dtype=np.int64)  # one list of 295 rows: a third 128-slot tile with 39 of them
    labels[[7, 100, 101, 250, 299]] = [-1, 1, 2, INT32_MAX, -1]
    _check_search(x, labels, 1, q, np.zeros((nq, 1), dtype=np.int64), (1, 8))


@pytest.mark.parametrize("nq", [70, 256])  # units of 64 pairs (two of them), units of 128
def test_search_every_key_list_length_at_both_unit_sizes(nq):
    """Every instantiation <KT, B> of the scan: k = 1, 2, 3, 8 are the key lists of 1, 2, 4 and 8 entries.  One list of
    130 rows is two tiles at B = 128 and three at B = 64, the last one partial; d = 192 is three K slices."""
    rng = np.random.default_rng(1200 + nq)
    x, q = R.integer_rows(rng, 130, 192), R.integer_rows(rng, nq, 192)
    _check_search(x, np.zeros(130, dtype=np.int64), 1, q, np.zeros((nq, 1), dtype=np.int64), (1, 2, 3, 8))


def test_search_units_of_128_pairs_d1024():
    rng = np.random.default_rng(11)
    x, q = R.integer_rows(rng, 600, 1024), R.integer_rows(rng, 300, 1024)
    labels = rng.integers(0, 3, 600)
    labels[labels == 2] = -1  # two lists of ~200 rows, probed by every query: units of 128, 128 and 44 pairs each
    labels[:A + 1] = 1
    probes = np.stack([rng.permutation(2) for _ in range(300)])
    probes[::7, 1] = -1
    storage = _check_search(x, labels, 2, q, probes, (5,))
    short = np.where(np.arange(600) < 6, np.arange(600) % 2, -1)  # lists of 3 rows: (-inf, -1) tails in the large unit
    _check_search(x, short, 2, q, probes, (4,))
    del storage


# ------------------------------------------------------------------------------------------ 3. equals brute force
def _pow4_rows(rng, n, d):
    """Rows whose normalisation is exact: d / 4 entries of +-1 (a power of 4 of them), so the unit row has entries
    +-2^-m and every score is an integer multiple of 4^-m, exact in fp32 in any order."""
    nnz = d // 4
    assert round(np.log2(nnz)) % 2 == 0
    x = np.zeros((n, d), dtype=np.float16)
    for r in range(n):
        x[r, rng.permutation(d)[:nnz]] = rng.choice([-1.0, 1.0], nnz)
    return x


@pytest.mark.parametrize("d", [64, 1024])
@pytest.mark.parametrize("k_lists", [1, 8])
def test_every_list_probed_equals_brute_force(k_lists, d):
    from sonar_amd import xsim
    from sonar_amd.index import IVFFlatIndex

    rng = np.random.default_rng(10 + k_lists + d)
    n, nq, k = 1000, 257, 4
    x, q, cent = _dev(_pow4_rows(rng, n, d)), _dev(_pow4_rows(rng, nq, d)), _dev(_pow4_rows(rng, k_lists, d))
    x[5], x[900] = q[0], q[0]  # exact duplicates: ties at the top
    ix = IVFFlatIndex(cent).add(x)
    assert ix.n_lists == k_lists and ix.ntotal == n and int(ix.list_sizes.sum()) == n
    score, idx = ix.search(q, k=k, nprobe=k_lists)
    xn, qn = xsim.normalize_rows(x), xsim.normalize_rows(q)
    bf_score, bf_idx = xsim.topk_normalized(qn, nq, xn, n, k)
    assert torch.equal(idx, bf_idx) and torch.equal(score, bf_score)
    assert idx[0, :2].tolist() == [5, 900] and score[0, 0].item() == 1.0
    bwd, _ = xsim.topk_normalized(xn, n, qn, nq, k)
    for margin in ("ratio", "distance"):
        got, want = xsim.margin_select(score, idx, bwd, margin), xsim.margin_select(bf_score, bf_idx, bwd, margin)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ------------------------------------------------------------------------------------------ 4. real-valued data
@functools.lru_cache(maxsize=None)
def _planted_index(d):
    """n 4096, K 16: (index over a quantiser fitted on the planted rows, x, q, target, labels of the rows)."""
    from sonar_amd.clustering import SphericalKMeans
    from sonar_amd.index import IVFFlatIndex

    x, truth, _, q, target = R.planted(4096, 16, d, 257)
    xd = _dev(x)
    km = SphericalKMeans(16, n_iter=2).fit(xd, init=xd[:16])
    ix = IVFFlatIndex(km).add(xd)
    torch.cuda.synchronize()
    assert np.array_equal(km.labels.cpu().numpy(), truth)
    return ix, x, q, target, truth


@pytest.mark.parametrize("nprobe", [1, 3])
@pytest.mark.parametrize("d", [64, 1024])
def test_real_valued_rows_decision_by_decision(d, nprobe):
    from sonar_amd import xsim

    ix, x, q, target, labels = _planted_index(d)
    k, tol = 4, d * 2.0 ** -23
    xd, qd = _dev(x), _dev(q)
    probes = ix.probe(qd, nprobe)
    score, idx = ix.search(qd, k=k, nprobe=nprobe)
    torch.cuda.synchronize()
    s, i, probes = score.cpu().numpy(), idx.cpu().numpy().astype(np.int64), probes.cpu().numpy()
    xn = xsim.normalize_rows(xd)[: len(x)].cpu().numpy().astype(np.float64)
    qn = xsim.normalize_rows(qd)[: len(q)].cpu().numpy().astype(np.float64)
    s64 = qn @ xn.T
    assert (i >= 0).all() and (i < len(x)).all()
    for r in range(len(q)):
        assert (labels[i[r]][:, None] == probes[r][None, :]).any(axis=1).all(), r  # every id lies in a probed list
        assert len(set(i[r].tolist())) == k, r
        assert np.abs(s[r] - s64[r, i[r]]).max() <= tol, (r, s[r], s64[r, i[r]])
        for j in range(k - 1):  # the total order on the engine's own scores
            assert s[r, j] > s[r, j + 1] or (s[r, j] == s[r, j + 1] and i[r, j] < i[r, j + 1]), (r, j)
        left = np.isin(labels, probes[r])
        left[i[r]] = False
        assert s64[r, left].max() <= s64[r, i[r, k - 1]] + 2 * tol, r
    assert np.array_equal(i[:, 0], target)  # the planted neighbour, found at nprobe = 1 already
    if nprobe == 1:
        assert np.array_equal(probes[:, 0], labels[target])


# ------------------------------------------------------------------------------------------ 5. company and layout
@pytest.mark.parametrize("d", [64, 1024])
def test_bits_do_not_depend_on_company_or_layout(d):
    from sonar_amd.index import IVFFlatIndex

    ix, x, q, _, labels = _planted_index(d)
    rng = np.random.default_rng(d)
    k, nq = 4, len(q)
    assert nq == 257
    xd, qd = _dev(x), _dev(q)
    probes = _i32(_distinct_probes(rng, nq, 16, 3))
    score, idx = ix.search(qd, k=k, probes=probes)
    again = ix.search(qd, k=k, probes=probes)
    assert torch.equal(score, again[0]) and torch.equal(idx, again[1])  # two runs
    for r in (0, 1, 63, 64, 65, 128, 255, 256):  # alone
        one = ix.search(qd[r: r + 1], k=k, probes=probes[r: r + 1])
        assert torch.equal(one[0][0], score[r]) and torch.equal(one[1][0], idx[r]), r
    perm = torch.from_numpy(rng.permutation(nq)).cuda()  # the queries in another order
    ps, pi = ix.search(qd[perm], k=k, probes=probes[perm])
    assert torch.equal(ps, score[perm]) and torch.equal(pi, idx[perm])
    # the corpus in another order, the lists given: other slots, other arrival order, other ids -- the same rows and bits
    cperm = rng.permutation(len(x))
    ix2 = IVFFlatIndex(ix.centroids_normalized).add(xd[_dev(cperm)], labels=_i32(labels[cperm]))
    s2, i2 = ix2.search(qd, k=k, probes=probes)
    assert torch.equal(s2, score) and np.array_equal(cperm[i2.cpu().numpy()], idx.cpu().numpy())
    # every row in ONE list: 257 pairs on one list run as units of 128 pairs and 128-slot tiles, a query alone as a unit of
    # 64 -- the same bits; and a row has the score it has in its list of the 16
    zeros = torch.zeros((nq, 1), dtype=torch.int32, device="cuda")
    one = IVFFlatIndex(ix.centroids_normalized[:1]).add(xd, labels=torch.zeros(len(x), dtype=torch.int32, device="cuda"))
    zs, zi = one.search(qd, k=k, probes=zeros)
    for r in (0, 64, 127, 128, 256):
        alone = one.search(qd[r: r + 1], k=k, probes=zeros[:1])
        assert torch.equal(alone[0][0], zs[r]) and torch.equal(alone[1][0], zi[r]), r
    own = ix.search(qd, k=1, nprobe=1)  # the planted neighbour is the best row of its list and of the corpus
    assert torch.equal(own[0][:, 0], zs[:, 0]) and torch.equal(own[1][:, 0], zi[:, 0])


# ------------------------------------------------------------------------------------------ 6. state_dict, train
def test_state_dict_round_trip_and_train():
    from sonar_amd.index import LIST_ALIGN, IVFFlatIndex

    ix, x, q, target, labels = _planted_index(64)
    qd = _dev(q)
    state = ix.state_dict()
    used = int(ix.list_offsets[-1])
    assert set(state) == {"centroids", "offsets", "sizes", "ids", "rows"} and LIST_ALIGN == A
    assert state["rows"].shape == (used, 64) and state["ids"].shape == (used,) and ix.ntotal == len(x)
    assert np.array_equal(ix.list_sizes.cpu().numpy(), np.bincount(labels, minlength=16))
    loaded = IVFFlatIndex.from_state_dict({k: v.cpu().cuda() for k, v in state.items()})
    other = IVFFlatIndex(ix.centroids_normalized).load_state_dict(state)
    for k, nprobe in ((1, 1), (4, 3), (8, 8)):
        want = ix.search(qd, k=k, nprobe=nprobe)
        for again in (loaded, other):
            got = again.search(qd, k=k, nprobe=nprobe)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(RuntimeError, match="already called"):
        ix.add(_dev(x))
    trained = IVFFlatIndex.train(_dev(x), 16, n_iter=3, seed=1).add(_dev(x))
    assert trained.n_lists == 16 and trained.ntotal == len(x)
    score, idx = trained.search(qd, k=2, nprobe=4)
    assert np.array_equal(idx[:, 0].cpu().numpy(), target)
