"""GPU: the int8 scalar-quantised IVF index (sonar_amd/csrc/ivf.hip, sonar_amd/index.py) against the numpy restatement in
tests/ivf_i8_ref.py.

The integer sums of the scan are exact and the rest of a score is three float32 roundings in a fixed order, so codes, scales,
scores and ids are compared for equality of bits on ANY data: real-valued rows, saturated rows, rows whose sum float32 cannot
hold.  Only the distance of a score from the float64 dot product of the fp16 rows is a tolerance, and it is the bound derived
in the restatement's header, pair by pair."""
import functools

import numpy as np
import pytest
import torch

from tests import ivf_i8_ref as Q
from tests import ivf_ref as R
from tests.test_gpu_ivf import PATTERNS, _dev, _distinct_probes, _i32, _labels

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
A = R.ALIGN


def _unit_rows(rng, n, d):
    return R.normalize64(rng.standard_normal((n, d))).astype(np.float16)


# ------------------------------------------------------------------------------------------------------ 1. encode
def _check_encode(x16, n=None):
    from sonar_amd import index

    codes, scales = index.encode_rows_int8(_dev(x16), n)
    torch.cuda.synchronize()
    n = len(x16) if n is None else n
    want_c, want_s = Q.encode(x16[:n])
    got_c, got_s = codes.cpu().numpy(), scales.cpu().numpy()
    assert got_c.dtype == np.int8 and got_s.dtype == np.float32 and got_c.shape == (n, x16.shape[1]) and got_s.shape == (n,)
    assert np.array_equal(got_s.view(np.int32), want_s.view(np.int32)), np.flatnonzero(got_s != want_s)[:5]
    bad = np.flatnonzero((got_c != want_c).any(axis=1))
    assert len(bad) == 0, (bad[:5], got_c[bad[0]], want_c[bad[0]])


@pytest.mark.parametrize("d", [64, 192, 1024])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_encode_is_the_restated_encoding(n, d):
    rng = np.random.default_rng(n * 1009 + d)
    _check_encode(_unit_rows(rng, n, d))
    # rows of any size, and the edges: zero, one-hot, +-amax only, exact halves, 65504, subnormals, -0, constant
    wild = (rng.standard_normal((n, d)) * 10.0 ** rng.integers(-6, 4, (n, 1))).astype(np.float16)
    _check_encode(np.concatenate([Q.edge_rows(rng, d), wild]))
    _check_encode(np.concatenate([wild, Q.edge_rows(rng, d)]), n)  # the first n rows of a larger matrix


# ------------------------------------------------------------------------------------------------------ 2. build
def _check_build(x16, labels, k, encoded):
    from sonar_amd import _lib, index

    n, d = x16.shape
    codes, scales, ids, off, sizes = index.build_lists_int8(_dev(x16), _i32(labels), k)
    torch.cuda.synchronize()
    codes, scales, ids, off, sizes = (t.cpu().numpy() for t in (codes, scales, ids, off, sizes))
    r_off, r_sizes, r_ids = R.build(labels, k)
    assert codes.dtype == np.int8 and scales.dtype == np.float32 and codes.shape == (len(ids), d)
    assert len(ids) == len(scales) == _lib.load().smi_ivf_slots_bound(n, k) >= r_off[k]
    assert np.array_equal(sizes, r_sizes) and np.array_equal(off, r_off) and (off % A == 0).all()
    total = int(off[k])
    for c in range(k):
        seg, want = ids[off[c]: off[c + 1]], r_ids[r_off[c]: r_off[c + 1]]
        assert np.array_equal(np.sort(seg), np.sort(want)), c  # the members in any order, and the -1 of the pad slots
    assert (ids[total:] == -1).all()
    want_c, want_s = encoded
    real = ids[:total] >= 0
    src = np.maximum(ids[:total], 0)
    assert np.array_equal(codes[:total], np.where(real[:, None], want_c[src], 0))  # pad slots: zero codes ...
    assert np.array_equal(scales[:total].view(np.int32), np.where(real, want_s[src], np.float32(0)).view(np.int32))  # scale +0


@pytest.mark.parametrize("d", [64, 192, 1024])
@pytest.mark.parametrize("k", [1, 3, 300])
@pytest.mark.parametrize("n", [1, A - 1, A, A + 1, 4099])
def test_build_is_the_list_layout_with_every_slot_encoded(n, k, d):
    rng = np.random.default_rng(n * 1000003 + k * 1009 + d)
    x = (rng.standard_normal((n, d)) * 10.0 ** rng.integers(-3, 3, (n, 1))).astype(np.float16)
    x[n // 2] = 0
    x[0, :2] = [-0.0, 65504.0]
    encoded = Q.encode(x)
    for pattern in PATTERNS:
        _check_build(x, _labels(rng, pattern, n, k), k, encoded)


# ------------------------------------------------------------------------------------------------------ 3. search, exact
def _check_search(x, labels, k_lists, q, probes, ks, storage=None, s=None):
    """Scores and ids of every row equal the restatement bit for bit, for every k of ks.  x / q: any fp16 rows."""
    from sonar_amd import index

    storage = storage or index.build_lists_int8(_dev(x), _i32(labels), k_lists)
    codes, scales, ids, off, _ = storage
    s = Q.scores(q, x) if s is None else s
    qd, pd = _dev(q), _i32(probes)
    for k in ks:
        score, idx = index.search_lists_int8(qd, pd, codes, scales, ids, off, k)
        torch.cuda.synchronize()
        want_s, want_i = Q.search(q, x, labels, k_lists, probes, k, s=s)
        got_s, got_i = score.cpu().numpy(), idx.cpu().numpy()
        assert got_s.dtype == np.float32 and got_i.dtype == np.int32 and got_s.shape == got_i.shape == (len(q), k)
        bad = np.flatnonzero((got_i != want_i).any(axis=1) | (got_s.astype(np.float64) != want_s).any(axis=1))
        assert len(bad) == 0, (k, bad[:5], got_i[bad[:2]], want_i[bad[:2]], got_s[bad[:2]], want_s[bad[:2]])
    return storage


def test_search_one_row_one_list():
    rng = np.random.default_rng(1)
    _check_search(_unit_rows(rng, 1, 64), [0], 1, _unit_rows(rng, 1, 64), [[0]], (1, 8))


def test_search_every_k_and_nprobe():
    rng = np.random.default_rng(2)
    x, q = _unit_rows(rng, 300, 64), _unit_rows(rng, 65, 64)
    labels = rng.integers(0, 8, 300)
    s, storage = Q.scores(q, x), None
    for nprobe in range(1, 9):
        storage = _check_search(x, labels, 8, q, _distinct_probes(rng, 65, 8, nprobe), range(1, 9), storage, s)


def test_search_one_long_list_many_tiles_several_query_blocks():
    rng = np.random.default_rng(3)
    x, q = _unit_rows(rng, 4099, 64), _unit_rows(rng, 257, 64)
    _check_search(x, np.zeros(4099, dtype=np.int64), 1, q, np.zeros((257, 1), dtype=np.int64), (1, 4, 8))


def test_search_lists_shorter_than_k_and_empty_lists():
    rng = np.random.default_rng(4)
    x, q = _unit_rows(rng, 4099, 64), _unit_rows(rng, 300, 64)
    labels = rng.integers(0, 300, 4099)
    labels[labels % 5 == 0] += 1  # every fifth list stays empty
    labels[:40] = np.arange(40) % 2 * 2 + 1  # two larger lists; most of the others hold ~17 rows, some fewer than 8
    probes = _distinct_probes(rng, 300, 300, 8)
    probes[:5] = np.arange(0, 40, 5).reshape(1, 8)  # rows that probe empty lists only: k x (-inf, -1)
    probes[5, :] = [0, 5, 10, 15, 20, 25, 30, 7]    # one short list among empty ones: a (-inf, -1) tail
    s = Q.scores(q, x)
    _check_search(x, labels, 300, q, probes, (8,), s=s)
    few = np.where(np.arange(4099) < 20, np.arange(4099) % 10, -1)  # lists of 2 rows, 290 empty, most rows left out
    _check_search(x, few, 300, q, rng.integers(0, 12, (300, 8)), (8, 3), s=s)  # repeated lists in a row: rows returned twice


def test_search_probe_entries_that_name_no_list():
    rng = np.random.default_rng(7)
    x, q = _unit_rows(rng, 500, 64), _unit_rows(rng, 70, 64)
    labels = rng.integers(0, 6, 500)
    probes = _distinct_probes(rng, 70, 6, 4)
    probes[rng.random(probes.shape) < 0.4] = -1
    probes[0], probes[69], probes[3, 1], probes[4, 0] = -1, -1, 6, INT32_MAX
    s = Q.scores(q, x)
    _check_search(x, labels, 6, q, probes, (1, 3, 8), s=s)
    _check_search(x, labels, 6, q, np.full((70, 2), -1), (2,), s=s)  # no pair at all: the scan has no unit


@pytest.mark.parametrize("nq", [66, 400])  # 3 nq pairs over 4 lists: units of 64 pairs, units of 128
def test_search_planted_ties_across_lists_and_tiles(nq):
    rng = np.random.default_rng(8)
    n, k_lists = 700, 4
    x, q = _unit_rows(rng, n, 64), _unit_rows(rng, nq, 64)
    q[0] = 0  # every candidate ties at +-0: the lowest ids of the probed lists
    labels = rng.integers(1, k_lists, n)
    labels[np.arange(0, n, 3)] = 0  # list 0: 234 rows = 4 tiles of 64 slots, 2 of 128
    copies = {3: 0, 300: 0, 699: 0, 50: 1, 333: 1, 598: 2, 20: 3}  # id -> list: q[1] copied into different lists and tiles
    for i, c in copies.items():
        x[i], labels[i] = q[1], c
    probes = np.tile([[2, 0, 1]], (nq, 1))
    probes[2:] = _distinct_probes(rng, nq - 2, k_lists, 3)
    _check_search(x, labels, k_lists, q, probes, (1, 4, 6, 8))
    s, i = Q.search(q[:2], x, labels, k_lists, probes[:2], 8)
    assert i[0].tolist() == sorted(np.flatnonzero(labels != 3)[:8].tolist()) and (s[0] == 0).all()
    assert i[1][:6].tolist() == [3, 50, 300, 333, 598, 699] and len(set(s[1][:6].tolist())) == 1 and s[1][6] < s[1][5]


def test_search_a_tile_that_holds_one_valid_row():
    rng = np.random.default_rng(9)
    x, q = _unit_rows(rng, A + 1, 64), _unit_rows(rng, 5, 64)
    _check_search(x, np.zeros(A + 1, dtype=np.int64), 1, q, np.zeros((5, 1), dtype=np.int64), (1, 8))
    x, q = _unit_rows(rng, 65, 64), _unit_rows(rng, 5, 64)  # one row in the second 64-slot tile
    _check_search(x, np.zeros(65, dtype=np.int64), 1, q, np.zeros((5, 1), dtype=np.int64), (2, 8))


@pytest.mark.parametrize("d", [64, 192, 1024])  # one slice half full, a full and a half-full one, eight
def test_search_every_slice_shape(d):
    rng = np.random.default_rng(d)
    x, q = _unit_rows(rng, 600, d), _unit_rows(rng, 130, d)
    edges = Q.edge_rows(rng, d)  # zero rows and scales, 65504, subnormals among them
    x[: len(edges)], q[: len(edges)] = edges, edges[::-1]
    labels = rng.integers(0, 5, 600)
    _check_search(x, labels, 5, q, _distinct_probes(rng, 130, 5, 4), (5,))


@pytest.mark.parametrize("nq", [255, 256, 257])
def test_search_at_the_threshold_between_the_two_unit_sizes(nq):
    """A unit is 128 pairs x 128-slot tiles from nq * nprobe >= 256 K on, 64 x 64 below (csrc/ivf.hip, unit_pairs)."""
    rng = np.random.default_rng(nq)
    x, q = _unit_rows(rng, 300, 192), _unit_rows(rng, nq, 192)
    labels = np.zeros(300, dtype=np.int64)  # one list of 295 rows: a third 128-slot tile with 39 of them
    labels[[7, 100, 101, 250, 299]] = [-1, 1, 2, INT32_MAX, -1]
    _check_search(x, labels, 1, q, np.zeros((nq, 1), dtype=np.int64), (1, 8))


@pytest.mark.parametrize("nq", [70, 256])  # units of 64 pairs (two of them), units of 128
def test_search_every_key_list_length_at_both_unit_sizes(nq):
    """Every instantiation <KT, B> of the scan: k = 1, 2, 3, 8 are the key lists of 1, 2, 4 and 8 entries.  One list of
    130 rows is two tiles at B = 128 and three at B = 64, the last one partial; d = 192 is a full K slice and a zero-filled
    half of one."""
    rng = np.random.default_rng(1200 + nq)
    x, q = _unit_rows(rng, 130, 192), _unit_rows(rng, nq, 192)
    _check_search(x, np.zeros(130, dtype=np.int64), 1, q, np.zeros((nq, 1), dtype=np.int64), (1, 2, 3, 8))


def test_search_units_of_128_pairs_d1024():
    rng = np.random.default_rng(11)
    x, q = _unit_rows(rng, 600, 1024), _unit_rows(rng, 300, 1024)
    labels = rng.integers(0, 3, 600)
    labels[labels == 2] = -1  # two lists of ~200 rows, probed by every query: units of 128, 128 and 44 pairs each
    labels[:A + 1] = 1
    probes = np.stack([rng.permutation(2) for _ in range(300)])
    probes[::7, 1] = -1
    s = Q.scores(q, x)
    _check_search(x, labels, 2, q, probes, (5,), s=s)
    short = np.where(np.arange(600) < 6, np.arange(600) % 2, -1)  # lists of 3 rows: (-inf, -1) tails in the large unit
    _check_search(x, short, 2, q, probes, (4,), s=s)


def _saturated(rng, n, d):
    return (rng.choice([-1.0, 1.0], (n, d)) * 0.5).astype(np.float16)


def test_search_saturated_rows_the_largest_sums():
    rng = np.random.default_rng(12)
    d = 1024
    x, q = _saturated(rng, 200, d), _saturated(rng, 70, d)
    x[3], x[150], x[77], q[0] = 0.5, 0.5, -0.5, 0.5  # acc = +-127^2 d: the largest there is, twice (a tie) and negated
    x[5] = -x[4]
    q[1] = x[4]
    labels = rng.integers(0, 2, 200)
    s = Q.scores(q, x)
    acc = Q.int_dots(Q.encode(q)[0], Q.encode(x)[0])
    assert acc[0, 3] == acc[0, 150] == -acc[0, 77] == acc[1, 4] == -acc[1, 5] == 127 * 127 * d
    _check_search(x, labels, 2, q, np.tile([[1, 0]], (70, 1)), (1, 8), s=s)
    got = Q.search(q[:1], x, labels, 2, [[1, 0]], 2, s=s[:1])
    assert got[1][0].tolist() == [3, 150] and got[0][0, 0] == np.float32(127 * 127 * d) * (np.float32(0.5) / np.float32(127)) * (np.float32(0.5) / np.float32(127))


def test_search_sums_float32_cannot_hold():
    """d = 2048, saturated mixed-sign rows with one element at half of amax (code 64): odd sums above 2^24, so (float)acc rounds
    (tests/test_ivf_i8_cpu.py shows why saturated rows alone stay exact at this d)."""
    rng = np.random.default_rng(13)
    d = 2048
    x, q = _saturated(rng, 150, d), _saturated(rng, 66, d)
    x[:, : d * 3 // 4] = 0.5  # three quarters agree: sums around 127^2 d / 2 * (1 +- ...) stay above 2^24 for most pairs
    q[:, : d * 3 // 4] = 0.5
    x[::2, -1] = 0.25
    acc = Q.int_dots(Q.encode(q)[0], Q.encode(x)[0])
    rounds = acc != acc.astype(np.float32).astype(np.int64)
    assert rounds[:, ::2].mean() > 0.9 and (acc % 2 == 1)[:, ::2].all() and acc.min() > 0
    labels = rng.integers(0, 2, 150)
    _check_search(x, labels, 2, q, np.tile([[0, 1]], (66, 1)), (8,))


# ------------------------------------------------------------------------------------------ 4. real-valued planted data
@functools.lru_cache(maxsize=None)
def _planted(d):
    """n 4099, K 16: (int8 index over a quantiser fitted on the planted rows, x, q, target, labels of the rows, and the
    device's normalised fp16 rows of corpus and queries as numpy: what the engine encodes)."""
    from sonar_amd import xsim
    from sonar_amd.clustering import SphericalKMeans
    from sonar_amd.index import IVFInt8Index

    x, truth, _, q, target = R.planted(4099, 16, d, 257)
    xd, qd = _dev(x), _dev(q)
    km = SphericalKMeans(16, n_iter=2).fit(xd, init=xd[:16])
    ix = IVFInt8Index(km).add(xd)
    torch.cuda.synchronize()
    assert np.array_equal(km.labels.cpu().numpy(), truth)
    xn = xsim.normalize_rows(xd)[: len(x)].cpu().numpy()
    qn = xsim.normalize_rows(qd)[: len(q)].cpu().numpy()
    return ix, x, q, target, truth, xn, qn, Q.scores(qn, xn)


@pytest.mark.parametrize("nprobe", [1, 3])
@pytest.mark.parametrize("d", [64, 1024])
def test_planted_data_bits_bound_and_decisions(d, nprobe):
    ix, x, q, target, labels, xn, qn, s = _planted(d)
    k = 4
    qd = _dev(q)
    probes = ix.probe(qd, nprobe)
    score, idx = ix.search(qd, k=k, nprobe=nprobe)
    torch.cuda.synchronize()
    got_s, got_i, probes = score.cpu().numpy(), idx.cpu().numpy().astype(np.int64), probes.cpu().numpy()
    want_s, want_i = Q.search(qn, xn, labels, 16, probes, k, s=s)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s.astype(np.float64), want_s)  # the bits, on real data
    assert (got_i >= 0).all()
    assert np.array_equal(got_i[:, 0], target)  # the planted neighbour, found at nprobe = 1 already
    if nprobe == 1:
        assert np.array_equal(probes[:, 0], labels[target])
    # against float64: every returned score within the derived bound of its pair, and no row of the probed lists that was
    # left out beats the k-th returned one by more than the two pairs' bounds together
    (cq, sq), (cx, sx) = Q.encode(qn), Q.encode(xn)
    s64 = qn.astype(np.float64) @ xn.astype(np.float64).T
    b = Q.bound(Q.l1(cq)[:, None], sq[:, None], Q.l1(cx)[None, :], sx[None, :], d, s)
    rows = np.arange(len(q))[:, None]
    err = np.abs(got_s.astype(np.float64) - s64[rows, got_i])
    print(f"d={d} nprobe={nprobe}: max |score - fp64| = {err.max():.3e}, max error / bound = {(err / b[rows, got_i]).max():.3f}")
    assert (err <= b[rows, got_i]).all()
    for r in range(len(q)):
        left = np.isin(labels, probes[r])
        left[got_i[r]] = False
        last = got_i[r, k - 1]
        assert (s64[r, left] <= s64[r, last] + b[r, last] + b[r, left]).all(), r


# ------------------------------------------------------------------------------------------ 5. company and layout
@pytest.mark.parametrize("d", [64, 1024])
def test_bits_do_not_depend_on_company_layout_or_run(d):
    from sonar_amd.index import IVFInt8Index

    ix, x, q, _, labels, *_ = _planted(d)
    rng = np.random.default_rng(d)
    k, nq = 4, len(q)
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
    ix2 = IVFInt8Index(ix.centroids_normalized).add(xd[_dev(cperm)], labels=_i32(labels[cperm]))
    s2, i2 = ix2.search(qd, k=k, probes=probes)
    assert torch.equal(s2, score) and np.array_equal(cperm[i2.cpu().numpy()], idx.cpu().numpy())
    # every row in ONE list: 257 pairs on one list run as units of 128 pairs and 128-slot tiles, a query alone as a unit of
    # 64 -- the same bits; and a row has the score it has in its list of the 16
    zeros = torch.zeros((nq, 1), dtype=torch.int32, device="cuda")
    one = IVFInt8Index(ix.centroids_normalized[:1]).add(xd, labels=torch.zeros(len(x), dtype=torch.int32, device="cuda"))
    zs, zi = one.search(qd, k=k, probes=zeros)
    for r in (0, 64, 127, 128, 256):
        alone = one.search(qd[r: r + 1], k=k, probes=zeros[:1])
        assert torch.equal(alone[0][0], zs[r]) and torch.equal(alone[1][0], zi[r]), r
    own = ix.search(qd, k=1, nprobe=1)  # the planted neighbour is the best row of its list and of the corpus
    assert torch.equal(own[0][:, 0], zs[:, 0]) and torch.equal(own[1][:, 0], zi[:, 0])


# ------------------------------------------------------------------------------------------ 6. refine
def _in_total_order(s, i):
    for r in range(len(s)):
        for j in range(s.shape[1] - 1):
            if not (s[r, j] > s[r, j + 1] or (s[r, j] == s[r, j + 1] and (i[r, j] < i[r, j + 1] or i[r, j] == -1))):
                return r, j
    return None


@pytest.mark.parametrize("d", [64, 1024])
def test_refine_rescoring_is_the_pair_cosine_in_total_order(d):
    from sonar_amd import mining, xsim
    from sonar_amd.index import IVFFlatIndex

    ix, x, q, target, labels, *_ = _planted(d)
    xd, qd = _dev(x), _dev(q)
    xn, qn = xsim.normalize_rows(xd), xsim.normalize_rows(qd)
    k, nq = 8, len(q)
    raw_s, raw_i = ix.search(qd, k=k, nprobe=3)
    score, idx = ix.search(qd, k=k, nprobe=3, refine=xn)
    torch.cuda.synchronize()
    assert score.dtype == torch.float32 and idx.dtype == torch.int32 and score.shape == idx.shape == (nq, k)
    assert torch.equal(torch.sort(idx, dim=1)[0], torch.sort(raw_i, dim=1)[0])  # the same candidates
    src = torch.arange(nq, device="cuda").repeat_interleave(k)
    cos = mining.pair_scores(qn, nq, xn, len(x), src, idx.reshape(-1).long(), None, None, "cosine").reshape(nq, k)
    assert torch.equal(cos, score)  # bit for bit the cosines of the returned ids
    assert _in_total_order(score.cpu().numpy(), idx.cpu().numpy()) is None
    flat = IVFFlatIndex(ix.centroids_normalized).add(xd, labels=_i32(labels))
    flat_s, flat_i = flat.search(qd, k=1, nprobe=3)
    assert torch.equal(idx[:, 0], flat_i[:, 0]) and np.array_equal(idx[:, 0].cpu().numpy(), target)
    # empty entries stay (-inf, -1) and last; exact duplicates tie and go by id
    probes = _i32(np.tile([[int(labels[target[0]]), -1]], (nq, 1)))
    probes[1] = -1
    assert target[0] not in (5, 6)
    few = np.where(np.isin(np.arange(len(x)), [target[0], 5, 6]), labels[target[0]], -1)
    dup = x.copy()
    dup[5], dup[6] = x[target[0]], x[target[0]]
    small = type(ix)(ix.centroids_normalized).add(_dev(dup), labels=_i32(few))
    s3, i3 = small.search(qd, k=4, probes=probes, refine=xsim.normalize_rows(_dev(dup)))
    s3, i3 = s3.cpu().numpy(), i3.cpu().numpy()
    assert i3[0].tolist() == sorted([5, 6, int(target[0])]) + [-1] and len(set(s3[0, :3].tolist())) == 1
    assert np.isneginf(s3[:, 3]).all() and (i3[1] == -1).all() and np.isneginf(s3[1]).all() and not np.isnan(s3).any()


# ------------------------------------------------------------------------------------------ 7. state_dict, train
def test_state_dict_round_trip_and_train():
    from sonar_amd.index import LIST_ALIGN, IVFInt8Index

    ix, x, q, target, labels, *_ = _planted(64)
    qd = _dev(q)
    state = ix.state_dict()
    used = int(ix.list_offsets[-1])
    assert set(state) == {"centroids", "offsets", "sizes", "ids", "rows", "scales"} and LIST_ALIGN == A
    assert state["rows"].shape == (used, 64) and state["rows"].dtype == torch.int8
    assert state["scales"].shape == state["ids"].shape == (used,) and state["scales"].dtype == torch.float32
    assert ix.ntotal == len(x) and np.array_equal(ix.list_sizes.cpu().numpy(), np.bincount(labels, minlength=16))
    loaded = IVFInt8Index.from_state_dict({k: v.cpu().cuda() for k, v in state.items()})
    other = IVFInt8Index(ix.centroids_normalized).load_state_dict(state)
    for k, nprobe in ((1, 1), (4, 3), (8, 8)):
        want = ix.search(qd, k=k, nprobe=nprobe)
        for again in (loaded, other):
            got = again.search(qd, k=k, nprobe=nprobe)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(RuntimeError, match="already called"):
        ix.add(_dev(x))
    trained = IVFInt8Index.train(_dev(x), 16, n_iter=3, seed=1).add(_dev(x))
    assert trained.n_lists == 16 and trained.ntotal == len(x)
    score, idx = trained.search(qd, k=2, nprobe=4)
    assert np.array_equal(idx[:, 0].cpu().numpy(), target)
