"""GPU: the product quantiser and the IVF-PQ index (sonar_amd/csrc/ivf.hip, sonar_amd/index.py) against the numpy restatement
in tests/ivf_pq_ref.py and against the flat index.

Codes and codebooks are specified down to their bits (one fp32 chain per key, integer sums, three correctly rounded
conversions) and are compared for equality on any data.  A score is, by contract, the flat index's score against the decoded
row: the search is compared bit for bit, scores and ids, with `search_lists` over `build_lists(pq_decode(codes))` on
real-valued data, and with the float64 restatement on integer-valued codebooks and queries, where every partial sum is exact.
Only the distance of a real-valued score from its float64 value is a tolerance: d * 2^-23, the bound tests/test_gpu_ivf.py
derives for the fp32 accumulation of normalised fp16 rows (a decoded row's norm is at most that of the rows it averages)."""
import functools

import numpy as np
import pytest
import torch

from tests import ivf_pq_ref as P
from tests import ivf_ref as R
from tests.test_gpu_ivf import PATTERNS, _dev, _distinct_probes, _i32, _labels

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
A = R.ALIGN
SHAPES = [(64, 8), (64, 64), (192, 16), (256, 32), (1024, 16)]  # (d, dsub)


def _unit_rows(rng, n, d):
    return R.normalize64(rng.standard_normal((n, d))).astype(np.float16)


def _u16(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ------------------------------------------------------------------------------------------------------ 1. encode
def _check_encode(x16, cb, n=None):
    from sonar_amd import index

    codes = index.pq_encode(_dev(x16), _dev(cb), n)
    torch.cuda.synchronize()
    n = len(x16) if n is None else n
    got, want = codes.cpu().numpy(), P.encode(x16[:n], cb)
    assert got.dtype == np.uint8 and got.shape == (n, cb.shape[0])
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    return got


@pytest.mark.parametrize("d,dsub", SHAPES)
@pytest.mark.parametrize("n", [1, 63, 257])
def test_encode_is_the_restated_encoding(n, d, dsub):
    rng = np.random.default_rng(n * 1009 + d + dsub)
    x, cb = _unit_rows(rng, n, d), P.random_codebooks(rng, d, dsub)
    _check_encode(x, cb)
    # a zero codeword, duplicate codewords (the last row's own subvector at codes 200 and 9: the lower code wins)
    cb[0, 7] = 0
    cb[0, 200], cb[0, 9] = x[n - 1, :dsub], x[n - 1, :dsub]
    got = _check_encode(np.concatenate([x, x[:1]]), cb, n)  # the first n rows of a larger matrix
    assert got[n - 1, 0] == 9
    # zero rows, and every row equidistant from two codewords of the last sub-quantiser: +-0.5 e_0 against x_0 = 0, the
    # others far away.  The two keys are equal bit for bit (the x_0 term adds +-0): code 17, not 130
    m = d // dsub - 1
    tie_x, tie_cb = x.copy(), cb.copy()
    tie_x[:, m * dsub] = 0
    tie_x[0] = 0
    tie_cb[m] = 4.0
    tie_cb[m, 17], tie_cb[m, 130] = 0, 0
    tie_cb[m, 17, 0], tie_cb[m, 130, 0] = 0.5, -0.5
    got = _check_encode(tie_x, tie_cb)
    assert (got[:, m] == 17).all()
    got = _check_encode(np.zeros((n, d), dtype=np.float16), np.zeros_like(cb))  # every key ties: code 0
    assert (got == 0).all()


# ------------------------------------------------------------------------------------------------------ 2. train
def _train(x, dsub, init, n_iter):
    from sonar_amd import index

    cb = index.pq_train(_dev(x), dsub, _i32(init), n_iter)
    torch.cuda.synchronize()
    return cb.cpu().numpy()


@pytest.mark.parametrize("n_iter", [1, 3])
@pytest.mark.parametrize("n,d,dsub", [(256, 64, 8), (300, 192, 16), (1000, 64, 64)])
def test_train_is_the_restated_training(n, d, dsub, n_iter):
    rng = np.random.default_rng(n + d + dsub)
    x = _unit_rows(rng, n, d)
    init = rng.permutation(n)[:256]
    want = P.train(x, init, dsub, n_iter)
    got = _train(x, dsub, init, n_iter)
    assert got.dtype == np.float16 and got.shape == (d // dsub, 256, dsub)
    bad = np.argwhere(_u16(got) != _u16(want[-1]))
    assert len(bad) == 0, (bad[:5], got[tuple(bad[0])], want[-1][tuple(bad[0])])
    assert np.array_equal(_u16(_train(x, dsub, init, n_iter)), _u16(got))  # two runs, the same bits
    assert np.array_equal(_u16(_train(x, dsub, init, 0)), _u16(want[0]))  # no round: the start
    # an init that names one row twice: the twin with the higher code never gets a member and keeps its value
    twin = init.copy()
    twin[200] = twin[9]
    got2 = _train(x, dsub, twin, n_iter)
    assert np.array_equal(_u16(got2), _u16(P.train(x, twin, dsub, n_iter)[-1]))
    assert np.array_equal(_u16(got2[:, 200]), _u16(x[twin[9]].reshape(d // dsub, dsub)))


# ------------------------------------------------------------------------------------------------------ 3. decode
@pytest.mark.parametrize("d,dsub", SHAPES)
def test_decode_is_the_gather_and_inverts_encode_on_the_codebooks_own_rows(d, dsub):
    from sonar_amd import index

    rng = np.random.default_rng(d + dsub)
    cb = P.random_codebooks(rng, d, dsub)
    cb[0, 0, :2] = [-0.0, 65504.0]  # bits travel, not values
    for n in (1, 257):
        codes = rng.integers(0, 256, (n, d // dsub)).astype(np.uint8)
        codes[0] = 0
        got = index.pq_decode(_dev(codes), _dev(cb))
        torch.cuda.synchronize()
        assert got.dtype == torch.float16 and tuple(got.shape) == (n, d)
        assert np.array_equal(_u16(got.cpu().numpy()), _u16(P.decode(codes, cb)))
    x = _unit_rows(rng, 256, d)
    own = P.init_codebooks(x, np.arange(256), dsub)  # codeword c of every sub-quantiser = that subvector of row c
    codes = index.pq_encode(_dev(x), _dev(own))
    back = index.pq_decode(codes, _dev(own))
    torch.cuda.synchronize()
    assert np.array_equal(codes.cpu().numpy(), np.tile(np.arange(256, dtype=np.uint8)[:, None], (1, d // dsub)))
    assert np.array_equal(_u16(back.cpu().numpy()), _u16(x))


# ------------------------------------------------------------------------------------------------------ 4. build
def _check_build(xd, enc, n, d, labels, k, cbd):
    from sonar_amd import _lib, index

    codes, ids, off, sizes = index.build_lists_pq(xd, _i32(labels), k, cbd)
    torch.cuda.synchronize()
    codes, ids, off, sizes = (t.cpu().numpy() for t in (codes, ids, off, sizes))
    r_off, r_sizes, r_ids = R.build(labels, k)
    assert codes.dtype == np.uint8 and codes.shape == (len(ids), enc.shape[1])
    assert len(ids) == _lib.load().smi_ivf_slots_bound(n, k) >= r_off[k]
    assert np.array_equal(sizes, r_sizes) and np.array_equal(off, r_off) and (off % A == 0).all()
    total = int(off[k])
    for c in range(k):
        seg, want = ids[off[c]: off[c + 1]], r_ids[r_off[c]: r_off[c + 1]]
        assert np.array_equal(np.sort(seg), np.sort(want)), c  # the members in any order, and the -1 of the pad slots
    assert (ids[total:] == -1).all()
    real = ids[:total] >= 0
    assert np.array_equal(codes[:total], np.where(real[:, None], enc[np.maximum(ids[:total], 0)], 0))  # pad slots: zero codes


@pytest.mark.parametrize("d,dsub", [(64, 8), (1024, 16)])
@pytest.mark.parametrize("k", [1, 3, 300])
@pytest.mark.parametrize("n", [1, A - 1, A, A + 1, 4099])
def test_build_is_the_list_layout_with_every_slot_encoded(n, k, d, dsub):
    """Every slot holds what `pq_encode` gives its row (the encoder itself is compared with the restatement above)."""
    from sonar_amd import index

    rng = np.random.default_rng(n * 1000003 + k * 1009 + d)
    x = _unit_rows(rng, n, d)
    x[n // 2] = 0
    xd, cbd = _dev(x), _dev(P.random_codebooks(rng, d, dsub))
    enc = index.pq_encode(xd, cbd).cpu().numpy()
    for pattern in PATTERNS:
        _check_build(xd, enc, n, d, _labels(rng, pattern, n, k), k, cbd)


# ------------------------------------------------------------------------------------------ 5. search = flat on decoded rows
def _check_search(x, cb, labels, k_lists, q, probes, ks):
    """Scores and ids of every row equal, bit for bit, what the flat index returns on the decoded rows, for every k of ks."""
    from sonar_amd import index

    xd, cbd, qd, pd, ld = _dev(x), _dev(cb), _dev(q), _i32(probes), _i32(labels)
    codes, ids, off, _ = index.build_lists_pq(xd, ld, k_lists, cbd)
    decoded = index.pq_decode(index.pq_encode(xd, cbd), cbd)
    f_rows, f_ids, f_off, _ = index.build_lists(decoded, ld, k_lists)
    assert torch.equal(off, f_off)
    out = None
    for k in ks:
        score, idx = index.search_lists_pq(qd, pd, codes, cbd, ids, off, k)
        want_s, want_i = index.search_lists(qd, pd, f_rows, f_ids, f_off, k)
        torch.cuda.synchronize()
        assert score.dtype == torch.float32 and idx.dtype == torch.int32 and tuple(score.shape) == tuple(idx.shape) == (len(q), k)
        got_s, got_i, want_s, want_i = (t.cpu().numpy() for t in (score, idx, want_s, want_i))
        bad = np.flatnonzero((got_i != want_i).any(axis=1) | (got_s.view(np.int32) != want_s.view(np.int32)).any(axis=1))
        assert len(bad) == 0, (k, bad[:5], got_i[bad[:2]], want_i[bad[:2]], got_s[bad[:2]], want_s[bad[:2]])
        out = got_s, got_i
    return out


def test_search_one_row_one_list():
    rng = np.random.default_rng(1)
    _check_search(_unit_rows(rng, 1, 64), P.random_codebooks(rng, 64, 8), [0], 1, _unit_rows(rng, 1, 64), [[0]], (1, 8))


@pytest.mark.parametrize("nprobe", [1, 3, 8])
def test_search_every_k_and_nprobe(nprobe):
    rng = np.random.default_rng(2)
    x, q, cb = _unit_rows(rng, 300, 64), _unit_rows(rng, 65, 64), P.random_codebooks(rng, 64, 16)
    _check_search(x, cb, rng.integers(0, 8, 300), 8, q, _distinct_probes(rng, 65, 8, nprobe), (1, 4, 8))


def test_search_one_long_list_many_tiles_several_query_blocks():
    rng = np.random.default_rng(3)
    x, q, cb = _unit_rows(rng, 4099, 64), _unit_rows(rng, 257, 64), P.random_codebooks(rng, 64, 8)
    _check_search(x, cb, np.zeros(4099, dtype=np.int64), 1, q, np.zeros((257, 1), dtype=np.int64), (1, 4, 8))


def test_search_lists_shorter_than_k_and_empty_lists():
    rng = np.random.default_rng(4)
    x, q, cb = _unit_rows(rng, 4099, 64), _unit_rows(rng, 300, 64), P.random_codebooks(rng, 64, 8)
    labels = rng.integers(0, 300, 4099)
    labels[labels % 5 == 0] += 1  # every fifth list stays empty
    labels[:40] = np.arange(40) % 2 * 2 + 1  # two larger lists; most of the others hold ~17 rows, some fewer than 8
    probes = _distinct_probes(rng, 300, 300, 8)
    probes[:5] = np.arange(0, 40, 5).reshape(1, 8)  # rows that probe empty lists only: k x (-inf, -1)
    probes[5, :] = [0, 5, 10, 15, 20, 25, 30, 7]    # one short list among empty ones: a (-inf, -1) tail
    s, i = _check_search(x, cb, labels, 300, q, probes, (8,))
    assert (i[:5] == -1).all() and np.isneginf(s[:5]).all() and i[5, 0] >= 0
    few = np.where(np.arange(4099) < 20, np.arange(4099) % 10, -1)  # lists of 2 rows, 290 empty, most rows left out
    _check_search(x, cb, few, 300, q, rng.integers(0, 12, (300, 8)), (8, 3))  # repeated lists in a row: rows returned twice


def test_search_probe_entries_that_name_no_list():
    rng = np.random.default_rng(7)
    x, q, cb = _unit_rows(rng, 500, 64), _unit_rows(rng, 70, 64), P.random_codebooks(rng, 64, 32)
    labels = rng.integers(0, 6, 500)
    probes = _distinct_probes(rng, 70, 6, 4)
    probes[rng.random(probes.shape) < 0.4] = -1
    probes[0], probes[69], probes[3, 1], probes[4, 0] = -1, -1, 6, INT32_MAX
    s, i = _check_search(x, cb, labels, 6, q, probes, (1, 3, 8))
    assert (i[0] == -1).all() and np.isneginf(s[69]).all()
    s, i = _check_search(x, cb, labels, 6, q, np.full((70, 2), -1), (2,))  # no pair at all: the scan has no unit
    assert (i == -1).all() and np.isneginf(s).all()


def test_search_a_tile_that_holds_one_valid_row():
    rng = np.random.default_rng(9)
    cb = P.random_codebooks(rng, 64, 8)
    x, q = _unit_rows(rng, A + 1, 64), _unit_rows(rng, 5, 64)
    _check_search(x, cb, np.zeros(A + 1, dtype=np.int64), 1, q, np.zeros((5, 1), dtype=np.int64), (1, 8))
    x, q = _unit_rows(rng, 65, 64), _unit_rows(rng, 5, 64)  # one row in the second 64-slot tile
    _check_search(x, cb, np.zeros(65, dtype=np.int64), 1, q, np.zeros((5, 1), dtype=np.int64), (2, 8))


@pytest.mark.parametrize("d,dsub", [(d, s) for d in (64, 192, 1024) for s in P.DSUBS])
def test_search_every_dim_and_every_dsub(d, dsub):
    rng = np.random.default_rng(d + dsub)
    x, q, cb = _unit_rows(rng, 600, d), _unit_rows(rng, 130, d), P.random_codebooks(rng, d, dsub)
    x[0], q[1] = 0, 0
    _check_search(x, cb, rng.integers(0, 5, 600), 5, q, _distinct_probes(rng, 130, 5, 4), (5,))


@pytest.mark.parametrize("nq", [255, 256, 257])
def test_search_at_the_threshold_between_the_two_unit_sizes(nq):
    """A unit is 128 pairs x 128-slot tiles from nq * nprobe >= 256 K on, 64 x 64 below (csrc/ivf.hip, unit_pairs)."""
    rng = np.random.default_rng(nq)
    x, q, cb = _unit_rows(rng, 300, 192), _unit_rows(rng, nq, 192), P.random_codebooks(rng, 192, 16)
    labels = np.zeros(300, dtype=np.int64)  # one list of 295 rows: a third 128-slot tile with 39 of them
    labels[[7, 100, 101, 250, 299]] = [-1, 1, 2, INT32_MAX, -1]
    _check_search(x, cb, labels, 1, q, np.zeros((nq, 1), dtype=np.int64), (1, 8))


@pytest.mark.parametrize("nq", [70, 256])  # units of 64 pairs (two of them), units of 128
def test_search_every_key_list_length_at_both_unit_sizes(nq):
    """Every instantiation <KT, B> of the scan: k = 1, 2, 3, 8 are the key lists of 1, 2, 4 and 8 entries.  One list of
    130 rows is two tiles at B = 128 and three at B = 64, the last one partial; d = 192 is three K slices."""
    rng = np.random.default_rng(1200 + nq)
    x, q, cb = _unit_rows(rng, 130, 192), _unit_rows(rng, nq, 192), P.random_codebooks(rng, 192, 16)
    _check_search(x, cb, np.zeros(130, dtype=np.int64), 1, q, np.zeros((nq, 1), dtype=np.int64), (1, 2, 3, 8))


def test_search_units_of_128_pairs_d1024():
    rng = np.random.default_rng(11)
    x, q, cb = _unit_rows(rng, 600, 1024), _unit_rows(rng, 300, 1024), P.random_codebooks(rng, 1024, 8)
    labels = rng.integers(0, 3, 600)
    labels[labels == 2] = -1  # two lists of ~200 rows, probed by every query: units of 128, 128 and 44 pairs each
    labels[:A + 1] = 1
    probes = np.stack([rng.permutation(2) for _ in range(300)])
    probes[::7, 1] = -1
    _check_search(x, cb, labels, 2, q, probes, (5,))
    short = np.where(np.arange(600) < 6, np.arange(600) % 2, -1)  # lists of 3 rows: (-inf, -1) tails in the large unit
    _check_search(x, cb, short, 2, q, probes, (4,))


@pytest.mark.parametrize("nq", [66, 400])  # 3 nq pairs over 4 lists: units of 64 pairs, units of 128
@pytest.mark.parametrize("d,dsub", [(64, 8), (1024, 16)])
def test_search_integer_valued_equals_the_restatement_with_planted_ties(nq, d, dsub):
    """Codebooks and queries with entries from {-1, 0, 1}: every partial sum is a small integer, the float64 restatement is the
    one right answer.  The rows are decoded code rows, so their nearest codewords reproduce them."""
    from sonar_amd import index

    rng = np.random.default_rng(8 + d)
    n, k_lists = 700, 4
    cb = P.integer_codebooks(rng, d, dsub)
    x = P.decode(rng.integers(0, 256, (n, d // dsub)), cb)
    q = R.integer_rows(rng, nq, d)
    q[0] = 0  # every candidate ties at 0: the lowest ids of the probed lists
    q[1] = x[3]
    labels = rng.integers(1, k_lists, n)
    labels[np.arange(0, n, 3)] = 0  # list 0: 234 rows = 4 tiles of 64 slots, 2 of 128
    copies = {3: 0, 300: 0, 699: 0, 50: 1, 333: 1, 598: 2, 20: 3}  # id -> list: x[3] copied into different lists and tiles
    for i, c in copies.items():
        x[i], labels[i] = x[3], c
    probes = np.tile([[2, 0, 1]], (nq, 1))
    probes[2:] = _distinct_probes(rng, nq - 2, k_lists, 3)
    codes = P.encode(x, cb)
    assert np.array_equal(P.decode(codes, cb), x)
    s64 = R.scores64(q, x)
    assert np.abs(s64).max() < 2 ** 11 and np.array_equal(s64, np.rint(s64))
    xd, cbd, qd, pd = _dev(x), _dev(cb), _dev(q), _i32(probes)
    got_codes, ids, off, _ = index.build_lists_pq(xd, _i32(labels), k_lists, cbd)
    for k in (1, 4, 6, 8):
        score, idx = index.search_lists_pq(qd, pd, got_codes, cbd, ids, off, k)
        torch.cuda.synchronize()
        want_s, want_i = P.search(q, codes, cb, labels, k_lists, probes, k, s=s64)
        got_s, got_i = score.cpu().numpy(), idx.cpu().numpy()
        bad = np.flatnonzero((got_i != want_i).any(axis=1) | (got_s.astype(np.float64) != want_s).any(axis=1))
        assert len(bad) == 0, (k, bad[:5], got_i[bad[:2]], want_i[bad[:2]], got_s[bad[:2]], want_s[bad[:2]])
    s, i = P.search(q[:2], codes, cb, labels, k_lists, probes[:2], 8, s=s64[:2])
    assert i[0].tolist() == sorted(np.flatnonzero(labels != 3)[:8].tolist()) and (s[0] == 0).all()
    assert i[1][:6].tolist() == [3, 50, 300, 333, 598, 699] and len(set(s[1][:6].tolist())) == 1 and s[1][6] < s[1][5]


# ------------------------------------------------------------------------------------------ 6. planted data
@functools.lru_cache(maxsize=None)
def _planted():
    """ivf_ref.planted(4096, 16, 256, 512, seed=1), dsub 8, four rounds, init seed 0 (the conditions tests/test_ivf_pq_cpu.py
    asserts on the restatement alone): (index, x, q, target, labels, the device's normalised rows and queries as numpy, the
    restated codebooks)."""
    from sonar_amd import xsim
    from sonar_amd.clustering import SphericalKMeans, init_rows
    from sonar_amd.index import IVFPQIndex, ProductQuantizer

    x, truth, _, q, target = R.planted(4096, 16, 256, 512, seed=1)
    xd, qd = _dev(x), _dev(q)
    km = SphericalKMeans(16, n_iter=2).fit(xd, init=xd[:16])
    pq = ProductQuantizer.train(xd, dsub=8, n_iter=4, seed=0)
    ix = IVFPQIndex(km, pq).add(xd)
    torch.cuda.synchronize()
    assert np.array_equal(km.labels.cpu().numpy(), truth)
    xn = xsim.normalize_rows(xd)[: len(x)].cpu().numpy()
    qn = xsim.normalize_rows(qd)[: len(q)].cpu().numpy()
    books = P.train(xn, init_rows(len(x), 256, 0).numpy(), 8, 4)
    return ix, x, q, target, truth, xn, qn, books


def test_planted_data_codes_scores_and_neighbours():
    from sonar_amd import index

    ix, x, q, target, labels, xn, qn, books = _planted()
    d, k = 256, 4
    cb = ix.codebooks.cpu().numpy()
    assert np.array_equal(_u16(cb), _u16(books[-1]))  # the trained codebooks, bit for bit
    state = ix.state_dict()
    ids = state["ids"].cpu().numpy()
    codes = P.encode(xn, cb)
    assert np.array_equal(state["rows"].cpu().numpy()[ids >= 0], codes[ids[ids >= 0]])
    err = [P.quantisation_error(xn, b) for b in (books[0], books[-1])]
    print(f"quantisation error: {err[0]:.4f} at the start, {err[1]:.4f} after four rounds")
    assert err[1] < err[0]
    decoded = P.decode(codes, cb)
    s64 = R.scores64(qn, decoded)
    qd = _dev(q)
    f_rows, f_ids, f_off, _ = index.build_lists(_dev(decoded), _i32(labels), 16)  # the flat lists of the decoded rows
    for nprobe in (1, 3):
        probes = ix.probe(qd, nprobe)
        score, idx = ix.search(qd, k=k, probes=probes)
        torch.cuda.synchronize()
        got_s, got_i = score.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
        assert np.array_equal(got_i[:, 0], target)  # every planted row first, at nprobe = 1 already
        if nprobe == 1:
            assert np.array_equal(probes.cpu().numpy()[:, 0], labels[target])
        # the restatement: the same neighbour first, every returned score within the fp32 accumulation's bound of its float64
        # value, and no row of the probed lists that was left out beats the k-th returned one by more than twice that
        want_s, want_i = P.search(qn, codes, cb, labels, 16, probes.cpu().numpy(), k, s=s64)
        assert np.array_equal(want_i[:, 0], got_i[:, 0]) and (got_i >= 0).all()
        tol = d * 2.0 ** -23
        rows = np.arange(len(q))[:, None]
        dev = np.abs(got_s.astype(np.float64) - s64[rows, got_i])
        print(f"nprobe={nprobe}: max |score - fp64| = {dev.max():.3e} (bound {tol:.3e})")
        assert (dev <= tol).all() and (np.abs(got_s.astype(np.float64) - want_s) <= tol).all()
        # the bits: the flat scan over the decoded rows as they are (IVFFlatIndex.add would normalise them again)
        fs, fi = index.search_lists(_dev(qn), probes, f_rows, f_ids, f_off, k)
        assert torch.equal(fs, score) and torch.equal(fi, idx)


def test_planted_data_refine_is_the_pair_cosine_in_total_order():
    from sonar_amd import mining, xsim
    from sonar_amd.index import IVFFlatIndex
    from tests.test_gpu_ivf_i8 import _in_total_order

    ix, x, q, target, labels, *_ = _planted()
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
    assert torch.equal(idx[:, 0], flat_i[:, 0])  # the refined top-1 is the flat index's
    assert np.array_equal(idx[:, 0].cpu().numpy(), target)
    # empty entries stay (-inf, -1) and last
    probes = _i32(np.tile([[int(labels[target[0]]), -1]], (nq, 1)))
    probes[1] = -1
    others = [i for i in (5, 6, 7) if i != target[0]][:2]
    few = np.where(np.isin(np.arange(len(x)), [target[0], *others]), labels[target[0]], -1)
    small = type(ix)(ix.centroids_normalized, ix.codebooks).add(xd, labels=_i32(few))
    s3, i3 = small.search(qd, k=4, probes=probes, refine=xn)
    s3, i3 = s3.cpu().numpy(), i3.cpu().numpy()
    assert sorted(i3[0, :3].tolist()) == sorted([*others, int(target[0])]) and i3[0, 0] == target[0] and i3[0, 3] == -1
    assert np.isneginf(s3[:, 3]).all() and (i3[1] == -1).all() and np.isneginf(s3[1]).all() and not np.isnan(s3).any()


# ------------------------------------------------------------------------------------------ 7. company and layout
def test_bits_do_not_depend_on_company_layout_unit_size_or_run():
    from sonar_amd.index import IVFPQIndex

    ix, x, q, _, labels, *_ = _planted()
    rng = np.random.default_rng(5)
    k, nq = 4, len(q)
    xd, qd = _dev(x), _dev(q)
    probes = _i32(_distinct_probes(rng, nq, 16, 3))
    score, idx = ix.search(qd, k=k, probes=probes)
    again = ix.search(qd, k=k, probes=probes)
    assert torch.equal(score, again[0]) and torch.equal(idx, again[1])  # two runs
    for r in (0, 1, 63, 64, 65, 128, 255, 256, 511):  # alone
        one = ix.search(qd[r: r + 1], k=k, probes=probes[r: r + 1])
        assert torch.equal(one[0][0], score[r]) and torch.equal(one[1][0], idx[r]), r
    perm = torch.from_numpy(rng.permutation(nq)).cuda()  # the queries in another order
    ps, pi = ix.search(qd[perm], k=k, probes=probes[perm])
    assert torch.equal(ps, score[perm]) and torch.equal(pi, idx[perm])
    # the corpus in another order, the lists given: other slots, other arrival order, other ids -- the same rows and bits.
    # Rows with equal codes tie and go by id, which the permutation changes: compare the scores, and the ids where no tie is
    cperm = rng.permutation(len(x))
    ix2 = IVFPQIndex(ix.centroids_normalized, ix.codebooks).add(xd[_dev(cperm)], labels=_i32(labels[cperm]))
    s2, i2 = ix2.search(qd, k=k, probes=probes)
    assert torch.equal(s2, score)
    sc, mapped, want = score.cpu().numpy(), cperm[i2.cpu().numpy()], idx.cpu().numpy()
    untied = np.ones_like(want, dtype=bool)
    untied[:, 1:] &= sc[:, 1:] != sc[:, :-1]
    untied[:, :-1] &= sc[:, :-1] != sc[:, 1:]
    assert untied.mean() > 0.9 and np.array_equal(mapped[untied], want[untied])
    # the rows of list 0 as the ONE list of an index: 512 pairs on one list run as units of 128 pairs and 128-slot tiles, a
    # query alone as a unit of 64 -- the same bits, and the bits list 0 of the 16 gives
    zeros = torch.zeros((nq, 1), dtype=torch.int32, device="cuda")
    one = IVFPQIndex(ix.centroids_normalized[:1], ix.codebooks).add(xd, labels=_i32(np.where(labels == 0, 0, -1)))
    zs, zi = one.search(qd, k=k, probes=zeros)
    for r in (0, 64, 127, 128, 256):
        alone = one.search(qd[r: r + 1], k=k, probes=zeros[:1])
        assert torch.equal(alone[0][0], zs[r]) and torch.equal(alone[1][0], zi[r]), r
    ws, wi = ix.search(qd, k=k, probes=zeros)  # list 0 of the 16: 512 pairs < 256 * 16, units of 64
    assert torch.equal(ws, zs) and torch.equal(wi, zi)


# ------------------------------------------------------------------------------------------ 8. the Python surface
def test_state_dict_round_trip_train_and_the_existing_indexes():
    from sonar_amd import xsim
    from sonar_amd.index import LIST_ALIGN, IVFFlatIndex, IVFInt8Index, IVFPQIndex, ProductQuantizer

    ix, x, q, target, labels, *_ = _planted()
    xd, qd = _dev(x), _dev(q)
    state = ix.state_dict()
    used = int(ix.list_offsets[-1])
    assert set(state) == {"centroids", "offsets", "sizes", "ids", "rows", "codebooks"} and LIST_ALIGN == A
    assert state["rows"].shape == (used, 32) and state["rows"].dtype == torch.uint8 and state["ids"].shape == (used,)
    assert state["codebooks"].shape == (32, 256, 8) and state["codebooks"].dtype == torch.float16
    assert ix.ntotal == len(x) and np.array_equal(ix.list_sizes.cpu().numpy(), np.bincount(labels, minlength=16))
    # storage: M bytes per row against 2 d
    assert state["rows"].numel() * 16 == used * 256 * 2
    loaded = IVFPQIndex.from_state_dict({k: v.cpu().cuda() for k, v in state.items()})
    other = IVFPQIndex(ix.centroids_normalized, ix.codebooks).load_state_dict(state)
    for k, nprobe in ((1, 1), (4, 3), (8, 8)):
        want = ix.search(qd, k=k, nprobe=nprobe)
        for again in (loaded, other):
            got = again.search(qd, k=k, nprobe=nprobe)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(RuntimeError, match="already called"):
        ix.add(xd)
    with pytest.raises(TypeError, match="IVFPQIndex"):
        ix.self_join(n=len(x))
    # the product quantiser on its own
    pq = ProductQuantizer(ix.codebooks)
    pq2 = ProductQuantizer.from_state_dict(pq.state_dict())
    codes = pq.encode(xd)
    assert torch.equal(codes, pq2.encode(xd)) and codes.shape == (len(x), 32) and pq.decode(codes).shape == (len(x), 256)
    ids = state["ids"].cpu().numpy()
    assert np.array_equal(state["rows"].cpu().numpy()[ids >= 0], codes.cpu().numpy()[ids[ids >= 0]])
    same = ProductQuantizer.train(xd, dsub=8, n_iter=4, seed=0)
    assert torch.equal(same.codebooks, ix.codebooks)  # one seed, one run
    # train
    trained = IVFPQIndex.train(xd, 16, dsub=16, n_iter=3, pq_iter=2, seed=1).add(xd)
    assert trained.n_lists == 16 and trained.ntotal == len(x) and trained.dsub == 16
    score, idx = trained.search(qd, k=8, nprobe=8, refine=xsim.normalize_rows(xd))
    found = (idx[:, 0].cpu().numpy() == target).mean()
    print(f"IVFPQIndex.train, dsub 16, refined: the planted row first for {found:.3f} of the queries")
    assert score.shape == idx.shape == (len(q), 8) and bool((idx >= 0).all()) and found > 0.9
    # the two existing indexes: their state dicts load as before
    for cls, keys in ((IVFFlatIndex, {"centroids", "offsets", "sizes", "ids", "rows"}),
                      (IVFInt8Index, {"centroids", "offsets", "sizes", "ids", "rows", "scales"})):
        old = cls(ix.centroids_normalized).add(xd, labels=_i32(labels))
        st = old.state_dict()
        assert set(st) == keys and st["rows"].shape[1] == 256
        new = cls.from_state_dict(st)
        a, b = old.search(qd, k=4, nprobe=2), new.search(qd, k=4, nprobe=2)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        with pytest.raises(ValueError, match="rows must be"):
            cls.from_state_dict({**st, "rows": state["rows"]})
