"""GPU: residual encoding against the list centroid for the IVF-PQ index (sonar_amd/csrc/ivf.hip, sonar_amd/index.py; DESIGN.md
3.22) against tests/ivf_pq_residual_ref.py and against the plain product quantiser on materialised residuals.

`pq_residuals` is compared with the restatement bit for bit.  The three fused entries (encode, train, build), which form the
residual inside their kernels, are compared for equality with the plain entries fed with `pq_residuals`' output: that is where
a fused kernel can go wrong and the materialised route cannot.  A score is, by contract, the flat index's score against the
decoded residual plus one fp32 add: the search is compared bit for bit, scores and ids, with `search_lists` over
`build_lists(pq_decode(codes))` called per probe column, `coarse` added in float32 and the columns merged in numpy; and with the
float64 restatement on integer-valued operands, where every sum is exact.  Only the distance of a real-valued score from its
float64 value is a tolerance: (d + 2) * 2^-23 (tests/ivf_pq_residual_ref.py derives it)."""
import functools

import numpy as np
import pytest
import torch

from tests import ivf_pq_ref as P
from tests import ivf_pq_residual_ref as PR
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


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _mixed_labels(rng, n, k):
    """Labels in [0, K) with some outside it: -1, K and INT32_MAX."""
    lab = rng.integers(0, k, n).astype(np.int64)
    bad = rng.random(n) < 0.25
    lab[bad] = rng.choice(np.array([-1, k, INT32_MAX]), int(bad.sum()))
    return lab.astype(np.int32)


# ------------------------------------------------------------------------------------------------------ 1. residuals
@pytest.mark.parametrize("d", [64, 192, 1024])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_residuals_are_the_restated_residuals(n, d):
    from sonar_amd import index

    for k in (1, 3, 300):
        rng = np.random.default_rng(n * 1009 + d + k)
        x, c = _unit_rows(rng, n, d), _unit_rows(rng, k, d)
        labels = _mixed_labels(rng, n, k)
        labels[0] = k - 1
        # the last row against its centroid: signed zeros, subnormals, and 1 + 2^-10 - 2^-24, which fp32 cannot hold
        c[labels[n - 1] if 0 <= labels[n - 1] < k else 0, :4] = [0.0, -(2.0 ** -24), 2.0 ** -24, 1.0]
        x[n // 2] = 0  # a zero row
        if n > 1:
            x[0] = c[k - 1]  # a row equal to its centroid: +0 everywhere
        x[n - 1, :4] = [-0.0, 2.0 ** -24, 1.0 + 2.0 ** -10, -1.0]
        got = index.pq_residuals(_dev(x), _i32(labels), _dev(c))
        torch.cuda.synchronize()
        assert got.dtype == torch.float16 and tuple(got.shape) == (n, d)
        got, want = got.cpu().numpy(), PR.residuals(x, labels, c)
        bad = np.argwhere(_u16(got) != _u16(want))
        assert len(bad) == 0, (k, bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
        if n > 1:
            assert not got[0].any() and not np.signbit(got[0]).any()
        out = ~((labels >= 0) & (labels < k))
        assert np.array_equal(_u16(got[out]), _u16(x[out]))  # a label out of range: the row itself
        # the first n rows of a larger matrix
        more = index.pq_residuals(_dev(np.concatenate([x, x[:1]])), _i32(labels), _dev(c))
        assert np.array_equal(_u16(more.cpu().numpy()), _u16(want))


# ------------------------------------------------------------------------------------------------------ 2. encode
@pytest.mark.parametrize("d,dsub", SHAPES)
@pytest.mark.parametrize("n", [1, 63, 257])
def test_encode_residual_is_encode_of_the_residuals(n, d, dsub):
    from sonar_amd import index

    rng = np.random.default_rng(n * 1013 + d + dsub)
    for k in (1, 3, 300):
        x, c, cb = _unit_rows(rng, n, d), _unit_rows(rng, k, d), P.random_codebooks(rng, d, dsub, scale=0.5)
        labels = _mixed_labels(rng, n, k)
        x[n // 2] = 0
        xd, ld, cd, cbd = _dev(x), _i32(labels), _dev(c), _dev(cb)
        got = index.pq_encode_residual(xd, ld, cd, cbd)
        res = index.pq_residuals(xd, ld, cd)
        want = index.pq_encode(res, cbd)
        torch.cuda.synchronize()
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, d // dsub)
        assert torch.equal(got, want), k
        if k == 3:  # ... which is the restated encoding of the restated residuals
            assert np.array_equal(got.cpu().numpy(), PR.encode(x, labels, c, cb))
            assert not torch.equal(got, index.pq_encode(xd, cbd)) or n == 1  # and not the plain codes


# ------------------------------------------------------------------------------------------------------ 3. train
@pytest.mark.parametrize("n_iter", [1, 3])
@pytest.mark.parametrize("n,d,dsub", [(256, 64, 8), (300, 192, 16), (1000, 64, 64)])
def test_train_residual_is_train_on_the_residuals(n, d, dsub, n_iter):
    from sonar_amd import index

    rng = np.random.default_rng(n + d + dsub)
    k = 5
    x, c = _unit_rows(rng, n, d), _unit_rows(rng, k, d)
    labels = _mixed_labels(rng, n, k)
    init = rng.permutation(n)[:256]
    xd, ld, cd, initd = _dev(x), _i32(labels), _dev(c), _i32(init)
    got = index.pq_train_residual(xd, ld, cd, dsub, initd, n_iter)
    res = index.pq_residuals(xd, ld, cd)
    want = index.pq_train(res, dsub, initd, n_iter)
    torch.cuda.synchronize()
    assert got.dtype == torch.float16 and tuple(got.shape) == (d // dsub, 256, dsub)
    got, want = got.cpu().numpy(), want.cpu().numpy()
    bad = np.argwhere(_u16(got) != _u16(want))
    assert len(bad) == 0, (bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(_u16(index.pq_train_residual(xd, ld, cd, dsub, initd, n_iter).cpu().numpy()), _u16(got))  # two runs
    start = index.pq_train_residual(xd, ld, cd, dsub, initd, 0).cpu().numpy()  # no round: the residuals of the init rows
    assert np.array_equal(_u16(start), _u16(P.init_codebooks(PR.residuals(x, labels, c), init, dsub)))
    if n_iter == 1:  # the restatement itself
        assert np.array_equal(_u16(got), _u16(PR.train(x, labels, c, init, dsub, 1)[-1]))


# ------------------------------------------------------------------------------------------------------ 4. build
def _check_build(xd, enc, n, labels, cd, cbd):
    """Slot by slot through the ids: every slot holds the codes `pq_encode` gives its row's materialised residual, and the
    layout is `build_lists_pq`'s on the residual matrix."""
    from sonar_amd import _lib, index

    k = cd.shape[0]
    codes, ids, off, sizes = (t.cpu().numpy() for t in index.build_lists_pq_residual(xd, _i32(labels), cd, cbd))
    r_off, r_sizes, r_ids = R.build(labels, k)
    assert codes.dtype == np.uint8 and codes.shape == (len(ids), enc.shape[1])
    assert len(ids) == _lib.load().smi_ivf_slots_bound(n, k) >= r_off[k]
    assert np.array_equal(sizes, r_sizes) and np.array_equal(off, r_off) and (off % A == 0).all()
    total = int(off[k])
    for c in range(k):
        seg, want = ids[off[c]: off[c + 1]], r_ids[r_off[c]: r_off[c + 1]]
        assert np.array_equal(np.sort(seg), np.sort(want)), c
    assert (ids[total:] == -1).all()
    real = ids[:total] >= 0
    assert np.array_equal(codes[:total], np.where(real[:, None], enc[np.maximum(ids[:total], 0)], 0))  # pad slots: zero codes
    return codes, ids, off, sizes


@pytest.mark.parametrize("d,dsub", [(64, 8), (1024, 16)])
@pytest.mark.parametrize("k", [1, 3, 300])
@pytest.mark.parametrize("n", [1, A - 1, A, A + 1, 4099])
def test_build_residual_is_build_on_the_materialised_residuals(n, k, d, dsub):
    from sonar_amd import index

    rng = np.random.default_rng(n * 1000003 + k * 1009 + d)
    x, c = _unit_rows(rng, n, d), _unit_rows(rng, k, d)
    x[n // 2] = 0
    xd, cd, cbd = _dev(x), _dev(c), _dev(P.random_codebooks(rng, d, dsub, scale=0.5))
    for pattern in PATTERNS:
        labels = _labels(rng, pattern, n, k)
        res = index.pq_residuals(xd, _i32(labels), cd)
        enc = index.pq_encode(res, cbd).cpu().numpy()
        codes, ids, off, sizes = _check_build(xd, enc, n, labels, cd, cbd)
        m_codes, m_ids, m_off, m_sizes = (t.cpu().numpy() for t in index.build_lists_pq(res, _i32(labels), k, cbd))
        assert np.array_equal(off, m_off) and np.array_equal(sizes, m_sizes)
        total = int(off[k])
        by_id, m_by_id = np.argsort(ids[:total], kind="stable"), np.argsort(m_ids[:total], kind="stable")
        assert np.array_equal(ids[:total][by_id], m_ids[:total][m_by_id])
        assert np.array_equal(codes[:total][by_id], m_codes[:total][m_by_id])


# ------------------------------------------------------------------------------ 5. search = flat on decoded residuals + coarse
def _garbage_where_no_list(rng, coarse, probes, k_lists):
    """NaN, inf and huge values in the coarse entries of probes that name no list: they are not read."""
    coarse = np.array(coarse, dtype=np.float32)
    none = (np.asarray(probes) < 0) | (np.asarray(probes) >= k_lists)
    coarse[none] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38], dtype=np.float32), int(none.sum()))
    return coarse


def _check_search(x, c, cb, labels, q, probes, coarse, ks):
    """Scores and ids of every row equal, bit for bit, the yardstick: per probe column the flat search over the decoded
    residuals with nprobe = 1, coarse added in float32, the columns merged in numpy.  Returns the last k's (scores, ids)."""
    from sonar_amd import index

    k_lists = len(c)
    probes = np.asarray(probes)
    xd, cd, cbd, qd, ld = _dev(x), _dev(c), _dev(cb), _dev(q), _i32(labels)
    codes, ids, off, _ = index.build_lists_pq_residual(xd, ld, cd, cbd)
    decoded = index.pq_decode(index.pq_encode_residual(xd, ld, cd, cbd), cbd)
    f_rows, f_ids, f_off, _ = index.build_lists(decoded, ld, k_lists)
    assert torch.equal(off, f_off)
    pd, coarsed = _i32(probes), _dev(np.asarray(coarse, dtype=np.float32))
    out = None
    for k in ks:
        score, idx = index.search_lists_pq_residual(qd, pd, coarsed, codes, cbd, ids, off, k)
        cols = [index.search_lists(qd, _i32(probes[:, p: p + 1]), f_rows, f_ids, f_off, k) for p in range(probes.shape[1])]
        torch.cuda.synchronize()
        assert score.dtype == torch.float32 and idx.dtype == torch.int32 and tuple(score.shape) == tuple(idx.shape) == (len(q), k)
        cols = [(s.cpu().numpy(), i.cpu().numpy()) for s, i in cols]
        want_s, want_i = PR.merge([PR.add_coarse(s, i, coarse[:, p]) for p, (s, i) in enumerate(cols)], [i for _, i in cols], k)
        assert want_s.dtype == np.float32
        got_s, got_i = score.cpu().numpy(), idx.cpu().numpy()
        bad = np.flatnonzero((got_i != want_i).any(axis=1) | (_bits32(got_s) != _bits32(want_s)).any(axis=1))
        assert len(bad) == 0, (k, bad[:5], got_i[bad[:2]], want_i[bad[:2]], got_s[bad[:2]], want_s[bad[:2]])
        assert not np.isnan(got_s).any() and (np.isneginf(got_s) == (got_i < 0)).all()
        out = got_s, got_i
    return out


def _coarse(rng, shape):
    return rng.uniform(-1, 1, shape).astype(np.float32)


def test_search_one_row_one_list():
    rng = np.random.default_rng(1)
    _check_search(_unit_rows(rng, 1, 64), _unit_rows(rng, 1, 64), P.random_codebooks(rng, 64, 8), [0], _unit_rows(rng, 1, 64), [[0]],
                  _coarse(rng, (1, 1)), (1, 8))


@pytest.mark.parametrize("nprobe", [1, 3, 8])
def test_search_every_k_and_nprobe(nprobe):
    rng = np.random.default_rng(2)
    x, c, q, cb = _unit_rows(rng, 300, 64), _unit_rows(rng, 8, 64), _unit_rows(rng, 65, 64), P.random_codebooks(rng, 64, 16)
    _check_search(x, c, cb, rng.integers(0, 8, 300), q, _distinct_probes(rng, 65, 8, nprobe), _coarse(rng, (65, nprobe)), (1, 4, 8))


def test_search_list_lengths_around_the_alignment_and_the_tile():
    """Lists of 1, 15, 16, 17 and 129 rows (two tiles at B = 128, three at B = 64) and empty ones, every query probing all."""
    rng = np.random.default_rng(3)
    lengths = [1, 15, 0, 16, 17, 0, 129, 0]
    labels = np.concatenate([np.full(m, c) for c, m in enumerate(lengths)])
    rng.shuffle(labels)
    n = len(labels)
    x, c, q, cb = _unit_rows(rng, n, 192), _unit_rows(rng, 8, 192), _unit_rows(rng, 70, 192), P.random_codebooks(rng, 192, 16)
    probes = _distinct_probes(rng, 70, 8, 8)
    s, i = _check_search(x, c, cb, labels, q, probes, _coarse(rng, (70, 8)), (1, 4, 8))
    assert (i >= 0).all()
    s, i = _check_search(x, c, cb, labels, q, np.tile([[2, 5, 7, 0]], (70, 1)), _coarse(rng, (70, 4)), (4,))  # three empty, one row
    assert (i[:, 0] >= 0).all() and (i[:, 1:] == -1).all()


def test_search_one_long_list_many_tiles_several_query_blocks():
    rng = np.random.default_rng(4)
    x, c, q, cb = _unit_rows(rng, 4099, 64), _unit_rows(rng, 1, 64), _unit_rows(rng, 257, 64), P.random_codebooks(rng, 64, 8)
    _check_search(x, c, cb, np.zeros(4099, dtype=np.int64), q, np.zeros((257, 1), dtype=np.int64), _coarse(rng, (257, 1)), (1, 4, 8))


def test_search_lists_shorter_than_k_empty_lists_and_repeated_lists():
    rng = np.random.default_rng(5)
    x, c, q, cb = _unit_rows(rng, 4099, 64), _unit_rows(rng, 300, 64), _unit_rows(rng, 300, 64), P.random_codebooks(rng, 64, 8)
    labels = rng.integers(0, 300, 4099)
    labels[labels % 5 == 0] += 1  # every fifth list stays empty
    labels[:40] = np.arange(40) % 2 * 2 + 1
    probes = _distinct_probes(rng, 300, 300, 8)
    probes[:5] = np.arange(0, 40, 5).reshape(1, 8)  # rows that probe empty lists only: k x (-inf, -1)
    probes[5, :] = [0, 5, 10, 15, 20, 25, 30, 7]
    s, i = _check_search(x, c, cb, labels, q, probes, _coarse(rng, (300, 8)), (8,))
    assert (i[:5] == -1).all() and np.isneginf(s[:5]).all() and i[5, 0] >= 0
    few = np.where(np.arange(4099) < 20, np.arange(4099) % 10, -1)  # lists of 2 rows, 290 empty, most rows left out
    _check_search(x, c, cb, few, q, rng.integers(0, 12, (300, 8)), _coarse(rng, (300, 8)), (8, 3))  # a list named twice: rows twice


def test_search_probe_entries_that_name_no_list_have_garbage_in_coarse():
    rng = np.random.default_rng(7)
    x, c, q, cb = _unit_rows(rng, 500, 64), _unit_rows(rng, 6, 64), _unit_rows(rng, 70, 64), P.random_codebooks(rng, 64, 32)
    labels = rng.integers(0, 6, 500)
    probes = _distinct_probes(rng, 70, 6, 4)
    probes[rng.random(probes.shape) < 0.4] = -1
    probes[0], probes[69], probes[3, 1], probes[4, 0] = -1, -1, 6, INT32_MAX
    coarse = _garbage_where_no_list(rng, _coarse(rng, probes.shape), probes, 6)
    s, i = _check_search(x, c, cb, labels, q, probes, coarse, (1, 3, 8))
    assert (i[0] == -1).all() and np.isneginf(s[69]).all()
    none = np.full((70, 2), -1)
    s, i = _check_search(x, c, cb, labels, q, none, _garbage_where_no_list(rng, np.zeros((70, 2)), none, 6), (2,))  # no unit at all
    assert (i == -1).all() and np.isneginf(s).all()


def test_search_a_tile_that_holds_one_valid_row():
    rng = np.random.default_rng(9)
    cb, c = P.random_codebooks(rng, 64, 8), _unit_rows(rng, 1, 64)
    x, q = _unit_rows(rng, A + 1, 64), _unit_rows(rng, 5, 64)
    _check_search(x, c, cb, np.zeros(A + 1, dtype=np.int64), q, np.zeros((5, 1), dtype=np.int64), _coarse(rng, (5, 1)), (1, 8))
    x, q = _unit_rows(rng, 65, 64), _unit_rows(rng, 5, 64)  # one row in the second 64-slot tile
    _check_search(x, c, cb, np.zeros(65, dtype=np.int64), q, np.zeros((5, 1), dtype=np.int64), _coarse(rng, (5, 1)), (2, 8))


@pytest.mark.parametrize("d,dsub", [(d, s) for d in (64, 192, 1024) for s in P.DSUBS])
def test_search_every_dim_and_every_dsub_and_the_distance_from_float64(d, dsub):
    """The bits against the yardstick, and every score within (d + 2) * 2^-23 of the float64 restatement on the same fp16
    residuals and fp32 coarse (normalised queries and centroids, unit-scale codebooks: every sum is below 4)."""
    rng = np.random.default_rng(d + dsub)
    n, nq, k_lists, k = 600, 130, 5, 5
    x, c, q, cb = _unit_rows(rng, n, d), _unit_rows(rng, k_lists, d), _unit_rows(rng, nq, d), P.random_codebooks(rng, d, dsub)
    x[0], q[1] = 0, 0
    labels = rng.integers(0, k_lists, n)
    probes = _distinct_probes(rng, nq, k_lists, 4)
    coarse = _coarse(rng, probes.shape)
    got_s, got_i = _check_search(x, c, cb, labels, q, probes, coarse, (k,))
    codes = PR.encode(x, labels, c, cb)
    s64 = R.scores64(q, P.decode(codes, cb))
    want_s, _ = PR.search(q, codes, cb, labels, k_lists, probes, coarse, k, s=s64)
    # the float64 value of every returned (query, row): its residual score plus the coarse entry of the probe naming its list
    col = (probes[:, None, :] == labels[got_i][:, :, None]).argmax(axis=2)
    own = s64[np.arange(nq)[:, None], got_i] + coarse[np.arange(nq)[:, None], col].astype(np.float64)
    tol = (d + 2) * 2.0 ** -23
    dev = max(np.abs(got_s.astype(np.float64) - own).max(), np.abs(got_s.astype(np.float64) - want_s).max())
    print(f"d={d} dsub={dsub}: max |score - fp64| = {dev:.3e} (bound {tol:.3e})")
    assert (got_i >= 0).all() and dev <= tol


@pytest.mark.parametrize("nq", [255, 256, 257])
def test_search_at_the_threshold_between_the_two_unit_sizes(nq):
    """A unit is 128 pairs x 128-slot tiles from nq * nprobe >= 256 K on, 64 x 64 below (csrc/ivf.hip, unit_pairs)."""
    rng = np.random.default_rng(nq)
    x, c, q, cb = _unit_rows(rng, 300, 192), _unit_rows(rng, 1, 192), _unit_rows(rng, nq, 192), P.random_codebooks(rng, 192, 16)
    labels = np.zeros(300, dtype=np.int64)  # one list of 295 rows: a third 128-slot tile with 39 of them
    labels[[7, 100, 101, 250, 299]] = [-1, 1, 2, INT32_MAX, -1]
    _check_search(x, c, cb, labels, q, np.zeros((nq, 1), dtype=np.int64), _coarse(rng, (nq, 1)), (1, 8))


@pytest.mark.parametrize("nq", [70, 256])  # units of 64 pairs (two of them), units of 128
def test_search_every_key_list_length_at_both_unit_sizes(nq):
    """Every instantiation <KT, B> of the residual scan: k = 1, 2, 3, 8 are the key lists of 1, 2, 4 and 8 entries."""
    rng = np.random.default_rng(1200 + nq)
    x, c, q, cb = _unit_rows(rng, 130, 192), _unit_rows(rng, 1, 192), _unit_rows(rng, nq, 192), P.random_codebooks(rng, 192, 16)
    _check_search(x, c, cb, np.zeros(130, dtype=np.int64), q, np.zeros((nq, 1), dtype=np.int64), _coarse(rng, (nq, 1)), (1, 2, 3, 8))


def test_search_units_of_128_pairs_d1024():
    rng = np.random.default_rng(11)
    x, c, q, cb = _unit_rows(rng, 600, 1024), _unit_rows(rng, 2, 1024), _unit_rows(rng, 300, 1024), P.random_codebooks(rng, 1024, 8)
    labels = rng.integers(0, 3, 600)
    labels[labels == 2] = -1  # two lists of ~200 rows, probed by every query: units of 128, 128 and 44 pairs each
    labels[:A + 1] = 1
    probes = np.stack([rng.permutation(2) for _ in range(300)])
    probes[::7, 1] = -1
    coarse = _garbage_where_no_list(rng, _coarse(rng, probes.shape), probes, 2)
    _check_search(x, c, cb, labels, q, probes, coarse, (5,))
    short = np.where(np.arange(600) < 6, np.arange(600) % 2, -1)  # lists of 3 rows: (-inf, -1) tails in the large unit
    _check_search(x, c, cb, short, q, probes, coarse, (4,))


# ------------------------------------------------------------------------------------------ 6. integer-valued operands
def _integer_case(nq, d, dsub):
    """Codebooks, centroids and queries with entries from {-1, 0, 1} and small-integer coarse.  A row is a decoded code row plus
    its centroid (entries in -2 .. 2: exact), so its residual is that code row exactly and its nearest codewords reproduce it.
    Returns (x, c, cb, labels, q, probes, coarse, codes, s64); what the planted ties must give is asserted here, on the
    restatement alone."""
    rng = np.random.default_rng(8 + d)
    n, k_lists = 700, 4
    cb = P.integer_codebooks(rng, d, dsub)
    c = R.integer_rows(rng, k_lists, d)
    r = P.decode(rng.integers(0, 256, (n, d // dsub)), cb)
    labels = rng.integers(1, k_lists, n)
    labels[np.arange(0, n, 3)] = 0  # list 0: 234 rows = 4 tiles of 64 slots, 2 of 128
    copies = {3: 0, 300: 0, 699: 0, 50: 1, 333: 1, 598: 2, 20: 3}  # id -> list: r[3] in different lists and tiles
    for i, l in copies.items():
        r[i], labels[i] = r[3], l
    x = (r.astype(np.float32) + c[labels].astype(np.float32)).astype(np.float16)
    assert np.array_equal(PR.residuals(x, labels, c), r)
    codes = PR.encode(x, labels, c, cb)
    assert np.array_equal(P.decode(codes, cb), r)
    q = R.integer_rows(rng, nq, d)
    q[0] = 0     # every residual score 0: the coarse terms and the ids decide
    q[1] = r[3]
    probes = np.tile([[2, 0, 1]], (nq, 1))
    probes[5:] = _distinct_probes(rng, nq - 5, k_lists, 3)
    coarse = rng.integers(-4, 5, (nq, 3)).astype(np.float32)
    coarse[0] = [1, 1, 1]  # all candidates tie at 1: the lowest ids of lists 2, 0 and 1
    coarse[1] = [3, 3, 3]  # the copies of r[3] tie across three lists: by id
    s64 = R.scores64(q, r)
    assert np.abs(s64).max() < 2 ** 11 and np.array_equal(s64, np.rint(s64))
    member = [np.flatnonzero(labels == l) for l in range(k_lists)]
    lead = lambda t, l: member[l][np.argmax(s64[t, member[l]])]  # noqa: E731  (the leader of list l for query t)
    # query 2: the leaders of lists 2 and 0 tie THROUGH the coarse term -- list 2 has coarse 2 and residual score s_a, list 0
    # coarse 2 + s_a - s_b and residual score s_b.  They meet only in the merge, and the lower id wins; list 1 is far behind
    a, b = lead(2, 2), lead(2, 0)
    coarse[2] = [2, 2 + s64[2, a] - s64[2, b], -50]
    # query 3: the leader of list 2 loses after the add to the SECOND of list 0; query 4: list 2 loses to everything
    coarse[3] = [np.sort(s64[3, member[0]])[-2] - s64[3, lead(3, 2)] - 1, 0, -60]
    coarse[4] = [-40, 0, 0]
    assert np.abs(coarse).max() < 2 ** 11
    s, i = PR.search(q[:5], codes, cb, labels, k_lists, probes[:5], coarse[:5], 8, s=s64[:5])
    assert i[0].tolist() == sorted(np.flatnonzero(labels != 3)[:8].tolist()) and (s[0] == 1).all()
    assert i[1][:6].tolist() == [3, 50, 300, 333, 598, 699] and len(set(s[1][:6].tolist())) == 1 and s[1][6] < s[1][5]
    top = 2 + s64[2, a]
    tied = sorted(m for l, p in ((2, 0), (0, 1)) for m in member[l] if s64[2, m] + coarse[2, p] == top)
    assert a in tied and b in tied and labels[a] != labels[b] and s[2, 0] == s[2, 1] == top
    assert i[2, : min(8, len(tied))].tolist() == tied[:8] and (len(tied) >= 8 or s[2, len(tied)] < top)
    assert lead(3, 2) not in i[3, :2] and (labels[i[3, :2]] == 0).all() and s[3, 1] > s64[3, lead(3, 2)] + coarse[3, 0]
    assert (labels[i[4]] != 2).all() and (i[4] >= 0).all()
    return x, c, cb, labels, q, probes, coarse, codes, s64


@pytest.mark.parametrize("nq", [66, 400])  # 3 nq pairs over 4 lists: units of 64 pairs, units of 128
@pytest.mark.parametrize("d,dsub", [(64, 8), (1024, 16)])
def test_search_integer_valued_equals_the_restatement_with_ties_planted_through_coarse(nq, d, dsub):
    """Every sum is a small integer: the float64 restatement is the one right answer, ids and scores."""
    from sonar_amd import index

    x, c, cb, labels, q, probes, coarse, codes, s64 = _integer_case(nq, d, dsub)
    xd, cd, cbd, qd, pd, coarsed = _dev(x), _dev(c), _dev(cb), _dev(q), _i32(probes), _dev(coarse)
    got_codes, ids, off, _ = index.build_lists_pq_residual(xd, _i32(labels), cd, cbd)
    for k in (1, 4, 6, 8):
        score, idx = index.search_lists_pq_residual(qd, pd, coarsed, got_codes, cbd, ids, off, k)
        torch.cuda.synchronize()
        want_s, want_i = PR.search(q, codes, cb, labels, len(c), probes, coarse, k, s=s64)
        got_s, got_i = score.cpu().numpy(), idx.cpu().numpy()
        bad = np.flatnonzero((got_i != want_i).any(axis=1) | (got_s.astype(np.float64) != want_s).any(axis=1))
        assert len(bad) == 0, (k, bad[:5], got_i[bad[:2]], want_i[bad[:2]], got_s[bad[:2]], want_s[bad[:2]])


# ------------------------------------------------------------------------------------------ 7. planted data, end to end
@functools.lru_cache(maxsize=None)
def _planted():
    """ivf_ref.planted(4096, 16, 256, 512, seed=1), dsub 8, four rounds, init seed 0 (the conditions
    tests/test_ivf_pq_residual_cpu.py asserts on the restatement alone): (residual index, x, q, target, labels, the device's
    normalised rows, queries and centroids as numpy, the restated codebooks, the fitted quantiser).  An index is built from
    the quantiser itself: from a tensor of centroids it would normalise them once more, and the residuals hang on their bits."""
    from sonar_amd import index, xsim
    from sonar_amd.clustering import SphericalKMeans, init_rows
    from sonar_amd.index import IVFPQResidualIndex

    x, truth, _, q, target = R.planted(4096, 16, 256, 512, seed=1)
    xd, qd = _dev(x), _dev(q)
    km = SphericalKMeans(16, n_iter=2).fit(xd, init=xd[:16])
    xnd = xsim.normalize_rows(xd)
    init = init_rows(len(x), 256, 0)
    cb = index.pq_train_residual(xnd, km.labels, km.centroids_normalized.contiguous(), 8, init.to(device="cuda", dtype=torch.int32), 4)
    ix = IVFPQResidualIndex(km, cb).add(xd)
    torch.cuda.synchronize()
    assert np.array_equal(km.labels.cpu().numpy(), truth)
    xn, qn = xnd[: len(x)].cpu().numpy(), xsim.normalize_rows(qd)[: len(q)].cpu().numpy()
    c16 = ix.centroids_normalized.cpu().numpy()
    books = PR.train(xn, truth, c16, init.numpy(), 8, 4)
    assert np.array_equal(ix.list_sizes.cpu().numpy(), np.bincount(truth, minlength=16))  # `add` labelled the rows alike
    return ix, x, q, target, truth, xn, qn, c16, books, km


def test_planted_data_codebooks_codes_scores_and_neighbours():
    from sonar_amd import index, mining, xsim
    from tests.test_ivf_pq_residual_cpu import SCAN_TOL

    ix, x, q, target, labels, xn, qn, c16, books, _ = _planted()
    d, k = 256, 4
    cb = ix.codebooks.cpu().numpy()
    assert np.array_equal(_u16(cb), _u16(books[-1]))  # the trained codebooks, bit for bit
    state = ix.state_dict()
    ids = state["ids"].cpu().numpy()
    res = PR.residuals(xn, labels, c16)
    codes = P.encode(res, cb)
    assert np.array_equal(state["rows"].cpu().numpy()[ids >= 0], codes[ids[ids >= 0]])  # every slot's codes
    # the preconditions, by the restatement on the centroids the device really has
    decoded = P.decode(codes, cb)
    s64 = R.scores64(qn, decoded)
    top_s, top_i = R.search(qn, decoded, labels, 16, labels[target][:, None], 2, s=s64)
    err = P.quantisation_error(res, cb, codes)
    print(f"residual quantisation error {err:.4f}; least gap to the runner-up {(top_s[:, 0] - top_s[:, 1]).min():.5f}")
    assert np.array_equal(top_i[:, 0], target) and (top_s[:, 0] - top_s[:, 1]).min() > SCAN_TOL
    xd, qd = _dev(x), _dev(q)
    qnd, c16d = xsim.normalize_rows(qd), ix._c16  # the centroid table, padded as the probe wants it
    for nprobe in (1, 3):
        score, idx = ix.search(qd, k=k, nprobe=nprobe)
        coarse, probes = xsim.topk_normalized(qnd, len(q), c16d, 16, nprobe)
        # search(q) is the scan fed with the probe's own scores, and search(probes=, coarse=) reproduces it
        fed = index.search_lists_pq_residual(qnd, probes, coarse, ix._rows, ix.codebooks, ix._ids, ix.list_offsets, k)
        assert torch.equal(fed[0], score) and torch.equal(fed[1], idx)
        given = ix.search(qd, k=k, probes=probes, coarse=coarse)
        assert torch.equal(given[0], score) and torch.equal(given[1], idx)
        torch.cuda.synchronize()
        got_s, got_i = score.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
        assert np.array_equal(got_i[:, 0], target)  # every planted row first, at nprobe = 1 already
        if nprobe == 1:
            assert np.array_equal(probes.cpu().numpy()[:, 0], labels[target])
        probes_h, coarse_h = probes.cpu().numpy(), coarse.cpu().numpy()
        want_s, want_i = PR.search(qn, codes, cb, labels, 16, probes_h, coarse_h, k, s=s64)
        tol = (d + 2) * 2.0 ** -23
        dev = np.abs(got_s.astype(np.float64) - want_s)
        print(f"nprobe={nprobe}: max |score - fp64| = {dev.max():.3e} (bound {tol:.3e})")
        assert np.array_equal(want_i[:, 0], got_i[:, 0]) and (got_i >= 0).all() and (dev <= tol).all()
        # without coarse: the restatement fed with pair_scores' cosines of the queries against the probed centroids
        src = torch.arange(len(q), device="cuda").repeat_interleave(nprobe)
        cos = mining.pair_scores(qnd, len(q), c16d, 16, src, probes.reshape(-1).long(), None, None, "cosine").reshape(len(q), nprobe)
        alone = ix.search(qd, k=k, probes=probes)
        fed = index.search_lists_pq_residual(qnd, probes, cos, ix._rows, ix.codebooks, ix._ids, ix.list_offsets, k)
        assert torch.equal(alone[0], fed[0]) and torch.equal(alone[1], fed[1])
        want_s, want_i = PR.search(qn, codes, cb, labels, 16, probes_h, cos.cpu().numpy(), k, s=s64)
        assert np.array_equal(want_i[:, 0], alone[1].cpu().numpy()[:, 0])
        assert (np.abs(alone[0].cpu().numpy().astype(np.float64) - want_s) <= tol).all()
    # probes that name no list, without coarse: clamped before pair_scores, not read by the scan
    probes = ix.probe(qd, 2)
    probes[::3, 1] = -1
    probes[1::3, 1] = 16
    s, i = ix.search(qd, k=2, probes=probes)
    s1, i1 = ix.search(qd, k=2, probes=probes[:, :1].contiguous())
    rows = torch.arange(len(q), device="cuda") % 3 != 2
    assert torch.equal(i[rows], i1[rows]) and not torch.isnan(s).any() and torch.equal(i[:, 0].cpu(), torch.from_numpy(target).int())


def test_planted_data_refine_state_dict_train_and_the_plain_index():
    from sonar_amd import index, xsim
    from sonar_amd.clustering import init_rows
    from sonar_amd.index import IVFPQIndex, IVFPQResidualIndex, ProductQuantizer

    ix, x, q, target, labels, xn, qn, c16, books, km = _planted()
    xd, qd = _dev(x), _dev(q)
    xnd, qnd = xsim.normalize_rows(xd), xsim.normalize_rows(qd)
    k, nq = 8, len(q)
    # refine re-scores against the original rows: refine_candidates on the raw candidates
    raw_s, raw_i = ix.search(qd, k=k, nprobe=3)
    score, idx = ix.search(qd, k=k, nprobe=3, refine=xnd)
    want = index.refine_candidates(qnd, nq, xnd, raw_i)
    assert torch.equal(score, want[0]) and torch.equal(idx, want[1]) and np.array_equal(idx[:, 0].cpu().numpy(), target)
    # state_dict: the plain index's storage plus the marker; neither class loads the other's
    state = ix.state_dict()
    used = int(ix.list_offsets[-1])
    assert set(state) == {"centroids", "offsets", "sizes", "ids", "rows", "codebooks", "by_residual"}
    assert state["rows"].shape == (used, 32) and state["rows"].dtype == torch.uint8 and ix.ntotal == len(x)
    loaded = IVFPQResidualIndex.from_state_dict({n: v.cpu().cuda() for n, v in state.items()})
    other = IVFPQResidualIndex(km, ix.codebooks).load_state_dict(state)
    for kk, nprobe in ((1, 1), (4, 3), (8, 8)):
        want = ix.search(qd, k=kk, nprobe=nprobe)
        for again in (loaded, other):
            got = again.search(qd, k=kk, nprobe=nprobe)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError, match="IVFPQResidualIndex: its codes are residuals"):
        IVFPQIndex.from_state_dict(state)
    with pytest.raises(RuntimeError, match="already called"):
        ix.add(xd)
    with pytest.raises(TypeError, match="IVFPQResidualIndex"):
        ix.self_join(n=len(x))
    # a plain IVFPQIndex on the same data returns what it returned before: search_lists_pq on its own storage, and its state
    # loads into IVFPQIndex and is refused by the residual class
    plain = IVFPQIndex(ix.centroids_normalized, ProductQuantizer.train(xd, dsub=8, n_iter=4, seed=0)).add(xd, labels=_i32(labels))
    probes = plain.probe(qd, 3)
    ps, pi = plain.search(qd, k=4, probes=probes)
    ws, wi = index.search_lists_pq(qnd, probes, plain._rows, plain.codebooks, plain._ids, plain.list_offsets, 4)
    assert torch.equal(ps, ws) and torch.equal(pi, wi) and np.array_equal(pi[:, 0].cpu().numpy(), target)
    pstate = plain.state_dict()
    assert set(pstate) == {"centroids", "offsets", "sizes", "ids", "rows", "codebooks"}
    again = IVFPQIndex.from_state_dict(pstate).search(qd, k=4, probes=probes)
    assert torch.equal(again[0], ps) and torch.equal(again[1], pi)
    with pytest.raises(ValueError, match=r"lacks \['by_residual'\]"):
        IVFPQResidualIndex.from_state_dict(pstate)
    # the residual codes are not the plain ones
    assert not torch.equal(state["rows"], pstate["rows"][: used])
    # train: k-means, the labels `add` will give, residual PQ training -- the pieces above, called in that order
    trained = IVFPQResidualIndex.train(xd, 16, dsub=16, n_iter=3, pq_iter=2, seed=1)
    c16d = trained._c16
    lab = xsim.topk_normalized(xnd, len(x), c16d, 16, 1)[1][:, 0].contiguous()
    want_cb = index.pq_train_residual(xnd, lab, trained.centroids_normalized.contiguous(), 16,
                                      init_rows(len(x), 256, 1).to(device="cuda", dtype=torch.int32), 2)
    assert torch.equal(trained.codebooks, want_cb) and trained.dsub == 16 and trained.n_lists == 16
    trained.add(xd)
    score, idx = trained.search(qd, k=8, nprobe=8, refine=xnd)
    found = (idx[:, 0].cpu().numpy() == target).mean()
    print(f"IVFPQResidualIndex.train, dsub 16, refined: the planted row first for {found:.3f} of the queries")
    assert trained.ntotal == len(x) and score.shape == idx.shape == (nq, 8) and bool((idx >= 0).all()) and found > 0.9


# ------------------------------------------------------------------------------------------ 8. company and layout
def test_bits_do_not_depend_on_company_layout_unit_size_or_run():
    from sonar_amd.index import IVFPQResidualIndex

    from sonar_amd import index, xsim

    ix, x, q, _, labels, *_, km = _planted()
    rng = np.random.default_rng(5)
    k, nq = 4, len(q)
    xd, qd = _dev(x), _dev(q)
    probes = _i32(_distinct_probes(rng, nq, 16, 3))
    coarse = _dev(_coarse(rng, (nq, 3)))
    score, idx = ix.search(qd, k=k, probes=probes, coarse=coarse)
    again = ix.search(qd, k=k, probes=probes, coarse=coarse)
    assert torch.equal(score, again[0]) and torch.equal(idx, again[1])  # two runs
    for r in (0, 1, 63, 64, 65, 128, 255, 256, 511):  # alone
        one = ix.search(qd[r: r + 1], k=k, probes=probes[r: r + 1], coarse=coarse[r: r + 1])
        assert torch.equal(one[0][0], score[r]) and torch.equal(one[1][0], idx[r]), r
    perm = torch.from_numpy(rng.permutation(nq)).cuda()  # the queries in another order
    ps, pi = ix.search(qd[perm], k=k, probes=probes[perm], coarse=coarse[perm])
    assert torch.equal(ps, score[perm]) and torch.equal(pi, idx[perm])
    # the corpus in another order, the labels permuted with it: other slots, other arrival order, other ids -- the same
    # residuals, codes and bits.  Rows with equal scores go by id, which the permutation changes: the ids where no tie is
    cperm = rng.permutation(len(x))
    ix2 = IVFPQResidualIndex(km, ix.codebooks).add(xd[_dev(cperm)], labels=_i32(labels[cperm]))
    s2, i2 = ix2.search(qd, k=k, probes=probes, coarse=coarse)
    assert torch.equal(s2, score)
    sc, mapped, want = score.cpu().numpy(), cperm[i2.cpu().numpy()], idx.cpu().numpy()
    untied = np.ones_like(want, dtype=bool)
    untied[:, 1:] &= sc[:, 1:] != sc[:, :-1]
    untied[:, :-1] &= sc[:, :-1] != sc[:, 1:]
    assert untied.mean() > 0.9 and np.array_equal(mapped[untied], want[untied])
    # list 0 as the ONE list of its own storage (centroid 0, the same bits): 512 pairs on one list run as units of 128 pairs
    # and 128-slot tiles, a query alone as a unit of 64 -- the same bits, and the bits list 0 of the 16 gives (512 pairs <
    # 256 * 16: units of 64)
    zeros = torch.zeros((nq, 1), dtype=torch.int32, device="cuda")
    c0, coarse0 = ix.centroids_normalized[:1].contiguous(), coarse[:, :1].contiguous()
    xnd, qnd = xsim.normalize_rows(xd), xsim.normalize_rows(qd)
    codes, ids, off, _ = index.build_lists_pq_residual(xnd, _i32(np.where(labels == 0, 0, -1)), c0, ix.codebooks)
    zs, zi = index.search_lists_pq_residual(qnd, zeros, coarse0, codes, ix.codebooks, ids, off, k)
    for r in (0, 64, 127, 128, 256):
        alone = index.search_lists_pq_residual(qnd[r: r + 1], zeros[:1], coarse0[r: r + 1], codes, ix.codebooks, ids, off, k)
        assert torch.equal(alone[0][0], zs[r]) and torch.equal(alone[1][0], zi[r]), r
    ws, wi = ix.search(qd, k=k, probes=zeros, coarse=coarse0)
    assert torch.equal(ws, zs) and torch.equal(wi, zi)
