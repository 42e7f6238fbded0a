"""GPU: filtered search over the IVF lists (sonar_amd/csrc/ivf_list_kernels.hpp, ivf_scan.hpp, sonar_amd/index.py; DESIGN.md
3.24) against the numpy restatement in tests/ivf_filter_ref.py -- the existing restatements on labels that keep, per distinct
query key, only the rows that count -- and, without any restatement, against the unkeyed kernels on storage built from those
labels.

Operands of the exact cases have entries from {-1, 0, 1} (ivf_ref.integer_rows): every score is a small integer, exact in fp32
in any order, so scores and ids must equal the yardstick bit for bit.  Row keys are drawn from five values (equal keys are
frequent, negative ones included), a case has at most six distinct query keys, and the slot keys of the slots that hold no row
are overwritten with a value that PASSES the predicate: they must never be looked at.  The shapes are the smallest that reach
each path of the unit, as in tests/test_gpu_ivf_range.py."""
import functools

import numpy as np
import pytest
import torch

from tests import ivf_filter_ref as F
from tests import ivf_i8_ref as Q
from tests import ivf_pq_ref as P
from tests import ivf_pq_residual_ref as PR
from tests import ivf_ref as R

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
KEYS = np.array([-7, -1, 0, 3, 1 << 20])  # what row keys are drawn from
QKEYS = np.array([-7, -1, 0, 3, 1 << 20, 2])  # ... and query keys: the five and one no row has


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i32(a):
    return _dev(np.asarray(a, dtype=np.int32))


def _distinct_probes(rng, nq, k_lists, nprobe):
    return np.stack([rng.permutation(k_lists)[:nprobe] for _ in range(nq)])


def _pad_key(accept, query_keys):
    """A key that passes against (nearly) every query of the case: below all of them, above all of them, or equal to one."""
    return INT32_MIN if accept & 1 else INT32_MAX if accept & 4 else int(np.asarray(query_keys)[0])


def _row_filter(ids, off, row_keys=None, mask=None, pad_key=None):
    """`index.slot_filter` with the keys of the slots that hold no visible row overwritten."""
    from sonar_amd import index

    flt = index.slot_filter(ids, off, None if row_keys is None else _i32(row_keys), None if mask is None else _dev(np.asarray(mask, dtype=bool)))
    assert flt.ids.shape == ids.shape and flt.ids.dtype == torch.int32 and (flt.keys is None) == (row_keys is None)
    if flt.keys is not None and pad_key is not None:
        flt.keys[flt.ids < 0] = pad_key
    return flt


def _same(got, want, what=None):
    """Device (scores fp32, ids int32) equal the yardstick's (float64 or fp32 scores, ids) exactly."""
    got_s, got_i = got[0].cpu().numpy(), got[1].cpu().numpy()
    want_s, want_i = np.asarray(want[0]), np.asarray(want[1])
    assert got_s.dtype == np.float32 and got_i.dtype == np.int32 and got_s.shape == got_i.shape == want_i.shape
    bad = np.flatnonzero((got_i != want_i).any(axis=1) | (got_s.astype(np.float64) != want_s.astype(np.float64)).any(axis=1))
    assert len(bad) == 0, (what, bad[:5], got_i[bad[:2]], want_i[bad[:2]], got_s[bad[:2]], want_s[bad[:2]])
    assert (np.isneginf(got_s) == (got_i < 0)).all(), what  # no id < 0 beside a finite score, no -inf beside a row
    return got_s, got_i


def _bits(t):
    return t[0].view(torch.int32), t[1]


# ------------------------------------------------------------------------------------------------------ 1. flat, exact
@functools.lru_cache(maxsize=None)
def _small_case():
    """n = 300, d = 128, 3 lists, 65 queries: a unit of 64 pairs and a unit of one."""
    from sonar_amd import index

    rng = np.random.default_rng(21)
    x, q = R.integer_rows(rng, 300, 128), R.integer_rows(rng, 65, 128)
    q[0] = 0  # every candidate ties at 0: the lowest allowed ids
    labels = rng.integers(0, 3, 300)
    row_keys, query_keys = rng.choice(KEYS, 300), rng.choice(QKEYS, 65)
    storage = index.build_lists(_dev(x), _i32(labels), 3)
    return x, q, labels, row_keys, query_keys, R.scores64(q, x), storage


@pytest.mark.parametrize("nprobe", [1, 2, 3])
def test_flat_every_accept_every_k(nprobe):
    from sonar_amd import index

    x, q, labels, row_keys, query_keys, s64, (rows, ids, off, _) = _small_case()
    rng = np.random.default_rng(nprobe)
    probes = _distinct_probes(rng, 65, 3, nprobe)
    probes[5, 0] = -1  # names no list
    qd, pd, qkd = _dev(q), _i32(probes), _i32(query_keys)
    for accept in range(8):
        flt = _row_filter(ids, off, row_keys, pad_key=_pad_key(accept, query_keys))
        assert torch.equal(flt.ids, ids)  # no mask: the ids themselves
        want8 = F.flat_search(q, x, labels, 3, probes, 8, row_keys, None, query_keys, accept, s=s64)
        for k in range(1, 9):
            got = index.search_lists(qd, pd, rows, flt.ids, off, k, flt.keys, qkd, accept)
            got_s, got_i = _same(got, (want8[0][:, :k], want8[1][:, :k]), (nprobe, accept, k))
            if accept == 7:  # everything passes: the unkeyed entry's bits
                plain = index.search_lists(qd, pd, rows, ids, off, k)
                assert all(torch.equal(a, b) for a, b in zip(_bits(got), _bits(plain)))
            if accept == 0:
                assert (got_i == -1).all() and np.isneginf(got_s).all()
            ok = got_i >= 0  # every result carries a key that passes
            qk = np.broadcast_to(query_keys[:, None], got_i.shape)[ok]
            cmp = np.sign(row_keys[got_i[ok]].astype(np.int64) - qk)
            assert ((accept >> (cmp + 1)) & 1).all()


# ------------------------------------------------------------------------------------------------------ 2. against the old kernel
@pytest.mark.parametrize("match", ["==", "<"])
def test_keyed_scan_equals_the_unkeyed_scan_on_storage_of_the_allowed_rows(match):
    """No restatement involved: for every distinct query key, the unkeyed `search_lists` on storage built from the masked
    labels, for the queries with that key, has the bits of the keyed result."""
    from sonar_amd import index

    x, q, labels, row_keys, query_keys, _, (rows, ids, off, _) = _small_case()
    accept = F.ACCEPT[match]
    rng = np.random.default_rng(5)
    probes = _distinct_probes(rng, 65, 3, 2)
    flt = _row_filter(ids, off, row_keys, pad_key=_pad_key(accept, query_keys))
    xd, qd = _dev(x), _dev(q)
    for k in (1, 8):
        got = index.search_lists(qd, _i32(probes), rows, flt.ids, off, k, flt.keys, _i32(query_keys), accept)
        for key, sel in F.groups(query_keys, 65):
            lab = F.masked_labels(labels, F.allowed(300, row_keys, None, key, accept))
            r2, i2, o2, _ = index.build_lists(xd, _i32(lab), 3)
            want = index.search_lists(_dev(q[sel]), _i32(probes[sel]), r2, i2, o2, k)
            seld = _dev(sel)
            assert torch.equal(got[0][seld].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1][seld], want[1]), (key, k)


# ------------------------------------------------------------------------------------------------------ 3. one long list
def test_one_long_list_many_tiles_several_units_few_or_no_allowed_rows():
    """4099 rows (13 pad slots), d = 64, 257 queries, k = 8, relation !=.  All rows but seven have key 5: a query with key 5 has
    seven allowed rows (the tail is (-inf, -1)), any other nearly all; with every row's key 5, a query with key 5 has none."""
    from sonar_amd import index

    rng = np.random.default_rng(3)
    x, q = R.integer_rows(rng, 4099, 64), R.integer_rows(rng, 257, 64)
    labels, probes = np.zeros(4099, dtype=np.int64), np.zeros((257, 1), dtype=np.int64)
    row_keys = np.full(4099, 5)
    row_keys[[0, 63, 64, 2047, 4098]], row_keys[[100, 3000]] = 1, -2
    query_keys = np.array([5, 1, -2, 9])[np.arange(257) % 4]
    rows, ids, off, _ = index.build_lists(_dev(x), _i32(labels), 1)
    assert ids.shape[0] == 4112
    s64 = R.scores64(q, x)
    qd, pd, qkd = _dev(q), _i32(probes), _i32(query_keys)
    flt = _row_filter(ids, off, row_keys, pad_key=77)  # 77 != every query key: a pad slot would pass
    want = F.flat_search(q, x, labels, 1, probes, 8, row_keys, None, query_keys, 5, s=s64)
    _, got_i = _same(index.search_lists(qd, pd, rows, flt.ids, off, 8, flt.keys, qkd, 5), want)
    five = query_keys == 5
    assert (got_i[five, 7] == -1).all() and (got_i[five, :7] >= 0).all() and (got_i[~five] >= 0).all()
    assert (np.sort(got_i[five, :7], axis=1) == np.array([0, 63, 64, 100, 2047, 3000, 4098])).all()
    flat = _row_filter(ids, off, np.full(4099, 5), pad_key=77)
    want = F.flat_search(q, x, labels, 1, probes, 8, np.full(4099, 5), None, query_keys, 5, s=s64)
    _, got_i = _same(index.search_lists(qd, pd, rows, flat.ids, off, 8, flat.keys, qkd, 5), want)
    assert (got_i[five] == -1).all() and (got_i[~five] >= 0).all()


# ------------------------------------------------------------------------------------------------------ 4. both unit sizes
def test_planted_ties_with_different_keys_at_both_unit_sizes():
    """3 nq pairs over 4 lists: units of 64 pairs at nq = 66, of 128 at nq = 400.  The planted ties of
    test_planted_ties_across_lists_and_tiles_at_both_unit_sizes -- an all-zero query, copies of a query across lists and
    tiles -- get different keys: among the allowed ties the lower id comes first.  The first 66 queries get the same bits
    in both runs, and a query alone the bits it gets in the batch."""
    from sonar_amd import index

    rng = np.random.default_rng(8)
    n, k_lists = 700, 4
    x, q = R.integer_rows(rng, n, 64), R.integer_rows(rng, 400, 64)
    q[0] = 0
    labels = rng.integers(1, k_lists, n)
    labels[np.arange(0, n, 3)] = 0  # list 0: 234 rows = 4 tiles of 64 slots, 2 of 128
    copies = {3: 0, 300: 0, 699: 0, 50: 1, 333: 1, 598: 2, 20: 3}  # id -> list
    for i, c in copies.items():
        x[i], labels[i] = q[1], c
    row_keys = rng.choice(KEYS, n)
    row_keys[[3, 300, 699, 50, 333, 598]] = [0, 3, 0, 3, 0, 0]  # the copies in the probed lists: four with key 0, two with 3
    query_keys = rng.choice(QKEYS, 400)
    query_keys[0], query_keys[1] = 3, 0
    probes = np.tile([[2, 0, 1]], (400, 1))
    probes[2:] = _distinct_probes(rng, 398, k_lists, 3)
    rows, ids, off, _ = index.build_lists(_dev(x), _i32(labels), k_lists)
    s64 = R.scores64(q, x)
    assert s64[1, 3] == s64[1].max() and (s64[1] == s64[1, 3]).sum() == 7
    qd, pd, qkd = _dev(q), _i32(probes), _i32(query_keys)
    for match in ("==", "!=", ">="):
        accept = F.ACCEPT[match]
        flt = _row_filter(ids, off, row_keys, pad_key=_pad_key(accept, query_keys))
        small = index.search_lists(qd[:66].contiguous(), pd[:66], rows, flt.ids, off, 8, flt.keys, qkd[:66], accept)
        big = index.search_lists(qd, pd, rows, flt.ids, off, 8, flt.keys, qkd, accept)
        want = F.flat_search(q, x, labels, k_lists, probes, 8, row_keys, None, query_keys, accept, s=s64)
        _same(small, (want[0][:66], want[1][:66]), match)
        _, got_i = _same(big, want, match)
        assert all(torch.equal(a[:66], b) for a, b in zip(_bits(big), _bits(small)))
        zero = np.flatnonzero((labels != 3) & F.passes(row_keys, 3, accept))[:8]  # query 0: all ties, the lowest allowed ids
        assert got_i[0].tolist() == zero.tolist()
        tied = [i for i in (3, 50, 300, 333, 598, 699) if F.passes(row_keys[[i]], 0, accept)[0]]
        assert got_i[1, : len(tied)].tolist() == tied and len(tied) == {"==": 4, "!=": 2, ">=": 6}[match]
        for r in (0, 1, 63, 64, 65, 170, 399):
            alone = index.search_lists(qd[r: r + 1].contiguous(), pd[r: r + 1], rows, flt.ids, off, 8, flt.keys, qkd[r: r + 1], accept)
            assert all(torch.equal(a[0], b[r]) for a, b in zip(_bits(alone), _bits(big))), (match, r)


# ------------------------------------------------------------------------------------------------------ 5. d = 1024
def test_d1024_nprobe4():
    from sonar_amd import index

    rng = np.random.default_rng(5)
    x, q = R.integer_rows(rng, 2000, 1024), R.integer_rows(rng, 130, 1024)
    labels, probes = rng.integers(0, 16, 2000), _distinct_probes(rng, 130, 16, 4)
    row_keys, query_keys = rng.choice(KEYS, 2000), rng.choice(QKEYS, 130)
    rows, ids, off, _ = index.build_lists(_dev(x), _i32(labels), 16)
    s64 = R.scores64(q, x)
    for match in ("==", "<="):
        accept = F.ACCEPT[match]
        flt = _row_filter(ids, off, row_keys, pad_key=_pad_key(accept, query_keys))
        got = index.search_lists(_dev(q), _i32(probes), rows, flt.ids, off, 8, flt.keys, _i32(query_keys), accept)
        _same(got, F.flat_search(q, x, labels, 16, probes, 8, row_keys, None, query_keys, accept, s=s64), match)


# ------------------------------------------------------------------------------------------------------ 6. the mask
def test_mask_alone_mask_with_keys_and_tensors_shorter_than_the_ids():
    from sonar_amd import index

    x, q, labels, row_keys, query_keys, s64, (rows, ids, off, _) = _small_case()
    rng = np.random.default_rng(6)
    probes = _distinct_probes(rng, 65, 3, 2)
    mask = rng.random(300) < 0.7
    mask[labels == 1] &= rng.random(int((labels == 1).sum())) < 0.05  # list 1 keeps fewer than 8 rows
    qd, pd, qkd, xd = _dev(q), _i32(probes), _i32(query_keys), _dev(x)
    # the mask alone: the existing entry on the filter's ids = an index built without the masked rows
    flt = _row_filter(ids, off, None, mask)
    assert flt.keys is None
    host_ids, f_ids = ids.cpu().numpy(), flt.ids.cpu().numpy()
    assert np.array_equal(f_ids, np.where((host_ids >= 0) & mask[np.maximum(host_ids, 0)], host_ids, -1))
    got = index.search_lists(qd, pd, rows, flt.ids, off, 8)
    _same(got, F.flat_search(q, x, labels, 3, probes, 8, None, mask, None, 7, s=s64))
    r2, i2, o2, _ = index.build_lists(xd, _i32(np.where(mask, labels, -1)), 3)
    built = index.search_lists(qd, pd, r2, i2, o2, 8)
    assert all(torch.equal(a, b) for a, b in zip(_bits(got), _bits(built)))
    # mask and keys together
    for match in ("==", "!=", ">"):
        accept = F.ACCEPT[match]
        both = _row_filter(ids, off, row_keys, mask, pad_key=_pad_key(accept, query_keys))
        assert torch.equal(both.ids, flt.ids)
        got = index.search_lists(qd, pd, rows, both.ids, off, 8, both.keys, qkd, accept)
        _same(got, F.flat_search(q, x, labels, 3, probes, 8, row_keys, mask, query_keys, accept, s=s64), match)
    # tensors shorter than the largest id: the uncovered rows are out
    for rk, m in ((row_keys[:200], None), (None, mask[:250]), (row_keys[:280], mask[:190])):
        short = _row_filter(ids, off, rk, m, pad_key=INT32_MIN)
        cover = min(len(t) for t in (rk, m) if t is not None)
        f_ids = short.ids.cpu().numpy()
        assert (f_ids < cover).all() and (f_ids >= 0).sum() == ((np.arange(300) < cover) & (True if m is None else np.pad(m, (0, 300 - len(m))))).sum()
        if rk is None:
            got = index.search_lists(qd, pd, rows, short.ids, off, 8)
            _same(got, F.flat_search(q, x, labels, 3, probes, 8, None, m, None, 7, s=s64))
        else:
            got = index.search_lists(qd, pd, rows, short.ids, off, 8, short.keys, qkd, 3)
            _same(got, F.flat_search(q, x, labels, 3, probes, 8, rk, m, query_keys, 3, s=s64))


# ------------------------------------------------------------------------------------------------------ 7. quantised lists
def _quantised_case(nq):
    """The 300 x 128 shape over 3 lists; nq = 65: a unit of 64 and one of one; nq = 256 at nprobe 3: two units of 128 a list."""
    rng = np.random.default_rng(70 + nq)
    x, q = R.integer_rows(rng, 300, 128), R.integer_rows(rng, nq, 128)
    labels = rng.integers(0, 3, 300)
    probes = _distinct_probes(rng, nq, 3, 3 if nq == 256 else 2)
    return rng, x, q, labels, probes, rng.choice(KEYS, 300), rng.choice(QKEYS, nq), rng.random(300) < 0.8


@pytest.mark.parametrize("nq", [65, 256])
def test_int8_lists(nq):
    from sonar_amd import index

    _, x, q, labels, probes, row_keys, query_keys, mask = _quantised_case(nq)
    codes, scales, ids, off, _ = index.build_lists_int8(_dev(x), _i32(labels), 3)
    s = Q.scores(q, x)
    for match, m in (("==", None), ("!=", mask), ("<", None)):
        accept = F.ACCEPT[match]
        flt = _row_filter(ids, off, row_keys, m, pad_key=_pad_key(accept, query_keys))
        got = index.search_lists_int8(_dev(q), _i32(probes), codes, scales, flt.ids, off, 8, flt.keys, _i32(query_keys), accept)
        want = F.search(Q, nq, 300, labels, row_keys, m, query_keys, accept,
                        lambda sel, lab: Q.search(q[sel], x, lab, 3, probes[sel], 8, s=s[sel]))
        _same(got, want, match)
    full = _row_filter(ids, off, row_keys)
    keyed = index.search_lists_int8(_dev(q), _i32(probes), codes, scales, full.ids, off, 8, full.keys, _i32(query_keys), 7)
    plain = index.search_lists_int8(_dev(q), _i32(probes), codes, scales, ids, off, 8)
    assert all(torch.equal(a, b) for a, b in zip(_bits(keyed), _bits(plain)))


@pytest.mark.parametrize("nq,dsub", [(65, 8), (65, 16), (256, 8), (256, 16)])
def test_pq_lists(nq, dsub):
    from sonar_amd import index

    rng, x, q, labels, probes, row_keys, query_keys, mask = _quantised_case(nq)
    cb = P.integer_codebooks(rng, 128, dsub)
    cbd = _dev(cb)
    codes, ids, off, _ = index.build_lists_pq(_dev(x), _i32(labels), 3, cbd)
    row_codes = P.encode(x, cb)
    s64 = R.scores64(q, P.decode(row_codes, cb))
    for match, m in (("==", None), ("!=", mask), (">=", None)):
        accept = F.ACCEPT[match]
        flt = _row_filter(ids, off, row_keys, m, pad_key=_pad_key(accept, query_keys))
        got = index.search_lists_pq(_dev(q), _i32(probes), codes, cbd, flt.ids, off, 8, flt.keys, _i32(query_keys), accept)
        want = F.search(P, nq, 300, labels, row_keys, m, query_keys, accept,
                        lambda sel, lab: P.search(q[sel], row_codes, cb, lab, 3, probes[sel], 8, s=s64[sel]))
        _same(got, want, match)
    full = _row_filter(ids, off, row_keys)
    keyed = index.search_lists_pq(_dev(q), _i32(probes), codes, cbd, full.ids, off, 8, full.keys, _i32(query_keys), 7)
    plain = index.search_lists_pq(_dev(q), _i32(probes), codes, cbd, ids, off, 8)
    assert all(torch.equal(a, b) for a, b in zip(_bits(keyed), _bits(plain)))


@pytest.mark.parametrize("nq", [65, 256])
def test_pq_residual_lists(nq):
    from sonar_amd import index

    rng, x, q, labels, probes, row_keys, query_keys, mask = _quantised_case(nq)
    cb, c = P.integer_codebooks(rng, 128, 8), R.integer_rows(rng, 3, 128)
    coarse = rng.integers(-4, 5, probes.shape).astype(np.float32)  # integer-valued: every sum stays exact
    cbd, cd, coarsed = _dev(cb), _dev(c), _dev(coarse)
    codes, ids, off, _ = index.build_lists_pq_residual(_dev(x), _i32(labels), cd, cbd)
    row_codes = PR.encode(x, labels, c, cb)
    s64 = R.scores64(q, P.decode(row_codes, cb))
    for match, m in (("==", None), ("!=", mask), ("<=", None)):
        accept = F.ACCEPT[match]
        flt = _row_filter(ids, off, row_keys, m, pad_key=_pad_key(accept, query_keys))
        got = index.search_lists_pq_residual(_dev(q), _i32(probes), coarsed, codes, cbd, flt.ids, off, 8, flt.keys,
                                             _i32(query_keys), accept)
        want = F.search(PR, nq, 300, labels, row_keys, m, query_keys, accept,
                        lambda sel, lab: PR.search(q[sel], row_codes, cb, lab, 3, probes[sel], coarse[sel], 8, s=s64[sel]))
        _same(got, want, match)
    full = _row_filter(ids, off, row_keys)
    keyed = index.search_lists_pq_residual(_dev(q), _i32(probes), coarsed, codes, cbd, full.ids, off, 8, full.keys, _i32(query_keys), 7)
    plain = index.search_lists_pq_residual(_dev(q), _i32(probes), coarsed, codes, cbd, ids, off, 8)
    assert all(torch.equal(a, b) for a, b in zip(_bits(keyed), _bits(plain)))


# ------------------------------------------------------------------------------------------------------ 8. range search
def _thresholds(s64, allowed_of, probes, labels, k_lists):
    """fp32 [nq]: by query number the score of one of its allowed candidates (high, middle or low in their order), 0, a
    negative value or -inf, as in tests/test_gpu_ivf_range.py."""
    thr = np.zeros(len(probes), dtype=np.float32)
    for r, row in enumerate(probes):
        mode = ("own", "own", 0.0, "own", -3.0, -np.inf)[r % 6]
        if mode == "own":
            cand = [np.flatnonzero((labels == c) & allowed_of(r)) for c in row if 0 <= c < k_lists]
            sc = np.sort(s64[r, np.concatenate(cand)])[::-1] if cand else np.zeros(0)
            thr[r] = sc[min(len(sc) - 1, (len(sc) * (1, 8, 20)[r % 3]) // 32)] if len(sc) else 0.0
        else:
            thr[r] = mode
    return thr


@pytest.mark.parametrize("nq", [66, 400])
def test_range_search_at_both_unit_sizes(nq):
    from sonar_amd import index

    rng = np.random.default_rng(80)
    n, k_lists = 700, 4
    x, q = R.integer_rows(rng, n, 64), R.integer_rows(rng, nq, 64)
    q[0] = 0
    labels = rng.integers(0, k_lists, n)
    probes = _distinct_probes(rng, nq, k_lists, 3)
    row_keys, query_keys, mask = rng.choice(KEYS, n), rng.choice(QKEYS, nq), rng.random(n) < 0.8
    rows, ids, off, _ = index.build_lists(_dev(x), _i32(labels), k_lists)
    s64 = R.scores64(q, x)
    qd, pd, qkd = _dev(q), _i32(probes), _i32(query_keys)
    for match, m in (("==", None), ("!=", mask), ("<", None)):
        accept = F.ACCEPT[match]
        thr = _thresholds(s64, lambda r: F.allowed(n, row_keys, m, query_keys[r], accept), probes, labels, k_lists)
        flt = _row_filter(ids, off, row_keys, m, pad_key=_pad_key(accept, query_keys))
        td = _dev(thr)
        res = index.range_search_lists(qd, pd, td, rows, flt.ids, off, True, None, flt.keys, qkd, accept)
        raw = index.range_search_lists(qd, pd, td, rows, flt.ids, off, False, None, flt.keys, qkd, accept)
        want_l, want_s, want_i = F.range_search(q, x, labels, k_lists, probes, thr, row_keys, m, query_keys, accept, s=s64)
        got_l, got_s, got_i = (t.cpu().numpy() for t in res)
        assert np.array_equal(got_l, want_l), (match, np.flatnonzero(np.diff(got_l) != np.diff(want_l))[:5])
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s.astype(np.float64), want_s) and (got_i >= 0).all()
        raw_l, raw_s, raw_i = (t.cpu().numpy() for t in raw)
        assert np.array_equal(raw_l, want_l)
        order = np.lexsort((raw_i, -raw_s.astype(np.float64), np.repeat(np.arange(nq), np.diff(raw_l))))
        assert np.array_equal(raw_i[order], want_i) and np.array_equal(raw_s[order].astype(np.float64), want_s)
        # the head of every segment is the keyed search(k = 8) cut at the threshold
        s8, i8 = (t.cpu().numpy() for t in index.search_lists(qd, pd, rows, flt.ids, off, 8, flt.keys, qkd, accept))
        for r in range(nq):
            keep = (i8[r] >= 0) & (s8[r] >= thr[r])
            k = min(8, int(got_l[r + 1] - got_l[r]))
            assert int(keep.sum()) == k and keep[:k].all(), (match, r)
            seg = slice(got_l[r], got_l[r] + k)
            assert np.array_equal(got_s[seg].view(np.int32), s8[r, :k].view(np.int32)) and np.array_equal(got_i[seg], i8[r, :k]), (match, r)
        if match == "==":  # everything passes: the unkeyed entries' bits
            all_keys = _row_filter(ids, off, row_keys)
            a = index.range_search_lists(qd, pd, td, rows, ids, off)
            b = index.range_search_lists(qd, pd, td, rows, all_keys.ids, off, True, None, all_keys.keys, qkd, 7)
            assert all(torch.equal(u, v) for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------------ 9. the Python surface
@functools.lru_cache(maxsize=None)
def _planted():
    from sonar_amd import xsim
    from sonar_amd.index import IVFFlatIndex

    n, k, d, nq = 4000, 16, 256, 200
    x, labels, centres, _, target = R.planted(n, k, d, nq, seed=11)
    xd = _dev(x)
    ix = IVFFlatIndex(_dev(centres.astype(np.float32))).add(xd, _i32(labels))
    xn = xsim.normalize_rows(xd)[:n].cpu().numpy().astype(np.float64)
    return ix, xd, xn, labels, target


def test_corpus_rows_against_their_own_index_never_return_themselves():
    """The queries are corpus rows; row_keys = arange(n), query_keys = the queries' own row numbers, `!=`."""
    ix, xd, xn, labels, target = _planted()
    n, d, nq, k, nprobe = 4000, 256, 200, 8, 2
    tol = d * 2.0 ** -23
    td = _dev(target)
    qd = xd[td].contiguous()
    s64 = xn[target] @ xn.T
    plain_s, plain_i = ix.search(qd, k=k, nprobe=nprobe)
    assert torch.equal(plain_i[:, 0], td.to(torch.int32))  # unfiltered, every query finds itself first
    probes = ix.probe(qd, nprobe)
    rows = ix.row_filter(keys=torch.arange(n, dtype=torch.int32, device="cuda"))
    got = ix.search(qd, k=k, probes=probes, rows=rows, query_keys=td.to(torch.int32), match="!=")
    assert all(torch.equal(a, b) for a, b in zip(got, ix.search(qd, k=k, nprobe=nprobe, rows=rows, query_keys=td.to(torch.int32), match="!=")))
    sc, idx = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert (idx >= 0).all() and (idx != target[:, None]).all()
    r = np.arange(nq)[:, None]
    assert np.abs(sc - s64[r, idx]).max() <= tol
    probed = (labels[None, None, :] == probes.cpu().numpy()[:, :, None]).any(axis=1)
    probed[np.arange(nq), target] = False  # the allowed rows of the probed lists
    best = np.where(probed, s64, -np.inf).max(axis=1)
    assert (sc[:, 0] >= best - tol).all() and (np.diff(sc, axis=1) <= 0).all()
    # the k - 1 results behind the query itself are the filtered search's first k - 1
    assert torch.equal(plain_i[:, 1:], got[1][:, : k - 1]) and torch.equal(plain_s[:, 1:].view(torch.int32), got[0][:, : k - 1].view(torch.int32))
    # language keys i % 4 and ==: every result has the query's key
    lang = torch.arange(n, dtype=torch.int32, device="cuda") % 4
    rows = ix.row_filter(keys=lang)
    sc, idx = ix.search(qd, k=k, nprobe=nprobe, rows=rows, query_keys=lang[td])
    idx = idx.cpu().numpy()
    assert (idx >= 0).all() and (idx % 4 == (target % 4)[:, None]).all() and (idx[:, 0] == target).all()
    # a mask: every other run of 16 rows does not exist (row i is in cluster i % 16: every list keeps half of its rows); with
    # keys and a date-like cut-off on top
    mask = torch.arange(n, device="cuda") // 16 % 2 == 0
    even = ix.row_filter(mask=mask)
    idx = ix.search(qd, k=k, nprobe=nprobe, rows=even)[1].cpu().numpy()
    assert (idx >= 0).all() and (idx // 16 % 2 == 0).all()
    dated = ix.row_filter(keys=torch.arange(n, dtype=torch.int32, device="cuda"), mask=mask)
    res = ix.range_search(qd, 0.45, nprobe=1, rows=dated, query_keys=td.to(torch.int32), match="<")
    lims, ids = res.lims.cpu().numpy(), res.ids.cpu().numpy()
    for j in range(nq):  # the rows of the query's list at or above 0.45, below the query's own number, visible rows only
        cand = (labels == labels[target[j]]) & (np.arange(n) < target[j]) & (np.arange(n) // 16 % 2 == 0)
        assert np.abs(s64[j, cand] - 0.45).min(initial=1.0) > tol, j  # no candidate within the fp32 bound of the threshold
        assert np.array_equal(np.sort(ids[lims[j]: lims[j + 1]]), np.flatnonzero(cand & (s64[j] >= 0.45))), j


def test_refine_composes_on_the_quantised_indexes():
    from sonar_amd import xsim
    from sonar_amd.index import IVFInt8Index, IVFPQIndex, IVFPQResidualIndex, refine_candidates

    n, k_lists, d, nq = 2000, 8, 128, 70
    x, labels, centres, q, target = R.planted(n, k_lists, d, nq, seed=3)
    xd, qd, cen = _dev(x), _dev(q), _dev(centres.astype(np.float32))
    xn = xsim.normalize_rows(xd)
    keys = torch.arange(n, dtype=torch.int32, device="cuda") % 3
    qk = _i32(target % 3)
    cb = IVFPQIndex.train(xd, k_lists, dsub=8, n_iter=2, pq_iter=2).codebooks
    for ix in (IVFInt8Index(cen), IVFPQIndex(cen, cb), IVFPQResidualIndex(cen, cb)):
        ix.add(xd, _i32(labels))
        rows = ix.row_filter(keys=keys)
        raw = ix.search(qd, k=8, nprobe=2, rows=rows, query_keys=qk, match="!=")
        fine = ix.search(qd, k=8, nprobe=2, rows=rows, query_keys=qk, match="!=", refine=xn)
        idx = raw[1].cpu().numpy()
        assert (idx >= 0).all() and (idx % 3 != (target % 3)[:, None]).all()
        want = refine_candidates(xsim.normalize_rows(qd), nq, xn, raw[1])
        assert all(torch.equal(a, b) for a, b in zip(_bits(fine), _bits(want)))
        assert torch.equal(torch.sort(fine[1], dim=1)[0], torch.sort(raw[1], dim=1)[0])


# ------------------------------------------------------------------------------------------------------ 10. capture
def test_a_keyed_search_is_capturable():
    ix, xd, _, _, target = _planted()
    td = _dev(target)
    qd = xd[td].contiguous()
    rows = ix.row_filter(keys=torch.arange(4000, dtype=torch.int32, device="cuda"))
    qk = td.to(torch.int32)
    eager = ix.search(qd, k=4, nprobe=2, rows=rows, query_keys=qk, match="!=")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ix.search(qd, k=4, nprobe=2, rows=rows, query_keys=qk, match="!=")  # warm-up: the one-time attribute calls
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ix.search(qd, k=4, nprobe=2, rows=rows, query_keys=qk, match="!=")
    out[0].fill_(0), out[1].fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(_bits(out), _bits(eager)))
