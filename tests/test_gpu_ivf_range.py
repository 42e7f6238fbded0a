"""GPU: the range search over the IVF-Flat lists (sonar_amd/csrc/ivf.hip, sonar_amd/index.py) against the
numpy restatement in tests/ivf_range_ref.py.

Operands of the exact cases have entries from {-1, 0, 1} (ivf_ref.integer_rows): every score is a small integer, exact in fp32
in any order, so lims, scores and ids must equal the restatement bit for bit.  A query's threshold is one of its own
candidates' scores (equality at the threshold is the rule's edge), or 0 (the pad slots and the empty unit rows score exactly
0 and must not appear), a negative value or -inf (every row of the probed lists), by query number.  The shapes are the
smallest that reach each path of the unit: one tile and many, one unit and several, units of 64 and of 128 pairs, the
boundaries of the inversion's one-block scan.  On real-valued planted rows the margins around the two thresholds are asserted
on the CPU (tests/test_ivf_range_cpu.py) to be orders of magnitude above the fp32 accumulation bound d * 2^-23."""
import functools

import numpy as np
import pytest
import torch

from tests import ivf_range_ref as G
from tests import ivf_ref as R

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
A = R.ALIGN
OWN, ZERO, NEG, ALL = "own", 0.0, -3.0, -np.inf  # what a query's threshold is


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i32(a):
    return _dev(np.asarray(a, dtype=np.int32))


def _candidates(labels, k_lists, row):
    labels = np.asarray(labels)
    cand = [np.flatnonzero(labels == c) for c in row if 0 <= c < k_lists]
    return np.concatenate(cand) if cand else np.zeros(0, dtype=np.int64)


def _thresholds(s64, labels, k_lists, probes, modes=(OWN, OWN, ZERO, OWN, NEG, ALL)):
    """fp32 [nq]: query r takes modes[r % len(modes)]; OWN: the score of one of its candidates, high in their order for one
    query, in the middle or low for the next (0 where it has none)."""
    thr = np.zeros(len(probes), dtype=np.float32)
    for r, row in enumerate(probes):
        mode = modes[r % len(modes)]
        if mode is OWN:
            sc = np.sort(s64[r, _candidates(labels, k_lists, row)])[::-1]
            thr[r] = sc[min(len(sc) - 1, (len(sc) * (1, 8, 20)[r % 3]) // 32)] if len(sc) else 0.0
        else:
            thr[r] = mode
    return thr


def _host(res):
    lims, sc, ids = (t.cpu().numpy() for t in res)
    assert lims.dtype == np.int64 and sc.dtype == np.float32 and ids.dtype == np.int32
    assert sc.shape == ids.shape == (int(lims[-1]),) and lims[0] == 0
    return lims, sc, ids


def _check_range(x, labels, k_lists, q, probes, thr, storage=None, cross=False):
    """lims, scores and ids equal the restatement; with sort=False the same lims and the same segments as multisets; cross:
    the head of every segment is `search_lists(k = 8)` cut at the threshold, bit for bit.  x / q: integer-valued fp16."""
    from sonar_amd import index

    storage = storage or index.build_lists(_dev(x), _i32(labels), k_lists)
    rows, ids, off, _ = storage
    s64 = R.scores64(q, x)
    assert np.abs(s64).max() < 2 ** 11 and np.array_equal(s64, np.rint(s64))
    thr = np.asarray(thr, dtype=np.float32)
    qd, pd, td = _dev(q), _i32(probes), _dev(thr)
    res = index.range_search_lists(qd, pd, td, rows, ids, off)
    raw = index.range_search_lists(qd, pd, td, rows, ids, off, sort=False)
    torch.cuda.synchronize()
    assert isinstance(res, index.RangeResult) and torch.equal(res.counts, res.lims[1:] - res.lims[:-1])
    want_l, want_s, want_i = G.range_search(q, x, labels, k_lists, probes, thr, s=s64)
    got_l, got_s, got_i = _host(res)
    assert np.array_equal(got_l, want_l), (np.flatnonzero(np.diff(got_l) != np.diff(want_l))[:5], np.diff(got_l)[:8], np.diff(want_l)[:8])
    bad = np.flatnonzero((got_i != want_i) | (got_s.astype(np.float64) != want_s))
    assert len(bad) == 0, (bad[:5], got_i[bad[:5]], want_i[bad[:5]], got_s[bad[:5]], want_s[bad[:5]])
    assert (got_i >= 0).all()  # no pad slot, ever
    raw_l, raw_s, raw_i = _host(raw)
    assert np.array_equal(raw_l, want_l)
    query = np.repeat(np.arange(len(q)), np.diff(raw_l))
    order = np.lexsort((raw_i, -raw_s.astype(np.float64), query))  # every segment into the total order, on the host
    assert np.array_equal(raw_i[order], want_i) and np.array_equal(raw_s[order].astype(np.float64), want_s)
    if cross:
        s8, i8 = index.search_lists(qd, pd, rows, ids, off, 8)
        s8, i8 = s8.cpu().numpy(), i8.cpu().numpy()
        for r in range(len(q)):
            keep = (i8[r] >= 0) & (s8[r] >= thr[r])
            m = min(8, int(got_l[r + 1] - got_l[r]))
            assert int(keep.sum()) == m and keep[:m].all(), r
            seg = slice(got_l[r], got_l[r] + m)
            assert np.array_equal(got_s[seg].view(np.int32), s8[r, :m].view(np.int32)) and np.array_equal(got_i[seg], i8[r, :m]), r
    return storage, (got_l, got_s, got_i)


def _distinct_probes(rng, nq, k_lists, nprobe):
    return np.stack([rng.permutation(k_lists)[:nprobe] for _ in range(nq)])


# ------------------------------------------------------------------------------------------------------ 1. exact cases
def test_one_row_one_list_at_above_and_below_its_score():
    rng = np.random.default_rng(1)
    x = R.integer_rows(rng, 1, 64)
    x[0, 0] = 1
    q = np.repeat(x, 6, axis=0)
    q[3:] = 0  # the row scores 0 against these, and so do the list's 15 pad slots
    s = float(R.scores64(q[:1], x)[0, 0])
    assert s >= 1
    thr = np.array([s, np.nextafter(np.float32(s), np.float32(np.inf)), -np.inf, 0.0, np.nextafter(np.float32(0), np.float32(1)),
                    -np.inf], dtype=np.float32)
    _, (lims, sc, ids) = _check_range(x, [0], 1, q, np.zeros((6, 1)), thr)
    assert np.diff(lims).tolist() == [1, 0, 1, 1, 0, 1] and (ids == 0).all() and sc.tolist() == [s, s, 0.0, 0.0]


def test_a_unit_of_64_pairs_and_a_unit_of_one_every_nprobe():
    rng = np.random.default_rng(2)
    x, q = R.integer_rows(rng, 300, 128), R.integer_rows(rng, 65, 128)
    labels = rng.integers(0, 3, 300)
    s64, storage = R.scores64(q, x), None
    for nprobe in (1, 2, 3):
        probes = _distinct_probes(rng, 65, 3, nprobe)
        thr = _thresholds(s64, labels, 3, probes)
        storage, (lims, _, _) = _check_range(x, labels, 3, q, probes, thr, storage, cross=True)
        sizes = np.bincount(labels, minlength=3)
        for r in np.flatnonzero(thr == -np.inf):  # the sum of the probed lists' sizes: no pad slot, no empty unit row
            assert lims[r + 1] - lims[r] == sizes[probes[r]].sum()


def test_one_long_list_many_tiles_several_units():
    rng = np.random.default_rng(3)
    x, q = R.integer_rows(rng, 4099, 64), R.integer_rows(rng, 257, 64)  # 4112 slots, 13 of them pads
    labels, probes = np.zeros(4099, dtype=np.int64), np.zeros((257, 1), dtype=np.int64)
    thr = _thresholds(None, labels, 1, probes, modes=(ZERO, ALL))
    _, (lims, _, _) = _check_range(x, labels, 1, q, probes, thr)
    assert (np.diff(lims)[1::2] == 4099).all()


# the list count walks the boundaries of the inversion's one-block scan (csrc/bucket.hpp), as in tests/test_gpu_ivf.py
@pytest.mark.parametrize("k_lists", [255, 256, 257, 513, 300])
def test_empty_lists_entries_that_name_no_list_and_lists_named_twice(k_lists):
    rng = np.random.default_rng(4)
    x, q = R.integer_rows(rng, 4099, 64), R.integer_rows(rng, 300, 64)
    labels = rng.integers(0, k_lists, 4099)
    labels[labels % 5 == 0] += 1  # every fifth list stays empty (at 256 lists the rows of list 255 get no list at all)
    labels[:40] = np.arange(40) % 2 * 2 + 1
    probes = _distinct_probes(rng, 300, k_lists, 8)
    probes[10:15] = np.arange(0, 40, 5).reshape(1, 8)  # queries that probe empty lists only, between non-empty neighbours
    probes[15, :] = [0, 5, 10, 15, 20, 25, 30, 7]
    probes[20, :3], probes[21, 7], probes[22, 0] = -1, k_lists, INT32_MAX
    probes[23] = -1
    probes[24] = [1, 3, 1, 3, 1, 6, 7, 1]  # lists named twice and more: their hits as often
    s64 = R.scores64(q, x)
    thr = _thresholds(s64, labels, k_lists, probes)
    thr[10], thr[11], thr[23], thr[24] = -np.inf, 0.0, -np.inf, -np.inf
    storage, (lims, _, ids) = _check_range(x, labels, k_lists, q, probes, thr)
    assert (np.diff(lims)[10:15] == 0).all() and lims[10] > 0 and lims[-1] > lims[15] and lims[24] == lims[23]
    sizes = np.bincount(labels, minlength=k_lists)
    assert lims[25] - lims[24] == 4 * sizes[1] + 2 * sizes[3] + sizes[6] + sizes[7]
    assert np.bincount(ids[lims[24]: lims[25]], minlength=4099)[labels == 1].tolist() == [4] * sizes[1]
    # no pair at all: the walk has no unit, the total is 0 and the second pass is skipped
    none = np.full((300, 2), -1)
    _, (lims, sc, ids) = _check_range(x, labels, k_lists, q, none, np.full(300, -np.inf), storage)
    assert (lims == 0).all() and len(sc) == len(ids) == 0


def test_d1024_nprobe4():
    rng = np.random.default_rng(5)
    x, q = R.integer_rows(rng, 2000, 1024), R.integer_rows(rng, 130, 1024)
    labels, probes = rng.integers(0, 16, 2000), _distinct_probes(rng, 130, 16, 4)
    _check_range(x, labels, 16, q, probes, _thresholds(R.scores64(q, x), labels, 16, probes), cross=True)


def test_planted_ties_across_lists_and_tiles_at_both_unit_sizes():
    """3 nq pairs over 4 lists: units of 64 pairs at nq = 66, of 128 at nq = 400 (csrc/ivf.hip, unit_pairs).  The planted ties
    of tests/test_gpu_ivf.py: an all-zero query (every candidate ties at 0) and copies of a query in different lists and
    tiles; the first 66 queries of both runs are the same and must get the same bits."""
    rng = np.random.default_rng(8)
    n, k_lists = 700, 4
    x, q = R.integer_rows(rng, n, 64), R.integer_rows(rng, 400, 64)
    q[0] = 0
    labels = rng.integers(1, k_lists, n)
    labels[np.arange(0, n, 3)] = 0  # list 0: 234 rows = 4 tiles of 64 slots, 2 of 128
    copies = {3: 0, 300: 0, 699: 0, 50: 1, 333: 1, 598: 2, 20: 3}  # id -> list
    for i, c in copies.items():
        x[i], labels[i] = q[1], c
    probes = np.tile([[2, 0, 1]], (400, 1))
    probes[2:] = _distinct_probes(rng, 398, k_lists, 3)
    s64 = R.scores64(q, x)
    thr = _thresholds(s64, labels, k_lists, probes)
    thr[0], thr[1] = 0.0, s64[1, 3]  # every row of lists 0, 1, 2 at score 0; the six copies in those lists
    storage, small = _check_range(x, labels, k_lists, q[:66], probes[:66], thr[:66], cross=True)
    _, big = _check_range(x, labels, k_lists, q, probes, thr, storage, cross=True)
    lims, sc, ids = small
    assert ids[: lims[1]].tolist() == np.flatnonzero(labels != 3).tolist() and (sc[: lims[1]] == 0).all()
    assert ids[lims[1]: lims[2]].tolist() == [3, 50, 300, 333, 598, 699]
    m = lims[66]
    assert np.array_equal(big[0][:67], lims) and np.array_equal(big[1][:m].view(np.int32), sc.view(np.int32))
    assert np.array_equal(big[2][:m], ids)


# ------------------------------------------------------------------------------------------------------ 2. misuse
def test_thresholds_lowered_between_the_passes_write_inside_their_segments_only():
    """smi_range_search_emit with more hits than smi_range_search_count counted: the surplus is lost, every written entry is
    a hit of the pair whose segment it is in, and nothing around the output or behind `total` is touched."""
    from sonar_amd import _lib, index

    rng = np.random.default_rng(12)
    n, k_lists, nq, nprobe, d, pad = 900, 5, 70, 3, 64, 4096
    x, q = R.integer_rows(rng, n, d), R.integer_rows(rng, nq, d)
    labels = rng.integers(0, k_lists, n)
    labels[labels == 2] = -1  # an empty list: pairs without a segment between the others
    probes = _distinct_probes(rng, nq, k_lists, nprobe)
    probes[5, 1] = -1
    s64 = R.scores64(q, x)
    thr = _thresholds(s64, labels, k_lists, probes, modes=(OWN,))
    thr[7] = np.inf  # a query without any segment
    rows, ids, off, _ = index.build_lists(_dev(x), _i32(labels), k_lists)
    lib = _lib.load()
    ws_bytes = lib.smi_range_search_ws_bytes(nq, k_lists, nprobe, d)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    qd, pd, td = _dev(q), _i32(probes), _dev(thr)
    counts = torch.empty(nq * nprobe, dtype=torch.int32, device="cuda")

    def inputs(t):
        return (qd.data_ptr(), nq, d, pd.data_ptr(), nprobe, t.data_ptr(), rows.data_ptr(), ids.data_ptr(), off.data_ptr(), k_lists)

    stream = _lib.current_stream_ptr()
    _lib.check(lib.smi_range_search_count(*inputs(td), counts.data_ptr(), ws.data_ptr(), ws_bytes, stream))
    base = torch.zeros(nq * nprobe + 1, dtype=torch.int64, device="cuda")
    base[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(base[-1].item())
    want = G.range_search(q, x, labels, k_lists, probes, thr, s=s64)
    assert total == want[0][-1] > 0
    SENT_S, SENT_I, tail = 12345.0, -7, 64
    score = torch.full((pad + total + tail + pad,), SENT_S, dtype=torch.float32, device="cuda")
    idx = torch.full((pad + total + tail + pad,), SENT_I, dtype=torch.int32, device="cuda")
    low = torch.full((nq,), -np.inf, dtype=torch.float32, device="cuda")  # every row of every probed list is a hit now
    _lib.check(lib.smi_range_search_emit(*inputs(low), base.data_ptr(), total, score[pad:].data_ptr(), idx[pad:].data_ptr(),
                                         ws.data_ptr(), ws_bytes, stream))
    torch.cuda.synchronize()
    score, idx, base = score.cpu().numpy(), idx.cpu().numpy(), base.cpu().numpy()
    assert (score[:pad] == SENT_S).all() and (idx[:pad] == SENT_I).all()
    assert (score[pad + total:] == SENT_S).all() and (idx[pad + total:] == SENT_I).all()
    score, idx = score[pad: pad + total], idx[pad: pad + total]
    assert (idx != SENT_I).all()  # every pair has at least as many hits as its segment holds: all of it is written
    for j in range(nq * nprobe):
        r, c = divmod(j, nprobe)
        seg = slice(base[j], base[j + 1])
        if base[j + 1] > base[j]:
            assert 0 <= probes[r, c] < k_lists and (labels[idx[seg]] == probes[r, c]).all(), j
            assert np.array_equal(score[seg].astype(np.float64), s64[r, idx[seg]]), j
            assert len(set(idx[seg].tolist())) == base[j + 1] - base[j], j


# ------------------------------------------------------------------------------------------------------ 3. determinism
def test_two_runs_and_a_query_alone_give_the_same_bits():
    from sonar_amd import index

    rng = np.random.default_rng(13)
    n, k_lists, nq = 1500, 6, 300
    x, q = R.integer_rows(rng, n, 128), R.integer_rows(rng, nq, 128)
    labels, probes = rng.integers(0, k_lists, n), _distinct_probes(rng, nq, k_lists, 3)
    thr = _thresholds(R.scores64(q, x), labels, k_lists, probes)
    rows, ids, off, _ = index.build_lists(_dev(x), _i32(labels), k_lists)
    qd, pd, td = _dev(q), _i32(probes), _dev(thr)
    one = index.range_search_lists(qd, pd, td, rows, ids, off)
    two = index.range_search_lists(qd, pd, td, rows, ids, off)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    lims = one.lims.cpu().numpy()
    for r in (0, 1, 63, 64, 170, 299):  # alone: a unit of 64 pairs with one row, at another position
        alone = index.range_search_lists(qd[r: r + 1].contiguous(), pd[r: r + 1], td[r: r + 1], rows, ids, off)
        seg = slice(lims[r], lims[r + 1])
        assert alone.lims.tolist() == [0, lims[r + 1] - lims[r]], r
        assert torch.equal(alone.scores.view(torch.int32), one.scores[seg].view(torch.int32)) and torch.equal(alone.ids, one.ids[seg]), r


# ------------------------------------------------------------------------------------------------------ 4. real-valued data
@functools.lru_cache(maxsize=None)
def _planted(n, k, d, nq):
    from sonar_amd import xsim
    from sonar_amd.index import IVFFlatIndex

    x, labels, centres, q, target = R.planted(n, k, d, nq, seed=11)
    xd, qd = _dev(x), _dev(q)
    ix = IVFFlatIndex(_dev(centres.astype(np.float32))).add(xd, _i32(labels))
    xn = xsim.normalize_rows(xd)[:n].cpu().numpy().astype(np.float64)
    qn = xsim.normalize_rows(qd)[:nq].cpu().numpy().astype(np.float64)
    return ix, qd, qn @ xn.T, labels, target


@pytest.mark.parametrize("n,k,d,nq", [(4000, 16, 256, 200), (3000, 12, 1024, 130)])
def test_planted_rows_the_neighbour_alone_and_the_whole_cluster(n, k, d, nq):
    ix, qd, s64, labels, target = _planted(n, k, d, nq)
    tol = d * 2.0 ** -23
    near = ix.range_search(qd, 0.9)
    lims, sc, ids = _host(near)
    assert np.array_equal(lims, np.arange(nq + 1)) and np.array_equal(ids, target)
    assert np.abs(sc - s64[np.arange(nq), target]).max() <= tol
    as_tensor = ix.range_search(qd, torch.full((nq,), 0.9, dtype=torch.float32, device="cuda"))
    assert all(torch.equal(a, b) for a, b in zip(near, as_tensor))
    cluster = ix.range_search(qd, 0.45, nprobe=1)
    lims, sc, ids = _host(cluster)
    assert np.array_equal(lims, np.arange(nq + 1) * (n // k)) and cluster.counts.tolist() == [n // k] * nq
    for r in range(nq):
        seg = slice(lims[r], lims[r + 1])
        assert np.array_equal(np.sort(ids[seg]), np.flatnonzero(labels == labels[target[r]])), r
        assert np.abs(sc[seg] - s64[r, ids[seg]]).max() <= tol, r
        assert ((np.diff(sc[seg]) < 0) | ((np.diff(sc[seg]) == 0) & (np.diff(ids[seg]) > 0))).all(), r
        assert ids[lims[r]] == target[r]
    total = int(lims[-1])
    with pytest.raises(ValueError, match=f"{total} hits, max_total = {total - 1}"):
        ix.range_search(qd, 0.45, max_total=total - 1)
    assert torch.equal(ix.range_search(qd, 0.45, max_total=total).ids, cluster.ids)
