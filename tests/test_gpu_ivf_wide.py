"""GPU: the paged search of the IVF-Flat index (smi_ivf_search_page; index.search_lists_page, IVFFlatIndex.search_page /
search_wide, probe_wide) against the restatement in tests/topk_wide_ref.py.

Exact equality of scores AND ids everywhere: the list-level tests run on the integer rows of tests/ivf_ref.py (entries from
{-1, 0, 1}: every fp32 sum is an exact small integer), the class-level ones, which normalise, on rows with 16 entries of +-1
(the norm is 4, the unit row has entries +-0.25 and every score is a multiple of 1/16, exact in any order)."""
import numpy as np
import pytest
import torch

from tests import ivf_ref as R
from tests import topk_wide_ref as W

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i32(a):
    return _dev(np.asarray(a, dtype=np.int32))


def _same(got_s, got_i, want_s, want_i, what=""):
    got_s, got_i = got_s.cpu().numpy(), got_i.cpu().numpy()
    assert got_s.dtype == np.float32 and got_i.dtype == np.int32 and got_s.shape == got_i.shape == want_i.shape, what
    bad = np.flatnonzero((got_i != want_i).any(axis=1) | (got_s.astype(np.float64) != want_s).any(axis=1))
    assert len(bad) == 0, (what, bad[:5], got_i[bad[:2]], want_i[bad[:2]], got_s[bad[:2]], want_s[bad[:2]])


def _lists_wide(qd, pd, rows, ids, off, k):
    """The pages of search_lists_page chained, as IVFFlatIndex.search_wide chains them."""
    from sonar_amd import index, xsim

    pages, below = [], None
    for kp in xsim.page_sizes(k):
        pages.append(index.search_lists_page(qd, pd, rows, ids, off, kp, below))
        below = xsim.last_entry(*pages[-1])
    torch.cuda.synchronize()
    return torch.cat([p[0] for p in pages], 1), torch.cat([p[1] for p in pages], 1)


def _check_lists(x, labels, k_lists, q, probes, ks, visible=None):
    """Scores and ids of every query equal the restatement, for every k of ks.  x / q: integer-valued fp16."""
    from sonar_amd import index

    rows, ids, off, _ = index.build_lists(_dev(x), _i32(labels), k_lists)
    if visible is not None:
        ids = index.slot_filter(ids, off, None, _dev(visible)).ids
    s64 = R.scores64(q, x)
    assert np.abs(s64).max() < 2 ** 11 and np.array_equal(s64, np.rint(s64))
    qd, pd = _dev(q), _i32(probes)
    for k in ks:
        want_s, want_i = W.search_wide(s64, labels, k_lists, probes, k, visible)
        _same(*_lists_wide(qd, pd, rows, ids, off, k), want_s, want_i, k)
    return s64


def _distinct_probes(rng, nq, k_lists, nprobe):
    return np.stack([rng.permutation(k_lists)[:nprobe] for _ in range(nq)])


# ------------------------------------------------------------------------------------------------- 1. the lists, exact
@pytest.mark.parametrize("nq", [66, 400])  # units of 64 pairs (two of them); units of 128: nq * nprobe >= 256 K
def test_page_scan_of_one_list_at_both_unit_sizes(nq):
    """One list of 295 of 300 rows (a third 128-slot tile with 39 of them), k at, behind and far behind a page."""
    rng = np.random.default_rng(nq)
    x, q = R.integer_rows(rng, 300, 128), R.integer_rows(rng, nq, 128)
    labels = np.zeros(300, dtype=np.int64)
    labels[[7, 100, 101, 250, 299]] = [-1, 1, 2, INT32_MAX, -1]
    s64 = _check_lists(x, labels, 1, q, np.zeros((nq, 1), dtype=np.int64), (16, 17, 64))
    # the condition on the inputs: the tie-break decides at the page boundaries in most rows
    vals = W.first_k(np.where((labels == 0)[None, :], s64, -np.inf), 50)[0]
    for a in (16, 32, 48):
        assert (vals[:, a - 1] == vals[:, a]).mean() >= 0.5, a


@pytest.mark.parametrize("nprobe", [9, 12])
def test_twelve_lists_and_every_list_probed_is_brute_force(nprobe):
    from sonar_amd import xsim

    rng = np.random.default_rng(40 + nprobe)
    x, q = R.integer_rows(rng, 600, 128), R.integer_rows(rng, 100, 128)
    labels = rng.integers(0, 12, 600)
    probes = _distinct_probes(rng, 100, 12, nprobe)
    s64 = _check_lists(x, labels, 12, q, probes, (16, 40))
    if nprobe == 12:
        for k in (16, 40):
            want_s, want_i = W.search_wide(s64, labels, 12, probes, k)
            bf = W.first_k(s64, k)
            assert np.array_equal(bf[0], want_s) and np.array_equal(bf[1], want_i)
            xn = torch.zeros((768, 128), dtype=torch.float16)
            xn[:600] = torch.from_numpy(x)
            qn = torch.zeros((256, 128), dtype=torch.float16)
            qn[:100] = torch.from_numpy(q)
            s, i = xsim.topk_wide_normalized(qn.cuda(), 100, xn.cuda(), 600, k)
            torch.cuda.synchronize()
            _same(s, i, want_s, want_i, ("topk_wide_normalized", k))


def test_lists_of_three_rows_fill_tails_and_partly_filled_parts():
    rng = np.random.default_rng(3)
    x, q = R.integer_rows(rng, 600, 128), R.integer_rows(rng, 300, 128)
    short = np.where(np.arange(600) < 36, np.arange(600) % 12, -1)
    probes = _distinct_probes(rng, 300, 12, 9)  # 27 candidates a query: the second page runs out, the third is fill
    _check_lists(x, short, 12, q, probes, (16, 40))
    _check_lists(x, short, 12, q, probes[:, :1], (64,))  # 3 candidates


def test_probe_tables_with_entries_that_name_no_list():
    rng = np.random.default_rng(4)
    x, q = R.integer_rows(rng, 600, 128), R.integer_rows(rng, 70, 128)
    labels = rng.integers(0, 12, 600)
    probes = _distinct_probes(rng, 70, 12, 10)
    probes[::7, 1] = -1
    probes[1::7, 4:] = 12
    probes[2::7, 0] = INT32_MAX
    probes[3] = -1  # a query without a pair
    _check_lists(x, labels, 12, q, probes, (16, 33))
    _check_lists(x, labels, 12, q, np.full((70, 3), -1), (16, 17))  # no pair at all: nothing but fill


def test_row_mask_equals_the_search_over_the_visible_rows():
    rng = np.random.default_rng(5)
    x, q = R.integer_rows(rng, 600, 128), R.integer_rows(rng, 100, 128)
    labels = rng.integers(0, 12, 600)
    visible = rng.random(600) < 0.6
    _check_lists(x, labels, 12, q, _distinct_probes(rng, 100, 12, 9), (16, 40), visible=visible)


@pytest.mark.parametrize("nq", [70, 256])
def test_three_k_slices(nq):
    """d = 192: three K slices; one list of 130 rows is two tiles at B = 128 and three at B = 64, the last one partial."""
    rng = np.random.default_rng(1200 + nq)
    x, q = R.integer_rows(rng, 130, 192), R.integer_rows(rng, nq, 192)
    _check_lists(x, np.zeros(130, dtype=np.int64), 1, q, np.zeros((nq, 1), dtype=np.int64), (16, 33))


def test_page_with_ceilings_that_are_no_candidate():
    """search_lists_page directly: one ceiling per query over all its lists, between scores, in front of and behind the
    ids that tie, exhausted queries."""
    from sonar_amd import index

    rng = np.random.default_rng(6)
    x, q = R.integer_rows(rng, 600, 128), R.integer_rows(rng, 100, 128)
    labels = rng.integers(0, 12, 600)
    probes = _distinct_probes(rng, 100, 12, 9)
    rows, ids, off, _ = index.build_lists(_dev(x), _i32(labels), 12)
    s64 = R.scores64(q, x)
    cs = rng.integers(-4, 12, 100).astype(np.float64)
    cs[::3] += 0.5
    ci = rng.integers(0, 700, 100).astype(np.int64)
    ci[::5] = 0
    ci[2::9] = -1
    cs[1], cs[4] = np.inf, -np.inf
    for k in (16, 7):
        want_s, want_i = W.search(s64, labels, 12, probes, k, (cs, ci))
        s, i = index.search_lists_page(_dev(q), _i32(probes), rows, ids, off, k,
                                       (_dev(cs.astype(np.float32)), _i32(ci)))
        torch.cuda.synchronize()
        _same(s, i, want_s, want_i, k)
    assert (want_i[2::9] == -1).all() and (want_i[4] == -1).all()


# ----------------------------------------------------------------------------------------- 2. the classes (they normalise)
def _sixteenth_rows(rng, n, d=64):
    """16 entries of +-1: the norm is 4, every cosine a multiple of 1/16."""
    x = np.zeros((n, d), dtype=np.float16)
    for r in range(n):
        x[r, rng.permutation(d)[:16]] = rng.choice([-1.0, 1.0], 16)
    return x


def _scores16(q, x):
    return R.scores64(q.astype(np.float64) / 4, x.astype(np.float64) / 4)


@pytest.mark.parametrize("nprobe", [9, 64])
def test_probe_wide_is_the_restated_order_of_the_centroids(nprobe):
    from sonar_amd.index import IVFFlatIndex, IVFInt8Index

    rng = np.random.default_rng(7)
    c, q = _sixteenth_rows(rng, 70), _sixteenth_rows(rng, 90)
    want = W.first_k(_scores16(q, c), nprobe)[1]
    vals = W.first_k(_scores16(q, c), 65)[0]
    assert (vals[:, nprobe - 1] == vals[:, nprobe]).mean() >= 0.5  # the tie-break decides the last probe
    for cls in (IVFFlatIndex, IVFInt8Index):
        got = cls(_dev(c)).probe_wide(_dev(q), nprobe)
        torch.cuda.synchronize()
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match="exceeds the 12 lists"):
        IVFFlatIndex(_dev(c[:12])).probe_wide(_dev(q), 13)


def test_search_wide_search_page_and_the_mask_on_the_class():
    from sonar_amd.index import IVFFlatIndex, PreTransformIndex

    rng = np.random.default_rng(8)
    c, x, q = _sixteenth_rows(rng, 12), _sixteenth_rows(rng, 600), _sixteenth_rows(rng, 100)
    labels = rng.integers(0, 12, 600)
    ix = IVFFlatIndex(_dev(c)).add(_dev(x), _i32(labels))
    s64, sc = _scores16(q, x), _scores16(q, c)
    for nprobe, k in ((9, 40), (12, 64), (1, 16)):
        probes = W.first_k(sc, nprobe)[1]
        want_s, want_i = W.search_wide(s64, labels, 12, probes, k)
        _same(*ix.search_wide(_dev(q), k, nprobe), want_s, want_i, (nprobe, k))
    probes = W.first_k(sc, 9)[1]
    # given probes; a page under the ceiling of the page before
    p1 = ix.search_page(_dev(q), 16, probes=_i32(probes))
    p2 = ix.search_page(_dev(q), 5, probes=_i32(probes), below=(p1[0][:, -1].contiguous(), p1[1][:, -1].contiguous()))
    want_s, want_i = W.search_wide(s64, labels, 12, probes, 21)
    _same(torch.cat([p1[0], p2[0]], 1), torch.cat([p1[1], p2[1]], 1), want_s, want_i, "pages")
    # the mask
    visible = rng.random(600) < 0.5
    flt = ix.row_filter(mask=_dev(visible))
    want_s, want_i = W.search_wide(s64, labels, 12, probes, 33, visible)
    _same(*ix.search_wide(_dev(q), 33, 9, rows=flt), want_s, want_i, "mask")
    assert PreTransformIndex.search_wide is not None


def test_search_wide_at_8_by_8_is_search_bit_for_bit():
    from sonar_amd.index import IVFFlatIndex

    g = torch.Generator().manual_seed(9)
    x = torch.randn(3000, 128, generator=g).cuda()
    q = (x[:300] + 0.3 * torch.randn(300, 128, generator=g).cuda())
    ix = IVFFlatIndex.train(x, 12, n_iter=2).add(x)
    s, i = ix.search(q, 8, 8)
    ws, wi = ix.search_wide(q, 8, 8)
    torch.cuda.synchronize()
    assert torch.equal(i, wi) and torch.equal(s.view(torch.int32), ws.view(torch.int32))
    assert torch.equal(ix.probe(q, 8), ix.probe_wide(q, 8))
    # and a wide result extends it: the first 8 of 40 over the same probes
    ws40, wi40 = ix.search_wide(q, 40, 8)
    torch.cuda.synchronize()
    assert torch.equal(wi40[:, :8], i) and torch.equal(ws40[:, :8].view(torch.int32), s.view(torch.int32))
    assert (ws40.diff(dim=1) <= 0).all()
