"""GPU: extend / remove / merge_from of the IVF indexes and the regroup under them (sonar_amd/csrc/ivf_regroup.hpp,
sonar_amd/index.py).

Everything is exact.  At list level the result is compared with the plain-loop restatement in tests/ivf_regroup_ref.py: a
regroup moves bytes, so offsets, sizes and the (id, payload bytes, aux bits) of every list are equal or wrong.  At class level
the yardstick is the existing `add`: an index that was extended, compacted or merged holds, list by list, the bits of the
index `add` builds from the same rows in one go, and -- a score depending on the two rows alone, ties on the ids -- returns
the same search results bit for bit."""
import numpy as np
import pytest
import torch

from tests import ivf_ref as R
from tests import ivf_regroup_ref as G

pytestmark = pytest.mark.gpu

A = R.ALIGN
INT32_MAX = 2 ** 31 - 1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i32(a):
    return _dev(np.asarray(a, dtype=np.int32))


def _np_bytes(t, width):
    """A device matrix as uint8 [rows, width bytes]."""
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().reshape(t.shape[0], width)


def _np_words(t):
    return None if t is None else t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------ 1. list level
def _payload(rng_ids, width):
    """Payload bytes as a function of the id (never all zero for a row: byte 0 is odd), zeros for id -1."""
    ids = np.asarray(rng_ids, dtype=np.int64)
    cols = (ids[:, None] * 31 + np.arange(width)[None, :] * 17) % 256
    cols[:, 0] |= 1
    return np.where(ids[:, None] >= 0, cols, 0).astype(np.uint8)


def _aux(ids):
    """32-bit aux words as a function of the id -- NaN and -0.0 patterns among them: bits travel, not values."""
    ids = np.asarray(ids, dtype=np.int64)
    words = ids * 2654435761 % (1 << 32)
    words = np.where(ids % 7 == 0, 0x7FC00001, np.where(ids % 7 == 1, 0x80000000, words))
    return np.where(ids >= 0, words, 0).astype(np.uint32)


PATTERNS = ("random", "sorted", "one", "empty lists", "skipped", "old empty gets rows", "on the boundary", "a list dies",
            "all removed", "explicit ids")


def _case(rng, pattern, n_old, n_new, k):
    """(old labels [n_old], removed bool [n_old], new labels [n_new], new ids [n_new] or None)"""
    old = rng.integers(0, k, n_old).astype(np.int64)
    new = rng.integers(0, k, n_new).astype(np.int64)
    removed = rng.random(n_old) < 0.3
    new_ids = None
    if pattern == "sorted":
        old.sort()
        new.sort()
    elif pattern == "one":
        old[:], new[:] = k - 1, k - 1
    elif pattern == "empty lists":  # only every third list takes rows (tests/test_gpu_ivf.py)
        old, new = old // 3 * 3, new // 3 * 3
    elif pattern == "skipped":
        bad = np.array([-1, k, INT32_MAX])
        old = np.where(rng.random(n_old) < 0.3, rng.choice(bad, n_old), old)
        new = np.where(rng.random(n_new) < 0.3, rng.choice(bad, n_new), new)
    elif pattern == "old empty gets rows":  # list 0 holds nothing before and every new row after
        old = np.where(old == 0, k - 1, old) if k > 1 else np.full(n_old, -1)
        new[:] = 0
        removed[:] = False
    elif pattern == "on the boundary":  # list 0 ends on a 16-slot boundary before (16 rows) and, with >= 16 new rows, after (32)
        old = np.where(old == 0, -1, old)
        old[:A] = 0
        removed[:A] = False
        new = np.where(new == 0, -1, new)
        new[: A if n_new >= A else 0] = 0
    elif pattern == "a list dies":  # the last list loses every row
        removed |= old == k - 1
        new = np.where(new == k - 1, -1, new)
    elif pattern == "all removed":
        removed[:] = True
    elif pattern == "explicit ids":
        new_ids = np.where(rng.random(n_new) < 0.25, rng.choice(np.array([-1, -7, -INT32_MAX]), n_new), 100000 + 3 * np.arange(n_new))
    return old, removed, new, new_ids


def _check_regroup(rng, pattern, n_old, n_new, k, width, with_aux):
    from sonar_amd import _lib, index

    old_lab, removed, new_lab, new_ids = _case(rng, pattern, n_old, n_new, k)
    # the old storage as the build lays it out, at the capacity the build would have, garbage beyond offsets[K]
    o_off, _, slot_row = R.build(old_lab, k)
    cap_old = int(_lib.load().smi_ivf_slots_bound(n_old, k))
    o_ids = np.full(cap_old, -1, dtype=np.int64)
    o_ids[: len(slot_row)] = slot_row
    effective = np.where((o_ids >= 0) & ~removed[np.maximum(o_ids, 0)], o_ids, -1)
    o_payload, o_aux = _payload(o_ids, width), _aux(o_ids)
    o_payload[int(o_off[k]):] = 0xEE
    n_payload, base = _payload(n_old + np.arange(n_new), width), n_old
    n_aux = _aux(n_old + np.arange(n_new))
    if new_ids is not None:
        n_payload, n_aux = _payload(np.abs(new_ids), width), _aux(np.abs(new_ids))
    want_off, want_sizes, want_lists = G.regroup(
        k, (effective, o_off, o_payload, o_aux if with_aux else None),
        (new_lab, new_ids, n_payload, n_aux if with_aux else None) if n_new else None, base)

    as_f32 = lambda w: _dev(w.view(np.int32)).view(torch.float32)
    old = (_dev(o_payload), as_f32(o_aux) if with_aux else None, _i32(effective), _i32(o_off))
    new = (_dev(n_payload), as_f32(n_aux) if with_aux else None, _i32(new_lab), None if new_ids is None else _i32(new_ids)) \
        if n_new else None
    rows, aux, ids, off, sizes = index.regroup_lists(k, old, new, old_rows_bound=min(n_old, cap_old), new_id_base=base)
    torch.cuda.synchronize()
    assert rows.shape == (ids.shape[0], width) and ids.shape[0] == max(_lib.load().smi_ivf_slots_bound(n_old + n_new, k), A)
    assert (aux is not None) == with_aux
    off, sizes, ids = off.cpu().numpy(), sizes.cpu().numpy(), ids.cpu().numpy()
    assert np.array_equal(off, want_off) and np.array_equal(sizes, want_sizes), (pattern, off, want_off)
    got = G.storage_lists(k, ids, off, sizes, _np_bytes(rows, width), _np_words(aux), width)
    assert got == [sorted(m) for m in want_lists], pattern


@pytest.mark.parametrize("with_aux", [False, True])
@pytest.mark.parametrize("width", [128, 64, 16, 8, 2, 1])
def test_regroup_is_the_restated_regroup(width, with_aux):
    """Every payload path (16-byte accesses at 128, 64 and 16 bytes per row; bytes at 8, 2 and 1), K in {1, 5, 37}, n_old 300
    and 5000 (several workgroups of the bucketing passes), n_new in {0, 1, 200}; every label pattern at every width."""
    rng = np.random.default_rng(width * 2 + with_aux)
    combos = [(k, n_old, n_new) for k in (1, 5, 37) for n_old in (300, 5000) for n_new in (0, 1, 200)]
    for j, (k, n_old, n_new) in enumerate(combos):
        for pattern in (PATTERNS[(j + width) % len(PATTERNS)], PATTERNS[(3 * j + 1 + with_aux) % len(PATTERNS)]):
            _check_regroup(rng, pattern, n_old, n_new, k, width, with_aux)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_regroup_every_pattern_with_all_sizes_at_once(pattern):
    rng = np.random.default_rng(len(pattern))
    for k, n_old, n_new in ((5, 300, 200), (37, 5000, 200), (5, 300, 0), (1, 300, 1)):
        _check_regroup(rng, pattern, n_old, n_new, k, 64, True)


def test_regroup_without_an_old_side_is_a_build_and_misaligned_rows_take_the_byte_path():
    from sonar_amd import index

    rng = np.random.default_rng(5)
    n, k, width = 300, 5, 16
    labels = rng.integers(-1, k + 1, n)
    payload = _payload(np.arange(n), width)
    want_off, want_sizes, want_lists = G.regroup(k, None, (labels, None, payload, None), 7)
    flat = torch.zeros(8 + n * width, dtype=torch.uint8, device="cuda")
    flat[8:] = _dev(payload).reshape(-1)
    shifted = flat[8:].view(n, width)  # 16-byte rows on a base that is 8 bytes off a 16-byte boundary
    assert shifted.data_ptr() % 16 == 8
    for rows_in in (_dev(payload), shifted):
        rows, aux, ids, off, sizes = index.regroup_lists(k, None, (rows_in, None, _i32(labels), None), new_id_base=7)
        torch.cuda.synchronize()
        assert aux is None and np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(sizes.cpu().numpy(), want_sizes)
        got = G.storage_lists(k, ids.cpu().numpy(), off.cpu().numpy(), sizes.cpu().numpy(), _np_bytes(rows, width), None, width)
        assert got == [sorted(m) for m in want_lists]


def test_regroup_drops_what_the_promised_bound_does_not_cover():
    """More survivors than old_rows_bound promises: a broken contract.  Nothing is written beyond the slots the bound covers
    (the storage ends there: a store behind it would be out of bounds), and what is written is still rows of the input."""
    from sonar_amd import _lib, index

    k, n_old, width = 5, 300, 16
    labels = np.arange(n_old) % k
    o_off, _, slot_row = R.build(labels, k)
    payload = _payload(slot_row, width)
    bound = 100  # 300 rows survive
    cap = int(_lib.load().smi_ivf_slots_bound(bound, k))
    rows, _, ids, off, sizes = index.regroup_lists(k, (_dev(payload), None, _i32(slot_row), _i32(o_off)), None, old_rows_bound=bound)
    torch.cuda.synchronize()
    assert ids.shape[0] == cap < int(o_off[k])
    ids, rows = ids.cpu().numpy(), _np_bytes(rows, width)
    assert np.array_equal(sizes.cpu().numpy(), np.full(k, n_old // k))  # the counts still tell of every row
    held = ids >= 0
    assert held.sum() > 0 and np.array_equal(rows[held], _payload(ids[held], width)) and len(np.unique(ids[held])) == held.sum()


def test_regroup_is_capturable():
    """One list-level regroup captured into a graph on a single stream and replayed twice gives the direct call's result
    (modelled on the capture test of tests/test_gpu_dedup.py)."""
    from sonar_amd import index

    rng = np.random.default_rng(9)
    k, n_old, n_new, width = 5, 300, 200, 64
    old_lab, new_lab = rng.integers(0, k, n_old), rng.integers(-1, k + 1, n_new)
    o_off, _, slot_row = R.build(old_lab, k)
    effective = np.where(rng.random(len(slot_row)) < 0.3, -1, slot_row)
    as_f32 = lambda w: _dev(w.view(np.int32)).view(torch.float32)
    old = (_dev(_payload(slot_row, width)), as_f32(_aux(slot_row)), _i32(effective), _i32(o_off))
    new = (_dev(_payload(n_old + np.arange(n_new), width)), as_f32(_aux(n_old + np.arange(n_new))), _i32(new_lab), None)
    call = lambda: index.regroup_lists(k, old, new, new_id_base=n_old)
    want = call()
    torch.cuda.synchronize()
    want_lists = G.storage_lists(k, want[2].cpu().numpy(), want[3].cpu().numpy(), want[4].cpu().numpy(), _np_bytes(want[0], width),
                                 _np_words(want[1]), width)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm up off the default stream, as torch's capture asks
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = call()
    for _ in range(2):
        for t in got:
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got[3], want[3]) and torch.equal(got[4], want[4])
        lists = G.storage_lists(k, got[2].cpu().numpy(), got[3].cpu().numpy(), got[4].cpu().numpy(), _np_bytes(got[0], width),
                                _np_words(got[1]), width)
        assert lists == want_lists


# ------------------------------------------------------------------------------------------------------ 2. class level
K, N1, N2, NQ = 5, 300, 200, 70
KINDS = ("flat", "l2", "int8", "pq8", "pq16", "residual")


def _make(kind, seed=0):
    """(a function that makes an empty index of the kind, d): the quantisers are fixed by the seed, so two indexes of one kind
    hold the same centroids and codebooks bit for bit."""
    from sonar_amd import index

    d = 128 if kind in ("pq8", "pq16", "residual") else 64
    gen = torch.Generator().manual_seed(seed)
    cent = torch.randint(-1, 2, (K, d), generator=gen).float()
    cent[:, 0] = 1.0  # no zero centroid
    cent = cent.cuda()
    if kind in ("pq8", "pq16", "residual"):
        dsub = 8 if kind == "pq8" else 16
        cb = (torch.randint(-2, 3, (d // dsub, 256, dsub), generator=gen).float() / 4).half().cuda()
    cls = {"flat": index.IVFFlatIndex, "l2": index.IVFFlatL2Index, "int8": index.IVFInt8Index, "pq8": index.IVFPQIndex,
           "pq16": index.IVFPQIndex, "residual": index.IVFPQResidualIndex}[kind]
    return (lambda: cls(cent, cb)) if kind in ("pq8", "pq16", "residual") else (lambda: cls(cent)), d


def _data(d, n, seed):
    """Integer-valued rows (tests/ivf_ref.integer_rows) with no zero row, labels with some rows left out, and queries."""
    rng = np.random.default_rng(seed)
    x = R.integer_rows(rng, n, d)
    x[:, 0] = 1
    labels = rng.integers(0, K, n)
    labels[rng.random(n) < 0.05] = -1
    q = R.integer_rows(rng, NQ, d)
    q[:, 1] = 1
    return _dev(x), _i32(labels), _dev(q)


def _lists(ix):
    """The index's storage as sorted (id, payload bytes, aux bits) per list, its layout checked on the way."""
    torch.cuda.synchronize()
    width = ix._rows.shape[1] * ix._rows.element_size()
    aux = getattr(ix, ix._aux_name) if ix._aux_name else None
    return G.storage_lists(ix.n_lists, ix._ids.cpu().numpy(), ix.list_offsets.cpu().numpy(), ix.list_sizes.cpu().numpy(),
                           _np_bytes(ix._rows, width), _np_words(aux), width)


def _same_bits(a, b):
    return all(torch.equal(s.contiguous().view(torch.int32), t.contiguous().view(torch.int32)) for s, t in zip(a, b))


def _assert_same_index(got, want, q, what):
    assert torch.equal(got.list_sizes, want.list_sizes) and torch.equal(got.list_offsets, want.list_offsets), what
    assert _lists(got) == _lists(want), what
    for k in (1, 8):
        for nprobe in (1, 5):
            assert _same_bits(got.search(q, k=k, nprobe=nprobe), want.search(q, k=k, nprobe=nprobe)), (what, k, nprobe)


@pytest.mark.parametrize("kind", KINDS)
def test_extend_is_the_one_shot_add(kind):
    make, d = _make(kind)
    x, labels, q = _data(d, N1 + N2, 1)
    want = make().add(x, labels)
    got = make().add(x[:N1], labels[:N1])
    assert got.extend(x[N1:], labels[N1:]) is got and got._generation == 1
    _assert_same_index(got, want, q, kind)
    assert got._rows.shape[0] == want._rows.shape[0]  # the same bound: smi_ivf_slots_bound(300 + 200, K)
    # labels by the quantiser, in three chunks
    want = make().add(x)
    got = make().add(x[:100]).extend(x[100:N1]).extend(x[N1:])
    _assert_same_index(got, want, q, kind + ", own labels")


@pytest.mark.parametrize("kind", KINDS)
def test_remove_is_the_add_without_the_rows(kind):
    make, d = _make(kind)
    x, labels, q = _data(d, N1 + N2, 2)
    drop = torch.from_numpy(np.random.default_rng(3).random(N1 + N2) < 0.3).cuda()
    want = make().add(x, torch.where(drop, torch.full_like(labels, -1), labels))
    got = make().add(x, labels)
    assert got.remove(mask=drop) is got and got._generation == 1
    _assert_same_index(got, want, q, kind + ", mask")
    named = torch.nonzero(drop)[:, 0]
    for ids in (named, named.to(torch.int32), torch.cat([named.flip(0), named[:7], torch.tensor([-1, N1 + N2, 2 ** 40]).cuda()])):
        _assert_same_index(make().add(x, labels).remove(ids=ids), want, q, kind + f", {ids.dtype} ids")
    # a mask longer than the ids handed out is fine; removing nothing leaves the index as it was
    longer = torch.cat([drop, torch.ones(9, dtype=torch.bool, device="cuda")])
    _assert_same_index(make().add(x, labels).remove(mask=longer), want, q, kind + ", long mask")
    _assert_same_index(make().add(x, labels).remove(ids=torch.zeros(0, dtype=torch.int64, device="cuda")), make().add(x, labels), q,
                       kind + ", nothing")


@pytest.mark.parametrize("kind", KINDS)
def test_merge_from_is_the_one_shot_add(kind):
    make, d = _make(kind)
    x, labels, q = _data(d, N1 + N2, 4)
    want = make().add(x, labels)
    a, b = make().add(x[:N1], labels[:N1]), make().add(x[N1:], labels[N1:])
    before = _lists(b)
    assert a.merge_from(b) is a and a._generation == 1 and b._generation == 0
    _assert_same_index(a, want, q, kind)
    assert _lists(b) == before  # the other index is left as it is
    # add_id: the second half under ids of the caller's choice
    a = make().add(x[:N1], labels[:N1]).merge_from(b, add_id=1000)
    assert _lists(a) == _lists(make().add(x[:N1], labels[:N1]).extend(x[N1:], labels[N1:], first_id=1000))
    if kind == "flat":
        other, _ = _make("flat", seed=1)
        with pytest.raises(ValueError, match="other centroids"):
            a.merge_from(other().add(x[N1:], labels[N1:]))


@pytest.mark.parametrize("kind", KINDS)
def test_chain_of_remove_extend_remove(kind):
    """remove, extend, remove: the rows that are left, under the ids they were given, are what one `add` and one `extend`
    with first_id build."""
    make, d = _make(kind)
    x, labels, q = _data(d, N1 + N2, 5)
    rng = np.random.default_rng(6)
    drop1, drop2 = _dev(rng.random(N1) < 0.3), _dev(rng.random(N1 + N2) < 0.3)
    got = make().add(x[:N1], labels[:N1]).remove(mask=drop1).extend(x[N1:], labels[N1:]).remove(mask=drop2)
    assert got._generation == 3
    gone = torch.cat([drop1, torch.zeros(N2, dtype=torch.bool, device="cuda")]) | drop2
    left = torch.where(gone, torch.full_like(labels, -1), labels)
    _assert_same_index(got, make().add(x, left), q, kind)
    # the same rows with the second chunk's ids moved: one add and one extend with first_id
    got = make().add(x[:N1], labels[:N1]).remove(mask=drop1).extend(x[N1:], labels[N1:], first_id=5000)
    got.remove(ids=5000 + torch.nonzero(drop2[N1:])[:, 0]).remove(ids=torch.nonzero(drop2[:N1])[:, 0])
    want = make().add(x[:N1], left[:N1]).extend(x[N1:], left[N1:], first_id=5000)
    _assert_same_index(got, want, q, kind + ", first_id")
    assert int(got._ids.max()) == int(want._ids.max()) >= 5000


def test_flat_range_search_self_join_and_wide_search_on_an_extended_index():
    make, d = _make("flat")
    x, labels, q = _data(d, N1 + N2, 7)
    want, got = make().add(x, labels), make().add(x[:N1], labels[:N1]).extend(x[N1:], labels[N1:])
    a, b = got.range_search(q, 0.2, nprobe=5), want.range_search(q, 0.2, nprobe=5)
    assert torch.equal(a.lims, b.lims) and int(a.lims[-1]) > NQ and _same_bits((a.scores, a.ids), (b.scores, b.ids))
    assert _same_bits(got.self_join(n=N1 + N2), want.self_join(n=N1 + N2))
    assert _same_bits(got.search_wide(q, k=32, nprobe=5), want.search_wide(q, k=32, nprobe=5))


def test_a_row_filter_belongs_to_its_generation():
    from sonar_amd.index import RowFilter

    make, d = _make("flat")
    x, labels, q = _data(d, N1 + N2, 8)
    rng = np.random.default_rng(8)
    keys, mask = _i32(rng.integers(0, 4, N1 + N2)), _dev(rng.random(N1 + N2) < 0.7)
    qk = _i32(rng.integers(0, 4, NQ))
    want, got = make().add(x, labels), make().add(x[:N1], labels[:N1])
    stale = got.row_filter(keys=keys[:N1], mask=mask[:N1])
    assert isinstance(stale, RowFilter) and stale.generation == 0
    got.search(q, rows=stale)
    got.extend(x[N1:], labels[N1:])
    # (with these sizes the storage grew, so the length would give the stale filter away too: make one of the new length)
    for old in (stale, RowFilter(torch.full_like(got._ids, -1), None)):
        with pytest.raises(ValueError, match="slots|generation"):
            got.search(q, rows=old)
    with pytest.raises(ValueError, match="generation 0, this index is at 1"):
        got.search(q, rows=RowFilter(torch.full_like(got._ids, -1), None))
    fresh, ref = got.row_filter(keys=keys, mask=mask), want.row_filter(keys=keys, mask=mask)
    assert fresh.generation == 1 and ref.generation == 0
    for kwargs in ({}, {"query_keys": qk, "match": "=="}, {"query_keys": qk, "match": "<"}):
        assert _same_bits(got.search(q, k=8, nprobe=5, rows=fresh, **kwargs), want.search(q, k=8, nprobe=5, rows=ref, **kwargs))
    # after remove the length is unchanged: only the generation tells
    before = got.row_filter(mask=mask)
    got.remove(ids=torch.arange(10, device="cuda"))
    assert before.ids.shape == got._ids.shape
    with pytest.raises(ValueError, match="generation 1, this index is at 2"):
        got.search(q, rows=before)


def test_residual_search_through_its_own_probe():
    make, d = _make("residual")
    x, labels, q = _data(d, N1 + N2, 9)
    want, got = make().add(x), make().add(x[:N1]).extend(x[N1:])
    for nprobe in (1, 5):
        probes = want.probe(q, nprobe)
        assert torch.equal(probes, got.probe(q, nprobe))
        assert _same_bits(got.search(q, k=8, nprobe=nprobe), want.search(q, k=8, nprobe=nprobe))  # the probe's coarse scores
        assert _same_bits(got.search(q, k=8, probes=probes), want.search(q, k=8, probes=probes))  # `coarse_scores`


def test_pretransform_extend_remove_and_merge():
    from sonar_amd.index import IVFFlatIndex, PreTransformIndex
    from sonar_amd.transforms import PCA

    rng = np.random.default_rng(10)
    x = _dev(rng.standard_normal((N1 + N2, 256)).astype(np.float16))
    q = _dev(rng.standard_normal((NQ, 256)).astype(np.float16))
    pca = PCA.fit(x, 128)
    cent = pca.apply(x[:K]).float()
    labels = _i32(rng.integers(0, K, N1 + N2))
    want = PreTransformIndex(pca, IVFFlatIndex(cent)).add(x, labels)
    got = PreTransformIndex(pca, IVFFlatIndex(cent)).add(x[:N1], labels[:N1])
    assert got.extend(x[N1:], labels[N1:]) is got
    assert _lists(got.index) == _lists(want.index)
    assert _same_bits(got.search(q, k=8, nprobe=5), want.search(q, k=8, nprobe=5))
    a = PreTransformIndex(pca, IVFFlatIndex(cent)).add(x[:N1], labels[:N1])
    b = PreTransformIndex(pca, IVFFlatIndex(cent)).add(x[N1:], labels[N1:])
    assert _lists(a.merge_from(b).index) == _lists(want.index)
    drop = _dev(rng.random(N1 + N2) < 0.3)
    assert _lists(a.remove(mask=drop).index) == _lists(IVFFlatIndex(cent).add(pca.apply(x), torch.where(drop, -1, labels).int()))
    with pytest.raises(ValueError, match="another transform"):
        a.merge_from(PreTransformIndex(PCA.fit(x[:N1], 128), IVFFlatIndex(cent)).add(x[N1:], labels[N1:]))
    with pytest.raises(TypeError, match="PreTransformIndex"):
        a.merge_from(b.index)


@pytest.mark.parametrize("kind", ("flat", "l2", "int8", "residual"))
def test_state_dict_round_trip_continues_at_the_largest_id(kind):
    make, d = _make(kind)
    x, labels, q = _data(d, N1 + N2, 11)
    n3 = 120
    labels[N1 + n3 - 1] = 0  # the last row of the second chunk is in the index: max(ids) + 1 is then the running id, 420
    drop = _dev(np.random.default_rng(12).random(N1) < 0.3)
    drop[N1 - 1] = True  # the largest id of the first chunk goes: the running id must not fall back behind the second chunk
    ix = make().add(x[:N1], labels[:N1]).extend(x[N1: N1 + n3], labels[N1: N1 + n3]).remove(mask=torch.cat([drop, drop[:n3] & False]))
    state = ix.state_dict()
    assert set(state) == set(make().add(x[:N1], labels[:N1]).state_dict())  # no new key
    back = type(ix).from_state_dict(state)
    assert back._next_id is None and _lists(back) == _lists(ix)
    rest = N1 + N2 - N1 - n3
    back.extend(x[N1 + n3:], labels[N1 + n3:])
    assert back._next_id == N1 + n3 + rest  # max(ids) + 1 = 300 + 120, then the 80 new rows
    left = torch.where(torch.cat([drop, torch.zeros(N2, dtype=torch.bool, device="cuda")]), torch.full_like(labels, -1), labels)
    _assert_same_index(back, make().add(x, left), q, kind)
