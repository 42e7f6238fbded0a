"""CPU: the regroup of IVF storage (tests/ivf_regroup_ref.py) -- the restatement against the build's, the
capacity rule, and every refusal of `extend` / `remove` / `merge_from` / `regroup_lists` / smi_lists_regroup that needs no device."""
import itertools

import numpy as np
import pytest
import torch

from tests import ivf_ref as R
from tests import ivf_regroup_ref as G
from tests.test_ivf_cpu import FakeDevice, boom, fake  # noqa: F401  (the stand-ins for device tensors)

f16, i32 = torch.float16, torch.int32


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def _storage(labels, k, ids=None, width=3, seed=0):
    """The storage tests/ivf_ref.build gives labels, as the `old` of G.regroup: payload and aux are functions of the id."""
    offsets, _, slot_ids = R.build(labels, k)
    ids = np.arange(len(labels)) if ids is None else np.asarray(ids)
    slot_ids = np.where(slot_ids >= 0, ids[np.maximum(slot_ids, 0)], -1)
    return slot_ids, offsets, _payload(slot_ids, width), _aux(slot_ids)


def _payload(ids, width=3):
    ids = np.asarray(ids, dtype=np.int64)
    cols = (ids[:, None] * 7 + np.arange(width)[None, :] * 13 + 1) % 251
    return np.where(ids[:, None] >= 0, cols, 0).astype(np.uint8)


def _aux(ids):
    ids = np.asarray(ids, dtype=np.int64)
    return np.where(ids >= 0, ids * 2654435761 % (1 << 32), 0).astype(np.uint32)


def _expect(labels, k, ids=None):
    """What a one-shot build of labels holds, as sorted lists of (id, payload, aux)."""
    offsets, sizes, slot_ids = R.build(labels, k)
    ids = np.arange(len(labels)) if ids is None else np.asarray(ids)
    lists = []
    for c in range(k):
        rows = [int(ids[s]) for s in slot_ids[offsets[c]: offsets[c + 1]] if s >= 0]
        lists.append(sorted((r, bytes(_payload([r])[0]), int(_aux([r])[0])) for r in rows))
    return offsets, sizes, lists


@pytest.mark.parametrize("k,n1,n2,seed", [(1, 5, 3, 0), (5, 300, 200, 1), (37, 300, 200, 2), (5, 16, 16, 3), (300, 40, 70, 4)])
def test_restatement_equals_the_build_of_the_union(k, n1, n2, seed):
    rng = np.random.default_rng(seed)
    l1, l2 = rng.integers(-1, k + 1, n1), rng.integers(-1, k + 1, n2)  # (some labels name no list)
    # extend
    off, sizes, lists = G.regroup(k, _storage(l1, k), (l2, None, _payload(n1 + np.arange(n2)), _aux(n1 + np.arange(n2))), n1)
    e_off, e_sizes, e_lists = _expect(np.concatenate([l1, l2]), k)
    assert np.array_equal(off, e_off) and np.array_equal(sizes, e_sizes) and [sorted(m) for m in lists] == e_lists
    # the documented order: survivors in slot order, then the new rows in row order
    assert all([r for r, _, _ in m] == sorted(r for r, _, _ in m) for m in lists)
    # removal: the build with the removed rows' labels set to -1
    drop = rng.random(n1) < 0.4
    ids, offsets, payload, aux = _storage(l1, k)
    effective = np.where((ids >= 0) & ~drop[np.maximum(ids, 0)], ids, -1)
    off, sizes, lists = G.regroup(k, (effective, offsets, payload, aux))
    e_off, e_sizes, e_lists = _expect(np.where(drop, -1, l1), k)
    assert np.array_equal(off, e_off) and np.array_equal(sizes, e_sizes) and [sorted(m) for m in lists] == e_lists
    # merge: the other storage's slots are the new rows, labelled with their list, ids shifted
    o_ids, o_off, o_payload, o_aux = _storage(l2, k, ids=n1 + np.arange(n2))
    slot_list = np.searchsorted(o_off[1:], np.arange(len(o_ids)), side="right")
    off, sizes, lists = G.regroup(k, _storage(l1, k), (slot_list, o_ids, o_payload, o_aux))
    e_off, e_sizes, e_lists = _expect(np.concatenate([l1, l2]), k)
    assert np.array_equal(off, e_off) and np.array_equal(sizes, e_sizes) and [sorted(m) for m in lists] == e_lists


def test_storage_lists_reads_a_storage_back():
    labels = np.array([2, 0, 2, 5, -1, 2, 0])
    ids, offsets, payload, aux = _storage(labels, 4)
    sizes = R.build(labels, 4)[1]
    assert G.storage_lists(4, ids, offsets, sizes, payload, aux, 3) == _expect(labels, 4)[2]
    broken = payload.copy()
    broken[int(offsets[1]) - 1, 0] = 1  # a pad slot with a byte set
    with pytest.raises(AssertionError):
        G.storage_lists(4, ids, offsets, sizes, broken, aux, 3)


def test_capacity_rule_by_enumeration():
    """No labelling of at most n_old survivors and n_new rows over K lists needs more than slots_bound(n_old + n_new, K)
    slots: the slots a labelling needs depend on the list sizes alone, so every composition is enumerated."""
    for k in (1, 2, 3):
        for total in range(0, 36):
            need = max((sum(R.round_up(s) for s in sizes)
                        for sizes in itertools.product(range(total + 1), repeat=k) if sum(sizes) <= total), default=0)
            assert need <= R.slots_bound(total, k), (k, total, need)
            if total:
                assert need == R.slots_bound(total, k), (k, total, need)  # the bound is attained: no smaller one would do
    # and the bound never shrinks with the row count: survivors <= old_rows_bound may be fewer than promised
    for k in (1, 3, 17):
        assert all(R.slots_bound(n, k) <= R.slots_bound(n + 1, k) for n in range(200))


# ------------------------------------------------------------------------------------------------------- refusals
def _filled(ix, slots=48, bound=40, aux=None):
    """An index that claims to hold rows, as the existing CPU tests make one."""
    ix._added = True
    ix._rows = fake(slots, ix._codebooks.shape[0] if hasattr(ix, "_codebooks") else 64, dtype=ix._ROWS_DTYPE)
    ix._ids, ix._offsets, ix._sizes = fake(slots, dtype=i32), fake(ix.n_lists + 1, dtype=i32), fake(ix.n_lists, dtype=i32)
    ix._next_id = ix._rows_bound = bound
    if ix._aux_name:
        setattr(ix, ix._aux_name, fake(slots))
    return ix


def test_python_refusals_need_no_device(monkeypatch):
    from sonar_amd import index
    from sonar_amd.index import (IVFFlatIndex, IVFFlatL2Index, IVFInt8Index, IVFPQIndex, IVFPQResidualIndex, RowFilter,
                                 regroup_lists)

    monkeypatch.setattr(index._lib, "load", boom)
    monkeypatch.setattr(index, "topk_normalized", boom)
    monkeypatch.setattr(index, "topk_bias_prepared", boom)
    monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=f16))
    monkeypatch.setattr(index, "prepare_rows", lambda t: (fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=f16),
                                                          fake((t.shape[0] + 255) // 256 * 256)))
    cb = fake(8, 256, 8, dtype=f16)
    make = (lambda: IVFFlatIndex(fake(3, 64)), lambda: IVFFlatL2Index(fake(3, 64)), lambda: IVFInt8Index(fake(3, 64)),
            lambda: IVFPQIndex(fake(3, 64), cb), lambda: IVFPQResidualIndex(fake(3, 64), cb))
    for new in make:
        ix = new()
        assert ix._generation == 0 and ix._next_id is None
        for call in (lambda: ix.extend(fake(8, 64)), lambda: ix.remove(ids=fake(3, dtype=i32)), lambda: ix.merge_from(new())):
            with pytest.raises(RuntimeError, match="before add"):
                call()
        _filled(ix)
        with pytest.raises(RuntimeError, match="already called"):
            ix.add(fake(8, 64))
        monkeypatch.setattr(index, "normalize_rows", boom)  # every refusal of extend below comes before anything is prepared
        monkeypatch.setattr(index, "prepare_rows", boom)
        # extend: dim, dtype, device, labels, first_id, id overflow
        with pytest.raises(RuntimeError, match="HIP device only"):
            ix.extend(torch.zeros(8, 64))
        with pytest.raises(TypeError):
            ix.extend([[0.0] * 64])
        with pytest.raises(ValueError, match="dim 128"):
            ix.extend(fake(8, 128))
        with pytest.raises(ValueError, match="multiple of 64"):
            ix.extend(fake(8, 96))
        with pytest.raises(ValueError, match="empty"):
            ix.extend(fake(0, 64))
        with pytest.raises(ValueError, match="fp16 or fp32"):
            ix.extend(fake(8, 64, dtype=torch.float64))
        for bad in (fake(8, dtype=torch.int64), fake(7, dtype=i32), fake(8, 1, dtype=i32)):
            with pytest.raises(ValueError, match="labels must be int32"):
                ix.extend(fake(8, 64), labels=bad)
        with pytest.raises(RuntimeError, match="HIP device only"):
            ix.extend(fake(8, 64), labels=torch.zeros(8, dtype=i32))
        for bad in (-1, 2.0, True):
            with pytest.raises(ValueError, match="first_id"):
                ix.extend(fake(8, 64), first_id=bad)
        with pytest.raises(ValueError, match="exceed"):
            ix.extend(fake(8, 64), first_id=index.ID_MAX - 7)
        ix._next_id = index.ID_MAX - 3
        with pytest.raises(ValueError, match="exceed"):
            ix.extend(fake(8, 64))
        ix._next_id = 40
        # remove: both, neither, dtypes, shapes, a short mask
        for kwargs in ({}, {"ids": fake(3, dtype=i32), "mask": fake(40, dtype=torch.bool)}):
            with pytest.raises(ValueError, match="one of the two"):
                ix.remove(**kwargs)
        with pytest.raises(RuntimeError, match="HIP device only"):
            ix.remove(ids=torch.zeros(3, dtype=i32))
        with pytest.raises(RuntimeError, match="HIP device only"):
            ix.remove(mask=torch.zeros(40, dtype=torch.bool))
        for bad in (fake(3), fake(3, 1, dtype=i32), fake(3, dtype=torch.int16)):
            with pytest.raises(ValueError, match="ids must be int32 or int64"):
                ix.remove(ids=bad)
        for bad in (fake(40, dtype=torch.uint8), fake(4, 10, dtype=torch.bool)):
            with pytest.raises(ValueError, match="mask must be bool"):
                ix.remove(mask=bad)
        with pytest.raises(ValueError, match="mask has 39 entries.*up to 40"):
            ix.remove(mask=fake(39, dtype=torch.bool))
        # merge_from: itself, another class, other lists, other centroids, other codebooks, id overflow
        monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=f16))
        monkeypatch.setattr(index, "prepare_rows", lambda t: (fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=f16),
                                                              fake((t.shape[0] + 255) // 256 * 256)))
        with pytest.raises(ValueError, match="into itself"):
            ix.merge_from(ix)
        with pytest.raises(TypeError, match="takes a"):
            ix.merge_from("index")
        another = make[2]() if type(ix) is IVFFlatIndex else make[0]()  # (a residual index is not a plain PQ index either)
        with pytest.raises(TypeError, match="takes a"):
            ix.merge_from(_filled(another))
        if type(ix) is IVFPQResidualIndex:
            with pytest.raises(TypeError, match="takes a"):
                ix.merge_from(_filled(make[3]()))
        with pytest.raises(RuntimeError, match="before add"):
            ix.merge_from(new())
        wide = type(ix)(fake(4, 64), *((cb,) if isinstance(ix, IVFPQIndex) else ()))
        with pytest.raises(ValueError, match="4 lists"):
            ix.merge_from(_filled(wide))
        # the quantisers are compared bit for bit: real values behind the stand-in class
        real = lambda *shape, v=0.0: torch.full(shape, v, dtype=f16).as_subclass(FakeDevice)
        other = _filled(new())
        ix._c16, other._c16 = real(256, 64), real(256, 64, v=1.0)
        with pytest.raises(ValueError, match="other centroids"):
            ix.merge_from(other)
        other._c16 = real(256, 64)
        if isinstance(ix, IVFPQIndex):
            ix._codebooks, other._codebooks = real(8, 256, 8), real(8, 256, 8, v=2.0)
            with pytest.raises(ValueError, match="other codebooks"):
                ix.merge_from(other)
            other._codebooks = real(8, 256, 8)
        for bad in (-1, 1.5, True):
            with pytest.raises(ValueError, match="add_id"):
                ix.merge_from(other, add_id=bad)
        with pytest.raises(ValueError, match="exceed"):
            ix.merge_from(other, add_id=index.ID_MAX - 39)
        assert ix._generation == 0  # nothing above went through

    # the generation rule of RowFilter: positional construction keeps generation 0; another generation is refused
    assert RowFilter(fake(48, dtype=i32), None).generation == 0 and RowFilter._fields == ("ids", "keys", "generation")
    ix = _filled(IVFFlatIndex(fake(3, 64)))
    q = fake(5, 64)
    monkeypatch.setattr(index, "normalize_rows", boom)
    stale = RowFilter(fake(48, dtype=i32), None)
    ix._generation = 2
    for call in (lambda f: ix.search(q, rows=f), lambda f: ix.range_search(q, 0.5, rows=f), lambda f: ix.search_wide(q, nprobe=2, rows=f),
                 lambda f: ix.search_page(q, rows=f)):
        with pytest.raises(ValueError, match="generation 0, this index is at 2"):
            call(stale)
        with pytest.raises(AssertionError, match="reached the device"):  # the current generation passes the check
            call(stale._replace(generation=2))

    # regroup_lists
    old = (fake(48, 64, dtype=f16), None, fake(48, dtype=i32), fake(4, dtype=i32))
    new = (fake(256, 64, dtype=f16), None, fake(8, dtype=i32), None)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_lists"):
            regroup_lists(bad, old, new)
    with pytest.raises(ValueError, match="old, new or both"):
        regroup_lists(3)
    with pytest.raises(TypeError, match="tuple of four"):
        regroup_lists(3, old[:3])
    with pytest.raises(RuntimeError, match="HIP device only"):
        regroup_lists(3, (torch.zeros(48, 64), None, old[2], old[3]))
    for key, bad, what in ((0, fake(48, dtype=f16), r"\[slots, width\]"), (2, fake(47, dtype=i32), "old ids must be int32"),
                           (2, fake(48, dtype=torch.int64), "old ids must be int32"), (3, fake(3, dtype=i32), "old offsets"),
                           (1, fake(48, dtype=f16), "aux must be contiguous fp32"), (1, fake(47), "47 entries for 48")):
        with pytest.raises(ValueError, match=what):
            regroup_lists(3, tuple(bad if j == key else t for j, t in enumerate(old)), None)
    for key, bad, what in ((0, fake(256, 128, dtype=f16), "the old rows"), (0, fake(256, 64, dtype=torch.int8), "the old rows"),
                           (1, fake(256), "both sides or with neither"), (2, fake(8, 1, dtype=i32), "labels must be int32"),
                           (2, fake(300, dtype=i32), "300 labels for 256"), (3, fake(7, dtype=i32), "new ids must be int32")):
        with pytest.raises(ValueError, match=what):
            regroup_lists(3, old, tuple(bad if j == key else t for j, t in enumerate(new)))
    for bad in (-1, 49, 1.0, True):
        with pytest.raises(ValueError, match="old_rows_bound"):
            regroup_lists(3, old, new, old_rows_bound=bad)
    for bad in (-1, index.ID_MAX - 7, 1.0):
        with pytest.raises(ValueError, match="new_id_base"):
            regroup_lists(3, old, new, new_id_base=bad)


def test_c_abi_sizing_and_refusals_without_a_device(lib):
    sb, ws, G_ = lib.smi_ivf_slots_bound, lib.smi_lists_regroup_ws_bytes, lib.smi_lists_regroup
    # cursor [K] | keys [old_slots + n_new], each rounded up to 16 bytes
    assert ws(48, 8, 3) == 16 + 56 * 4 and ws(0, 5, 3) == 16 + 32 and ws(48, 0, 7) == 32 + 48 * 4
    for bad in ((0, 0, 3), (48, 8, 0), (-1, 8, 3), (48, -1, 3), (1 << 31, 0, 3), (0, 1 << 31, 3), (48, 8, 1 << 31),
                (1 << 30, 1 << 30, 3)):
        assert ws(*bad) == 0, bad
    p, q, big = 0x1000, 0x2000, 1 << 40  # never dereferenced: every call below is refused on its arguments
    cap = sb(40 + 8, 3)
    good = dict(old_rows=p, old_aux=None, old_ids=p, old_offsets=p, old_slots=48, old_rows_bound=40, new_rows=p, new_aux=None,
                new_labels=p, new_ids=None, new_id_base=40, n_new=8, row_bytes=128, K=3, list_rows=q, list_aux=None, list_ids=q,
                capacity=cap, list_offsets=q, list_sizes=q, ws=q, ws_bytes=big, stream=None)
    INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -3
    if not torch.cuda.is_available():
        assert G_(*good.values()) == NO_DEVICE  # the refusals come before have_device(): a good call gets that far
        assert G_(*{**good, "old_slots": 0, "old_rows_bound": 0, "old_rows": None, "old_ids": None, "old_offsets": None,
                    "capacity": sb(8, 3)}.values()) == NO_DEVICE  # a pure build from encoded rows
        assert G_(*{**good, "n_new": 0, "new_rows": None, "new_labels": None, "capacity": sb(40, 3)}.values()) == NO_DEVICE
        assert G_(*{**good, "row_bytes": 1}.values()) == NO_DEVICE
    cases = [
        ("null rows", {"list_rows": None}, INVALID, "null argument"),
        ("null ids", {"list_ids": None}, INVALID, "null argument"),
        ("null offsets", {"list_offsets": None}, INVALID, "null argument"),
        ("null sizes", {"list_sizes": None}, INVALID, "null argument"),
        ("K", {"K": 0}, INVALID, "at least one list"),
        ("negative", {"n_new": -1}, INVALID, "negative"),
        ("both empty", {"old_slots": 0, "old_rows_bound": 0, "n_new": 0}, INVALID, "both sides"),
        ("big K", {"K": 1 << 31}, UNSUPPORTED, "fit int32"),
        ("big items", {"old_slots": 1 << 30, "n_new": 1 << 30}, UNSUPPORTED, "fit int32"),
        ("row_bytes", {"row_bytes": 0}, INVALID, "row_bytes"),
        ("null old rows", {"old_rows": None}, INVALID, "null old_rows"),
        ("null old ids", {"old_ids": None}, INVALID, "null old_rows"),
        ("null old offsets", {"old_offsets": None}, INVALID, "null old_rows"),
        ("null new rows", {"new_rows": None}, INVALID, "null new_rows"),
        ("null labels", {"new_labels": None}, INVALID, "null new_rows"),
        ("bound above slots", {"old_rows_bound": 49}, INVALID, "old_rows_bound"),
        ("negative bound", {"old_rows_bound": -1}, INVALID, "old_rows_bound"),
        ("old aux alone", {"old_aux": p}, INVALID, "go together"),
        ("new aux alone", {"new_aux": p}, INVALID, "go together"),
        ("list aux alone", {"list_aux": q}, INVALID, "go together"),
        ("old aux missing", {"new_aux": p, "list_aux": q}, INVALID, "go together"),
        ("new aux missing", {"old_aux": p, "list_aux": q}, INVALID, "go together"),
        ("list aux missing", {"old_aux": p, "new_aux": p}, INVALID, "go together"),
        ("id overflow", {"new_id_base": (1 << 31) - 256 - 7}, UNSUPPORTED, "row ids must fit int32"),
        ("negative id base", {"new_id_base": -1}, UNSUPPORTED, "row ids must fit int32"),
        ("rows in place", {"list_rows": p}, INVALID, "not in place"),
        ("ids in place", {"list_ids": p}, INVALID, "not in place"),
        ("offsets in place", {"list_offsets": p}, INVALID, "not in place"),
        ("aux in place", {"old_aux": p, "new_aux": p, "list_aux": p}, INVALID, "not in place"),
        ("ids are the new ids", {"new_ids": q}, INVALID, "not in place"),
        ("small capacity", {"capacity": cap - 1}, INVALID, "smi_ivf_slots_bound"),
        ("big slots", {"old_slots": 1 << 30, "old_rows_bound": 1 << 30, "n_new": 0, "K": 1 << 30, "capacity": big}, UNSUPPORTED,
         "slot numbers must fit int32"),
        ("null ws", {"ws": None}, INVALID, "null workspace"),
        ("short ws", {"ws_bytes": ws(48, 8, 3) - 1}, INVALID, "smi_lists_regroup_ws_bytes"),
        ("misaligned ws", {"ws": q + 8}, INVALID, "16-byte aligned"),
    ]
    for name, change, rc, text in cases:
        got = G_(*{**good, **change}.values())
        assert got == rc and text.encode() in lib.smi_last_error(), (name, got, lib.smi_last_error())
    # a bound of 40 of 48 slots is what makes the capacity of the union enough: with the slots as the bound it is too small
    assert sb(48 + 8, 3) > cap and G_(*{**good, "old_rows_bound": 48}.values()) == INVALID
