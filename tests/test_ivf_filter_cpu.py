"""CPU: filtered search over the IVF lists.  The numpy restatement (tests/ivf_filter_ref.py: the existing
restatements on masked labels) against a plain double loop; the `accept` table; the seven C entries in the binding, the header
and the library, with every refusal of theirs -- the twin's, in the twin's order and words, and their own behind its null
checks; and every refusal of the Python layer.  Nothing here needs a device."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import ivf_filter_ref as F
from tests import ivf_ref as R
from tests.test_ivf_cpu import FakeDevice, boom, fake  # noqa: F401  (the stand-ins for device tensors)

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
TWINS = {"smi_ivf_search_keyed": "smi_ivf_search", "smi_ivf_i8_search_keyed": "smi_ivf_i8_search",
         "smi_ivf_pq_search_keyed": "smi_ivf_pq_search", "smi_ivf_pq_search_residual_keyed": "smi_ivf_pq_search_residual",
         "smi_range_search_count_keyed": "smi_range_search_count", "smi_range_search_emit_keyed": "smi_range_search_emit"}
NAMES = ("smi_slot_filter", *TWINS)


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


# ------------------------------------------------------------------------------------------------------- restatement
def test_accept_table_over_signed_key_pairs():
    from sonar_amd import index

    assert index.MATCH_ACCEPT == F.ACCEPT == {"==": 2, "!=": 5, "<": 1, "<=": 3, ">": 4, ">=": 6}
    keys = [INT32_MIN, INT32_MIN + 1, -7, -1, 0, 1, 7, INT32_MAX - 1, INT32_MAX]
    ops = {"==": lambda a, b: a == b, "!=": lambda a, b: a != b, "<": lambda a, b: a < b, "<=": lambda a, b: a <= b,
           ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}
    rk = np.array(keys, dtype=np.int32)
    for qk in keys:
        for rel, op in ops.items():
            assert F.passes(rk, qk, F.ACCEPT[rel]).tolist() == [op(a, qk) for a in keys], (rel, qk)
        assert not F.passes(rk, qk, 0).any() and F.passes(rk, qk, 7).all()
    # the three bits are the three outcomes of one compare: every mask is the union of its bits
    for accept in range(8):
        want = np.zeros(len(keys), dtype=bool)
        for bit, rel in enumerate(("<", "==", ">")):
            if accept >> bit & 1:
                want |= F.passes(rk, 0, F.ACCEPT[rel])
        assert np.array_equal(F.passes(rk, 0, accept), want)


@pytest.mark.parametrize("accept", range(8))
def test_restatement_equals_a_plain_double_loop(accept):
    rng = np.random.default_rng(accept)
    n, k_lists, nq = 70, 4, 11
    x, q = R.integer_rows(rng, n, 64), R.integer_rows(rng, nq, 64)
    x[7] = x[40] = x[41] = x[3]  # ties: equal rows in different lists and in one
    q[0] = 0                     # every candidate scores 0
    labels = rng.integers(0, k_lists, n)
    labels[labels == 3] = -1     # an empty list, rows in no list
    probes = np.stack([rng.permutation(k_lists)[:3] for _ in range(nq)])
    probes[1], probes[2] = [1, 1, 2], [-1, k_lists, INT32_MAX]  # a list named twice; no list named
    row_keys = rng.integers(-2, 3, n)
    row_keys[:2] = [INT32_MIN, INT32_MAX]
    query_keys = rng.integers(-2, 3, nq)
    query_keys[3], query_keys[4] = INT32_MIN, INT32_MAX
    mask = rng.random(n) < 0.8
    for rk, m, qk in ((row_keys, None, query_keys), (row_keys, mask, query_keys), (None, mask, None), (row_keys, None, None),
                      (row_keys[:50], mask[:60], query_keys)):
        for k in (1, 8):
            got = F.flat_search(q, x, labels, k_lists, probes, k, rk, m, qk, accept)
            want = F.flat_search_loop(q, x, labels, k_lists, probes, k, rk, m, qk, accept)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if accept == 7:  # everything passes: the unfiltered restatement
        got, want = F.flat_search(q, x, labels, k_lists, probes, 8, row_keys, None, query_keys, 7), R.search(q, x, labels, k_lists, probes, 8)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if accept == 0:
        got = F.flat_search(q, x, labels, k_lists, probes, 8, row_keys, None, query_keys, 0)
        assert (got[1] == -1).all() and np.isneginf(got[0]).all()
    # the range restatement is the same rule: its segments are the allowed rows at or above the threshold
    thr = np.array([0.0, -np.inf, 1.0] * 4, dtype=np.float32)[:nq]
    lims, sc, ids = F.range_search(q, x, labels, k_lists, probes, thr, row_keys, mask, query_keys, accept)
    full = F.flat_search_loop(q, x, labels, k_lists, probes, 3 * n, row_keys, mask, query_keys, accept)
    for r in range(nq):
        keep = (full[1][r] >= 0) & (full[0][r].astype(np.float32) >= thr[r])
        assert np.array_equal(ids[lims[r]: lims[r + 1]], full[1][r][keep]) and np.array_equal(sc[lims[r]: lims[r + 1]], full[0][r][keep])


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_symbols_are_bound_declared_and_exported(lib):
    from sonar_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sonar_mi355.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert name in _lib.SYMBOLS and f" {name}(" in header and f" T {name}\n" in exported, name
    assert lib.smi_abi_version() == 7 and "#define SMI_ABI_VERSION 7" in header
    for keyed, twin in TWINS.items():  # the twin's argument list plus (slot_keys, query_keys, accept)
        assert _lib.SYMBOLS[keyed][1] == _lib.SYMBOLS[twin][1] + [_lib.C.c_void_p, _lib.C.c_void_p, _lib.C.c_int32], keyed


def test_keyed_entries_refuse_what_their_twins_refuse_and_their_own_arguments(lib):
    if lib.smi_device_count() > 0:
        pytest.skip("a HIP device is visible: the made-up pointers must never reach a kernel")
    p, big = 0x1000, 1 << 40  # never dereferenced: every call below is refused
    head = dict(qn=p, nq=100, d=64, probes=p)
    tail = dict(ids=p, offsets=p, K=7, k=5, idx=p, score=p, ws=p, ws_bytes=big, stream=None)
    rng_head = dict(**head, nprobe=4, threshold=p, rows=p, ids=p, offsets=p, K=7)
    good = {
        "smi_ivf_search": dict(**head, nprobe=4, rows=p, **tail),
        "smi_ivf_i8_search": dict(**head, nprobe=4, codes=p, scales=p, **tail),
        "smi_ivf_pq_search": dict(**head, nprobe=4, codes=p, dsub=8, codebooks=p, **tail),
        "smi_ivf_pq_search_residual": dict(**head, coarse=p, nprobe=4, codes=p, dsub=8, codebooks=p, **tail),
        "smi_range_search_count": dict(**rng_head, pair_counts=p, ws=p, ws_bytes=big, stream=None),
        "smi_range_search_emit": dict(**rng_head, pair_base=p, total=5, score=p, idx=p, ws=p, ws_bytes=big, stream=None),
    }
    sizing = {
        "smi_ivf_search": lambda c: lib.smi_ivf_search_workspace_bytes(c["nq"], c["K"], c["nprobe"], c["k"], c["d"]),
        "smi_ivf_i8_search": lambda c: lib.smi_ivf_i8_search_workspace_bytes(c["nq"], c["K"], c["nprobe"], c["k"], c["d"]),
        "smi_ivf_pq_search": lambda c: lib.smi_ivf_pq_search_workspace_bytes(c["nq"], c["K"], c["nprobe"], c["k"], c["d"], c["dsub"]),
        "smi_ivf_pq_search_residual": lambda c: lib.smi_ivf_pq_search_workspace_bytes(c["nq"], c["K"], c["nprobe"], c["k"], c["d"], c["dsub"]),
        "smi_range_search_count": lambda c: lib.smi_range_search_ws_bytes(c["nq"], c["K"], c["nprobe"], c["d"]),
        "smi_range_search_emit": lambda c: lib.smi_range_search_ws_bytes(c["nq"], c["K"], c["nprobe"], c["d"]),
    }
    keys = dict(slot_keys=p, query_keys=p, accept=2)
    wrong = []
    for keyed, twin in TWINS.items():
        g = good[twin]
        need = sizing[twin](g)
        assert need > 0
        # the twin's refusals, one at a time and two at once, and the call it accepts: same code, same words
        changes = [{name: None} for name, v in g.items() if v == p] + [
            {"d": 96}, {"d": 0}, {"K": 0}, {"nq": 0}, {"nq": 1 << 31}, {"K": 1 << 31}, {"nprobe": 0}, {"nprobe": 9},
            {"nq": 1 << 29, "nprobe": 8}, {"ws": p + 8}, {"ws_bytes": need - 1}, {"ws_bytes": need},
            {"qn": None, "d": 96}, {"d": 96, "K": 0}, {"K": 0, "nq": 0}, {"nprobe": 9, "ws": None}, {"ws": None, "ws_bytes": 0}, {}]
        if "k" in g:
            changes += [{"k": 0}, {"k": 9}, {"k": 9, "nprobe": 9}, {"nq": 0, "k": 0}]
        if "dsub" in g:
            changes += [{"dsub": 7}, {"dsub": 16, "d": 72}, {"codebooks": p + 8}, {"dsub": 7, "ws": None}]
        if "total" in g:
            changes += [{"total": -1}, {"total": -1, "ws_bytes": need - 1}, {"total": -1, "nprobe": 0}]
        if twin == "smi_ivf_i8_search":
            changes += [{"d": 131072 + 64}]
        for change in changes:
            call = {**g, **change}
            rc_t = getattr(lib, twin)(*call.values())
            err_t = lib.smi_last_error().decode()
            rc_k = getattr(lib, keyed)(*call.values(), *keys.values())
            err_k = lib.smi_last_error().decode()
            if rc_t == 0 or (rc_k, err_k) != (rc_t, err_t):
                wrong.append((keyed, change, rc_t, err_t, rc_k, err_k))
        # the twin's sizing value is accepted: the call gets as far as the device
        rc = getattr(lib, keyed)(*{**g, "ws_bytes": need}.values(), *keys.values())
        if rc == 0 or "no HIP device visible" not in lib.smi_last_error().decode():
            wrong.append((keyed, "sizing value", rc, lib.smi_last_error().decode()))
        # their own, behind the null checks and in front of everything else, in this order
        own = [({"slot_keys": None}, {}, "null slot_keys or query_keys"), ({"query_keys": None}, {}, "null slot_keys or query_keys"),
               ({"slot_keys": p + 4}, {}, "slot_keys must be 16-byte aligned"), ({"slot_keys": p + 8}, {}, "slot_keys must be 16-byte aligned"),
               ({"accept": -1}, {}, "accept=-1 must be in [0, 7]"), ({"accept": 8}, {}, "accept=8 must be in [0, 7]"),
               ({"accept": 0}, {}, "no HIP device visible"), ({"accept": 7}, {}, "no HIP device visible"),
               ({"query_keys": p + 4}, {}, "no HIP device visible"),  # only the 16-byte loads of the slot keys need alignment
               ({"slot_keys": None}, {"qn": None}, "null argument"), ({"accept": 8}, {"offsets": None}, "null argument"),
               ({"slot_keys": None, "accept": 8}, {}, "null slot_keys or query_keys"),
               ({"slot_keys": p + 4, "accept": 8}, {}, "slot_keys must be 16-byte aligned"),
               ({"query_keys": None}, {"d": 96}, "null slot_keys or query_keys"), ({"accept": 8}, {"nprobe": 9}, "accept=8"),
               ({"accept": 9}, {"ws": None}, "accept=9"), ({"slot_keys": p + 4}, {"nq": 0}, "slot_keys must be 16-byte aligned")]
        for kchange, change, text in own:
            rc = getattr(lib, keyed)(*{**g, **change}.values(), *{**keys, **kchange}.values())
            err = lib.smi_last_error().decode()
            if rc == 0 or text not in err:
                wrong.append((keyed, kchange, change, text, rc, err))
        # the code of a refused key argument is that of any argument
        assert getattr(lib, keyed)(*g.values(), p, p, 8) == getattr(lib, twin)(*{**g, "qn": None}.values()) != 0
    assert not wrong, wrong[:5]


def test_slot_filter_refusals_without_a_device(lib):
    if lib.smi_device_count() > 0:
        pytest.skip("a HIP device is visible: the made-up pointers must never reach a kernel")
    p = 0x1000
    good = dict(ids=p, offsets=p, K=7, row_keys=p, row_mask=p, n=100, slot_ids=p, slot_keys=p, slots=160, stream=None)
    cases = [({"ids": None}, "null argument"), ({"offsets": None}, "null argument"), ({"slot_ids": None}, "null argument"),
             ({"row_keys": None, "row_mask": None, "slot_keys": None}, "nothing to filter by"),
             ({"row_keys": None}, "go together"), ({"slot_keys": None}, "go together"),
             ({"slot_ids": p + 4}, "16-byte aligned"), ({"slot_keys": p + 8}, "16-byte aligned"),
             ({"K": 0}, "K=0: at least one list"), ({"n": 0}, "n=0: empty input"), ({"slots": 0}, "slots=0: empty storage"),
             ({"n": 1 << 31}, "must fit int32"), ({"K": 1 << 31}, "must fit int32"), ({"slots": 1 << 31}, "must fit int32"),
             ({"ids": None, "K": 0}, "null argument"), ({"slot_ids": p + 4, "K": 0}, "16-byte aligned"), ({"K": 0, "n": 0}, "K=0"),
             ({}, "no HIP device visible"), ({"row_mask": None}, "no HIP device visible"),
             ({"row_keys": None, "slot_keys": None}, "no HIP device visible")]
    wrong = []
    for change, text in cases:
        rc = lib.smi_slot_filter(*{**good, **change}.values())
        err = lib.smi_last_error().decode()
        if rc == 0 or text not in err:
            wrong.append((change, text, rc, err))
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------------- Python refusals
def test_python_refusals_need_no_device(monkeypatch):
    from sonar_amd import index
    from sonar_amd.index import IVFFlatIndex, IVFInt8Index, IVFPQIndex, IVFPQResidualIndex, RowFilter

    f16, i32 = torch.float16, torch.int32
    monkeypatch.setattr(index._lib, "load", boom)
    monkeypatch.setattr(index, "topk_normalized", boom)
    monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=f16))
    cb = fake(8, 256, 8, dtype=f16)
    q = fake(5, 64)
    for ix in (IVFFlatIndex(fake(3, 64)), IVFInt8Index(fake(3, 64)), IVFPQIndex(fake(3, 64), cb), IVFPQResidualIndex(fake(3, 64), cb)):
        with pytest.raises(RuntimeError, match="row_filter before add"):
            ix.row_filter(keys=fake(100, dtype=i32))
        ix._added = True
        ix._ids, ix._offsets = fake(48, dtype=i32), fake(4, dtype=i32)
        with pytest.raises(ValueError, match="give keys, mask or both"):
            ix.row_filter()
        with pytest.raises(TypeError, match="keys must be a torch.Tensor"):
            ix.row_filter(keys=[1, 2, 3])
        with pytest.raises(RuntimeError, match="keys: the index runs on a HIP device only"):
            ix.row_filter(keys=torch.zeros(100, dtype=i32))
        with pytest.raises(RuntimeError, match="mask: the index runs on a HIP device only"):
            ix.row_filter(mask=torch.ones(100, dtype=torch.bool))
        for bad in (fake(100, dtype=torch.int64), fake(100), fake(100, 1, dtype=i32), fake(0, dtype=i32)):
            with pytest.raises(ValueError, match=r"keys must be int32 \[n\]"):
                ix.row_filter(keys=bad)
        for bad in (fake(100, dtype=torch.uint8), fake(100, dtype=i32), fake(4, 25, dtype=torch.bool), fake(0, dtype=torch.bool)):
            with pytest.raises(ValueError, match=r"mask must be bool \[n\]"):
                ix.row_filter(keys=fake(100, dtype=i32), mask=bad)
        with pytest.raises(AssertionError, match="reached the device"):  # nothing left to refuse
            ix.row_filter(keys=fake(100, dtype=i32), mask=fake(90, dtype=torch.bool))
        keyed, plain = RowFilter(fake(48, dtype=i32), fake(48, dtype=i32)), RowFilter(fake(48, dtype=i32), None)
        qk = fake(5, dtype=i32)
        monkeypatch.setattr(index, "normalize_rows", boom)  # every refusal below comes before anything is normalised
        for bad in ("=", "is", None, 2, "=<", "<>"):
            with pytest.raises(ValueError, match="match = .*one of == != < <= > >="):
                ix.search(q, rows=keyed, query_keys=qk, match=bad)
        with pytest.raises(ValueError, match="query_keys needs rows="):
            ix.search(q, query_keys=qk)
        with pytest.raises(ValueError, match="query_keys needs a RowFilter built with keys"):
            ix.search(q, rows=plain, query_keys=qk)
        for bad in (fake(48, dtype=i32), (fake(48, dtype=i32), None), "rows"):
            with pytest.raises(TypeError, match="rows must be a RowFilter"):
                ix.search(q, rows=bad)
        for bad in (RowFilter(fake(32, dtype=i32), None), RowFilter(fake(64, dtype=i32), fake(64, dtype=i32)),
                    RowFilter(fake(48, dtype=torch.int64), None)):
            with pytest.raises(ValueError, match=r"rows: a RowFilter of .* slots, this index has \[48\]"):
                ix.search(q, rows=bad)
        with pytest.raises(RuntimeError, match="rows.ids: the index runs on a HIP device only"):
            ix.search(q, rows=RowFilter(torch.zeros(48, dtype=i32), None))
        with pytest.raises(TypeError, match="query_keys must be a torch.Tensor"):
            ix.search(q, rows=keyed, query_keys=[0] * 5)
        with pytest.raises(RuntimeError, match="query_keys: the index runs on a HIP device only"):
            ix.search(q, rows=keyed, query_keys=torch.zeros(5, dtype=i32))
        for bad in (fake(4, dtype=i32), fake(6, dtype=i32), fake(5, 1, dtype=i32), fake(5, dtype=torch.int64), fake(5)):
            with pytest.raises(ValueError, match=r"query_keys must be int32 \[5\]"):
                ix.search(q, rows=keyed, query_keys=bad)
        with pytest.raises(TypeError):  # keyword-only
            ix.search(q, 1, 1, None, None, keyed) if isinstance(ix, IVFInt8Index) else ix.search(q, 1, 1, None, None, None, None, keyed)
        monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=f16))
    # range_search takes the same three
    ix = IVFFlatIndex(fake(3, 64))
    ix._added = True
    ix._rows, ix._ids, ix._offsets = fake(48, 64, dtype=f16), fake(48, dtype=i32), fake(4, dtype=i32)
    keyed = RowFilter(fake(48, dtype=i32), fake(48, dtype=i32))
    monkeypatch.setattr(index, "normalize_rows", boom)
    with pytest.raises(ValueError, match="match = 'like'"):
        ix.range_search(q, 0.5, rows=keyed, query_keys=fake(5, dtype=i32), match="like")
    with pytest.raises(ValueError, match="query_keys needs rows="):
        ix.range_search(q, 0.5, query_keys=fake(5, dtype=i32))
    with pytest.raises(ValueError, match=r"this index has \[48\]"):
        ix.range_search(q, 0.5, rows=RowFilter(fake(16, dtype=i32), None))
    with pytest.raises(ValueError, match=r"query_keys must be int32 \[5\]"):
        ix.range_search(q, 0.5, rows=keyed, query_keys=fake(7, dtype=i32))
    # the functional form: the three trailing arguments go together and are checked
    qn, sto = fake(256, 64, dtype=f16), (fake(48, 64, dtype=f16), fake(48, dtype=i32), fake(4, dtype=i32))
    pr, sk, qk = fake(5, 2, dtype=i32), fake(48, dtype=i32), fake(5, dtype=i32)
    for fn, args in ((index.search_lists, (qn, pr, *sto, 4)), (index.range_search_lists, (qn, pr, fake(5), *sto, True, None)),
                     (index.search_lists_int8, (qn, pr, fake(48, 64, dtype=torch.int8), fake(48), *sto[1:], 4)),
                     (index.search_lists_pq, (qn, pr, fake(48, 8, dtype=torch.uint8), cb, *sto[1:], 4)),
                     (index.search_lists_pq_residual, (qn, pr, fake(5, 2), fake(48, 8, dtype=torch.uint8), cb, *sto[1:], 4))):
        for bad in ((sk, qk, None), (sk, None, 2), (None, qk, 2), (None, None, 2)):
            with pytest.raises(ValueError, match="slot_keys, query_keys and accept go together"):
                fn(*args, *bad)
        for bad in (-1, 8, 2.0, True, "=="):
            with pytest.raises(ValueError, match="accept = .*3-bit mask"):
                fn(*args, sk, qk, bad)
        for bad in (fake(47, dtype=i32), fake(48, dtype=torch.int64), fake(48, 1, dtype=i32)):
            with pytest.raises(ValueError, match=r"slot_keys must be int32 \[48\]"):
                fn(*args, bad, qk, 2)
        for bad in (fake(6, dtype=i32), fake(5, dtype=torch.int64)):
            with pytest.raises(ValueError, match=r"query_keys must be int32 \[5\]"):
                fn(*args, sk, bad, 2)
        with pytest.raises(RuntimeError, match="slot_keys: the index runs on a HIP device only"):
            fn(*args, torch.zeros(48, dtype=i32), qk, 2)
        with pytest.raises(AssertionError, match="reached the device"):  # nothing left to refuse
            fn(*args, sk, qk, 2)
