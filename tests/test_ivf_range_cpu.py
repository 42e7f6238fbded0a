"""CPU: the range search over the IVF-Flat lists.  The numpy restatement (tests/ivf_range_ref.py) against
its plain-loop twin; the three C entries in the binding, the header and the library; every refusal of the C entries, in the
house order, and of the Python layer, none of which needs a device; and the planted-data condition the GPU test leans on."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import ivf_range_ref as G
from tests import ivf_ref as R
from tests.test_ivf_cpu import FakeDevice, boom, fake  # noqa: F401  (the stand-ins for device tensors)

INT32_MAX = 2 ** 31 - 1
NAMES = ("smi_range_search_ws_bytes", "smi_range_search_count", "smi_range_search_emit")


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


# ------------------------------------------------------------------------------------------------------- restatement
def _same(a, b):
    return all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))


def test_restatement_equals_a_plain_loop():
    rng = np.random.default_rng(0)
    n, k_lists, nq = 90, 5, 14
    x, q = R.integer_rows(rng, n, 64), R.integer_rows(rng, nq, 64)
    x[7] = x[40] = x[41] = x[3]  # ties: equal rows in different lists and in one
    q[0] = 0                     # every candidate scores 0
    labels = rng.integers(0, k_lists, n)
    labels[labels == 3] = -1     # an empty list, rows in no list
    labels[[3, 7, 40, 41]] = [0, 1, 1, 2]
    probes = np.stack([rng.permutation(k_lists)[:3] for _ in range(nq)])
    probes[1] = [1, 1, 2]                  # a list named twice: its hits twice
    probes[2] = [-1, k_lists, INT32_MAX]   # names no list
    probes[3] = [3, 3, -1]                 # the empty list
    probes[4, 1] = -1
    s = R.scores64(q, x)
    thr = np.array([np.sort(s[r])[::-1][r % 9] for r in range(nq)], dtype=np.float32)  # equal to one of the scores
    thr[0], thr[5], thr[6], thr[7], thr[8] = 0.0, -np.inf, np.nan, -3.0, np.inf
    got, want = G.range_search(q, x, labels, k_lists, probes, thr, s=s), G.range_search_loop(q, x, labels, k_lists, probes, thr)
    assert _same(got, want)
    lims, sc, ids = got
    assert lims[0] == 0 and len(lims) == nq + 1 and lims[-1] == len(sc) == len(ids) and (np.diff(lims) >= 0).all()
    # the queries that name no list or an empty one, a NaN and a +inf threshold: no hit
    assert lims[3] - lims[2] == 0 and lims[4] - lims[3] == 0 and lims[7] - lims[6] == 0 and lims[9] - lims[8] == 0
    # threshold 0 on the all-zero query and -inf: every row of the probed lists
    for r in (0, 5):
        assert lims[r + 1] - lims[r] == sum(int((labels == c).sum()) for c in probes[r] if 0 <= c < k_lists)
    assert (ids[lims[0]: lims[1]] == np.sort(ids[lims[0]: lims[1]])).all()  # all ties: id order
    # the list named twice: every hit twice, neighbours in the order
    seg = ids[lims[1]: lims[2]]
    twice = seg[np.isin(seg, np.flatnonzero(labels == 1))]
    assert len(twice) % 2 == 0 and (twice[::2] == twice[1::2]).all()
    for r in range(nq):
        a, b = lims[r], lims[r + 1]
        assert (np.diff(sc[a:b]) <= 0).all() and (sc[a:b].astype(np.float32) >= thr[r]).all()
    # a float threshold is compared in fp32: 0.1 (float64) is below float32(0.1), which a score of float32(0.1) still meets
    x1, q1 = np.array([[np.float32(0.1)] + [0] * 63], dtype=np.float64), np.array([[1.0] + [0] * 63])
    assert len(G.range_search(q1, x1, [0], 1, [[0]], [0.1])[2]) == len(G.range_search_loop(q1, x1, [0], 1, [[0]], [0.1])[2]) == 1


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_symbols_are_bound_declared_and_exported(lib):
    from sonar_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sonar_mi355.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert name in _lib.SYMBOLS and f" {name}(" in header and f" T {name}\n" in exported, name
    assert lib.smi_abi_version() == 7 and "#define SMI_ABI_VERSION 7" in header
    # the names stay clear of the patterns two recorded goldens close over
    assert not any(n.startswith(("smi_ivf_", "smi_pq_")) or n.endswith("_workspace_bytes") for n in NAMES)


def test_c_abi_sizing_and_refusals_without_a_device(lib):
    if lib.smi_device_count() > 0:
        pytest.skip("a HIP device is visible: the made-up pointers must never reach a kernel")
    sz, count, emit = (getattr(lib, n) for n in NAMES)
    # the inverted probe table and nothing else: counts [K] | offsets [K + 1] | unit offsets [K + 1] | cursor [K] | pairs [P]
    assert sz(100, 7, 4, 64) == 32 + 32 + 32 + 32 + 1600 and sz(3, 1, 1, 1024) == 16 * 5 and sz(300, 513, 8, 192) % 16 == 0
    p, big = 0x1000, 1 << 40  # never dereferenced: every call below is refused
    need = sz(100, 7, 4, 64)
    good_c = dict(qn=p, nq=100, d=64, probes=p, nprobe=4, threshold=p, rows=p, ids=p, offsets=p, K=7, pair_counts=p, ws=p,
                  ws_bytes=big, stream=None)
    good_e = dict(qn=p, nq=100, d=64, probes=p, nprobe=4, threshold=p, rows=p, ids=p, offsets=p, K=7, pair_base=p, total=5,
                  score=p, idx=p, ws=p, ws_bytes=big, stream=None)
    # (change, the text of the refusal, whether it is a refusal on shape: the sizing call returns 0 exactly there)
    shared = [
        ({"qn": None}, "null argument", False), ({"probes": None}, "null argument", False),
        ({"threshold": None}, "null argument", False), ({"rows": None}, "null argument", False),
        ({"ids": None}, "null argument", False), ({"offsets": None}, "null argument", False),
        ({"d": 96}, "d=96 must be a multiple of 64", True), ({"d": 0}, "d=0 must be a multiple of 64", True),
        ({"K": 0}, "K=0: at least one list", True), ({"nq": 0}, "nq=0: empty input", True),
        ({"nq": 1 << 31}, "must fit int32", True), ({"K": 1 << 31}, "must fit int32", True),
        ({"nprobe": 0}, "nprobe=0 must be in [1, 8]", True), ({"nprobe": 9}, "nprobe=9 must be in [1, 8]", True),
        ({"nq": 1 << 29, "nprobe": 8}, "nq * nprobe = 4294967296 must fit int32", True),
        ({"ws": None}, "null workspace", False), ({"ws": p + 8}, "workspace must be 16-byte aligned", False),
        ({"ws_bytes": need - 1}, f"workspace of {need - 1} bytes, smi_range_search_ws_bytes(nq, K, nprobe, d) = {need}", False),
        # two at once: the first in the house order answers
        ({"qn": None, "d": 96}, "null argument", True), ({"d": 96, "K": 0}, "d=96 must be a multiple of 64", True),
        ({"K": 0, "nq": 0}, "K=0: at least one list", True), ({"nq": 0, "nprobe": 9}, "nq=0: empty input", True),
        ({"nprobe": 9, "ws": None}, "nprobe=9 must be in [1, 8]", True),
        ({"nq": 1 << 29, "nprobe": 8, "ws": None}, "nq * nprobe = 4294967296 must fit int32", True),
        ({"ws": None, "ws_bytes": 0}, "null workspace", False), ({"ws": p + 4, "ws_bytes": 0}, "workspace must be 16-byte aligned", False),
    ]
    own_c = [({"pair_counts": None}, "null argument", False), ({"pair_counts": None, "nprobe": 9}, "null argument", True),
             ({}, "no HIP device visible", False)]
    own_e = [({"pair_base": None}, "null argument", False), ({"score": None}, "null argument", False),
             ({"idx": None}, "null argument", False), ({"idx": None, "total": -1}, "null argument", False),
             ({"total": -1}, "total=-1: the last entry of pair_base", False),
             ({"total": -1, "ws_bytes": need - 1}, f"workspace of {need - 1} bytes", False),
             ({"total": -1, "nprobe": 0}, "nprobe=0 must be in [1, 8]", True),
             ({"total": 0}, "no HIP device visible", False), ({}, "no HIP device visible", False)]
    wrong = []
    for fn, good, cases in ((count, good_c, shared + own_c), (emit, good_e, shared + own_e)):
        for change, text, on_shape in cases:
            call = {**good, **change}
            rc = fn(*call.values())
            err = lib.smi_last_error().decode()
            bytes_ = sz(call["nq"], call["K"], call["nprobe"], call["d"])
            after = lib.smi_last_error().decode()
            if rc == 0 or text not in err or after != err or (bytes_ == 0) != on_shape:
                wrong.append((fn.__name__, change, text, rc, err, after, bytes_))
    assert not wrong, wrong[:5]
    # the codes: an argument, a shape, no device
    assert count(None, 100, 64, p, 4, p, p, p, p, 7, p, p, big, None) == emit(*{**good_e, "total": -1}.values()) != 0
    codes = {count(*{**good_c, **c}.values()) for c in ({"d": 96}, {"nq": 1 << 31}, {"nq": 1 << 29, "nprobe": 8})}
    assert len(codes) == 1 and codes.isdisjoint({0, count(*{**good_c, "nprobe": 9}.values()), count(*good_c.values())})


# ------------------------------------------------------------------------------------------------------- Python refusals
def test_python_refusals_need_no_device(monkeypatch):
    from sonar_amd import index
    from sonar_amd.index import IVFFlatIndex, IVFInt8Index, IVFPQIndex, IVFPQResidualIndex, RangeResult

    f16, f32, i32 = torch.float16, torch.float32, torch.int32
    monkeypatch.setattr(index._lib, "load", boom)
    monkeypatch.setattr(index, "topk_normalized", boom)
    monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=f16))
    cb = fake(8, 256, 8, dtype=f16)
    for other, holds in ((IVFInt8Index(fake(3, 64)), "an IVFInt8Index holds int8 codes"),
                         (IVFPQIndex(fake(3, 64), cb), "an IVFPQIndex holds product-quantiser codes"),
                         (IVFPQResidualIndex(fake(3, 64), cb), "an IVFPQResidualIndex holds product-quantiser codes of residuals")):
        with pytest.raises(TypeError, match=f"range_search needs the fp16 lists of an IVFFlatIndex; {holds}"):
            other.range_search(fake(5, 64), 0.5)
    ix = IVFFlatIndex(fake(3, 64))
    q = fake(5, 64)
    with pytest.raises(RuntimeError, match="range_search before add"):
        ix.range_search(q, 0.5)
    ix._added = True
    ix._rows, ix._ids, ix._offsets = fake(48, 64, dtype=f16), fake(48, dtype=i32), fake(4, dtype=i32)
    monkeypatch.setattr(index, "normalize_rows", boom)  # every refusal below comes before anything is normalised
    for bad in (0, 9, 1.0, True):
        with pytest.raises(ValueError, match=r"nprobe = .*\[1, 8\]"):
            ix.range_search(q, 0.5, nprobe=bad)
    with pytest.raises(ValueError, match="exceeds the 3 lists"):
        ix.range_search(q, 0.5, nprobe=4)
    with pytest.raises(ValueError, match="dim 128"):
        ix.range_search(fake(5, 128), 0.5)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ix.range_search(torch.zeros(5, 64), 0.5)
    for bad in (fake(5, 2, dtype=torch.int64), fake(4, 2, dtype=i32), fake(5, 9, dtype=i32), fake(5, dtype=i32)):
        with pytest.raises(ValueError, match="probes"):
            ix.range_search(q, 0.5, probes=bad)
    for bad in ("0.5", None, [0.5] * 5, np.zeros(5, dtype=np.float32), True):
        with pytest.raises(TypeError, match="threshold must be a torch.Tensor"):
            ix.range_search(q, bad)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ix.range_search(q, torch.zeros(5))
    for bad in (fake(4), fake(6), fake(5, 1), fake(5, dtype=f16), fake(5, dtype=torch.float64), fake(1)):
        with pytest.raises(ValueError, match=r"threshold must be a float or fp32 \[5\]"):
            ix.range_search(q, bad)
    with pytest.raises(ValueError, match="threshold is NaN"):
        ix.range_search(q, float("nan"))
    for bad in (-1, 1.0, True):
        with pytest.raises(ValueError, match="max_total"):
            ix.range_search(q, 0.5, max_total=bad)
    # the functional form
    qn, args = fake(256, 64, dtype=f16), (fake(48, 64, dtype=f16), fake(48, dtype=i32), fake(4, dtype=i32))
    with pytest.raises(ValueError, match="contiguous fp16"):
        index.range_search_lists(fake(256, 64), fake(5, 2, dtype=i32), fake(5), *args)
    for bad in (fake(257, 2, dtype=i32), fake(5, 9, dtype=i32), fake(5, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="probes"):
            index.range_search_lists(qn, bad, fake(5), *args)
    with pytest.raises(ValueError, match="qn has dim 64, the lists 128"):
        index.range_search_lists(qn, fake(5, 2, dtype=i32), fake(5), fake(48, 128, dtype=f16), *args[1:])
    with pytest.raises(ValueError, match=r"fp32 \[5\]"):
        index.range_search_lists(qn, fake(5, 2, dtype=i32), fake(6), *args)
    with pytest.raises(ValueError, match="max_total"):
        index.range_search_lists(qn, fake(5, 2, dtype=i32), fake(5), *args, max_total=-2)
    with pytest.raises(AssertionError, match="reached the device"):  # nothing left to refuse
        index.range_search_lists(qn, fake(5, 2, dtype=i32), fake(5), *args)
    # the result type
    res = RangeResult(torch.tensor([0, 2, 2, 5]), torch.zeros(5), torch.zeros(5, dtype=i32))
    assert res.counts.tolist() == [2, 0, 3] and res[0] is res.lims and len(res) == 3


# ------------------------------------------------------------------------------------------------------- planted data
@pytest.mark.parametrize("n,k,d,nq", [(4000, 16, 256, 200), (3000, 12, 1024, 130)])
def test_planted_data_conditions_the_gpu_test_relies_on(n, k, d, nq):
    """No float64 score of a query against any row lies within 1e-3 of the thresholds 0.9 and 0.45 (the
    fp32 accumulation moves a score by at most d * 2^-23 <= 1.3e-4); at 0.9 the only hit is the target, at 0.45 the hits
    are the target's cluster."""
    x, labels, centres, q, target = R.planted(n, k, d, nq, seed=11)
    assert d * 2.0 ** -23 <= 1.3e-4 < 1e-3
    s = R.scores64(q, x)
    own = labels[None, :] == labels[target][:, None]  # the rows of the list a query probes at nprobe = 1
    assert (own.sum(axis=1) == n // k).all() and n // k == 250
    for t in (0.9, 0.45):
        assert np.abs(s - t).min() > 1e-3
    hit9, hit45 = s >= 0.9, s >= 0.45
    assert (hit9.sum(axis=1) == 1).all() and hit9[np.arange(nq), target].all()
    assert np.array_equal(hit45, own)
    # the queries' nearest centre is their target's: nprobe = 1 by the quantiser probes that list
    assert np.array_equal((R.normalize64(q) @ centres.T).argmax(axis=1), labels[target])
