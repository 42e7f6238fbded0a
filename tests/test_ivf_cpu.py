"""CPU: the IVF-Flat index -- the numpy restatement against brute force and against a plain loop, the slot bound and the
alignment rule, the planted-data condition the GPU tests rely on, and every refusal of the Python layer and of the C-ABI
(sonar_amd/index.py, sonar_amd/csrc/ivf.hip, tests/ivf_ref.py).  Nothing here needs a device."""
import itertools

import numpy as np
import pytest
import torch

from tests import ivf_ref as R
from tests import kmeans_ref as KR

INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def _skipping_labels(rng, n, k):
    labels = rng.integers(0, k, n).astype(np.int64)
    skip = rng.random(n) < 0.3
    labels[skip] = rng.choice([-1, k, INT32_MAX], size=int(skip.sum()))
    return labels


@pytest.mark.parametrize("n,k,d", [(1, 1, 64), (300, 3, 128), (257, 7, 64), (130, 16, 1024)])
def test_every_list_probed_equals_stable_sorted_brute_force(n, k, d):
    rng = np.random.default_rng(n + k)
    x, q = R.integer_rows(rng, n, d), R.integer_rows(rng, 33, d)
    q[0] = 0  # every candidate ties: the lowest row numbers
    labels = rng.integers(0, k, n)
    probes = np.stack([rng.permutation(k) for _ in range(len(q))])  # every list, in any order
    s = R.scores64(q, x)
    assert np.array_equal(s, np.rint(s)) and np.abs(s).max() < 2 ** 11  # exact in fp32 in any order
    for kk in (1, 4, 8):
        got, want = R.search(q, x, labels, k, probes, kk, s=s), R.brute_force(q, x, kk, s=s)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert list(want[1][0][: min(kk, n)]) == list(range(min(kk, n)))


def test_restated_search_edges():
    rng = np.random.default_rng(2)
    x, q = R.integer_rows(rng, 40, 64), R.integer_rows(rng, 3, 64)
    labels = np.arange(40) % 4
    labels[:3] = [-1, 4, INT32_MAX]  # rows 0..2 are in no list
    s, i = R.search(q, x, labels, 4, [[-1, 9], [0, -1], [3, 3]], 8)
    assert (i[0] == -1).all() and np.isneginf(s[0]).all()  # no list named: k x (-inf, -1)
    assert set(i[1].tolist()) <= set(range(4, 40, 4))  # list 0 without row 0: 9 rows, the 8 best
    assert len(set(i[1].tolist())) == 8 and (np.diff(s[1]) <= 0).all()
    assert np.array_equal(i[2][0::2], i[2][1::2]) and np.array_equal(s[2][0::2], s[2][1::2])  # a list named twice: twice
    s3, i3 = R.search(q, x[:5], np.array([0, 0, 1, 1, 1]), 2, [[0]] * 3, 4)  # fewer than k candidates
    assert (i3[:, 2:] == -1).all() and np.isneginf(s3[:, 2:]).all() and (i3[:, :2] >= 0).all()
    # ties: equal scores come out by ascending id whatever list they sit in
    xt = np.tile(x[:1], (6, 1))
    st, it = R.search(x[:1], xt, [1, 0, 1, 0, 1, 0], 2, [[1, 0]], 4)
    assert it[0].tolist() == [0, 1, 2, 3] and len(set(st[0].tolist())) == 1


@pytest.mark.parametrize("n,k", R.BOUND_CROSSES)
def test_restated_build_equals_a_plain_loop_and_respects_the_bound(n, k, lib):
    rng = np.random.default_rng(n * 7 + k)
    a = lib.smi_ivf_list_align()
    assert a == R.ALIGN and a in (16, 32, 64)
    bound = lib.smi_ivf_slots_bound(n, k)
    assert bound == R.slots_bound(n, k)
    kinds = {
        "random": rng.integers(0, k, n),
        "sorted": np.sort(rng.integers(0, k, n)),
        "reversed": np.sort(rng.integers(0, k, n))[::-1],
        "one list": np.full(n, k - 1),
        "skips": _skipping_labels(rng, n, k),
        "one row each": np.arange(n) % k,  # the labelling that pads the most
    }
    worst = 0
    for name, labels in kinds.items():
        off, sizes, ids = R.build(labels, k)
        off2, sizes2, ids2 = R.build_loop(labels, k)
        assert np.array_equal(off, off2) and np.array_equal(sizes, sizes2) and np.array_equal(ids, ids2), name
        assert (off % a == 0).all() and off[k] <= bound, name
        assert np.array_equal(np.diff(off), R.round_up(sizes)), name
        real = ids[ids >= 0]
        ok = (np.asarray(labels) >= 0) & (np.asarray(labels) < k)
        assert len(set(real.tolist())) == len(real) == int(ok.sum()) == sizes.sum(), name
        for c in range(min(k, 20)):
            seg = ids[off[c]: off[c + 1]]
            assert (seg[: sizes[c]] >= 0).all() and (seg[sizes[c]:] == -1).all(), name
            assert (np.asarray(labels)[seg[: sizes[c]]] == c).all(), name
        worst = max(worst, int(off[k]))
    # the bound is attained: min(n, k) lists hold one row each and list 0 takes all the others
    m = min(n, k)
    tight = np.concatenate([np.arange(m), np.zeros(n - m, dtype=np.int64)])
    assert R.build(tight, k)[0][k] == bound and worst <= bound


def test_slot_bound_is_the_maximum_over_all_labellings_of_small_cases():
    for n, k, a in [(5, 2, 4), (6, 3, 4), (4, 5, 4), (7, 2, 2), (9, 3, 4)]:
        most = 0
        for labels in itertools.product(range(k), repeat=n):
            most = max(most, int(R.build(labels, k, a)[0][k]))
        assert most == R.slots_bound(n, k, a), (n, k, a)


@pytest.mark.parametrize("d", [64, 1024])
def test_planted_neighbours_are_found_at_nprobe_1_by_the_restatement(d):
    """The generator of tests/test_gpu_ivf.py through float64 alone: k-means recovers the planted lists, every query's
    nearest list is its target's, by a margin fp16 centroids and fp32 sums cannot overturn, and its best candidate there
    is the target, by a margin far above the engine's d * 2^-23."""
    n, k, nq = 4096, 16, 257
    x, truth, _, q, target = R.planted(n, k, d, nq)
    rounds = KR.fit(x, x[:k].copy(), 2)
    assert np.array_equal(rounds[-1]["labels"], truth)
    cn = KR.normalize64(rounds[-1]["centroids"])
    probe, _, margin = KR.assign(q, cn)
    assert np.array_equal(probe, truth[target]) and margin.min() >= 0.1, margin.min()
    s, i = R.search(q, x, truth, k, probe[:, None], 4)
    assert np.array_equal(i[:, 0], target)
    assert (s[:, 0] - s[:, 1]).min() >= 0.05, (s[:, 0] - s[:, 1]).min()


# ------------------------------------------------------------------------------------------------------- refusals
class FakeDevice(torch.Tensor):
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta").as_subclass(FakeDevice)


def boom(*a, **k):
    raise AssertionError("reached the device")


def test_python_refusals_need_no_device(monkeypatch):
    from sonar_amd import index
    from sonar_amd.clustering import SphericalKMeans
    from sonar_amd.index import IVFFlatIndex

    assert index.LIST_ALIGN == R.ALIGN and index.UNIT_QUERIES == 64
    with pytest.raises(RuntimeError, match="before fit"):
        IVFFlatIndex(SphericalKMeans(3))
    with pytest.raises(TypeError):
        IVFFlatIndex(np.zeros((3, 64)))
    with pytest.raises(RuntimeError, match=r"HIP device only \(no CPU path\)"):
        IVFFlatIndex(torch.zeros(3, 64))
    with pytest.raises(RuntimeError, match=r"HIP device only"):
        IVFFlatIndex.train(torch.zeros(8, 64), 3)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_clusters"):
            IVFFlatIndex.train(fake(8, 64), bad)

    monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=torch.float16))
    monkeypatch.setattr(index, "topk_normalized", boom)
    for shape, what in (((3,), r"\[rows, dim\]"), ((3, 96), "multiple of 64"), ((0, 64), "empty")):
        with pytest.raises(ValueError, match=what):
            IVFFlatIndex(fake(*shape))
    ix = IVFFlatIndex(fake(3, 64))
    assert ix.n_lists == 3 and ix.dim == 64
    monkeypatch.setattr(index._lib, "load", boom)
    for what in ("list_sizes", "list_offsets", "ntotal", "state_dict"):
        with pytest.raises(RuntimeError, match="before add"):
            v = getattr(ix, what)
            v() if callable(v) else None
    with pytest.raises(RuntimeError, match="before add"):
        ix.search(fake(5, 64))
    # add
    with pytest.raises(RuntimeError, match="HIP device only"):
        ix.add(torch.zeros(8, 64))
    with pytest.raises(TypeError):
        ix.add([[0.0] * 64])
    with pytest.raises(ValueError, match="dim 128"):
        ix.add(fake(8, 128))
    with pytest.raises(ValueError, match="multiple of 64"):
        ix.add(fake(8, 96))
    with pytest.raises(ValueError, match="empty"):
        ix.add(fake(0, 64))
    with pytest.raises(RuntimeError, match="HIP device only"):
        ix.add(fake(8, 64), labels=torch.zeros(8, dtype=torch.int32))
    for bad in (fake(8, dtype=torch.int64), fake(7, dtype=torch.int32), fake(8, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="labels must be int32"):
            ix.add(fake(8, 64), labels=bad)
    with pytest.raises(TypeError):
        ix.add(fake(8, 64), labels=[0] * 8)
    # search, on an index that claims to hold rows
    ix._added = True
    with pytest.raises(RuntimeError, match="already called"):
        ix.add(fake(8, 64))
    q = fake(5, 64)
    for bad in (0, 9, 1.0, True):
        with pytest.raises(ValueError, match=r"k = .*\[1, 8\]"):
            ix.search(q, k=bad)
        with pytest.raises(ValueError, match=r"nprobe = .*\[1, 8\]"):
            ix.search(q, nprobe=bad)
    with pytest.raises(ValueError, match="exceeds the 3 lists"):
        ix.search(q, nprobe=4)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ix.search(torch.zeros(5, 64))
    with pytest.raises(ValueError, match="dim 128"):
        ix.search(fake(5, 128))
    with pytest.raises(ValueError, match=r"\[rows, dim\]"):
        ix.search(fake(5))
    with pytest.raises(RuntimeError, match="HIP device only"):
        ix.search(q, probes=torch.zeros(5, 2, dtype=torch.int32))
    with pytest.raises(TypeError):
        ix.search(q, probes=[[0]] * 5)
    for bad in (fake(5, 2, dtype=torch.int64), fake(4, 2, dtype=torch.int32), fake(5, dtype=torch.int32),
                fake(5, 9, dtype=torch.int32), fake(5, 0, dtype=torch.int32)):
        with pytest.raises(ValueError, match="probes"):
            ix.search(q, probes=bad)
    # load_state_dict
    with pytest.raises(ValueError, match="lacks"):
        ix.load_state_dict({"centroids": fake(3, 64, dtype=torch.float16)})
    state = {"centroids": fake(3, 64, dtype=torch.float16), "offsets": fake(4, dtype=torch.int32),
             "sizes": fake(3, dtype=torch.int32), "ids": fake(16, dtype=torch.int32), "rows": fake(16, 64, dtype=torch.float16)}
    for key, bad, what in (("centroids", fake(4, 64, dtype=torch.float16), "this index has"),
                           ("centroids", fake(3, 64), "fp16"),
                           ("centroids", torch.zeros(3, 64, dtype=torch.float16), "HIP device only"),
                           ("offsets", fake(3, dtype=torch.int32), "offsets must be int32"),
                           ("sizes", fake(3, dtype=torch.int64), "sizes must be int32"),
                           ("ids", fake(15, dtype=torch.int32), "ids must be int32"),
                           ("rows", fake(16, 128, dtype=torch.float16), "rows must be fp16")):
        with pytest.raises((ValueError, RuntimeError), match=what):
            ix.load_state_dict({**state, key: bad})


def test_c_abi_sizing_and_refusals_without_a_device(lib):
    a = lib.smi_ivf_list_align()
    sb, bw, sw = lib.smi_ivf_slots_bound, lib.smi_ivf_build_workspace_bytes, lib.smi_ivf_search_workspace_bytes
    assert sb(1, 1) == a and sb(a + 1, 1) == 2 * a and sb(4099, 300) == 300 * a + (4099 - 300) // a * a
    assert sb(0, 3) == 0 and sb(3, 0) == 0 and sb(1 << 31, 3) == 0 and sb(3, 1 << 31) == 0
    assert sb(1 << 30, 1 << 30) == 0  # a * 2^30 slots do not fit int32
    assert bw(1000, 7, 1024) == 32 and bw(1000, 7, 1024) % 16 == 0  # cursor [K]
    assert bw(1000, 7, 96) == 0 and bw(1000, 0, 64) == 0 and bw(0, 7, 64) == 0 and bw(1 << 31, 7, 64) == 0
    assert bw(1 << 30, 1 << 30, 64) == 0
    # pair counts [K] | pair offsets [K + 1] | unit offsets [K + 1] | cursor [K] | pairs [nq nprobe] | 2 x [nprobe][nq][k]
    assert sw(100, 7, 4, 5, 64) == 2 * 32 + 2 * 32 + 1600 + 2 * 8000
    for bad in ((0, 7, 4, 5, 64), (100, 0, 4, 5, 64), (100, 7, 0, 5, 64), (100, 7, 9, 5, 64), (100, 7, 4, 0, 64),
                (100, 7, 4, 9, 64), (100, 7, 4, 5, 96), (1 << 31, 7, 1, 1, 64), (100, 1 << 31, 1, 1, 64),
                (1 << 29, 7, 8, 1, 64)):
        assert sw(*bad) == 0, bad
    p = 0x1000  # never dereferenced: every call below is refused on its arguments
    big = 1 << 40
    cap = sb(100, 7)
    B, S = lib.smi_ivf_build, lib.smi_ivf_search
    cases = {
        "build d": B(p, p, 100, 96, 7, p, p, cap, p, p, p, big, None),
        "build K": B(p, p, 100, 64, 0, p, p, cap, p, p, p, big, None),
        "build n": B(p, p, 0, 64, 7, p, p, cap, p, p, p, big, None),
        "build big n": B(p, p, 1 << 31, 64, 7, p, p, big, p, p, p, big, None),
        "build big K": B(p, p, 100, 64, 1 << 31, p, p, big, p, p, p, big, None),
        "build big slots": B(p, p, 1 << 30, 64, 1 << 30, p, p, big, p, p, p, big, None),
        "build null x": B(None, p, 100, 64, 7, p, p, cap, p, p, p, big, None),
        "build null labels": B(p, None, 100, 64, 7, p, p, cap, p, p, p, big, None),
        "build null rows": B(p, p, 100, 64, 7, None, p, cap, p, p, p, big, None),
        "build null ids": B(p, p, 100, 64, 7, p, None, cap, p, p, p, big, None),
        "build null offsets": B(p, p, 100, 64, 7, p, p, cap, None, p, p, big, None),
        "build null sizes": B(p, p, 100, 64, 7, p, p, cap, p, None, p, big, None),
        "build small capacity": B(p, p, 100, 64, 7, p, p, cap - 1, p, p, p, big, None),
        "build null ws": B(p, p, 100, 64, 7, p, p, cap, p, p, None, big, None),
        "build short ws": B(p, p, 100, 64, 7, p, p, cap, p, p, p, bw(100, 7, 64) - 1, None),
        "build misaligned ws": B(p, p, 100, 64, 7, p, p, cap, p, p, p + 8, big, None),
        "search d": S(p, 100, 96, p, 4, p, p, p, 7, 5, p, p, p, big, None),
        "search K": S(p, 100, 64, p, 4, p, p, p, 0, 5, p, p, p, big, None),
        "search nq": S(p, 0, 64, p, 4, p, p, p, 7, 5, p, p, p, big, None),
        "search big nq": S(p, 1 << 31, 64, p, 4, p, p, p, 7, 5, p, p, p, big, None),
        "search big pairs": S(p, 1 << 29, 64, p, 8, p, p, p, 7, 5, p, p, p, big, None),
        "search k 0": S(p, 100, 64, p, 4, p, p, p, 7, 0, p, p, p, big, None),
        "search k 9": S(p, 100, 64, p, 4, p, p, p, 7, 9, p, p, p, big, None),
        "search nprobe 0": S(p, 100, 64, p, 0, p, p, p, 7, 5, p, p, p, big, None),
        "search nprobe 9": S(p, 100, 64, p, 9, p, p, p, 7, 5, p, p, p, big, None),
        "search null q": S(None, 100, 64, p, 4, p, p, p, 7, 5, p, p, p, big, None),
        "search null probes": S(p, 100, 64, None, 4, p, p, p, 7, 5, p, p, p, big, None),
        "search null rows": S(p, 100, 64, p, 4, None, p, p, 7, 5, p, p, p, big, None),
        "search null ids": S(p, 100, 64, p, 4, p, None, p, 7, 5, p, p, p, big, None),
        "search null offsets": S(p, 100, 64, p, 4, p, p, None, 7, 5, p, p, p, big, None),
        "search null idx": S(p, 100, 64, p, 4, p, p, p, 7, 5, None, p, p, big, None),
        "search null score": S(p, 100, 64, p, 4, p, p, p, 7, 5, p, None, p, big, None),
        "search null ws": S(p, 100, 64, p, 4, p, p, p, 7, 5, p, p, None, big, None),
        "search short ws": S(p, 100, 64, p, 4, p, p, p, 7, 5, p, p, p, sw(100, 7, 4, 5, 64) - 1, None),
        "search misaligned ws": S(p, 100, 64, p, 4, p, p, p, 7, 5, p, p, p + 4, big, None),
    }
    assert all(rc != 0 for rc in cases.values()), {k: v for k, v in cases.items() if v == 0}
    assert B(p, p, 100, 64, 7, p, p, cap - 1, p, p, p, big, None) == -1 and b"smi_ivf_slots_bound" in lib.smi_last_error()
    assert B(p, p, 100, 96, 7, p, p, cap, p, p, p, big, None) == -2 and b"multiple of 64" in lib.smi_last_error()
    assert S(p, 100, 64, p, 4, p, p, p, 7, 5, p, p, p, 16, None) == -1
    assert b"smi_ivf_search_workspace_bytes" in lib.smi_last_error()
    assert S(p, 100, 64, p, 9, p, p, p, 7, 5, p, p, p, big, None) == -1 and b"nprobe" in lib.smi_last_error()
