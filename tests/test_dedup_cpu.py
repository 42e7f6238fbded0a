"""CPU: semantic de-duplication -- the numpy restatement (tests/dedup_ref.py) against a plain double loop and against the
literal SemDeDup recipe, its tie rules, the planted-data condition the GPU test relies on, and every refusal of the Python
layer and of the C-ABI with its sizing function (sonar_amd/dedup.py, sonar_amd/csrc/ivf.hip).  Nothing here needs a device."""
import numpy as np
import pytest
import torch

from tests import dedup_ref as D
from tests import ivf_ref as R

INT32_MAX = 2 ** 31 - 1

# the planted data of tests/test_gpu_dedup.py: 1024 groups of 4 rows over 8 lists, d = 1024
PLANTED = dict(n_groups=1024, group_size=4, k=8, d=1024, seed=0)
THRESHOLD = 0.9


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def _priorities(rng, n):
    return {"none": None, "random": rng.standard_normal(n).astype(np.float32),
            "ties": rng.integers(0, 3, n).astype(np.float32)}


@pytest.mark.parametrize("n,k,d", [(1, 1, 64), (40, 3, 64), (150, 4, 128), (70, 300, 64)])
def test_restatement_equals_the_double_loop(n, k, d):
    rng = np.random.default_rng(n + k)
    x = R.integer_rows(rng, n, d)
    if n > 20:
        x[7], x[19] = x[3], x[3]  # exact duplicates: ties among the candidates
    labels = rng.integers(0, k, n)
    labels[rng.random(n) < 0.2] = -1
    if n > 20:
        labels[[3, 7, 19]] = 0
    off, _, ids = R.build(labels, k)
    for name, p in _priorities(rng, n).items():
        got_s, got_i = D.self_join(x, ids, off, n, p)
        want_s, want_i = D.self_join_loop(x, ids, off, n, p)
        assert np.array_equal(got_s, want_s) and np.array_equal(got_i, want_i), name
        assert np.array_equal(got_s[got_i >= 0], np.rint(got_s[got_i >= 0]))  # integer rows: exact integer scores
        assert (got_s[labels < 0] == -np.inf).all() and (got_i[labels < 0] == -1).all()  # rows in no list
        assert np.array_equal(got_i < 0, got_s == -np.inf)
        for i in np.flatnonzero(got_i >= 0):
            j = got_i[i]
            assert labels[j] == labels[i] and j != i
            assert D.precedes(0 if p is None else p[j], j, 0 if p is None else p[i], i)


def test_restatement_equals_the_semdedup_recipe_on_unique_priorities():
    rng = np.random.default_rng(5)
    n, k, d = 200, 3, 64
    x = R.normalize64(rng.standard_normal((n, d))).astype(np.float16)
    labels = rng.integers(0, k, n)
    priority = rng.permutation(n).astype(np.float32)  # unique
    off, _, ids = R.build(labels, k)
    max_sim, nearest = D.self_join(x, ids, off, n, priority)
    for c in range(k):
        m, col_max = D.semdedup_recipe(x, np.flatnonzero(labels == c), priority)
        assert (np.diff(priority[m]) < 0).all()
        assert np.array_equal(max_sim[m], col_max)
        assert nearest[m[0]] == -1 and (nearest[m[1:]] >= 0).all()  # the best row of a cluster has no predecessor
    for thr in (0.0, 0.2, 0.5):  # SemDeDup drops the columns whose max exceeds 1 - eps
        keep = D.keep_mask(max_sim, thr)
        assert np.array_equal(~keep, max_sim > thr) and keep[max_sim == -np.inf].all()


def test_tie_rules():
    # list 0 = rows 0 .. 5; rows 1, 2, 4 are copies of one row: equal scores against everything
    x = np.zeros((6, 64), dtype=np.float16)
    x[0, :4], x[1, :2], x[3, :3], x[5, 1:3] = 1, 1, 1, 1
    x[2], x[4] = x[1], x[1]
    off, _, ids = R.build(np.zeros(6, dtype=np.int64), 1)
    s, i = D.self_join(x, ids, off, 6)
    # no priority: the first occurrence is kept; equal scores go to the lower id
    assert i.tolist() == [-1, 0, 0, 0, 0, 0] and s.tolist() == [-np.inf, 2, 2, 3, 2, 2]
    # row 5 scores 1 against rows 1, 2 and 4 and 2 against rows 0 and 3: the lower id of the best score
    assert s[5] == 2 and i[5] == 0
    p = np.array([0, 5, 5, 1, 5, 0], dtype=np.float32)  # equal priorities: the lower id precedes
    s, i = D.self_join(x, ids, off, 6, p)
    # row 0 comes after rows 1, 2, 4 (score 2) and 3 (score 3); row 3 after 1, 2, 4, which tie at 2 -> id 1; row 5 after all:
    # rows 0 and 3 tie at 2 -> id 0
    assert i.tolist() == [3, -1, 1, 1, 1, 0] and s.tolist() == [3, -np.inf, 2, 2, 2, 2]
    # a strict threshold: a score equal to it is kept
    assert D.keep_mask(s, 3.0).all() and D.keep_mask(s, 2.0).tolist() == [False, True, True, True, True, True]
    assert D.keep_mask(s, 1.5).tolist() == [False, True, False, False, False, False]
    # a row alone in its list, and pad slots, contribute nothing
    off, _, ids = R.build(np.array([0, 1, 1, -1, 7, 1]), 2)
    s, i = D.self_join(x, ids, off, 6)
    assert i.tolist() == [-1, -1, 1, -1, -1, 1] and s[[0, 3, 4]].tolist() == [-np.inf] * 3


def test_planted_groups_have_the_gap_the_gpu_test_relies_on():
    x, labels, group = D.planted_groups(**PLANTED)
    n, d, k = len(x), PLANTED["d"], PLANTED["k"]
    assert x.dtype == np.float16 and x.shape == (4096, 1024) and np.array_equal(labels, group % k)
    assert (np.bincount(group) == PLANTED["group_size"]).all()
    xn = R.normalize64(x.astype(np.float64))
    s = xn @ xn.T  # ALL pairs, not only those of a list: the condition holds under any clustering of the rows
    same = group[:, None] == group[None, :]
    lo_in, hi_out = s[same & ~np.eye(n, dtype=bool)].min(), s[~same].max()
    assert lo_in > 0.95 and hi_out < 0.5, (lo_in, hi_out)
    off, _, ids = R.build(labels, k)
    max_sim, nearest = D.self_join(xn, ids, off, n)
    finite = max_sim[nearest >= 0]
    # in-group pairs above 0.95, every other pair below 0.5: no decision within 0.05 of the threshold, 400 times the tolerance
    assert np.abs(finite - THRESHOLD).min() > 0.05 > 400 * d * 2.0 ** -23
    keep = D.keep_mask(max_sim, THRESHOLD)
    first = np.array([np.flatnonzero(group == g)[0] for g in range(PLANTED["n_groups"])])
    assert keep.sum() == PLANTED["n_groups"] and keep[first].all()  # the first row of every group, and nothing else


# ------------------------------------------------------------------------------------------------------- refusals
class FakeDevice(torch.Tensor):
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta").as_subclass(FakeDevice)


def boom(*a, **k):
    raise AssertionError("reached the device")


def test_python_refusals_need_no_device(monkeypatch):
    from sonar_amd import dedup, index
    from sonar_amd.index import IVFFlatIndex, IVFInt8Index

    monkeypatch.setattr(dedup._lib, "load", boom)
    monkeypatch.setattr(dedup, "normalize_rows", boom)
    monkeypatch.setattr(dedup, "topk_normalized", boom)
    rows, ids, off = fake(32, 64, dtype=torch.float16), fake(32, dtype=torch.int32), fake(4, dtype=torch.int32)
    # self_join
    with pytest.raises(TypeError):
        dedup.self_join(np.zeros((32, 64), dtype=np.float16), ids, off, 20)
    with pytest.raises(RuntimeError, match=r"HIP device only \(no CPU path\)"):
        dedup.self_join(torch.zeros(32, 64, dtype=torch.float16), ids, off, 20)
    for bad, what in ((fake(32, 64), "contiguous fp16"), (fake(32, 96, dtype=torch.float16), "multiple of 64"),
                      (fake(32, dtype=torch.float16), r"\[rows, dim\]"), (fake(0, 64, dtype=torch.float16), "empty"),
                      (fake(24, 64, dtype=torch.float16), "multiple of 16")):
        with pytest.raises(ValueError, match=what):
            dedup.self_join(bad, ids, off, 20)
    for bad in (0, -3, 2.0, True, None):
        with pytest.raises(ValueError, match="n = "):
            dedup.self_join(rows, ids, off, bad)
    for bad in (fake(32, dtype=torch.int64), fake(16, dtype=torch.int32), fake(32, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="ids must be int32"):
            dedup.self_join(rows, bad, off, 20)
    with pytest.raises(RuntimeError, match="HIP device only"):
        dedup.self_join(rows, torch.zeros(32, dtype=torch.int32), off, 20)
    with pytest.raises(TypeError):
        dedup.self_join(rows, [0] * 32, off, 20)
    for bad in (fake(4, dtype=torch.int64), fake(1, dtype=torch.int32), fake(2, 2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="offsets must be int32"):
            dedup.self_join(rows, ids, bad, 20)
    with pytest.raises(TypeError):
        dedup.self_join(rows, ids, [0, 16, 32], 20)
    with pytest.raises(TypeError, match="priority"):
        dedup.self_join(rows, ids, off, 20, priority=[0.0] * 20)
    with pytest.raises(RuntimeError, match="HIP device only"):
        dedup.self_join(rows, ids, off, 20, priority=torch.zeros(20))
    for bad in (fake(20, dtype=torch.float16), fake(19), fake(20, 1)):
        with pytest.raises(ValueError, match=r"priority must be float32 \[20\]"):
            dedup.self_join(rows, ids, off, 20, priority=bad)
    # semdedup
    x = fake(20, 64)
    ix = IVFFlatIndex.__new__(IVFFlatIndex)
    ix._k, ix._d, ix._added = 3, 64, False
    for kw in ({}, {"threshold": 0.9, "eps": 0.1}):
        with pytest.raises(ValueError, match="exactly one of threshold and eps"):
            dedup.semdedup(x, n_lists=3, **kw)
    for kw in ({"threshold": "0.9"}, {"eps": True}):
        with pytest.raises(TypeError, match="a number"):
            dedup.semdedup(x, n_lists=3, **kw)
    assert dedup._threshold(None, 0.25) == 0.75 and dedup._threshold(0.5, None) == 0.5
    with pytest.raises(ValueError, match="priority = 'centre'"):
        dedup.semdedup(x, n_lists=3, eps=0.1, priority="centre")
    for kw in ({}, {"index": ix, "n_lists": 3}):
        with pytest.raises(ValueError, match="exactly one of index"):
            dedup.semdedup(x, eps=0.1, **kw)
    i8 = IVFInt8Index.__new__(IVFInt8Index)
    with pytest.raises(TypeError, match="IVFFlatIndex.*int8"):
        dedup.semdedup(x, index=i8, eps=0.1)
    with pytest.raises(TypeError, match="IVFFlatIndex.*int8"):
        i8.self_join()
    with pytest.raises(TypeError, match="must be an IVFFlatIndex"):
        dedup.semdedup(x, index=object(), eps=0.1)
    with pytest.raises(TypeError):
        dedup.semdedup(np.zeros((20, 64)), index=ix, eps=0.1)
    with pytest.raises(RuntimeError, match="HIP device only"):
        dedup.semdedup(torch.zeros(20, 64), index=ix, eps=0.1)
    with pytest.raises(ValueError, match="multiple of 64"):
        dedup.semdedup(fake(20, 96), index=ix, eps=0.1)
    with pytest.raises(TypeError, match="priority"):
        dedup.semdedup(x, index=ix, eps=0.1, priority=[0.0] * 20)
    with pytest.raises(ValueError, match=r"priority must be float32 \[20\]"):
        dedup.semdedup(x, index=ix, eps=0.1, priority=fake(21))
    with pytest.raises(RuntimeError, match="before add"):
        dedup.semdedup(x, index=ix, eps=0.1)
    with pytest.raises(RuntimeError, match="before add"):
        ix.self_join(n=20)
    ix._added = True
    with pytest.raises(ValueError, match="dim 128"):
        dedup.semdedup(fake(20, 128), index=ix, eps=0.1)
    ix._rows, ix._ids, ix._offsets = rows, ids, off
    with pytest.raises(ValueError, match="give n"):
        ix.self_join()
    with pytest.raises(ValueError, match=r"priority must be float32 \[20\]"):
        ix.self_join(priority=fake(19), n=20)
    assert index.LIST_ALIGN == R.ALIGN
    # keep_at re-thresholds the stored scores, strictly
    res = dedup.DedupResult(None, torch.tensor([-np.inf, 0.5, 0.9, 0.95]), None, None)
    assert res.keep_at(0.9).tolist() == [True, True, True, False] and res.keep_at(0.4).tolist() == [True, False, False, False]


def test_c_abi_sizing(lib):
    ws = lib.smi_ivf_dedup_workspace_bytes
    # padded list sizes [K] | their prefix sum [K + 1] | unit offsets [K + 1] | cursor [K] | priorities fp32 [slots]
    assert ws(160, 100, 7, 64) == 2 * 32 + 2 * 32 + 640 and ws(16, 1, 1, 1024) == 4 * 16 + 64
    assert ws(160, 100, 7, 64) % 16 == 0
    for bad in ((0, 100, 7, 64), (160, 0, 7, 64), (160, 100, 0, 64), (160, 100, 7, 96), (160, 100, 7, 0), (150, 100, 7, 64),
                (1 << 31, 100, 7, 64), (160, 1 << 31, 7, 64), (160, 100, 1 << 31, 64), (-16, 100, 7, 64)):
        assert ws(*bad) == 0, bad


def test_c_abi_refusals_without_a_device(lib):
    cases = D.refusal_cases(lib)
    assert all(rc != 0 for rc in cases.values()), {k: v for k, v in cases.items() if v == 0}
    p, big = 0x1000, 1 << 40
    f = lib.smi_ivf_dedup
    assert f(p, p, p, 7, 160, 96, p, 100, p, p, p, big, None) == -2 and b"multiple of 64" in lib.smi_last_error()
    assert f(p, p, p, 7, 150, 64, p, 100, p, p, p, big, None) == -1 and b"multiple of 16" in lib.smi_last_error()
    assert f(p, p, p, 7, 160, 64, p, 100, p, p, p, 16, None) == -1
    assert b"smi_ivf_dedup_workspace_bytes" in lib.smi_last_error()
    assert f(p, p, p, 7, 1 << 31, 64, p, 100, p, p, p, big, None) == -2 and b"int32" in lib.smi_last_error()
