"""CPU: the paged top-k -- the numpy restatement against a plain double loop, the paging identity on scores
with heavy ties, the page sizes, exhausted rows and ceilings that are no candidate; every refusal of the Python layer
(sonar_amd/xsim.py, clustering.py, index.py) and of the four new C-ABI entries.  Nothing here needs a device."""
import re

import numpy as np
import pytest
import torch

from tests import topk_wide_ref as W


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def _tied_scores(rng, m: int, levels: int):
    """m candidates with integer scores from `levels` values and ids that are neither sorted nor dense."""
    return rng.integers(0, levels, m).astype(np.float64), rng.permutation(3 * m)[:m].astype(np.int64)


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("m,levels", [(0, 1), (1, 1), (5, 2), (23, 3), (40, 1)])
def test_restated_page_equals_a_plain_double_loop(m, levels):
    rng = np.random.default_rng(100 * m + levels)
    s, i = _tied_scores(rng, m, levels)
    ceilings = [None, (1.0, 7), (0.5, 0), (0.0, -1), (-1.0, 0), (float(levels), 0)]
    ceilings += [(s[j], i[j]) for j in range(min(m, 4))]
    for k in (1, 3, 16):
        for c in ceilings:
            a, b = W.page(s, i, k, c), W.page_loop(s, i, k, c)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (k, c)


def test_page_sizes():
    assert W.page_sizes(1) == [1] and W.page_sizes(16) == [16] and W.page_sizes(17) == [16, 1]
    assert W.page_sizes(40) == [16, 16, 8] and W.page_sizes(64) == [16] * 4
    for k in range(1, 65):
        p = W.page_sizes(k)
        assert sum(p) == k and len(p) == -(-k // 16) and all(v == 16 for v in p[:-1]) and p[-1] == (k % 16 or 16)
    from sonar_amd import xsim

    assert xsim.PAGE == W.PAGE and xsim.WIDE_MAX == W.WIDE_MAX
    assert all(xsim.page_sizes(k) == W.page_sizes(k) for k in range(1, 65))


@pytest.mark.parametrize("levels", [1, 2, 5])
def test_paging_identity_on_heavy_ties(levels):
    """The pages concatenated are the first k of the full sort, k = 1 .. 64.  levels = 1: every candidate ties, and the id
    half of the ceiling decides whole pages."""
    rng = np.random.default_rng(levels)
    for m in (70, 100):
        s, i = _tied_scores(rng, m, levels)
        full = W.full_sort(s, i, 64)
        if levels == 1:
            assert np.array_equal(full[1], np.sort(i)[:64])
        for k in range(1, 65):
            ws, wi = W.wide(s, i, k)
            assert np.array_equal(ws, full[0][:k]) and np.array_equal(wi, full[1][:k]), k


def test_an_exhausted_row_stays_exhausted_and_fill_follows_the_candidates():
    rng = np.random.default_rng(9)
    s, i = _tied_scores(rng, 20, 3)
    ws, wi = W.wide(s, i, 64)
    assert (wi[:20] >= 0).all() and (wi[20:] == -1).all() and np.isneginf(ws[20:]).all()
    assert sorted(wi[:20].tolist()) == sorted(i.tolist())
    # the page after a page that ended in fill, and the one after that
    ps, pi = W.page(s, i, 16, (ws[31], wi[31]))
    assert (pi == -1).all() and np.isneginf(ps).all()
    ps, pi = W.page(s, i, 16, (ps[-1], pi[-1]))
    assert (pi == -1).all()
    # a page that ends exactly at the last candidate is not yet exhausted: the next one is all fill
    s16, i16 = s[:16], i[:16]
    p1 = W.page(s16, i16, 16)
    assert (p1[1] >= 0).all()
    p2 = W.page(s16, i16, 16, (p1[0][-1], p1[1][-1]))
    assert (p2[1] == -1).all()


def test_a_ceiling_that_is_no_candidate():
    s = np.array([3.0, 1.0, 0.0, 1.0, 0.0, 2.0])
    i = np.array([10, 11, 12, 13, 14, 15])
    assert W.page(s, i, 16, (0.5, 0))[1][:3].tolist() == [12, 14, -1]          # between two integer scores
    assert W.page(s, i, 16, (1.0, 0))[1][:5].tolist() == [11, 13, 12, 14, -1]  # a score that exists, an id in front of all
    assert W.page(s, i, 16, (1.0, 12))[1][:4].tolist() == [13, 12, 14, -1]     # ... between the two that tie
    assert W.page(s, i, 16, (1.0, 99))[1][:3].tolist() == [12, 14, -1]         # ... behind both
    assert W.page(s, i, 16, (9.0, 0))[1][:6].tolist() == [10, 15, 11, 13, 12, 14]
    assert W.page(s, i, 16, (-1.0, 0))[1][0] == -1
    assert W.page(s, i, 16, (float("inf"), 5))[1][0] == 10 and W.page(s, i, 16, (float("-inf"), 5))[1][0] == -1


def test_matrix_forms_agree_with_the_row_forms():
    rng = np.random.default_rng(4)
    s = rng.integers(-2, 3, (7, 50)).astype(np.float64)
    for k in (5, 16, 17, 40, 64):
        fs, fi = W.first_k(s, k, offset=1000)
        ceil, got_s, got_i = None, [], []
        for kp in W.page_sizes(k):
            ps, pi = W.brute_force(s, kp, 1000, ceil)
            got_s.append(ps), got_i.append(pi)
            ceil = (ps[:, -1], pi[:, -1])
        assert np.array_equal(np.concatenate(got_s, 1), fs) and np.array_equal(np.concatenate(got_i, 1), fi)
    # the index: every list probed is brute force; one ceiling per query over all its lists
    labels = rng.integers(0, 6, 50)
    probes = np.tile(np.arange(6), (7, 1))
    for k in (16, 33):
        a, b = W.search_wide(s, labels, 6, probes, k), W.first_k(s, k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    vis = rng.random(50) < 0.5
    a = W.search_wide(s, labels, 6, probes, 20, visible=vis)
    b = W.first_k(np.where(vis, s, -np.inf), 20)
    keep = np.isfinite(b[0])
    assert np.array_equal(a[1][keep], b[1][keep]) and (a[1][~keep] == -1).all()
    none = W.search(s, labels, 6, np.full((7, 3), -1), 16)
    assert (none[1] == -1).all()


# ------------------------------------------------------------------------------------------------------- refusals
class FakeDevice(torch.Tensor):
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta").as_subclass(FakeDevice)


def boom(*a, **k):
    raise AssertionError("reached the device")


BAD_COUNTS = (0, 65, True, 4.0)


def test_python_refusals_of_the_brute_force_calls(monkeypatch):
    from sonar_amd import clustering, xsim
    from sonar_amd.clustering import SphericalKMeans

    monkeypatch.setattr(xsim._lib, "load", boom)
    monkeypatch.setattr(xsim, "normalize_rows", boom)
    xn, yn = fake(256, 64, dtype=torch.float16), fake(512, 64, dtype=torch.float16)
    for bad in BAD_COUNTS:
        with pytest.raises(ValueError, match=r"k = .*\[1, 64\]"):
            xsim.topk_wide_normalized(xn, 100, yn, 300, bad)
        with pytest.raises(ValueError, match=r"k = .*\[1, 64\]"):
            xsim.topk_wide(fake(100, 64), fake(300, 64), bad)
        with pytest.raises(ValueError, match=r"k = .*\[1, 64\]"):
            SphericalKMeans(3).predict_wide(fake(5, 64), bad)
    for bad in (0, 17, 65, True, 4.0):
        with pytest.raises(ValueError, match=r"k = .*\[1, 16\]"):
            xsim.topk_page_normalized(xn, 100, yn, 300, bad)
    with pytest.raises(RuntimeError, match="before fit"):
        SphericalKMeans(3).predict_wide(fake(5, 64), 64)
    # `predict` keeps its check
    with pytest.raises(ValueError, match=r"\[1, 8\]"):
        SphericalKMeans(3).predict(fake(5, 64), 9)
    # below: type, shape, dtype, device
    ok_s, ok_i = fake(100), fake(100, dtype=torch.int32)
    for bad in ((ok_s,), ok_s, (ok_s, [0] * 100), "x"):
        with pytest.raises(TypeError, match="below"):
            xsim.topk_page_normalized(xn, 100, yn, 300, 16, below=bad)
    for bad, what in (((fake(99), ok_i), r"scores must be fp32 \[100\]"), ((fake(100, 1), ok_i), "scores must be fp32"),
                      ((fake(100, dtype=torch.float16), ok_i), "scores must be fp32"),
                      ((ok_s, fake(100, dtype=torch.int64)), "ids must be int32"),
                      ((ok_s, fake(101, dtype=torch.int32)), r"ids must be int32 \[100\]")):
        with pytest.raises(ValueError, match=what):
            xsim.topk_page_normalized(xn, 100, yn, 300, 16, below=bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        xsim.topk_page_normalized(xn, 100, yn, 300, 16, below=(torch.zeros(100), ok_i))
    with pytest.raises(RuntimeError, match="HIP device"):
        xsim.topk_page_normalized(xn, 100, yn, 300, 16, below=(ok_s, torch.zeros(100, dtype=torch.int32)))
    assert clustering.SphericalKMeans.predict_wide.__doc__


def test_python_refusals_of_the_index_calls(monkeypatch):
    from sonar_amd import index
    from sonar_amd.index import IVFFlatIndex, IVFInt8Index

    monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=torch.float16))
    ix = IVFFlatIndex(fake(3, 64))
    monkeypatch.setattr(index, "topk_normalized", boom)
    monkeypatch.setattr(index, "topk_wide_normalized", boom)
    monkeypatch.setattr(index._lib, "load", boom)
    q = fake(5, 64)
    with pytest.raises(RuntimeError, match="before add"):
        ix.search_wide(q)
    with pytest.raises(RuntimeError, match="before add"):
        ix.search_page(q)
    ix._added = True
    ix._ids = fake(48, dtype=torch.int32)
    for bad in BAD_COUNTS:
        with pytest.raises(ValueError, match=r"k = .*\[1, 64\]"):
            ix.search_wide(q, k=bad)
        with pytest.raises(ValueError, match=r"nprobe = .*\[1, 64\]"):
            ix.search_wide(q, nprobe=bad)
        with pytest.raises(ValueError, match=r"nprobe = .*\[1, 64\]"):
            ix.search_page(q, nprobe=bad)
        with pytest.raises(ValueError, match=r"nprobe = .*\[1, 64\]"):
            ix.probe_wide(q, bad)
        with pytest.raises(ValueError, match=r"nprobe = .*\[1, 64\]"):
            IVFInt8Index(fake(3, 64)).probe_wide(q, bad)
    for bad in (0, 17, True, 4.0):
        with pytest.raises(ValueError, match=r"k = .*\[1, 16\]"):
            ix.search_page(q, k=bad)
    # probe's rule where nprobe exceeds the lists
    with pytest.raises(ValueError, match="exceeds the 3 lists"):
        ix.probe_wide(q, 4)
    with pytest.raises(ValueError, match="exceeds the 3 lists"):
        ix.search_wide(q, nprobe=9)
    with pytest.raises(ValueError, match="exceeds the 3 lists"):
        ix.search_page(q, nprobe=4)
    # the old entries keep theirs
    with pytest.raises(ValueError, match=r"nprobe = .*\[1, 8\]"):
        ix.probe(q, 9)
    with pytest.raises(ValueError, match=r"k = .*\[1, 8\]"):
        ix.search(q, k=9)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ix.search_wide(torch.zeros(5, 64), nprobe=2)
    with pytest.raises(ValueError, match="dim 128"):
        ix.search_wide(fake(5, 128), nprobe=2)
    for bad in (fake(5, 2, dtype=torch.int64), fake(4, 2, dtype=torch.int32), fake(5, 65, dtype=torch.int32),
                fake(5, 0, dtype=torch.int32)):
        with pytest.raises(ValueError, match="probes"):
            ix.search_wide(q, probes=bad)
    with pytest.raises(TypeError, match="RowFilter"):
        ix.search_wide(q, nprobe=2, rows=fake(48, dtype=torch.int32))
    with pytest.raises(TypeError):
        ix.search_wide(q, nprobe=2, query_keys=fake(5, dtype=torch.int32))  # the key predicate is out of scope
    ok_s, ok_i = fake(5), fake(5, dtype=torch.int32)
    for bad, exc in (((fake(4), ok_i), ValueError), ((ok_s, fake(5, dtype=torch.int64)), ValueError), ((ok_s,), TypeError),
                     ((torch.zeros(5), ok_i), RuntimeError)):
        with pytest.raises(exc, match="below"):
            ix.search_page(q, nprobe=2, below=bad)
    # the list function
    qn, rows, ids, off = fake(256, 64, dtype=torch.float16), fake(48, 64, dtype=torch.float16), fake(48, dtype=torch.int32), \
        fake(4, dtype=torch.int32)
    probes = fake(5, 9, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"k = .*\[1, 16\]"):
        index.search_lists_page(qn, probes, rows, ids, off, 17)
    with pytest.raises(ValueError, match="probes"):
        index.search_lists_page(qn, fake(5, 65, dtype=torch.int32), rows, ids, off, 16)
    with pytest.raises(ValueError, match="dim"):
        index.search_lists_page(qn, probes, fake(48, 128, dtype=torch.float16), ids, off, 16)
    with pytest.raises(ValueError, match="below"):
        index.search_lists_page(qn, probes, rows, ids, off, 16, below=(fake(6), fake(6, dtype=torch.int32)))
    # search_lists keeps its probe limit
    with pytest.raises(ValueError, match=r"1\.\.8"):
        index.search_lists(qn, probes, rows, ids, off, 8)


def test_pretransform_forwards_search_wide():
    from sonar_amd.index import PreTransformIndex

    assert callable(PreTransformIndex.search_wide) and callable(PreTransformIndex.probe_wide)


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_new_symbols_are_declared_bound_and_exported(lib):
    import os
    import subprocess

    from sonar_amd import _lib

    names = {"smi_xsim_topk_page_ws_bytes", "smi_xsim_topk_page", "smi_ivf_search_page_ws_bytes",
             "smi_ivf_search_page"}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "sonar_mi355.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(smi_[a-z0-9_]+)\s*\(", header))
    assert names <= set(_lib.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert names <= set(re.findall(r"\bT (smi_[a-z0-9_]+)", out))


def test_c_abi_sizing_and_refusals_of_the_brute_force_page(lib):
    pw, P = lib.smi_xsim_topk_page_ws_bytes, lib.smi_xsim_topk_page
    # lists of 16 whatever k, one chunk per 256 rows of y up to 8 | both tile-major copies | one 64-bit key per padded x row
    want = 2 * 4 * 8 * 1024 * 16 + (1024 + 100096) * 1024 * 2 + 1024 * 8
    assert pw(1000, 100000, 16, 1024) == want and pw(1000, 100000, 1, 1024) == want
    assert pw(1, 1, 16, 64) == 2 * 4 * 1 * 256 * 16 + 2 * 256 * 64 * 2 + 256 * 8
    for bad in ((0, 5, 1, 64), (5, 0, 1, 64), (5, 5, 0, 64), (5, 5, 17, 64), (5, 5, 16, 96), (5, 5, 16, 0), (1 << 31, 5, 1, 64),
                (5, 1 << 31, 1, 64)):
        assert pw(*bad) == 0, bad
    # the old sizing call keeps its limit
    assert lib.smi_xsim_workspace_bytes(5, 5, 9, 64) == 0 and lib.smi_xsim_workspace_bytes(5, 5, 8, 64) > 0
    p, big = 0x1000, 1 << 40  # never dereferenced: every call below is refused on its arguments
    cases = {
        "k 0": P(p, 100, p, 300, 64, 0, 0, p, p, p, p, p, big, None),
        "k 17": P(p, 100, p, 300, 64, 17, 0, p, p, p, p, p, big, None),
        "d": P(p, 100, p, 300, 96, 16, 0, p, p, p, p, p, big, None),
        "nx": P(p, 0, p, 300, 64, 16, 0, p, p, p, p, p, big, None),
        "ny": P(p, 100, p, 0, 64, 16, 0, p, p, p, p, p, big, None),
        "big nx": P(p, 1 << 31, p, 300, 64, 16, 0, p, p, p, p, p, big, None),
        "null x": P(None, 100, p, 300, 64, 16, 0, p, p, p, p, p, big, None),
        "null y": P(p, 100, None, 300, 64, 16, 0, p, p, p, p, p, big, None),
        "null idx": P(p, 100, p, 300, 64, 16, 0, p, p, None, p, p, big, None),
        "null score": P(p, 100, p, 300, 64, 16, 0, p, p, p, None, p, big, None),
        "ceil score alone": P(p, 100, p, 300, 64, 16, 0, p, None, p, p, p, big, None),
        "ceil idx alone": P(p, 100, p, 300, 64, 16, 0, None, p, p, p, p, big, None),
        "null ws": P(p, 100, p, 300, 64, 16, 0, p, p, p, p, None, big, None),
        "short ws": P(p, 100, p, 300, 64, 16, 0, p, p, p, p, p, pw(100, 300, 16, 64) - 1, None),
        "misaligned ws": P(p, 100, p, 300, 64, 16, 0, p, p, p, p, p + 8, big, None),
    }
    assert all(rc != 0 for rc in cases.values()), {k: v for k, v in cases.items() if v == 0}
    assert P(p, 100, p, 300, 64, 17, 0, None, None, p, p, p, big, None) == -2 and b"k=17 outside [1,16]" in lib.smi_last_error()
    assert P(p, 100, p, 300, 64, 16, 0, None, None, p, p, p, 16, None) == -1
    assert b"smi_xsim_topk_page_ws_bytes" in lib.smi_last_error()
    # every check passed: only the device is missing (null ceilings are no refusal)
    if not torch.cuda.is_available():
        assert P(p, 100, p, 300, 64, 16, 0, None, None, p, p, p, big, None) == -3
        assert P(p, 100, p, 300, 64, 16, 0, p, p, p, p, p, pw(100, 300, 16, 64), None) == -3
    # the old entry keeps its refusal
    assert lib.smi_xsim_topk(p, 100, p, 300, 64, 9, 0, p, p, p, big, None) == -2 and b"outside [1,8]" in lib.smi_last_error()
    assert lib.smi_xsim_merge_topk(p, p, 4, 100, 9, p, p, None) == -2


def test_c_abi_sizing_and_refusals_of_the_index_page(lib):
    import ctypes as C

    sw, sp = lib.smi_ivf_search_workspace_bytes, lib.smi_ivf_search_page_ws_bytes

    def S(*a):
        """The cases below give the ceilings in front of the outputs; the entry takes them behind its twin's arguments."""
        cs, ci = (None if v is None else C.cast(v, t) for v, t in ((a[10], C.POINTER(C.c_float)), (a[11], C.POINTER(C.c_int32))))
        return lib.smi_ivf_search_page(*a[:10], *a[12:], cs, ci)

    # the search's layout and one 64-bit ceiling key per query
    assert sp(100, 7, 4, 5, 64) == sw(100, 7, 4, 5, 64) + 800
    assert sp(100, 7, 64, 16, 64) == 2 * 32 + 2 * 32 + 100 * 64 * 4 + 2 * 100 * 64 * 16 * 4 + 800
    for bad in ((0, 7, 4, 5, 64), (100, 0, 4, 5, 64), (100, 7, 0, 5, 64), (100, 7, 65, 5, 64), (100, 7, 4, 0, 64),
                (100, 7, 4, 17, 64), (100, 7, 4, 5, 96), (1 << 31, 7, 1, 1, 64), (100, 1 << 31, 1, 1, 64),
                (1 << 26, 7, 64, 1, 64)):
        assert sp(*bad) == 0, bad
    assert sw(100, 7, 9, 5, 64) == 0 and sw(100, 7, 4, 9, 64) == 0  # the old sizing call keeps its limits
    p, big = 0x1000, 1 << 40
    cases = {
        "d": S(p, 100, 96, p, 4, p, p, p, 7, 5, p, p, p, p, p, big, None),
        "K": S(p, 100, 64, p, 4, p, p, p, 0, 5, p, p, p, p, p, big, None),
        "nq": S(p, 0, 64, p, 4, p, p, p, 7, 5, p, p, p, p, p, big, None),
        "big pairs": S(p, 1 << 26, 64, p, 64, p, p, p, 7, 5, p, p, p, p, p, big, None),
        "k 0": S(p, 100, 64, p, 4, p, p, p, 7, 0, p, p, p, p, p, big, None),
        "k 17": S(p, 100, 64, p, 4, p, p, p, 7, 17, p, p, p, p, p, big, None),
        "nprobe 0": S(p, 100, 64, p, 0, p, p, p, 7, 5, p, p, p, p, p, big, None),
        "nprobe 65": S(p, 100, 64, p, 65, p, p, p, 7, 5, p, p, p, p, p, big, None),
        "null q": S(None, 100, 64, p, 4, p, p, p, 7, 5, p, p, p, p, p, big, None),
        "null probes": S(p, 100, 64, None, 4, p, p, p, 7, 5, p, p, p, p, p, big, None),
        "null rows": S(p, 100, 64, p, 4, None, p, p, 7, 5, p, p, p, p, p, big, None),
        "null ids": S(p, 100, 64, p, 4, p, None, p, 7, 5, p, p, p, p, p, big, None),
        "null offsets": S(p, 100, 64, p, 4, p, p, None, 7, 5, p, p, p, p, p, big, None),
        "ceil score alone": S(p, 100, 64, p, 4, p, p, p, 7, 5, p, None, p, p, p, big, None),
        "ceil idx alone": S(p, 100, 64, p, 4, p, p, p, 7, 5, None, p, p, p, p, big, None),
        "null idx": S(p, 100, 64, p, 4, p, p, p, 7, 5, p, p, None, p, p, big, None),
        "null score": S(p, 100, 64, p, 4, p, p, p, 7, 5, p, p, p, None, p, big, None),
        "null ws": S(p, 100, 64, p, 4, p, p, p, 7, 5, p, p, p, p, None, big, None),
        "short ws": S(p, 100, 64, p, 4, p, p, p, 7, 5, p, p, p, p, p, sp(100, 7, 4, 5, 64) - 1, None),
        "misaligned ws": S(p, 100, 64, p, 4, p, p, p, 7, 5, p, p, p, p, p + 4, big, None),
    }
    assert all(rc != 0 for rc in cases.values()), {k: v for k, v in cases.items() if v == 0}
    assert S(p, 100, 64, p, 65, p, p, p, 7, 5, None, None, p, p, p, big, None) == -1 and b"nprobe=65" in lib.smi_last_error()
    assert S(p, 100, 64, p, 4, p, p, p, 7, 17, None, None, p, p, p, big, None) == -1 and b"k=17" in lib.smi_last_error()
    assert S(p, 100, 64, p, 4, p, p, p, 7, 5, None, None, p, p, p, 16, None) == -1
    assert b"smi_ivf_search_page_ws_bytes" in lib.smi_last_error()
    if not torch.cuda.is_available():
        assert S(p, 100, 64, p, 64, p, p, p, 7, 16, None, None, p, p, p, big, None) == -3
        assert S(p, 100, 64, p, 9, p, p, p, 7, 16, p, p, p, p, p, sp(100, 7, 9, 16, 64), None) == -3
    # a sizing call leaves the last error as it was
    S(p, 100, 64, p, 65, p, p, p, 7, 5, None, None, p, p, p, big, None)
    before = lib.smi_last_error()
    assert sp(100, 7, 65, 5, 64) == 0 and lib.smi_last_error() == before
