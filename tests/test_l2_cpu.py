"""CPU: squared-Euclidean / inner-product search and Euclidean k-means -- the numpy restatement
(tests/l2_ref.py) against plain loops, `math.fsum` and exact rationals; the conditions on the data that tests/test_gpu_l2.py
relies on; every refusal of the Python layer (sonar_amd/xsim.py, clustering.py, index.py) and of the new C-ABI entries.
Nothing here needs a device."""
import math
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import kmeans_ref as KR
from tests import l2_ref as L


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


# ------------------------------------------------------------------------------------------------- the restatement
def test_restated_topk_equals_a_plain_double_loop():
    rng = np.random.default_rng(0)
    x, y = L.int_rows(rng, 7, 16), L.sparse_int_rows(rng, 12, 16)
    x[2] = 0                     # a zero row: scores -h_y
    y[3] = y[9] = y[5]           # equal rows tie
    x[4] = 0
    y[:, :] = np.where(np.arange(12)[:, None] == 7, 0, y)  # a zero y row: bias -0, score +0
    bias = -L.half_norms(y)
    for k in range(1, 9):
        a, b = L.topk(x, y, bias, k, 100), L.topk_loop(x, y, bias, k, 100)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]), k
    # a row where every candidate ties: ids ascending
    same = np.repeat(y[5:6], 12, axis=0)
    s, i = L.topk(x, same, -L.half_norms(same), 8)
    assert (i == np.arange(8)[None, :]).all() and (s == s[:, :1]).all()
    assert np.array_equal(L.topk_loop(x, same, -L.half_norms(same), 8)[1], i)
    # fewer rows than k: fill
    s, i = L.topk(x, y[:3], bias[:3], 5)
    assert np.isneginf(s[:, 3:]).all() and (i[:, 3:] == -1).all()
    d, i2, _ = L.topk_l2(x, y[:3], 5)
    assert np.isposinf(d[:, 3:]).all() and (d[:, :3] >= 0).all() and (np.diff(d[:, :3], axis=1) >= 0).all()
    # the distances ARE the squared distances on integer rows
    d, i, _ = L.topk_l2(x, y, 12)
    exact = ((x.astype(np.float64)[:, None, :] - y.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    assert np.array_equal(d.astype(np.float64), np.take_along_axis(exact, i, axis=1))
    assert not np.signbit(L.scores(x, y, bias)[:, 7]).any()  # a zero score is +0


@pytest.mark.parametrize("d", [8, 64, 192, 520, 1024])
def test_half_norms_against_fsum(d):
    rng = np.random.default_rng(d)
    x = (rng.standard_normal((9, d)) * rng.uniform(0.01, 100.0, (9, 1))).astype(np.float16)
    h = L.half_norms(x)
    for r in range(len(x)):
        exact = 0.5 * math.fsum(float(v) * float(v) for v in x[r])
        assert h[r] == np.float32(exact) or abs(float(h[r]) - exact) <= 2.0 ** -23 * exact
    # the float64 sum itself, in the restated order, is within 2^-50 relative of fsum: read it back through a second route
    sq = x.astype(np.float64) ** 2
    p = np.zeros((len(x), 64))
    for c in range(d // 8):
        for e in range(8):
            p[:, c % 64] += sq[:, c * 8 + e]
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lane ^ off]
    for r in range(len(x)):
        exact = math.fsum(float(v) * float(v) for v in x[r])
        assert abs(p[r, 0] - exact) <= 2.0 ** -50 * exact
    assert np.array_equal((0.5 * p[:, 0]).astype(np.float32), h)  # the loop form IS the restatement
    ints = L.int_rows(rng, 9, d)
    assert np.array_equal(L.half_norms(ints).astype(np.float64), 0.5 * (ints.astype(np.float64) ** 2).sum(axis=1))
    rows16, hp = L.prepare(ints.astype(np.float32))
    assert rows16.shape == (256, d) and (rows16[9:] == 0).all() and (hp[9:] == 0).all() and np.array_equal(rows16[:9], ints)


def test_finalize_against_exact_rationals():
    rng = np.random.default_rng(1)
    k, d = 9, 16
    counts = np.array([1, 2, 3, 7, 0, 1000, 12345, 5, 64], dtype=np.int32)  # counts that are no powers of two, and an empty one
    sums = rng.integers(-2 ** 40, 2 ** 40, (k, d)).astype(np.int64)
    sums[3, :4] = [2 ** 62 + 12345, -(2 ** 60) - 7, 1, -1]  # above 2^53: int64 -> float64 rounds
    prev32 = rng.standard_normal((k, d)).astype(np.float32)
    prev16 = rng.standard_normal((256, d)).astype(np.float16)
    prev_h = rng.random(256).astype(np.float32)
    c32, c16, h, empty = L.finalize(sums, counts, prev32, prev16, prev_h)
    assert empty == 1
    for c in range(k):
        if counts[c] == 0:
            assert np.array_equal(c32[c], prev32[c]) and np.array_equal(c16[c], prev16[c]) and h[c] == prev_h[c]
            continue
        for j in range(d):
            q = Fraction(float(int(sums[c, j]))) / (1 << 24) / int(counts[c])  # fl64(sum) is the only rounding so far
            q64 = q.numerator / q.denominator                                  # int / int: correctly rounded to float64
            assert c32[c, j] == np.float32(q64), (c, j)
        with np.errstate(over="ignore"):
            assert np.array_equal(c16[c], c32[c].astype(np.float16))
    assert np.array_equal(h[counts > 0], L.half_norms(c16)[counts > 0])
    # where the mean is representable the centroid is the mean
    x = L.int_rows(rng, 64, 16)
    s, n = KR.update(x, np.zeros(64, dtype=np.int32), 1)
    c32, _, _, _ = L.finalize(s, n, np.zeros((1, 16), np.float32), np.zeros((256, 16), np.float16), np.zeros(256, np.float32))
    assert np.array_equal(c32[0].astype(np.float64), x.astype(np.float64).mean(axis=0))


def test_objective_sum_is_a_float64_sum():
    rng = np.random.default_rng(2)
    for n in (1, 255, 1000, 3000):
        s = (rng.standard_normal(n) * 100).astype(np.float32)
        exact = math.fsum(float(v) for v in s)
        assert abs(L.objective_sum(s) - exact) <= n * 2.0 ** -53 * float(np.abs(s).sum())
    ints = rng.integers(-1000, 1000, 3000).astype(np.float32)
    assert L.objective_sum(ints) == float(ints.astype(np.float64).sum())


# ------------------------------------------------------------------------------ what the GPU tests rely on
@pytest.mark.parametrize("nx,ny,d", L.EXACT_SHAPES)
def test_conditions_on_the_exact_data(nx, ny, d):
    """The data of tests/test_gpu_l2.py (same seeds).  The L2 top-1 differs from the inner-product and from the cosine top-1
    in at least half of the rows (a kernel that forgot the bias, or normalised, fails on most rows); in at least 0.05 of the
    rows two adjacent positions of the 8 best tie, so the tie-break decides; every score and half norm is exact in fp32."""
    rng = np.random.default_rng(nx * 7 + ny + d)
    x, y = L.int_rows(rng, nx, d), L.sparse_int_rows(rng, ny, d)
    not_ip, not_cos, tied_rows, per_k, exact = L.data_conditions(x, y)
    print(f"{nx} x {ny} x {d}: L2 top-1 != IP top-1 in {not_ip:.2f}, != cosine top-1 in {not_cos:.2f} of the rows; "
          f"adjacent tie among the 8 best in {tied_rows:.2f}; per position {[round(p, 3) for p in per_k]}")
    assert not_ip >= 0.5 and not_cos >= 0.5
    assert tied_rows >= 0.05
    assert exact


def test_the_planted_gap_is_above_twice_the_bound():
    x, y, truth = L.planted()
    gap, bound = L.planted_gap(x, y, truth)
    print(f"planted: smallest gap {gap:.2e}, largest bound {bound:.2e}")
    assert gap > 2 * bound
    assert truth.shape == (75, 4) and len(y) == 300


def test_two_clusters_on_one_ray():
    """Rows at distances 1 and 3 along one direction: Euclidean k-means separates them, the spherical fit cannot (both
    clusters have the same direction) -- asserted on the restatements."""
    x, truth, init = L.ray_clusters()
    rounds = L.fit(x, init, 3)
    assert np.array_equal(rounds[-1]["labels"], truth)
    sph = KR.fit(x, init, 3)
    assert (sph[-1]["labels"] == truth).mean() < 0.9
    # inertia = sum of squared distances to the assigned centroid
    r = rounds[-1]
    diff = x.astype(np.float64) - r["c16"].astype(np.float64)[r["labels"]]
    inertia = L.inertia(L.half_norms(x), r["objective"], len(x))
    assert abs(inertia - (diff ** 2).sum()) <= 1e-3 * (diff ** 2).sum()


def test_kmeans_restatement_handles_empty_and_duplicate_centroids():
    rng = np.random.default_rng(4)
    x = L.int_rows(rng, 200, 16)
    init = np.concatenate([x[:3], x[:1]]).astype(np.float32)  # centroid 3 == centroid 0: ties go to the lower index
    rounds = L.fit(x, init, 2)
    assert (rounds[0]["labels"] != 3).all() and rounds[1]["empty"] == 1 and rounds[1]["counts"][3] == 0
    assert np.array_equal(rounds[1]["c32"][3], init[3]) and rounds[0]["moved"] == 200


# ------------------------------------------------------------------------------------------------------- refusals
class FakeDevice(torch.Tensor):
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta").as_subclass(FakeDevice)


def boom(*a, **k):
    raise AssertionError("reached the device")


def test_python_refusals_of_the_brute_force_calls(monkeypatch):
    from sonar_amd import xsim

    monkeypatch.setattr(xsim._lib, "load", boom)
    x16, y16 = fake(256, 64, dtype=torch.float16), fake(512, 64, dtype=torch.float16)
    bias, hx = fake(512), fake(256)
    for bad in (0, 9, True, 4.0):
        with pytest.raises(ValueError, match=r"k must be in \[1, 8\]"):
            xsim.topk_bias_prepared(x16, 100, y16, 300, bias, bad)
        with pytest.raises(ValueError, match=r"k must be in \[1, 8\]"):
            xsim.topk_l2_prepared(x16, 100, hx, y16, 300, bias, bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        xsim.prepare_rows(torch.zeros(4, 64))
    with pytest.raises(ValueError, match=r"\[rows, dim\]"):
        xsim.prepare_rows(fake(4))
    with pytest.raises(ValueError, match="empty"):
        xsim.prepare_rows(fake(0, 64))
    with pytest.raises(ValueError, match="multiple of 8"):
        xsim.prepare_rows(fake(4, 20))
    with pytest.raises(ValueError, match="nx = 0"):
        xsim.topk_bias_prepared(x16, 0, y16, 300, bias)
    with pytest.raises(ValueError, match="x16 must be the contiguous fp16"):
        xsim.topk_bias_prepared(x16, 300, y16, 300, bias)            # 300 rows pad to 512
    with pytest.raises(ValueError, match="y16 must be the contiguous fp16"):
        xsim.topk_bias_prepared(x16, 100, fake(512, 64), 300, bias)  # fp32
    with pytest.raises(TypeError, match="x16"):
        xsim.topk_bias_prepared(None, 100, y16, 300, bias)
    with pytest.raises(RuntimeError, match="HIP device"):
        xsim.topk_bias_prepared(torch.zeros(256, 64, dtype=torch.float16), 100, y16, 300, bias)
    with pytest.raises(ValueError, match="same dimension"):
        xsim.topk_bias_prepared(x16, 100, fake(512, 128, dtype=torch.float16), 300, bias)
    with pytest.raises(ValueError, match="multiple of 64"):
        xsim.topk_bias_prepared(fake(256, 96, dtype=torch.float16), 100, fake(512, 96, dtype=torch.float16), 300, bias)
    for bad, exc, what in ((fake(300), ValueError, r"bias must be contiguous fp32 \[512\]"),
                           (fake(512, dtype=torch.float16), ValueError, "bias must be contiguous fp32"),
                           (None, TypeError, "bias"), (torch.zeros(512), RuntimeError, "HIP device")):
        with pytest.raises(exc, match=what):
            xsim.topk_bias_prepared(x16, 100, y16, 300, bad)
    with pytest.raises(ValueError, match=r"x_half_norms must be contiguous fp32 \[256\]"):
        xsim.topk_l2_prepared(x16, 100, fake(100), y16, 300, bias)
    with pytest.raises(ValueError, match=r"y_half_norms must be contiguous fp32 \[512\]"):
        xsim.topk_l2_prepared(x16, 100, hx, y16, 300, fake(300))
    assert "never needed unit rows" in xsim.topk_ip.__doc__


def test_python_refusals_of_kmeans(monkeypatch):
    from sonar_amd import clustering
    from sonar_amd.clustering import KMeans

    monkeypatch.setattr(clustering._lib, "load", boom)
    monkeypatch.setattr(clustering, "prepare_rows", boom)
    for bad in (0, True, 2.0):
        with pytest.raises(ValueError, match="n_clusters"):
            KMeans(bad)
    with pytest.raises(ValueError, match="n_iter"):
        KMeans(3, n_iter=-1)
    km = KMeans(3)
    with pytest.raises(RuntimeError, match="HIP device"):
        km.fit(torch.zeros(10, 64))
    with pytest.raises(ValueError, match="multiple of 64"):
        km.fit(fake(10, 96))
    with pytest.raises(ValueError, match="exceeds the 2 rows"):
        km.fit(fake(2, 64))
    with pytest.raises(ValueError, match=r"init must be \[3, 64\]"):
        km.fit(fake(10, 64), init=fake(4, 64))
    for what in ("step", "predict", "centroids", "centroids_f16", "centroid_half_norms", "history"):
        with pytest.raises(RuntimeError, match="before fit"):
            (getattr(km, what)() if what == "step" else km.predict(fake(5, 64)) if what == "predict" else getattr(km, what))
    with pytest.raises(ValueError, match=r"\[1, 8\]"):
        km.predict(fake(5, 64), 9)
    with pytest.raises(TypeError, match="prepare_rows"):
        km.fit_normalized(fake(256, 64, dtype=torch.float16), 10)
    with pytest.raises(TypeError, match="as they are"):
        km.centroids_normalized
    with pytest.raises(TypeError, match="k <= 8"):
        km.predict_wide(fake(5, 64))
    x16 = fake(256, 64, dtype=torch.float16)
    with pytest.raises(ValueError, match="contiguous fp16"):
        km.fit_prepared(fake(256, 64), fake(256), 10)
    with pytest.raises(ValueError, match="does not match"):
        km.fit_prepared(x16, fake(256), 300)
    with pytest.raises(ValueError, match="half_norms"):
        km.fit_prepared(x16, fake(100), 10)


def test_python_refusals_of_the_index(monkeypatch):
    from sonar_amd import index
    from sonar_amd.clustering import KMeans, SphericalKMeans
    from sonar_amd.index import IVFFlatIndex, IVFFlatL2Index

    monkeypatch.setattr(index, "prepare_rows",
                        lambda t: (fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=torch.float16),
                                   fake((t.shape[0] + 255) // 256 * 256)))
    monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=torch.float16))
    ix = IVFFlatL2Index(fake(3, 64))
    monkeypatch.setattr(index, "topk_bias_prepared", boom)
    monkeypatch.setattr(index._lib, "load", boom)
    q = fake(5, 64)
    with pytest.raises(RuntimeError, match="before fit"):
        IVFFlatL2Index(KMeans(3))
    with pytest.raises(TypeError, match="Euclidean centroids"):
        IVFFlatL2Index(SphericalKMeans(3))
    with pytest.raises(RuntimeError, match="HIP device"):
        IVFFlatL2Index(torch.zeros(3, 64))
    for call in (lambda: ix.search(q), lambda: ix.state_dict(), lambda: ix.list_sizes, lambda: ix.row_filter(mask=fake(9, dtype=torch.bool))):
        with pytest.raises(RuntimeError, match="before add"):
            call()
    with pytest.raises(ValueError, match="dim 128"):
        ix.add(fake(10, 128))
    with pytest.raises(ValueError, match="labels"):
        ix.add(fake(10, 64), labels=fake(9, dtype=torch.int32))
    ix._added = True
    ix._ids = fake(48, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="already called"):
        ix.add(fake(10, 64))
    for bad in (0, 9, True, 4.0):
        with pytest.raises(ValueError, match=r"k = .*\[1, 8\]"):
            ix.search(q, k=bad)
        with pytest.raises(ValueError, match=r"nprobe = .*\[1, 8\]"):
            ix.search(q, nprobe=bad)
        with pytest.raises(ValueError, match=r"nprobe = .*\[1, 8\]"):
            ix.probe(q, bad)
    with pytest.raises(ValueError, match="exceeds the 3 lists"):
        ix.search(q, nprobe=4)
    with pytest.raises(ValueError, match="exceeds the 3 lists"):
        ix.probe(q, 4)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ix.search(torch.zeros(5, 64))
    with pytest.raises(ValueError, match="dim 128"):
        ix.search(fake(5, 128))
    for bad in (fake(5, 2, dtype=torch.int64), fake(4, 2, dtype=torch.int32), fake(5, 9, dtype=torch.int32)):
        with pytest.raises(ValueError, match="probes"):
            ix.search(q, probes=bad)
    with pytest.raises(TypeError, match="RowFilter"):
        ix.search(q, rows=fake(48, dtype=torch.int32))
    with pytest.raises(TypeError, match="query_keys"):
        ix.search(q, query_keys=fake(5, dtype=torch.int32))
    with pytest.raises(TypeError, match="refine"):
        ix.search(q, refine=fake(256, 64, dtype=torch.float16))
    for name in ("range_search", "search_wide", "self_join", "probe_wide"):
        with pytest.raises(TypeError, match="DESIGN.md 7"):
            getattr(ix, name)(q)
    with pytest.raises(TypeError, match="as they are"):
        ix.centroids_normalized
    # the states are kept apart, both ways
    l2_state = {"centroids": fake(3, 64, dtype=torch.float16), "offsets": fake(4, dtype=torch.int32), "sizes": fake(3, dtype=torch.int32),
                "rows": fake(48, 64, dtype=torch.float16), "bias": fake(48), "ids": fake(48, dtype=torch.int32)}
    with pytest.raises(ValueError, match="metric_l2"):
        IVFFlatL2Index.from_state_dict(l2_state)            # the marker is missing: a cosine index's state
    with pytest.raises(ValueError, match="state lacks"):
        IVFFlatL2Index.from_state_dict({k: v for k, v in l2_state.items() if k != "bias"})
    with pytest.raises(ValueError, match="IVFFlatL2Index"):
        IVFFlatIndex.from_state_dict({**l2_state, "metric_l2": fake(1, dtype=torch.uint8)})
    # the list functions
    q16, rows, ids, off = fake(256, 64, dtype=torch.float16), fake(48, 64, dtype=torch.float16), fake(48, dtype=torch.int32), \
        fake(4, dtype=torch.int32)
    probes = fake(5, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"k = .*\[1, 8\]"):
        index.search_lists_l2(q16, probes, rows, fake(48), ids, off, 9)
    with pytest.raises(ValueError, match="probes"):
        index.search_lists_l2(q16, fake(5, 9, dtype=torch.int32), rows, fake(48), ids, off, 8)
    with pytest.raises(ValueError, match="dim"):
        index.search_lists_l2(q16, probes, fake(48, 128, dtype=torch.float16), fake(48), ids, off, 8)
    with pytest.raises(ValueError, match=r"bias must be contiguous fp32 \[48\]"):
        index.search_lists_l2(q16, probes, rows, fake(47), ids, off, 8)
    with pytest.raises(ValueError, match="half_norms"):
        index.slot_bias(ids, fake(10, dtype=torch.float16))
    with pytest.raises(ValueError, match="ids"):
        index.slot_bias(fake(48, dtype=torch.int64), fake(10))


# ------------------------------------------------------------------------------------------------------- the C ABI
NAMES = {"smi_l2_prepare", "smi_l2_topk_ws_bytes", "smi_l2_topk", "smi_l2_slot_bias", "smi_l2_flat_search_ws_bytes",
         "smi_l2_flat_search", "smi_l2_kmeans_finalize", "smi_l2_kmeans_fit_ws_bytes", "smi_l2_kmeans_fit"}


def test_new_symbols_are_declared_bound_and_exported(lib):
    import os
    import subprocess

    from sonar_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "sonar_mi355.h")).read(), flags=re.S)
    assert NAMES <= set(re.findall(r"\b(smi_[a-z0-9_]+)\s*\(", header))
    assert NAMES <= set(_lib.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert NAMES <= set(re.findall(r"\bT (smi_[a-z0-9_]+)", out))
    # the pinned name sets stay as they are: no new smi_ivf_ / smi_pq_ entry, no new *_workspace_bytes
    assert not any(n.startswith(("smi_ivf_", "smi_pq_")) or n.endswith("_workspace_bytes") for n in NAMES)


def _no_device(rc):
    return rc == -3 if not torch.cuda.is_available() else True


def test_c_abi_of_prepare_and_topk(lib):
    tw, T, Pr = lib.smi_l2_topk_ws_bytes, lib.smi_l2_topk, lib.smi_l2_prepare
    # lists for one chunk per 256 rows of y up to 8 | both tile-major copies
    assert tw(1000, 100000, 4, 1024) == 8 * 1024 * 4 * 8 + (1024 + 100096) * 1024 * 2
    assert tw(1, 1, 1, 64) == 1 * 256 * 1 * 8 + 2 * 256 * 64 * 2 and tw(1, 1, 3, 64) == 256 * 4 * 8 + 2 * 256 * 64 * 2
    lib.smi_l2_topk(None, 1, None, 1, 64, 1, 0, None, None, None, None, 0, None)
    before = lib.smi_last_error()
    for bad in ((0, 5, 1, 64), (5, 0, 1, 64), (5, 5, 0, 64), (5, 5, 9, 64), (5, 5, 8, 96), (5, 5, 8, 0), (1 << 31, 5, 1, 64),
                (5, 1 << 31, 1, 64)):
        assert tw(*bad) == 0, bad
    assert lib.smi_last_error() == before  # a sizing call leaves the last error alone
    p, big = 0x1000, 1 << 40  # never dereferenced: every call below is refused on its arguments
    cases = {
        "k 0": T(p, 100, p, 300, 64, 0, 0, p, p, p, p, big, None),
        "k 9": T(p, 100, p, 300, 64, 9, 0, p, p, p, p, big, None),
        "d": T(p, 100, p, 300, 96, 8, 0, p, p, p, p, big, None),
        "nx": T(p, 0, p, 300, 64, 8, 0, p, p, p, p, big, None),
        "ny": T(p, 100, p, 0, 64, 8, 0, p, p, p, p, big, None),
        "big nx": T(p, 1 << 31, p, 300, 64, 8, 0, p, p, p, p, big, None),
        "null x": T(None, 100, p, 300, 64, 8, 0, p, p, p, p, big, None),
        "null y": T(p, 100, None, 300, 64, 8, 0, p, p, p, p, big, None),
        "null bias": T(p, 100, p, 300, 64, 8, 0, None, p, p, p, big, None),
        "misaligned bias": T(p, 100, p, 300, 64, 8, 0, p + 4, p, p, p, big, None),
        "null idx": T(p, 100, p, 300, 64, 8, 0, p, None, p, p, big, None),
        "null score": T(p, 100, p, 300, 64, 8, 0, p, p, None, p, big, None),
        "null ws": T(p, 100, p, 300, 64, 8, 0, p, p, p, None, big, None),
        "short ws": T(p, 100, p, 300, 64, 8, 0, p, p, p, p, tw(100, 300, 8, 64) - 1, None),
        "misaligned ws": T(p, 100, p, 300, 64, 8, 0, p, p, p, p + 8, big, None),
    }
    assert all(rc != 0 for rc in cases.values()), {k: v for k, v in cases.items() if v == 0}
    assert T(p, 100, p, 300, 64, 9, 0, p, p, p, p, big, None) == -2 and b"k=9 outside [1,8]" in lib.smi_last_error()
    assert T(p, 100, p, 300, 64, 8, 0, None, p, p, p, big, None) == -1 and b"y_bias" in lib.smi_last_error()
    assert T(p, 100, p, 300, 64, 8, 0, p, p, p, p, 16, None) == -1 and b"smi_l2_topk_ws_bytes" in lib.smi_last_error()
    assert _no_device(T(p, 100, p, 300, 64, 8, 0, p, p, p, p, tw(100, 300, 8, 64), None))
    cases = {
        "null src": Pr(None, 1, 10, 64, p, p, None), "null dst": Pr(p, 1, 10, 64, None, p, None),
        "dtype": Pr(p, 2, 10, 64, p, p, None), "rows": Pr(p, 1, 0, 64, p, p, None), "big rows": Pr(p, 1, 1 << 31, 64, p, p, None),
        "d": Pr(p, 1, 10, 20, p, p, None), "d 0": Pr(p, 1, 10, 0, p, p, None), "misaligned src": Pr(p + 2, 1, 10, 64, p, p, None),
        "misaligned dst": Pr(p, 1, 10, 64, p + 8, p, None), "misaligned norms": Pr(p, 1, 10, 64, p, p + 2, None),
    }
    assert all(rc != 0 for rc in cases.values()), {k: v for k, v in cases.items() if v == 0}
    assert _no_device(Pr(p, 0, 10, 8, p, None, None))  # fp32 source, d = 8, no half norms: every check passed


def test_c_abi_of_the_flat_search_and_slot_bias(lib):
    sw, fw, F, B = lib.smi_ivf_search_workspace_bytes, lib.smi_l2_flat_search_ws_bytes, lib.smi_l2_flat_search, lib.smi_l2_slot_bias
    assert fw(100, 7, 4, 5, 64) == sw(100, 7, 4, 5, 64) > 0  # the flat search's layout
    lib.smi_l2_slot_bias(None, 1, None, None, None)
    before = lib.smi_last_error()
    for bad in ((0, 7, 4, 5, 64), (100, 0, 4, 5, 64), (100, 7, 0, 5, 64), (100, 7, 9, 5, 64), (100, 7, 4, 0, 64), (100, 7, 4, 9, 64),
                (100, 7, 4, 5, 96), (1 << 31, 7, 1, 1, 64), (100, 1 << 31, 1, 1, 64)):
        assert fw(*bad) == 0, bad
    assert lib.smi_last_error() == before
    p, big = 0x1000, 1 << 40
    cases = {
        "d": F(p, 100, 96, p, 4, p, p, p, p, 7, 5, p, p, p, big, None),
        "K": F(p, 100, 64, p, 4, p, p, p, p, 0, 5, p, p, p, big, None),
        "nq": F(p, 0, 64, p, 4, p, p, p, p, 7, 5, p, p, p, big, None),
        "k 0": F(p, 100, 64, p, 4, p, p, p, p, 7, 0, p, p, p, big, None),
        "k 9": F(p, 100, 64, p, 4, p, p, p, p, 7, 9, p, p, p, big, None),
        "nprobe 0": F(p, 100, 64, p, 0, p, p, p, p, 7, 5, p, p, p, big, None),
        "nprobe 9": F(p, 100, 64, p, 9, p, p, p, p, 7, 5, p, p, p, big, None),
        "null q": F(None, 100, 64, p, 4, p, p, p, p, 7, 5, p, p, p, big, None),
        "null probes": F(p, 100, 64, None, 4, p, p, p, p, 7, 5, p, p, p, big, None),
        "null rows": F(p, 100, 64, p, 4, None, p, p, p, 7, 5, p, p, p, big, None),
        "null bias": F(p, 100, 64, p, 4, p, None, p, p, 7, 5, p, p, p, big, None),
        "misaligned bias": F(p, 100, 64, p, 4, p, p + 4, p, p, 7, 5, p, p, p, big, None),
        "null ids": F(p, 100, 64, p, 4, p, p, None, p, 7, 5, p, p, p, big, None),
        "null offsets": F(p, 100, 64, p, 4, p, p, p, None, 7, 5, p, p, p, big, None),
        "null idx": F(p, 100, 64, p, 4, p, p, p, p, 7, 5, None, p, p, big, None),
        "null score": F(p, 100, 64, p, 4, p, p, p, p, 7, 5, p, None, p, big, None),
        "null ws": F(p, 100, 64, p, 4, p, p, p, p, 7, 5, p, p, None, big, None),
        "short ws": F(p, 100, 64, p, 4, p, p, p, p, 7, 5, p, p, p, fw(100, 7, 4, 5, 64) - 1, None),
        "misaligned ws": F(p, 100, 64, p, 4, p, p, p, p, 7, 5, p, p, p + 4, big, None),
    }
    assert all(rc != 0 for rc in cases.values()), {k: v for k, v in cases.items() if v == 0}
    assert F(p, 100, 64, p, 4, p, p, p, p, 7, 5, p, p, p, 16, None) == -1 and b"smi_l2_flat_search_ws_bytes" in lib.smi_last_error()
    assert _no_device(F(p, 100, 64, p, 4, p, p, p, p, 7, 5, p, p, p, fw(100, 7, 4, 5, 64), None))
    assert B(None, 10, p, p, None) != 0 and B(p, 10, None, p, None) != 0 and B(p, 10, p, None, None) != 0 and B(p, 0, p, p, None) != 0
    assert _no_device(B(p, 10, p, p, None))


def test_c_abi_of_kmeans(lib):
    kw, Fit, Fin = lib.smi_l2_kmeans_fit_ws_bytes, lib.smi_l2_kmeans_fit, lib.smi_l2_kmeans_finalize
    up16 = lambda b: (b + 15) // 16 * 16  # noqa: E731
    # the update's workspace (cursor [K] | total [4] | order [n] | labels in bucket order [n]) | smi_l2_topk's at k = 1 | new
    # labels [n] | the centroids' bias [padded K] | the partial records
    assert kw(1000, 7, 64) == (up16(28) + 16 + 2 * up16(4000)) + lib.smi_l2_topk_ws_bytes(1000, 7, 1, 64) + up16(4000) + 1024 + 3072
    lib.smi_l2_kmeans_finalize(None, None, 1, 64, None, None, None, None, None)
    before = lib.smi_last_error()
    for bad in ((0, 7, 64), (1000, 0, 64), (1000, 7, 96), (1000, 7, 0), (1 << 31, 7, 64), (1000, 1 << 31, 64)):
        assert kw(*bad) == 0, bad
    assert lib.smi_last_error() == before
    p, big = 0x1000, 1 << 40

    def fit(**kw_):
        a = dict(x=p, n=1000, d=64, K=7, n_iter=1, resume=0, c32=p, c16=p, ch=p, labels=p, scores=p, sums=p, counts=p, obj=p, moved=p,
                 empty=p, ws=p, ws_bytes=big)
        a.update(kw_)
        return Fit(*a.values(), None)

    cases = {name: fit(**{name: None}) for name in ("x", "c32", "c16", "ch", "labels", "scores", "sums", "counts", "obj", "moved",
                                                     "empty", "ws")}
    cases.update({"n": fit(n=0), "K": fit(K=0), "d": fit(d=96), "n_iter": fit(n_iter=-1), "resume": fit(resume=2), "big n": fit(n=1 << 31),
                  "short ws": fit(ws_bytes=kw(1000, 7, 64) - 1), "misaligned ws": fit(ws=p + 8), "misaligned x": fit(x=p + 2)})
    assert all(rc != 0 for rc in cases.values()), {k: v for k, v in cases.items() if v == 0}
    assert fit(ws_bytes=16) == -1 and b"smi_l2_kmeans_fit_ws_bytes" in lib.smi_last_error()
    assert _no_device(fit(ws_bytes=kw(1000, 7, 64)))
    cases = {
        "null sums": Fin(None, p, 7, 64, p, p, p, p, None), "null counts": Fin(p, None, 7, 64, p, p, p, p, None),
        "null c32": Fin(p, p, 7, 64, None, p, p, p, None), "null c16": Fin(p, p, 7, 64, p, None, p, p, None),
        "null ch": Fin(p, p, 7, 64, p, p, None, p, None), "null empty": Fin(p, p, 7, 64, p, p, p, None, None),
        "K": Fin(p, p, 0, 64, p, p, p, p, None), "d": Fin(p, p, 7, 96, p, p, p, p, None), "misaligned": Fin(p, p, 7, 64, p + 4, p, p, p, None),
    }
    assert all(rc != 0 for rc in cases.values()), {k: v for k, v in cases.items() if v == 0}
    assert _no_device(Fin(p, p, 7, 64, p, p, p, p, None))
