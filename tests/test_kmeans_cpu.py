"""CPU: spherical k-means -- the fixed-point claim the exact update rests on, the numpy restatement against Python big
integers and against planted data, the seeded row initialisation, the refusals of the Python layer and of the C-ABI
(sonar_amd/clustering.py, sonar_amd/csrc/kmeans.hip, tests/kmeans_ref.py).  Nothing here needs a device."""
import numpy as np
import pytest
import torch

from tests import kmeans_ref as R


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def test_every_finite_fp16_is_an_integer_multiple_of_2_to_minus_24():
    bits = np.arange(1 << 16, dtype=np.uint16)
    h = bits.view(np.float16)
    finite = np.isfinite(h)
    assert int(finite.sum()) == 63488
    v = h[finite].astype(np.float64) * 2.0 ** 24
    assert np.array_equal(v, np.rint(v))
    small = np.abs(h[finite].astype(np.float64)) <= 1.0
    assert np.abs(v[small]).max() == 2.0 ** 24  # |x| <= 1: the integer is at most 2^24
    assert np.abs(v).max() == 65504.0 * 2.0 ** 24 < 2.0 ** 41
    # the restatement's conversion, from the bit fields: (1024 + m) << (e - 1), subnormals m, as csrc/kmeans.hip does it
    e, m = ((bits >> 10) & 31).astype(np.int64), (bits & 1023).astype(np.int64)
    q = np.where(e > 0, (m | 1024) << np.maximum(e - 1, 0), m) * np.where(bits & 0x8000, -1, 1)
    q = np.where(e == 31, 0, q)
    assert np.array_equal(q, R.fixed(h))
    assert (R.fixed(h)[~finite] == 0).all()


def test_restated_sums_equal_python_big_integers():
    rng = np.random.default_rng(1)
    n, d, k = 97, 64, 5
    x = rng.standard_normal((n, d)).astype(np.float16)
    x[3, 7], x[4, 9] = np.inf, np.nan
    x[5] = np.float16(65504.0)
    labels = rng.integers(-1, k + 1, n)  # -1 and k: skipped rows
    sums, counts = R.update(x, labels, k)
    from fractions import Fraction

    for c in range(k):
        rows = [i for i in range(n) if labels[i] == c]
        assert counts[c] == len(rows)
        for j in range(d):
            exact = sum((Fraction(float(x[i, j])) for i in rows if np.isfinite(x[i, j])), Fraction(0)) * (1 << 24)
            assert exact.denominator == 1 and int(exact) == int(sums[c, j])


def test_finalize_restated():
    sums = np.array([[1 << 24, 0], [(1 << 25) + 1, 3], [0, 0], [5, 5]], dtype=np.int64)
    counts = np.array([1, 2, 2, 0], dtype=np.int32)
    prev = np.full((4, 2), 9.0, dtype=np.float32)
    c, empty = R.finalize(sums, counts, prev)
    assert empty == 2 and (c[2] == 9.0).all() and (c[3] == 9.0).all()
    assert c[0, 0] == 1.0 and c[0, 1] == 0.0
    assert c[1, 0] == 2.0 and c[1, 1] == np.float32(3 * 2.0 ** -24)  # 2^25 + 1 has 26 bits: rounds to 2^25


@pytest.mark.parametrize("n,k,d", R.PLANTED_SHAPES)
def test_planted_clusters_are_recovered_with_a_wide_margin(n, k, d):
    x, truth, init = R.planted(n, k, d)
    rounds = R.fit(x, init, 4)
    assert len(rounds) == 5
    for r in rounds:
        assert np.array_equal(r["labels"], truth)
        assert r["margin"].min() >= 0.1, r["margin"].min()
    assert all(r["empty"] == 0 for r in rounds[1:])
    obj = [r["scores"].sum() for r in rounds]
    assert obj[1] > obj[0]  # the members' mean is closer to them than their first member


def test_restated_empty_and_duplicate_clusters():
    x, truth, init = R.planted(200, 4, 64)
    init = np.concatenate([init, init[:1]])  # a duplicate of centroid 0: ties go to the lower index, it gets no row
    rounds = R.fit(x, init, 1)
    assert np.array_equal(rounds[0]["labels"], truth)
    # the first update finds it empty and keeps it where it was (from there it may win rows later: it is x[0] itself)
    assert rounds[1]["empty"] == 1 and np.array_equal(rounds[1]["centroids"][4], init[4].astype(np.float32))
    assert not np.array_equal(rounds[1]["centroids"][0], init[0].astype(np.float32))


def test_row_initialisation_is_seeded_and_distinct():
    from sonar_amd.clustering import init_rows

    a, b, c = init_rows(1000, 37, 5), init_rows(1000, 37, 5), init_rows(1000, 37, 6)
    assert a.dtype == torch.int64 and a.device.type == "cpu" and a.shape == (37,)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert len(set(a.tolist())) == 37 and 0 <= int(a.min()) and int(a.max()) < 1000
    assert sorted(init_rows(9, 9, 0).tolist()) == list(range(9))
    with pytest.raises(ValueError, match="exceeds"):
        init_rows(5, 6, 0)


def test_python_refusals_need_no_device():
    from sonar_amd.clustering import SphericalKMeans, update

    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_clusters"):
            SphericalKMeans(bad)
    for bad in (-1, 1.5, False):
        with pytest.raises(ValueError, match="n_iter"):
            SphericalKMeans(3, n_iter=bad)
    km = SphericalKMeans(3, n_iter=2)
    x = torch.zeros(8, 64)
    with pytest.raises(RuntimeError, match="HIP device only"):
        km.fit(x)
    with pytest.raises(RuntimeError, match="HIP device only"):
        km.fit_normalized(x.half(), 8)
    with pytest.raises(TypeError):
        km.fit(np.zeros((8, 64)))
    for what in ("predict", "step"):
        with pytest.raises(RuntimeError, match="before fit"):
            getattr(km, what)(*(() if what == "step" else (x,)))
    with pytest.raises(RuntimeError, match="before fit"):
        km.centroids
    with pytest.raises(RuntimeError, match="before fit"):
        km.history
    for bad in (0, 9, 1.0, True):
        with pytest.raises(ValueError, match=r"\[1, 8\]"):
            km.predict(x, k=bad)
    with pytest.raises(RuntimeError, match="HIP device only"):
        update(x.half(), torch.zeros(8, dtype=torch.int32), 3)


def test_shape_refusals_come_before_any_launch(monkeypatch):
    """Rank, dimension, K > n and the shape of init are checked on meta tensors that claim to be on the device: nothing
    could be launched on them, so a refusal that came late would surface as a different error."""
    from sonar_amd import clustering
    from sonar_amd.clustering import SphericalKMeans

    class FakeDevice(torch.Tensor):
        is_cuda = True

    def fake(*shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device="meta").as_subclass(FakeDevice)

    def boom(*a, **k):
        raise AssertionError("reached the device")

    monkeypatch.setattr(clustering, "normalize_rows", boom)
    monkeypatch.setattr(clustering._lib, "load", boom)
    km = SphericalKMeans(4)
    with pytest.raises(ValueError, match=r"\[rows, dim\]"):
        km.fit(fake(8))
    with pytest.raises(ValueError, match=r"\[rows, dim\]"):
        km.fit(fake(2, 8, 64))
    with pytest.raises(ValueError, match="multiple of 64"):
        km.fit(fake(8, 96))
    with pytest.raises(ValueError, match="empty"):
        km.fit(fake(0, 64))
    with pytest.raises(ValueError, match="exceeds"):
        km.fit(fake(3, 64))
    with pytest.raises(ValueError, match="exceeds"):
        km.fit_normalized(fake(256, 64, dtype=torch.float16), 3)
    for shape in ((3, 64), (4, 128), (4,)):
        with pytest.raises(ValueError, match="init"):
            km.fit(fake(8, 64), init=fake(*shape))
    with pytest.raises(RuntimeError, match="HIP device only"):
        km.fit(fake(8, 64), init=torch.zeros(4, 64))
    with pytest.raises(ValueError, match="padded rows"):
        km.fit_normalized(fake(256, 64, dtype=torch.float16), 257)
    with pytest.raises(ValueError, match="fp16"):
        km.fit_normalized(fake(256, 64), 8)


def test_c_abi_refusals_without_a_device(lib):
    from sonar_amd import _lib

    assert _lib.ABI_VERSION == 7 and lib.smi_abi_version() == 7
    wsb = lib.smi_kmeans_workspace_bytes
    assert wsb(1000, 7, 1024) > 0 and wsb(1000, 7, 1024) % 16 == 0
    assert wsb(1000, 7, 96) == 0 and wsb(1000, 0, 64) == 0 and wsb(0, 7, 64) == 0 and wsb(1 << 31, 7, 64) == 0
    assert wsb(2000, 7, 1024) >= wsb(1000, 7, 1024) >= wsb(1, 7, 1024)
    # update: cursor [K] | total | order [n] | bucketed labels [n]; finalise: flags [K] | fp16 rows [padded K][d]
    assert wsb(100000, 7, 64) == 32 + 16 + 2 * 400000
    assert wsb(1, 300, 1024) == 1200 + 512 * 1024 * 2
    p = 0x1000  # never dereferenced: every call below is refused on its arguments
    need = wsb(100, 7, 64)
    cases = {
        "update d": lib.smi_kmeans_update(p, p, 100, 96, 7, p, p, p, 1 << 30, None),
        "update K": lib.smi_kmeans_update(p, p, 100, 64, 0, p, p, p, 1 << 30, None),
        "update n": lib.smi_kmeans_update(p, p, 0, 64, 7, p, p, p, 1 << 30, None),
        "update big n": lib.smi_kmeans_update(p, p, 1 << 31, 64, 7, p, p, p, 1 << 40, None),
        "update null x": lib.smi_kmeans_update(None, p, 100, 64, 7, p, p, p, 1 << 30, None),
        "update null labels": lib.smi_kmeans_update(p, None, 100, 64, 7, p, p, p, 1 << 30, None),
        "update null sums": lib.smi_kmeans_update(p, p, 100, 64, 7, None, p, p, 1 << 30, None),
        "update null counts": lib.smi_kmeans_update(p, p, 100, 64, 7, p, None, p, 1 << 30, None),
        "update null ws": lib.smi_kmeans_update(p, p, 100, 64, 7, p, p, None, 1 << 30, None),
        "update short ws": lib.smi_kmeans_update(p, p, 100, 64, 7, p, p, p, need - 1, None),
        "update misaligned ws": lib.smi_kmeans_update(p, p, 100, 64, 7, p, p, p + 8, 1 << 30, None),
        "finalize d": lib.smi_kmeans_finalize(p, p, 7, 96, p, p, p, p, 1 << 30, None),
        "finalize K": lib.smi_kmeans_finalize(p, p, 0, 64, p, p, p, p, 1 << 30, None),
        "finalize null": lib.smi_kmeans_finalize(p, p, 7, 64, None, p, p, p, 1 << 30, None),
        "finalize null count": lib.smi_kmeans_finalize(p, p, 7, 64, p, p, None, p, 1 << 30, None),
        "finalize short ws": lib.smi_kmeans_finalize(p, p, 7, 64, p, p, p, p, wsb(1, 7, 64) - 1, None),
        "fit d": lib.smi_kmeans_fit(p, 100, 96, 7, 1, 0, p, p, p, p, p, p, p, p, p, p, 1 << 40, None),
        "fit K": lib.smi_kmeans_fit(p, 100, 64, 0, 1, 0, p, p, p, p, p, p, p, p, p, p, 1 << 40, None),
        "fit n_iter": lib.smi_kmeans_fit(p, 100, 64, 7, -1, 0, p, p, p, p, p, p, p, p, p, p, 1 << 40, None),
        "fit resume": lib.smi_kmeans_fit(p, 100, 64, 7, 1, 2, p, p, p, p, p, p, p, p, p, p, 1 << 40, None),
        "fit null": lib.smi_kmeans_fit(p, 100, 64, 7, 1, 0, p, p, None, p, p, p, p, p, p, p, 1 << 40, None),
        "fit short ws": lib.smi_kmeans_fit(p, 100, 64, 7, 1, 0, p, p, p, p, p, p, p, p, p, p,
                                           need + lib.smi_xsim_workspace_bytes(100, 7, 1, 64) + 400 + 3072 - 1, None),
    }
    assert all(rc != 0 for rc in cases.values()), {k: v for k, v in cases.items() if v == 0}
    assert lib.smi_kmeans_update(p, p, 100, 64, 7, p, p, p, need - 1, None) == -1
    assert b"smi_kmeans_workspace_bytes" in lib.smi_last_error()
    assert lib.smi_kmeans_update(p, p, 100, 96, 7, p, p, p, 1 << 30, None) == -2 and b"multiple of 64" in lib.smi_last_error()
