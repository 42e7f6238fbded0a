"""CPU: the PCA / OPQ transforms -- the numpy restatement (tests/transforms_ref.py) against numpy itself, the Procrustes step,
the planted-data criterion the GPU test repeats on the device, and every refusal of the Python layer (sonar_amd/transforms.py,
sonar_amd/index.py `PreTransformIndex`) and of the C-ABI (sonar_amd/csrc/gram.hip).  Nothing here needs a device."""
import itertools
import math
import re

import numpy as np
import pytest
import torch

from tests import transforms_ref as R


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


# ------------------------------------------------------------------------------------------------------- restatement
def test_chunked_integer_gram_equals_the_plain_product():
    rng = np.random.default_rng(0)
    x = rng.integers(-8, 9, (3 * 64 + 5, 64)).astype(np.float16)
    y = rng.integers(-8, 9, (3 * 64 + 5, 128)).astype(np.float16)
    for chunk in (1, 64, 100, 1000):
        assert np.array_equal(R.gram_int(x, y, chunk), x.astype(np.int64).T @ y.astype(np.int64))
    g = R.gram_int(x, chunk=64)
    assert np.array_equal(g, g.T) and np.array_equal(g, R.gram64(x).astype(np.int64))
    with pytest.raises(AssertionError, match="exact range"):
        R.gram_int(np.full((2 ** 12, 64), 64.0), chunk=2 ** 12)  # 2^12 products of 2^12
    with pytest.raises(AssertionError, match="integer-valued"):
        R.gram_int(np.full((4, 64), 0.5))


def test_restated_pca_against_numpy():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((500, 64)) * np.linspace(2.0, 0.1, 64)) @ np.linalg.qr(rng.standard_normal((64, 64)))[0] + 0.3
    c, mu = R.covariance(x)
    assert np.allclose(c, np.cov(x, rowvar=False), rtol=0, atol=1e-12 * np.abs(c).max())
    assert np.allclose(mu, x.mean(axis=0), rtol=0, atol=1e-14)
    m, b, ev, _ = R.pca(x, 16)
    assert np.allclose(ev, np.linalg.eigvalsh(c)[::-1][:16], rtol=0, atol=1e-12 * ev[0])
    assert np.all(np.diff(ev) <= 0)
    assert np.abs(m @ m.T - np.eye(16)).max() < 1e-12
    assert np.abs(m @ c @ m.T - np.diag(ev)).max() < 1e-12 * ev[0]
    assert np.allclose(b, -(m @ mu), rtol=0, atol=1e-14)
    # the projected, centred rows are uncorrelated with the stated variances
    z = x @ m.T + b
    assert np.abs(np.cov(z, rowvar=False) - np.diag(ev)).max() < 1e-10 * ev[0]
    assert R.pca(x, 16, center=False)[1] is None


def test_sign_rule():
    v = np.array([[0.5, -0.5, 0.1, -3.0], [-0.5, 0.5, -0.2, 3.0], [0.1, 0.1, 0.2, 1.0]])
    f = R.fix_signs(v)
    # column 0: tie between rows 0 and 1, the lower index decides (+0.5 stays); column 1: the same tie, -0.5 flips;
    # column 2: tie between rows 1 and 2 (|-0.2| = |0.2|), row 1 decides and flips; column 3: tie of 3.0, row 0 flips
    assert np.array_equal(f[:, 0], v[:, 0]) and np.array_equal(f[:, 1], -v[:, 1])
    assert np.array_equal(f[:, 2], -v[:, 2]) and np.array_equal(f[:, 3], -v[:, 3])
    from sonar_amd.transforms import _fix_signs

    assert np.array_equal(_fix_signs(torch.from_numpy(v)).numpy(), f)
    rng = np.random.default_rng(2)
    w = rng.standard_normal((64, 64))
    assert np.array_equal(_fix_signs(torch.from_numpy(w)).numpy(), R.fix_signs(w))


def test_balanced_allocation_follows_its_rule_and_fills_every_bin():
    from sonar_amd.transforms import balanced_bins

    rng = np.random.default_rng(3)
    for trial in range(20):
        ev = np.sort(rng.uniform(0.5, 50.0, 8) ** (1 + trial % 3))[::-1]
        bins = R.balanced_bins(ev, 2)
        assert bins == balanced_bins(ev, 2)
        assert sorted(i for b in bins for i in b) == list(range(8)) and all(len(b) == 4 for b in bins)
        # the stated rule, replayed: every eigenvalue went to the bin with the smaller running sum that had room
        acc, fill = [0.0, 0.0], [0, 0]
        where = {i: b for b in range(2) for i in bins[b]}
        for i in range(8):
            open_bins = [b for b in range(2) if fill[b] < 4]
            want = min(open_bins, key=lambda b: (acc[b], b))
            assert where[i] == want, (trial, i)
            acc[want] += math.log(ev[i])
            fill[want] += 1
        # against brute force over all 70 splits: the greedy need not be optimal (only its rule is asserted), but on these
        # spectra it is always better balanced than no allocation at all (the first four against the last four)
        logs = np.log(ev)
        gap = lambda b0: abs(logs[list(b0)].sum() - logs[[i for i in range(8) if i not in b0]].sum())
        best = min(gap(c) for c in itertools.combinations(range(8), 4))
        assert best <= gap(bins[0]) + 1e-12
        assert gap(bins[0]) < gap((0, 1, 2, 3)), (trial, gap(bins[0]), gap((0, 1, 2, 3)))
    assert R.balanced_bins([4.0, 0.0, 0.0, 0.0], 2) == [[0, 3], [1, 2]] == balanced_bins([4.0, 0.0, 0.0, 0.0], 2)
    with pytest.raises(ValueError, match="bins"):
        balanced_bins([1.0, 2.0, 3.0], 2)


def test_procrustes_step_never_raises_the_error_and_stays_orthogonal():
    rng = np.random.default_rng(4)
    x = R.planted(4, 512, 64).astype(np.float64)
    r = np.linalg.qr(rng.standard_normal((64, 64)))[0]
    for _ in range(3):
        xhat = np.round((x @ r) * 8) / 8  # any fixed reconstruction
        r2 = R.procrustes(x, xhat)
        assert np.abs(r2.T @ r2 - np.eye(64)).max() < 1e-12
        assert np.linalg.norm(x @ r2 - xhat) <= np.linalg.norm(x @ r - xhat) * (1 + 1e-12)
        r = r2


def test_planted_data_opq_beats_plain_pq():
    """The criterion of DESIGN.md 3.25 on the restatement: 4096 x 128 planted rows, dsub 16, 256 codewords from the first
    256 rows, 8 Lloyd rounds."""
    x = R.planted(0).astype(np.float64)
    init = np.arange(256)
    plain, _ = R.pq_error(x, 16, init, 8)
    r, history = R.opq(x, 16, 1, 8, init)
    print(f"planted data: plain PQ {plain:.4f}, OPQ start {history[0]:.4f}, after one Procrustes round {history[1]:.4f}")
    assert np.abs(r.T @ r - np.eye(128)).max() < 1e-12
    assert history[0] <= 0.6 * plain and history[-1] <= 0.6 * plain, (plain, history)


# ------------------------------------------------------------------------------------------------------- refusals
class FakeDevice(torch.Tensor):
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta").as_subclass(FakeDevice)


def boom(*a, **k):
    raise AssertionError("reached the device")


def test_python_refusals_need_no_device(monkeypatch):
    from sonar_amd import index, transforms
    from sonar_amd.index import IVFFlatIndex, PreTransformIndex
    from sonar_amd.transforms import OPQ, PCA, LinearTransform, column_sums, gram

    header = open(index.__file__.replace("sonar_amd/index.py", "include/sonar_mi355.h")).read()
    assert int(re.search(r"#define SMI_GRAM_CHUNK_ROWS (\d+)", header).group(1)) == transforms.GRAM_CHUNK_ROWS == R.CHUNK_ROWS
    assert 1024 <= transforms.GRAM_CHUNK_ROWS <= 8192
    monkeypatch.setattr(transforms._lib, "load", boom)
    monkeypatch.setattr(transforms, "normalize_rows", boom)
    f16 = lambda *s: fake(*s, dtype=torch.float16)
    # gram / column_sums
    for fn in (gram, column_sums):
        with pytest.raises(TypeError):
            fn(np.zeros((4, 64), dtype=np.float16))
        with pytest.raises(RuntimeError, match=r"HIP device only \(no CPU path\)"):
            fn(torch.zeros(4, 64, dtype=torch.float16))
        with pytest.raises(ValueError, match="multiple of 64"):
            fn(f16(4, 96))
        with pytest.raises(ValueError, match=r"\[rows, dim\]"):
            fn(f16(4))
        with pytest.raises(ValueError, match="contiguous fp16"):
            fn(fake(4, 64))
        for bad in (0, 5, True, 2.0):
            with pytest.raises(ValueError, match="n = "):
                fn(f16(4, 64), n=bad)
    with pytest.raises(RuntimeError, match="HIP device only"):
        gram(f16(4, 64), torch.zeros(4, 64, dtype=torch.float16))
    with pytest.raises(ValueError, match="contiguous fp16"):
        gram(f16(4, 64), fake(4, 64))
    with pytest.raises(ValueError, match="n = 4"):
        gram(f16(4, 64), f16(3, 128))  # y has fewer rows than the call takes
    with pytest.raises(ValueError, match="exceeds 8192"):
        gram(f16(4, 8256))
    # LinearTransform
    with pytest.raises(TypeError):
        LinearTransform(np.zeros((128, 64)))
    with pytest.raises(RuntimeError, match="HIP device only"):
        LinearTransform(torch.zeros(128, 64))
    for shape, what in (((128,), r"\[d_out, d_in\]"), ((128, 96), "d_in = 96"), ((64, 64), "d_out = 64"), ((192, 64), "d_out = 192")):
        with pytest.raises(ValueError, match=what):
            LinearTransform(fake(*shape))
    with pytest.raises(ValueError, match="floating-point"):
        LinearTransform(fake(128, 64, dtype=torch.int32))
    with pytest.raises(ValueError, match="bias must be"):
        LinearTransform(fake(128, 64), fake(64))
    with pytest.raises(RuntimeError, match="HIP device only"):
        LinearTransform(fake(128, 64), torch.zeros(128))
    t = LinearTransform(fake(128, 64), fake(128))
    assert (t.d_in, t.d_out) == (64, 128) and t.matrix.dtype == torch.float16 and t.matrix64.dtype == torch.float64
    assert t.bias.dtype == torch.float32 and LinearTransform(fake(128, 64)).bias is None
    with pytest.raises(RuntimeError, match="HIP device only"):
        t.apply(torch.zeros(4, 64))
    with pytest.raises(ValueError, match="dim 128"):
        t.apply(fake(4, 128))
    with pytest.raises(ValueError, match="fp16 or fp32"):
        t.apply(fake(4, 64, dtype=torch.float64))
    with pytest.raises(ValueError, match="empty"):
        t.apply(fake(0, 64))
    with pytest.raises(ValueError, match="lacks"):
        LinearTransform.from_state_dict({})
    # PCA.fit
    with pytest.raises(RuntimeError, match="HIP device only"):
        PCA.fit(torch.zeros(300, 128))
    with pytest.raises(ValueError, match="multiple of 64"):
        PCA.fit(fake(300, 96))
    with pytest.raises(ValueError, match="fp16 or fp32"):
        PCA.fit(fake(300, 128, dtype=torch.bfloat16))
    for bad in (64, 192, 384, 0, True, 128.0):
        with pytest.raises(ValueError, match="d_out = "):
            PCA.fit(fake(300, 256), d_out=bad)
    with pytest.raises(ValueError, match="d_out = 64"):
        PCA.fit(fake(300, 64))  # the default d_out = d is no multiple of 128
    with pytest.raises(ValueError, match="at least 2 rows"):
        PCA.fit(fake(1, 128))
    # OPQ.fit
    with pytest.raises(RuntimeError, match="HIP device only"):
        OPQ.fit(torch.zeros(300, 128), 16)
    for bad in (12, 0, 128, True):
        with pytest.raises(ValueError, match="dsub = "):
            OPQ.fit(fake(300, 128), bad)
    with pytest.raises(ValueError, match="does not divide"):
        index._check_dsub(16, 72)  # OPQ.fit's own check; behind "dim a multiple of 64" every legal dsub divides
    with pytest.raises(ValueError, match="multiple of 128"):
        OPQ.fit(fake(300, 192), 16)
    for name in ("n_iter", "pq_iter"):
        for bad in (-1, 1.5, True):
            with pytest.raises(ValueError, match=name):
                OPQ.fit(fake(300, 128), 16, **{name: bad})
    for bad in (255, 301, True):
        with pytest.raises(ValueError, match="n_train"):
            OPQ.fit(fake(300, 128), 16, n_train=bad)
    with pytest.raises(ValueError, match="n_train"):
        OPQ.fit(fake(200, 128), 16)  # fewer rows than codewords
    # PreTransformIndex
    monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=torch.float16))
    ix = IVFFlatIndex(fake(3, 128))
    with pytest.raises(ValueError, match="gives dim 128, the index takes 64"):
        PreTransformIndex(t, IVFFlatIndex(fake(3, 64)))
    with pytest.raises(TypeError, match="LinearTransform"):
        PreTransformIndex(fake(128, 64), ix)
    with pytest.raises(TypeError, match="index must be"):
        PreTransformIndex(t, t)
    pt = PreTransformIndex(t, ix)
    assert pt.dim == 64 and pt.n_lists == 3
    with pytest.raises(RuntimeError, match="before add"):
        pt.ntotal
    with pytest.raises(ValueError, match="dim 128"):
        pt.add(fake(8, 128))
    with pytest.raises(RuntimeError, match="HIP device only"):
        pt.search(torch.zeros(5, 64))
    with pytest.raises(ValueError, match="refine must be"):
        pt.search(fake(5, 64), refine=f16(10, 128))  # the corpus of the transformed space
    with pytest.raises(TypeError, match="positional"):
        pt.search(fake(5, 64), 1, 1, None, f16(10, 64))  # refine goes by keyword: never silently to the wrapped class
    with pytest.raises(TypeError, match="index_cls"):
        PreTransformIndex.from_state_dict({}, LinearTransform)


def test_c_abi_sizing_and_refusals_without_a_device(lib):
    ws, G = lib.smi_gram_ws_bytes, lib.smi_gram
    tile = 128 * 128 * 8
    chunk = R.CHUNK_ROWS
    assert ws(1, 64, 64) == tile and ws(chunk, 128, 128) == tile and ws(chunk + 1, 128, 128) == 2 * tile
    assert ws(32 * chunk, 192, 64) == 32 * 2 * tile and ws(32 * chunk + 1, 192, 64) == 17 * 2 * tile  # spans of 2 chunks
    assert ws(1 << 20, 1024, 1024) == 32 * 64 * tile
    for bad in ((0, 64, 64), (-1, 64, 64), (10, 0, 64), (10, 64, 32), (10, 96, 64), (10, 64, 8256), (10, 8256, 64),
                ((1 << 31) - 255, 64, 64), (1 << 40, 64, 64)):
        assert ws(*bad) == 0, bad
    assert ws((1 << 31) - 256, 64, 64) > 0
    p, big = 0x1000, 1 << 50  # never dereferenced: every call below is refused on its arguments
    cases = {
        "null x": (G(None, p, 10, 64, 64, p, p, big, None), -1, "null"),
        "null out": (G(p, p, 10, 64, 64, None, p, big, None), -1, "null"),
        "null ws": (G(p, p, 10, 64, 64, p, None, big, None), -1, "null workspace"),
        "n 0": (G(p, p, 0, 64, 64, p, p, big, None), -1, "n < 1"),
        "d1 32": (G(p, p, 10, 32, 64, p, p, big, None), -2, "multiples of 64"),
        "d2 96": (G(p, p, 10, 64, 96, p, p, big, None), -2, "multiples of 64"),
        "d1 big": (G(p, p, 10, 8256, 64, p, p, big, None), -2, "8192"),
        "big n": (G(p, p, (1 << 31) - 255, 64, 64, p, p, big, None), -2, "2^31 - 256"),
        "sym d": (G(p, None, 10, 64, 128, p, p, big, None), -1, "symmetric"),
        "short ws": (G(p, p, 10, 64, 64, p, p, tile - 1, None), -1, "smi_gram_ws_bytes"),
        "misaligned ws": (G(p, p, 10, 64, 64, p, p + 8, big, None), -1, "16-byte aligned"),
    }
    for name, (rc, want, _) in cases.items():
        assert rc == want, (name, rc)
    # the texts, one call at a time (smi_last_error is the last refusal's)
    assert G(p, p, 10, 64, 96, p, p, big, None) == -2 and b"multiples of 64" in lib.smi_last_error()
    assert G(p, p, 10, 64, 64, p, p, tile - 1, None) == -1 and b"smi_gram_ws_bytes" in lib.smi_last_error()
    assert G(None, p, 10, 64, 64, p, p, big, None) == -1 and b"null" in lib.smi_last_error()
    # the symmetric form is content with the tile slots of its upper triangle: 3 of 4 at d = 256
    assert ws(10, 256, 256) == 4 * tile
    assert G(p, None, 10, 256, 256, p, p, 3 * tile - 1, None) == -1 and b"T (T + 1) / 2" in lib.smi_last_error()
    assert G(p, p, 10, 256, 256, p, p, 3 * tile, None) == -1 and b"smi_gram_ws_bytes(n, d1, d2) = " in lib.smi_last_error()
    if not torch.cuda.is_available():
        assert G(p, None, 10, 256, 256, p, p, 3 * tile, None) == -3  # past every argument check
        assert G(p, p, 10, 64, 64, p, p, big, None) == -3 and b"no HIP device" in lib.smi_last_error()
