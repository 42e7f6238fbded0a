"""CPU: residual encoding against the list centroid for the IVF-PQ index.  The residual rule against exact
rational arithmetic, the restated search (tests/ivf_pq_residual_ref.py) against a plain double loop, the planted-data
conditions the GPU test relies on, every refusal of the Python layer and of the C entry points, and the separation of the
plain and the residual state dicts; none of it needs a device."""
import functools

import numpy as np
import pytest
import torch

from tests import ivf_pq_ref as P
from tests import ivf_pq_residual_ref as PR
from tests import ivf_ref as R
from tests.test_ivf_cpu import FakeDevice, boom, fake  # noqa: F401  (the stand-ins for device tensors)
from tests.test_ivf_i8_cpu import f32_round
from tests.test_ivf_pq_cpu import EXTREME, F, f16_round


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


# ------------------------------------------------------------------------------------------------------- the residual
def test_residual_rule_is_two_roundings_of_the_exact_difference():
    """fp16_rn(fp32_rn(x - c)) in exact rationals, on pairs whose fp32 difference is inexact too, and a label out of range."""
    rng = np.random.default_rng(0)
    # 1 + 2^-10 against 2^-24: the difference needs 25 significant bits; 65504 against a subnormal: far more
    hard = np.array([[1.0 + 2.0 ** -10, 2.0 ** -24], [-(1.0 + 2.0 ** -10), 2.0 ** -24], [65504.0, 2.0 ** -24], [0.5 + 2.0 ** -11, -3 * 2.0 ** -24],
                     [1.0, 1.0], [0.0, -0.0], [-0.0, 0.0], [2.0 ** -24, -(2.0 ** -24)], [0.333, -0.333], [1023 * 2.0 ** -24, 1.0],
                     [2049.0 * 2.0 ** -11, 7e-5], [-3.14, 1e-3]], dtype=np.float16)
    vals = np.concatenate([EXTREME[np.abs(EXTREME) < 60000], R.normalize64(rng.standard_normal((4, 64))).astype(np.float16).reshape(-1)])
    xs = np.concatenate([hard[:, 0], rng.choice(vals, 500)])
    cs = np.concatenate([hard[:, 1], rng.choice(vals, 500)])
    d = 64
    n = len(xs) // d
    x, c = xs[: n * d].reshape(n, d), cs[: n * d].reshape(n, d)
    labels = np.arange(n)
    got = PR.residuals(x, labels, c)
    assert got.dtype == np.float16 and got.shape == x.shape
    inexact = 0
    for xv, cv, g in zip(x.reshape(-1), c.reshape(-1), got.reshape(-1)):
        diff = F(xv) - F(cv)
        in32 = f32_round(diff)
        inexact += in32 != diff
        assert F(g) == f16_round(in32), (xv, cv, g)
        assert F(np.float32(xv) - np.float32(cv)) == in32  # numpy's float32 subtraction is the correctly rounded one
    assert inexact >= 4
    assert got[0, 4] == 0 and not np.signbit(got[0, 4])  # a row equal to its centroid: +0
    # a label outside [0, K) addresses nothing: the residual is the row itself, bit for bit
    for bad in (-1, n, 2 ** 31 - 1):
        lab = labels.copy()
        lab[1] = bad
        out = PR.residuals(x, lab, c)
        assert np.array_equal(out[1].view(np.uint16), x[1].view(np.uint16)) and np.array_equal(out[0].view(np.uint16), got[0].view(np.uint16))
    # a residual of normalised operands is a multiple of 2^-24 with |r| <= 2: the exact int64 training sums carry over
    xn, cn = (R.normalize64(rng.standard_normal((50, d))).astype(np.float16) for _ in range(2))
    r = PR.residuals(xn, np.arange(50), cn)
    assert np.abs(r.astype(np.float64)).max() <= 2 and np.array_equal(np.rint(r.astype(np.float64) * 2 ** 24), r.astype(np.float64) * 2 ** 24)


def test_restated_training_and_encoding_are_the_plain_ones_on_the_residuals():
    rng = np.random.default_rng(1)
    n, d, dsub, k = 300, 64, 16, 5
    x, c = R.normalize64(rng.standard_normal((n, d))).astype(np.float16), R.normalize64(rng.standard_normal((k, d))).astype(np.float16)
    labels = rng.integers(-1, k + 1, n)
    init = rng.permutation(n)[:256]
    r = PR.residuals(x, labels, c)
    books = PR.train(x, labels, c, init, dsub, 2)
    assert len(books) == 3
    assert np.array_equal(books[0].view(np.uint16), P.init_codebooks(r, init, dsub).view(np.uint16))  # starts from the residuals
    assert np.array_equal(books[-1].view(np.uint16), P.train(r, init, dsub, 2)[-1].view(np.uint16))
    assert np.array_equal(PR.encode(x, labels, c, books[-1]), P.encode(r, books[-1]))
    moved = labels.copy()
    moved[0] = (labels[0] + 1) % k if 0 <= labels[0] < k else 0
    assert not np.array_equal(PR.encode(x[:1], moved[:1], c, books[-1]), PR.encode(x[:1], labels[:1], c, books[-1]))  # codes depend on the label


# ------------------------------------------------------------------------------------------------------- search
def search_loop(q16, x16, labels, k_lists, probes, coarse, k):
    """Every (probed list, member) a candidate of score q . x + coarse; a stable sort by (score descending, id ascending)."""
    out_s, out_i = [], []
    for r, row in enumerate(probes):
        cand = []
        for p, c in enumerate(row):
            if 0 <= c < k_lists:
                for i in range(len(x16)):
                    if labels[i] == c:
                        s = float(sum(float(a) * float(b) for a, b in zip(q16[r], x16[i]))) + float(coarse[r, p])
                        cand.append((-s, i))
        cand.sort()
        cand = cand[:k] + [(np.inf, -1)] * (k - min(k, len(cand)))
        out_s.append([-s for s, _ in cand])
        out_i.append([i for _, i in cand])
    return np.array(out_s), np.array(out_i)


def test_restated_search_equals_a_plain_loop():
    rng = np.random.default_rng(4)
    n, d, dsub, k_lists, nq = 120, 64, 16, 5, 9
    cb = P.integer_codebooks(rng, d, dsub)
    codes = rng.integers(0, 256, (n, d // dsub)).astype(np.uint8)
    codes[7] = codes[3]
    q = R.integer_rows(rng, nq, d)
    labels = rng.integers(-1, k_lists + 1, n)
    labels[3], labels[7] = 2, 0  # the same decoded row in two lists
    probes = rng.integers(-1, k_lists + 1, (nq, 3))
    probes[0] = [2, -1, 0]
    coarse = rng.integers(-3, 4, (nq, 3)).astype(np.float32)
    coarse[probes < 0] = np.nan  # the entry of a probe that names no list is not read
    coarse[probes >= k_lists] = np.inf
    coarse[0] = [1, np.nan, 1]  # rows 3 and 7 tie through equal coarse terms: the lower id first
    x = P.decode(codes, cb)
    q[0] = x[3]
    for k in (1, 4, 8):
        got = PR.search(q, codes, cb, labels, k_lists, probes, coarse, k)
        loop = search_loop(q, x, labels, k_lists, probes, coarse, k)
        assert np.array_equal(got[0], loop[0]) and np.array_equal(got[1], loop[1]) and not np.isnan(got[0]).any()
    s, i = PR.search(q, codes, cb, labels, k_lists, probes, coarse, 8)
    assert i[0, 0] == 3 and i[0, 1] == 7 and s[0, 0] == s[0, 1]
    coarse[0] = [0, np.nan, 1]  # ... and row 7 leads once its list's coarse term is the larger
    assert PR.search(q, codes, cb, labels, k_lists, probes, coarse, 2)[1][0].tolist() == [7, 3]
    # coarse 0 everywhere and distinct lists per row: the plain restatement
    probes = np.stack([rng.permutation(k_lists)[:3] for _ in range(nq)])
    zero = PR.search(q, codes, cb, labels, k_lists, probes, np.zeros((nq, 3), dtype=np.float32), 8)
    plain = P.search(q, codes, cb, labels, k_lists, probes, 8)
    assert np.array_equal(zero[0], plain[0]) and np.array_equal(zero[1], plain[1])


# ------------------------------------------------------------------------------------------------------- planted data
SCAN_TOL = (256 + 2) * 2.0 ** -23  # the scan tolerance (d + 2) * 2^-23 at d = 256


def planted_conditions(x, labels, c16, q, target, init, dsub, n_iter=4):
    """By the restatement alone: (plain quantisation error, residual quantisation error of the residuals, the number of
    queries whose planted neighbour is first in its list, the least gap to the runner-up of that list, the residual
    codebooks of every round).  Inside one list the coarse term is one constant: the order is the residual scores'."""
    plain = P.quantisation_error(x, P.train(x, init, dsub, n_iter)[-1])
    r = PR.residuals(x, labels, c16)
    books = PR.train(x, labels, c16, init, dsub, n_iter)
    codes = P.encode(r, books[-1])
    res = P.quantisation_error(r, books[-1], codes)
    decoded = P.decode(codes, books[-1])
    top_s, top_i = R.search(q, decoded, labels, len(c16), labels[target][:, None], 2, s=R.scores64(q, decoded))
    return plain, res, int((top_i[:, 0] == target).sum()), float((top_s[:, 0] - top_s[:, 1]).min()), books


@functools.lru_cache(maxsize=None)
def planted_data():
    """ivf_ref.planted(4096, 16, 256, 512, seed=1), the init the index really uses (clustering.init_rows, seed 0) and, as
    centroids, the fp16 normalised means of the planted clusters."""
    from sonar_amd.clustering import init_rows

    x, labels, _, q, target = R.planted(4096, 16, 256, 512, seed=1)
    means = np.stack([x[labels == c].astype(np.float64).sum(axis=0) for c in range(16)])
    return x, labels, R.normalize64(means).astype(np.float16), q, target, init_rows(len(x), 256, 0).numpy()


@pytest.mark.parametrize("dsub", [8, 16])
def test_planted_data_conditions_the_gpu_test_relies_on(dsub):
    x, labels, c16, q, target, init = planted_data()
    plain, res, first, gap, _ = planted_conditions(x, labels, c16, q, target, init, dsub)
    print(f"dsub {dsub}: quantisation error plain {plain:.4f}, residual {res:.4f}; planted row first {first} / 512, least gap {gap:.5f}")
    assert res < plain
    assert first == 512
    assert gap > SCAN_TOL


# ------------------------------------------------------------------------------------------------------- refusals
def test_python_refusals_need_no_device(monkeypatch):
    from sonar_amd import index
    from sonar_amd.index import IVFPQIndex, IVFPQResidualIndex

    f16, f32, i32, u8 = torch.float16, torch.float32, torch.int32, torch.uint8
    monkeypatch.setattr(index._lib, "load", boom)
    monkeypatch.setattr(index, "topk_normalized", boom)
    monkeypatch.setattr(index, "pair_scores", boom)
    monkeypatch.setattr(index, "normalize_rows", boom)
    x16, cb, c16, lab = fake(8, 64, dtype=f16), fake(8, 256, 8, dtype=f16), fake(3, 64, dtype=f16), fake(8, dtype=i32)
    init = fake(256, dtype=i32)
    calls = {
        "pq_residuals": lambda x=x16, l=lab, c=c16: index.pq_residuals(x, l, c),
        "pq_encode_residual": lambda x=x16, l=lab, c=c16: index.pq_encode_residual(x, l, c, cb),
        "pq_train_residual": lambda x=x16, l=lab, c=c16: index.pq_train_residual(x, l, c, 8, init, 2),
        "build_lists_pq_residual": lambda x=x16, l=lab, c=c16: index.build_lists_pq_residual(x, l, c, cb),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="contiguous fp16"):
            call(x=fake(8, 64))
        with pytest.raises(RuntimeError, match="HIP device only"):
            call(x=torch.zeros(8, 64, dtype=f16))
        with pytest.raises(ValueError, match="labels must be int32"):
            call(l=fake(8, dtype=torch.int64))
        with pytest.raises(ValueError, match="labels"):
            call(l=fake(9, dtype=i32))
        with pytest.raises(TypeError, match="labels"):
            call(l=[0] * 8)
        for bad in (fake(3, 64), fake(3, 128, dtype=f16), fake(3, 128, dtype=f16)[:, ::2]):
            with pytest.raises(ValueError, match=r"centroids must be a contiguous fp16 \[K, 64\]"):
                call(c=bad)
        with pytest.raises(TypeError, match="centroids"):
            call(c=None)
        with pytest.raises(RuntimeError, match="centroids: the index runs on a HIP device only"):
            call(c=torch.zeros(3, 64, dtype=f16))
        with pytest.raises(ValueError, match="centroids is empty"):
            call(c=fake(0, 64, dtype=f16))
    with pytest.raises(ValueError, match="codebooks cover dim"):
        index.pq_encode_residual(x16, lab, c16, fake(16, 256, 8, dtype=f16))
    with pytest.raises(ValueError, match="codebooks cover dim"):
        index.build_lists_pq_residual(x16, lab, c16, fake(16, 256, 8, dtype=f16))
    with pytest.raises(TypeError, match="codebooks"):
        index.build_lists_pq_residual(x16, lab, c16, None)
    with pytest.raises(ValueError, match="dsub = 7"):
        index.pq_train_residual(x16, lab, c16, 7, init)
    with pytest.raises(ValueError, match="n_iter"):
        index.pq_train_residual(x16, lab, c16, 8, init, n_iter=-1)
    with pytest.raises(ValueError, match="init must be int32"):
        index.pq_train_residual(x16, lab, c16, 8, fake(255, dtype=i32))
    # the search function
    args = (fake(16, dtype=i32), fake(4, dtype=i32))
    probes, coarse, codes = fake(8, 2, dtype=i32), fake(8, 2, dtype=f32), fake(16, 8, dtype=u8)
    with pytest.raises(ValueError, match=r"k = .*\[1, 8\]"):
        index.search_lists_pq_residual(x16, probes, coarse, codes, cb, *args, 9)
    for bad in (fake(9, 2, dtype=i32), fake(8, 9, dtype=i32), fake(8, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="probes"):
            index.search_lists_pq_residual(x16, bad, coarse, codes, cb, *args)
    for bad in (fake(8, 2, dtype=f16), fake(8, 3), fake(8), fake(7, 2)):
        with pytest.raises(ValueError, match=r"coarse must be fp32 \[8, 2\]"):
            index.search_lists_pq_residual(x16, probes, bad, codes, cb, *args)
    with pytest.raises(TypeError, match="coarse"):
        index.search_lists_pq_residual(x16, probes, None, codes, cb, *args)
    with pytest.raises(RuntimeError, match="coarse: the index runs on a HIP device only"):
        index.search_lists_pq_residual(x16, probes, torch.zeros(8, 2), codes, cb, *args)
    with pytest.raises(ValueError, match="codes must be contiguous uint8"):
        index.search_lists_pq_residual(x16, probes, coarse, fake(16, 64, dtype=torch.int8), cb, *args)
    with pytest.raises(ValueError, match="codebooks cover dim"):
        index.search_lists_pq_residual(x16, probes, coarse, codes, fake(16, 256, 8, dtype=f16), *args)

    # the index
    with pytest.raises(RuntimeError, match="HIP device only"):
        IVFPQResidualIndex.train(torch.zeros(300, 64), 3)
    with pytest.raises(ValueError, match="dsub = 5"):
        IVFPQResidualIndex.train(fake(300, 64), 3, dsub=5)
    with pytest.raises(ValueError, match="exceeds the 255 rows"):
        IVFPQResidualIndex.train(fake(255, 64), 3)
    monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=f16))
    with pytest.raises(ValueError, match="the product quantiser has dim 64, the centroids 128"):
        IVFPQResidualIndex(fake(3, 128), cb)
    ix = IVFPQResidualIndex(fake(3, 64), cb)
    assert isinstance(ix, IVFPQIndex) and ix.n_lists == 3 and ix.dim == 64 and ix.dsub == 8
    with pytest.raises(RuntimeError, match="before add"):
        ix.search(fake(5, 64))
    with pytest.raises(RuntimeError, match="before add"):
        ix.state_dict()
    with pytest.raises(TypeError, match="IVFPQResidualIndex holds product-quantiser codes of residuals"):
        ix.self_join()
    with pytest.raises(ValueError, match="dim 128"):
        ix.add(fake(8, 128))
    with pytest.raises(ValueError, match="labels must be int32"):
        ix.add(fake(8, 64), labels=fake(7, dtype=i32))
    ix._added = True
    with pytest.raises(RuntimeError, match="already called"):
        ix.add(fake(8, 64))
    monkeypatch.setattr(index, "normalize_rows", boom)  # everything below is refused before anything is normalised
    q = fake(5, 64)
    for bad in (0, 9, 1.0, True):
        with pytest.raises(ValueError, match=r"k = .*\[1, 8\]"):
            ix.search(q, k=bad)
        with pytest.raises(ValueError, match=r"nprobe = .*\[1, 8\]"):
            ix.search(q, nprobe=bad)
    with pytest.raises(ValueError, match="exceeds the 3 lists"):
        ix.search(q, nprobe=4)
    with pytest.raises(ValueError, match="dim 128"):
        ix.search(fake(5, 128))
    for bad in (fake(5, 2, dtype=torch.int64), fake(4, 2, dtype=i32), fake(5, 9, dtype=i32)):
        with pytest.raises(ValueError, match="probes"):
            ix.search(q, probes=bad)
    with pytest.raises(ValueError, match="coarse belongs to probes"):
        ix.search(q, coarse=fake(5, 1))
    for bad in (fake(5, 2, dtype=f16), fake(5, 3), fake(4, 2), fake(5)):
        with pytest.raises(ValueError, match=r"coarse must be fp32 \[5, 2\]"):
            ix.search(q, probes=fake(5, 2, dtype=i32), coarse=bad)
    with pytest.raises(TypeError, match="coarse"):
        ix.search(q, probes=fake(5, 2, dtype=i32), coarse=[[0.0, 0.0]] * 5)
    with pytest.raises(RuntimeError, match="coarse: the index runs on a HIP device only"):
        ix.search(q, probes=fake(5, 2, dtype=i32), coarse=torch.zeros(5, 2))
    with pytest.raises(TypeError):
        ix.search(q, refine=np.zeros((8, 64), dtype=np.float16))
    for bad in (fake(8, 64), fake(8, 128, dtype=f16), fake(8, dtype=f16), fake(8, 128, dtype=f16)[:, ::2]):
        with pytest.raises(ValueError, match="refine"):
            ix.search(q, refine=bad)


def test_plain_and_residual_state_dicts_do_not_load_into_each_other(monkeypatch):
    """A plain state keeps loading into IVFPQIndex as before; the marker `by_residual` tells a residual state apart, and
    neither class takes the other's."""
    from sonar_amd import index
    from sonar_amd.index import IVFPQIndex, IVFPQResidualIndex

    f16, i32, u8 = torch.float16, torch.int32, torch.uint8
    cb = fake(8, 256, 8, dtype=f16)
    # real (host) tensors behind the device stand-in: load_state_dict reads offsets[K] and copies
    dev = lambda t: t.as_subclass(FakeDevice)  # noqa: E731
    plain = {"centroids": dev(torch.zeros(3, 64, dtype=f16)), "offsets": dev(torch.tensor([0, 16, 16, 32], dtype=i32)),
             "sizes": dev(torch.tensor([5, 0, 7], dtype=i32)), "ids": dev(torch.zeros(32, dtype=i32)),
             "rows": dev(torch.zeros(32, 8, dtype=u8)), "codebooks": dev(torch.zeros(8, 256, 8, dtype=f16))}
    residual = {**plain, "by_residual": dev(torch.ones(1, dtype=u8))}
    monkeypatch.setattr(index._lib, "load", boom)
    monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=f16))
    loaded = IVFPQIndex.from_state_dict(plain)
    assert type(loaded) is IVFPQIndex and loaded.n_lists == 3 and loaded.dsub == 8 and loaded._added
    assert IVFPQIndex(fake(3, 64), cb).load_state_dict(plain)._added
    with pytest.raises(ValueError, match="IVFPQResidualIndex: its codes are residuals"):
        IVFPQIndex.from_state_dict(residual)
    with pytest.raises(ValueError, match="IVFPQResidualIndex: its codes are residuals"):
        IVFPQIndex(fake(3, 64), cb).load_state_dict(residual)
    loaded = IVFPQResidualIndex.from_state_dict(residual)
    assert type(loaded) is IVFPQResidualIndex and loaded.n_lists == 3 and loaded._added
    with pytest.raises(ValueError, match=r"lacks \['by_residual'\]"):
        IVFPQResidualIndex.from_state_dict(plain)
    with pytest.raises(ValueError, match=r"lacks \['by_residual'\]"):
        IVFPQResidualIndex(fake(3, 64), cb).load_state_dict(plain)
    with pytest.raises(ValueError, match=r"lacks \['codebooks'\]"):
        IVFPQResidualIndex.from_state_dict({k: v for k, v in residual.items() if k != "codebooks"})


def test_c_abi_refusals_without_a_device(lib):
    """The residual entries refuse what the plain ones refuse, with the same codes, plus null labels / coarse, null or
    misaligned centroids / out and K out of range; the workspaces are sized by the plain index's sizing functions."""
    tw, bw, sw = lib.smi_pq_train_workspace_bytes, lib.smi_ivf_pq_build_workspace_bytes, lib.smi_ivf_pq_search_workspace_bytes
    p = 0x1000  # never dereferenced: every call below is refused on its arguments
    big = 1 << 40
    cap = lib.smi_ivf_slots_bound(100, 7)
    Rs, E, T, B, S = (lib.smi_pq_residuals, lib.smi_pq_encode_residual, lib.smi_pq_train_residual, lib.smi_ivf_pq_build_residual,
                      lib.smi_ivf_pq_search_residual)
    INVALID, UNSUPPORTED = -1, -2
    cases = {
        # smi_pq_residuals(xn, labels, n, d, centroids, K, out, stream)
        "residuals d": (Rs(p, p, 100, 96, p, 7, p, None), UNSUPPORTED),
        "residuals n": (Rs(p, p, 0, 64, p, 7, p, None), INVALID),
        "residuals big n": (Rs(p, p, 1 << 31, 64, p, 7, p, None), UNSUPPORTED),
        "residuals K": (Rs(p, p, 100, 64, p, 0, p, None), INVALID),
        "residuals big K": (Rs(p, p, 100, 64, p, 1 << 31, p, None), UNSUPPORTED),
        "residuals null x": (Rs(None, p, 100, 64, p, 7, p, None), INVALID),
        "residuals null labels": (Rs(p, None, 100, 64, p, 7, p, None), INVALID),
        "residuals null centroids": (Rs(p, p, 100, 64, None, 7, p, None), INVALID),
        "residuals misaligned centroids": (Rs(p, p, 100, 64, p + 8, 7, p, None), INVALID),
        "residuals null out": (Rs(p, p, 100, 64, p, 7, None, None), INVALID),
        "residuals misaligned out": (Rs(p, p, 100, 64, p, 7, p + 2, None), INVALID),
        # smi_pq_encode_residual(xn, labels, n, d, centroids, K, dsub, codebooks, codes, stream)
        "encode d": (E(p, p, 100, 96, p, 7, 8, p, p, None), UNSUPPORTED),
        "encode dsub": (E(p, p, 100, 64, p, 7, 12, p, p, None), UNSUPPORTED),
        "encode dsub divides": (E(p, p, 100, 192, p, 7, 128, p, p, None), UNSUPPORTED),
        "encode n": (E(p, p, 0, 64, p, 7, 8, p, p, None), INVALID),
        "encode big n": (E(p, p, 1 << 31, 64, p, 7, 8, p, p, None), UNSUPPORTED),
        "encode K": (E(p, p, 100, 64, p, 0, 8, p, p, None), INVALID),
        "encode big K": (E(p, p, 100, 64, p, 1 << 31, 8, p, p, None), UNSUPPORTED),
        "encode null x": (E(None, p, 100, 64, p, 7, 8, p, p, None), INVALID),
        "encode null labels": (E(p, None, 100, 64, p, 7, 8, p, p, None), INVALID),
        "encode null centroids": (E(p, p, 100, 64, None, 7, 8, p, p, None), INVALID),
        "encode misaligned centroids": (E(p, p, 100, 64, p + 8, 7, 8, p, p, None), INVALID),
        "encode null codebooks": (E(p, p, 100, 64, p, 7, 8, None, p, None), INVALID),
        "encode misaligned codebooks": (E(p, p, 100, 64, p, 7, 8, p + 8, p, None), INVALID),
        "encode null codes": (E(p, p, 100, 64, p, 7, 8, p, None, None), INVALID),
        # smi_pq_train_residual(xn, labels, n, d, centroids, K, dsub, init, n_iter, codebooks, ws, ws_bytes, stream)
        "train d": (T(p, p, 1000, 96, p, 7, 8, p, 3, p, p, big, None), UNSUPPORTED),
        "train dsub": (T(p, p, 1000, 64, p, 7, 12, p, 3, p, p, big, None), UNSUPPORTED),
        "train n": (T(p, p, 0, 64, p, 7, 8, p, 3, p, p, big, None), INVALID),
        "train big n": (T(p, p, 1 << 31, 64, p, 7, 8, p, 3, p, p, big, None), UNSUPPORTED),
        "train big d": (T(p, p, 1000, 1 << 24, p, 7, 8, p, 3, p, p, big, None), UNSUPPORTED),
        "train K": (T(p, p, 1000, 64, p, 0, 8, p, 3, p, p, big, None), INVALID),
        "train big K": (T(p, p, 1000, 64, p, 1 << 31, 8, p, 3, p, p, big, None), UNSUPPORTED),
        "train n_iter": (T(p, p, 1000, 64, p, 7, 8, p, -1, p, p, big, None), INVALID),
        "train null x": (T(None, p, 1000, 64, p, 7, 8, p, 3, p, p, big, None), INVALID),
        "train null labels": (T(p, None, 1000, 64, p, 7, 8, p, 3, p, p, big, None), INVALID),
        "train null centroids": (T(p, p, 1000, 64, None, 7, 8, p, 3, p, p, big, None), INVALID),
        "train misaligned centroids": (T(p, p, 1000, 64, p + 4, 7, 8, p, 3, p, p, big, None), INVALID),
        "train null init": (T(p, p, 1000, 64, p, 7, 8, None, 3, p, p, big, None), INVALID),
        "train null codebooks": (T(p, p, 1000, 64, p, 7, 8, p, 3, None, p, big, None), INVALID),
        "train misaligned codebooks": (T(p, p, 1000, 64, p, 7, 8, p, 3, p + 4, p, big, None), INVALID),
        "train null ws": (T(p, p, 1000, 64, p, 7, 8, p, 3, p, None, big, None), INVALID),
        "train short ws": (T(p, p, 1000, 64, p, 7, 8, p, 3, p, p, tw(1000, 64, 8) - 1, None), INVALID),
        "train misaligned ws": (T(p, p, 1000, 64, p, 7, 8, p, 3, p, p + 8, big, None), INVALID),
        # smi_ivf_pq_build_residual(xn, labels, n, d, K, centroids, dsub, codebooks, codes, ids, cap, offsets, sizes, ws, ws_bytes, stream)
        "build d": (B(p, p, 100, 96, 7, p, 8, p, p, p, cap, p, p, p, big, None), UNSUPPORTED),
        "build dsub": (B(p, p, 100, 64, 7, p, 12, p, p, p, cap, p, p, p, big, None), UNSUPPORTED),
        "build dsub divides": (B(p, p, 100, 192, 7, p, 128, p, p, p, cap, p, p, p, big, None), UNSUPPORTED),
        "build K": (B(p, p, 100, 64, 0, p, 8, p, p, p, cap, p, p, p, big, None), INVALID),
        "build n": (B(p, p, 0, 64, 7, p, 8, p, p, p, cap, p, p, p, big, None), INVALID),
        "build big n": (B(p, p, 1 << 31, 64, 7, p, 8, p, p, p, big, p, p, p, big, None), UNSUPPORTED),
        "build big K": (B(p, p, 100, 64, 1 << 31, p, 8, p, p, p, big, p, p, p, big, None), UNSUPPORTED),
        "build big slots": (B(p, p, 1 << 30, 64, 1 << 30, p, 8, p, p, p, big, p, p, p, big, None), UNSUPPORTED),
        "build null x": (B(None, p, 100, 64, 7, p, 8, p, p, p, cap, p, p, p, big, None), INVALID),
        "build null labels": (B(p, None, 100, 64, 7, p, 8, p, p, p, cap, p, p, p, big, None), INVALID),
        "build null centroids": (B(p, p, 100, 64, 7, None, 8, p, p, p, cap, p, p, p, big, None), INVALID),
        "build misaligned centroids": (B(p, p, 100, 64, 7, p + 8, 8, p, p, p, cap, p, p, p, big, None), INVALID),
        "build null codebooks": (B(p, p, 100, 64, 7, p, 8, None, p, p, cap, p, p, p, big, None), INVALID),
        "build misaligned codebooks": (B(p, p, 100, 64, 7, p, 8, p + 8, p, p, cap, p, p, p, big, None), INVALID),
        "build null codes": (B(p, p, 100, 64, 7, p, 8, p, None, p, cap, p, p, p, big, None), INVALID),
        "build null ids": (B(p, p, 100, 64, 7, p, 8, p, p, None, cap, p, p, p, big, None), INVALID),
        "build null offsets": (B(p, p, 100, 64, 7, p, 8, p, p, p, cap, None, p, p, big, None), INVALID),
        "build null sizes": (B(p, p, 100, 64, 7, p, 8, p, p, p, cap, p, None, p, big, None), INVALID),
        "build small capacity": (B(p, p, 100, 64, 7, p, 8, p, p, p, cap - 1, p, p, p, big, None), INVALID),
        "build null ws": (B(p, p, 100, 64, 7, p, 8, p, p, p, cap, p, p, None, big, None), INVALID),
        "build short ws": (B(p, p, 100, 64, 7, p, 8, p, p, p, cap, p, p, p, bw(100, 7, 64, 8) - 1, None), INVALID),
        "build misaligned ws": (B(p, p, 100, 64, 7, p, 8, p, p, p, cap, p, p, p + 8, big, None), INVALID),
        # smi_ivf_pq_search_residual(qn, nq, d, probes, coarse, nprobe, codes, dsub, codebooks, ids, offsets, K, k, idx, score, ws, ws_bytes, stream)
        "search d": (S(p, 100, 96, p, p, 4, p, 8, p, p, p, 7, 5, p, p, p, big, None), UNSUPPORTED),
        "search dsub": (S(p, 100, 64, p, p, 4, p, 12, p, p, p, 7, 5, p, p, p, big, None), UNSUPPORTED),
        "search dsub divides": (S(p, 100, 192, p, p, 4, p, 128, p, p, p, 7, 5, p, p, p, big, None), UNSUPPORTED),
        "search K": (S(p, 100, 64, p, p, 4, p, 8, p, p, p, 0, 5, p, p, p, big, None), INVALID),
        "search big K": (S(p, 100, 64, p, p, 4, p, 8, p, p, p, 1 << 31, 5, p, p, p, big, None), UNSUPPORTED),
        "search nq": (S(p, 0, 64, p, p, 4, p, 8, p, p, p, 7, 5, p, p, p, big, None), INVALID),
        "search big nq": (S(p, 1 << 31, 64, p, p, 4, p, 8, p, p, p, 7, 5, p, p, p, big, None), UNSUPPORTED),
        "search big pairs": (S(p, 1 << 29, 64, p, p, 8, p, 8, p, p, p, 7, 5, p, p, p, big, None), UNSUPPORTED),
        "search k 0": (S(p, 100, 64, p, p, 4, p, 8, p, p, p, 7, 0, p, p, p, big, None), INVALID),
        "search k 9": (S(p, 100, 64, p, p, 4, p, 8, p, p, p, 7, 9, p, p, p, big, None), INVALID),
        "search nprobe 0": (S(p, 100, 64, p, p, 0, p, 8, p, p, p, 7, 5, p, p, p, big, None), INVALID),
        "search nprobe 9": (S(p, 100, 64, p, p, 9, p, 8, p, p, p, 7, 5, p, p, p, big, None), INVALID),
        "search null q": (S(None, 100, 64, p, p, 4, p, 8, p, p, p, 7, 5, p, p, p, big, None), INVALID),
        "search null probes": (S(p, 100, 64, None, p, 4, p, 8, p, p, p, 7, 5, p, p, p, big, None), INVALID),
        "search null coarse": (S(p, 100, 64, p, None, 4, p, 8, p, p, p, 7, 5, p, p, p, big, None), INVALID),
        "search null codes": (S(p, 100, 64, p, p, 4, None, 8, p, p, p, 7, 5, p, p, p, big, None), INVALID),
        "search null codebooks": (S(p, 100, 64, p, p, 4, p, 8, None, p, p, 7, 5, p, p, p, big, None), INVALID),
        "search misaligned codebooks": (S(p, 100, 64, p, p, 4, p, 8, p + 8, p, p, 7, 5, p, p, p, big, None), INVALID),
        "search null ids": (S(p, 100, 64, p, p, 4, p, 8, p, None, p, 7, 5, p, p, p, big, None), INVALID),
        "search null offsets": (S(p, 100, 64, p, p, 4, p, 8, p, p, None, 7, 5, p, p, p, big, None), INVALID),
        "search null idx": (S(p, 100, 64, p, p, 4, p, 8, p, p, p, 7, 5, None, p, p, big, None), INVALID),
        "search null score": (S(p, 100, 64, p, p, 4, p, 8, p, p, p, 7, 5, p, None, p, big, None), INVALID),
        "search null ws": (S(p, 100, 64, p, p, 4, p, 8, p, p, p, 7, 5, p, p, None, big, None), INVALID),
        "search short ws": (S(p, 100, 64, p, p, 4, p, 8, p, p, p, 7, 5, p, p, p, sw(100, 7, 4, 5, 64, 8) - 1, None), INVALID),
        "search misaligned ws": (S(p, 100, 64, p, p, 4, p, 8, p, p, p, 7, 5, p, p, p + 4, big, None), INVALID),
    }
    wrong = {k: v for k, v in cases.items() if v[0] != v[1]}
    assert not wrong, wrong
    assert Rs(p, p, 100, 64, p + 8, 7, p, None) == INVALID and b"centroids must be 16-byte aligned" in lib.smi_last_error()
    assert E(p, p, 100, 64, None, 7, 8, p, p, None) == INVALID and b"null centroids" in lib.smi_last_error()
    assert E(p, p, 100, 64, p, 7, 12, p, p, None) == UNSUPPORTED and b"dsub=12 must be 8, 16, 32 or 64" in lib.smi_last_error()
    assert T(p, p, 1000, 64, p, 7, 8, p, 3, p, p, 16, None) == INVALID and b"smi_pq_train_workspace_bytes" in lib.smi_last_error()
    assert B(p, p, 100, 64, 7, p, 8, p, p, p, cap - 1, p, p, p, big, None) == INVALID and b"smi_ivf_slots_bound" in lib.smi_last_error()
    assert S(p, 100, 64, p, p, 4, p, 8, p, p, p, 7, 5, p, p, p, 16, None) == INVALID
    assert b"smi_ivf_pq_search_workspace_bytes" in lib.smi_last_error()
