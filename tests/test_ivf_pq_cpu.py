"""CPU: the product quantiser and the IVF-PQ index.  The numpy restatement (tests/ivf_pq_ref.py) against
plain loops, exact rational and big-integer arithmetic; the planted-data conditions the GPU test relies on; and every refusal
of the Python layer and of the C entry points, none of which needs a device."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import ivf_pq_ref as P
from tests import ivf_ref as R
from tests.test_ivf_cpu import FakeDevice, boom, fake  # noqa: F401  (the stand-ins for device tensors)
from tests.test_ivf_i8_cpu import f32_round


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def F(v) -> Fraction:
    return Fraction(float(v))


def f16_round(v: Fraction) -> Fraction:
    """v rounded to the nearest fp16, ties to even, subnormals included (|v| < 65520)."""
    if v == 0:
        return Fraction(0)
    a = abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    ulp = Fraction(2) ** (max(e, -14) - 10)
    r = round(a / ulp) * ulp
    assert r < 65520
    return r if v > 0 else -r


# ------------------------------------------------------------------------------------------------------- the encoder
EXTREME = np.array([0.0, -0.0, 2.0 ** -24, -(2.0 ** -24), 1023 * 2.0 ** -24, 2.0 ** -14, 65504.0, -65504.0, 1.0, -1.0, 0.333, -3.14,
                    2049.0 * 2.0 ** -11, 1e-3, -7e-5, 12345.0], dtype=np.float16)


def test_a_product_of_two_fp16_is_exact_in_float32():
    """22 significant bits, magnitude 2^-48 .. 2^32: on subnormals, 65504 and mixed signs, and on random pairs."""
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 1 << 16, 4000).astype(np.uint16).view(np.float16)
    vals = np.concatenate([EXTREME, bits[np.isfinite(bits)]])
    a, b = vals[:, None].astype(np.float32), vals[None, :].astype(np.float32)
    prod = a * b
    assert prod.dtype == np.float32
    exact = vals[:, None].astype(np.float64) * vals[None, :].astype(np.float64)  # 22 bits: exact in float64 too
    assert np.array_equal(prod.astype(np.float64), exact)
    for x in EXTREME:
        for c in EXTREME:
            assert F(np.float32(x) * np.float32(c)) == F(x) * F(c)
    nz = np.abs(exact[exact != 0])
    assert nz.min() >= 2.0 ** -48 and nz.max() < 2.0 ** 32


def key_exact(x, c):
    """The contract's chain in exact rationals with one float32 rounding per step."""
    n2 = Fraction(0)
    for cj in c:
        n2 = f32_round(n2 + F(cj) * F(cj))
    key = -n2 / 2
    for xj, cj in zip(x, c):
        key = f32_round(key + F(xj) * F(cj))
    return key


def key_loop(x, c):
    """The chain as a plain float32 loop."""
    n2 = np.float32(0)
    for cj in c:
        n2 = np.float32(n2 + np.float32(cj) * np.float32(cj))
    key = np.float32(-0.5) * n2
    for xj, cj in zip(x, c):
        key = np.float32(key + np.float32(xj) * np.float32(cj))
    return key


@pytest.mark.parametrize("dsub", [8, 16, 64])
def test_restated_encoder_equals_a_plain_loop_and_exact_rational_arithmetic(dsub):
    rng = np.random.default_rng(dsub)
    d, n = 64, 6
    cb = P.random_codebooks(rng, d, dsub, scale=3.0)
    x = R.normalize64(rng.standard_normal((n, d))).astype(np.float16)
    # extreme patterns in rows and codewords: subnormals, the largest finite value, mixed signs
    x[0, :16], x[1, :16] = EXTREME, EXTREME[::-1]
    cb[0, 3, :8], cb[0, 4, :8], cb[0, 5, :8] = EXTREME[:8], EXTREME[8:], -EXTREME[:8]
    cb[:, 7] = 0
    key = P.keys(x, cb)
    m_all = d // dsub
    codes = P.encode(x, cb)
    assert codes.dtype == np.uint8 and codes.shape == (n, m_all)
    for r in range(n):
        for m in range(m_all):
            sub = x[r, m * dsub: (m + 1) * dsub]
            cands = list(range(0, 256, 37)) + [3, 4, 5, 7] if (r, m) != (0, 0) else range(256)
            for c in cands:
                want = key_exact(sub, cb[m, c])
                assert F(key[r, m, c]) == want == F(key_loop(sub, cb[m, c])), (r, m, c)
            loop = [key_loop(sub, cb[m, c]) for c in range(256)] if r < 2 else list(key[r, m])
            best = max(range(256), key=lambda c: (loop[c], -c))  # the largest key, ties to the lower code
            assert codes[r, m] == best
    # the largest key is the Euclidean nearest codeword (float64, away from ties)
    x64 = x.astype(np.float64).reshape(n, m_all, 1, dsub)
    dist = ((x64 - cb.astype(np.float64)[None]) ** 2).sum(axis=3)
    near = dist.argmin(axis=2)
    part = np.partition(dist, 1, axis=2)
    clear = part[:, :, 1] - part[:, :, 0] > 1e-3 * (1 + part[:, :, 0])
    assert clear.mean() > 0.5 and np.array_equal(near[clear], codes[clear])


def test_ties_go_to_the_lower_code():
    rng = np.random.default_rng(1)
    d, dsub = 64, 8
    cb = P.random_codebooks(rng, d, dsub, scale=2.0)
    x = R.normalize64(rng.standard_normal((5, d))).astype(np.float16)
    # duplicate codewords: the row's own subvector at codes 200 and 9 (and nowhere else)
    cb[0, 200], cb[0, 9] = x[0, :8], x[0, :8]
    cb[1, 255], cb[1, 254] = x[0, 8:16], x[0, 8:16]
    # x equidistant from two codewords: +-e_0 scaled against x with x_0 = 0 (keys equal bit for bit: the x_0 term adds +-0)
    cb[2] = 4.0  # far away
    cb[2, 17], cb[2, 130] = 0, 0
    cb[2, 17, 0], cb[2, 130, 0] = 0.5, -0.5
    x[1, 16] = 0
    x[1, 17:24] = 0.001
    # a zero row against a zero codeword and its duplicate
    x[2] = 0
    cb[3, 77], cb[3, 5] = 0, 0
    codes = P.encode(x, cb)
    assert codes[0, 0] == 9 and codes[0, 1] == 254
    key = P.keys(x[1:2], cb)[0, 2]
    assert key[17] == key[130] == key.max() and codes[1, 2] == 17
    assert codes[2, 3] == 5 and P.keys(x[2:3], cb)[0, 3, 5] == 0
    zero = P.encode(np.zeros((1, d), dtype=np.float16), np.zeros_like(cb))
    assert (zero == 0).all()  # every key ties at -0 / +0: code 0


# ------------------------------------------------------------------------------------------------------- training
def test_restated_training_round_equals_big_integer_sums():
    rng = np.random.default_rng(2)
    n, d, dsub = 300, 64, 16
    x = R.normalize64(rng.standard_normal((n, d))).astype(np.float16)
    x[:3, :4] = [[65504.0, -65504.0, 2.0 ** -24, -0.0]] * 3  # rows need not be normalised for the arithmetic to hold
    init = rng.permutation(n)[:256]
    cb0 = P.init_codebooks(x, init, dsub)
    for c in (0, 100, 255):
        assert np.array_equal(cb0[2, c], x[init[c], 32:48])
    cb1, codes = P.train_round(x, cb0)
    sums, counts = P.sums_counts(x, codes, dsub)
    m_all = d // dsub
    for m in range(m_all):
        for c in range(256):
            members = [r for r in range(n) if codes[r, m] == c]
            assert counts[m, c] == len(members)
            for j in range(dsub):
                big = sum(int(F(x[r, m * dsub + j]) * 2 ** 24) for r in members)  # Python integers
                assert int(sums[m, c, j]) == big
                if members:
                    want = f16_round(f32_round(f32_round(Fraction(big)) / len(members)) / 2 ** 24)
                    assert F(cb1[m, c, j]) == want, (m, c, j)
                else:
                    assert cb1[m, c, j].view(np.uint16) == cb0[m, c, j].view(np.uint16)
    assert counts.sum(axis=1).tolist() == [n] * m_all
    assert len(P.train(x, init, dsub, 2)) == 3 and np.array_equal(P.train(x, init, dsub, 2)[1].view(np.uint16), cb1.view(np.uint16))


def test_finalise_rounding_equals_exact_rational_arithmetic():
    """count in {1, 3, 7, 255} and sums float32 cannot hold: every conversion rounds to nearest even."""
    rng = np.random.default_rng(3)
    counts = np.array([1, 3, 7, 255] * 16, dtype=np.int64)
    sums = np.concatenate([rng.integers(-2 ** 24, 2 ** 24, 16), rng.integers(-2 ** 32, 2 ** 32, 16),
                           [2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 2 ** 25 + 2, 2 ** 25 + 6, 3 * 2 ** 23 + 1, 1, -1, 0, 255 * 2 ** 24,
                            255 * 2 ** 24 - 1, 2 ** 39 + 2 ** 15, 2 ** 39 + 3 * 2 ** 15, 7 * 2 ** 10 + 3, 2 ** 31 - 1, -(2 ** 33) + 5],
                           rng.integers(-2 ** 31, 2 ** 31, 16)]).astype(np.int64)
    prev = np.full((1, 64, 1), 9.0, dtype=np.float16)
    got = P.finalize(sums.reshape(1, 64, 1), counts.reshape(1, 64), prev)
    assert got.dtype == np.float16
    rounded = 0
    for s, c, g in zip(sums.tolist(), counts.tolist(), got.reshape(-1)):
        s32 = f32_round(Fraction(s))
        rounded += s32 != s
        assert F(np.float32(s)) == s32  # numpy's int64 -> float32 conversion is the correctly rounded one
        assert F(g) == f16_round(f32_round(s32 / c) / 2 ** 24), (s, c)
    assert rounded >= 16
    keep = P.finalize(np.array([[[5]]]), np.array([[0]]), prev[:, :1])
    assert keep[0, 0, 0] == 9.0


# ------------------------------------------------------------------------------------------------------- search
def search_loop(q16, x16, labels, k_lists, probes, k):
    out_s, out_i = [], []
    for r, row in enumerate(probes):
        cand = []
        for c in row:
            if 0 <= c < k_lists:
                for i in range(len(x16)):
                    if labels[i] == c:
                        s = float(sum(float(a) * float(b) for a, b in zip(q16[r], x16[i])))
                        cand.append((-s, i))
        cand.sort()
        cand = cand[:k] + [(np.inf, -1)] * (k - min(k, len(cand)))
        out_s.append([-s for s, _ in cand])
        out_i.append([i for _, i in cand])
    return np.array(out_s), np.array(out_i)


def test_restated_search_equals_a_plain_loop_and_the_flat_restatement_on_decoded_rows():
    rng = np.random.default_rng(4)
    n, d, dsub, k_lists, nq = 120, 64, 16, 5, 9
    cb = P.integer_codebooks(rng, d, dsub)
    codes = rng.integers(0, 256, (n, d // dsub)).astype(np.uint8)
    codes[7] = codes[3]  # a tie: the lower row first
    q = R.integer_rows(rng, nq, d)
    labels = rng.integers(-1, k_lists + 1, n)
    labels[7] = labels[3] = 2
    probes = rng.integers(-1, k_lists + 1, (nq, 3))
    probes[0] = [2, -1, 0]
    x = P.decode(codes, cb)
    q[0] = x[3]  # rows 3 and 7 are its two best, tied
    for r in (0, 7, 119):
        assert np.array_equal(x[r], np.concatenate([cb[m, codes[r, m]] for m in range(d // dsub)]))
    for k in (1, 4, 8):
        got = P.search(q, codes, cb, labels, k_lists, probes, k)
        flat = R.search(q, x, labels, k_lists, probes, k)
        loop = search_loop(q, x, labels, k_lists, probes, k)
        for a, b in zip(got, flat):
            assert np.array_equal(a, b)
        assert np.array_equal(got[0], loop[0]) and np.array_equal(got[1], loop[1])
    i = P.search(q, codes, cb, labels, k_lists, probes, 8)[1][0]
    assert list(i).index(3) + 1 == list(i).index(7)


def test_planted_data_conditions_the_gpu_test_relies_on():
    """ivf_ref.planted(4096, 16, 256, 512, seed=1), dsub = 8, four rounds, init seed 0: by the restatement alone the planted
    row is first among the rows of its list for every query, and the quantisation error falls below the initial one."""
    from sonar_amd.clustering import init_rows

    x, labels, _, q, target = R.planted(4096, 16, 256, 512, seed=1)
    init = init_rows(len(x), 256, 0).numpy()
    books = P.train(x, init, 8, 4)
    errs = []
    for cb in books:
        codes = P.encode(x, cb)
        errs.append(P.quantisation_error(x, cb, codes))
    print("quantisation error per round:", [round(e, 4) for e in errs])
    assert all(e < errs[0] for e in errs[1:])
    xd = P.decode(codes, books[-1])
    s = R.scores64(q, xd)
    top_s, top_i = R.search(q, xd, labels, 16, labels[target][:, None], 8, s=s)
    first = (top_i[:, 0] == target).sum()
    among = (top_i == target[:, None]).any(axis=1).sum()
    gap = (top_s[:, 0] - top_s[:, 1]).min()
    print(f"planted row first: {first} / 512, among the first 8: {among} / 512, least gap to the second {gap:.4f}")
    assert first == 512 and among == 512
    assert gap > 2 * 256 * 2.0 ** -23  # the fp32 accumulation of the scan cannot change the order (tests/test_gpu_ivf.py)


# ------------------------------------------------------------------------------------------------------- refusals
def test_python_refusals_need_no_device(monkeypatch):
    from sonar_amd import index
    from sonar_amd.index import IVFFlatIndex, IVFInt8Index, IVFPQIndex, ProductQuantizer

    f16, i32, u8 = torch.float16, torch.int32, torch.uint8
    assert index.PQ_CODEWORDS == P.CW and index.PQ_DSUBS == P.DSUBS
    monkeypatch.setattr(index._lib, "load", boom)
    monkeypatch.setattr(index, "topk_normalized", boom)
    monkeypatch.setattr(index, "pair_scores", boom)
    # codebooks
    with pytest.raises(TypeError):
        ProductQuantizer(np.zeros((8, 256, 8), dtype=np.float16))
    with pytest.raises(RuntimeError, match=r"HIP device only \(no CPU path\)"):
        ProductQuantizer(torch.zeros(8, 256, 8, dtype=f16))
    for bad in (fake(8, 256, 8), fake(8, 255, 8, dtype=f16), fake(8, 256, 12, dtype=f16), fake(8, 256, 128, dtype=f16),
                fake(256, 8, dtype=f16), fake(0, 256, 8, dtype=f16), fake(8, 256, 16, dtype=f16)[:, :, ::2]):
        with pytest.raises(ValueError, match="codebooks must be contiguous fp16"):
            ProductQuantizer(bad)
    with pytest.raises(ValueError, match="multiple of 64"):
        ProductQuantizer(fake(3, 256, 8, dtype=f16))
    with pytest.raises(ValueError, match=r"lacks \['codebooks'\]"):
        ProductQuantizer.from_state_dict({})
    pq = ProductQuantizer(fake(8, 256, 8, dtype=f16))
    assert (pq.dim, pq.dsub, pq.n_subquantizers) == (64, 8, 8) and set(pq.state_dict()) == {"codebooks"}
    # train
    with pytest.raises(RuntimeError, match="HIP device only"):
        ProductQuantizer.train(torch.zeros(300, 64))
    with pytest.raises(TypeError):
        ProductQuantizer.train(np.zeros((300, 64)))
    monkeypatch.setattr(index, "normalize_rows", boom)
    for dsub, what in ((12, "dsub = 12"), (True, "dsub = True"), (8.0, "dsub = 8.0"), (128, "dsub = 128")):
        with pytest.raises(ValueError, match=what):
            ProductQuantizer.train(fake(300, 64), dsub=dsub)
    with pytest.raises(ValueError, match="multiple of 64"):
        ProductQuantizer.train(fake(300, 96), dsub=32)
    for bad in (-1, 2.0, True):
        with pytest.raises(ValueError, match="n_iter"):
            ProductQuantizer.train(fake(300, 64), n_iter=bad)
    with pytest.raises(ValueError, match="exceeds the 255 rows"):
        ProductQuantizer.train(fake(255, 64))
    for bad in (torch.zeros(255, dtype=torch.int64), torch.zeros(256), [0] * 256, torch.zeros(256, 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="init must be an integer tensor of 256"):
            ProductQuantizer.train(fake(300, 64), init=bad)
    for bad in (torch.full((256,), 300), torch.full((256,), -1)):
        with pytest.raises(ValueError, match=r"outside \[0, 300\)"):
            ProductQuantizer.train(fake(300, 64), init=bad)
    # encode / decode and the functions
    with pytest.raises(ValueError, match="dim 128"):
        pq.encode(fake(5, 128))
    with pytest.raises(RuntimeError, match="HIP device only"):
        pq.encode(torch.zeros(5, 64))
    for bad in (fake(5, 8), fake(5, 9, dtype=u8), fake(5, dtype=u8), fake(0, 8, dtype=u8), fake(5, 16, dtype=u8)[:, ::2]):
        with pytest.raises(ValueError, match=r"codes must be contiguous uint8 \[rows, 8\]"):
            pq.decode(bad)
    with pytest.raises(RuntimeError, match="HIP device only"):
        pq.decode(torch.zeros(5, 8, dtype=u8))
    with pytest.raises(TypeError):
        pq.decode([[0] * 8])
    x16, cb = fake(8, 64, dtype=f16), fake(8, 256, 8, dtype=f16)
    with pytest.raises(ValueError, match="contiguous fp16"):
        index.pq_encode(fake(8, 64), cb)
    with pytest.raises(ValueError, match="the rows have 128"):
        index.pq_encode(fake(8, 128, dtype=f16), cb)
    for bad in (0, 9, True, 2.0):
        with pytest.raises(ValueError, match="n = "):
            index.pq_encode(x16, cb, bad)
    with pytest.raises(ValueError, match="init must be int32"):
        index.pq_train(x16, 8, fake(256, dtype=torch.int64))
    with pytest.raises(ValueError, match="init must be int32"):
        index.pq_train(x16, 8, fake(255, dtype=i32))
    with pytest.raises(ValueError, match="dsub = 7"):
        index.pq_train(x16, 7, fake(256, dtype=i32))
    with pytest.raises(ValueError, match="n_iter"):
        index.pq_train(x16, 8, fake(256, dtype=i32), n_iter=-1)
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError, match="n_lists"):
            index.build_lists_pq(x16, fake(8, dtype=i32), bad, cb)
    with pytest.raises(ValueError, match="9 labels for 8 rows"):
        index.build_lists_pq(x16, fake(9, dtype=i32), 3, cb)
    with pytest.raises(ValueError, match="labels must be int32"):
        index.build_lists_pq(x16, fake(8, dtype=torch.int64), 3, cb)
    with pytest.raises(ValueError, match="codebooks cover dim"):
        index.build_lists_pq(x16, fake(8, dtype=i32), 3, fake(16, 256, 8, dtype=f16))
    with pytest.raises(TypeError, match="codebooks"):
        index.build_lists_pq(x16, fake(8, dtype=i32), 3, None)
    args = (fake(16, dtype=i32), fake(4, dtype=i32))
    with pytest.raises(ValueError, match=r"k = .*\[1, 8\]"):
        index.search_lists_pq(x16, fake(8, 2, dtype=i32), fake(16, 8, dtype=u8), cb, *args, 9)
    with pytest.raises(ValueError, match="probes"):
        index.search_lists_pq(x16, fake(9, 2, dtype=i32), fake(16, 8, dtype=u8), cb, *args)
    with pytest.raises(ValueError, match="probes"):
        index.search_lists_pq(x16, fake(8, 9, dtype=i32), fake(16, 8, dtype=u8), cb, *args)
    with pytest.raises(ValueError, match="codes must be contiguous uint8"):
        index.search_lists_pq(x16, fake(8, 2, dtype=i32), fake(16, 64, dtype=torch.int8), cb, *args)
    with pytest.raises(ValueError, match="codebooks cover dim"):
        index.search_lists_pq(x16, fake(8, 2, dtype=i32), fake(16, 8, dtype=u8), fake(16, 256, 8, dtype=f16), *args)

    # the index
    monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=f16))
    with pytest.raises(ValueError, match="the product quantiser has dim 64, the centroids 128"):
        IVFPQIndex(fake(3, 128), pq)
    with pytest.raises(TypeError):
        IVFPQIndex(fake(3, 64), None)
    with pytest.raises(RuntimeError, match="HIP device only"):
        IVFPQIndex(torch.zeros(3, 64), pq)
    with pytest.raises(ValueError, match="dsub = 5"):
        IVFPQIndex.train(fake(300, 64), 3, dsub=5)
    ix = IVFPQIndex(fake(3, 64), cb)
    assert ix.n_lists == 3 and ix.dim == 64 and ix.dsub == 8 and tuple(ix.codebooks.shape) == (8, 256, 8)
    for what in ("list_sizes", "list_offsets", "ntotal", "state_dict"):
        with pytest.raises(RuntimeError, match="before add"):
            v = getattr(ix, what)
            v() if callable(v) else None
    with pytest.raises(RuntimeError, match="before add"):
        ix.search(fake(5, 64))
    with pytest.raises(TypeError, match="IVFPQIndex holds product-quantiser codes"):
        ix.self_join()
    with pytest.raises(ValueError, match="dim 128"):
        ix.add(fake(8, 128))
    for bad in (fake(8, dtype=torch.int64), fake(7, dtype=i32)):
        with pytest.raises(ValueError, match="labels must be int32"):
            ix.add(fake(8, 64), labels=bad)
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
    with pytest.raises(ValueError, match="dim 128"):
        ix.search(fake(5, 128))
    for bad in (fake(5, 2, dtype=torch.int64), fake(4, 2, dtype=i32), fake(5, 9, dtype=i32)):
        with pytest.raises(ValueError, match="probes"):
            ix.search(q, probes=bad)
    monkeypatch.setattr(index, "normalize_rows", boom)  # refine: refused before anything is normalised or searched
    with pytest.raises(TypeError):
        ix.search(q, refine=np.zeros((8, 64), dtype=np.float16))
    for bad in (fake(8, 64), fake(8, 128, dtype=f16), fake(8, dtype=f16), fake(8, 128, dtype=f16)[:, ::2]):
        with pytest.raises(ValueError, match="refine"):
            ix.search(q, refine=bad)
    # load_state_dict
    state = {"centroids": fake(3, 64, dtype=f16), "offsets": fake(4, dtype=i32), "sizes": fake(3, dtype=i32),
             "ids": fake(16, dtype=i32), "rows": fake(16, 8, dtype=u8), "codebooks": cb}
    with pytest.raises(ValueError, match=r"lacks \['codebooks'\]"):
        ix.load_state_dict({k: v for k, v in state.items() if k != "codebooks"})
    for key, bad, what in (("centroids", fake(4, 64, dtype=f16), "this index has"),
                           ("ids", fake(15, dtype=i32), "ids must be int32"),
                           ("rows", fake(16, 64, dtype=u8), r"rows must be uint8 \[slots, 8\]"),
                           ("rows", fake(16, 8, dtype=torch.int8), "rows must be uint8"),
                           ("codebooks", fake(16, 256, 8, dtype=f16), "codebooks cover dim"),
                           ("codebooks", fake(8, 256, 8), "codebooks must be contiguous fp16")):
        with pytest.raises((ValueError, RuntimeError), match=what):
            ix.load_state_dict({**state, key: bad})
    # what the two existing classes accept and refuse is what it was
    monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=f16))
    flat_state = {**{k: v for k, v in state.items() if k != "codebooks"}, "rows": fake(16, 64, dtype=f16)}
    with pytest.raises(ValueError, match=r"rows must be fp16 \[slots, 64\]"):
        IVFFlatIndex(fake(3, 64)).load_state_dict({**flat_state, "rows": fake(16, 8, dtype=f16)})
    with pytest.raises(ValueError, match=r"rows must be int8 \[slots, 64\]"):
        IVFInt8Index(fake(3, 64)).load_state_dict({**flat_state, "rows": fake(16, 64, dtype=f16), "scales": fake(16)})


def test_c_abi_sizing_and_refusals_without_a_device(lib):
    sb = lib.smi_ivf_slots_bound
    tw, bw, sw = lib.smi_pq_train_workspace_bytes, lib.smi_ivf_pq_build_workspace_bytes, lib.smi_ivf_pq_search_workspace_bytes
    # training: codes [n, M] | sums int64 [256 d] | counts int32 [256 M]
    assert tw(1000, 64, 8) == 8000 + 256 * 64 * 8 + 256 * 8 * 4
    assert tw(3, 1024, 64) == 48 + 256 * 1024 * 8 + 256 * 16 * 4 and tw(300, 192, 16) % 16 == 0
    for bad in ((0, 64, 8), (1000, 96, 8), (1000, 64, 12), (1000, 64, 128), (1000, 192, 128), (1000, 64, 0), (1 << 31, 64, 8),
                (1000, 0, 8), (1000, 1 << 24, 8)):
        assert tw(*bad) == 0, bad
    assert bw(1000, 7, 1024, 16) == lib.smi_ivf_build_workspace_bytes(1000, 7, 1024) == 32
    for bad in ((1000, 7, 96, 8), (1000, 0, 64, 8), (0, 7, 64, 8), (1 << 31, 7, 64, 8), (1 << 30, 1 << 30, 64, 8), (1000, 7, 64, 12),
                (1000, 7, 64, 128), (1000, 7, 64, 4)):
        assert bw(*bad) == 0, bad
    assert sw(100, 7, 4, 5, 64, 8) == lib.smi_ivf_search_workspace_bytes(100, 7, 4, 5, 64)
    assert sw(100, 7, 4, 5, 192, 64) > 0 and sw(100, 7, 4, 5, 1024, 32) > 0
    for bad in ((0, 7, 4, 5, 64, 8), (100, 0, 4, 5, 64, 8), (100, 7, 0, 5, 64, 8), (100, 7, 9, 5, 64, 8), (100, 7, 4, 0, 64, 8),
                (100, 7, 4, 9, 64, 8), (100, 7, 4, 5, 96, 8), (1 << 31, 7, 1, 1, 64, 8), (100, 1 << 31, 1, 1, 64, 8),
                (1 << 29, 7, 8, 1, 64, 8), (100, 7, 4, 5, 64, 12), (100, 7, 4, 5, 64, 128), (100, 7, 4, 5, 192, 128)):
        assert sw(*bad) == 0, bad
    p = 0x1000  # never dereferenced: every call below is refused on its arguments
    big = 1 << 40
    cap = sb(100, 7)
    E, D, T, B, S = lib.smi_pq_encode, lib.smi_pq_decode, lib.smi_pq_train, lib.smi_ivf_pq_build, lib.smi_ivf_pq_search
    cases = {
        "encode d": E(p, 100, 96, 8, p, p, None),
        "encode dsub": E(p, 100, 64, 12, p, p, None),
        "encode dsub divides": E(p, 100, 192, 128, p, p, None),
        "encode n": E(p, 0, 64, 8, p, p, None),
        "encode big n": E(p, 1 << 31, 64, 8, p, p, None),
        "encode null x": E(None, 100, 64, 8, p, p, None),
        "encode null codebooks": E(p, 100, 64, 8, None, p, None),
        "encode misaligned codebooks": E(p, 100, 64, 8, p + 8, p, None),
        "encode null codes": E(p, 100, 64, 8, p, None, None),
        "decode d": D(p, 100, 96, 8, p, p, None),
        "decode dsub": D(p, 100, 64, 24, p, p, None),
        "decode n": D(p, 0, 64, 8, p, p, None),
        "decode null codes": D(None, 100, 64, 8, p, p, None),
        "decode null codebooks": D(p, 100, 64, 8, None, p, None),
        "decode misaligned codebooks": D(p, 100, 64, 8, p + 2, p, None),
        "decode null rows": D(p, 100, 64, 8, p, None, None),
        "decode misaligned rows": D(p, 100, 64, 8, p, p + 8, None),
        "train d": T(p, 1000, 96, 8, p, 3, p, p, big, None),
        "train dsub": T(p, 1000, 64, 12, p, 3, p, p, big, None),
        "train n": T(p, 0, 64, 8, p, 3, p, p, big, None),
        "train big n": T(p, 1 << 31, 64, 8, p, 3, p, p, big, None),
        "train big d": T(p, 1000, 1 << 24, 8, p, 3, p, p, big, None),
        "train n_iter": T(p, 1000, 64, 8, p, -1, p, p, big, None),
        "train null x": T(None, 1000, 64, 8, p, 3, p, p, big, None),
        "train null init": T(p, 1000, 64, 8, None, 3, p, p, big, None),
        "train null codebooks": T(p, 1000, 64, 8, p, 3, None, p, big, None),
        "train misaligned codebooks": T(p, 1000, 64, 8, p, 3, p + 4, p, big, None),
        "train null ws": T(p, 1000, 64, 8, p, 3, p, None, big, None),
        "train short ws": T(p, 1000, 64, 8, p, 3, p, p, tw(1000, 64, 8) - 1, None),
        "train misaligned ws": T(p, 1000, 64, 8, p, 3, p, p + 8, big, None),
        "build d": B(p, p, 100, 96, 7, 8, p, p, p, cap, p, p, p, big, None),
        "build dsub": B(p, p, 100, 64, 7, 12, p, p, p, cap, p, p, p, big, None),
        "build dsub divides": B(p, p, 100, 192, 7, 128, p, p, p, cap, p, p, p, big, None),
        "build K": B(p, p, 100, 64, 0, 8, p, p, p, cap, p, p, p, big, None),
        "build n": B(p, p, 0, 64, 7, 8, p, p, p, cap, p, p, p, big, None),
        "build big n": B(p, p, 1 << 31, 64, 7, 8, p, p, p, big, p, p, p, big, None),
        "build big K": B(p, p, 100, 64, 1 << 31, 8, p, p, p, big, p, p, p, big, None),
        "build big slots": B(p, p, 1 << 30, 64, 1 << 30, 8, p, p, p, big, p, p, p, big, None),
        "build null x": B(None, p, 100, 64, 7, 8, p, p, p, cap, p, p, p, big, None),
        "build null labels": B(p, None, 100, 64, 7, 8, p, p, p, cap, p, p, p, big, None),
        "build null codebooks": B(p, p, 100, 64, 7, 8, None, p, p, cap, p, p, p, big, None),
        "build misaligned codebooks": B(p, p, 100, 64, 7, 8, p + 8, p, p, cap, p, p, p, big, None),
        "build null codes": B(p, p, 100, 64, 7, 8, p, None, p, cap, p, p, p, big, None),
        "build null ids": B(p, p, 100, 64, 7, 8, p, p, None, cap, p, p, p, big, None),
        "build null offsets": B(p, p, 100, 64, 7, 8, p, p, p, cap, None, p, p, big, None),
        "build null sizes": B(p, p, 100, 64, 7, 8, p, p, p, cap, p, None, p, big, None),
        "build small capacity": B(p, p, 100, 64, 7, 8, p, p, p, cap - 1, p, p, p, big, None),
        "build null ws": B(p, p, 100, 64, 7, 8, p, p, p, cap, p, p, None, big, None),
        "build short ws": B(p, p, 100, 64, 7, 8, p, p, p, cap, p, p, p, bw(100, 7, 64, 8) - 1, None),
        "build misaligned ws": B(p, p, 100, 64, 7, 8, p, p, p, cap, p, p, p + 8, big, None),
        "search d": S(p, 100, 96, p, 4, p, 8, p, p, p, 7, 5, p, p, p, big, None),
        "search dsub": S(p, 100, 64, p, 4, p, 12, p, p, p, 7, 5, p, p, p, big, None),
        "search dsub divides": S(p, 100, 192, p, 4, p, 128, p, p, p, 7, 5, p, p, p, big, None),
        "search K": S(p, 100, 64, p, 4, p, 8, p, p, p, 0, 5, p, p, p, big, None),
        "search nq": S(p, 0, 64, p, 4, p, 8, p, p, p, 7, 5, p, p, p, big, None),
        "search big nq": S(p, 1 << 31, 64, p, 4, p, 8, p, p, p, 7, 5, p, p, p, big, None),
        "search big pairs": S(p, 1 << 29, 64, p, 8, p, 8, p, p, p, 7, 5, p, p, p, big, None),
        "search k 0": S(p, 100, 64, p, 4, p, 8, p, p, p, 7, 0, p, p, p, big, None),
        "search k 9": S(p, 100, 64, p, 4, p, 8, p, p, p, 7, 9, p, p, p, big, None),
        "search nprobe 0": S(p, 100, 64, p, 0, p, 8, p, p, p, 7, 5, p, p, p, big, None),
        "search nprobe 9": S(p, 100, 64, p, 9, p, 8, p, p, p, 7, 5, p, p, p, big, None),
        "search null q": S(None, 100, 64, p, 4, p, 8, p, p, p, 7, 5, p, p, p, big, None),
        "search null probes": S(p, 100, 64, None, 4, p, 8, p, p, p, 7, 5, p, p, p, big, None),
        "search null codes": S(p, 100, 64, p, 4, None, 8, p, p, p, 7, 5, p, p, p, big, None),
        "search null codebooks": S(p, 100, 64, p, 4, p, 8, None, p, p, 7, 5, p, p, p, big, None),
        "search misaligned codebooks": S(p, 100, 64, p, 4, p, 8, p + 8, p, p, 7, 5, p, p, p, big, None),
        "search null ids": S(p, 100, 64, p, 4, p, 8, p, None, p, 7, 5, p, p, p, big, None),
        "search null offsets": S(p, 100, 64, p, 4, p, 8, p, p, None, 7, 5, p, p, p, big, None),
        "search null idx": S(p, 100, 64, p, 4, p, 8, p, p, p, 7, 5, None, p, p, big, None),
        "search null score": S(p, 100, 64, p, 4, p, 8, p, p, p, 7, 5, p, None, p, big, None),
        "search null ws": S(p, 100, 64, p, 4, p, 8, p, p, p, 7, 5, p, p, None, big, None),
        "search short ws": S(p, 100, 64, p, 4, p, 8, p, p, p, 7, 5, p, p, p, sw(100, 7, 4, 5, 64, 8) - 1, None),
        "search misaligned ws": S(p, 100, 64, p, 4, p, 8, p, p, p, 7, 5, p, p, p + 4, big, None),
    }
    assert all(rc != 0 for rc in cases.values()), {k: v for k, v in cases.items() if v == 0}
    for what in ("encode", "decode", "train", "build", "search"):
        assert cases[f"{what} dsub"] == -2 and cases[f"{what} d"] == -2, what
        assert cases[f"{what} null codebooks"] == -1, what
    assert cases["encode dsub divides"] == cases["build dsub divides"] == cases["search dsub divides"] == -2
    assert E(p, 100, 64, 12, p, p, None) == -2 and b"dsub=12 must be 8, 16, 32 or 64" in lib.smi_last_error()
    assert E(p, 100, 192, 128, p, p, None) == -2 and b"dsub" in lib.smi_last_error()
    assert S(p, 100, 64, p, 4, p, 8, p + 8, p, p, 7, 5, p, p, p, big, None) == -1 and b"codebooks must be 16-byte aligned" in lib.smi_last_error()
    assert B(p, p, 100, 64, 7, 8, p, p, p, cap - 1, p, p, p, big, None) == -1 and b"smi_ivf_slots_bound" in lib.smi_last_error()
    assert S(p, 100, 64, p, 4, p, 8, p, p, p, 7, 5, p, p, p, 16, None) == -1
    assert b"smi_ivf_pq_search_workspace_bytes" in lib.smi_last_error()
    assert T(p, 1000, 64, 8, p, 3, p, p, 16, None) == -1 and b"smi_pq_train_workspace_bytes" in lib.smi_last_error()
    assert T(p, 1000, 64, 8, p, -1, p, p, big, None) == -1 and b"n_iter" in lib.smi_last_error()
