"""CPU: the int8 scalar-quantised IVF index -- the numpy restatement (tests/ivf_i8_ref.py) against exact rational arithmetic
and against a plain loop, the derived error bound and the planted-data conditions the GPU tests rely on, and every refusal
of the Python layer and of the C-ABI (sonar_amd/index.py, sonar_amd/csrc/ivf.hip).  Nothing here needs a device."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import ivf_i8_ref as Q
from tests import ivf_ref as R
from tests import kmeans_ref as KR
from tests.test_ivf_cpu import FakeDevice, boom, fake  # noqa: F401  (the stand-ins for device tensors)

INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


# ------------------------------------------------------------------------------------------------------- the encoder
def f32_round(v: Fraction) -> Fraction:
    """v rounded to the nearest float32, ties to even, as an exact Fraction (normal range only)."""
    if v == 0:
        return Fraction(0)
    a = abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and -126 <= e <= 127
    ulp = Fraction(2) ** (e - 23)
    r = round(a / ulp) * ulp  # Python rounds a Fraction's exact half to the even integer
    return r if v > 0 else -r


def encode_exact(row16):
    x = [Fraction(float(v)) for v in row16]
    amax = max(abs(v) for v in x)
    if amax == 0:
        return [0] * len(x), Fraction(0)
    inv, scale = f32_round(Fraction(127) / amax), f32_round(amax / 127)
    return [max(-127, min(127, round(f32_round(v * inv)))) for v in x], scale


def test_f32_round_is_numpys_float32():
    rng = np.random.default_rng(0)
    for a, b in zip(rng.standard_normal(200), rng.standard_normal(200)):
        a32, b32 = np.float32(a), np.float32(b)
        for got, want in ((f32_round(Fraction(float(a32)) / Fraction(float(b32))), a32 / b32),
                          (f32_round(Fraction(float(a32)) * Fraction(float(b32))), a32 * b32)):
            assert got == Fraction(float(want))
    assert f32_round(Fraction(2 ** 24 + 1)) == 2 ** 24 and f32_round(Fraction(2 ** 24 + 3)) == 2 ** 24 + 4  # ties to even


@pytest.mark.parametrize("d", [64, 192])
def test_restated_encoder_equals_exact_rational_arithmetic(d):
    rng = np.random.default_rng(d)
    x = np.concatenate([Q.edge_rows(rng, d), R.normalize64(rng.standard_normal((20, d))).astype(np.float16),
                        (rng.standard_normal((10, d)) * 10.0 ** rng.integers(-6, 4, (10, 1))).astype(np.float16)])
    codes, scales = Q.encode(x)
    assert codes.dtype == np.int8 and scales.dtype == np.float32
    for r in range(len(x)):
        want_c, want_s = encode_exact(x[r])
        assert codes[r].tolist() == want_c, r
        assert Fraction(float(scales[r])) == want_s, r
    assert not codes[0].any() and scales[0] == 0  # the zero row
    assert np.count_nonzero(codes[1]) == 1 and codes[1, d // 3] == -127  # one-hot
    assert set(np.abs(codes[2]).tolist()) == {127}  # +-amax only
    assert np.abs(codes).max() == 127 and codes.min() == -127  # -128 is never a code


def test_exact_half_ties_go_to_the_even_code():
    x = Q.half_tie_rows(1024)
    codes, scales = Q.encode(x)
    m = (np.arange(1024) % 254) - 127
    want = np.where(m % 2 == 0, m, m + 1)  # rint(m + 1/2): the even one of m, m + 1
    assert np.float32(127) / np.float32(127 * 2.0 ** -7) == 128
    for row, top in ((0, 127), (1, -127)):
        assert codes[row, 0] == top and np.array_equal(codes[row, 1:], want[1:])
    assert (codes[0, 1:] % 2 == 0).all() and scales[0] == scales[1] == np.float32(2.0 ** -7)


# ------------------------------------------------------------------------------------------------------- the search
def search_loop(q16, x16, labels, k_lists, probes, k):
    """`Q.search` as a plain loop: Python integers for the sums, one float32 operation at a time for the score."""
    (cq, sq), (cx, sx) = Q.encode(q16), Q.encode(x16)
    out_s, out_i = [], []
    for r, row in enumerate(probes):
        cand = []
        for c in row:
            if 0 <= c < k_lists:
                for i in range(len(x16)):
                    if labels[i] == c:
                        acc = sum(int(a) * int(b) for a, b in zip(cq[r], cx[i]))
                        cand.append((-float(np.float32(np.float32(np.float32(acc) * sx[i]) * sq[r])), i))
        cand = sorted(cand)[:k]
        out_s.append([-s for s, _ in cand] + [-np.inf] * (k - len(cand)))
        out_i.append([i for _, i in cand] + [-1] * (k - len(cand)))
    return np.array(out_s), np.array(out_i, dtype=np.int64)


def test_restated_search_equals_a_plain_loop():
    rng = np.random.default_rng(3)
    x = R.normalize64(rng.standard_normal((60, 64))).astype(np.float16)
    q = R.normalize64(rng.standard_normal((6, 64))).astype(np.float16)
    x[7], x[31], x[50] = q[0], q[0], q[0]  # exact ties across lists: by id
    x[9] = 0
    labels = rng.integers(0, 5, 60)
    labels[:3] = [-1, 5, INT32_MAX]
    labels[labels == 4] = 3  # list 4 is empty
    probes = np.array([[0, 1, 2, 3], [4, -1, 9, 4], [2, 2, -1, 5], [3, 1, 4, 0], [1, 0, 3, 2], [4, 3, -1, -1]])
    for k in (1, 3, 8):
        got, want = Q.search(q, x, labels, 5, probes, k), search_loop(q, x, labels, 5, probes, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), k
    s, i = Q.search(q, x, labels, 5, probes, 8)
    assert i[0][:3].tolist() == [7, 31, 50] and len(set(s[0][:3].tolist())) == 1
    assert (i[1] == -1).all() and np.isneginf(s[1]).all()
    assert np.array_equal(i[2][0::2], i[2][1::2])  # a list named twice contributes twice


def test_largest_sums_and_a_conversion_that_rounds():
    """Saturated rows: |acc| = 127^2 d, the largest there is at a d.  With mixed signs acc = 127^2 (d - 2 m), an even number
    below 2^25 at d = 2048, which float32 holds exactly; one element at half of amax (code 64: 63.5 ties to even) makes acc
    odd and above 2^24, so float32(acc) rounds and the restatement must round it to nearest even."""
    d = 2048
    x = np.full((3, d), 0.5, dtype=np.float16)
    x[1:, :257] *= -1
    x[2, -1] = 0.25
    codes = Q.encode(x)[0]
    assert codes[2, -1] == 64 and set(np.abs(codes[:2]).ravel().tolist()) == {127}
    acc = Q.int_dots(codes, codes)
    assert acc[0, 0] == 127 * 127 * d and acc[0, 1] == 127 * 127 * 1534 == int(np.float32(acc[0, 1]))
    assert acc[0, 2] == 127 * (127 * 1533 + 64) > 2 ** 24 and acc[0, 2] % 2 == 1
    assert abs(int(np.float32(acc[0, 2])) - int(acc[0, 2])) == 1  # the conversion rounds
    top = Q.encode(np.full((1, Q.MAX_DIM), 1.0, dtype=np.float16))[0]
    assert Q.int_dots(top, top)[0, 0] == 127 * 127 * Q.MAX_DIM < 2 ** 31


# ------------------------------------------------------------------------------------------------------- planted data
@pytest.mark.parametrize("d", [64, 1024])
def test_error_bound_and_planted_neighbours_on_the_shapes_of_the_gpu_test(d):
    """tests/test_gpu_ivf_i8.py's generator through the restatement alone: every score of every (query, row) pair lies within
    the derived bound of the float64 dot product; k-means recovers the planted lists and every query's nearest list is its
    target's; and at nprobe = 1 the planted neighbour comes first by a gap the bounds of the two rows cannot close."""
    n, k, nq = 4099, 16, 257
    x, truth, _, q, target = R.planted(n, k, d, nq)
    (cq, sq), (cx, sx) = Q.encode(q), Q.encode(x)
    s = Q.scores_from_codes(cq, sq, cx, sx)
    s64 = q.astype(np.float64) @ x.astype(np.float64).T
    b = Q.bound(Q.l1(cq)[:, None], sq[:, None], Q.l1(cx)[None, :], sx[None, :], d, s)
    err = np.abs(s.astype(np.float64) - s64)
    assert (err <= b).all(), (err / b).max()
    rounds = KR.fit(x, x[:k].copy(), 2)
    assert np.array_equal(rounds[-1]["labels"], truth)
    probe, _, margin = KR.assign(q, KR.normalize64(rounds[-1]["centroids"]))
    assert np.array_equal(probe, truth[target]) and margin.min() >= 0.1, margin.min()
    top_s, top_i = Q.search(q, x, truth, k, probe[:, None], 4, s=s)
    assert np.array_equal(top_i[:, 0], target)
    gap = (top_s[:, 0] - top_s[:, 1]).min()
    assert gap > 2 * b.max(), (gap, b.max())  # in float64 too the neighbour is first: the two rows' bounds cannot close it


# ------------------------------------------------------------------------------------------------------- refusals
def test_python_refusals_need_no_device(monkeypatch):
    from sonar_amd import index
    from sonar_amd.clustering import SphericalKMeans
    from sonar_amd.index import IVFFlatIndex, IVFInt8Index

    assert index.INT8_MAX_DIM == Q.MAX_DIM
    with pytest.raises(RuntimeError, match="before fit"):
        IVFInt8Index(SphericalKMeans(3))
    with pytest.raises(TypeError):
        IVFInt8Index(np.zeros((3, 64)))
    with pytest.raises(RuntimeError, match=r"HIP device only \(no CPU path\)"):
        IVFInt8Index(torch.zeros(3, 64))
    with pytest.raises(RuntimeError, match=r"HIP device only"):
        IVFInt8Index.train(torch.zeros(8, 64), 3)

    monkeypatch.setattr(index, "normalize_rows", lambda t: fake((t.shape[0] + 255) // 256 * 256, t.shape[1], dtype=torch.float16))
    monkeypatch.setattr(index, "topk_normalized", boom)
    monkeypatch.setattr(index, "pair_scores", boom)
    for shape, what in (((3,), r"\[rows, dim\]"), ((3, 96), "multiple of 64"), ((0, 64), "empty"),
                        ((3, Q.MAX_DIM + 64), "could overflow")):
        with pytest.raises(ValueError, match=what):
            IVFInt8Index(fake(*shape))
    IVFFlatIndex(fake(3, Q.MAX_DIM + 64))  # the flat index has no such limit
    assert IVFInt8Index(fake(3, Q.MAX_DIM)).dim == Q.MAX_DIM
    ix = IVFInt8Index(fake(3, 64))
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
    with pytest.raises(ValueError, match="empty"):
        ix.add(fake(0, 64))
    for bad in (fake(8, dtype=torch.int64), fake(7, dtype=torch.int32), fake(8, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="labels must be int32"):
            ix.add(fake(8, 64), labels=bad)
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
    with pytest.raises(TypeError):
        ix.search(q, probes=[[0]] * 5)
    for bad in (fake(5, 2, dtype=torch.int64), fake(4, 2, dtype=torch.int32), fake(5, 9, dtype=torch.int32)):
        with pytest.raises(ValueError, match="probes"):
            ix.search(q, probes=bad)
    # refine: refused before anything is normalised or searched
    monkeypatch.setattr(index, "normalize_rows", boom)
    with pytest.raises(TypeError):
        ix.search(q, refine=np.zeros((8, 64), dtype=np.float16))
    with pytest.raises(RuntimeError, match="HIP device only"):
        ix.search(q, refine=torch.zeros(8, 64, dtype=torch.float16))
    for bad in (fake(8, 64), fake(8, 128, dtype=torch.float16), fake(8, dtype=torch.float16),
                fake(8, 128, dtype=torch.float16)[:, ::2]):
        with pytest.raises(ValueError, match="refine"):
            ix.search(q, refine=bad)
    # the functions
    x16 = fake(8, 64, dtype=torch.float16)
    for fn in (index.encode_rows_int8, lambda t: index.build_lists_int8(t, fake(8, dtype=torch.int32), 3)):
        with pytest.raises(TypeError):
            fn(np.zeros((8, 64), dtype=np.float16))
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn(torch.zeros(8, 64, dtype=torch.float16))
        with pytest.raises(ValueError, match="contiguous fp16"):
            fn(fake(8, 64))
        with pytest.raises(ValueError, match="could overflow"):
            fn(fake(8, Q.MAX_DIM + 64, dtype=torch.float16))
    for bad in (0, 9, True, 2.0):
        with pytest.raises(ValueError, match="n = "):
            index.encode_rows_int8(x16, bad)
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError, match="n_lists"):
            index.build_lists_int8(x16, fake(8, dtype=torch.int32), bad)
    with pytest.raises(ValueError, match="9 labels for 8 rows"):
        index.build_lists_int8(x16, fake(9, dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="labels must be int32"):
        index.build_lists_int8(x16, fake(8, dtype=torch.int64), 3)
    i32 = torch.int32
    with pytest.raises(TypeError, match="scales"):
        index.search_lists_int8(x16, fake(8, 2, dtype=i32), fake(16, 64, dtype=torch.int8), None, fake(16, dtype=i32), fake(4, dtype=i32))
    with pytest.raises(ValueError, match=r"k = .*\[1, 8\]"):
        index.search_lists_int8(x16, fake(8, 2, dtype=i32), fake(16, 64, dtype=torch.int8), fake(16), fake(16, dtype=i32), fake(4, dtype=i32), 9)
    with pytest.raises(ValueError, match="probes"):
        index.search_lists_int8(x16, fake(9, 2, dtype=i32), fake(16, 64, dtype=torch.int8), fake(16), fake(16, dtype=i32), fake(4, dtype=i32))
    # load_state_dict
    with pytest.raises(ValueError, match=r"lacks \['scales'\]"):
        ix.load_state_dict({"centroids": fake(3, 64, dtype=torch.float16), "offsets": fake(4, dtype=i32),
                            "sizes": fake(3, dtype=i32), "ids": fake(16, dtype=i32), "rows": fake(16, 64, dtype=torch.int8)})
    state = {"centroids": fake(3, 64, dtype=torch.float16), "offsets": fake(4, dtype=i32), "sizes": fake(3, dtype=i32),
             "ids": fake(16, dtype=i32), "rows": fake(16, 64, dtype=torch.int8), "scales": fake(16)}
    for key, bad, what in (("centroids", fake(4, 64, dtype=torch.float16), "this index has"),
                           ("ids", fake(15, dtype=i32), "ids must be int32"),
                           ("rows", fake(16, 64, dtype=torch.float16), "rows must be int8"),
                           ("rows", fake(16, 128, dtype=torch.int8), "rows must be int8"),
                           ("scales", fake(15), "scales must be fp32"),
                           ("scales", fake(16, dtype=torch.float16), "scales must be fp32"),
                           ("scales", torch.zeros(16), "scales must be fp32")):
        with pytest.raises((ValueError, RuntimeError), match=what):
            ix.load_state_dict({**state, key: bad})


def test_c_abi_sizing_and_refusals_without_a_device(lib):
    sb, bw, sw = lib.smi_ivf_slots_bound, lib.smi_ivf_i8_build_workspace_bytes, lib.smi_ivf_i8_search_workspace_bytes
    big_d = Q.MAX_DIM + 64
    assert bw(1000, 7, 1024) == lib.smi_ivf_build_workspace_bytes(1000, 7, 1024) == 32
    assert bw(1000, 7, Q.MAX_DIM) == 32 and bw(1000, 7, big_d) == 0
    assert bw(1000, 7, 96) == 0 and bw(1000, 0, 64) == 0 and bw(0, 7, 64) == 0 and bw(1 << 31, 7, 64) == 0
    assert bw(1 << 30, 1 << 30, 64) == 0
    # the flat search's workspace | query codes [nq, d] | query scales [nq]
    assert sw(100, 7, 4, 5, 64) == lib.smi_ivf_search_workspace_bytes(100, 7, 4, 5, 64) + 6400 + 400
    assert sw(3, 7, 4, 5, 192) == lib.smi_ivf_search_workspace_bytes(3, 7, 4, 5, 192) + 576 + 16 and sw(3, 7, 4, 5, 192) % 16 == 0
    assert sw(3, 7, 1, 1, Q.MAX_DIM) > 0
    for bad in ((0, 7, 4, 5, 64), (100, 0, 4, 5, 64), (100, 7, 0, 5, 64), (100, 7, 9, 5, 64), (100, 7, 4, 0, 64),
                (100, 7, 4, 9, 64), (100, 7, 4, 5, 96), (1 << 31, 7, 1, 1, 64), (100, 1 << 31, 1, 1, 64),
                (1 << 29, 7, 8, 1, 64), (100, 7, 4, 5, big_d)):
        assert sw(*bad) == 0, bad
    p = 0x1000  # never dereferenced: every call below is refused on its arguments
    big = 1 << 40
    cap = sb(100, 7)
    E, B, S = lib.smi_ivf_i8_encode, lib.smi_ivf_i8_build, lib.smi_ivf_i8_search
    cases = {
        "encode d": E(p, 100, 96, p, p, None),
        "encode big d": E(p, 100, big_d, p, p, None),
        "encode n": E(p, 0, 64, p, p, None),
        "encode big n": E(p, 1 << 31, 64, p, p, None),
        "encode null x": E(None, 100, 64, p, p, None),
        "encode null codes": E(p, 100, 64, None, p, None),
        "encode null scales": E(p, 100, 64, p, None, None),
        "build d": B(p, p, 100, 96, 7, p, p, p, cap, p, p, p, big, None),
        "build big d": B(p, p, 100, big_d, 7, p, p, p, cap, p, p, p, big, None),
        "build K": B(p, p, 100, 64, 0, p, p, p, cap, p, p, p, big, None),
        "build n": B(p, p, 0, 64, 7, p, p, p, cap, p, p, p, big, None),
        "build big n": B(p, p, 1 << 31, 64, 7, p, p, p, big, p, p, p, big, None),
        "build big K": B(p, p, 100, 64, 1 << 31, p, p, p, big, p, p, p, big, None),
        "build big slots": B(p, p, 1 << 30, 64, 1 << 30, p, p, p, big, p, p, p, big, None),
        "build null x": B(None, p, 100, 64, 7, p, p, p, cap, p, p, p, big, None),
        "build null labels": B(p, None, 100, 64, 7, p, p, p, cap, p, p, p, big, None),
        "build null codes": B(p, p, 100, 64, 7, None, p, p, cap, p, p, p, big, None),
        "build null scales": B(p, p, 100, 64, 7, p, None, p, cap, p, p, p, big, None),
        "build null ids": B(p, p, 100, 64, 7, p, p, None, cap, p, p, p, big, None),
        "build null offsets": B(p, p, 100, 64, 7, p, p, p, cap, None, p, p, big, None),
        "build null sizes": B(p, p, 100, 64, 7, p, p, p, cap, p, None, p, big, None),
        "build small capacity": B(p, p, 100, 64, 7, p, p, p, cap - 1, p, p, p, big, None),
        "build null ws": B(p, p, 100, 64, 7, p, p, p, cap, p, p, None, big, None),
        "build short ws": B(p, p, 100, 64, 7, p, p, p, cap, p, p, p, bw(100, 7, 64) - 1, None),
        "build misaligned ws": B(p, p, 100, 64, 7, p, p, p, cap, p, p, p + 8, big, None),
        "search d": S(p, 100, 96, p, 4, p, p, p, p, 7, 5, p, p, p, big, None),
        "search big d": S(p, 100, big_d, p, 4, p, p, p, p, 7, 5, p, p, p, big, None),
        "search K": S(p, 100, 64, p, 4, p, p, p, p, 0, 5, p, p, p, big, None),
        "search nq": S(p, 0, 64, p, 4, p, p, p, p, 7, 5, p, p, p, big, None),
        "search big nq": S(p, 1 << 31, 64, p, 4, p, p, p, p, 7, 5, p, p, p, big, None),
        "search big pairs": S(p, 1 << 29, 64, p, 8, p, p, p, p, 7, 5, p, p, p, big, None),
        "search k 0": S(p, 100, 64, p, 4, p, p, p, p, 7, 0, p, p, p, big, None),
        "search k 9": S(p, 100, 64, p, 4, p, p, p, p, 7, 9, p, p, p, big, None),
        "search nprobe 0": S(p, 100, 64, p, 0, p, p, p, p, 7, 5, p, p, p, big, None),
        "search nprobe 9": S(p, 100, 64, p, 9, p, p, p, p, 7, 5, p, p, p, big, None),
        "search null q": S(None, 100, 64, p, 4, p, p, p, p, 7, 5, p, p, p, big, None),
        "search null probes": S(p, 100, 64, None, 4, p, p, p, p, 7, 5, p, p, p, big, None),
        "search null codes": S(p, 100, 64, p, 4, None, p, p, p, 7, 5, p, p, p, big, None),
        "search null scales": S(p, 100, 64, p, 4, p, None, p, p, 7, 5, p, p, p, big, None),
        "search null ids": S(p, 100, 64, p, 4, p, p, None, p, 7, 5, p, p, p, big, None),
        "search null offsets": S(p, 100, 64, p, 4, p, p, p, None, 7, 5, p, p, p, big, None),
        "search null idx": S(p, 100, 64, p, 4, p, p, p, p, 7, 5, None, p, p, big, None),
        "search null score": S(p, 100, 64, p, 4, p, p, p, p, 7, 5, p, None, p, big, None),
        "search null ws": S(p, 100, 64, p, 4, p, p, p, p, 7, 5, p, p, None, big, None),
        "search short ws": S(p, 100, 64, p, 4, p, p, p, p, 7, 5, p, p, p, sw(100, 7, 4, 5, 64) - 1, None),
        "search flat-sized ws": S(p, 100, 64, p, 4, p, p, p, p, 7, 5, p, p, p, lib.smi_ivf_search_workspace_bytes(100, 7, 4, 5, 64), None),
        "search misaligned ws": S(p, 100, 64, p, 4, p, p, p, p, 7, 5, p, p, p + 4, big, None),
    }
    assert all(rc != 0 for rc in cases.values()), {k: v for k, v in cases.items() if v == 0}
    assert cases["encode big d"] == cases["build big d"] == cases["search big d"] == -2
    assert E(p, 100, big_d, p, p, None) == -2 and b"could overflow" in lib.smi_last_error()
    assert B(p, p, 100, 64, 7, p, p, p, cap - 1, p, p, p, big, None) == -1 and b"smi_ivf_slots_bound" in lib.smi_last_error()
    assert B(p, p, 100, 96, 7, p, p, p, cap, p, p, p, big, None) == -2 and b"multiple of 64" in lib.smi_last_error()
    assert S(p, 100, 64, p, 4, p, p, p, p, 7, 5, p, p, p, 16, None) == -1
    assert b"smi_ivf_i8_search_workspace_bytes" in lib.smi_last_error()
    assert S(p, 100, 64, p, 9, p, p, p, p, 7, 5, p, p, p, big, None) == -1 and b"nprobe" in lib.smi_last_error()
    assert E(p, 100, 64, None, p, None) == -1 and E(p, 100, 96, p, p, None) == -2
