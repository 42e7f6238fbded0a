"""CPU: L2 search over the product-quantised lists, plain and residual -- the numpy restatement
(tests/ivf_pq_l2_ref.py) against plain loops, `math.fsum` and int64 arithmetic; the conditions on the data that
tests/test_gpu_ivf_pq_l2.py relies on; every refusal of the Python layer (sonar_amd/index.py), the markers that keep the
states of the four product-quantised classes apart, and the refusals and sizing of the new C-ABI entries.  Nothing here needs
a device."""
import math
import re

import numpy as np
import pytest
import torch

from tests import ivf_pq_l2_ref as Q
from tests import ivf_pq_ref as P
from tests import ivf_pq_residual_ref as PR
from tests import l2_ref as L


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _small_case(seed=0, n=40, nq=9, d=16, k_lists=4, dsub=8):
    rng = np.random.default_rng(seed)
    y, q = L.sparse_int_rows(rng, n, d), L.int_rows(rng, nq, d)
    c = L.int_rows(rng, k_lists, d)
    labels = L.assign(y, c, L.half_norms(c))[0]
    cb = Q.scaled_integer_codebooks(rng, d, dsub)
    return y, q, c, labels, cb


# ------------------------------------------------------------------------------------------------- the restatement
def _loop_search(q, rows64, labels, k_lists, probes, k, visible=None):
    """A plain double loop in Python floats over the reconstructed rows, Python's stable sort: exact on integer data."""
    out_s = np.full((len(q), k), -np.inf)
    out_i = np.full((len(q), k), -1, dtype=np.int64)
    for m in range(len(q)):
        cand = []
        for c in probes[m]:
            if not 0 <= c < k_lists:
                continue
            for n in range(len(rows64)):
                if labels[n] != c or (visible is not None and not visible[n]):
                    continue
                dot = half = 0.0
                for a, b in zip(q[m].tolist(), rows64[n].tolist()):
                    dot += a * b
                    half += b * b
                cand.append((dot - 0.5 * half, n))
        cand.sort(key=lambda t: t[1])
        cand.sort(key=lambda t: -t[0])  # stable: ties to the lower id
        for j, (v, n) in enumerate(cand[:k]):
            out_s[m, j], out_i[m, j] = v + 0.0, n
    return out_s, out_i


def test_restated_searches_equal_a_plain_double_loop():
    y, q, c, labels, cb = _small_case()
    q[2] = 0
    y[3] = y[9] = y[5]  # equal rows tie
    labels = labels.copy()
    labels[3] = labels[9] = labels[5]
    rng = np.random.default_rng(1)
    probes = np.stack([rng.permutation(4)[:3] for _ in range(len(q))])
    probes[1, 0], probes[4] = -1, [7, -3, 4]  # an entry, and a whole row, that names no list
    visible = rng.random(len(y)) < 0.7
    hq = L.half_norms(q).astype(np.float64)
    # plain
    codes = P.encode(y, cb)
    rows = Q.reconstruct(codes, cb)
    for k in (1, 4, 8):
        for vis in (None, visible):
            dist, ids, raw = Q.search_plain(q, codes, cb, labels, 4, probes, k, vis)
            want_s, want_i = _loop_search(q, rows, labels, 4, probes, k, vis)
            assert np.array_equal(ids, want_i) and np.array_equal(raw.astype(np.float64), want_s), (k, vis is None)
            assert np.array_equal(dist.astype(np.float64)[ids >= 0], (2 * (hq[:, None] - want_s))[ids >= 0])
    assert (ids[4] == -1).all() and np.isposinf(dist[4]).all() and np.isneginf(raw[4]).all()
    zeros = Q.scores_plain(q, codes, cb)
    assert (zeros == 0).any() and not np.signbit(zeros[zeros == 0]).any()  # a zero score is +0
    # residual
    rcodes = PR.encode(y, labels, c, cb)
    rrows = Q.reconstruct(rcodes, cb, labels, c)
    for k in (1, 4, 8):
        for vis in (None, visible):
            dist, ids, raw = Q.search_residual(q, rcodes, cb, labels, c, probes, None, k, vis)
            want_s, want_i = _loop_search(q, rrows, labels, 4, probes, k, vis)
            assert np.array_equal(ids, want_i) and np.array_equal(raw.astype(np.float64), want_s), (k, vis is None)
    # the distances ARE the squared distances to the reconstructed rows
    dist, ids, _ = Q.search_residual(q, rcodes, cb, labels, c, np.tile(np.arange(4), (len(q), 1)), None, 8)
    exact = Q.exact_sq_dist(q, rrows)
    assert np.array_equal(dist.astype(np.int64), np.take_along_axis(exact, ids, axis=1))
    assert np.array_equal(np.sort(exact, axis=1)[:, :8], dist.astype(np.int64))
    # the garbage in the coarse entry of a probe that names no list is not read
    coarse = Q.coarse(q, c, probes)
    coarse[1, 0] = np.nan
    coarse[4] = [np.inf, -np.inf, 3e38]
    a = Q.search_residual(q, rcodes, cb, labels, c, probes, coarse, 8)
    b = Q.search_residual(q, rcodes, cb, labels, c, probes, None, 8)
    assert np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[2]), _bits(b[2]))


@pytest.mark.parametrize("d,dsub", [(64, 8), (192, 64), (520, 8), (1024, 16)])
def test_bias_against_fsum_and_exact_on_integers(d, dsub):
    rng = np.random.default_rng(d + dsub)
    n, k_lists = 9, 3
    cb = (rng.standard_normal((d // dsub, 256, dsub)) * rng.uniform(0.01, 30.0, (d // dsub, 256, 1))).astype(np.float16)
    c = (rng.standard_normal((k_lists, d)) * 3.0).astype(np.float16)
    codes = rng.integers(0, 256, (n, d // dsub)).astype(np.uint8)
    labels = np.array([0, 1, 2, 0, 1, 2, -1, 3, 0])  # two labels outside [0, K): no centroid
    r = P.decode(codes, cb)
    cr = Q.list_centroids(labels, c)
    assert not cr[6].any() and not cr[7].any() and np.array_equal(cr[8], c[0])
    # the plain bias is the half norm of the decoded row, negated: the same bits
    assert np.array_equal(_bits(Q.bias_plain(codes, cb)), _bits(-L.half_norms(r)))
    s1 = Q.ordered_sum(cr.astype(np.float64) * r.astype(np.float64))
    s2 = Q.ordered_sum(r.astype(np.float64) ** 2)
    got = Q.bias_residual(codes, cb, labels, c)
    for i in range(n):
        e1 = math.fsum(float(a) * float(b) for a, b in zip(cr[i], r[i]))
        e2 = math.fsum(float(b) * float(b) for b in r[i])
        m1 = math.fsum(abs(float(a) * float(b)) for a, b in zip(cr[i], r[i]))
        assert abs(s1[i] - e1) <= 2.0 ** -50 * m1 and abs(s2[i] - e2) <= 2.0 ** -50 * e2
        exact = e1 + 0.5 * e2
        assert got[i] == -np.float32(exact) or abs(float(got[i]) + exact) <= 2.0 ** -23 * (m1 + 0.5 * e2)
    assert np.array_equal(_bits(got[6:8]), _bits(Q.bias_plain(codes, cb)[6:8]))  # no centroid: the plain bias
    # integers: exact
    cbi, ci = Q.scaled_integer_codebooks(rng, d, dsub), L.int_rows(rng, k_lists, d)
    ri, cri = P.decode(codes, cbi).astype(np.int64), Q.list_centroids(labels, ci).astype(np.int64)
    assert np.array_equal(Q.bias_plain(codes, cbi).astype(np.float64), -0.5 * (ri * ri).sum(axis=1))
    assert np.array_equal(Q.bias_residual(codes, cbi, labels, ci).astype(np.float64),
                          -((cri * ri).sum(axis=1) + 0.5 * (ri * ri).sum(axis=1)))
    # a zero decoded row: bias -0 (plain: what prepare_rows(...)[1].neg() gives), a pad slot +0
    cbi[:, 0] = 0
    zero = np.zeros((1, d // dsub), dtype=np.uint8)
    assert _bits(Q.bias_plain(zero, cbi))[0] == 0x80000000
    assert _bits(Q.slot_bias(Q.bias_plain(zero, cbi), [-1, 0]))[0] == 0


def test_the_residual_identity_in_int64():
    """q . y^ - 1/2 ||y^||^2 = coarse + q . r^ - (c . r^ + 1/2 ||r^||^2), y^ = c + r^: in twice the units, exactly."""
    y, q, c, labels, cb = Q.int_case(300, 20, 64, 5)
    codes = PR.encode(y, labels, c, cb)
    r = P.decode(codes, cb).astype(np.int64)
    cl = Q.list_centroids(labels, c).astype(np.int64)
    qi = q.astype(np.int64)
    yh = cl + r
    lhs2 = 2 * qi @ yh.T - (yh * yh).sum(axis=1)[None, :]
    coarse2 = 2 * qi @ cl.T - (cl * cl).sum(axis=1)[None, :]
    rhs2 = coarse2 + 2 * qi @ r.T - (2 * (cl * r).sum(axis=1) + (r * r).sum(axis=1))[None, :]
    assert np.array_equal(lhs2, rhs2)
    # ... and the restated float32 expression holds those values
    bias = Q.bias_residual(codes, cb, labels, c)
    assert np.array_equal(2 * bias.astype(np.float64), -(2 * (cl * r).sum(axis=1) + (r * r).sum(axis=1)))
    pre = L.scores(q, P.decode(codes, cb), bias)
    coarse = L.scores(q, c, -L.half_norms(c))[:, labels]
    total = (pre + coarse).astype(np.float32)
    assert np.array_equal(2 * total.astype(np.float64), lhs2)
    hq = L.half_norms(q)
    assert np.array_equal(L.sq_dist(hq, total).astype(np.int64), Q.exact_sq_dist(q, yh))
    # the residual of an integer row against an integer centroid is exact, and so is the reconstruction
    assert np.array_equal(PR.residuals(y, labels, c).astype(np.int64), y.astype(np.int64) - cl)


@pytest.mark.parametrize("n,nq,d,n_lists", [(1500, 40, 64, 8), (1500, 300, 64, 8), (1100, 40, 64, 12), (1100, 400, 64, 12),
                                            (1100, 70, 192, 12), (1100, 40, 128, 12)])
def test_conditions_on_the_exact_data(n, nq, d, n_lists):
    """The integer cases of the GPU tests: every bias and score a multiple of 1/2 below 2^24, and the nearest reconstructed
    row is NOT the row of the largest inner product for most queries -- a scan that dropped the bias would be caught."""
    y, q, c, labels, cb = Q.int_case(n, nq, d, n_lists)
    assert np.bincount(labels, minlength=n_lists).min() >= 1
    codes = P.encode(y, cb)
    bias = Q.bias_plain(codes, cb)
    share, exact = Q.data_conditions(q, Q.reconstruct(codes, cb), bias, Q.scores_plain(q, codes, cb))
    assert exact and share > 0.5, share
    rcodes = PR.encode(y, labels, c, cb)
    rbias = Q.bias_residual(rcodes, cb, labels, c)
    total = (L.scores(q, P.decode(rcodes, cb), rbias) + L.scores(q, c, -L.half_norms(c))[:, labels]).astype(np.float32)
    share, exact = Q.data_conditions(q, Q.reconstruct(rcodes, cb, labels, c), rbias, total)
    assert exact and share > 0.5, share
    assert len(np.unique(codes, axis=0)) > n // 2 and len(np.unique(rcodes, axis=0)) > n // 2  # the codes tell rows apart


def test_the_bound_of_real_valued_residual_scores():
    """The bound is small against the scores it bounds, and holds for the restatement's own float32 chain."""
    rng = np.random.default_rng(3)
    n, nq, d, k_lists, dsub = 200, 30, 64, 5, 8
    y = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float16)
    q = rng.standard_normal((nq, d)).astype(np.float16)
    c = y[:k_lists].copy()
    labels = L.assign(y, c, L.half_norms(c))[0]
    cb = P.random_codebooks(rng, d, dsub, scale=4.0)
    codes = PR.encode(y, labels, c, cb)
    s64, bound = Q.residual_score_bound(q, codes, cb, labels, c)
    assert bound.max() < 1e-3 and (bound > 0).all()
    pre = L.scores(q, P.decode(codes, cb), Q.bias_residual(codes, cb, labels, c))
    total = (pre + L.scores(q, c, -L.half_norms(c))[:, labels]).astype(np.float32)
    assert (np.abs(total.astype(np.float64) - s64) <= bound).all()


# ------------------------------------------------------------------------------------------------------- refusals
class FakeDevice(torch.Tensor):
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta").as_subclass(FakeDevice)


def boom(*a, **k):
    raise AssertionError("reached the device")


f16, i32, u8 = torch.float16, torch.int32, torch.uint8


def _patched(monkeypatch):
    from sonar_amd import index

    pad = lambda r: (r + 255) // 256 * 256  # noqa: E731
    monkeypatch.setattr(index, "prepare_rows", lambda t: (fake(pad(t.shape[0]), t.shape[1], dtype=f16), fake(pad(t.shape[0]))))
    monkeypatch.setattr(index, "normalize_rows", lambda t: fake(pad(t.shape[0]), t.shape[1], dtype=f16))
    return index


@pytest.mark.parametrize("name", ["IVFPQL2Index", "IVFPQResidualL2Index"])
def test_python_refusals_of_the_classes(monkeypatch, name):
    from sonar_amd.clustering import KMeans, SphericalKMeans
    from sonar_amd.transforms import LinearTransform

    index = _patched(monkeypatch)
    cls = getattr(index, name)
    cb = fake(8, 256, 8, dtype=f16)
    ix = cls(fake(3, 64), cb)
    monkeypatch.setattr(index, "topk_bias_prepared", boom)
    monkeypatch.setattr(index._lib, "load", boom)
    q = fake(5, 64)
    assert ix.dim == 64 and ix.n_lists == 3 and ix.dsub == 8 and tuple(ix.codebooks.shape) == (8, 256, 8)
    with pytest.raises(RuntimeError, match="before fit"):
        cls(KMeans(3), cb)
    with pytest.raises(TypeError, match=f"an {name} needs Euclidean centroids"):
        cls(SphericalKMeans(3), cb)
    with pytest.raises(RuntimeError, match="HIP device"):
        cls(torch.zeros(3, 64), cb)
    with pytest.raises(ValueError, match="the product quantiser has dim 128"):
        cls(fake(3, 64), fake(16, 256, 8, dtype=f16))
    with pytest.raises(ValueError, match="codebooks must be contiguous fp16"):
        cls(fake(3, 64), fake(8, 256, 8))
    with pytest.raises(ValueError, match="dsub = 12"):
        cls.train(fake(300, 64), 3, dsub=12)
    for call in (lambda: ix.search(q), lambda: ix.state_dict(), lambda: ix.list_sizes, lambda: ix.extend(fake(4, 64)),
                 lambda: ix.remove(ids=fake(2, dtype=i32)), lambda: ix.row_filter(mask=fake(9, dtype=torch.bool))):
        with pytest.raises(RuntimeError, match="before add"):
            call()
    with pytest.raises(ValueError, match="dim 128"):
        ix.add(fake(10, 128))
    with pytest.raises(ValueError, match="labels"):
        ix.add(fake(10, 64), labels=fake(9, dtype=i32))
    ix._added = True
    ix._ids = fake(48, dtype=i32)
    with pytest.raises(RuntimeError, match="already called"):
        ix.add(fake(10, 64))
    for bad in (0, 9, True, 4.0):
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
    for bad in (fake(5, 2, dtype=torch.int64), fake(4, 2, dtype=i32), fake(5, 9, dtype=i32)):
        with pytest.raises(ValueError, match="probes"):
            ix.search(q, probes=bad)
    with pytest.raises(TypeError, match="RowFilter"):
        ix.search(q, rows=fake(48, dtype=i32))
    # the flat L2 class's sentence
    with pytest.raises(TypeError, match=re.escape("query_keys: the keyed scan has no L2 twin (DESIGN.md 7); filter with "
                                                   "rows=index.row_filter(mask=...)")):
        ix.search(q, query_keys=fake(5, dtype=i32))
    with pytest.raises(TypeError, match="refine must be None or the pair"):
        ix.search(q, refine=fake(256, 64, dtype=f16))
    with pytest.raises(ValueError, match=r"refine must hold the contiguous fp16 \[rows, 64\]"):
        ix.search(q, refine=(fake(256, 128, dtype=f16), fake(256)))
    with pytest.raises(ValueError, match=r"refine must hold the fp32 \[256\] half norms"):
        ix.search(q, refine=(fake(256, 64, dtype=f16), fake(255)))
    if name == "IVFPQResidualL2Index":
        with pytest.raises(ValueError, match="coarse belongs to probes"):
            ix.search(q, coarse=fake(5, 1))
        with pytest.raises(ValueError, match=r"coarse must be fp32 \[5, 2\]"):
            ix.search(q, probes=fake(5, 2, dtype=i32), coarse=fake(5, 3))
    else:
        with pytest.raises(TypeError, match="coarse"):
            ix.search(q, coarse=fake(5, 1))
    for attr in ("range_search", "search_wide", "self_join"):
        with pytest.raises(TypeError, match="product-quantiser codes"):
            getattr(ix, attr)(q)
    with pytest.raises(TypeError, match="DESIGN.md 7"):
        ix.probe_wide(q)
    with pytest.raises(TypeError, match="as they are"):
        ix.centroids_normalized
    other = getattr(index, "IVFPQL2Index" if name == "IVFPQResidualL2Index" else "IVFPQResidualL2Index")(fake(3, 64), cb)
    with pytest.raises(TypeError, match=f"a {name} takes a {name}"):
        ix.merge_from(other)
    # behind a transform: the wrapper's own refine is a cosine re-score
    eye = LinearTransform.__new__(LinearTransform)
    eye._w = fake(64, 64, dtype=f16)
    eye.apply = lambda t: t
    wrapped = index.PreTransformIndex(eye, ix)
    with pytest.raises(TypeError, match=r"index\.search\(transform\.apply\(q\), refine="):
        wrapped.search(q, refine=fake(256, 64, dtype=f16))


def test_the_four_product_quantised_states_are_kept_apart(monkeypatch):
    index = _patched(monkeypatch)
    monkeypatch.setattr(index._lib, "load", boom)
    base = {"centroids": fake(3, 64, dtype=f16), "offsets": fake(4, dtype=i32), "sizes": fake(3, dtype=i32),
            "rows": fake(48, 8, dtype=u8), "ids": fake(48, dtype=i32), "codebooks": fake(8, 256, 8, dtype=f16)}
    one = fake(1, dtype=u8)
    states = {"IVFPQIndex": base, "IVFPQResidualIndex": {**base, "by_residual": one},
              "IVFPQL2Index": {**base, "bias": fake(48), "metric_l2": one},
              "IVFPQResidualL2Index": {**base, "bias": fake(48), "metric_l2": one, "by_residual": one}}
    for cls_name in states:
        cls = getattr(index, cls_name)
        for state_name, state in states.items():
            if cls_name == state_name:
                # its own state passes every check up to the read-back of the offsets (a meta tensor has no value)
                with pytest.raises((RuntimeError, NotImplementedError)):
                    cls.from_state_dict(state)
            else:
                with pytest.raises(ValueError, match="the state is that of|state lacks"):
                    cls.from_state_dict(state)
    # neither flat class loads them
    for state in (states["IVFPQL2Index"], states["IVFPQResidualL2Index"]):
        with pytest.raises(ValueError, match="IVFFlatL2Index|rows must be fp16"):
            index.IVFFlatIndex.from_state_dict(state)
        with pytest.raises(ValueError, match="rows must be fp16"):
            index.IVFFlatL2Index.from_state_dict(state)
    # and the L2 classes name what is missing
    with pytest.raises(ValueError, match=r"state lacks \['bias'\]"):
        index.IVFPQL2Index.from_state_dict({k: v for k, v in states["IVFPQL2Index"].items() if k != "bias"})
    with pytest.raises(ValueError, match=r"lacks \['metric_l2'\].*normalised"):
        index.IVFPQL2Index.from_state_dict({**base, "bias": fake(48)})
    with pytest.raises(ValueError, match="bias must be fp32"):
        index.IVFPQL2Index.from_state_dict({**states["IVFPQL2Index"], "bias": fake(47)})
    with pytest.raises(ValueError, match="IVFPQL2Index or IVFPQResidualL2Index"):
        index.IVFPQIndex.from_state_dict(states["IVFPQL2Index"])


def test_python_refusals_of_the_list_functions(monkeypatch):
    index = _patched(monkeypatch)
    monkeypatch.setattr(index._lib, "load", boom)
    codes, cb, cent = fake(48, 8, dtype=u8), fake(8, 256, 8, dtype=f16), fake(3, 64, dtype=f16)
    ids, off, labels = fake(48, dtype=i32), fake(4, dtype=i32), fake(48, dtype=i32)
    B = index.pq_l2_bias
    with pytest.raises(ValueError, match="codebooks must be contiguous fp16"):
        B(codes, fake(8, 256, 12, dtype=f16))
    with pytest.raises(ValueError, match=r"codes must be contiguous uint8 \[rows, 8\]"):
        B(fake(48, 9, dtype=u8), cb)
    with pytest.raises(RuntimeError, match="HIP device"):
        B(torch.zeros(48, 8, dtype=u8), cb)
    with pytest.raises(ValueError, match="give centroids, or neither"):
        B(codes, cb, labels)
    with pytest.raises(ValueError, match="give centroids, or neither"):
        B(codes, cb, ids=ids, offsets=off)
    with pytest.raises(ValueError, match="one of the two"):
        B(codes, cb, None, cent)
    with pytest.raises(ValueError, match="one of the two"):
        B(codes, cb, labels, cent, ids=ids, offsets=off)
    with pytest.raises(ValueError, match="give ids with them"):
        B(codes, cb, None, cent, offsets=off)
    with pytest.raises(ValueError, match="labels must be int32"):
        B(codes, cb, fake(47, dtype=i32), cent)
    with pytest.raises(ValueError, match="offsets must be int32"):
        B(codes, cb, None, cent, ids=ids, offsets=fake(5, dtype=i32))
    with pytest.raises(ValueError, match="ids must be int32"):
        B(codes, cb, ids=fake(48, dtype=torch.int64))
    with pytest.raises(ValueError, match="centroids must be a contiguous fp16"):
        B(codes, cb, labels, fake(3, 128, dtype=f16))
    S = index.search_lists_pq_l2
    q16, probes, bias = fake(256, 64, dtype=f16), fake(5, 2, dtype=i32), fake(48)
    with pytest.raises(ValueError, match=r"k = .*\[1, 8\]"):
        S(q16, probes, codes, cb, bias, ids, off, 9)
    with pytest.raises(ValueError, match="probes"):
        S(q16, fake(5, 9, dtype=i32), codes, cb, bias, ids, off, 8)
    with pytest.raises(ValueError, match="codebooks cover dim"):
        S(fake(256, 128, dtype=f16), probes, codes, cb, bias, ids, off, 8)
    with pytest.raises(ValueError, match="codes must be contiguous uint8"):
        S(q16, probes, fake(48, 8, dtype=torch.int8), cb, bias, ids, off, 8)
    with pytest.raises(ValueError, match=r"bias must be contiguous fp32 \[48\]"):
        S(q16, probes, codes, cb, fake(47), ids, off, 8)
    with pytest.raises(ValueError, match=r"coarse must be fp32 \[5, 2\]"):
        S(q16, probes, codes, cb, bias, ids, off, 8, fake(5, 3))


# ------------------------------------------------------------------------------------------------------- the C ABI
NAMES = {"smi_l2_pq_bias", "smi_l2_pq_search_ws_bytes", "smi_l2_pq_search", "smi_l2_pq_search_residual"}


def test_new_symbols_are_declared_bound_and_exported(lib):
    import os
    import subprocess

    from sonar_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sonar_mi355.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert NAMES <= set(re.findall(r"\b(smi_[a-z0-9_]+)\s*\(", header))
    assert NAMES <= set(_lib.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert NAMES <= set(re.findall(r"\bT (smi_[a-z0-9_]+)", out))
    # only functions were added: the revision stays, and so do the pinned sets of smi_ivf_ / smi_pq_ entries
    assert lib.smi_abi_version() == _lib.ABI_VERSION == 7 and "#define SMI_ABI_VERSION 7" in text
    assert not any(n.startswith(("smi_ivf_", "smi_pq_")) or n.endswith("_workspace_bytes") for n in NAMES)
    assert "fl32(fl32(acc + bias) + coarse)" in text and "fl32(acc + bias)" in text  # the score contract is written down


def test_c_abi_of_the_searches(lib):
    pw, w, S, R = lib.smi_ivf_pq_search_workspace_bytes, lib.smi_l2_pq_search_ws_bytes, lib.smi_l2_pq_search, \
        lib.smi_l2_pq_search_residual
    assert w(100, 7, 4, 5, 64, 8) == pw(100, 7, 4, 5, 64, 8) > 0  # the PQ search's layout
    lib.smi_l2_pq_bias(None, 1, 64, 8, None, None, None, None, None, 0, None, None)
    before = lib.smi_last_error()
    for bad in ((0, 7, 4, 5, 64, 8), (100, 0, 4, 5, 64, 8), (100, 7, 0, 5, 64, 8), (100, 7, 9, 5, 64, 8), (100, 7, 4, 0, 64, 8),
                (100, 7, 4, 9, 64, 8), (100, 7, 4, 5, 96, 8), (100, 7, 4, 5, 64, 12), (100, 7, 4, 5, 64, 128), (1 << 31, 7, 1, 1, 64, 8),
                (100, 1 << 31, 1, 1, 64, 8)):
        assert w(*bad) == 0, bad
    assert lib.smi_last_error() == before  # a sizing call leaves the last error alone
    p, big = 0x1000, 1 << 40  # never dereferenced: every call below is refused on its arguments

    def plain(q=p, nq=100, d=64, probes=p, nprobe=4, codes=p, dsub=8, cb=p, bias=p, ids=p, off=p, K=7, k=5, idx=p, score=p, ws=p,
              ws_bytes=big):
        return S(q, nq, d, probes, nprobe, codes, dsub, cb, bias, ids, off, K, k, idx, score, ws, ws_bytes, None)

    def res(coarse=p, q=p, nq=100, d=64, probes=p, nprobe=4, codes=p, dsub=8, cb=p, bias=p, ids=p, off=p, K=7, k=5, idx=p, score=p,
            ws=p, ws_bytes=big):
        return R(q, nq, d, probes, coarse, nprobe, codes, dsub, cb, bias, ids, off, K, k, idx, score, ws, ws_bytes, None)

    changes = [dict(d=96), dict(K=0), dict(nq=0), dict(k=0), dict(k=9), dict(nprobe=0), dict(nprobe=9), dict(q=None),
               dict(probes=None), dict(codes=None), dict(bias=None), dict(bias=p + 4), dict(ids=None), dict(off=None), dict(idx=None),
               dict(score=None), dict(ws=None), dict(ws_bytes=w(100, 7, 4, 5, 64, 8) - 1), dict(ws=p + 4), dict(dsub=12),
               dict(dsub=128), dict(cb=None), dict(cb=p + 8)]
    for fn in (plain, res):
        got = {str(c): fn(**c) for c in changes}
        assert all(rc not in (0, -3) for rc in got.values()), got  # refused on its arguments, not for want of a device
    assert res(coarse=None) == -1 and b"null argument" in lib.smi_last_error()
    assert res(coarse=p + 2) == -1 and b"coarse" in lib.smi_last_error()
    assert plain(bias=p + 4) == -1 and b"list_bias must be 16-byte aligned" in lib.smi_last_error()
    assert plain(dsub=12) == -2 and b"dsub=12" in lib.smi_last_error()
    assert plain(cb=None) == -1 and b"null codebooks" in lib.smi_last_error()
    assert plain(k=9) != 0 and b"k=9" in lib.smi_last_error()
    assert plain(ws_bytes=16) == -1 and b"smi_l2_pq_search_ws_bytes" in lib.smi_last_error()
    if not torch.cuda.is_available():  # every check passed: only the missing device answers
        assert plain(ws_bytes=w(100, 7, 4, 5, 64, 8)) == -3 and res(ws_bytes=w(100, 7, 4, 5, 64, 8)) == -3


def test_c_abi_of_the_bias(lib):
    p = 0x1000

    def B(codes=p, n=10, d=64, dsub=8, cb=p, ids=None, off=None, labels=None, cent=None, K=0, out=p):
        return lib.smi_l2_pq_bias(codes, n, d, dsub, cb, ids, off, labels, cent, K, out, None)

    changes = [dict(codes=None), dict(out=None), dict(n=0), dict(n=1 << 31), dict(d=96), dict(d=0), dict(dsub=12), dict(cb=None),
               dict(cb=p + 8), dict(labels=p), dict(off=p, ids=p), dict(cent=p, K=3), dict(cent=p, K=3, labels=p, off=p, ids=p),
               dict(cent=p, K=3, off=p), dict(cent=p + 8, K=3, labels=p), dict(cent=p, K=0, labels=p), dict(cent=p, K=1 << 31, labels=p)]
    got = {str(c): B(**c) for c in changes}
    assert all(rc not in (0, -3) for rc in got.values()), got  # refused on its arguments, not for want of a device
    assert B(labels=p) == -1 and b"give centroids, or neither" in lib.smi_last_error()
    assert B(cent=p, K=3) == -1 and b"one of the two" in lib.smi_last_error()
    assert B(cent=p, K=3, off=p) == -1 and b"give slot_ids" in lib.smi_last_error()
    if not torch.cuda.is_available():
        assert B() == -3 and B(ids=p) == -3 and B(cent=p, K=3, labels=p) == -3 and B(cent=p, K=3, off=p, ids=p) == -3
