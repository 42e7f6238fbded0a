"""GPU: smi_gram against the exact integer product and its derived fp32 bound, `column_sums`, `LinearTransform.apply` against
fp64, the PCA and OPQ fits, and `PreTransformIndex` (sonar_amd/transforms.py, sonar_amd/csrc/gram.hip, DESIGN.md 3.25;
restated in tests/transforms_ref.py)."""
import functools

import numpy as np
import pytest
import torch

from tests import transforms_ref as R

pytestmark = pytest.mark.gpu

CHUNK = R.CHUNK_ROWS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ints(rng, n, d):
    return rng.integers(-8, 9, (n, d)).astype(np.float16)


def _unit_rows(rng, n, d):
    x = rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16)


# ------------------------------------------------------------------------------------------------------------ gram
@pytest.mark.parametrize("d1,d2", [(64, 64), (128, 128), (64, 192), (192, 64)])
def test_gram_is_exact_on_integers(d1, d2):
    from sonar_amd.transforms import GRAM_CHUNK_ROWS, gram

    assert GRAM_CHUNK_ROWS == CHUNK
    rng = np.random.default_rng(d1 * 1000 + d2)
    big = 3 * CHUNK + 17
    x, y = _ints(rng, big, d1), _ints(rng, big, d2)
    xd, yd = _dev(x), _dev(y)
    for n in (1, 31, 32, 33, CHUNK - 1, CHUNK, CHUNK + 1, big):
        want = R.gram_int(x[:n], y[:n])
        got = gram(xd, yd, n=n)
        assert got.dtype == torch.float64 and tuple(got.shape) == (d1, d2)
        assert np.array_equal(got.cpu().numpy(), want.astype(np.float64)), (d1, d2, n)
        if d1 == d2:
            sym = gram(xd, n=n)
            assert torch.equal(sym, gram(xd, xd.clone(), n=n)), n
            assert torch.equal(sym, sym.t()), n
            assert np.array_equal(sym.cpu().numpy(), R.gram_int(x[:n]).astype(np.float64)), n


@pytest.mark.parametrize("n,d1,d2", [(33 * CHUNK + 17, 64, 256), (3 * 32 * CHUNK + 5, 64, 128)])
def test_gram_is_exact_where_a_span_holds_several_chunks(n, d1, d2):
    """Above 32 chunks a work unit walks several chunks and adds every chunk after its first into its fp64 tile: 17 spans of 2
    chunks with a partial last chunk, and 24 spans of 4 with a last span of 5 rows.  64 NaN rows lie behind n."""
    from sonar_amd.transforms import gram

    rng = np.random.default_rng(n)
    x, y = _ints(rng, n, d1), _ints(rng, n, d2)
    xd = _dev(np.concatenate([x, np.full((64, d1), np.nan, dtype=np.float16)]))
    yd = _dev(np.concatenate([y, np.full((64, d2), np.nan, dtype=np.float16)]))
    assert np.array_equal(gram(xd, yd, n=n).cpu().numpy(), R.gram_int(x, y).astype(np.float64))
    assert np.array_equal(gram(yd, xd, n=n).cpu().numpy(), R.gram_int(y, x).astype(np.float64))
    for a, ad in ((x, xd), (y, yd)):  # one tile, and the upper triangle of 2 x 2 tiles
        sym = gram(ad, n=n)
        assert torch.equal(sym, sym.t()) and torch.equal(sym, gram(ad, ad.clone(), n=n))
        assert np.array_equal(sym.cpu().numpy(), R.gram_int(a).astype(np.float64))


def test_gram_restarts_its_fp32_sums_every_chunk():
    """Products of 4096 over three chunks and one product of 1: every chunk's sum is below 2^24 and exact, the sum over all
    rows, 3 * 2^23 - 4095, is odd and above 2^24, where fp32 holds even numbers only.  One fp32 accumulator over all rows, or
    over any two chunks, cannot give it; neither can chunks twice as long."""
    from sonar_amd.transforms import gram

    n = 3 * CHUNK
    x = np.full((n, 64), 64.0, dtype=np.float16)
    x[2 * CHUNK + 5] = 1.0
    want = R.gram_int(x)
    assert want[0, 0] == 3 * 2 ** 23 - 4095 and float(np.float32(want[0, 0])) != want[0, 0]
    with pytest.raises(AssertionError, match="exact range"):
        R.gram_int(x, chunk=2 * CHUNK)
    xd = _dev(x)
    assert np.array_equal(gram(xd).cpu().numpy(), want.astype(np.float64))
    assert np.array_equal(gram(xd, xd.clone()).cpu().numpy(), want.astype(np.float64))


def test_gram_reads_nothing_behind_n_and_repeats_its_bits():
    from sonar_amd.transforms import gram

    rng = np.random.default_rng(7)
    n, d1, d2 = CHUNK + 77, 128, 192
    x, y = _unit_rows(rng, n, d1), _unit_rows(rng, n, d2)
    clean = gram(_dev(x), _dev(y))
    xb = _dev(np.concatenate([x, np.full((64, d1), np.nan, dtype=np.float16)]))
    yb = _dev(np.concatenate([y, np.full((64, d2), np.nan, dtype=np.float16)]))
    guarded = gram(xb, yb, n=n)
    assert bool(torch.isfinite(guarded).all()) and torch.equal(guarded, clean)
    assert torch.equal(gram(xb, n=n), gram(_dev(x)))
    assert torch.equal(gram(xb, yb, n=n), guarded)  # a second run
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        other = gram(xb, yb, n=n)
    stream.synchronize()
    assert torch.equal(other, guarded)
    # Inf and NaN inside the rows propagate
    x2 = x.copy()
    x2[5, 3] = np.inf
    g = gram(_dev(x2), _dev(y)).cpu().numpy()
    assert not np.isfinite(g[3]).any() and np.isfinite(np.delete(g, 3, axis=0)).all()


def test_gram_on_real_values_stays_inside_the_derived_bound():
    """|out - out64| <= (CHUNK - 1) 2^-24 sum_r |x_ri y_rj| elementwise: the any-order fp32 bound of one chunk (exact products,
    at most CHUNK of them added in fp32); the fp64 adds across chunks are far below it.  Measured on the MI355X: the largest
    ratio to the bound is recorded in profiles/transforms_experiments.txt."""
    from sonar_amd.transforms import gram

    rng = np.random.default_rng(11)
    n, d = 2 * CHUNK + 5, 128
    x, y = _unit_rows(rng, n, d), _unit_rows(rng, n, d)
    for a, b in ((x, y), (x, None)):
        got = gram(_dev(a), None if b is None else _dev(b)).cpu().numpy()
        ratio = np.abs(got - R.gram64(a, b)) / R.gram_bound(a, b)
        print(f"gram {'cross' if b is not None else 'symmetric'} n={n} d={d}: largest |error| / bound = {ratio.max():.3e}")
        assert ratio.max() <= 1.0


def test_column_sums_are_exact():
    from sonar_amd.transforms import column_sums

    rng = np.random.default_rng(13)
    x = _unit_rows(rng, 1000, 64)
    want = np.round(x.astype(np.float64) * 2.0 ** 24).astype(np.int64)
    assert np.array_equal(want * 2.0 ** -24, x.astype(np.float64))  # every fp16 is a multiple of 2^-24
    got = column_sums(_dev(x))
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want.sum(axis=0))
    assert np.array_equal(column_sums(_dev(x), n=333).cpu().numpy(), want[:333].sum(axis=0))


# ------------------------------------------------------------------------------------------------------------ apply
@pytest.mark.parametrize("n,d_in,d_out", [(1, 64, 128), (127, 64, 128), (300, 128, 256)])
def test_apply_against_fp64(n, d_in, d_out):
    from sonar_amd.transforms import LinearTransform

    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, d_in)).astype(np.float16)
    w = (rng.standard_normal((d_out, d_in)) / np.sqrt(d_in))
    b = rng.standard_normal(d_out)
    for bias in (b, None):
        t = LinearTransform(_dev(w), None if bias is None else _dev(bias))
        w16 = t.matrix.cpu().numpy().astype(np.float64)
        assert np.array_equal(w16, w.astype(np.float32).astype(np.float16).astype(np.float64))
        b32 = np.zeros(d_out) if bias is None else t.bias.cpu().numpy().astype(np.float64)
        x64 = x.astype(np.float64)
        y64 = x64 @ w16.T + b32
        bound = 2.0 ** -11 * np.abs(y64) + d_in * 2.0 ** -24 * (np.abs(x64) @ np.abs(w16).T) + 2.0 ** -24 * np.abs(b32)
        y = t.apply(_dev(x))
        assert y.dtype == torch.float16 and tuple(y.shape) == (n, d_out)
        err = np.abs(y.cpu().numpy().astype(np.float64) - y64)
        print(f"apply n={n} d_in={d_in} d_out={d_out} bias={bias is not None}: largest |error| / bound = {(err / bound).max():.3f}")
        assert (err <= bound).all()
        # fp32 rows are rounded to fp16 first
        assert torch.equal(t.apply(_dev(x.astype(np.float32))), y)


def test_apply_bits_do_not_depend_on_the_company_and_the_tail_does_not_leak():
    from sonar_amd.transforms import LinearTransform

    rng = np.random.default_rng(17)
    n, d_in, d_out = 300, 128, 256
    x = rng.standard_normal((n, d_in)).astype(np.float16)
    t = LinearTransform(_dev(rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)), _dev(rng.standard_normal(d_out)))
    xd = _dev(x)
    y = t.apply(xd)
    for r in (0, 7, 127, 128, 255, 256, 299):  # rows of the full blocks and of the padded tail
        assert torch.equal(t.apply(xd[r:r + 1].contiguous())[0], y[r]), r
    moved = x.copy()
    moved[[290, 130, 3]] = x[[7, 7, 299]]
    ym = t.apply(_dev(moved))
    assert torch.equal(ym[290], y[7]) and torch.equal(ym[130], y[7]) and torch.equal(ym[3], y[299])
    # rows behind n in the allocation are poison: the full blocks stop at 256, the tail goes through its own zeroed copy
    big = _dev(np.concatenate([x, np.full((212, d_in), np.nan, dtype=np.float16)]))
    assert torch.equal(t.apply(big[:n]), y) and bool(torch.isfinite(y.float()).all())
    back = LinearTransform.from_state_dict(t.state_dict())
    assert torch.equal(back.apply(xd), y) and torch.equal(back.matrix64, t.matrix64)


# ------------------------------------------------------------------------------------------------------------ PCA
def test_pca_on_integer_data():
    from sonar_amd.transforms import PCA

    rng = np.random.default_rng(19)
    n, d = 3000, 256
    mix = np.linalg.qr(rng.standard_normal((d, d)))[0]
    x = np.clip(np.round((rng.standard_normal((n, d)) * np.linspace(3.0, 0.3, d)) @ mix + 1.0), -8, 8).astype(np.float16)
    c, mu = R.covariance(x)  # the Gram of integers is exact on the device, so C is this matrix up to fp64 rounding
    norm = np.linalg.norm(c, 2)
    for d_out in (128, None):  # cutting the dimension, and all of it
        t = PCA.fit(_dev(x), d_out)
        k = d_out or d
        m = t.matrix64.cpu().numpy()
        assert m.shape == (k, d) and tuple(t.matrix.shape) == (k, d) and t.matrix.dtype == torch.float16
        ev = t.explained_variance.numpy()
        assert ev.shape == (k,) and np.abs(ev - np.linalg.eigvalsh(c)[::-1][:k]).max() <= 1e-10 * norm
        assert np.all(np.diff(ev) <= 0)
        assert np.abs(m @ m.T - np.eye(k)).max() <= 1e-10
        proj = m @ c @ m.T
        assert np.abs(proj - np.diag(np.diag(proj))).max() <= 1e-9 * norm
        assert np.all(np.diff(np.diag(proj)) <= 1e-9 * norm) and np.abs(np.diag(proj) - ev).max() <= 1e-9 * norm
        lead = np.abs(m).argmax(axis=1)  # the sign rule: the largest-magnitude component of every axis is positive
        assert (m[np.arange(k), lead] > 0).all()
        assert np.abs(t.mean.cpu().numpy() - mu).max() <= 1e-14 * 8
        assert np.abs(t.bias.cpu().numpy() - (-(m @ mu)).astype(np.float32)).max() <= 2e-6
        y = t.apply(_dev(x))
        assert tuple(y.shape) == (n, k)
    u = PCA.fit(_dev(x), center=False)
    assert u.bias is None
    c0 = R.gram64(x) / (n - 1)
    assert np.abs(u.explained_variance.numpy() - np.linalg.eigvalsh(c0)[::-1]).max() <= 1e-10 * np.linalg.norm(c0, 2)


# ------------------------------------------------------------------------------------------------------------ OPQ
def test_opq_on_planted_data():
    """DESIGN.md 3.25's criterion on the device: 4096 x 128 planted rows, dsub 16, two rounds."""
    from sonar_amd.index import IVFPQIndex, ProductQuantizer
    from sonar_amd.transforms import OPQ, _relative_error
    from sonar_amd.xsim import normalize_rows

    x = _dev(R.planted(0))
    n = x.shape[0]
    opq = OPQ.fit(x, 16, n_iter=2, pq_iter=8, seed=0)
    pq = ProductQuantizer.train(x, dsub=16, n_iter=16, seed=0)  # as many Lloyd rounds as the two trainings of the fit
    plain = _relative_error(normalize_rows(x), pq.decode(pq.encode(x)), n)
    print(f"planted data on the device: plain PQ {plain:.4f}, OPQ history {[round(h, 4) for h in opq.history]}")
    assert len(opq.history) == 2 and opq.history[-1] <= 0.6 * plain
    m = opq.matrix64.cpu().numpy()
    assert np.abs(m @ m.T - np.eye(128)).max() <= 1e-10
    assert opq.bias is None and opq.dsub == 16 and tuple(opq.codebooks.shape) == (8, 256, 16)
    again = OPQ.fit(x, 16, n_iter=2, pq_iter=8, seed=0)
    if torch.equal(again.matrix, opq.matrix):
        print("OPQ: one seed gave one matrix bit for bit (the host LAPACK repeated itself)")
        assert again.history == opq.history and torch.equal(again.codebooks, opq.codebooks)
    else:
        print("OPQ: the host LAPACK did not repeat its bits; the histories agree to 1e-9")
        assert np.allclose(again.history, opq.history, rtol=0, atol=1e-9)
    # the codebooks belong to the rotated rows: an IVF-PQ index behind the rotation starts from them
    IVFPQIndex(opq.apply(x)[:8].float(), opq.codebooks)


# ------------------------------------------------------------------------------------------------------------ index
@functools.lru_cache(maxsize=None)
def _corpus():
    rng = np.random.default_rng(23)
    x = R.planted(23, 2000, 128)
    q = (x[rng.permutation(2000)[:50]].astype(np.float32) + 0.05 * rng.standard_normal((50, 128)).astype(np.float32))
    return _dev(x), _dev(q.astype(np.float16))


@pytest.mark.parametrize("kind", ["flat", "pq"])
def test_pretransform_index(kind):
    from sonar_amd.index import IVFFlatIndex, IVFPQIndex, PreTransformIndex
    from sonar_amd.mining import pair_scores
    from sonar_amd.transforms import OPQ, PCA
    from sonar_amd.xsim import normalize_rows

    x, q = _corpus()
    n, nq = x.shape[0], q.shape[0]
    if kind == "flat":
        t, cls = PCA.fit(x, 128), IVFFlatIndex
        inner = IVFFlatIndex.train(t.apply(x), 8, n_iter=4)
    else:
        t, cls = OPQ.fit(x, 16, n_iter=1, pq_iter=4), IVFPQIndex
        inner = IVFPQIndex(IVFFlatIndex.train(t.apply(x), 8, n_iter=4).centroids_normalized.float(), t.codebooks)
    wrapped = PreTransformIndex(t, inner).add(x)
    assert wrapped.ntotal == n and int(wrapped.list_sizes.sum()) == n and wrapped.dim == 128
    qt = t.apply(q)
    s, i = wrapped.search(q, k=4, nprobe=2)
    s0, i0 = inner.search(qt, k=4, nprobe=2)
    assert torch.equal(s, s0) and torch.equal(i, i0) and bool((i >= 0).all())
    assert torch.equal(wrapped.probe(q, 2), inner.probe(qt, 2))
    # refine: the cosines of the untransformed rows
    xn, qn = normalize_rows(x), normalize_rows(q)
    sr, ir = wrapped.search(q, k=4, nprobe=2, refine=xn)
    assert torch.equal(ir.sort(dim=1)[0], i.sort(dim=1)[0])
    src = torch.arange(nq, device=q.device).repeat_interleave(4)
    want = pair_scores(qn, nq, xn, n, src, ir.reshape(-1), None, None, "cosine").reshape(nq, 4)
    assert torch.equal(sr, want) and bool((sr[:, :-1] >= sr[:, 1:]).all())
    exact = (qn[:nq].double() @ xn[:n].double().t()).gather(1, ir.long())
    assert float((sr.double() - exact).abs().max()) <= 128 * 2.0 ** -24 * 2
    # a keyed search passes through
    keys = (torch.arange(n, device=x.device) % 3).to(torch.int32)
    qk = (torch.arange(nq, device=x.device) % 3).to(torch.int32)
    rf = wrapped.row_filter(keys=keys)
    sk, ik = wrapped.search(q, k=4, nprobe=2, rows=rf, query_keys=qk, match="==")
    sk0, ik0 = inner.search(qt, k=4, nprobe=2, rows=rf, query_keys=qk, match="==")
    assert torch.equal(sk, sk0) and torch.equal(ik, ik0)
    assert bool(((ik < 0) | (keys[ik.clamp(min=0).long()] == qk[:, None])).all()) and bool((ik[:, 0] >= 0).all())
    if kind == "flat":
        rr, rr0 = wrapped.range_search(q, 0.5, nprobe=2), inner.range_search(qt, 0.5, nprobe=2)
        assert all(torch.equal(a, b) for a, b in zip(rr, rr0)) and int(rr.lims[-1]) > 0
    # persistence
    back = PreTransformIndex.from_state_dict(wrapped.state_dict(), cls)
    sb, ib = back.search(q, k=4, nprobe=2)
    assert torch.equal(sb, s) and torch.equal(ib, i)
