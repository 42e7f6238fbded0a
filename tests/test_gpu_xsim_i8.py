"""GPU: the int8 brute-force top-k (sonar_amd/csrc/xsim_i8.hip, sonar_amd.xsim.topk_int8*, mining precision="int8") against
the numpy restatement in tests/xsim_i8_ref.py.

The integer sums are exact and the rest of a score is three float32 roundings in a fixed order, so scores and ids are compared
for equality of bits on ANY data unless said otherwise.  The rows given to the kernel are fp16 matrices padded with zero rows to
a multiple of 256, as normalize_rows lays them out; most tests build them in numpy so that the restatement sees the same bits."""
import functools

import numpy as np
import pytest
import torch

from tests import ivf_i8_ref as Q
from tests import ivf_ref as R
from tests import xsim_i8_ref as X
from tests.test_gpu_ivf import _dev
from tests.test_gpu_ivf_i8 import _in_total_order, _saturated, _unit_rows

pytestmark = pytest.mark.gpu


def _padded(a16):
    a16 = np.asarray(a16, dtype=np.float16)
    out = np.zeros(((len(a16) + 255) // 256 * 256, a16.shape[1]), dtype=np.float16)
    out[: len(a16)] = a16
    return _dev(out)


def _run(x, y, k, off=0, xd=None, yd=None):
    from sonar_amd import xsim

    xd = _padded(x) if xd is None else xd
    yd = _padded(y) if yd is None else yd
    score, idx = xsim.topk_int8_normalized(xd, len(x), yd, len(y), k, refine=False, y_index_offset=off)
    torch.cuda.synchronize()
    assert score.dtype == torch.float32 and idx.dtype == torch.int32 and score.shape == idx.shape == (len(x), k)
    return score.cpu().numpy(), idx.cpu().numpy()


def _check(x, y, ks, off=0, s=None):
    """Scores and ids of every row equal the restatement bit for bit, for every k of ks.  x / y: any fp16 rows."""
    s = Q.scores(x, y) if s is None else s
    xd, yd = _padded(x), _padded(y)
    for k in ks:
        got_s, got_i = _run(x, y, k, off, xd, yd)
        want_s, want_i = X.topk(x, y, k, off, s=s)
        bad = np.flatnonzero((got_i != want_i).any(axis=1) | (got_s.view(np.int32) != want_s.view(np.int32)).any(axis=1))
        assert len(bad) == 0, (k, bad[:5], got_i[bad[:2]], want_i[bad[:2]], got_s[bad[:2]], want_s[bad[:2]])
    return s


# ------------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("ny", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("nx", [1, 255, 256, 257])
def test_tile_and_pad_edges(nx, ny):
    rng = np.random.default_rng(nx * 1009 + ny)
    _check(_unit_rows(rng, nx, 64), _unit_rows(rng, ny, 64), (1, 2, 4, 8))


def test_a_pad_row_never_wins_when_every_score_is_negative():
    rng = np.random.default_rng(2)
    x = np.abs(_unit_rows(rng, 257, 64))
    y = -np.abs(_unit_rows(rng, 300, 64))  # 212 pad rows behind them, each scoring +0
    s = _check(x, y, (1, 3, 8))
    assert (s < 0).all()
    got_s, got_i = _run(x, y[:5], 8)  # fewer rows than k: the pad rows do not fill the list either
    assert (got_s[:, :5] < 0).all() and np.isneginf(got_s[:, 5:]).all() and (got_i[:, 5:] == -1).all()


@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("ny", [2307, 4352])  # 10 tiles: 5 chunks of 2, 3 empty; 17 tiles: 5 chunks of 3, one of 2, 2 empty
def test_chunk_edges(ny, d):
    rng = np.random.default_rng(ny + d)
    _check(_unit_rows(rng, 40, d), _unit_rows(rng, ny, d), (1, 4))


@pytest.mark.parametrize("ny", [2307, 4352])
def test_empty_chunks_leave_empty_lists(ny):
    """The partial lists in the workspace, read back: a chunk without tiles holds (-inf, 0x7fffffff) in every entry, whatever
    the workspace held before (here: small positive floats that would beat the all-negative scores)."""
    from sonar_amd import _lib, index

    lib = _lib.load()
    rng = np.random.default_rng(ny)
    nx, d, k = 40, 64, 4
    x, y = np.abs(_unit_rows(rng, nx, d)), -np.abs(_unit_rows(rng, ny, d))
    (xc, xs), (yc, ys) = index.encode_rows_int8(_padded(x)), index.encode_rows_int8(_padded(y))
    nbytes = lib.smi_xsim_workspace_bytes(nx, ny, k, d // 2)
    assert nbytes == X.workspace_bytes(nx, ny, k, d)  # from 2048 padded y rows on: an exact fit
    ws = torch.full((nbytes,), 0x11, dtype=torch.uint8, device="cuda")
    idx = torch.empty((nx, k), dtype=torch.int32, device="cuda")
    score = torch.empty((nx, k), dtype=torch.float32, device="cuda")
    _lib.check(lib.smi_xsim_topk_i8(xc.data_ptr(), xs.data_ptr(), nx, yc.data_ptr(), ys.data_ptr(), ny, d, k, 0, idx.data_ptr(),
                                    score.data_ptr(), ws.data_ptr(), nbytes, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    want_s, want_i = X.topk(x, y, k)
    assert np.array_equal(score.cpu().numpy(), want_s) and np.array_equal(idx.cpu().numpy(), want_i)
    nty = (ny + 255) // 256
    tpc = (nty + 7) // 8
    used = (nty + tpc - 1) // tpc
    assert used < 8
    lists = 8 * 256 * k
    ps = ws[: lists * 4].view(torch.float32).reshape(8, 256, k).cpu().numpy()
    pi = ws[lists * 4: lists * 8].view(torch.int32).reshape(8, 256, k).cpu().numpy()
    assert np.isneginf(ps[used:]).all() and (pi[used:] == 0x7FFFFFFF).all()
    assert np.isfinite(ps[:used, :nx]).all() and (pi[:used, :nx] < ny).all()


@pytest.mark.parametrize("d", [64, 128, 192, 1024])  # slices per tile: 1, 2, 3 (shorter than the 4-slot ring), 16
def test_every_slice_shape(d):
    rng = np.random.default_rng(d)
    _check(_unit_rows(rng, 130, d), _unit_rows(rng, 700, d), (1, 5))


@pytest.mark.parametrize("ny", [3, 300])
def test_every_k(ny):
    rng = np.random.default_rng(ny)
    x, y = _unit_rows(rng, 70, 64), _unit_rows(rng, ny, 64)
    _check(x, y, range(1, 9))
    if ny < 8:
        got_s, got_i = _run(x, y, 8)
        assert np.isneginf(got_s[:, ny:]).all() and (got_i[:, ny:] == -1).all() and (got_i[:, :ny] >= 0).all()


# The fp16 and the int8 kernel are two instantiations of one tile walk (csrc/xsim_walk.hpp).  On operands from {-1, 0, 1} -- fp16
# rows for one, the same values as int8 codes with every scale exactly 1.0 for the other -- a score is a small integer, exact in
# fp32 sums and in int32 sums times 1.0 alike, so the two passes must return the same bits, those of the stable-sorted fp64
# reference.  300 x 513: three chunks of one tile, the last tile one valid row; 257 x 2305: chunks of two tiles, three empty.
_WALK_PAIR = [(300, 513, 128, k, True) for k in range(1, 9)] + [(257, 2305, 64, k, False) for k in (1, 4)]


@pytest.mark.parametrize("nx,ny,d,k,plant", _WALK_PAIR)
def test_the_fp16_and_the_int8_walk_agree_bit_for_bit(nx, ny, d, k, plant):
    from sonar_amd import xsim
    from tests.test_gpu_xsim_kernels import _assert_same, _exact_case, _first_k, _mine, _pad256

    x, y, vals, idx = _exact_case(nx, ny, d, plant)
    # a condition on the INPUTS (reference alone): the k-th and (k+1)-th scores tie often enough that the tie-break matters
    share = (vals[:, k - 1] == vals[:, k]).double().mean().item()
    print(f"{nx} x {ny} x {d}, k = {k}: k-th / (k+1)-th tie in {share:.1%} of the rows")
    assert share >= 0.1, share
    want_s, want_i = _first_k(vals, idx, k)
    f_s, f_i = _mine(x, y, k)
    enc = [(_pad256(t).to(torch.int8).cuda(), torch.ones((t.shape[0] + 255) // 256 * 256, dtype=torch.float32, device="cuda"))
           for t in (x, y)]
    assert all(torch.equal(c.cpu().half()[: t.shape[0]], t) for (c, _), t in zip(enc, (x, y)))  # the codes ARE the fp16 values
    q_s, q_i = xsim.topk_int8_normalized(None, nx, None, ny, k, refine=False, x_enc=enc[0], y_enc=enc[1])
    torch.cuda.synchronize()
    q_s, q_i = q_s.cpu(), q_i.cpu().long()
    for what, s, i in (("fp16", f_s, f_i), ("int8", q_s, q_i)):
        _assert_same(i, want_i, f"{what} indices")
        _assert_same(s.view(torch.int32), want_s.view(torch.int32), f"{what} score bits")
    _assert_same(q_i, f_i, "int8 against fp16 indices")
    _assert_same(q_s.view(torch.int32), f_s.view(torch.int32), "int8 against fp16 score bits")


def test_ties_go_by_index_within_a_tile_across_tiles_and_across_chunks():
    rng = np.random.default_rng(5)
    x, y = _unit_rows(rng, 20, 64), _unit_rows(rng, 2307, 64)
    copies = [5, 200, 300, 700, 1500, 2306]  # tile 0 twice, tile 1 (the same chunk), tiles 2 and 5 (other chunks), the last row
    for i in copies:
        y[i] = x[1]
    y[1000] = y[10] = x[2]
    s = _check(x, y, (1, 2, 6, 8), off=1000)
    got_s, got_i = _run(x, y, 8, off=1000)
    assert got_i[1][:6].tolist() == [1000 + i for i in copies] and len(set(got_s[1][:6].tolist())) == 1
    assert got_s[1][6] < got_s[1][5] and got_i[2][:2].tolist() == [1010, 2000]
    assert _in_total_order(got_s, got_i) is None
    _check(x, y, (8,), off=0, s=s)
    # ties the last rounding makes: a zero query row scores +0 against every row -- the lowest indices
    x[0] = 0
    got_s, got_i = _run(x, y, 8, off=7)
    assert got_i[0].tolist() == list(range(7, 15)) and (got_s[0].view(np.int32) == 0).all()


def test_saturated_rows_and_sums_float32_cannot_hold():
    rng = np.random.default_rng(13)
    d = 2048
    x, y = _saturated(rng, 66, d), _saturated(rng, 300, d)
    x[:, : d * 3 // 4] = 0.5  # three quarters agree: the sums stay above 2^24 for most pairs
    y[:, : d * 3 // 4] = 0.5
    y[::2, -1] = 0.25  # code 64: odd sums, so (float)acc rounds
    y[7], y[290], y[33], x[0] = 0.5, 0.5, -0.5, 0.5  # acc = +-127^2 d: the largest there is, twice (a tie) and negated
    acc = Q.int_dots(Q.encode(x)[0], Q.encode(y)[0])
    rounds = acc != acc.astype(np.float32).astype(np.int64)
    assert rounds[1:, 0:7:2].mean() > 0.9 and acc[0, 7] == acc[0, 290] == -acc[0, 33] == 127 * 127 * d > 2 ** 24
    _check(x, y, (1, 8))
    got_s, got_i = _run(x, y, 2)
    assert got_i[0].tolist() == [7, 290]


@pytest.mark.parametrize("d", [64, 192])
def test_edge_rows_and_equality_with_the_index(d):
    """Zero rows, -0 elements, subnormals, 65504 among real rows, on both sides: the restatement's bits, and the bits and ids a
    one-list int8 IVF index returns for the same rows at nprobe = 1."""
    from sonar_amd import index

    rng = np.random.default_rng(d)
    x, y = _unit_rows(rng, 70, d), _unit_rows(rng, 600, d)
    edges = Q.edge_rows(rng, d)
    y[: len(edges)], x[: len(edges)] = edges, edges[::-1]
    y[300:300 + len(edges)] = edges
    s = _check(x, y, (1, 5, 8))
    assert not np.signbit(s[s == 0]).any()  # no -0 from encoded rows: a zero row's sums are 0
    yd = _dev(y)
    storage = index.build_lists_int8(yd, torch.zeros(len(y), dtype=torch.int32, device="cuda"), 1)
    codes, scales, ids, off, _ = storage
    probes = torch.zeros((len(x), 1), dtype=torch.int32, device="cuda")
    for k in (1, 5, 8):
        want_s, want_i = index.search_lists_int8(_dev(x), probes, codes, scales, ids, off, k)
        torch.cuda.synchronize()
        got_s, got_i = _run(x, y, k)
        assert np.array_equal(got_s.view(np.int32), want_s.cpu().numpy().view(np.int32)), k
        assert np.array_equal(got_i, want_i.cpu().numpy()), k


# ------------------------------------------------------------------------------------------------------ 2. planted data
@functools.lru_cache(maxsize=None)
def _planted(d):
    """tests/ivf_ref.planted(1100, 16, d, 300) through the device's normalisation: the padded fp16 matrices of corpus and queries
    on the device, their rows as numpy (what the engine encodes), the restated scores and the float64 ones."""
    from sonar_amd import xsim

    x, _, _, q, target = R.planted(1100, 16, d, 300)
    xn, qn = xsim.normalize_rows(_dev(x)), xsim.normalize_rows(_dev(q))
    torch.cuda.synchronize()
    xh, qh = xn[: len(x)].cpu().numpy(), qn[: len(q)].cpu().numpy()
    return x, q, target, xn, qn, xh, qh, Q.scores(qh, xh), R.scores64(qh, xh)


@pytest.mark.parametrize("d", [64, 1024])
def test_planted_data_bits_bound_and_neighbours(d):
    from sonar_amd import xsim

    x, q, target, xn, qn, xh, qh, s, s64 = _planted(d)
    assert not xn[len(x):].any() and not qn[len(q):].any()  # zero pad rows
    k = 4
    score, idx = xsim.topk_int8_normalized(qn, len(q), xn, len(x), k, refine=False)
    torch.cuda.synchronize()
    got_s, got_i = score.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
    want_s, want_i = X.topk(qh, xh, k, s=s)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s.view(np.int32), want_s.view(np.int32))
    assert np.array_equal(got_i[:, 0], target)
    (cq, sq), (cx, sx) = Q.encode(qh), Q.encode(xh)
    b = Q.bound(Q.l1(cq)[:, None], sq[:, None], Q.l1(cx)[None, :], sx[None, :], d, s)
    rows = np.arange(len(q))[:, None]
    err = np.abs(got_s.astype(np.float64) - s64[rows, got_i])
    print(f"d={d}: max |score - fp64| = {err.max():.3e}, max error / bound = {(err / b[rows, got_i]).max():.3f}")
    assert (err <= b[rows, got_i]).all()
    # the whole call from raw rows, and an encoding made once
    from sonar_amd import index

    s2, i2 = xsim.topk_int8(_dev(q), _dev(x), k, refine=False)
    enc = index.encode_rows_int8(xn)
    s3, i3 = xsim.topk_int8_normalized(qn, len(q), None, len(x), k, refine=False, y_enc=enc)
    assert torch.equal(s2, score) and torch.equal(i2, idx) and torch.equal(s3, score) and torch.equal(i3, idx)


@pytest.mark.parametrize("d", [64, 1024])
def test_invariance_alone_in_a_batch_permuted_and_between_runs(d):
    from sonar_amd import xsim

    x, q, _, xn, qn, xh, qh, *_ = _planted(d)
    rng = np.random.default_rng(d)
    k, nq, n = 4, len(q), len(x)
    run = lambda a, na, b, nb: xsim.topk_int8_normalized(a, na, b, nb, k, refine=False)  # noqa: E731
    score, idx = run(qn, nq, xn, n)
    again = run(qn, nq, xn, n)
    assert torch.equal(score, again[0]) and torch.equal(idx, again[1])  # two runs
    for r in (0, 1, 255, 256, 299):  # alone
        one = run(_padded(qh[r: r + 1]), 1, xn, n)
        assert torch.equal(one[0][0], score[r]) and torch.equal(one[1][0], idx[r]), r
    perm = rng.permutation(nq)  # the queries in another order
    ps, pi = run(_padded(qh[perm]), nq, xn, n)
    dperm = _dev(perm)
    assert torch.equal(ps, score[dperm]) and torch.equal(pi, idx[dperm])
    cperm = rng.permutation(n)  # the corpus in another order: the same rows and bits, modulo the id map (no ties here)
    s2, i2 = run(qn, nq, _padded(xh[cperm]), n)
    assert torch.equal(s2, score) and np.array_equal(cperm[i2.cpu().numpy()], idx.cpu().numpy())


def test_equality_with_a_one_list_int8_index_searched_at_nprobe_1():
    """The class path: IVFInt8Index with one list, add() and search(nprobe=1) normalising the raw rows themselves, returns the
    bits and ids of the brute-force pass over the same normalised rows."""
    from sonar_amd import xsim
    from sonar_amd.index import IVFInt8Index

    x, q, target, xn, qn, *_ = _planted(64)
    xd, qd = _dev(x), _dev(q)
    ix = IVFInt8Index(xd[:1]).add(xd, labels=torch.zeros(len(x), dtype=torch.int32, device="cuda"))
    for k in (1, 4, 8):
        want_s, want_i = ix.search(qd, k=k, nprobe=1)
        got_s, got_i = xsim.topk_int8_normalized(qn, len(q), xn, len(x), k, refine=False)
        torch.cuda.synchronize()
        assert torch.equal(got_s.view(torch.int32), want_s.view(torch.int32)) and torch.equal(got_i, want_i), k
    assert np.array_equal(got_i[:, 0].cpu().numpy(), target)


# ------------------------------------------------------------------------------------------------------ 3. refine, mining
@pytest.mark.parametrize("d", [64, 1024])
def test_refine_is_the_pair_cosine_of_the_restated_candidates_in_total_order(d):
    from sonar_amd import mining, xsim

    x, q, target, xn, qn, xh, qh, s, _ = _planted(d)
    nq, n = len(q), len(x)
    for k, cand in ((4, 8), (1, 8), (3, 5), (8, 8)):
        score, idx = xsim.topk_int8_normalized(qn, nq, xn, n, k, candidates=cand)
        torch.cuda.synchronize()
        assert score.dtype == torch.float32 and idx.dtype == torch.int32 and score.shape == idx.shape == (nq, k)
        src = torch.arange(nq, device="cuda").repeat_interleave(k)
        cos = mining.pair_scores(qn, nq, xn, n, src, idx.reshape(-1).long(), None, None, "cosine").reshape(nq, k)
        assert torch.equal(cos, score)  # bit for bit the cosines of the returned ids
        assert _in_total_order(score.cpu().numpy(), idx.cpu().numpy()) is None
        # the candidates are the restated int8 top-`cand`, re-ordered by their device cosines
        _, cand_i = X.topk(qh, xh, cand, s=s)
        csrc = torch.arange(nq, device="cuda").repeat_interleave(cand)
        ccos = mining.pair_scores(qn, nq, xn, n, csrc, _dev(cand_i.reshape(-1)), None, None, "cosine").reshape(nq, cand)
        want_s, want_i = X.refine(cand_i, ccos.cpu().numpy(), k)
        assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(score.cpu().numpy().view(np.int32), want_s.view(np.int32))
    s4, i4 = xsim.topk_int8_normalized(qn, nq, xn, n, 4, candidates=8, y_index_offset=500)
    fs, fi = xsim.topk_normalized(qn, nq, xn, n, 4)
    assert np.array_equal(np.sort(i4.cpu().numpy() - 500, axis=1), np.sort(fi.cpu().numpy(), axis=1))  # the fp16 top-4, as sets
    assert np.array_equal(i4[:, 0].cpu().numpy() - 500, target)
    s5, i5 = xsim.topk_int8(_dev(q), _dev(x), 4)
    assert torch.equal(s5, s4) and torch.equal(i5 + 500, i4)
    # fewer rows than candidates: (-inf, -1) last
    s6, i6 = xsim.topk_int8_normalized(qn, nq, _padded(xh[:3]), 3, 2, candidates=8)
    s7, i7 = xsim.topk_int8_normalized(qn, nq, _padded(xh[:3]), 3, 4, candidates=4, y_index_offset=9)
    assert (i6.cpu().numpy() >= 0).all() and (i7[:, 3] == -1).all() and torch.isneginf(s7[:, 3]).all()
    assert (i7[:, :3] >= 9).all() and torch.equal(i6 + 9, i7[:, :2]) and torch.equal(s6, s7[:, :2])


@pytest.mark.parametrize("retrieval", ["fwd", "intersect", "max"])
def test_mining_int8_mines_the_planted_pairs(retrieval):
    from sonar_amd import mining

    x, q, target, *_ = _planted(64)
    xd, qd = _dev(x), _dev(q)
    out = {}
    for precision in ("fp16", "int8"):
        src, trg, score = mining.mine_bitexts(qd, xd, retrieval=retrieval, margin="ratio", k=4, threshold=None, precision=precision)
        torch.cuda.synchronize()
        out[precision] = (src.cpu().numpy(), trg.cpu().numpy(), score.cpu().numpy())
    # every query has a planted neighbour and takes part in exactly that pair.  Margin scores are not compared bit for bit:
    # the neighbour means of the two precisions come from different arithmetic.
    for precision, (src, trg, score) in out.items():
        order = np.argsort(src, kind="stable")
        assert np.array_equal(src[order], np.arange(len(q))) and np.array_equal(trg[order], target), precision
        assert score.min() > 1.10, (precision, score.min())
    # a threshold in the planted gap: by tests/mining_ref.py in float64 on this data the planted pairs score 1.121 .. 1.243,
    # the best candidate of a corpus row without a query 1.027 at most
    for precision in ("fp16", "int8"):
        src, trg, score = mining.mine_bitexts(qd, xd, retrieval=retrieval, margin="ratio", k=4, threshold=1.07, precision=precision)
        src, trg = src.cpu().numpy(), trg.cpu().numpy()
        order = np.argsort(src, kind="stable")
        assert np.array_equal(src[order], np.arange(len(q))) and np.array_equal(trg[order], target), precision
    # bwd: every corpus row with its best query; above the threshold only the planted pairs are left
    src, trg, score = mining.mine_bitexts(qd, xd, retrieval="bwd", margin="ratio", k=4, threshold=1.07, precision="int8")
    order = np.argsort(src.cpu().numpy(), kind="stable")
    assert np.array_equal(src.cpu().numpy()[order], np.arange(len(q))) and np.array_equal(trg.cpu().numpy()[order], target)


def test_xsim_error_int8_on_aligned_planted_rows():
    from sonar_amd import xsim

    x, q, target, *_ = _planted(64)
    xd, qd = _dev(x[target]), _dev(q)  # aligned: q[i] <-> x[target[i]]
    for margin in ("cosine", "ratio"):
        e16, p16 = xsim.xsim_error(qd, xd, margin=margin)
        e8, p8 = xsim.xsim_error(qd, xd, margin=margin, precision="int8")
        assert e16 == e8 == 0.0 and torch.equal(p16, p8)


def test_graph_capture_replays_the_eager_result():
    from sonar_amd import index, xsim

    x, q, target, xn, qn, *_ = _planted(64)
    enc_x, enc_q = index.encode_rows_int8(xn), index.encode_rows_int8(qn)
    call = lambda: xsim.topk_int8_normalized(qn, len(q), xn, len(x), 4, x_enc=enc_q, y_enc=enc_x)  # noqa: E731
    eager = call()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm up off the default stream, as torch's capture asks
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    out[0].fill_(0), out[1].fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0].view(torch.int32), eager[0].view(torch.int32)) and torch.equal(out[1], eager[1])
    assert np.array_equal(out[1][:, 0].cpu().numpy(), target)
