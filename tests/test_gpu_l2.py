"""GPU: squared-Euclidean / inner-product search and Euclidean k-means (sonar_amd/csrc/l2.hip, kmeans.hip, ivf.hip;
sonar_amd.xsim.topk_l2, clustering.KMeans, index.IVFFlatL2Index) against the restatement in tests/l2_ref.py.

On the integer data of l2_ref (x entries in {-3 .. 3}, y the same with a per-row share of zeros) every dot product, half norm
and score is a multiple of 1/2 below 2^24, exact in fp32 whatever the order of the accumulation: scores and ids are compared
for equality of bits on every row (tests/test_l2_cpu.py asserts the conditions on the data: the L2 order differs from the
inner-product and the cosine order in most rows, and ties between adjacent positions are common).  On real-valued rows the
fp32 accumulation of the MFMA tile is not restated; there a score is held to the bound l2_ref.score_bound of float64."""
import functools

import numpy as np
import pytest
import torch

from tests import l2_ref as L

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared cases are read-only)


def _np16(t):
    return t.detach().cpu().numpy().view(np.float16) if t.dtype == torch.float16 else t.detach().cpu().numpy()


def _padded(a16):
    return _dev(L.prepare(np.asarray(a16, dtype=np.float16))[0])


def _bias(b, ny):
    out = np.zeros(L.pad256(ny), dtype=np.float32)
    out[:ny] = np.asarray(b, dtype=np.float32)[:ny]
    return _dev(out)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _run(x, y, bias, k, off=0, xd=None, yd=None):
    from sonar_amd import xsim

    xd = _padded(x) if xd is None else xd
    yd = _padded(y) if yd is None else yd
    score, idx = xsim.topk_bias_prepared(xd, len(x), yd, len(y), _bias(bias, len(y)), k, off)
    torch.cuda.synchronize()
    assert score.dtype == torch.float32 and idx.dtype == torch.int32 and score.shape == idx.shape == (len(x), k)
    return score.cpu().numpy(), idx.cpu().numpy()


def _check(x, y, bias, ks, off=0):
    """Scores and ids of every row equal the restatement bit for bit, for every k of ks (rows with exact scores)."""
    s = L.scores(x, y, bias)
    xd, yd = _padded(x), _padded(y)
    for k in ks:
        got_s, got_i = _run(x, y, bias, k, off, xd, yd)
        want_s, want_i = L.topk_of(s, k, off)
        bad = np.flatnonzero((got_i != want_i).any(axis=1) | (_bits(got_s) != _bits(want_s)).any(axis=1))
        assert len(bad) == 0, (k, bad[:5], got_i[bad[:2]], want_i[bad[:2]], got_s[bad[:2]], want_s[bad[:2]])


# ------------------------------------------------------------------------------------------------------ 1. smi_l2_prepare
@pytest.mark.parametrize("rows", [1, 255, 257])
@pytest.mark.parametrize("d", [64, 192, 1024])
@pytest.mark.parametrize("src", ["fp16", "fp32"])
def test_prepare_rows_and_half_norms_bit_for_bit(src, d, rows):
    from sonar_amd import xsim

    rng = np.random.default_rng(rows * 31 + d)
    for kind in ("integer", "real"):
        a = L.int_rows(rng, rows, d).astype(np.float32) if kind == "integer" else (
            rng.standard_normal((rows, d)) * rng.uniform(0.01, 30.0, (rows, 1))).astype(np.float32)
        if rows > 2:
            a[1] = 0.0
        a = a.astype(np.float16) if src == "fp16" else a
        rows16, h = xsim.prepare_rows(_dev(a))
        torch.cuda.synchronize()
        want16, want_h = L.prepare(a)  # the mirrored order: bit for bit on real rows too
        assert rows16.dtype == torch.float16 and h.dtype == torch.float32 and tuple(h.shape) == (L.pad256(rows),)
        assert _same_bits(_np16(rows16), want16), kind
        assert _same_bits(h.cpu().numpy(), want_h), kind
        assert (_bits(_np16(rows16))[rows:] == 0).all() and (_bits(h.cpu().numpy())[rows:] == 0).all()


# ---------------------------------------------------------------------------------------------------------- 2. smi_l2_topk
@functools.lru_cache(maxsize=None)
def _exact_case(nx, ny, d):
    rng = np.random.default_rng(nx * 7 + ny + d)  # (the seeds of tests/test_l2_cpu.py)
    x, y = L.int_rows(rng, nx, d), L.sparse_int_rows(rng, ny, d)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


# k is every value in 1 .. 8 over the set
@pytest.mark.parametrize("nx,ny,d,ks", [(257, 256, 128, (1, 3, 8)), (513, 2305, 64, (2, 5, 7)), (300, 2305, 1024, (1, 4, 6))])
def test_l2_scores_and_ids_equal_the_restatement(nx, ny, d, ks):
    x, y = _exact_case(nx, ny, d)
    _check(x, y, -L.half_norms(y), ks)


def test_one_row_against_one_row():
    x, y = np.full((1, 64), 2.0, dtype=np.float16), np.full((1, 64), -1.0, dtype=np.float16)
    _check(x, y, -L.half_norms(y), (1, 8))
    got_s, got_i = _run(x, y, -L.half_norms(y), 2)
    assert got_s[0, 0] == -128.0 - 32.0 and got_i[0].tolist() == [0, -1] and np.isneginf(got_s[0, 1])


def test_zero_rows_and_copies_across_lanes_waves_tiles_and_chunks():
    """300 x 513: three chunks of one tile, the last tile one valid row.  Five copies of one y row sit in different lane
    groups (rows 3, 21), another column wave (100), another tile (300) and the last chunk's only valid row (512); x rows 0 .. 4
    ARE that row, so their five nearest tie at distance 0 and come by id.  A zero x row scores -h_y everywhere (the shortest y
    rows win); a zero y row has bias -0 and scores +0 against everything."""
    x, y = (a.copy() for a in _exact_case(300, 513, 64))
    copies = [3, 21, 100, 300, 512]
    y[copies] = y[7]
    y[40] = 0
    x[:5] = y[7]
    x[9] = 0
    bias = -L.half_norms(y)
    assert np.signbit(bias[40]) and bias[40] == 0
    _check(x, y, bias, range(1, 9))
    got_s, got_i = _run(x, y, bias, 8)
    assert got_i[0, :6].tolist() == sorted(copies + [7]) and (got_s[0, :6] == got_s[0, 0]).all()
    want = L.topk_l2(x, y, 8)
    assert (want[0][:5, :6] == 0).all()  # distance 0 to the copies
    zero = got_s[:, :][got_i == 40]
    assert len(zero) and not np.signbit(zero).any() and (zero == 0).all()  # a zero score is +0


@pytest.mark.parametrize("ny", [1, 15, 16, 17, 40])
def test_few_rows_fill_and_index_offset(ny):
    x, y = _exact_case(300, 513, 64)
    y = y[:ny]
    bias = -L.half_norms(y)
    _check(x, y, bias, (3, 8), off=1000)
    got_s, got_i = _run(x, y, bias, 8, off=1000)
    assert (got_i[:, : min(ny, 8)] >= 1000).all() and (got_i[:, : min(ny, 8)] < 1000 + ny).all()
    assert np.isneginf(got_s[:, ny:]).all() and (got_i[:, ny:] == -1).all()


def test_a_pad_row_never_enters_whatever_its_bias():
    """Every valid score is negative; the pad rows of y score 0 + their bias, here +1000: they must not enter, and k above
    the number of rows is fill."""
    from sonar_amd import xsim

    x, y = _exact_case(300, 513, 64)
    y = y[:300]
    bias = np.full(512, 1000.0, dtype=np.float32)
    bias[:300] = -L.half_norms(y) - 5000.0
    score, idx = xsim.topk_bias_prepared(_padded(x), 300, _padded(y), 300, _dev(bias), 8)
    torch.cuda.synchronize()
    want_s, want_i = L.topk(x, y, bias, 8)
    assert _same_bits(score.cpu().numpy(), want_s) and np.array_equal(idx.cpu().numpy(), want_i)
    assert (want_s < 0).all()


def _real_rows(rng, n, d):
    return (rng.standard_normal((n, d)) * rng.uniform(0.2, 3.0, (n, 1))).astype(np.float16)


def test_zero_bias_is_topk_normalized_bit_for_bit_on_real_rows():
    from sonar_amd import xsim

    rng = np.random.default_rng(3)
    for nx, ny, d, k in [(300, 2305, 64, 8), (130, 700, 192, 1), (257, 513, 1024, 4)]:
        x, y = _real_rows(rng, nx, d), _real_rows(rng, ny, d)
        xd, yd = _padded(x), _padded(y)
        got = xsim.topk_bias_prepared(xd, nx, yd, ny, torch.zeros(L.pad256(ny), device="cuda"), k)
        want = xsim.topk_normalized(xd, nx, yd, ny, k)
        torch.cuda.synchronize()
        assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
        ip = xsim.topk_ip(_dev(x), _dev(y), k)  # the inner product on rows as they are: the same pass
        assert torch.equal(ip[1], want[1]) and torch.equal(ip[0].view(torch.int32), want[0].view(torch.int32))


@pytest.mark.parametrize("nx,ny,d,k", [(300, 2305, 64, 8), (257, 700, 1024, 3)])
def test_real_rows_within_the_bound_of_float64(nx, ny, d, k):
    """Every returned score is within d 2^-23 sum|x_c||y_c| + 2^-24 (|s| + h) of its float64 value, and no row left out beats
    the last one returned by more than the two bounds: every row, nothing excused."""
    rng = np.random.default_rng(nx + d)
    x, y = _real_rows(rng, nx, d), _real_rows(rng, ny, d)
    hy = L.half_norms(y)
    got_s, got_i = _run(x, y, -hy, k)
    s64 = L.dots64(x, y) - hy.astype(np.float64)[None, :]
    bound = L.score_bound(x, y, s64, hy)
    rows = np.arange(nx)[:, None]
    assert (got_i >= 0).all() and all(len(set(r)) == k for r in got_i.tolist())
    err = np.abs(got_s.astype(np.float64) - s64[rows, got_i])
    print(f"{nx} x {ny} x {d}: worst |score - float64| / bound = {(err / bound[rows, got_i]).max():.3f}")
    assert (err <= bound[rows, got_i]).all()
    assert (got_s[:, :-1] >= got_s[:, 1:]).all()
    last = got_i[:, -1]
    out = np.ones((nx, ny), dtype=bool)
    out[rows, got_i] = False
    slack = bound + bound[np.arange(nx), last][:, None]
    assert (np.where(out, s64 - s64[np.arange(nx), last][:, None] - slack, -1.0) <= 0).all()


def test_two_calls_and_a_subset_of_the_rows_give_the_same_bits():
    rng = np.random.default_rng(5)
    x, y = _real_rows(rng, 513, 192), _real_rows(rng, 1100, 192)
    bias = -L.half_norms(y)
    a = _run(x, y, bias, 5)
    b = _run(x, y, bias, 5)
    assert _same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    pick = np.array([0, 3, 255, 256, 300, 512])
    c = _run(x[pick], y, bias, 5)
    assert _same_bits(c[0], a[0][pick]) and np.array_equal(c[1], a[1][pick])
    one = _run(x[511:512], y, bias, 5)
    assert _same_bits(one[0], a[0][511:512]) and np.array_equal(one[1], a[1][511:512])


def test_one_graph_capture_is_replayed():
    from sonar_amd import _lib

    lib = _lib.load()
    x, y = _exact_case(300, 513, 64)
    nx, ny, d, k = 300, 513, 64, 4
    xd, yd = _padded(x), _padded(y)
    bias = _bias(-L.half_norms(y), ny)
    need = int(lib.smi_l2_topk_ws_bytes(nx, ny, k, d))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    idx = torch.full((nx, k), -7, dtype=torch.int32, device="cuda")
    score = torch.full((nx, k), -7.0, dtype=torch.float32, device="cuda")

    def call():
        _lib.check(lib.smi_l2_topk(xd.data_ptr(), nx, yd.data_ptr(), ny, d, k, 0, bias.data_ptr(), idx.data_ptr(),
                                   score.data_ptr(), ws.data_ptr(), need, _lib.current_stream_ptr()))

    call()  # (the kernels' attributes are set outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    want_s, want_i = L.topk(x, y, -L.half_norms(y), k)
    for _ in range(2):
        idx.fill_(-7)
        score.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(score.cpu().numpy(), want_s) and np.array_equal(idx.cpu().numpy(), want_i)


def test_refusals_launch_nothing_and_the_workspace_is_not_overrun():
    from sonar_amd import _lib

    lib = _lib.load()
    x, y = _exact_case(300, 513, 64)
    nx, ny, d, k, guard, SENT = 300, 513, 64, 4, 256, -77
    xd, yd = _padded(x), _padded(y)
    bias = _bias(-L.half_norms(y), ny)
    need = int(lib.smi_l2_topk_ws_bytes(nx, ny, k, d))
    big = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = big[guard:guard + need]
    idx = torch.full((nx, k), SENT, dtype=torch.int32, device="cuda")
    score = torch.full((nx, k), float(SENT), dtype=torch.float32, device="cuda")
    st = _lib.current_stream_ptr()
    P = lambda t: t.data_ptr()  # noqa: E731
    refused = [
        lib.smi_l2_topk(P(xd), nx, P(yd), ny, d, k, 0, P(bias), P(idx), P(score), P(ws), need - 1, st),
        lib.smi_l2_topk(P(xd), nx, P(yd), ny, d, k, 0, None, P(idx), P(score), P(ws), need, st),
        lib.smi_l2_topk(P(xd), nx, P(yd), ny, d, k, 0, P(bias) + 4, P(idx), P(score), P(ws), need, st),
        lib.smi_l2_topk(P(xd), nx, P(yd), ny, d, 9, 0, P(bias), P(idx), P(score), P(ws), need, st),
        lib.smi_l2_topk(P(xd), nx, P(yd), ny, 96, k, 0, P(bias), P(idx), P(score), P(ws), need, st),
        lib.smi_l2_topk(P(xd), nx, P(yd), ny, d, k, 0, P(bias), P(idx), P(score), None, need, st),
    ]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused), refused
    assert (idx == SENT).all() and (score == SENT).all() and (big == 0xA5).all()
    _lib.check(lib.smi_l2_topk(P(xd), nx, P(yd), ny, d, k, 0, P(bias), P(idx), P(score), P(ws), need, st))
    torch.cuda.synchronize()
    want_s, want_i = L.topk(x, y, -L.half_norms(y), k)
    assert _same_bits(score.cpu().numpy(), want_s) and np.array_equal(idx.cpu().numpy(), want_i)
    assert (big[:guard] == 0xA5).all() and (big[guard + need:] == 0xA5).all()


def test_topk_l2_distances_and_the_planted_nearest_set():
    """xsim.topk_l2 end to end.  Integer data: distances and ids equal the restatement, non-decreasing, fill (+inf, -1).
    Planted real data (l2_ref.planted; the gap between consecutive candidates is asserted above twice the bound in
    tests/test_l2_cpu.py): the four nearest are the planted ones, in order."""
    from sonar_amd import xsim

    x, y = _exact_case(257, 256, 128)
    for src in (x, x.astype(np.float32)):
        dist, idx = xsim.topk_l2(_dev(src), _dev(y), 8)
        torch.cuda.synchronize()
        want_d, want_i, _ = L.topk_l2(x, y, 8)
        assert _same_bits(dist.cpu().numpy(), want_d) and np.array_equal(idx.cpu().numpy(), want_i)
        assert (dist[:, :-1] <= dist[:, 1:]).all() and (dist >= 0).all()
    exact = ((x.astype(np.float64)[:, None, :] - y.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    assert np.array_equal(np.take_along_axis(exact, want_i, axis=1), want_d.astype(np.float64))  # they ARE the distances
    dist, idx = xsim.topk_l2(_dev(x), _dev(y[:3]), 5)
    assert torch.isposinf(dist[:, 3:]).all() and (idx[:, 3:] == -1).all() and torch.isfinite(dist[:, :3]).all()
    px, py, truth = L.planted()
    dist, idx = xsim.topk_l2(_dev(px), _dev(py), truth.shape[1])
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), truth)
    assert (dist[:, :-1] <= dist[:, 1:]).all()
    d64 = ((px.astype(np.float64)[:, None, :] - py.astype(np.float64)[truth]) ** 2).sum(axis=2)
    assert np.abs(dist.cpu().numpy() - d64).max() <= 2 * L.planted_gap(px, py, truth)[1] + 2.0 ** -22 * float(L.half_norms(px).max())


# ------------------------------------------------------------------------------------------------------------ 3. k-means
# The update and the finalise are exact given the labels: sums, counts, both centroid matrices, the half norms and the empty
# count are compared for equality of bits, and so are the records (the objective is the float64 sum of the device's scores in
# the restated order).  The FIRST assignment is against integer rows (the initial centroids are rows of x), so its scores are
# exact and labels and scores equal the restatement's bits too.  From the first update on the centroids are means, real-valued:
# the fp32 accumulation of the MFMA tile is not restated, so a later assignment is held to (a) the bits smi_l2_topk returns
# for the same rows, centroids and bias, and (b) float64, decision by decision: the float64 score of the label the device
# chose is within the two scores' bounds (l2_ref.score_bound) of the row's best -- every row, nothing excused.
def _km_state(km):
    torch.cuda.synchronize()
    return (km.centroids.cpu().numpy().view(np.uint32).copy(), _bits(_np16(km.centroids_f16)).copy(),
            km.centroid_half_norms.cpu().numpy().view(np.uint32).copy(), km.labels.cpu().numpy().copy(),
            km.scores.cpu().numpy().view(np.uint32).copy(), km.counts.cpu().numpy().copy(), km.sums.cpu().numpy().copy())


def _same_history(a, b):
    return (np.array_equal(np.array(a["objective"]).view(np.uint64), np.array(b["objective"]).view(np.uint64))
            and a["moved"] == b["moved"] and a["empty"] == b["empty"] and a["inertia"] == b["inertia"])


def _check_assignment(km, x, xd, hx_d):
    """The current labels / scores of km against its own centroids: (a) and (b) above.  Returns (labels, scores)."""
    from sonar_amd import xsim

    n, k = len(x), km.n_clusters
    labels, sc = km.labels.cpu().numpy(), km.scores.cpu().numpy()
    c16, h = _np16(km.centroids_f16), km.centroid_half_norms.cpu().numpy()
    ts, ti = xsim.topk_bias_prepared(xd, n, km._c16, k, km._ch.neg(), 1)
    assert np.array_equal(ti.cpu().numpy()[:, 0], labels) and _same_bits(ts.cpu().numpy()[:, 0], sc)
    s64 = L.dots64(x, c16) - h.astype(np.float64)[None, :]
    bound = L.score_bound(x, c16, s64, h)
    rows = np.arange(n)
    best = s64.argmax(axis=1)
    gap = s64[rows, best] - s64[rows, labels]
    assert (gap <= bound[rows, best] + bound[rows, labels]).all(), float(gap.max())
    assert (np.abs(sc.astype(np.float64) - s64[rows, labels]) <= bound[rows, labels]).all()
    return labels, sc


@pytest.mark.parametrize("n,k,d", [(1000, 7, 64), (3000, 40, 192)])
def test_kmeans_rounds_against_the_restatement(n, k, d):
    from sonar_amd import xsim
    from sonar_amd.clustering import KMeans

    T = 5
    rng = np.random.default_rng(n + k)
    # integer rows around k integer centres: clusters that move for a few rounds
    centres = rng.integers(-3, 4, (k, d))
    x = np.clip(centres[rng.integers(0, k, n)] + rng.integers(-2, 3, (n, d)) * (rng.random((n, d)) < 0.5), -6, 6).astype(np.float16)
    init = x[rng.permutation(n)[:k]].astype(np.float32)
    xd, hx_d = xsim.prepare_rows(_dev(x))
    km = KMeans(k, n_iter=0).fit(_dev(x), init=_dev(init))
    first = L.fit(x, init, 0)[0]  # exact: labels, scores and records equal the restatement
    labels, sc = _check_assignment(km, x, xd, hx_d)
    assert np.array_equal(labels, first["labels"]) and _same_bits(sc, first["scores"])
    h = km.history
    assert h["objective"] == [first["objective"]] and h["moved"] == [n] and h["empty"] == []
    assert h["inertia"] == [L.inertia(L.half_norms(x), first["objective"], n)]
    c32, c16, ch = init, init.astype(np.float16), L.half_norms(init.astype(np.float16))
    padded = np.zeros((L.pad256(k), d), dtype=np.float16)
    assert _same_bits(_np16(km.centroids_f16), c16) and _same_bits(km.centroid_half_norms.cpu().numpy(), ch)
    moved = []
    for t in range(1, T + 1):
        km.step()
        sums, counts = L.KR.update(x, labels, k)
        padded[:k] = c16
        c32, c16, ch, empty = L.finalize(sums, counts, c32, padded, ch)
        assert np.array_equal(km.sums.cpu().numpy(), sums) and np.array_equal(km.counts.cpu().numpy(), counts)
        assert _same_bits(km.centroids.cpu().numpy(), c32) and _same_bits(_np16(km.centroids_f16), c16)
        assert _same_bits(km.centroid_half_norms.cpu().numpy(), ch)
        assert (_bits(_np16(km._c16))[k:] == 0).all() and (km._ch[k:] == 0).all()
        new, sc = _check_assignment(km, x, xd, hx_d)
        h = km.history
        assert h["empty"][t - 1] == empty and h["moved"][t] == int((new != labels).sum())
        assert np.float64(h["objective"][t]).view(np.uint64) == np.float64(L.objective_sum(sc)).view(np.uint64)
        moved.append(h["moved"][t])
        labels = new
    print(f"{n} x {k} x {d}: rows that moved per round {moved}; inertia {[round(v, 1) for v in h['inertia']]}")
    assert moved[0] > 0 and h["inertia"][1] < h["inertia"][0]
    # the inertia IS the sum of the squared distances to the assigned fp16 centroids
    diff = x.astype(np.float64) - c16.astype(np.float64)[labels]
    assert abs(h["inertia"][-1] - (diff ** 2).sum()) <= 1e-5 * (diff ** 2).sum()
    # fit(0) + T x fit(resume) == fit(T), and a second run gives the same bits
    whole = KMeans(k, n_iter=T).fit(_dev(x), init=_dev(init))
    prepared = KMeans(k, n_iter=T).fit_prepared(xd, hx_d, n, init=_dev(init))
    for other in (whole, prepared):
        assert all(np.array_equal(a, b) for a, b in zip(_km_state(km), _km_state(other)))
        assert _same_history(km.history, other.history)


def test_kmeans_an_empty_cluster_and_a_duplicate_centroid():
    from sonar_amd.clustering import KMeans

    rng = np.random.default_rng(9)
    x = L.int_rows(rng, 600, 64)
    init = np.concatenate([x[:4], x[:1]]).astype(np.float32)  # centroid 4 == centroid 0: ties go to the lower index
    km = KMeans(5, n_iter=0).fit(_dev(x), init=_dev(init))
    want = L.fit(x, init, 0)[0]
    assert np.array_equal(km.labels.cpu().numpy(), want["labels"]) and (want["labels"] != 4).all()
    km.step()
    assert km.history["empty"] == [1] and int(km.counts[4]) == 0 and int(km.counts.sum()) == 600
    assert np.array_equal(km.centroids[4].cpu().numpy(), init[4])                     # all three kept
    assert _same_bits(_np16(km.centroids_f16)[4], init[4].astype(np.float16))
    assert _same_bits(km.centroid_half_norms.cpu().numpy()[4:5], L.half_norms(init[4:5].astype(np.float16)))
    assert not np.array_equal(km.centroids[0].cpu().numpy(), init[0])
    one = KMeans(1, n_iter=2).fit(_dev(x))
    assert (one.labels == 0).all() and int(one.counts[0]) == 600 and one.history["moved"] == [600, 0, 0]
    assert np.array_equal(one.centroids.cpu().numpy()[0].astype(np.float64),
                          (x.astype(np.float64).sum(axis=0) / 600).astype(np.float32).astype(np.float64))


def test_kmeans_separates_two_clusters_on_one_ray():
    """Distances 1 and 3 along one direction: every label is recovered (the spherical fit cannot: tests/test_l2_cpu.py)."""
    from sonar_amd import xsim
    from sonar_amd.clustering import KMeans

    x, truth, init = L.ray_clusters()
    km = KMeans(2, n_iter=3).fit(_dev(x), init=_dev(init))
    assert np.array_equal(km.labels.cpu().numpy(), truth)
    assert km.history["moved"][-1] == 0 and km.history["empty"] == [0, 0, 0]
    # predict is topk_l2 against the centroids
    lab, dist = km.predict(_dev(x))
    want_d, want_i = xsim.topk_l2(_dev(x), km.centroids_f16, 1)
    assert torch.equal(lab, km.labels) and torch.equal(lab, want_i[:, 0]) and torch.equal(dist, want_d[:, 0])
    lab2, dist2 = km.predict(_dev(x), 2)
    assert lab2.shape == (len(x), 2) and torch.equal(lab2[:, 0], km.labels) and (dist2[:, 0] <= dist2[:, 1]).all()


# -------------------------------------------------------------------------------------------------------------- 4. index
@functools.lru_cache(maxsize=None)
def _index_case(n, nq, d, n_lists):
    rng = np.random.default_rng(n + nq + d + n_lists)
    y, q = L.sparse_int_rows(rng, n, d), L.int_rows(rng, nq, d)
    centroids = L.int_rows(rng, n_lists, d)
    labels = L.assign(y, centroids, L.half_norms(centroids))[0]
    for a in (y, q, centroids, labels):
        a.setflags(write=False)
    return y, q, centroids, labels


def _check_search(ix, q, y, labels, probes, k, visible=None, rows=None):
    dist, idx = ix.search(_dev(q), k, probes.shape[1], probes=_dev(probes.astype(np.int32)), rows=rows)
    torch.cuda.synchronize()
    want_d, want_i, _ = L.search(q, y, labels, probes, k, visible)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int32
    assert _same_bits(dist.cpu().numpy(), want_d) and np.array_equal(idx.cpu().numpy(), want_i)
    return want_d, want_i


@pytest.mark.parametrize("nq", [40, 300])  # units of 64 pairs, and of 128 (nq * nprobe >= 256 lists)
def test_index_over_all_lists_is_topk_l2(nq):
    from sonar_amd import xsim
    from sonar_amd.index import IVFFlatL2Index

    y, q, centroids, labels = _index_case(1500, nq, 64, 8)
    ix = IVFFlatL2Index(_dev(centroids)).add(_dev(y))
    assert np.array_equal(np.bincount(labels, minlength=8), ix.list_sizes.cpu().numpy()) and ix.ntotal == 1500
    for k in (1, 5, 8):
        dist, idx = ix.search(_dev(q), k, 8)  # probes by the index: all 8 lists
        brute = xsim.topk_l2(_dev(q), _dev(y), k)
        want_d, want_i, _ = L.topk_l2(q, y, k)
        assert torch.equal(idx, brute[1]) and torch.equal(dist.view(torch.int32), brute[0].view(torch.int32))
        assert _same_bits(dist.cpu().numpy(), want_d) and np.array_equal(idx.cpu().numpy(), want_i)


@pytest.mark.parametrize("nq,d", [(40, 64), (400, 64), (70, 192)])  # 12 lists: units of 64 below 3072 pairs, of 128 from there on
def test_index_probes_masks_and_entries_that_name_no_list(nq, d):
    from sonar_amd.index import IVFFlatL2Index

    y, q, centroids, labels = _index_case(1100, nq, d, 12)
    ix = IVFFlatL2Index(_dev(centroids)).add(_dev(y))
    rng = np.random.default_rng(nq)
    own = ix.probe(_dev(q), 8).cpu().numpy()
    want_probe = L.topk(q, centroids, -L.half_norms(centroids), 8)[1]
    assert np.array_equal(own, want_probe)
    _check_search(ix, q, y, labels, own, 8)
    dist, idx = ix.search(_dev(q), 8, 8)
    want_d, want_i, _ = L.search(q, y, labels, own, 8)
    assert _same_bits(dist.cpu().numpy(), want_d) and np.array_equal(idx.cpu().numpy(), want_i)
    probes = np.stack([rng.permutation(12)[:4] for _ in range(nq)])
    probes[::3, 1] = -1          # entries that name no list
    probes[1::3, 2] = 12 + 5
    probes[5] = [-1, 99, -7, 12]  # a query that probes nothing
    for k in (1, 4, 8):
        want_d, want_i = _check_search(ix, q, y, labels, probes, k)
    assert (want_i[5] == -1).all() and np.isposinf(want_d[5]).all()
    visible = rng.random(1100) < 0.4
    rows = ix.row_filter(mask=_dev(visible))
    want_d, want_i = _check_search(ix, q, y, labels, probes, 8, visible, rows)
    assert visible[want_i[want_i >= 0]].all() and (want_i == -1).any()


def test_index_lists_of_three_rows_and_given_labels():
    from sonar_amd.index import IVFFlatL2Index

    y, q, centroids, _ = _index_case(1100, 40, 64, 12)
    y = y[:36]
    labels = (np.arange(36) % 12).astype(np.int32)  # three rows per list, whatever the centroids say
    ix = IVFFlatL2Index(_dev(centroids)).add(_dev(y), labels=_dev(labels))
    assert (ix.list_sizes == 3).all()
    probes = np.stack([np.roll(np.arange(12), i)[:8] for i in range(40)])
    want_d, want_i = _check_search(ix, q, y, labels, probes, 8)
    _check_search(ix, q, y, labels, probes[:, :2], 8)  # 6 candidates: two fill entries
    assert (L.search(q, y, labels, probes[:, :2], 8)[1][:, 6:] == -1).all()


def test_index_state_dict_round_trip_and_one_capture():
    from sonar_amd.index import IVFFlatIndex, IVFFlatL2Index

    y, q, centroids, labels = _index_case(1100, 70, 192, 12)
    ix = IVFFlatL2Index(_dev(centroids)).add(_dev(y))
    state = ix.state_dict()
    assert {"centroids", "offsets", "sizes", "rows", "bias", "ids", "metric_l2"} == set(state)
    used = int(state["offsets"][12])
    assert state["rows"].shape == (used, 192) and state["bias"].shape == (used,) and used % 16 == 0
    ids, bias = state["ids"].cpu().numpy(), state["bias"].cpu().numpy()
    want_bias = np.where(ids >= 0, -L.half_norms(y)[np.maximum(ids, 0)], np.float32(0.0))
    assert _same_bits(bias, want_bias.astype(np.float32))
    again = IVFFlatL2Index.from_state_dict(state)
    qd = _dev(q)
    a, b = ix.search(qd, 8, 4), again.search(qd, 8, 4)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    other = IVFFlatL2Index(_dev(centroids))
    other.load_state_dict(state)
    c = other.search(qd, 8, 4)
    assert torch.equal(a[1], c[1]) and torch.equal(a[0].view(torch.int32), c[0].view(torch.int32))
    with pytest.raises(ValueError, match="IVFFlatL2Index"):
        IVFFlatIndex.from_state_dict(state)
    # one capture of search with given probes
    probes = ix.probe(qd, 4)
    eager = ix.search(qd, 8, probes=probes)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ix.search(qd, 8, probes=probes)  # warm-up: the one-time attribute calls
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ix.search(qd, 8, probes=probes)
    out[0].fill_(0), out[1].fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[1], eager[1]) and torch.equal(out[0].view(torch.int32), eager[0].view(torch.int32))
    assert torch.equal(eager[1], a[1])


def test_index_trains_its_own_quantiser():
    """train -> add -> search end to end on real rows: the nearest row over all lists is the brute-force nearest row."""
    from sonar_amd import xsim
    from sonar_amd.index import IVFFlatL2Index

    px, py, truth = L.planted()
    ix = IVFFlatL2Index.train(_dev(py), 6, n_iter=3).add(_dev(py))
    dist, idx = ix.search(_dev(px), 4, 6)
    brute = xsim.topk_l2(_dev(px), _dev(py), 4)
    assert np.array_equal(idx.cpu().numpy(), truth) and torch.equal(idx, brute[1])
    # (two kernels, two fp32 accumulations of real-valued rows: each within the bound of float64)
    assert (dist - brute[0]).abs().max().item() <= 4 * L.planted_gap(px, py, truth)[1] + 2.0 ** -21 * float(L.half_norms(px).max())
