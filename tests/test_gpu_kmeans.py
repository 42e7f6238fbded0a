"""GPU: spherical k-means (sonar_amd/csrc/kmeans.hip, sonar_amd/clustering.py) against the numpy restatement in
tests/kmeans_ref.py.

Update and finalise are exact, so they are compared for equality of bits: the sums are integers (every finite fp16 is a
multiple of 2^-24), the fp32 centroids one round to nearest even of them, the fp16 rows whatever `xsim.normalize_rows`
makes of those.  The assignment is the mining kernel's top-1, an fp32 accumulation of d products of fp16 operands with
norms <= 1: each score is within d * 2^-24 of its float64 value, so the float64 score of the label the device chose is
within 2 * d * 2^-24 of the row's best -- a condition on every row, no row excluded.  On planted data the float64 margin
between the best and the second best centroid is >= 0.1 (asserted on the CPU in tests/test_kmeans_cpu.py), three orders
of magnitude above that, so there the labels themselves must equal the planted ones."""
import functools

import numpy as np
import pytest
import torch

from tests import kmeans_ref as R

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
SENT = -77


def _np16(t):
    return t.detach().cpu().numpy().view(np.float16) if t.dtype == torch.float16 else t.detach().cpu().numpy()


def _unit_rows(rng, n, d):
    x = rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16)


def _update(x16, labels, k):
    from sonar_amd import clustering

    sums, counts = clustering.update(torch.from_numpy(x16).cuda(), torch.from_numpy(np.asarray(labels, dtype=np.int32)).cuda(), k)
    torch.cuda.synchronize()
    return sums.cpu().numpy(), counts.cpu().numpy()


def _check_update(x16, labels, k):
    sums, counts = _update(x16, labels, k)
    rs, rc = R.update(x16, labels, k)
    assert np.array_equal(counts, rc)
    assert np.array_equal(sums, rs)
    return sums, counts


# ------------------------------------------------------------------------------------------------ update
# a sampled cross of n in {1, 63, 64, 65, 255, 256, 257, 1000, 4099}, K in {1, 2, 7, 255, 256, 257, 300}, d in {64, 192, 1024};
# and K = 513: a thread of the one-block scan (csrc/bucket.hpp) owns ceil(K / 256) clusters -- one at 256, two at 257 with
# half the threads owning none, three at 513
UPDATE_SHAPES = [(1, 1, 64), (1, 300, 1024), (63, 2, 64), (63, 255, 192), (64, 7, 192), (64, 1, 1024), (65, 255, 64),
                 (65, 2, 1024), (255, 256, 192), (255, 7, 1024), (256, 257, 64), (256, 2, 192), (257, 300, 1024),
                 (257, 1, 64), (1000, 7, 1024), (1000, 256, 64), (1000, 257, 192), (4099, 1, 1024), (4099, 300, 192),
                 (4099, 255, 64), (4099, 7, 1024), (4099, 513, 64)]
PATTERNS = ("random", "sorted", "reversed", "one", "skipped")


def _labels(rng, pattern, n, k):
    lab = rng.integers(0, k, n).astype(np.int64)
    if pattern == "sorted":
        lab.sort()
    elif pattern == "reversed":
        lab = np.sort(lab)[::-1].copy()
    elif pattern == "one":
        lab[:] = k - 1
    elif pattern == "skipped":
        bad = rng.choice(np.array([-1, k, INT32_MAX, -2 ** 31]), n)
        lab = np.where(rng.random(n) < 0.3, bad, lab)
    return lab.astype(np.int32)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n,k,d", UPDATE_SHAPES)
def test_update_equals_the_integer_sums(n, k, d, pattern):
    rng = np.random.default_rng(n * 1000003 + k * 1009 + d)
    _check_update(_unit_rows(rng, n, d), _labels(rng, pattern, n, k), k)


def test_update_one_cluster_larger_than_a_work_unit():
    """Every row in one cluster, 64 times the members a work unit (SMI_KMEANS_UNIT_ROWS = clustering.UNIT_ROWS) takes: the
    cluster is summed by many units.  Rows of +1.0 give 4099 * 2^24 in every column."""
    from sonar_amd import clustering

    n, k, d = 4099, 3, 1024
    assert clustering.UNIT_ROWS == 64 and n > 64 * clustering.UNIT_ROWS
    x = np.ones((n, d), dtype=np.float16)
    sums, counts = _check_update(x, np.full(n, 1, dtype=np.int32), k)
    assert (sums[1] == 4099 * 2 ** 24).all() and (sums[0] == 0).all() and (sums[2] == 0).all()
    assert counts.tolist() == [0, 4099, 0]


def test_update_special_values():
    rng = np.random.default_rng(5)
    n, k, d = 1000, 7, 192
    labels = rng.integers(0, k, n).astype(np.int32)
    # the smallest subnormal: the integer 1
    tiny = np.full((n, d), 2.0 ** -24, dtype=np.float16)
    sums, counts = _check_update(tiny, labels, k)
    assert np.array_equal(sums, np.repeat(counts.astype(np.int64)[:, None], d, axis=1))
    # +x and -x in the same cluster cancel to a zero sum
    half = _unit_rows(rng, n // 2, d)
    x = np.concatenate([half, -half])
    lab2 = np.concatenate([labels[: n // 2], labels[: n // 2]])
    sums, counts = _check_update(x, lab2, k)
    assert (sums == 0).all() and counts.sum() == n
    # Inf and NaN elements contribute 0 there and nothing else changes
    x = _unit_rows(rng, n, d)
    clean, _ = R.update(x, labels, k)
    x[17, 3], x[17, 100] = np.inf, np.nan
    x[500, 0] = -np.inf
    sums, _ = _check_update(x, labels, k)
    diff = np.argwhere(sums != clean)
    assert {tuple(r) for r in diff.tolist()} <= {(labels[17], 3), (labels[17], 100), (labels[500], 0)}
    # the largest finite fp16 (outside what normalised rows hold, inside the contract)
    big = np.full((257, 64), 65504.0, dtype=np.float16)
    big[::2] *= -1
    _check_update(big, np.zeros(257, dtype=np.int32), 2)


def test_update_is_invariant_under_row_permutation():
    rng = np.random.default_rng(6)
    n, k, d = 4099, 37, 1024
    x, labels = _unit_rows(rng, n, d), _labels(rng, "skipped", n, k)
    a = _update(x, labels, k)
    for _ in range(2):
        p = rng.permutation(n)
        b = _update(x[p], labels[p], k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = _update(x, labels, k)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


def test_c_abi_refusals_launch_nothing_and_the_workspace_is_not_overrun():
    from sonar_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(8)
    n, k, d, guard = 1000, 7, 64, 256
    x16 = _unit_rows(rng, n, d)
    labels = _labels(rng, "skipped", n, k)
    x, lab = torch.from_numpy(x16).cuda(), torch.from_numpy(labels).cuda()
    need = int(lib.smi_kmeans_workspace_bytes(n, k, d))
    big = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = big[guard:guard + need]
    sums = torch.full((k, d), SENT, dtype=torch.int64, device="cuda")
    counts = torch.full((k,), SENT, dtype=torch.int32, device="cuda")
    c32 = torch.full((k, d), float(SENT), dtype=torch.float32, device="cuda")
    c16 = torch.full((256, d), float(SENT), dtype=torch.float16, device="cuda")
    empty = torch.full((1,), SENT, dtype=torch.int32, device="cuda")
    st = _lib.current_stream_ptr()
    P = lambda t: t.data_ptr()  # noqa: E731
    refused = [
        lib.smi_kmeans_update(P(x), P(lab), n, d, k, P(sums), P(counts), P(ws), need - 1, st),
        lib.smi_kmeans_update(P(x), P(lab), n, 96, k, P(sums), P(counts), P(ws), need, st),
        lib.smi_kmeans_update(P(x), P(lab), n, d, 0, P(sums), P(counts), P(ws), need, st),
        lib.smi_kmeans_update(None, P(lab), n, d, k, P(sums), P(counts), P(ws), need, st),
        lib.smi_kmeans_update(P(x), None, n, d, k, P(sums), P(counts), P(ws), need, st),
        lib.smi_kmeans_update(P(x), P(lab), n, d, k, None, P(counts), P(ws), need, st),
        lib.smi_kmeans_update(P(x), P(lab), n, d, k, P(sums), None, P(ws), need, st),
        lib.smi_kmeans_update(P(x), P(lab), n, d, k, P(sums), P(counts), None, need, st),
        lib.smi_kmeans_finalize(P(sums), P(counts), k, d, P(c32), P(c16), P(empty), P(ws),
                                int(lib.smi_kmeans_workspace_bytes(1, k, d)) - 1, st),
        lib.smi_kmeans_finalize(P(sums), P(counts), k, 96, P(c32), P(c16), P(empty), P(ws), need, st),
        lib.smi_kmeans_finalize(P(sums), P(counts), 0, d, P(c32), P(c16), P(empty), P(ws), need, st),
        lib.smi_kmeans_finalize(None, P(counts), k, d, P(c32), P(c16), P(empty), P(ws), need, st),
        lib.smi_kmeans_finalize(P(sums), P(counts), k, d, None, P(c16), P(empty), P(ws), need, st),
        lib.smi_kmeans_finalize(P(sums), P(counts), k, d, P(c32), None, P(empty), P(ws), need, st),
        lib.smi_kmeans_finalize(P(sums), P(counts), k, d, P(c32), P(c16), None, P(ws), need, st),
        lib.smi_kmeans_fit(P(x), n, d, k, 1, 0, P(c32), P(c16), P(lab), P(c32), P(sums), P(counts), P(c32), P(counts),
                           P(counts), P(ws), need, st),  # the workspace of update alone is too small for fit
    ]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused), refused
    assert (sums == SENT).all() and (counts == SENT).all() and (c32 == SENT).all() and (c16 == SENT).all()
    assert (empty == SENT).all() and (big == 0xA5).all()
    # the accepted call stays inside its window
    _lib.check(lib.smi_kmeans_update(P(x), P(lab), n, d, k, P(sums), P(counts), P(ws), need, st))
    torch.cuda.synchronize()
    rs, rc = R.update(x16, labels, k)
    assert np.array_equal(sums.cpu().numpy(), rs) and np.array_equal(counts.cpu().numpy(), rc)
    assert (big[:guard] == 0xA5).all() and (big[guard + need:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------ finalise
@pytest.mark.parametrize("n,k,d", [(777, 300, 1024), (1000, 7, 64), (257, 257, 192)])
def test_finalize_bits_and_kept_clusters(n, k, d):
    from sonar_amd import clustering, xsim

    rng = np.random.default_rng(k)
    x = _unit_rows(rng, n, d)
    labels = rng.integers(0, k, n).astype(np.int32)
    empty_c, zero_c = k // 2, k - 1
    labels[labels == empty_c] = 0          # a cluster without members
    labels[labels == zero_c] = 0           # a cluster whose two members cancel
    x[1], labels[0], labels[1] = -x[0], zero_c, zero_c
    sums, counts = clustering.update(torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda(), k)
    rs, rc = R.update(x, labels, k)
    assert rc[empty_c] == 0 and rc[zero_c] == 2 and (rs[zero_c] == 0).all()
    live = R.live_clusters(rs, rc)
    assert not live[empty_c] and not live[zero_c] and int((~live).sum()) >= 2

    pad = (k + 255) // 256 * 256
    prev32 = rng.standard_normal((k, d)).astype(np.float32)
    prev16 = rng.standard_normal((pad, d)).astype(np.float16)  # NOT the normalised prev32: both rows must be kept as they are
    c32, c16 = torch.from_numpy(prev32).cuda(), torch.from_numpy(prev16).cuda()
    empty = clustering.finalize(sums, counts, c32, c16)
    torch.cuda.synchronize()
    want32, want_empty = R.finalize(rs, rc, prev32)
    assert int(empty.item()) == want_empty
    got32 = c32.cpu().numpy()
    assert np.array_equal(got32.view(np.uint32), want32.view(np.uint32))
    norm = _np16(xsim.normalize_rows(c32))
    got16 = _np16(c16)
    assert np.array_equal(got16[:k][live].view(np.uint16), norm[:k][live].view(np.uint16))
    assert np.array_equal(got16[:k][~live].view(np.uint16), prev16[:k][~live].view(np.uint16))
    assert (got16[k:].view(np.uint16) == 0).all()


# ------------------------------------------------------------------------------------------------ fit
@functools.lru_cache(maxsize=None)
def _planted(n, k, d):
    return R.planted(n, k, d)  # computed once, shared, never written


def _state(km):
    torch.cuda.synchronize()
    return (km.centroids.cpu().numpy().view(np.uint32).copy(), _np16(km.centroids_normalized).view(np.uint16).copy(),
            km.labels.cpu().numpy().copy(), km.scores.cpu().numpy().view(np.uint32).copy(), km.counts.cpu().numpy().copy(),
            km.sums.cpu().numpy().copy())


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def _same_history(a, b):
    # the objectives are compared as bits
    return (np.array_equal(np.array(a["objective"]).view(np.uint64), np.array(b["objective"]).view(np.uint64))
            and a["moved"] == b["moved"] and a["empty"] == b["empty"])


@pytest.mark.parametrize("n,k,d", R.PLANTED_SHAPES)
def test_fit_recovers_planted_clusters_and_is_reproducible(n, k, d):
    from sonar_amd.clustering import SphericalKMeans

    T = 4
    x, truth, init = _planted(n, k, d)
    xd, initd = torch.from_numpy(x).cuda(), torch.from_numpy(init).cuda()
    stepped = SphericalKMeans(k, n_iter=0).fit(xd, init=initd)
    assert np.array_equal(stepped.labels.cpu().numpy(), truth)
    for _ in range(T):
        labels, scores = stepped.step()
        assert np.array_equal(labels.cpu().numpy(), truth)  # every round
        assert labels is stepped.labels and scores is stepped.scores
    whole = SphericalKMeans(k, n_iter=T).fit(xd, init=initd)
    again = SphericalKMeans(k, n_iter=T).fit(xd, init=initd)
    assert _same(_state(whole), _state(stepped)) and _same_history(whole.history, stepped.history)
    assert _same(_state(whole), _state(again)) and _same_history(whole.history, again.history)
    h = whole.history
    assert len(h["objective"]) == T + 1 and h["moved"] == [n] + [0] * T and h["empty"] == [0] * T
    assert np.array_equal(whole.counts.cpu().numpy(), np.bincount(truth, minlength=k))
    # the recorded objective is an fp64 sum of the scores: any order is within (n - 1) u sum|s| of the exact sum
    s = whole.scores.cpu().numpy().astype(np.float64)
    assert abs(h["objective"][-1] - s.sum()) <= (n - 1) * 2.0 ** -53 * np.abs(s).sum()
    assert h["objective"][1] > h["objective"][0]
    # every objective of the stepped run, against the scores of that round
    replay = SphericalKMeans(k, n_iter=0).fit(xd, init=initd)
    for t in range(T + 1):
        if t:
            replay.step()
        s = replay.scores.cpu().numpy().astype(np.float64)
        assert abs(h["objective"][t] - s.sum()) <= (n - 1) * 2.0 ** -53 * np.abs(s).sum(), t


def test_fit_duplicate_centroid_stays_empty_and_single_cluster():
    from sonar_amd.clustering import SphericalKMeans

    x, truth, init = _planted(600, 5, 64)
    dup = np.concatenate([init, init[:1]])  # centroid 5 == centroid 0: ties go to the lower index
    km = SphericalKMeans(6, n_iter=0).fit(torch.from_numpy(x).cuda(), init=torch.from_numpy(dup).cuda())
    assert np.array_equal(km.labels.cpu().numpy(), truth)  # no row goes to the duplicate
    km.step()  # the first update finds it empty and keeps it where it was
    assert km.history["empty"] == [1] and int(km.counts[5]) == 0 and int(km.counts.sum()) == 600
    assert np.array_equal(km.centroids[5].cpu().numpy(), dup[5].astype(np.float32))
    assert not np.array_equal(km.centroids[0].cpu().numpy(), dup[0].astype(np.float32))
    one = SphericalKMeans(1, n_iter=2).fit(torch.from_numpy(x).cuda())
    assert (one.labels == 0).all() and int(one.counts[0]) == 600 and one.history["moved"] == [600, 0, 0]


def test_fit_row_initialisation_follows_the_seed():
    from sonar_amd.clustering import SphericalKMeans, init_rows

    x, _, _ = _planted(600, 5, 64)
    xd = torch.from_numpy(x).cuda()
    a = SphericalKMeans(5, n_iter=0, seed=3).fit(xd)
    rows = init_rows(600, 5, 3).numpy()
    assert np.array_equal(a.centroids.cpu().numpy(), x[rows].astype(np.float32))
    b = SphericalKMeans(5, n_iter=2, seed=3).fit(xd)
    c = SphericalKMeans(5, n_iter=2, seed=3).fit(xd)
    assert _same(_state(b), _state(c))


def test_fit_on_unclustered_data_decision_by_decision():
    """Random directions, K = 37: no margin to lean on.  Every round: (a) the float64 score of each device label against the
    device's own fp16 centroids is within 2 d 2^-24 of the row's best -- all rows, the bound is a condition; (b) given
    those labels, update and finalise are exact."""
    from sonar_amd import xsim
    from sonar_amd.clustering import SphericalKMeans

    n, k, d, T = 1000, 37, 1024, 5
    rng = np.random.default_rng(11)
    # Gaussian points of an 8-dimensional subspace: full-rank Gaussian rows at d = 1024 are so far apart that every row
    # stays with the centroid it contributed to and nothing moves after the first round
    xd = torch.from_numpy((rng.standard_normal((n, 8)) @ rng.standard_normal((8, d))).astype(np.float32)).cuda()
    xn = xsim.normalize_rows(xd)
    xn16 = _np16(xn)[:n]
    x64 = xn16.astype(np.float64)
    km = SphericalKMeans(k, n_iter=0, seed=2).fit_normalized(xn, n)
    bound = 2 * d * 2.0 ** -24
    moved = []
    for t in range(T + 1):
        labels = km.labels.cpu().numpy()
        c32 = km.centroids.cpu().numpy()
        c16 = _np16(km.centroids_normalized)
        s = x64 @ c16.astype(np.float64).T
        chosen = s[np.arange(n), labels]
        worst = float((s.max(axis=1) - chosen).max())
        print(f"round {t}: worst float64 gap of a chosen label {worst:.3e} (bound {bound:.3e})")
        assert worst <= bound
        assert np.abs(km.scores.cpu().numpy().astype(np.float64) - chosen).max() <= bound / 2
        if t == T:
            break
        km.step()
        rs, rc = R.update(xn16, labels, k)
        assert np.array_equal(km.sums.cpu().numpy(), rs) and np.array_equal(km.counts.cpu().numpy(), rc)
        want32, want_empty = R.finalize(rs, rc, c32)
        assert np.array_equal(km.centroids.cpu().numpy().view(np.uint32), want32.view(np.uint32))
        assert np.array_equal(_np16(km.centroids_normalized).view(np.uint16),
                              _np16(xsim.normalize_rows(km.centroids))[:k].view(np.uint16))
        assert km.history["empty"][t] == want_empty
        moved.append(int((km.labels.cpu().numpy() != labels).sum()))
    print("rows that moved per round:", moved)
    assert km.history["moved"] == [n] + moved and min(moved) > 0  # every round made decisions


# ------------------------------------------------------------------------------------------------ predict
def test_predict_is_the_existing_topk():
    from sonar_amd import xsim
    from sonar_amd.clustering import SphericalKMeans

    n, k, d = 1000, 37, 1024
    rng = np.random.default_rng(12)
    xd = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float16)).cuda()
    km = SphericalKMeans(k, n_iter=3, seed=1).fit(xd)
    lab, sc = km.predict(xd, 1)
    assert lab.shape == (n,) and torch.equal(lab, km.labels) and torch.equal(sc, km.scores)
    lab4, sc4 = km.predict(xd, 4)
    xn = xsim.normalize_rows(xd)
    cn = xsim.normalize_rows(km.centroids)
    want_s, want_i = xsim.topk_normalized(xn, n, cn, k, 4)
    assert lab4.shape == (n, 4) and torch.equal(lab4, want_i) and torch.equal(sc4, want_s)
    assert torch.equal(lab4[:, 0], km.labels)
    with pytest.raises(ValueError, match="dim"):
        km.predict(xd[:, :64].contiguous())
