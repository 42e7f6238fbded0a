"""GPU: DTW alignment (sonar_amd/csrc/align.hip, sonar_amd/alignment.py) against the CPU restatement of its contract in
tests/alignment_ref.py.

Most of this file is exact equality: the recurrence is one fp32 add per cell and comparisons, so path, length and the
bits of the distance must equal the restatement's.  The shapes cross the 64-row strip, the 64-step phase and the 16-step
code word in both directions.  The one tolerance -- random fp16 embeddings, where the device's fp32 dot products differ
from an fp64 reference -- is derived in that test."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import alignment_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (7, 1), (16, 17), (63, 65), (64, 64), (65, 129), (130, 70), (257, 300)]
BAND_SHAPES = [(65, 129), (130, 70), (257, 300)]
KINDS = ("integer", "random", "corridor", "inf")


@functools.lru_cache(maxsize=None)
def _cost(shape, kind):
    nx, ny = shape
    rng = np.random.default_rng(1000 * nx + ny)
    if kind == "integer":      # three values: nearly every cell has tied predecessors
        c = rng.integers(0, 3, (nx, ny)).astype(np.float32)
    elif kind == "random":
        c = rng.random((nx, ny)).astype(np.float32)
    elif kind == "inf":
        c = np.full((nx, ny), np.inf, dtype=np.float32)
    else:                      # +inf walls around one random monotone corridor
        c = np.full((nx, ny), np.inf, dtype=np.float32)
        i = j = 0
        c[0, 0] = rng.random()
        while (i, j) != (nx - 1, ny - 1):
            moves = [(di, dj) for di, dj in ((1, 0), (0, 1), (1, 1)) if i + di < nx and j + dj < ny]
            di, dj = moves[rng.integers(len(moves))]
            i, j = i + di, j + dj
            c[i, j] = rng.random()
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _ref(shape, kind, radius=0):
    return R.dtw(_cost(shape, kind), radius)


def _bits(v):
    return np.float32(v).tobytes()


def _same(got, want):
    path, dist = got
    assert path.dtype == torch.int64 and path.dim() == 2 and path.shape[1] == 2
    assert [tuple(p) for p in path.tolist()] == list(want[0])
    assert _bits(dist) == _bits(want[1]), (dist, want[1])


def _dev(c):
    return torch.from_numpy(np.array(c)).cuda()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_from_cost_equals_restatement(shape):
    from sonar_amd.alignment import dtw_from_cost

    for kind in KINDS:
        got = dtw_from_cost(_dev(_cost(shape, kind)))
        _same(got, _ref(shape, kind))
        if kind == "inf":
            assert math.isinf(got[1]) and got[1] > 0
        if kind == "corridor":
            assert math.isfinite(got[1])
    # -0 at the origin: D[0][0] = c[0][0], not 0 + c[0][0]
    if shape == (1, 1):
        assert _bits(dtw_from_cost(torch.tensor([[-0.0]], device="cuda"))[1]) == _bits(-0.0)


@pytest.mark.parametrize("shape", BAND_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("radius", [1, 3, 8, "max"])
def test_band_equals_banded_restatement(shape, radius):
    from sonar_amd.alignment import dtw_from_cost

    r = max(shape) if radius == "max" else radius
    for kind in ("integer", "random"):
        got = dtw_from_cost(_dev(_cost(shape, kind)), radius=r)
        _same(got, _ref(shape, kind, r))
        if radius == "max":
            _same(got, _ref(shape, kind))
        else:
            assert all(R.admissible(i, j, shape[0], shape[1], r) for i, j in got[0].tolist())


def test_ragged_batch_equals_single_pairs():
    from sonar_amd.alignment import dtw_from_cost

    pairs = [(s, k) for n, s in enumerate(SHAPES) for k in (KINDS[n % 4], KINDS[(n + 1) % 4])]
    costs = [_dev(_cost(s, k)) for s, k in pairs]
    costs.insert(3, torch.zeros((0, 5), device="cuda"))        # an empty document among them
    costs.append(torch.zeros((4, 0), device="cuda"))
    pairs = pairs[:3] + [None] + pairs[3:] + [None]
    for radius in (None, 3):
        got = dtw_from_cost(costs, radius=radius)
        assert len(got) == len(costs)
        for c, g, pair in zip(costs, got, pairs):
            if pair is None:
                assert g[0].shape == (0, 2) and g[1] == math.inf
                continue
            alone = dtw_from_cost(c, radius=radius)
            assert torch.equal(g[0], alone[0]) and _bits(g[1]) == _bits(alone[1])
            _same(g, _ref(pair[0], pair[1], radius or 0))
    only_empty = dtw_from_cost([torch.zeros((0, 3), device="cuda")])
    assert only_empty[0][0].shape == (0, 2) and only_empty[0][1] == math.inf


def _half_rows(n, d, rng):
    """Rows with four entries of +-0.5 among the first 8 of d: unit norm, every dot product a multiple of 0.25."""
    x = np.zeros((n, d), dtype=np.float32)
    for row in x:
        row[rng.choice(8, 4, replace=False)] = rng.choice([-0.5, 0.5], 4)
    return x


@pytest.mark.parametrize("d", [64, 1024])
@pytest.mark.parametrize("shape", [(70, 131), (257, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_align_exact_embeddings(shape, d):
    from sonar_amd.alignment import dtw_align

    rng = np.random.default_rng(d + shape[0])
    x, y = _half_rows(shape[0], d, rng), _half_rows(shape[1], d, rng)
    cost = (1.0 - x.astype(np.float64) @ y.astype(np.float64).T).astype(np.float32)   # exact: multiples of 0.25
    assert len(np.unique(cost)) == 9 and (np.linalg.norm(x, axis=1) == 1).all()
    for dtype in (torch.float32, torch.float16):
        got = dtw_align(torch.from_numpy(x).to(dtype).cuda(), torch.from_numpy(y).to(dtype).cuda())
        _same(got, R.dtw(cost))
    got = dtw_align(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), radius=8)
    _same(got, R.dtw(cost, 8))


def test_align_batch_has_the_bits_of_single_pairs():
    """The summation order of a cost does not depend on the pair's place in the batch: random fp16 rows, d = 128."""
    from sonar_amd.alignment import dtw_align

    rng = np.random.default_rng(3)
    xo, yo = [0, 70, 70, 135, 136], [0, 40, 45, 175, 180]
    x = torch.from_numpy(rng.standard_normal((xo[-1], 128)).astype(np.float16)).cuda()
    y = torch.from_numpy(rng.standard_normal((yo[-1], 128)).astype(np.float16)).cuda()
    x[5] = 0                                                     # a zero row costs 1 against everything
    got = dtw_align(x, y, x_offsets=xo, y_offsets=torch.tensor(yo))
    assert len(got) == 4 and got[1][0].shape == (0, 2) and got[1][1] == math.inf
    for b in (0, 2, 3):
        alone = dtw_align(x[xo[b]:xo[b + 1]], y[yo[b]:yo[b + 1]])
        assert torch.equal(got[b][0], alone[0]) and _bits(got[b][1]) == _bits(alone[1])
        assert got[b][0][0].tolist() == [0, 0] and got[b][0][-1].tolist() == [xo[b + 1] - xo[b] - 1, yo[b + 1] - yo[b] - 1]


def _dtw64(c64):
    """The optimal DTW distance of an fp64 cost matrix, in fp64."""
    nx, ny = c64.shape
    D = np.full((nx + 1, ny + 1), np.inf)
    D[0, 0] = 0.0
    for i in range(1, nx + 1):
        for j in range(1, ny + 1):
            D[i, j] = min(D[i - 1, j], D[i, j - 1], D[i - 1, j - 1]) + c64[i - 1, j - 1]
    return D[nx, ny]


def test_align_random_embeddings_within_derived_bound():
    """Random fp16 embeddings, d = 1024, 130 x 70.  c64 = 1 - x . y of the SAME normalised fp16 rows in fp64, L = nx+ny-1.
      eps_c = d 2^-24 (1 + 2^-10)^2 + 2^-23: the fp32 dot-product bound d u |x||y| for rows of norm <= 1 + 2^-10 (fp16
              rounding of a unit row), plus the rounding of the subtraction (|1 - s| <= 2);
      every device cost is within eps_c of c64;
      the device path's cost in fp64 is at most the fp64 optimum + 2 (L eps_c + L^2 2^-23): each of the two paths has at
              most L cells, each cost off by eps_c, and L fp32 adds on partial sums <= 2 L, each off by <= 2 L 2^-24;
      the device distance is within half of that of its own path's fp64 cost.
    Derived, not tuned."""
    from sonar_amd.alignment import DtwPlan
    from sonar_amd.xsim import normalize_rows

    nx, ny, d = 130, 70, 1024
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.standard_normal((nx, d)).astype(np.float16)).cuda()
    y = torch.from_numpy((rng.standard_normal((ny, d)) + 0.3).astype(np.float16)).cuda()
    xn, yn = normalize_rows(x), normalize_rows(y)
    plan = DtwPlan([0, nx], [0, ny], x.device)
    plan.run(xn, yn)
    (path, dist), = plan.results()
    cost = plan.costs().reshape(nx, ny).cpu().numpy()
    c64 = 1.0 - xn[:nx].cpu().numpy().astype(np.float64) @ yn[:ny].cpu().numpy().astype(np.float64).T
    L = nx + ny - 1
    eps_c = d * 2.0 ** -24 * (1 + 2.0 ** -10) ** 2 + 2.0 ** -23
    slack = 2 * (L * eps_c + L * L * 2.0 ** -23)
    err_c = float(np.abs(cost - c64).max())
    cells = [tuple(p) for p in path.tolist()]
    own = R.path_cost64(c64, cells)
    best = _dtw64(c64)
    print(f"max cost error {err_c:.3e} (eps_c {eps_c:.3e}); path {own:.9f} optimum {best:.9f} distance {dist:.9f} "
          f"(slack {slack:.3e})")
    assert err_c <= eps_c
    assert cells[0] == (0, 0) and cells[-1] == (nx - 1, ny - 1) and len(cells) <= L
    assert all((b[0] - a[0], b[1] - a[1]) in ((1, 0), (0, 1), (1, 1)) for a, b in zip(cells, cells[1:]))
    assert own <= best + slack
    assert abs(dist - own) <= slack / 2
    # and the DP on the device's own costs is the restatement's, exactly
    want = R.dtw(cost)
    assert cells == want[0] and _bits(dist) == _bits(want[1])


def test_planted_alignment_is_recovered():
    """y is x with rows 10..12 merged into their mean and two rows duplicated, with small noise."""
    from sonar_amd.alignment import beads, dtw_align

    rng = np.random.default_rng(21)
    n, d = 30, 256
    x = rng.standard_normal((n, d)).astype(np.float32)
    rows, want = [], []
    for i in range(n):
        if i in (11, 12):
            want.append((i, len(rows) - 1))
            continue
        for _ in range(2 if i in (20, 25) else 1):
            want.append((i, len(rows)))
            rows.append(x[10:13].mean(0) if i == 10 else x[i])
    y = np.stack(rows) + 0.01 * rng.standard_normal((len(rows), d)).astype(np.float32)
    path, dist = dtw_align(torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.float32)).cuda())
    assert [tuple(p) for p in path.tolist()] == want
    table = beads(path)
    assert ([10, 11, 12], [10]) in table and ([20], [18, 19]) in table and ([25], [24, 25]) in table
    assert sum(len(s) == 1 and len(t) == 1 for s, t in table) == n - 5


def test_entry_is_capturable():
    """One call under graph capture replays to the same result: the entry reads nothing back."""
    from sonar_amd.alignment import DtwPlan

    shapes = [(65, 129), (7, 1), (130, 70)]
    flat = torch.cat([_dev(_cost(s, "random")).reshape(-1) for s in shapes])
    xo, yo = [0, 65, 72, 202], [0, 129, 130, 200]
    plan = DtwPlan(xo, yo, flat.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.run_cost(flat, 8)
    torch.cuda.current_stream().wait_stream(side)
    eager = plan.results()
    for s, g in zip(shapes, eager):
        _same(g, _ref(s, "random", 8))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.run_cost(flat, 8)
    plan.path.zero_()
    plan.path_len.zero_()
    plan.distance.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, plan.results()):
        assert torch.equal(a[0], b[0]) and _bits(a[1]) == _bits(b[1])
