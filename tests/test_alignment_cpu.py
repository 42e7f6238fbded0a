"""CPU: DTW alignment -- the restatement of the contract (tests/alignment_ref.py) against brute-force enumeration of all
monotone paths, the band rule, `beads`, the new C-ABI symbols and every refusal of the Python layer and of the two C
entries (sonar_amd/alignment.py, sonar_amd/csrc/align.hip).  No device is needed: the entries validate first."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import alignment_ref as R


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def _bruteforce_prefix_optimum(cost):
    """D_bf[i][j] = the least cost over ALL monotone paths (0, 0) -> (i, j), each accumulated in fp32 from the origin.
    fl32(a + c) is monotone in a, so this is what the recurrence must give, bit for bit."""
    nx, ny = cost.shape
    D = np.empty((nx, ny), dtype=np.float32)
    for i in range(nx):
        for j in range(ny):
            D[i, j] = min(R.path_cost32(cost, p) for p in R.all_monotone_paths(i + 1, j + 1))
    return D


def _tie_rule_path(D):
    """From the end cell to the predecessor with the least optimum, the first of up / left / diagonal among equals."""
    i, j = D.shape[0] - 1, D.shape[1] - 1
    path = [(i, j)]
    while (i, j) != (0, 0):
        cands = [(i + di, j + dj) for di, dj in R.MOVES.values() if i + di >= 0 and j + dj >= 0]
        best = cands[0]
        for cand in cands[1:]:
            if D[cand] < D[best]:
                best = cand
        i, j = best
        path.append(best)
    return path[::-1]


@pytest.mark.parametrize("kind", ["integer", "random"])
def test_restatement_equals_bruteforce_up_to_4x4(kind):
    rng = np.random.default_rng(11)
    tied = 0
    for nx, ny in R.shapes_up_to(4):
        for trial in range(6):
            if kind == "integer":   # three values: most cells have tied predecessors
                cost = rng.integers(0, 3, (nx, ny)).astype(np.float32)
            else:
                cost = rng.random((nx, ny)).astype(np.float32)
            path, dist = R.dtw(cost)
            D = _bruteforce_prefix_optimum(cost)
            assert dist.tobytes() == D[-1, -1].tobytes(), (nx, ny, trial)
            assert path == _tie_rule_path(D), (nx, ny, trial, cost)
            assert path[0] == (0, 0) and path[-1] == (nx - 1, ny - 1) and len(path) <= nx + ny - 1
            assert all((b[0] - a[0], b[1] - a[1]) in ((1, 0), (0, 1), (1, 1)) for a, b in zip(path, path[1:]))
            assert R.path_cost32(cost, path).tobytes() == dist.tobytes()
            for i in range(1, nx):   # inner cells whose least predecessor optimum is shared: the tie rule decides there
                for j in range(1, ny):
                    preds = [D[i - 1, j], D[i, j - 1], D[i - 1, j - 1]]
                    tied += preds.count(min(preds)) > 1
    if kind == "integer":
        assert tied > 100   # of 216 inner cells: the inputs did exercise the tie rule


def test_restatement_special_values():
    inf = np.float32(np.inf)
    assert R.dtw(np.zeros((0, 5), dtype=np.float32)) == ([], inf) and R.dtw(np.zeros((3, 0), dtype=np.float32)) == ([], inf)
    # all +inf: every comparison is a tie -> up wherever up exists, then left along the first row
    path, dist = R.dtw(np.full((3, 4), inf))
    assert dist == inf and path == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 3)]
    # a wall of +inf with one gate
    cost = np.ones((4, 4), dtype=np.float32)
    cost[2, :] = inf
    cost[2, 1] = 1
    path, dist = R.dtw(cost)
    assert (2, 1) in path and np.isfinite(dist)
    assert R.dtw(np.array([[-0.0]], dtype=np.float32))[1].tobytes() == np.float32(-0.0).tobytes()   # D[0][0] = c[0][0]


def test_band_admissibility():
    for n in (2, 5, 17):   # square: the cells within r of the diagonal
        for r in (1, 2, 4):
            adm = R.admissible_matrix(n, n, r)
            i, j = np.indices((n, n))
            assert (adm == (np.abs(i - j) <= r)).all()
    for nx, ny in ((3, 9), (9, 3), (7, 40), (1, 6), (6, 1), (1, 1)):
        for r in (1, 3):
            adm = R.admissible_matrix(nx, ny, r)
            assert adm[0, 0] and adm[-1, -1]
            assert (adm == R.admissible_matrix(ny, nx, r).T).all()
            assert all(adm[i, j] == R.admissible(i, j, nx, ny, r) for i in range(nx) for j in range(ny))
            assert (adm <= R.admissible_matrix(nx, ny, r + 1)).all()
    assert R.admissible_matrix(1, 9, 1).all() and R.admissible_matrix(9, 1, 1).all()   # a single row / column: everything
    assert R.admissible_matrix(5, 9, 0).all() and R.admissible(4, 0, 5, 9, None)
    # 3 x 9, r = 1: |8 i - 2 j| <= 8
    assert [int(R.admissible_matrix(3, 9, 1)[1].argmax()), int(R.admissible_matrix(3, 9, 1)[1].sum())] == [0, 9]
    assert R.admissible_matrix(3, 9, 1)[0].tolist() == [True] * 5 + [False] * 4
    # a radius of max(nx, ny) or more admits every cell
    assert R.admissible_matrix(13, 40, 40).all() and not R.admissible_matrix(13, 40, 11).all()


def test_radius_one_keeps_the_corners_connected_below_40():
    for nx in range(1, 40):
        for ny in range(1, 40):
            assert R.connected(nx, ny, 1), (nx, ny)
    rng = np.random.default_rng(5)
    for nx, ny in ((9, 31), (31, 9), (12, 12)):   # and the banded recurrence finds a path inside the band
        cost = rng.random((nx, ny)).astype(np.float32)
        path, dist = R.dtw(cost, 1)
        assert all(R.admissible(i, j, nx, ny, 1) for i, j in path) and np.isfinite(dist)
        assert dist >= R.dtw(cost)[1]
        assert R.dtw(cost, max(nx, ny))[0] == R.dtw(cost)[0]


def test_beads():
    from sonar_amd.alignment import beads

    path = [(0, 0), (1, 1), (1, 2), (2, 3), (3, 3), (4, 4)]
    assert beads(path) == [([0], [0]), ([1], [1, 2]), ([2, 3], [3]), ([4], [4])]
    assert beads(torch.tensor(path)) == beads(path)
    assert beads([(0, 0), (0, 1), (1, 1)]) == [([0, 1], [0, 1])]   # a staircase: n-m
    assert beads([]) == [] and beads([(0, 0)]) == [([0], [0])]
    got = beads(R.dtw(np.random.default_rng(2).random((9, 14)).astype(np.float32))[0])
    assert [i for s, _ in got for i in s] == list(range(9)) and [j for _, t in got for j in t] == list(range(14))


def test_new_symbols_declared_and_exported(lib):
    from sonar_amd import _lib

    for name in ("smi_dtw_workspace_bytes", "smi_dtw_align_cost", "smi_dtw_align"):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
    assert lib.smi_abi_version() == 7  # only functions were added


def _offs(*v):
    return (C.c_int64 * len(v))(*v)


def test_workspace_formula(lib):
    # plan 32 B a pair | line ny | codes strips * steps / 16 * 64 | skewed cost strips * steps * 64 | cost nx * ny (4 B each)
    def need(nx, ny):
        strips, steps = (nx + 63) // 64, (ny + 63 + 15) // 16 * 16
        return 32 + 4 * (ny + strips * steps // 16 * 64 + strips * steps * 64 + nx * ny)

    assert lib.smi_dtw_workspace_bytes(1, _offs(0, 130), _offs(0, 70)) == need(130, 70)
    assert lib.smi_dtw_workspace_bytes(1, _offs(0, 1), _offs(0, 1)) == need(1, 1)
    assert lib.smi_dtw_workspace_bytes(3, _offs(0, 130, 130, 131), _offs(0, 70, 75, 76)) == \
        need(130, 70) + need(1, 1) + 32 + 4 * 5   # the empty pair: its plan entry and its line
    assert lib.smi_dtw_workspace_bytes(0, _offs(0), _offs(0)) == 0
    assert lib.smi_dtw_workspace_bytes(1, _offs(5, 3), _offs(0, 4)) == 0
    assert lib.smi_dtw_workspace_bytes(1, _offs(0, 2 ** 20), _offs(0, 2 ** 20)) == 0   # beyond int32 cells
    assert lib.smi_dtw_workspace_bytes(1, None, _offs(0, 4)) == 0


def test_invalid_arguments_fail_before_any_device_call(lib):
    """Every argument is validated first: a bad call fails as SMI_ERR_INVALID_ARG / SMI_ERR_UNSUPPORTED whether or not a
    device is there; without one, only a VALID call gets as far as SMI_ERR_NO_DEVICE."""
    buf = (C.c_char * (1 << 20))()
    p = C.addressof(buf)
    xo, yo = _offs(0, 40, 40, 100), _offs(0, 50, 60, 90)
    need = lib.smi_dtw_workspace_bytes(3, xo, yo)
    assert 0 < need <= 1 << 20

    def cost(**kw):
        a = dict(c=p, n=3, xo=xo, yo=yo, xd=p, yd=p, r=0, path=p, plen=p, dist=p, ws=p, wsb=need)
        a.update(kw)
        return lib.smi_dtw_align_cost(a["c"], a["n"], a["xo"], a["yo"], a["xd"], a["yd"], a["r"], a["path"], a["plen"],
                                      a["dist"], a["ws"], a["wsb"], None)

    def align(**kw):
        a = dict(x=p, y=p, d=1024, n=3, xo=xo, yo=yo, xd=p, yd=p, r=0, path=p, plen=p, dist=p, ws=p, wsb=need)
        a.update(kw)
        return lib.smi_dtw_align(a["x"], a["y"], a["d"], a["n"], a["xo"], a["yo"], a["xd"], a["yd"], a["r"], a["path"],
                                 a["plen"], a["dist"], a["ws"], a["wsb"], None)

    for call in (cost, align):
        assert call(r=-1) == -1 and b"radius" in lib.smi_last_error()
        assert call(n=0) == -1 and call(n=-3) == -1
        assert call(n=65536) == -2 and b"65535" in lib.smi_last_error()
        assert call(xo=_offs(0, 40, 39, 100)) == -1 and b"non-decreasing" in lib.smi_last_error()
        assert call(yo=_offs(-1, 50, 60, 90)) == -1
        assert call(xo=_offs(0, 2 ** 20, 2 ** 20, 2 ** 20 + 5), yo=_offs(0, 2 ** 20, 2 ** 20, 2 ** 20 + 5)) == -2
        assert b"int32" in lib.smi_last_error()
        assert call(xo=_offs(0, 1, 1, 2), yo=_offs(0, 2 ** 30 + 1, 2 ** 30 + 1, 2 ** 30 + 2)) == -2
        assert call(xo=None) == -1 and call(yo=None) == -1 and call(xd=None) == -1 and call(yd=None) == -1
        assert call(path=None) == -1 and call(plen=None) == -1 and call(dist=None) == -1 and call(ws=None) == -1
        assert call(ws=p + 4) == -1 and b"aligned" in lib.smi_last_error()
        assert call(wsb=31) == -1 and b"smi_dtw_workspace_bytes" in lib.smi_last_error()
    assert cost(c=None) == -1
    assert cost(wsb=need - 4 * (40 * 50 + 60 * 30) - 1) == -1   # the given-cost entry needs no room for the costs ...
    assert align(wsb=need - 1) == -1                           # ... the embedding entry does
    assert align(x=None) == -1 and align(y=None) == -1
    assert align(d=96) == -2 and align(d=0) == -2 and align(d=-64) == -2
    if not torch.cuda.is_available():
        assert cost() == -3 and b"no HIP device" in lib.smi_last_error()
        assert cost(wsb=need - 4 * (40 * 50 + 60 * 30)) == -3 and align() == -3 and align(r=5, d=64) == -3


def test_python_layer_value_errors():
    """Raised before the tensors are looked at: CPU tensors (which the engine refuses later) get this far."""
    from sonar_amd import alignment as A

    x, y = torch.zeros(5, 64), torch.zeros(6, 64)
    for kw in (dict(radius=-1), dict(radius=1.5), dict(radius=True), dict(radius="3"),
               dict(x_offsets=[0, 5]), dict(y_offsets=[0, 6]),
               dict(x_offsets=[0, 3, 5], y_offsets=[0, 6]), dict(x_offsets=[0, 3, 2], y_offsets=[0, 1, 6]),
               dict(x_offsets=[-1, 5], y_offsets=[0, 6]), dict(x_offsets=[0, 6], y_offsets=[0, 6]),
               dict(x_offsets=[0], y_offsets=[0])):
        with pytest.raises(ValueError):
            A.dtw_align(x, y, **kw)
    with pytest.raises(ValueError):
        A.dtw_align(x, torch.zeros(6, 128))
    with pytest.raises(ValueError):
        A.dtw_align(torch.zeros(5), y)
    for bad in (torch.zeros(5), [torch.zeros(2, 2), torch.zeros(4)], [], [np.zeros((2, 2))]):
        with pytest.raises(ValueError):
            A.dtw_from_cost(bad)
    for r in (-2, 0.5, False):
        with pytest.raises(ValueError):
            A.dtw_from_cost(torch.zeros(3, 3), radius=r)
    # valid arguments get past the checks and stop at the engine's "no CPU path"
    for kw in (dict(), dict(radius=0), dict(radius=4), dict(x_offsets=[0, 2, 5], y_offsets=torch.tensor([0, 0, 6]))):
        with pytest.raises(RuntimeError, match="HIP device only"):
            A.dtw_align(x, y, **kw)
    with pytest.raises(RuntimeError, match="HIP device only"):
        A.dtw_from_cost([torch.zeros(3, 3), torch.zeros(0, 2)], radius=None)
    with pytest.raises(ValueError):
        A.DtwPlan([0, 5], [0, 6, 7], "cpu")
    with pytest.raises(ValueError):
        A.DtwPlan([0, 2 ** 20], [0, 2 ** 20], "cpu")
    assert math.isinf(R.dtw(np.zeros((0, 0), dtype=np.float32))[1])
