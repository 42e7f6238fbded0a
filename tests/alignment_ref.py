"""CPU restatement of the DTW alignment contract (include/sonar_mi355.h: smi_dtw_align_cost), loop for
loop, in numpy fp32.  Not pinned to the fastdtw package (it is not installed next to this engine): the tie order is the
one its pure-Python `__dtw` is believed to use.

Recurrence.  For a pair with nx, ny >= 1 rows and cost c[i][j] (fp32):
  D[0][0] = c[0][0];
  D[i][j] = fl32(min(D[i-1][j], D[i][j-1], D[i-1][j-1]) + c[i][j]) over the predecessors that exist and are admissible.
  All arithmetic is fp32, one add per cell; the minimum is taken over the predecessors' D BEFORE the add.
Ties.  The first predecessor in the order up (i-1, j), left (i, j-1), diagonal (i-1, j-1): a later candidate replaces an
  earlier one only if it is strictly less.
Special values.  +inf costs are allowed (a forbidden cell); NaN costs are outside the contract.
Result.  The path from (0, 0) to (nx-1, ny-1) in ascending order, nx + ny - 1 entries or fewer, and D[nx-1][ny-1].  An
  empty side gives path length 0 and distance +inf.
Band.  radius 0 / None: the full matrix.  r >= 1: cell (i, j) is admissible iff
  |i (ny-1) - j (nx-1)| <= r max(nx-1, ny-1, 1)   (exact integers); inadmissible cells behave as D = +inf.
Cost from embeddings.  Rows are fp16, normalised; c[i][j] = fl32(1 - s), s the fp32-accumulated dot product in ascending k.
"""
import itertools
import math

import numpy as np

UP, LEFT, DIAG = 0, 1, 2
MOVES = {UP: (-1, 0), LEFT: (0, -1), DIAG: (-1, -1)}


def admissible(i, j, nx, ny, radius):
    if not radius:
        return True
    return abs(i * (ny - 1) - j * (nx - 1)) <= radius * max(nx - 1, ny - 1, 1)


def admissible_matrix(nx, ny, radius):
    """admissible() for every cell at once (int64; exact far beyond the shapes the tests use)."""
    i = np.arange(nx, dtype=np.int64)[:, None]
    j = np.arange(ny, dtype=np.int64)[None, :]
    if not radius:
        return np.ones((nx, ny), dtype=bool)
    return np.abs(i * (ny - 1) - j * (nx - 1)) <= radius * max(nx - 1, ny - 1, 1)


def dtw(cost, radius=None):
    """-> (path [(i, j), ...], distance np.float32) of the contract above."""
    c = np.asarray(cost, dtype=np.float32)
    nx, ny = c.shape
    if nx == 0 or ny == 0:
        return [], np.float32(np.inf)
    inf = np.float32(np.inf)
    D = np.full((nx, ny), inf, dtype=np.float32)
    back = np.full((nx, ny), -1, dtype=np.int8)
    adm = admissible_matrix(nx, ny, radius)
    for i in range(nx):
        for j in range(ny):
            if not adm[i, j]:
                continue
            if i == 0 and j == 0:
                D[0, 0] = c[0, 0]
                continue
            best, move = None, -1
            for m, (di, dj) in MOVES.items():   # in the order up, left, diagonal
                pi, pj = i + di, j + dj
                if pi < 0 or pj < 0 or not adm[pi, pj]:
                    continue
                if best is None or D[pi, pj] < best:
                    best, move = D[pi, pj], m
            if best is None:   # an admissible cell that nothing leads to (does not happen for r >= 1, see connected())
                continue
            D[i, j] = best + c[i, j]   # np.float32 + np.float32 -> np.float32: the one rounding
            back[i, j] = move
    path = [(nx - 1, ny - 1)]
    while path[-1] != (0, 0):
        i, j = path[-1]
        m = int(back[i, j])
        assert m >= 0, "the end cell is not connected to the origin"
        path.append((i + MOVES[m][0], j + MOVES[m][1]))
    path.reverse()
    assert len(path) <= nx + ny - 1
    return path, D[nx - 1, ny - 1]


def connected(nx, ny, radius):
    """Is (nx-1, ny-1) reachable from (0, 0) through admissible cells by the three steps?"""
    seen = {(0, 0)} if admissible(0, 0, nx, ny, radius) else set()
    for i in range(nx):
        for j in range(ny):
            if (i, j) in seen or not admissible(i, j, nx, ny, radius):
                continue
            if any((i + di, j + dj) in seen for di, dj in MOVES.values()):
                seen.add((i, j))
    return (nx - 1, ny - 1) in seen


def all_monotone_paths(nx, ny):
    """Every path from (0, 0) to (nx-1, ny-1) by the steps (1, 0), (0, 1), (1, 1) -- brute force for tiny shapes."""
    def walk(path):
        i, j = path[-1]
        if (i, j) == (nx - 1, ny - 1):
            yield list(path)
            return
        for di, dj in ((1, 0), (0, 1), (1, 1)):
            if i + di < nx and j + dj < ny:
                path.append((i + di, j + dj))
                yield from walk(path)
                path.pop()
    yield from walk([(0, 0)])


def path_cost32(cost, path):
    """The path's cost accumulated the way the recurrence does: fp32, cell after cell from the origin."""
    c = np.asarray(cost, dtype=np.float32)
    acc = c[path[0]]
    for cell in path[1:]:
        acc = np.float32(acc + c[cell])
    return acc


def path_cost64(cost64, path):
    return math.fsum(float(cost64[i, j]) for i, j in path)


def cosine_cost(xn16, yn16):
    """c[i][j] = fl32(1 - s), s = the fp32 dot product of the fp16 rows accumulated in ascending k."""
    x = np.asarray(xn16, dtype=np.float16).astype(np.float32)
    y = np.asarray(yn16, dtype=np.float16).astype(np.float32)
    s = np.zeros((x.shape[0], y.shape[0]), dtype=np.float32)
    for k in range(x.shape[1]):
        s = (s + np.outer(x[:, k], y[:, k])).astype(np.float32)   # the fp16 products are exact in fp32: one rounding
    return (np.float32(1) - s).astype(np.float32)


def shapes_up_to(n):
    return list(itertools.product(range(1, n + 1), repeat=2))
