"""CPU: bitext mining -- the reference restatement against itself, the new C-ABI symbols, argument validation without
a device, and the Python layer's ValueErrors (sonar_amd/mining.py, tests/mining_ref.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import mining_ref as R


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def _random_candidates(rng, nx, ny, values, bad=0.0):
    fb = rng.integers(0, ny, nx)
    bb = rng.integers(0, nx, ny)
    fs = rng.choice(values, nx).astype(np.float32)
    bs = rng.choice(values, ny).astype(np.float32)
    if bad:
        fb[rng.random(nx) < bad] = -1
        bb[rng.random(ny) < bad] = nx
        fs[rng.random(nx) < bad] = np.nan
        bs[rng.random(ny) < bad] = np.nan
    return fb, fs, bb, bs


@pytest.mark.parametrize("bad", [0.0, 0.15])
def test_sequential_max_equals_bruteforce_and_parallel_rounds(bad):
    """LASER's sorted walk == "take the best remaining pair" == the engine's rounds, on small inputs full of ties
    (scores from five values, -0 and +0 among them) with and without excluded candidates."""
    rng = np.random.default_rng(7)
    values = np.array([-0.5, -0.0, 0.0, 0.25, 0.5], dtype=np.float32)
    contested = []
    for trial in range(60):
        nx, ny = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        fb, fs, bb, bs = _random_candidates(rng, nx, ny, values, bad)
        cands = R.candidates(fb, fs, bb, bs)
        walk = R.max_accepted(cands, nx, ny)
        assert walk == R.max_accepted_bruteforce(cands, nx, ny), (trial, cands)
        par, rounds, history = R.parallel_rounds(cands, nx, ny)
        assert par == sorted(walk), (trial, cands)
        assert rounds == len(history) and all(a > b for a, b in zip(history, history[1:]))
        srcs, trgs = [cands[c][0] for c in walk], [cands[c][1] for c in walk]
        assert len(set(srcs)) == len(srcs) and len(set(trgs)) == len(trgs) and len(walk) <= min(nx, ny)
        assert not any(R.excluded(cands[c], nx, ny) for c in walk)
        contested.append(R.contested_share(fb, fs, bb, bs, nx, ny))
    assert np.mean(contested) > 0.3  # the inputs did exercise the tie order


def test_reference_retrievals_and_threshold():
    # x0 <-> y1 mutual; x1 -> y1 (loses y1); y0 -> x1; x2 has no neighbour; y2's score is NaN
    fb, fs = np.array([1, 1, -1]), np.array([0.5, 0.25, 0.75], dtype=np.float32)
    bb, bs = np.array([1, 0, 2]), np.array([0.125, 0.5, np.nan], dtype=np.float32)
    assert R.mine(fb, fs, bb, bs, 3, 3, "fwd") == [(0, 1, 0.5), (1, 1, 0.25)]
    assert R.mine(fb, fs, bb, bs, 3, 3, "bwd") == [(1, 0, 0.125), (0, 1, 0.5)]
    assert R.mine(fb, fs, bb, bs, 3, 3, "intersect") == [(0, 1, 0.5)]
    got = R.mine(fb, fs, bb, bs, 3, 3, "max")
    assert got == [(0, 1, 0.5), (1, 0, 0.125)]          # candidate order: forward 0, backward 0
    assert R.final_order(got, "max") == got
    assert R.mine(fb, fs, bb, bs, 3, 3, "max", threshold=0.125) == [(0, 1, 0.5)]   # strict
    assert R.mine(fb, fs, bb, bs, 3, 3, "fwd", threshold=0.25) == [(0, 1, 0.5)]


def test_reference_chain_needs_many_rounds():
    """Scores rising along x0 -> y0 -> x1 -> y1 ...: only the top of the chain can win a round."""
    n = 12
    fb, bb = np.arange(n), np.minimum(np.arange(n) + 1, n - 1)
    fs = np.arange(n, dtype=np.float32) * 2
    bs = np.arange(n, dtype=np.float32) * 2 + 1
    acc, rounds, _ = R.parallel_rounds(R.candidates(fb, fs, bb, bs), n, n)
    assert rounds >= n - 1
    assert acc == sorted(R.max_accepted(R.candidates(fb, fs, bb, bs), n, n))


def test_new_symbols_declared_and_exported(lib):
    from sonar_amd import _lib

    for name in ("smi_xsim_pair_scores", "smi_xsim_mine_workspace_bytes", "smi_xsim_mine"):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
    assert _lib.SMI_MINE == {"fwd": 0, "bwd": 1, "intersect": 2, "max": 3}
    assert lib.smi_abi_version() == 7  # only functions were added


def test_mine_workspace_formula(lib):
    # block counts (one int32 per 256 candidates) + one counter; max adds two 8-byte slots, a state byte and a taken byte
    # per candidate
    assert lib.smi_xsim_mine_workspace_bytes(1000, 600, 0) == (4 + 1) * 4
    assert lib.smi_xsim_mine_workspace_bytes(1000, 600, 1) == (3 + 1) * 4
    assert lib.smi_xsim_mine_workspace_bytes(1000, 600, 2) == (4 + 1) * 4
    assert lib.smi_xsim_mine_workspace_bytes(1000, 600, 3) == (7 + 1) * 4 + 1600 * 10
    assert lib.smi_xsim_mine_workspace_bytes(0, 5, 3) == 0
    assert lib.smi_xsim_mine_workspace_bytes(5, 5, 4) == 0
    assert lib.smi_xsim_mine_workspace_bytes(2 ** 30, 2 ** 30, 3) == 0   # nx + ny beyond int32


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device behaviour")
def test_invalid_arguments_fail_before_any_device_call(lib):
    """Every argument is validated first: a bad call fails as SMI_ERR_INVALID_ARG / SMI_ERR_UNSUPPORTED with no device,
    and only a VALID call gets as far as SMI_ERR_NO_DEVICE."""
    buf = (C.c_char * 65536)()
    p = C.addressof(buf)
    inf = -math.inf

    def mine(**kw):
        a = dict(fb=p, fs=p, nx=100, bb=p, bs=p, ny=50, r=3, thr=inf, os=p, ot=p, osc=p, oc=p, ws=p, wsb=65536)
        a.update(kw)
        return lib.smi_xsim_mine(a["fb"], a["fs"], a["nx"], a["bb"], a["bs"], a["ny"], a["r"], a["thr"], a["os"], a["ot"],
                                 a["osc"], a["oc"], a["ws"], a["wsb"], None)

    assert mine() == -3 and b"no HIP device" in lib.smi_last_error()
    assert mine(r=4) == -1 and mine(r=-1) == -1
    assert mine(nx=0) == -1 and mine(ny=-2) == -1
    assert mine(nx=2 ** 31 - 10, ny=10) == -2 and b"int32" in lib.smi_last_error()
    assert mine(thr=math.nan) == -1
    assert mine(fb=None) == -1 and mine(bs=None) == -1 and mine(oc=None) == -1 and mine(ws=None) == -1
    assert mine(r=0, bb=None, bs=None) == -3 and mine(r=1, fb=None, fs=None) == -3 and mine(r=2, bs=None) == -3
    assert mine(r=2, bb=None) == -1
    need = lib.smi_xsim_mine_workspace_bytes(100, 50, 3)
    assert mine(wsb=need - 1) == -1 and b"smi_xsim_mine_workspace_bytes" in lib.smi_last_error()
    assert mine(wsb=need) == -3
    assert mine(ws=p + 4) == -1 and b"aligned" in lib.smi_last_error()

    def pairs(**kw):
        a = dict(xn=p, nx=10, yn=p, ny=10, d=64, si=p, ti=p, m=5, fs=p, bs=p, k=4, margin=0, out=p)
        a.update(kw)
        return lib.smi_xsim_pair_scores(a["xn"], a["nx"], a["yn"], a["ny"], a["d"], a["si"], a["ti"], a["m"], a["fs"],
                                        a["bs"], a["k"], a["margin"], a["out"], None)

    assert pairs() == -3
    assert pairs(k=0) == -2 and pairs(k=9) == -2 and pairs(d=96) == -2 and pairs(d=0) == -2
    assert pairs(margin=3) == -1 and pairs(m=0) == -1 and pairs(nx=0) == -1
    assert pairs(xn=None) == -1 and pairs(si=None) == -1 and pairs(out=None) == -1
    assert pairs(fs=None) == -1 and pairs(bs=None, margin=1) == -1
    assert pairs(fs=None, bs=None, margin=2) == -3   # the score lists may be NULL for the plain cosine


def test_python_layer_value_errors():
    """Raised before the tensors are looked at: CPU tensors (which the engine refuses later) get this far."""
    from sonar_amd import mining

    x, y = torch.zeros(5, 64), torch.zeros(6, 64)
    for kw in (dict(mode="align"), dict(retrieval="best"), dict(margin="ratios"), dict(k=0), dict(k=9), dict(k=2.0),
               dict(mode="score"), dict(mode="score", pairs=(torch.zeros(2),)), dict(threshold=math.nan)):
        with pytest.raises(ValueError):
            mining.mine_bitexts(x, y, **kw)
        with pytest.raises(ValueError):
            mining.mine_bitexts_normalized(x, 5, y, 6, **kw)
    # valid names get past the checks and stop at the engine's "no CPU path"
    for kw in (dict(), dict(margin="absolute"), dict(mode="search", k=8), dict(mode="score", pairs=([0], [1]))):
        with pytest.raises(RuntimeError, match="HIP device only"):
            mining.mine_bitexts(x, y, **kw)
    with pytest.raises(ValueError, match="one side only"):
        mining.mine_bitexts_normalized(x, 3, y, 6, k=4)
