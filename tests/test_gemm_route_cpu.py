"""CPU: the GEMM router (csrc/gemm_route.hpp) answers every case of tests/golden/gemm_routes.json as the launchers of the commit
before the router existed did.  The table was recorded from those launchers (each patched to write down kernel family, template
arguments, grid, LDS bytes, ksplit, part stride and raster instead of launching); it is replayed through smi_gemm_route and
smi_gemm_splitk_parts, which need no device.  Lines [0 | 1, ...] are single cases; lines [2 | 3 | 4, ...] hold the default switches over
the whole M x N x K grid, one request per line (format.grid_lines in the file)."""
import ctypes as C
import itertools
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_TM, OUT_TM = 1 << 12, 1 << 13
INVALID_ARG, UNSUPPORTED, NO_DEVICE = -1, -2, -3  # smi_status (include/sonar_mi355.h)


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")) as f:
        return json.load(f)


def _route(lib, epi_sel, m, n, k, ldo, bias, fold, nparts, stats, ksplit, slab, cus):
    from sonar_amd import _lib

    info = _lib.GemmRouteInfo()
    assert lib.smi_gemm_route(epi_sel, m, n, k, ldo, bias, fold, nparts, stats, ksplit, slab, cus, C.byref(info)) == 0
    got = [getattr(info, name) for name, _ in info._fields_ if name != "reserved"]
    return got if got[0] else [0]


def test_routes_match_the_recorded_table(lib, table):
    """The per-case lines: bias absent, fold and statistics kinds, other CU counts, and one switch at a time off its default."""
    from sonar_amd import _lib

    names = table["format"]["switches"]
    by_switch = {}
    for case in table["cases"]:
        if case[0] < 2:
            by_switch.setdefault((case[13], case[14]), []).append(case)
    assert len(by_switch) == 15  # the defaults + 14 single switch settings
    bad, reached = [], set()
    for (sw, value), cases in by_switch.items():
        with _lib.tuning(**({names[sw]: value} if sw >= 0 else {})):
            for case in cases:
                kind, args, want = case[0], case[1:13], case[15:]
                if kind == 0:
                    got = _route(lib, *args)
                    reached.add(want[0])
                else:
                    got = [lib.smi_gemm_splitk_parts(args[1], args[2], args[3], args[9], args[11])]
                if got != want:
                    bad.append((case[:15], want, got))
    assert not bad, (len(bad), bad[:10])
    # the sweep (these cases and the answers of the grid lines) reaches every engine and the refusal
    reached |= {c[1] for c in table["cases"] if c[0] == 2}
    assert reached == set(range(len(_lib.GEMM_ENGINE_NAMES))), sorted(reached)


def _expand(numbers):
    out = []
    for x in numbers:  # -r: the entry before it r more times
        out.extend([out[-1]] * -x if x < 0 else [x])
    return out


def test_default_switch_rows_cover_the_whole_grid(lib, table):
    """Default switches, 256 CUs: every epilogue x layout x engine selector of the plain entry, every ksplit x slab type x layout of
    the split-K entry and every max_parts of the part count, each over the complete M x N x K grid, point by point."""
    grid = table["format"]["grid"]
    assert grid == {"m": [128, 256, 512, 1024, 1280, 1536, 2048, 2560, 4096, 16384],
                    "n": [128, 256, 512, 1024, 2048, 3072, 8192, 256256], "k": [64, 128, 256, 512, 1024, 2048, 4096, 8192]}
    points = list(itertools.product(grid["m"], grid["n"], grid["k"]))
    answers = [None] + [c[1:] for c in table["cases"] if c[0] == 2]
    plain, split, parts, bad = set(), set(), set(), []
    for line in table["cases"]:
        if line[0] == 3:
            epi_sel, bias, ksplit, slab, cus, epi = line[1:7]
            assert bias == 1 and cus == 256
            (split if ksplit else plain).add((epi_sel & IN_TM, ksplit, slab) if ksplit else epi_sel)
            ids = _expand(line[7:])
            assert len(ids) == len(points)
            for (m, n, k), i in zip(points, ids):
                want = [answers[i][0], epi] + answers[i][1:] if i else [0]
                got = _route(lib, epi_sel, m, n, k, n // 2 if not ksplit and epi == 6 else n, bias, 0, 0, 0, ksplit, slab, cus)
                if got != want:
                    bad.append((line[1:7], (m, n, k), want, got))
        elif line[0] == 4:
            parts.add(line[1])
            want = _expand(line[3:])
            assert len(want) == len(points) and line[2] == 256
            bad += [(line[:3], p, w) for p, w in zip(points, want) if lib.smi_gemm_splitk_parts(*p, line[1], line[2]) != w]
    assert not bad, (len(bad), bad[:10])
    assert plain == {e | (s << 8) | lay for e in range(10) for s in (0, 1, 2) for lay in (0, IN_TM, IN_TM | OUT_TM)}
    assert split == {(lay, ks, slab) for lay in (0, IN_TM) for ks in (1, 2, 3, 4, 8, 12, 16) for slab in (0, 1)}
    assert parts == {1, 8, 16}


def test_engine_names_agree_with_the_header():
    from sonar_amd import _lib

    src = open(os.path.join(ROOT, "include", "sonar_mi355.h")).read()
    names = re.search(r"#define SMI_GEMM_ENGINE_NAMES[^{]*\{([^}]*)\}", src).group(1)
    assert tuple(re.findall(r'"(\w+)"', names)) == _lib.GEMM_ENGINE_NAMES
    values = dict(re.findall(r"SMI_GEMM_ENGINE_(\w+) = (\d+)", src))
    assert [values[n.upper()] for n in _lib.GEMM_ENGINE_NAMES] == [str(i) for i in range(len(_lib.GEMM_ENGINE_NAMES))]
    assert values["COUNT"] == str(len(_lib.GEMM_ENGINE_NAMES))


def test_refusal_is_unsupported_after_the_argument_checks(lib):
    from sonar_amd import _lib

    p = C.c_void_p(0x1000)  # never dereferenced: every call below is refused before a launch
    glu = 6 | (2 << 8) | IN_TM | OUT_TM  # the GLU epilogue with a tile-major output: only the 4-wave engine, from 128 tiles up
    assert _route(lib, glu, 256, 256, 256, 128, 1, 0, 0, 0, 0, 0, 256) == [0]
    assert lib.smi_gemm_tn(glu, None, p, p, p, 256, 256, 256, 128, None) == INVALID_ARG
    assert lib.smi_gemm_tn(glu, p, p, p, p, 256, 200, 256, 128, None) == UNSUPPORTED
    assert b"gemm shape" in lib.smi_last_error()
    rc = lib.smi_gemm_tn(glu, p, p, p, p, 256, 256, 256, 128, None)
    if torch.cuda.is_available():
        assert rc == UNSUPPORTED and b"no engine takes this combination" in lib.smi_last_error()
    else:
        assert rc == NO_DEVICE
    # split-K: K = 192 does not split into 2 parts of whole 64-column tiles
    assert _route(lib, 0, 128, 128, 192, 128, 1, 0, 0, 0, 2, _lib.SMI_F32, 256) == [0]
    assert lib.smi_gemm_tn_splitk(p, p, p, None, 128, 128, 192, 2, 0, _lib.SMI_F32, None) == INVALID_ARG
    assert lib.smi_gemm_tn_splitk(p, p, p, p, 128, 128, 192, 17, 0, _lib.SMI_F32, None) == UNSUPPORTED
    rc = lib.smi_gemm_tn_splitk(p, p, p, p, 128, 128, 192, 2, 0, _lib.SMI_F32, None)
    if torch.cuda.is_available():
        assert rc == UNSUPPORTED and b"does not split" in lib.smi_last_error()
    else:
        assert rc == NO_DEVICE


def test_route_query_rejects_bad_arguments(lib):
    from sonar_amd import _lib

    info = _lib.GemmRouteInfo()
    assert lib.smi_gemm_route(0, 128, 128, 64, 128, 1, 0, 0, 0, 0, 0, 256, None) == INVALID_ARG
    assert lib.smi_gemm_route(0, 128, 128, 64, 128, 1, 5, 0, 0, 0, 0, 256, C.byref(info)) == INVALID_ARG
    assert lib.smi_gemm_route(0, 128, 128, 64, 128, 1, 0, 0, 3, 0, 0, 256, C.byref(info)) == INVALID_ARG
    assert lib.smi_gemm_splitk_parts(0, 128, 64, 8, 256) == INVALID_ARG
