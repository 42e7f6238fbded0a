"""CPU: every public *_workspace_bytes function returns what it returned before the layouts were stated once (WsLayout in
csrc/api_common.hpp).  tests/golden/workspace_bytes.json was recorded from the library built at commit 888cf21, the parent of
that change: the functions' arguments over small grids with alignment remainders (K and n that are no multiples of 4), the
refusals that return 0, and for DTW a few offset vectors with empty pairs.  smi_kmeans_fit has no sizing function: its entries
hold the need its refusal of a too-small workspace names."""
import ctypes as C
import json
import os
import re

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def _kmeans_fit_need(lib, n, K, d):
    """The refusal of a workspace of 0 bytes (checked before any device is looked for) ends in `= <need>`."""
    p = C.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
    rc = lib.smi_kmeans_fit(p, n, d, K, 1, 0, p, p, p, p, p, p, p, p, p, p, 0, None)
    m = re.search(r"= (\d+)$", lib.smi_last_error().decode())
    assert rc != 0 and m, lib.smi_last_error()
    return int(m.group(1))


def test_workspace_bytes_are_the_recorded_ones(lib):
    entries = json.load(open(GOLDEN))
    assert 300 <= len(entries) <= 600 and sum(e["bytes"] == 0 for e in entries) >= 50
    from sonar_amd import _lib

    sizing = {s for s in _lib.SYMBOLS if s.endswith("_workspace_bytes")}
    assert sizing and sizing <= {e["fn"] for e in entries}, sizing - {e["fn"] for e in entries}
    wrong = []
    for e in entries:
        fn, args = e["fn"], e["args"]
        if fn == "smi_kmeans_fit":
            got = _kmeans_fit_need(lib, *args)
        elif fn == "smi_dtw_workspace_bytes":
            n_pairs, xo, yo = args
            got = lib.smi_dtw_workspace_bytes(n_pairs, (C.c_int64 * len(xo))(*xo), (C.c_int64 * len(yo))(*yo))
        else:
            got = getattr(lib, fn)(*args)
        if got != e["bytes"]:
            wrong.append((fn, args, e["bytes"], got))
    assert not wrong, wrong[:10]
