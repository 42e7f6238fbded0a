"""CPU: every IVF / PQ entry of csrc/ivf.hip refuses what it refused, with the code and the text it gave, and in the order
it checked, before the host halves of the file were stated once.  tests/golden/ivf_refusals.json was recorded by
tests/golden/make_golden_ivf_refusals.py from the library built at commit 9fc8101, the parent of that change: per entry its
refusals one at a time and two neighbouring ones at once (the first one answers: that is the order), and for every case
what the entry's sizing function returns for the same shape -- 0 exactly where the entry refuses on shape -- which also
must leave smi_last_error() alone.  Pointers are made-up aligned integers, never dereferenced as long as the calls are
refused; where a HIP device is visible a regression that stopped refusing would launch kernels on them, so the test is for
the machine without one.

tests/golden/metric_refusals.json holds the same for the entries whose host halves were stated once after that: the paged
and the L2 flat search, the two k-means fits and the brute-force top-k entries beside them (METRIC_ENTRIES of the
recorder), from the library built at commit 9098134, the parent of that change."""
import ctypes
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ivf_refusals.json")
GOLDEN_METRIC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_refusals.json")
METRIC = {"smi_ivf_search_page", "smi_l2_flat_search", "smi_kmeans_fit", "smi_l2_kmeans_fit", "smi_l2_topk", "smi_xsim_topk_page",
          "smi_xsim_topk"}


def _library():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    if lib.smi_device_count() > 0:
        pytest.skip("a HIP device is visible: the made-up pointers must never reach a kernel")
    return _lib, lib


def test_refusals_are_the_recorded_ones():
    _lib, lib = _library()
    entries = json.load(open(GOLDEN))
    ivf = {s for s in _lib.SYMBOLS if s.startswith(("smi_ivf_", "smi_pq_")) and _lib.SYMBOLS[s][1][-1:] == [_lib.C.c_void_p]}
    assert ivf == set(entries), ivf ^ set(entries)
    assert sum(len(e["cases"]) for e in entries.values()) >= 400
    _replay(_lib, lib, entries)


def test_metric_refusals_are_the_recorded_ones():
    _lib, lib = _library()
    entries = json.load(open(GOLDEN_METRIC))
    assert METRIC == set(entries), METRIC ^ set(entries)
    assert sum(len(e["cases"]) for e in entries.values()) >= 250
    _replay(_lib, lib, entries)


def _replay(_lib, lib, entries):
    wrong = []
    for fn, e in entries.items():
        names, sizing = e["args"], e["sizing"]
        for c in e["cases"]:
            call = {**dict(zip(names, e["good"])), **c["change"]}
            # (a made-up address for an argument declared as a typed pointer goes through a cast)
            rc = getattr(lib, fn)(*(ctypes.cast(call[a], t) if isinstance(call[a], int) and issubclass(t, ctypes._Pointer)
                                    else call[a] for a, t in zip(names, _lib.SYMBOLS[fn][1])))
            got = {"rc": rc, "error": lib.smi_last_error().decode()}
            if sizing:
                got["bytes"] = getattr(lib, sizing["fn"])(*(call[a] for a in sizing["args"]))
                got["error after sizing"] = lib.smi_last_error().decode()
            want = {k: c[k] for k in ("rc", "error", "bytes") if k in c}
            if sizing:
                want["error after sizing"] = c["error"]
            if got != want:
                wrong.append((fn, c["case"], want, got))
    assert not wrong, wrong[:10]
