#!/usr/bin/env python3
"""Record tests/golden/ivf_refusals.json: what every IVF / PQ entry of csrc/ivf.hip answers to calls it refuses on their
arguments -- the return code and the smi_last_error() text -- and what its sizing function returns for the same shape --
and tests/golden/metric_refusals.json: the same for the paged and Euclidean entries that came after (METRIC_ENTRIES).

    python tests/golden/make_golden_ivf_refusals.py [ivf] [metric]     (on a machine without a HIP device, library built)

Per entry: its arguments with values it accepts, and its refusals IN THE ORDER THE ENTRY CHECKS THEM, each as the arguments
to replace.  A case is one refusal, or two neighbours of that order at once (the first one must answer: that fixes the
order), or one of a few pairs given by hand.  Pointers are made-up aligned integers and are never dereferenced: the
recorder asserts that no call got as far as looking for a device.  tests/test_ivf_refusals_cpu.py replays the file.
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from sonar_amd import _lib  # noqa: E402

P, BIG, I31 = 0x1000, 1 << 40, 1 << 31
MAX = 0x7fffff00
SHAPE, ARG = True, False  # is the refusal one of the shape (the sizing function then returns 0) or of a pointer / a size?

lib = _lib.load()
CAP = lib.smi_ivf_slots_bound(100, 7)


def nulls(*names):
    return [(f"null {n}", {n: None}, ARG) for n in names]


def shape(n):  # check_shape, then what follows it
    return [("d", {"d": 96}, SHAPE), ("d 0", {"d": 0}, SHAPE), (f"{n} 0", {n: 0}, SHAPE), (f"big {n}", {n: I31}, SHAPE)]


def shape_k(n):
    return [("d", {"d": 96}, SHAPE), ("d 0", {"d": 0}, SHAPE), ("K 0", {"K": 0}, SHAPE), (f"{n} 0", {n: 0}, SHAPE),
            (f"big {n}", {n: I31}, SHAPE), ("big K", {"K": I31}, SHAPE)]


I8_DIM = [("big d", {"d": 131072 + 64}, SHAPE)]
DSUB = [("dsub", {"dsub": 12}, SHAPE), ("dsub 0", {"dsub": 0}, SHAPE), ("dsub 128", {"d": 192, "dsub": 128}, SHAPE)]
CODEBOOKS = [("null codebooks", {"codebooks": None}, ARG), ("misaligned codebooks", {"codebooks": P + 8}, ARG)]
CENTROIDS = [("null centroids", {"centroids": None}, ARG), ("misaligned centroids", {"centroids": P + 8}, ARG)]
CENTROIDS_K = CENTROIDS + [("K 0", {"K": 0}, ARG), ("big K", {"K": I31}, ARG)]  # where nothing else has looked at K


def ws(sizing, *args):
    return [("null ws", {"ws": None}, ARG), ("misaligned ws", {"ws": P + 8}, ARG),
            ("short ws", {"ws_bytes": getattr(lib, sizing)(*args) - 1}, ARG)]


BUILD_TAIL = [("big slots", {"n": 1 << 30, "K": 1 << 30, "capacity": BIG}, SHAPE), ("small capacity", {"capacity": CAP - 1}, ARG)]
SEARCH_TAIL = [("k 0", {"k": 0}, SHAPE), ("k 9", {"k": 9}, SHAPE), ("nprobe 0", {"nprobe": 0}, SHAPE),
               ("nprobe 9", {"nprobe": 9}, SHAPE), ("big pairs", {"nq": 1 << 29, "nprobe": 8}, SHAPE)]


def build(rows, extra=(), res=()):
    return [("xn", P), ("labels", P), ("n", 100), ("d", 64), ("K", 7), *res, *extra, *((r, P) for r in rows), ("ids", P),
            ("capacity", CAP), ("offsets", P), ("sizes", P), ("ws", P), ("ws_bytes", BIG), ("stream", None)]


def search(rows, res=()):
    return [("qn", P), ("nq", 100), ("d", 64), ("probes", P), *res, ("nprobe", 4), *rows, ("ids", P), ("offsets", P), ("K", 7),
            ("k", 5), ("idx", P), ("score", P), ("ws", P), ("ws_bytes", BIG), ("stream", None)]


PQ = [("dsub", 8), ("codebooks", P)]
TRAIN_TAIL = [("dsub", 8), ("init", P), ("n_iter", 3), ("codebooks", P), ("ws", P), ("ws_bytes", BIG), ("stream", None)]
TRAIN_LATE = [("n_iter", {"n_iter": -1}, ARG), ("big d", {"d": 1 << 24}, SHAPE), ("many blocks", {"n": MAX, "d": 1 << 17}, SHAPE)]
BW, SW = ("n", "K", "d"), ("nq", "K", "nprobe", "k", "d")
BUILD_PAIRS = [("d + K 0", {"d": 96, "K": 0}, SHAPE), ("big n + small capacity", {"n": I31, "capacity": CAP - 1}, SHAPE)]
PQ_PAIRS = [("dsub + misaligned codebooks", {"dsub": 12, "codebooks": P + 8}, SHAPE)]

# name: (arguments, (sizing function, its arguments) or None, refusals in the entry's order, further pairs)
ENTRIES = {
    "smi_ivf_build": (build(["rows"]), ("smi_ivf_build_workspace_bytes", BW),
                      nulls("xn", "labels", "rows", "ids", "offsets", "sizes") + shape_k("n") + BUILD_TAIL
                      + ws("smi_ivf_build_workspace_bytes", 100, 7, 64), BUILD_PAIRS),
    "smi_ivf_search": (search([("rows", P)]), ("smi_ivf_search_workspace_bytes", SW),
                       nulls("qn", "probes", "rows", "ids", "offsets", "idx", "score") + shape_k("nq") + SEARCH_TAIL
                       + ws("smi_ivf_search_workspace_bytes", 100, 7, 4, 5, 64), []),
    "smi_ivf_dedup": ([("rows", P), ("ids", P), ("offsets", P), ("K", 7), ("slots", 160), ("d", 64), ("priority", P), ("n", 100),
                       ("max_sim", P), ("nearest", P), ("ws", P), ("ws_bytes", BIG), ("stream", None)],
                      ("smi_ivf_dedup_workspace_bytes", ("slots", "n", "K", "d")),
                      nulls("rows", "ids", "offsets", "max_sim", "nearest") + shape_k("n")
                      + [("slots 0", {"slots": 0}, SHAPE), ("big slots", {"slots": I31}, SHAPE), ("slots % 16", {"slots": 150}, SHAPE),
                         ("many units", {"slots": MAX, "K": MAX}, SHAPE)] + ws("smi_ivf_dedup_workspace_bytes", 160, 100, 7, 64),
                      [("big slots + slots % 16", {"slots": I31 + 8}, SHAPE)]),
    "smi_ivf_i8_encode": ([("xn", P), ("n", 100), ("d", 64), ("codes", P), ("scales", P), ("stream", None)], None,
                          nulls("xn", "codes", "scales") + shape("n") + I8_DIM, []),
    "smi_ivf_i8_build": (build(["codes", "scales"]), ("smi_ivf_i8_build_workspace_bytes", BW),
                         nulls("xn", "labels", "codes", "scales", "ids", "offsets", "sizes") + shape_k("n") + BUILD_TAIL
                         + ws("smi_ivf_i8_build_workspace_bytes", 100, 7, 64) + I8_DIM, BUILD_PAIRS),
    "smi_ivf_i8_search": (search([("codes", P), ("scales", P)]), ("smi_ivf_i8_search_workspace_bytes", SW),
                          nulls("qn", "probes", "codes", "scales", "ids", "offsets", "idx", "score") + shape_k("nq") + SEARCH_TAIL
                          + I8_DIM + ws("smi_ivf_i8_search_workspace_bytes", 100, 7, 4, 5, 64)
                          + [("flat-sized ws", {"ws_bytes": lib.smi_ivf_search_workspace_bytes(100, 7, 4, 5, 64)}, ARG)], []),
    "smi_pq_encode": ([("xn", P), ("n", 100), ("d", 64), *PQ, ("codes", P), ("stream", None)], None,
                      nulls("xn", "codes") + shape("n") + DSUB + CODEBOOKS, PQ_PAIRS),
    "smi_pq_decode": ([("codes", P), ("n", 100), ("d", 64), *PQ, ("rows", P), ("stream", None)], None,
                      nulls("codes", "rows") + [("misaligned rows", {"rows": P + 8}, ARG)] + shape("n") + DSUB + CODEBOOKS, PQ_PAIRS),
    "smi_pq_train": ([("xn", P), ("n", 1000), ("d", 64), *TRAIN_TAIL], ("smi_pq_train_workspace_bytes", ("n", "d", "dsub")),
                     nulls("xn", "init") + shape("n") + DSUB + CODEBOOKS + TRAIN_LATE
                     + ws("smi_pq_train_workspace_bytes", 1000, 64, 8), PQ_PAIRS),
    "smi_ivf_pq_build": (build(["codes"], PQ), ("smi_ivf_pq_build_workspace_bytes", BW + ("dsub",)),
                         nulls("xn", "labels", "codes", "ids", "offsets", "sizes") + shape_k("n") + BUILD_TAIL
                         + ws("smi_ivf_pq_build_workspace_bytes", 100, 7, 64, 8) + DSUB + CODEBOOKS, BUILD_PAIRS + PQ_PAIRS),
    "smi_ivf_pq_search": (search([("codes", P), *PQ]), ("smi_ivf_pq_search_workspace_bytes", SW + ("dsub",)),
                          nulls("qn", "probes", "codes", "ids", "offsets", "idx", "score") + shape_k("nq") + SEARCH_TAIL + DSUB
                          + CODEBOOKS + ws("smi_ivf_pq_search_workspace_bytes", 100, 7, 4, 5, 64, 8), PQ_PAIRS),
    "smi_pq_residuals": ([("xn", P), ("labels", P), ("n", 100), ("d", 64), ("centroids", P), ("K", 7), ("out", P), ("stream", None)],
                         None, nulls("xn", "labels", "out") + [("misaligned out", {"out": P + 2}, ARG)] + shape("n") + CENTROIDS_K, []),
    "smi_pq_encode_residual": ([("xn", P), ("labels", P), ("n", 100), ("d", 64), ("centroids", P), ("K", 7), *PQ, ("codes", P),
                                ("stream", None)], None,
                               nulls("xn", "labels", "codes") + shape("n") + DSUB + CODEBOOKS + CENTROIDS_K, PQ_PAIRS),
    "smi_pq_train_residual": ([("xn", P), ("labels", P), ("n", 1000), ("d", 64), ("centroids", P), ("K", 7), *TRAIN_TAIL],
                              ("smi_pq_train_workspace_bytes", ("n", "d", "dsub")),
                              nulls("xn", "init", "labels") + shape("n") + DSUB + CODEBOOKS + CENTROIDS_K + TRAIN_LATE
                              + ws("smi_pq_train_workspace_bytes", 1000, 64, 8), PQ_PAIRS),
    "smi_ivf_pq_build_residual": (build(["codes"], PQ, [("centroids", P)]), ("smi_ivf_pq_build_workspace_bytes", BW + ("dsub",)),
                                  nulls("xn", "labels", "codes", "ids", "offsets", "sizes") + shape_k("n") + BUILD_TAIL
                                  + ws("smi_ivf_pq_build_workspace_bytes", 100, 7, 64, 8) + DSUB + CODEBOOKS + CENTROIDS,
                                  BUILD_PAIRS + PQ_PAIRS),
    "smi_ivf_pq_search_residual": (search([("codes", P), *PQ], [("coarse", P)]), ("smi_ivf_pq_search_workspace_bytes", SW + ("dsub",)),
                                   nulls("qn", "probes", "codes", "ids", "offsets", "idx", "score", "coarse") + shape_k("nq")
                                   + SEARCH_TAIL + DSUB + CODEBOOKS + ws("smi_ivf_pq_search_workspace_bytes", 100, 7, 4, 5, 64, 8),
                                   PQ_PAIRS),
}


def ceil_pair():  # the ceilings of a page: both or neither
    return [("ceil_score alone", {"ceil_score": P}, ARG), ("ceil_idx alone", {"ceil_score": None, "ceil_idx": P}, ARG)]


def topk_shape(kmax, big=True):  # the shape refusals of a brute-force top-k, in its order
    return ([("k 0", {"k": 0}, SHAPE), (f"k {kmax + 1}", {"k": kmax + 1}, SHAPE), ("d", {"d": 96}, SHAPE), ("d 0", {"d": 0}, SHAPE),
             ("nx 0", {"nx": 0}, SHAPE), ("ny 0", {"ny": 0}, SHAPE)]
            + ([("big nx", {"nx": I31}, SHAPE), ("big ny", {"ny": I31}, SHAPE)] if big else []))


def misaligned(*names):
    return [(f"misaligned {n}", {n: P + 8}, ARG) for n in names]


KM_NULLS = ("centroids_f32", "centroids_f16", "labels", "scores", "sums", "counts", "objective", "moved", "empty")
KM_SHAPE = [("d", {"d": 96}, SHAPE), ("d 0", {"d": 0}, SHAPE), ("K 0", {"K": 0}, SHAPE), ("n 0", {"n": 0}, SHAPE),
            ("big n", {"n": I31}, SHAPE), ("big K", {"K": I31}, SHAPE), ("n_iter", {"n_iter": -1}, ARG),
            ("resume", {"resume": 2}, ARG)]


def km_fit(x, extra=()):
    return [(x, P), ("n", 1000), ("d", 64), ("K", 7), ("n_iter", 3), ("resume", 0), ("centroids_f32", P), ("centroids_f16", P),
            *extra, ("labels", P), ("scores", P), ("sums", P), ("counts", P), ("objective", P), ("moved", P), ("empty", P),
            ("ws", P), ("ws_bytes", BIG), ("stream", None)]


def topk(extra):
    return [("x", P), ("nx", 100), ("y", P), ("ny", 300), ("d", 64), ("k", 5), ("y_off", 0), *extra, ("idx", P), ("score", P),
            ("ws", P), ("ws_bytes", BIG), ("stream", None)]


PAGE_TAIL = [("k 0", {"k": 0}, SHAPE), ("k 17", {"k": 17}, SHAPE), ("nprobe 0", {"nprobe": 0}, SHAPE),
             ("nprobe 65", {"nprobe": 65}, SHAPE), ("big pairs", {"nq": 1 << 29, "nprobe": 8}, SHAPE)]
CEIL = [("ceil_score", None), ("ceil_idx", None)]
TW = ("nx", "ny", "k", "d")

# The entries whose host halves were stated once after ivf_refusals.json was recorded.  smi_kmeans_fit has no sizing function
# of its own: the shape predicate it shares is smi_kmeans_workspace_bytes', and any workspace of 16 bytes is short.
# smi_xsim_topk's sizing function does not look at d % 64: none is recorded for it.
METRIC_ENTRIES = {
    "smi_ivf_search_page": (search([("rows", P)]) + CEIL, ("smi_ivf_search_page_ws_bytes", SW),
                            nulls("qn", "probes", "rows", "ids", "offsets", "idx", "score") + ceil_pair() + shape_k("nq")
                            + PAGE_TAIL + ws("smi_ivf_search_page_ws_bytes", 100, 7, 4, 5, 64)
                            + [("search-sized ws", {"ws_bytes": lib.smi_ivf_search_workspace_bytes(100, 7, 4, 5, 64)}, ARG)],
                            [("k 16 + nprobe 64 + short ws", {"k": 16, "nprobe": 64, "ws_bytes": 16}, ARG)]),
    "smi_l2_flat_search": (search([("rows", P), ("bias", P)]), ("smi_l2_flat_search_ws_bytes", SW),
                           nulls("qn", "probes", "rows", "bias", "ids", "offsets", "idx", "score") + shape_k("nq") + SEARCH_TAIL
                           + misaligned("bias") + ws("smi_l2_flat_search_ws_bytes", 100, 7, 4, 5, 64), []),
    "smi_kmeans_fit": (km_fit("xn"), ("smi_kmeans_workspace_bytes", ("n", "K", "d")),
                       nulls("xn", *KM_NULLS) + KM_SHAPE
                       + [("null ws", {"ws": None}, ARG), ("misaligned ws", {"ws": P + 8}, ARG), ("short ws", {"ws_bytes": 16}, ARG)],
                       [("short ws, K 300", {"K": 300, "ws_bytes": 16}, ARG), ("short ws, d 1024", {"d": 1024, "ws_bytes": 16}, ARG)]),
    "smi_l2_kmeans_fit": (km_fit("x", [("half_norms", P)]), ("smi_l2_kmeans_fit_ws_bytes", ("n", "K", "d")),
                          nulls("x", "half_norms", *KM_NULLS) + KM_SHAPE + misaligned("x", "centroids_f32", "centroids_f16")
                          + ws("smi_l2_kmeans_fit_ws_bytes", 1000, 7, 64),
                          [("short ws, K 300", {"K": 300, "ws_bytes": 16}, ARG), ("short ws, d 1024", {"d": 1024, "ws_bytes": 16}, ARG)]),
    "smi_l2_topk": (topk([("y_bias", P)]), ("smi_l2_topk_ws_bytes", TW),
                    nulls("x", "y", "idx", "score", "y_bias") + topk_shape(8) + misaligned("x", "y", "y_bias")
                    + ws("smi_l2_topk_ws_bytes", 100, 300, 5, 64), []),
    "smi_xsim_topk_page": (topk(CEIL), ("smi_xsim_topk_page_ws_bytes", TW),
                           nulls("x", "y", "idx", "score") + ceil_pair() + topk_shape(16)
                           + ws("smi_xsim_topk_page_ws_bytes", 100, 300, 5, 64), []),
    "smi_xsim_topk": (topk([]), None,
                      nulls("x", "y", "idx", "score", "ws") + topk_shape(8, big=False)
                      + [("short ws", {"ws_bytes": lib.smi_xsim_workspace_bytes(100, 300, 5, 64) - 1}, ARG)], []),
}
FILES = {"ivf": (ENTRIES, "ivf_refusals.json"), "metric": (METRIC_ENTRIES, "metric_refusals.json")}


def c_args(fn, values):  # a made-up address for an argument declared as a typed pointer
    return [ctypes.cast(v, t) if isinstance(v, int) and issubclass(t, ctypes._Pointer) else v
            for t, v in zip(_lib.SYMBOLS[fn][1], values)]


def record(entries, file):
    out, odd = {}, []
    for fn, (args, sizing, refusals, pairs) in entries.items():
        names, good = [a for a, _ in args], dict(args)
        assert len(names) == len(_lib.SYMBOLS[fn][1]), fn
        cases, single = [], {}
        todo = [(label, change, is_shape, None) for label, change, is_shape in refusals]
        for (la, ca, sa, _), (lb, cb, sb, _) in zip(todo[:-1], todo[1:len(refusals)]):
            if all(ca[a] == cb[a] for a in set(ca) & set(cb)):  # two values for one argument: no such call
                todo.append((f"{la} + {lb}", {**ca, **cb}, sa or sb, la))
        todo += [(label, change, is_shape, None) for label, change, is_shape in pairs]
        for label, change, is_shape, first in todo:
            assert set(change) <= set(names), (fn, label)
            call = {**good, **change}
            rc = getattr(lib, fn)(*c_args(fn, [call[a] for a in names]))
            text = lib.smi_last_error().decode()
            assert rc not in (0, -3), (fn, label, rc, text)  # neither accepted nor refused for want of a device
            case = {"case": label, "change": change, "rc": rc, "error": text}
            if sizing:
                case["bytes"] = getattr(lib, sizing[0])(*(call[a] for a in sizing[1]))
                assert (case["bytes"] == 0) == is_shape, (fn, label, case["bytes"])
                assert lib.smi_last_error().decode() == text, (fn, label)
            single.setdefault(label, (rc, text))
            if first and single[first] != (rc, text):  # (a text that names both arguments differs rightly: look at them)
                odd.append((fn, label, single[first], (rc, text)))
            cases.append(case)
        out[fn] = {"args": names, "good": [good[a] for a in names], "sizing": sizing and {"fn": sizing[0], "args": list(sizing[1])},
                   "cases": cases}
    for o in odd:
        print("the pair does not answer as its first refusal alone:", *o)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), file)
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(
            f' {json.dumps(fn)}: {{"args": {json.dumps(e["args"])}, "good": {json.dumps(e["good"])}, '
            f'"sizing": {json.dumps(e["sizing"])}, "cases": [\n'
            + ",\n".join("  " + json.dumps(c) for c in e["cases"]) + "]}" for fn, e in out.items()) + "\n}\n")
    print(path, sum(len(e["cases"]) for e in out.values()), "cases")


if __name__ == "__main__":
    for which in sys.argv[1:] or FILES:
        record(*FILES[which])
