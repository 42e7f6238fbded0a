#!/usr/bin/env python3
"""Record tests/golden/ivf_refusals.json: what every IVF / PQ entry of csrc/ivf.hip answers to calls it refuses on their
arguments -- the return code and the smi_last_error() text -- and what its sizing function returns for the same shape.

    python tests/golden/make_golden_ivf_refusals.py          (on a machine without a HIP device, library built)

Per entry: its arguments with values it accepts, and its refusals IN THE ORDER THE ENTRY CHECKS THEM, each as the arguments
to replace.  A case is one refusal, or two neighbours of that order at once (the first one must answer: that fixes the
order), or one of a few pairs given by hand.  Pointers are made-up aligned integers and are never dereferenced: the
recorder asserts that no call got as far as looking for a device.  tests/test_ivf_refusals_cpu.py replays the file.
"""
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


def main():
    out, odd = {}, []
    for fn, (args, sizing, refusals, pairs) in ENTRIES.items():
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
            rc = getattr(lib, fn)(*(call[a] for a in names))
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
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ivf_refusals.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(
            f' {json.dumps(fn)}: {{"args": {json.dumps(e["args"])}, "good": {json.dumps(e["good"])}, '
            f'"sizing": {json.dumps(e["sizing"])}, "cases": [\n'
            + ",\n".join("  " + json.dumps(c) for c in e["cases"]) + "]}" for fn, e in out.items()) + "\n}\n")
    print(path, sum(len(e["cases"]) for e in out.values()), "cases")


if __name__ == "__main__":
    main()
