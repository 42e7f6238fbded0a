"""Filtered search over the IVF lists (sonar_amd.index) on one MI355X: one JSON line, also written to
profiles/ivf_filter_bench.json.

  Data: tools/bench_ivf.py's -- n = 1 M rows x 1024 fp16 with planted clusters, K = 1024 and K = 16 384 lists, 262 144
  queries, query j a noisy copy of the corpus row target[j]; k = 4, nprobe in {1, 4, 8}.  Row i speaks language
  (i // K) % 16 (independent of its cluster i % K), a query the language of its target.
  Per K and nprobe, each in event windows of `--launches` back-to-back calls, median / min / max over `--reps` windows, of the
  list function (inversion of the probe table + scan + merge) and, from a torch.profiler trace of one call, of the scan
  kernel alone:
    "unkeyed"   search_lists: the parent's kernel, unchanged -- the yardstick, in the same run on the same data;
    "accept7"   the keyed scan where everything passes: the work is identical, what differs is the fold's load and compare;
    "language"  == over the 16 language keys;
    "not_self"  != with row_keys = arange(n) and the query's own source row as its key;
  the whole `search` calls without a filter and with each of the two, and `row_filter` itself.  Flat lists in every cell; int8
  and PQ (dsub 8, trained on `--pq-train-rows` rows) lists in the cell `--quantised-cell` (K, nprobe).
  The run checks itself: every result carries an allowed key; with "language" every query finds its planted neighbour
  first (it speaks the query's language); with "not_self" no query returns its source row, and the results are the
  unfiltered results with that row taken out.
  Derived expectation, to read next to the measurement (no pass mark): the fold gains one L2-resident 16-byte load per four
  slots and a compare per candidate, and the prologue one 4-byte load per pair; the int8 work showed that the fold is visible
  in the scan time (profiles/ivf_i8_experiments.txt), so keyed / unkeyed at accept 7 is expected a little above 1.
    python tools/bench_ivf_filter.py [--rows 1000000] [--queries 262144] [--reps 5] [--launches 3]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ivf import queries  # noqa: E402
from bench_kmeans import planted, windows_ms  # noqa: E402

LANGS, K_RESULTS = 16, 4
SCANS = ("ivf_scan_lists", "ivf_i8_scan_lists", "ivf_pq_scan_lists")


def scan_trace(fn):
    """Device time in us of the list-walking kernel of one call, from a torch.profiler trace; a note where that is not
    available."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        us = sum(ev.device_time for ev in prof.events() if ev.device_time > 0 and any(s in ev.name for s in SCANS))
        return round(us, 2) if us else None
    except Exception as e:  # noqa: BLE001  (a measurement aid: the timed figures do not depend on it)
        return {"unavailable": repr(e)[:200]}


def ratio(a, b):
    return round(a / b, 4) if isinstance(a, (int, float)) and isinstance(b, (int, float)) and b else None


def scans(search, ids, lang_filter, self_filter, q_lang, q_self, reps, launches):
    """The four scans of one kind of list: search(ids, slot_keys, query_keys, accept) -> (scores, ids)."""
    legs = {"unkeyed": lambda: search(ids, None, None, None),
            "accept7": lambda: search(lang_filter.ids, lang_filter.keys, q_lang, 7),
            "language": lambda: search(lang_filter.ids, lang_filter.keys, q_lang, 2),
            "not_self": lambda: search(self_filter.ids, self_filter.keys, q_self, 5)}
    r = {}
    for name, fn in legs.items():
        r[name] = {"list_search_ms": windows_ms(fn, reps, launches), "scan_trace_us": scan_trace(fn)}
    base = r["unkeyed"]
    for name in ("accept7", "language", "not_self"):
        r[name]["list_search_over_unkeyed"] = ratio(r[name]["list_search_ms"]["median"], base["list_search_ms"]["median"])
        r[name]["scan_over_unkeyed"] = ratio(r[name]["scan_trace_us"], base["scan_trace_us"])
    ms = base["list_search_ms"]
    r["unkeyed"]["spread_max_over_min"] = ratio(ms["max"], ms["min"])
    # the self-check
    plain, same, lang, noself = (legs[name]() for name in ("unkeyed", "accept7", "language", "not_self"))
    torch.cuda.synchronize()
    return r, plain, same, lang, noself


def check(plain, same, lang, noself, row_lang, q_lang, target, exact):
    """exact: the scores are the flat scan's cosines, so the planted neighbour must come first; on quantised lists the queries
    that find it among their k results are counted."""
    ok = {"accept7_bits": bool(torch.equal(plain[0].view(torch.int32), same[0].view(torch.int32)) and torch.equal(plain[1], same[1]))}
    li = lang[1].long()
    have = li >= 0
    ok["language_keys_allowed"] = bool((row_lang[li.clamp(min=0)] == q_lang[:, None])[have].all())
    found = (lang[1] == target[:, None]).any(dim=1)
    ok["language_neighbour_first" if exact else "language_neighbour_found"] = int(
        (lang[1][:, 0] == target).sum() if exact else found.sum())
    ok["not_self_never_self"] = bool((noself[1] != target[:, None]).all())
    # the unfiltered results with the source row taken out are the head of the filtered results
    k = plain[1].shape[1]
    keep = plain[1] != target[:, None]
    order = torch.sort((~keep).int(), dim=1, stable=True)[1]
    head = torch.gather(plain[1], 1, order)[:, : k - 1]
    hit = (~keep).any(dim=1)
    ok["not_self_is_unfiltered_without_self"] = bool(torch.equal(torch.where(hit[:, None], head, plain[1][:, : k - 1]), noself[1][:, : k - 1]))
    # (on quantised lists the planted neighbour is recorded, not required: what they rank first is their quality, not the filter's)
    ok["ok"] = (ok["accept7_bits"] and ok["language_keys_allowed"] and ok["not_self_never_self"]
                and ok["not_self_is_unfiltered_without_self"]
                and (not exact or ok["language_neighbour_first"] == target.shape[0]))
    return ok


def run(x, q, target, k_lists, nprobes, quantised_nprobe, pq_train_rows, reps, launches):
    from sonar_amd import clustering, index, xsim

    n, d = x.shape
    nq = q.shape[0]
    xn, qn = xsim.normalize_rows(x), xsim.normalize_rows(q)
    km = clustering.SphericalKMeans(k_lists, n_iter=2).fit_normalized(xn, n, init=x[:k_lists])
    ix = index.IVFFlatIndex(km).add(x)
    torch.cuda.synchronize()
    sizes = ix.list_sizes
    res = {"n": n, "d": d, "K": k_lists, "nq": nq, "k": K_RESULTS,
           "list_size_min_mean_max": [int(sizes.min()), round(float(sizes.float().mean()), 1), int(sizes.max())]}
    arange = torch.arange(n, dtype=torch.int32, device="cuda")
    row_lang = (arange // k_lists % LANGS).contiguous()
    q_lang, q_self = row_lang[target.long()].contiguous(), target.contiguous()
    res["row_filter_ms"] = {"keys": windows_ms(lambda: ix.row_filter(keys=row_lang), reps, launches),
                            "mask": windows_ms(lambda: ix.row_filter(mask=row_lang < 8), reps, launches)}
    lang_filter, self_filter = ix.row_filter(keys=row_lang), ix.row_filter(keys=arange)
    for nprobe in nprobes:
        probes = ix.probe(q, nprobe).contiguous()
        flat = lambda ids, sk, qk, acc: index.search_lists(qn, probes, ix._rows, ids, ix._offsets, K_RESULTS, sk, qk, acc)  # noqa: E731
        cell, *results = scans(flat, ix._ids, lang_filter, self_filter, q_lang, q_self, reps, launches)
        cell["check"] = check(*results, row_lang, q_lang, target, True)
        cell["search_ms"] = {
            "unfiltered": windows_ms(lambda: ix.search(q, k=K_RESULTS, nprobe=nprobe), reps, launches),
            "language": windows_ms(lambda: ix.search(q, k=K_RESULTS, nprobe=nprobe, rows=lang_filter, query_keys=q_lang), reps, launches),
            "not_self": windows_ms(lambda: ix.search(q, k=K_RESULTS, nprobe=nprobe, rows=self_filter, query_keys=q_self, match="!="),
                                   reps, launches)}
        res[f"nprobe{nprobe}"] = {"flat": cell}
        if nprobe == quantised_nprobe:
            i8 = index.build_lists_int8(xn, km.labels, k_lists)
            f8 = index.slot_filter(i8[2], i8[3], row_lang), index.slot_filter(i8[2], i8[3], arange)
            fn = lambda ids, sk, qk, acc: index.search_lists_int8(qn, probes, i8[0], i8[1], ids, i8[3], K_RESULTS, sk, qk, acc)  # noqa: E731
            cell, *results = scans(fn, i8[2], *f8, q_lang, q_self, reps, launches)
            cell["check"] = check(*results, row_lang, q_lang, target, False)
            res[f"nprobe{nprobe}"]["int8"] = cell
            del i8, f8
            rows = min(pq_train_rows, n)
            cb = index.pq_train(xn, 8, clustering.init_rows(rows, 256, 0).to(device="cuda", dtype=torch.int32), 4, rows)
            pq = index.build_lists_pq(xn, km.labels, k_lists, cb)
            fp = index.slot_filter(pq[1], pq[2], row_lang), index.slot_filter(pq[1], pq[2], arange)
            fn = lambda ids, sk, qk, acc: index.search_lists_pq(qn, probes, pq[0], cb, ids, pq[2], K_RESULTS, sk, qk, acc)  # noqa: E731
            cell, *results = scans(fn, pq[1], *fp, q_lang, q_self, reps, launches)
            cell["check"] = check(*results, row_lang, q_lang, target, False)
            res[f"nprobe{nprobe}"]["pq8"] = cell
            del pq, fp
            torch.cuda.empty_cache()
    res["ok"] = all(kind["check"]["ok"] for p in nprobes for kind in res[f"nprobe{p}"].values())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--lists", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--quantised-cell", type=int, nargs=2, default=[1024, 4], metavar=("K", "NPROBE"))
    ap.add_argument("--pq-train-rows", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_filter_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivf_filter needs an MI355X: there is no CPU path")
    n, d, nq = args.rows, args.dim, args.queries
    out = {"metric": "ivf_keyed_over_unkeyed_list_search",
           "config": f"{n} x {d} fp16 planted clusters, {nq} queries, k = {K_RESULTS}, {LANGS} language keys, one MI355X",
           "expectation": "derived, unmeasured: the keyed fold adds one L2-resident 16-byte load per four slots and a compare per "
                          "candidate; keyed / unkeyed at accept 7 a little above 1; no pass mark"}
    for k_lists in args.lists:
        x, _ = planted(n, k_lists, d, seed=k_lists)
        q, target = queries(x, nq, seed=k_lists + 1)
        qp = args.quantised_cell[1] if k_lists == args.quantised_cell[0] else None
        out[f"K{k_lists}"] = run(x, q, target, k_lists, args.nprobe, qp, args.pq_train_rows, args.reps, args.launches)
        del x, q, target
        torch.cuda.empty_cache()
    first = out[f"K{args.lists[0]}"][f"nprobe{args.nprobe[0]}"]["flat"]
    out["value"] = first["accept7"]["list_search_over_unkeyed"]
    out["ok"] = all(out[f"K{k}"]["ok"] for k in args.lists)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not out["ok"]:
        raise SystemExit("the self-check failed: a result with a key that does not pass, or a planted neighbour that was not found")


if __name__ == "__main__":
    main()
