"""Cost of the matches of the reported rows only (sat_search_pairs_matches) against the whole-database route, alternated
in one process, warmed, medians of --reps runs.  Prints one JSON object (profiles/pair_matches_cost.json).

For the bench shape (32-SSE query x 125 000 32-SSE entries) and BASELINE configs[4] (d1twfa_, 101 SSEs, x 100 000
entries of the C5 order mix), r = 128, M = 4, wall time of each route from the first launch to its rows on the host:

* whole database: sat_search_matches with maps + the plain LSOLN top-k search - what `-m 4 -k 10` runs (both calls and
  their kernels are the ones the library had before the pair-match mode)
* reported rows: the plain LSOLN top-k search + sat_search_pairs_matches on its K rows, K = 10 and K = 1000
* refine (r = 128, C = 1000, R = 4096, K = 10) without and with the pair-match call on its K rows at R

    python scripts/pair_matches_cost.py [--reps 5] [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_satabsearch_amd as sat  # noqa: E402
from cuda_satabsearch_amd import workloads  # noqa: E402

M = 4


def med(v):
    return float(np.median(v))


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def whole_route(s, r, k):
    s.search_matches(M, True, r, maps=True)
    s.search_async(True, True, r)
    return s.topk_hits(k, lsoln=True)


def rows_route(s, r, k):
    s.search_async(True, True, r)
    hits, _ = s.topk_hits(k, lsoln=True)
    return s.search_pairs_matches(np.zeros(hits.shape[1], np.int32), hits["entry"][0], M, True, r, maps=True)


def refine_route(s, r, c, big_r, k, matches):
    hits, _, _ = s.search_refine(k, c, big_r, True, True, r)
    if matches:
        return s.search_pairs_matches(np.zeros(hits.shape[1], np.int32), hits["entry"][0], M, True, big_r, maps=True)
    return hits


def shape(s, db, q, reps, r=128, c=1000, big_r=4096):
    s.upload(db)
    s.set_queries([q])
    routes = {
        "whole_db_matches_plus_topk10_ms": lambda: whole_route(s, r, 10),
        "topk10_plus_pair_matches_ms": lambda: rows_route(s, r, 10),
        "topk1000_plus_pair_matches_ms": lambda: rows_route(s, r, 1000),
        "refine_ms": lambda: refine_route(s, r, c, big_r, 10, False),
        "refine_plus_pair_matches_ms": lambda: refine_route(s, r, c, big_r, 10, True),
    }
    for fn in routes.values():                                  # warm-up: code objects, scratch
        fn()
    runs = {name: [] for name in routes}
    kernel = {"pair_matches_k10_kernel_ms": [], "pair_matches_k1000_kernel_ms": [], "pair_matches_refine_rows_kernel_ms": []}
    launch = {}
    for _ in range(reps):                                       # alternated
        for name, fn in routes.items():
            t, out = wall(fn)
            runs[name].append(t)
            if name == "topk10_plus_pair_matches_ms":
                kernel["pair_matches_k10_kernel_ms"].append(out[4])
                launch["k10"] = s.last_launch_info()
            elif name == "topk1000_plus_pair_matches_ms":
                kernel["pair_matches_k1000_kernel_ms"].append(out[4])
                launch["k1000"] = s.last_launch_info()
            elif name == "refine_plus_pair_matches_ms":
                kernel["pair_matches_refine_rows_kernel_ms"].append(out[4])
                launch["refine_rows"] = s.last_launch_info()
    res = {"entries": len(db), "r": r, "M": M, "C": c, "R": big_r}
    res.update({name: med(v) for name, v in runs.items()})
    res.update({name: med(v) for name, v in kernel.items()})
    whole = res["whole_db_matches_plus_topk10_ms"]
    res["ratio_k10_vs_whole_db"] = res["topk10_plus_pair_matches_ms"] / whole
    res["ratio_k1000_vs_whole_db"] = res["topk1000_plus_pair_matches_ms"] / whole
    res["refine_matches_overhead"] = res["refine_plus_pair_matches_ms"] / res["refine_ms"]
    res["runs"] = runs
    res["launch"] = launch
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="bench shape only, one run (for a kernel-trace run)")
    args = ap.parse_args()
    res = {}
    with sat.Searcher(0) as s:
        res["bench_shape"] = shape(s, sat.synth.make_db(125_000, 32), sat.synth.make_query(32), 1 if args.quick else args.reps)
        if not args.quick:
            q4 = workloads.config4_query()
            res["configs4"] = shape(s, workloads.config4_db(), (q4[1], q4[2], q4[3]), args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
