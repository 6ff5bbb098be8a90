"""Cost of the polish (sat_search_refine_polish) against the refine it extends and against the pair-match call that runs
the same record and map passes, alternated in one process, warmed, medians of --reps runs.  Prints one JSON object
(profiles/polish_cost.json).

For the bench shape (32-SSE query x 125 000 32-SSE entries) and BASELINE configs[4] (d1twfa_, 101 SSEs, x 100 000
entries of the C5 order mix), r = 128, K = 10, C = 1000, wall time of each route from the first launch to its rows:

* refine to R (R = 128: the ranking of stage 1 re-scored, and R = 1024)
* refine + polish to R with T = 1, 4, 8
* on the refine's candidate list: search_pairs_matches (M = T, maps) and search_pairs_polish (T) at R - the same record
  and map passes, so the difference of their kernel times is the price of the selection and polish kernels

    python scripts/polish_cost.py [--reps 5] [--quick]
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

K, C, TOPS = 10, 1000, (1, 4, 8)


def med(v):
    return float(np.median(v))


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def shape(s, db, q, reps, r=128, bigs=(128, 1024)):
    s.upload(db)
    s.set_queries([q])
    s.search_async(True, False, r)
    cand = s.topk_hits(C)["entry"][0].astype(np.int32)
    zeros = np.zeros(len(cand), np.int32)
    routes = {}
    for big in bigs:
        routes["refine_R%d_ms" % big] = lambda big=big: s.search_refine(K, C, big, True, True, r)
        for t in TOPS:
            routes["refine_polish_R%d_T%d_ms" % (big, t)] = lambda big=big, t=t: s.search_refine_polish(K, C, big, t, True, True, r)
            routes["pairs_matches_R%d_M%d_ms" % (big, t)] = lambda big=big, t=t: s.search_pairs_matches(zeros, cand, t, True, big)
            routes["pairs_polish_R%d_T%d_ms" % (big, t)] = lambda big=big, t=t: s.search_pairs_polish(zeros, cand, t, True, big)
    for fn in routes.values():                                  # warm-up: code objects, scratch
        fn()
    runs = {name: [] for name in routes}
    kernel = {}
    for _ in range(reps):                                       # alternated
        for name, fn in routes.items():
            t, out = wall(fn)
            runs[name].append(t)
            if name.startswith("pairs_"):
                kernel.setdefault(name.replace("_ms", "_kernel_ms"), []).append(out[-1])
    res = {"entries": len(db), "r": r, "K": K, "C": C}
    res.update({name: med(v) for name, v in runs.items()})
    res.update({name: med(v) for name, v in kernel.items()})
    for big in bigs:
        for t in TOPS:
            res["polish_over_refine_R%d_T%d" % (big, t)] = res["refine_polish_R%d_T%d_ms" % (big, t)] / res["refine_R%d_ms" % big]
            res["new_kernels_R%d_T%d_kernel_ms" % (big, t)] = (res["pairs_polish_R%d_T%d_kernel_ms" % (big, t)] -
                                                            res["pairs_matches_R%d_M%d_kernel_ms" % (big, t)])
    res["runs"] = runs
    res["launch"] = s.last_launch_info()
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
