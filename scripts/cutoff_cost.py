"""Cost of the p-value cutoff (sat_hits_cutoff) after a search, against the two ways a user had before: the best
k = 10 rows per query (sat_topk_hits) and the full score download (sat_results).  Every case runs on the same finished
search (the selection never searches), warmed, alternated in one process, medians of --reps runs.  Prints one JSON
object (profiles/cutoff_cost.json).

* bench shape: one 32-SSE query x 125 000 32-SSE entries, r = 128
* q200 shape (scripts/run_config.py q200): 200 database members as queries x 15 000 size-sorted entries of 4..40 SSEs

Cutoffs: P = 1e-3, 0.0108 (just above the p-value of a truncated norm2 of 2) and 1 (every row).  Each time is host
wall clock around the call, which ends in a device synchronise and the copy of its rows.  Kernel times: run the same
script under `rocprofv3 --kernel-trace --stats` (--reps 1 keeps that run short).

    python scripts/cutoff_cost.py [--reps 5] [--only bench|q200]
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

CUTOFFS = (1e-3, 0.0108, 1.0)


def med(v):
    return float(np.median(v))


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def shape(s, db, queries, reps):
    s.upload(db)
    s.set_queries(queries)
    search_ms = s.search(True, False, 128)[2]
    cases = {"topk10": lambda: s.topk_hits(10), "results": lambda: s.results()}
    for p in CUTOFFS:
        cases["cutoff_%g" % p] = lambda p=p: s.hits_cutoff(p)
    for fn in cases.values():                                   # warm-up: code objects, sort plans, buffers
        fn()
        fn()
    runs = {name: [] for name in cases}
    for _ in range(reps):                                       # alternated
        for name, fn in cases.items():
            runs[name].append(wall(fn)[0])
    rows = {"cutoff_%g" % p: int(sum(len(r) for r in s.hits_cutoff(p))) for p in CUTOFFS}
    d2h = {}
    for name, fn in cases.items():
        before = s.d2h_bytes()
        fn()
        d2h[name] = s.d2h_bytes() - before
    return {"queries": len(queries), "entries": len(db), "search_ms": search_ms,
            "median_ms": {k: med(v) for k, v in runs.items()}, "rows": rows, "d2h_bytes": d2h, "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["bench", "q200"])
    a = ap.parse_args()
    out = {"reps": a.reps, "cutoffs": list(CUTOFFS)}
    with sat.Searcher(0) as s:
        if a.only in (None, "bench"):
            out["bench_shape"] = shape(s, sat.synth.make_db(125_000, 32), [sat.synth.make_query(32)], a.reps)
        if a.only in (None, "q200"):
            db = sat.synth.make_db(15_000, 4, 40, sort=True)
            pick = np.random.default_rng(5).choice(len(db), 200, replace=False)
            queries = [(*db.dense(int(i)), db.ssetypes(int(i))) for i in pick]
            out["q200_shape"] = shape(s, db, queries, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
