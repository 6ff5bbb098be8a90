"""Cost of the fitted statistics (sat_score_histogram, sat_stats_fit) after a search, beside the selection calls they
feed, on the q200 shape (scripts/run_config.py q200: 200 database members as queries x 15 000 size-sorted entries of
4..40 SSEs).  Every case runs on the same finished search, warmed, alternated in one process, --reps runs each; times
are host wall clock around the call, which ends in a device synchronise and the copy of its result.  Prints one JSON
object (profiles/fit_cost.json).

* histogram       sat_score_histogram: the LDS histogram pass and 200 x 4097 x 4 bytes to the host
* count_1e-3      sat_hits_cutoff with no row buffer: the flag / count pass alone (cutoff_count), 4 bytes per query
* cutoff_1e-3     sat_hits_cutoff(1e-3), -p's selection on the built-in statistics
* topk10          sat_topk_hits(10), -k's selection on the built-in statistics
* fit             sat_stats_fit(0.01): histogram, 200 fits on the host, 200 tables to the device
* cutoff_fitted / topk10_fitted   the two selections again with the fit installed

Copied into the scripts/ of an older checkout it runs the cases that library has (the A/B run of the default path: the
selections on the built-in statistics must cost what they cost before).  Kernel times: the same script under `rocprofv3 --kernel-trace --stats` (--reps 1).

    python scripts/fit_cost.py [--reps 7] [--restarts 128]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_satabsearch_amd as sat  # noqa: E402
from cuda_satabsearch_amd import _native  # noqa: E402


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--restarts", type=int, default=128)
    a = ap.parse_args()
    raw = C.CDLL(_native.DEVICE_LIB)
    has_fit = hasattr(raw, "sat_stats_fit")
    db = sat.synth.make_db(15_000, 4, 40, sort=True)
    pick = np.random.default_rng(5).choice(len(db), 200, replace=False)
    queries = [(*db.dense(int(i)), db.ssetypes(int(i))) for i in pick]
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries)
        search_ms = s.search(True, False, a.restarts)[2]
        lib, counts = s._lib, np.zeros(len(queries), np.int32)
        cases = {
            "count_1e-3": lambda: lib.sat_hits_cutoff(s._ctx, 1e-3, 0, counts.ctypes.data, 0, None, None),
            "cutoff_1e-3": lambda: s.hits_cutoff(1e-3),
            "topk10": lambda: s.topk_hits(10),
        }
        if has_fit:
            cases["histogram"] = s.score_histogram
        for fn in cases.values():                     # warm-up: code objects, sort plans, buffers
            fn()
            fn()
        runs = {name: [] for name in cases}
        for _ in range(a.reps):                       # alternated
            for name, fn in cases.items():
                runs[name].append(wall(fn))
        out = {"library": os.path.basename(os.path.dirname(_native.DEVICE_LIB)), "queries": len(queries), "entries": len(db),
               "restarts": a.restarts, "search_ms": search_ms, "reps": a.reps}
        if has_fit:
            fitted = {"fit": lambda: s.fit_statistics(0.01), "cutoff_fitted": lambda: s.hits_cutoff(1e-3),
                      "topk10_fitted": lambda: s.topk_hits(10)}
            for fn in fitted.values():
                fn()
            runs.update({name: [] for name in fitted})
            for _ in range(a.reps):
                for name, fn in fitted.items():
                    runs[name].append(wall(fn))
            fits = s.fit_statistics(0.01)
            out["fitted_queries"] = int(fits["fitted"].sum())
            out["a_range"] = [float(fits["a"].min()), float(fits["a"].max())]
            out["b_range"] = [float(fits["b"].min()), float(fits["b"].max())]
            out["rows_fitted_1e-3"] = int(sum(len(r) for r in s.hits_cutoff(1e-3)))
            s.set_statistics(None)
        out["rows_builtin_1e-3"] = int(sum(len(r) for r in s.hits_cutoff(1e-3)))
        out["median_ms"] = {k: float(np.median(v)) for k, v in runs.items()}
        out["min_max_ms"] = {k: [float(min(v)), float(max(v))] for k, v in runs.items()}
        out["runs"] = runs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
