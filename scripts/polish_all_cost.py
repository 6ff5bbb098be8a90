"""Cost of the whole-database polish (sat_polish_all_set) against the plain search, against itself with
the polish forced onto one wave per map, and against the only way the parent commit had to the same rows:
search_pairs_polish over all nq x N pairs.  Routes alternated in one process, warmed, medians of --reps runs; wall time
from the first launch to the rows standing in device memory (the pair route: on the host, where it puts them).  Prints
one JSON object (profiles/polish_all_cost.json).

Shapes, r = 128: the bench shape (32-SSE query x 125 000 32-SSE entries), a 19-SSE query x 100 000 size-sorted entries
of 8..32 SSEs, a 101-SSE query x 10 000 entries of the C5 order mix (reported only).

SAT_EXP_POLISH_GROUP is read when a context is created, so the forced width 64 runs on a context of its own made under
it.  A library is loaded once per process, so --parent-lib PATH (a libsatabsearch.so built from the parent commit) runs
its routes - the pair route at T = 8 and, as the yardstick between the two processes, the plain search - in a child
process through SAT_DEVICE_LIB, after this process's own runs.

    python scripts/polish_all_cost.py [--reps 5] [--quick] [--parent-lib PATH]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/polish_all_cost.py --passes
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_satabsearch_amd as sat  # noqa: E402
from cuda_satabsearch_amd import workloads  # noqa: E402

R, TOPS = 128, (1, 4, 8)


def shapes(quick):
    q2 = workloads.load_queries("d2phlb1.input")[0]
    out = [("bench_shape", lambda: sat.synth.make_db(125_000, 32), sat.synth.make_query(32)),
           ("q19_sorted_8_32", lambda: workloads.mixed_db(100_000), (q2[1], q2[2], q2[3]))]
    if not quick:
        q4 = workloads.config4_query()
        out.append(("q101_c5_10000", lambda: workloads.config4_db(10_000), (q4[1], q4[2], q4[3])))
    return out


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def timed(routes, reps):
    for fn in routes.values():                                  # warm-up: code objects, scratch
        fn()
    runs = {name: [] for name in routes}
    for _ in range(reps):                                       # alternated
        for name, fn in routes.items():
            runs[name].append(wall(fn))
    res = {name: float(np.median(v)) for name, v in runs.items()}
    res["spread"] = {name: float(max(v) - min(v)) for name, v in runs.items()}
    res["runs"] = runs
    return res


def searcher(db, q, env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    s = sat.Searcher(0)
    for k, v in old.items():
        if v is None:
            del os.environ[k]
        else:
            os.environ[k] = v
    s.upload(db)
    s.set_queries([q])
    return s


def mode(s, tops):
    def run():
        s.set_polish_all(tops)
        s.search_async(True, False, R)
        s.sync()
        s.set_polish_all(0)
    return run


def plain(s):
    def run():
        s.search_async(True, False, R)
        s.sync()
    return run


def pairs(s, n, tops):
    zeros, every = np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
    return lambda: s.search_pairs_polish(zeros, every, tops, True, R)


def own_routes(db, q, reps):
    s, wide = searcher(db, q), searcher(db, q, {"SAT_EXP_POLISH_GROUP": "64"})
    routes = {"plain_ms": plain(s)}
    for t in TOPS:
        routes["all_T%d_ms" % t] = mode(s, t)
    routes["all_T8_width64_ms"] = mode(wide, 8)
    routes["pairs_T8_ms"] = pairs(s, len(db), 8)
    res = timed(routes, reps)
    s.set_polish_all(8)
    s.search_async(True, False, R)
    s.sync()
    res["launch"] = s.last_launch_info()
    res["entries"] = len(db)
    s.close()
    wide.close()
    return res


def parent_routes(db, q, reps):
    s = searcher(db, q)
    res = timed({"parent_plain_ms": plain(s), "parent_pairs_T8_ms": pairs(s, len(db), 8)}, reps)
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="two shapes, one run (for a kernel-trace run)")
    ap.add_argument("--parent-lib", help="libsatabsearch.so of the parent commit: its routes run in a child process")
    ap.add_argument("--as-parent", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--passes", action="store_true",
                    help="only the mode at T = 8, three searches a shape behind a warm-up: the run to put under "
                         "rocprofv3 --kernel-trace --stats for the split into passes")
    args = ap.parse_args()
    reps = 1 if args.quick else args.reps
    res = {}
    if args.passes:
        for name, make, q in shapes(True):
            s = searcher(make(), q)
            for _ in range(4):
                mode(s, 8)()
            s.close()
        return
    for name, make, q in shapes(args.quick):
        db = make()
        res[name] = parent_routes(db, q, reps) if args.as_parent else own_routes(db, q, reps)
    if args.parent_lib and not args.as_parent:
        env = dict(os.environ, SAT_DEVICE_LIB=os.path.abspath(args.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--as-parent", "--reps", str(reps)] + (["--quick"] if args.quick else [])
        run = subprocess.run(cmd, env=env, capture_output=True)
        if run.returncode != 0:
            sys.stderr.write(run.stderr.decode()[-2000:])
            print(json.dumps(res))
            sys.exit("the parent library's routes failed (status %d); this library's are printed" % run.returncode)
        child = json.loads(run.stdout)
        for name, r in res.items():
            for k, v in child[name].items():
                if k in ("spread", "runs"):
                    r[k].update(v)
                else:
                    r[k] = v
            # the two processes are compared through their plain searches
            r["parent_pairs_T8_over_all_T8"] = (r["parent_pairs_T8_ms"] / r["parent_plain_ms"]) / (r["all_T8_ms"] / r["plain_ms"])
    for r in ([] if args.as_parent else res.values()):
        for t in TOPS:
            r["all_T%d_over_plain" % t] = r["all_T%d_ms" % t] / r["plain_ms"]
        r["width64_over_groups_T8"] = r["all_T8_width64_ms"] / r["all_T8_ms"]
        r["pairs_T8_over_all_T8"] = r["pairs_T8_ms"] / r["all_T8_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
