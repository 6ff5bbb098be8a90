"""Cost of clustering the database around representatives on the GPU (sat_cover_*, CLI -a -D P).  Writes one
JSON object (profiles/cover_cost.json).

* the add pass: sat_cover_add against sat_cluster_add - what it replaces in the run - on the same searched state: 200
  database members as queries x 15 000 size-sorted entries of 4..40 SSEs, at P = 1e-3 (few edges) and P = 1 (every row
  an edge: the contention worst case).  Warmed twice, then --reps alternated runs, every add into an empty accumulator.
  "call_ms": host wall clock around the call and a sync.  "kernel_us": the kernels' own device time when the script runs
  itself under `rocprofv3 --kernel-trace` (--rocprof).  --variant NAME=LIB repeats the pass in a child process on another
  build of the device library (SAT_DEVICE_LIB), e.g. one compiled with -DSAT_COVER_PEEL=0: no combining before the atomic.
* the solve at 15 000 nodes for three planted graphs - 300 stars of 50, the random graph of the tests scaled (200 000
  cells), the perfect matching (7 500 rounds: the round-count worst case): wall clock of sat_cover_solve, --reps runs of
  the same matrix, and the time per round with it.  The graphs are planted through the test hook, 1 000 queries a batch.
* end to end (--parent-cli: the command line of the parent commit, built to a second path): `-a db -D 1e-3` of this tree
  against `-a db -L 1e-3` of the parent, alternated, --cli-reps runs each.
* sharded: the bytes a two-shard solve copies to the host, counted by sat_multi_stat_d2h_bytes.

    python scripts/cover_cost.py [--reps 9] [--rocprof] [--variant NAME=LIB] [--parent-cli PATH --cli-reps 2] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import cuda_satabsearch_amd as sat  # noqa: E402
from cluster_cost import cli_run, summary  # noqa: E402

CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
CUTOFFS = (1e-3, 1.0)
WARM = 2
N = 15_000


def add_pass(reps):
    """cluster_add and cover_add alternated on one searched state, each into an empty accumulator begun outside the clock"""
    db = sat.synth.make_db(N, 4, 40, sort=True)
    idx = np.random.default_rng(5).choice(len(db), 200, replace=False).astype(np.int32)
    out = {}
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries_from_db(idx, 0)
        search_ms = s.search(True, False, 128)[2]
        for p in CUTOFFS:
            def timed(begin, add):
                begin()
                s.sync()
                t0 = time.perf_counter()
                add(p, idx)
                s.sync()
                return (time.perf_counter() - t0) * 1e3

            runs = {"cluster_add": [], "cover_add": []}
            for k in range(WARM + reps):
                c = timed(s.cluster_begin, s.cluster_add)
                v = timed(s.cover_begin, s.cover_add)
                if k >= WARM:
                    runs["cluster_add"].append(c)
                    runs["cover_add"].append(v)
            rep, degree, edges, rounds = s.cover_solve()
            out["q200 P=%g" % p] = {"queries": len(idx), "entries": len(db), "search_ms": search_ms, "edges": edges, "rounds": rounds,
                                   "call_ms": {k: summary(v) for k, v in runs.items()}, "call_runs_ms": runs,
                                   "dispatches": WARM + reps}
        s.cover_end()
        s.cluster_end()
    return out


def kernel_times(trace_dir, table, reps):
    """cut the trace's cluster_add / cover_add dispatches into the cases, in order"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return "no kernel trace was written"
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    durations = {"cluster_add": [], "cover_add": []}
    for r in rows:
        for k in durations:
            if k in r["Kernel_Name"] and "levels" not in r["Kernel_Name"]:
                durations[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    at = 0
    for case, row in table.items():
        n = row["dispatches"]
        cut = {k: v[at + WARM:at + n] for k, v in durations.items()}
        if any(len(v) != reps for v in cut.values()):
            return "the trace holds %s dispatches, not the runs'" % {k: len(v) for k, v in durations.items()}
        row["kernel_us"] = {k: summary(v) for k, v in cut.items()}
        row["kernel_runs_us"] = cut
        at += n
    return "ok"


def planted_cells(name):
    """(query rows, entry columns) of the planted graph over N nodes; one direction is enough - the add sets both bits"""
    rng = np.random.default_rng(1)
    if name == "stars":                                         # 300 hubs, 49 leaves each: hub 50 i, leaves behind it
        leaves = np.arange(N)
        leaves = leaves[leaves % 50 != 0]
        return leaves // 50 * 50, leaves
    if name == "random":                                        # the tests' 20 000 cells over 1 500 nodes, ten times over
        return rng.integers(0, N, 200_000), rng.integers(0, N, 200_000)
    return np.arange(1, N, 2), np.arange(0, N, 2)               # perfect matching


def solves(reps):
    db = sat.synth.make_db(N, 8, 20, sort=False)                # the tests' planted database: norm2 = 16 qualifies at 1e-3
    out = {}
    batch = 1000
    with sat.Searcher(0) as s:
        s.upload(db)
        for name in ("stars", "random", "matching"):
            q, e = planted_cells(name)
            s.cover_begin()
            for lo in range(0, N, batch):
                hi = min(lo + batch, N)
                keep = (q >= lo) & (q < hi)
                scores = np.zeros((hi - lo, N), np.int32)
                scores[q[keep] - lo, e[keep]] = 8 * (db.orders[q[keep]] + db.orders[e[keep]])
                s.set_queries_from_db(np.arange(lo, hi), lo)
                s.search(True, False, 1)
                s.debug_set_scores(scores)
                s.cover_add(1e-3, np.arange(lo, hi))
            s.sync()
            runs = []
            for k in range(WARM + reps):
                t0 = time.perf_counter()
                rep, degree, edges, rounds = s.cover_solve()
                if k >= WARM:
                    runs.append((time.perf_counter() - t0) * 1e3)
            sizes, clusters = sat.report.cover_sizes(rep)
            out[name] = {"nodes": N, "edges": edges, "rounds": rounds, "clusters": clusters, "largest": int(sizes.max()),
                         "matrix_bytes": N * ((N + 63) // 64) * 8, "solve_ms": summary(runs), "solve_runs_ms": runs,
                         "us_per_round": float(np.median(runs)) * 1e3 / max(rounds, 1)}
    return out


def sharded_bytes():
    """two shards on GPU 0: what the solve copies to the host, beside the formula"""
    db = sat.synth.make_db(N, 4, 40, sort=True)
    with sat.MultiSearcher(2, devices=[0, 0]) as m:
        m.upload(db)
        m.set_queries_from_db(np.arange(64), 0)
        m.search_only(True, False, 1)
        m.cover_begin()
        m.cover_add(1.0, np.arange(64))
        before = m.d2h_bytes()
        rep, degree, edges, rounds = m.cover_solve()
        moved = m.d2h_bytes() - before
    matrix = N * ((N + 63) // 64) * 8
    return {"shards": 2, "nodes": N, "matrix_bytes": matrix, "solve_d2h_bytes": moved, "rounds": rounds,
            "per_extra_shard_d2h_bytes": moved - (8 * N + 24 + 8 * (rounds // 64 + 1)), "per_extra_shard_h2d_bytes": matrix}


def end_to_end(parent_cli, reps):
    db = sat.synth.make_db(N, 4, 40, sort=True)
    with tempfile.TemporaryDirectory() as tmp:
        db.write_ascii(os.path.join(tmp, "db.ascii"))
        runs = {"D": [], "L_parent": []}
        for _ in range(reps):                                   # alternated
            runs["D"].append(cli_run(CLI, ["-a", "db.ascii", "-D", "0.001"], tmp))
            runs["L_parent"].append(cli_run(parent_cli, ["-a", "db.ascii", "-L", "0.001"], tmp))
    return {"entries": N, "pvalue": 1e-3, "restarts": 128, "runs": runs,
            "wall_s": {k: summary([r["wall_s"] for r in v]) for k, v in runs.items()},
            "gpu_ms": {k: summary([r["gpu_ms"] for r in v]) for k, v in runs.items()}}


def traced_add_pass(reps, rocprof, env=None):
    """the add pass in a child process (another library: env), under rocprofv3 when asked"""
    with tempfile.TemporaryDirectory() as tmp:
        table = os.path.join(tmp, "passes.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--inner", table, "--reps", str(reps)]
        if rocprof:
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "--"] + cmd
        p = subprocess.run(cmd, capture_output=True, env=dict(os.environ, **(env or {})))
        if p.returncode != 0 or not os.path.exists(table):
            raise SystemExit("the add pass failed: %s" % p.stderr.decode()[-600:])
        passes = json.load(open(table))
        trace = kernel_times(os.path.join(tmp, "trace"), passes, reps) if rocprof else "not traced"
    return passes, trace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rocprof", action="store_true", help="run the add pass under rocprofv3 --kernel-trace for the kernels' own times")
    ap.add_argument("--inner", help=argparse.SUPPRESS)
    ap.add_argument("--variant", action="append", default=[], help="NAME=LIB: the add pass once more on that build of the device library")
    ap.add_argument("--parent-cli")
    ap.add_argument("--cli-reps", type=int, default=2)
    ap.add_argument("--skip-solves", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.inner:                                                 # the child: the add pass, its table to a file
        with open(a.inner, "w") as fh:
            json.dump(add_pass(a.reps), fh)
        return
    out = {"reps": a.reps, "cutoffs": list(CUTOFFS)}
    out["add_pass"], out["kernel_trace"] = traced_add_pass(a.reps, a.rocprof)
    for spec in a.variant:
        name, lib = spec.split("=", 1)
        passes, trace = traced_add_pass(a.reps, a.rocprof, {"SAT_DEVICE_LIB": os.path.abspath(lib)})
        out["add_pass " + name] = passes
        out["kernel_trace " + name] = trace
    if not a.skip_solves:
        out["solve"] = solves(a.reps)
        out["sharded"] = sharded_bytes()
    if a.parent_cli:
        out["end_to_end"] = end_to_end(os.path.abspath(a.parent_cli), a.cli_reps)
    text = json.dumps(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
