"""Cost of the transitive search on the GPU (sat_reach_*, sat_search_reach).  Writes one JSON object
(profiles/reach_cost.json).

* the add pass: sat_reach_add against sat_cluster_add on the same scores - 200 database members as queries x 15 000
  size-sorted entries of 4..40 SSEs at r = 128 -, both into an empty accumulator, warmed twice, then --reps alternated
  runs; cutoffs P = 1e-3 and P = 1 (every row a step: the contention case).  sat_cluster.hip is the parent commit's file,
  byte for byte, so this library's cluster_add is the parent's.  "call_ms": host wall clock around the call, both ending
  synchronised, each with the upload of the queries' table pointers and its wait.  "kernel_us": the kernels' own device
  time when the script runs itself under `rocprofv3 --kernel-trace` (--rocprof), in a run of its own.
* the compaction: sat_reach_frontier(0) and sat_reach_rows over N = 15 000 and N = 1 000 000 nodes with 0, 200 and N
  of them reached (as seeds).  "call_ms": wall clock of the Python call - three launches, the count's copy and the
  rows', and the host buffer of N records the call makes.  "kernel_us" (--rocprof): the summed device time of the
  call's reach_count, reach_scan and reach_scatter dispatches.
* end to end (--entries N): sat_search_reach from one seed on N entries with planted families - every tenth of the
  entries drawn, each ten times over, shuffled - against the all-vs-all clustering of the same database at the same P
  (what `-a -L P` runs: batches of 256, search, sat_cluster_add, labels).
* the bench line (--parent-lib PATH: the device library built from the parent commit): `bench.py --gpus 1 --steps 300
  --warmup 3` of this tree and of the parent's library (loaded through SAT_DEVICE_LIB), --bench-runs each, alternated
  with the side that goes first changing from pair to pair.

    python scripts/reach_cost.py [--reps 9] [--rocprof] [--entries 15000] [--parent-lib PATH --bench-runs 4] [--out FILE]
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
import cuda_satabsearch_amd as sat  # noqa: E402

CUTOFFS = (1e-3, 1.0)
WARM = 2


def summary(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def clocked(s, call):
    s.sync()
    t0 = time.perf_counter()
    call()
    s.sync()
    return (time.perf_counter() - t0) * 1e3


def passes(reps):
    db = sat.synth.make_db(15_000, 4, 40, sort=True)
    idx = np.random.default_rng(5).choice(len(db), 200, replace=False).astype(np.int32)
    out = {}
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries_from_db(idx, 0)
        search_ms = s.search(True, False, 128)[2]
        for p in CUTOFFS:
            runs = {"cluster_add": [], "reach_add": []}
            for k in range(WARM + reps):                        # alternated; the first WARM of each are dropped
                s.cluster_begin()                               # empty accumulators every time, outside the clock
                c = clocked(s, lambda: s.cluster_add(p, idx))
                s.reach_begin()
                r = clocked(s, lambda: s.reach_add(1, p, idx))
                if k >= WARM:
                    runs["cluster_add"].append(c)
                    runs["reach_add"].append(r)
            rows, count = s.reach_rows(cap=0)
            edges = s.cluster_labels()[2]
            out["q200 P=%g" % p] = {"queries": len(idx), "entries": len(db), "search_ms": search_ms, "steps": int(edges),
                                    "reached": int(count), "call_ms": {k: summary(v) for k, v in runs.items()}, "call_runs_ms": runs,
                                    "dispatches": WARM + reps}
    return out


def compaction(reps):
    db = sat.synth.make_db(15_000, 4, 40, sort=True)
    out = {}
    with sat.Searcher(0) as s:
        s.upload(db)
        for n in (15_000, 1_000_000):
            for reached in (0, 200, n):
                seeds = np.linspace(0, n - 1, reached).astype(np.int32) if reached else None
                s.reach_begin(seeds, n_nodes=n)
                runs = {"frontier": [], "rows": []}
                for k in range(WARM + reps):
                    f = clocked(s, lambda: s.reach_frontier(0, cap=n))
                    r = clocked(s, lambda: s.reach_rows(cap=n))
                    if k >= WARM:
                        runs["frontier"].append(f)
                        runs["rows"].append(r)
                out["N=%d reached=%d" % (n, reached)] = {"call_ms": {k: summary(v) for k, v in runs.items()}, "call_runs_ms": runs,
                                                         "dispatches": WARM + reps}
        s.reach_end()
    return out


def end_to_end(entries, p=1e-3):
    base = sat.synth.make_db(entries // 10, 4, 40, sort=False)
    members = np.random.default_rng(7).permutation(np.repeat(np.arange(len(base)), 10))
    db = base.subset(members)
    n = len(db)
    out = {"entries": n, "families": len(base), "members": 10, "pvalue": p, "restarts": 128}
    with sat.Searcher(0) as s:
        s.upload(db)
        t0 = time.perf_counter()
        rows, info = s.search_reach([0], p, maxstart=128)
        out["search_reach"] = {"wall_s": time.perf_counter() - t0, "info": info, "depths": np.bincount(rows["depth"]).tolist(),
                               "family_of_seed_reached": int(np.isin(np.nonzero(members == members[0])[0], rows["node"]).sum()),
                               "d2h_bytes": s.d2h_bytes()}
        before = s.d2h_bytes()
        t0 = time.perf_counter()
        s.cluster_begin()
        for lo in range(0, n, 256):
            idx = np.arange(lo, min(lo + 256, n), dtype=np.int32)
            s.set_queries_from_db(idx, lo)
            s.search_async(True, False, 128)
            s.cluster_add(p, idx)
        labels, degrees, edges = s.cluster_labels()
        out["all_vs_all_cluster"] = {"wall_s": time.perf_counter() - t0, "edges": int(edges),
                                     "component_of_seed": int((labels == labels[0]).sum()), "d2h_bytes": s.d2h_bytes() - before}
    return out


def bench_alternated(parent_lib, runs):
    """bench.py of this tree and of the parent's library, alternated: the JSON line's rate and step time of every run"""
    command = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "300", "--warmup", "3"]
    sides = (("this", {}), ("parent", {"SAT_DEVICE_LIB": os.path.abspath(parent_lib)}))
    out = {"command": "bench.py --gpus 1 --steps 300 --warmup 3", "order": [],
           "parent_is": "the device library built from the parent commit, loaded through SAT_DEVICE_LIB", "this": [], "parent": []}
    for k in range(runs):
        for side, env in (sides if k % 2 == 0 else sides[::-1]):        # this, parent, parent, this, ...: neither always goes first
            p = subprocess.run(command, env={**os.environ, **env}, capture_output=True, text=True, cwd=ROOT)
            if p.returncode != 0:
                raise SystemExit("bench.py (%s) failed: %s" % (side, p.stderr[-400:]))
            line = json.loads(p.stdout.strip().splitlines()[-1])
            out["order"].append(side)
            out[side].append({"scorings_per_s": line["value"], "ms_per_step": line["ms_per_step"]})
    return out


def kernel_times(trace_dir, passes_table, compaction_table, reps):
    """cut the trace's dispatches into the cases, in order: cluster_add / reach_add for the passes; for the compaction
    the three kernels of every call summed (the passes' own reach_rows call per cutoff comes first and is skipped)"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return "no kernel trace was written"
    durations = {"cluster_add": [], "reach_add": [], "reach_count": [], "reach_scan": [], "reach_scatter": []}
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        for k in durations:
            if k + "(" in r["Kernel_Name"] or r["Kernel_Name"].endswith(k):
                durations[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    at = 0
    for case, row in passes_table.items():
        n = row["dispatches"]
        cut = {k: durations[k][at + WARM:at + n] for k in ("cluster_add", "reach_add")}
        if any(len(v) != reps for v in cut.values()):
            return "the trace holds %d / %d dispatches, not the runs'" % (len(durations["cluster_add"]), len(durations["reach_add"]))
        row["kernel_us"] = {k: summary(v) for k, v in cut.items()}
        row["kernel_runs_us"] = cut
        at += n
    three = [durations[k] for k in ("reach_count", "reach_scan", "reach_scatter")]
    calls = [a + b + c for a, b, c in zip(*three)]
    at = len(passes_table)                                      # one reach_rows call per cutoff of the passes
    if len({len(v) for v in three}) != 1 or len(calls) != at + sum(2 * row["dispatches"] for row in compaction_table.values()):
        return "the trace holds %s compaction dispatches, not the runs'" % [len(v) for v in three]
    for case, row in compaction_table.items():
        n = row["dispatches"]
        mine = calls[at:at + 2 * n]                             # frontier, rows, frontier, rows, ...
        cut = {"frontier": mine[2 * WARM::2], "rows": mine[2 * WARM + 1::2]}
        row["kernel_us"] = {k: summary(v) for k, v in cut.items()}
        row["kernel_runs_us"] = cut
        at += 2 * n
    return "ok"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rocprof", action="store_true", help="the add passes once more under rocprofv3 --kernel-trace, for the kernels' own times")
    ap.add_argument("--inner", help=argparse.SUPPRESS)
    ap.add_argument("--entries", type=int, default=0)
    ap.add_argument("--parent-lib", help="libsatabsearch.so built from the parent commit: the bench line, alternated")
    ap.add_argument("--bench-runs", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.inner:                                                 # the traced child: the passes and the compaction, their tables to a file
        with open(a.inner, "w") as fh:
            json.dump({"passes": passes(a.reps), "compaction": compaction(a.reps)}, fh)
        return
    out = {"reps": a.reps, "cutoffs": list(CUTOFFS), "passes": passes(a.reps), "kernel_trace": "not traced", "compaction": compaction(a.reps),
           "notes": "call_ms of the compaction is the Python call: it includes the allocation (and for rows the zero fill) of a host "
                    "buffer of cap = N records.  At P = 1e-3 no row of the q200 shape qualifies (random synthetic structures): both "
                    "passes only read."}
    if a.rocprof:
        with tempfile.TemporaryDirectory() as tmp:
            table = os.path.join(tmp, "tables.json")
            p = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "--",
                                sys.executable, os.path.abspath(__file__), "--inner", table, "--reps", str(a.reps)], capture_output=True)
            if p.returncode != 0 or not os.path.exists(table):
                out["kernel_trace"] = "the traced run failed: %s" % p.stderr.decode()[-300:]
            else:
                traced = json.load(open(table))
                out["kernel_trace"] = kernel_times(os.path.join(tmp, "trace"), traced["passes"], traced["compaction"], a.reps)
                out["passes_traced"] = traced["passes"]
                out["compaction_traced"] = traced["compaction"]
    if a.entries:
        out["end_to_end"] = end_to_end(a.entries)
    if a.parent_lib:
        out["bench_alternated"] = bench_alternated(a.parent_lib, a.bench_runs)
    text = json.dumps(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
