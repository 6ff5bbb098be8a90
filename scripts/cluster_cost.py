"""Cost of clustering the database on the GPU (sat_cluster_add, CLI -a -L P).  Writes one JSON object
(profiles/cluster_cost.json).

* the pass: sat_cluster_add against sat_cutoff_count - sat_hits_cutoff asked for its counts only -, the flag pass that
  reads the same scores through the same predicate.  Both on the same searched state, warmed twice, then --reps
  alternated runs, every add into an empty accumulator; cutoffs P = 1e-3 and P = 1 (every row an edge: the contention
  case, reported, not judged).
    q200 shape: 200 database members as queries x 15 000 size-sorted entries of 4..40 SSEs;
    one -a batch: the first 256 entries of that database as queries.
  Two clocks.  "call_ms": host wall clock around the call, both ending synchronised (the count pass by its own copy,
  the add by sat_sync) - each includes the upload of the queries' table pointers and its wait.  "kernel_us": the
  kernels' own device time, when the script runs itself under `rocprofv3 --kernel-trace` (--rocprof): the durations of
  the cutoff_count and cluster_add dispatches in the trace, in the order the runs made them.
* end to end (--entries N, needs --parent-cli: the command line of the parent commit, built to a second path):
  `-a db -L 1e-3` of this tree against `-a db -p 1e-3` of the parent, alternated, --cli-reps runs each: wall clock of
  the process, the summed "GPU execution time" lines, stdout bytes, and the "copied N bytes" line of either.

    python scripts/cluster_cost.py [--reps 9] [--rocprof] [--entries 15000 --parent-cli PATH --cli-reps 2] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_satabsearch_amd as sat  # noqa: E402

CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
CUTOFFS = (1e-3, 1.0)
WARM = 2


def summary(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def passes(reps):
    """the alternated runs; returns the wall-clock table and, case by case, how many dispatches of either kernel the
    case made (a trace is cut by these)"""
    db = sat.synth.make_db(15_000, 4, 40, sort=True)
    shapes = {"q200": np.random.default_rng(5).choice(len(db), 200, replace=False).astype(np.int32),
              "batch256": np.arange(256, dtype=np.int32)}
    out = {}
    with sat.Searcher(0) as s:
        lib, ctx = s._lib, s._ctx
        s.upload(db)
        for name, idx in shapes.items():
            s.set_queries_from_db(idx, 0)
            search_ms = s.search(True, False, 128)[2]
            counts = np.zeros(len(idx), np.int32)
            for p in CUTOFFS:
                def count():
                    t0 = time.perf_counter()
                    rows = lib.sat_hits_cutoff(ctx, p, 0, counts.ctypes.data, 0, None, None)
                    assert rows >= 0
                    return (time.perf_counter() - t0) * 1e3, rows

                def add():
                    s.cluster_begin()                           # an empty accumulator every time, outside the clock
                    s.sync()
                    t0 = time.perf_counter()
                    s.cluster_add(p, idx)
                    s.sync()
                    return (time.perf_counter() - t0) * 1e3

                runs = {"count": [], "add": []}
                for k in range(WARM + reps):                    # alternated; the first WARM of each are dropped
                    c, rows = count()
                    a = add()
                    if k >= WARM:
                        runs["count"].append(c)
                        runs["add"].append(a)
                out["%s P=%g" % (name, p)] = {"queries": len(idx), "entries": len(db), "search_ms": search_ms, "rows": int(rows),
                                              "call_ms": {k: summary(v) for k, v in runs.items()}, "call_runs_ms": runs,
                                              "dispatches": WARM + reps}
                labels, degrees, edges = s.cluster_labels()
                out["%s P=%g" % (name, p)].update(edges=edges, clusters=int(len(set(labels.tolist()))))
    return out


def kernel_times(trace_dir, table, reps):
    """cut the trace's cutoff_count / cluster_add dispatches into the cases, in order"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return "no kernel trace was written"
    durations = {"cutoff_count": [], "cluster_add": []}
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        for k in durations:
            if k in r["Kernel_Name"]:
                durations[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    at = 0
    for case, row in table.items():
        if "dispatches" not in row:
            continue
        n = row["dispatches"]
        cut = {"count": durations["cutoff_count"][at + WARM:at + n], "add": durations["cluster_add"][at + WARM:at + n]}
        if len(cut["count"]) != reps or len(cut["add"]) != reps:
            return "the trace holds %d / %d dispatches, not the runs'" % (len(durations["cutoff_count"]), len(durations["cluster_add"]))
        row["kernel_us"] = {k: summary(v) for k, v in cut.items()}
        row["kernel_runs_us"] = cut
        at += n
    return "ok"


def cli_run(cli, args, cwd):
    t0 = time.perf_counter()
    p = subprocess.run([cli] + args, input=b"", cwd=cwd, capture_output=True)
    wall = time.perf_counter() - t0
    err = p.stderr.decode()
    if p.returncode != 0:
        raise SystemExit("%s %s failed: %s" % (cli, " ".join(args), err[-400:]))
    copied = re.search(r"copied (\d+) bytes of results", err)
    return {"wall_s": wall, "gpu_ms": sum(float(x) for x in re.findall(r"GPU execution time ([0-9.]+) ms", err)),
            "stdout_bytes": len(p.stdout), "d2h_bytes": int(copied.group(1)) if copied else None,
            "head": p.stdout[:200].decode(errors="replace").splitlines()[0] if p.stdout else ""}


def end_to_end(entries, parent_cli, reps):
    db = sat.synth.make_db(entries, 4, 40, sort=True)
    with tempfile.TemporaryDirectory() as tmp:
        db.write_ascii(os.path.join(tmp, "db.ascii"))
        runs = {"L": [], "p_parent": []}
        for _ in range(reps):                                   # alternated
            runs["L"].append(cli_run(CLI, ["-a", "db.ascii", "-L", "0.001"], tmp))
            runs["p_parent"].append(cli_run(parent_cli, ["-a", "db.ascii", "-p", "0.001"], tmp))
    return {"entries": entries, "pvalue": 1e-3, "restarts": 128, "runs": runs,
            "wall_s": {k: summary([r["wall_s"] for r in v]) for k, v in runs.items()},
            "gpu_ms": {k: summary([r["gpu_ms"] for r in v]) for k, v in runs.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rocprof", action="store_true", help="run the passes under rocprofv3 --kernel-trace for the kernels' own times")
    ap.add_argument("--inner", help=argparse.SUPPRESS)
    ap.add_argument("--entries", type=int, default=15_000)
    ap.add_argument("--parent-cli")
    ap.add_argument("--cli-reps", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.inner:                                                 # the traced child: the passes, their table to a file
        with open(a.inner, "w") as fh:
            json.dump(passes(a.reps), fh)
        return
    out = {"reps": a.reps, "cutoffs": list(CUTOFFS)}
    if a.rocprof:
        with tempfile.TemporaryDirectory() as tmp:
            table = os.path.join(tmp, "passes.json")
            p = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "--",
                                sys.executable, os.path.abspath(__file__), "--inner", table, "--reps", str(a.reps)],
                               capture_output=True)
            if p.returncode != 0 or not os.path.exists(table):
                raise SystemExit("the traced run failed: %s" % p.stderr.decode()[-600:])
            out["passes"] = json.load(open(table))
            out["kernel_trace"] = kernel_times(os.path.join(tmp, "trace"), out["passes"], a.reps)
    else:
        out["passes"] = passes(a.reps)
        out["kernel_trace"] = "not traced"
    if a.parent_cli:
        out["end_to_end"] = end_to_end(a.entries, os.path.abspath(a.parent_cli), a.cli_reps)
    text = json.dumps(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
