"""Cost of profiling a query's SSEs over its hits on the GPU (sat_profile_rows, CLI -W P).  Writes one JSON
object (profiles/profile_cost.json).

* the pass: sat_profile_rows against the parent's passes over the same searched state - sat_cluster_add at P = 1e-3 (few
  rows count: a block leaves after its count) and sat_cover_add at P = 1 (every row counts: every block does its
  n1 (n1 + 1) / 2 atomics) - for 200 database members as queries x 15 000 size-sorted entries of 4..40 SSEs, and for 16
  queries of 97..111 SSEs against the same entries.  Warmed twice, then --reps alternated runs, every add into an empty
  accumulator.  "call_ms": host wall clock around the call and a sync - the profile's includes its copy to the host
  ("d2h_bytes").  "kernel_us": the kernels' own device time when the script runs itself under `rocprofv3 --kernel-trace`
  (--rocprof); the profile's is profile_add plus profile_mirror.
* the price of keeping maps: the search of the 200 queries with lsoln = 1 against lsoln = 0, alternated, queued and
  waited for without a copy.
* end to end (--parent-cli: the command line of the parent commit, built to a second path): `-a db -W 1e-3` of this tree
  against `-a db -L 1e-3` of the parent on 15 000 entries, alternated, --cli-reps runs each, with the bytes either copied
  from the GPU.

    python scripts/profile_cost.py [--reps 9] [--rocprof] [--parent-cli PATH --cli-reps 2] [--out FILE]
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
WARM = 2
N = 15_000
# (the cutoff, the parent's pass it is measured against)
CASES = ((1e-3, "cluster_add"), (1.0, "cover_add"))


def clocked(s, call):
    s.sync()
    t0 = time.perf_counter()
    call()
    s.sync()
    return (time.perf_counter() - t0) * 1e3


def measure(s, name, nodes, reps, out):
    """both cutoffs on the searched state of `s`: the parent's pass and the profile alternated"""
    for p, other in CASES:
        begin, add = (s.cluster_begin, s.cluster_add) if other == "cluster_add" else (s.cover_begin, s.cover_add)
        runs = {other: [], "profile_rows": []}
        hits = None
        for k in range(WARM + reps):
            begin()
            a = clocked(s, lambda: add(p, np.maximum(nodes, 0)))
            before = s.d2h_bytes()
            holder = []
            b = clocked(s, lambda: holder.append(s.profile_rows(p, nodes)))
            hits, moved = holder[0][0], s.d2h_bytes() - before
            if k >= WARM:
                runs[other].append(a)
                runs["profile_rows"].append(b)
        out["%s P=%g" % (name, p)] = {"queries": len(nodes), "entries": s.n_entries, "against": other, "counted_rows": int(hits.sum()),
                                     "d2h_bytes": moved, "call_ms": {k: summary(v) for k, v in runs.items()}, "call_runs_ms": runs,
                                     "dispatches": WARM + reps}


def passes(reps):
    db = sat.synth.make_db(N, 4, 40, sort=True)
    idx = np.random.default_rng(5).choice(len(db), 200, replace=False).astype(np.int32)
    out, search = {}, {"lsoln0": [], "lsoln1": []}
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries_from_db(idx, 0)
        for k in range(WARM + reps):
            t0 = clocked(s, lambda: s.search_async(True, False, 128))
            t1 = clocked(s, lambda: s.search_async(True, True, 128))
            if k >= WARM:
                search["lsoln0"].append(t0)
                search["lsoln1"].append(t1)
        measure(s, "q200", idx, reps, out)
        big = [sat.synth.make_query(n, seed=sat.synth.QUERY_SEED + n) for n in np.linspace(97, 111, 16).astype(int)]
        s.set_queries(big)
        s.search_async(True, True, 128)
        measure(s, "q16 of 97..111", np.full(16, -1, np.int32), reps, out)
        s.cover_end()
        s.cluster_end()
    return {"passes": out, "search_ms": {k: summary(v) for k, v in search.items()}, "search_runs_ms": search,
            "map_bytes_on_device": int(db.orders[idx].astype(np.int64).sum()) * N}


def kernel_times(trace_dir, table, reps):
    """cut the trace's dispatches of the passes' kernels into the cases, in order"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return "no kernel trace was written"
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    durations = {"cluster_add": [], "cover_add": [], "profile_add": [], "profile_mirror": []}
    for r in rows:
        for k in durations:
            if k in r["Kernel_Name"] and "levels" not in r["Kernel_Name"]:
                durations[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    durations["profile_mirror"] = durations["profile_mirror"][1:]       # the empty launch that loads the code object
    at = {k: 0 for k in durations}
    for case, row in table.items():
        n, other = row["dispatches"], row["against"]
        cut = {}
        for k in (other, "profile_add", "profile_mirror"):
            cut[k] = durations[k][at[k] + WARM:at[k] + n]
            at[k] += n
            if len(cut[k]) != reps:
                return "the trace holds %s dispatches, not the runs'" % {k: len(v) for k, v in durations.items()}
        cut["profile_rows"] = [a + b for a, b in zip(cut["profile_add"], cut["profile_mirror"])]
        row["kernel_us"] = {k: summary(v) for k, v in cut.items()}
        row["kernel_runs_us"] = cut
    return "ok"


def end_to_end(parent_cli, reps):
    db = sat.synth.make_db(N, 4, 40, sort=True)
    with tempfile.TemporaryDirectory() as tmp:
        db.write_ascii(os.path.join(tmp, "db.ascii"))
        runs = {"W": [], "L_parent": []}
        for _ in range(reps):                                   # alternated
            runs["W"].append(cli_run(CLI, ["-a", "db.ascii", "-W", "0.001"], tmp))
            runs["L_parent"].append(cli_run(parent_cli, ["-a", "db.ascii", "-L", "0.001"], tmp))
    return {"entries": N, "pvalue": 1e-3, "restarts": 128, "runs": runs,
            "wall_s": {k: summary([r["wall_s"] for r in v]) for k, v in runs.items()},
            "gpu_ms": {k: summary([r["gpu_ms"] for r in v]) for k, v in runs.items()},
            "d2h_bytes": {k: v[0]["d2h_bytes"] for k, v in runs.items()},
            "stdout_bytes": {k: v[0]["stdout_bytes"] for k, v in runs.items()}}


def traced_passes(reps, rocprof):
    """the passes in a child process, under rocprofv3 when asked"""
    with tempfile.TemporaryDirectory() as tmp:
        table = os.path.join(tmp, "passes.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--inner", table, "--reps", str(reps)]
        if rocprof:
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "--"] + cmd
        p = subprocess.run(cmd, capture_output=True)
        if p.returncode != 0 or not os.path.exists(table):
            raise SystemExit("the passes failed: %s" % p.stderr.decode()[-600:])
        result = json.load(open(table))
        trace = kernel_times(os.path.join(tmp, "trace"), result["passes"], reps) if rocprof else "not traced"
    return result, trace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rocprof", action="store_true", help="run the passes under rocprofv3 --kernel-trace for the kernels' own times")
    ap.add_argument("--inner", help=argparse.SUPPRESS)
    ap.add_argument("--parent-cli")
    ap.add_argument("--cli-reps", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.inner:                                                 # the child: the passes, their table to a file
        with open(a.inner, "w") as fh:
            json.dump(passes(a.reps), fh)
        return
    out = {"reps": a.reps}
    result, out["kernel_trace"] = traced_passes(a.reps, a.rocprof)
    out.update(result)
    if a.parent_cli:
        out["end_to_end"] = end_to_end(os.path.abspath(a.parent_cli), a.cli_reps)
    text = json.dumps(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
