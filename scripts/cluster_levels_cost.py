"""Cost of clustering the database at several p-values in one pass (sat_cluster_add_levels, CLI -a -H P1,..,PL;
DESIGN.md 6p).  Writes one JSON object (profiles/cluster_levels_cost.json).

* the pass (--parent-lib: the device library of the parent commit, built to a second path): sat_cluster_add_levels of
  this tree at L = 1, 4, 8 against the parent's sat_cluster_add called L times - once is its L = 1 - on the same searched
  states, the two of scripts/cluster_cost.py:
    q200 shape: 200 database members as queries x 15 000 size-sorted entries of 4..40 SSEs;
    one -a batch: the first 256 entries of that database as queries.
  Two cutoff sets: "none" - cutoffs so small that no row qualifies, nothing is added (self rows are no edges whatever
  their p-value) - and "all" - the tightest level already takes every row: every row an edge of every level, the
  contention case, reported, not judged.  A library is one process (SAT_DEVICE_LIB is read when the package loads it), so
  the alternation is of processes: --rounds times this tree, the parent and - with --climb-all-lib, this tree built with
  -DSAT_CLUSTER_CLIMB_ALL, the early stop compiled out - that one, each process under `rocprofv3 --kernel-trace` of its
  own, warmed twice per case, then --reps runs, every add into an empty accumulator.  Two clocks, as cluster_cost.py:
  "call_ms" - host wall clock around the add call(s), ending synchronised - and "kernel_us" - the durations of the
  cluster_add / cluster_add_levels dispatches in the trace, the parent's L dispatches of a run summed.
* end to end (--parent-cli: the command line of the parent commit): `-a db -H 1e-5,1e-4,1e-3,1e-2` of this tree against
  `-a db -L 1e-3` of the parent, --entries size-sorted entries of 4..40 SSEs at r = 128, alternated, --cli-reps runs each:
  wall clock of the process and the summed "GPU execution time" lines.
* the bench line (--bench, with --parent-lib): `bench.py --gpus 1 --steps 100` with this tree's library and with the
  parent's through SAT_DEVICE_LIB, alternated three times.

    python scripts/cluster_levels_cost.py --parent-lib PATH [--climb-all-lib PATH] [--reps 9] [--rounds 3]
                                          [--parent-cli PATH --entries 15000 --cli-reps 3] [--bench] [--out FILE]
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
LEVELS = (1, 4, 8)
WARM = 2
H_LIST = "1e-5,1e-4,1e-3,1e-2"


def cutoffs(kind, levels):
    """"none": no row's p-value is that small; "all": the tightest is above every row's (the largest a row of a score
    >= 0 shows is 0.943..)"""
    if kind == "none":
        return np.geomspace(1e-300, 1e-290, levels)[:levels] if levels > 1 else np.array([1e-300])
    return np.linspace(0.95, 1.0, levels) if levels > 1 else np.array([1.0])


def summary(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def passes(reps, leveled):
    """one library's runs: case -> wall clocks, and the kernel dispatches each run made (the trace is cut by them)"""
    db = sat.synth.make_db(15_000, 4, 40, sort=True)
    shapes = {"q200": np.random.default_rng(5).choice(len(db), 200, replace=False).astype(np.int32),
              "batch256": np.arange(256, dtype=np.int32)}
    out = {}
    with sat.Searcher(0) as s:
        s.upload(db)
        for name, idx in shapes.items():
            s.set_queries_from_db(idx, 0)
            search_ms = s.search(True, False, 128)[2]
            for kind in ("none", "all"):
                for levels in LEVELS:
                    cuts = cutoffs(kind, levels)

                    def run():
                        if leveled:
                            s.cluster_begin_levels(cuts)                # an empty accumulator every time, outside the clock
                            s.sync()
                            t0 = time.perf_counter()
                            s.cluster_add_levels(idx)
                            s.sync()
                            return (time.perf_counter() - t0) * 1e3
                        total = 0.0
                        for p in cuts:                                  # what L runs of -L cost: an empty accumulator each
                            s.cluster_begin()
                            s.sync()
                            t0 = time.perf_counter()
                            s.cluster_add(float(p), idx)
                            s.sync()
                            total += (time.perf_counter() - t0) * 1e3
                        return total

                    runs = [run() for _ in range(WARM + reps)][WARM:]
                    if leveled:
                        edges = [int(e) for e in s.cluster_labels_levels()[2]]
                    else:
                        edges = [int(s.cluster_labels()[2])]            # of the last cutoff, the loosest
                    out["%s %s L=%d" % (name, kind, levels)] = {
                        "queries": len(idx), "entries": len(db), "search_ms": search_ms, "cutoffs": cuts.tolist(), "edges": edges,
                        "call_ms": summary(runs), "call_runs_ms": runs, "runs": WARM + reps, "dispatches_per_run": 1 if leveled else levels}
    return out


def kernel_times(trace_dir, table, leveled):
    """the trace's cluster_add / cluster_add_levels dispatches cut into the cases, in order; a run's dispatches summed"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return "no kernel trace was written"
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    want = "cluster_add_levels(" if leveled else "cluster_add("
    durations = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if want in r["Kernel_Name"]]
    at = 0
    for case, row in table.items():
        per, runs = row["dispatches_per_run"], row["runs"]
        cut = durations[at:at + per * runs]
        if len(cut) != per * runs:
            return "the trace holds %d dispatches of %s, fewer than the runs made" % (len(durations), want)
        sums = [float(sum(cut[k * per:(k + 1) * per])) for k in range(runs)][WARM:]
        row["kernel_us"] = summary(sums)
        row["kernel_runs_us"] = sums
        at += per * runs
    return "ok" if at == len(durations) else "the trace holds %d dispatches, the runs made %d" % (len(durations), at)


def traced(lib, reps, leveled):
    """one process of the passes under rocprofv3 --kernel-trace, its device library `lib` (None: this tree's)"""
    env = dict(os.environ)
    env.pop("SAT_DEVICE_LIB", None)
    if lib:
        env["SAT_DEVICE_LIB"] = os.path.abspath(lib)
    with tempfile.TemporaryDirectory() as tmp:
        table = os.path.join(tmp, "passes.json")
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "--",
                            sys.executable, os.path.abspath(__file__), "--inner", table, "--reps", str(reps)]
                           + (["--inner-leveled"] if leveled else []), capture_output=True, env=env)
        if p.returncode != 0 or not os.path.exists(table):
            raise SystemExit("the traced run failed: %s" % p.stderr.decode()[-600:])
        out = json.load(open(table))
        status = kernel_times(os.path.join(tmp, "trace"), out, leveled)
    return out, status


def merge(rounds):
    """the rounds of one library: per case the runs of every round together"""
    out = {}
    for case in rounds[0]:
        row = dict(rounds[0][case])
        for key in ("call_runs_ms", "kernel_runs_us"):
            if key in row:
                row[key] = [v for r in rounds for v in r[case][key]]
        row["call_ms"] = summary(row["call_runs_ms"])
        if "kernel_runs_us" in row:
            row["kernel_us"] = summary(row["kernel_runs_us"])
        row["rounds"] = len(rounds)
        out[case] = row
    return out


def cli_run(cli, args, cwd):
    t0 = time.perf_counter()
    p = subprocess.run([cli] + args, input=b"", cwd=cwd, capture_output=True)
    wall = time.perf_counter() - t0
    err = p.stderr.decode()
    if p.returncode != 0:
        raise SystemExit("%s %s failed: %s" % (cli, " ".join(args), err[-400:]))
    return {"wall_s": wall, "gpu_ms": sum(float(x) for x in re.findall(r"GPU execution time ([0-9.]+) ms", err)),
            "stdout_bytes": len(p.stdout), "head": p.stdout.decode(errors="replace").splitlines()[:5]}


def end_to_end(entries, parent_cli, reps):
    db = sat.synth.make_db(entries, 4, 40, sort=True)
    with tempfile.TemporaryDirectory() as tmp:
        db.write_ascii(os.path.join(tmp, "db.ascii"))
        runs = {"H4": [], "L_parent": []}
        for _ in range(reps):                                   # alternated
            runs["H4"].append(cli_run(CLI, ["-a", "db.ascii", "-H", H_LIST], tmp))
            runs["L_parent"].append(cli_run(parent_cli, ["-a", "db.ascii", "-L", "0.001"], tmp))
            print("end to end: %.1f s / %.1f s" % (runs["H4"][-1]["wall_s"], runs["L_parent"][-1]["wall_s"]), file=sys.stderr, flush=True)
    return {"entries": entries, "levels": H_LIST, "parent_pvalue": 1e-3, "restarts": 128, "runs": runs,
            "wall_s": {k: summary([r["wall_s"] for r in v]) for k, v in runs.items()},
            "gpu_ms": {k: summary([r["gpu_ms"] for r in v]) for k, v in runs.items()}}


def bench_lines(parent_lib, reps=3):
    runs = {"tree": [], "parent": []}
    for _ in range(reps):                                       # alternated
        for key, lib in (("tree", None), ("parent", parent_lib)):
            env = dict(os.environ)
            env.pop("SAT_DEVICE_LIB", None)
            if lib:
                env["SAT_DEVICE_LIB"] = os.path.abspath(lib)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "100"], capture_output=True,
                               env=env, cwd=ROOT)
            if p.returncode != 0:
                raise SystemExit("bench.py failed: %s" % p.stderr.decode()[-400:])
            line = json.loads(p.stdout.decode().strip().splitlines()[-1])
            runs[key].append({k: line[k] for k in ("value", "ms_per_step") if k in line})
            print("bench %s: %r" % (key, runs[key][-1]), file=sys.stderr, flush=True)
    return {"runs": runs, "value": {k: summary([r["value"] for r in v]) for k, v in runs.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib")
    ap.add_argument("--climb-all-lib")
    ap.add_argument("--inner", help=argparse.SUPPRESS)
    ap.add_argument("--inner-leveled", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--entries", type=int, default=15_000)
    ap.add_argument("--parent-cli")
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.inner:                                                 # the traced child: one library's passes, their table to a file
        with open(a.inner, "w") as fh:
            json.dump(passes(a.reps, a.inner_leveled), fh)
        return
    out = {"reps": a.reps, "rounds": a.rounds, "levels": list(LEVELS)}

    def save():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(out) + "\n")

    if a.parent_lib:
        libs = [("levels", None, True), ("parent_add", a.parent_lib, False)]
        if a.climb_all_lib:
            libs.append(("levels_climb_all", a.climb_all_lib, True))
        rounds = {key: [] for key, _, _ in libs}
        trace = {}
        for _ in range(a.rounds):                               # alternated
            for key, lib, leveled in libs:
                table, trace[key] = traced(lib, a.reps, leveled)
                rounds[key].append(table)
                print("passes: %s, trace %s" % (key, trace[key]), file=sys.stderr, flush=True)
        out["passes"] = {key: merge(r) for key, r in rounds.items()}
        out["kernel_trace"] = trace
        save()
    if a.parent_cli:
        out["end_to_end"] = end_to_end(a.entries, os.path.abspath(a.parent_cli), a.cli_reps)
        save()
    if a.bench and a.parent_lib:
        out["bench"] = bench_lines(a.parent_lib)
        save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
