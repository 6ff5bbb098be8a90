"""Cost of scoring a search against a classification on the GPU (sat_eval_rows, CLI -a -E classes).
Writes one JSON object (profiles/eval_cost.json).  Run by hand on a machine with an MI355X.

* the pass: sat_eval_rows - the table zeroing, eval_histogram, eval_reduce and the 32-byte rows back - beside
  sat_score_histogram, whose code is the parent commit's, on the same searched states:
    q200: 200 database members as queries x 15 000 size-sorted entries of 4..40 SSEs;
    big16: 16 queries of 97..111 SSEs x the same 15 000 entries;
  each with the scores of the search and ("equal") with every score set to 7, the contention worst case: every row of a
  block lands on one LDS word.  Classes: a seeded 7-way split, a tenth of the structures unclassified.  Two clocks:
  "call_ms" - host wall clock around the call, ending synchronised, warmed twice, then --reps runs alternated between the
  two calls - and, under --trace (the script runs itself under `rocprofv3 --kernel-trace`), "kernel_us": the dispatches
  of a call summed (eval_histogram + eval_reduce against score_histogram; the memsets are in neither).
  "tables_bytes": what one shard's tables are - a batch's traffic to the host per shard when the database is sharded.
* end to end (--parent-cli: the command line of the parent commit): `-a db -E classes` of this tree against
  `-a db -L 1e-3` of the parent, --entries size-sorted entries of 4..40 SSEs at r = 128, alternated, --cli-reps runs each:
  wall clock of the process, the summed "GPU execution time" lines, the bytes copied from the GPU.

    python scripts/eval_cost.py [--reps 9] [--trace] [--parent-cli PATH --entries 15000 --cli-reps 3] [--out FILE]
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
from cuda_satabsearch_amd import _native, report  # noqa: E402

CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
WARM = 2


def summary(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def classes_of(n, seed=7):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 7, n).astype(np.int32)
    cls[rng.random(n) < 0.1] = -1
    return cls


def timed(s, call):
    s.sync()
    t0 = time.perf_counter()
    call()
    s.sync()
    return (time.perf_counter() - t0) * 1e3


def passes(reps):
    """case -> the wall clocks of both calls; the order of the cases and runs is what the trace is cut by"""
    db = sat.synth.make_db(15_000, 4, 40, sort=True)
    big = sat.synth.make_db(16, 97, 111, sort=True)
    node_class = classes_of(len(db))
    out = {}
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_eval_classes(node_class)
        for name in ("q200", "big16"):
            if name == "q200":
                idx = np.random.default_rng(5).choice(len(db), 200, replace=False).astype(np.int32)
                s.set_queries_from_db(idx, 0)
                n1s = db.orders[idx]
            else:
                idx = np.nonzero(node_class >= 0)[0][:16].astype(np.int32)     # their nodes: any classified ones
                s.set_queries([(*big.dense(q), big.ssetypes(q)) for q in range(16)], 0)
                n1s = big.orders
            search_ms = s.search(True, False, 128)[2]
            for scores in ("search", "equal"):
                if scores == "equal":
                    s.debug_set_scores(np.full((len(idx), len(db)), 7, np.int32))
                runs = {"eval": [], "hist": []}
                for _ in range(WARM + reps):                        # alternated
                    runs["eval"].append(timed(s, lambda: s.eval_rows(idx, 50)))
                    runs["hist"].append(timed(s, s.score_histogram))
                rows = s.eval_rows(idx, 50)
                defined = (rows["positives"] > 0) & (rows["negatives"] > 0)
                out["%s %s" % (name, scores)] = {
                    "queries": len(idx), "entries": len(db), "search_ms": search_ms, "runs": WARM + reps,
                    "tables_bytes": int((2 * (2 * n1s.astype(np.int64) * (n1s - 1) + 1) * 4).sum()),
                    "defined": int(defined.sum()),
                    "mean_auc": float(np.mean([report.eval_ratios(r)[0] for r in rows[defined]])) if defined.any() else None,
                    "eval_call_ms": summary(runs["eval"][WARM:]), "eval_call_runs_ms": runs["eval"][WARM:],
                    "hist_call_ms": summary(runs["hist"][WARM:]), "hist_call_runs_ms": runs["hist"][WARM:]}
    return out


def kernel_times(trace_dir, table):
    """the trace's dispatches cut into the cases, in order: per run eval_histogram + eval_reduce, then score_histogram,
    and one more eval pair after each case's runs"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return "no kernel trace was written"
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    took = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"]]
            for k in ("eval_histogram(", "eval_reduce(", "score_histogram(")}
    at = {k: 0 for k in took}
    for case, row in table.items():
        runs = row["runs"]
        cut = {k: took[k][at[k]:at[k] + runs] for k in took}
        if any(len(v) != runs for v in cut.values()):
            return "the trace holds fewer dispatches than the runs made (%s)" % {k: len(v) for k, v in took.items()}
        row["eval_histogram_us"] = summary(cut["eval_histogram("][WARM:])
        row["eval_reduce_us"] = summary(cut["eval_reduce("][WARM:])
        row["eval_kernels_us"] = summary([a + b for a, b in zip(cut["eval_histogram("], cut["eval_reduce("])][WARM:])
        row["score_histogram_us"] = summary(cut["score_histogram("][WARM:])
        for k in took:
            at[k] += runs + (0 if k == "score_histogram(" else 1)
    return "ok"


def traced(reps):
    with tempfile.TemporaryDirectory() as tmp:
        table = os.path.join(tmp, "passes.json")
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "--",
                            sys.executable, os.path.abspath(__file__), "--inner", table, "--reps", str(reps)], capture_output=True)
        if p.returncode != 0 or not os.path.exists(table):
            raise SystemExit("the traced run failed: %s" % p.stderr.decode()[-600:])
        out = json.load(open(table))
        status = kernel_times(os.path.join(tmp, "trace"), out)
    return out, status


def cli_run(cli, args, cwd):
    t0 = time.perf_counter()
    p = subprocess.run([cli] + args, input=b"", cwd=cwd, capture_output=True)
    wall = time.perf_counter() - t0
    err = p.stderr.decode()
    if p.returncode != 0:
        raise SystemExit("%s %s failed: %s" % (cli, " ".join(args), err[-400:]))
    return {"wall_s": wall, "gpu_ms": sum(float(x) for x in re.findall(r"GPU execution time ([0-9.]+) ms", err)),
            "d2h_bytes": int(re.findall(r"copied (\d+) bytes of results", err)[-1]),
            "stdout_bytes": len(p.stdout), "head": p.stdout.decode(errors="replace").splitlines()[:3]}


def end_to_end(entries, parent_cli, reps):
    db = sat.synth.make_db(entries, 4, 40, sort=True)
    node_class = classes_of(entries)
    with tempfile.TemporaryDirectory() as tmp:
        db.write_ascii(os.path.join(tmp, "db.ascii"))
        with open(os.path.join(tmp, "db.classes"), "w") as fh:
            fh.write("".join("%s c%d\n" % (name, c) for name, c in zip(db.names, node_class) if c >= 0))
        runs = {"E": [], "L_parent": []}
        for _ in range(reps):                                   # alternated
            runs["E"].append(cli_run(CLI, ["-a", "db.ascii", "-E", "db.classes"], tmp))
            runs["L_parent"].append(cli_run(parent_cli, ["-a", "db.ascii", "-L", "0.001"], tmp))
            print("end to end: %.1f s / %.1f s" % (runs["E"][-1]["wall_s"], runs["L_parent"][-1]["wall_s"]), file=sys.stderr, flush=True)
    return {"entries": entries, "parent_pvalue": 1e-3, "restarts": 128, "runs": runs,
            "wall_s": {k: summary([r["wall_s"] for r in v]) for k, v in runs.items()},
            "gpu_ms": {k: summary([r["gpu_ms"] for r in v]) for k, v in runs.items()},
            "d2h_bytes": {k: v[0]["d2h_bytes"] for k, v in runs.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--inner", help=argparse.SUPPRESS)
    ap.add_argument("--entries", type=int, default=15_000)
    ap.add_argument("--parent-cli")
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.inner:                                                 # the traced child: the passes, their table to a file
        with open(a.inner, "w") as fh:
            json.dump(passes(a.reps), fh)
        return
    out = {"reps": a.reps, "block_rows": _native.EVAL_BLOCK_ROWS, "window_bins": _native.EVAL_WINDOW_BINS}

    def save():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(out) + "\n")

    if a.trace:
        out["passes"], out["kernel_trace"] = traced(a.reps)
    else:
        out["passes"] = passes(a.reps)
    save()
    if a.parent_cli:
        out["end_to_end"] = end_to_end(a.entries, os.path.abspath(a.parent_cli), a.cli_reps)
        save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
