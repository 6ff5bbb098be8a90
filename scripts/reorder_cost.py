"""Cost of reporting the hits that match only out of sequence order (sat_baseline_keep, sat_reorder_hits, CLI -X B;
DESIGN.md 6u).  Writes one JSON object (profiles/reorder_cost.json).

* the selection: sat_reorder_hits (kinds = circular | permuted, no baseline condition) against sat_hits_cutoff on the
  same scores - the unordered search of 200 database members as queries x 15 000 size-sorted entries of 4..40 SSEs - at
  P = 1e-3 (few rows qualify: the map of almost no row is read) and at P = 1 (every row passes the p-value test, every map
  is read: the worst case).  Counts only (no row buffer: the flag / count pass and 4 bytes a query) and the whole call with
  rows and maps.  Warmed twice, then --reps alternated runs.  "call_ms": host wall clock around the call and a sync;
  "kernel_us": the kernels' own device time when the script runs itself under `rocprofv3 --kernel-trace` (--rocprof).
* sat_baseline_keep against a device-to-device copy of the same 12 bytes a row (torch, one uint8 tensor onto another).
* end to end (--cli): `-a db -X 0 -p 1e-3 -F 0.1` against two runs of `-a db -p 1e-3 -F 0.1` - what a user did before,
  one run per LORDER setting; -a searches with LORDER = T, so the second run stands in for the LORDER = F run, which costs
  the search at least as much - on --cli-entries entries, alternated, --cli-reps runs each, with the bytes copied from the
  GPU and printed.

    python scripts/reorder_cost.py [--reps 9] [--rocprof] [--cli --cli-entries 15000 --cli-reps 2] [--out FILE]
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
CUTOFFS = (1e-3, 1.0)
KINDS = 6
KERNELS = ("cutoff_count", "cutoff_compact", "cutoff_finish", "reorder_count", "reorder_compact", "reorder_finish", "baseline_keep")


def clocked(s, call):
    s.sync()
    t0 = time.perf_counter()
    call()
    s.sync()
    return (time.perf_counter() - t0) * 1e3


def passes(reps):
    import torch
    db = sat.synth.make_db(N, 4, 40, sort=True)
    idx = np.random.default_rng(5).choice(len(db), 200, replace=False).astype(np.int32)
    nq = len(idx)
    out = {}
    with sat.Searcher(0) as s:
        lib, ctx = s._lib, s._ctx
        s.upload(db)
        s.set_queries_from_db(idx, 0)
        s.search_async(True, False, 128)
        # the baseline against a copy of the same bytes
        rows = nq * N
        src = torch.empty(12 * rows, dtype=torch.uint8, device="cuda:0")
        dst = torch.empty_like(src)
        keep = {"baseline_keep": [], "d2d_copy": []}
        for k in range(WARM + reps):
            a = clocked(s, s.baseline_keep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src)
            torch.cuda.synchronize()
            b = (time.perf_counter() - t0) * 1e3
            if k >= WARM:
                keep["baseline_keep"].append(a)
                keep["d2d_copy"].append(b)
        del src, dst
        out["baseline"] = {"rows": rows, "bytes": 12 * rows, "call_ms": {k: summary(v) for k, v in keep.items()}, "call_runs_ms": keep,
                           "dispatches": WARM + reps}
        s.search_async(False, True, 128)
        s.sync()
        counts = np.zeros(nq, np.int32)
        for p in CUTOFFS:
            total = [lib.sat_hits_cutoff(ctx, p, 0, counts.ctypes.data, 0, None, None),
                     lib.sat_reorder_hits(ctx, p, 0.0, KINDS, 0, counts.ctypes.data, 0, None, None)]
            assert min(total) >= 0, lib.sat_last_error()
            hits = np.zeros(max(total[0], 1), sat.search._HIT_DTYPE)
            rrows = np.zeros(max(total[1], 1), sat.search._REORDER_DTYPE)
            # (with maps where the rows are few: 444 bytes a row of 3 M rows would time the copy, not the selection)
            maps = np.empty((max(total), 111), np.int32) if max(total) <= 100_000 else None
            mp = maps.ctypes.data if maps is not None else None
            calls = {
                "hits_cutoff counts": lambda: lib.sat_hits_cutoff(ctx, p, 0, counts.ctypes.data, 0, None, None),
                "reorder_hits counts": lambda: lib.sat_reorder_hits(ctx, p, 0.0, KINDS, 0, counts.ctypes.data, 0, None, None),
                "hits_cutoff rows": lambda: lib.sat_hits_cutoff(ctx, p, 0, counts.ctypes.data, len(hits), hits.ctypes.data, mp),
                "reorder_hits rows": lambda: lib.sat_reorder_hits(ctx, p, 0.0, KINDS, 0, counts.ctypes.data, len(rrows), rrows.ctypes.data, mp),
            }
            runs = {k: [] for k in calls}
            for k in range(WARM + reps):
                for name, call in calls.items():                # alternated
                    ms = clocked(s, call)
                    if k >= WARM:
                        runs[name].append(ms)
            out["q200 P=%g" % p] = {"queries": nq, "entries": N, "rows_hits_cutoff": int(total[0]), "rows_reorder_hits": int(total[1]), "rows_with_maps": maps is not None,
                                    "call_ms": {k: summary(v) for k, v in runs.items()}, "call_runs_ms": runs,
                                    "dispatches": WARM + reps}
    return {"passes": out}


def kernel_times(trace_dir, table, reps):
    """the trace's dispatches of the selection kernels, cut into the cases in order: a case dispatches the count kernels
    2 + 2 times a round (the counts-only call, the call with rows) and the others once"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return "no kernel trace was written"
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    durations = {k: [] for k in KERNELS}
    for r in rows:
        for k in KERNELS:
            if k in r["Kernel_Name"]:
                durations[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    durations["reorder_finish"] = durations["reorder_finish"][1:]       # the empty launch that loads the code object
    n = WARM + reps
    keep = durations["baseline_keep"][WARM:n]
    if len(keep) != reps:
        return "the trace holds %s dispatches, not the runs'" % {k: len(v) for k, v in durations.items()}
    table["baseline"]["kernel_us"] = {"baseline_keep": summary(keep)}
    at = {k: 0 for k in KERNELS}
    for p in CUTOFFS:
        row = table["q200 P=%g" % p]
        cut = {}
        for k in KERNELS[:6]:
            per_round = 2 if k.endswith("_count") else 1
            skip = 1 if k.endswith("_count") else 0             # the probing call of its family, before the rounds
            got = durations[k][at[k] + skip:at[k] + skip + n * per_round]
            at[k] += skip + n * per_round
            if row["rows_%s" % ("hits_cutoff" if k.startswith("cutoff") else "reorder_hits")] == 0 and not k.endswith("_count"):
                at[k] -= skip + n * per_round                   # no row qualified: the call ended behind its count pass
                continue
            if len(got) != n * per_round:
                return "the trace holds %s dispatches, not the runs'" % {k: len(v) for k, v in durations.items()}
            cut[k] = got[WARM * per_round:]
        row["kernel_us"] = {k: summary(v) for k, v in cut.items()}
        row["kernel_runs_us"] = cut
    return "ok"


def end_to_end(entries, reps):
    db = sat.synth.make_db(entries, 4, 40, sort=True)
    with tempfile.TemporaryDirectory() as tmp:
        db.write_ascii(os.path.join(tmp, "db.ascii"))
        runs = {"X": [], "p_first": [], "p_second": []}
        for _ in range(reps):                                   # alternated
            runs["X"].append(cli_run(CLI, ["-a", "db.ascii", "-X", "0", "-p", "0.001", "-F", "0.1"], tmp))
            runs["p_first"].append(cli_run(CLI, ["-a", "db.ascii", "-p", "0.001", "-F", "0.1"], tmp))
            runs["p_second"].append(cli_run(CLI, ["-a", "db.ascii", "-p", "0.001", "-F", "0.1"], tmp))
    both = [a["wall_s"] + b["wall_s"] for a, b in zip(runs["p_first"], runs["p_second"])]
    return {"entries": entries, "pvalue": 1e-3, "censor": 0.1, "restarts": 128, "runs": runs,
            "wall_s": {"X": summary([r["wall_s"] for r in runs["X"]]), "two_p_runs": summary(both)},
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
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--cli-entries", type=int, default=N)
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
    if a.cli:
        out["end_to_end"] = end_to_end(a.cli_entries, a.cli_reps)
    text = json.dumps(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
