"""Cost of setting a query batch whose queries are database members: sat_queries_set (dense arrays expanded on the host,
grouped into the blob there, the blob copied) against sat_queries_from_db (the indices copied, the blob built on the
device).  Host wall clock from "indices known" to "batch ready to search"; both calls end synchronised.  Writes one JSON
object (profiles/queries_from_db_cost.json).

* library, one process, the two ways alternated, medians of --reps runs after a warm-up:
    256 queries of 8..32 SSEs and 256 queries of 97..111 SSEs, drawn from a database of such entries.  The dense
    way is timed twice: the C call alone (arrays at pitch 111 already expanded) and with the expansion of the entries
    into those arrays (numpy here; the command line's C loop is faster, so the truth for -q lies between the two).
* command line, end to end: `-a db -k 10` against `-q db -k 10` fed every SID in file order, on a size-sorted synthetic
  database of --entries entries of 4..40 SSEs and on the 586-entry example database; wall clock of the whole process,
  alternated, --cli-reps runs; the two stdouts must be equal.

    python scripts/queries_from_db_cost.py [--reps 9] [--cli-reps 3] [--entries 15000] [--out profiles/queries_from_db_cost.json]
"""
import argparse
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_satabsearch_amd as sat  # noqa: E402

CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
PITCH = sat.structures.MAXDIM


def med(v):
    return float(np.median(v))


def expand(db, idx):
    """what the command line does per batch of -q: the entries as dense arrays at pitch 111, types from the diagonal"""
    n1s = np.ascontiguousarray(db.orders[idx], np.int32)
    tabs = np.zeros((len(idx), PITCH, PITCH), np.uint8)
    dmats = np.zeros((len(idx), PITCH, PITCH), np.float32)
    types = np.zeros((len(idx), PITCH), np.uint8)
    for k, e in enumerate(idx):
        t, d = db.dense(int(e))
        n = t.shape[0]
        tabs[k, :n, :n] = t
        dmats[k, :n, :n] = d
        types[k, :n] = np.diagonal(t)
    return n1s, tabs, dmats, types


def library_case(s, db, nq, reps):
    lib, ctx = s._lib, s._ctx
    s.upload(db)
    idx = np.ascontiguousarray(np.random.default_rng(11).choice(len(db), nq, replace=len(db) < nq), np.int32)

    def dense_call(arrays):
        n1s, tabs, dmats, types = arrays
        s._check(lib.sat_queries_set(ctx, nq, n1s.ctypes.data, tabs.ctypes.data, dmats.ctypes.data, PITCH, types.ctypes.data, 0))

    arrays = expand(db, idx)
    cases = {
        "queries_set_call": lambda: dense_call(arrays),
        "queries_set_with_expansion": lambda: dense_call(expand(db, idx)),
        "queries_from_db": lambda: s._check(lib.sat_queries_from_db(ctx, nq, idx.ctypes.data, 0)),
    }
    for fn in cases.values():                                   # warm-up: code objects, allocations
        fn()
        fn()
    runs = {name: [] for name in cases}
    for _ in range(reps):                                       # alternated
        for name, fn in cases.items():
            t0 = time.perf_counter()
            fn()
            runs[name].append((time.perf_counter() - t0) * 1e3)
    h2d = {}
    for name in ("queries_set_call", "queries_from_db"):
        before = s.query_h2d_bytes()
        cases[name]()
        h2d[name] = s.query_h2d_bytes() - before
    dense_call(arrays)
    want = s.debug_query_blob()
    cases["queries_from_db"]()
    assert np.array_equal(s.debug_query_blob(), want), "the two batches differ"
    return {"queries": nq, "entries": len(db), "orders": [int(db.orders[idx].min()), int(db.orders[idx].max())],
            "median_ms": {k: med(v) for k, v in runs.items()}, "h2d_bytes": h2d, "runs_ms": runs}


def cli_case(path, names, reps, k=10):
    cwd, db = os.path.dirname(path), os.path.basename(path)
    sids = "".join(n + "\n" for n in names).encode()
    modes = {"q": (["-q", db, "-k", str(k)], sids), "a": (["-a", db, "-k", str(k)], b"")}
    runs, digest, search_ms = {m: [] for m in modes}, {}, {m: [] for m in modes}
    for _ in range(reps):                                       # alternated
        for m, (args, stdin) in modes.items():
            t0 = time.perf_counter()
            p = subprocess.run([CLI] + args, input=stdin, cwd=cwd, capture_output=True, check=True)
            runs[m].append(time.perf_counter() - t0)
            digest[m] = hashlib.sha256(p.stdout).hexdigest()
            search_ms[m].append(sum(float(line.split()[3]) for line in p.stderr.decode().splitlines()
                                    if line.startswith("GPU execution time")))
    assert digest["q"] == digest["a"], "-a and -q print different bytes"
    return {"entries": len(names), "k": k, "median_s": {m: med(v) for m, v in runs.items()},
            "median_search_ms": {m: med(v) for m, v in search_ms.items()}, "runs_s": runs, "stdout_sha256": digest["a"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--entries", type=int, default=15_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "queries_from_db_cost.json"))
    a = ap.parse_args()
    out = {"reps": a.reps, "cli_reps": a.cli_reps}
    with sat.Searcher(0) as s:
        out["small_queries"] = library_case(s, sat.synth.make_db(2000, 8, 32, seed=21), 256, a.reps)
        out["large_queries"] = library_case(s, sat.synth.make_db(400, 97, 111, seed=22), 256, a.reps)
    with tempfile.TemporaryDirectory() as tmp:
        db = sat.synth.make_db(a.entries, 4, 40, sort=True, name_format="s%06d")        # SIDs are cut to 7 characters
        db.write_ascii(os.path.join(tmp, "synth.ascii"))
        out["cli_synthetic"] = cli_case(os.path.join(tmp, "synth.ascii"), db.names, a.cli_reps)
        small = os.path.join(ROOT, "tests", "golden", "inputs", "tableauxdistmatrixdb.small.ascii.gz")
        with gzip.open(small, "rb") as fi, open(os.path.join(tmp, "small.ascii"), "wb") as fo:
            shutil.copyfileobj(fi, fo)
        names = sat.StructSet.read(os.path.join(tmp, "small.ascii")).names
        out["cli_small_586"] = cli_case(os.path.join(tmp, "small.ascii"), names, max(a.cli_reps, 5))
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
