"""Cost of setting a batch of motif queries - chosen SSE lists of database members: sat_queries_set with
the sub-arrays cut on the host (dense arrays at the motifs' pitch, grouped into the blob there, the blob copied)
against sat_queries_from_db_sses (the indices, the offsets and the lists copied, the sub-triangles gathered and the blob
built on the device).  Host wall clock from "entries and lists known" to "batch ready to search"; both calls end
synchronised.  Writes one JSON object (profiles/motif_queries_cost.json).

One process, the ways alternated, --reps runs after a warm-up, every run kept (median, minimum and maximum are
reported beside them): 256 motifs of 5..12 SSEs, each a random ascending or shuffled list, drawn from a database of
entries of 8..32 SSEs and from one of entries of 97..111 SSEs.  The dense way is timed twice: the C call alone
(sub-arrays already cut) and with the cut (numpy here; a C loop is faster, so a host program lies between the two).

    python scripts/motif_queries_cost.py [--reps 9] [--out profiles/motif_queries_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_satabsearch_amd as sat  # noqa: E402
from cuda_satabsearch_amd.search import _pack_sse_lists  # noqa: E402

PITCH = 16                              # every motif here has at most 12 SSEs


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def cut(db, idx, lists):
    """the motifs as dense arrays at pitch 16, types from the diagonal: cell (i, k) is the entry's (l[i], l[k])"""
    n1s = np.array([len(l) for l in lists], np.int32)
    tabs = np.zeros((len(idx), PITCH, PITCH), np.uint8)
    dmats = np.zeros((len(idx), PITCH, PITCH), np.float32)
    types = np.zeros((len(idx), PITCH), np.uint8)
    for k, (e, l) in enumerate(zip(idx, lists)):
        t, d = db.dense(int(e))
        m = len(l)
        tabs[k, :m, :m] = t[np.ix_(l, l)]
        dmats[k, :m, :m] = d[np.ix_(l, l)]
        types[k, :m] = np.diagonal(t)[l]
    return n1s, tabs, dmats, types


def library_case(s, db, nq, reps):
    lib, ctx = s._lib, s._ctx
    s.upload(db)
    rng = np.random.default_rng(11)
    idx = np.ascontiguousarray(rng.choice(len(db), nq, replace=len(db) < nq), np.int32)
    lists = []
    for q, e in enumerate(idx):
        n = int(db.orders[e])
        l = rng.choice(n, size=int(rng.integers(5, min(12, n) + 1)), replace=False)
        lists.append(np.sort(l) if q % 2 == 0 else l)          # every other one ascending
    begin, sse = _pack_sse_lists(lists, nq)

    def dense_call(arrays):
        n1s, tabs, dmats, types = arrays
        s._check(lib.sat_queries_set(ctx, nq, n1s.ctypes.data, tabs.ctypes.data, dmats.ctypes.data, PITCH, types.ctypes.data, 0))

    arrays = cut(db, idx, lists)
    cases = {
        "queries_set_call": lambda: dense_call(arrays),
        "queries_set_with_cut": lambda: dense_call(cut(db, idx, lists)),
        "queries_from_db_sses": lambda: s._check(lib.sat_queries_from_db_sses(ctx, nq, idx.ctypes.data, begin.ctypes.data,
                                                                              sse.ctypes.data, 0)),
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
    for name in ("queries_set_call", "queries_from_db_sses"):
        before = s.query_h2d_bytes()
        cases[name]()
        h2d[name] = s.query_h2d_bytes() - before
    assert h2d["queries_from_db_sses"] == 8 * nq + 4 + int(begin[-1])
    dense_call(arrays)
    want = s.debug_query_blob()
    cases["queries_from_db_sses"]()
    assert np.array_equal(s.debug_query_blob(), want), "the two batches differ"
    sizes = [len(l) for l in lists]
    return {"queries": nq, "entries": len(db), "entry_orders": [int(db.orders[idx].min()), int(db.orders[idx].max())],
            "motif_sses": [min(sizes), max(sizes)], "list_bytes": int(begin[-1]),
            "ms": {k: spread(v) for k, v in runs.items()}, "h2d_bytes": h2d, "runs_ms": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motif_queries_cost.json"))
    a = ap.parse_args()
    out = {"reps": a.reps}
    with sat.Searcher(0) as s:
        out["from_small_entries"] = library_case(s, sat.synth.make_db(2000, 8, 32, seed=21), 256, a.reps)
        out["from_large_entries"] = library_case(s, sat.synth.make_db(400, 97, 111, seed=22), 256, a.reps)
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
