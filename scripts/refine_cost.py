"""Cost and recall of the two-stage search (sat_search_refine), alternated in one process, warmed, medians of --reps
runs.  Prints one JSON object (profiles/refine_cost.json).

* bench shape: 32-SSE query x 125 000 32-SSE entries, r = 128, C = 1000, R = 4096, against a plain r = 4096 search;
  stage 2 alone through sat_search_pairs over the same candidates, and its SA steps/s next to the plain kernel's
* small case: one query, C = 10 and 100, stage 2 with the chosen split against SAT_EXP_REFINE_SPLIT = R (no split)
* configs[2]: d2phlb1 + multiquery x 100 000 entries, refine r = 128, C = 500, R = 4096, against plain r = 4096
* recall (with --golden): the reference's 586-entry database, its five example queries, C in {10, 40, 160}: how many
  of the plain r = 4096 top-10 entries the refine's top 10 holds

    python scripts/refine_cost.py [--reps 5] [--golden DIR] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_satabsearch_amd as sat  # noqa: E402
from cuda_satabsearch_amd import workloads  # noqa: E402

STEPS = 100


def med(v):
    return float(np.median(v))


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def pairs_ms(s, q, e, maxstart):
    """sat_search_pairs' kernel_ms (launch .. sync of both passes) without maps"""
    q = np.ascontiguousarray(q, np.int32)
    e = np.ascontiguousarray(e, np.int32)
    scores = np.zeros(len(q), np.int32)
    ms = C.c_double(0.0)
    s._check(s._lib.sat_search_pairs(s._ctx, 1, 0, int(maxstart), len(q), q.ctypes.data, e.ctypes.data,
                                     scores.ctypes.data, None, C.byref(ms)))
    return ms.value


def candidates(s, c, r):
    s.search(True, False, r)
    hits = s.topk_hits(c)
    nq = hits.shape[0]
    return np.repeat(np.arange(nq, dtype=np.int32), hits.shape[1]), hits["entry"].ravel().astype(np.int32)


def bench_shape(s, reps, k=10, c=1000, r=128, big_r=4096):
    db, q = sat.synth.make_db(125_000, 32), sat.synth.make_query(32)
    s.upload(db)
    s.set_queries([q])
    n = len(db)
    pq, pe = candidates(s, c, r)
    s.search(True, False, big_r)                                # warm-up
    s.search_refine(k, c, big_r, True, False, r)
    pairs_ms(s, pq, pe, big_r)
    plain, stage1, stage2, total = [], [], [], []
    for _ in range(reps):                                       # alternated
        plain.append(s.search(True, False, big_r)[2])
        stage1.append(s.search(True, False, r)[2])
        stage2.append(pairs_ms(s, pq, pe, big_r))
        total.append(wall(lambda: s.search_refine(k, c, big_r, True, False, r))[0])
    info = s.last_launch_info()
    return {"entries": n, "k": k, "C": c, "r": r, "R": big_r,
            "plain_R_ms": med(plain), "stage1_ms": med(stage1), "stage2_ms": med(stage2), "refine_total_wall_ms": med(total),
            "speedup_vs_plain": med(plain) / med(total),
            "plain_steps_per_s": n * big_r * STEPS / (med(plain) / 1e3),
            "stage2_steps_per_s": c * big_r * STEPS / (med(stage2) / 1e3),
            "runs": {"plain": plain, "stage1": stage1, "stage2": stage2, "total": total}, "launch": info}


def small_case(s, s_nosplit, reps, big_r=4096):
    db, q = sat.synth.make_db(125_000, 32), sat.synth.make_query(32)
    out = {}
    for ctx in (s, s_nosplit):
        ctx.upload(db)
        ctx.set_queries([q])
    for c in (10, 100):
        pq, pe = candidates(s, c, 128)
        pairs_ms(s, pq, pe, big_r)
        pairs_ms(s_nosplit, pq, pe, big_r)
        split, nosplit = [], []
        for _ in range(reps):
            split.append(pairs_ms(s, pq, pe, big_r))
            nosplit.append(pairs_ms(s_nosplit, pq, pe, big_r))
        out["C%d" % c] = {"stage2_split_ms": med(split), "stage2_nosplit_ms": med(nosplit),
                          "gain": med(nosplit) / med(split), "launch_split": s.last_launch_info(),
                          "launch_nosplit": s_nosplit.last_launch_info(), "runs": {"split": split, "nosplit": nosplit}}
    return out


def configs2(s, reps, k=10, c=500, r=128, big_r=4096):
    db = workloads.config2_db()
    qs = [(t, d, ty) for _, t, d, ty in workloads.config2_queries()]
    s.upload(db)
    s.set_queries(qs)
    s.search(True, False, big_r)
    s.search_refine(k, c, big_r, True, False, r)
    plain, total = [], []
    for _ in range(reps):
        plain.append(s.search(True, False, big_r)[2])
        total.append(wall(lambda: s.search_refine(k, c, big_r, True, False, r))[0])
    scorings = len(db) * len(qs)
    return {"entries": len(db), "queries": len(qs), "k": k, "C": c, "r": r, "R": big_r,
            "plain_R_ms": med(plain), "plain_R_scorings_per_s": scorings / (med(plain) / 1e3),
            "refine_wall_ms": med(total), "refine_scorings_per_s": scorings / (med(total) / 1e3),
            "speedup_vs_plain": med(plain) / med(total), "runs": {"plain": plain, "refine": total}}


def recall(s, golden, k=10, r=128, big_r=4096):
    db = sat.StructSet.read(os.path.join(golden, "tableauxdistmatrixdb.small.ascii"))
    s.upload(db)
    out = {}
    for f in ("d1ubia_.input", "d2phlb1.input", "1qlp_sheetbc.input", "d1ae6h1.input", "d1twfa_.input"):
        qs = sat.StructSet.read(os.path.join(golden, f), "query", skip_header_lines=2)
        t, d = qs.dense(0)
        s.set_queries([(t, d, qs.ssetypes(0))])
        s.search(True, False, big_r)
        ref = set(int(x) for x in s.topk_hits(k)[0]["entry"])
        out[f] = {}
        for c in (10, 40, 160):
            got = set(int(x) for x in s.search_refine(k, c, big_r, True, False, r)[0][0]["entry"])
            out[f]["C%d" % c] = len(ref & got)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--golden", default=None, help="unpacked tests/golden/inputs (for the 586-entry database)")
    ap.add_argument("--quick", action="store_true", help="bench shape only, one run (for a kernel-trace run)")
    args = ap.parse_args()
    res = {}
    with sat.Searcher(0) as s:
        res["bench_shape"] = bench_shape(s, 1 if args.quick else args.reps)
        if not args.quick:
            os.environ["SAT_EXP_REFINE_SPLIT"] = "4096"
            with sat.Searcher(0) as s_nosplit:
                del os.environ["SAT_EXP_REFINE_SPLIT"]
                res["small_case"] = small_case(s, s_nosplit, args.reps)
            res["configs2"] = configs2(s, args.reps)
            if args.golden:
                res["recall_small_db"] = recall(s, args.golden)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
