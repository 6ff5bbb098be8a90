"""Cost of several matches per entry (sat_search_matches) against a plain LSOLN = T search, alternated in one process:
the bench shape (32-SSE query x 125 000 32-SSE entries, r = 128) and BASELINE configs[4] (d1twfa_, 101 SSEs, x 100 000
entries of the C5 order mix, r = 128), -m 4 with and without maps.  Also how many entries of the reference's 586-entry
database get two or more matches for its example queries.  Prints one JSON object.

    python scripts/matches_cost.py [--reps 5] [--skip-gain]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_satabsearch_amd as sat  # noqa: E402
from cuda_satabsearch_amd import workloads  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        out.append(fn())
    return out


def shape(s, db, q, reps, m):
    s.upload(db)
    s.set_query(q[0], q[1], q[2], 0)
    s.search(True, True, 128)                                   # warm-up: code objects, scratch
    s.search_matches(m, True, 128, maps=True)
    plain, nomaps, maps = [], [], []
    for _ in range(reps):                                       # alternated
        plain.append(s.search(True, True, 128)[2])
        nomaps.append(s.search_matches(m, True, 128, maps=False)[4])
        maps.append(s.search_matches(m, True, 128, maps=True)[4])
    med = lambda v: float(np.median(v))
    return {"plain_lsoln_ms": med(plain), "matches_nomaps_ms": med(nomaps), "matches_maps_ms": med(maps),
            "ratio_nomaps": med(nomaps) / med(plain), "ratio_maps": med(maps) / med(plain),
            "runs": {"plain": plain, "nomaps": nomaps, "maps": maps}, "launch": s.last_launch_info()}


def gain(s, golden):
    db = sat.StructSet.read(os.path.join(golden, "tableauxdistmatrixdb.small.ascii"))
    s.upload(db)
    out = {}
    for f, lorder in (("d1ubia_.input", True), ("d2phlb1.input", True), ("d2phlb1_TFT.input", False),
                      ("1qlp_sheetbc.input", True), ("d1ae6h1.input", True), ("d1twfa_.input", True)):
        qs = sat.StructSet.read(os.path.join(golden, f), "query", skip_header_lines=2)
        t, d = qs.dense(0)
        s.set_query(t, d, qs.ssetypes(0), 0)
        counts = s.search_matches(8, lorder, 128, maps=False)[0][0]
        out[f] = {"entries": int(len(db)), "two_or_more": int((counts >= 2).sum()), "mean_count": float(counts.mean())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--golden", default=None, help="unpacked tests/golden/inputs (for the 586-entry database)")
    args = ap.parse_args()
    res = {}
    with sat.Searcher(0) as s:
        res["bench_shape"] = shape(s, sat.synth.make_db(125_000, 32), sat.synth.make_query(32), args.reps, 4)
        q4 = workloads.config4_query()
        res["configs4"] = shape(s, workloads.config4_db(), (q4[1], q4[2], q4[3]), args.reps, 4)
        if args.golden:
            res["gain_small_db"] = gain(s, args.golden)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
