"""What the built-in Gumbel table makes of polished scores, from the CPU reference alone
(tests/polish_lib.py; no GPU): the example database x the five golden queries at r = 128 - per query the Gumbel a, b
fitted (`-F 0.1`: sat_gumbel_fit_binned on the score histogram) to the plain scores, to the polished scores at T = 1 and
8 and (--long) to the plain scores at r = 2048, and beside each the rows with p <= 0.01 under the built-in table and
under that fit.  Prints one JSON object (profiles/polish_all_stats.json).

    python scripts/polish_all_stats.py [--long] [--step N] [--jobs 8]
"""
import argparse
import ctypes as C
import gzip
import json
import os
import shutil
import sys
import tempfile
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cuda_satabsearch_amd as sat  # noqa: E402
from cuda_satabsearch_amd import _native  # noqa: E402

JOBS = (("d2phlb1.input", True), ("d2phlb1_TFT.input", False), ("d1twfa_.input", True), ("d1ubia_.input", True),
        ("d1ae6h1.input", True))
TOPS = (1, 8)
CENSOR, PMAX, BINS = 0.1, 0.01, 4096
_state = {}


def load_db():
    src = os.path.join(ROOT, "tests", "golden", "inputs")
    tmp = tempfile.mkdtemp(prefix="polish_all_stats_")
    with gzip.open(os.path.join(src, "tableauxdistmatrixdb.small.ascii.gz"), "rb") as fi, open(os.path.join(tmp, "db.ascii"), "wb") as fo:
        shutil.copyfileobj(fi, fo)
    db = sat.StructSet.read(os.path.join(tmp, "db.ascii"))
    shutil.rmtree(tmp)
    return db


def one_entry(job):
    """(plain r128, polished T = 1, T = 8, plain at the largest restart count) of one (query, entry)"""
    import matches_lib
    import polish_lib
    name, lorder, e, rmax = job
    if "db" not in _state:
        _state["db"] = load_db()
    db = _state["db"]
    if name not in _state:
        qs = sat.StructSet.read(os.path.join(ROOT, "tests", "golden", "inputs", name), "query", skip_header_lines=2)
        _state[name] = (*qs.dense(0), qs.ssetypes(0))
    q = _state[name]
    sc, mp = matches_lib.restarts(db, e, q, lorder, rmax)
    pair = polish_lib.Pair.of(db, e, q)
    pol = [int(polish_lib.polish_ranked(pair, sc[:128], mp[:128], lorder, t)[0]) for t in TOPS]
    return int(sc[:128].max()), pol[0], pol[1], int(sc.max())


def statistics(scores, n1, orders):
    """the fit of `scores` and the rows under PMAX by the built-in table and by the fit"""
    h = _native.host_lib()
    scores = np.ascontiguousarray(scores, np.int32)
    orders = np.ascontiguousarray(orders, np.int32)
    counts, below = np.zeros(BINS, np.uint32), C.c_int32(0)
    h.sat_stat_histogram(scores.ctypes.data, len(scores), n1, orders.ctypes.data, counts.ctypes.data, C.byref(below))
    f = _native.Fit()
    h.sat_gumbel_fit_binned(counts.ctypes.data, CENSOR, C.byref(f))
    builtin = sum(h.sat_pv_gumbel(h.sat_z_gumbel_trunc(h.sat_norm2(int(s), n1, int(o)))) <= PMAX for s, o in zip(scores, orders))
    out = {"mean_score": float(scores.mean()), "rows_p_le_0.01_builtin": int(builtin), "fitted": int(f.fitted)}
    if f.fitted:
        z, p = np.zeros(BINS), np.zeros(BINS)
        h.sat_gumbel_fit_table(f.a, f.b, z.ctypes.data, p.ctypes.data)
        bins = [0 if s < 0 else h.sat_stat_bin(int(s), n1, int(o)) for s, o in zip(scores, orders)]
        out.update({"a": f.a, "b": f.b, "rows_p_le_0.01_fit": int((p[bins] <= PMAX).sum())})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--long", action="store_true", help="also plain r = 2048 (16 x the time)")
    ap.add_argument("--step", type=int, default=1)
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    db = load_db()
    entries = list(range(0, len(db), args.step))
    rmax = 2048 if args.long else 128
    res = {"entries": len(db), "rows": len(entries), "r": 128, "censor": CENSOR, "pmax": PMAX, "queries": {}}
    with Pool(args.jobs) as pool:
        for name, lorder in JOBS:
            rows = np.array(pool.map(one_entry, [(name, lorder, e, rmax) for e in entries], chunksize=4))
            qs = sat.StructSet.read(os.path.join(ROOT, "tests", "golden", "inputs", name), "query", skip_header_lines=2)
            n1, orders = int(qs.orders[0]), db.orders[entries]
            job = {"n1": n1, "lorder": lorder, "plain_r128": statistics(rows[:, 0], n1, orders),
                   "polish_T1": statistics(rows[:, 1], n1, orders), "polish_T8": statistics(rows[:, 2], n1, orders)}
            if args.long:
                job["plain_r2048"] = statistics(rows[:, 3], n1, orders)
            res["queries"][name] = job
            print(name, json.dumps(job), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
