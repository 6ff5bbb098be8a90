"""What the polish is worth against more restarts, on the GPU: all 586 entries of the example database under the five
golden queries.  For T = 1, 2, 4, 8 at r = 128 against the plain search at r = 256 / 512 / 1024 / 2048 (the same streams
continued): the mean gain over plain r = 128, the share of rows that reach the r = 2048 score and the share strictly
above it.  Prints one JSON object (profiles/polish_quality.json).

    python scripts/polish_quality.py [--step N]       # every N-th entry (DESIGN.md 6h compares with the CPU reference)
"""
import argparse
import gzip
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_satabsearch_amd as sat  # noqa: E402

JOBS = (("d2phlb1.input", True), ("d2phlb1_TFT.input", False), ("d1twfa_.input", True), ("d1ubia_.input", True),
        ("d1ae6h1.input", True))
PLAIN = (256, 512, 1024, 2048)
TOPS = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=1)
    args = ap.parse_args()
    src = os.path.join(ROOT, "tests", "golden", "inputs")
    tmp = tempfile.mkdtemp(prefix="polish_quality_")
    with gzip.open(os.path.join(src, "tableauxdistmatrixdb.small.ascii.gz"), "rb") as fi, \
            open(os.path.join(tmp, "db.ascii"), "wb") as fo:
        shutil.copyfileobj(fi, fo)
    db = sat.StructSet.read(os.path.join(tmp, "db.ascii"))
    e = np.arange(0, len(db), args.step, dtype=np.int32)
    q = np.zeros(len(e), np.int32)
    res = {"entries": len(db), "rows": len(e), "step": args.step, "r": 128, "jobs": {}}
    with sat.Searcher(0) as s:
        s.upload(db)
        for name, lorder in JOBS:
            qs = sat.StructSet.read(os.path.join(src, name), "query", skip_header_lines=2)
            s.set_queries([(*qs.dense(0), qs.ssetypes(0))], 0)
            base = s.search_pairs(q, e, lorder, False, 128)[0].astype(np.int64)
            plain = {r: s.search_pairs(q, e, lorder, False, r)[0].astype(np.int64) for r in PLAIN}
            job = {"n1": int(qs.orders[0]), "lorder": lorder, "plain_r128_reaches_r2048": float(np.mean(base >= plain[2048]))}
            for r in PLAIN:
                job["plain_r%d_mean_gain" % r] = float(np.mean(plain[r] - base))
            for t in TOPS:
                sc, bs, _, mv, _, _ = s.search_pairs_polish(q, e, t, lorder, 128)
                assert np.array_equal(bs, base)
                job["polish_T%d" % t] = {"mean_gain": float(np.mean(sc - base)), "reaches_r2048": float(np.mean(sc >= plain[2048])),
                                         "above_r2048": float(np.mean(sc > plain[2048])), "improved": float(np.mean(sc > base)),
                                         "moves_mean": float(np.mean(mv)), "moves_max": int(mv.max())}
            res["jobs"][name] = job
    shutil.rmtree(tmp)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
