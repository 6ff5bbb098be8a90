"""What the exact search (sat_search_exact) proves, improves and costs.  Prints one JSON object
(profiles/exact_cost.json).

On the example database (tests/golden/inputs, 586 entries), at r = 128 and the default node budget: the 8-SSE ubiquitin
query and three SID@list motifs of 5 / 8 / 12 SSEs - the share of rows proven, the share improved, the mean and the
largest gain, the nodes a row (median, maximum), and the pass's time against the incumbent search's.  One motif again at
r = 1 and r = 4096 and with every row polished first (sat_polish_all_set(8)).  A 6-SSE query x 15 000 synthetic entries
of 4..40 SSEs.  The worst single launch: the largest time of any one exact_pass launch is bounded here by the pass's
whole time under SAT_EXP_SCRATCH_KB (one row budget a launch).

Times: the call's kernel_ms (events on the stream around both parts) minus the plain search's, medians of --reps
alternated runs behind a warm-up.

    python scripts/exact_cost.py [--reps 9]
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
from cuda_satabsearch_amd import workloads  # noqa: E402

R = 128


def example_db():
    tmp = tempfile.mkdtemp(prefix="exact_cost_")
    path = os.path.join(tmp, "db.ascii")
    with gzip.open(os.path.join(workloads.GOLDEN_INPUTS, "tableauxdistmatrixdb.small.ascii.gz"), "rb") as fi, open(path, "wb") as fo:
        shutil.copyfileobj(fi, fo)
    db = sat.StructSet.read(path)
    shutil.rmtree(tmp)
    return db


def motif(db, min_order, m, seed):
    """m SSEs, ascending, of the first entry of at least min_order SSEs: (entry, list)"""
    e = int(np.nonzero(db.orders >= min_order)[0][0])
    rng = np.random.default_rng(seed)
    return e, np.sort(rng.choice(int(db.orders[e]), size=m, replace=False)).astype(np.uint8)


def measure(s, r, max_nodes, reps):
    """the rows' statistics, and the medians of `reps` alternated plain / exact runs"""
    plain, exact = [], []
    s.search(True, True, r)
    s.search_exact(True, r, max_nodes)
    for _ in range(reps):
        plain.append(s.search(True, True, r)[2])
        exact.append(s.search_exact(True, r, max_nodes)[2])
    scores, _ = s.results(lsoln=True)
    base, flags, nodes = s.exact_results()
    gain = (scores - base)[scores > base]
    stats = s.exact_stats()
    assert int(stats["improved"].sum()) == gain.size and int(stats["proven"].sum()) == int((~flags).sum())
    p, x = float(np.median(plain)), float(np.median(exact))
    return {"rows": int(scores.size), "proven_share": float((~flags).mean()), "improved_share": float((scores > base).mean()),
            "mean_gain": float(gain.mean()) if gain.size else 0.0, "max_gain": int(gain.max()) if gain.size else 0,
            "nodes_median": float(np.median(nodes)), "nodes_max": int(nodes.max()),
            "incumbent_ms": p, "exact_call_ms": x, "pass_ms": x - p, "pass_over_incumbent": (x - p) / p if p > 0 else None,
            "runs_ms": {"plain": plain, "exact": exact}, "restarts": r, "max_nodes": int(max_nodes), "polish_all": s.polish_all()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--max-nodes", type=int, default=1 << 18)
    args = ap.parse_args()
    res = {}
    db = example_db()
    ubq = workloads.load_queries("d1ubia_.input")[0]
    motifs = {"motif5": motif(db, 20, 5, 5), "motif8": motif(db, 25, 8, 8), "motif12": motif(db, 30, 12, 12)}
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries([(ubq[1], ubq[2], ubq[3])])
        res["d1ubia_8"] = measure(s, R, args.max_nodes, args.reps)
        for name, (e, l) in motifs.items():
            s.set_queries_from_db([e], sses=[l])
            res[name] = dict(measure(s, R, args.max_nodes, args.reps), entry=db.names[e], sses=[int(v) + 1 for v in l])
        e, l = motifs["motif8"]
        s.set_queries_from_db([e], sses=[l])
        res["motif8_r1"] = measure(s, 1, args.max_nodes, args.reps)
        res["motif8_r4096"] = measure(s, 4096, args.max_nodes, args.reps)
        s.set_polish_all(8)
        res["motif8_polish8"] = measure(s, R, args.max_nodes, args.reps)
        s.set_polish_all(0)
        for name, (e, l) in (("motif12_nodes_2p22", motifs["motif12"]),):
            s.set_queries_from_db([e], sses=[l])
            res[name] = measure(s, R, 1 << 22, 3)
    synth = sat.synth.make_db(15_000, 4, 40, sort=True, seed=31)
    q6 = sat.synth.planted_query(synth, 9000, keep=6.0 / float(synth.orders[9000]), seed=6)
    with sat.Searcher(0) as s:
        s.upload(synth)
        s.set_queries([q6])
        res["q%d_synth_15000" % len(q6[2])] = measure(s, R, args.max_nodes, args.reps)
        res["launch"] = s.last_launch_info()
    # the worst launch: one row a launch (a scratch budget below one row's nodes), so the pass's time bounds every launch's
    os.environ["SAT_EXP_SCRATCH_KB"] = "1"
    with sat.Searcher(0) as s:
        s.upload(db.subset(np.argsort(db.orders)[-8:]))
        e, l = motif(db.subset(np.argsort(db.orders)[-8:]), 30, 12, 12)
        s.set_queries_from_db([e], sses=[l])
        times = []
        for _ in range(5):
            plain_ms = s.search(True, True, 1)[2]
            times.append(s.search_exact(True, 1, args.max_nodes)[2] - plain_ms)
        _, flags, nodes = s.exact_results()
        res["worst_launch"] = {"rows": 8, "launches": 8, "pass_ms_of_8_single_row_launches": float(np.median(times)),
                               "unproven": int(flags.sum()), "nodes_max": int(nodes.max()), "info": s.last_launch_info()}
    del os.environ["SAT_EXP_SCRATCH_KB"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
