"""Helpers of the reordered-hits tests (-X B, sat_reorder_hits): the order of a map restated in Python from the rule of
csrc/host/sat_reorder.h - not from its C -, the rows a selection must return, made in numpy from parts that are not the
code under test, and the planted circular permutants with their oracle figures."""
import numpy as np

import cuda_satabsearch_amd as sat

SEQ, CIRC, PERM = 1, 2, 4
MAXDIM = 111

# the mixed batch: whole-entry queries of 1, 2, 8, 10, 12 and 16 SSEs - six map pitches - against sixteen entries
MIXED_ORDERS = (1, 2, 6, 8, 8, 10, 12, 12, 14, 16, 17, 20, 24, 32, 33, 40)
MIXED_QUERIES = (0, 1, 3, 5, 6, 9)
MIXED_R = 16

# the planted circular permutants: entry e of the 14-entry database, its SSEs rotated by c = n // 2, context seed 1234,
# r = 16, query ordinal e.  (unordered score = n (n - 1), ordered score) as the CPU oracle gives them
PLANTED_ORDERS = (6, 8, 8, 10, 12, 12, 14, 16, 17, 20, 24, 32, 33, 40)
PLANTED = {1: (56, 4), 3: (90, 6), 4: (132, 10), 7: (240, 30)}
PLANTED_R = 16


def kind(m):
    """(kind, matched, descents, cut) by the issue's words: the images of the matched query SSEs in query order, the
    places where they step down; sequential without one, circular with one when the last image lies below the first,
    else permuted; cut = the 1-based query SSE that starts the second run of a circular map"""
    at = [i for i, j in enumerate(m) if j >= 0]
    img = [int(m[i]) for i in at]
    down = [s for s in range(1, len(img)) if img[s] < img[s - 1]]
    if not down:
        return SEQ, len(img), 0, 0
    if len(down) == 1 and img[-1] < img[0]:
        return CIRC, len(img), 1, at[down[0]] + 1
    return PERM, len(img), len(down), 0


def mixed_db():
    return sat.synth.make_db(len(MIXED_ORDERS), orders=list(MIXED_ORDERS), seed=5, sort=False)


def planted_db(name_format="s%07d"):
    """(name_format: the command line reads names of up to 7 characters from stdin)"""
    return sat.synth.make_db(len(PLANTED_ORDERS), orders=list(PLANTED_ORDERS), seed=5, sort=False, name_format=name_format)


def rotation(n):
    """the list c .. n - 1, 0 .. c - 1 with c = n // 2, and the cut a circular map of it onto its source has"""
    c = n // 2
    return list(range(c, n)) + list(range(c)), n - c + 1


def tiled(db, n):
    """the structures of db repeated to n entries, with names of their own"""
    tabs, dmats, orders = [], [], []
    for e in range(n):
        t, d = db.dense(e % len(db))
        tabs.append(t)
        dmats.append(d)
        orders.append(int(db.orders[e % len(db)]))
    return sat.StructSet.from_dense(orders, tabs, dmats, ["t%06d" % e for e in range(n)])


def expected_rows(scores, maps, stats, base_scores, base_p, n1s, max_p, min_base_p, kinds, k=None):
    """Per query the rows sat_reorder_hits must return, as a list of dicts, and their maps.
    scores int32[nq, n], maps int32[nq, n, 111]: sat_results of the unordered search; stats: topk_hits(n) of it - the rows
    carry every row's statistics doubles; base_scores, base_p [nq, n]: the ordered search's, by entry."""
    nq, n = scores.shape
    out, out_maps = [], []
    for q in range(nq):
        ranked = stats[q]
        assert sorted(ranked["entry"].tolist()) == list(range(n))
        rows, rmaps = [], []
        for h in ranked:                                    # descending score, ties in database order
            e = int(h["entry"])
            assert int(h["score"]) == int(scores[q, e])
            kd = kind(maps[q, e, :int(n1s[q])])
            if h["pvalue"] <= max_p and (min_base_p <= 0 or base_p[q, e] >= min_base_p) and (kinds & kd[0]):
                rows.append(dict(hit=h, base_pvalue=base_p[q, e], base_score=int(base_scores[q, e]), kind=kd[0], matched=kd[1],
                                 descents=kd[2], cut=kd[3]))
                rmaps.append(maps[q, e])
        if k:
            rows, rmaps = rows[:k], rmaps[:k]
        out.append(rows)
        out_maps.append(np.array(rmaps, np.int32).reshape(-1, MAXDIM))
    return out, out_maps


def same_rows(got, got_maps, want, want_maps, what=""):
    assert len(got) == len(want), what
    for q in range(len(want)):
        assert len(got[q]) == len(want[q]), (what, q, len(got[q]), len(want[q]))
        for r, (g, w) in enumerate(zip(got[q], want[q])):
            assert g["hit"].tobytes() == w["hit"].tobytes(), (what, q, r)
            assert g["base_pvalue"].tobytes() == np.float64(w["base_pvalue"]).tobytes(), (what, q, r)
            for f in ("base_score", "kind", "matched", "descents", "cut"):
                assert int(g[f]) == w[f], (what, q, r, f, int(g[f]), w[f])
            assert int(g["pad"]) == 0
        if got_maps is not None:
            assert got_maps[q].dtype == np.int32 and np.array_equal(got_maps[q].reshape(-1, MAXDIM), want_maps[q]), (what, q)


def kinds_present(want):
    return set(r["kind"] for rows in want for r in rows)
