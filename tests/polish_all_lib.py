"""Shared by the tests of the whole-database polish (tests/test_gpu_polish_all.py): the CPU reference of a (database,
query batch), the synthetic database of the lane-group edges, and - run as a script in a child process, because
SAT_EXP_POLISH_GROUP is read when a context is created - that database's polished rows under the environment it was
started with."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GROUP_ORDERS = (1, 2, 15, 16, 16, 17, 31, 32, 32, 33, 64, 65)      # unsorted: 5 entries of up to 16 SSEs, 4 of 17..32
GROUP_CASES = ((3, 64), (8, 64), (8, 2))                            # (tops, restarts)
GROUP_FIRST = 5                                                     # ordinal of the first query


class Reference:
    """The CPU reference of a (database, query batch): the restarts' own bests of a pair are computed once, at the
    largest restart count asked for (restart r is the same stream whatever the count), and shared by the tests."""

    def __init__(self, db, queries, first_ordinal=0):
        self.db, self.queries, self.first = db, queries, first_ordinal
        self.runs, self.pairs = {}, {}

    def restarts(self, q, e, lorder, maxstart):
        import matches_lib
        key = (q, e, lorder)
        if key not in self.runs or len(self.runs[key][0]) < maxstart:
            self.runs[key] = matches_lib.restarts(self.db, e, self.queries[q], lorder, maxstart, self.first + q)
        sc, mp = self.runs[key]
        return sc[:maxstart], mp[:maxstart]

    def all_rows(self, lorder, maxstart, tops):
        """(scores [nq, N], base [nq, N], maps [nq, N, 111]) of every (query, entry), as a polished search lays them out"""
        import polish_lib
        nq, n = len(self.queries), len(self.db)
        scores, base = np.zeros((nq, n), np.int32), np.zeros((nq, n), np.int32)
        maps = np.full((nq, n, 111), -1, np.int32)
        for q in range(nq):
            n1 = len(self.queries[q][2])
            for e in range(n):
                if (q, e) not in self.pairs:
                    self.pairs[(q, e)] = polish_lib.Pair.of(self.db, e, self.queries[q])
                sc, mp = self.restarts(q, e, lorder, maxstart)
                got = polish_lib.polish_ranked(self.pairs[(q, e)], sc, mp, lorder, tops)
                scores[q, e], base[q, e] = got[0], got[1]
                maps[q, e, :n1] = np.asarray(got[4])[:n1]
        return scores, base, maps


def polished(db, queries, tops, lorder, maxstart, first_ordinal=0):
    """(scores, base, maps) of a polished search of a fresh context"""
    import cuda_satabsearch_amd as sat
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries, first_ordinal)
        s.set_polish_all(tops)
        scores, maps, _ = s.search(lorder, True, maxstart)
        return scores, s.results_base(), maps


def group_db():
    """the database of GROUP_ORDERS and queries of 1, 16, 17, 33 and 111 SSEs: the list compaction of a 16-lane group in
    1, 1, 2, 3 and 7 trips"""
    import cuda_satabsearch_amd as sat
    db = sat.synth.make_db(len(GROUP_ORDERS), orders=np.array(GROUP_ORDERS, np.int32), seed=77, sort=False)
    queries = [sat.synth.make_query(1, seed=41), sat.synth.planted_query(db, 7, keep=0.5, seed=42),
               sat.synth.planted_query(db, 9, keep=17 / 33.0, seed=43), sat.synth.planted_query(db, 11, keep=33 / 65.0, seed=44),
               sat.synth.make_query(111, seed=45)]
    assert [len(q[2]) for q in queries] == [1, 16, 17, 33, 111]
    return db, queries


def group_rows():
    """the polished rows of every case of GROUP_CASES, LORDER T then F: {name: array}"""
    db, queries = group_db()
    out = {}
    for tops, maxstart in GROUP_CASES:
        for lorder in (True, False):
            sc, base, maps = polished(db, queries, tops, lorder, maxstart, GROUP_FIRST)
            key = "T%d_r%d_%s" % (tops, maxstart, "T" if lorder else "F")
            out[key + "_scores"], out[key + "_base"], out[key + "_maps"] = sc, base, maps
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **group_rows())
