"""Call sequences on ONE context (tests/test_gpu_history.py, tests/test_history_cpu.py): worlds, operations with their
CPU references, a model of the documented context state, and seeded schedules.

* A WORLD is (database, query batch, first ordinal), synthetic with fixed seeds: six databases (largest entry <= 16,
  <= 32, 33..48 and 111 SSEs; 150 entries for the shards; 1100 entries, which with four queries leave the single-launch
  plan) and the batches of COMBOS.  A database's restart counts are 1, 3 and its RMAX (100, 64, 32, 16, 16, 8).  The
  planted queries come from a few source structures whose leading blocks stand in every database (IMPLANTS), so that
  every world has hits, related entries and an entry with two matches: tests/test_history_cpu.py checks that no
  reference is vacuous.
* An OPERATION is a kind and parameters.  run() calls the library, expect() computes the same tuple of arrays from CPU
  code only: oracle_lib.search (whole rows), matches_lib / polish_lib (restarts, the greedy rule, the polish) and
  select_lib (the selection passes, the fit, the clustering).  No GPU context is ever a reference.  References are cached
  per (world, parameters), so a schedule that comes back to a world costs nothing more.
* The MODEL restates include/satabsearch.h: what is resident, whether and how the batch was searched, the installed fit,
  the accumulator (plain or leveled), the polish-all setting, the cover accumulator, whether classes are installed, and
  the baseline as (search, fit) at keep time.  It says which calls must succeed and which score matrix they read.
* schedule(seed) is a greedy cover: walks of WALK_STEPS steps, each on a fresh context, that between them run every
  ordered pair (kind A directly followed by kind B) the model allows.  Test infrastructure only.
* The kinds of NEW_KINDS (the leveled accumulator, the cover, the evaluation, motif batches, the profile, the baseline and
  the reordered hits) came later.  schedule(seed, multi) still walks the 27 kinds of KINDS and returns the walks it always
  returned; schedule(seed, multi, new=True) walks ALL_KINDS and follows every allowed pair with a new kind in it, over
  the six databases and one more, "dperm", whose implants are rotated and block-swapped source structures."""
import collections

import numpy as np

import cuda_satabsearch_amd as sat
import cover_lib
import eval_lib
import matches_lib
import motif_lib
import oracle_lib
import polish_all_lib as pal
import polish_lib
import profile_lib
import reorder_lib
import select_lib
from cuda_satabsearch_amd.search import _EVAL_DTYPE, _REORDER_DTYPE

MAXDIM = 111
WALK_STEPS = 40
SEED, WALKS, MULTI_WALKS = 1, 24, 12     # schedule(SEED) has WALKS walks, schedule(SEED, True) MULTI_WALKS (test_history_cpu.py)
NEW_WALKS, NEW_MULTI_WALKS = 41, 27       # schedule(SEED, False, True) and schedule(SEED, True, True)
MAX_LEVELS = 8                           # SAT_MAX_CLUSTER_LEVELS

# ---------------------------------------------------------------- worlds
RMAX = {"d16": 100, "d32": 64, "d48": 32, "d111": 16, "d150": 16, "d1100": 8}


def rmax_of(name):
    """the largest restart count of database `name` (the permutant world: 16)"""
    return RMAX.get(name, 16)


# the batches a database is searched with (a batch made from a database stays with it)
COMBOS = {"d16": ("q1", "q5", "db"), "d32": ("q1", "q5", "q2", "q4", "db"), "d48": ("q2", "q5", "db"),
          "d111": ("q5",), "d150": ("q2", "q4"), "d1100": ("q4",)}
# the databases and batches of the new schedule: the old ones, the permutant world, and motif batches where "db" is
NEW_COMBOS = dict({k: v + (("motif",) if "db" in v else ()) for k, v in COMBOS.items()}, dperm=("q2", "q4", "db", "motif"))
FIRST = {"q1": 0, "q5": 5, "q2": 2, "q4": 1, "db": 3, "motif": 3}
BIG = ("d1100",)       # 4400 rows: whole-row references only (no polished search, no search_matches), to keep the CPU side short
LARGEST, SMALLEST = ("d111", "q5"), ("d16", "q1")        # they differ in entries, queries, largest n1 and largest n2

_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


DB_SEEDS = {"d16": 300}        # chosen so that each of its worlds shows a polish whose winner is not the best restart
SOURCE_ORDERS = (32, 32, 65, 111, 16)
# (database: {entry: (order, source)}): the leading block of a source structure stands at these entries, so that the
# planted queries of every batch have a real hit in every database they are searched with
IMPLANTS = {"d16": {1: (16, 4), 3: (12, 4)},
            "d32": {0: (32, 0), 15: (24, 0), 20: (32, 1), 33: (17, 2), 5: (1, 3), 11: (2, 3), 8: (16, 4)},
            "d48": {5: (32, 0), 3: (20, 0), 2: (48, 2), 9: (33, 3), 7: (32, 1), 13: (6, 3), 11: (16, 4)},
            "d111": {1: (111, 3), 2: (65, 2), 4: (97, 3)},
            "d150": {7: (48, 2), 0: (32, 0), 20: (32, 1), 30: (16, 4)},
            "d1100": {3: (32, 0), 20: (32, 1), 900: (8, 2), 40: (16, 4)},
            "dperm": {2: (32, 0), 11: (24, 1), 17: (16, 4), 23: (20, 0)}}
# "dperm": (entry: (order, source, how)) - the leading block of a source structure with its SSEs rotated by half
# (reorder_lib.rotation: a circular map onto the source) or with two inner blocks swapped (a permuted one)
PERMUTANTS = {5: (32, 0, "rot"), 8: (32, 1, "rot"), 14: (16, 4, "rot"), 20: (32, 0, "swap"), 26: (32, 1, "swap"), 29: (24, 0, "rot")}


def permutation(order, how):
    """the entry's SSE i is the source's SSE permutation[i]"""
    if how == "rot":
        return reorder_lib.rotation(order)[0]
    a, b, c = order // 4, order // 2, 3 * order // 4                             # blocks 0 | 2 | 1 | 3
    return list(range(a)) + list(range(b, c)) + list(range(a, b)) + list(range(c, order))


def motif():
    """the 8-SSE query: source structure 4 holds it twice"""
    return _memo("motif", lambda: sat.synth.make_query(8, seed=49))


def source():
    """the structures the planted queries come from; the last one (16 SSEs) is the 8-SSE motif twice in one chain, so
    that an entry with two non-overlapping matches of it exists"""
    def make():
        src = sat.synth.make_db(len(SOURCE_ORDERS), orders=np.array(SOURCE_ORDERS, np.int32), seed=0x50C, sort=False)
        t, d = src.dense(4)
        t8, d8, _ = motif()
        for at in (0, 8):
            t[at:at + 8, at:at + 8], d[at:at + 8, at:at + 8] = t8, d8
        ii, jj = np.tril_indices(16)
        o = int(src.cell_off[4])
        src.tab[o:o + ii.size], src.dist[o:o + ii.size] = t[ii, jj], d[ii, jj]
        return src
    return _memo("source", make)


def _orders(name):
    if name == "d16":
        o = np.array([7, 16, 1, 12, 9], np.int32)
    elif name == "d111":
        o = np.array([60, 111, 65, 72, 97, 61, 88, 111, 64, 100, 66, 80], np.int32)
    else:
        n, lo, hi = {"d32": (40, 3, 32), "d48": (18, 6, 48), "d150": (150, 6, 48), "d1100": (1100, 8, 32), "dperm": (30, 5, 32)}[name]
        o = np.random.default_rng(len(name) * 1000 + n).integers(lo, hi + 1, n).astype(np.int32)
    for k, (order, _) in IMPLANTS[name].items():
        o[k] = order
    if name == "dperm":
        for k, (order, _, _) in PERMUTANTS.items():
            o[k] = order
    return o


def db(name):
    """the database `name`, unsorted"""
    def make():
        o = _orders(name)
        d = sat.synth.make_db(len(o), orders=o, seed=DB_SEEDS.get(name, 0xD0 + len(o)), sort=False)
        for k, (order, s) in IMPLANTS[name].items():
            t, dm = source().dense(s)
            ii, jj = np.tril_indices(order)
            at = int(d.cell_off[k])
            d.tab[at:at + ii.size], d.dist[at:at + ii.size] = t[ii, jj], dm[ii, jj]
        for k, (order, s, how) in (PERMUTANTS if name == "dperm" else {}).items():
            t, dm = source().dense(s)
            perm = np.array(permutation(order, how))
            t, dm = t[np.ix_(perm, perm)], dm[np.ix_(perm, perm)]
            ii, jj = np.tril_indices(order)
            at = int(d.cell_off[k])
            d.tab[at:at + ii.size], d.dist[at:at + ii.size] = t[ii, jj], dm[ii, jj]
        return d
    return _memo(("db", name), make)


def classes(name):
    """the classification of database `name`: an implant (or permutant) has its source as its class, the others 5 + e mod 3,
    and every fifth of those is unclassified"""
    def make():
        n = len(db(name))
        c = np.array([-1 if e % 5 == 4 else 5 + e % 3 for e in range(n)], np.int32)
        for k, v in list(IMPLANTS[name].items()) + list((PERMUTANTS if name == "dperm" else {}).items()):
            c[k] = v[1]
        return c
    return _memo(("classes", name), make)


def motif_lists(name):
    """the SSE lists of the motif batch of database `name`, one per entry of db_indices: the first SSEs backwards, the whole
    entry, every other SSE, the entry rotated by half - in turn"""
    out = []
    for q, e in enumerate(db_indices(name).tolist()):
        o = int(db(name).orders[e])
        out.append([list(range(min(o, 9) - 1, -1, -1)), None, list(range(0, o, 2)), reorder_lib.rotation(o)[0]][q % 4])
    return out


def db_indices(name):
    """the entries set_queries_from_db takes from database `name`: any order, one repeat"""
    n = len(db(name))
    idx = list(IMPLANTS[name])[:4] + [(3 * i + 1) % n for i in range(2)]       # related entries and unrelated ones
    return np.array(idx + idx[:1], np.int32)


def batch(key):
    """(queries [(tab, dmat, types)], first ordinal) of batch `key`: "q1" one query of 8 SSEs (set_query), "q5" five of
    3, 16, 17, 40 and 111 SSEs (every class; planted and foreign), "q2" 24 and 32 SSEs, "q4" four of 20..32 SSEs,
    ("db", name) entries of that database."""
    def make():
        src, sy = source(), sat.synth
        if key == "q1":
            qs = [motif()]
        elif key == "q5":
            qs = [sy.make_query(3, seed=51), sy.planted_query(src, 4, keep=1.0, seed=52), sy.make_query(17, seed=53),
                  sy.planted_query(src, 2, keep=40 / 65.0, seed=54), sy.planted_query(src, 3, keep=1.0, jitter=0.5, seed=55)]
        elif key == "q2":
            qs = [sy.planted_query(src, 1, keep=0.75, seed=56), sy.planted_query(src, 0, keep=1.0, seed=57)]
        elif key == "q4":
            qs = [sy.make_query(20, seed=58), sy.planted_query(src, 0, keep=1.0, seed=59), sy.make_query(28, seed=60),
                  sy.planted_query(src, 1, keep=0.75, seed=61)]
        elif key[0] == "motif":
            qs = motif_lib.dense_queries(db(key[1]), db_indices(key[1]), motif_lists(key[1]))      # cut on the host
        else:
            d = db(key[1])
            qs = [d.dense(int(i)) + (d.ssetypes(int(i)),) for i in db_indices(key[1])]
        return qs, FIRST[key if isinstance(key, str) else key[0]]
    return _memo(("batch", key), make)


def n1s_of(bkey):
    return [len(q[2]) for q in batch(bkey)[0]]


# ---------------------------------------------------------------- the CPU reference of a world
Searched = collections.namedtuple("Searched", "lorder r lsoln tops")          # tops > 0: a polished search


class WorldRef:
    """Everything the library may return for (database, batch), from CPU code.  Whole-row scores come from
    oracle_lib.search, restarts from the chain oracle (shared by every restart count: restart r is one stream)."""

    def __init__(self, dbname, bkey):
        self.db = db(dbname)
        self.queries, self.first = batch(bkey)
        self.n, self.nq = len(self.db), len(self.queries)
        self.n1s = [len(q[2]) for q in self.queries]
        self.n1max = max(self.n1s)
        self.rmax = rmax_of(dbname)
        self.pal = pal.Reference(self.db, self.queries, self.first)
        self.memo = {}

    def restarts(self, q, e, lorder, r):
        self.pal.restarts(q, e, lorder, max(r, self.rmax))                       # one run serves every count
        return self.pal.restarts(q, e, lorder, r)

    def pair(self, q, e):
        if (q, e) not in self.pal.pairs:
            self.pal.pairs[(q, e)] = polish_lib.Pair.of(self.db, e, self.queries[q])
        return self.pal.pairs[(q, e)]

    def plain(self, lorder, r):
        """(scores [nq, n], maps [nq, n, 111]) of the plain search"""
        def make():
            out = [oracle_lib.search(self.db, *self.queries[q], lorder, True, r, query_ordinal=self.first + q)[:2]
                   for q in range(self.nq)]
            return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
        return _memo2(self.memo, ("plain", lorder, r), make)

    def polished(self, lorder, r, tops):
        """(scores, base, maps) of the polished search"""
        def make():
            for q in range(self.nq):
                for e in range(self.n):
                    self.restarts(q, e, lorder, r)
            return self.pal.all_rows(lorder, r, tops)
        return _memo2(self.memo, ("polished", lorder, r, tops), make)

    def matrix(self, sd):
        """(scores, maps or None): what the result calls read after the search `sd`"""
        if sd.tops:
            sc, _, mp = self.polished(sd.lorder, sd.r, sd.tops)
        else:
            sc, mp = self.plain(sd.lorder, sd.r)
        return sc, (mp if sd.lsoln else None)

    def fits(self, sd, fit):
        """the sat_fit records of the model's fit descriptor: None, ("fit", censor) or ("set", name)"""
        if fit is None:
            return None
        if fit[0] == "fit":
            return self.select(sd, None).fit(fit[1])
        rec = np.zeros(self.nq, select_lib._FIT_DTYPE)
        for q in range(self.nq):
            if q == 0 or q < self.nq - 1:                                        # the last of several keeps the built-ins
                rec[q]["a"], rec[q]["b"], rec[q]["fitted"] = 2.0 + 0.5 * q, 0.75, 1
        return rec

    def select(self, sd, fit):
        def make():
            sc, mp = self.matrix(sd)
            return select_lib.Reference(sc, self.n1s, self.db.orders, self.fits(sd, fit), mp)
        return _memo2(self.memo, ("select", sd, fit), make)

    def pcut(self, sd, fit, frac, nodes=None):
        """a cutoff from the reference's own p-values: the one `frac` of the way up its distinct values (with `nodes`,
        the queries' nodes: those of the rows that are edges, not a structure against itself)"""
        ref = self.select(sd, fit)
        rows = [ref.rows(q) for q in range(self.nq)]
        if nodes is not None:
            rows = [r[r["entry"] != nodes[q]] for q, r in enumerate(rows)]
        pv = np.unique(np.concatenate([r["pvalue"] for r in rows]))
        return float(pv[int(frac * (len(pv) - 1))])

    def pvalues(self, sd, fit):
        """float64[nq, n]: every row's p-value by entry - what sat_baseline_keep keeps of the search `sd` under `fit`"""
        def make():
            ref, out = self.select(sd, fit), np.zeros((self.nq, self.n), np.float64)
            for q in range(self.nq):
                out[q, ref.rows(q)["entry"]] = ref.rows(q)["pvalue"]
            return out
        return _memo2(self.memo, ("pvalues", sd, fit), make)

    def base_cut(self, base, frac):
        """a min_base_pvalue from the baseline's own distinct p-values (None: no condition)"""
        if frac is None:
            return 0.0
        pv = np.unique(self.pvalues(*base))
        return float(pv[int(frac * (len(pv) - 1))])

    def edges(self, sd, fit, cut, qnodes):
        """(a, b): the rows of the search with pvalue <= cut as pairs (query's node, entry), self pairs included"""
        ref = self.select(sd, fit)
        a, b = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
        for q in range(self.nq):
            ents = ref.rows(q)["entry"][ref.rows(q)["pvalue"] <= cut].astype(np.int64)
            a.append(np.full(len(ents), qnodes[q], np.int64))
            b.append(ents)
        return np.concatenate(a), np.concatenate(b)

    def profile(self, sd, fit, cut, qnodes):
        """(hits uint32[nq], [joint uint32[n1, n1]]) of sat_profile_rows at `cut`"""
        ref, mp = self.select(sd, fit), self.matrix(sd)[1]
        hits, joint = np.zeros(self.nq, np.uint32), []
        for q in range(self.nq):
            ents = ref.rows(q)["entry"][ref.rows(q)["pvalue"] <= cut]
            h, j = profile_lib.expected(np.asarray(mp[q])[ents].reshape(-1, mp.shape[2]), ents, self.n1s[q], qnodes[q])
            hits[q] = h
            joint.append(j)
        return hits, joint

    def reorder(self, sd, fit, base, cut, base_cut, kinds, k):
        """(rows per query as _REORDER_DTYPE arrays, their maps) of sat_reorder_hits: reorder_lib.expected_rows over the
        unordered search's matrix, its ranked rows and the baseline (Searched, fit) kept before"""
        sc, mp = self.matrix(sd)
        ref = self.select(sd, fit)
        want, _ = reorder_lib.expected_rows(sc, mp, [ref.rows(q) for q in range(self.nq)], self.matrix(base[0])[0],
                                            self.pvalues(*base), self.n1s, cut, base_cut, kinds, k)
        rows, maps = [], []
        for q in range(self.nq):
            out = np.zeros(len(want[q]), _REORDER_DTYPE)
            for i, r in enumerate(want[q]):
                out[i]["hit"] = r["hit"]
                for f in ("base_pvalue", "base_score", "kind", "matched", "descents", "cut"):
                    out[i][f] = r[f]
            rows.append(out)
            maps.append(ref.row_maps(q, out["hit"]["entry"]))
        return rows, maps

    def pairs(self, count):
        """a list of `count` (query, entry) pairs: any order, repeats"""
        rng = np.random.default_rng(count * 7919 + self.n * 31 + self.nq)
        return rng.integers(0, self.nq, count).astype(np.int32), rng.integers(0, self.n, count).astype(np.int32)

    def match_rows(self, q, e, lorder, r, m):
        """(counts [P], scores [P, M], restarts [P, M], maps [P, M, n1max]) of the pairs, by the greedy rule"""
        counts = np.zeros(len(q), np.int32)
        scores, rs = np.zeros((len(q), m), np.int32), np.zeros((len(q), m), np.int32)
        maps = np.full((len(q), m, self.n1max), -1, np.int32)
        for p, (qi, ei) in enumerate(zip(q.tolist(), e.tolist())):
            c, sc, rr, mp = matches_lib.select_matches(*self.restarts(qi, ei, lorder, r), m)
            counts[p], scores[p], rs[p] = c, sc, rr
            maps[p, :, :self.n1s[qi]] = mp[:, :self.n1s[qi]]
        return counts, scores, rs, maps

    def polish_rows(self, q, e, lorder, r, tops):
        """(scores, base, restarts, moves [P], maps [P, n1max]) of the pairs"""
        out = [np.zeros(len(q), np.int32) for _ in range(4)] + [np.full((len(q), self.n1max), -1, np.int32)]
        for p, (qi, ei) in enumerate(zip(q.tolist(), e.tolist())):
            got = _memo2(self.memo, ("polish", qi, ei, lorder, r, tops), lambda: polish_lib.polish_ranked(
                self.pair(qi, ei), *self.restarts(qi, ei, lorder, r), lorder, tops))
            for k in range(4):
                out[k][p] = got[k]
            out[4][p, :self.n1s[qi]] = np.asarray(got[4])[:self.n1s[qi]]
        return tuple(out)

    def refine(self, lorder, r, cand, big_r, k, lsoln, tops=0):
        """the ranking rule of the refine calls restated: each query's best C rows of the plain search at r in best-k
        order, their stage-2 scores (the plain search at R, or its polish), the best K by (score descending, entry
        ascending) with the built-in statistics of the stage-2 score.  (hits [nq, K], maps [nq, K, 111], stage-1 scores,
        scores before the polish)"""
        c = min(cand, self.n)
        kk = min(k, c)
        stage1 = self.plain(lorder, r)[0]
        hits = np.zeros((self.nq, kk), select_lib._HIT_DTYPE)
        maps = np.full((self.nq, kk, MAXDIM), -1, np.int32)
        first, base = np.zeros((self.nq, kk), np.int32), np.zeros((self.nq, kk), np.int32)
        for q in range(self.nq):
            cands = np.argsort(-stage1[q].astype(np.int64), kind="stable")[:c]
            if tops:
                qq = np.full(len(cands), q, np.int32)
                s2, b2, _, _, m2 = self.polish_rows(qq, cands.astype(np.int32), lorder, big_r, tops)
            else:
                sc, mp = self.plain(lorder, big_r)
                s2, b2, m2 = sc[q, cands], sc[q, cands], mp[q, cands]
            order = sorted(range(len(cands)), key=lambda i: (-int(s2[i]), int(cands[i])))[:kk]
            for row, i in enumerate(order):
                e = int(cands[i])
                norm2 = 2.0 * int(s2[i]) / float(self.n1s[q] + int(self.db.orders[e]))
                hits[q, row] = (e, s2[i], norm2) + select_lib.builtin_stats(norm2)
                maps[q, row, :self.n1s[q]] = m2[i][:self.n1s[q]]
                first[q, row], base[q, row] = stage1[q, e], b2[i]
        return hits, (maps if lsoln else None), first, base


def _memo2(memo, key, make):
    if key not in memo:
        memo[key] = make()
    return memo[key]


def world_ref(dbname, bkey):
    return _memo(("ref", dbname, bkey), lambda: WorldRef(dbname, bkey))


# ---------------------------------------------------------------- operations
Op = collections.namedtuple("Op", "kind args")


def op(kind, **args):
    return Op(kind, tuple(sorted(args.items())))


MOVES = ("upload", "upload_dense", "set_queries", "set_query", "set_queries_from_db", "set_polish_all", "polish_all_off",
         "cluster_begin", "cluster_add", "cluster_end")                          # no data comes back
SEARCHES = ("search", "search_async_results", "upload_search", "search_matches", "search_refine", "search_refine_polish")
PAIR_SEARCHES = ("search_pairs", "search_pairs_matches", "search_pairs_polish")
RESULTS = ("results", "results_base", "topk_hits", "hits_cutoff", "score_histogram", "fit_statistics", "set_statistics")
KINDS = MOVES + SEARCHES + PAIR_SEARCHES + RESULTS + ("cluster_labels",)
# the kinds added since (DESIGN.md 6p .. 6u)
NEW_MOVES = ("set_queries_motif", "cluster_begin_levels", "cluster_add_levels", "cover_begin", "cover_add", "cover_end",
             "set_eval_classes", "eval_classes_off", "baseline_keep", "baseline_drop")
NEW_DATA = ("cluster_labels_levels", "cover_solve", "eval_rows", "eval_tables", "profile_rows", "baseline_results", "reorder_hits",
            "search_reordered")
NEW_KINDS = NEW_MOVES + NEW_DATA
ALL_KINDS = KINDS + NEW_KINDS
DATA_KINDS = tuple(k for k in ALL_KINDS if k not in MOVES + NEW_MOVES)
# what sat_multi has (search_topk and search_fit stand for topk_hits and fit_statistics: they search again, the same way)
OLD_MULTI_KINDS = ("upload", "set_queries", "set_queries_from_db", "set_polish_all", "polish_all_off", "cluster_begin", "cluster_add",
                   "search", "search_matches", "search_refine", "search_refine_polish", "search_pairs_matches", "search_pairs_polish",
                   "topk_hits", "hits_cutoff", "score_histogram", "fit_statistics", "set_statistics", "cluster_labels")
MULTI_KINDS = OLD_MULTI_KINDS + tuple(k for k in NEW_KINDS if k not in ("cover_end", "eval_tables"))
# the counts a kind has of its own, smallest and largest
COUNTS = {"pairs": (1, 7, 30), "m": (1, 3, 8), "tops": (1, 3, 8), "k": (1, 3, 10), "cand": (4, 12)}
QUERY_SETTING = ("set_queries", "set_query", "set_queries_from_db", "set_queries_motif")


def level_cuts(dbname, levels):
    """the `levels` strictly ascending cutoffs of a leveled accumulator begun on database `dbname`: the call comes before
    the adds, so they are quantiles (0.05 .. 0.7) of the distinct built-in p-values of the database searched with its own
    entries (else its first batch) at its largest restart count - and, where those are too few, of them and the midpoints
    between them, taken again until there are enough"""
    def make():
        w = world_ref(dbname, ("db", dbname) if "db" in NEW_COMBOS[dbname] else NEW_COMBOS[dbname][0])
        pv = np.unique(w.pvalues(Searched(True, w.rmax, False, 0), None))
        pv = pv[(pv > 0.0) & (pv < 1.0)]
        while len(pv) < 2 * levels:
            pv = np.unique(np.concatenate([pv, (pv[1:] + pv[:-1]) / 2, pv[:1] / 2, (pv[-1:] + 1.0) / 2]))
        at = np.unique(np.linspace(0.05 * (len(pv) - 1), 0.7 * (len(pv) - 1), levels).round().astype(int))
        assert len(at) == levels, (dbname, levels, len(pv))
        return tuple(float(x) for x in pv[at])
    return _memo(("level_cuts", dbname, levels), make)


class Model:
    """The documented state of a context (include/satabsearch.h), restated."""

    def __init__(self, multi=False, new=False):
        self.multi, self.new = multi, new    # new: operations are drawn over NEW_COMBOS
        self.db = self.batch = None          # names of the resident database and the current batch
        self.searched = None                 # Searched of the search the result buffers hold, None: not for this batch
        self.fit = None                      # the installed fit: None, ("fit", censor), ("set", name)
        self.cluster = None                  # the accumulator: [nodes, [(world, Searched, fit, frac, query nodes)], levels]
        self.tops = 0                        # sat_polish_all_set       (levels: None plain, else (database, count): level_cuts)
        self.cover = None                    # the cover accumulator: [nodes, [adds, as the accumulator's]]
        self.classes = False                 # is classes(self.db) installed?
        self.baseline = None                 # (Searched, fit) as they were at sat_baseline_keep; of (self.db, self.batch)

    def leveled(self):
        return self.cluster is not None and self.cluster[2] is not None

    def legal(self, kind):
        """must the call succeed now?"""
        if self.multi and kind not in MULTI_KINDS:
            return False
        if self.new and self.db is not None:          # what the worlds do not have (draw returns None): the second schedule's
            needs = {"set_query": "q1", "set_queries_from_db": "db", "set_queries_motif": "motif"}      # routes know it
            if kind in needs and needs[kind] not in NEW_COMBOS[self.db]:
                return False
            if kind in ("set_polish_all", "search_matches") and self.db in BIG:
                return False
        if kind in ("upload", "upload_dense", "set_queries", "set_query", "set_polish_all", "polish_all_off", "eval_classes_off",
                    "baseline_drop"):
            return True
        if kind in ("set_queries_from_db", "cluster_begin", "set_queries_motif", "cluster_begin_levels", "cover_begin",
                    "set_eval_classes"):
            return self.db is not None
        if kind == "upload_search":
            return self.batch is not None
        if kind in SEARCHES or kind in PAIR_SEARCHES or kind == "search_reordered":
            return self.db is not None and self.batch is not None
        if kind == "cluster_end":
            return self.cluster is not None
        if kind in ("cluster_labels", "cluster_labels_levels"):                   # the calls of the other kind are SAT_ESTATE
            return self.cluster is not None and self.leveled() == (kind == "cluster_labels_levels")
        if kind in ("cluster_add", "cluster_add_levels"):
            return self.cluster is not None and self.leveled() == (kind == "cluster_add_levels") and self.searched is not None
        if kind in ("cover_solve", "cover_end"):
            return self.cover is not None
        if kind == "cover_add":
            return self.cover is not None and self.searched is not None
        if kind == "results_base":
            return self.searched is not None and self.searched.tops > 0
        if kind == "baseline_results":
            return self.baseline is not None
        if kind == "reorder_hits":                                                # (a baseline is always of the current shape:
            return self.baseline is not None and bool(self.searched and self.searched.lsoln)      # what changes it drops it)
        if kind == "profile_rows":
            return bool(self.searched and self.searched.lsoln)
        if kind in ("eval_rows", "eval_tables"):
            return self.searched is not None and self.classes
        return self.searched is not None                                          # the other result calls, baseline_keep

    def flags(self):
        sd = self.searched
        return (self.db is not None, self.batch is not None, sd is not None, bool(sd and sd.lsoln), bool(sd and sd.tops),
                self.fit is not None, self.cluster is not None, self.tops > 0,
                self.leveled(), self.cover is not None, self.classes, self.baseline is not None) + (
                    tuple(b in NEW_COMBOS[self.db] for b in ("q1", "db")) + (self.db in BIG,) if self.new and self.db else ())

    def world(self):
        return world_ref(self.db, self.batch)

    def apply(self, o):
        a, kind = dict(o.args), o.kind
        if kind in ("upload", "upload_dense", "upload_search"):
            self.db, self.searched, self.fit, self.cluster = a["db"], None, None, None
            self.cover, self.classes, self.baseline = None, False, None
        if kind in QUERY_SETTING:
            self.batch, self.searched, self.fit, self.baseline = a["batch"], None, None, None
        if kind in ("set_polish_all", "polish_all_off"):
            self.tops = a["tops"] if kind == "set_polish_all" else 0
        if kind in ("search", "search_async_results", "upload_search"):
            self.searched, self.fit = Searched(a["lorder"], a["r"], a["lsoln"], self.tops), None
        if kind in ("search_matches", "search_refine", "search_refine_polish"):      # match 0 / stage 1: a plain search
            self.searched, self.fit = Searched(a["lorder"], a["r"], False, 0), None
        if kind == "topk_hits" and self.multi:
            self.fit = None                                                       # search_topk searches again
        if kind == "fit_statistics":
            self.fit = ("fit", a["censor"])
        if kind == "set_statistics":
            self.fit = None if a["fit"] == "none" else ("set", a["fit"])
        if kind == "cluster_begin":
            self.cluster = [len(db(self.db)), [], None]
        if kind == "cluster_begin_levels":                                        # a begin of either kind replaces what there was
            self.cluster = [len(db(self.db)), [], (self.db, a["levels"])]
        if kind in ("cluster_add", "cluster_add_levels"):
            self.cluster[1].append((self.db, self.batch, self.searched, self.fit, a.get("frac"), self.query_nodes()))
        if kind == "cluster_end":
            self.cluster = None
        if kind == "cover_begin":
            self.cover = [len(db(self.db)), []]
        if kind == "cover_add":
            self.cover[1].append((self.db, self.batch, self.searched, self.fit, a["frac"], self.query_nodes()))
        if kind == "cover_end":
            self.cover = None
        if kind in ("set_eval_classes", "eval_classes_off"):
            self.classes = kind == "set_eval_classes"
        if kind == "baseline_keep":                   # the rows as they are now: the search, the fit, the polish in `searched`
            self.baseline = (self.searched, self.fit)
        if kind == "baseline_drop":
            self.baseline = None
        if kind == "search_reordered":                # ordered search, its fit, keep; unordered search with maps, its fit
            fit = None if a["censor"] is None else ("fit", a["censor"])
            self.baseline = (Searched(True, a["r"], False, self.tops), fit)
            self.searched, self.fit = Searched(False, a["r"], True, self.tops), fit

    def query_nodes(self):
        """query q's node: its entry for a batch made of the database, any node otherwise"""
        nodes = self.cluster[0] if self.cluster else len(db(self.db))
        if not isinstance(self.batch, str):
            return tuple(int(i) for i in db_indices(self.batch[1]))
        return tuple((7 * q + 2) % nodes for q in range(len(n1s_of(self.batch))))


# ---- expect: the tuple of arrays an operation must return, from the state BEFORE it
def _flat_rows(rows, maps, counts):
    out = [np.asarray(counts, np.int32), np.concatenate(rows)]
    if maps is not None:
        out.append(np.concatenate(maps).reshape(-1, MAXDIM))
    return tuple(out)


def _expect(o, m):
    a, kind = dict(o.args), o.kind
    graph = kind in ("cluster_labels", "cluster_labels_levels", "cover_solve")   # of an accumulator: whatever the batch is now
    w = world_ref(a["db"], m.batch) if kind == "upload_search" else m.world() if not graph else None
    sd = m.searched
    if kind in ("search", "search_async_results", "upload_search"):
        sc, mp = w.matrix(Searched(a["lorder"], a["r"], a["lsoln"], m.tops))
        return (sc,) if mp is None else (sc, mp)
    if kind == "results":
        sc, mp = w.matrix(sd)
        return (sc,) if not a["lsoln"] else (sc, mp)
    if kind == "results_base":
        return (w.polished(sd.lorder, sd.r, sd.tops)[1],)
    if kind in ("search_matches", "search_pairs_matches"):
        if kind == "search_matches":
            q, e = np.divmod(np.arange(w.nq * w.n, dtype=np.int32), np.int32(w.n))
        else:
            q, e = w.pairs(a["pairs"])
        c, sc, rs, mp = w.match_rows(q, e, a["lorder"], a["r"], a["m"])
        return (c, sc, rs, mp) if a["maps"] else (c, sc, rs)
    if kind == "search_pairs":
        q, e = w.pairs(a["pairs"])
        sc, mp = w.plain(a["lorder"], a["r"])
        return (sc[q, e], mp[q, e]) if a["lsoln"] else (sc[q, e],)
    if kind == "search_pairs_polish":
        return w.polish_rows(*w.pairs(a["pairs"]), a["lorder"], a["r"], a["tops"])
    if kind in ("search_refine", "search_refine_polish"):
        hits, mp, first, base = w.refine(a["lorder"], a["r"], a["cand"], a["big_r"], a["k"], a["lsoln"], a.get("tops", 0))
        out = (hits, first) + ((base,) if kind == "search_refine_polish" else ())
        return out + ((mp,) if a["lsoln"] else ())
    if kind == "topk_hits":
        rows, mp = w.select(sd, None if m.multi else m.fit).topk(a["k"])      # search_topk searches again: the fit is gone
        return (rows, mp) if a["maps"] else (rows,)
    if kind == "hits_cutoff":
        rows, mp, counts = w.select(sd, m.fit).cutoff(w.pcut(sd, m.fit, a["frac"]), a["k"])
        return _flat_rows(rows, mp if a["maps"] else None, counts)
    if kind == "score_histogram":
        return w.select(sd, None).histogram()
    if kind == "fit_statistics":                                                  # the fit, then the rows it gives
        fit = ("fit", a["censor"])
        rows, _, counts = w.select(sd, fit).cutoff(w.pcut(sd, fit, 0.5), None)
        return (w.fits(sd, fit),) + _flat_rows(rows, None, counts)
    if kind == "set_statistics":
        return (w.select(sd, None if a["fit"] == "none" else ("set", a["fit"])).topk(3)[0],)
    if kind == "cluster_labels":
        nodes, adds, _ = m.cluster
        return _single_linkage(nodes, *_added_edges(adds))
    if kind == "cluster_labels_levels":
        nodes, adds, cuts = m.cluster[0], m.cluster[1], level_cuts(*m.cluster[2])
        per = [_single_linkage(nodes, *_added_edges(adds, cut)) for cut in cuts]
        labels, deg = np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
        for j in range(len(cuts) - 1):
            assert np.array_equal(labels[j + 1][labels[j]], labels[j + 1])          # the reference is nested too
        return labels, deg, np.array([p[2][0] for p in per], np.uint64)
    if kind == "cover_solve":
        nodes, adds = m.cover
        ea, eb = _added_edges(adds)
        rep, _, deg, edges, rounds = cover_lib.cover(nodes, ea, eb)
        cover_lib.check_invariants(nodes, ea, eb, rep)
        return rep, deg, np.array([edges, rounds], np.int64)
    if kind == "eval_rows":
        return (eval_lib.expected_rows(w.matrix(sd)[0], w.n1s, m.query_nodes(), classes(m.db), a["rocn"]).astype(_EVAL_DTYPE),)
    if kind == "eval_tables":
        return (eval_lib.expected_tables(w.matrix(sd)[0], w.n1s, m.query_nodes(), classes(m.db)),)
    if kind == "profile_rows":
        hits, joint = w.profile(sd, m.fit, w.pcut(sd, m.fit, a["frac"]), m.query_nodes())
        offset, words = profile_offsets(w.n1s, a["gaps"])
        packed = np.full(words, PROFILE_FILL, np.uint32)                          # words between the matrices are not written
        for q, j in enumerate(joint):
            packed[offset[q]:offset[q] + j.size] = j.ravel()
        return hits, packed
    if kind == "baseline_results":
        return w.matrix(m.baseline[0])[0], w.pvalues(*m.baseline)
    if kind == "reorder_hits":
        rows, mp = w.reorder(sd, m.fit, m.baseline, w.pcut(sd, m.fit, a["frac"]), w.base_cut(m.baseline, a["base_frac"]),
                             a["kinds"], a["k"])
        return _flat_rows(rows, mp if a["maps"] else None, [len(r) for r in rows])
    if kind == "search_reordered":                # the state it leaves, read back: scores and maps, the baseline, ranked rows
        after = _clone(m)
        after.apply(o)
        sc, mp = w.matrix(after.searched)
        out = () if m.multi else (sc, mp)
        return out + (w.matrix(after.baseline[0])[0], w.pvalues(*after.baseline), w.select(after.searched, after.fit).topk(3)[0])
    raise ValueError(kind)


PROFILE_FILL = 0xDEADBEEF


def profile_offsets(n1s, gaps):
    """(each query's first word, the words of the buffer) of a profile: packed, or with 5 + q words left free in front of
    query q's matrix"""
    offset, at = [], 0
    for q, n1 in enumerate(n1s):
        at += (5 + q) if gaps else 0
        offset.append(at)
        at += n1 * n1
    return np.array(offset, np.int64), at + (3 if gaps else 0)


def _added_edges(adds, cut=None):
    """(a, b): the edges of an accumulator's adds, each at its own cutoff (`cut`: a level's, for every add); a structure
    against itself is none"""
    ea, eb = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for dbname, bkey, asd, afit, frac, qnodes in adds:
        aw = world_ref(dbname, bkey)
        a, b = aw.edges(asd, afit, aw.pcut(asd, afit, frac, qnodes) if cut is None else cut, qnodes)
        ea.append(a)
        eb.append(b)
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    keep = ea != eb
    return ea[keep], eb[keep]


def _single_linkage(nodes, ea, eb):
    deg = (np.bincount(ea, minlength=nodes) + np.bincount(eb, minlength=nodes)).astype(np.int32)
    return select_lib.components(nodes, ea, eb), deg, np.array([len(ea)], np.int64)


def _state_key(o, m):
    cl = None if o.kind not in ("cluster_labels", "cluster_labels_levels") else (m.cluster[0], tuple(m.cluster[1]), m.cluster[2])
    cv = None if o.kind != "cover_solve" else (m.cover[0], tuple(m.cover[1]))
    return (o, m.multi and o.kind == "search_reordered", m.db, m.batch, m.searched, m.fit, m.tops, cl, cv, m.baseline)


def expect(o, m):
    """the arrays operation `o` must return on a context in state `m` (cached)"""
    return _memo(("expect", _state_key(o, m)), lambda: _expect(o, m))


# ---- run: the same tuple from the library
def _upload_dense(s, d):
    pitch = int(d.orders.max())
    tabs, dmats = np.zeros((len(d), pitch, pitch), np.uint8), np.zeros((len(d), pitch, pitch), np.float32)
    for e in range(len(d)):
        tabs[e], dmats[e] = d.dense(e, pitch)
    s.upload_dense(d.orders, tabs, dmats, pitch)


def _rows_of(s, m, got, maps):
    rows, mp = got if maps else (got, None)
    return _flat_rows(rows, mp, [len(r) for r in rows])


def run(s, o, m):
    """run operation `o` on searcher `s` (a Searcher, or a MultiSearcher when m.multi) whose state is `m`"""
    a, kind = dict(o.args), o.kind
    sd = m.searched
    if kind in ("upload", "upload_dense"):
        return s.upload(db(a["db"])) if kind == "upload" else _upload_dense(s, db(a["db"]))
    if kind == "set_query":
        return s.set_query(*batch(a["batch"])[0][0], FIRST["q1"])
    if kind == "set_queries":
        return s.set_queries(*batch(a["batch"]))
    if kind == "set_queries_from_db":
        return s.set_queries_from_db(db_indices(a["batch"][1]), FIRST["db"])
    if kind in ("set_polish_all", "polish_all_off"):
        return s.set_polish_all(a.get("tops", 0))
    if kind == "cluster_begin":
        return s.cluster_begin()
    if kind == "cluster_end":
        return s.cluster_end()
    if kind == "cluster_add":
        return s.cluster_add(m.world().pcut(sd, m.fit, a["frac"], m.query_nodes()), m.query_nodes())
    if kind == "cluster_labels":
        labels, deg, edges = s.cluster_labels()
        return labels, deg, np.array([edges], np.int64)
    if kind == "set_queries_motif":
        return s.set_queries_from_db(db_indices(a["batch"][1]), FIRST["motif"], sses=motif_lists(a["batch"][1]))
    if kind == "cluster_begin_levels":
        return s.cluster_begin_levels(level_cuts(m.db, a["levels"]))
    if kind == "cluster_add_levels":
        return s.cluster_add_levels(m.query_nodes())
    if kind in ("cover_begin", "cover_end", "baseline_keep", "baseline_drop", "cluster_labels_levels", "baseline_results"):
        return getattr(s, kind)()
    if kind == "cover_add":
        return s.cover_add(m.world().pcut(sd, m.fit, a["frac"], m.query_nodes()), m.query_nodes())
    if kind in ("set_eval_classes", "eval_classes_off"):
        return s.set_eval_classes(classes(m.db) if kind == "set_eval_classes" else None)
    if kind == "cover_solve":
        rep, deg, edges, rounds = s.cover_solve()
        return rep, deg, np.array([edges, rounds], np.int64)
    if kind == "eval_rows":
        return (s.eval_rows(m.query_nodes(), a["rocn"]),)
    if kind == "eval_tables":
        return (np.concatenate([t.ravel() for t in s.eval_tables(m.query_nodes())]),)
    if kind == "profile_rows":
        n1s = n1s_of(m.batch)
        offset, words = profile_offsets(n1s, a["gaps"])
        hits, joint = np.zeros(len(n1s), np.uint32), np.full(words, PROFILE_FILL, np.uint32)
        s.profile_rows_raw(m.world().pcut(sd, m.fit, a["frac"]), m.query_nodes(), hits, joint, offset if a["gaps"] else None)
        return hits, joint
    if kind == "reorder_hits":
        w = m.world()
        got = s.reorder_hits(w.pcut(sd, m.fit, a["frac"]), w.base_cut(m.baseline, a["base_frac"]), a["kinds"], a["k"], a["maps"])
        return _rows_of(s, m, got, a["maps"])
    if kind == "search_reordered":
        s.search_reordered(a["r"], a["censor"])
        w = m.world()
        if m.multi:
            return s.baseline_results() + (np.stack([r[:3] for r in s.hits_cutoff(1.0, 3)]),)
        sc, mp = s.results(True)
        return (sc.reshape(w.nq, w.n), mp.reshape(w.nq, w.n, MAXDIM)) + s.baseline_results() + (s.topk_hits(3),)
    w = world_ref(a["db"], m.batch) if kind == "upload_search" else m.world()
    shape = (w.nq, w.n)
    if kind in ("search", "search_async_results", "upload_search", "results"):
        if kind == "search":
            sc, mp = s.search(a["lorder"], a["lsoln"], a["r"])[:2]
        else:
            if kind == "search_async_results":
                s.search_async(a["lorder"], a["lsoln"], a["r"])
            elif kind == "upload_search":
                s.upload_search(db(a["db"]), a["lorder"], a["lsoln"], a["r"])
            sc, mp = s.results(a["lsoln"])
        return (sc.reshape(shape),) if mp is None else (sc.reshape(shape), mp.reshape(shape + (MAXDIM,)))
    if kind == "results_base":
        return (s.results_base().reshape(shape),)
    if kind == "search_matches":
        c, sc, rs, mp = s.search_matches(a["m"], a["lorder"], a["r"], a["maps"])[:4]
        flat = (c.ravel(), sc.reshape(-1, a["m"]), rs.reshape(-1, a["m"]))
        return flat + ((mp.reshape(-1, a["m"], w.n1max),) if a["maps"] else ())
    if kind == "search_pairs":
        sc, mp = s.search_pairs(*w.pairs(a["pairs"]), a["lorder"], a["lsoln"], a["r"])
        return (sc, mp) if a["lsoln"] else (sc,)
    if kind == "search_pairs_matches":
        got = s.search_pairs_matches(*w.pairs(a["pairs"]), a["m"], a["lorder"], a["r"], a["maps"])
        return got[:4] if a["maps"] else got[:3]
    if kind == "search_pairs_polish":
        return s.search_pairs_polish(*w.pairs(a["pairs"]), a["tops"], a["lorder"], a["r"])[:5]
    if kind == "search_refine":
        hits, mp, first = s.search_refine(a["k"], a["cand"], a["big_r"], a["lorder"], a["lsoln"], a["r"])
        return (hits, first) + ((mp,) if a["lsoln"] else ())
    if kind == "search_refine_polish":
        hits, mp, first, base = s.search_refine_polish(a["k"], a["cand"], a["big_r"], a["tops"], a["lorder"], a["lsoln"], a["r"])
        return (hits, first, base) + ((mp,) if a["lsoln"] else ())
    if kind == "topk_hits":
        if m.multi:
            rows, mp = s.search_topk(a["k"], sd.lorder, sd.lsoln, sd.r)[:2]
            return (rows, mp) if a["maps"] else (rows,)
        got = s.topk_hits(a["k"], a["maps"])
        return got if a["maps"] else (got,)
    if kind == "hits_cutoff":
        return _rows_of(s, m, s.hits_cutoff(w.pcut(sd, m.fit, a["frac"]), a["k"], a["maps"]), a["maps"])
    if kind == "score_histogram":
        return s.score_histogram()
    if kind == "fit_statistics":
        fit = ("fit", a["censor"])
        fits = s.search_fit(a["censor"], sd.lorder, sd.lsoln, sd.r)[0] if m.multi else s.fit_statistics(a["censor"])
        return (fits,) + _rows_of(s, m, s.hits_cutoff(w.pcut(sd, fit, 0.5)), False)
    if kind == "set_statistics":
        s.set_statistics(None if a["fit"] == "none" else w.fits(sd, ("set", a["fit"])))
        if m.multi:
            return (np.stack([r[:3] for r in s.hits_cutoff(1.0, 3)]),)
        return (s.topk_hits(3),)
    raise ValueError(kind)


def same(got, want):
    """the first difference between two tuples of arrays as text, or None: exact, byte for byte"""
    if len(got) != len(want):
        return "%d arrays, the reference has %d" % (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape or g.dtype != w.dtype:
            return "array %d is %s %s, the reference %s %s" % (i, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            flat_g, flat_w = g.reshape(-1), w.reshape(-1)
            bad = [k for k in range(len(flat_g)) if flat_g[k].tobytes() != flat_w[k].tobytes()]
            return "array %d differs at %d of %d places, first flat index %d: got %s, the reference %s" % (
                i, len(bad), len(flat_g), bad[0], flat_g[bad[0]], flat_w[bad[0]])
    return None


# ---------------------------------------------------------------- drawing an operation's parameters
def _pick(rng, values, avoid=None):
    values = [v for v in values if v != avoid] or list(values)
    return values[int(rng.integers(len(values)))]


def draw(kind, m, rng, size=None, last=None):
    """operation of `kind` with parameters legal in state `m`; size "lo" / "hi" asks for the smallest / largest counts,
    `last` ({name: count}, updated) for counts that differ from the ones used before"""
    def count(name):
        c = COUNTS[name]
        v = c[0] if size == "lo" else c[-1] if size == "hi" else _pick(rng, c, (last or {}).get(name))
        if last is not None:
            last[name] = v
        return v

    def restarts():
        return rmax_of(m.db) if size == "hi" else 1 if size == "lo" else _pick(rng, (1, 3, rmax_of(m.db)))

    flag = lambda: bool(rng.integers(2))
    combos = NEW_COMBOS if m.new else COMBOS                                      # the new schedule has one more database
    if kind in ("upload", "upload_dense", "upload_search"):
        fits = [d for d in combos if m.batch is None or (m.batch in combos[d] if isinstance(m.batch, str) else m.batch[1] == d)]
        if kind == "upload_dense":
            fits = [d for d in fits if d not in ("d150", "d1100")]
        if m.tops:
            fits = [d for d in fits if d not in BIG]
        name = _pick(rng, fits, m.db)
        if kind != "upload_search":
            return op(kind, db=name)
        return op(kind, db=name, lorder=flag(), lsoln=flag(), r=_pick(rng, (1, 3, rmax_of(name))))
    if kind == "set_query":
        return op(kind, batch="q1") if m.db is None or "q1" in combos[m.db] else None
    if kind == "set_queries":
        fits = [b for b in ("q5", "q2", "q4") if m.db is None or b in combos[m.db]]
        return op(kind, batch=_pick(rng, fits, m.batch))
    if kind == "set_queries_from_db":
        return op(kind, batch=("db", m.db)) if "db" in combos[m.db] else None
    if kind in ("set_polish_all", "search_matches") and m.db in BIG:
        return None
    if kind == "set_polish_all":
        return op(kind, tops=count("tops"))
    if kind in ("polish_all_off", "cluster_begin", "cluster_end", "cluster_labels", "score_histogram", "results_base"):
        return op(kind)
    if kind == "cluster_add":
        return op(kind, frac=_pick(rng, (0.1, 0.4)))
    if kind in ("search", "search_async_results"):
        return op(kind, lorder=flag(), lsoln=flag(), r=restarts())
    if kind == "search_matches":
        return op(kind, lorder=flag(), r=restarts(), m=count("m"), maps=flag())
    if kind == "search_pairs":
        return op(kind, lorder=flag(), r=restarts(), pairs=count("pairs"), lsoln=flag())
    if kind == "search_pairs_matches":
        return op(kind, lorder=flag(), r=restarts(), pairs=count("pairs"), m=count("m"), maps=flag())
    if kind == "search_pairs_polish":
        return op(kind, lorder=flag(), r=restarts(), pairs=count("pairs"), tops=count("tops"))
    if kind in ("search_refine", "search_refine_polish"):
        more = {"tops": count("tops")} if kind == "search_refine_polish" else {}
        return op(kind, lorder=flag(), r=_pick(rng, (1, 3)), big_r=rmax_of(m.db), cand=count("cand"), k=min(count("k"), 4),
                  lsoln=flag(), **more)
    if kind == "results":
        return op(kind, lsoln=m.searched.lsoln and flag())
    if kind == "topk_hits":
        return op(kind, k=count("k"), maps=m.searched.lsoln and flag())
    if kind == "hits_cutoff":
        return op(kind, frac=_pick(rng, (0.15, 0.6)), k=count("k") if size else _pick(rng, (None, 2)), maps=m.searched.lsoln and flag())
    if kind == "fit_statistics":
        return op(kind, censor=_pick(rng, (0.0, 0.1)))
    if kind == "set_statistics":
        return op(kind, fit=_pick(rng, ("ab", "none")))
    if kind == "set_queries_motif":
        return op(kind, batch=("motif", m.db)) if "motif" in combos[m.db] else None
    if kind == "cluster_begin_levels":
        return op(kind, levels=MAX_LEVELS if size == "hi" else 1 if size == "lo" else _pick(rng, (1, 3, MAX_LEVELS)))
    if kind in ("cluster_add_levels", "cover_begin", "cover_end", "set_eval_classes", "eval_classes_off", "baseline_keep",
                "baseline_drop", "cluster_labels_levels", "cover_solve", "eval_tables", "baseline_results"):
        return op(kind)
    if kind == "cover_add":
        return op(kind, frac=_pick(rng, (0.1, 0.4)))
    if kind == "eval_rows":
        return op(kind, rocn=_pick(rng, (1, 3, 50)))
    if kind == "profile_rows":
        return op(kind, frac=_pick(rng, (0.15, 0.6)), gaps=flag())
    if kind == "reorder_hits":
        return op(kind, frac=_pick(rng, (0.3, 0.8)), base_frac=_pick(rng, (None, 0.5)), kinds=_pick(rng, (7, 6, 2, 5)),
                  k=count("k") if size else _pick(rng, (None, 2)), maps=flag())
    if kind == "search_reordered":
        return op(kind, r=restarts(), censor=_pick(rng, (None, 0.0, 0.1)))
    raise ValueError(kind)


# ---------------------------------------------------------------- which pairs of kinds the model allows
def _successors(m, kinds):
    """(kind, state after a representative operation of it) for every kind legal in `m`: legality depends on the flags
    only, and of an operation's parameters only lsoln moves a flag"""
    for kind in kinds:
        if m.legal(kind):
            for lsoln in ((False, True) if kind in ("search", "search_async_results", "upload_search") else (False,)):
                nxt = _clone(m)
                nxt.apply(_representative(kind, lsoln))
                yield kind, nxt


def kinds_of(multi=False, new=False):
    """the kinds a schedule walks: the 27 (19 on shards) of the first schedule, or those and the new ones"""
    if new:
        return MULTI_KINDS if multi else ALL_KINDS
    return OLD_MULTI_KINDS if multi else KINDS


def allowed_pairs(multi=False, new=False):
    """every (A, B): B is legal in some reachable state right after A, found by walking the model over its flags; new: over
    the kinds of kinds_of(multi, True), and of those pairs the ones with a new kind in them"""
    def make():
        kinds = kinds_of(multi, new)
        start = Model(multi, new)
        seen, todo, pairs = {start.flags()}, [start], set()
        while todo:
            for kind, nxt in _successors(todo.pop(), kinds):
                pairs.update((kind, b) for b in kinds if nxt.legal(b))
                if nxt.flags() not in seen:
                    seen.add(nxt.flags())
                    todo.append(nxt)
        return frozenset(p for p in pairs if not new or p[0] in NEW_KINDS or p[1] in NEW_KINDS)
    return _memo(("allowed", multi, new), make)


def _route(m, last, todo, kinds):
    """the first kind of a shortest run of operations from state `m` that ends in a pair of `todo`, or None"""
    if m.new:
        return _route_by_flags(m, last, todo, kinds)
    seen, level = {(last, m.flags())}, [(None, last, m)]
    while level:
        nxt_level = []
        for first, prev, state in level:
            for kind, nxt in _successors(state, kinds):
                if (prev, kind) in todo:
                    return first or kind
                if (kind, nxt.flags()) not in seen:
                    seen.add((kind, nxt.flags()))
                    nxt_level.append((first or kind, kind, nxt))
        level = nxt_level
    return None


def _route_by_flags(m, last, todo, kinds):
    """_route for the second schedule, whose states are many more: the same search over sets of flags, each expanded once
    (what is legal and the flags that follow depend on the flags only)"""
    def successors(flags, state):
        return _memo(("successors", m.multi, flags), lambda: [(kind, nxt, nxt.flags()) for kind, nxt in _successors(state, kinds)])

    seen, level = {(last, m.flags())}, [(None, last, m, m.flags())]
    while level:
        nxt_level = []
        for first, prev, state, flags in level:
            for kind, nxt, nxt_flags in successors(flags, state):
                if (prev, kind) in todo:
                    return first or kind
                if (kind, nxt_flags) not in seen:
                    seen.add((kind, nxt_flags))
                    nxt_level.append((first or kind, kind, nxt, nxt_flags))
        level = nxt_level
    return None


def _clone(m):
    c = Model(m.multi, m.new)
    c.db, c.batch, c.searched, c.fit, c.tops = m.db, m.batch, m.searched, m.fit, m.tops
    c.cluster = None if m.cluster is None else [m.cluster[0], list(m.cluster[1]), m.cluster[2]]
    c.cover = None if m.cover is None else [m.cover[0], list(m.cover[1])]
    c.classes, c.baseline = m.classes, m.baseline
    return c


def _representative(kind, lsoln):
    return op(kind, db="d16", batch="q1", lorder=True, lsoln=lsoln, r=1, tops=3, censor=0.0, fit="ab", frac=0.1, levels=1)


# ---------------------------------------------------------------- schedules
def schedule(seed, multi=False, new=False):
    """walks (lists of operations, each for a fresh context) that between them follow every allowed pair of kinds; new: the
    second schedule, over old and new kinds and NEW_COMBOS, for the pairs with a new kind in them"""
    def make():
        rng = np.random.default_rng(seed)
        kinds = kinds_of(multi, new)
        todo = set(allowed_pairs(multi, new))
        walks = []
        while todo:
            before = len(todo)
            m, walk, last, counts = Model(multi, new), [], None, {}
            while len(walk) < WALK_STEPS:
                cands = [k for k in kinds if m.legal(k)]
                # a pair not yet followed - of those the kind with the most unfollowed pairs behind it; else toward one
                fresh = [k for k in cands if (last, k) in todo]
                weight = [sum(1 for p in todo if p[0] == k) for k in fresh]
                best = [k for k, x in zip(fresh, weight) if x == max(weight)]
                toward = [] if fresh else [_route(m, last, todo, kinds)]
                o = None
                for kind in rng.permutation(best).tolist() + rng.permutation(fresh).tolist() + toward + rng.permutation(cands).tolist():
                    o = draw(kind, m, rng, None, counts) if kind else None
                    if o is not None:
                        break
                todo.discard((last, o.kind))
                walk.append(o)
                m.apply(o)
                last = o.kind
            walks.append(walk)
            if len(todo) == before:
                raise AssertionError("the cover does not advance: %s" % sorted(todo)[:5])
        return walks + ([_named_walk(multi), _sizes_walk(multi)] if new else [_nodes_walk(multi)])
    return _memo(("schedule", seed, multi) + ((new,) if new else ()), make)


def _set_batch(dbname, b):
    if b == "q1":
        return op("set_query", batch=b)
    return op("set_queries_from_db", batch=("db", dbname)) if b == "db" else op("set_queries", batch=b)


def _named_walk(multi):
    """the sequences tests/test_history_cpu.py names, on the permutant world: a baseline kept across a search; a baseline
    kept under a polished search with the polish then off; a begin of each accumulator kind over the live other; a cover
    and a leveled add from one search; the evaluation and the profile behind a pair search; a motif batch"""
    pair = op("search_pairs_matches", lorder=True, r=3, pairs=7, m=3, maps=True)
    ops = [op("upload", db="dperm"), op("set_queries", batch="q4"), op("set_eval_classes"),
           op("search_reordered", r=16, censor=0.0), op("search", lorder=False, lsoln=True, r=3),
           op("reorder_hits", frac=0.8, base_frac=None, kinds=7, k=None, maps=True),
           op("cluster_begin"), op("cluster_add", frac=0.4), op("cluster_begin_levels", levels=3), op("cover_begin"),
           op("cluster_add_levels"), op("cover_add", frac=0.4), op("cluster_labels_levels"), op("cover_solve"),
           op("cluster_begin"), op("cluster_add", frac=0.1), op("cluster_labels"),
           pair, op("eval_rows", rocn=3), pair, op("profile_rows", frac=0.6, gaps=True),
           op("set_polish_all", tops=3), op("search", lorder=True, lsoln=False, r=3), op("baseline_keep"), op("polish_all_off"),
           op("search", lorder=False, lsoln=True, r=3), op("reorder_hits", frac=0.8, base_frac=0.5, kinds=6, k=2, maps=False),
           op("baseline_results"), op("set_queries_motif", batch=("motif", "dperm")), op("search_reordered", r=16, censor=None),
           op("reorder_hits", frac=0.8, base_frac=0.5, kinds=7, k=None, maps=True), op("profile_rows", frac=0.6, gaps=False),
           op("set_queries_from_db", batch=("db", "dperm")), op("search", lorder=False, lsoln=True, r=16), op("eval_rows", rocn=1),
           op("cover_begin"), op("cover_add", frac=0.4), op("cover_solve"), op("cluster_begin"), op("cluster_add", frac=0.4),
           op("cluster_labels")]
    return ops + ([] if multi else [op("eval_tables"), op("cover_end"), op("cluster_end")])


def _sizes_walk(multi):
    """every new data kind at 25, 200 and 25 rows on one context: behind a smaller batch, and behind a larger one"""
    ops = []
    for dbname, b, r in (("d16", "db", 3), ("d32", "q5", 3), ("d16", "db", 100)):
        ops += [op("upload", db=dbname), _set_batch(dbname, b), op("set_eval_classes"), op("search_reordered", r=r, censor=0.1),
                op("cluster_begin_levels", levels=MAX_LEVELS), op("cluster_add_levels"), op("cover_begin"), op("cover_add", frac=0.4)]
        data = [op("cluster_labels_levels"), op("cover_solve"), op("eval_rows", rocn=3), op("eval_tables"),
                op("profile_rows", frac=0.6, gaps=r > 3), op("baseline_results"),
                op("reorder_hits", frac=0.8, base_frac=None, kinds=7, k=None, maps=True)]
        ops += [o for o in data if not multi or o.kind in MULTI_KINDS]
    return ops


def _nodes_walk(multi):
    """the accumulator over 40, 5, 18, 5 and 12 nodes on one context, each filled from two query batches: the greedy
    walks begin too few accumulators to move the node count up and down twice"""
    ops = []
    for dbname, first, second in (("d32", "q5", "db"), ("d16", "db", "q5"), ("d48", "q2", "db"), ("d16", "q1", "db"),
                                  ("d111", "q5", "q5")):
        if multi:
            first, second = ("q5" if b == "q1" else b for b in (first, second))
        ops += [op("upload", db=dbname), _set_batch(dbname, first), op("search", lorder=True, lsoln=False, r=3), op("cluster_begin"),
                op("cluster_add", frac=0.4), _set_batch(dbname, second), op("search", lorder=False, lsoln=False, r=rmax_of(dbname)),
                op("cluster_add", frac=0.1), op("cluster_labels")]
    return ops


def grow_shrink_grow(kind, multi=False):
    """scenario 1: `kind` at its largest world and counts, another family at the smallest world, `kind` at its smallest
    world and counts, then at the largest again - with whatever the model needs in front of each"""
    rng = np.random.default_rng(len(kind))
    other = "search_matches" if "polish" in kind or kind == "results_base" else "search_pairs_polish"
    ops, m = [], Model(multi)

    def add(o):
        ops.append(o)
        m.apply(o)

    def goto(world, size, target):
        dbname, b = world
        if multi and b == "q1":
            b = "q2" if dbname != "d16" else "db"
        if target == "results_base":
            add(op("set_polish_all", tops=COUNTS["tops"][0 if size == "lo" else -1]))
        elif m.tops:
            add(op("polish_all_off"))
        if target != "upload_search":
            add(op("upload", db=dbname))
        add(_set_batch(dbname, b))
        if target in RESULTS or target == "cluster_labels" or target in NEW_DATA[:-1]:
            add(op("search", lorder=True, lsoln=True, r=rmax_of(dbname) if size == "hi" else 3))
        if target == "cluster_labels":
            add(op("cluster_begin"))
            add(op("cluster_add", frac=0.4))
        if target == "cluster_labels_levels":
            add(op("cluster_begin_levels", levels=MAX_LEVELS if size == "hi" else 1))
            add(op("cluster_add_levels"))
        if target == "cover_solve":
            add(op("cover_begin"))
            add(op("cover_add", frac=0.4))
        if target in ("eval_rows", "eval_tables"):
            add(op("set_eval_classes"))
        if target in ("baseline_results", "reorder_hits"):
            add(op("baseline_keep"))
        if target == "reorder_hits":                                              # the unordered search over the ordered baseline
            add(op("search", lorder=False, lsoln=True, r=rmax_of(dbname) if size == "hi" else 3))

    largest = None
    for world, size, what in ((LARGEST, "hi", kind), (SMALLEST, "lo", other), (SMALLEST, "lo", kind), (LARGEST, "hi", kind)):
        goto(world, size, what)
        if what == "upload_search":
            add(op(what, db=world[0], lorder=True, lsoln=size == "hi", r=rmax_of(world[0]) if size == "hi" else 1))
        else:
            add(largest if size == "hi" and largest else draw(what, m, rng, size))
        largest = largest or ops[-1]
    return ops


def shard_sequence():
    """150 -> 12 -> 40 -> 5 -> 150 entries under one two-query batch: sat_multi's padded rows and the per-shard floors go
    up and down while the gathers' buffers only grow"""
    return [op("upload", db="d150"), op("set_queries", batch="q2"), op("search", lorder=True, lsoln=True, r=16),
            op("topk_hits", k=10, maps=True), op("search_matches", lorder=True, r=3, m=3, maps=True),
            op("upload", db="d111"), op("search", lorder=False, lsoln=True, r=3), op("topk_hits", k=3, maps=True),
            op("search_pairs_polish", lorder=True, r=16, pairs=7, tops=3),
            op("upload", db="d32"), op("search_matches", lorder=False, r=64, m=8, maps=True),
            op("search", lorder=True, lsoln=True, r=64), op("hits_cutoff", frac=0.6, k=None, maps=True), op("score_histogram"),
            op("upload", db="d16"), op("search", lorder=True, lsoln=True, r=100), op("fit_statistics", censor=0.0),
            op("upload", db="d150"), op("search", lorder=True, lsoln=True, r=1), op("topk_hits", k=3, maps=True),
            op("search_refine", lorder=True, r=1, big_r=16, cand=12, k=3, lsoln=True)]


def dimensions(o, m):
    """the sizes operation `o` works at in state `m` (after it): for the rise-and-fall conditions"""
    a, out = dict(o.args), {}
    if m.db is not None:
        d = db(m.db)
        out["entries"], out["n2"] = len(d), int(d.orders.max())
    if m.batch is not None:
        n1s = n1s_of(m.batch)
        out["queries"], out["n1"] = len(n1s), max(n1s)
    for name in ("pairs", "m", "tops", "k"):
        if name in a and a[name] is not None:
            out[name] = a[name]
    if o.kind == "cluster_begin":
        out["nodes"] = m.cluster[0]
    return out


def rises_and_falls(walk, multi=False):
    """{dimension: (rises, falls)} along one walk"""
    m, last, out = Model(multi), {}, collections.defaultdict(lambda: [0, 0])
    for o in walk:
        m.apply(o)
        for name, v in dimensions(o, m).items():
            if name in last and v != last[name]:
                out[name][0 if v > last[name] else 1] += 1
            last[name] = v
    return {k: tuple(v) for k, v in out.items()}


# ---------------------------------------------------------------- the walks of tests/test_gpu_caller_stream.py
def caller_stream_walks(first=4, second=4):
    """the walks that run once more on every kind of caller's stream, as (name, operations): `first` greedy walks of the
    first schedule and `second` of the second one, chosen - most kinds not yet seen first, the lower index among equals -
    so that with the two hand-made walks of the second schedule every kind of ALL_KINDS occurs
    (tests/test_history_cpu.py asserts it)"""
    def make():
        old, new = schedule(SEED)[:-1], schedule(SEED, False, True)[:-2]              # (the greedy ones)
        hand = schedule(SEED, False, True)[-2:]
        seen = {o.kind for w in hand for o in w}
        out = []
        for name, walks, count in (("walk", old, first), ("new_walk", new, second)):
            taken = []
            for _ in range(count):
                gain = [-1 if i in taken else len({o.kind for o in w} - seen) for i, w in enumerate(walks)]
                i = int(np.argmax(gain))
                taken.append(i)
                seen |= {o.kind for o in walks[i]}
            out += [("%s%d" % (name, i), walks[i]) for i in sorted(taken)]
        return out + [("named", hand[0]), ("sizes", hand[1])]
    return _memo(("caller_stream_walks", first, second), make)
