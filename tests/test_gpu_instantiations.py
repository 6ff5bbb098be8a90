"""Every instantiation of the SA kernel against the CPU reference, by name (-m gpu).

The SA kernel is compiled 328 times (sat_debug_sa_instances lists them: 200 plain, 32 match, 64 pair, 32 pair-match);
pick_sa_kernel (sat_launch.hip) chooses among them at run time.  For every one of them this module holds a RECIPE - an API
call, a query batch, a database, LORDER / LSOLN and SAT_EXP_* overrides - that makes the default host path launch exactly
that kernel, and asserts (a) that sat_last_launch_info() names it for the pass in question and (b) that the results are
the CPU reference's bit for bit.  The expected name of a recipe is worked out HERE from the recipe (the rules of
prepare_sa / pick_sa_kernel written down once more, below), never read from the enumeration: a dispatcher that picks
another kernel than the rules promise fails (a), whatever it computes.

How a recipe steers each template argument (sat_launch.hip, sat_capi.hip, sat_pairs.hip, sat_db.hip):
  family   the API call: search / search_matches / search_pairs / search_pairs_matches.
  N1P      the query order: <= 16, <= 32, <= 64, above (sat_queries_set).
  M2W, CELLS   entries x queries of a class <= 4096 go out as ONE launch laid out for the database's largest entry
           (launch_search); the pair families launch per order bucket of the listed entries (build_pair_items).  Four
           databases with largest orders 32 / 48 / 64 / 111 give <1, FULL8>, <2, FULL5>, <2, TRI5>, <4, TRI5>.
  WPL      satk::compaction_shape of the query orders: one value for the whole batch, or 0 when they differ.
  OPT      bit 0 LORDER, bit 1 LSOLN, bits 2-3 SAT_EXP_LPC (1, 2: four-word sets only); SAT_EXP_LPC=0 for the one-lane
           specialisations; -1 under SAT_EXP_GENERAL=1, under a non-default QLDS, with several lanes per chain on
           narrower sets, in the match families and in the pair family's map pass.
  QLDS     the 16 class keeps its query cells in LDS, the others in L1/L2 unless SAT_EXP_QLDS=1.

Every case runs maxstart = 100 (no multiple of 64: the second wave of chains is partly empty) on a batch of one planted
and one foreign query (dense and sparse maps).  The CPU references are computed once per (query, database, LORDER) and
shared by the recipes of all families: oracle_lib.search for search and search_pairs, matches_lib.matches for the two
match families.

The closing test checks that the recipes' names and the UNREACHABLE list together are exactly the enumerated list.
Two more cases run the DEFAULT launch plan (no override) at small shapes: a search cut into one launch per order bucket
and class on side streams, and a launch large enough for pick_epw to choose the entries per workgroup."""
import os
import re

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import matches_lib
import oracle_lib

pytestmark = pytest.mark.gpu

MAXSTART = 100
MAX_MATCHES = 3
FULL8, FULL5, TRI5 = 0, 1, 2
KERNEL = {"plain": "sat_sa_kernel", "match": "sat_sa_match_kernel", "pair": "sat_sa_pair_kernel",
          "pair_match": "sat_sa_pair_match_kernel"}
BUCKET_MAX = (16, 32, 48, 64, 80, 96, 111)             # kBucketMax


# ---------------------------------------------------------------- the host's rules, written down once more
def class_of(n1):
    return 16 if n1 <= 16 else 32 if n1 <= 32 else 64 if n1 <= 64 else 112


def wpl_of(n1):
    """satk::compaction_shape: map words per lane of a query of n1 SSEs"""
    n1w = (n1 + 3) // 4
    lpi = (n1w + 3) // 4
    return -(-n1w // lpi)


def layout_of(n2max):
    """(satk::set_words, satk::cell_layout) of a launch whose largest entry has n2max SSEs"""
    return (1, FULL8) if n2max <= 32 else (2, FULL5) if n2max <= 48 else (2, TRI5) if n2max <= 64 else (4, TRI5)


def bucket_of(n2):
    return next(b for b, top in enumerate(BUCKET_MAX) if n2 <= top)


def kernel_name(family, n1p, m2w, qlds, cells, opt=-1, wpl=0):
    targs = {"plain": f"{opt}, {wpl}, ", "pair": f"{opt}, "}.get(family, "")
    return f"{KERNEL[family]}<{n1p}, {m2w}, {'true' if qlds else 'false'}, {targs}{cells}>"


def names_in(info):
    return re.findall(r"sat_sa_[a-z_]*kernel<[^>]*>", info)


# ---------------------------------------------------------------- data: four databases, two queries per round shape
# Entry k of every database is the leading block of pool structure k, so a query planted in pool structure k has a
# dense match in entry k of all four.  Both edges of each range, and an order-1 and an order-2 entry; not sorted.
DB_ORDERS = {
    32: [1, 2, 3, 7, 11, 15, 16, 17, 19, 23, 27, 30, 31, 32, 32, 5, 13, 29],
    48: [33, 34, 35, 37, 39, 41, 43, 45, 47, 48, 48, 40, 36, 44, 1, 20, 33, 46],
    64: [49, 50, 51, 53, 55, 57, 59, 61, 63, 64, 64, 56, 2, 30, 49, 60, 52, 62],
    111: [65, 66, 70, 75, 80, 81, 88, 96, 97, 100, 105, 110, 111, 111, 1, 24, 40, 60, 72, 104],
}
POOL = 24
# (planted order, foreign order) per words-per-lane value of a class; both queries of a batch have that value
BATCHES = {
    16: {1: (4, 3), 2: (8, 5), 3: (12, 9), 4: (16, 13)},
    32: {3: (24, 17), 4: (32, 25)},
    64: {3: (36, 33), 4: (64, 37)},
    112: {4: (111, 65)},
}
# a batch of two different values: the planted query of the first, the foreign query of the last
MIXED = {16: (4, 13), 32: (24, 25), 64: (36, 37)}

for _c, _b in BATCHES.items():
    for _w, _orders in _b.items():
        assert all(class_of(n) == _c and wpl_of(n) == _w for n in _orders)


def batch_orders(n1p, wpl):
    """(planted order, foreign order) of the class's batch with `wpl` words per lane; wpl = 0: the mixed batch"""
    return MIXED[n1p] if wpl == 0 else BATCHES[n1p][wpl]


class Data:
    """The databases, the queries and the shared references."""

    def __init__(self):
        pool = sat.synth.make_db(POOL, 111, 111, seed=4242)
        tabs, dists = [], []
        rng = np.random.default_rng(99)
        for k in range(POOL):
            t, d = pool.dense(k)
            if k % 2 == 0:                          # distances on a 0.5 A grid: exact 4.0 A differences can occur
                types = np.diagonal(d).copy()
                d = (np.round(d * 2) / 2).astype(np.float32)
                d[np.arange(111), np.arange(111)] = types
            for _ in range(12):                     # '?' codes, also inside the leading blocks
                i, j = sorted(rng.choice(111 if _ < 6 else 30, 2, replace=False))
                t[i, j] = t[j, i] = 0x44
            tabs.append(t)
            dists.append(d)
        self.pool = (tabs, dists)
        self.db = {top: sat.StructSet.from_dense(orders, tabs[:len(orders)], dists[:len(orders)])
                   for top, orders in DB_ORDERS.items()}
        self._queries = {}
        self._plain = {}
        self._matches = {}

    def query(self, n1, planted):
        """The planted or the foreign query of n1 SSEs.  Planted: n1 of the first SSEs of an even pool structure (0.5 A
        grid), its distances moved by 0, +-0.5 or +-4.0 A exactly."""
        key = (n1, planted)
        if key not in self._queries:
            if planted:
                rng = np.random.default_rng(500 + n1)
                src = 2 * (n1 % 7)                                     # entries 0, 2, .., 12 of every database
                t, d = self.pool[0][src], self.pool[1][src]
                sel = np.sort(rng.choice(min(111, n1 + n1 // 3 + 1), size=n1, replace=False))
                t, d = t[np.ix_(sel, sel)].copy(), d[np.ix_(sel, sel)].copy()
                noise = rng.choice(np.array([0, 0, 0, 0.5, -0.5, 4.0, -4.0], np.float32), size=(n1, n1))
                noise = np.tril(noise, -1)
                types = np.diagonal(t).copy()
                d = np.abs(d + noise + noise.T).astype(np.float32)
                d[np.arange(n1), np.arange(n1)] = types.astype(np.float32)
                self._queries[key] = (t, d, types)
            else:
                self._queries[key] = sat.synth.make_query(n1, seed=1000 + n1)
        return self._queries[key]

    def batch(self, orders):
        """[planted query, foreign query] of the two orders; set with first ordinal 0, so the planted query always
        draws from the streams of ordinal 0 and the foreign one from those of ordinal 1"""
        return [self.query(orders[0], True), self.query(orders[1], False)]

    def plain(self, top, n1, planted, lorder):
        """oracle_lib.search of one query over database `top`: (scores, maps)"""
        key = (top, n1, planted, lorder)
        if key not in self._plain:
            qt, qd, qty = self.query(n1, planted)
            sc, mp, _ = oracle_lib.search(self.db[top], qt, qd, qty, lorder, True, MAXSTART, query_ordinal=0 if planted else 1)
            self._plain[key] = (sc, mp)
        return self._plain[key]

    def matches(self, top, n1, planted, lorder):
        """matches_lib.matches of one query for every entry of database `top`: (counts, scores, restarts, maps)"""
        key = (top, n1, planted, lorder)
        if key not in self._matches:
            db = self.db[top]
            rows = [matches_lib.matches(db, e, self.query(n1, planted), lorder, MAXSTART, MAX_MATCHES, 0 if planted else 1)
                    for e in range(len(db))]
            self._matches[key] = tuple(np.array([r[k] for r in rows]) for k in range(4))
        return self._matches[key]


@pytest.fixture(scope="module")
def data():
    return Data()


# ---------------------------------------------------------------- the recipes
# override sets (read when a context is created: one context per test serves all its steps)
LPC0, LPC1, LPC2 = {"SAT_EXP_LPC": "0"}, {"SAT_EXP_LPC": "1"}, {"SAT_EXP_LPC": "2"}
GENERAL, QLDS, DEFAULT = {"SAT_EXP_GENERAL": "1"}, {"SAT_EXP_QLDS": "1"}, {}
OVERRIDES = {"lpc0": LPC0, "lpc1": LPC1, "lpc2": LPC2, "general": GENERAL, "qlds": QLDS, "default": DEFAULT}


def plain_name(n1p, ov, top, wpl_batch, lorder, lsoln):
    """prepare_sa + pick_sa_kernel for one launch of the plain family over database `top`"""
    m2w, cells = layout_of(top)
    kq = n1p < 32
    bits = int(lorder) | int(lsoln) << 1
    if ov == "general":
        return kernel_name("plain", n1p, m2w, kq, cells)
    if ov == "qlds":                                # the specialisations exist for the default placement only
        return kernel_name("plain", n1p, m2w, True, cells)
    if ov == "lpc0":                                # compaction exactly when LORDER: only then WPL matters
        return kernel_name("plain", n1p, m2w, kq, cells, bits, wpl_batch if lorder else 0)
    lanes = {"lpc1": 1, "lpc2": 2}[ov]
    if m2w == 4:                                    # several lanes per chain are specialised for four-word sets
        return kernel_name("plain", n1p, 4, kq, TRI5, bits | lanes << 2, 0)
    return kernel_name("plain", n1p, m2w, kq, cells)


def plain_steps(n1p, ov):
    """(database, batch wpl, lorder, lsoln) of every search of the plain recipe (class, override set)"""
    wpls = sorted(BATCHES[n1p]) + ([0] if n1p in MIXED else [])
    steps = []
    for top in DB_ORDERS:
        if ov == "lpc0":
            # LORDER: every words-per-lane value of the class and the mixed batch, LSOLN on and off (OPT 3 and 1);
            # without LORDER the round shape is no template argument: one batch (OPT 2 and 0)
            steps += [(top, w, True, ls) for w in wpls for ls in (True, False)]
            steps += [(top, max(wpls), False, ls) for ls in (True, False)]
        elif ov in ("lpc1", "lpc2"):
            # four-word sets: OPT 4..11, all four option pairs; narrower sets: the general kernel with several lanes
            steps += [(top, max(wpls), lo, ls) for lo in (True, False) for ls in ((True, False) if top == 111 else (True,))]
        else:
            # the general kernel reads everything at run time: the mixed batch where the class has one
            steps += [(top, wpls[-1], lo, True) for lo in (True, False)]
    return steps


def pair_names(family, n1p, ov, top, lorder):
    """The kernels of a pair search that lists every entry of database `top`: ({score / record pass}, {map pass}).
    Launches go per order bucket, laid out for the bucket's largest listed entry."""
    kq = n1p < 32
    first, maps = set(), set()
    for b in set(bucket_of(n) for n in DB_ORDERS[top]):
        m2w, cells = layout_of(max(n for n in DB_ORDERS[top] if bucket_of(n) == b))
        if family == "pair_match":
            first.add(kernel_name(family, n1p, m2w, kq or ov == "qlds", cells))
            maps.add(kernel_name(family, n1p, m2w, kq or ov == "qlds", cells))
        elif ov == "qlds":
            first.add(kernel_name(family, n1p, m2w, True, cells))
            maps.add(kernel_name(family, n1p, m2w, True, cells))
        else:                                       # lpc0: LSOLN-off specialisations score, the general kernel maps
            first.add(kernel_name(family, n1p, m2w, kq, cells, int(lorder)))
            maps.add(kernel_name(family, n1p, m2w, kq, cells))
    return first, maps


def recipes():
    out = []
    for n1p in (16, 32, 64, 112):
        for ov in ("lpc0", "lpc1", "lpc2", "general") + (("qlds",) if n1p >= 32 else ()):
            out.append(("plain", n1p, ov))
        for family, ovs in (("match", ("default", "qlds")), ("pair", ("lpc0", "qlds")), ("pair_match", ("default", "qlds"))):
            for ov in ovs:
                if ov != "qlds" or n1p >= 32:
                    out.append((family, n1p, ov))
    return out


def other_family_steps(n1p, ov):
    """(database, lorder) of the searches of a match / pair / pair-match recipe: the options are arguments there (the
    pair family's LORDER is a template argument of its score pass), so the default placement runs both LORDER values
    and the forced one LORDER = F"""
    return [(top, lo) for top in DB_ORDERS for lo in ((False,) if ov == "qlds" else (True, False))]


def planned_names(family, n1p, ov):
    """every instantiation the recipe launches under a comparison"""
    if family == "plain":
        return {plain_name(n1p, ov, top, w, lo, ls) for top, w, lo, ls in plain_steps(n1p, ov)}
    names = set()
    for top, lo in other_family_steps(n1p, ov):
        if family == "match":
            m2w, cells = layout_of(top)
            names.add(kernel_name("match", n1p, m2w, n1p < 32 or ov == "qlds", cells))
        else:
            first, maps = pair_names(family, n1p, ov, top, lo)
            names |= first | maps
    return names


# Instantiations no input reaches through the host code.  Dead code: DESIGN 6f lists them for removal.
UNREACHABLE = {}
for _m2w, _cells in ((1, FULL8), (2, FULL5), (2, TRI5), (4, TRI5)):
    for _family in KERNEL:
        # size_workgroup starts the 16 class with its query cells in LDS (SAT_EXP_QLDS cannot turn that off: `|| n1p <
        # 32`) and gives them up only when 64 chains do not fit 160 KiB; the largest 16-class workgroup (256 chains, a
        # 111-SSE entry) takes under 40 KiB
        UNREACHABLE[kernel_name(_family, 16, _m2w, False, _cells)] = \
            "size_workgroup: qlds = n1p < 32 is dropped only when lds_bytes exceeds 160 KiB, a 16-class workgroup never does"
    for _opt in (1, 3):
        # refresh_descriptors: class_wpl is 0 only for queries of different compaction_shape; 65..111 SSEs all give 4
        UNREACHABLE[kernel_name("plain", 112, _m2w, False, _cells, _opt, 0)] = \
            "compaction_shape: every order of the 112 class has wpl = 4, so class_wpl is never 0 (mixed)"

LAUNCHED = set()            # names this run launched under a comparison
RAN = set()                 # recipes this run completed


# ---------------------------------------------------------------- running a recipe
def fresh_searcher(monkeypatch, overrides):
    for k in list(os.environ):
        if k.startswith("SAT_EXP_"):
            monkeypatch.delenv(k)
    for k, v in overrides.items():
        monkeypatch.setenv(k, v)
    assert sat.device_count() >= 1, "GPU tests need a HIP device (no CPU path exists)"
    return sat.Searcher(0)


def run_plain(s, data, n1p, ov):
    for top in DB_ORDERS:
        s.upload(data.db[top])
        for t, wpl, lorder, lsoln in plain_steps(n1p, ov):
            if t != top:
                continue
            orders = batch_orders(n1p, wpl)
            s.set_queries(data.batch(orders), 0)
            scores, maps, _ = s.search(lorder, lsoln, MAXSTART)
            want = plain_name(n1p, ov, top, wpl, lorder, lsoln)
            what = f"{want}: db {top}, queries {orders}, lorder {lorder}, lsoln {lsoln}"
            assert names_in(s.last_launch_info()) == [want], f"{what}: launched {s.last_launch_info()}"
            for qi, n1 in enumerate(orders):
                osc, omp = data.plain(top, n1, qi == 0, lorder)
                assert np.array_equal(scores[qi], osc), f"{what}: scores of query {qi} differ at entries {np.nonzero(scores[qi] != osc)[0]}"
                if lsoln:
                    assert np.array_equal(maps[qi], omp), f"{what}: maps of query {qi} differ"
            LAUNCHED.add(want)


def run_match(s, data, n1p, ov):
    orders = batch_orders(n1p, max(BATCHES[n1p]))
    for top, lorder in other_family_steps(n1p, ov):
        s.upload(data.db[top])
        s.set_queries(data.batch(orders), 0)
        counts, scores, restarts, maps, _ = s.search_matches(MAX_MATCHES, lorder, MAXSTART)
        m2w, cells = layout_of(top)
        want = kernel_name("match", n1p, m2w, n1p < 32 or ov == "qlds", cells)
        what = f"{want}: db {top}, queries {orders}, lorder {lorder}"
        rec, rep = s.last_launch_info().split(" | ")
        assert rec.startswith("record pass") and rep.startswith("replay pass")
        assert names_in(rec) == [want] and names_in(rep) == [want], f"{what}: launched {s.last_launch_info()}"
        for qi, n1 in enumerate(orders):
            oc, osc, ors, omp = data.matches(top, n1, qi == 0, lorder)
            assert np.array_equal(counts[qi], oc), f"{what}: counts of query {qi}"
            assert np.array_equal(scores[qi], osc), f"{what}: scores of query {qi}"
            assert np.array_equal(restarts[qi], ors), f"{what}: restarts of query {qi}"
            assert np.array_equal(maps[qi][..., :n1], omp[..., :n1]), f"{what}: maps of query {qi}"
            assert (maps[qi][..., n1:] == -1).all()
        LAUNCHED.add(want)


def pair_list(n, seed):
    """every (query, entry) of a two-query batch and n entries, shuffled"""
    q, e = np.repeat(np.arange(2), n), np.tile(np.arange(n), 2)
    perm = np.random.default_rng(seed).permutation(2 * n)
    return q[perm].astype(np.int32), e[perm].astype(np.int32)


def run_pair(s, data, n1p, ov):
    orders = batch_orders(n1p, max(BATCHES[n1p]))
    for top, lorder in other_family_steps(n1p, ov):
        s.upload(data.db[top])
        s.set_queries(data.batch(orders), 0)
        q, e = pair_list(len(DB_ORDERS[top]), top + n1p)
        scores, maps = s.search_pairs(q, e, lorder, True, MAXSTART)
        first, second = pair_names("pair", n1p, ov, top, lorder)
        what = f"db {top}, queries {orders}, lorder {lorder}"
        score_info, map_info = s.last_launch_info().split(" | ")
        assert score_info.startswith("score pass") and map_info.startswith("map pass")
        assert set(names_in(score_info)) == first, f"{what}: score pass launched {score_info}, expected {sorted(first)}"
        assert set(names_in(map_info)) == second, f"{what}: map pass launched {map_info}, expected {sorted(second)}"
        for qi, n1 in enumerate(orders):
            osc, omp = data.plain(top, n1, qi == 0, lorder)
            rows = q == qi
            assert np.array_equal(scores[rows], osc[e[rows]]), f"{what}: scores of query {qi}"
            assert np.array_equal(maps[rows], omp[e[rows]]), f"{what}: maps of query {qi}"
        LAUNCHED.update(first | second)


def run_pair_match(s, data, n1p, ov):
    orders = batch_orders(n1p, max(BATCHES[n1p]))
    for top, lorder in other_family_steps(n1p, ov):
        s.upload(data.db[top])
        s.set_queries(data.batch(orders), 0)
        q, e = pair_list(len(DB_ORDERS[top]), top + n1p + 1)
        counts, scores, restarts, maps, _ = s.search_pairs_matches(q, e, MAX_MATCHES, lorder, MAXSTART)
        first, second = pair_names("pair_match", n1p, ov, top, lorder)
        what = f"db {top}, queries {orders}, lorder {lorder}"
        rec, sel, rep = s.last_launch_info().split(" | ")
        assert rec.startswith("record pass") and sel == "select" and rep.startswith("map pass")
        assert set(names_in(rec)) == first, f"{what}: record pass launched {rec}, expected {sorted(first)}"
        assert set(names_in(rep)) == second, f"{what}: map pass launched {rep}, expected {sorted(second)}"
        for qi, n1 in enumerate(orders):
            oc, osc, ors, omp = data.matches(top, n1, qi == 0, lorder)
            rows = q == qi
            assert np.array_equal(counts[rows], oc[e[rows]]), f"{what}: counts of query {qi}"
            assert np.array_equal(scores[rows], osc[e[rows]]), f"{what}: scores of query {qi}"
            assert np.array_equal(restarts[rows], ors[e[rows]]), f"{what}: restarts of query {qi}"
            assert np.array_equal(maps[rows][..., :n1], omp[e[rows]][..., :n1]), f"{what}: maps of query {qi}"
        LAUNCHED.update(first | second)


RUNNERS = {"plain": run_plain, "match": run_match, "pair": run_pair, "pair_match": run_pair_match}


@pytest.mark.parametrize("family,n1p,ov", recipes(), ids=lambda v: str(v))
def test_instantiations_equal_the_reference_under_their_own_name(monkeypatch, data, family, n1p, ov):
    """One (family, query class, override set): every search of the recipe launches the instantiation the recipe names
    - compared with the info string, not with the enumeration - and returns the reference's bits."""
    with fresh_searcher(monkeypatch, OVERRIDES[ov]) as s:
        RUNNERS[family](s, data, n1p, ov)
    RAN.add((family, n1p, ov))


def test_every_instantiation_is_compared_or_unreachable():
    """{names the recipes launch under a comparison} and UNREACHABLE are disjoint and together the enumerated list.  The
    recipes' names are planned from the recipe tables; each recipe test asserts that its searches launched exactly
    those, and when the whole module ran, the names actually launched must be the planned ones."""
    listed = sat.sa_kernel_instances()
    assert len(listed) == len(set(listed)) == 328
    planned = set()
    for r in recipes():
        planned |= planned_names(*r)
    assert not planned & set(UNREACHABLE), sorted(planned & set(UNREACHABLE))
    assert planned | set(UNREACHABLE) == set(listed), (sorted(set(listed) - planned - set(UNREACHABLE)),
                                                        sorted((planned | set(UNREACHABLE)) - set(listed)))
    per_family = {f: sum(n.startswith(k + "<") for n in planned) for f, k in KERNEL.items()}
    assert per_family == {"plain": 188, "match": 28, "pair": 60, "pair_match": 28}
    assert len(UNREACHABLE) == 24
    assert LAUNCHED <= planned
    if RAN == set(recipes()):
        assert LAUNCHED == planned, sorted(planned - LAUNCHED)


# ---------------------------------------------------------------- the default launch plan at small shapes
def sub_query(data, src, n1, seed):
    rng = np.random.default_rng(seed)
    t, d = data.pool[0][src], data.pool[1][src]
    sel = np.sort(rng.choice(111, size=n1, replace=False))
    return t[np.ix_(sel, sel)].copy(), d[np.ix_(sel, sel)].copy(), np.diagonal(t)[sel].copy()


def oracle_of_batch(db, queries, lorder, lsoln, maxstart, idx):
    """oracle_lib.search of every query of a batch (ordinals from 0) over entries idx, on a few threads: the oracle is a
    C call that shares no state between calls"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda a: oracle_lib.search(db, *a[1], lorder, lsoln, maxstart, entries=idx, query_ordinal=a[0]),
                             enumerate(queries)))


PLAN_MAXSTART = 40
# 18 orders per class, every words-per-lane value of the class among them
PLAN_ORDERS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 16, 9,
               17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 17, 32,
               33, 34, 35, 36, 37, 38, 40, 43, 46, 49, 52, 55, 58, 60, 62, 63, 64, 33,
               65, 66, 68, 70, 73, 76, 80, 84, 88, 92, 96, 100, 104, 107, 109, 110, 111, 65]


@pytest.mark.parametrize("lorder", [True, False])
def test_default_plan_one_launch_per_bucket_and_class(monkeypatch, data, lorder):
    """No override.  launch_search keeps ONE launch per class while entries x queries OF THAT CLASS stay at or under 4096
    (`view.n * nqc`, not the whole batch), so 18 queries per class need 228 entries or more to split: 231 entries, 33 in
    each of the seven order buckets, both edges of every bucket included, against 72 queries with mixed words per lane
    in every class that has several.  The plan is then one launch per bucket and class on side streams, LSOLN on, cut
    by the slab budget where needed.  Scores and maps of every query are compared with the oracle on every third entry
    (77 entries, every bucket among them: the CPU reference of all 16 632 pairs would take several times the few
    seconds a test may); the restart count is 40, which one wave of chains covers: the launch plan does not depend on
    it."""
    orders = []
    for lo, hi in zip((1,) + tuple(b + 1 for b in BUCKET_MAX[:-1]), BUCKET_MAX):
        orders += [lo, hi, hi] + [lo + (7 * k) % (hi - lo + 1) for k in range(30)]
    rng = np.random.default_rng(7)
    orders = [orders[i] for i in rng.permutation(len(orders))]
    src = [int(x) for x in rng.integers(0, POOL, len(orders))]
    db = sat.StructSet.from_dense(orders, [data.pool[0][k] for k in src], [data.pool[1][k] for k in src])
    assert len(db) == 231 and len(db) * 18 > 4096
    queries = [sub_query(data, (5 * i) % POOL, n1, 3000 + i) for i, n1 in enumerate(PLAN_ORDERS)]
    idx = np.arange(0, len(db), 3)
    assert set(bucket_of(orders[i]) for i in idx) == set(range(7))
    with fresh_searcher(monkeypatch, {}) as s:
        s.upload(db)
        s.set_queries(queries, 0)
        scores, maps, _ = s.search(lorder, True, PLAN_MAXSTART)
        info = s.last_launch_info()
    launches = info.split("; ")
    assert len(launches) == 7 * 4, info
    got = set(names_in(info))
    assert len(names_in(info)) == 28
    for n1p in (16, 32, 64, 112):
        seen = set()
        for n in got:
            m = re.match(r"sat_sa_kernel<(\d+), (\d), (true|false), (-?\d+), (\d), (\d)>", n)
            if int(m.group(1)) == n1p:
                seen.add((int(m.group(2)), int(m.group(6))))
                assert m.group(3) == ("true" if n1p < 32 else "false")
                if lorder and int(m.group(4)) in (1, 3):
                    assert int(m.group(5)) == (4 if n1p == 112 else 0), n      # mixed words per lane
        assert seen == {(1, FULL8), (2, FULL5), (2, TRI5), (4, TRI5)}, (n1p, info)
    want = oracle_of_batch(db, queries, lorder, True, PLAN_MAXSTART, idx)
    for qi, (osc, omp, _) in enumerate(want):
        assert np.array_equal(scores[qi][idx], osc), f"scores of query {qi} ({PLAN_ORDERS[qi]} SSEs)"
        assert np.array_equal(maps[qi][idx], omp), f"maps of query {qi} ({PLAN_ORDERS[qi]} SSEs)"


def test_default_plan_entries_per_workgroup_unforced(monkeypatch, data):
    """No override.  130 class-16 queries against 65 entries of at most 16 SSEs are 8450 pairs in one launch (one
    launch: the entries lie in one order bucket), at or above the 8192 from which launch_setup asks pick_epw.  The
    choice E is the heuristic's and is only recorded; the launch geometry must be the one reported, and the
    scores of every query the oracle's on every second entry, the last one - with E > 1 and 65 entries the one beside a
    spare slot - included."""
    rng = np.random.default_rng(11)
    orders = [1, 2, 16, 16] + [int(x) for x in rng.integers(3, 17, 61)]
    src = [int(x) for x in rng.integers(0, POOL, len(orders))]
    db = sat.StructSet.from_dense(orders, [data.pool[0][k] for k in src], [data.pool[1][k] for k in src])
    queries = [sub_query(data, i % POOL, 1 + (i * 5) % 16, 4000 + i) for i in range(130)]
    assert len(db) == 65 and len(db) * len(queries) >= 8192
    with fresh_searcher(monkeypatch, {}) as s:
        s.upload(db)
        s.set_queries(queries, 0)
        scores, _, _ = s.search(True, False, MAXSTART)
        info = s.last_launch_info()
    m = re.fullmatch(r"(sat_sa_kernel<16, 1, true, (-?\d+), 0, 0>) grid (\d+) x (\d+) block (\d+) x (\d+) lds (\d+)", info)
    assert m, info
    grid_x, grid_y, epw, threads = (int(m.group(k)) for k in (3, 4, 5, 6))
    print(f"pick_epw chose E = {epw}: {info}")
    assert epw >= 1 and grid_x == (len(db) + epw - 1) // epw and grid_y == len(queries) and threads % 64 == 0
    idx = np.arange(0, len(db), 2)
    assert idx[-1] == len(db) - 1
    for qi, (osc, _, _) in enumerate(oracle_of_batch(db, queries, True, False, MAXSTART, idx)):
        assert np.array_equal(scores[qi][idx], osc), f"scores of query {qi}"
