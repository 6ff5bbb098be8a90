"""Transitive search on the GPU (-m gpu): sat_reach_begin / add / frontier / rows / end, sat_search_reach and their shards.
The expected keys, supports and rows never come from the code under test: they are reach_lib's accumulator - numpy's
restatement of the key and a breadth-first walk in Python - over the planted score matrix itself, or over hits_cutoff(P)'s
rows of the same searches."""
import ctypes as C
import os

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import report

import reach_lib as rl

pytestmark = pytest.mark.gpu
SMALL_DB = "tableauxdistmatrixdb.small.ascii"
N = 1500                                                   # > 1024: two blocks of rows per query, the second ragged
BATCHES = (np.arange(0, 700), np.arange(700, 701), np.arange(701, 1500))      # 700, 1 and 799 queries
CHAIN = np.arange(990, 1060)                               # 70 nodes across the block edge at 1024
P = 1e-3


# ---------------------------------------------------------------- 1. planted graphs, step API
@pytest.fixture(scope="module")
def planted_db():
    """the database the graphs are planted in.  Their premises are checked here: a planted cell is under the cutoff for
    every pair of orders, a zero score is above it; norm2 = 16 has the p-value 0, which packs as 0 bits, and the two smaller
    planted scores differ in p as floats"""
    db = sat.synth.make_db(N, 8, 20, sort=False)
    lo, hi = int(db.orders.min()), int(db.orders.max())
    for n1 in (lo, hi):
        for n2 in (lo, hi):
            for norm2 in (6, 8, 16):
                st = report.stats(norm2 // 2 * (n1 + n2), n1, n2)
                assert st[0] == float(norm2) and st[2] == planted_pvalue(norm2) <= P
            assert report.stats(0, n1, n2)[2] > P
    assert planted_pvalue(16) == 0.0 < np.float32(planted_pvalue(8)) < np.float32(planted_pvalue(6))
    return db


@pytest.fixture(scope="module")
def planted_searcher(planted_db):
    with sat.Searcher(0) as s:
        s.upload(planted_db)
        yield s


def planted_graphs():
    """name -> (query rows, entry columns, norm2 planted there, seeds, batches)"""
    g = {}
    others = np.delete(np.arange(N), 700)
    g["star"] = (np.full(N - 1, 700), others, 16, [700], BATCHES)
    cliques = [np.arange(100, 140), np.arange(1040, 1080)]              # the second one straddles the block edge
    cells = [(i, j) for c in cliques for i in c for j in c if i != j] + [(139, 1040)]
    q, e = np.array([c[0] for c in cells]), np.array([c[1] for c in cells])
    g["two cliques, seeded before the bridge"] = (q, e, 16, [100], BATCHES)
    g["two cliques, seeded behind the bridge"] = (q, e, 16, [1050], BATCHES)
    g["diagonal"] = (np.arange(N), np.arange(N), 16, [3], BATCHES)
    g["chain"] = (CHAIN[:-1], CHAIN[1:], 16, [int(CHAIN[0])], (CHAIN,))
    # node 1030 is reachable at depths 2 (0 -> 1 -> 1030) and 3 (0 -> 2 -> 4 -> 1030); 30 has the parents 10 (norm2 6) and
    # 20 (norm2 8: the lower p) at depth 2; 31 has the parents 10 and 20 at equal scores
    q = np.array([0, 0, 1, 2, 4, 0, 0, 10, 20, 10, 20])
    e = np.array([1, 2, 1030, 4, 1030, 10, 20, 30, 30, 31, 31])
    n2 = np.array([16, 16, 16, 16, 16, 16, 16, 6, 8, 16, 16])
    g["depths and ties"] = (q, e, n2, [0], BATCHES)
    return g


def planted_scores(db, q, e, norm2):
    """0 everywhere, norm2 = `norm2` on the planted cells: 2 * score / (n1 + n2)"""
    scores = np.zeros((N, N), np.int32)
    scores[q, e] = (np.asarray(norm2) // 2) * (db.orders[q] + db.orders[e])
    return scores


def planted_pvalue(norm2):
    """the p-value of a row whose norm2 is that integer, for any pair of orders: the built-in table's entry"""
    return report.stats(int(norm2) * 8, 8, 8)[2]


def walk_planted(s, db, q, e, norm2, seeds, batches, repeat=1):
    """The walk by the step API next to reach_lib's: level d takes the nodes at depth d - 1, and every batch that holds
    one of them is searched (one restart, only to reach the searched state), its scores overwritten - the planted rows of
    the level's nodes, 0 elsewhere - and added `repeat` times.  Returns (the expected accumulator, the levels added)."""
    scores = planted_scores(db, q, e, norm2)
    norm2 = np.broadcast_to(np.asarray(norm2), np.shape(q))
    pv = np.array([planted_pvalue(x) for x in norm2])
    acc = rl.Accumulator(N, seeds)
    s.reach_begin(seeds)
    current = None
    for d in range(1, 63):
        frontier = acc.frontier(d - 1)
        before = s.d2h_bytes()
        got, count = s.reach_frontier(d - 1, cap=N)
        assert s.d2h_bytes() - before == 4 + 4 * len(frontier)
        assert count == len(frontier) and np.array_equal(got, frontier), "depth %d" % (d - 1)
        if len(frontier) == 0:
            return acc, d - 1
        for b, batch in enumerate(batches):
            active = np.isin(batch, frontier)
            if not active.any():
                continue
            if current != b:
                s.set_queries_from_db(batch, int(batch[0]))
                s.search(True, False, 1)
                current = b
            s.debug_set_scores(scores[batch] * active[:, None])
            before = s.d2h_bytes()
            for _ in range(repeat):
                s.reach_add(d, P, batch)
            assert s.d2h_bytes() == before                              # nothing comes back from an add
            cells = np.isin(q, batch[active])
            for _ in range(repeat):
                acc.add(d, q[cells], e[cells], pv[cells])
    return acc, 62


def same_state(s, acc, what):
    want = acc.rows()
    before = s.d2h_bytes()
    rows, count = s.reach_rows(cap=N)
    assert s.d2h_bytes() - before == 4 + 20 * len(want), what
    assert count == len(want), what
    rl.same_rows(rows, want, what)
    return rows


@pytest.mark.parametrize("name", list(planted_graphs()))
def test_planted_graph(planted_searcher, planted_db, name):
    s = planted_searcher
    q, e, norm2, seeds, batches = planted_graphs()[name]
    acc, levels = walk_planted(s, planted_db, q, e, norm2, seeds, batches)
    rows = same_state(s, acc, name)
    by_node = {int(r["node"]): r for r in rows}
    p16, p8 = np.float32(planted_pvalue(16)), np.float32(planted_pvalue(8))
    if name == "star":
        assert len(rows) == N and levels == 2 and (rows["depth"][rows["node"] != 700] == 1).all()
        assert (rows["parent"][rows["node"] != 700] == 700).all() and by_node[700]["support"] == 0
    if name == "two cliques, seeded before the bridge":
        assert len(rows) == 80 and by_node[139]["depth"] == 1 and by_node[1040]["depth"] == 2 and by_node[1079]["depth"] == 3
        assert by_node[1040]["parent"] == 139 and by_node[1079]["parent"] == 1040 and by_node[100]["support"] == 39
    if name == "two cliques, seeded behind the bridge":                 # the walk is directed: the near clique stays out
        assert len(rows) == 40 and rows["node"].min() == 1040 and levels == 2
        assert s.reach_frontier(63 - 1, cap=4)[1] == 0
    if name == "diagonal":
        assert len(rows) == 1 and tuple(rows[0])[:4] == (3, 0, -1, 0) and levels == 1
    if name == "chain":
        assert levels == 62 and np.array_equal(rows["node"], CHAIN[:63]) and np.array_equal(rows["depth"], np.arange(63))
        assert np.array_equal(rows["parent"][1:], CHAIN[:62]) and (rows["support"][1:] == 1).all()
        # the scores of the whole chain: depth 63 cannot be added, and nothing moved
        s.debug_set_scores(planted_scores(planted_db, q, e, norm2)[CHAIN])
        with pytest.raises(sat.SatError, match=r"\[-1\].*depth must be 1\.\.62 \(got 63\)"):
            s.reach_add(63, P, CHAIN)
        with pytest.raises(sat.SatError, match=r"\[-1\].*depth must be 0\.\.62 \(got 63\)"):
            s.reach_frontier(63, cap=4)
        same_state(s, acc, "chain, after the rejected add")
        assert report.reach_path(rows, int(CHAIN[62])) == CHAIN[:63][::-1].tolist()
    if name == "depths and ties":
        assert by_node[1030]["depth"] == 2 and by_node[1030]["parent"] == 1 and by_node[1030]["support"] == 2
        assert by_node[30]["parent"] == 20 and by_node[30]["pvalue"] == p8 and by_node[30]["support"] == 2      # the lower p, from the higher node
        assert by_node[31]["parent"] == 10 and by_node[31]["pvalue"] == p16 and by_node[31]["support"] == 2      # a tie: the lower node
        assert by_node[4]["depth"] == 2 and len(rows) == 9


def test_planted_graph_with_the_pass_cut_into_chunks(monkeypatch, planted_db):
    """SAT_EXP_SELECT_KEYS = 204 800 leaves 100 queries (of two blocks of 1024 rows each) to a launch of the add pass: the
    batches of 700 and 799 queries go in 7 and 8 launches, and both cliques' queries lie in launches that do not start at
    the batch's first query (100 .. 139 of the first batch, 339 .. 378 of the third)"""
    monkeypatch.setenv("SAT_EXP_SELECT_KEYS", str(100 * 2048))          # read when the context is created
    q, e, norm2, seeds, batches = planted_graphs()["two cliques, seeded before the bridge"]
    with sat.Searcher(0) as s:
        s.upload(planted_db)
        acc, levels = walk_planted(s, planted_db, q, e, norm2, seeds, batches)
        rows = same_state(s, acc, "chunked")
    assert len(rows) == 80 and levels == 4 and rows["depth"].max() == 3


def test_planted_rows_added_twice(planted_searcher, planted_db):
    s = planted_searcher
    q, e, norm2, seeds, batches = planted_graphs()["two cliques, seeded before the bridge"]
    once, _ = walk_planted(s, planted_db, q, e, norm2, seeds, batches)
    twice, _ = walk_planted(s, planted_db, q, e, norm2, seeds, batches, repeat=2)
    assert np.array_equal(once.keys, twice.keys) and np.array_equal(2 * once.support, twice.support) and once.support.any()
    same_state(s, twice, "added twice")


def test_external_queries(planted_searcher, planted_db):
    """queries 5 and 9 of the batch; the first stands for an external structure (node -1): its row against entry 5 is no
    self row, it loses the tie for node 20 against node 9, and alone it is recorded as parent -1.  Node 9's row against
    itself is none."""
    s, db = planted_searcher, planted_db
    batch = np.array([5, 9])
    q, e = np.array([5, 5, 9, 5, 9]), np.array([5, 20, 20, 1400, 9])
    s.reach_begin([9])
    s.set_queries_from_db(batch, 0)
    s.search(True, False, 1)
    s.debug_set_scores(planted_scores(db, q, e, 16)[batch])
    s.reach_add(1, P, [-1, 9])
    acc = rl.Accumulator(N, [9])
    acc.add(1, np.where(q == 5, -1, q), e, np.full(len(q), planted_pvalue(16)))
    rows = same_state(s, acc, "external")
    assert [tuple(r)[:4] for r in rows] == [(5, 1, -1, 1), (9, 0, -1, 0), (20, 1, 9, 2), (1400, 1, -1, 1)]
    # no seeds at all: an external start
    s.reach_begin()
    assert s.reach_rows(cap=4)[1] == 0 and s.reach_frontier(0, cap=4)[1] == 0
    s.reach_add(1, P, [-1, -1])
    rows, count = s.reach_rows(cap=N)
    assert count == 4 and [tuple(r)[:4] for r in rows] == [(5, 1, -1, 1), (9, 1, -1, 1), (20, 1, -1, 2), (1400, 1, -1, 1)]


# ---------------------------------------------------------------- 2. byte counts and caps
def test_byte_counts_and_caps(planted_searcher, planted_db):
    s = planted_searcher
    q, e, norm2, seeds, batches = planted_graphs()["star"]
    acc, _ = walk_planted(s, planted_db, q, e, norm2, seeds, batches)
    want = acc.rows()
    assert len(want) == N
    lib, ctx = s._lib, s._ctx
    for cap in (0, 1, 7, 1024, 1025, N - 1, N, N + 5):
        c = min(cap, N - 1)
        before = s.d2h_bytes()
        nodes, count = s.reach_frontier(1, cap=cap)
        assert s.d2h_bytes() - before == 4 + 4 * c
        assert count == N - 1 and np.array_equal(nodes, acc.frontier(1)[:cap])
        c = min(cap, N)
        before = s.d2h_bytes()
        rows, count = s.reach_rows(cap=cap)
        assert s.d2h_bytes() - before == 4 + 20 * c
        assert count == N
        rl.same_rows(rows, want[:cap], "cap %d" % cap)
    # a capped call writes nothing past the cap
    buf = np.full(16, -7, np.int32)
    count = C.c_int32(0)
    assert lib.sat_reach_frontier(ctx, 1, 5, buf.ctypes.data, C.byref(count)) == 0
    assert count.value == N - 1 and np.array_equal(buf[:5], np.arange(5)) and (buf[5:] == -7).all()
    # cap None: the count first, then the nodes
    before = s.d2h_bytes()
    nodes, count = s.reach_frontier(0)
    assert s.d2h_bytes() - before == 4 + 4 + 4 and nodes.tolist() == [700] and count == 1


# ---------------------------------------------------------------- 3. search_reach on real scores
SEED_NAME = "d1ubia_"
RESTARTS = 128
FIRST = 1000                                               # the run's first query ordinal
# The cutoff of the example run: at r = 128 the walk from d1ubia_ stops after the seed alone at P = 1e-6, after two levels
# ([1, 2] and [1, 3] queries) at 1e-5 and 1e-4, and searches three levels of [1, 3, 1] queries at 1e-3, 3e-3 and 1e-2 -
# five nodes, one of them at depth 2 - before nothing new turns up.
REACH_P = 1e-3


@pytest.fixture(scope="module")
def small(golden_dir):
    """the 586-entry example database with its example query, d1ubia_, appended as entry 586: sat_search_reach takes its
    seeds from the resident database, and d1ubia_ is no entry of the file"""
    db = sat.StructSet.read(os.path.join(golden_dir, SMALL_DB))
    query = sat.StructSet.read(os.path.join(golden_dir, "d1ubia_.input"), "query", skip_header_lines=2).subset([0])
    assert len(db) == 586 and len(query) == 1 and query.orders[0] == 8 and query.names[0].lower() == SEED_NAME
    assert SEED_NAME not in [n.lower() for n in db.names]
    return sat.StructSet(np.concatenate([db.orders, query.orders]), db.names + [SEED_NAME],
                         np.concatenate([db.cell_off, query.cell_off + len(db.tab)]), np.concatenate([db.tab, query.tab]),
                         np.concatenate([db.dist, query.dist]))


def compose(s, db, seed, p, first, max_depth=62, max_queries=None, censor=None):
    """search_reach rebuilt from its steps: level d's queries are the nodes at depth d - 1, ascending, with the ordinals
    first + (queries searched before them), searched 256 at a time; hits_cutoff(p)'s rows are the steps; the walk is
    reach_lib's.  Returns (rows, info without the times, the level sizes)."""
    n = len(db)
    max_queries = n if max_queries is None else max_queries
    acc = rl.Accumulator(n, [seed])
    searched, levels, sizes = 0, 0, []
    d = 1
    while True:
        frontier = acc.frontier(d - 1)
        if len(frontier) == 0:
            stop = "exhausted"
            break
        if d - 1 == max_depth:
            stop = "depth"
            break
        if searched + len(frontier) > max_queries:
            stop = "budget"
            break
        for at in range(0, len(frontier), 256):
            part = frontier[at:at + 256]
            s.set_queries_from_db(part, first + searched + at)
            s.search(True, False, RESTARTS)
            if censor is not None:
                s.fit_statistics(censor)
            for node, rows in zip(part, s.hits_cutoff(p)):
                acc.add(d, np.full(len(rows), node), rows["entry"], rows["pvalue"])
        searched += len(frontier)
        levels += 1
        sizes.append(len(frontier))
        d += 1
    rows = acc.rows()
    return rows, {"levels": levels, "queries": searched, "reached": len(rows), "stop": stop}, sizes


def same_run(got, want, what):
    rows, info = got
    rl.same_rows(rows, want[0], what)
    assert {k: info[k] for k in want[1]} == want[1], what
    assert info["search_ms"] > 0 and info["pass_ms"] > 0, what


@pytest.fixture(scope="module")
def example(small):
    """the seed's node, and the composition's (rows, info, level sizes) of the plain run"""
    seed = small.names.index(SEED_NAME)
    with sat.Searcher(0) as s:
        s.upload(small)
        return seed, compose(s, small, seed, REACH_P, FIRST)


@pytest.fixture(scope="module")
def example_fitted(small, example):
    with sat.Searcher(0) as s:
        s.upload(small)
        return compose(s, small, example[0], REACH_P, FIRST, censor=0.1)


@pytest.fixture(scope="module")
def example_polished(small, example):
    with sat.Searcher(0) as s:
        s.upload(small)
        s.set_polish_all(2)
        return compose(s, small, example[0], REACH_P, FIRST)


def test_the_example_walk(example):
    """the expectation itself is a walk worth the name (the level sizes observed are in REACH_P's comment)"""
    seed, (rows, info, sizes) = example
    print("level sizes at P = %g: %s, %d reached, stop: %s" % (REACH_P, sizes, len(rows), info["stop"]))
    assert info["levels"] >= 3 and (rows["depth"] >= 2).any()
    assert rows[rows["node"] == seed]["depth"][0] == 0 and sizes[0] == 1
    for r in rows[rows["depth"] >= 1]:                                  # every chain of parents leads back to the seed
        path = report.reach_path(rows, int(r["node"]))
        assert path[-1] == seed and len(path) == r["depth"] + 1


@pytest.mark.parametrize("batch", [256, 7, 1])
def test_search_reach_equals_its_steps(small, example, batch):
    seed, want = example
    with sat.Searcher(0) as s:
        s.upload(small)
        got = s.search_reach([seed], REACH_P, batch=batch, first_query_ordinal=FIRST, maxstart=RESTARTS)
        same_run(got, want, "batch %d" % batch)
        # the accumulator stays: the step calls read it
        rows, count = s.reach_rows(cap=len(small))
        rl.same_rows(rows, want[0], "reach_rows after the run")
        # a capped run returns the uncapped count
        rows, info = s.search_reach([seed], REACH_P, batch=batch, first_query_ordinal=FIRST, maxstart=RESTARTS, cap=3)
        rl.same_rows(rows, want[0][:3], "capped")
        assert info["reached"] == len(want[0])


@pytest.mark.parametrize("before", ["no query was ever set", "a batch of five was searched"])
def test_a_capped_run_leaves_the_searcher_on_the_last_batch(small, example, before):
    """max_depth = 2 ends the run behind the level of three queries, and cap = 1 keeps that level out of the rows: the
    searcher must still know the batch the library holds, or results() would size its buffers by the batch before"""
    seed, (want, _, sizes) = example
    assert sizes[1] == 3
    tail = want["node"][want["depth"] == 1]
    with sat.Searcher(0) as s, sat.Searcher(0) as fresh:
        s.upload(small)
        fresh.upload(small)
        if before.startswith("a batch"):
            s.set_queries_from_db(np.arange(5), 0)
            s.search(True, False, 4)
        rows, info = s.search_reach([seed], REACH_P, max_depth=2, batch=7, first_query_ordinal=FIRST, maxstart=RESTARTS, cap=1)
        assert len(rows) == 1 and info["levels"] == 2 and info["stop"] == "depth" and info["reached"] > 1
        assert s.n_queries == 3 and s._n1s.tolist() == small.orders[tail].tolist()
        fresh.set_queries_from_db(tail, FIRST + 1)
        plain = fresh.search(True, False, RESTARTS)[0]
        scores = s.results()[0]
        assert scores.shape == (3, len(small)) and np.array_equal(scores, plain)
        cut, cut_fresh = s.hits_cutoff(REACH_P), fresh.hits_cutoff(REACH_P)
        assert len(cut) == 3 and all(np.array_equal(a, b) for a, b in zip(cut, cut_fresh))
        assert len(s.fit_statistics(0.1)) == 3
    with sat.MultiSearcher(2, devices=[0, 0]) as m:
        m.upload(small)
        m.search_reach([seed], REACH_P, max_depth=2, batch=7, first_query_ordinal=FIRST, maxstart=RESTARTS, cap=1)
        assert m.n_queries == 3
        assert all(np.array_equal(a, b) for a, b in zip(m.hits_cutoff(REACH_P), cut_fresh))


def test_search_reach_stops_at_a_level_boundary(small, example):
    seed, (rows, info, sizes) = example
    with sat.Searcher(0) as s:
        s.upload(small)
        # the budget holds two levels and one query less than the third
        budget = sizes[0] + sizes[1] + sizes[2] - 1
        want = compose(s, small, seed, REACH_P, FIRST, max_queries=budget)
        assert want[1] == {"levels": 2, "queries": sizes[0] + sizes[1], "reached": len(want[0]), "stop": "budget"}
        assert want[0]["depth"].max() == 2
        same_run(s.search_reach([seed], REACH_P, max_queries=budget, batch=7, first_query_ordinal=FIRST, maxstart=RESTARTS), want, "budget")
        # exactly the three levels fit
        budget += 1
        want = compose(s, small, seed, REACH_P, FIRST, max_queries=budget)
        assert want[1]["levels"] >= 3
        same_run(s.search_reach([seed], REACH_P, max_queries=budget, batch=7, first_query_ordinal=FIRST, maxstart=RESTARTS), want, "budget + 1")
        # max_depth = 1: the seed's own hits and no more
        want = compose(s, small, seed, REACH_P, FIRST, max_depth=1)
        assert want[1]["levels"] == 1 and want[1]["stop"] == "depth" and want[0]["depth"].max() == 1
        same_run(s.search_reach([seed], REACH_P, max_depth=1, first_query_ordinal=FIRST, maxstart=RESTARTS), want, "max_depth 1")


def test_search_reach_fitted(small, example, example_fitted):
    seed, plain = example
    want = example_fitted
    with sat.Searcher(0) as s:
        s.upload(small)
        assert not np.array_equal(want[0]["pvalue"], plain[0]["pvalue"]) or len(want[0]) != len(plain[0])       # the fit did move the rows
        same_run(s.search_reach([seed], REACH_P, censor=0.1, batch=7, first_query_ordinal=FIRST, maxstart=RESTARTS), want, "censor 0.1")


@pytest.mark.parametrize("scratch_kb", [0, 256], ids=["polished", "polished, 256 KB of scratch"])
def test_search_reach_polished(monkeypatch, small, example, example_polished, scratch_kb):
    seed, want = example[0], example_polished
    if scratch_kb:
        monkeypatch.setenv("SAT_EXP_SCRATCH_KB", str(scratch_kb))       # read when the context is created
    with sat.Searcher(0) as s:
        s.upload(small)
        s.set_polish_all(2)
        same_run(s.search_reach([seed], REACH_P, batch=7, first_query_ordinal=FIRST, maxstart=RESTARTS), want, "polished")
        info = s.last_launch_info()
        assert info.startswith("polish all (2 tops, "), info
        launches = int(info.split("polish all (2 tops, ")[1].split(" launches")[0])
        assert (launches > 1) == bool(scratch_kb), info                 # the small budget did cut the last batch's search


# ---------------------------------------------------------------- 4. shards
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2", "3"])
def test_shards_equal_one_context(small, example, example_fitted, example_polished, planted_db, devices):
    seed, want = example
    with sat.MultiSearcher(len(devices), devices=devices) as m:         # the sharded loop's own fit and polished search
        m.upload(small)
        same_run(m.search_reach([seed], REACH_P, censor=0.1, batch=7, first_query_ordinal=FIRST, maxstart=RESTARTS), example_fitted,
                 "%d shards, censor 0.1" % len(devices))
        m.set_polish_all(2)
        same_run(m.search_reach([seed], REACH_P, batch=7, first_query_ordinal=FIRST, maxstart=RESTARTS), example_polished,
                 "%d shards, polished" % len(devices))
    with sat.MultiSearcher(len(devices), devices=devices) as m:
        m.upload(small)
        for batch in (256, 7):
            same_run(m.search_reach([seed], REACH_P, batch=batch, first_query_ordinal=FIRST, maxstart=RESTARTS), want,
                     "%d shards, batch %d" % (len(devices), batch))
        rows, count = m.reach_rows(cap=len(small))
        rl.same_rows(rows, want[0], "reach_rows of the shards")
        depth1 = want[0]["node"][want[0]["depth"] == 1]
        nodes, count = m.reach_frontier(1, cap=2)
        assert count == len(depth1) and np.array_equal(nodes, depth1[:2])
        # the checks are made before any shard works
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 0: node %d " % len(small)):
            m.reach_add(1, 0.5, [len(small)] + [0] * (m.n_queries - 1))
        with pytest.raises(sat.SatError, match=r"\[-1\].*seed 1: node 4 listed twice"):
            m.reach_begin([4, 4])
        rl.same_rows(m.reach_rows(cap=len(small))[0], want[0], "after the rejected calls")
        m.reach_end()
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_reach_begin"):
            m.reach_rows(cap=4)
    # the planted case: every shard's scores are its columns of the planted matrix
    q, e, norm2, seeds, batches = planted_graphs()["depths and ties"]
    scores = planted_scores(planted_db, q, e, norm2)
    pv = np.array([planted_pvalue(x) for x in norm2])
    acc = rl.Accumulator(N, seeds)
    with sat.MultiSearcher(len(devices), devices=devices) as m:
        m.upload(planted_db)
        begin = m.shards()
        m.reach_begin(seeds)
        for d in (1, 2, 3):
            frontier = acc.frontier(d - 1)
            got, count = m.reach_frontier(d - 1, cap=N)
            assert count == len(frontier) and np.array_equal(got, frontier)
            m.set_queries_from_db(frontier, 0)
            m.search_only(True, False, 1)
            for g in range(m.ndev):
                part = np.ascontiguousarray(scores[frontier][:, begin[g]:begin[g + 1]])
                assert m._lib.sat_debug_set_scores(m._lib.sat_debug_multi_ctx(m._m, g), part.ctypes.data) == 0
            before = m.d2h_bytes()
            m.reach_add(d, P, frontier)
            assert m.d2h_bytes() == before
            cells = np.isin(q, frontier)
            acc.add(d, q[cells], e[cells], pv[cells])
        before = m.d2h_bytes()
        rows, count = m.reach_rows(cap=N)
        assert m.d2h_bytes() - before == m.ndev * 12 * N
        rl.same_rows(rows, acc.rows(), "planted, %d shards" % m.ndev)
        assert len(rows) == 9 and rows[rows["node"] == 30]["parent"][0] == 20 and rows[rows["node"] == 1030]["depth"][0] == 2


# ---------------------------------------------------------------- 5. states and arguments
def test_states_and_arguments(small, example):
    seed, want = example
    n = len(small)
    nodes = np.arange(8, dtype=np.int32)
    with sat.Searcher(0) as s:
        lib, ctx = s._lib, s._ctx
        with pytest.raises(sat.SatError, match=r"\[-5\].*no database"):
            s.reach_begin([0], n_nodes=n)
        with pytest.raises(sat.SatError, match=r"\[-5\].*no database"):
            s.search_reach([0], 0.5)
        s.upload(small)
        s.set_queries_from_db(nodes, 0)
        s.search(True, False, 4)
        for call in (lambda: s.reach_add(1, 0.5, nodes), lambda: s.reach_frontier(0, cap=1), lambda: s.reach_rows(cap=1)):
            with pytest.raises(sat.SatError, match=r"\[-5\].*sat_reach_begin"):          # before begin
                call()
        for bad_n, text in ((0, "n_nodes must be >= 1"), (n - 1, "ordinal %d" % (n - 1)), (1 << 27, r"n_nodes = 134217728")):
            with pytest.raises(sat.SatError, match=r"\[-1\].*" + text):
                s.reach_begin([0], n_nodes=bad_n)
        for seeds, text in (([0, n], "seed 1: node %d outside 0..%d" % (n, n - 1)), ([0, -1], "seed 1: node -1 outside"),
                            ([3, 5, 7, 5, 3], "seed 3: node 5 listed twice")):
            with pytest.raises(sat.SatError, match=r"\[-1\].*" + text):
                s.reach_begin(seeds)
        assert lib.sat_reach_begin(ctx, n, 2, None) == -1 and lib.sat_reach_begin(ctx, n, -1, None) == -1
        s.reach_begin([2])
        s.set_queries_from_db(nodes, 0)
        with pytest.raises(sat.SatError, match=r"\[-5\].*no search has run"):             # add before a search
            s.reach_add(1, 0.5, nodes)
        s.search(True, False, 4)
        acc = rl.Accumulator(n, [2])
        for node, rows in zip(nodes, s.hits_cutoff(0.5)):
            acc.add(1, np.full(len(rows), node), rows["entry"], rows["pvalue"])
        s.reach_add(1, 0.5, nodes)
        rl.same_rows(s.reach_rows(cap=n)[0], acc.rows(), "first add")
        # every rejected call leaves the accumulator as it was
        for depth in (0, -1, 63):
            with pytest.raises(sat.SatError, match=r"\[-1\].*depth must be 1\.\.62"):
                s.reach_add(depth, 0.5, nodes)
        bad = nodes.copy()
        bad[3] = -2
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 3: node -2 outside -1\.\.%d" % (n - 1)):
            s.reach_add(1, 0.5, bad)
        bad[3], bad[7] = -1, n
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 7: node %d " % n):
            s.reach_add(1, 0.5, bad)
        assert lib.sat_reach_add(ctx, 1, 0.5, None) == -1
        for p in (float("nan"), float("inf"), -1.0):
            with pytest.raises(sat.SatError, match=r"\[-1\].*max_pvalue"):
                s.reach_add(1, p, nodes)
        count = C.c_int32(0)
        buf = np.zeros(4, np.int32)
        assert lib.sat_reach_frontier(ctx, 0, 4, buf.ctypes.data, None) == -1 and lib.sat_reach_frontier(ctx, 0, -1, buf.ctypes.data, C.byref(count)) == -1
        assert lib.sat_reach_frontier(ctx, 0, 4, None, C.byref(count)) == -1 and lib.sat_reach_rows(ctx, 4, None, C.byref(count)) == -1
        assert lib.sat_reach_rows(ctx, 0, None, None) == -1 and lib.sat_reach_frontier(ctx, -1, 4, buf.ctypes.data, C.byref(count)) == -1
        rl.same_rows(s.reach_rows(cap=n)[0], acc.rows(), "after the rejected calls")
        # the refusals of the loop
        for kw, text in (({"max_depth": 0}, "max_depth must be 1..62"), ({"max_depth": 63}, "max_depth must be 1..62"),
                         ({"max_queries": 0}, "max_queries must be >= 1"), ({"batch": 0}, "batch must be 1..256"),
                         ({"batch": 257}, "batch must be 1..256"), ({"censor": 0.6}, "censor must lie in"), ({"maxstart": 0}, "maxstart")):
            with pytest.raises(sat.SatError, match=r"\[-1\].*" + text):
                s.search_reach([seed], 0.5, **kw)
        for seeds, text in (([], "bad seed list"), ([n], "seed 0: entry %d outside 0..%d" % (n, n - 1)), ([1, 1], "seed 1: node 1 listed twice")):
            with pytest.raises(sat.SatError, match=r"\[-1\].*" + text):
                s.search_reach(seeds, 0.5)
        with pytest.raises(sat.SatError, match=r"\[-1\].*max_pvalue"):
            s.search_reach([seed], float("nan"))
        rl.same_rows(s.reach_rows(cap=n)[0], acc.rows(), "after the refused runs")
        # searches and query changes keep the accumulator, an upload drops it
        s.set_queries_from_db(nodes[:3], 0)
        s.search(True, False, 4)
        rl.same_rows(s.reach_rows(cap=n)[0], acc.rows(), "after a query change and a search")
        s.upload(small)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_reach_begin"):
            s.reach_rows(cap=1)
        s.reach_begin([2])
        s.reach_end()
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_reach_begin"):
            s.reach_frontier(0, cap=1)
        # after search_reach the context serves the last batch, as after a plain search of it ...
        rows, info = s.search_reach([seed], REACH_P, batch=7, first_query_ordinal=FIRST, maxstart=RESTARTS)
        last_level = want[0]["node"][want[0]["depth"] == info["levels"] - 1]
        tail = last_level[len(last_level) - ((len(last_level) - 1) % 7 + 1):]
        assert s.n_queries == len(tail)
        scores = s.results()[0]
        cut = s.hits_cutoff(REACH_P)
        with sat.Searcher(0) as fresh:
            fresh.upload(small)
            fresh.set_queries_from_db(tail, FIRST + info["queries"] - len(tail))
            plain = fresh.search(True, False, RESTARTS)[0]
            assert np.array_equal(scores, plain)
            for a, b in zip(cut, fresh.hits_cutoff(REACH_P)):
                assert np.array_equal(a, b)
            # ... and a following plain search is what a fresh context gives
            s.set_queries_from_db(nodes, 7)
            fresh.set_queries_from_db(nodes, 7)
            assert np.array_equal(s.search(True, False, RESTARTS)[0], fresh.search(True, False, RESTARTS)[0])
        # ordinals a key's parent field cannot hold: refused before anything is sized by them
        for top in ((1 << 27) - 1, 0x7FFFFFFF, 0xFFFFFFFF):
            ordinal = np.arange(n, dtype=np.int64)
            ordinal[-1] = top
            s.upload(small, db_ordinal=ordinal)
            with pytest.raises(sat.SatError, match=r"\[-1\].*a resident entry has ordinal %d .*nodes up to 134217726" % top):
                s.search_reach([seed], REACH_P)
            with pytest.raises(sat.SatError, match=r"\[-5\].*sat_reach_begin"):
                s.reach_rows(cap=1)
        # ordinals of a shard: the nodes are the ordinals
        s.upload(small, db_ordinal=np.arange(n) + 100)
        rows, info = s.search_reach([seed], REACH_P, first_query_ordinal=FIRST, maxstart=RESTARTS, max_depth=1)
        assert rows["node"].min() >= 100 and rows[rows["depth"] == 0]["node"].tolist() == [seed + 100]
        assert set(rows["parent"][rows["depth"] == 1].tolist()) == {seed + 100}
