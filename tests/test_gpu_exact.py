"""The exact search on the GPU (Searcher.search_exact): against the brute-force reference of
tests/exact_lib.py, against the plain search it starts from, against the host twin under a small budget - across runs,
launch cuts and shards -, on the example database, its refusals and what works on its rows afterwards."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cuda_satabsearch_amd as sat

import exact_lib as xl
import motif_lib as ml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def db():
    got = xl.gpu_db()
    assert len(got) == 201 and got.orders[:200].max() == 14 and got.orders[:200].min() == 1 and got.orders[200] == 111
    return got


@pytest.fixture(scope="module")
def queries(db):
    return xl.gpu_queries(db)


@pytest.fixture(scope="module")
def searcher(db, queries):
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries, xl.GPU_FIRST)
        yield s


@pytest.fixture(scope="module")
def pairs(db, queries):
    return {(q, e): xl.Pair(db, e, queries[q]) for q in range(len(queries)) for e in range(len(db))}


@pytest.fixture(scope="module")
def plain1(searcher):
    """the plain search at one restart, LORDER: (scores, maps)"""
    scores, maps, _ = searcher.search(True, True, 1)
    return scores.copy(), maps.copy()


@pytest.mark.parametrize("lorder", [True, False])
def test_rows_are_the_brute_force_optimum(searcher, pairs, queries, db, lorder):
    """ordered: every row, the 111-SSE entry's too; unordered: the rows of queries of up to 5 SSEs and entries of up to 10"""
    scores, maps, _ = searcher.search_exact(lorder, 4, xl.FULL_BUDGET if lorder else 1 << 22)
    base, unproven, nodes = searcher.exact_results()
    compared = 0
    for (q, e), pair in pairs.items():
        assert pair.feasible(maps[q, e], lorder) and pair.full_score(maps[q, e]) == scores[q, e], (q, e)
        assert (maps[q, e, pair.n1:] == -1).all() and scores[q, e] >= base[q, e]
        if not lorder and (pair.n1 > 5 or pair.n2 > 10):
            continue
        assert not unproven[q, e], (q, e, nodes[q, e])
        assert scores[q, e] == pair.optimum(lorder)[0], (q, e, pair.n1, pair.n2)
        compared += 1
    assert compared == (len(pairs) if lorder else sum(1 for p in pairs.values() if p.n1 <= 5 and p.n2 <= 10)) and compared >= 500


def test_relation_to_the_plain_search(searcher, plain1):
    """At one restart SA is weak.  On the CPU (the oracle's SA, which the GPU's equals bit for bit, then the host twin at
    the default budget) the 2010 rows of this database split into 1025 improved and 985 left alone, 6 rows of the 111-SSE
    entry unproven; without the proof pass none improves."""
    pscores, pmaps = plain1
    scores, maps, _ = searcher.search_exact(True, 1)
    base, unproven, _ = searcher.exact_results()
    assert np.array_equal(base, pscores) and int(unproven.sum()) == 6 and unproven[:, :200].sum() == 0
    same = scores == base
    assert np.array_equal(scores[same], pscores[same]) and np.array_equal(maps[same], pmaps[same])
    assert (scores[~same] > base[~same]).all()
    assert (int((~same).sum()), int(same.sum())) == (1025, 985)
    assert (~same).sum() >= 0.05 * same.size and same.sum() >= 0.30 * same.size


@pytest.fixture(scope="module")
def budget_host(db, queries, plain1):
    """the host twin at 64 nodes a row from the plain search's rows"""
    return xl.host_rows(db, queries, True, xl.BUDGET_NODES, plain1[0], plain1[1])


def _same_rows(got, want):
    for k in range(4):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k


def test_budget_rows_are_the_host_twins(searcher, budget_host, plain1):
    hs, hm, hf, hn = budget_host
    assert int(hf.sum()) == 1127 and hn.max() <= xl.BUDGET_NODES          # (counted on the CPU)
    runs = []
    for _ in range(2):
        scores, maps, _ = searcher.search_exact(True, 1, xl.BUDGET_NODES)
        base, flags, nodes = searcher.exact_results()
        assert np.array_equal(base, plain1[0])
        runs.append((scores, maps, flags, nodes))
    _same_rows(runs[0], (hs, hm, hf, hn))
    _same_rows(runs[1], runs[0])
    stats = searcher.exact_stats()
    assert np.array_equal(stats["rows"], np.full(len(hs), hs.shape[1])) and np.array_equal(stats["proven"], (~hf).sum(axis=1))
    assert np.array_equal(stats["improved"], (hs > plain1[0]).sum(axis=1)) and np.array_equal(stats["gain"], (hs - plain1[0]).sum(axis=1))
    assert np.array_equal(stats["nodes"], hn.sum(axis=1, dtype=np.uint64))


def test_budget_rows_under_a_small_launch_budget(budget_host, tmp_path):
    """SAT_EXP_SCRATCH_KB is read when a context is created: a child process.  64 KB are 1024 rows of 64 nodes a launch: 102 entries x
    the 10 queries, and no launch crosses an order bucket"""
    out = str(tmp_path / "rows.npz")
    env = dict(os.environ, SAT_EXP_SCRATCH_KB="64")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "exact_lib.py"), out], check=True, env=env, timeout=300)
    got = np.load(out)
    info = bytes(got["info"]).decode()
    assert "exact pass (64 nodes a row" in info and "3 launches of up to 1020 rows" in info, info
    _same_rows((got["scores"], got["maps"], got["flags"], got["nodes"]), budget_host)


def test_budget_rows_on_three_shards(db, queries, budget_host, plain1):
    with sat.MultiSearcher(3, devices=[0, 0, 0]) as m:
        m.upload(db)
        m.set_queries(queries, xl.GPU_FIRST)
        m.search_exact(True, 1, xl.BUDGET_NODES)
        scores, maps, base, flags, nodes = m.exact_results()
        assert len(m.shards()) == 4 and np.array_equal(base, plain1[0])
        _same_rows((scores, maps, flags, nodes), budget_host)
        stats = m.exact_stats()
        assert np.array_equal(stats["proven"], (~flags).sum(axis=1)) and np.array_equal(stats["nodes"], nodes.sum(axis=1, dtype=np.uint64))
        assert np.array_equal(stats["rows"], np.full(len(queries), len(db)))


def test_example_database_equals_the_host_twin(golden_dir):
    """the ubiquitin query against the example database's entries of up to 20 SSEs, default budget"""
    whole = sat.StructSet.read(os.path.join(golden_dir, "tableauxdistmatrixdb.small.ascii"))
    small = whole.subset(np.nonzero(whole.orders <= 20)[0])
    qs = sat.StructSet.read(os.path.join(golden_dir, "d1ubia_.input"), "query", skip_header_lines=2)
    query = qs.dense(0) + (qs.ssetypes(0),)
    assert len(query[2]) == 8 and len(small) >= 50
    with sat.Searcher(0) as s:
        s.upload(small)
        s.set_queries([query])
        pscores, pmaps, _ = s.search(True, True, 16)
        scores, maps, _ = s.search_exact(True, 16)
        base, flags, nodes = s.exact_results()
    assert np.array_equal(base, pscores)
    _same_rows((scores, maps, flags, nodes), xl.host_rows(small, [query], True, 1 << 18, pscores, pmaps))
    assert (scores >= base).all()


def test_refusals_leave_the_last_search_readable(db, queries):
    with sat.Searcher(0) as s:
        s.set_queries(queries)
        with pytest.raises(sat.SatError, match=r"^\[-1\].*no database"):
            s.search_exact(True, 2)
        s.upload(db)
        s.set_queries(queries)
        before = s.search(True, True, 2)
        with pytest.raises(sat.SatError, match=r"^\[-1\].*exact one"):
            s.exact_results()
        with pytest.raises(sat.SatError, match=r"^\[-1\].*max_nodes"):
            s.search_exact(True, 2, 0)
        with pytest.raises(sat.SatError, match=r"^\[-1\].*max_nodes"):
            s.search_exact(True, 2, (1 << 32) + 1)
        after = s.results(lsoln=True)
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
        # a 17-SSE query anywhere in the batch, either order; nothing is launched
        for lorder in (True, False):
            s.set_queries(queries[:3] + [sat.synth.make_query(17, seed=5)] + queries[3:5])
            with pytest.raises(sat.SatError, match=r"^\[-1\].*query 3 has 17 SSEs"):
                s.search_exact(lorder, 2)
        kept = s.search(True, True, 2)
        with pytest.raises(sat.SatError, match=r"^\[-1\].*17 SSEs"):
            s.search_exact(True, 2)
        again = s.results(lsoln=True)
        assert np.array_equal(again[0], kept[0]) and np.array_equal(again[1], kept[1])
        # an exact search, then a plain one: the exact results are gone
        s.set_queries(queries)
        s.search_exact(True, 2, 64)
        s.exact_results()
        s.search(True, False, 2)
        with pytest.raises(sat.SatError, match=r"^\[-1\].*exact one"):
            s.exact_stats()


def test_downstream_calls_work_on_the_exact_rows(searcher, db):
    scores, maps, _ = searcher.search_exact(True, 1)
    again, amaps = searcher.results(lsoln=True)
    assert np.array_equal(again, scores) and np.array_equal(amaps, maps)
    base, flags, nodes = searcher.exact_results()
    hits, hmaps = searcher.topk_hits(5, lsoln=True)
    for q in range(scores.shape[0]):
        order = np.lexsort((np.arange(len(db)), -scores[q].astype(np.int64)))[:5]
        assert np.array_equal(hits[q]["entry"], order) and np.array_equal(hits[q]["score"], scores[q][order])
        assert np.array_equal(hmaps[q], maps[q][order])
    rows, rmaps = searcher.hits_cutoff(1.0, lsoln=True)
    for q in range(scores.shape[0]):
        assert np.array_equal(rows[q]["score"], scores[q][rows[q]["entry"]]) and np.array_equal(rmaps[q], maps[q][rows[q]["entry"]])
    stats = searcher.exact_stats()
    assert np.array_equal(stats["rows"], np.full(scores.shape[0], len(db))) and np.array_equal(stats["proven"], (~flags).sum(axis=1))
    assert np.array_equal(stats["improved"], (scores > base).sum(axis=1)) and np.array_equal(stats["gain"], (scores - base).sum(axis=1))
    assert np.array_equal(stats["nodes"], nodes.sum(axis=1, dtype=np.uint64))


def test_polished_incumbents(searcher, pairs):
    """with sat_polish_all_set on the incumbents are the polished rows: base = the polished search's scores, the proven
    rows the same optimum"""
    searcher.set_polish_all(2)
    try:
        pscores, pmaps, _ = searcher.search(True, True, 4)
        scores, maps, _ = searcher.search_exact(True, 4)
        base, flags, _ = searcher.exact_results()
    finally:
        searcher.set_polish_all(0)
    assert np.array_equal(base, pscores) and not flags[:, :200].any()
    same = scores == base
    assert np.array_equal(maps[same], pmaps[same]) and (scores[~same] > base[~same]).all()
    for (q, e), pair in list(pairs.items())[::13]:
        assert flags[q, e] or scores[q, e] == pair.optimum(True)[0]


def test_motifs_from_the_resident_database(db):
    """queries set by set_queries_from_db(..., sses=...) give the rows of the same motifs set from host arrays"""
    entries = [200, 200, 13, 27]
    sses = [[3, 10, 11, 40, 77, 100], [5, 6, 7, 8, 9, 20, 21, 60, 61, 62, 90, 110], None, [0, 2]]
    rows = []
    with sat.Searcher(0) as s:
        s.upload(db)
        for from_db in (True, False):
            if from_db:
                s.set_queries_from_db(entries, 2, sses=sses)
            else:
                s.set_queries(ml.dense_queries(db, entries, sses), 2)
            scores, maps, _ = s.search_exact(True, 2, 1 << 12)
            rows.append((scores, maps) + s.exact_results())
    for a, b in zip(*rows):
        assert np.array_equal(a, b)
    assert rows[0][3].any() and not rows[0][3].all()         # (the 12-SSE motif is not proven at 4096 nodes a row)
