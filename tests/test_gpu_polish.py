"""The polish of the best restarts' maps on the GPU (-m gpu): sat_search_pairs_polish, sat_search_refine_polish and their
multi-GPU forms against the CPU reference (tests/polish_lib.py) bit for bit - scores, base scores, restarts, moves, maps -
on the edge database and on the set-width / cell-layout / 64-lane edges; independence of the forced execution modes and of
the sharding; and the command line's -P against the library."""
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import edge_cases as ec
import matches_lib
import polish_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
SMALL = "tableauxdistmatrixdb.small.ascii"
EDGE_QUERIES = ("EQ001", "EQ002", "EQ008", "EQ033", "EQ064", "EQ097", "EQ111", "EQFAR")     # 1 .. 111 SSEs
NAMES = ("scores", "base scores", "restarts", "moves", "maps")


def load_query(golden_dir, name, index=0):
    qs = sat.StructSet.read(os.path.join(golden_dir, name), "query", skip_header_lines=2)
    t, d = qs.dense(index)
    return t, d, qs.ssetypes(index)


class Reference:
    """The CPU reference of a (database, query batch): the restarts' own bests of a pair are computed once, at the
    largest restart count asked for (restart r is the same stream whatever the count), and shared by the tests."""

    def __init__(self, db, queries, first_ordinal=0):
        self.db, self.queries, self.first = db, queries, first_ordinal
        self.runs, self.pairs = {}, {}

    def restarts(self, q, e, lorder, maxstart):
        key = (q, e, lorder)
        if key not in self.runs or len(self.runs[key][0]) < maxstart:
            self.runs[key] = matches_lib.restarts(self.db, e, self.queries[q], lorder, maxstart, self.first + q)
        sc, mp = self.runs[key]
        return sc[:maxstart], mp[:maxstart]

    def rows(self, q, e, lorder, maxstart, tops):
        """(scores, base, restarts, moves, maps[P, n1max]) of the pairs (q[p], e[p])"""
        n1max = max(len(x[2]) for x in self.queries)
        out = [np.zeros(len(q), np.int32) for _ in range(4)] + [np.full((len(q), n1max), -1, np.int32)]
        for p, (qi, ei) in enumerate(zip(q, e)):
            qi, ei = int(qi), int(ei)
            if (qi, ei) not in self.pairs:
                self.pairs[(qi, ei)] = polish_lib.Pair.of(self.db, ei, self.queries[qi])
            sc, mp = self.restarts(qi, ei, lorder, maxstart)
            got = polish_lib.polish_ranked(self.pairs[(qi, ei)], sc, mp, lorder, tops)
            for k in range(4):
                out[k][p] = got[k]
            out[4][p] = got[4][:n1max]
        return out


def assert_rows_equal(got, want, what=""):
    for k in range(5):
        bad = np.nonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(axis=1))[0]
        assert bad.size == 0, "%s%s differ at pairs %s: gpu %s reference %s" % (what, NAMES[k], bad[:8], got[k][bad[:4]],
                                                                                want[k][bad[:4]])


def run_pairs(db, queries, q, e, tops, lorder, maxstart, first_ordinal=0):
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries, first_ordinal)
        return s.search_pairs_polish(q, e, tops, lorder, maxstart)[:5]


# ---------------------------------------------------------------- the edge database
@pytest.fixture(scope="module")
def edge(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, ec.EDGE_DB))
    queries = []
    for name in EDGE_QUERIES:
        qs = sat.StructSet.read(os.path.join(golden_dir, ec.query_file(name)), "query")
        queries.append((*qs.dense(0), qs.ssetypes(0)))
    assert len(db) == 28 and [len(x[2]) for x in queries] == [1, 2, 8, 33, 64, 97, 111, 40]
    # every query x every entry, then a tenth of the pairs once more, all in a shuffled order
    rng = np.random.default_rng(17)
    q, e = np.divmod(np.arange(len(queries) * len(db)), len(db))
    rep = rng.integers(0, len(q), len(q) // 10)
    q, e = np.concatenate([q, q[rep]]), np.concatenate([e, e[rep]])
    perm = rng.permutation(len(q))
    return db, queries, q[perm].astype(np.int32), e[perm].astype(np.int32), Reference(db, queries)


@pytest.mark.parametrize("lorder", [True, False], ids=["LORDER_T", "LORDER_F"])
@pytest.mark.parametrize("maxstart,tops,part", [(100, 8, 1), (3, 8, 1), (300, 4, 4)], ids=["r100_T8", "r3_T8", "r300_T4"])
def test_edge_database_equals_the_cpu_reference(edge, lorder, maxstart, tops, part):
    """r = 3 < T: the pair's three restarts are all polished; r = 300: the chains' restart loop, on a quarter of the pairs"""
    db, queries, q, e, ref = edge
    q, e = q[::part], e[::part]
    got = run_pairs(db, queries, q, e, tops, lorder, maxstart)
    want = ref.rows(q, e, lorder, maxstart, tops)
    assert_rows_equal(got, want)
    assert (got[0] >= got[1]).all()
    if maxstart >= 100:
        assert (got[3] > 0).any() and (got[0] > got[1]).any(), "the polish moved nothing"
        assert (got[2] != np.array([int(np.argmax(ref.restarts(int(a), int(b), lorder, maxstart)[0])) for a, b in zip(q, e)])).any(), \
            "the winner was rank 0 everywhere"


# ---------------------------------------------------------------- set widths, cell layouts, the 64-lane edge
@pytest.fixture(scope="module")
def width_db():
    """two entries of each of 32, 33, 48, 49, 64, 65, 96, 97 and 111 SSEs (one-, two- and four-word db sets; full and
    triangle cell layouts; one and two trips of the polish kernel's lanes), not in size order; queries of 16, 17, 32"""
    orders = np.array([64, 33, 111, 32, 97, 48, 65, 49, 96, 96, 49, 65, 48, 97, 32, 111, 33, 64], np.int32)
    db = sat.synth.make_db(len(orders), orders=orders, seed=91, sort=False)
    queries = [sat.synth.planted_query(db, 2, keep=16 / 111.0, seed=5), sat.synth.planted_query(db, 0, keep=17 / 64.0, seed=6),
               sat.synth.planted_query(db, 8, keep=32 / 96.0, seed=7)]
    return db, queries, Reference(db, queries, 3)


@pytest.mark.parametrize("lorder", [True, False], ids=["LORDER_T", "LORDER_F"])
def test_set_width_and_lane_edges_equal_the_cpu_reference(width_db, lorder):
    db, queries, ref = width_db
    assert sorted(len(x[2]) for x in queries) == [16, 17, 32]
    q, e = np.divmod(np.arange(len(queries) * len(db), dtype=np.int32), len(db))
    got = run_pairs(db, queries, q, e, 8, lorder, 64, 3)
    assert_rows_equal(got, ref.rows(q, e, lorder, 64, 8))
    assert (got[3] > 0).any()


# ---------------------------------------------------------------- beside the other searches
def test_base_scores_are_search_pairs_and_results_stay(edge):
    db, queries, q, e, _ = edge
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries, 0)
        scores, maps, _ = s.search(True, True, 16)
        ranked = s.topk_hits(5)
        for lorder in (True, False):
            plain, _ = s.search_pairs(q, e, lorder, False, 100)
            got = s.search_pairs_polish(q, e, 4, lorder, 100)
            assert np.array_equal(got[1], plain)
        assert "| select | map pass: sat_sa_pair_match_kernel<" in s.last_launch_info() and s.last_launch_info().endswith(" | polish")
        # the buffers behind results() / topk_hits() still hold the search before the pair calls
        again, again_maps = s.results(True)
        assert np.array_equal(again, scores) and np.array_equal(again_maps, maps)
        assert s.topk_hits(5).tobytes() == ranked.tobytes()
        # bytes: four ints and a map per pair
        before = s.d2h_bytes()
        s.search_pairs_polish(q[:50], e[:50], 8, True, 16)
        assert s.d2h_bytes() - before == 50 * (16 + 111)
        none = s.search_pairs_polish([], [], 3, True, 64)
        assert none[0].shape == (0,) and s.last_launch_info() == ""


def test_bad_arguments_are_rejected(edge):
    db, queries, q, e, _ = edge
    with sat.Searcher(0) as fresh:
        with pytest.raises(sat.SatError, match=r"\[-5\]"):
            fresh.search_pairs_polish([0], [0], 2, True, 16)                     # no database
        fresh.upload(db)
        with pytest.raises(sat.SatError, match=r"\[-5\]"):
            fresh.search_pairs_polish([0], [0], 2, True, 16)                     # no query
        fresh.set_queries(queries, 0)
        for tops in (0, 9, -1):
            with pytest.raises(sat.SatError, match=r"\[-1\]"):
                fresh.search_pairs_polish([0], [0], tops, True, 16)
            with pytest.raises(sat.SatError, match=r"\[-1\]"):
                fresh.search_refine_polish(3, 5, 16, tops, True, False, 16)
        with pytest.raises(sat.SatError, match=r"\[-1\]"):
            fresh.search_pairs_polish([0], [0], 2, True, 0)
        for bq, be in ((len(queries), 0), (-1, 0), (0, len(db)), (0, -1)):
            with pytest.raises(sat.SatError, match="pair 1"):
                fresh.search_pairs_polish([0, bq], [0, be], 2, True, 16)
        # outputs other than the scores may be NULL
        sc = np.zeros(2, np.int32)
        pq, pe = np.array([2, 3], np.int32), np.array([6, 20], np.int32)
        assert fresh._lib.sat_search_pairs_polish(fresh._ctx, 1, 16, 2, 2, pq.ctypes.data, pe.ctypes.data, sc.ctypes.data,
                                                  None, None, None, None, None) == 0
        assert np.array_equal(sc, fresh.search_pairs_polish(pq, pe, 2, True, 16)[0])


@pytest.mark.parametrize("env", [{"SAT_EXP_GENERAL": "1"}, {"SAT_EXP_LPC": "1"}, {"SAT_EXP_EPW": "2"},
                                 {"SAT_EXP_REFINE_SPLIT": "64"}], ids=lambda e: ",".join(f"{k[8:]}={v}" for k, v in e.items()))
def test_forced_execution_modes(monkeypatch, edge, env):
    db, queries, q, e, ref = edge
    q, e = q[::3], e[::3]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for lorder in (True, False):
        assert_rows_equal(run_pairs(db, queries, q, e, 8, lorder, 300 if "SAT_EXP_REFINE_SPLIT" in env else 100),
                          ref.rows(q, e, lorder, 300 if "SAT_EXP_REFINE_SPLIT" in env else 100, 8), str(env) + ": ")


# ---------------------------------------------------------------- refine
def expected_ranking(scores, k):
    """rows by descending score, ties in database order: (entries, scores)"""
    order = np.lexsort((np.arange(len(scores)), -scores.astype(np.int64)))[:k]
    return order, scores[order]


def test_refine_polish_at_the_same_restarts_ranks_the_pair_scores(edge):
    db, queries, _, _, _ = edge
    n, nq = len(db), len(queries)
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries, 0)
        q, e = np.divmod(np.arange(nq * n, dtype=np.int32), n)
        pol = s.search_pairs_polish(q, e, 4, True, 100)
        hits, maps, first, base = s.search_refine_polish(6, n, 100, 4, True, True, 100)
        plain = s.results()[0]
        ref_hits, _, _ = s.search_refine(6, n, 100, True, False, 100)
    sc, bs, mp = pol[0].reshape(nq, n), pol[1].reshape(nq, n), pol[4].reshape(nq, n, -1)
    for b in range(nq):
        order, want = expected_ranking(sc[b], 6)
        assert np.array_equal(hits["entry"][b], order) and np.array_equal(hits["score"][b], want)
        assert np.array_equal(base[b], bs[b][order]) and np.array_equal(first[b], plain[b][order])
        n1 = len(queries[b][2])
        assert np.array_equal(maps[b][:, :mp.shape[-1]], mp[b][order]) and (maps[b][:, n1:] == -1).all()
        # the statistics are the built-in table's: a row whose polish changed nothing is refine's row
        same = {int(h["entry"]): h for h in ref_hits[b]}
        for h in hits[b]:
            if int(h["entry"]) in same and same[int(h["entry"])]["score"] == h["score"]:
                assert h.tobytes() == same[int(h["entry"])].tobytes()
    assert (hits["score"] > base).any()


# ---------------------------------------------------------------- shards
def test_one_two_and_three_shards_on_one_gpu_give_the_same_rows(golden_dir):
    db = sat.synth.make_db(300, 4, 111, sort=True, seed=31)
    qs = [sat.synth.planted_query(db, 280, keep=0.6), load_query(golden_dir, "d2phlb1.input")]
    rng = np.random.default_rng(8)
    q, e = rng.integers(0, 2, 200).astype(np.int32), rng.integers(0, len(db), 200).astype(np.int32)
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(qs, 2)
        ref = s.search_pairs_polish(q, e, 8, True, 128)[:5]
        ref_refine = s.search_refine_polish(10, 40, 256, 4, True, True, 32)
    assert (ref[3] > 0).any()
    for shards in (1, 2, 3):
        with sat.MultiSearcher(shards, devices=[0] * shards) as m:
            m.upload(db)
            m.set_queries(qs, 2)
            assert_rows_equal(m.search_pairs_polish(q, e, 8, True, 128)[:5], ref, "%d shards: " % shards)
            got = m.search_refine_polish(10, 40, 256, 4, True, True, 32)
            with pytest.raises(sat.SatError):
                m.search_pairs_polish([0], [len(db)], 3, True, 64)
        assert got[0].tobytes() == ref_refine[0].tobytes(), "%d shards" % shards
        for a, b in zip(got[1:], ref_refine[1:]):
            assert np.array_equal(a, b), "%d shards" % shards


# ---------------------------------------------------------------- command line
def format_rows(names, n1, hits, maps, lsoln):
    out = []
    for h, mp in zip(hits, maps if lsoln else [None] * len(hits)):
        out.append("%-8s %d %g %g %g\n" % (names[h["entry"]], h["score"], h["norm2"], h["zscore"], h["pvalue"]))
        if lsoln:
            out.extend("%3d %3d\n" % (i + 1, j + 1) for i, j in enumerate(mp[:n1]) if j >= 0)
    return out


@pytest.mark.parametrize("name,args,restarts,cand", [("d2phlb1_TTT", [], 128, 5), ("d2phlb1_TFT", ["-R", "512", "-C", "20"], 512, 20),
                                                     ("multiquery", ["-G", "0,0", "-C", "12"], 128, 12), ("qmode", ["-R", "256"], 256, 5)])
def test_cli_polish_rows_are_the_librarys(golden_dir, name, args, restarts, cand):
    small = sat.StructSet.read(os.path.join(golden_dir, SMALL))
    if name == "qmode":
        picks = [3, 100, 250, 411]
        stdin = "".join(small.names[i] + "\n" for i in picks).encode()
        args = ["-q", SMALL] + args
        queries = [small.dense(i) + (small.ssetypes(i),) for i in picks]
        lorder, lsoln = True, False
    else:
        stdin = open(os.path.join(golden_dir, name + ".input"), "rb").read()
        flags = stdin.decode().splitlines()[1].split()
        lorder, lsoln = flags[1] == "T", flags[2] == "T"
        count = len(sat.StructSet.read(os.path.join(golden_dir, name + ".input"), "query", skip_header_lines=2))
        queries = [load_query(golden_dir, name + ".input", i) for i in range(count)]
    base = subprocess.run([CLI, "-k", "5", *(["-q", SMALL] if name == "qmode" else [])], input=stdin, cwd=golden_dir,
                          capture_output=True, timeout=120)
    p = subprocess.run([CLI, "-P", "4", "-k", "5", *args], input=stdin, cwd=golden_dir, capture_output=True, timeout=120)
    assert base.returncode == 0 and p.returncode == 0, p.stderr.decode()[-400:]
    with sat.Searcher(0) as s:
        s.upload(small)
        s.set_queries(queries, 0)
        hits, maps, _, _ = s.search_refine_polish(5, cand, restarts, 4, lorder, lsoln, 128)
    lines = base.stdout.decode().splitlines(keepends=True)
    heads = [lines[i:i + 3] for i, l in enumerate(lines) if l.startswith("# cudaSaTabsearch")]
    want = []
    for b, (head, query) in enumerate(zip(heads, queries)):
        want += head + ["# POLISH tops = 4 restarts = %d candidates = %d\n" % (restarts, cand)]
        want += format_rows(small.names, len(query[2]), hits[b], maps[b] if lsoln else None, lsoln)
    assert p.stdout.decode() == "".join(want)
    assert len(heads) == len(queries) and p.stdout.count(b"# POLISH") == len(queries)
