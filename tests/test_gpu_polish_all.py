"""The whole-database polish on the GPU (-m gpu): sat_polish_all_set turns a plain search into a polished one.  Scores,
base scores and maps of every row against the CPU reference (tests/polish_lib.py) bit for bit on the edge database and on
the edges of the lane-group polish kernel, under every forced group width; agreement with sat_search_pairs_polish; the
result calls downstream of the polished buffers; the life of the mode; shards; forced execution modes; the command
line's -P T -A against the library; and every search cut into several launches by a 16 KB scratch budget."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import edge_cases as ec
import matches_lib
import polish_all_lib as pal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
SMALL = "tableauxdistmatrixdb.small.ascii"
EDGE_QUERIES = ("EQ001", "EQ002", "EQ008", "EQ033", "EQ064", "EQ097", "EQ111", "EQFAR")     # 1 .. 111 SSEs


def assert_same(got, want, what=""):
    for name, g, w in zip(("scores", "base scores", "maps"), got, want):
        bad = np.argwhere((g != w).reshape(g.shape[0], g.shape[1], -1).any(axis=2))
        assert bad.size == 0, "%s%s differ at (query, entry) %s: got %s want %s" % (
            what, name, bad[:6].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


# ---------------------------------------------------------------- 1. the edge database
@pytest.fixture(scope="module")
def edge(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, ec.EDGE_DB))
    queries = []
    for name in EDGE_QUERIES:
        qs = sat.StructSet.read(os.path.join(golden_dir, ec.query_file(name)), "query")
        queries.append((*qs.dense(0), qs.ssetypes(0)))
    assert len(db) == 28 and [len(x[2]) for x in queries] == [1, 2, 8, 33, 64, 97, 111, 40]
    return db, queries, pal.Reference(db, queries)


@pytest.mark.parametrize("lorder", [True, False], ids=["LORDER_T", "LORDER_F"])
@pytest.mark.parametrize("maxstart,tops", [(100, 8), (3, 8)], ids=["r100_T8", "r3_T8"])
def test_edge_database_equals_the_cpu_reference(edge, lorder, maxstart, tops):
    """every (query, entry) of the batch; r = 3 < T: the row's three restarts are all polished"""
    db, queries, ref = edge
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries, 0)
        s.set_polish_all(tops)
        assert s.polish_all() == tops
        scores, maps, ms = s.search(lorder, True, maxstart)
        base = s.results_base()
        info = s.last_launch_info()
        s.set_polish_all(0)
        plain, _, _ = s.search(lorder, True, maxstart)
    assert_same((scores, base, maps), ref.all_rows(lorder, maxstart, tops))
    assert np.array_equal(base, plain), "the base scores are not the plain search's"
    assert (scores >= base).all() and ms > 0
    assert info.startswith("polish all (%d tops, 1 launches of up to %d pairs): record pass (" % (tops, len(db) * len(queries)))
    assert info.endswith(" | polish")
    if maxstart >= 100:
        assert (scores > base).any(), "the polish moved nothing"


# ---------------------------------------------------------------- 2. the edges of the lane groups
@pytest.fixture(scope="module")
def group():
    db, queries = pal.group_db()
    return db, queries, pal.Reference(db, queries, pal.GROUP_FIRST), pal.group_rows()


@pytest.mark.parametrize("lorder", [True, False], ids=["LORDER_T", "LORDER_F"])
@pytest.mark.parametrize("tops,maxstart", pal.GROUP_CASES, ids=["T3_r64", "T8_r64", "T8_r2"])
def test_group_edges_equal_the_cpu_reference(group, tops, maxstart, lorder):
    """entries of 1, 2, 15, 16, 16 | 17, 31, 32, 32 | 33, 64, 65 SSEs: neither class fills its waves or workgroups; queries
    whose matched list takes 1, 2, 3 and 7 trips of a 16-lane group"""
    db, queries, ref, rows = group
    key = "T%d_r%d_%s" % (tops, maxstart, "T" if lorder else "F")
    got = (rows[key + "_scores"], rows[key + "_base"], rows[key + "_maps"])
    assert_same(got, ref.all_rows(lorder, maxstart, tops))
    if maxstart >= 64:
        assert (got[0] > got[1]).any()


@pytest.mark.parametrize("width", ["16", "32", "64"])
def test_forced_group_width_gives_the_same_rows(group, tmp_path, width):
    """the override is read when a context is created: a child process per width"""
    rows = group[3]
    out = str(tmp_path / "rows.npz")
    env = dict(os.environ, SAT_EXP_POLISH_GROUP=width)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "polish_all_lib.py"), out], env=env, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-600:]
    forced = np.load(out)
    assert sorted(forced.files) == sorted(rows)
    for name in rows:
        assert np.array_equal(forced[name], rows[name]), "SAT_EXP_POLISH_GROUP=%s: %s differs" % (width, name)


# ---------------------------------------------------------------- 3. the pair route
@pytest.fixture(scope="module")
def synth300():
    db = sat.synth.make_db(300, 8, 32, seed=23, sort=True)
    queries = [sat.synth.planted_query(db, 280, keep=0.6, seed=3), sat.synth.planted_query(db, 120, keep=0.9, seed=4)]
    return db, queries


def test_rows_are_the_pair_searchs(synth300):
    db, queries = synth300
    n, nq = len(db), len(queries)
    q, e = np.divmod(np.arange(nq * n, dtype=np.int32), n)
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries, 1)
        pol = s.search_pairs_polish(q, e, 4, True, 64)
        s.set_polish_all(4)
        scores, maps, _ = s.search(True, True, 64)
        base = s.results_base()
        # without lsoln the maps stay inside
        again, none, _ = s.search(True, False, 64)
        with pytest.raises(sat.SatError, match=r"\[-5\]"):
            s.results(True)
    assert np.array_equal(scores.ravel(), pol[0]) and np.array_equal(base.ravel(), pol[1])
    assert np.array_equal(again, scores) and none is None
    n1max = pol[4].shape[1]
    assert np.array_equal(maps.reshape(nq * n, -1)[:, :n1max], pol[4]) and (maps[:, :, n1max:] == -1).all()
    assert (scores > base).any()


# ---------------------------------------------------------------- 4. downstream of the polished buffers
def downstream(s):
    out = [s.topk_hits(5).tobytes()]
    out += [r.tobytes() for r in s.hits_cutoff(0.05)]
    out += [x.tobytes() for x in s.score_histogram()]
    out.append(s.fit_statistics(0.1).tobytes())
    out += [r.tobytes() for r in s.hits_cutoff(0.05)]
    return out


def test_result_calls_work_on_polished_rows(synth300):
    db, queries = synth300
    with sat.Searcher(0) as s, sat.Searcher(0) as t:
        for x in (s, t):
            x.upload(db)
            x.set_queries(queries, 1)
        s.set_polish_all(4)
        scores, _, _ = s.search(True, False, 64)
        plain, _, _ = t.search(True, False, 64)
        assert not np.array_equal(plain, scores)
        t.debug_set_scores(scores)
        assert downstream(s) == downstream(t)
    # with the best rows only, nothing proportional to the database leaves the GPU
    copied = []
    for n in (100, 300):
        part = sat.synth.make_db(n, 8, 32, seed=23, sort=True)
        with sat.Searcher(0) as s:
            s.upload(part)
            s.set_queries(queries, 1)
            s.set_polish_all(4)
            s.search_async(True, False, 64)
            before = s.d2h_bytes()
            s.topk_hits(5)
            copied.append(s.d2h_bytes() - before)
    assert copied[0] == copied[1]


# ---------------------------------------------------------------- 5. the life of the mode
def test_life_of_the_mode(synth300):
    db, queries = synth300
    n = len(db)
    q, e = np.array([0, 1, 1], np.int32), np.array([7, 280, 33], np.int32)
    with sat.Searcher(0) as s, sat.Searcher(0) as t:
        for x in (s, t):
            x.upload(db)
            x.set_queries(queries, 1)
        want = t.search(True, True, 32)
        with pytest.raises(sat.SatError, match=r"\[-5\]"):
            t.results_base()                                    # a plain search
        for tops in (-1, 9):
            with pytest.raises(sat.SatError, match=r"\[-1\]"):
                s.set_polish_all(tops)
        s.set_polish_all(2)
        # it survives an upload and a new batch
        s.upload(db)
        s.set_queries(queries, 1)
        assert s.polish_all() == 2
        pol = s.search(True, True, 32)
        assert (pol[0] >= want[0]).all() and (pol[0] > want[0]).any()
        assert np.array_equal(s.results_base(), want[0])
        s.upload_search(db, True, False, 32)
        assert np.array_equal(s.results()[0], pol[0]) and np.array_equal(s.results_base(), want[0])
        # what the mode does not touch
        with pytest.raises(sat.SatError, match=r"\[-5\]"):
            s.search_timed(True, False, 32)
        for call in (lambda x: x.search_matches(2, True, 32)[:4], lambda x: x.search_pairs(q, e, True, True, 32),
                     lambda x: x.search_pairs_polish(q, e, 2, True, 32)[:5], lambda x: x.search_refine(4, 10, 64, True, True, 32)):
            for a, b in zip(call(s), call(t)):
                assert a.tobytes() == b.tobytes()
        # off again: the plain search bit for bit
        s.set_polish_all(0)
        assert s.polish_all() == 0
        off = s.search(True, True, 32)
        assert np.array_equal(off[0], want[0]) and np.array_equal(off[1], want[1])
        with pytest.raises(sat.SatError, match=r"\[-5\]"):
            s.results_base()
        assert s.search_timed(True, False, 32) is not None
    with sat.MultiSearcher(2, devices=[0, 0]) as m, sat.MultiSearcher(2, devices=[0, 0]) as plain:
        for x in (m, plain):
            x.upload(db)
            x.set_queries(queries, 1)
        m.set_polish_all(2)
        for a, b in zip(m.search_refine(4, 10, 64, True, True, 32), plain.search_refine(4, 10, 64, True, True, 32)):
            assert a.tobytes() == b.tobytes()
    assert n == 300


# ---------------------------------------------------------------- 6. shards
def test_one_two_and_three_shards_on_one_gpu_give_the_same_rows(synth300):
    db, queries = synth300
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries, 1)
        s.set_polish_all(4)
        scores, maps, _ = s.search(True, True, 64)
        top, top_maps = s.topk_hits(5, True)
        cut, cut_maps = s.hits_cutoff(0.05, None, True)
        fits = s.fit_statistics(0.1)
        fitted = s.hits_cutoff(0.05)
    for shards in (1, 2, 3):
        what = "%d shards" % shards
        with sat.MultiSearcher(shards, devices=[0] * shards) as m:
            m.upload(db)
            m.set_queries(queries, 1)
            m.set_polish_all(4)
            got = m.search(True, True, 64)
            assert np.array_equal(got[0], scores) and np.array_equal(got[1], maps), what
            got = m.search_topk(5, True, True, 64)
            assert got[0].tobytes() == top.tobytes() and np.array_equal(got[1], top_maps), what
            got = m.search_cutoff(0.05, None, True, True, 64)
            for b in range(len(queries)):
                assert got[0][b].tobytes() == cut[b].tobytes() and np.array_equal(got[1][b], cut_maps[b]), what
            got = m.search_fit(0.1, True, False, 64)[0]
            assert got.tobytes() == fits.tobytes(), what
            for a, b in zip(m.hits_cutoff(0.05), fitted):
                assert a.tobytes() == b.tobytes(), what


# ---------------------------------------------------------------- 7. forced execution modes
@pytest.mark.parametrize("env", [{"SAT_EXP_GENERAL": "1"}, {"SAT_EXP_LPC": "1"}, {"SAT_EXP_EPW": "2"},
                                 {"SAT_EXP_REFINE_SPLIT": "64"}], ids=lambda e: ",".join(f"{k[8:]}={v}" for k, v in e.items()))
def test_forced_execution_modes(monkeypatch, group, env):
    db, queries, ref, rows = group
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for lorder in (True, False):
        key = "T8_r64_%s" % ("T" if lorder else "F")
        got = pal.polished(db, queries, 8, lorder, 64, pal.GROUP_FIRST)
        assert_same(got, (rows[key + "_scores"], rows[key + "_base"], rows[key + "_maps"]), str(env) + ": ")


# ---------------------------------------------------------------- 8. command line
def format_rows(names, n1, hits, maps, lsoln):
    out = []
    for h, mp in zip(hits, maps if lsoln else [None] * len(hits)):
        out.append("%-8s %d %g %g %g\n" % (names[h["entry"]], h["score"], h["norm2"], h["zscore"], h["pvalue"]))
        if lsoln:
            out.extend("%3d %3d\n" % (i + 1, j + 1) for i, j in enumerate(mp[:n1]) if j >= 0)
    return out


def load_query(golden_dir, name, index=0):
    qs = sat.StructSet.read(os.path.join(golden_dir, name), "query", skip_header_lines=2)
    t, d = qs.dense(index)
    return t, d, qs.ssetypes(index)


def gumbel_line(f):
    if not f["fitted"]:
        return "# GUMBEL not fitted\n"
    return "# GUMBEL a = %.17g b = %.17g rows = %d censored = %d below = %d\n" % (f["a"], f["b"], f["rows"], f["censored"], f["below"])


@pytest.mark.parametrize("name,args", [("d2phlb1_TTT", []), ("d2phlb1_TTT", ["-k", "5"]), ("d2phlb1_TFT", ["-p", "0.05"]),
                                       ("d2phlb1_TTT", ["-F", "0.1", "-k", "5"]), ("multiquery", ["-G", "0,0"]), ("qmode", [])],
                         ids=["listing", "k5", "p0.05", "F0.1_k5", "G00", "qmode"])
def test_cli_all_rows_are_the_librarys(golden_dir, name, args):
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
    plain_args = [a for a in args if a not in ("-F", "0.1")]
    base = subprocess.run([CLI, *plain_args], input=stdin, cwd=golden_dir, capture_output=True, timeout=120)
    p = subprocess.run([CLI, "-P", "4", "-A", *args], input=stdin, cwd=golden_dir, capture_output=True, timeout=120)
    assert base.returncode == 0 and p.returncode == 0, p.stderr.decode()[-400:]
    with sat.Searcher(0) as s:
        s.upload(small)
        s.set_queries(queries, 0)
        s.set_polish_all(4)
        s.search_async(lorder, lsoln, 128)
        fits = s.fit_statistics(0.1) if "-F" in args else None
        if "-p" in args:
            got = s.hits_cutoff(0.05, None, lsoln)
            hits, maps = got if lsoln else (got, None)
        elif "-F" in args:
            got = s.hits_cutoff(1.0, 5, lsoln)
            hits, maps = got if lsoln else (got, None)
        elif "-k" in args:
            got = s.topk_hits(5, lsoln)
            hits, maps = got if lsoln else (got, None)
        else:
            got = s.topk_hits(len(small), lsoln)                 # every row with its statistics; the listing is in database order
            hits, maps = got if lsoln else (got, None)
            order = [np.argsort(h["entry"], kind="stable") for h in hits]
            hits = [h[o] for h, o in zip(hits, order)]
            maps = [m[o] for m, o in zip(maps, order)] if lsoln else None
    lines = base.stdout.decode().splitlines(keepends=True)
    heads = [lines[i:i + 3] for i, l in enumerate(lines) if l.startswith("# cudaSaTabsearch")]
    assert len(heads) == len(queries)
    want = []
    for b, (head, query) in enumerate(zip(heads, queries)):
        want += head + ["# POLISH tops = 4 all rows\n"]
        if fits is not None:
            want.append(gumbel_line(fits[b]))
        want += format_rows(small.names, len(query[2]), hits[b], maps[b] if lsoln else None, lsoln)
    assert p.stdout.decode() == "".join(want)
    assert p.stdout.count(b"# POLISH") == len(queries)


# ---------------------------------------------------------------- 9. the cut paths
CUT_KB = 16


@pytest.fixture(scope="module")
def cut_pairs(group):
    """all 60 (query, entry) pairs of the group database, shuffled"""
    db, queries = group[0], group[1]
    q, e = np.divmod(np.random.default_rng(9).permutation(len(queries) * len(db)).astype(np.int32), np.int32(len(db)))
    return q, e


@pytest.mark.parametrize("lorder", [True, False], ids=["LORDER_T", "LORDER_F"])
def test_a_16_kb_scratch_budget_cuts_every_search_and_changes_no_result(monkeypatch, group, cut_pairs, lorder):
    """SAT_EXP_SCRATCH_KB = 16 leaves 16384 / 4 = 4096 words of scratch: every search of the group database (12 entries of
    up to 65 SSEs, queries of 1, 16, 17, 33 and 111 SSEs, 64 restarts) is cut into several launches, and every row still
    equals the CPU reference.

    * Record slabs of a pair-match / polish list.  The list's largest entry has 65 SSEs, satk::set_words(65) = 4, so a
      pair's slab is (1 + 4) x 64 restarts = 320 words and 4096 / 320 = 12 pairs fit: the 60 rows of the polished
      search are 5 launches of 12 (each the one launch of its own pair-match plan: both in the launch string), the 60 shuffled
      pairs of search_pairs_matches 5 launches of 12 with SatPairItem::slab counted from each launch's first pair.
    * Map pass of the pair modes: min(16 KB, 256 MB) = 4096 words.  A best-map slab is ceil(n1max / 4) words x 64 chains
      (1, 3 or 8 restarts per item size the workgroup for 64): 256 words for the class of the 1- and 16-SSE queries,
      320 for 17 SSEs, 576 for 33, 1792 for 111 - at most 16, 12, 7 and 2 items per launch.  The 111-SSE query meets the
      5 entries of up to 16 SSEs in one item group: launches of 2, 2 and 1 items, in search_pairs and in the polished
      search's launch of that query.
    * LSOLN slabs of the plain search.  Four query classes, each one launch of the 12 entries, on four lanes of
      4096 / 4 = 1024 words: 1024 / 256 = 4 workgroups = 2 entries x 2 queries, 1024 / 320 = 3 entries, 1024 / 576 = 1
      entry, and below one slab of 1792 words the floor of 1 entry: 6 + 4 + 12 + 12 launches."""
    db, queries, ref, _ = group
    q, e = cut_pairs
    n, nq, npairs = len(db), len(queries), len(q)
    assert n == 12 and nq == 5 and npairs == 60
    monkeypatch.setenv("SAT_EXP_SCRATCH_KB", str(CUT_KB))              # read when the context is created
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries, pal.GROUP_FIRST)
        s.set_polish_all(8)
        scores, maps, _ = s.search(lorder, True, 64)
        base, info_all = s.results_base(), s.last_launch_info()
        s.set_polish_all(0)
        counts, mscores, mrestarts, mmaps, _ = s.search_pairs_matches(q, e, 3, lorder, 64)
        info_matches = s.last_launch_info()
        pscores, pmaps = s.search_pairs(q, e, lorder, True, 64)
        plain, plain_maps, _ = s.search(lorder, True, 64)
    # 1. the polished search
    assert_same((scores, base, maps), ref.all_rows(lorder, 64, 8), "polished search: ")
    assert info_all.startswith("polish all (8 tops, 5 launches of up to 12 pairs): record pass (64 restarts, "), info_all
    assert ", 1 launches of up to 12 pairs): " in info_all, info_all      # each of the 5 is one launch of its own plan
    # 2. search_pairs_matches; 3. search_pairs; 4. the plain search: slot 0 of the selection is the best restart
    assert "5 launches of up to 12 pairs): " in info_matches, info_matches
    for p in range(npairs):
        n1 = len(queries[q[p]][2])
        c, sc, rs, mp = matches_lib.select_matches(*ref.restarts(int(q[p]), int(e[p]), lorder, 64), 3)
        what = "pair %d (query %d, entry %d)" % (p, q[p], e[p])
        got = (int(counts[p]), list(mscores[p]), list(mrestarts[p]))
        assert got == (c, list(sc), list(rs)), "%s: gpu %s reference %s" % (what, got, (c, list(sc), list(rs)))
        assert np.array_equal(mmaps[p, :, :n1], mp[:, :n1]) and (mmaps[p, :, n1:] == -1).all(), what + ": match maps"
        assert pscores[p] == sc[0] and plain[q[p], e[p]] == sc[0], what + ": best score"
        for name, got_map in (("search_pairs", pmaps[p]), ("search", plain_maps[q[p], e[p]])):
            assert np.array_equal(got_map[:n1], mp[0, :n1]) and (got_map[n1:] == -1).all(), "%s: map of %s" % (what, name)
