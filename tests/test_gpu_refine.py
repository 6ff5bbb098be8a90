"""Pair search and refine on the GPU (-m gpu): sat_search_pairs against sat_search and the CPU oracle, the restart
split and forced layouts, sat_search_refine against its composition from existing calls, the multi-GPU path, the
command line's -R / -C, and the bytes copied back - all bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import _native
import oracle_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
MAXDIM = 111


def load_query(golden_dir, name, index=0):
    qs = sat.StructSet.read(os.path.join(golden_dir, name), "query", skip_header_lines=2)
    t, d = qs.dense(index)
    return t, d, qs.ssetypes(index)


def sub_query(db, src, n1, seed):
    rng = np.random.default_rng(seed)
    t, d = db.dense(src)
    sel = np.sort(rng.choice(int(db.orders[src]), size=n1, replace=False))
    return t[np.ix_(sel, sel)].copy(), d[np.ix_(sel, sel)].copy(), np.diagonal(t)[sel].copy()


@pytest.fixture(scope="module")
def wide_db():
    """Orders uniform on [1, 111]: every db bucket, bit-set width and cell layout."""
    return sat.synth.make_db(230, 1, 111, sort=False, seed=77)


@pytest.fixture(scope="module")
def wide_queries(wide_db):
    """One batch with queries of 8, 19, 32 and 101 SSEs: every query size class."""
    srcs = [int(np.argmax(wide_db.orders >= n)) for n in (8, 19, 32, 101)]
    return [sub_query(wide_db, s, n, seed=s) for s, n in zip(srcs, (8, 19, 32, 101))]


@pytest.fixture(scope="module")
def searcher(wide_db, wide_queries):
    assert sat.device_count() >= 1, "GPU tests need a HIP device (no CPU path exists)"
    s = sat.Searcher(0)
    s.upload(wide_db)
    s.set_queries(wide_queries)
    yield s
    s.close()


def random_pairs(nq, n, count, seed):
    """unsorted, with duplicates"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, nq, count).astype(np.int32)
    e = rng.integers(0, n, count).astype(np.int32)
    dup = rng.integers(0, count, count // 8)
    q = np.concatenate([q, q[dup]])
    e = np.concatenate([e, e[dup]])
    perm = rng.permutation(len(q))
    return q[perm], e[perm]


def assert_pairs_equal_search(s, q, e, lorder, lsoln, maxstart, ref=None):
    if ref is None:
        ref = s.search(lorder, lsoln, maxstart)
    scores, maps = s.search_pairs(q, e, lorder, lsoln, maxstart)
    rs, rm = ref[0], ref[1]
    assert np.array_equal(scores, rs[q, e]), "pair scores differ from sat_search"
    if lsoln:
        assert np.array_equal(maps, rm[q, e]), "pair maps differ from sat_search's LSOLN maps"
    else:
        assert maps is None


# ---------------------------------------------------------------- 1. pairs equal the plain search
@pytest.mark.parametrize("maxstart", [1, 63, 128, 300, 4096])
@pytest.mark.parametrize("lorder,lsoln", [(True, True), (True, False), (False, True), (False, False)])
def test_pairs_equal_the_plain_search(searcher, wide_db, lorder, lsoln, maxstart):
    q, e = random_pairs(4, len(wide_db), 300, seed=maxstart + 7 * lorder + 13 * lsoln)
    assert_pairs_equal_search(searcher, q, e, lorder, lsoln, maxstart)
    info = searcher.last_launch_info()
    assert info.startswith("score pass (%d restarts, " % maxstart) and "sat_sa_pair_kernel<" in info
    assert ("| map pass: " in info) == lsoln


def test_pairs_leave_the_search_buffers_alone(searcher, wide_db):
    ref = searcher.search(True, False, 64)
    q, e = random_pairs(4, len(wide_db), 50, seed=3)
    searcher.search_pairs(q, e, True, True, 256)
    assert np.array_equal(searcher.results()[0], ref[0])


def test_empty_pair_list_and_bad_indices(searcher, wide_db):
    scores, maps = searcher.search_pairs([], [], True, True, 128)
    assert scores.shape == (0,) and maps.shape == (0, MAXDIM)
    with pytest.raises(sat.SatError):
        searcher.search_pairs([4], [0], True, False, 128)
    with pytest.raises(sat.SatError):
        searcher.search_pairs([0], [len(wide_db)], True, False, 128)


# ---------------------------------------------------------------- 2. the split and the layouts do not matter
@pytest.mark.parametrize("env", [{"SAT_EXP_REFINE_SPLIT": "64"}, {"SAT_EXP_REFINE_SPLIT": "256"},
                                 {"SAT_EXP_REFINE_SPLIT": "1000"}, {"SAT_EXP_GENERAL": "1"}, {"SAT_EXP_LPC": "1"},
                                 {"SAT_EXP_EPW": "2"}, {"SAT_EXP_GENERAL": "1", "SAT_EXP_REFINE_SPLIT": "64"}])
def test_split_and_layouts_do_not_change_results(searcher, wide_db, wide_queries, monkeypatch, env):
    maxstart = 1000
    ref = searcher.search(True, True, maxstart)
    q, e = random_pairs(4, len(wide_db), 200, seed=11)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with sat.Searcher(0) as s:          # the overrides are read when a context is created
        s.upload(wide_db)
        s.set_queries(wide_queries)
        assert_pairs_equal_search(s, q, e, True, True, maxstart, ref)
        if "SAT_EXP_REFINE_SPLIT" in env:
            assert s.last_launch_info().startswith("score pass (%d restarts, %s per item)" % (maxstart, env["SAT_EXP_REFINE_SPLIT"]))


# ---------------------------------------------------------------- 3. against the oracle
def test_pairs_equal_the_oracle_at_4096(searcher, wide_db, wide_queries):
    rng = np.random.default_rng(5)
    q = np.array([0, 1, 2] * 5 + [3], np.int32)
    e = rng.integers(0, len(wide_db), len(q)).astype(np.int32)
    scores, maps = searcher.search_pairs(q, e, True, True, 4096)
    for p in range(len(q)):
        qt, qd, qtypes = wide_queries[int(q[p])]
        os_, om, _ = oracle_lib.search(wide_db, qt, qd, qtypes, True, True, 4096, query_ordinal=int(q[p]), entries=[int(e[p])])
        assert scores[p] == os_[0], f"pair {p}"
        assert np.array_equal(maps[p], om[0]), f"map of pair {p}"


# ---------------------------------------------------------------- 4. refine is the composition
def expected_refine(s, k, c, r, big_r, lorder, lsoln):
    """The rows refine must return, from existing calls only: sat_topk_hits at r gives the candidates, a plain
    search at R their scores (and maps), then sort and take the top k; statistics from the host library."""
    host = _native.host_lib()
    n = s.n_entries
    c = min(c, n)
    s.search(lorder, False, r)
    first = s.topk_hits(c)
    stage1 = s.search(lorder, False, r)[0]
    scores, maps, _ = s.search(lorder, lsoln, big_r)
    nq = first.shape[0]
    kk = min(k, c)
    rows = []
    for qi in range(nq):
        cand = first[qi]["entry"]
        order = sorted(cand, key=lambda x: (-int(scores[qi, x]), int(x)))[:kk]
        n1 = s._n1s[qi]
        row = []
        for x in order:
            sc = int(scores[qi, x])
            norm2 = host.sat_norm2(sc, n1, int(s._orders[x]))
            z = host.sat_z_gumbel_trunc(norm2)
            row.append((int(x), sc, norm2, z, host.sat_pv_gumbel(z), int(stage1[qi, x]),
                        maps[qi, x] if lsoln else None))
        rows.append(row)
    return rows


def assert_refine_rows(hits, maps, first, rows):
    for qi, row in enumerate(rows):
        assert [int(h) for h in hits[qi]["entry"]] == [r[0] for r in row]
        assert [int(h) for h in hits[qi]["score"]] == [r[1] for r in row]
        want = np.array([(r[0], r[1], r[2], r[3], r[4]) for r in row], hits.dtype)
        assert hits[qi].tobytes() == want.tobytes(), "norm2 / z / p differ"
        assert [int(f) for f in first[qi]] == [r[5] for r in row]
        if maps is not None:
            assert np.array_equal(maps[qi], np.array([r[6] for r in row]))


@pytest.fixture(scope="module")
def refine_searcher(wide_db, wide_queries):
    s = sat.Searcher(0)
    s.upload(wide_db)
    s.set_queries(wide_queries)
    s._n1s = [len(q[2]) for q in wide_queries]
    s._orders = wide_db.orders
    yield s
    s.close()


@pytest.mark.parametrize("lorder,lsoln", [(True, True), (False, False)])
@pytest.mark.parametrize("cmul", [1, 4, None])
def test_refine_is_the_composition(refine_searcher, wide_db, lorder, lsoln, cmul):
    s, k = refine_searcher, 10
    c = k * cmul if cmul else len(wide_db) + 5
    hits, maps, first = s.search_refine(k, c, 4096, lorder, lsoln, 128)
    assert "|| stage 2: score pass (4096 restarts, " in s.last_launch_info()
    assert hits.shape == (4, k)
    assert_refine_rows(hits, maps, first, expected_refine(s, k, c, 128, 4096, lorder, lsoln))


def test_refine_at_the_same_restarts_is_topk_hits(refine_searcher):
    s = refine_searcher
    hits, maps, first = s.search_refine(10, 40, 128, True, True, 128)
    s.search(True, True, 128)
    ref, rmaps = s.topk_hits(10, lsoln=True)
    assert hits.tobytes() == ref.tobytes()
    assert np.array_equal(maps, rmaps)
    assert np.array_equal(first, ref["score"])


def test_refine_argument_checks(refine_searcher):
    s = refine_searcher
    for args in [(5, 3, 128), (5, 0, 128), (5, 10, 0), (0, 10, 128)]:
        with pytest.raises(sat.SatError):
            s.search_refine(*args)


# ---------------------------------------------------------------- 5. multi-GPU
def test_multi_refine_on_three_shards_equals_one_context(golden_dir):
    db = sat.synth.make_db(700, 4, 70, sort=True, seed=31)
    qs = [sat.synth.planted_query(db, 650, keep=0.6), load_query(golden_dir, "d2phlb1.input"),
          sat.synth.planted_query(db, 230, keep=0.7)]
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(qs, 2)
        ref = s.search_refine(10, 60, 2048, True, True, 64)
    with sat.MultiSearcher(3, devices=[0, 0, 0]) as m:
        m.upload(db)
        m.set_queries(qs, 2)
        begin = m.shards()
        got = m.search_refine(10, 60, 2048, True, True, 64)
        stage1 = m.search_topk(60, True, False, 64)[0]
    # the candidates straddle the shard edges
    shard = np.searchsorted(np.asarray(begin[1:-1]), stage1["entry"], side="right")
    assert len(np.unique(shard)) > 1
    assert ref[0].tobytes() == got[0].tobytes()
    assert np.array_equal(ref[1], got[1]) and np.array_equal(ref[2], got[2])


# ---------------------------------------------------------------- 6. the command line
def _format_rows(names, n1, rows, lsoln):
    out = []
    for entry, score, norm2, z, p, _, mp in rows:
        out.append("%-8s %d %g %g %g\n" % (names[entry], score, norm2, z, p))
        if lsoln:
            out.extend("%3d %3d\n" % (i + 1, j + 1) for i, j in enumerate(mp[:n1]) if j >= 0)
    return out


def _blocks(text):
    """header lines (3 per query) of a -k output"""
    lines = text.splitlines(keepends=True)
    return [lines[i:i + 3] for i, l in enumerate(lines) if l.startswith("# cudaSaTabsearch")]


@pytest.mark.parametrize("name,args", [("d2phlb1_TTT", []), ("d2phlb1_TFT", ["-G", "0,0"]), ("multiquery", []),
                                       ("qmode", [])])
def test_cli_refine_rows(golden_dir, name, args):
    small = sat.StructSet.read(os.path.join(golden_dir, "tableauxdistmatrixdb.small.ascii"))
    if name == "qmode":
        picks = [3, 100, 250, 411]
        stdin = "".join(small.names[i] + "\n" for i in picks).encode()
        args = ["-q", "tableauxdistmatrixdb.small.ascii"] + args
        queries = [small.dense(i) + (small.ssetypes(i),) for i in picks]
        lorder, lsoln = True, False
    else:
        stdin = open(os.path.join(golden_dir, name + ".input"), "rb").read()
        flags = stdin.decode().splitlines()[1].split()
        lorder, lsoln = flags[1] == "T", flags[2] == "T"
        nqf = len(sat.StructSet.read(os.path.join(golden_dir, name + ".input"), "query", skip_header_lines=2))
        queries = [load_query(golden_dir, name + ".input", i) for i in range(nqf)]
    base = subprocess.run([CLI, "-k", "10", *args], input=stdin, cwd=golden_dir, capture_output=True)
    p = subprocess.run([CLI, "-k", "10", "-R", "4096", "-C", "40", *args], input=stdin, cwd=golden_dir, capture_output=True)
    assert base.returncode == 0 and p.returncode == 0, p.stderr.decode()[-400:]
    assert b"refine: stage 2 " in p.stderr and b"40 candidates per query x 4096 restarts" in p.stderr
    with sat.Searcher(0) as s:
        s.upload(small)
        s.set_queries(queries)
        s._n1s = [len(q[2]) for q in queries]
        s._orders = small.orders
        rows = expected_refine(s, 10, 40, 128, 4096, lorder, lsoln)
    want = []
    for head, row, q in zip(_blocks(base.stdout.decode()), rows, queries):
        want += head + _format_rows(small.names, len(q[2]), row, lsoln)
    assert p.stdout.decode() == "".join(want)


# ---------------------------------------------------------------- 7. bytes copied back
def test_refine_copies_back_rows_not_the_database(refine_searcher, wide_db):
    s, nq, k, c = refine_searcher, 4, 10, 40
    for lsoln in (True, False):
        before = s.d2h_bytes()
        s.search_refine(k, c, 512, True, lsoln, 128)
        moved = s.d2h_bytes() - before
        hit = 32 + 4 + (MAXDIM * 4 if lsoln else 0)      # a row, its stage-1 score, its map
        assert moved == nq * k * hit + nq * c * 4          # and the candidate indices
    assert moved < nq * len(wide_db) * 4
