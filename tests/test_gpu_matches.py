"""Several matches per entry on the GPU (-m gpu): sat_search_matches / sat_multi_search_matches against sat_search
(match 0) and against the single-chain CPU reference with the greedy rule (tests/matches_lib.py), bit for bit, over
every size class, query batches, forced execution layouts and the command line's -m."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import matches_lib
import oracle_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
M = 8


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
def searcher():
    assert sat.device_count() >= 1, "GPU tests need a HIP device (no CPU path exists)"
    s = sat.Searcher(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def small_db(golden_dir):
    return sat.StructSet.read(os.path.join(golden_dir, "tableauxdistmatrixdb.small.ascii"))


@pytest.fixture(scope="module")
def wide_db():
    """Orders uniform on [1, 111]: every db bucket, bit-set width and cell layout."""
    return sat.synth.make_db(230, 1, 111, sort=False, seed=77)


def assert_match0_is_search(s, lorder, maxstart, counts, scores, maps):
    ref, refmaps, _ = s.search(lorder, True, maxstart)
    ref = ref.reshape(counts.shape)
    refmaps = refmaps.reshape(counts.shape + (refmaps.shape[-1],))
    assert (counts >= 1).all() and (counts <= scores.shape[-1]).all()
    assert np.array_equal(scores[..., 0], ref), "match 0 scores differ from sat_search"
    n = maps.shape[-1]
    assert np.array_equal(maps[..., 0, :], refmaps[..., :n]), "match 0 maps differ from sat_search's LSOLN maps"


def assert_equals_reference(db, q, lorder, maxstart, entries, counts, scores, restarts, maps, query_ordinal=0):
    """counts / scores / restarts / maps of the sampled entries equal select_matches() over the chain oracle."""
    n1 = len(q[2])
    mm = scores.shape[-1]
    for e in entries:
        c, sc, rs, mp = matches_lib.matches(db, int(e), q, lorder, maxstart, mm, query_ordinal)
        got = (int(counts[e]), list(scores[e]), list(restarts[e]))
        assert got == (c, list(sc), list(rs)), f"entry {e}: gpu {got} reference {(c, list(sc), list(rs))}"
        assert np.array_equal(maps[e, :, :n1], mp[:, :n1]), f"maps of entry {e}"


# ---------------------------------------------------------------- match 0 is sat_search
@pytest.mark.parametrize("qfile,lorder", [("d1ubia_.input", True), ("d2phlb1.input", True), ("d2phlb1.input", False),
                                          ("d1twfa_.input", True)])
@pytest.mark.parametrize("maxstart", [1, 7, 128, 300])
def test_match0_is_the_plain_search_on_the_small_db(searcher, small_db, golden_dir, qfile, lorder, maxstart):
    searcher.upload(small_db)
    searcher.set_query(*load_query(golden_dir, qfile))
    counts, scores, restarts, maps, _ = searcher.search_matches(4, lorder, maxstart)
    assert_match0_is_search(searcher, lorder, maxstart, counts[0], scores[0], maps[0])
    assert ((restarts[0] >= 0) == (np.arange(4)[None, :] < counts[0][:, None])).all()


@pytest.mark.parametrize("n1", [1, 5, 8, 17, 32, 33, 64, 65, 101, 111])
def test_every_size_class_equals_the_reference(searcher, wide_db, n1):
    searcher.upload(wide_db)
    rng = np.random.default_rng(n1)
    src = int(rng.choice(np.nonzero(wide_db.orders >= n1)[0]))
    q = sub_query(wide_db, src, n1, n1)
    searcher.set_query(*q)
    for lorder in (True, False):
        counts, scores, restarts, maps, _ = searcher.search_matches(M, lorder, 128)
        assert_match0_is_search(searcher, lorder, 128, counts[0], scores[0], maps[0])
        if n1 in (8, 32, 101):
            entries = np.arange(n1 % 7, len(wide_db), 29)
            assert_equals_reference(wide_db, q, lorder, 128, entries, counts[0], scores[0], restarts[0], maps[0])


def test_query_batch(searcher, wide_db):
    searcher.upload(wide_db)
    qs = [sub_query(wide_db, int(np.nonzero(wide_db.orders >= n1)[0][0]), n1, 3 + n1) for n1 in (8, 40, 101, 13)]
    searcher.set_queries(qs, 5)
    counts, scores, restarts, maps, _ = searcher.search_matches(M, True, 64)
    assert maps.shape == (4, len(wide_db), M, 101)
    assert_match0_is_search(searcher, True, 64, counts, scores, maps)
    entries = np.arange(2, len(wide_db), 37)
    for qi, q in enumerate(qs):
        assert_equals_reference(wide_db, q, True, 64, entries, counts[qi], scores[qi], restarts[qi], maps[qi], 5 + qi)


@pytest.mark.parametrize("env", [{"SAT_EXP_LPC": "0", "SAT_EXP_COMPACT": "0"}, {"SAT_EXP_LPC": "0", "SAT_EXP_COMPACT": "1"},
                                 {"SAT_EXP_LPC": "1", "SAT_EXP_COMPACT": "1"}, {"SAT_EXP_LPC": "2", "SAT_EXP_COMPACT": "1"},
                                 {"SAT_EXP_LPC": "2", "SAT_EXP_COMPACT": "0"}, {"SAT_EXP_QLDS": "1"},
                                 {"SAT_EXP_EPW": "2"}, {"SAT_EXP_EPW": "3"}, {"SAT_EXP_CHAINS": "64"}],
                         ids=lambda e: ",".join(f"{k[8:]}={v}" for k, v in e.items()))
def test_forced_execution_modes(monkeypatch, env):
    """Lanes per chain, compaction, query cells in LDS, entries per workgroup, chains per slot: results unchanged."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    db = sat.synth.make_db(151, 6, 40, seed=21)
    big = sat.synth.make_db(23, 70, 111, sort=True, seed=34)
    with sat.Searcher(0) as s:
        for d, src, keep in ((db, 140, 0.8), (big, 20, 0.6)):
            s.upload(d)
            q = sat.synth.planted_query(d, src, keep=keep)
            s.set_query(*q)
            for lorder, r in ((True, 128), (False, 100)):
                counts, scores, restarts, maps, _ = s.search_matches(M, lorder, r)
                assert_match0_is_search(s, lorder, r, counts[0], scores[0], maps[0])
                assert_equals_reference(d, q, lorder, r, np.arange(1, len(d), 11), counts[0], scores[0], restarts[0], maps[0])


def test_many_restarts(searcher, small_db, golden_dir):
    searcher.upload(small_db)
    q = load_query(golden_dir, "d2phlb1.input")
    searcher.set_query(*q)
    counts, scores, restarts, maps, _ = searcher.search_matches(M, True, 4096)
    assert_equals_reference(small_db, q, True, 4096, [3, 200], counts[0], scores[0], restarts[0], maps[0])
    assert_match0_is_search(searcher, True, 4096, counts[0], scores[0], maps[0])


# ---------------------------------------------------------------- properties at scale
def test_properties_on_a_large_mixed_database(searcher):
    db = sat.synth.make_db(20000, 4, 111, sort=True, seed=8)
    searcher.upload(db)
    q = sat.synth.planted_query(db, 15000, keep=0.4)
    qt, qd, qtypes = q
    n1 = len(qtypes)
    searcher.set_query(*q)
    for lorder in (True, False):
        counts, scores, restarts, maps, _ = searcher.search_matches(M, lorder, 128)
        c, s, r, m = counts[0], scores[0], restarts[0], maps[0]
        used = np.arange(M)[None, :] < c[:, None]
        assert (s[~used] == 0).all() and (r[~used] == -1).all() and (m[~used] == -1).all()
        assert (np.diff(s, axis=1)[used[:, 1:]] <= 0).all(), "scores must not increase"
        assert (s[:, 1:][used[:, 1:]] > 0).all()
        qt_c, qd_c, qty_c = (np.ascontiguousarray(qt, np.uint8), np.ascontiguousarray(qd, np.float32),
                             np.ascontiguousarray(qtypes, np.uint8))
        ql = oracle_lib._Query(n1, qt_c.shape[1], qt_c.ctypes.data, qd_c.ctypes.data, qty_c.ctypes.data)
        full = oracle_lib.lib().sa_oracle_full_score
        full.restype = C.c_int
        full.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        multi = np.nonzero(c >= 2)[0]
        check = np.union1d(multi, np.arange(0, len(db), 97))
        for e in check:
            t, d = db.dense(int(e))
            t, d = np.ascontiguousarray(t, np.uint8), np.ascontiguousarray(d, np.float32)
            types2 = np.diagonal(t)
            seen = set()
            for k in range(int(c[e])):
                mp = m[e, k, :n1].astype(np.int32)
                js = mp[mp >= 0]
                assert len(set(js.tolist())) == len(js), f"entry {e} match {k} not injective"
                assert (types2[js] == qtypes[mp >= 0]).all(), f"entry {e} match {k} breaks types"
                if lorder:
                    assert (np.diff(js) > 0).all(), f"entry {e} match {k} breaks the order"
                assert seen.isdisjoint(js.tolist()), f"entry {e} match {k} overlaps an earlier match"
                seen |= set(js.tolist())
                mc = np.ascontiguousarray(mp)
                fs = full(C.byref(ql), t.ctypes.data, d.ctypes.data, t.shape[1], mc.ctypes.data)
                assert fs == s[e, k], f"entry {e} match {k}: full score {fs} != {s[e, k]}"
        c2, s2, r2, m2, _ = searcher.search_matches(M, lorder, 128, maps=False)
        assert m2 is None
        assert np.array_equal(c2, counts) and np.array_equal(s2, scores) and np.array_equal(r2, restarts)
        assert multi.size > 0


# ---------------------------------------------------------------- API edges, multi, CLI
def test_one_match_and_bad_counts(searcher, small_db, golden_dir):
    searcher.upload(small_db)
    searcher.set_query(*load_query(golden_dir, "d2phlb1.input"))
    counts, scores, restarts, maps, _ = searcher.search_matches(1, True, 128)
    assert (counts == 1).all()
    assert_match0_is_search(searcher, True, 128, counts[0], scores[0], maps[0])
    lib = searcher._lib
    n = len(small_db)
    bufs = [np.zeros(n * 9, np.int32) for _ in range(3)]
    for bad in (0, 9):
        rc = lib.sat_search_matches(searcher._ctx, 1, 128, bad, bufs[0].ctypes.data, bufs[1].ctypes.data,
                                    bufs[2].ctypes.data, None, None)
        assert rc == -1, f"max_matches={bad}: {rc}"
    rc = lib.sat_search_matches(searcher._ctx, 1, 0, 2, bufs[0].ctypes.data, bufs[1].ctypes.data, bufs[2].ctypes.data,
                                None, None)
    assert rc == -1


def test_buffers_follow_rows_and_matches_separately(small_db, golden_dir):
    """The output buffers are sized per kind: a call with a large M over one query, then a small M over more queries
    (more rows, fewer row x M slots) must get count buffers that hold every row - results as the reference's."""
    qs = [load_query(golden_dir, "d2phlb1.input"), load_query(golden_dir, "d1ubia_.input"),
          load_query(golden_dir, "multiquery.input", 0), load_query(golden_dir, "multiquery.input", 2)]
    with sat.Searcher(0) as s:
        s.upload(small_db)
        s.set_query(*qs[0])
        s.search_matches(8, True, 64)
        s.set_queries(qs, 0)
        counts, scores, restarts, maps, _ = s.search_matches(2, True, 64)
        assert_match0_is_search(s, True, 64, counts, scores, maps)
        entries = np.arange(0, len(small_db), 53)
        for qi, q in enumerate(qs):
            assert_equals_reference(small_db, q, True, 64, entries, counts[qi], scores[qi], restarts[qi], maps[qi], qi)
        # fewer rows again, with more slots per row and no maps
        s.set_query(*qs[1])
        c1, s1, r1, m1, _ = s.search_matches(8, True, 64, maps=False)
        c2, s2, r2, m2, _ = s.search_matches(8, True, 64)
        assert m1 is None and np.array_equal(c1, c2) and np.array_equal(s1, s2) and np.array_equal(r1, r2)
        assert_equals_reference(small_db, qs[1], True, 64, entries, c2[0], s2[0], r2[0], m2[0])


def test_launch_info_names_both_passes(searcher, small_db, golden_dir):
    searcher.upload(small_db)
    searcher.set_query(*load_query(golden_dir, "d2phlb1.input"))
    searcher.search_matches(3, True, 128)
    info = searcher.last_launch_info()
    assert info.startswith("record pass: sat_sa_match_kernel<") and " | replay pass: sat_sa_match_kernel<" in info
    searcher.search_matches(3, True, 128, maps=False)
    info = searcher.last_launch_info()
    assert info.startswith("record pass: sat_sa_match_kernel<") and "replay" not in info


def test_multi_shards_on_one_gpu_equal_one_context(golden_dir):
    db = sat.synth.make_db(700, 4, 70, sort=True, seed=31)
    qs = [sat.synth.planted_query(db, 650, keep=0.6), load_query(golden_dir, "d2phlb1.input")]
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(qs, 2)
        ref = s.search_matches(M, True, 64)
    with sat.MultiSearcher(3, devices=[0, 0, 0]) as m:
        m.upload(db)
        m.set_queries(qs, 2)
        got = m.search_matches(M, True, 64)
    for a, b in zip(ref[:4], got[:4]):
        assert np.array_equal(a, b)


def _strip_more_matches(text):
    """The output without the name:k rows and the map lines under them; and those rows as {(name, k): score}."""
    kept, extra, skipping = [], {}, False
    for line in text.splitlines(keepends=True):
        first = line.split()[0] if line.strip() else ""
        is_map = line[:1] in (" ", "") or first.isdigit()
        if line.startswith("#") or not is_map:
            skipping = False
            name = first
            if ":" in name and not line.startswith("#"):
                base, k = name.rsplit(":", 1)
                extra[(base, int(k))] = int(line.split()[1])
                skipping = True
                continue
        if not skipping:
            kept.append(line)
    return "".join(kept), extra


def _assert_mixed_matches(text, db, picks):
    """-m 3 over both size classes, two queries: each (query, class) block's name:k rows are exactly search_matches'
    matches 2..count of that class's entries, each with its LSOLN map lines; the large class's come in the deferred
    blocks after every query's small-class block, with that pass's two blanks before the p-value."""
    qs = db.subset(picks)
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries([(*qs.dense(q), qs.ssetypes(q)) for q in range(len(picks))])
        counts, scores, _, maps, _ = s.search_matches(3, True, 64)
    blocks = text.split("# cudaSaTabsearch")[1:]
    assert len(blocks) == 2 * len(picks)
    large_rows = 0
    for b, block in enumerate(blocks):
        q, large = b % len(picks), b >= len(picks)
        n1 = int(qs.orders[q])
        row = re.compile(r"^\S+:\d -?\d+ \S+ \S+%s\S+$" % ("  " if large else " "))
        got, cur = {}, None
        for line in block.splitlines()[3:]:
            if line[:1] == " " or line.split()[0].isdigit():           # a map line
                if cur:
                    got[cur].append(tuple(int(v) for v in line.split()))
                continue
            cur = None
            if ":" in line.split()[0]:
                assert row.match(line), line
                base, k = line.split()[0].rsplit(":", 1)
                cur = (base, int(k), int(line.split()[1]))
                got[cur] = []
        want = {}
        for e in np.nonzero((db.orders > 96) == large)[0]:
            for k in range(1, int(counts[q, e])):
                m = maps[q, e, k, :n1]
                want[(db.names[e], k + 1, int(scores[q, e, k]))] = [(i + 1, int(m[i]) + 1) for i in range(n1) if m[i] >= 0]
        assert got == want, (q, large)
        large_rows += len(want) if large else 0
    assert large_rows, "no large-class entry had a second match"


@pytest.mark.parametrize("name,args", [("d2phlb1_TTT", []), ("d2phlb1_TFT", []), ("d2phlb1_TTT", ["-k", "400"]), ("multiquery", ["-G", "0,0,0"]),
                                       ("mixed", [])])
def test_cli_more_matches(golden_dir, small_db, tmp_path, name, args):
    cwd = golden_dir
    if name == "mixed":
        # both size classes, inline LSOLN queries (-q would turn LSOLN off): one query from each class
        db = sat.synth.make_db(60, 70, 111, sort=False, seed=11)
        assert (db.orders > 96).sum() > 3 and (db.orders <= 96).sum() > 3
        sat.synth.write_ascii(db, tmp_path / "mix.ascii")
        picks = [int(np.argmax(db.orders <= 96)), int(np.argmax(db.orders > 96))]
        db.subset(picks).write_ascii(tmp_path / "q.body")
        stdin, cwd = b"mix.ascii\nT T T\n" + (tmp_path / "q.body").read_bytes(), str(tmp_path)
    else:
        stdin = open(os.path.join(golden_dir, name + ".input"), "rb").read()
    base = subprocess.run([CLI, "-r", "64", *args], input=stdin, cwd=cwd, capture_output=True)
    more = subprocess.run([CLI, "-r", "64", "-m", "3", *args], input=stdin, cwd=cwd, capture_output=True)
    assert base.returncode == 0 and more.returncode == 0, more.stderr.decode()[-400:]
    kept, extra = _strip_more_matches(more.stdout.decode())
    assert kept == base.stdout.decode()
    assert extra, "no entry had a second match"
    if name == "mixed":
        _assert_mixed_matches(more.stdout.decode(), db, picks)
    if name in ("multiquery", "mixed"):
        return
    lines = stdin.decode().splitlines()
    lorder = lines[1].split()[1] == "T"
    with sat.Searcher(0) as s:
        s.upload(small_db)
        s.set_query(*load_query(golden_dir, name + ".input"))
        counts, scores, _, _, _ = s.search_matches(3, lorder, 64, maps=False)
    index = {n: i for i, n in enumerate(small_db.names)}
    want = {}
    for e in range(len(small_db)):
        for k in range(1, int(counts[0, e])):
            want[(small_db.names[e], k + 1)] = int(scores[0, e, k])
    if args[:1] == ["-k"]:
        assert all(want[key] == v for key, v in extra.items()) and all(key[0] in index for key in extra)
    else:
        assert extra == want
