"""Matches of chosen (query, entry) pairs on the GPU (-m gpu): sat_search_pairs_matches / sat_multi_search_pairs_matches
against the single-chain CPU reference with the greedy rule (tests/matches_lib.py) and against the rows of the
whole-database call sat_search_matches, bit for bit; independence of the cut into items, the forced layouts and the cut
into calls; the bytes copied; shards; and the command line's -M against -m and against the library."""
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import matches_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
SMALL = "tableauxdistmatrixdb.small.ascii"
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
def searcher():
    assert sat.device_count() >= 1, "GPU tests need a HIP device (no CPU path exists)"
    s = sat.Searcher(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def small_db(golden_dir):
    return sat.StructSet.read(os.path.join(golden_dir, SMALL))


@pytest.fixture(scope="module")
def wide_db():
    """Orders uniform on [1, 111]: every db bucket, bit-set width and cell layout."""
    return sat.synth.make_db(230, 1, 111, sort=False, seed=77)


def wide_queries(db):
    """one query of every size class (16, 32, 64, 112), not in class order"""
    return [sub_query(db, int(np.nonzero(db.orders >= n1)[0][0]), n1, 3 + n1) for n1 in (8, 40, 101, 13, 30)]


def shuffled_pairs(nq, n, count, seed):
    """`count` pairs over all queries and entries in random order, a tenth of them repeated"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, nq, count)
    e = rng.integers(0, n, count)
    rep = rng.integers(0, count, max(count // 10, 1))
    q, e = np.concatenate([q, q[rep]]), np.concatenate([e, e[rep]])
    perm = rng.permutation(len(q))
    return q[perm].astype(np.int32), e[perm].astype(np.int32)


def assert_rows_of(whole, q, e, got, maps=True):
    """got = search_pairs_matches' arrays equal rows (q[p], e[p]) of search_matches' arrays `whole`"""
    names = ("counts", "scores", "restarts", "maps")
    for k in range(4 if maps else 3):
        assert np.array_equal(got[k], whole[k][q, e]), names[k]
    if not maps:
        assert got[3] is None


# ---------------------------------------------------------------- against the CPU reference
@pytest.mark.parametrize("lorder", [True, False])
def test_equals_the_cpu_reference(searcher, small_db, golden_dir, lorder):
    qs = [load_query(golden_dir, "d1ubia_.input"), load_query(golden_dir, "d2phlb1.input"),
          load_query(golden_dir, "d1twfa_.input")]
    searcher.upload(small_db)
    searcher.set_queries(qs, 4)
    rng = np.random.default_rng(5 + lorder)
    e = rng.choice(len(small_db), 36, replace=False).astype(np.int32)           # drawn from all 586 entries
    q = (np.arange(len(e)) % len(qs)).astype(np.int32)
    counts, scores, restarts, maps, _ = searcher.search_pairs_matches(q, e, 8, lorder, 128)
    assert maps.shape == (len(e), 8, max(len(x[2]) for x in qs))
    more = 0
    for p in range(len(e)):
        n1 = len(qs[q[p]][2])
        c, sc, rs, mp = matches_lib.matches(small_db, int(e[p]), qs[q[p]], lorder, 128, 8, 4 + int(q[p]))
        got = (int(counts[p]), list(scores[p]), list(restarts[p]))
        assert got == (c, list(sc), list(rs)), f"pair {p} (query {q[p]}, entry {e[p]}): gpu {got} reference {(c, list(sc), list(rs))}"
        assert np.array_equal(maps[p, :, :n1], mp[:, :n1]), f"maps of pair {p}"
        assert (maps[p, :, n1:] == -1).all()
        more += c > 1
    assert more, "no sampled pair had a second match"


# ---------------------------------------------------------------- against the whole-database call
@pytest.mark.parametrize("maxstart", [1, 64, 128, 4096])
@pytest.mark.parametrize("mm", [1, 3, 8])
def test_equals_the_rows_of_search_matches(searcher, wide_db, maxstart, mm):
    qs = wide_queries(wide_db)
    searcher.upload(wide_db)
    searcher.set_queries(qs, 2)
    q, e = shuffled_pairs(len(qs), len(wide_db), 150 if maxstart == 4096 else 400, maxstart + mm)
    for lorder in (True, False):
        whole = searcher.search_matches(mm, lorder, maxstart)
        ranked = searcher.topk_hits(3)
        got = searcher.search_pairs_matches(q, e, mm, lorder, maxstart)
        assert_rows_of(whole, q, e, got)
        got = searcher.search_pairs_matches(q, e, mm, lorder, maxstart, maps=False)
        assert_rows_of(whole, q, e, got, maps=False)
        # the buffers behind the ranked rows still hold the search before the pair calls
        again = searcher.topk_hits(3)
        assert np.array_equal(ranked[0], again[0])
        if mm > 1 and maxstart >= 64:
            assert (got[0] > 1).any(), "no pair had a second match"


def test_slot_zero_is_the_plain_search(searcher, wide_db):
    qs = wide_queries(wide_db)
    searcher.upload(wide_db)
    searcher.set_queries(qs, 0)
    q, e = shuffled_pairs(len(qs), len(wide_db), 200, 3)
    scores, maps, _ = searcher.search(True, True, 128)
    got = searcher.search_pairs_matches(q, e, 4, True, 128)
    assert np.array_equal(got[1][:, 0], scores[q, e])
    assert np.array_equal(got[3][:, 0, :], maps[q, e][:, :got[3].shape[-1]])


# ---------------------------------------------------------------- independence
def run_pairs(db, qs, q, e, mm, lorder, maxstart, maps=True):
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(qs, 1)
        got = s.search_pairs_matches(q, e, mm, lorder, maxstart, maps)
        return got[:4], s.last_launch_info()


@pytest.fixture(scope="module")
def wide_reference(wide_db):
    qs = wide_queries(wide_db)
    q, e = shuffled_pairs(len(qs), len(wide_db), 120, 9)
    ref = {lorder: run_pairs(wide_db, qs, q, e, 8, lorder, 1024)[0] for lorder in (True, False)}
    return qs, q, e, ref


@pytest.mark.parametrize("split", ["64", "512", "4096"])
def test_restart_split_does_not_change_results(monkeypatch, wide_db, wide_reference, split):
    qs, q, e, ref = wide_reference
    monkeypatch.setenv("SAT_EXP_REFINE_SPLIT", split)
    for lorder in (True, False):
        got, info = run_pairs(wide_db, qs, q, e, 8, lorder, 1024)
        assert "%d per item" % min(int(split), 1024) in info
        for a, b in zip(ref[lorder], got):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("env", [{"SAT_EXP_LPC": "0", "SAT_EXP_COMPACT": "0"}, {"SAT_EXP_LPC": "0", "SAT_EXP_COMPACT": "1"},
                                 {"SAT_EXP_LPC": "1", "SAT_EXP_COMPACT": "1"}, {"SAT_EXP_LPC": "2", "SAT_EXP_COMPACT": "0"},
                                 {"SAT_EXP_QLDS": "1"}, {"SAT_EXP_EPW": "2"}, {"SAT_EXP_EPW": "3"}, {"SAT_EXP_CHAINS": "64"},
                                 {"SAT_EXP_GENERAL": "1"}],
                         ids=lambda e: ",".join(f"{k[8:]}={v}" for k, v in e.items()))
def test_forced_execution_modes(monkeypatch, wide_db, wide_reference, env):
    """Lanes per chain, compaction, query cells in LDS, entries per workgroup, chains per slot: results unchanged."""
    qs, q, e, ref = wide_reference
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for lorder in (True, False):
        got, _ = run_pairs(wide_db, qs, q, e, 8, lorder, 1024)
        for a, b in zip(ref[lorder], got):
            assert np.array_equal(a, b)


def test_two_calls_and_reused_buffers(searcher, wide_db, wide_reference):
    """The list cut into two calls, then calls with more and with fewer pairs on the same context: same rows."""
    qs, q, e, ref = wide_reference
    searcher.upload(wide_db)
    searcher.set_queries(qs, 1)
    half = len(q) // 3
    a = searcher.search_pairs_matches(q[:half], e[:half], 8, True, 1024)
    b = searcher.search_pairs_matches(q[half:], e[half:], 8, True, 1024)
    for k in range(4):
        assert np.array_equal(np.concatenate([a[k], b[k]]), ref[True][k])
    big_q, big_e = np.tile(q, 3), np.tile(e, 3)
    big = searcher.search_pairs_matches(big_q, big_e, 8, True, 1024)
    for k in range(4):
        assert np.array_equal(big[k], np.concatenate([ref[True][k]] * 3))
    few = searcher.search_pairs_matches(q[:5], e[:5], 8, True, 1024)
    for k in range(4):
        assert np.array_equal(few[k], ref[True][k][:5])
    # fewer matches per pair, no maps; then nothing at all
    whole = searcher.search_matches(2, True, 64)
    got = searcher.search_pairs_matches(q, e, 2, True, 64, maps=False)
    assert_rows_of(whole, q, e, got, maps=False)
    none = searcher.search_pairs_matches([], [], 3, True, 64)
    assert none[0].shape == (0,) and none[1].shape == (0, 3) and searcher.last_launch_info() == ""


def test_launch_info_names_the_passes(searcher, wide_db, wide_reference):
    qs, q, e, _ = wide_reference
    searcher.upload(wide_db)
    searcher.set_queries(qs, 1)
    searcher.search_pairs_matches(q, e, 3, True, 256)
    info = searcher.last_launch_info()
    assert info.startswith("record pass (256 restarts, ") and "sat_sa_pair_match_kernel<" in info
    assert " | select | map pass: sat_sa_pair_match_kernel<" in info
    searcher.search_pairs_matches(q, e, 3, True, 256, maps=False)
    info = searcher.last_launch_info()
    assert info.endswith(" | select") and "map pass" not in info


# ---------------------------------------------------------------- API edges
def test_bad_arguments_are_rejected(searcher, small_db, golden_dir):
    lib = searcher._lib
    q, e = np.zeros(4, np.int32), np.arange(4, dtype=np.int32)
    bufs = [np.zeros(4 * 9, np.int32) for _ in range(3)]

    def call(ctx, maxstart, mm, n, qq, ee):
        return lib.sat_search_pairs_matches(ctx, 1, maxstart, mm, n, qq.ctypes.data, ee.ctypes.data, bufs[0].ctypes.data,
                                            bufs[1].ctypes.data, bufs[2].ctypes.data, None, None)

    with sat.Searcher(0) as fresh:
        assert call(fresh._ctx, 128, 2, 4, q, e) == -5                       # no database
        fresh.upload(small_db)
        assert call(fresh._ctx, 128, 2, 4, q, e) == -5                       # no query
    searcher.upload(small_db)
    searcher.set_query(*load_query(golden_dir, "d2phlb1.input"))
    assert call(searcher._ctx, 128, 2, 4, q, e) == 0
    for bad in (0, 9, -1):
        assert call(searcher._ctx, 128, bad, 4, q, e) == -1
    assert call(searcher._ctx, 0, 2, 4, q, e) == -1
    assert call(searcher._ctx, 128, 2, -1, q, e) == -1
    for bq, be in ((1, 0), (-1, 0), (0, len(small_db)), (0, -1)):
        qq, ee = q.copy(), e.copy()
        qq[2], ee[2] = bq, be
        assert call(searcher._ctx, 128, 2, 4, qq, ee) == -1
        assert b"pair 2" in lib.sat_last_error()


# ---------------------------------------------------------------- bytes
def test_bytes_copied_do_not_depend_on_the_database(golden_dir):
    db = sat.synth.make_db(300, 4, 90, sort=True, seed=12)
    db4 = sat.synth.make_db(1200, 4, 90, sort=True, seed=12)
    qs = [sat.synth.planted_query(db, 250, keep=0.6), load_query(golden_dir, "d2phlb1.input")]
    q, e = shuffled_pairs(len(qs), len(db), 70, 4)
    grown = []
    for d in (db, db4):
        with sat.Searcher(0) as s:
            s.upload(d)
            s.set_queries(qs, 0)
            steps = []
            for mm, maps in ((3, True), (8, False), (1, True)):
                before = s.d2h_bytes()
                s.search_pairs_matches(q, e, mm, True, 64, maps)
                steps.append(s.d2h_bytes() - before)
                # the documented amount (include/satabsearch.h)
                assert steps[-1] == 4 * len(q) * (1 + 2 * mm) + (MAXDIM * len(q) * mm if maps else 0)
            grown.append(steps)
    assert grown[0] == grown[1]


# ---------------------------------------------------------------- shards
def test_three_shards_on_one_gpu_equal_one_context(golden_dir):
    db = sat.synth.make_db(700, 4, 111, sort=True, seed=31)
    qs = [sat.synth.planted_query(db, 650, keep=0.6), load_query(golden_dir, "d2phlb1.input")]
    q, e = shuffled_pairs(len(qs), len(db), 300, 6)
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(qs, 2)
        ref = s.search_pairs_matches(q, e, 8, True, 256)
        ref_nomaps = s.search_pairs_matches(q, e, 3, False, 64, maps=False)
    with sat.MultiSearcher(3, devices=[0, 0, 0]) as m:
        m.upload(db)
        m.set_queries(qs, 2)
        begin = m.shards()
        assert all(((e >= begin[g]) & (e < begin[g + 1])).any() for g in range(3)), "a shard got no pair"
        got = m.search_pairs_matches(q, e, 8, True, 256)
        got_nomaps = m.search_pairs_matches(q, e, 3, False, 64, maps=False)
        with pytest.raises(sat.SatError):
            m.search_pairs_matches([0], [len(db)], 3, True, 64)
    for a, b in zip(ref[:4], got[:4]):
        assert np.array_equal(a, b)
    for a, b in zip(ref_nomaps[:3], got_nomaps[:3]):
        assert np.array_equal(a, b)
    assert got_nomaps[3] is None


# ---------------------------------------------------------------- command line
def cli(cwd, args, stdin):
    p = subprocess.run([CLI, *args], input=stdin, cwd=cwd, capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-600:]
    return p.stdout.decode()


def parse_blocks(text):
    """[(query id, [(name, score, [map lines])])] of an output, rows in printed order"""
    blocks = []
    for block in text.split("# cudaSaTabsearch")[1:]:
        lines = block.splitlines()
        qid = lines[1].split("=")[1].strip()
        rows = []
        for line in lines[3:]:
            if line[:1] == " " or line.split()[0].isdigit():                   # a map line
                rows[-1][2].append(tuple(int(v) for v in line.split()))
            else:
                rows.append((line.split()[0], int(line.split()[1]), []))
        blocks.append((qid, rows))
    return blocks


def strip_extras(text):
    """the output without the name:k rows and the map lines under them"""
    kept, skipping = [], False
    for line in text.splitlines(keepends=True):
        is_map = line[:1] == " " or (line.strip() and line.split()[0].isdigit())
        if line.startswith("#") or not is_map:
            skipping = not line.startswith("#") and ":" in line.split()[0]
        if not skipping:
            kept.append(line)
    return "".join(kept)


def assert_extras_are_the_library_slots(text, db, queries, mm, lorder, maxstart, lsoln):
    """Every name:k row (and its map lines) of every block is slot k - 1 of search_matches' row (query, entry) at
    `maxstart`, all of that row's matches 2..count are there, and there is at least one such row."""
    index = {n: i for i, n in enumerate(db.names)}
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries, 0)
        counts, scores, _, maps, _ = s.search_matches(mm, lorder, maxstart)
    blocks = parse_blocks(text)
    assert len(blocks) == len(queries)
    extras = 0
    for b, (_, rows) in enumerate(blocks):
        n1 = len(queries[b][2])
        seen = {}
        for name, score, lines in rows:
            base, _, k = name.partition(":")
            e, k = index[base], int(k or 1) - 1
            seen.setdefault(e, []).append(k)
            if k == 0:
                continue
            extras += 1
            assert k < counts[b, e] and score == scores[b, e, k], (b, name)
            want = [(i + 1, int(maps[b, e, k, i]) + 1) for i in range(n1) if maps[b, e, k, i] >= 0] if lsoln else []
            assert lines == want, (b, name)
        for e, ks in seen.items():
            assert ks == list(range(int(counts[b, e]))), (b, db.names[e], ks)
    assert extras, "no printed row had a second match"


@pytest.mark.parametrize("gpus", [[], ["-G", "0,0"]], ids=["one", "two-shards"])
def test_cli_k_equals_the_existing_m_k(golden_dir, gpus):
    stdin = open(os.path.join(golden_dir, "d2phlb1_TTT.input"), "rb").read()
    old = cli(golden_dir, ["-r", "64", "-k", "400", "-m", "3"], stdin)
    new = cli(golden_dir, ["-r", "64", "-k", "400", "-M", "3", *gpus], stdin)
    assert new == old
    assert any(":" in name for _, rows in parse_blocks(new) for name, _, _ in rows), "no entry had a second match"
    assert strip_extras(new) == cli(golden_dir, ["-r", "64", "-k", "400", *gpus], stdin)


def inline_case(golden_dir, name, options):
    """stdin of an example input with its option line replaced, its queries, and LORDER"""
    lines = open(os.path.join(golden_dir, name + ".input"), "rb").read().split(b"\n")
    stdin = b"\n".join([lines[0], options.encode()] + lines[2:])
    count = len(sat.StructSet.read(os.path.join(golden_dir, name + ".input"), "query", skip_header_lines=2))
    return stdin, [load_query(golden_dir, name + ".input", i) for i in range(count)], options.split()[1] == "T"


# (the cases below are ones whose printed rows do have further matches: a LORDER = F search of the example queries
# places the query over most of a structure and seldom leaves room for a second, disjoint placement)
@pytest.mark.parametrize("gpus", [[], ["-G", "0,0"]], ids=["one", "two-shards"])
@pytest.mark.parametrize("name,options", [("d2phlb1_TTT", "T T T"), ("multiquery", "T F T")])
def test_cli_cutoff(golden_dir, small_db, gpus, name, options):
    stdin, queries, lorder = inline_case(golden_dir, name, options)
    base = cli(golden_dir, ["-r", "128", "-p", "0.2", *gpus], stdin)
    more = cli(golden_dir, ["-r", "128", "-p", "0.2", "-M", "3", *gpus], stdin)
    assert strip_extras(more) == base
    assert 0 < sum(len(rows) for _, rows in parse_blocks(base)) < len(queries) * len(small_db)          # a real cutoff
    assert_extras_are_the_library_slots(more, small_db, queries, 3, lorder, 128, True)


@pytest.mark.parametrize("gpus", [[], ["-G", "0,0"]], ids=["one", "two-shards"])
@pytest.mark.parametrize("name,options", [("d2phlb1_TTT", "T T T"), ("multiquery", "T T T")])
def test_cli_refine(golden_dir, small_db, gpus, name, options):
    """-R: the matches are those at the stage-2 restarts, slot 0 the refined row itself"""
    stdin, queries, lorder = inline_case(golden_dir, name, options)
    args = ["-r", "16", "-R", "1024", "-k", "10", "-C", "40"]
    base = cli(golden_dir, [*args, *gpus], stdin)
    more = cli(golden_dir, [*args, "-M", "3", *gpus], stdin)
    assert strip_extras(more) == base
    assert all(len(rows) == 10 for _, rows in parse_blocks(base))
    assert_extras_are_the_library_slots(more, small_db, queries, 3, lorder, 1024, True)


@pytest.mark.parametrize("gpus", [[], ["-G", "0,0"]], ids=["one", "two-shards"])
def test_cli_sid_list(golden_dir, small_db, gpus):
    """-q: options T T F, so the extra rows come without map lines"""
    sids = open(os.path.join(golden_dir, "qmode_sids.txt"), "rb").read()
    args = ["-q", SMALL, "-r", "64", "-k", "5"]
    base = cli(golden_dir, [*args, *gpus], sids)
    more = cli(golden_dir, [*args, "-M", "2", *gpus], sids)
    assert more == cli(golden_dir, [*args, "-m", "2"], sids)
    assert strip_extras(more) == base
    blocks = parse_blocks(more)
    assert all(not lines for _, rows in blocks for _, _, lines in rows)
    index = {n.lower(): i for i, n in enumerate(small_db.names)}
    picks = [index[qid.lower()] for qid, _ in blocks]
    queries = [(*small_db.dense(i), small_db.ssetypes(i)) for i in picks]
    assert_extras_are_the_library_slots(more, small_db, queries, 2, True, 64, False)
