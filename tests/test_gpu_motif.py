"""Motif queries on the GPU (-m gpu): sat_queries_from_db_sses builds a query from a chosen list of a resident entry's
SSEs.  The batch's bytes against sat_queries_set's for the host-cut dense sub-arrays, over both edges of every size
class, permuted lists and non-finite cells; the searches that follow, against the dense batch and against the oracle;
the state the call leaves and the bytes it copies; its errors; the shards of sat_multi_queries_from_db_sses; and the
command line's -Q against -q with SID@list lines, and -E over them."""
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import edge_cases as ec
import motif_lib as ml
import oracle_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")


@pytest.fixture(scope="module")
def edge(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, ec.EDGE_DB))
    assert len(db) == 28 and tuple(db.orders) == ec.EDGE_ORDERS
    return db


@pytest.fixture(scope="module")
def packed():
    return ml.packed_db()


def R_(*a):
    return list(range(*a))


# (entry, list) of the packed database, orders 1 2 15 16 17 31 32 33 64 65 111 (entries 0 .. 10)
SINGLE = {
    "m=1 of 111": (10, [57]),
    "m=1 of 1": (0, [0]),
    "first 16": (10, R_(16)), "first 17": (10, R_(17)), "first 32": (10, R_(32)), "first 33": (10, R_(33)),
    "first 64": (10, R_(64)), "first 65": (10, R_(65)),
    "last 1": (10, R_(110, 111)), "last 16": (10, R_(95, 111)), "last 17": (10, R_(94, 111)), "last 65": (10, R_(46, 111)),
    "last 5 of 17": (4, R_(12, 17)),
    "reversed 33": (10, R_(32, -1, -1)), "reversed 111": (10, R_(110, -1, -1)), "reversed 16 of 16": (3, R_(15, -1, -1)),
    "every other": (10, R_(0, 111, 2)), "every other, odd": (10, R_(1, 111, 2)),
    "both ends of the NaN": (4, [16, 3, 5]), "both ends of the NaN, ascending": (4, [3, 16]), "neither end of the NaN": (4, [0, 1, 2, 15]),
    "both ends of the -inf": (10, [110, 0, 50]), "both ends of the -inf, ascending": (10, [0, 110]),
    "neither end of the -inf": (10, R_(1, 110)),
    "both ends of the +inf": (7, [31, 32]), "the 2-SSE entry swapped": (1, [1, 0]),
}
# whole entries and motifs, an entry twice with different lists, reverse file order
MIXED_ENTRIES = [10, 10, 9, 8, 7, 4, 4, 3, 1, 0]
MIXED_SSES = [R_(110, -1, -2), [110, 0, 50, 7], None, R_(20, 53), [32, 31, 0], [16, 3, 5], None, R_(15, -1, -1), [1, 0], []]


def assert_same_bytes(got, want, what):
    assert got.size == want.size, "%s: %d bytes, want %d" % (what, got.size, want.size)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d bytes differ, the first at %d (got %d want %d)" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


# ---------------------------------------------------------------- 1. blob bytes
def test_blob_bytes_equal_the_host_cut_batch(packed):
    with sat.Searcher(0) as s:
        s.upload(packed)
        for what, (e, l) in SINGLE.items():
            s.set_queries(ml.dense_queries(packed, [e], [l]), 3)
            want = s.debug_query_blob()
            s.set_queries_from_db([e], 3, sses=[l])
            assert (s.n1, s.n1max, s._n1s.tolist(), s.n_queries) == (len(l), len(l), [len(l)], 1), what
            assert_same_bytes(s.debug_query_blob(), want, what)
        # the identity list: the dense sub-arrays', and the plain call's
        for e in range(len(packed)):
            ident = R_(int(packed.orders[e]))
            s.set_queries_from_db([e], 3)
            plain = s.debug_query_blob()
            s.set_queries(ml.dense_queries(packed, [e], [ident]), 3)
            dense = s.debug_query_blob()
            for l in (ident, None, []):
                s.set_queries_from_db([e], 3, sses=[l])
                got = s.debug_query_blob()
                assert_same_bytes(got, plain, "identity of entry %d against the plain call" % e)
                assert_same_bytes(got, dense, "identity of entry %d" % e)
        # every single case as one batch, and the mixed batch
        for what, entries, sses in (("all singles", [e for e, _ in SINGLE.values()], [l for _, l in SINGLE.values()]),
                                    ("mixed", MIXED_ENTRIES, MIXED_SSES)):
            s.set_queries(ml.dense_queries(packed, entries, sses), 5)
            want = s.debug_query_blob()
            s.set_queries_from_db(entries, 5, sses=sses)
            assert_same_bytes(s.debug_query_blob(), want, what)
            lens = [len(l) if l else int(packed.orders[e]) for e, l in zip(entries, sses)]
            assert s._n1s.tolist() == lens and s.n1 == lens[0] and s.n1max == max(lens) and s.n_queries == len(lens)
        # five SSEs of the 111-SSE entry are a 16-wide query: its segment is as long as the 16-SSE entry's
        s.set_queries_from_db([10], 0, sses=[[100, 3, 50, 7, 110]])
        small = s.debug_query_blob().size
        s.set_queries_from_db([3], 0)
        assert s.debug_query_blob().size == small
        # the sentinel where the cell is not finite: the raw cells were read
        s.set_queries_from_db([4], 0, sses=[[16, 3, 5]])
        qdist = s.debug_query_blob()[:16 * 4 * 16].view(np.float32).reshape(4, 16, 4)       # [group][column i][k in the group]
        assert qdist[0, 0, 1] == np.float32(1.0e30) and qdist[0, 1, 0] == np.float32(1.0e30) and qdist[0, 2, 0] < 1.0e29


def test_blob_bytes_on_the_edge_database(edge):
    """the 28-entry database: ? codes, cells of 100 A and above, entries above 96 SSEs"""
    entries = [20, 17, 17, 5, 24, 3, 0, 1]
    sses = [[100, 3, 99, 70, 2, 1], [95, 2, 3, 40, 94, 90, 10, 66, 80, 70], None, R_(0, 111, 3), [30, 1, 2, 29, 20, 4], R_(96, 31, -1),
            R_(17), [0]]
    with sat.Searcher(0) as s:
        s.upload(edge)
        s.set_queries(ml.dense_queries(edge, entries, sses), 0)
        want = s.debug_query_blob()
        s.set_queries_from_db(entries, 0, sses=sses)
        assert_same_bytes(s.debug_query_blob(), want, "edge")


# ---------------------------------------------------------------- 2. search results
def test_searches_equal_those_of_the_dense_batch(packed):
    with sat.Searcher(0) as s:
        s.upload(packed)
        want, got = [], []
        for out, from_db in ((want, False), (got, True)):
            if from_db:
                s.set_queries_from_db(MIXED_ENTRIES, 7, sses=MIXED_SSES)
            else:
                s.set_queries(ml.dense_queries(packed, MIXED_ENTRIES, MIXED_SSES), 7)
            for lorder in (True, False):
                scores, maps, _ = s.search(lorder, True, 100)
                out += [scores, maps, s.topk_hits(5)]
        for w, g in zip(want, got):
            assert w.shape == g.shape and w.tobytes() == g.tobytes()
        # several matches of one motif
        e, l = 10, R_(40, 20, -2)
        s.set_queries(ml.dense_queries(packed, [e], [l]), 7)
        want = s.search_matches(2, True, 32)[:4]
        s.set_queries_from_db([e], 7, sses=[l])
        got = s.search_matches(2, True, 32)[:4]
        for w, g in zip(want, got):
            assert w.shape == g.shape and w.tobytes() == g.tobytes()


ORACLE_MOTIFS = [(3, [4, 20, 50, 96, 70]), (6, R_(2, 10)), (18, [1, 0, 7, 4, 2])]     # of a 97-SSE entry; ascending; permuted


def test_motif_searches_equal_the_oracle(edge):
    entries, sses = [e for e, _ in ORACLE_MOTIFS], [l for _, l in ORACLE_MOTIFS]
    with sat.Searcher(0) as s:
        s.upload(edge)
        s.set_queries_from_db(entries, 0, sses=sses)
        scores, maps, _ = s.search(True, True, 16)
    assert scores.shape == (3, len(edge))
    for q, (t, d, ty) in enumerate(ml.dense_queries(edge, entries, sses)):
        oscores, omaps, _ = oracle_lib.search(edge, t, d, ty, True, True, 16, query_ordinal=q)
        assert np.array_equal(scores[q], oscores), q
        m = t.shape[0]
        assert np.array_equal(maps[q][:, :m], omaps[:, :m]), q
        assert (maps[q][:, m:] == -1).all()
    # the ascending motif is found in its own entry (a permuted one, under LORDER = T, need not be)
    assert scores[1, entries[1]] == scores[1].max()


# ---------------------------------------------------------------- 3. state
def test_state_after_the_call(edge, packed):
    idx = np.array([0, 5, 9, 21, 5], np.int32)
    sses = [[16, 0, 3], R_(10, 80), None, [], R_(110, 100, -1)]
    total = 3 + 70 + 10
    dense = ml.dense_queries(edge, idx, sses)
    with sat.Searcher(0) as s:
        s.upload(edge)
        s.set_queries(dense, 0)
        blob_bytes = s.debug_query_blob().size
        s.search(True, False, 16)
        s.fit_statistics(0.1)
        s.set_polish_all(2)
        before = s.query_h2d_bytes()
        s.set_queries_from_db(idx, 0, sses=sses)
        assert s.query_h2d_bytes() - before == 8 * len(idx) + 4 + total
        assert s.polish_all() == 2
        s.set_polish_all(0)
        assert s._lib.sat_query_count(s._ctx) == len(idx) and s.n_queries == len(idx)
        assert s._n1s.tolist() == [3, 70, 16, 1, 10]
        with pytest.raises(sat.SatError, match=r"\[-5\]"):
            s.results()
        with pytest.raises(sat.SatError, match=r"\[-5\]"):
            s.topk_hits(3)
        s.search(True, False, 16)
        hits = s.topk_hits(5)                  # the built-in statistics: the fit went with the old batch
        before = s.query_h2d_bytes()
        s.set_queries(dense, 0)
        assert s.query_h2d_bytes() - before == blob_bytes
        s.search(True, False, 16)
        assert s.topk_hits(5).tobytes() == hits.tobytes()
        # the old call still copies 4 bytes a query; all whole entries through the new one 8 a query and 4
        before = s.query_h2d_bytes()
        s.set_queries_from_db(idx, 0)
        assert s.query_h2d_bytes() - before == 4 * len(idx)
        before = s.query_h2d_bytes()
        s.set_queries_from_db(idx, 0, sses=[None] * len(idx))
        assert s.query_h2d_bytes() - before == 8 * len(idx) + 4
        # the batch is a copy: another database goes up under it
        s.set_queries(dense, 0)
        s.upload(packed)
        want = s.search(True, True, 16)[:2]
        s.upload(edge)
        s.set_queries_from_db(idx, 0, sses=sses)
        s.upload(packed)
        got = s.search(True, True, 16)[:2]
        assert got[0].shape == (len(idx), len(packed))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---------------------------------------------------------------- 4. errors
def raw_call(s, entries, begin, sse, null=None):
    e = np.asarray(entries, np.int32)
    b = np.asarray(begin, np.int32)
    l = np.asarray(sse if len(sse) else [0], np.uint8)
    return s._lib.sat_queries_from_db_sses(s._ctx, len(e), None if null == "entry" else e.ctypes.data,
                                           None if null == "begin" else b.ctypes.data, None if null == "sse" else l.ctypes.data, 1)


def test_errors_leave_the_previous_batch(edge):
    idx = [6, 2, 14]
    sses = [R_(5, 25), [1, 0], None]
    with sat.Searcher(0) as s:
        with pytest.raises(sat.SatError, match=r"\[-5\].*no database"):
            s.set_queries_from_db([0], 0, sses=[[0]])
        s.upload(edge)
        s.set_queries_from_db(idx, 1, sses=sses)
        want = s.search(True, False, 32)[0]
        blob = s.debug_query_blob()

        def intact(what):
            """the batch set above, as the context holds it now: asked after every refusal, before any call that succeeds"""
            assert s._lib.sat_query_count(s._ctx) == 3, what
            assert (s.n_queries, s.n1, s.n1max, s._n1s.tolist()) == (3, 20, 111, [20, 2, 111]), what
            assert_same_bytes(s.debug_query_blob(), blob, what)
            assert s.results()[0].tobytes() == want.tobytes(), what              # the searched state was not cleared
            assert s.search(True, False, 32)[0].tobytes() == want.tobytes(), what

        intact("the batch itself")
        for bad_entries, bad_sses, message in (
                ([3, -1, 4], [None, [0], None], r"query 1: entry -1 "),
                ([3, 4, len(edge)], [None, [0], [0]], r"query 2: entry 28 "),
                ([3, 2, 4], [None, [0, 1, 0], None], r"query 1: 3 SSEs listed, entry 2 has 2"),          # longer than the order
                ([3, 18, 4], [None, [0, 8, 1], None], r"query 1: SSE 8 outside 0\.\.7 of entry 18"),
                ([3, 4, 18], [None, None, [7, 3, 5, 3]], r"query 2: SSE 3 listed twice"),
                ([], [], r"")):
            with pytest.raises(sat.SatError, match=r"\[-1\].*" + message):
                s.set_queries_from_db(bad_entries, 1, sses=bad_sses)
            intact(message or "no queries")
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 0: SSE 2 listed twice"):
            s.set_queries_from_db([3], 1, sses=[[2, 2]])
        intact("a one-query batch, refused")
        for null in ("entry", "begin", "sse"):
            assert raw_call(s, [3, 4], [0, 1, 2], [0, 0], null) == -1
            intact("null " + null)
        assert raw_call(s, [3, 4], [1, 1, 2], [0, 0]) == -1 and b"sse_begin[0] is 1" in s._lib.sat_last_error()
        intact("sse_begin[0] != 0")
        assert raw_call(s, [3, 4, 5], [0, 2, 1, 2], [0, 1]) == -1 and b"query 1: sse_begin descends from 2 to 1" in s._lib.sat_last_error()
        intact("sse_begin descends")
        # the helper's own call is a good one, and only now is the batch replaced
        assert raw_call(s, [3, 4], [0, 1, 2], [0, 0]) == 0
        assert s._lib.sat_query_count(s._ctx) == 2 and s.debug_query_blob().size != blob.size


# ---------------------------------------------------------------- 5. shards
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2", "3"])
def test_shards_build_and_exchange_their_motifs(edge, devices):
    with sat.MultiSearcher(len(devices), devices=devices) as m:
        m.upload(edge)
        begin = m.shards()
        picks, lists = [], []
        for g in range(len(devices)):
            first, last = int(begin[g]), int(begin[g + 1]) - 1       # the first and the last entry of every shard
            picks += [first, last]
            lists += [R_(int(edge.orders[first]) - 1, -1, -2), None if g == 1 else [0]]
        # reverse file order, a whole entry, an entry a second time with another list
        idx = np.array(picks[::-1] + [5, 20, picks[0]], np.int32)
        sses = lists[::-1] + [R_(3, 103), [100, 3, 99, 70, 2, 1], None]
        owner = np.searchsorted(begin, idx, side="right") - 1
        assert len(set(owner.tolist())) == len(devices)
        dense = ml.dense_queries(edge, idx, sses)
        with sat.Searcher(0) as s:
            s.upload(edge)
            s.set_queries(dense, 2)
            one_blob = s.debug_query_blob()
        m.set_queries(dense, 2)
        want = m.search(True, True, 32)[:2] + m.search_topk(4, False, True, 32)[:2]
        sent = [m.debug_shard_queries(g)[1] for g in range(len(devices))]
        m.set_queries_from_db(idx, 2, sses=sses)
        assert m.n_queries == len(idx) and m.n1max == max(len(l) if l else int(edge.orders[e]) for e, l in zip(idx, sses))
        for g in range(len(devices)):
            blob, h2d = m.debug_shard_queries(g)
            assert_same_bytes(blob, one_blob, "shard %d" % g)
            # each shard is sent the indices, the offsets and the lists of its own queries
            own = sum(len(l) for l, o in zip(sses, owner) if l and o == g)
            assert h2d - sent[g] == 8 * len(idx) + 4 + own, g
        got = m.search(True, True, 32)[:2] + m.search_topk(4, False, True, 32)[:2]
        for w, g in zip(want, got):
            assert w.shape == g.shape and w.tobytes() == g.tobytes()
        # every refusal leaves every shard's batch as it is: asked after each one, before any call that succeeds
        sent = [m.debug_shard_queries(g)[1] for g in range(len(devices))]
        for bad_entries, bad_sses, message in (
                ([0, 4], [None, [3]], r"query 1: SSE 3 outside 0\.\.2 of entry 4"),
                ([0, len(edge)], [None, [0]], r"query 1: entry 28 "),
                ([0, -1], [[0], None], r"query 1: entry -1 "),
                ([27, 2], [None, [0, 1, 0]], r"query 1: 3 SSEs listed, entry 2 has 2"),
                ([27, 18, 0], [[0], [7, 3, 5, 3], None], r"query 1: SSE 3 listed twice"),
                ([], [], r"")):
            with pytest.raises(sat.SatError, match=r"\[-1\].*" + message):
                m.set_queries_from_db(bad_entries, 2, sses=bad_sses)
            for g in range(len(devices)):
                blob, h2d = m.debug_shard_queries(g)
                assert_same_bytes(blob, one_blob, "shard %d after %s" % (g, message))
                assert h2d == sent[g], (g, message)                # and nothing was sent to it
            assert m.search(True, True, 32)[0].tobytes() == want[0].tobytes(), message


# ---------------------------------------------------------------- 6. command line
def cli(golden_dir, args, stdin, restarts=16):
    return subprocess.run([CLI, "-r", str(restarts), *args], input=stdin, cwd=golden_dir, capture_output=True, timeout=120)


CLI_ENTRIES = [6, 3, 18, 5, 20, 21, 18, 0]
CLI_SSES = [R_(2, 10), [4, 20, 50, 96, 70], [1, 0, 7, 4, 2], None, [100, 3, 99, 70, 2, 1], None, R_(8), [16]]


@pytest.mark.parametrize("args", [[], ["-k", "3"], ["-m", "2"], ["-p", "1", "-F", "0.1"], ["-G", "0,0"]],
                         ids=["plain", "k3", "m2", "p1F", "G00"])
def test_cli_Q_prints_what_q_prints(golden_dir, edge, args):
    stdin = ml.stdin_lines(edge, CLI_ENTRIES, CLI_SSES)
    q = cli(golden_dir, ["-q", ec.EDGE_DB, *args], stdin)
    Q = cli(golden_dir, ["-Q", ec.EDGE_DB, *args], stdin)
    assert q.returncode == 0 and Q.returncode == 0, Q.stderr.decode()[-400:]
    assert q.stdout.count(b"# QUERY ID") >= len(CLI_ENTRIES) and Q.stdout == q.stdout
    # the list's line stands in the motifs' blocks and in no other: after # DBFILE, 1-based, in the order given
    blocks = q.stdout.split(b"# cudaSaTabsearch")[1:]
    ranked = bool(args) and args[0] in ("-k", "-p")
    assert len(blocks) == len(CLI_ENTRIES) * (1 if ranked else 2)
    for b, block in enumerate(blocks):
        l = CLI_SSES[b % len(CLI_ENTRIES)]
        lines = block.split(b"\n")
        assert lines[1].startswith(b"# QUERY ID = " + edge.names[CLI_ENTRIES[b % len(CLI_ENTRIES)]].encode())
        if l is None:
            assert b"# QUERY SSES" not in block
        else:
            assert lines[3] == ("# QUERY SSES = " + ml.spell(l)).encode() and block.count(b"# QUERY SSES") == 1


def test_cli_a_motif_finds_its_entry(golden_dir, edge):
    """the planted case: eight SSEs of the 64-SSE entry rank that entry first, with the score the oracle gives the cut
    sub-structure against it - its best over the database"""
    e, l = 6, [3, 9, 14, 22, 31, 40, 52, 60]
    t, d, ty = ml.cut(edge, e, l)
    oscores = oracle_lib.search(edge, t, d, ty, True, False, 128, query_ordinal=0)[0]
    assert oscores[e] == oscores.max() and (oscores == oscores.max()).sum() == 1
    p = cli(golden_dir, ["-Q", ec.EDGE_DB, "-k", "3"], ml.stdin_lines(edge, [e], [l]), restarts=128)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    lines = p.stdout.split(b"\n")
    assert lines[3] == b"# QUERY SSES = 4,10,15,23,32,41,53,61"
    assert lines[4].split()[:2] == [edge.names[e].encode(), str(int(oscores[e])).encode()]
    # norm2 is the stand-alone query's: n1 = 8
    assert float(lines[4].split()[2]) == pytest.approx(2.0 * oscores[e] / (8 + 64), rel=1e-5)


def test_cli_E_scores_a_motif_as_its_entry(golden_dir, edge, tmp_path):
    """-Q -E with motif lines: the query's node and class are its entry's and the entry itself stays excluded; u2 follows
    from the rows -k prints for the same stdin (pairs of a positive above a negative count 2, ties 1)"""
    cls = ["c%d" % (k % 3) if k % 7 != 6 else None for k in range(len(edge))]
    path = tmp_path / "edge.classes"
    path.write_text("".join("%s %s\n" % (edge.names[k], c) for k, c in enumerate(cls) if c))
    entries, sses = [5, 3, 17, 0], [R_(2, 10), None, [95, 2, 3, 40, 94], [16, 0, 3]]
    assert all(cls[e] for e in entries)
    stdin = ml.stdin_lines(edge, entries, sses)
    rows = cli(golden_dir, ["-Q", ec.EDGE_DB, "-k", str(len(edge))], stdin)
    got = cli(golden_dir, ["-Q", ec.EDGE_DB, "-E", str(path)], stdin)
    assert rows.returncode == 0 and got.returncode == 0, got.stderr.decode()[-400:]
    blocks = rows.stdout.decode().split("# cudaSaTabsearch")[1:]
    lines = [line.split() for line in got.stdout.decode().splitlines() if not line.startswith("#")]
    assert len(blocks) == len(lines) == len(entries)
    for e, block, cols in zip(entries, blocks, lines):
        score = {r.split()[0]: int(r.split()[1]) for r in block.splitlines()[1:] if r and not r.startswith("#")}
        assert len(score) == len(edge)
        others = [k for k in range(len(edge)) if k != e and cls[k]]
        pos = [score[edge.names[k]] for k in others if cls[k] == cls[e]]
        neg = [score[edge.names[k]] for k in others if cls[k] != cls[e]]
        u2 = sum(2 * (p > n) + (p == n) for p in pos for n in neg)
        assert cols[:5] == [edge.names[e], cls[e], str(len(pos)), str(len(neg)), str(u2)], cols
