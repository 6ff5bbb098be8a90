"""A query's SSEs profiled over its hits on the GPU (-m gpu): sat_profile_rows, its shards and the command line's -W P.
The expected numbers never come from the new kernel: the same search with lsoln, then hits_cutoff(P) with maps - the
compaction and sort route - and in numpy the rows of the query's own node dropped, A = (maps >= 0), joint = A.T @ A
(profile_lib.expected).  One case recomputes the p-values from the scores on the host instead."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import report
import profile_lib as pl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
SMALL_DB = "tableauxdistmatrixdb.small.ascii"
R = 8
P_MID = 1e-3
# both size classes of every kernel family, and both sides of a 64-bit word of SSEs; five queries a batch
BATCH_ORDERS = {"A": (1, 8, 32, 65, 111), "B": (2, 33, 64, 12, 20)}
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)        # wave and block edges, two blocks plus one row


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def query_structs(batch):
    """the batch's random query structures as a StructSet"""
    orders = BATCH_ORDERS[batch]
    made = [sat.synth.make_query(n, seed=sat.synth.QUERY_SEED + 17 * n) for n in orders]
    return sat.StructSet.from_dense(orders, [m[0] for m in made], [m[1] for m in made], ["q%06d" % n for n in orders])


def query_triples(batch):
    qs = query_structs(batch)
    return [qs.dense(j) + (qs.ssetypes(j),) for j in range(len(qs))]


def with_copies(n, sources, copies, seed, lo=8, hi=20, keep=0.8, jitter=0.5):
    """(database, where) - a synthetic database of n entries in which `copies` near copies of each structure of
    `sources` (those of at least 4 SSEs) stand at random places: where[j] lists the places of source j's"""
    base = sat.synth.make_db(n, lo, hi, sort=False, name_format="s%06d")
    tabs, dmats, orders = [], [], base.orders.copy()
    for s in range(n):
        t, d = base.dense(s)
        tabs.append(t)
        dmats.append(d)
    rng = np.random.default_rng(seed)
    big = [j for j in range(len(sources)) if sources.orders[j] >= 4]
    places = rng.permutation(n)[:copies * len(big)] if n >= copies * len(big) else rng.permutation(n)
    where = {j: [] for j in range(len(sources))}
    for i, at in enumerate(places.tolist()):
        j = big[i % len(big)]
        t, d, _ = sat.synth.planted_query(sources, j, keep=keep, jitter=jitter, seed=seed + 31 * i)
        tabs[at], dmats[at], orders[at] = t, d, len(t)
        where[j].append(at)
    return sat.StructSet.from_dense(orders, tabs, dmats, list(base.names)), where


@functools.lru_cache(maxsize=None)
def database(n, batch):
    return with_copies(n, query_structs(batch), 3, 1000 + n)[0]


def expected_of(s, p, nodes=None):
    """(hits, [joint]) of the searched state at cutoff p by the existing route: hits_cutoff with maps, then numpy"""
    rows, maps = s.hits_cutoff(p, lsoln=True)
    hits, joints = [], []
    for q in range(len(rows)):
        h, j = pl.expected(np.asarray(maps[q]).reshape(-1, sat.MAXDIM), rows[q]["entry"], int(s._n1s[q]), None if nodes is None else int(nodes[q]))
        hits.append(h)
        joints.append(j)
    return np.array(hits, np.uint32), joints


def same(got, want, what=""):
    assert got[0].dtype == np.uint32 and np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert len(got[1]) == len(want[1])
    for q, (g, w) in enumerate(zip(got[1], want[1])):
        assert g.dtype == np.uint32 and g.shape == w.shape and np.array_equal(g, w), (what, q)
        assert np.array_equal(g, g.T)


def profile_bytes(n1s):
    return 4 * len(n1s) + 4 * int((np.asarray(n1s, np.int64) ** 2).sum())


@pytest.fixture(scope="module")
def searcher():
    with sat.Searcher(0) as s:
        yield s


# ---------------------------------------------------------------- 1. shapes and cutoffs
@pytest.mark.parametrize("batch", sorted(BATCH_ORDERS))
@pytest.mark.parametrize("n", SIZES)
def test_shapes_and_cutoffs(searcher, n, batch):
    s = searcher
    s.upload(database(n, batch))
    s.set_queries(query_triples(batch))
    s.search(True, True, R)
    middle = None
    for p in (0.0, P_MID, 1.0):
        want = expected_of(s, p)
        if p == 1.0:
            assert (want[0] == n).all()                                 # every row counts
            assert [int(j[0, 0]) for j in want[1]] == [int((m[:, 0] >= 0).sum()) for m in s.results(True)[1]]
        if p == P_MID:
            middle = want[0]
        before = s.d2h_bytes()
        got = s.profile_rows(p)
        assert s.d2h_bytes() - before == profile_bytes(BATCH_ORDERS[batch])
        same(got, want, "n = %d, p = %g" % (n, p))
        same(s.profile_rows(p, np.full(5, -1)), want, "no query is a node")
    print("middle cutoff, n = %d batch %s: hits %s" % (n, batch, middle.tolist()))
    if n > 1:       # (a database of one row has no cutoff that counts a row and not all)
        assert any(0 < h < n for h in middle.tolist()), middle


def test_expected_from_the_scores_on_the_host(searcher):
    """the second anchor: every row's p-value recomputed on the host from the score sat_results returns"""
    n, batch = 1025, "A"
    db = database(n, batch)
    s = searcher
    s.upload(db)
    s.set_queries(query_triples(batch))
    s.search(True, True, R)
    scores, maps = s.results(True)
    got = s.profile_rows(P_MID)
    for q, n1 in enumerate(BATCH_ORDERS[batch]):
        pv = np.array([report.stats(scores[q, e], n1, db.orders[e])[2] for e in range(n)])
        hits, joint = pl.matrices(maps[q, pv <= P_MID, :n1] >= 0)
        assert got[0][q] == hits and np.array_equal(got[1][q], joint), q
    assert 0 < got[0].sum() < 5 * n


def test_offsets_with_gaps(searcher):
    n, batch = 65, "B"
    s = searcher
    s.upload(database(n, batch))
    s.set_queries(query_triples(batch))
    s.search(True, True, R)
    want = s.profile_rows(1.0)
    sizes = [n1 * n1 for n1 in BATCH_ORDERS[batch]]
    # the matrices in another order than the queries', with gaps of 3, 0, 7, 1 words between them and 5 before the first
    order, gaps = [3, 0, 4, 2, 1], [5, 3, 0, 7, 1]
    offset, at = np.zeros(5, np.int64), 0
    for q, gap in zip(order, gaps):
        at += gap
        offset[q] = at
        at += sizes[q]
    joint = np.full(at + 9, 0xDEADBEEF, np.uint32)
    hits = np.full(5, 0xDEADBEEF, np.uint32)
    s.profile_rows_raw(1.0, None, hits, joint, offset)
    assert np.array_equal(hits, want[0])
    written = np.zeros(len(joint), bool)
    for q in range(5):
        assert np.array_equal(joint[offset[q]:offset[q] + sizes[q]].reshape(want[1][q].shape), want[1][q]), q
        written[offset[q]:offset[q] + sizes[q]] = True
    assert (joint[~written] == 0xDEADBEEF).all() and (~written).sum() == sum(gaps) + 9


# ---------------------------------------------------------------- 2. queries that are entries; motifs; settings
FAMILY_N = 300


@functools.lru_cache(maxsize=None)
def family_db():
    """300 entries among which stand six near copies each of two base structures (orders 16 and 40)"""
    bases = [sat.synth.make_query(n, seed=sat.synth.QUERY_SEED + 5 * n) for n in (16, 40)]
    src = sat.StructSet.from_dense([16, 40], [b[0] for b in bases], [b[1] for b in bases], ["base16", "base40"])
    return with_copies(FAMILY_N, src, 6, 77, keep=0.85, jitter=0.5)


def member_queries():
    db, where = family_db()
    return db, np.array(where[0][:3] + where[1][:2], np.int32)


def test_a_database_member_with_and_without_its_node(searcher):
    db, members = member_queries()
    s = searcher
    s.upload(db)
    s.set_queries_from_db(members)
    s.search(True, True, R)
    with_own = expected_of(s, P_MID)
    without = expected_of(s, P_MID, members)
    # the expected side first: every query's own row is a hit, and some query has other hits but not everything
    assert np.array_equal(with_own[0], without[0] + 1)
    assert any(0 < h < FAMILY_N - 1 for h in without[0].tolist()), without[0]
    _, maps = s.results(True)
    for q, e in enumerate(members):
        own = (maps[q, e, :db.orders[e]] >= 0).astype(np.uint32)
        assert own.any() and np.array_equal(with_own[1][q] - without[1][q], np.outer(own, own))
        assert np.array_equal(np.diag(with_own[1][q]), np.diag(without[1][q]) + own)       # one higher on every matched SSE
    same(s.profile_rows(P_MID, members), without, "own rows excluded")
    same(s.profile_rows(P_MID), with_own, "query_node = None")
    some = members.copy()
    some[[1, 3]] = -1
    mixed = (np.where(some < 0, with_own[0], without[0]), [with_own[1][q] if some[q] < 0 else without[1][q] for q in range(5)])
    same(s.profile_rows(P_MID, some), mixed, "two of the five are no nodes")
    same(s.profile_rows(P_MID, members + FAMILY_N), with_own, "nodes that no ordinal equals exclude nothing")
    # P = 1 counts every row but the query's own
    got = s.profile_rows(1.0, members)
    assert (got[0] == FAMILY_N - 1).all()
    same(got, expected_of(s, 1.0, members), "P = 1")


def test_a_motif_query_with_its_source_node(searcher):
    db, where = family_db()
    e = where[1][0]
    order = int(db.orders[e])
    lists = [[5, 2, 9, 0, 7, 11, 3], list(range(order - 1, -1, -2)), None]
    nodes = np.array([e, e, where[0][0]], np.int32)
    s = searcher
    s.upload(db)
    s.set_queries_from_db(nodes, sses=lists)
    assert s._n1s.tolist() == [7, len(lists[1]), int(db.orders[nodes[2]])]
    s.search(True, True, R)
    for p in (P_MID, 1.0):
        want = expected_of(s, p, nodes)
        same(s.profile_rows(p, nodes), want, "motif, p = %g" % p)
    assert (want[0] == FAMILY_N - 1).all()


@pytest.mark.parametrize("setting", ["lorder_off", "fit", "polish_all"])
def test_settings_are_followed(setting):
    """LORDER = F; an installed fit selects by its p-values; polish-all counts the polished maps - each against the
    existing route under the same setting"""
    db, members = member_queries()
    with sat.Searcher(0) as s:
        s.upload(db)
        if setting == "polish_all":
            s.set_polish_all(2)
        s.set_queries_from_db(members)
        s.search(setting != "lorder_off", True, R)
        plain = expected_of(s, P_MID, members)
        if setting == "fit":
            fits = s.fit_statistics(0.05)
            assert fits["fitted"].any()
        want = expected_of(s, P_MID, members)
        if setting == "fit":
            assert not np.array_equal(want[0], plain[0])                # the fitted p-values select other rows
        assert want[0].sum() > 0
        same(s.profile_rows(P_MID, members), want, setting)
        if setting == "polish_all":
            assert s.polish_all() == 2
            base = s.results_base()
            assert (s.results()[0] >= base).all() and (s.results()[0] > base).any()


def test_chunk_walk(monkeypatch):
    """1025 entries are two blocks a query; 2050 keys hold one query, so five queries take five launches: the numbers are
    the one-launch numbers"""
    n, batch = 1025, "A"
    out = []
    for keys in (None, 2 * n):
        if keys is None:
            monkeypatch.delenv("SAT_EXP_SELECT_KEYS", raising=False)
        else:
            monkeypatch.setenv("SAT_EXP_SELECT_KEYS", str(keys))
        with sat.Searcher(0) as s:                                      # the override is read when a context is created
            s.upload(database(n, batch))
            s.set_queries(query_triples(batch))
            s.search(True, True, R)
            out.append([s.profile_rows(p) for p in (P_MID, 1.0)])
            if keys is None:
                for p, got in zip((P_MID, 1.0), out[0]):
                    same(got, expected_of(s, p), "one launch")
    for one, cut in zip(*out):
        same(cut, one, "five launches")
    assert out[0][0][0].sum() > 0


# ---------------------------------------------------------------- 3. shards
@pytest.mark.parametrize("devices", [[0], [0, 0, 0]], ids=["1", "3"])
def test_shards_equal_one_context(devices):
    db, members = member_queries()
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries_from_db(members)
        s.search(True, True, R)
        single = [s.profile_rows(p, members) for p in (P_MID, 1.0)]
        same(single[0], expected_of(s, P_MID, members))
        n1s = s._n1s.copy()
    with sat.MultiSearcher(len(devices), devices=devices) as m:
        m.upload(db)
        m.set_queries_from_db(members)
        with pytest.raises(sat.SatError, match=r"\[-5\].*no search"):
            m.profile_rows(P_MID, members)
        m.search_only(True, False, R)
        with pytest.raises(sat.SatError, match=r"\[-5\].*without lsoln"):
            m.profile_rows(P_MID, members)
        m.search_only(True, True, R)
        for p, want in zip((P_MID, 1.0), single):
            before = m.d2h_bytes()
            same(m.profile_rows(p, members), want, "%d shards, p = %g" % (len(devices), p))
            assert m.d2h_bytes() - before == len(devices) * profile_bytes(n1s)
        hits, joint = np.zeros(5, np.uint32), np.zeros(int((n1s.astype(np.int64) ** 2).sum()), np.uint32)
        before = m.d2h_bytes()
        for bad in (-1.0, float("nan")):
            with pytest.raises(sat.SatError, match=r"\[-1\].*max_pvalue"):
                m.profile_rows_raw(bad, members, hits, joint)
        with pytest.raises(sat.SatError, match=r"\[-1\].*null array"):
            m.profile_rows_raw(P_MID, members, None, joint)
        assert m.d2h_bytes() == before and not hits.any() and not joint.any()
        same(m.profile_rows(P_MID, members), single[0], "after the refused calls")


# ---------------------------------------------------------------- 4. state
def test_state_errors_and_what_is_left_alone():
    db, members = member_queries()
    rng = np.random.default_rng(3)
    classes = rng.integers(0, 4, FAMILY_N).astype(np.int32)
    with sat.Searcher(0) as s:
        hits, joint = np.full(5, 7, np.uint32), np.full(40 * 40 * 5, 7, np.uint32)
        with pytest.raises(sat.SatError, match=r"\[-5\]"):
            s.profile_rows_raw(P_MID, None, hits, joint)
        s.upload(db)
        s.set_queries_from_db(members)
        with pytest.raises(sat.SatError, match=r"\[-5\].*no search"):
            s.profile_rows(P_MID)
        s.search(True, False, R)
        with pytest.raises(sat.SatError, match=r"\[-5\].*without lsoln"):
            s.profile_rows(P_MID)
        s.search(True, True, R)
        before = s.d2h_bytes()
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(sat.SatError, match=r"\[-1\].*max_pvalue"):
                s.profile_rows_raw(bad, members, hits, joint)
        with pytest.raises(sat.SatError, match=r"\[-1\].*null array"):
            s.profile_rows_raw(P_MID, members, None, joint)
        with pytest.raises(sat.SatError, match=r"\[-1\].*null array"):
            s.profile_rows_raw(P_MID, members, hits, None)
        assert s.d2h_bytes() == before and (hits == 7).all() and (joint == 7).all()
        assert s._lib.sat_profile_rows(None, 0.5, None, hits.ctypes.data, joint.ctypes.data, None) == -1
        # the searched state, live accumulators and installed classes around a profile call
        s.cluster_begin()
        s.cover_begin()
        s.set_eval_classes(classes)
        s.cluster_add(P_MID, members)
        s.cover_add(P_MID, members)

        def state():
            scores, maps = s.results(True)
            rows, rmaps = s.hits_cutoff(P_MID, lsoln=True)
            return scores, maps, rows, rmaps, s.cluster_labels(), s.cover_solve(), s.eval_rows(members)

        def flat(x):
            return [y for part in x for y in flat(part)] if isinstance(x, (list, tuple)) else [x]

        was = state()
        first = s.profile_rows(P_MID, members)
        second = s.profile_rows(P_MID, members)
        same(second, first, "a second call")
        same(first, expected_of(s, P_MID, members))
        now = state()
        for a, b in zip(flat(was), flat(now)):
            assert np.array_equal(a, b)
        # a profile at another cutoff and of other nodes in between changes nothing either
        s.profile_rows(1.0)
        same(s.profile_rows(P_MID, members), first, "after a profile at another cutoff")
        s.cluster_end()
        s.cover_end()
        # a new query batch: the state error again, until it is searched
        s.set_queries_from_db(members[:2])
        with pytest.raises(sat.SatError, match=r"\[-5\].*no search"):
            s.profile_rows(P_MID)


# ---------------------------------------------------------------- 5. command line
def cli(cwd, args, stdin=b"not read\n"):
    return subprocess.run([CLI, "-r", "16", *args], input=stdin, cwd=cwd, capture_output=True, timeout=300)


@pytest.fixture(scope="module")
def small(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, SMALL_DB))
    assert len(db) == 586
    return db


def library_table(db, entries, lists, dbfile, p, fraction, batch=256, **settings):
    """report.profile_table of the library's own calls, batch by batch as the command line cuts them"""
    hits, joints = [], []
    with sat.Searcher(0) as s:
        s.upload(db)
        for lo in range(0, len(entries), batch):
            part = np.asarray(entries[lo:lo + batch], np.int32)
            s.set_queries_from_db(part, lo, sses=None if lists is None else lists[lo:lo + batch])
            s.search(True, True, 16)
            h, j = s.profile_rows(p, part)
            hits += h.tolist()
            joints += j
    types = [db.ssetypes(e) if lists is None or not lists[q] else db.ssetypes(e)[lists[q]] for q, e in enumerate(entries)]
    return report.profile_table([db.names[e] for e in entries], types, hits, joints, dbfile, p, fraction, 16, sses=lists, **settings), hits


def test_cli_all_vs_all(golden_dir, small):
    want, hits = library_table(small, list(range(586)), None, SMALL_DB, 1e-3, 0.5)
    assert sum(hits) > 0 and min(hits) == 0
    got = cli(golden_dir, ["-a", SMALL_DB, "-W", "1e-3"])
    assert got.returncode == 0, got.stderr.decode()[-400:]
    assert got.stdout.decode().splitlines() == want
    assert got.stdout.count(b"# CORE sses = ") > 10 and b"# CORE none\n" in got.stdout
    # no row and no map crossed: the bytes are the counters'
    assert b"copied %d bytes of results from the GPU(s)\n" % profile_bytes(small.orders) in got.stderr
    # the shards cannot show
    again = cli(golden_dir, ["-a", SMALL_DB, "-W", "1e-3", "-g", "1"])
    two = cli(golden_dir, ["-a", SMALL_DB, "-W", "1e-3", "-G", "0,0"])
    assert again.returncode == 0 and two.returncode == 0, two.stderr.decode()[-400:]
    assert again.stdout == got.stdout and two.stdout == got.stdout


def test_cli_query_lists_and_motifs(golden_dir, small):
    names = list(small.names)
    picks = [3, 100, 585, 250]
    big = max(picks, key=lambda e: small.orders[e])
    motif = list(range(int(small.orders[big]) - 1, -1, -2))[:6]
    assert len(motif) >= 2
    stdin = "".join(names[e] + "\n" for e in picks) + "%s@%s\n" % (names[big], ",".join(str(i + 1) for i in motif))
    entries, lists = picks + [big], [None] * len(picks) + [motif]
    want, _ = library_table(small, entries, lists, SMALL_DB, 0.01, 0.25)
    assert "# QUERY SSES = " + ",".join(str(i + 1) for i in motif) in want
    for option in ("-Q", "-q"):
        got = cli(golden_dir, [option, SMALL_DB, "-W", "0.01", "-f", "0.25"], stdin.encode())
        assert got.returncode == 0, got.stderr.decode()[-400:]
        assert got.stdout.decode().splitlines() == want, option
    # -q with SIDs alone, the settings' header lines, and LORDER's default
    want, _ = library_table(small, picks, None, SMALL_DB, 0.01, 0.5)
    got = cli(golden_dir, ["-q", SMALL_DB, "-W", "0.01"], "".join(names[e] + "\n" for e in picks).encode())
    assert got.returncode == 0 and got.stdout.decode().splitlines() == want
    got = cli(golden_dir, ["-q", SMALL_DB, "-W", "0.01", "-P", "2", "-A", "-F", "0.05"], "".join(names[e] + "\n" for e in picks).encode())
    assert got.returncode == 0, got.stderr.decode()[-400:]
    out = got.stdout.decode().splitlines()
    assert out[0] == want[0] and out[1] == "# POLISH tops = 2 all rows" and out[2].startswith("# GUMBEL censor = 0.05 fitted = ")
    assert out[3].startswith("# QUERY %s sses = " % names[picks[0]])


def test_cli_query_file_has_no_node(golden_dir):
    """a query that comes from a file is no entry: its own copy in the database counts, and LSOLN = F in the input does
    not matter"""
    got = cli(golden_dir, ["-W", "1"], open(os.path.join(golden_dir, "d1ubia_.input"), "rb").read())
    assert got.returncode == 0, got.stderr.decode()[-400:]
    out = got.stdout.decode().splitlines()
    assert out[0].startswith("# PROFILE dbfile = ") and out[0].endswith(" pvalue <= 1 fraction >= 0.5 restarts = 16 queries = 1")
    n = int(out[1].split()[-1])
    assert out[1].startswith("# QUERY ") and n > 0
    n1 = int(out[1].split()[5])
    assert out[2].startswith("# CORE ") and len(out) == 3 + n1
    assert all(int(x) <= n for line in out[3:] for x in line.split()[2:])


def test_cli_core_feeds_back_as_a_motif_query(tmp_path):
    """the loop the mode exists for: a family member's # CORE line, fed back as a -Q line, is accepted and finds the
    family's members among its hits at the same cutoff"""
    db, where = family_db()
    db.write_ascii(str(tmp_path / "family.ascii"))
    member = where[0][0]
    got = cli(str(tmp_path), ["-Q", "family.ascii", "-W", "1e-3"], (db.names[member] + "\n").encode())
    assert got.returncode == 0, got.stderr.decode()[-400:]
    out = got.stdout.decode().splitlines()
    hits = int(out[1].split()[-1])
    assert out[2].startswith("# CORE sses = "), out[:3]
    line = out[2].split(" ")[-1]
    assert line.startswith(db.names[member] + "@") and hits >= 3
    back = cli(str(tmp_path), ["-Q", "family.ascii", "-p", "1e-3"], (line + "\n").encode())
    assert back.returncode == 0, back.stderr.decode()[-400:]
    assert ("# QUERY SSES = " + line.split("@")[1]).encode() in back.stdout
    found = set(r.split()[0] for r in back.stdout.decode().splitlines() if not r.startswith("#"))
    family = set(db.names[e] for e in where[0])
    assert len(found & family) >= 4, (found, family)
