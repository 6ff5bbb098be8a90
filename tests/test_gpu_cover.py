"""Clustering the database around representatives on the GPU (-m gpu): sat_cover_begin / add / solve / end, their shards
and the command line's -a -D P.  The expected tables never come from the code under test: they are cover_lib's naive
greedy loop over edges taken from the planted score matrix itself, from hits_cutoff(P)'s rows of the same search, or from
the rows `-a -p P` prints."""
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import _native, report
import cover_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
SMALL_DB = "tableauxdistmatrixdb.small.ascii"
N = 1500                                       # > 1024: two blocks of rows per query, the second ragged
BATCHES = ((0, 700), (700, 701), (701, 1500))  # 700, 1 and 799 queries
P = 1e-3                                       # the planted graphs' cutoff
P_REAL = 1e-3                                  # the real scores' (test_real_scores says what it must give)


def solve_bytes(n, rounds, degree=True):
    """what a solve copies to the host (include/satabsearch.h): rep, degree, three counters and a flag per batch of rounds"""
    return 4 * n * (2 if degree else 1) + 24 + 8 * (rounds // _native.COVER_ROUND_BATCH + 1)


def check(got, want, what):
    """(rep, degree, edges, rounds) of a solve against cover_lib.cover's tuple, the sizes through report.cover_sizes"""
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    cover_lib.same(got, want, what)
    sizes, clusters = report.cover_sizes(got[0])
    assert np.array_equal(sizes, want[1]), what
    assert clusters == want[4] + int((want[1] == 1).sum()), what


def row_edges(rows, nodes):
    """the (query node, entry) pairs of hits_cutoff's rows"""
    a = np.concatenate([np.full(len(r), nodes[q], np.int64) for q, r in enumerate(rows)])
    b = np.concatenate([r["entry"].astype(np.int64) for r in rows])
    return a, b


# ---------------------------------------------------------------- 1. planted graphs
@pytest.fixture(scope="module")
def planted_db():
    return sat.synth.make_db(N, 8, 20, sort=False)


def planted_graphs():
    """name -> the planted cells (query rows, entry columns); a cell (q, e) is the row of query q against entry e"""
    rng = np.random.default_rng(1)
    g = {}
    order = rng.permutation(N - 1)
    g["path"] = (order + 1, order)                                          # (i + 1 -> i), dealt in shuffled order
    perm = rng.permutation(N)
    g["shuffled path"] = (perm[1:], perm[:-1])                              # a path through the nodes in random order
    g["star"] = (np.arange(N - 1), np.full(N - 1, N - 1))                   # every query's row against entry 1499
    clique = [np.arange(100, 140), np.arange(1004, 1044)]                   # the second one straddles the block edge at 1024
    cells = [(i, j) for c in clique for i in c for j in c if i != j] + [(139, 1004)]
    g["two cliques and a bridge"] = (np.array([c[0] for c in cells]), np.array([c[1] for c in cells]))
    g["random"] = (rng.integers(0, N, 20000), rng.integers(0, N, 20000))
    g["one query row"] = (np.full(N, 700), np.arange(N))                    # the batch of one query
    g["diagonal"] = (np.arange(N), np.arange(N))                            # self rows only
    g["perfect matching"] = (np.arange(1, N, 2), np.arange(0, N, 2))
    q, e = rng.integers(0, N, 6000), rng.integers(0, N, 6000)
    g["both directions"] = (np.concatenate([q, e]), np.concatenate([e, q]))
    # as the score matrix holds them: a cell drawn twice is one row
    for name, (q, e) in g.items():
        cells = np.zeros((N, N), bool)
        cells[q, e] = True
        g[name] = np.nonzero(cells)
    return g


@pytest.fixture(scope="module")
def planted_expected():
    """name -> cover_lib's table, computed once and left alone"""
    return {name: cover_lib.cover(N, q, e) for name, (q, e) in planted_graphs().items()}


def planted_scores(db, n, cells_q, cells_e):
    """0 everywhere, norm2 = 16 on the planted cells"""
    scores = np.zeros((n, n), np.int32)
    scores[cells_q, cells_e] = 8 * (db.orders[cells_q] + db.orders[cells_e])
    return scores


def plant(s, db, cells_q, cells_e, repeat=1, batches=BATCHES, begin=True, nodes=None):
    """One accumulator (of `nodes` nodes: default the entries) over the batches: every batch is searched (one restart,
    only to reach the searched state), its scores are overwritten and added `repeat` times"""
    n = len(db.orders)
    scores = planted_scores(db, n, cells_q, cells_e)
    if begin:
        s.cover_begin()
    for lo, hi in batches:
        s.set_queries_from_db(np.arange(lo, hi), lo)
        s.search(True, False, 1)
        s.debug_set_scores(scores[lo:hi])
        before = s.d2h_bytes()
        for _ in range(repeat):
            s.cover_add(P, np.arange(lo, hi))
        assert s.d2h_bytes() == before                      # nothing comes back from an add
    before = s.d2h_bytes()
    got = s.cover_solve()
    assert s.d2h_bytes() - before == solve_bytes(nodes or n, got[3])
    return got


@pytest.fixture(scope="module")
def planted_searcher(planted_db):
    with sat.Searcher(0) as s:
        s.upload(planted_db)
        yield s


def test_planted_p_values(planted_db):
    """the planted score is under the cutoff for every pair of orders of the database, a zero score is above it"""
    for n1 in (int(planted_db.orders.min()), int(planted_db.orders.max())):
        for n2 in (int(planted_db.orders.min()), int(planted_db.orders.max())):
            assert report.stats(8 * (n1 + n2), n1, n2)[2] <= P < report.stats(0, n1, n2)[2]


@pytest.mark.parametrize("name", list(planted_graphs()))
def test_planted_graph(planted_searcher, planted_db, planted_expected, name):
    q, e = planted_graphs()[name]
    want = planted_expected[name]
    rep, size, degree, edges, rounds = want
    if name == "diagonal":
        assert edges == 0 and rounds == 0 and np.array_equal(rep, np.arange(N))
    if name in ("star", "one query row"):
        assert rounds == 1 and (rep == (N - 1 if name == "star" else 700)).all() and edges == N - 1
    if name == "path":
        assert rounds == 500 and rep[:6].tolist() == [1, 1, 1, 4, 4, 4] and cover_lib.components(N, q, e) == 1
    if name == "shuffled path":
        assert edges == N - 1 and rounds > 400
    if name == "perfect matching":
        assert rounds == N // 2 and np.array_equal(rep, np.arange(N) // 2 * 2)
    if name == "two cliques and a bridge":
        # the bridge's ends 139 and 1004 have one neighbour more than their cliques' other members: 139 is picked first
        # and takes its clique and 1004; the second clique's smallest node left, 1005, takes the rest
        assert rounds == 2 and (rep[100:140] == 139).all() and rep[1004] == 139 and (rep[1005:1044] == 1005).all()
    if name == "both directions":
        assert edges <= 6000 and (degree.sum() == 2 * edges)
    got = plant(planted_searcher, planted_db, q, e, repeat=3)
    check(got, want, name)
    cover_lib.check_invariants(N, q, e, got[0])


# ---------------------------------------------------------------- 2. small sizes: the word edges of the bit matrix
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_word_edges(n):
    db = sat.synth.make_db(n, 8, 20, sort=False)
    rng = np.random.default_rng(n)
    with sat.Searcher(0) as s:
        s.upload(db)
        # a random graph; then the last node - the last valid bit of the last word - against all the others
        q, e = rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n)
        got = plant(s, db, q, e, batches=((0, n),))
        check(got, cover_lib.cover(n, q, e), "random, n = %d" % n)
        q, e = np.full(n, n - 1), np.arange(n)
        want = cover_lib.cover(n, q, e)
        assert (want[0] == n - 1).all() and want[3] == n - 1 and want[2][n - 1] == n - 1       # no padding bit counts
        check(plant(s, db, q, e, batches=((0, n),)), want, "last node against all, n = %d" % n)
        q, e = np.arange(n), np.full(n, n - 1)
        check(plant(s, db, q, e, batches=((0, n),)), want, "all against the last node, n = %d" % n)
        # rep alone: fewer bytes
        rep = np.zeros(n, np.int32)
        before = s.d2h_bytes()
        assert s._lib.sat_cover_solve(s._ctx, rep.ctypes.data, None, None, None) == 0
        assert s.d2h_bytes() - before == solve_bytes(n, want[4], degree=False) and np.array_equal(rep, want[0])


def test_ordinals_in_no_order():
    """entries whose ordinals in the whole database are a random permutation: the 64 rows of a wave fall into up to
    eleven words of the query's row, more groups than the add combines - the rest go lane by lane - and a dense graph
    keeps every lane busy.  The edges end at the ORDINALS of the planted entries"""
    n = 700
    db = sat.synth.make_db(n, 8, 20, sort=False)
    rng = np.random.default_rng(23)
    ordinal = rng.permutation(n)
    cells = rng.random((n, n)) < 0.3
    q, e = np.nonzero(cells)
    want = cover_lib.cover(n, q, ordinal[e])
    assert want[3] > 80000 and want[4] >= 3
    with sat.Searcher(0) as s:
        s.upload(db, db_ordinal=ordinal)
        s.cover_begin(n)
        s.set_queries_from_db(np.arange(n), 0)
        s.search(True, False, 1)
        s.debug_set_scores(planted_scores(db, n, q, e))
        for _ in range(2):
            s.cover_add(P, np.arange(n))
        got = s.cover_solve()
    check(got, want, "ordinals in no order")
    cover_lib.check_invariants(n, q, ordinal[e], got[0])


# ---------------------------------------------------------------- 3. the accumulator's life
def test_solve_add_solve_and_begin_after_upload(planted_db, planted_expected):
    graphs = planted_graphs()
    q1, e1 = graphs["path"]
    q2, e2 = graphs["two cliques and a bridge"]
    with sat.Searcher(0) as s:
        with pytest.raises(sat.SatError, match=r"\[-5\].*no database"):
            s.cover_begin(N)
        s.upload(planted_db)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_cover_begin"):
            s.cover_solve()
        check(plant(s, planted_db, q1, e1), planted_expected["path"], "first solve")
        # more rows into the same accumulator: one solve over the union
        got = plant(s, planted_db, q2, e2, begin=False)
        union = cover_lib.cover(N, np.concatenate([q1, q2]), np.concatenate([e1, e2]))
        assert not np.array_equal(union[0], planted_expected["path"][0]) and union[3] > planted_expected["path"][3]
        check(got, union, "solve, add more, solve again")
        check(s.cover_solve(), union, "a second solve of the same matrix")
        # bad arguments leave it as it was
        nodes = np.arange(*BATCHES[-1], dtype=np.int32)
        bad = nodes.copy()
        bad[3] = N
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 3: node 1500 "):
            s.cover_add(P, bad)
        for p in (float("nan"), float("inf"), -1.0):
            with pytest.raises(sat.SatError, match=r"\[-1\].*max_pvalue"):
                s.cover_add(p, nodes)
        assert s._lib.sat_cover_add(s._ctx, 0.5, None) == -1 and s._lib.sat_cover_solve(s._ctx, None, None, None, None) == -1
        with pytest.raises(sat.SatError, match=r"\[-1\].*n_nodes"):
            s.cover_begin(0)
        with pytest.raises(sat.SatError, match=r"\[-1\].*ordinal 1499"):
            s.cover_begin(N - 1)
        check(s.cover_solve(), union, "after the rejected calls")
        # an upload drops it; begin afterwards starts empty
        s.upload(planted_db)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_cover_begin"):
            s.cover_solve()
        s.cover_begin()
        rep, degree, edges, rounds = s.cover_solve()
        assert np.array_equal(rep, np.arange(N)) and not degree.any() and edges == 0 and rounds == 0
        # more nodes than entries: the rest stay singletons
        s.cover_begin(N + 70)
        got = plant(s, planted_db, q2, e2, begin=False, nodes=N + 70)
        check(got, cover_lib.cover(N + 70, q2, e2), "more nodes than entries")
        s.cover_end()
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_cover_begin"):
            s.cover_solve()


def cluster_expected(n, a, b):
    """(labels, degrees, edges) as sat_cluster_labels defines them: rows counted, self rows nowhere"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    keep = a != b
    a, b = a[keep], b[keep]
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for x, y in zip(a.tolist(), b.tolist()):
        x, y = find(x), find(y)
        if x != y:
            parent[max(x, y)] = min(x, y)
    degrees = (np.bincount(a, minlength=n) + np.bincount(b, minlength=n)).astype(np.int32)
    return np.array([find(v) for v in range(n)], np.int32), degrees, int(len(a))


def test_a_cover_and_a_cluster_accumulator_coexist(planted_searcher, planted_db, planted_expected):
    """both fed the same rows on one context: each gives its own expected table"""
    s = planted_searcher
    q, e = planted_graphs()["both directions"]
    scores = planted_scores(planted_db, N, q, e)
    s.cover_begin()
    s.cluster_begin()
    for lo, hi in BATCHES:
        s.set_queries_from_db(np.arange(lo, hi), lo)
        s.search(True, False, 1)
        s.debug_set_scores(scores[lo:hi])
        s.cover_add(P, np.arange(lo, hi))
        s.cluster_add(P, np.arange(lo, hi))
    labels, degrees, edges = s.cluster_labels()
    check(s.cover_solve(), planted_expected["both directions"], "cover beside a cluster accumulator")
    want = cluster_expected(N, q, e)
    assert np.array_equal(labels, want[0]) and np.array_equal(degrees, want[1]) and edges == want[2]
    assert edges == 2 * planted_expected["both directions"][3]             # rows there, distinct pairs here
    again = s.cluster_labels()
    assert np.array_equal(again[0], labels) and np.array_equal(again[1], degrees) and again[2] == edges
    s.cluster_end()
    check(s.cover_solve(), planted_expected["both directions"], "after cluster_end")
    s.cover_end()


def test_call_sequence(planted_searcher, planted_db):
    """search, cover_add, hits_cutoff, cluster_add on one context: the rows and labels of the same calls without the
    cover calls"""
    s = planted_searcher
    q, e = planted_graphs()["random"]
    lo, hi = BATCHES[0]
    scores = planted_scores(planted_db, N, q, e)[lo:hi]
    nodes = np.arange(lo, hi)

    def sequence(with_cover):
        if with_cover:
            s.cover_begin()
        s.cluster_begin()
        s.set_queries_from_db(nodes, lo)
        s.search(True, False, 1)
        s.debug_set_scores(scores)
        if with_cover:
            s.cover_add(P, nodes)
        rows = s.hits_cutoff(P)
        s.cluster_add(P, nodes)
        out = (rows, s.cluster_labels(), s.cover_solve() if with_cover else None)
        s.cluster_end()
        return out

    plain = sequence(False)
    mixed = sequence(True)
    assert len(plain[0]) == len(mixed[0]) == hi - lo
    for r0, r1 in zip(plain[0], mixed[0]):
        assert np.array_equal(r0, r1)
    for x, y in zip(plain[1], mixed[1]):
        assert np.array_equal(x, y)
    keep = (q >= lo) & (q < hi)
    check(mixed[2], cover_lib.cover(N, q[keep], e[keep]), "the cover of the sequence")
    s.cover_end()


# ---------------------------------------------------------------- 4. real scores, shards
@pytest.fixture(scope="module")
def small(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, SMALL_DB))
    assert len(db) == 586
    return db


SMALL_BATCHES = ((0, 256), (256, 512), (512, 586))


@pytest.fixture(scope="module")
def small_single(small):
    """(the solve of one context, cover_lib's table of hits_cutoff(P_REAL)'s rows of the same searches, those rows' pairs)"""
    n = len(small)
    a, b = [], []
    with sat.Searcher(0) as s:
        s.upload(small)
        s.cover_begin()
        for lo, hi in SMALL_BATCHES:
            s.set_queries_from_db(np.arange(lo, hi), lo)
            s.search(True, False, 16)
            qa, qb = row_edges(s.hits_cutoff(P_REAL), np.arange(lo, hi))
            a.append(qa)
            b.append(qb)
            s.cover_add(P_REAL, np.arange(lo, hi))
        got = s.cover_solve()
    a, b = np.concatenate(a), np.concatenate(b)
    return got, cover_lib.cover(n, a, b), (a, b)


def test_real_scores(small_single):
    got, want, (a, b) = small_single
    n = 586
    # the expected side first, so that a degenerate graph cannot hide a failure: enough clusters of three or more, and
    # more clusters than single linkage makes of the same edges - chains are cut
    sizes_of_reps = want[1][want[0] == np.arange(n)]
    assert (sizes_of_reps >= 3).sum() >= 10, sizes_of_reps
    assert len(sizes_of_reps) > cover_lib.components(n, a, b)
    check(got, want, "real scores, P = %g" % P_REAL)
    cover_lib.check_invariants(n, a, b, got[0])


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2", "3"])
def test_shards_equal_one_context(small, small_single, devices):
    """every shard adds the rows of its own entries; the solve ORs the matrices and gives one context's result"""
    n = len(small)
    with sat.MultiSearcher(len(devices), devices=devices) as m:
        m.upload(small)
        assert m.ndev == len(devices)
        m.set_queries_from_db(np.arange(4), 0)
        m.search_only(True, False, 1)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_cover_begin"):
            m.cover_add(0.5, np.arange(4))
        m.cover_begin()
        for lo, hi in SMALL_BATCHES:
            m.set_queries_from_db(np.arange(lo, hi), lo)
            m.search_only(True, False, 16)
            before = m.d2h_bytes()
            m.cover_add(P_REAL, np.arange(lo, hi))
            assert m.d2h_bytes() == before
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 1: node 586 "):
            m.cover_add(0.5, [0, n] + [0] * (SMALL_BATCHES[-1][1] - SMALL_BATCHES[-1][0] - 2))
        before = m.d2h_bytes()
        got = m.cover_solve()
        # the other shards' matrices cross once each, then the solve's own bytes
        assert m.d2h_bytes() - before == (len(devices) - 1) * n * ((n + 63) // 64) * 8 + solve_bytes(n, got[3])
        single = small_single[0]
        assert np.array_equal(got[0], single[0]) and np.array_equal(got[1], single[1]) and got[2:] == single[2:]
        again = m.cover_solve()                              # the OR is idempotent
        assert np.array_equal(again[0], single[0]) and np.array_equal(again[1], single[1]) and again[2:] == single[2:]


# ---------------------------------------------------------------- 5. command line
def cli(golden_dir, args):
    return subprocess.run([CLI, "-r", "16", *args], input=b"not read\n", cwd=golden_dir, capture_output=True, timeout=300)


def table_from_rows(stdout, names):
    """the -D table that follows from the rows `-a db -p P` printed: names -> cover_lib"""
    index = {name: i for i, name in enumerate(names)}
    assert len(index) == len(names)
    a, b, q = [], [], None
    for line in stdout.decode().splitlines():
        if line.startswith("# QUERY ID = "):
            q = index[line[len("# QUERY ID = "):].strip()]
        elif not line.startswith("#"):
            a.append(q)
            b.append(index[line.split()[0]])
    rep, size, degree, edges, rounds = cover_lib.cover(len(names), a, b)
    lines = ["%-8s %-8s %d %d" % (name, names[rep[v]], size[v], degree[v]) for v, name in enumerate(names)]
    return lines, int((rep == np.arange(len(names))).sum()), int((size == 1).sum()), edges, rounds


@pytest.mark.parametrize("options", [[], ["-G", "0,0"], ["-F", "0.1"], ["-P", "2", "-A"]], ids=["plain", "G00", "F0.1", "P2A"])
def test_cli_table_follows_from_the_p_rows(golden_dir, options):
    cutoff = "0.001"
    names = list(sat.StructSet.read(os.path.join(golden_dir, SMALL_DB)).names)
    rows = cli(golden_dir, ["-a", SMALL_DB, "-p", cutoff, *options])
    got = cli(golden_dir, ["-a", SMALL_DB, "-D", cutoff, *options])
    assert rows.returncode == 0 and got.returncode == 0, got.stderr.decode()[-400:]
    lines, clusters, singletons, edges, rounds = table_from_rows(rows.stdout, names)
    out = got.stdout.decode().splitlines()
    assert out[0] == ("# COVER dbfile = %s entries = %d pvalue <= %s restarts = 16 clusters = %d singletons = %d edges = %d "
                      "rounds = %d" % (SMALL_DB, len(names), cutoff, clusters, singletons, edges, rounds))
    head = 1
    if "-P" in options:
        assert out[head] == "# POLISH tops = 2 all rows"
        head += 1
    if "-F" in options:
        fitted = rows.stdout.count(b"# GUMBEL a = ")
        assert out[head] == "# GUMBEL censor = 0.1 fitted = %d of %d" % (fitted, len(names)) and fitted > 0
        head += 1
    assert out[head:] == lines
    assert edges > 0 and 1 < clusters < len(names) and rounds > 0
    assert got.stderr.count(b"GPU execution time") == rows.stderr.count(b"GPU execution time") == (len(names) + 255) // 256


def test_cli_trivial_tables(golden_dir, small):
    """-D 1: every row is an edge, the graph is complete and the first structure represents everyone.  -D 0: the rows
    `-p 0` prints - none but rows whose p-value is exactly 0 - and with no such row every structure is alone"""
    names, n = list(small.names), len(small)
    got = cli(golden_dir, ["-a", SMALL_DB, "-D", "1"])
    assert got.returncode == 0, got.stderr.decode()[-400:]
    out = got.stdout.decode().splitlines()
    assert out[0] == "# COVER dbfile = %s entries = %d pvalue <= 1 restarts = 16 clusters = 1 singletons = 0 edges = %d rounds = 1" % (
        SMALL_DB, n, n * (n - 1) // 2)
    assert out[1:] == ["%-8s %-8s %d %d" % (name, names[0], n, n - 1) for name in names]
    rows = cli(golden_dir, ["-a", SMALL_DB, "-p", "0"])
    got = cli(golden_dir, ["-a", SMALL_DB, "-D", "0"])
    assert rows.returncode == 0 and got.returncode == 0, got.stderr.decode()[-400:]
    lines, clusters, singletons, edges, rounds = table_from_rows(rows.stdout, names)
    out = got.stdout.decode().splitlines()
    assert out[0] == "# COVER dbfile = %s entries = %d pvalue <= 0 restarts = 16 clusters = %d singletons = %d edges = %d rounds = %d" % (
        SMALL_DB, n, clusters, singletons, edges, rounds)
    assert out[1:] == lines
    if edges == 0:
        assert clusters == singletons == n and lines == ["%-8s %-8s 1 0" % (name, name) for name in names]


def test_cli_without_D_prints_what_it_printed(golden_dir):
    """-a db -L P is not touched by the new option: it prints no COVER line and the same bytes twice"""
    one = cli(golden_dir, ["-a", SMALL_DB, "-L", "0.001"])
    two = cli(golden_dir, ["-a", SMALL_DB, "-L", "0.001"])
    assert one.returncode == 0 and one.stdout == two.stdout and one.stdout.startswith(b"# CLUSTER dbfile = ")
    assert b"COVER" not in one.stdout and b"rounds" not in one.stdout
