"""Single-linkage clustering of the database on the GPU (-m gpu): sat_cluster_begin / add / labels / end, their shards
and the command line's -a -L P.  The expected labels, degrees and edge counts never come from the code under test: they
are a union-find in Python over edges taken from the planted score matrix itself, from hits_cutoff(P)'s rows of the same
search, or from the rows `-a -p P` prints."""
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import report
import edge_cases as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
SMALL_DB = "tableauxdistmatrixdb.small.ascii"
N = 1500                                       # > 1024: two blocks of rows per query, the second ragged
BATCHES = ((0, 700), (700, 701), (701, 1500))  # 700, 1 and 799 queries
P = 1e-3


# ---------------------------------------------------------------- the reference
def components(n, a, b):
    """label[v] = the smallest node of v's connected component under the edges (a[i], b[i]): a plain union-find"""
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        x, y = find(x), find(y)
        if x != y:
            parent[max(x, y)] = min(x, y)
    return np.array([find(v) for v in range(n)], np.int32)


def components_by_propagation(n, a, b):
    """the same labels for long edge lists, in numpy: every node takes the smallest label among itself and its
    neighbours, then its label's label, until nothing moves - labels only fall, stay inside the component, and at the
    fixed point are constant along every edge, so each is its component's smallest node"""
    labels = np.arange(n)
    while True:
        low = np.minimum(labels[a], labels[b])
        new = labels.copy()
        np.minimum.at(new, a, low)
        np.minimum.at(new, b, low)
        new = new[new]
        if np.array_equal(new, labels):
            return labels.astype(np.int32)
        labels = new


def expected(n, a, b):
    """(labels, degrees, edges) of the rows (a[i], b[i]) by the definition: self rows are no edges and are counted
    nowhere, repeats count each time.  The union-find runs over each pair once - repeats do not change a component -
    and hands lists of more than 30 000 pairs (the dense graphs of the real scores at large cutoffs) to the propagation;
    test_planted_graph checks the two against each other."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    keep = a != b
    a, b = a[keep], b[keep]
    degrees = (np.bincount(a, minlength=n) + np.bincount(b, minlength=n)).astype(np.int32)
    pairs = np.unique(np.minimum(a, b) * n + np.maximum(a, b))
    find = components if len(pairs) <= 30000 else components_by_propagation
    return find(n, pairs // n, pairs % n), degrees, int(len(a))


def same(got, want, what):
    labels, degrees, edges = got
    assert labels.dtype == np.int32 and degrees.dtype == np.int32
    assert np.array_equal(labels, want[0]), "%s: labels differ at %s" % (what, np.nonzero(labels != want[0])[0][:8])
    assert np.array_equal(degrees, want[1]), "%s: degrees differ at %s" % (what, np.nonzero(degrees != want[1])[0][:8])
    assert edges == want[2], "%s: %d edges, expected %d" % (what, edges, want[2])


def row_edges(rows, nodes, offset=0):
    """the (query node, entry) pairs of hits_cutoff's rows: nodes[q] for every row of query q, the rows' entries"""
    a = np.concatenate([np.full(len(r), nodes[q], np.int64) for q, r in enumerate(rows)])
    b = np.concatenate([r["entry"].astype(np.int64) for r in rows]) + offset
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
    clique = [np.arange(100, 140), np.arange(1040, 1080)]                   # the second one straddles the block edge
    cells = [(i, j) for c in clique for i in c for j in c if i != j] + [(139, 1040)]
    g["two cliques and a bridge"] = (np.array([c[0] for c in cells]), np.array([c[1] for c in cells]))
    g["random"] = (rng.integers(0, N, 20000), rng.integers(0, N, 20000))
    g["one query row"] = (np.full(N, 700), np.arange(N))                    # the batch of one query: one root, 1499 edges
    g["diagonal"] = (np.arange(N), np.arange(N))                            # self rows only
    # as the score matrix holds them: a cell drawn twice is one row
    for name, (q, e) in g.items():
        cells = np.zeros((N, N), bool)
        cells[q, e] = True
        g[name] = np.nonzero(cells)
    return g


def plant(s, db, cells_q, cells_e, repeat=1):
    """One accumulator over the three batches: every batch is searched (one restart, only to reach the searched state),
    its scores are overwritten - 0 everywhere, norm2 = 16 on the planted cells - and added `repeat` times."""
    scores = np.zeros((N, N), np.int32)
    scores[cells_q, cells_e] = 8 * (db.orders[cells_q] + db.orders[cells_e])
    s.cluster_begin()
    for lo, hi in BATCHES:
        s.set_queries_from_db(np.arange(lo, hi), lo)
        s.search(True, False, 1)
        s.debug_set_scores(scores[lo:hi])
        before = s.d2h_bytes()
        for _ in range(repeat):
            s.cluster_add(P, np.arange(lo, hi))
        assert s.d2h_bytes() == before                      # nothing comes back from an add
    before = s.d2h_bytes()
    got = s.cluster_labels()
    assert s.d2h_bytes() - before == 8 * N + 8
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
            assert report.stats(8 * (n1 + n2), n1, n2)[0] == 16.0
            assert report.stats(8 * (n1 + n2), n1, n2)[2] <= P < report.stats(0, n1, n2)[2]


@pytest.mark.parametrize("name", list(planted_graphs()))
def test_planted_graph(planted_searcher, planted_db, name):
    q, e = planted_graphs()[name]
    want = expected(N, q, e)
    if name == "diagonal":
        assert want[2] == 0 and not want[1].any() and np.array_equal(want[0], np.arange(N))
    if name in ("path", "shuffled path", "star", "one query row"):
        assert not want[0].any() and want[2] == N - 1
    if name == "random":
        assert 19000 < want[2] <= 20000
        assert np.array_equal(components_by_propagation(N, q, e), want[0])
    if name == "two cliques and a bridge":
        assert (want[0][100:140] == 100).all() and (want[0][1040:1080] == 100).all() and (want[0] != np.arange(N)).sum() == 79
    same(plant(planted_searcher, planted_db, q, e), want, name)


def test_planted_graph_added_twice(planted_searcher, planted_db):
    q, e = planted_graphs()["random"]
    once = expected(N, q, e)
    got = plant(planted_searcher, planted_db, q, e, repeat=2)
    same(got, (once[0], 2 * once[1], 2 * once[2]), "random, twice")
    # labels may be read between adds: the accumulator goes on
    s = planted_searcher
    s.cluster_add(P, np.arange(*BATCHES[-1]))
    lo, hi = BATCHES[-1]
    keep = (q >= lo) & (q < hi)
    third = expected(N, q[keep], e[keep])
    labels, degrees, edges = s.cluster_labels()
    assert np.array_equal(labels, once[0]) and np.array_equal(degrees, 2 * once[1] + third[1]) and edges == 2 * once[2] + third[2]


# ---------------------------------------------------------------- 2. real scores
@pytest.fixture(scope="module")
def small(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, SMALL_DB))
    assert len(db) == 586
    return db


SMALL_BATCHES = ((0, 256), (256, 512), (512, 586))


def cutoffs_of(pvalues):
    distinct = np.unique(pvalues)
    return np.unique(np.concatenate([distinct, np.nextafter(distinct, -np.inf), [0.0, 1.0]]).clip(0.0, None))


@pytest.fixture(scope="module")
def small_cutoffs(small):
    """every distinct p-value the rows of the all-vs-all search show (r = 16, LORDER T), nextafter below each, 0 and 1"""
    with sat.Searcher(0) as s:
        s.upload(small)
        pv = []
        for lo, hi in SMALL_BATCHES:
            s.set_queries_from_db(np.arange(lo, hi), lo)
            s.search(True, False, 16)
            pv += [r["pvalue"] for r in s.hits_cutoff(1.0)]
    return cutoffs_of(np.concatenate(pv))


@pytest.fixture(scope="module")
def small_single(small, small_cutoffs):
    """cutoff -> ((labels, degrees, edges) of one context, the same from hits_cutoff(P)'s rows of the same searches)"""
    out = {}
    n = len(small)
    with sat.Searcher(0) as s:
        s.upload(small)
        for p in small_cutoffs:
            s.cluster_begin()
            a, b = [], []
            for lo, hi in SMALL_BATCHES:
                s.set_queries_from_db(np.arange(lo, hi), lo)
                s.search(True, False, 16)
                qa, qb = row_edges(s.hits_cutoff(float(p)), np.arange(lo, hi))
                a.append(qa)
                b.append(qb)
                s.cluster_add(float(p), np.arange(lo, hi))
            out[float(p)] = (s.cluster_labels(), expected(n, np.concatenate(a), np.concatenate(b)))
    return out


def test_real_scores_every_cutoff(small_single, small_cutoffs):
    assert len(small_cutoffs) >= 4 and small_cutoffs[0] == 0.0 and small_cutoffs[-1] == 1.0
    interesting = []
    for p, (got, want) in small_single.items():
        same(got, want, "P = %r" % p)
        sizes = np.bincount(want[0])
        if (sizes >= 2).sum() >= 2 and (sizes == 1).sum() >= 1:
            interesting.append(p)
    assert interesting, "no cutoff of %s cuts the database into >= 2 clusters of >= 2 members and >= 1 singleton" % (
        small_cutoffs.tolist(),)
    # P = 1 takes every row: one component, every node 2 * (N - 1) edges
    got = small_single[1.0][0]
    assert not got[0].any() and (got[1] == 2 * 585).all() and got[2] == 586 * 585


# ---------------------------------------------------------------- 3. fitted and polished rows
@pytest.fixture(scope="module")
def edge(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, ec.EDGE_DB))
    assert len(db) == 28 and tuple(db.orders) == ec.EDGE_ORDERS
    return db


@pytest.mark.parametrize("mode", ["fitted", "polished", "polished and fitted"])
def test_add_follows_hits_cutoff(edge, mode):
    n = len(edge)
    nodes = np.arange(n)
    with sat.Searcher(0) as s:
        s.upload(edge)
        s.set_queries_from_db(nodes, 0)
        s.search(True, False, 16)
        plain = np.concatenate([r["pvalue"] for r in s.hits_cutoff(1.0)])
        if "polished" in mode:
            s.set_polish_all(2)
            s.search(True, False, 16)
        if "fitted" in mode:
            fits = s.fit_statistics(0.05)
            assert fits["fitted"].any()
        pv = np.concatenate([r["pvalue"] for r in s.hits_cutoff(1.0)])
        assert len(pv) == n * n and not np.array_equal(np.sort(pv), np.sort(plain))      # the rows' statistics did move
        for p in cutoffs_of(pv):
            a, b = row_edges(s.hits_cutoff(float(p)), nodes)
            s.cluster_begin()
            s.cluster_add(float(p), nodes)
            same(s.cluster_labels(), expected(n, a, b), "%s, P = %r" % (mode, p))
        if "fitted" in mode:                                   # the add left the fit installed
            assert np.array_equal(np.concatenate([r["pvalue"] for r in s.hits_cutoff(1.0)]), pv)


# ---------------------------------------------------------------- 4. state and errors
def test_state_and_errors(edge):
    n = len(edge)
    nodes = np.arange(n, dtype=np.int32)
    with sat.Searcher(0) as s:
        lib, ctx = s._lib, s._ctx
        with pytest.raises(sat.SatError, match=r"\[-5\].*no database"):
            s.cluster_begin(n)
        s.upload(edge)
        s.set_queries_from_db(nodes, 0)
        s.search(True, False, 16)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_cluster_begin"):          # add before begin
            s.cluster_add(0.5, nodes)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_cluster_begin"):
            s.cluster_labels()
        with pytest.raises(sat.SatError, match=r"\[-1\].*n_nodes"):
            s.cluster_begin(0)
        s.cluster_begin()
        s.set_queries_from_db(nodes, 0)
        with pytest.raises(sat.SatError, match=r"\[-5\].*no search has run"):          # add before a search
            s.cluster_add(0.5, nodes)
        s.search(True, False, 16)
        a, b = row_edges(s.hits_cutoff(0.5), nodes)
        want = expected(n, a, b)
        assert want[2] > 0
        s.cluster_add(0.5, nodes)
        same(s.cluster_labels(), want, "first add")
        # every rejected call leaves the accumulator as it was
        bad = nodes.copy()
        bad[3] = -1
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 3: node -1 "):
            s.cluster_add(0.5, bad)
        bad[3], bad[27] = 3, n
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 27: node 28 "):
            s.cluster_add(0.5, bad)
        assert lib.sat_cluster_add(ctx, 0.5, None) == -1
        for p in (float("nan"), float("inf"), -1.0):
            with pytest.raises(sat.SatError, match=r"\[-1\].*max_pvalue"):
                s.cluster_add(p, nodes)
        with pytest.raises(sat.SatError, match=r"\[-1\].*n_nodes"):
            s.cluster_begin(-3)
        assert lib.sat_cluster_labels(ctx, None, None, None) == -1
        same(s.cluster_labels(), want, "after the rejected calls")
        # degree and edges may be NULL: fewer bytes
        labels = np.zeros(n, np.int32)
        before = s.d2h_bytes()
        assert lib.sat_cluster_labels(ctx, labels.ctypes.data, None, None) == 0
        assert s.d2h_bytes() - before == 4 * n and np.array_equal(labels, want[0])
        # more nodes than entries: the rest stay singletons; begin again resets
        s.cluster_begin(n + 5)
        labels, degrees, edges = s.cluster_labels()
        assert np.array_equal(labels, np.arange(n + 5)) and not degrees.any() and edges == 0
        s.cluster_add(0.5, nodes + 5)                          # the queries are nodes 5 .. n + 4 now
        same(s.cluster_labels(), expected(n + 5, a + 5, b), "shifted query nodes")
        s.cluster_begin()
        s.cluster_add(0.5, nodes)
        same(s.cluster_labels(), want, "begin twice")
        # searches and query changes keep the accumulator, an upload drops it
        s.set_queries_from_db(nodes[:5], 0)
        s.search(True, False, 16)
        same(s.cluster_labels(), want, "after a query change and a search")
        s.upload(edge)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_cluster_begin"):
            s.cluster_labels()
        s.search(True, False, 16)                              # (the batch of five is still set)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_cluster_begin"):
            s.cluster_add(0.5, nodes[:5])
        # ordinals of a shard: n_nodes must cover them
        s.upload(edge, db_ordinal=np.arange(n) + 100)
        with pytest.raises(sat.SatError, match=r"\[-1\].*ordinal 127"):
            s.cluster_begin(127)
        s.cluster_begin(128)
        s.set_queries_from_db(nodes, 0)
        s.search(True, False, 16)
        a, b = row_edges(s.hits_cutoff(0.5), nodes, offset=100)
        s.cluster_add(0.5, nodes)
        same(s.cluster_labels(), expected(128, a, b), "entries at ordinals 100 .. 127")
        s.cluster_end()
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_cluster_begin"):
            s.cluster_labels()


# ---------------------------------------------------------------- 5. shards
@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]], ids=["1", "2", "3"])
def test_shards_equal_one_context(small, small_cutoffs, small_single, devices):
    """Real scores only: the bindings expose no shard's context to plant scores through.  Every cutoff of test 2, the
    shards' accumulators joined on the host, against the arrays of the single context."""
    n = len(small)
    with sat.MultiSearcher(len(devices), devices=devices) as m:
        m.upload(small)
        assert m.ndev == len(devices)
        m.set_queries_from_db(np.arange(4), 0)
        m.search_only(True, False, 1)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_cluster_begin"):
            m.cluster_add(0.5, np.arange(4))
        for p in small_cutoffs:
            m.cluster_begin()
            for lo, hi in SMALL_BATCHES:
                m.set_queries_from_db(np.arange(lo, hi), lo)
                m.search_only(True, False, 16)
                before = m.d2h_bytes()
                m.cluster_add(float(p), np.arange(lo, hi))
                assert m.d2h_bytes() == before
            before = m.d2h_bytes()
            got = m.cluster_labels()
            assert m.d2h_bytes() - before == len(devices) * (8 * n + 8)
            same(got, small_single[float(p)][0], "%d shards, P = %r" % (len(devices), p))
        # search_only leaves a searched state the other device-side calls work on
        rows = m.hits_cutoff(float(small_cutoffs[1]))
        assert len(rows) == SMALL_BATCHES[-1][1] - SMALL_BATCHES[-1][0]
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 1: node 586 "):
            m.cluster_add(0.5, [0, n] + [0] * (len(rows) - 2))


# ---------------------------------------------------------------- 6. command line
def cli(golden_dir, args):
    return subprocess.run([CLI, "-r", "16", *args], input=b"not read\n", cwd=golden_dir, capture_output=True, timeout=300)


def table_from_rows(stdout, names):
    """the -L table that follows from the rows `-a db -p P` printed: names -> union-find -> representatives by degree"""
    index = {name: i for i, name in enumerate(names)}
    assert len(index) == len(names)
    a, b, q = [], [], None
    for line in stdout.decode().splitlines():
        if line.startswith("# QUERY ID = "):
            q = index[line[len("# QUERY ID = "):].strip()]
        elif not line.startswith("#"):
            a.append(q)
            b.append(index[line.split()[0]])
    labels, degrees, edges = expected(len(names), a, b)
    sizes = np.bincount(labels, minlength=len(names))
    lines = []
    for v, name in enumerate(names):
        members = np.nonzero(labels == labels[v])[0]
        rep = members[np.argmax(degrees[members])]
        lines.append("%-8s %-8s %d %d" % (name, names[rep], sizes[labels[v]], degrees[v]))
    return lines, int((sizes > 0).sum()), int((sizes == 1).sum()), edges


@pytest.mark.parametrize("db,options", [(SMALL_DB, []), (SMALL_DB, ["-G", "0,0"]), (SMALL_DB, ["-F", "0.05"]),
                                        (SMALL_DB, ["-P", "2", "-A"])], ids=["plain", "G00", "F0.05", "P2A"])
def test_cli_table_follows_from_the_p_rows(golden_dir, db, options):
    cutoff = "0.001"
    names = list(sat.StructSet.read(os.path.join(golden_dir, db)).names)
    rows = cli(golden_dir, ["-a", db, "-p", cutoff, *options])
    got = cli(golden_dir, ["-a", db, "-L", cutoff, *options])
    assert rows.returncode == 0 and got.returncode == 0, got.stderr.decode()[-400:]
    lines, clusters, singletons, edges = table_from_rows(rows.stdout, names)
    out = got.stdout.decode().splitlines()
    assert out[0] == "# CLUSTER dbfile = %s entries = %d pvalue <= %s restarts = 16 clusters = %d singletons = %d edges = %d" % (
        db, len(names), cutoff, clusters, singletons, edges)
    head = 1
    if "-P" in options:
        assert out[head] == "# POLISH tops = 2 all rows"
        head += 1
    if "-F" in options:
        fitted = rows.stdout.count(b"# GUMBEL a = ")
        assert out[head] == "# GUMBEL censor = 0.05 fitted = %d of %d" % (fitted, len(names)) and fitted > 0
        head += 1
    assert out[head:] == lines
    assert edges > 0 and 1 < clusters < len(names)
    # the batches' stderr lines are the ones the -p run prints
    assert got.stderr.count(b"GPU execution time") == rows.stderr.count(b"GPU execution time") == (len(names) + 255) // 256


def test_cli_without_L_prints_what_it_printed(golden_dir, small):
    """-a db -k 3 is not touched by the new option: two runs print the same bytes, and they are the bytes of -Q db with
    every SID on stdin (what the parent commit's -a prints)."""
    one = cli(golden_dir, ["-a", SMALL_DB, "-k", "3"])
    two = cli(golden_dir, ["-a", SMALL_DB, "-k", "3"])
    sids = "".join(n + "\n" for n in small.names).encode()
    ref = subprocess.run([CLI, "-r", "16", "-Q", SMALL_DB, "-k", "3"], input=sids, cwd=golden_dir, capture_output=True, timeout=300)
    assert one.returncode == 0 and ref.returncode == 0
    assert one.stdout.count(b"# QUERY ID") == 586 and one.stdout == two.stdout == ref.stdout
    assert b"CLUSTER" not in one.stdout
