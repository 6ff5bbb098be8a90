"""Single-linkage clustering at several p-values in one pass (-m gpu): sat_cluster_begin_levels / add_levels /
labels_levels, their shards and the command line's -a -H P1,..,PL.  The expected arrays never come from the leveled calls:
per level they are a union-find in Python over the edges of the planted score matrix or of hits_cutoff(P_j)'s rows, and
the arrays of the plain accumulator (sat_cluster_add at P_j) on the same searched state."""
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import report
import edge_cases as ec
from test_cluster_levels_cpu import CLASSES, LEVELS, first_level, nested_by_definition, planted_score
from test_gpu_cluster import BATCHES, N, SMALL_BATCHES, SMALL_DB, expected, row_edges, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
L = len(LEVELS)


def same_levels(got, want, what):
    """got: the three arrays of cluster_labels_levels; want[j]: (labels, degrees, edges) of level j"""
    labels, degrees, edges = got
    assert labels.shape == degrees.shape == (len(want), len(want[0][0])) and edges.shape == (len(want),)
    assert labels.dtype == np.int32 and degrees.dtype == np.int32 and edges.dtype == np.uint64
    for j, w in enumerate(want):
        same((labels[j], degrees[j], int(edges[j])), w, "%s, level %d" % (what, j))
    assert nested_by_definition(labels) == 0, what
    for j in range(len(want) - 1):
        assert np.array_equal(labels[j + 1], labels[j + 1][labels[j]])
    report.cluster_levels_table(labels, degrees)                # sat_cluster_nested agrees


# ---------------------------------------------------------------- 1. planted graphs
@pytest.fixture(scope="module")
def planted_db():
    return sat.synth.make_db(N, 8, 20, sort=False)


@pytest.fixture(scope="module")
def planted_searcher(planted_db):
    with sat.Searcher(0) as s:
        s.upload(planted_db)
        yield s


def planted_graphs():
    """name -> (query rows, entry columns, classes) of the planted cells; every other cell is class 0"""
    rng = np.random.default_rng(2)
    g = {}
    i = np.arange(N - 1)
    g["path"] = (i + 1, i, i % 6)                                              # a class-0 link cuts it at every level
    g["star"] = (i, np.full(N - 1, N - 1), i % 6)
    a, b = np.arange(100, 140), np.arange(1004, 1044)                          # the second clique straddles the block edge
    cells = [(x, y, 5) for c in (a, b) for x in c for y in c if x != y] + [(139, 1004, 3), (1043, 1300, 1)]
    g["two cliques, a bridge and a tail"] = tuple(np.array(c) for c in zip(*cells))
    q, e = rng.integers(0, N, 20000), rng.integers(0, N, 20000)
    g["random"] = (q, e, rng.integers(0, 6, 20000))
    g["one query row"] = (np.full(N, 700), np.arange(N), np.arange(N) % 6)
    # query 3's first block all class 2; query 5's second, ragged block classes 1..5 in turn
    g["uniform block and mixed block"] = (np.concatenate([np.full(1024, 3), np.full(N - 1024, 5)]), np.arange(N),
                                          np.concatenate([np.full(1024, 2), 1 + np.arange(N - 1024) % 5]))
    q, e = rng.integers(0, N, 3000), rng.integers(0, N, 3000)
    g["levels without edges of their own"] = (q, e, rng.choice([5, 3, 1], 3000))
    g["lane 63"] = (np.array([10]), np.array([63]), np.array([1]))
    g["last row"] = (np.array([10]), np.array([N - 1]), np.array([1]))
    g["rows 1023 and 1024"] = (np.array([10, 10]), np.array([1023, 1024]), np.array([1, 1]))
    g["diagonal"] = (np.arange(N), np.arange(N), np.full(N, 5))
    out = {}
    for name, (q, e, k) in g.items():
        # as the score matrix holds them: a cell drawn twice is one row, of the class written last
        cls = np.zeros((N, N), np.int8)
        cls[q, e] = k
        out[name] = cls
    return out


def scores_of(db, cls):
    n = db.orders.astype(np.int64)
    return ((cls.astype(np.int64) * (n[:, None] + n[None, :]) + 1) // 2).astype(np.int32)


def expected_levels(cls):
    """want[j] = expected() over the cells whose class first qualifies at a level <= j"""
    want = []
    for j in range(L):
        q, e = np.nonzero((cls > 0) & (L - cls <= j))
        want.append(expected(N, q, e))
    return want


def batches_of(s, scores, batches, add):
    """every batch searched (one restart, only to reach the searched state), its scores overwritten, then add(lo, hi):
    nothing may come back from it"""
    for lo, hi in batches:
        s.set_queries_from_db(np.arange(lo, hi), lo)
        s.search(True, False, 1)
        s.debug_set_scores(scores[lo:hi])
        before = s.d2h_bytes()
        add(lo, hi)
        assert s.d2h_bytes() == before


def plant_levels(s, scores, repeat=1, batches=BATCHES, levels=LEVELS):
    s.cluster_begin_levels(levels)
    batches_of(s, scores, batches, lambda lo, hi: [s.cluster_add_levels(np.arange(lo, hi)) for _ in range(repeat)])
    before = s.d2h_bytes()
    got = s.cluster_labels_levels()
    assert s.d2h_bytes() - before == len(levels) * (8 * N + 8)
    return got


def plant_plain(s, scores, p):
    s.cluster_begin()
    batches_of(s, scores, BATCHES, lambda lo, hi: s.cluster_add(p, np.arange(lo, hi)))
    return s.cluster_labels()


def test_classes_and_first_levels():
    assert [first_level(k) for k in CLASSES] == [0, 1, 2, 3, 4, 5] and L == 5
    assert planted_score(0, 8, 20) == 0


@pytest.mark.parametrize("name", list(planted_graphs()))
def test_planted_graph(planted_searcher, planted_db, name):
    s, cls = planted_searcher, planted_graphs()[name]
    scores = scores_of(planted_db, cls)
    want = expected_levels(cls)
    if name == "diagonal":
        assert all(w[2] == 0 and np.array_equal(w[0], np.arange(N)) for w in want)
    if name in ("lane 63", "last row"):
        assert [w[2] for w in want] == [0, 0, 0, 0, 1]
    if name == "rows 1023 and 1024":
        assert [w[2] for w in want] == [0, 0, 0, 0, 2] and (want[4][0] != np.arange(N)).sum() == 2
    if name == "two cliques, a bridge and a tail":
        assert [len(set(w[0].tolist())) for w in want] == [N - 78, N - 78, N - 79, N - 79, N - 80]
    if name == "levels without edges of their own":
        for j in (1, 3):
            assert want[j][2] == want[j - 1][2] and np.array_equal(want[j][0], want[j - 1][0])
        assert want[0][2] < want[2][2] < want[4][2]
    if name in ("path", "star", "one query row", "random"):
        assert len({w[2] for w in want}) == L                   # every level has edges of its own
    got = plant_levels(s, scores)
    same_levels(got, want, name)
    if name == "levels without edges of their own":
        for j in (1, 3):
            assert all(np.array_equal(got[i][j], got[i][j - 1]) for i in range(3))
    # per level, the plain accumulator at that level's cutoff on the same scores
    for j, p in enumerate(LEVELS):
        same(plant_plain(s, scores, p), want[j], "%s, plain at %g" % (name, p))


def test_added_twice_and_in_reverse_order(planted_searcher, planted_db):
    s, cls = planted_searcher, planted_graphs()["random"]
    scores = scores_of(planted_db, cls)
    want = expected_levels(cls)
    got = plant_levels(s, scores, repeat=2)
    same_levels(got, [(w[0], 2 * w[1], 2 * w[2]) for w in want], "random, twice")
    same_levels(plant_levels(s, scores, batches=BATCHES[::-1]), want, "random, batches reversed")
    # labels may be read between adds: the accumulator goes on
    lo, hi = BATCHES[0]
    s.cluster_add_levels(np.arange(lo, hi))
    part = np.zeros_like(cls)
    part[lo:hi] = cls[lo:hi]
    third = expected_levels(part)
    same_levels(s.cluster_labels_levels(), [(w[0], w[1] + t[1], w[2] + t[2]) for w, t in zip(want, third)], "random, one batch again")


def test_one_level_and_eight_levels_planted(planted_searcher, planted_db):
    """L = 1 and L = 8 on the random graph: cutoffs between and at the edges of the classes, 0 and 1 included"""
    s, cls = planted_searcher, planted_graphs()["random"]
    scores = scores_of(planted_db, cls)
    want5 = expected_levels(cls)
    same_levels(plant_levels(s, scores, levels=[1e-3]), [want5[2]], "L = 1")
    assert report.stats(0, 8, 8)[2] < 0.99
    every = (np.zeros(N, np.int32), np.full(N, 2 * (N - 1), np.int32), N * (N - 1))    # every row but the self rows
    nothing = expected(N, [], [])
    levels = [0.0, 1e-5, 1e-4, 1e-3, 0.05, 0.5, 0.99, 1.0]     # class 0 is about 0.94: an edge at the last two
    want = [nothing] + want5 + [every, every]
    same_levels(plant_levels(s, scores, levels=levels), want, "L = 8")


# ---------------------------------------------------------------- 2. real scores
@pytest.fixture(scope="module")
def small(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, SMALL_DB))
    assert len(db) == 586
    return db


@pytest.fixture(scope="module")
def small_runs(small):
    """The example database all-vs-all as 256 / 256 / 74 at r = 16, on one context.  Eight cutoffs taken from the
    distinct p-values its rows show - 0, 1, one that is exactly a row's p-value and the double just below it among
    them; per cutoff the arrays expected from hits_cutoff(P_j)'s rows and those of the plain accumulator; and what the
    leveled accumulator returned for the eight."""
    n = len(small)
    with sat.Searcher(0) as s:
        s.upload(small)

        def batches(step):
            for lo, hi in SMALL_BATCHES:
                s.set_queries_from_db(np.arange(lo, hi), lo)
                s.search(True, False, 16)
                step(lo, hi)

        pv = []
        batches(lambda lo, hi: pv.extend(r["pvalue"] for r in s.hits_cutoff(1.0)))
        distinct = np.unique(np.concatenate(pv))
        inner = distinct[(distinct > 0.0) & (distinct < 1.0)]
        assert len(inner) >= 2
        exact = inner[len(inner) // 3]
        cuts = [0.0, 1.0, exact, np.nextafter(exact, -np.inf)]
        # four more of the rows' own p-values, spread over them (fixed values in between, should they be too few)
        for p in inner[np.linspace(0, len(inner) - 1, 5).astype(int)].tolist() + [0.3, 0.6, 0.9, 0.01]:
            if len(cuts) < 8 and p not in cuts:
                cuts.append(p)
        cuts = np.array(sorted(cuts))
        assert len(cuts) == 8 and cuts[0] == 0.0 and cuts[-1] == 1.0 and exact in cuts and np.nextafter(exact, -np.inf) in cuts
        rows = [([], []) for _ in cuts]

        def leveled_step(lo, hi):
            for j, p in enumerate(cuts):
                a, b = row_edges(s.hits_cutoff(float(p)), np.arange(lo, hi))
                rows[j][0].append(a)
                rows[j][1].append(b)
            before = s.d2h_bytes()
            s.cluster_add_levels(np.arange(lo, hi))
            assert s.d2h_bytes() == before

        s.cluster_begin_levels(cuts)
        batches(leveled_step)
        before = s.d2h_bytes()
        leveled = s.cluster_labels_levels()
        assert s.d2h_bytes() - before == 8 * (8 * n + 8)
        want = [expected(n, np.concatenate(a), np.concatenate(b)) for a, b in rows]
        plain = []
        for p in cuts:
            s.cluster_begin()
            batches(lambda lo, hi: s.cluster_add(float(p), np.arange(lo, hi)))
            plain.append(s.cluster_labels())
        # L = 1 at a handful of the cutoffs
        single = {}
        for j in (0, 2, 5, 6, 7):
            s.cluster_begin_levels([cuts[j]])
            batches(lambda lo, hi: s.cluster_add_levels(np.arange(lo, hi)))
            single[j] = s.cluster_labels_levels()
    return cuts, leveled, want, plain, single


def test_real_scores_eight_levels(small_runs):
    cuts, leveled, want, plain, _ = small_runs
    same_levels(leveled, want, "example database")
    for j in range(8):
        same(plain[j], want[j], "plain at %r" % cuts[j])
    assert len({w[2] for w in want}) >= 6                       # the levels do differ
    # (P = 0 is not empty: a few rows' p-values underflow to 0.)  P = 1 takes every row: one component
    assert want[0][2] < want[6][2] < want[7][2] == 586 * 585 and not want[7][0].any()


def test_real_scores_one_level_is_the_plain_accumulator(small_runs):
    cuts, _, _, plain, single = small_runs
    assert len(single) == 5
    for j, got in single.items():
        assert got[0].shape == (1, 586)
        labels, degrees, edges = plain[j]
        assert got[0][0].tobytes() == labels.tobytes() and got[1][0].tobytes() == degrees.tobytes() and int(got[2][0]) == edges


@pytest.fixture(scope="module")
def edge(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, ec.EDGE_DB))
    assert len(db) == 28 and tuple(db.orders) == ec.EDGE_ORDERS
    return db


@pytest.mark.parametrize("mode", ["fitted", "polished", "polished and fitted"])
def test_levels_follow_hits_cutoff(edge, mode):
    n = len(edge)
    nodes = np.arange(n)
    with sat.Searcher(0) as s:
        s.upload(edge)
        s.set_queries_from_db(nodes, 0)
        if "polished" in mode:
            s.set_polish_all(2)
        s.search(True, False, 16)
        if "fitted" in mode:
            assert s.fit_statistics(0.05)["fitted"].any()
        # three of the rows' own p-values: those the rows between DIFFERENT structures show bring edges of their own;
        # under the built-in table these rows show fewer than three values, and a self row's p-value joins them
        rows = s.hits_cutoff(1.0)
        pv = np.unique(np.concatenate([r["pvalue"][r["entry"] != q] for q, r in enumerate(rows)]))
        cuts = set(pv[[len(pv) // 6, len(pv) // 2, (5 * len(pv)) // 6]].tolist())
        for p in np.unique(np.concatenate([r["pvalue"] for r in rows]))[::-1].tolist():
            if len(cuts) < 3:
                cuts.add(p)
        cuts = np.array(sorted(cuts))
        assert len(cuts) == 3
        want = [expected(n, *row_edges(s.hits_cutoff(float(p)), nodes)) for p in cuts]
        assert want[0][2] <= want[1][2] < want[2][2]
        s.cluster_begin_levels(cuts)
        s.cluster_add_levels(nodes)
        same_levels(s.cluster_labels_levels(), want, mode)
        for p, w in zip(cuts, want):
            s.cluster_begin()
            s.cluster_add(float(p), nodes)
            same(s.cluster_labels(), w, "%s, plain at %r" % (mode, p))


# ---------------------------------------------------------------- 3. state and errors
def test_state_and_errors(edge):
    n = len(edge)
    nodes = np.arange(n, dtype=np.int32)
    cuts = np.array([0.2, 0.95], np.float64)     # the rows between different structures show 0.16.. and 0.94.. only
    with sat.Searcher(0) as s:
        lib, ctx = s._lib, s._ctx
        with pytest.raises(sat.SatError, match=r"\[-5\].*no database"):
            s.cluster_begin_levels(cuts, n)
        s.upload(edge)
        s.set_queries_from_db(nodes, 0)
        s.search(True, False, 16)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_cluster_begin"):          # before begin
            s.cluster_add_levels(nodes)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_cluster_begin"):
            s.cluster_labels_levels()
        with pytest.raises(sat.SatError, match=r"\[-1\].*n_nodes"):
            s.cluster_begin_levels(cuts, 0)
        s.cluster_begin_levels(cuts)
        s.set_queries_from_db(nodes, 0)
        with pytest.raises(sat.SatError, match=r"\[-5\].*no search has run"):          # before a search
            s.cluster_add_levels(nodes)
        s.search(True, False, 16)
        want = [expected(n, *row_edges(s.hits_cutoff(float(p)), nodes)) for p in cuts]
        assert 0 < want[0][2] < want[1][2]
        s.cluster_add_levels(nodes)
        same_levels(s.cluster_labels_levels(), want, "first add")
        # every rejected call leaves the accumulator as it was
        assert lib.sat_cluster_add_levels(ctx, None) == -1
        assert b"query_node is null" in lib.sat_last_error()
        bad = nodes.copy()
        bad[3] = -1
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 3: node -1 "):
            s.cluster_add_levels(bad)
        bad[3], bad[27] = 3, n
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 27: node 28 "):
            s.cluster_add_levels(bad)
        assert lib.sat_cluster_begin_levels(ctx, n, 2, None) == -1
        assert b"null" in lib.sat_last_error()
        for levels, message in (([], r"n_levels must be 1\.\.8 \(got 0\)"), ([0.1] * 9, r"n_levels must be 1\.\.8 \(got 9\)"),
                                ([0.1, 0.05], r"level 1: .*above level 0"), ([0.1, 0.1], r"level 1: .*above level 0"),
                                ([0.1, 0.2, 0.2], r"level 2: .*above level 1"), ([0.1, 1.5], r"level 1: .*\[0, 1\]"),
                                ([-0.1, 0.5], r"level 0: .*\[0, 1\]"), ([0.1, float("nan")], r"level 1: .*\[0, 1\]"),
                                ([float("inf")], r"level 0: .*\[0, 1\]")):
            with pytest.raises(sat.SatError, match=r"\[-1\].*" + message):
                s.cluster_begin_levels(levels)
        with pytest.raises(sat.SatError, match=r"\[-1\].*n_nodes"):
            s.cluster_begin_levels(cuts, -3)
        assert lib.sat_cluster_labels_levels(ctx, None, None, None) == -1
        # the calls of the other kind: SAT_ESTATE, and the message says which kind is active
        with pytest.raises(sat.SatError, match=r"\[-5\].*leveled.*sat_cluster_begin_levels"):
            s.cluster_add(0.5, nodes)
        with pytest.raises(sat.SatError, match=r"\[-5\].*leveled.*sat_cluster_begin_levels"):
            s.cluster_labels()
        same_levels(s.cluster_labels_levels(), want, "after the rejected calls")
        # degree and edges may be NULL: fewer bytes
        labels = np.zeros((2, n), np.int32)
        before = s.d2h_bytes()
        assert lib.sat_cluster_labels_levels(ctx, labels.ctypes.data, None, None) == 0
        assert s.d2h_bytes() - before == 2 * 4 * n and np.array_equal(labels[0], want[0][0]) and np.array_equal(labels[1], want[1][0])
        degrees = np.zeros((2, n), np.int32)
        before = s.d2h_bytes()
        assert lib.sat_cluster_labels_levels(ctx, labels.ctypes.data, degrees.ctypes.data, None) == 0
        assert s.d2h_bytes() - before == 2 * 8 * n and np.array_equal(degrees[1], want[1][1])
        # a plain accumulator replaces the leveled one, and refuses its calls; a rejected plain begin leaves it alone
        s.cluster_begin()
        assert lib.sat_cluster_add_levels(ctx, nodes.ctypes.data) == -5
        with pytest.raises(sat.SatError, match=r"\[-5\].*plain.*sat_cluster_begin\)"):
            s.cluster_add_levels(nodes)
        levels2 = np.zeros((2, n), np.int32)
        assert lib.sat_cluster_labels_levels(ctx, levels2.ctypes.data, None, None) == -5
        assert b"plain" in lib.sat_last_error()
        with pytest.raises(sat.SatError, match=r"\[-1\].*level 1"):
            s.cluster_begin_levels([0.5, 0.1])                                        # the plain one stays
        s.cluster_add(float(cuts[1]), nodes)
        same(s.cluster_labels(), want[1], "plain after leveled")
        # begin again resets; more nodes than entries: the rest stay singletons
        s.cluster_begin_levels(cuts, n + 5)
        labels, degrees, edges = s.cluster_labels_levels()
        assert all(np.array_equal(l, np.arange(n + 5)) for l in labels) and not degrees.any() and not edges.any()
        s.cluster_add_levels(nodes + 5)
        want5 = [expected(n + 5, row_edges(s.hits_cutoff(float(p)), nodes)[0] + 5, row_edges(s.hits_cutoff(float(p)), nodes)[1]) for p in cuts]
        same_levels(s.cluster_labels_levels(), want5, "shifted query nodes")
        s.cluster_begin_levels(cuts)
        s.cluster_add_levels(nodes)
        same_levels(s.cluster_labels_levels(), want, "begin twice")
        # searches and query changes keep the accumulator, an upload drops it
        s.set_queries_from_db(nodes[:5], 0)
        s.search(True, False, 16)
        same_levels(s.cluster_labels_levels(), want, "after a query change and a search")
        s.upload(edge)
        assert lib.sat_cluster_labels_levels(ctx, levels2.ctypes.data, None, None) == -5
        assert b"sat_cluster_begin" in lib.sat_last_error() and b"plain" not in lib.sat_last_error()
        s.search(True, False, 16)
        with pytest.raises(sat.SatError, match=r"\[-5\].*no cluster accumulator"):
            s.cluster_add_levels(nodes[:5])
        # sat_cluster_end drops it too
        s.cluster_begin_levels(cuts)
        s.cluster_end()
        with pytest.raises(sat.SatError, match=r"\[-5\].*no cluster accumulator"):
            s.cluster_labels_levels()
        with pytest.raises(sat.SatError, match=r"\[-5\].*no cluster accumulator"):
            s.cluster_labels()


# ---------------------------------------------------------------- 4. shards
@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]], ids=["1", "2", "3"])
def test_shards_equal_one_context(small, small_runs, devices):
    cuts, leveled, want, _, _ = small_runs
    n = len(small)
    with sat.MultiSearcher(len(devices), devices=devices) as m:
        m.upload(small)
        m.set_queries_from_db(np.arange(4), 0)
        m.search_only(True, False, 1)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_cluster_begin"):
            m.cluster_add_levels(np.arange(4))
        with pytest.raises(sat.SatError, match=r"\[-1\].*level 1"):
            m.cluster_begin_levels([0.5, 0.5])
        m.cluster_begin_levels(cuts)
        for lo, hi in SMALL_BATCHES:
            m.set_queries_from_db(np.arange(lo, hi), lo)
            m.search_only(True, False, 16)
            before = m.d2h_bytes()
            m.cluster_add_levels(np.arange(lo, hi))
            assert m.d2h_bytes() == before
        before = m.d2h_bytes()
        got = m.cluster_labels_levels()
        assert m.d2h_bytes() - before == len(devices) * 8 * (8 * n + 8)
        same_levels(got, want, "%d shards" % len(devices))
        assert all(np.array_equal(g, l) for g, l in zip(got, leveled))
        with pytest.raises(sat.SatError, match=r"\[-5\].*leveled"):
            m.cluster_add(0.5, np.arange(SMALL_BATCHES[-1][0], SMALL_BATCHES[-1][1]))
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 1: node 586 "):
            m.cluster_add_levels([0, n] + [0] * (SMALL_BATCHES[-1][1] - SMALL_BATCHES[-1][0] - 2))


# ---------------------------------------------------------------- 5. command line
CLI_LEVELS = ("1e-4", "1e-3", "0.05")


def cli(golden_dir, args):
    return subprocess.run([CLI, "-r", "16", *args], input=b"not read\n", cwd=golden_dir, capture_output=True, timeout=300)


@pytest.mark.parametrize("options", [[], ["-G", "0,0"], ["-F", "0.05"], ["-P", "2", "-A"]], ids=["plain", "G00", "F0.05", "P2A"])
def test_cli_levels_are_the_L_runs_side_by_side(golden_dir, options):
    n = 586
    got = cli(golden_dir, ["-a", SMALL_DB, "-H", ",".join(CLI_LEVELS), *options])
    assert got.returncode == 0, got.stderr.decode()[-400:]
    out = got.stdout.decode().splitlines()
    assert out[0] == "# CLUSTER dbfile = %s entries = %d levels = 3 restarts = 16" % (SMALL_DB, n)
    extra = ("-P" in options) + ("-F" in options)
    table = [line.split() for line in out[1 + 3 + extra:]]
    assert len(table) == n and all(len(t) == 1 + 3 * 3 for t in table)
    counts = []
    for j, p in enumerate(CLI_LEVELS):
        one = cli(golden_dir, ["-a", SMALL_DB, "-L", p, *options])
        assert one.returncode == 0, one.stderr.decode()[-400:]
        ref = one.stdout.decode().splitlines()
        head = "# CLUSTER dbfile = %s entries = %d pvalue <= %s restarts = 16 " % (SMALL_DB, n, ref[0].split()[10])
        assert ref[0].startswith(head) and "LEVEL" not in one.stdout.decode()
        assert out[1 + j] == "# LEVEL %d pvalue <= %s %s" % (j + 1, ref[0].split()[10], ref[0][len(head):])
        assert out[4:4 + extra] == ref[1:1 + extra]                                    # the # POLISH / # GUMBEL lines
        assert [t[:1] + t[1 + 3 * j:4 + 3 * j] for t in table] == [line.split() for line in ref[1 + extra:]]
        # and the bytes: a level's three columns are formatted as -L formats them
        if j == 0:
            assert [line[:len(r)] for line, r in zip(out[4 + extra:], ref[1 + extra:])] == ref[1 + extra:]
        counts.append(int(ref[0].split()[-1]))
    assert 0 < counts[0] < counts[1] < counts[2]
    assert got.stderr.count(b"GPU execution time") == (n + 255) // 256


def test_cli_without_H_prints_what_it_printed(golden_dir, small):
    """-a db -k 3 is not touched by the new option: the bytes of -Q db with every SID on stdin, no clustering line"""
    one = cli(golden_dir, ["-a", SMALL_DB, "-k", "3"])
    sids = "".join(name + "\n" for name in small.names).encode()
    ref = subprocess.run([CLI, "-r", "16", "-Q", SMALL_DB, "-k", "3"], input=sids, cwd=golden_dir, capture_output=True, timeout=300)
    assert one.returncode == 0 and ref.returncode == 0
    assert one.stdout.count(b"# QUERY ID") == 586 and one.stdout == ref.stdout
    assert b"CLUSTER" not in one.stdout and b"LEVEL " not in one.stdout
