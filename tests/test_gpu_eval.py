"""A search scored against a classification on the GPU (-m gpu): sat_eval_classes / rows / tables, their shards and the
command line's -E.  The expected rows never come from the code under test: they are pair counts in numpy (eval_lib) over
the score matrix itself - planted with debug_set_scores, copied with results(), or parsed from the rows `-k` prints."""
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import _native, report
import edge_cases as ec
import eval_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
SMALL_DB = "tableauxdistmatrixdb.small.ascii"
N = 1500                                       # the database of test_gpu_cluster.py: one block of rows, ragged
BATCHES = ((0, 700), (700, 701), (701, 1500))  # 700, 1 and 799 queries
B = _native.EVAL_BLOCK_ROWS                    # rows of one query a block of eval_histogram counts


def seven_way(n, seed, unclassified=0.0):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 7, n).astype(np.int32)
    cls[rng.random(n) < unclassified] = -1
    return cls


def eval_batch(s, nodes, rocn, scores=None, searched=False):
    """eval_rows of the batch `nodes` (entries of the resident database, taken as queries) with everything the call
    promises checked around it: exactly 32 bytes a query come back, a second call gives the same rows, the result
    buffers are byte for byte what they were.  scores: planted over a one-restart search."""
    if not searched:
        s.set_queries_from_db(nodes, int(nodes[0]))
        s.search(True, False, 1)
    if scores is not None:
        s.debug_set_scores(scores)
    held = s.results()[0].copy()
    before = s.d2h_bytes()
    rows = s.eval_rows(nodes, rocn)
    assert s.d2h_bytes() - before == 32 * len(nodes)
    again = s.eval_rows(nodes, rocn)
    assert rows.tobytes() == again.tobytes()
    assert s.results()[0].tobytes() == held.tobytes()
    return rows, held.reshape(len(nodes), -1)


# ---------------------------------------------------------------- 1. planted matrices
@pytest.fixture(scope="module")
def planted_db():
    return sat.synth.make_db(N, 8, 20, sort=False)


@pytest.fixture(scope="module")
def planted_searcher(planted_db):
    with sat.Searcher(0) as s:
        s.upload(planted_db)
        yield s


def planted_cases(orders):
    """name -> (scores [N, N], node_class [N], rocn)"""
    rng = np.random.default_rng(2)
    m = (orders.astype(np.int64) * (orders - 1))[:, None]                  # each query's largest score
    random = rng.integers(-50, 400, (N, N))                                # orders 8..20: m = 56..380, so some are clamped
    ends = np.stack([-m, m, -m - 5, m + 1000, m - 1, 1 - m, np.full_like(m, 2**30), np.full_like(m, -2**30), 0 * m], 0)[
        rng.integers(0, 9, (N, N)), np.arange(N)[:, None], 0]
    top_on_the_diagonal = random.copy()
    top_on_the_diagonal[np.arange(N), np.arange(N)] = 2**30
    return {
        "all scores equal": (np.full((N, N), 7), seven_way(N, 3), 50),
        "both ends of the range and beyond": (ends, seven_way(N, 4), 5),
        "random scores": (random, seven_way(N, 5), 50),
        "random scores, one negative counted": (random, seven_way(N, 5), 1),
        "random scores, more negatives asked for than there are": (random, seven_way(N, 5), 2000),
        "a class that is the query alone": (random, np.arange(N, dtype=np.int32), 50),
        "one class for everybody": (random, np.zeros(N, np.int32), 50),
        "unclassified entries and queries": (random, seven_way(N, 6, unclassified=0.3), 50),
        "the self row carries the top score": (top_on_the_diagonal, seven_way(N, 7), 50),
    }


CASE_NAMES = list(planted_cases(np.full(N, 8)))


@pytest.fixture(scope="module")
def cases(planted_db):
    return planted_cases(planted_db.orders)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_planted_matrix(planted_searcher, planted_db, cases, name):
    s = planted_searcher
    scores, node_class, rocn = cases[name]
    scores = scores.astype(np.int32)
    s.set_eval_classes(node_class)
    got = []
    for lo, hi in BATCHES:
        rows, held = eval_batch(s, np.arange(lo, hi), rocn, scores[lo:hi])
        assert np.array_equal(held, scores[lo:hi])
        got.append(rows)
    got = np.concatenate(got)
    want = eval_lib.expected_rows(scores, planted_db.orders, np.arange(N), node_class, rocn)
    eval_lib.same_rows(got, want, name)
    if name == "a class that is the query alone":
        assert not got["positives"].any() and (got["negatives"] == N - 1).all()
    if name == "one class for everybody":
        assert not got["negatives"].any() and (got["positives"] == N - 1).all() and not got["u2"].any()
    if name == "unclassified entries and queries":
        out = node_class < 0
        assert out.sum() > 300 and (got["query_class"][out] == -1).all() and not got["positives"][out].any() and not got["negatives"][out].any()
        assert (got["positives"] + got["negatives"])[~out].max() == (~out).sum() - 1
    if name == "all scores equal":
        assert (got["u2"] == got["positives"].astype(np.uint64) * got["negatives"].astype(np.uint64)).all()        # AUC 1/2
    if name == "the self row carries the top score":
        assert (got["positives"] + got["negatives"] == N - 1).all()


# ---------------------------------------------------------------- 2. row-block edges
@pytest.mark.parametrize("n", [1, 2, B - 1, B, B + 1, 2 * B + 1])
def test_row_block_edges(n):
    db = sat.synth.make_db(n, 3, 5, sort=False)
    rng = np.random.default_rng(n)
    nodes = np.unique([0, n // 2, n - 1]).astype(np.int32)
    node_class = rng.integers(0, 3, n).astype(np.int32)
    node_class[rng.random(n) < 0.1] = -1
    node_class[nodes] = 1
    scores = rng.integers(-25, 25, (len(nodes), n)).astype(np.int32)
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_eval_classes(node_class)
        rows, _ = eval_batch(s, nodes, 50, scores)
        eval_lib.same_rows(rows, eval_lib.expected_rows(scores, db.orders[nodes], nodes, node_class, 50), "%d entries" % n)
        assert (rows["positives"] + rows["negatives"] == (node_class >= 0).sum() - 1).all()
        tables = s.eval_tables(nodes)
        for q, t in enumerate(tables):
            assert t.shape == (2, 2 * db.orders[nodes[q]] * (db.orders[nodes[q]] - 1) + 1)
            assert t[0].sum() == rows["positives"][q] and t[1].sum() == rows["negatives"][q]


# ---------------------------------------------------------------- 3. table-size classes: real scores
def real_rows(s, db, node_class, batches, rocn, maxstart=16):
    """(rows of every batch, the expected rows from results()) of an all-vs-all search of `db`"""
    got, want = [], []
    for lo, hi in batches:
        nodes = np.arange(lo, hi)
        s.set_queries_from_db(nodes, lo)
        s.search(True, False, maxstart)
        rows, held = eval_batch(s, nodes, rocn, searched=True)
        got.append(rows)
        want.append(eval_lib.expected_rows(held, db.orders[nodes], nodes, node_class, rocn))
        for q, t in zip(nodes[:3], s.eval_tables(nodes)[:3]):               # the raw tables: counts by clamped score
            c, m = int(node_class[q]), int(db.orders[q]) * (int(db.orders[q]) - 1)
            counted = (node_class >= 0) & (np.arange(len(db)) != q)
            for side, keep in enumerate((counted & (node_class == c), counted & (node_class != c))):
                want_t = np.bincount(eval_lib.clamp(held[q - lo][keep], db.orders[q]) + m, minlength=2 * m + 1) if c >= 0 else 0
                assert np.array_equal(t[side], want_t + np.zeros(2 * m + 1, np.int64))
    return np.concatenate(got), np.concatenate(want)


@pytest.fixture(scope="module")
def edge(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, ec.EDGE_DB))
    assert db.orders.min() == 1 and db.orders.max() == 111
    return db


@pytest.fixture(scope="module")
def small(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, SMALL_DB))
    assert len(db) == 586
    return db


SMALL_BATCHES = ((0, 256), (256, 512), (512, 586))


@pytest.mark.parametrize("polish", [0, 2], ids=["plain", "polished"])
def test_edge_database(edge, polish):
    """orders 1..111: a 1-SSE query has one bin, a 111-SSE query 24 421 a side - far outside the LDS window"""
    n = len(edge)
    node_class = (np.arange(n) % 3).astype(np.int32)
    node_class[::5] = -1
    with sat.Searcher(0) as s:
        s.upload(edge)
        s.set_polish_all(polish)
        s.set_eval_classes(node_class)
        got, want = real_rows(s, edge, node_class, ((0, n),), 4)
        eval_lib.same_rows(got, want, "edge database")
        assert (got["query_class"] == node_class).all() and got["u2"].any() and got["t2"].any()
        one = int(np.nonzero(edge.orders == 1)[0][0])
        assert s.eval_tables(np.arange(n))[one].shape == (2, 1)
        # every query's whole range and a little beyond it, planted: most rows of the large queries miss the LDS window
        m = (edge.orders.astype(np.int64) * (edge.orders - 1))[:, None]
        planted = np.random.default_rng(9).integers(-m - 3, m + 4, (n, n)).astype(np.int32)
        assert (planted > _native.EVAL_WINDOW_BINS).sum() > n and (planted < -300).sum() > n
        rows, _ = eval_batch(s, np.arange(n), 4, planted, searched=True)
        eval_lib.same_rows(rows, eval_lib.expected_rows(planted, edge.orders, np.arange(n), node_class, 4), "edge database, planted")


@pytest.fixture(scope="module")
def small_classes():
    return seven_way(586, 11, unclassified=0.1)


@pytest.fixture(scope="module")
def small_single(small, small_classes):
    """polish -> the single context's rows of the 586-entry example at r = 16, checked against results() once"""
    out = {}
    with sat.Searcher(0) as s:
        s.upload(small)
        s.set_eval_classes(small_classes)
        for polish in (0, 2):
            s.set_polish_all(polish)
            got, want = real_rows(s, small, small_classes, SMALL_BATCHES, 50)
            eval_lib.same_rows(got, want, "586 entries, polish %d" % polish)
            out[polish] = got
    return out


def test_small_database(small_single, small_classes):
    """(the comparison with results() is the fixture's) every classified query has both kinds of rows under a 7-way
    split of 586, and the ratios are proportions"""
    for polish, rows in small_single.items():
        defined = (rows["positives"] > 0) & (rows["negatives"] > 0)
        assert np.array_equal(defined, small_classes >= 0) and np.array_equal(rows["query_class"], small_classes)
        ratios = np.array([report.eval_ratios(r) for r in rows[defined]])
        assert (ratios >= 0.0).all() and (ratios <= 1.0).all()


# ---------------------------------------------------------------- 4. shards
@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]], ids=["1", "2", "3"])
def test_shards_equal_one_context(small, small_classes, small_single, devices):
    with sat.MultiSearcher(len(devices), devices=devices) as m:
        m.upload(small)
        m.set_queries_from_db(np.arange(4), 0)
        m.search_only(True, False, 1)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_eval_classes"):
            m.eval_rows(np.arange(4))
        m.set_eval_classes(small_classes)
        for polish in (0, 2):
            m.set_polish_all(polish)
            got = []
            for lo, hi in SMALL_BATCHES:
                m.set_queries_from_db(np.arange(lo, hi), lo)
                m.search_only(True, False, 16)
                before = m.d2h_bytes()
                got.append(m.eval_rows(np.arange(lo, hi), 50))
                if len(devices) == 1:
                    assert m.d2h_bytes() - before == 32 * (hi - lo)        # one shard: no table crosses
                assert got[-1].tobytes() == m.eval_rows(np.arange(lo, hi), 50).tobytes()
            assert np.concatenate(got).tobytes() == small_single[polish].tobytes(), "%d shards, polish %d" % (len(devices), polish)
        nq = SMALL_BATCHES[-1][1] - SMALL_BATCHES[-1][0]
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 1: node 586 "):
            m.eval_rows([0, 586] + [0] * (nq - 2))
        with pytest.raises(sat.SatError, match=r"\[-1\].*rocn"):
            m.eval_rows(np.arange(nq), 0)
        m.set_eval_classes(None)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_eval_classes"):
            m.eval_rows(np.arange(nq))


# ---------------------------------------------------------------- 5. state
def test_state_and_arguments(edge):
    n = len(edge)
    nodes = np.arange(n, dtype=np.int32)
    node_class = (nodes % 2).astype(np.int32)
    with sat.Searcher(0) as s:
        with pytest.raises(sat.SatError, match=r"\[-5\].*no database"):
            s.set_eval_classes(node_class)
        s.set_eval_classes(None)                                            # removing nothing is fine
        s.upload(edge)
        s.set_eval_classes(node_class)
        s.set_queries_from_db(nodes, 0)
        with pytest.raises(sat.SatError, match=r"\[-5\].*no search has run"):
            s.eval_rows(nodes)
        s.search(True, False, 16)
        want = s.eval_rows(nodes, 3)
        eval_lib.same_rows(want, eval_lib.expected_rows(s.results()[0], edge.orders, nodes, node_class, 3), "edge, two classes")
        # SAT_EINVAL: nothing changes, the installed classes included
        lib, ctx = s._lib, s._ctx
        rows = np.zeros(n, eval_lib.EVAL_DTYPE)
        for bad, text in (((nodes.ctypes.data, 0, rows.ctypes.data), "rocn must be >= 1"), ((None, 3, rows.ctypes.data), "null"),
                          ((nodes.ctypes.data, 3, None), "null")):
            assert lib.sat_eval_rows(ctx, *bad) == -1 and text in lib.sat_last_error().decode()
        shifted = nodes.copy()
        shifted[5] = n
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 5: node %d outside 0\.\.%d" % (n, n - 1)):
            s.eval_rows(shifted, 3)
        shifted[5] = -1
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 5: node -1 "):
            s.eval_rows(shifted, 3)
        with pytest.raises(sat.SatError, match=r"\[-1\].*n_nodes must be >= 1"):
            s.set_eval_classes(np.zeros(0, np.int32))
        with pytest.raises(sat.SatError, match=r"\[-1\].*ordinal %d" % (n - 1)):
            s.set_eval_classes(node_class[:n - 1])
        assert not rows.view(np.uint8).any()
        assert s.eval_rows(nodes, 3).tobytes() == want.tobytes()
        # more nodes than entries: the queries may be any of them
        wide = np.concatenate([node_class, [1, 0, -1]]).astype(np.int32)
        s.set_eval_classes(wide)
        moved = s.eval_rows(np.full(n, n + 1, np.int32), 3)                 # every query is node n + 1, of class 0: no self row
        ordinals = np.arange(n)
        for q in (0, n - 1):
            sc = eval_lib.clamp(s.results()[0].reshape(n, n)[q], edge.orders[q])
            assert tuple(moved[q])[:5] == eval_lib.pair_counts(sc[node_class[ordinals] == 0], sc[node_class[ordinals] == 1], 3)
        s.set_eval_classes(node_class)
        # an installed fit survives, and does not matter: the ranking is by raw score
        s.fit_statistics(0.05)
        cut = s.hits_cutoff(0.5)
        assert s.eval_rows(nodes, 3).tobytes() == want.tobytes()
        again = s.hits_cutoff(0.5)
        assert len(cut) == len(again) and all(a.tobytes() == b.tobytes() for a, b in zip(cut, again))
        # a cluster accumulator survives
        s.cluster_begin()
        s.cluster_add(0.5, nodes)
        held = s.cluster_labels()
        assert s.eval_rows(nodes, 3).tobytes() == want.tobytes()
        now = s.cluster_labels()
        assert all(np.array_equal(a, b) for a, b in zip(held, now)) and held[2] > 0
        # removed classes; an upload drops them
        s.set_eval_classes(None)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_eval_classes"):
            s.eval_rows(nodes, 3)
        s.set_eval_classes(node_class)
        s.upload(edge)
        s.set_queries_from_db(nodes, 0)
        s.search(True, False, 16)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_eval_classes"):
            s.eval_rows(nodes, 3)
        with pytest.raises(sat.SatError, match=r"\[-5\].*sat_eval_classes"):
            s.eval_tables(nodes)
        # ordinals of a shard: the classes are the whole database's
        s.upload(edge, db_ordinal=np.arange(n) + 100)
        with pytest.raises(sat.SatError, match=r"\[-1\].*ordinal %d" % (n + 99)):
            s.set_eval_classes(np.zeros(n + 99, np.int32))
        whole = np.full(n + 100, -1, np.int32)
        whole[100:] = node_class
        whole[:100] = 1
        s.set_eval_classes(whole)
        s.set_queries_from_db(nodes, 0)
        s.search(True, False, 16)
        got = s.eval_rows(nodes + 100, 3)
        eval_lib.same_rows(got, eval_lib.expected_rows(s.results()[0], edge.orders, nodes + 100, whole, 3, ordinals=np.arange(n) + 100),
                           "entries at ordinals 100 ..")


# ---------------------------------------------------------------- 6. command line
def cli(golden_dir, args, stdin=b"not read\n"):
    return subprocess.run([CLI, "-r", "16", "-s", "77", *args], input=stdin, cwd=golden_dir, capture_output=True, timeout=300)


def scores_from_rows(stdout, names):
    """(query indices, scores [nq, entries]) of the blocks `-k entries` printed"""
    index = {name: i for i, name in enumerate(names)}
    assert len(index) == len(names)
    queries, scores = [], []
    for line in stdout.decode().splitlines():
        if line.startswith("# QUERY ID = "):
            queries.append(index[line[len("# QUERY ID = "):].strip()])
            scores.append(np.full(len(names), -2**31, np.int64))
        elif not line.startswith("#"):
            name, score = line.split()[:2]
            scores[-1][index[name]] = int(score)
    scores = np.array(scores)
    assert (scores > -2**31).all()
    return np.array(queries), scores


@pytest.fixture(scope="module")
def class_file(small, tmp_path_factory):
    """a seeded 7-way split of the 586 names, a tenth of them not listed, two names the database does not have, comments"""
    rng = np.random.default_rng(21)
    tokens = ["a.%d.%d" % (k, k * k) for k in range(7)]
    listed = rng.random(586) >= 0.1
    pick = rng.integers(0, 7, 586)
    path = tmp_path_factory.mktemp("classes") / "small.classes"
    lines = ["# name class", ""]
    lines += ["%s\t%s" % (name, tokens[pick[v]]) for v, name in enumerate(small.names) if listed[v]]
    lines[40:40] = ["nobody1 a.0.0", "   # indented comment", "nobody2   z.9"]
    path.write_text("\n".join(lines))                                      # no trailing newline
    # ids in order of first appearance among the listed names
    order, node_class = [], np.full(586, -1, np.int32)
    for v in np.nonzero(listed)[0]:
        if tokens[pick[v]] not in order:
            order.append(tokens[pick[v]])
        node_class[v] = order.index(tokens[pick[v]])
    return str(path), node_class, order


@pytest.mark.parametrize("options,sids", [([], None), (["-G", "0,0"], None), (["-P", "2", "-A"], None), ([], [5, 300, 17, 585, 5]),
                                          (["-N", "3"], None)],
                         ids=["plain", "G00", "P2A", "Q", "N3"])
def test_cli_lines_follow_from_the_k_rows(golden_dir, small, class_file, options, sids):
    path, node_class, tokens = class_file
    names = list(small.names)
    source = ["-a", SMALL_DB] if sids is None else ["-Q", SMALL_DB]
    stdin = b"not read\n" if sids is None else "".join(names[i] + "\n" for i in sids).encode()
    rocn = 3 if "-N" in options else 50
    listing = [o for o in options if o not in ("-N", "3")]
    rows = cli(golden_dir, source + ["-k", "586"] + listing, stdin)
    got = cli(golden_dir, source + ["-E", path] + options, stdin)
    assert rows.returncode == 0 and got.returncode == 0, got.stderr.decode()[-400:]
    queries, scores = scores_from_rows(rows.stdout, names)
    assert queries.tolist() == (list(range(586)) if sids is None else sids)
    want = eval_lib.expected_rows(scores, small.orders[queries], queries, node_class, rocn)
    lines = report.eval_table([names[q] for q in queries], tokens, want, SMALL_DB, path, 586, int((node_class >= 0).sum()), 16, rocn,
                              polish_all=2 if "-P" in options else 0)
    out = got.stdout.decode().splitlines()
    assert out == lines
    assert out[0].startswith("# EVAL dbfile = %s classes = %s entries = 586 classified = " % (SMALL_DB, path)) and " distinct = 7 " in out[0]
    # the means again, from the printed lines alone
    head = 3 if "-P" in options else 2
    cols = [line.split() for line in out[head:]]
    assert len(cols) == len(queries) and all(len(c) == 9 for c in cols)
    both = [c for c in cols if c[7] != "NA"]
    assert all((c[7] == "NA") == (c[8] == "NA") == (int(c[2]) == 0 or int(c[3]) == 0) for c in cols)
    auc = [int(c[4]) / (2.0 * int(c[2]) * int(c[3])) for c in both]
    rocs = [int(c[5]) / (2.0 * int(c[2]) * int(c[6])) for c in both]
    assert all("%.6f" % a == c[7] and "%.6f" % r == c[8] for a, r, c in zip(auc, rocs, both))
    assert out[head - 1] == "# MEAN queries = %d auc = %.6f rocn = %.6f" % (len(both), sum(auc) / len(both), sum(rocs) / len(both))
    assert len(both) > 0.8 * len(queries) and any(c[1] == "-" for c in cols) == bool((node_class[queries] < 0).any())
    assert b"WARNING: 2 names of " in got.stderr and got.stderr.count(b"GPU execution time") == rows.stderr.count(b"GPU execution time")
    assert b"# QUERY ID" not in got.stdout


def test_cli_without_E_prints_what_it_printed(golden_dir, small):
    one = cli(golden_dir, ["-a", SMALL_DB, "-k", "3"])
    two = cli(golden_dir, ["-a", SMALL_DB, "-k", "3"])
    assert one.returncode == 0 and one.stdout.count(b"# QUERY ID") == 586 and one.stdout == two.stdout and b"EVAL" not in one.stdout
