"""Queries taken from the resident database on the GPU (-m gpu): sat_queries_from_db builds a batch on the device from
entry indices.  The batch's bytes against sat_queries_set's for the same structures, over every size class and both edges
of each, non-finite distances, `?` codes and cells of 100 A and above; the searches that follow; the state the call
leaves; its errors; the shards of sat_multi_queries_from_db; and the command line's -Q and -a against -q."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import edge_cases as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
PACKED_ORDERS = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 111)      # both edges of the classes 16, 32, 64 and 112


def dense_queries(db, idx):
    return [db.dense(int(e)) + (db.ssetypes(int(e)),) for e in idx]


@pytest.fixture(scope="module")
def edge(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, ec.EDGE_DB))
    assert len(db) == 28 and tuple(db.orders) == ec.EDGE_ORDERS
    assert (db.tab == ec.UNKNOWN).any() and (db.dist >= 100.0).any()
    return db


@pytest.fixture(scope="module")
def packed():
    """a packed upload made here: the orders at the class edges, a NaN, a +inf and a -inf distance cell, every type code"""
    base = sat.synth.make_db(len(PACKED_ORDERS), orders=np.array(PACKED_ORDERS, np.int32), seed=77, sort=False)
    tab, dist = base.tab.copy(), base.dist.copy()

    def cell(s, i, j):
        return int(base.cell_off[s]) + i * (i + 1) // 2 + j

    dist[cell(4, 16, 3)] = np.nan            # 17 SSEs: the last row of the entry
    dist[cell(7, 32, 31)] = np.inf           # 33 SSEs
    dist[cell(10, 110, 0)] = -np.inf         # 111 SSEs
    dist[cell(1, 1, 0)] = np.nan             # 2 SSEs: the only off-diagonal cell
    for i, ty in enumerate((0, 1, 2, 3, 3, 2, 1, 0)):
        tab[cell(3, i, i)] = ty              # 16 SSEs
        tab[cell(10, 100 + i, 100 + i)] = ty
    db = sat.StructSet(base.orders, base.names, base.cell_off, tab, dist)
    assert tuple(db.orders) == PACKED_ORDERS and np.isnan(db.dist).sum() == 2 and np.isinf(db.dist).sum() == 2
    assert set(db.ssetypes(3).tolist()) == {0, 1, 2, 3}
    return db


def index_lists(n):
    order = np.arange(n, dtype=np.int32)
    repeat = np.concatenate([order[::3], order[:4], order[::3][::-1]]).astype(np.int32)
    return {"file order": order, "reversed": order[::-1].copy(), "repeat": repeat}


# ---------------------------------------------------------------- 1. blob bytes
@pytest.mark.parametrize("which", ["edge", "packed"])
def test_blob_bytes_equal_the_host_built_batch(edge, packed, which):
    db = edge if which == "edge" else packed
    with sat.Searcher(0) as s:
        s.upload(db)
        for what, idx in index_lists(len(db)).items():
            s.set_queries(dense_queries(db, idx), 3)
            want = s.debug_query_blob()
            s.set_queries_from_db(idx, 3)
            got = s.debug_query_blob()
            assert got.size == want.size, what
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, "%s, %s: %d bytes differ, the first at %d (got %d want %d)" % (
                which, what, bad.size, bad[0], got[bad[0]], want[bad[0]])
        # the sentinel is in the batch where the cells are not finite: the raw cells were read
        s.set_queries_from_db([1], 0)
        blob = s.debug_query_blob()
        if which == "packed":
            qdist = blob[:16 * 4 * 16].view(np.float32).reshape(4, 16, 4)       # [group][column i][k in the group]
            assert qdist[0, 1, 0] == np.float32(1.0e30) and qdist[0, 0, 1] == np.float32(1.0e30)


# ---------------------------------------------------------------- 2. search results
@pytest.mark.parametrize("which", ["edge", "packed"])
def test_searches_equal_those_of_the_dense_batch(edge, packed, which):
    db = edge if which == "edge" else packed
    idx = index_lists(len(db))["repeat"]
    with sat.Searcher(0) as s:
        s.upload(db)
        want, got = [], []
        for out, from_db in ((want, False), (got, True)):
            if from_db:
                s.set_queries_from_db(idx, 7)
            else:
                s.set_queries(dense_queries(db, idx), 7)
            for lorder in (True, False):
                scores, maps, _ = s.search(lorder, True, 100)
                out += [scores, maps, s.topk_hits(5)]
        for w, g in zip(want, got):
            assert w.shape == g.shape and w.tobytes() == g.tobytes()
        # a batch of one query of one SSE
        one = int(np.nonzero(db.orders == 1)[0][0])
        s.set_queries(dense_queries(db, [one]), 7)
        want = s.search(True, True, 100)[:2]
        s.set_queries_from_db([one], 7)
        got = s.search(True, True, 100)[:2]
        assert got[0].shape == (1, len(db)) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---------------------------------------------------------------- 3. state
def test_state_after_the_call(edge, packed):
    idx = np.array([0, 5, 9, 21, 5], np.int32)
    with sat.Searcher(0) as s:
        s.upload(edge)
        s.set_queries(dense_queries(edge, idx), 0)
        blob_bytes = s.debug_query_blob().size
        s.search(True, False, 16)
        s.fit_statistics(0.1)
        s.set_polish_all(2)
        before = s.query_h2d_bytes()
        s.set_queries_from_db(idx, 0)
        assert s.query_h2d_bytes() - before == 4 * len(idx)
        assert s.polish_all() == 2
        s.set_polish_all(0)
        assert s._lib.sat_query_count(s._ctx) == len(idx) and s.n_queries == len(idx)
        with pytest.raises(sat.SatError, match=r"\[-5\]"):
            s.results()
        with pytest.raises(sat.SatError, match=r"\[-5\]"):
            s.topk_hits(3)
        s.search(True, False, 16)
        hits = s.topk_hits(5)                  # the built-in statistics: the fit went with the old batch
        before = s.query_h2d_bytes()
        s.set_queries(dense_queries(edge, idx), 0)
        assert s.query_h2d_bytes() - before == blob_bytes
        s.search(True, False, 16)
        assert s.topk_hits(5).tobytes() == hits.tobytes()
        # the batch is a copy: another database goes up under it
        s.upload(packed)
        want = s.search(True, True, 16)[:2]
        s.upload(edge)
        s.set_queries_from_db(idx, 0)
        s.upload(packed)
        got = s.search(True, True, 16)[:2]
        assert got[0].shape == (len(idx), len(packed))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---------------------------------------------------------------- 4. errors
def test_errors_leave_the_previous_batch(edge):
    idx = np.array([6, 2, 14], np.int32)
    with sat.Searcher(0) as s:
        with pytest.raises(sat.SatError, match=r"\[-5\].*no database"):
            s.set_queries_from_db([0])
        s.upload(edge)
        s.set_queries_from_db(idx, 1)
        want = s.search(True, False, 32)[0]
        blob = s.debug_query_blob()
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 1: entry -1 "):
            s.set_queries_from_db([3, -1, 4], 1)
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 2: entry 28 "):
            s.set_queries_from_db([3, 4, len(edge)], 1)
        with pytest.raises(sat.SatError, match=r"\[-1\]"):
            s.set_queries_from_db([], 1)
        assert s._lib.sat_queries_from_db(s._ctx, 3, None, 1) == -1
        assert s._lib.sat_query_count(s._ctx) == 3 and np.array_equal(s.debug_query_blob(), blob)
        s.n_queries, s._batch = 3, True
        assert np.array_equal(s.search(True, False, 32)[0], want)


def test_queued_work_is_waited_for():
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    db = sat.synth.make_db(3000, 8, 24, seed=4)
    idx = np.array([10, 2000, 2999], np.int32)
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries_from_db(idx, 0)
        want = s.search(True, False, 256)[0]
        s.search_async(True, False, 256)
        s.set_queries_from_db(idx[::-1].copy(), 0)       # returns only after the queued search
        dev = np.empty_like(want)
        assert hip.hipMemcpy(dev.ctypes.data, s.device_scores_ptr(), dev.nbytes, 2) == 0     # device -> host, no wait of its own
        assert np.array_equal(dev, want)


# ---------------------------------------------------------------- 5. shards
@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]], ids=["1", "2", "3"])
def test_shards_build_and_exchange_their_queries(edge, devices):
    with sat.MultiSearcher(len(devices), devices=devices) as m:
        m.upload(edge)
        begin = m.shards()
        picks = []
        for g in range(len(devices)):
            picks += [int(begin[g]), int(begin[g + 1]) - 1]            # the first and the last entry of every shard
        idx = np.array(picks[::-1] + [1, picks[0], 20], np.int32)
        assert len(set(np.searchsorted(begin, idx, side="right").tolist())) == len(devices)
        m.set_queries(dense_queries(edge, idx), 2)
        want = m.search(True, True, 32)[:2] + m.search_topk(4, False, True, 32)[:2]
        m.set_queries_from_db(idx, 2)
        got = m.search(True, True, 32)[:2] + m.search_topk(4, False, True, 32)[:2]
        for w, g in zip(want, got):
            assert w.shape == g.shape and w.tobytes() == g.tobytes()
        with pytest.raises(sat.SatError, match=r"\[-1\].*query 0: entry 28 "):
            m.set_queries_from_db([len(edge)], 2)
        assert m.search(True, True, 32)[0].tobytes() == want[0].tobytes()


# ---------------------------------------------------------------- 6. command line
def cli(golden_dir, args, stdin):
    return subprocess.run([CLI, "-r", "16", *args], input=stdin, cwd=golden_dir, capture_output=True, timeout=120)


@pytest.mark.parametrize("args", [[], ["-k", "3"], ["-p", "0.5"], ["-G", "0,0"]], ids=["plain", "k3", "p0.5", "G00"])
def test_cli_Q_prints_what_q_prints(golden_dir, args):
    stdin = ec.edge_sids()[1].encode()
    q = cli(golden_dir, ["-q", ec.EDGE_DB, *args], stdin)
    Q = cli(golden_dir, ["-Q", ec.EDGE_DB, *args], stdin)
    assert q.returncode == 0 and Q.returncode == 0, Q.stderr.decode()[-400:]
    assert q.stdout.count(b"# QUERY ID") >= 7 and Q.stdout == q.stdout


def test_cli_all_vs_all(golden_dir, edge):
    q = cli(golden_dir, ["-q", ec.EDGE_DB, "-k", "3"], "".join(n + "\n" for n in edge.names).encode())
    a = cli(golden_dir, ["-a", ec.EDGE_DB, "-k", "3"], b"not read\n")
    assert q.returncode == 0 and a.returncode == 0, a.stderr.decode()[-400:]
    assert q.stdout.count(b"# QUERY ID") == len(edge) and a.stdout == q.stdout


def test_cli_unknown_sid(golden_dir):
    stdin = (ec.edge_name(3) + "\nnosuch1\n").encode()
    q = cli(golden_dir, ["-q", ec.EDGE_DB], stdin)
    Q = cli(golden_dir, ["-Q", ec.EDGE_DB], stdin)
    assert q.returncode == Q.returncode == 1 and Q.stdout == q.stdout == b""
    assert b"ERROR: query nosuch1 not found\n" in q.stderr and b"ERROR: query nosuch1 not found\n" in Q.stderr
