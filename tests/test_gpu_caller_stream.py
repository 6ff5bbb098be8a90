"""The promise of sat_use_stream (-m gpu): "queue all further work of this context on the caller's stream" - the way
bench.py runs the product, and what INTEGRATION.md names for ordering a search with a caller's copies and collectives.
Every other GPU module runs on the context's private stream and reads results through a call that synchronises it.  Here
the caller owns the stream (tests/stream_lib.py, tests/native/stream_probe.hip): the default stream, a blocking and a
non-blocking one; the caller's own work - a delay kernel of D microseconds, a device-side copy of the score buffer - is
queued around the library's, and nothing is synchronised that the header does not say is.

0. a control on memory the test owns: the delay really lets an unordered host read see the state before it; when it does
   not hold, the race tests are skipped with that reason rather than passing vacuously.
a. a device-side consumer queued straight behind search_async sees the whole search (the joins of every side lane);
b. so does a host read behind an event the caller records there - the benchmark's pattern;
c. the next search does not overwrite the score buffer ahead of the caller's pending copy of it (the fork);
d. set_queries and upload do not free or replace the buffer under that copy;
e. every host-reading call family waits for the caller's work in front of it;
f. ten call-history walks, every kind of call among them, with the delay in front of every step;
g. upload_search equals upload + search on every stream kind, in one piece and in three;
h. use_stream / use_own_stream drain the stream they leave, and the polish-all setting survives the switches;
i. two contexts on one caller's stream; search_timed there;
j. torch's current stream, as bench.py hands it over.
Expected values come from the CPU (oracle_lib and, through history_lib, matches_lib, polish_lib, select_lib), never from
a second GPU context - except in g, whose statement is "equal to upload + search".  Where a test compares a whole row with
an earlier, synchronised search of the same context, a sample of that row across all order buckets is held against the
oracle.  MultiSearcher has no use_stream: its shards keep their private streams, and nothing here covers it."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import report
import exact_lib as xl
import history_lib as hl
import oracle_lib
import reach_lib as rl
import stream_lib as sl
from test_gpu_history import data_steps, follow

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The delay in front of the library's work, microseconds.  Measured on the MI355X: the control below
# held in 20 of 20 fresh tries at 1, 2, 5 and 10 ms; the smallest of them doubled.
D_US = 2000
KINDS = sl.KINDS
FIRST = 3                                   # ordinal of the first query of the batch


def control(d_us, n=4096):
    """(what an unordered read saw while the delay ran, what it saw behind an event recorded behind the fill)"""
    st = sl.stream_create(False)
    try:
        with sl.buffer_i32(n) as buf:
            sl.fill_i32(st, buf, 0, n)
            sl.stream_sync(st)
            sl.busy(st, d_us)
            sl.fill_i32(st, buf, 7, n)
            early = sl.read_unordered(buf, n)
            sl.wait_behind(st)
            late = sl.read_unordered(buf, n)
            return early, late
    finally:
        sl.stream_sync(st)
        sl.stream_destroy(st)


@pytest.fixture(scope="module")
def window():
    """the race tests ask for this: they mean something only while the delay opens the window"""
    control(D_US)                                                       # (the first launch also loads the code object)
    early, late = control(D_US)
    if not ((early == 0).all() and (late == 7).all()):
        pytest.skip("the control does not hold: a delay of %d us did not keep an unordered read in front of the work "
                    "behind it (%d of %d words already written)" % (D_US, int((early != 0).sum()), early.size))
    return D_US


def test_control_the_delay_opens_the_window():
    """on a non-blocking stream: fill 0, synchronise, then delay and fill 7 - a plain hipMemcpy at once sees 0
    everywhere (it is not ordered behind the stream, and the delay outlasts it), and 7 everywhere behind an event
    recorded behind the fill.  The delay itself lasts about D: not shorter, and its cap does not cut in."""
    control(D_US)
    for _ in range(3):
        t0 = time.perf_counter()
        early, late = control(D_US)
        took = time.perf_counter() - t0
        print("control: %d words early, %d late, %.2f ms" % ((early != 0).sum(), (late != 7).sum(), took * 1e3))
        assert (early == 0).all(), "%d of %d words were written before the delay ended" % ((early != 0).sum(), early.size)
        assert (late == 7).all()
        assert took >= D_US * 1e-6
    st = sl.stream_create(False)
    try:
        sl.wait_behind(st)
        t0 = time.perf_counter()
        sl.busy(st, D_US)
        sl.wait_behind(st)
        took = time.perf_counter() - t0
        print("the delay alone: %.3f ms" % (took * 1e3))
        assert took >= D_US * 1e-6                          # the iteration cap (8 per microsecond) has not cut it short
    finally:
        sl.stream_destroy(st)


# ---------------------------------------------------------------- the database, the queries, the restarts, the oracle
class World:
    """6000 entries of 4..70 SSEs, sorted by size (five order buckets), under a 12-SSE and a 40-SSE query (two size
    classes): ten launches on seven side streams.  r: the restart count at which the search - of both queries, and of
    the 40-SSE one alone - lasts at least 1.1 D, by search_timed on the day.  Oracle rows are made once per
    (query, lorder) on a sample of ten entries per bucket, the first and the last of each among them."""

    def __init__(self):
        self.db, self.queries = sl.world_inputs()
        self.n = len(self.db)
        sample = []
        for lo in range(1, 81, 16):
            idx = np.nonzero((self.db.orders >= lo) & (self.db.orders < lo + 16))[0]
            assert len(idx) >= 10, lo
            sample += idx[np.linspace(0, len(idx) - 1, 10).astype(int)].tolist()
        self.sample = np.array(sample)
        assert len(self.sample) >= 48
        self._oracle = {}
        need = 1.1 * D_US * 1e-3
        with sat.Searcher(0) as s:
            s.upload(self.db)
            self.r, self.ms = 32, {}
            while True:
                self.r *= 2
                assert self.r <= 1024, "the search stays under %.2f ms up to 1024 restarts: %s" % (need, self.ms)
                for name in ("both", "one"):
                    s.set_queries(self.queries, FIRST) if name == "both" else s.set_query(*self.queries[1], FIRST + 1)
                    s.search(True, False, 1)
                    self.ms[name] = min(s.search_timed(lorder, False, self.r)[0] for lorder in (True, False))
                    assert s.last_launch_info().count(";") + 1 >= 2
                if min(self.ms.values()) >= need:
                    break
        print("world: %d restarts, the search lasts %s ms" % (self.r, self.ms))

    def oracle(self, q, lorder):
        """scores of query q on the sample"""
        if (q, lorder) not in self._oracle:
            self._oracle[(q, lorder)] = oracle_lib.search(self.db, *self.queries[q], lorder, False, self.r, entries=self.sample,
                                                          query_ordinal=FIRST + q)[0]
        return self._oracle[(q, lorder)]

    def check(self, rows, lorder, queries=(0, 1)):
        """rows [len(queries), n] (or flat) against the oracle on the sample"""
        rows = np.asarray(rows).reshape(len(queries), self.n)
        for k, q in enumerate(queries):
            want = self.oracle(q, lorder)
            bad = np.nonzero(rows[k][self.sample] != want)[0]
            assert len(bad) == 0, "query %d, lorder %s: %d of %d sampled entries differ from the oracle, first entry %d: %d, oracle %d" % (
                q, lorder, len(bad), len(want), self.sample[bad[0]], rows[k][self.sample[bad[0]]], want[bad[0]])


@pytest.fixture(scope="module")
def world():
    return World()


def launches(s):
    return s.last_launch_info().count(";") + 1


@pytest.fixture(params=KINDS)
def on_stream(request):
    """(stream handle, a Searcher that queues on it): the searcher is closed before the stream goes"""
    with sl.caller_stream(request.param) as st:
        with sat.Searcher(0) as s:
            s.use_stream(st)
            yield st, s


# ---------------------------------------------------------------- a. consumer behind the search
def test_consumer_queued_behind_the_search_sees_all_of_it(window, world, on_stream):
    st, s = on_stream
    n2 = 2 * world.n
    with sl.buffer_i32(n2) as snap:
        s.upload(world.db)
        s.set_queries(world.queries, FIRST)
        s.search_async(False, False, 1)                     # other rows in the buffer; the descriptors are made
        s.sync()
        sl.fill_i32(st, snap, -1, n2)
        sl.busy(st, window)
        s.search_async(True, False, world.r)
        sl.copy_i32(st, snap, s.device_scores_ptr(), n2)
        assert launches(s) >= 2
        sl.wait_behind(st)                                  # the caller waits for its own copy, not for the context
        got = sl.read_unordered(snap, n2)
        world.check(got, True)
        full, _ = s.results()
        assert np.array_equal(got.reshape(2, world.n), full)


# ---------------------------------------------------------------- b. the event the benchmark records
def test_event_recorded_behind_the_search_covers_all_of_it(world, on_stream):
    """a fresh upload leaves the one score row zeroed, and the first search of one query fills that buffer: what a host
    read sees behind the caller's event is the whole search, whichever lane ran a launch and whichever stream the
    library queued on"""
    st, s = on_stream
    s.upload(world.db)
    s.set_query(*world.queries[1], FIRST + 1)
    ptr = s.device_scores_ptr()
    sl.wait_behind(st)
    assert (sl.read_unordered(ptr, world.n) == 0).all()
    s.search_async(True, False, world.r)
    ev = sl.event_create()
    try:
        sl.event_record(ev, st)
        assert s.device_scores_ptr() == ptr and launches(s) >= 2
        sl.event_sync(ev)
        got = sl.read_unordered(ptr, world.n)
    finally:
        sl.event_destroy(ev)
    world.check(got, True, (1,))
    assert np.array_equal(got, s.results()[0])


# ---------------------------------------------------------------- c. the next search and the caller's pending read
def test_next_search_waits_for_the_callers_pending_read(window, world, on_stream):
    st, s = on_stream
    n2 = 2 * world.n
    with sl.buffer_i32(n2) as snap:
        s.upload(world.db)
        s.set_queries(world.queries, FIRST)
        first = s.search(True, False, world.r)[0].copy()
        second = s.search(False, False, world.r)[0].copy()
        world.check(first, True)
        world.check(second, False)
        assert (first != second).mean() > 0.25              # the two searches can be told apart
        sl.fill_i32(st, snap, -1, n2)
        s.search_async(True, False, world.r)
        assert launches(s) >= 2
        sl.busy(st, window)
        sl.copy_i32(st, snap, s.device_scores_ptr(), n2)
        s.search_async(False, False, world.r)
        assert launches(s) >= 2
        now, _ = s.results()
        sl.wait_behind(st)
        got = sl.read_unordered(snap, n2).reshape(2, world.n)
        assert np.array_equal(got, first), "%d rows of the snapshot are not the first search's (%d are the second's)" % (
            (got != first).sum(), ((got != first) & (got == second)).sum())
        assert np.array_equal(now, second)


# ---------------------------------------------------------------- d. buffers are not freed under the caller
@pytest.mark.parametrize("how", ["set_queries", "upload"])
def test_score_buffer_is_not_replaced_under_the_callers_read(window, world, on_stream, how):
    """the buffer in front of the caller's copy holds another search's row (no LORDER, one restart), so the snapshot
    tells the queued search from what lay there before; that the buffer was replaced is read from the device: the
    allocation behind device_scores_ptr() (hipMemGetAddressRange) is larger afterwards, and an allocation does not
    grow in place - the new one may reuse the address, so the pointer alone says nothing"""
    st, s = on_stream
    q0, q1 = world.queries
    with sl.buffer_i32(world.n) as snap:
        s.upload(world.db)
        s.set_query(*q1, FIRST + 1)
        first = s.search(True, False, world.r)[0].copy()
        world.check(first, True, (1,))
        other = s.search(False, False, 1)[0]
        assert (other != first).mean() > 0.25
        sl.fill_i32(st, snap, -1, world.n)
        s.search_async(True, False, world.r)
        sl.busy(st, window)
        before = s.device_scores_ptr()
        before_bytes = sl.alloc_bytes(before)
        assert before_bytes >= 4 * world.n
        sl.copy_i32(st, snap, before, world.n)
        if how == "set_queries":
            s.set_queries([q0, q1, q0], FIRST)              # three rows: the buffer of one row is too small
            rows = s.search(True, False, world.r)[0]
            world.check(rows[:2], True)
        else:
            bigger = sat.synth.make_db(7000, 4, 70, seed=22, sort=True)
            s.upload(bigger)                                # the query stays; 7000 rows do not fit into 6000
            rows = s.search(True, False, 64)[0]
            some = np.arange(0, 7000, 601)
            assert np.array_equal(rows[some], oracle_lib.search(bigger, *q1, True, False, 64, entries=some, query_ordinal=FIRST + 1)[0])
        after_bytes = sl.alloc_bytes(s.device_scores_ptr())
        print("score buffer: %#x, %d bytes -> %#x, %d bytes" % (before, before_bytes, s.device_scores_ptr(), after_bytes))
        assert after_bytes >= 4 * rows.size and after_bytes > before_bytes
        assert np.array_equal(sl.read_unordered(s.device_scores_ptr(), rows.size), rows.ravel())
        got = sl.read_unordered(snap, world.n)              # (both calls have waited for the stream)
        assert np.array_equal(got, first), "%d rows of the snapshot are not the queued search's (%d are the search's before it)" % (
            (got != first).sum(), ((got != first) & (got == other)).sum())


# ---------------------------------------------------------------- e. host-reading calls wait for the caller's stream
def host_reading_ops():
    """every call family that copies to the host, on the 40 entries and five queries of history_lib's d32 / q5 world"""
    op = hl.op
    pairs = dict(lorder=True, r=3, pairs=7)
    return [op("upload", db="d32"), op("set_queries", batch="q5"), op("set_eval_classes"),
            op("search_async_results", lorder=True, lsoln=True, r=3), op("results", lsoln=True),
            op("topk_hits", k=3, maps=True), op("hits_cutoff", frac=0.6, k=None, maps=True), op("score_histogram"),
            op("fit_statistics", censor=0.0), op("profile_rows", frac=0.6, gaps=False), op("eval_rows", rocn=3),
            op("cluster_begin"), op("cluster_add", frac=0.4), op("cluster_labels"),
            op("cover_begin"), op("cover_add", frac=0.4), op("cover_solve"),
            op("search_matches", lorder=True, r=3, m=3, maps=True), op("search_pairs", lsoln=True, **pairs),
            op("search_pairs_matches", m=3, maps=True, **pairs), op("search_pairs_polish", tops=3, **pairs),
            op("search_refine", lorder=True, r=1, big_r=hl.rmax_of("d32"), cand=12, k=3, lsoln=True)]


def test_host_reading_calls_wait_for_the_callers_work(window, on_stream):
    st, s = on_stream
    ops = host_reading_ops()
    assert follow(s, ops, before_step=lambda s_, m: sl.busy(st, window)) == data_steps(ops) == 15


@pytest.fixture(scope="module")
def exact_rows():
    """tests/test_gpu_exact.py's database and queries: the host twin at 64 nodes a row from the oracle's plain rows"""
    db = xl.gpu_db()
    queries = xl.gpu_queries(db)
    base, maps = xl.sa_rows(db, queries, True, 1, xl.GPU_FIRST)
    return db, queries, base, xl.host_rows(db, queries, True, xl.BUDGET_NODES, base, maps)


def test_exact_search_waits_for_the_callers_work(window, on_stream, exact_rows):
    st, s = on_stream
    db, queries, base, (hs, hm, hf, hn) = exact_rows
    sl.busy(st, window)
    s.upload(db)
    sl.busy(st, window)
    s.set_queries(queries, xl.GPU_FIRST)
    sl.busy(st, window)
    scores, maps, _ = s.search_exact(True, 1, xl.BUDGET_NODES)
    sl.busy(st, window)
    gbase, flags, nodes = s.exact_results()
    assert np.array_equal(gbase, base)
    for k, (g, w) in enumerate(((scores, hs), (maps, hm), (flags, hf), (nodes, hn))):
        assert np.array_equal(g, w), k


REACH_N, REACH_P = 40, 1e-3
REACH_EDGES = ((0, 1), (0, 5), (1, 2), (5, 3), (2, 3), (3, 0), (7, 8))       # 3 at depth 2 from 5, a second step from 2; 7 -> 8 unreached


def test_reach_calls_wait_for_the_callers_work(window, on_stream):
    """the step API of the transitive search over planted scores (norm2 16: p-value 0; score 0: above the cutoff), as
    tests/test_gpu_reach.py plants them, against reach_lib's accumulator"""
    st, s = on_stream
    db = sat.synth.make_db(REACH_N, 8, 20, seed=31, sort=False)
    lo, hi = int(db.orders.min()), int(db.orders.max())
    for n1 in (lo, hi):
        for n2 in (lo, hi):
            assert report.stats(8 * (n1 + n2), n1, n2)[2] == 0.0 and report.stats(0, n1, n2)[2] > REACH_P
    q, e = np.array(REACH_EDGES).T
    scores = np.zeros((REACH_N, REACH_N), np.int32)
    scores[q, e] = 8 * (db.orders[q] + db.orders[e])
    nodes = np.arange(REACH_N)
    acc = rl.Accumulator(REACH_N, [0])
    s.upload(db)
    s.set_queries_from_db(nodes, 0)
    s.search(True, False, 1)                                # only to reach the searched state
    s.reach_begin([0])
    for d in range(1, 6):
        frontier = acc.frontier(d - 1)
        sl.busy(st, window)
        got, count = s.reach_frontier(d - 1)
        assert count == len(frontier) and np.array_equal(got, frontier), d
        if not len(frontier):
            break
        active = np.isin(nodes, frontier)
        s.debug_set_scores(scores * active[:, None])
        sl.busy(st, window)
        s.reach_add(d, REACH_P, nodes)
        cells = np.isin(q, frontier)
        acc.add(d, q[cells], e[cells], np.zeros(int(cells.sum())))
    assert d == 4
    sl.busy(st, window)
    rows, count = s.reach_rows()
    want = acc.rows()
    assert count == len(want) == 5
    rl.same_rows(rows, want, "reach")
    by_node = {int(r["node"]): r for r in rows}
    assert by_node[3]["depth"] == 2 and by_node[3]["parent"] == 5 and by_node[3]["support"] == 2 and by_node[0]["support"] == 1


# ---------------------------------------------------------------- f. the call-history walks on a caller's stream
@pytest.mark.parametrize("walk", range(10), ids=[name for name, _ in hl.caller_stream_walks()])
def test_history_walk_on_a_callers_stream(on_stream, walk):
    """tests/test_gpu_history.py's follow(), every comparison of it, with the delay queued in front of every step"""
    st, s = on_stream
    ops = hl.caller_stream_walks()[walk][1]
    assert follow(s, ops, before_step=lambda s_, m: sl.busy(st, D_US)) == data_steps(ops)


# ---------------------------------------------------------------- g. upload_search under each stream kind
@pytest.mark.parametrize("lsoln", [True, False])
@pytest.mark.parametrize("pieces", [0, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_overlapped_upload_on_a_callers_stream(monkeypatch, world, kind, pieces, lsoln):
    """tests/test_gpu_parity.py::test_overlapped_upload_and_first_search on a caller's stream - the header's three cases
    of sat_db_upload_search: both contexts queue on the one stream (on the default stream the pieces are copied and
    searched in turn: same results)"""
    if pieces:
        monkeypatch.setenv("SAT_EXP_UPLOAD_PIECES", str(pieces))
    db, queries = world.db, world.queries
    ordinal = np.arange(len(db)) + 1000
    with sl.caller_stream(kind) as st:
        with sat.Searcher(0) as a, sat.Searcher(0) as b:
            a.use_stream(st)
            b.use_stream(st)
            a.upload(db, db_ordinal=ordinal)
            a.set_queries(queries, FIRST)
            want, want_maps, _ = a.search(True, lsoln, 64)
            b.set_queries(queries, FIRST)
            sl.busy(st, D_US)
            b.upload_search(db, True, lsoln, 64, db_ordinal=ordinal)
            got, got_maps = b.results(lsoln=lsoln)
            assert np.array_equal(got, want) and (not lsoln or np.array_equal(got_maps, want_maps))
            want2, _, _ = a.search(False, False, 64)
            got2, _, _ = b.search(False, False, 64)
            assert np.array_equal(got2, want2)
    sample = np.random.default_rng(1).choice(len(db), 24, replace=False)
    ref, ref_maps, _ = oracle_lib.search(db, *queries[0], True, True, 64, entries=sample, query_ordinal=FIRST, db_ordinal=ordinal)
    assert np.array_equal(got[0][sample], ref)
    assert not lsoln or np.array_equal(got_maps[0][sample], ref_maps)


def test_overlapped_upload_rejects_a_bad_cell_on_the_default_stream(monkeypatch):
    """the refusal of tests/test_gpu_parity.py::test_overlapped_upload_rejects_what_the_plain_upload_rejects: the same
    error text, and the context is left without a database"""
    monkeypatch.setenv("SAT_EXP_UPLOAD_PIECES", "4")
    db = sat.synth.make_db(4000, 6, 20, seed=8)
    q = sat.synth.make_query(10, seed=2)
    tab = db.tab.copy()
    tab[int(db.cell_off[3900]) + 3 * 4 // 2 + 1] = 0x99
    with sat.Searcher(0) as s:
        s.use_stream(0)
        s.set_query(*q, 0)
        with pytest.raises(sat.SatError, match="entry 3900: tableau code"):
            s.upload_search(sat.StructSet(db.orders, db.names, db.cell_off, tab, db.dist), True, False, 64)
        with pytest.raises(sat.SatError, match="no database"):
            s.search()
        s.upload_search(db, True, False, 64)
        got, _ = s.results()
    some = np.arange(0, 4000, 173)
    assert np.array_equal(got[some], oracle_lib.search(db, *q, True, False, 64, entries=some)[0])


# ---------------------------------------------------------------- h. switching streams
@pytest.mark.parametrize("kind", KINDS)
def test_switching_streams_drains_the_one_left(window, kind):
    """A (of each kind) -> the private stream -> B (non-blocking) -> the default stream, a search in flight behind the
    caller's delay at every switch; each stream is destroyed only after the context has left it.  The polish-all
    setting made before the first switch holds throughout: every search is a polished one (history_lib's d32 / q5
    world, whose polished rows come from polish_lib)."""
    w = hl.world_ref("d32", "q5")
    rows = lambda lorder, r, lsoln: w.matrix(hl.Searched(lorder, r, lsoln, 3))
    with sat.Searcher(0) as s:
        with sl.caller_stream(kind) as a:
            s.use_stream(a)
            s.upload(hl.db("d32"))
            s.set_queries(*hl.batch("q5"))
            s.set_polish_all(3)
            sl.busy(a, window)
            s.search_async(True, True, 3)
            s.use_own_stream()
            sc, mp = s.results(True)
            want = rows(True, 3, True)
            assert np.array_equal(sc, want[0]) and np.array_equal(mp, want[1])
        with sl.caller_stream("nonblocking") as b:
            s.search_async(False, False, 3)                 # on the private stream
            s.use_stream(b)
            assert np.array_equal(s.results()[0], rows(False, 3, False)[0])
            sl.busy(b, window)
            s.search_async(True, False, 1)
            s.use_stream(0)
            assert np.array_equal(s.results()[0], rows(True, 1, False)[0])
            assert s.polish_all() == 3
            assert np.array_equal(s.results_base(), w.polished(True, 1, 3)[1])
        sl.busy(0, window)
        assert np.array_equal(s.search(False, False, 1)[0], rows(False, 1, False)[0])       # on the default stream, b gone


# ---------------------------------------------------------------- i. two contexts on one stream; search_timed
def test_two_contexts_on_one_callers_stream(window, world, on_stream):
    st, x = on_stream
    small = sat.synth.make_db(3000, 8, 24, seed=4)
    q = sat.synth.make_query(16)
    some = np.arange(0, 3000, 97)
    with sat.Searcher(0) as y:
        y.use_stream(st)
        x.upload(world.db)
        x.set_queries(world.queries, FIRST)
        y.upload(small)
        y.set_query(*q, 0)
        sl.busy(st, window)
        x.search_async(True, False, world.r)
        y.search_async(True, False, 64)
        mine, _ = y.results()
        theirs, _ = x.results()
        world.check(theirs, True)
        assert np.array_equal(mine[some], oracle_lib.search(small, *q, True, False, 64, entries=some)[0])
        sl.busy(st, window)
        total, kernel = x.search_timed(True, False, world.r)
        assert total > 0 and kernel > 0
        assert np.array_equal(x.results()[0], theirs)
        y.use_own_stream()                                  # y is closed first, but x's stream outlives both anyway


# ---------------------------------------------------------------- j. torch, as bench.py does it
def test_torch_stream_as_the_benchmark_hands_it_over(world, tmp_path):
    """use_stream(torch's current stream), search_async, a clone of device_scores_tensor() with nothing synchronised,
    then the search with the other LORDER: after torch.cuda.synchronize() the clone is the first search's row - on
    torch's default stream and inside `with torch.cuda.stream(torch.cuda.Stream())`.  In a process of its own
    (tests/torch_stream_child.py), which imports torch before the device library as bench.py does: the two then share
    one HIP runtime, which a process that has loaded the library first does not give them."""
    out = str(tmp_path / "rows.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_stream_child.py"), out, str(world.r), str(FIRST)],
                   check=True, timeout=120)
    rows = np.load(out)
    for where in ("current", "side"):
        first, second = rows[where + "_clone"], rows[where + "_results"]
        world.check(first, True)
        world.check(second, False)
        assert (first.reshape(2, -1) != second).mean() > 0.25
