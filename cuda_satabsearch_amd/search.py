"""GPU search: thin object wrapper over the C ABI (include/satabsearch.h).

Argument names and meaning follow the reference kernel contract
(nvcc_src_current/cudaSaTabsearch_kernel.cu:756-802): lorder, lsoln, maxstart,
scores per db entry, ssemap[entry][query SSE] = matched db SSE or -1.
"""
import ctypes as C

import numpy as np

from . import _native
from ._native import SatError
from .structures import StructSet

MAXDIM = _native.MAXDIM
DEFAULT_MAXSTART = 128   # saparams.h:40
DEFAULT_SEED = 1234      # cudaSaTabsearch.cu:263, :871


def device_count():
    return int(_native.device_lib().sat_device_count())


def sa_kernel_instances():
    """Test hook (satabsearch_debug.h): the names of every SA kernel instantiation the library can launch, spelled as
    last_launch_info() spells them.  Needs no device."""
    lib = _native.device_lib()
    if not hasattr(lib, "sat_debug_sa_instances"):
        raise SatError(f"{_native.DEVICE_LIB} does not export sat_debug_sa_instances (a build from before the hook)")
    return lib.sat_debug_sa_instances().decode().splitlines()


def _pack_queries(queries):
    """a list of (qtab[n1, n1+], qdmat, qssetypes) triples as sat_queries_set takes a batch: (nq, pitch, n1s int32[nq],
    tabs uint8[nq, pitch, pitch], dmats float32[nq, pitch, pitch], types uint8[nq, pitch])"""
    nq = len(queries)
    pitch = max(int(np.asarray(q[0]).shape[0]) for q in queries)
    n1s = np.empty(nq, np.int32)
    tabs = np.zeros((nq, pitch, pitch), np.uint8)
    dmats = np.zeros((nq, pitch, pitch), np.float32)
    types = np.zeros((nq, pitch), np.uint8)
    for k, (t, d, ty) in enumerate(queries):
        t = np.asarray(t, np.uint8)
        d = np.asarray(d, np.float32)
        n1 = t.shape[0]
        n1s[k] = n1
        tabs[k, :n1, :n1] = t[:, :n1]
        dmats[k, :n1, :n1] = d[:, :n1]
        types[k, :n1] = np.asarray(ty, np.uint8)[:n1] if ty is not None else np.diagonal(t)[:n1]
    return nq, pitch, n1s, tabs, dmats, types


def _pack_sse_lists(sses, nq):
    """the motif lists of set_queries_from_db as sat_queries_from_db_sses takes them: (sse_begin int32[nq + 1], sse
    uint8[total], never of size 0); an item that is None or empty - the whole entry - is an empty range"""
    if len(sses) != nq:
        raise ValueError("sses needs one item per query")
    lists = [np.zeros(0, np.int64) if l is None else np.asarray(l, dtype=np.int64).ravel() for l in sses]
    if any(((l < 0) | (l > 255)).any() for l in lists):
        raise ValueError("an SSE index outside 0..255")
    begin = np.zeros(nq + 1, np.int32)
    begin[1:] = np.cumsum([len(l) for l in lists])
    sse = np.zeros(max(int(begin[-1]), 1), np.uint8)
    if begin[-1]:
        sse[:begin[-1]] = np.concatenate(lists)
    return begin, sse


def _pair_lists(queries, entries):
    """a pair list as the pair searches take it: two int32 arrays of one length"""
    q = np.ascontiguousarray(queries, dtype=np.int32).ravel()
    e = np.ascontiguousarray(entries, dtype=np.int32).ravel()
    if q.shape != e.shape:
        raise ValueError("queries and entries differ in length")
    return q, e


def _search_matches(obj, fn, handle, max_matches, lorder, maxstart, maps):
    nq, n, m = obj.n_queries, obj.n_entries, max(int(max_matches), 1)
    counts = np.zeros((nq, n), np.int32)
    scores = np.zeros((nq, n, m), np.int32)
    restarts = np.zeros((nq, n, m), np.int32)
    ssemaps = np.full((nq, n, m, MAXDIM), -1, np.int32) if maps else None
    ms = C.c_double(0.0)
    obj._check(fn(handle, int(bool(lorder)), int(maxstart), int(max_matches), counts.ctypes.data, scores.ctypes.data,
                  restarts.ctypes.data, ssemaps.ctypes.data if maps else None, C.byref(ms)))
    return counts, scores, restarts, (ssemaps[..., :obj.n1max] if maps else None), ms.value


def _search_pairs_matches(obj, fn, handle, queries, entries, max_matches, lorder, maxstart, maps):
    """shared by Searcher / MultiSearcher.search_pairs_matches"""
    q, e = _pair_lists(queries, entries)
    p, m = len(q), max(int(max_matches), 1)
    counts = np.zeros(p, np.int32)
    scores = np.zeros((p, m), np.int32)
    restarts = np.zeros((p, m), np.int32)
    ssemaps = np.full((p, m, MAXDIM), -1, np.int32) if maps else None
    ms = C.c_double(0.0)
    obj._check(fn(handle, int(bool(lorder)), int(maxstart), int(max_matches), p, q.ctypes.data, e.ctypes.data,
                  counts.ctypes.data, scores.ctypes.data, restarts.ctypes.data, ssemaps.ctypes.data if maps else None,
                  C.byref(ms)))
    return counts, scores, restarts, (ssemaps[..., :obj.n1max] if maps else None), ms.value


def _search_pairs_polish(obj, fn, handle, queries, entries, tops, lorder, maxstart):
    """shared by Searcher / MultiSearcher.search_pairs_polish"""
    q, e = _pair_lists(queries, entries)
    p = len(q)
    scores, base, restarts, moves = (np.zeros(p, np.int32) for _ in range(4))
    ssemaps = np.full((p, MAXDIM), -1, np.int32)
    ms = C.c_double(0.0)
    obj._check(fn(handle, int(bool(lorder)), int(maxstart), int(tops), p, q.ctypes.data, e.ctypes.data, scores.ctypes.data,
                  base.ctypes.data, restarts.ctypes.data, moves.ctypes.data, ssemaps.ctypes.data, C.byref(ms)))
    return scores, base, restarts, moves, ssemaps[:, :getattr(obj, "n1max", MAXDIM)], ms.value


# struct sat_hit (include/satabsearch.h) as a numpy record: the rows of topk_hits, search_topk and search_refine
_HIT_DTYPE = np.dtype([("entry", np.int32), ("score", np.int32), ("norm2", np.float64), ("zscore", np.float64),
                       ("pvalue", np.float64)], align=True)
assert _HIT_DTYPE.itemsize == C.sizeof(_native.Hit)


# struct sat_fit (include/satabsearch.h) as a numpy record: fit_statistics, set_statistics, search_fit
_REORDER_DTYPE = np.dtype([("hit", _HIT_DTYPE), ("base_pvalue", np.float64), ("base_score", np.int32), ("kind", np.int32),
                           ("matched", np.int32), ("descents", np.int32), ("cut", np.int32), ("pad", np.int32)], align=True)
assert _REORDER_DTYPE.itemsize == C.sizeof(_native.ReorderHit) == 64
KIND_SEQUENTIAL, KIND_CIRCULAR, KIND_PERMUTED, KIND_ALL = 1, 2, 4, 7

_EXACT_STAT_DTYPE = np.dtype([("rows", np.int64), ("proven", np.int64), ("improved", np.int64), ("gain", np.int64),
                              ("nodes", np.uint64)])
_REACH_DTYPE = np.dtype([("node", np.int32), ("depth", np.int32), ("parent", np.int32), ("support", np.int32),
                         ("pvalue", np.float32)])
assert _REACH_DTYPE.itemsize == C.sizeof(_native.ReachRow) == 20
REACH_STOP = {_native.REACH_EXHAUSTED: "exhausted", _native.REACH_DEPTH: "depth", _native.REACH_BUDGET: "budget"}
_FIT_DTYPE = np.dtype([("a", np.float64), ("b", np.float64), ("rows", np.int32), ("censored", np.int32),
                       ("below", np.int32), ("fitted", np.int32)], align=True)
assert _FIT_DTYPE.itemsize == C.sizeof(_native.Fit)
STAT_BINS = _native.STAT_BINS
_EVAL_DTYPE = np.dtype([("u2", np.uint64), ("t2", np.uint64), ("positives", np.int32), ("negatives", np.int32),
                        ("n_used", np.int32), ("query_class", np.int32)], align=True)
assert _EVAL_DTYPE.itemsize == C.sizeof(_native.Eval) == 32


def _score_histogram(obj, fn, handle, nq):
    """shared by Searcher / MultiSearcher.score_histogram: (counts uint32[nq, 4096], below int32[nq])"""
    counts = np.zeros((nq, STAT_BINS), np.uint32)
    below = np.zeros(nq, np.int32)
    obj._check(fn(handle, counts.ctypes.data, below.ctypes.data))
    return counts, below


def _fit_records(fits, nq):
    """set_statistics' argument as sat_fit records: a _FIT_DTYPE array, or a sequence of (a, b) pairs / None per
    query (None: that query keeps the built-in constants)"""
    if isinstance(fits, np.ndarray) and fits.dtype == _FIT_DTYPE:
        rec = np.ascontiguousarray(fits).ravel()
    else:
        rec = np.zeros(len(fits), _FIT_DTYPE)
        for q, f in enumerate(fits):
            if f is not None:
                rec[q]["a"], rec[q]["b"], rec[q]["fitted"] = float(f[0]), float(f[1]), 1
    if len(rec) != nq:
        raise ValueError("one fit per query is needed")
    return rec


def _search_refine(obj, call, k, candidates, refine_maxstart, lsoln):
    """shared by Searcher / MultiSearcher.search_refine: `call(hits, maps, first)` runs the C entry point"""
    nq = getattr(obj, "n_queries", 1)
    kk = max(1, min(int(k), int(candidates), obj.n_entries))
    hits = np.zeros((nq, kk), _HIT_DTYPE)
    maps = np.full((nq, kk, MAXDIM), -1, np.int32) if lsoln else None
    first = np.zeros((nq, kk), np.int32)
    n = call(hits.ctypes.data, maps.ctypes.data if lsoln else None, first.ctypes.data)
    if n < 0:
        obj._check(n)
    return hits, maps, first


def _search_refine_polish(obj, call, k, candidates, refine_maxstart, lsoln):
    """shared by Searcher / MultiSearcher.search_refine_polish: `call(hits, maps, first, base)` runs the C entry point"""
    base = []

    def with_base(h, m, f):
        base.append(np.zeros(max(1, min(int(k), int(candidates), obj.n_entries)) * getattr(obj, "n_queries", 1), np.int32))
        return call(h, m, f, base[0].ctypes.data)

    hits, maps, first = _search_refine(obj, with_base, k, candidates, refine_maxstart, lsoln)
    return hits, maps, first, base[0].reshape(first.shape)


def _hits_cutoff(obj, nq, lsoln, first, again, dtype=_HIT_DTYPE):
    """shared by Searcher.hits_cutoff / MultiSearcher.search_cutoff: `first(counts, capacity, hits, maps)` runs the C
    entry point once; when the rows did not fit, `again` (same arguments) selects them again into a buffer of the
    returned size.  Returns (list of nq hit arrays, list of nq int32[rows, 111] map arrays or None).  (dtype: the rows
    of reorder_hits, which has the same contract.)"""
    counts = np.zeros(nq, np.int32)
    cap = max(int(getattr(obj, "_cutoff_cap", 0)), 256)
    for call in (first, again):
        hits = np.zeros(cap, dtype)
        maps = np.full((cap, MAXDIM), -1, np.int32) if lsoln else None
        n = call(counts.ctypes.data, cap, hits.ctypes.data, maps.ctypes.data if lsoln else None)
        if n < 0:
            obj._check(n)
        if n <= cap:
            break
        cap = n
    obj._cutoff_cap = cap
    cuts = np.cumsum(counts)[:-1]
    rows = np.split(hits[:n], cuts)
    return rows, (np.split(maps[:n], cuts) if lsoln else None)


def _baseline_results(obj, fn, handle, nq):
    """shared by Searcher / MultiSearcher.baseline_results"""
    scores = np.empty((nq, obj.n_entries), np.int32)
    pvalues = np.empty((nq, obj.n_entries), np.float64)
    obj._check(fn(handle, scores.ctypes.data, pvalues.ctypes.data))
    return scores, pvalues


def _reorder_hits(obj, fn, handle, nq, max_pvalue, min_base_pvalue, kinds, k, lsoln):
    """shared by Searcher / MultiSearcher.reorder_hits"""
    call = lambda c, cap, h, m: fn(handle, float(max_pvalue), float(min_base_pvalue), int(kinds), int(k or 0), c, cap, h, m)
    rows, maps = _hits_cutoff(obj, nq, lsoln, call, call, _REORDER_DTYPE)
    return (rows, maps) if lsoln else rows


def _cluster_add(obj, fn, handle, max_pvalue, query_nodes):
    """shared by Searcher / MultiSearcher.cluster_add"""
    nodes = np.ascontiguousarray(query_nodes, dtype=np.int32).ravel()
    if len(nodes) != getattr(obj, "n_queries", 1):
        raise ValueError("one node per query of the batch is needed")
    obj._check(fn(handle, float(max_pvalue), nodes.ctypes.data))


def _cluster_labels(obj, fn, handle, n_nodes):
    """shared by Searcher / MultiSearcher.cluster_labels: (labels int32[n], degrees int32[n], edges)"""
    labels = np.zeros(n_nodes, np.int32)
    degrees = np.zeros(n_nodes, np.int32)
    edges = C.c_ulonglong(0)
    obj._check(fn(handle, labels.ctypes.data, degrees.ctypes.data, C.byref(edges)))
    return labels, degrees, int(edges.value)


def _reach_begin(obj, call, seeds):
    """shared by Searcher / MultiSearcher.reach_begin: call(n_seeds, pointer)"""
    seeds = np.ascontiguousarray(() if seeds is None else seeds, dtype=np.int32).ravel()
    obj._check(call(len(seeds), seeds.ctypes.data if len(seeds) else None))


def _reach_add(obj, fn, handle, depth, max_pvalue, query_nodes):
    """shared by Searcher / MultiSearcher.reach_add"""
    nodes = np.ascontiguousarray(query_nodes, dtype=np.int32).ravel()
    if len(nodes) != getattr(obj, "n_queries", 1):
        raise ValueError("one node per query of the batch is needed")
    obj._check(fn(handle, int(depth), float(max_pvalue), nodes.ctypes.data))


def _reach_frontier(obj, fn, handle, depth, cap):
    """shared by Searcher / MultiSearcher.reach_frontier: (nodes int32[min(cap, count)], count).  cap None: all of them,
    by a call that asks for the count alone first"""
    count = C.c_int32(0)
    if cap is None:
        obj._check(fn(handle, int(depth), 0, None, C.byref(count)))
        cap = count.value
    nodes = np.empty(int(cap), np.int32)
    obj._check(fn(handle, int(depth), int(cap), nodes.ctypes.data if cap else None, C.byref(count)))
    return nodes[:min(int(cap), count.value)].copy(), int(count.value)


def _reach_rows(obj, fn, handle, cap):
    """shared by Searcher / MultiSearcher.reach_rows: (rows [min(cap, count)], count); cap None as _reach_frontier"""
    count = C.c_int32(0)
    if cap is None:
        obj._check(fn(handle, 0, None, C.byref(count)))
        cap = count.value
    rows = np.zeros(int(cap), _REACH_DTYPE)
    obj._check(fn(handle, int(cap), rows.ctypes.data if cap else None, C.byref(count)))
    return rows[:min(int(cap), count.value)].copy(), int(count.value)


def _search_reach(obj, fn, handle, n_nodes, seeds, max_pvalue, max_depth, max_queries, batch, censor, first_query_ordinal, cap,
                  lorder, maxstart):
    """shared by Searcher / MultiSearcher.search_reach: (rows, info dict)"""
    seeds = np.ascontiguousarray(seeds, dtype=np.int32).ravel()
    cap = int(n_nodes if cap is None else cap)
    rows = np.zeros(cap, _REACH_DTYPE)
    count = C.c_int32(0)
    info = _native.ReachInfo()
    obj._check(fn(handle, len(seeds), seeds.ctypes.data if len(seeds) else None, int(bool(lorder)), int(maxstart), float(max_pvalue),
                  int(max_depth), int(n_nodes if max_queries is None else max_queries), int(batch),
                  -1.0 if censor is None else float(censor), int(first_query_ordinal), cap, rows.ctypes.data if cap else None,
                  C.byref(count), C.byref(info)))
    return rows[:min(cap, count.value)].copy(), {
        "levels": int(info.levels), "queries": int(info.queries), "reached": int(info.reached), "stop": REACH_STOP[int(info.stop)],
        "search_ms": float(info.search_ms), "pass_ms": float(info.pass_ms)}


def _reach_last_batch(obj, frontier_fn, handle, out, batch, order_of):
    """the Python side of the batch a search_reach left in the library: the tail of the last level searched, read from
    the accumulator the run left (4 bytes a node) - the rows may be capped and need not show that level"""
    info = out[1]
    if not info["queries"]:
        return
    level, _ = _reach_frontier(obj, frontier_fn, handle, info["levels"] - 1, None)
    last = level[len(level) - ((len(level) - 1) % int(batch) + 1):]
    n1s = np.array([order_of(int(v)) for v in last], np.int32)
    obj.n1, obj.n1max, obj._n1s, obj.n_queries, obj._batch = int(n1s[0]), int(n1s.max()), n1s, len(last), True


def _cluster_levels(pvalues):
    """the cutoffs of cluster_begin_levels as the library takes them: (count, float64 array)"""
    cuts = np.ascontiguousarray(pvalues, dtype=np.float64).ravel()
    return len(cuts), cuts


def _cluster_add_levels(obj, fn, handle, query_nodes):
    """shared by Searcher / MultiSearcher.cluster_add_levels"""
    nodes = np.ascontiguousarray(query_nodes, dtype=np.int32).ravel()
    if len(nodes) != getattr(obj, "n_queries", 1):
        raise ValueError("one node per query of the batch is needed")
    obj._check(fn(handle, nodes.ctypes.data))


def _cluster_labels_levels(obj, fn, handle, n_levels, n_nodes):
    """shared by Searcher / MultiSearcher.cluster_labels_levels: (labels int32[L, n], degrees int32[L, n], edges uint64[L])"""
    if not n_levels:
        obj._check(fn(handle, None, None, None))            # the library's state error
    labels = np.zeros((n_levels, n_nodes), np.int32)
    degrees = np.zeros((n_levels, n_nodes), np.int32)
    edges = np.zeros(n_levels, np.uint64)
    obj._check(fn(handle, labels.ctypes.data, degrees.ctypes.data, edges.ctypes.data))
    return labels, degrees, edges


def _cover_solve(obj, fn, handle, n_nodes):
    """shared by Searcher / MultiSearcher.cover_solve: (rep int32[n], degrees int32[n], edges, rounds)"""
    rep = np.zeros(n_nodes, np.int32)
    degrees = np.zeros(n_nodes, np.int32)
    edges = C.c_ulonglong(0)
    rounds = C.c_int(0)
    obj._check(fn(handle, rep.ctypes.data, degrees.ctypes.data, C.byref(edges), C.byref(rounds)))
    return rep, degrees, int(edges.value), int(rounds.value)


def _eval_nodes(obj, query_nodes):
    """the queries' nodes as the evaluation calls take them"""
    nodes = np.ascontiguousarray(query_nodes, dtype=np.int32).ravel()
    if len(nodes) != getattr(obj, "n_queries", 1):
        raise ValueError("one node per query of the batch is needed")
    return nodes


def _profile_rows_raw(obj, fn, handle, max_pvalue, query_node, hits, joint, offset):
    """shared by Searcher / MultiSearcher.profile_rows_raw"""
    node = None if query_node is None else np.ascontiguousarray(query_node, dtype=np.int32).ravel()
    if node is not None and len(node) != getattr(obj, "n_queries", 1):
        raise ValueError("one node per query of the batch is needed")
    off = None if offset is None else np.ascontiguousarray(offset, dtype=np.int64).ravel()
    if off is not None and len(off) != getattr(obj, "n_queries", 1):
        raise ValueError("one offset per query of the batch is needed")
    ptr = lambda a: None if a is None else a.ctypes.data
    obj._check(fn(handle, float(max_pvalue), ptr(node), ptr(hits), ptr(joint), ptr(off)))


def _profile_rows(obj, fn, handle, max_pvalue, query_node):
    """shared by Searcher / MultiSearcher.profile_rows"""
    n1s = obj._n1s.astype(np.int64)
    cuts = np.concatenate([[0], np.cumsum(n1s * n1s)])
    hits = np.zeros(len(n1s), np.uint32)
    joint = np.zeros(max(int(cuts[-1]), 1), np.uint32)
    _profile_rows_raw(obj, fn, handle, max_pvalue, query_node, hits, joint, None)
    return hits, [joint[cuts[q]:cuts[q + 1]].reshape(int(n1s[q]), int(n1s[q])) for q in range(len(n1s))]


def _eval_rows(obj, fn, handle, query_nodes, rocn):
    """shared by Searcher / MultiSearcher.eval_rows"""
    nodes = _eval_nodes(obj, query_nodes)
    rows = np.zeros(len(nodes), _EVAL_DTYPE)
    obj._check(fn(handle, nodes.ctypes.data, int(rocn), rows.ctypes.data))
    return rows


class Searcher:
    """One HIP device, one resident database shard, one current query."""

    def __init__(self, device=0, seed=DEFAULT_SEED):
        self._lib = _native.device_lib()
        self._ctx = self._lib.sat_ctx_create(int(device), int(seed))
        if not self._ctx:
            raise SatError(self._lib.sat_last_error().decode())
        self.device = int(device)
        self.n_entries = 0
        self.n1 = 0

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.sat_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise SatError(f"[{rc}] {self._lib.sat_last_error().decode()}")

    # ---- database -----------------------------------------------------------
    def upload(self, db: StructSet, db_ordinal=None):
        """Upload a (shard of a) database.  db_ordinal[e] = position of entry e in the
        whole database's file order; it keys the random streams so that sharding does
        not change results.  Default: 0..N-1."""
        n = len(db)
        ordinal = None
        if db_ordinal is not None:
            ordinal = np.ascontiguousarray(db_ordinal, dtype=np.int64)
            if ordinal.shape[0] != n:
                raise ValueError("db_ordinal length mismatch")
        self._check(self._lib.sat_db_upload_packed(
            self._ctx, n, db.orders.ctypes.data, db.cell_off.ctypes.data, db.tab.ctypes.data,
            db.dist.ctypes.data, ordinal.ctypes.data if ordinal is not None else None))
        self.n_entries = n
        self._orders = db.orders.copy()
        self._ordinal = ordinal

    def upload_search(self, db: StructSet, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART, db_ordinal=None):
        """upload() and the first search of the query (batch) set before, overlapped: each piece of the
        shard is searched while the next one is copied (sat_db_upload_search).  Collect with results()."""
        n = len(db)
        ordinal = None
        if db_ordinal is not None:
            ordinal = np.ascontiguousarray(db_ordinal, dtype=np.int64)
            if ordinal.shape[0] != n:
                raise ValueError("db_ordinal length mismatch")
        self.n_entries = 0
        self._check(self._lib.sat_db_upload_search(
            self._ctx, n, db.orders.ctypes.data, db.cell_off.ctypes.data, db.tab.ctypes.data,
            db.dist.ctypes.data, ordinal.ctypes.data if ordinal is not None else None,
            int(bool(lorder)), int(bool(lsoln)), int(maxstart)))
        self.n_entries = n
        self._orders = db.orders.copy()
        self._ordinal = ordinal

    def upload_dense(self, orders, tabs, dmats, pitch, db_ordinal=None):
        orders = np.ascontiguousarray(orders, dtype=np.int32)
        tabs = np.ascontiguousarray(tabs, dtype=np.uint8)
        dmats = np.ascontiguousarray(dmats, dtype=np.float32)
        ordinal = None if db_ordinal is None else np.ascontiguousarray(db_ordinal, dtype=np.int64)
        self._check(self._lib.sat_db_upload_dense(
            self._ctx, orders.shape[0], orders.ctypes.data, tabs.ctypes.data, dmats.ctypes.data, int(pitch),
            ordinal.ctypes.data if ordinal is not None else None))
        self.n_entries = int(orders.shape[0])
        self._orders = orders.copy()
        self._ordinal = ordinal

    # ---- query --------------------------------------------------------------
    def set_query(self, qtab, qdmat, qssetypes=None, query_ordinal=0):
        """qtab / qdmat: dense [n1, P] matrices (P >= n1); SSE types default to the
        tableau diagonal (cudaSaTabsearch.cu:410-412)."""
        qtab = np.ascontiguousarray(qtab, dtype=np.uint8)
        qdmat = np.ascontiguousarray(qdmat, dtype=np.float32)
        n1, pitch = qtab.shape[0], qtab.shape[1]
        if qdmat.shape != qtab.shape:
            raise ValueError("qtab and qdmat shapes differ")
        if qssetypes is None:
            qssetypes = np.ascontiguousarray(np.diagonal(qtab)[:n1])
        qssetypes = np.ascontiguousarray(qssetypes, dtype=np.uint8)
        self._check(self._lib.sat_query_set(self._ctx, n1, qtab.ctypes.data, qdmat.ctypes.data, pitch,
                                            qssetypes.ctypes.data, int(query_ordinal)))
        self.n1 = n1
        self.n1max = n1
        self._n1s = np.array([n1], np.int32)
        self.n_queries = 1
        self._batch = False

    def set_queries(self, queries, first_query_ordinal=0):
        """Set a batch of queries scored together by one search(): `queries` is a list of
        (qtab[n1, n1+], qdmat, qssetypes) triples.  search() then returns scores[nq, N]
        (and ssemaps[nq, N, 111]); query q draws from the streams of ordinal
        first_query_ordinal + q."""
        nq, pitch, n1s, tabs, dmats, types = _pack_queries(queries)
        self._check(self._lib.sat_queries_set(self._ctx, nq, n1s.ctypes.data, tabs.ctypes.data, dmats.ctypes.data,
                                              pitch, types.ctypes.data, int(first_query_ordinal)))
        self.n1 = int(n1s[0])
        self.n1max = int(n1s.max())
        self._n1s = np.array(n1s, np.int32)
        self.n_queries = nq
        self._batch = True

    def set_queries_from_db(self, entries, first_query_ordinal=0, sses=None):
        """Set a batch of queries that are entries of the uploaded database (sat_queries_from_db): query q is entry
        entries[q] (any order, repeats allowed).  The batch is built on the device from the resident cells - only the
        indices cross from the host - and is byte for byte the batch set_queries makes of the same structures, so every
        search returns the same results.
        sses: motif queries (sat_queries_from_db_sses) - one item per query, None or empty for the whole entry, else the
        0-based indices of the entry's SSEs the query is made of, in the order given (query SSE i is entry SSE
        sses[q][i]); the query's order is the list's length."""
        idx = np.ascontiguousarray(entries, dtype=np.int32).ravel()
        if sses is None:
            self._check(self._lib.sat_queries_from_db(self._ctx, len(idx), idx.ctypes.data if len(idx) else None,
                                                      int(first_query_ordinal)))
            n1s = self._orders[idx]
        else:
            begin, sse = _pack_sse_lists(sses, len(idx))
            self._check(self._lib.sat_queries_from_db_sses(self._ctx, len(idx), idx.ctypes.data if len(idx) else None,
                                                           begin.ctypes.data, sse.ctypes.data, int(first_query_ordinal)))
            n1s = np.where(np.diff(begin) > 0, np.diff(begin), self._orders[idx])
        self.n1 = int(n1s[0])
        self.n1max = int(n1s.max())
        self._n1s = np.array(n1s, np.int32)
        self.n_queries = len(idx)
        self._batch = True

    def query_h2d_bytes(self):
        """Bytes set_query / set_queries (the whole batch) and set_queries_from_db (4 per query; with sses 8 per query,
        4 and the lists) have copied host -> device so far (sat_stat_query_h2d_bytes)."""
        return int(self._lib.sat_stat_query_h2d_bytes(self._ctx))

    def debug_query_blob(self):
        """Test hook (satabsearch_debug.h): the current query batch as it lies on the device, uint8[bytes]."""
        n = self._lib.sat_debug_query_blob(self._ctx, None, 0)
        if n < 0:
            self._check(int(n))
        blob = np.empty(int(n), np.uint8)
        n = self._lib.sat_debug_query_blob(self._ctx, blob.ctypes.data, blob.size)
        if n < 0:
            self._check(int(n))
        return blob

    def set_query_from(self, queries: StructSet, s, query_ordinal=None):
        t, d = queries.dense(s)
        self.set_query(t, d, queries.ssetypes(s), s if query_ordinal is None else query_ordinal)

    # ---- search -------------------------------------------------------------
    def search(self, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART):
        """Returns (scores int32[N], ssemaps int32[N, 111] or None, kernel_ms)."""
        nq = getattr(self, "n_queries", 1)
        scores = np.empty((nq, self.n_entries), np.int32)
        ssemaps = np.full((nq, self.n_entries, MAXDIM), -1, np.int32) if lsoln else None
        ms = C.c_double(0.0)
        self._check(self._lib.sat_search(self._ctx, int(bool(lorder)), int(bool(lsoln)), int(maxstart),
                                         scores.ctypes.data, ssemaps.ctypes.data if lsoln else None,
                                         C.byref(ms)))
        if not getattr(self, "_batch", False):
            return scores[0], (ssemaps[0] if lsoln else None), ms.value
        return scores, ssemaps, ms.value

    def search_matches(self, max_matches, lorder=True, maxstart=DEFAULT_MAXSTART, maps=True):
        """Up to `max_matches` non-overlapping matches per (query, entry) (sat_search_matches): returns
        (counts int32[nq, N], scores int32[nq, N, M], restarts int32[nq, N, M],
        maps int32[nq, N, M, n1max] or None, kernel_ms) - always with the query axis, n1max = the largest
        query order.  Match 0 is search()'s score and LSOLN map; slots past the count hold 0, -1, all -1."""
        return _search_matches(self, self._lib.sat_search_matches, self._ctx, max_matches, lorder, maxstart, maps)

    def search_pairs(self, queries, entries, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART):
        """Scores of chosen (query, entry) pairs only (sat_search_pairs): queries[p] indexes the current batch,
        entries[p] the resident shard.  Returns (scores int32[P], maps int32[P, 111] or None): exactly what
        search() gives for those rows at the same maxstart."""
        q, e = _pair_lists(queries, entries)
        scores = np.zeros(len(q), np.int32)
        maps = np.full((len(q), MAXDIM), -1, np.int32) if lsoln else None
        ms = C.c_double(0.0)
        self._check(self._lib.sat_search_pairs(self._ctx, int(bool(lorder)), int(bool(lsoln)), int(maxstart), len(q),
                                               q.ctypes.data, e.ctypes.data, scores.ctypes.data,
                                               maps.ctypes.data if lsoln else None, C.byref(ms)))
        return scores, maps

    def search_pairs_matches(self, queries, entries, max_matches, lorder=True, maxstart=DEFAULT_MAXSTART, maps=True):
        """The matches of chosen (query, entry) pairs only (sat_search_pairs_matches): queries[p] indexes the current
        batch, entries[p] the resident shard.  Returns (counts int32[P], scores int32[P, M], restarts int32[P, M],
        maps int32[P, M, n1max] or None, kernel_ms): exactly search_matches()' rows (queries[p], entries[p]) at the
        same maxstart and max_matches."""
        return _search_pairs_matches(self, self._lib.sat_search_pairs_matches, self._ctx, queries, entries, max_matches,
                                     lorder, maxstart, maps)

    def search_refine(self, k, candidates, refine_maxstart, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART):
        """Two-stage search (sat_search_refine): every entry at maxstart, then each query's best `candidates`
        at refine_maxstart.  Returns (hits [nq, k'] shaped like topk_hits with stage-2 scores, maps int32[nq, k', 111]
        or None, stage-1 scores int32[nq, k']), k' = min(k, candidates, N)."""
        return _search_refine(self, lambda h, m, f: self._lib.sat_search_refine(
            self._ctx, int(bool(lorder)), int(bool(lsoln)), int(maxstart), int(candidates), int(refine_maxstart), int(k),
            h, m, f), k, candidates, refine_maxstart, lsoln)

    def search_pairs_polish(self, queries, entries, tops, lorder=True, maxstart=DEFAULT_MAXSTART):
        """Chosen (query, entry) pairs with the own-best maps of their `tops` best restarts polished to local optima
        (sat_search_pairs_polish).  Returns (scores int32[P], base_scores int32[P] = search_pairs' scores, restarts
        int32[P], moves int32[P], maps int32[P, n1max], kernel_ms)."""
        return _search_pairs_polish(self, self._lib.sat_search_pairs_polish, self._ctx, queries, entries, tops, lorder, maxstart)

    def search_refine_polish(self, k, candidates, refine_maxstart, tops, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART):
        """search_refine with the polish as stage 2 (sat_search_refine_polish): returns (hits ranked by polished score,
        polished maps or None, stage-1 scores, scores before the polish int32[nq, k'])."""
        return _search_refine_polish(self, lambda h, m, f, b: self._lib.sat_search_refine_polish(
            self._ctx, int(bool(lorder)), int(bool(lsoln)), int(maxstart), int(candidates), int(refine_maxstart), int(tops),
            int(k), h, m, f, b), k, candidates, refine_maxstart, lsoln)

    def search_exact(self, lorder=True, maxstart=DEFAULT_MAXSTART, max_nodes=_native.EXACT_DEFAULT_NODES):
        """Exact search for queries of up to 16 SSEs (sat_search_exact): the search this searcher's settings make gives
        every row an incumbent, then a branch and bound on the GPU proves every row optimal or replaces it by a strictly
        better map, within max_nodes nodes a row.  Returns (scores, ssemaps, kernel_ms) shaped like search(lsoln=True);
        the rows stand in the ordinary buffers, so results, topk_hits, hits_cutoff and the rest work on them.
        exact_results() has the base scores, the unproven flags and the node counts."""
        ms = C.c_double(0.0)
        self._check(self._lib.sat_search_exact(self._ctx, int(bool(lorder)), int(maxstart), int(max_nodes), C.byref(ms)))
        scores, maps = self.results(lsoln=True)
        return scores, maps, ms.value

    def exact_results(self):
        """(base_scores int32, unproven bool, nodes uint32) of the last exact search, shaped like results()' scores
        (sat_exact_results).  Raises unless the last search was an exact one."""
        nq = getattr(self, "n_queries", 1)
        base = np.empty((nq, self.n_entries), np.int32)
        flag = np.empty((nq, self.n_entries), np.uint8)
        nodes = np.empty((nq, self.n_entries), np.uint32)
        self._check(self._lib.sat_exact_results(self._ctx, base.ctypes.data, flag.ctypes.data, nodes.ctypes.data))
        if not getattr(self, "_batch", False):
            return base[0], flag[0].astype(bool), nodes[0]
        return base, flag.astype(bool), nodes

    def exact_stats(self):
        """Per query of the last exact search, reduced on the device (sat_exact_stats): a structured array [nq] with
        rows, proven, improved, gain (the summed score - base) and nodes."""
        stats = np.zeros(getattr(self, "n_queries", 1), _EXACT_STAT_DTYPE)
        self._check(self._lib.sat_exact_stats(self._ctx, stats.ctypes.data))
        return stats

    def set_polish_all(self, tops):
        """Whole-database polish (sat_polish_all_set): with tops in 1..8 every plain whole-database search of this
        searcher - search, search_async, upload_search - gives every row the score (and with lsoln the map) that
        search_pairs_polish(tops) gives its pair, in the ordinary result buffers: results, topk_hits, hits_cutoff,
        score_histogram and fit_statistics then work on polished rows.  0 turns it off.  A setting like the stream:
        it survives upload and set_queries.  search_matches, the pair searches and stage 1 of the refine calls stay
        plain; search_timed raises while it is on."""
        self._check(self._lib.sat_polish_all_set(self._ctx, int(tops)))

    def polish_all(self):
        """The maps polished per row by a whole-database search, 0 = the mode is off (sat_polish_all_get)."""
        return int(self._lib.sat_polish_all_get(self._ctx))

    def results_base(self):
        """The rows' scores before the polish of the last polished search (sat_results_base), shaped like results()'
        scores: bit for bit the plain search's.  Raises unless the last search was a polished one."""
        nq = getattr(self, "n_queries", 1)
        base = np.empty((nq, self.n_entries), np.int32)
        self._check(self._lib.sat_results_base(self._ctx, base.ctypes.data))
        return base if getattr(self, "_batch", False) else base[0]

    def use_stream(self, stream_handle):
        """Queue all further work on the caller's HIP stream (0 / None = default stream),
        e.g. torch.cuda.current_stream().cuda_stream."""
        self._check(self._lib.sat_use_stream(self._ctx, C.c_void_p(int(stream_handle or 0))))

    def use_own_stream(self):
        self._check(self._lib.sat_use_own_stream(self._ctx))

    def search_async(self, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART):
        """Queue the search on the context's current stream (no sync, no copy); results
        stay in device memory."""
        self._check(self._lib.sat_search_async(self._ctx, int(bool(lorder)), int(bool(lsoln)), int(maxstart)))

    def results(self, lsoln=False):
        """Wait for a queued search_async and fetch (scores, ssemaps or None)."""
        nq = getattr(self, "n_queries", 1)
        scores = np.empty((nq, self.n_entries), np.int32)
        ssemaps = np.full((nq, self.n_entries, MAXDIM), -1, np.int32) if lsoln else None
        self._check(self._lib.sat_results(self._ctx, int(bool(lsoln)), scores.ctypes.data,
                                          ssemaps.ctypes.data if lsoln else None))
        if not getattr(self, "_batch", False):
            return scores[0], (ssemaps[0] if lsoln else None)
        return scores, ssemaps

    def topk(self, k, query=0):
        """(entry_index int32[k'], scores int32[k']) of the best k hits of the last search,
        sorted on the device by descending score, ties in database order."""
        idx = np.empty(k, np.int32)
        sc = np.empty(k, np.int32)
        n = self._lib.sat_topk(self._ctx, int(query), int(k), idx.ctypes.data, sc.ctypes.data)
        if n < 0:
            self._check(n)
        return idx[:n], sc[:n]

    def topk_hits(self, k, lsoln=False):
        """Best-k rows of every query of the last search, ranked on the device with their statistics:
        a structured array [nq, k'] with fields entry, score, norm2, zscore, pvalue (and the rows'
        solution maps int32[nq, k', 111] when lsoln)."""
        nq = getattr(self, "n_queries", 1)
        k = min(int(k), self.n_entries)
        hits = np.zeros((nq, k), _HIT_DTYPE)
        maps = np.full((nq, k, MAXDIM), -1, np.int32) if lsoln else None
        n = self._lib.sat_topk_hits(self._ctx, k, hits.ctypes.data, maps.ctypes.data if lsoln else None)
        if n < 0:
            self._check(n)
        return (hits, maps) if lsoln else hits

    def hits_cutoff(self, max_pvalue, k=None, lsoln=False):
        """Every row of the last search whose p-value is <= max_pvalue (sat_hits_cutoff), selected on the device:
        a list of nq structured arrays shaped like topk_hits' rows, each in topk_hits order and cut to its first k
        (k None or <= 0: no cut); with lsoln also a list of nq int32[rows, 111] map arrays."""
        nq = getattr(self, "n_queries", 1)
        call = lambda c, cap, h, m: self._lib.sat_hits_cutoff(self._ctx, float(max_pvalue), int(k or 0), c, cap, h, m)
        rows, maps = _hits_cutoff(self, nq, lsoln, call, call)
        return (rows, maps) if lsoln else rows

    # ---- hits out of sequence order (sat_baseline_*, sat_reorder_hits) ----------
    def baseline_keep(self):
        """Keep the rows of the last search - score and p-value, an installed fit followed - on the device as the
        baseline of reorder_hits (sat_baseline_keep): 12 bytes a row, nothing crosses to the host, no wait.  An upload
        and every query-setting call drop it; searches and fits leave it alone."""
        self._check(self._lib.sat_baseline_keep(self._ctx))

    def baseline_drop(self):
        self._check(self._lib.sat_baseline_drop(self._ctx))

    def baseline_results(self):
        """The kept baseline: (scores int32[nq, n_entries], pvalues float64[nq, n_entries])."""
        return _baseline_results(self, self._lib.sat_baseline_results, self._ctx, getattr(self, "n_queries", 1))

    def reorder_hits(self, max_pvalue, min_base_pvalue=0.0, kinds=KIND_CIRCULAR | KIND_PERMUTED, k=None, lsoln=False):
        """The rows of the last search (one with lsoln) that hits_cutoff(max_pvalue) returns, whose kept baseline p-value
        is >= min_base_pvalue and whose map's order is one of `kinds` (an OR of KIND_SEQUENTIAL, KIND_CIRCULAR,
        KIND_PERMUTED), selected on the device (sat_reorder_hits): a list of nq structured arrays with fields hit (a
        hits_cutoff row), base_pvalue, base_score, kind, matched, descents, cut; in hits_cutoff's order, cut to the first
        k; with lsoln also the list of int32[rows, 111] maps."""
        return _reorder_hits(self, self._lib.sat_reorder_hits, self._ctx, getattr(self, "n_queries", 1), max_pvalue,
                             min_base_pvalue, kinds, k, lsoln)

    def search_reordered(self, maxstart=DEFAULT_MAXSTART, censor=None):
        """The ordered search, kept as the baseline, then the unordered search with maps (sat_search_reordered); censor
        not None: each fitted to its own scores (fit_statistics).  reorder_hits - and every other selection call - then
        works on the unordered search.  Returns the two searches' kernel_ms."""
        ms = C.c_double(0.0)
        self._check(self._lib.sat_search_reordered(self._ctx, int(maxstart), -1.0 if censor is None else float(censor), C.byref(ms)))
        return ms.value

    def score_histogram(self):
        """The histogram of the last search's norm2 scores, made on the device (sat_score_histogram):
        (counts uint32[nq, 4096], below int32[nq]) - bin floor(norm2 * 256), the last bin the overflow; rows with a
        negative score are counted in `below`."""
        return _score_histogram(self, self._lib.sat_score_histogram, self._ctx, getattr(self, "n_queries", 1))

    def fit_statistics(self, censor=0.0):
        """Fit every query's Gumbel parameters to the last search's own scores (sat_stats_fit: histogram on the device,
        maximum-likelihood fit with the top `censor` of the rows right-censored) and install them: topk_hits and
        hits_cutoff then give z and p from the fit, until the next search.  Returns a record array [nq] with fields
        a, b, rows, censored, below, fitted (fitted 0: no fit exists, that query keeps the built-in constants)."""
        fits = np.zeros(getattr(self, "n_queries", 1), _FIT_DTYPE)
        self._check(self._lib.sat_stats_fit(self._ctx, float(censor), fits.ctypes.data))
        return fits

    def set_statistics(self, fits):
        """Install the caller's Gumbel parameters for the last search (sat_stats_set): a fit_statistics() array, or
        one (a, b) pair / None per query; None puts every query back on the built-in constants."""
        if fits is None:
            self._check(self._lib.sat_stats_set(self._ctx, None))
            return
        rec = _fit_records(fits, getattr(self, "n_queries", 1))
        self._check(self._lib.sat_stats_set(self._ctx, rec.ctypes.data))

    # ---- clustering (sat_cluster_*) ------------------------------------------
    def cluster_begin(self, n_nodes=None):
        """Start (or restart, emptied) the single-linkage accumulator over n_nodes nodes - the structures of the whole
        database in file order; default: the uploaded entries, right when this searcher holds the whole database with
        the default ordinals."""
        n = self.n_entries if n_nodes is None else int(n_nodes)
        self._check(self._lib.sat_cluster_begin(self._ctx, n))
        self._cluster_nodes, self._cluster_levels = n, 0

    def cluster_add(self, max_pvalue, query_nodes):
        """Add the rows of the last search whose p-value - as hits_cutoff tests it: an installed fit and polished rows
        are followed - is <= max_pvalue as edges between query_nodes[q] and the entry's ordinal in the whole database
        (sat_cluster_add); a structure against itself is no edge.  Nothing is copied back."""
        _cluster_add(self, self._lib.sat_cluster_add, self._ctx, max_pvalue, query_nodes)

    def cluster_labels(self):
        """(labels int32[n_nodes]: the smallest node of each node's connected component; degrees int32[n_nodes]: edges
        at each node, repeats counted; edges: their total) of what has been added so far (sat_cluster_labels); more
        cluster_add calls may follow.  report.cluster_table turns them into representatives and sizes."""
        if not getattr(self, "_cluster_nodes", 0):
            self._check(self._lib.sat_cluster_labels(self._ctx, None, None, None))      # the library's state error
        return _cluster_labels(self, self._lib.sat_cluster_labels, self._ctx, self._cluster_nodes)

    def cluster_end(self):
        """Free the accumulator, plain or leveled (sat_cluster_end)."""
        self._check(self._lib.sat_cluster_end(self._ctx))
        self._cluster_nodes = 0
        self._cluster_levels = 0

    # ---- transitive search (sat_reach_*, sat_search_reach) ---------------------
    def reach_begin(self, seeds=None, n_nodes=None):
        """Start (or restart, emptied) the transitive search's accumulator over n_nodes nodes (default as cluster_begin)
        with the nodes `seeds` at depth 0 (sat_reach_begin); no seeds: an external start."""
        n = self.n_entries if n_nodes is None else int(n_nodes)
        _reach_begin(self, lambda c, p: self._lib.sat_reach_begin(self._ctx, n, c, p), seeds)

    def reach_add(self, depth, max_pvalue, query_nodes):
        """Add the rows of the last search that qualify as cluster_add has it as directed steps query_nodes[q] -> the
        entry's node at `depth` (1..62): a node keeps the shallowest depth, then the smallest p, then the smallest parent;
        its support counts every step to it (sat_reach_add).  query_nodes[q] == -1: an external query.  Nothing is copied
        back."""
        _reach_add(self, self._lib.sat_reach_add, self._ctx, depth, max_pvalue, query_nodes)

    def reach_frontier(self, depth, cap=None):
        """(the first `cap` nodes at exactly `depth`, ascending, int32; their uncapped count), compacted on the device
        (sat_reach_frontier).  cap None: all of them."""
        return _reach_frontier(self, self._lib.sat_reach_frontier, self._ctx, depth, cap)

    def reach_rows(self, cap=None):
        """(the first `cap` reached nodes, ascending, as records node, depth, parent, support, pvalue; their uncapped
        count) (sat_reach_rows).  parent -1: a seed or an external query.  report.reach_table prints them."""
        return _reach_rows(self, self._lib.sat_reach_rows, self._ctx, cap)

    def reach_end(self):
        """Free the accumulator (sat_reach_end)."""
        self._check(self._lib.sat_reach_end(self._ctx))

    def search_reach(self, seeds, max_pvalue, max_depth=_native.REACH_MAX_DEPTH, max_queries=None, batch=256, censor=None,
                     first_query_ordinal=0, cap=None, lorder=True, maxstart=DEFAULT_MAXSTART):
        """Transitive search from the entries `seeds` (sat_search_reach): level d searches the nodes first reached at
        depth d - 1, in ascending node order and batches of `batch`, and adds their hits at max_pvalue, until nothing new
        turns up, max_depth is reached or a level would take the queries past max_queries (default: every node once).
        censor not None: each batch fitted to its own scores.  Returns (rows as reach_rows, info: levels, queries,
        reached, stop = "exhausted" / "depth" / "budget", search_ms, pass_ms).  Afterwards the searcher holds the last
        batch, as after set_queries_from_db and search."""
        out = _search_reach(self, self._lib.sat_search_reach, self._ctx, self.n_entries, seeds, max_pvalue, max_depth,
                            max_queries, batch, censor, first_query_ordinal, cap, lorder, maxstart)
        ordinal = getattr(self, "_ordinal", None)
        entry_of = None if ordinal is None else {int(o): e for e, o in reversed(list(enumerate(ordinal)))}
        _reach_last_batch(self, self._lib.sat_reach_frontier, self._ctx, out, batch,
                          lambda v: self._orders[v if entry_of is None else entry_of[v]])
        return out

    # ---- the same at several cutoffs in one pass (sat_cluster_*_levels) -------
    def cluster_begin_levels(self, pvalues, n_nodes=None):
        """Start the LEVELED accumulator: cluster_begin for the 1..8 strictly ascending cutoffs `pvalues` (each in
        [0, 1]) at once, replacing whatever accumulator there was.  A searcher holds one accumulator, plain or leveled;
        the calls of the other kind raise."""
        n = self.n_entries if n_nodes is None else int(n_nodes)
        count, cuts = _cluster_levels(pvalues)
        self._check(self._lib.sat_cluster_begin_levels(self._ctx, n, count, cuts.ctypes.data))
        self._cluster_nodes, self._cluster_levels = n, count

    def cluster_add_levels(self, query_nodes):
        """cluster_add at every level's cutoff in one pass over the rows of the last search (sat_cluster_add_levels):
        a row is an edge of every level whose cutoff its p-value does not exceed.  Nothing is copied back."""
        _cluster_add_levels(self, self._lib.sat_cluster_add_levels, self._ctx, query_nodes)

    def cluster_labels_levels(self):
        """(labels int32[L, n_nodes], degrees int32[L, n_nodes], edges uint64[L]), tightest level first: per level what
        cluster_labels returns for the same adds at that level's cutoff (sat_cluster_labels_levels).  The levels are
        nested: labels[j + 1][labels[j]] == labels[j + 1].  report.cluster_levels_table turns them into tables."""
        return _cluster_labels_levels(self, self._lib.sat_cluster_labels_levels, self._ctx, getattr(self, "_cluster_levels", 0),
                                      getattr(self, "_cluster_nodes", 0))

    # ---- clustering around representatives (sat_cover_*) ----------------------
    def cover_begin(self, n_nodes=None):
        """Start (or restart, emptied) the cover accumulator over n_nodes nodes (default as cluster_begin): the graph
        itself as a bit matrix on the device, n_nodes^2 / 8 bytes.  It lives beside a cluster accumulator."""
        n = self.n_entries if n_nodes is None else int(n_nodes)
        self._check(self._lib.sat_cover_begin(self._ctx, n))
        self._cover_nodes = n

    def cover_add(self, max_pvalue, query_nodes):
        """cluster_add's rows as UNDIRECTED edges of the graph (sat_cover_add): a pair seen twice or in both directions
        is one edge.  Nothing is copied back."""
        _cluster_add(self, self._lib.sat_cover_add, self._ctx, max_pvalue, query_nodes)

    def cover_solve(self):
        """(rep int32[n_nodes], degrees int32[n_nodes]: distinct neighbours, edges: distinct pairs, rounds: the clusters
        of two or more members) of the greedy cover of what has been added so far (sat_cover_solve): every node is its
        representative or adjacent to it, no two representatives are adjacent.  More cover_add calls may follow.
        report.cover_sizes turns rep into cluster sizes."""
        if not getattr(self, "_cover_nodes", 0):
            self._check(self._lib.sat_cover_solve(self._ctx, None, None, None, None))     # the library's state error
        return _cover_solve(self, self._lib.sat_cover_solve, self._ctx, self._cover_nodes)

    def cover_end(self):
        """Free the cover accumulator (sat_cover_end)."""
        self._check(self._lib.sat_cover_end(self._ctx))
        self._cover_nodes = 0

    # ---- evaluation against a classification (sat_eval_*) -----------------------
    def set_eval_classes(self, node_class):
        """Install the classes of the nodes - the structures of the whole database in file order; int32, < 0 =
        unclassified - or remove them (None).  An upload drops them (sat_eval_classes)."""
        if node_class is None:
            self._check(self._lib.sat_eval_classes(self._ctx, 0, None))
            return
        cls = np.ascontiguousarray(node_class, dtype=np.int32).ravel()
        self._check(self._lib.sat_eval_classes(self._ctx, len(cls), cls.ctypes.data))

    def eval_rows(self, query_nodes, rocn=50):
        """Score the last search against the installed classes (sat_eval_rows): one record per query with the fields
        u2, t2, positives, negatives, n_used, query_class; report.eval_ratios turns one into (AUC, ROC-n).  The tables
        are made and reduced on the device: 32 bytes a query come back."""
        return _eval_rows(self, self._lib.sat_eval_rows, self._ctx, query_nodes, rocn)

    def eval_tables(self, query_nodes):
        """The raw tables eval_rows reduces (sat_eval_tables), for shards and tests: a list with one uint32[2, bins]
        array per query - positives, then negatives, by score; bins = 2 n1 (n1 - 1) + 1, bin = score + n1 (n1 - 1).
        Integer counts: the tables of the shards of a database add up to the whole database's."""
        nodes = _eval_nodes(self, query_nodes)
        bins = 2 * self._n1s.astype(np.int64) * (self._n1s - 1) + 1
        cuts = np.concatenate([[0], np.cumsum(2 * bins)])
        counts = np.zeros(int(cuts[-1]), np.uint32)
        self._check(self._lib.sat_eval_tables(self._ctx, nodes.ctypes.data, counts.ctypes.data, None))
        return [counts[cuts[q]:cuts[q + 1]].reshape(2, int(bins[q])) for q in range(len(nodes))]

    # ---- a query's SSEs profiled over its hits (sat_profile_rows) ----------------
    def profile_rows(self, max_pvalue, query_node=None):
        """Profile the last search, which must have run with lsoln (sat_profile_rows): (hits uint32[nq], a list with one
        uint32[n1, n1] array per query).  A row counts when its p-value is <= max_pvalue and its entry is not the query's
        own node (query_node[q], an index into the whole database; < 0 or None: the query is no entry); joint[i][k] is
        the counted rows whose map matches SSE i and SSE k, the diagonal those that match SSE i at all.  Counted on the
        device: 4 + 4 n1^2 bytes a query come back.  report.profile_core turns a matrix into the conserved core."""
        return _profile_rows(self, self._lib.sat_profile_rows, self._ctx, max_pvalue, query_node)

    def profile_rows_raw(self, max_pvalue, query_node, hits, joint, offset=None):
        """sat_profile_rows into the caller's uint32 arrays: query q's matrix at joint[offset[q]], packed in query order
        without offsets.  None passes a null pointer."""
        _profile_rows_raw(self, self._lib.sat_profile_rows, self._ctx, max_pvalue, query_node, hits, joint, offset)

    def debug_set_scores(self, scores):
        """Test hook (satabsearch_debug.h): overwrite the last search's device scores with int32[nq, N]."""
        sc = np.ascontiguousarray(scores, dtype=np.int32)
        if sc.size != getattr(self, "n_queries", 1) * self.n_entries:
            raise ValueError("scores must be [n_queries, n_entries]")
        self._check(self._lib.sat_debug_set_scores(self._ctx, sc.ctypes.data))

    def d2h_bytes(self):
        """Bytes this context's result calls have copied device -> host so far."""
        return int(self._lib.sat_stat_d2h_bytes(self._ctx))

    def last_launch_info(self):
        """Kernel instantiations and launch geometry of the last search."""
        return self._lib.sat_last_launch_info(self._ctx).decode()

    def sync(self):
        self._check(self._lib.sat_sync(self._ctx))

    def search_timed(self, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART, repeats=1):
        """HIP-event time of `repeats` back-to-back searches on the launch stream (ms)."""
        total, kern = C.c_double(0.0), C.c_double(0.0)
        self._check(self._lib.sat_search_timed(self._ctx, int(bool(lorder)), int(bool(lsoln)), int(maxstart),
                                               int(repeats), C.byref(total), C.byref(kern)))
        return total.value, kern.value

    def device_scores_ptr(self):
        return self._lib.sat_device_scores(self._ctx)

    def device_scores_tensor(self):
        """int32 torch tensor aliasing the context's device score buffer (for RCCL gathers)."""
        import torch

        class _Holder:
            pass

        h = _Holder()
        h.__cuda_array_interface__ = {
            "shape": (getattr(self, "n_queries", 1) * self.n_entries,), "typestr": "<i4", "data": (int(self.device_scores_ptr()), False),
            "version": 3, "strides": None,
        }
        return torch.as_tensor(h, device=f"cuda:{self.device}")


class MultiSearcher:
    """One search over several GPUs from one host thread (sat_multi_* of the C ABI): cost-balanced
    contiguous shards, the queries on every GPU, one gather of the shard rows to device 0."""

    def __init__(self, ndev=0, devices=None, seed=DEFAULT_SEED):
        self._lib = _native.device_lib()
        dev = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
        self._m = self._lib.sat_multi_create(int(ndev), dev.ctypes.data if dev is not None else None, int(seed))
        if not self._m:
            raise SatError(self._lib.sat_last_error().decode())
        self.ndev = int(self._lib.sat_multi_device_count(self._m))
        self.n_entries = 0
        self.n_queries = 0

    def close(self):
        if getattr(self, "_m", None):
            self._lib.sat_multi_destroy(self._m)
            self._m = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise SatError(f"[{rc}] {self._lib.sat_last_error().decode()}")

    @property
    def gather_kind(self):
        return self._lib.sat_multi_gather_kind(self._m).decode()

    def upload(self, db: StructSet):
        self._check(self._lib.sat_multi_db_upload_packed(self._m, len(db), db.orders.ctypes.data, db.cell_off.ctypes.data,
                                                         db.tab.ctypes.data, db.dist.ctypes.data))
        self.n_entries = len(db)
        self._orders = db.orders.copy()

    def shards(self):
        begin = np.zeros(self.ndev + 1, np.int32)
        self._check(self._lib.sat_multi_shards(self._m, begin.ctypes.data))
        return begin

    def set_queries(self, queries, first_query_ordinal=0):
        nq, pitch, n1s, tabs, dmats, types = _pack_queries(queries)
        self._check(self._lib.sat_multi_queries_set(self._m, nq, n1s.ctypes.data, tabs.ctypes.data, dmats.ctypes.data,
                                                    pitch, types.ctypes.data, int(first_query_ordinal)))
        self.n_queries = nq
        self._n1s = np.array(n1s, np.int32)
        self.n1max = int(n1s.max())

    def set_queries_from_db(self, entries, first_query_ordinal=0, sses=None):
        """Searcher.set_queries_from_db with entries[q] an index into the whole database (sat_multi_queries_from_db,
        with sses sat_multi_queries_from_db_sses): the shard that holds an entry builds its query, the other shards get
        it by a device-to-device copy."""
        idx = np.ascontiguousarray(entries, dtype=np.int32).ravel()
        if sses is None:
            self._check(self._lib.sat_multi_queries_from_db(self._m, len(idx), idx.ctypes.data if len(idx) else None,
                                                            int(first_query_ordinal)))
            n1s = self._orders[idx]
        else:
            begin, sse = _pack_sse_lists(sses, len(idx))
            self._check(self._lib.sat_multi_queries_from_db_sses(self._m, len(idx), idx.ctypes.data if len(idx) else None,
                                                                 begin.ctypes.data, sse.ctypes.data, int(first_query_ordinal)))
            n1s = np.where(np.diff(begin) > 0, np.diff(begin), self._orders[idx])
        self.n_queries = len(idx)
        self._n1s = np.array(n1s, np.int32)
        self.n1max = int(n1s.max())

    def debug_shard_queries(self, shard):
        """Test hook (satabsearch_debug.h): shard `shard`'s query batch as it lies on its device, uint8[bytes], and the
        bytes its context has been sent for query batches so far."""
        ctx = self._lib.sat_debug_multi_ctx(self._m, int(shard))
        if not ctx:
            raise SatError("no shard %d" % shard)
        n = self._lib.sat_debug_query_blob(ctx, None, 0)
        self._check(int(min(n, 0)))
        blob = np.empty(int(n), np.uint8)
        self._check(int(min(self._lib.sat_debug_query_blob(ctx, blob.ctypes.data, blob.size), 0)))
        return blob, int(self._lib.sat_stat_query_h2d_bytes(ctx))

    def search(self, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART):
        """Returns (scores int32[nq, N], ssemaps int32[nq, N, 111] or None, wall_ms), database order."""
        scores = np.empty((self.n_queries, self.n_entries), np.int32)
        ssemaps = np.full((self.n_queries, self.n_entries, MAXDIM), -1, np.int32) if lsoln else None
        ms = C.c_double(0.0)
        self._check(self._lib.sat_multi_search(self._m, int(bool(lorder)), int(bool(lsoln)), int(maxstart), scores.ctypes.data,
                                               ssemaps.ctypes.data if lsoln else None, C.byref(ms)))
        return scores, ssemaps, ms.value

    def search_matches(self, max_matches, lorder=True, maxstart=DEFAULT_MAXSTART, maps=True):
        """Searcher.search_matches over every shard, database order (wall_ms instead of kernel_ms)."""
        return _search_matches(self, self._lib.sat_multi_search_matches, self._m, max_matches, lorder, maxstart, maps)

    def search_pairs_matches(self, queries, entries, max_matches, lorder=True, maxstart=DEFAULT_MAXSTART, maps=True):
        """Searcher.search_pairs_matches with entries[p] an index into the whole database: every pair runs on the shard
        that holds its entry (wall_ms instead of kernel_ms)."""
        return _search_pairs_matches(self, self._lib.sat_multi_search_pairs_matches, self._m, queries, entries, max_matches,
                                     lorder, maxstart, maps)

    def search_pairs_polish(self, queries, entries, tops, lorder=True, maxstart=DEFAULT_MAXSTART):
        """Searcher.search_pairs_polish with entries[p] an index into the whole database (wall_ms instead of kernel_ms)."""
        return _search_pairs_polish(self, self._lib.sat_multi_search_pairs_polish, self._m, queries, entries, tops, lorder,
                                    maxstart)

    def search_refine_polish(self, k, candidates, refine_maxstart, tops, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART):
        """Searcher.search_refine_polish over every shard (sat_multi_search_refine_polish)."""
        ms = C.c_double(0.0)
        return _search_refine_polish(self, lambda h, m, f, b: self._lib.sat_multi_search_refine_polish(
            self._m, int(bool(lorder)), int(bool(lsoln)), int(maxstart), int(candidates), int(refine_maxstart), int(tops),
            int(k), h, m, f, b, C.byref(ms)), k, candidates, refine_maxstart, lsoln)

    def set_polish_all(self, tops):
        """Searcher.set_polish_all on every shard (sat_multi_polish_all_set): search, search_topk, search_cutoff and
        search_fit then work on polished rows, exactly those of one searcher holding the whole database."""
        self._check(self._lib.sat_multi_polish_all_set(self._m, int(tops)))

    def search_topk(self, k, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART):
        k = min(int(k), self.n_entries)
        hits = np.zeros((self.n_queries, k), _HIT_DTYPE)
        maps = np.full((self.n_queries, k, MAXDIM), -1, np.int32) if lsoln else None
        ms = C.c_double(0.0)
        self._check(self._lib.sat_multi_search_topk(self._m, int(bool(lorder)), int(bool(lsoln)), int(maxstart), k,
                                                    hits.ctypes.data, maps.ctypes.data if lsoln else None, C.byref(ms)))
        return hits, maps, ms.value

    def search_refine(self, k, candidates, refine_maxstart, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART):
        """Searcher.search_refine over every shard (sat_multi_search_refine); hits name entries of the whole database."""
        ms = C.c_double(0.0)
        return _search_refine(self, lambda h, m, f: self._lib.sat_multi_search_refine(
            self._m, int(bool(lorder)), int(bool(lsoln)), int(maxstart), int(candidates), int(refine_maxstart), int(k),
            h, m, f, C.byref(ms), None), k, candidates, refine_maxstart, lsoln)

    def search_cutoff(self, max_pvalue, k=None, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART):
        """Search every shard, then Searcher.hits_cutoff over the whole database (sat_multi_search_cutoff; a short
        buffer is refilled by sat_multi_hits_cutoff, without a new search): (rows, maps or None, wall_ms), entries
        indexed in the whole database."""
        ms = C.c_double(0.0)
        rows, maps = _hits_cutoff(
            self, self.n_queries, lsoln,
            lambda c, cap, h, m: self._lib.sat_multi_search_cutoff(self._m, int(bool(lorder)), int(bool(lsoln)), int(maxstart),
                                                                   float(max_pvalue), int(k or 0), c, cap, h, m, C.byref(ms)),
            lambda c, cap, h, m: self._lib.sat_multi_hits_cutoff(self._m, float(max_pvalue), int(k or 0), c, cap, h, m))
        return rows, maps, ms.value

    def hits_cutoff(self, max_pvalue, k=None, lsoln=False):
        """The rows of search_cutoff selected again from every shard's last search (sat_multi_hits_cutoff)."""
        call = lambda c, cap, h, m: self._lib.sat_multi_hits_cutoff(self._m, float(max_pvalue), int(k or 0), c, cap, h, m)
        rows, maps = _hits_cutoff(self, self.n_queries, lsoln, call, call)
        return (rows, maps) if lsoln else rows

    def baseline_keep(self):
        """Searcher.baseline_keep on every shard (sat_multi_baseline_keep)."""
        self._check(self._lib.sat_multi_baseline_keep(self._m))

    def baseline_drop(self):
        self._check(self._lib.sat_multi_baseline_drop(self._m))

    def baseline_results(self):
        """Searcher.baseline_results over the whole database (sat_multi_baseline_results)."""
        return _baseline_results(self, self._lib.sat_multi_baseline_results, self._m, self.n_queries)

    def reorder_hits(self, max_pvalue, min_base_pvalue=0.0, kinds=KIND_CIRCULAR | KIND_PERMUTED, k=None, lsoln=False):
        """Searcher.reorder_hits over every shard, entries indexed in the whole database: exactly what one context
        holding the whole database returns (sat_multi_reorder_hits)."""
        return _reorder_hits(self, self._lib.sat_multi_reorder_hits, self._m, self.n_queries, max_pvalue, min_base_pvalue,
                             kinds, k, lsoln)

    def search_reordered(self, maxstart=DEFAULT_MAXSTART, censor=None):
        """Searcher.search_reordered on every shard (sat_multi_search_reordered).  Returns wall_ms."""
        ms = C.c_double(0.0)
        self._check(self._lib.sat_multi_search_reordered(self._m, int(maxstart), -1.0 if censor is None else float(censor), C.byref(ms)))
        return ms.value

    def score_histogram(self):
        """Searcher.score_histogram summed over every shard's last search (sat_multi_score_histogram)."""
        return _score_histogram(self, self._lib.sat_multi_score_histogram, self._m, self.n_queries)

    def search_fit(self, censor=0.0, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART):
        """Search every shard without a gather, sum the shards' histograms, fit once and install the fit on every shard
        (sat_multi_search_fit): (fits as Searcher.fit_statistics, wall_ms).  hits_cutoff then returns rows with the
        fitted statistics, without a new search."""
        fits = np.zeros(self.n_queries, _FIT_DTYPE)
        ms = C.c_double(0.0)
        self._check(self._lib.sat_multi_search_fit(self._m, int(bool(lorder)), int(bool(lsoln)), int(maxstart), float(censor),
                                                   fits.ctypes.data, C.byref(ms)))
        return fits, ms.value

    def search_only(self, lorder=True, lsoln=False, maxstart=DEFAULT_MAXSTART):
        """Search every shard and wait; nothing is gathered or copied (sat_multi_search_only).  hits_cutoff,
        score_histogram and cluster_add then work on it.  Returns wall_ms."""
        ms = C.c_double(0.0)
        self._check(self._lib.sat_multi_search_only(self._m, int(bool(lorder)), int(bool(lsoln)), int(maxstart), C.byref(ms)))
        return ms.value

    def search_exact(self, lorder=True, maxstart=DEFAULT_MAXSTART, max_nodes=_native.EXACT_DEFAULT_NODES):
        """Searcher.search_exact on every shard; the rows stay on the shards (sat_multi_search_exact).  Returns wall_ms;
        exact_results() brings the rows back."""
        ms = C.c_double(0.0)
        self._check(self._lib.sat_multi_search_exact(self._m, int(bool(lorder)), int(maxstart), int(max_nodes), C.byref(ms)))
        return ms.value

    def exact_results(self, maps=True):
        """The whole database's rows of the last exact search in file order (sat_multi_exact_results): (scores int32[nq, N],
        ssemaps int32[nq, N, 111] or None, base_scores int32[nq, N], unproven bool[nq, N], nodes uint32[nq, N]) - what one
        Searcher holding the whole database returns."""
        shape = (self.n_queries, self.n_entries)
        scores, base = np.empty(shape, np.int32), np.empty(shape, np.int32)
        flag, nodes = np.empty(shape, np.uint8), np.empty(shape, np.uint32)
        ssemaps = np.full(shape + (MAXDIM,), -1, np.int32) if maps else None
        self._check(self._lib.sat_multi_exact_results(self._m, scores.ctypes.data, ssemaps.ctypes.data if maps else None,
                                                      base.ctypes.data, flag.ctypes.data, nodes.ctypes.data))
        return scores, ssemaps, base, flag.astype(bool), nodes

    def exact_stats(self):
        """Searcher.exact_stats summed over the shards (sat_multi_exact_stats)."""
        stats = np.zeros(self.n_queries, _EXACT_STAT_DTYPE)
        self._check(self._lib.sat_multi_exact_stats(self._m, stats.ctypes.data))
        return stats

    def cluster_begin(self):
        """Searcher.cluster_begin on every shard, over the whole database's nodes (sat_multi_cluster_begin)."""
        self._check(self._lib.sat_multi_cluster_begin(self._m))
        self._cluster_levels = 0

    def cluster_add(self, max_pvalue, query_nodes):
        """Searcher.cluster_add on every shard: each adds the edges that end at its own entries."""
        _cluster_add(self, self._lib.sat_multi_cluster_add, self._m, max_pvalue, query_nodes)

    def cluster_labels(self):
        """Searcher.cluster_labels of the whole database: the shards' labels joined, degrees and edges summed
        (sat_multi_cluster_labels) - exactly what one searcher holding the whole database returns."""
        return _cluster_labels(self, self._lib.sat_multi_cluster_labels, self._m, self.n_entries)

    def reach_begin(self, seeds=None):
        """Searcher.reach_begin on every shard, over the whole database's nodes (sat_multi_reach_begin)."""
        _reach_begin(self, lambda c, p: self._lib.sat_multi_reach_begin(self._m, c, p), seeds)

    def reach_add(self, depth, max_pvalue, query_nodes):
        """Searcher.reach_add on every shard: each adds the steps that end at its own entries."""
        _reach_add(self, self._lib.sat_multi_reach_add, self._m, depth, max_pvalue, query_nodes)

    def reach_frontier(self, depth, cap=None):
        """Searcher.reach_frontier of the whole database: the shards' keys joined on the host (sat_multi_reach_frontier)."""
        return _reach_frontier(self, self._lib.sat_multi_reach_frontier, self._m, depth, cap)

    def reach_rows(self, cap=None):
        """Searcher.reach_rows of the whole database: the shards' keys joined by minimum, their supports summed
        (sat_multi_reach_rows) - exactly what one searcher holding the whole database returns."""
        return _reach_rows(self, self._lib.sat_multi_reach_rows, self._m, cap)

    def reach_end(self):
        """Free every shard's accumulator (sat_multi_reach_end)."""
        self._check(self._lib.sat_multi_reach_end(self._m))

    def search_reach(self, seeds, max_pvalue, max_depth=_native.REACH_MAX_DEPTH, max_queries=None, batch=256, censor=None,
                     first_query_ordinal=0, cap=None, lorder=True, maxstart=DEFAULT_MAXSTART):
        """Searcher.search_reach over every shard (sat_multi_search_reach); search_ms and pass_ms are wall clock."""
        out = _search_reach(self, self._lib.sat_multi_search_reach, self._m, self.n_entries, seeds, max_pvalue, max_depth,
                            max_queries, batch, censor, first_query_ordinal, cap, lorder, maxstart)
        _reach_last_batch(self, self._lib.sat_multi_reach_frontier, self._m, out, batch, lambda v: self._orders[v])
        return out

    def cover_begin(self):
        """Searcher.cover_begin on every shard, over the whole database's nodes (sat_multi_cover_begin)."""
        self._check(self._lib.sat_multi_cover_begin(self._m))

    def cover_add(self, max_pvalue, query_nodes):
        """Searcher.cover_add on every shard: each adds the rows of its own entries to its own matrix."""
        _cluster_add(self, self._lib.sat_multi_cover_add, self._m, max_pvalue, query_nodes)

    def cover_solve(self):
        """Searcher.cover_solve of the whole database: the shards' matrices ORed onto the first shard's device and solved
        there (sat_multi_cover_solve) - exactly what one searcher holding the whole database returns."""
        return _cover_solve(self, self._lib.sat_multi_cover_solve, self._m, self.n_entries)

    def cluster_begin_levels(self, pvalues):
        """Searcher.cluster_begin_levels on every shard, over the whole database's nodes (sat_multi_cluster_begin_levels)."""
        count, cuts = _cluster_levels(pvalues)
        self._check(self._lib.sat_multi_cluster_begin_levels(self._m, count, cuts.ctypes.data))
        self._cluster_levels = count

    def cluster_add_levels(self, query_nodes):
        """Searcher.cluster_add_levels on every shard: each adds the edges that end at its own entries."""
        _cluster_add_levels(self, self._lib.sat_multi_cluster_add_levels, self._m, query_nodes)

    def cluster_labels_levels(self):
        """Searcher.cluster_labels_levels of the whole database: per level the shards' labels joined, degrees and edges
        summed (sat_multi_cluster_labels_levels) - exactly what one searcher holding the whole database returns."""
        return _cluster_labels_levels(self, self._lib.sat_multi_cluster_labels_levels, self._m, getattr(self, "_cluster_levels", 0),
                                      self.n_entries)

    def set_eval_classes(self, node_class):
        """Searcher.set_eval_classes on every shard, over the whole database's nodes (sat_multi_eval_classes)."""
        if node_class is None:
            self._check(self._lib.sat_multi_eval_classes(self._m, None))
            return
        cls = np.ascontiguousarray(node_class, dtype=np.int32).ravel()
        if len(cls) != self.n_entries:
            raise ValueError("one class per structure of the database is needed")
        self._check(self._lib.sat_multi_eval_classes(self._m, cls.ctypes.data))

    def eval_rows(self, query_nodes, rocn=50):
        """Searcher.eval_rows of the whole database: each shard makes the tables of its own entries, the host sums and
        reduces them (sat_multi_eval_rows) - exactly what one searcher holding the whole database returns."""
        return _eval_rows(self, self._lib.sat_multi_eval_rows, self._m, query_nodes, rocn)

    def profile_rows(self, max_pvalue, query_node=None):
        """Searcher.profile_rows of the whole database: each shard profiles its own entries and the host adds the
        matrices (sat_multi_profile_rows) - exactly what one searcher holding the whole database returns."""
        return _profile_rows(self, self._lib.sat_multi_profile_rows, self._m, max_pvalue, query_node)

    def profile_rows_raw(self, max_pvalue, query_node, hits, joint, offset=None):
        """Searcher.profile_rows_raw over every shard."""
        _profile_rows_raw(self, self._lib.sat_multi_profile_rows, self._m, max_pvalue, query_node, hits, joint, offset)

    def set_statistics(self, fits):
        """Searcher.set_statistics on every shard (sat_multi_stats_set)."""
        rec = None if fits is None else _fit_records(fits, self.n_queries)
        self._check(self._lib.sat_multi_stats_set(self._m, rec.ctypes.data if rec is not None else None))

    def d2h_bytes(self):
        return int(self._lib.sat_multi_stat_d2h_bytes(self._m))
