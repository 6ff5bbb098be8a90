"""The selection passes at block and wave edges and across query chunks (-m gpu): best-k (sat_topk, sat_topk_hits,
stage 1 of the refine), the p-value cutoff (count, compact, finish), the score histogram and sat_cluster_add, byte for
byte against tests/select_lib.py - plain numpy and the host library, never the device library's own rows.

Scores are planted with sat_debug_set_scores on prefixes of one unsorted synthetic database: 1023, 1024 and 1025 entries
(one cutoff block of 1024 rows less one, exactly, plus one) and 8191, 8192, 8193 (the same for a histogram block of 8192
rows).  SAT_EXP_SELECT_KEYS (satabsearch_debug.h) cuts the query list of every pass into chunks at these small shapes;
no result may depend on it."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd.search import _FIT_DTYPE
import select_lib
from select_lib import BINS, MAXDIM, Reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
SMALL_DB = "tableauxdistmatrixdb.small.ascii"
N_ALL = 8193
CUTOFF_SHAPES = (1023, 1024, 1025)
HIST_SHAPES = (8191, 8192, 8193)
N1S = (4, 7, 9, 12, 15, 17, 20)
NQ = len(N1S)
HIT = 32                                                   # sizeof(sat_hit)
# the queries as nodes of the clustering: 3 and 4 share a node; query 1 (every row qualifies) meets its own node in row
# 100 and query 2 (rows = 63 mod 64) in row 255 - self rows, which are no edges
QUERY_NODES = (5, 100, 255, 700, 700, 2, 9)
EDGE_PATTERNS = ("none", "all", "lane 63", "lane 0", "last", "block edge", "waves")
# for the chunked runs: queries 2 and 3 qualify nowhere - an empty query between non-empty ones, a whole chunk empty
CHUNK_PATTERNS = ("all", "lane 63", "none", "none", "last", "block edge", "waves")
CHUNK_FITS = (None, (0.40, 0.36), None, None, (0.35, 0.30), None, (0.45, 0.40))
CHUNK_N = 1025


# ---------------------------------------------------------------- the database, the queries, the planted scores
@functools.lru_cache(None)
def database():
    """8 193 entries of 4..12 SSEs, unsorted; entries 56..71 and 1016..1031 share one order, so that rows planted with
    one norm2 carry one score in a run across a wave edge (63 | 64) and across the block edge (1023 | 1024)"""
    orders = np.random.default_rng(7).integers(4, 13, N_ALL).astype(np.int32)
    orders[56:72] = 9
    orders[1016:1032] = 9
    return sat.synth.make_db(N_ALL, orders=orders, sort=False)


@functools.lru_cache(None)
def queries():
    return [sat.synth.make_query(n1, seed=200 + n1) for n1 in N1S]


def totals(n):
    """n1 + n2 of every (query, entry) of the prefix of n entries, int64[NQ, n]"""
    return np.asarray(N1S, np.int64)[:, None] + database().orders[:n].astype(np.int64)[None, :]


def masks(n, patterns):
    """bool[NQ, n]: the rows of each query that qualify"""
    e = np.arange(n)
    lane, wave = e % 64, (e % 1024) // 64
    known = {
        "none": np.zeros(n, bool),
        "all": np.ones(n, bool),
        "lane 63": lane == 63,
        "lane 0": lane == 0,
        "last": e == n - 1,
        "block edge": (e == 1023) | (e == 1024),
        "waves": (lane % 4 == 0) & (lane // 4 < wave),        # wave w of every block: its lanes 0, 4, .., 4 (w - 1)
    }
    return np.stack([known[p] for p in patterns])


def edge_scores(n):
    """norm2 == 10 on the qualifying rows, 0 on the others"""
    return np.where(masks(n, EDGE_PATTERNS), 5 * totals(n), 0).astype(np.int32)


@functools.lru_cache(None)
def edge_cutoff():
    """a p-value strictly between the built-in statistics' p at norm2 == 10 and at norm2 == 0"""
    p10, p0 = select_lib.builtin_stats(10.0)[1], select_lib.builtin_stats(0.0)[1]
    assert 0.0 < p10 < p0 <= 1.0
    p = (p10 + p0) / 2
    assert p10 < p < p0
    return p


def histogram_scores(n):
    """ordinary scores, negatives, and each entry's first overflowing score and the one below it, through every block;
    rows 8190, 8191 and 8192 - the end of the first block, the whole second one - negative for the even queries, in
    the overflow bin for the odd ones"""
    rng = np.random.default_rng(11)
    tot = totals(n)
    sc = rng.integers(0, 40, (NQ, n))
    sc[:, ::7] = -rng.integers(1, 9, sc[:, ::7].shape)
    first_over = -(-(BINS - 1) * tot // 512)
    sc[:, 5::13] = first_over[:, 5::13]
    sc[:, 6::13] = first_over[:, 6::13] - 1
    for r in (8190, 8191, 8192):
        if r < n:
            sc[0::2, r] = -3
            sc[1::2, r] = first_over[1::2, r]
    return sc.astype(np.int32)


def table_scores(n):
    """every entry whose n1 + n2 is a multiple of 4 takes one of the scores that sit on an edge of the built-in table's
    index (int)norm2: norm2 exactly -2, just above -1, -0.5, just below +1, exactly +1 (truncation toward zero sends
    the three in the middle to index 0), +-128 and +-130 (the clamp to -128..127) and +-(2^30 - 1), the ends of the
    domain the sort keys hold"""
    rng = np.random.default_rng(13)
    tot = totals(n)
    sc = rng.integers(0, 3 * tot)
    top = (1 << 30) - 1
    kinds = [-tot, -tot // 2 + 1, -tot // 4, tot // 2 - 1, tot // 2, 65 * tot, -65 * tot, 64 * tot, -64 * tot,
             np.full_like(tot, top), np.full_like(tot, -top)]
    for q in range(NQ):
        at = np.nonzero(tot[q] % 4 == 0)[0]
        for i, kind in enumerate(kinds):
            sc[q][at[i::len(kinds)]] = kind[q][at[i::len(kinds)]]
    assert (np.abs(sc) < (1 << 30)).all()
    return sc.astype(np.int32)


def chunk_scores():
    """norm2 == 10 on the qualifying rows; the others spread over [0, 1), so that the histogram has bins to fit"""
    tot = totals(CHUNK_N)
    low = np.random.default_rng(17).integers(0, (tot + 1) // 2)
    assert (2 * low < tot).all()
    return np.where(masks(CHUNK_N, CHUNK_PATTERNS), 5 * tot, low).astype(np.int32)


def chunk_fits():
    fits = np.zeros(NQ, _FIT_DTYPE)
    for q, f in enumerate(CHUNK_FITS):
        if f:
            fits[q]["a"], fits[q]["b"], fits[q]["fitted"] = f[0], f[1], 1
    return fits


# ---------------------------------------------------------------- the searchers and the references, made once
@pytest.fixture(scope="module")
def shape():
    """n -> (a searcher holding the first n entries and the queries, after search(True, True, 1); the maps it left)"""
    assert sat.device_count() >= 1, "GPU tests need a HIP device (no CPU path exists)"
    made = {}

    def get(n):
        if n not in made:
            s = sat.Searcher(0)
            made[n] = [s, None]
            s.upload(database().subset(np.arange(n)))
            s.set_queries(queries())
            maps = s.search(True, True, 1)[1]
            made[n][1] = maps if n in CUTOFF_SHAPES else None            # (the histogram reads no maps)
        return made[n]

    yield get
    for s, _ in made.values():
        s.close()


_references = {}


def reference(what, n, maps, scores, fits=None):
    """the Reference of a planted set, computed once and shared"""
    if (what, n) not in _references:
        _references[what, n] = Reference(scores, N1S, database().orders[:n], fits, maps)
    return _references[what, n]


def same_rows(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s rows, want %s" % (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), "%s: rows differ first at %s" % (
        what, np.argwhere(got != want)[:4].tolist())


def same_cutoff(got, got_maps, want, want_maps, what):
    assert [len(g) for g in got] == [len(w) for w in want], "%s: counts" % what
    for q in range(NQ):
        same_rows(got[q], want[q], "%s, query %d" % (what, q))
        if want_maps is not None:
            assert got_maps[q].dtype == np.int32 and got_maps[q].shape == (len(want[q]), MAXDIM)
            assert np.array_equal(got_maps[q], want_maps[q]), "%s, query %d: maps differ" % (what, q)


def same_clusters(got, want, what):
    labels, degrees, edges = got
    assert labels.dtype == np.int32 and degrees.dtype == np.int32
    assert np.array_equal(labels, want[0]), "%s: labels differ at %s" % (what, np.nonzero(labels != want[0])[0][:8])
    assert np.array_equal(degrees, want[1]), "%s: degrees differ at %s" % (what, np.nonzero(degrees != want[1])[0][:8])
    assert edges == want[2], "%s: %d edges, expected %d" % (what, edges, want[2])


# ---------------------------------------------------------------- 1. the planted sets are what they claim to be
@pytest.mark.parametrize("n", CUTOFF_SHAPES)
def test_planted_edges(shape, n):
    s, maps = shape(n)
    m, sc, orders = masks(n, EDGE_PATTERNS), edge_scores(n), database().orders
    ref = reference("edges", n, maps, sc)
    p = edge_cutoff()
    first_block = np.zeros(1024, bool)
    first_block[:min(n, 1024)] = m[6][:1024]
    assert first_block.reshape(16, 64).sum(axis=1).tolist() == list(range(16))      # wave w holds w qualifying rows
    assert m[2][63] and m[3][0] and m[3][64] and m[4][n - 1] and m[4].sum() == 1
    assert m[5].sum() == (0, 1, 2)[n - 1023] and not m[0].any() and m[1].all()
    for q in range(NQ):
        rows = ref.rows(q)
        assert (rows["norm2"][rows["score"] > 0] == 10.0).all() and (rows["norm2"][rows["score"] == 0] == 0.0).all()
        assert np.array_equal(np.sort(rows["entry"][rows["pvalue"] <= p]), np.nonzero(m[q])[0])     # P separates them
    # equal scores in a run across a wave edge and across the block edge: the tie order is decided there
    assert len(set(orders[56:72])) == 1 and len(set(sc[1][56:72])) == 1 and len(set(orders[1016:1032])) == 1
    if n == 1025:
        assert sc[5][1023] == sc[5][1024] > 0 and sc[1][1023] == sc[1][1024]
    got, _ = s.results()
    s.debug_set_scores(sc)
    assert np.array_equal(s.results()[0], sc) and got.shape == sc.shape


# ---------------------------------------------------------------- 2. best-k
@pytest.mark.parametrize("n", CUTOFF_SHAPES)
def test_best_k_at_the_block_edge(shape, n):
    s, maps = shape(n)
    sc = edge_scores(n)
    ref = reference("edges", n, maps, sc)
    s.debug_set_scores(sc)
    for k in (1, n - 1, n, n + 5):
        got, got_maps = s.topk_hits(k, lsoln=True)
        want, want_maps = ref.topk(k)
        same_rows(got, want, "k = %d" % k)
        assert np.array_equal(got_maps, want_maps), "k = %d: maps differ" % k
    for k in (1, n + 5):                                                # sat_topk: one query, a chunk of its own
        entry, score = s.topk(k, query=NQ - 1)
        want = ref.rows(NQ - 1)[:k]
        assert np.array_equal(entry, want["entry"]) and np.array_equal(score, want["score"]) and len(entry) == min(k, n)


# ---------------------------------------------------------------- 3. the p-value cutoff
@pytest.mark.parametrize("n", CUTOFF_SHAPES)
def test_cutoff_at_the_block_edge(shape, n):
    s, maps = shape(n)
    sc = edge_scores(n)
    ref = reference("edges", n, maps, sc)
    s.debug_set_scores(sc)
    p = edge_cutoff()
    counts = masks(n, EDGE_PATTERNS).sum(axis=1)
    for k in (None, 1, 3):
        got, got_maps = s.hits_cutoff(p, k=k, lsoln=True)
        want, want_maps, want_counts = ref.cutoff(p, k)
        assert list(want_counts) == [min(int(c), k) if k else int(c) for c in counts]
        same_cutoff(got, got_maps, want, want_maps, "P, k = %s" % k)
    for p_all in (0.0, 1.0):
        got, got_maps = s.hits_cutoff(p_all, lsoln=True)
        want, want_maps, want_counts = ref.cutoff(p_all)
        assert list(want_counts) == [0 if p_all == 0.0 else n] * NQ
        same_cutoff(got, got_maps, want, want_maps, "P = %g" % p_all)


# ---------------------------------------------------------------- 4. the clustering
@pytest.mark.parametrize("n", CUTOFF_SHAPES)
def test_cluster_add_at_the_block_edge(shape, n):
    s, maps = shape(n)
    sc = edge_scores(n)
    ref = reference("edges", n, maps, sc)
    s.debug_set_scores(sc)
    p = edge_cutoff()
    want = ref.components(p, QUERY_NODES)
    m = masks(n, EDGE_PATTERNS)
    assert m[1][100] and m[2][255]                                       # the self rows qualify
    assert want[2] == int(m.sum()) - 2 and want[1].sum() == 2 * want[2] and want[2] > 2 ** 10
    s.cluster_begin()
    s.cluster_add(p, QUERY_NODES)
    same_clusters(s.cluster_labels(), want, "P")
    for p_all in (0.0, 1.0):
        s.cluster_begin()
        s.cluster_add(p_all, QUERY_NODES)
        same_clusters(s.cluster_labels(), ref.components(p_all, QUERY_NODES), "P = %g" % p_all)
    s.cluster_end()


# ---------------------------------------------------------------- 5. the histogram
@pytest.mark.parametrize("n", HIST_SHAPES)
def test_histogram_at_the_block_edge(shape, n):
    s, _ = shape(n)
    sc = histogram_scores(n)
    s.debug_set_scores(sc)
    counts, below = s.score_histogram()
    want, want_below = select_lib.host_histogram(sc, N1S, database().orders[:n])
    assert counts.dtype == want.dtype and below.dtype == want_below.dtype
    assert np.array_equal(below, want_below), "below: %s, want %s" % (below, want_below)
    assert np.array_equal(counts, want), "counts differ at %s" % np.argwhere(counts != want)[:6].tolist()
    assert (want.sum(axis=1) + want_below == n).all() and (want_below > n // 10).all() and (want[:, BINS - 1] > n // 14).all()
    if n == N_ALL:                                                      # the second block is row 8192 alone
        head, head_below = select_lib.host_histogram(sc[:, :8192], N1S, database().orders[:8192])
        assert list(want_below - head_below) == [1, 0] * 3 + [1]
        assert list(want[:, BINS - 1] - head[:, BINS - 1]) == [0, 1] * 3 + [0]


# ---------------------------------------------------------------- 6. the index of the built-in table
def test_table_index_truncation_and_clamp(shape):
    n = CHUNK_N
    s, maps = shape(n)
    sc = table_scores(n)
    ref = reference("table", n, maps, sc)
    s.debug_set_scores(sc)
    allrows = np.concatenate([ref.rows(q) for q in range(NQ)])
    x = np.clip(np.trunc(allrows["norm2"]), -128, 127)
    assert {-128.0, -2.0, 0.0, 1.0, 127.0} <= set(x.tolist())
    assert (allrows["norm2"] < -128).any() and (allrows["norm2"] > 128).any() and (allrows["norm2"] == -0.5).any()
    assert ((allrows["norm2"] > -1) & (allrows["norm2"] < -0.5)).any() and ((allrows["norm2"] > 0.5) & (allrows["norm2"] < 1)).any()
    inside = (allrows["norm2"] > -1) & (allrows["norm2"] < 1)             # one index, 0: one p-value
    assert len(set(allrows["pvalue"][inside].tolist())) == 1
    got, got_maps = s.topk_hits(n, lsoln=True)
    want, want_maps = ref.topk(n)
    same_rows(got, want, "every row")
    assert np.array_equal(got_maps, want_maps)
    distinct = np.unique(allrows["pvalue"])
    assert len(distinct) >= 6
    for lo, hi in zip(distinct, distinct[1:]):
        p = float((lo + hi) / 2)
        assert lo <= p <= hi
        want, _, _ = ref.cutoff(p)
        same_cutoff(s.hits_cutoff(p), None, want, None, "P = %r" % p)
    got, got_maps = s.hits_cutoff(float(distinct[1]), lsoln=True)
    want, want_maps, _ = ref.cutoff(float(distinct[1]))
    same_cutoff(got, got_maps, want, want_maps, "P = %r with maps" % distinct[1])


# ---------------------------------------------------------------- 7. the same results under every chunking
def chunk_reference(maps):
    sc, fits = chunk_scores(), chunk_fits()
    ref = reference("chunks", CHUNK_N, maps, sc, fits)
    qual = masks(CHUNK_N, CHUNK_PATTERNS)
    inside, outside = [], []
    for q in range(NQ):
        rows = ref.rows(q)
        inside.append(rows["pvalue"][qual[q][rows["entry"]]])
        outside.append(rows["pvalue"][~qual[q][rows["entry"]]])
    hi, lo = float(np.concatenate(inside).max()), float(np.concatenate(outside).min())
    assert hi < lo                                                       # fitted or not, norm2 == 10 is under every other row
    p = (hi + lo) / 2
    assert hi < p < lo
    return sc, fits, ref, p


@pytest.mark.parametrize("keys", [None, 1, 2 * CHUNK_N, 3 * CHUNK_N + 5, 4 * CHUNK_N, 7 * CHUNK_N, 100 * CHUNK_N])
def test_chunking_does_not_change_results(shape, monkeypatch, keys):
    """keys -> queries per chunk of best-k / of the cutoff passes: unset 7 / 7, 1: 1 / 1, 2n: 2 / 1, 3n + 5: 3 / 1,
    4n: 4 / 2 (queries 2 and 3 are a chunk without a row), 7n: 7 / 3, 100n: 7 / 7"""
    n = CHUNK_N
    real_maps = shape(n)[1]
    sc, fits, ref, p = chunk_reference(real_maps)
    assert [int(c) for c in ref.cutoff(p)[2]] == [n, 16, 0, 0, 1, 2, 120]
    if keys is None:
        monkeypatch.delenv("SAT_EXP_SELECT_KEYS", raising=False)
    else:
        monkeypatch.setenv("SAT_EXP_SELECT_KEYS", str(keys))
    with sat.Searcher(0) as s:                                          # the override is read when a context is created
        s.upload(database().subset(np.arange(n)))
        s.set_queries(queries())
        real, maps, _ = s.search(True, True, 1)
        assert np.array_equal(maps, real_maps)
        s.debug_set_scores(sc)
        s.set_statistics(fits)

        def moved(call):
            before = s.d2h_bytes()
            out = call()
            return out, s.d2h_bytes() - before

        for k in (3, n):
            (got, got_maps), nbytes = moved(lambda: s.topk_hits(k, lsoln=True))
            want, want_maps = ref.topk(k)
            same_rows(got, want, "best %d" % k)
            assert np.array_equal(got_maps, want_maps) and nbytes == NQ * k * (HIT + 4 * MAXDIM)
        for k in (None, 3):
            want, want_maps, counts = ref.cutoff(p, k)
            s._cutoff_cap = int(counts.sum())                            # one call: the rows fit
            (got, got_maps), nbytes = moved(lambda: s.hits_cutoff(p, k=k, lsoln=True))
            same_cutoff(got, got_maps, want, want_maps, "cutoff, k = %s" % k)
            assert nbytes == 4 * NQ + int(counts.sum()) * (HIT + 4 * MAXDIM)
        s._cutoff_cap = int(ref.cutoff(p)[2].sum())
        (got, nbytes) = moved(lambda: s.hits_cutoff(p))
        same_cutoff(got, None, ref.cutoff(p)[0], None, "cutoff without maps")
        assert nbytes == 4 * NQ + int(ref.cutoff(p)[2].sum()) * HIT
        s.cluster_begin()
        _, nbytes = moved(lambda: s.cluster_add(p, QUERY_NODES))
        assert nbytes == 0
        got, nbytes = moved(s.cluster_labels)
        same_clusters(got, ref.components(p, QUERY_NODES), "clusters")
        assert nbytes == 8 * n + 8
        s.cluster_end()
        (counts, below), nbytes = moved(s.score_histogram)
        want, want_below = ref.histogram()
        assert np.array_equal(counts, want) and np.array_equal(below, want_below) and nbytes == NQ * (BINS + 1) * 4
        got, nbytes = moved(lambda: s.fit_statistics(0.01))
        new_fits = ref.fit(0.01)
        assert got.tobytes() == new_fits.tobytes() and nbytes == NQ * (BINS + 1) * 4
        assert 0 < new_fits["fitted"].sum() < NQ                          # fitted and unfitted queries again
        refit = reference("chunks refitted", n, real_maps, sc, new_fits)
        same_rows(s.topk_hits(5), refit.topk(5)[0], "best 5 under the new fit")
        # stage 1 of the refine ranks through the same chunks: 40 candidates of a search at 1 restart, again at 8
        k, c = 10, 40
        (hits, hit_maps, first), nbytes = moved(lambda: s.search_refine(k, c, 8, True, True, 1))
        assert nbytes == NQ * k * (HIT + 4 + 4 * MAXDIM) + NQ * c * 4
        again, again_maps, _ = s.search(True, True, 8)
        stage1 = reference("real, 1 restart", n, real_maps, real)
        stage2 = Reference(again, N1S, database().orders[:n], None, again_maps)
        for q in range(NQ):
            rows = stage2.rows(q)
            rows = rows[np.isin(rows["entry"], stage1.rows(q)["entry"][:c])][:k]
            same_rows(hits[q], rows, "refine, query %d" % q)
            assert np.array_equal(first[q], real[q][rows["entry"]])
            assert np.array_equal(hit_maps[q], stage2.row_maps(q, rows["entry"]))


def test_three_shards_chunked_equal_one_context(shape, monkeypatch):
    n, r = CHUNK_N, 8
    shape(n)                                                             # (made outside the override)
    db = database().subset(np.arange(n))
    monkeypatch.delenv("SAT_EXP_SELECT_KEYS", raising=False)
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries())
        real, maps, _ = s.search(True, True, r)
        ref = Reference(real, N1S, db.orders, None, maps)
        distinct = np.unique(np.concatenate([ref.rows(q)["pvalue"] for q in range(NQ)]))
        p = float((distinct[len(distinct) // 2 - 1] + distinct[len(distinct) // 2]) / 2)
        want = {}
        for k in (None, 3):
            got, got_maps = s.hits_cutoff(p, k=k, lsoln=True)
            same_cutoff(got, got_maps, *ref.cutoff(p, k)[:2], "one context, k = %s" % k)
            want[k] = ([g.tobytes() for g in got], [g.tobytes() for g in got_maps])
        assert 0 < sum(len(g) for g in got) and len(ref.cutoff(p)[0][0]) < n
        s.cluster_begin()
        s.cluster_add(p, QUERY_NODES)
        clusters = s.cluster_labels()
        same_clusters(clusters, ref.components(p, QUERY_NODES), "one context")
        fits = s.fit_statistics(0.01)
        assert fits.tobytes() == ref.fit(0.01).tobytes() and fits["fitted"].any()
        fitted = Reference(real, N1S, db.orders, fits, maps)
        pv = np.unique(fitted.rows(0)["pvalue"])
        p_fit = float((pv[len(pv) // 2 - 1] + pv[len(pv) // 2]) / 2)
        rows_fit = s.hits_cutoff(p_fit)
        same_cutoff(rows_fit, None, fitted.cutoff(p_fit)[0], None, "one context, fitted")
        s.cluster_begin()
        s.cluster_add(p_fit, QUERY_NODES)
        clusters_fit = s.cluster_labels()
        same_clusters(clusters_fit, fitted.components(p_fit, QUERY_NODES), "one context, fitted")
    monkeypatch.setenv("SAT_EXP_SELECT_KEYS", str(2 * n))
    with sat.MultiSearcher(3, devices=[0, 0, 0]) as m:
        m.upload(db)
        m.set_queries(queries())
        for k in (None, 3):
            got, got_maps, _ = m.search_cutoff(p, k=k, lorder=True, lsoln=True, maxstart=r)
            assert ([g.tobytes() for g in got], [g.tobytes() for g in got_maps]) == want[k], "3 shards, k = %s" % k
        m.cluster_begin()
        m.cluster_add(p, QUERY_NODES)
        same_clusters(m.cluster_labels(), clusters, "3 shards")
        got_fits, _ = m.search_fit(0.01, lorder=True, lsoln=False, maxstart=r)
        assert got_fits.tobytes() == fits.tobytes()
        same_cutoff(m.hits_cutoff(p_fit), None, rows_fit, None, "3 shards, fitted")
        m.cluster_begin()
        m.cluster_add(p_fit, QUERY_NODES)
        same_clusters(m.cluster_labels(), clusters_fit, "3 shards, fitted")


@pytest.mark.parametrize("args", [("-k", "3"), ("-p", "1e-3"), ("-F", "0.1", "-k", "3"), ("-L", "1e-3")],
                         ids=["k3", "p1e-3", "F0.1-k3", "L1e-3"])
def test_cli_all_vs_all_chunked(golden_dir, args):
    """586 entries, batches of 256 queries: 58 607 keys are chunks of 100, 100 and 56 queries in best-k"""
    env = {k: v for k, v in os.environ.items() if k != "SAT_EXP_SELECT_KEYS"}
    out = []
    for extra in ({}, {"SAT_EXP_SELECT_KEYS": "58607"}):
        run = subprocess.run([CLI, "-a", SMALL_DB, "-r", "16", *args], input=b"", cwd=golden_dir, capture_output=True,
                             timeout=300, env=dict(env, **extra))
        assert run.returncode == 0, run.stderr.decode()[-400:]
        out.append(run.stdout)
    assert out[0] == out[1] and len(out[0]) > 586 * 8
