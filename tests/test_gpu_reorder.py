"""Hits that match only out of sequence order, selected on the GPU (-m gpu): sat_baseline_*, sat_reorder_hits,
sat_search_reordered, their shards and the command line's -X B.  The expected rows never come from the new kernels:
sat_results of two plain searches on the same context, topk_hits(n) for every row's statistics doubles, and the order
of each map by reorder_lib's Python restatement (reorder_lib.expected_rows).  The planted circular permutants are
pinned to the CPU oracle when the test runs."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import report, search
from cuda_satabsearch_amd.search import SatError
import motif_lib
import oracle_lib
import reorder_lib as rl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
EDGE_SIZES = (1023, 1024, 1025, 2049)          # a block of the selection passes holds 1024 rows of one query
EDGE_R = 4
ALL = rl.SEQ | rl.CIRC | rl.PERM


# ---------------------------------------------------------------- the two searches and their parts
def by_entry(stats, field):
    """[nq, n] of a topk_hits(n) field, indexed by entry"""
    out = np.empty(stats.shape, stats[field].dtype)
    for q in range(stats.shape[0]):
        out[q, stats[q]["entry"]] = stats[q][field]
    return out


def two_searches(s, r, censor=None):
    """The ordered search kept as the baseline, then the unordered search with maps - each step a plain call - and the
    parts the expected rows are made of."""
    n = s.n_entries
    base_scores, _, _ = s.search(True, False, r)
    base_fits = s.fit_statistics(censor) if censor is not None else None
    base_p = by_entry(s.topk_hits(n), "pvalue")
    before = s.d2h_bytes()
    s.baseline_keep()
    assert s.d2h_bytes() == before, "keeping the baseline copies nothing to the host"
    scores, maps, _ = s.search(False, True, r)
    fits = s.fit_statistics(censor) if censor is not None else None
    stats = s.topk_hits(n)
    return dict(base_scores=base_scores.reshape(-1, n), base_p=base_p, scores=scores.reshape(-1, n), maps=maps.reshape(-1, n, rl.MAXDIM),
                stats=stats, n1s=s._n1s.copy(), base_fits=base_fits, fits=fits)


def want_rows(parts, max_p, min_base_p, kinds, k=None):
    return rl.expected_rows(parts["scores"], parts["maps"], parts["stats"], parts["base_scores"], parts["base_p"], parts["n1s"],
                            max_p, min_base_p, kinds, k)


def check(s, parts, max_p, min_base_p, kinds, k=None, what=""):
    want, want_maps = want_rows(parts, max_p, min_base_p, kinds, k)
    before = s.d2h_bytes()
    got, got_maps = s.reorder_hits(max_p, min_base_p, kinds, k=k, lsoln=True)
    total = sum(len(w) for w in want)
    if total <= 256:                                        # (a larger result is selected twice: the buffer grows)
        assert s.d2h_bytes() - before == 4 * len(want) + (64 + 444) * total, what
    rl.same_rows(got, got_maps, want, want_maps, what)
    return want


@pytest.fixture(scope="module")
def mixed():
    """the mixed batch searched twice on a context of its own: (searcher, parts)"""
    with sat.Searcher(0) as s:
        s.upload(rl.mixed_db())
        s.set_queries_from_db(list(rl.MIXED_QUERIES))
        yield s, two_searches(s, rl.MIXED_R)


@pytest.fixture(scope="module")
def searcher():
    with sat.Searcher(0) as s:
        yield s


# ---------------------------------------------------------------- 1. the mixed batch, every mask
def test_mixed_batch_has_every_kind(mixed):
    s, parts = mixed
    want, _ = want_rows(parts, 1.0, 0.0, ALL)
    assert [len(w) for w in want] == [len(rl.MIXED_ORDERS)] * len(rl.MIXED_QUERIES)
    kinds = [r["kind"] for rows in want for r in rows]
    print("kinds of the %d rows: seq %d circ %d perm %d" % (len(kinds), kinds.count(rl.SEQ), kinds.count(rl.CIRC), kinds.count(rl.PERM)))
    assert rl.kinds_present(want) == {rl.SEQ, rl.CIRC, rl.PERM}        # no mask below passes vacuously
    # only a circular map has a cut
    assert all(r["cut"] == 0 for rows in want for r in rows if r["kind"] != rl.CIRC)


@pytest.mark.parametrize("kinds", range(1, 8))
def test_mixed_batch_every_mask_at_p_1(mixed, kinds):
    s, parts = mixed
    want = check(s, parts, 1.0, 0.0, kinds, what="kinds = %d" % kinds)
    assert rl.kinds_present(want) == {b for b in (rl.SEQ, rl.CIRC, rl.PERM) if kinds & b}
    # the hit part of every row is the row hits_cutoff gives
    plain = s.hits_cutoff(1.0)
    got = s.reorder_hits(1.0, 0.0, kinds)
    for q in range(len(plain)):
        rows = {int(h["entry"]): h.tobytes() for h in plain[q]}
        assert all(rows[int(g["hit"]["entry"])] == g["hit"].tobytes() for g in got[q])


def cutoff_with_empty_queries(parts):
    """a p-value that some queries' best rows pass and others' do not"""
    best = np.sort(np.array([parts["stats"][q]["pvalue"].min() for q in range(len(parts["n1s"]))]))
    gaps = [(best[i + 1] / max(best[i], 1e-300), i) for i in range(len(best) - 1) if best[i + 1] > best[i]]
    assert gaps, best
    i = max(gaps)[1]
    return float(np.sqrt(best[i] * best[i + 1])) if best[i] > 0 else float(best[i + 1] / 2)


@pytest.mark.parametrize("kinds", range(1, 8))
def test_mixed_batch_every_mask_at_a_cutoff_that_empties_queries(mixed, kinds):
    s, parts = mixed
    p = cutoff_with_empty_queries(parts)
    every, _ = want_rows(parts, p, 0.0, ALL)
    assert any(len(w) == 0 for w in every) and any(len(w) > 0 for w in every), (p, [len(w) for w in every])
    check(s, parts, p, 0.0, kinds, what="p = %g kinds = %d" % (p, kinds))


def test_min_base_pvalue(mixed):
    s, parts = mixed
    base = np.unique(parts["base_p"])
    assert len(base) >= 3
    between = float((base[len(base) // 2 - 1] + base[len(base) // 2]) / 2)
    counts = []
    for b in (0.0, between, 1.0):
        want = check(s, parts, 1.0, b, ALL, what="min_base_pvalue = %g" % b)
        counts.append(sum(len(w) for w in want))
    print("rows at min_base_pvalue 0, %g, 1: %s" % (between, counts))
    assert counts[0] == parts["scores"].size and counts[0] > counts[1] > counts[2] >= 0
    # both conditions and a mask together
    check(s, parts, cutoff_with_empty_queries(parts), between, rl.CIRC | rl.PERM)


def raw_call(s, max_p, min_base_p, kinds, max_rows, counts, capacity, rows, maps):
    return s._lib.sat_reorder_hits(s._ctx, float(max_p), float(min_base_p), int(kinds), int(max_rows),
                                   None if counts is None else counts.ctypes.data, int(capacity),
                                   None if rows is None else rows.ctypes.data, None if maps is None else maps.ctypes.data)


def test_max_rows_capacity_and_growth(mixed):
    s, parts = mixed
    nq = len(parts["n1s"])
    want, want_maps = want_rows(parts, 1.0, 0.0, rl.CIRC | rl.PERM)
    full = [len(w) for w in want]
    total = sum(full)
    assert total > 8 and max(full) > 3
    counts = np.full(nq, -7, np.int32)
    # no row buffer: the counts alone
    before = s.d2h_bytes()
    assert raw_call(s, 1.0, 0.0, 6, 0, counts, 0, None, None) == total
    assert counts.tolist() == full and s.d2h_bytes() - before == 4 * nq
    # a short buffer: the same, and not a byte of it written
    rows = np.zeros(total, search._REORDER_DTYPE)
    rows["pad"] = 99
    maps = np.full((total, rl.MAXDIM), -5, np.int32)
    counts[:] = -7
    before = s.d2h_bytes()
    assert raw_call(s, 1.0, 0.0, 6, 0, counts, total - 1, rows, maps) == total
    assert counts.tolist() == full and s.d2h_bytes() - before == 4 * nq
    assert (rows["pad"] == 99).all() and (maps == -5).all()
    # grown: the rows
    before = s.d2h_bytes()
    assert raw_call(s, 1.0, 0.0, 6, 0, counts, total, rows, maps) == total
    assert s.d2h_bytes() - before == 4 * nq + (64 + 444) * total
    cuts = np.cumsum(counts)[:-1]
    rl.same_rows(np.split(rows, cuts), np.split(maps, cuts), want, want_maps, "grown")
    # without maps: 64 bytes a row
    before = s.d2h_bytes()
    assert raw_call(s, 1.0, 0.0, 6, 0, counts, total, rows, None) == total
    assert s.d2h_bytes() - before == 4 * nq + 64 * total
    # cut to max_rows
    for k in (1, 3):
        check(s, parts, 1.0, 0.0, 6, k=k, what="max_rows = %d" % k)
        assert raw_call(s, 1.0, 0.0, 6, k, counts, 0, None, None) == sum(min(k, c) for c in full)
        assert counts.tolist() == [min(k, c) for c in full]


def test_bad_arguments_change_nothing(mixed):
    s, parts = mixed
    nq = len(parts["n1s"])
    counts = np.full(nq, -7, np.int32)
    before = s.d2h_bytes()
    bad = [(1.0, 0.0, 6, None), (float("nan"), 0.0, 6, counts), (-0.5, 0.0, 6, counts), (float("inf"), 0.0, 6, counts),
           (1.0, float("nan"), 6, counts), (1.0, -1e-9, 6, counts), (1.0, float("inf"), 6, counts),
           (1.0, 0.0, 0, counts), (1.0, 0.0, 8, counts), (1.0, 0.0, -1, counts)]
    for max_p, min_base_p, kinds, c in bad:
        assert raw_call(s, max_p, min_base_p, kinds, 0, c, 0, None, None) == -1, (max_p, min_base_p, kinds)      # SAT_EINVAL
    assert (counts == -7).all() and s.d2h_bytes() == before
    assert s._lib.sat_reorder_hits(None, 1.0, 0.0, 6, 0, counts.ctypes.data, 0, None, None) == -1
    check(s, parts, 1.0, 0.0, 6, what="after the refusals")


# ---------------------------------------------------------------- 2. block edges, chunks of the query list
@functools.lru_cache(maxsize=None)
def tiled(n):
    return rl.tiled(rl.mixed_db(), n)


@pytest.mark.parametrize("chunked", [False, True], ids=["one chunk", "SELECT_KEYS = 2n"])
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_block_edges(monkeypatch, n, chunked):
    if chunked:
        monkeypatch.setenv("SAT_EXP_SELECT_KEYS", str(2 * n))      # read when the context is created
    else:
        monkeypatch.delenv("SAT_EXP_SELECT_KEYS", raising=False)
    with sat.Searcher(0) as s:
        s.upload(tiled(n))
        s.set_queries_from_db(list(rl.MIXED_QUERIES))
        parts = two_searches(s, EDGE_R)
        assert np.array_equal(s.baseline_results()[0], parts["base_scores"])
        mid = float(np.median(parts["stats"]["pvalue"]))
        for max_p, min_base_p, kinds in ((1.0, 0.0, ALL), (1.0, 0.0, rl.CIRC | rl.PERM), (mid, 0.0, rl.CIRC), (mid, mid, ALL), (1.0, 0.0, rl.SEQ)):
            want = check(s, parts, max_p, min_base_p, kinds, what="n = %d p = %g b = %g kinds = %d" % (n, max_p, min_base_p, kinds))
            if kinds == ALL and max_p == 1.0:
                assert [len(w) for w in want] == [n] * len(rl.MIXED_QUERIES)
                assert rl.kinds_present(want) == {rl.SEQ, rl.CIRC, rl.PERM}
        check(s, parts, 1.0, 0.0, rl.CIRC | rl.PERM, k=5)


# ---------------------------------------------------------------- 3. the baseline's lifetime
def test_baseline_results_and_what_keeps_it(searcher):
    s = searcher
    db = rl.mixed_db()
    s.upload(db)
    s.set_queries_from_db(list(rl.MIXED_QUERIES))
    nq, n = len(rl.MIXED_QUERIES), len(db)
    with pytest.raises(SatError, match="no search has run"):
        s.baseline_keep()
    with pytest.raises(SatError, match="no baseline"):
        s.baseline_results()
    parts = two_searches(s, rl.MIXED_R)
    before = s.d2h_bytes()
    kept = s.baseline_results()
    assert s.d2h_bytes() - before == 12 * nq * n
    assert np.array_equal(kept[0], parts["base_scores"]) and kept[1].tobytes() == parts["base_p"].tobytes()
    # either output alone: 4 or 8 bytes a row
    one = np.empty((nq, n), np.int32)
    before = s.d2h_bytes()
    s._check(s._lib.sat_baseline_results(s._ctx, one.ctypes.data, None))
    assert s.d2h_bytes() - before == 4 * nq * n and np.array_equal(one, kept[0])
    two = np.empty((nq, n), np.float64)
    before = s.d2h_bytes()
    s._check(s._lib.sat_baseline_results(s._ctx, None, two.ctypes.data))
    assert s.d2h_bytes() - before == 8 * nq * n and two.tobytes() == kept[1].tobytes()
    # searches, a fit, the polish setting, and the accumulators keep it
    s.search(False, True, 4)
    s.fit_statistics(0.1)
    s.set_polish_all(2)
    s.set_polish_all(0)
    s.cluster_begin(n)
    s.cover_begin(n)
    s.set_eval_classes(np.zeros(n, np.int32))
    s.search(True, True, 2)
    again = s.baseline_results()
    assert np.array_equal(again[0], kept[0]) and again[1].tobytes() == kept[1].tobytes()
    s.cluster_end()
    s.cover_end()
    # and the selection works on whatever search is the last one with maps
    s.search(False, True, rl.MIXED_R)
    check(s, parts, 1.0, 0.0, ALL, what="searched again")
    # a search without maps: refused, the baseline stays
    s.search(False, False, rl.MIXED_R)
    with pytest.raises(SatError, match="without lsoln"):
        s.reorder_hits(1.0)
    assert np.array_equal(s.baseline_results()[0], kept[0])
    # dropped on request
    s.baseline_drop()
    s.search(False, True, rl.MIXED_R)
    with pytest.raises(SatError, match="no baseline"):
        s.reorder_hits(1.0)
    with pytest.raises(SatError, match="no baseline"):
        s.baseline_results()


def set_one(s, db):
    t, d = db.dense(3)
    s.set_query(t, d, db.ssetypes(3), 0)


DROPS = {
    "upload": lambda s, db: s.upload(db),
    "set_query": set_one,
    "set_queries": lambda s, db: s.set_queries([db.dense(e) + (db.ssetypes(e),) for e in (3, 5)]),
    "set_queries_from_db": lambda s, db: s.set_queries_from_db([3, 5]),
    "set_queries_from_db, the same batch again": lambda s, db: s.set_queries_from_db(list(rl.MIXED_QUERIES)),
    "set_queries_from_db_sses": lambda s, db: s.set_queries_from_db([3, 5], sses=[[2, 0, 1], None]),
}


@pytest.mark.parametrize("how", sorted(DROPS))
def test_what_drops_the_baseline(searcher, how):
    s = searcher
    db = rl.mixed_db()
    s.upload(db)
    s.set_queries_from_db(list(rl.MIXED_QUERIES))
    s.search(True, False, 2)
    s.baseline_keep()
    s.baseline_results()
    DROPS[how](s, db)
    if how == "upload":
        s.set_queries_from_db(list(rl.MIXED_QUERIES))
    with pytest.raises(SatError, match="no baseline"):
        s.baseline_results()
    s.search(False, True, 2)
    with pytest.raises(SatError, match=r"^\[-5\] no baseline"):
        s.reorder_hits(1.0)


def test_state_errors_and_a_baseline_of_another_shape(searcher):
    s = searcher
    db = rl.mixed_db()
    s.upload(db)
    s.set_queries_from_db(list(rl.MIXED_QUERIES))
    with pytest.raises(SatError, match=r"^\[-5\] no search has run"):
        s.reorder_hits(1.0)
    s.search_reordered(2)
    rows = s.reorder_hits(1.0, 0.0, ALL)
    assert [len(r) for r in rows] == [len(db)] * len(rl.MIXED_QUERIES)
    nq, n = len(rl.MIXED_QUERIES), len(db)
    for shape in ((nq - 1, n), (nq, n + 1), (n, nq)):
        s._check(s._lib.sat_debug_baseline_shape(s._ctx, *shape))
        with pytest.raises(SatError, match=r"^\[-5\] the baseline holds %d x %d rows, the last search %d x %d" % (shape + (nq, n))):
            s.reorder_hits(1.0)
    s._check(s._lib.sat_debug_baseline_shape(s._ctx, nq, n))
    assert [r.tobytes() for r in s.reorder_hits(1.0, 0.0, ALL)] == [r.tobytes() for r in rows]


# ---------------------------------------------------------------- 4. fitted statistics, the convenience call
def test_search_reordered_fits_each_search_to_its_own_scores(searcher):
    s = searcher
    n = 1025
    s.upload(tiled(n))
    s.set_queries_from_db(list(rl.MIXED_QUERIES))
    parts = two_searches(s, EDGE_R, censor=0.1)
    assert parts["base_fits"]["fitted"].any() and parts["fits"]["fitted"].any()
    q = int(np.flatnonzero(parts["base_fits"]["fitted"] & parts["fits"]["fitted"])[0])
    assert (parts["base_fits"][q]["a"], parts["base_fits"][q]["b"]) != (parts["fits"][q]["a"], parts["fits"][q]["b"])
    mid = float(np.median(parts["stats"]["pvalue"]))
    base_mid = float(np.median(parts["base_p"]))
    wants = [want_rows(parts, p, b, kinds) for p, b, kinds in ((1.0, 0.0, ALL), (mid, base_mid, rl.CIRC | rl.PERM))]
    # base_pvalue is the ordered search's FITTED double: not what the built-in table gives the same score
    builtin = np.array([[report.stats(parts["base_scores"][q, e], parts["n1s"][q], tiled(n).orders[e])[2] for e in range(n)]])
    assert (builtin[0] != parts["base_p"][q]).any()
    # the one call on a fresh batch gives the same baseline and the same rows
    s.set_queries_from_db(list(rl.MIXED_QUERIES))
    ms = s.search_reordered(EDGE_R, censor=0.1)
    assert ms > 0
    kept = s.baseline_results()
    assert np.array_equal(kept[0], parts["base_scores"]) and kept[1].tobytes() == parts["base_p"].tobytes()
    for (p, b, kinds), (want, want_maps) in zip(((1.0, 0.0, ALL), (mid, base_mid, rl.CIRC | rl.PERM)), wants):
        got, got_maps = s.reorder_hits(p, b, kinds, lsoln=True)
        rl.same_rows(got, got_maps, want, want_maps, "search_reordered, p = %g" % p)
    assert 0 < sum(len(w) for w in wants[1][0]) < sum(len(w) for w in wants[0][0])
    # every other selection call works on the unordered search
    assert np.array_equal(s.results(True)[0], parts["scores"])
    # without a censor nothing is fitted
    s.search_reordered(EDGE_R)
    assert kept[1].tobytes() != s.baseline_results()[1].tobytes() and np.array_equal(s.baseline_results()[0], kept[0])
    with pytest.raises(SatError, match="censor"):
        s.search_reordered(EDGE_R, censor=0.75)


# ---------------------------------------------------------------- 5. shards
@pytest.mark.parametrize("censor", [None, 0.1], ids=["built-in", "fitted"])
def test_two_shards_equal_one_context(searcher, censor):
    n = 1025
    db = tiled(n)
    s = searcher
    s.upload(db)
    s.set_queries_from_db(list(rl.MIXED_QUERIES))
    s.search_reordered(EDGE_R, censor=censor)
    one_base = s.baseline_results()
    mid = float(np.median(s.topk_hits(n)["pvalue"]))
    cases = ((1.0, 0.0, ALL, None), (mid, 0.0, rl.CIRC | rl.PERM, None), (1.0, mid, rl.PERM, 7))
    one = [s.reorder_hits(p, b, kinds, k=k, lsoln=True) for p, b, kinds, k in cases]
    with sat.MultiSearcher(2, devices=[0, 0]) as m:
        m.upload(db)
        assert m.ndev == 2 and 0 < m.shards()[1] < n
        m.set_queries_from_db(list(rl.MIXED_QUERIES))
        with pytest.raises(SatError, match="no search has run"):
            m.baseline_keep()
        m.search_only(False, True, EDGE_R)
        with pytest.raises(SatError, match="no baseline"):
            m.reorder_hits(1.0)
        assert m.search_reordered(EDGE_R, censor=censor) > 0
        two_base = m.baseline_results()
        assert np.array_equal(two_base[0], one_base[0]) and two_base[1].tobytes() == one_base[1].tobytes()
        for (p, b, kinds, k), (rows, maps) in zip(cases, one):
            got, got_maps = m.reorder_hits(p, b, kinds, k=k, lsoln=True)
            assert [g.tobytes() for g in got] == [r.tobytes() for r in rows], (p, b, kinds, k)
            assert [g.tobytes() for g in got_maps] == [r.tobytes() for r in maps], (p, b, kinds, k)
        assert sum(len(r) for r in one[1][0]) > 0
        m.baseline_drop()
        with pytest.raises(SatError, match="no baseline"):
            m.reorder_hits(1.0)


# ---------------------------------------------------------------- 6. planted circular permutants
def planted_figures(db, e):
    """the oracle's two scores of the source row and its unordered map, computed now"""
    n = int(db.orders[e])
    lst, cut = rl.rotation(n)
    qt, qd, ty = motif_lib.cut(db, e, lst)
    unordered, maps, _ = oracle_lib.search(db, qt, qd, ty, False, True, rl.PLANTED_R, seed=1234, query_ordinal=e)
    ordered, _, _ = oracle_lib.search(db, qt, qd, ty, True, False, rl.PLANTED_R, seed=1234, query_ordinal=e)
    return lst, cut, unordered, ordered, maps


@pytest.mark.parametrize("e", sorted(rl.PLANTED))
def test_planted_circular_permutant(searcher, e):
    db = rl.planted_db()
    n = int(db.orders[e])
    lst, cut, unordered, ordered, omaps = planted_figures(db, e)
    assert (int(unordered[e]), int(ordered[e])) == rl.PLANTED[e] and unordered[e] == n * (n - 1)
    assert rl.kind(omaps[e, :n]) == (rl.CIRC, n, 1, cut) and cut == n - n // 2 + 1
    s = searcher
    s.upload(db)
    s.set_queries_from_db([e], first_query_ordinal=e, sses=[lst])
    s.search_reordered(rl.PLANTED_R)
    rows, maps = s.reorder_hits(1.0, 0.0, rl.CIRC, lsoln=True)
    at = np.flatnonzero(rows[0]["hit"]["entry"] == e)
    assert len(at) == 1, rows[0]
    row = rows[0][at[0]]
    assert at[0] == 0, "the source entry ranks first"
    assert (int(row["hit"]["score"]), int(row["base_score"])) == rl.PLANTED[e]
    assert (int(row["kind"]), int(row["matched"]), int(row["descents"]), int(row["cut"])) == (rl.CIRC, n, 1, cut)
    assert maps[0][at[0]][:n].tolist() == lst
    # the whole row set is the oracle's
    base = s.baseline_results()[0]
    assert np.array_equal(base[0], ordered) and np.array_equal(s.results(True)[0][0], unordered)


def test_planted_circular_permutants_through_the_command_line(tmp_path, searcher):
    """-Q db -p 1 -X 0 -x c with motif lines on stdin: query b of the list is entry b, so its ordinal is the entry's;
    the planted entries are rotated, the others whole.  The output is the header lines and report.reorder_table of the
    same batch through the library, and the source rows carry the oracle's figures."""
    db = rl.planted_db("s%06d")
    dbfile = str(tmp_path / "planted.ascii")
    sat.synth.write_ascii(db, dbfile)
    entries = list(range(8))
    sses = [rl.rotation(int(db.orders[e]))[0] if e in rl.PLANTED else None for e in entries]
    p = subprocess.run([CLI, "-Q", dbfile, "-p", "1", "-X", "0", "-x", "c", "-r", str(rl.PLANTED_R)],
                       input=motif_lib.stdin_lines(db, entries, sses), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-800:]
    s = searcher
    s.upload(db)
    s.set_queries_from_db(entries, sses=sses)
    s.search_reordered(rl.PLANTED_R)
    rows, maps = s.reorder_hits(1.0, 0.0, rl.CIRC, lsoln=True)
    want = []
    for q, e in enumerate(entries):
        want += report.header_lines(db.names[e], dbfile, True, False, True)
        if sses[q] is not None:
            want.append("# QUERY SSES = " + motif_lib.spell(sses[q]))
        want += report.reorder_table(db.names, rows[q], maps[q], int(s._n1s[q]), 0.0, rl.CIRC)
    assert p.stdout.decode().splitlines() == want
    for e, (full, ordered) in rl.PLANTED.items():
        n = int(db.orders[e])
        line = "%-8s %d " % (db.names[e], full)
        block = p.stdout.decode().split("# QUERY ID = %-8s\n" % db.names[e])[1].split("# cudaSaTabsearch")[0].splitlines()
        source = [l for l in block if l.startswith(line)]
        assert len(source) == 1 and source[0].split()[5:] == [str(ordered), source[0].split()[6], "circ", str(n), "1", str(n - n // 2 + 1)]


def test_command_line_with_a_fit_and_two_shards(tmp_path, searcher):
    """-a -X B -p P -F c -k K -G 0,0 against the library's own calls: both # GUMBEL lines, the cut to K"""
    n = 200
    db = tiled(n)
    dbfile = str(tmp_path / "tiled.ascii")
    sat.synth.write_ascii(db, dbfile)
    with sat.MultiSearcher(2, devices=[0, 0]) as m:
        m.upload(db)
        m.set_queries_from_db(list(range(n)))
        base_fits, _ = m.search_fit(0.1, True, False, EDGE_R)
        m.baseline_keep()
        fits, _ = m.search_fit(0.1, False, True, EDGE_R)
        rows, maps = m.reorder_hits(0.5, 0.01, rl.CIRC | rl.PERM, k=3, lsoln=True)
    print("rows: %d of at most %d" % (sum(len(r) for r in rows), 3 * n))
    assert 0 < sum(len(r) for r in rows) <= 3 * n and max(len(r) for r in rows) == 3
    want = []
    for q in range(n):
        want += report.header_lines(db.names[q], dbfile, True, False, True)
        f = fits[q]
        want.append("# GUMBEL a = %.17g b = %.17g rows = %d censored = %d below = %d" % (f["a"], f["b"], f["rows"], f["censored"], f["below"])
                    if f["fitted"] else "# GUMBEL not fitted")
        want += report.reorder_table(db.names, rows[q], maps[q], int(db.orders[q]), 0.01, rl.CIRC | rl.PERM, base_fit=base_fits[q])
    p = subprocess.run([CLI, "-a", dbfile, "-p", "0.5", "-X", "0.01", "-F", "0.1", "-k", "3", "-G", "0,0", "-r", str(EDGE_R)],
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-800:]
    assert p.stdout.decode().splitlines() == want
