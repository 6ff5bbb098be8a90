"""GPU parity tests (-m gpu): the HIP kernel, called through the C ABI, against the CPU
oracle running the same counter-based Philox streams.  Integer work: bit-exact scores
and bit-identical SSE maps.  (The oracle itself is pinned to the reference's `-c` output
in test_oracle_golden.py; the only difference between the two oracle modes is the
random stream.)"""
import os

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import oracle_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def searcher():
    assert sat.device_count() >= 1, "GPU tests need a HIP device (no CPU path exists)"
    s = sat.Searcher(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def small_db(golden_dir):
    return sat.StructSet.read(os.path.join(golden_dir, "tableauxdistmatrixdb.small.ascii"))


def load_query(golden_dir, name, index=0):
    qs = sat.StructSet.read(os.path.join(golden_dir, name), "query", skip_header_lines=2)
    t, d = qs.dense(index)
    return t, d, qs.ssetypes(index)


def check(searcher, db, q, lorder, lsoln, maxstart, entries=None, query_ordinal=0, seed=1234):
    qt, qd, qtypes = q
    searcher.set_query(qt, qd, qtypes, query_ordinal)
    scores, maps, _ = searcher.search(lorder, lsoln, maxstart)
    idx = np.arange(len(db)) if entries is None else np.asarray(entries)
    oscores, omaps, _ = oracle_lib.search(db, qt, qd, qtypes, lorder, lsoln, maxstart, entries=idx,
                                          query_ordinal=query_ordinal, seed=seed)
    bad = np.nonzero(scores[idx] != oscores)[0]
    assert bad.size == 0, f"{bad.size} score mismatches, first at entry {idx[bad[:5]]}: gpu {scores[idx][bad[:5]]} oracle {oscores[bad[:5]]}"
    if lsoln:
        assert np.array_equal(maps[idx], omaps), "SSE maps differ"
    return scores, maps


# ---------------------------------------------------------------- reference example data
@pytest.mark.parametrize("qfile,qi,lorder,lsoln", [
    ("c1_d1ubia_small.input", 0, True, False),      # BASELINE configs[1]: 8 SSEs, T T F
    ("d2phlb1.input", 0, True, True),               # 19 SSEs with solution maps
    ("d2phlb1.input", 0, False, True),              # LORDER = F window [0, n2)
    ("multiquery.input", 1, True, False),           # 13 SSEs
    ("d1twfa_.input", 0, True, True),               # 101 SSEs: widest query class
])
def test_small_db_bit_exact(searcher, small_db, golden_dir, qfile, qi, lorder, lsoln):
    searcher.upload(small_db)
    check(searcher, small_db, load_query(golden_dir, qfile, qi), lorder, lsoln, 128)


@pytest.mark.parametrize("maxstart", [1, 63, 64, 100, 128, 300, 1024])
def test_restart_counts(searcher, small_db, golden_dir, maxstart):
    """maxstart below / not a multiple of / above the workgroup size (lanes loop)."""
    searcher.upload(small_db)
    entries = np.arange(0, len(small_db), 7)
    check(searcher, small_db, load_query(golden_dir, "d2phlb1.input"), True, True, maxstart, entries=entries)


def test_known_answer_rows(searcher, golden_dir):
    """Near-self match of the 1-entry example db: score 54 and the identity map, as the
    reference prints for d1ubia_.input (expected/d1ubia_.r128.out)."""
    db = sat.StructSet.read(os.path.join(golden_dir, "tableauxdistmatrixdb.test.ascii"))
    searcher.upload(db)
    q = load_query(golden_dir, "d1ubia_.input")
    scores, maps = check(searcher, db, q, True, True, 128)
    assert scores[0] == 54
    assert list(maps[0][:8]) == list(range(8))
    lines = sat.report.result_lines(db.names, db.orders, scores, 8, maps)
    expected = open(os.path.join(ROOT, "tests/golden/expected/d1ubia_.r128.out")).read().splitlines()[3:]
    assert lines == expected


# ---------------------------------------------------------------- every size class
@pytest.fixture(scope="module")
def wide_db():
    """Orders uniform on [1, 111]: every db bucket and bit-set width."""
    return sat.synth.make_db(230, 1, 111, sort=False, seed=77)


@pytest.mark.parametrize("n1", [1, 2, 5, 16, 17, 32, 33, 64, 65, 96, 111])
def test_all_query_and_db_classes(searcher, wide_db, n1):
    searcher.upload(wide_db)
    rng = np.random.default_rng(n1)
    src = int(rng.choice(np.nonzero(wide_db.orders >= n1)[0]))
    t, d = wide_db.dense(src)
    sel = np.sort(rng.choice(int(wide_db.orders[src]), size=n1, replace=False))
    q = (t[np.ix_(sel, sel)].copy(), d[np.ix_(sel, sel)].copy(), np.diagonal(t)[sel].copy())
    scores, _ = check(searcher, wide_db, q, True, True, 128)
    if n1 >= 5:
        assert scores[src] == scores.max()        # the planted source is the best hit
    check(searcher, wide_db, q, False, False, 64, entries=np.arange(0, len(wide_db), 3))


def test_large_everything_lds_spill_regime(searcher):
    """BASELINE configs[4] shape: >= 64-SSE query, LSOLN = T, db entries up to 111 SSEs:
    the query cells no longer fit beside the db entry in LDS."""
    db = sat.synth.make_db(48, 90, 111, sort=True, seed=5)
    searcher.upload(db)
    q = sat.synth.planted_query(db, 40, keep=0.95)
    assert len(q[2]) >= 64
    check(searcher, db, q, True, True, 128)
    check(searcher, db, q, True, True, 256)


# ---------------------------------------------------------------- every execution mode
@pytest.mark.parametrize("env", [{"SAT_EXP_LPC": "0", "SAT_EXP_COMPACT": "0"}, {"SAT_EXP_LPC": "0", "SAT_EXP_COMPACT": "1"},
                                 {"SAT_EXP_LPC": "1", "SAT_EXP_COMPACT": "1"}, {"SAT_EXP_LPC": "2", "SAT_EXP_COMPACT": "1"},
                                 {"SAT_EXP_LPC": "2", "SAT_EXP_COMPACT": "0"}, {"SAT_EXP_QLDS": "1"}],
                         ids=lambda e: ",".join(f"{k[8:]}={v}" for k, v in e.items()))
def test_forced_execution_modes(monkeypatch, env):
    """The launch heuristics (lanes per chain, work compaction, query cells in LDS) only change
    how the work is laid out; forced through the library's tuning overrides (read when a context is
    created), every layout must give the oracle's bits, for both LORDER modes and with solution maps."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    db = sat.synth.make_db(150, 6, 40, seed=21)
    with sat.Searcher(0) as forced:
        forced.upload(db)
        for src, keep in ((140, 0.8), (20, 1.0)):
            q = sat.synth.planted_query(db, src, keep=keep)
            check(forced, db, q, True, True, 128)
            check(forced, db, q, False, True, 100)


@pytest.mark.parametrize("epw", [2, 3, 4])
def test_several_entries_per_workgroup(monkeypatch, epw):
    """Big launches put 2+ entries into one workgroup (entry slots with their own LDS carve; the host picks
    the count from the CU's LDS granules).  Forced here on small databases whose entry counts leave spare
    slots in the last workgroup: scores and solution maps must be the oracle's for every slot count, for a
    query batch (slabs of best maps per slot and query), and for large entries with several lanes per chain."""
    monkeypatch.setenv("SAT_EXP_EPW", str(epw))
    db = sat.synth.make_db(151, 6, 40, seed=33)
    big = sat.synth.make_db(23, 70, 111, sort=True, seed=34)
    with sat.Searcher(0) as s:
        s.upload(db)
        q = sat.synth.planted_query(db, 120, keep=0.9)
        check(s, db, q, True, True, 128)
        check(s, db, q, False, True, 70)
        check(s, db, q, True, False, 128)
        assert f"block {epw} x " in s.last_launch_info()
        queries = [sat.synth.planted_query(db, src, keep=0.8, seed=src) for src in (3, 77, 150)]
        s.set_queries(queries, 2)
        scores, maps, _ = s.search(True, True, 128)
        for qi, (qt, qd, qty) in enumerate(queries):
            osc, omp, _ = oracle_lib.search(db, qt, qd, qty, True, True, 128, query_ordinal=2 + qi)
            assert np.array_equal(scores[qi], osc), f"query {qi}"
            assert np.array_equal(maps[qi], omp), f"maps of query {qi}"
        s.upload(big)
        qb = sat.synth.planted_query(big, 20, keep=0.6)
        check(s, big, qb, True, True, 128)


@pytest.mark.parametrize("general", [False, True], ids=["specialised", "general"])
def test_round_shapes_of_every_query_order_class(wide_db, monkeypatch, general):
    """The compacted rounds serve a listed row with ceil(n1w/4) lanes x up to 4 map words, pad the
    maps to whole words per lane and send a step's last rows to 1- and 2-word shapes.  One query
    order from every (lanes per row, words per lane, padding) class, LSOLN off so that the
    option-specialised instantiations run, and again through the general kernel
    (SAT_EXP_GENERAL), which picks the shape at run time."""
    if general:
        monkeypatch.setenv("SAT_EXP_GENERAL", "1")
    with sat.Searcher(0) as searcher:              # the override is read when the context is created
        searcher.upload(wide_db)
        entries = np.arange(0, len(wide_db), 4)
        for n1 in (3, 4, 8, 9, 12, 13, 19, 21, 24, 25, 28, 36, 37, 40, 45, 48, 52, 61, 68, 77, 84, 100, 109):
            rng = np.random.default_rng(1000 + n1)
            src = int(rng.choice(np.nonzero(wide_db.orders >= n1)[0]))
            t, d = wide_db.dense(src)
            sel = np.sort(rng.choice(int(wide_db.orders[src]), size=n1, replace=False))
            q = (t[np.ix_(sel, sel)].copy(), d[np.ix_(sel, sel)].copy(), np.diagonal(t)[sel].copy())
            check(searcher, wide_db, q, True, False, 64, entries=entries)


def test_batch_of_mixed_round_shapes(searcher, wide_db):
    """Queries of one size class but different words-per-lane counts in one batch: the launch
    cannot use an instantiation with a fixed count and must still give every query's bits."""
    searcher.upload(wide_db)
    queries = []
    for n1 in (17, 21, 24, 29, 32):          # 32 class: 3, 3, 3, 4, 4 words per lane
        rng = np.random.default_rng(2000 + n1)
        src = int(rng.choice(np.nonzero(wide_db.orders >= n1)[0]))
        t, d = wide_db.dense(src)
        sel = np.sort(rng.choice(int(wide_db.orders[src]), size=n1, replace=False))
        queries.append((t[np.ix_(sel, sel)].copy(), d[np.ix_(sel, sel)].copy(), np.diagonal(t)[sel].copy()))
    searcher.set_queries(queries, 5)
    scores, _, _ = searcher.search(True, False, 64)
    idx = np.arange(0, len(wide_db), 5)
    for qi, (qt, qd, qtypes) in enumerate(queries):
        oscores, _, _ = oracle_lib.search(wide_db, qt, qd, qtypes, True, False, 64, entries=idx, query_ordinal=5 + qi)
        assert np.array_equal(scores[qi][idx], oscores), f"query {qi} of the batch differs"


# ---------------------------------------------------------------- keys of the streams
def test_sharding_does_not_change_results(searcher):
    db = sat.synth.make_db(600, 8, 32)
    q = sat.synth.planted_query(db, 123)
    searcher.upload(db)
    whole, wmaps = check(searcher, db, q, True, True, 128, entries=np.arange(0, 600, 11))
    for lo, hi in [(0, 150), (150, 600)]:
        shard = db.subset(np.arange(lo, hi))
        searcher.upload(shard, db_ordinal=np.arange(lo, hi))
        searcher.set_query(*q, 0)
        s, m, _ = searcher.search(True, True, 128)
        assert np.array_equal(s, whole[lo:hi]) and np.array_equal(m, wmaps[lo:hi])


def test_query_ordinal_and_seed_key_the_streams(searcher, small_db, golden_dir):
    q = load_query(golden_dir, "d2phlb1.input")
    searcher.upload(small_db)
    entries = np.arange(0, len(small_db), 5)
    s0, _ = check(searcher, small_db, q, True, False, 128, entries=entries, query_ordinal=0)
    s3, _ = check(searcher, small_db, q, True, False, 128, entries=entries, query_ordinal=3)
    assert not np.array_equal(s0, s3)
    with sat.Searcher(0, seed=99) as other:
        other.upload(small_db)
        s99, _ = check(other, small_db, q, True, False, 128, entries=entries, seed=99)
    assert not np.array_equal(s0, s99)


def test_dense_upload_equals_packed(searcher, small_db, golden_dir):
    q = load_query(golden_dir, "c1_d1ubia_small.input")
    searcher.upload(small_db)
    searcher.set_query(*q, 0)
    a, _, _ = searcher.search(True, False, 128)
    pitch = 96
    tabs = np.zeros((len(small_db), pitch, pitch), np.uint8)
    dmats = np.zeros((len(small_db), pitch, pitch), np.float32)
    for s in range(len(small_db)):
        tabs[s], dmats[s] = small_db.dense(s, pitch)
    searcher.upload_dense(small_db.orders, tabs, dmats, pitch)
    searcher.set_query(*q, 0)
    b, _, _ = searcher.search(True, False, 128)
    assert np.array_equal(a, b)


# ---------------------------------------------------------------- query batches
def test_query_batch_equals_one_by_one(searcher, small_db, golden_dir):
    """A batch (grid = entries x queries) gives, row by row, what single-query searches give:
    mixed size classes (8, 13, 19, 101 SSEs), LSOLN maps, query ordinals first..first+3."""
    qs = [load_query(golden_dir, "multiquery.input", 0), load_query(golden_dir, "multiquery.input", 1),
          load_query(golden_dir, "d2phlb1.input"), load_query(golden_dir, "multiquery.input", 2)]
    searcher.upload(small_db)
    entries = np.arange(0, len(small_db), 9)
    searcher.set_queries(qs, first_query_ordinal=5)
    scores, maps, _ = searcher.search(True, True, 128)
    assert scores.shape == (4, len(small_db)) and maps.shape == (4, len(small_db), 111)
    for k, q in enumerate(qs):
        osc, omaps, _ = oracle_lib.search(small_db, *q, True, True, 128, entries=entries, query_ordinal=5 + k)
        assert np.array_equal(scores[k][entries], osc), f"query {k}"
        assert np.array_equal(maps[k][entries], omaps), f"query {k}"
    searcher.set_query(*qs[2], 7)
    one, onemaps, _ = searcher.search(True, True, 128)
    assert np.array_equal(one, scores[2]) and np.array_equal(onemaps, maps[2])


def test_large_query_batch_on_small_db(searcher, small_db):
    """-q style workload: many db members as queries against the same small database."""
    pick = np.nonzero((small_db.orders >= 4) & (small_db.orders <= 40))[0][:48]
    qs = [(*small_db.dense(int(s)), small_db.ssetypes(int(s))) for s in pick]
    searcher.upload(small_db)
    searcher.set_queries(qs)
    scores, _, ms = searcher.search(True, False, 128)
    # each query structure is in the database: its own entry is the top hit (or ties it)
    for k, s in enumerate(pick):
        assert scores[k][s] == scores[k].max()
    k = 17
    osc, _, _ = oracle_lib.search(small_db, *qs[k], True, False, 128, query_ordinal=k, entries=np.arange(0, 586, 13))
    assert np.array_equal(scores[k][np.arange(0, 586, 13)], osc)
    print(f"48 queries x 586 entries: {ms:.2f} ms -> {48 * 586 / ms * 1e3:,.0f} scorings/s")


def test_device_topk(searcher, small_db, golden_dir):
    qs = [load_query(golden_dir, "d2phlb1.input"), load_query(golden_dir, "multiquery.input", 1)]
    searcher.upload(small_db)
    searcher.set_queries(qs)
    scores, _, _ = searcher.search(True, False, 128)
    for qi in range(2):
        idx, sc = searcher.topk(25, query=qi)
        order = np.lexsort((np.arange(len(small_db)), -scores[qi].astype(np.int64)))[:25]
        assert np.array_equal(idx, order) and np.array_equal(sc, scores[qi][order])
    idx, sc = searcher.topk(10_000, query=0)          # k larger than the database
    assert len(idx) == len(small_db) and (np.diff(sc) <= 0).all()


def test_device_topk_rows_carry_the_hosts_statistics(searcher, small_db, golden_dir):
    """sat_topk_hits: the best k rows of EVERY query of a batch from one segmented sort, with norm2 /
    z / p computed on the device - bit-identical to csrc/host/sat_gumbel.c (z from the norm2 score
    truncated to an int, as the reference does) - and the rows' solution maps after an LSOLN search."""
    from cuda_satabsearch_amd import _native
    host = _native.host_lib()
    qs = [load_query(golden_dir, "d2phlb1.input"), load_query(golden_dir, "multiquery.input", 0),
          load_query(golden_dir, "multiquery.input", 2)]                    # 19, 8 and 101 SSEs
    searcher.upload(small_db)
    searcher.set_queries(qs)
    scores, maps, _ = searcher.search(True, True, 128)
    k = 12
    hits, hmaps = searcher.topk_hits(k, lsoln=True)
    assert hits.shape == (3, k) and hmaps.shape == (3, k, 111)
    n = len(small_db)
    for qi, q in enumerate(qs):
        n1 = len(q[2])
        order = np.lexsort((np.arange(n), -scores[qi].astype(np.int64)))[:k]
        assert np.array_equal(hits[qi]["entry"], order) and np.array_equal(hits[qi]["score"], scores[qi][order])
        for r, e in enumerate(order):
            norm2 = host.sat_norm2(int(scores[qi][e]), n1, int(small_db.orders[e]))
            z = host.sat_z_gumbel_trunc(norm2)
            # bit for bit: compare the doubles' bytes, not their values
            assert np.float64(norm2).tobytes() == hits[qi]["norm2"][r].tobytes()
            assert np.float64(z).tobytes() == hits[qi]["zscore"][r].tobytes()
            assert np.float64(host.sat_pv_gumbel(z)).tobytes() == hits[qi]["pvalue"][r].tobytes()
        assert np.array_equal(hmaps[qi], maps[qi][order])
    # negative and fractional norm2 scores exercise the truncation toward zero
    assert (hits["norm2"] < 1.0).any() and (hits["norm2"] > 1.0).any()
    with pytest.raises(sat.SatError, match="without lsoln"):
        searcher.search_async(True, False, 64)
        searcher.topk_hits(3, lsoln=True)


def test_topk_download_is_k_rows_per_query():
    """After a search of 100 000 entries the best-10 path copies 10 rows per query to the host
    (32 bytes each), not the 400 KB score array: the context's own byte counter is the witness."""
    db = sat.synth.make_db(100_000, 8, 32, sort=True)
    qs = [sat.synth.make_query(32), sat.synth.make_query(16), sat.synth.planted_query(db, 70_000)]
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(qs)
        s.search_async(True, False, 64)
        before = s.d2h_bytes()
        hits = s.topk_hits(10)
        assert s.d2h_bytes() - before == 3 * 10 * 32
        full, _ = s.results()
        assert s.d2h_bytes() - before == 3 * 10 * 32 + 3 * 100_000 * 4
    for qi in range(3):
        order = np.lexsort((np.arange(len(db)), -full[qi].astype(np.int64)))[:10]
        assert np.array_equal(hits[qi]["entry"], order)
    assert hits[2]["entry"][0] == 70_000


# ---------------------------------------------------------------- edge cases
def test_degenerate_structures(searcher):
    """1-SSE structures, a query whose SSE types do not occur in an entry, all-'??' codes."""
    orders = np.array([1, 1, 2, 3, 4], np.int32)
    tabs = np.zeros((5, 4, 4), np.uint8)
    dmats = np.zeros((5, 4, 4), np.float32)
    tabs[1, 0, 0] = 1                                   # single helix
    tabs[2][[0, 1], [0, 1]] = [1, 1]; tabs[2, 1, 0] = tabs[2, 0, 1] = 0x44
    tabs[3][[0, 1, 2], [0, 1, 2]] = [3, 3, 3]           # only 3-10 helices
    for s in range(5):
        n = orders[s]
        dmats[s][:n, :n] = 5.0 + np.arange(n * n).reshape(n, n) % 7
        dmats[s] = np.tril(dmats[s], -1) + np.tril(dmats[s], -1).T
    tabs[4][[0, 1, 2, 3], [0, 1, 2, 3]] = [0, 1, 2, 3]
    tabs[4][np.tril_indices(4, -1)] = 0x23
    tabs[4] = np.tril(tabs[4]) + np.tril(tabs[4], -1).T
    db = sat.StructSet.from_dense(orders, tabs, dmats)
    searcher.upload(db)
    qt = np.array([[0, 0x23, 0x44], [0x23, 1, 0x23], [0x44, 0x23, 2]], np.uint8)
    qd = np.array([[0, 6, 9], [6, 1, 7], [9, 7, 2]], np.float32)
    for lorder in (True, False):
        check(searcher, db, (qt, qd, np.array([0, 1, 2], np.uint8)), lorder, True, 128)
    one = (np.array([[1]], np.uint8), np.array([[1.0]], np.float32), np.array([1], np.uint8))
    check(searcher, db, one, True, True, 64)


def test_distance_threshold_boundary(searcher):
    """|d1 - d2| <= 4.0f is evaluated in float, exactly as the reference does: pairs
    engineered to sit on both sides of the boundary after float rounding."""
    rng = np.random.default_rng(3)
    n = 12
    types = rng.integers(0, 2, n).astype(np.uint8)
    base = np.round(rng.uniform(5, 40, (n, n)), 3).astype(np.float32)
    base = np.tril(base, -1) + np.tril(base, -1).T
    codes = rng.choice([0x00, 0x11, 0x23, 0x32], size=(n, n)).astype(np.uint8)
    codes = np.tril(codes, -1) + np.tril(codes, -1).T
    codes[np.arange(n), np.arange(n)] = types
    tabs, dmats = [], []
    for off in (4.0, 3.999, 4.001, np.float32(4.0) + np.float32(2.0 ** -21), -4.0):
        d = (base + np.float32(off)).astype(np.float32)
        d[np.arange(n), np.arange(n)] = types
        tabs.append(codes); dmats.append(np.abs(d))
    db = sat.StructSet.from_dense(np.full(5, n, np.int32), np.array(tabs), np.array(dmats))
    searcher.upload(db)
    qd = base.copy(); qd[np.arange(n), np.arange(n)] = types
    scores, _ = check(searcher, db, (codes, qd, types), True, True, 128)
    assert len(set(scores.tolist())) > 1


@pytest.mark.parametrize("lorder", [True, False])
def test_dense_initial_maps_take_the_rows_form(searcher, lorder):
    """The full score of an initial map walks matched pairs, or - when the densest map of a wave would
    make that the dearer form - the rows in step (sat_sa_kernel.hpp, `walk_pairs`): an all-hit database
    (every entry the query's source structure, thinit matches half its SSEs) sends waves to the rows,
    a database of small strangers to the pair walk, and a mix of the two has both kinds of wave in one
    launch.  32-SSE query class (one-word sets) and a 40-SSE query (two-word query set); bit-exact
    against the oracle either way."""
    for n1, seed in ((32, 5), (40, 6)):
        base = sat.synth.make_db(1, n1, n1, seed=seed)
        t, d = base.dense(0)
        strangers = sat.synth.make_db(24, 6, 14, seed=seed + 10)
        orders = [n1] * 24 + [int(o) for o in strangers.orders]
        tabs = [t] * 24 + [strangers.dense(i)[0] for i in range(24)]
        dmats = [d] * 24 + [strangers.dense(i)[1] for i in range(24)]
        pick = np.random.default_rng(seed).permutation(48)
        db = sat.StructSet.from_dense([orders[i] for i in pick], [tabs[i] for i in pick], [dmats[i] for i in pick])
        searcher.upload(db)
        q = sat.synth.planted_query(base, 0, keep=1.0, jitter=0.5)
        scores, _ = check(searcher, db, q, lorder, True, 128)
        assert scores.max() > 4 * n1            # the hits are hits


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_randomized_structures(searcher, seed):
    """Random structures over the reader's whole alphabet (all 25 code combinations incl.
    '?', all four SSE types) with distances on a coarse grid, so that |d1 - d2| lands on
    exactly 4.0 and its float neighbours all the time; many orders, both LORDER modes."""
    rng = np.random.default_rng(seed)
    n = 90
    orders = rng.integers(1, 41, n).astype(np.int32)
    pmax = int(orders.max())
    tabs = np.zeros((n, pmax, pmax), np.uint8)
    dmats = np.zeros((n, pmax, pmax), np.float32)
    grid = np.concatenate([np.arange(4, 30, 0.5), [8.0 + 2.0 ** -20, 12.0 - 2.0 ** -20, 16.0 + 2.0 ** -19]]).astype(np.float32)
    for s_ in range(n):
        m = int(orders[s_])
        codes = (rng.integers(0, 5, (m, m)) << 4 | rng.integers(0, 5, (m, m))).astype(np.uint8)
        codes = np.tril(codes, -1) + np.tril(codes, -1).T
        d = rng.choice(grid, (m, m)).astype(np.float32)
        d = np.tril(d, -1) + np.tril(d, -1).T
        types = rng.integers(0, 4, m).astype(np.uint8) if rng.random() < 0.7 else np.full(m, rng.integers(0, 4), np.uint8)
        codes[np.arange(m), np.arange(m)] = types
        d[np.arange(m), np.arange(m)] = types
        tabs[s_, :m, :m], dmats[s_, :m, :m] = codes, d
    db = sat.StructSet.from_dense(orders, tabs, dmats)
    searcher.upload(db)
    for qsrc in rng.choice(np.nonzero(orders >= 3)[0], 3, replace=False):
        m = int(orders[qsrc])
        keep = np.sort(rng.choice(m, size=max(2, m - int(rng.integers(0, 3))), replace=False))
        t, d = db.dense(int(qsrc))
        q = (t[np.ix_(keep, keep)].copy(), d[np.ix_(keep, keep)].copy(), np.diagonal(t)[keep].copy())
        check(searcher, db, q, True, True, 96)
        check(searcher, db, q, False, True, 64)


def test_non_finite_and_odd_distances(searcher):
    """NaN / inf / negative / huge distances: the reference's float test |d1 - d2| <= 4 is
    simply false for NaN and inf; the kernel maps them to its sentinel - same scores."""
    rng = np.random.default_rng(11)
    db = sat.synth.make_db(24, 10, 24, seed=3)
    dist = db.dist.copy()
    off = rng.choice(dist.size, 60, replace=False)
    dist[off[:15]] = np.nan
    dist[off[15:30]] = np.inf
    dist[off[30:40]] = -np.inf
    dist[off[40:50]] = -dist[off[40:50]]
    dist[off[50:]] = 1.0e20
    odd = sat.StructSet(db.orders, db.names, db.cell_off, db.tab, dist)
    qt, qd, qtypes = sat.synth.planted_query(db, 5, keep=0.9)
    qd = qd.copy()
    qd[1, 3] = qd[3, 1] = np.nan
    qd[2, 5] = qd[5, 2] = np.inf
    searcher.upload(odd)
    for lorder in (True, False):
        check(searcher, odd, (qt, qd, qtypes), lorder, True, 128)


def test_inputs_outside_the_kernel_domain_are_rejected():
    with sat.Searcher(0) as s:
        db = sat.synth.make_db(3, 6, 6)
        tab = db.tab.copy()
        tab[1] = 0x83                          # off-diagonal code with a nibble above 7
        with pytest.raises(sat.SatError, match="nibble"):
            s.upload(sat.StructSet(db.orders, db.names, db.cell_off, tab, db.dist))
        dist = db.dist.copy()
        dist[1] = 3.0e30
        with pytest.raises(sat.SatError, match="out of range"):
            s.upload(sat.StructSet(db.orders, db.names, db.cell_off, db.tab, dist))
        s.upload(db)
        qt, qd, qtypes = sat.synth.make_query(6)
        bad = qt.copy(); bad[0, 1] = bad[1, 0] = 0x90
        with pytest.raises(sat.SatError, match="nibble"):
            s.set_query(bad, qd, qtypes)
        qtypes2 = qtypes.copy(); qtypes2[0] = 9
        with pytest.raises(sat.SatError, match="type code"):
            s.set_query(qt, qd, qtypes2)


def test_threaded_upload_scan_finds_the_first_bad_entry():
    """Databases of 4096+ entries are validated by several host threads (branch-free scan, then a
    cell-by-cell re-check of the earliest flagged entry): the reported entry must be the first bad
    one in file order whichever thread's range it falls in, and values that only LOOK suspicious to
    the scan's wider net (the unused diagonal distances) must not be rejected."""
    with sat.Searcher(0) as s:
        db = sat.synth.make_db(9000, 6, 12, seed=3)
        tri = lambda e, i, j: int(db.cell_off[e]) + i * (i + 1) // 2 + j
        for first, later in ((8123, 8900), (17, 8123), (4500, 4501)):
            tab = db.tab.copy(); dist = db.dist.copy()
            tab[tri(later, 3, 1)] = 0x99
            dist[tri(first, 4, 2)] = -7.0e29
            with pytest.raises(sat.SatError, match=f"entry {first}: distance"):
                s.upload(sat.StructSet(db.orders, db.names, db.cell_off, tab, dist))
        tab = db.tab.copy()
        tab[tri(7000, 2, 2)] = 7                       # a type code above 3 on the diagonal
        with pytest.raises(sat.SatError, match="entry 7000: SSE 2 has type code 7"):
            s.upload(sat.StructSet(db.orders, db.names, db.cell_off, tab, db.dist))
        dist = db.dist.copy()
        dist[tri(5000, 3, 3)] = 5.0e30                 # diagonal distances are never read: accepted
        dist[tri(5001, 2, 1)] = np.inf                 # non-finite: accepted, becomes the sentinel
        s.upload(sat.StructSet(db.orders, db.names, db.cell_off, db.tab, dist))
        assert s.n_entries == 9000


def test_error_behaviour():
    with sat.Searcher(0) as s:
        with pytest.raises(sat.SatError, match="no database"):
            s.search()
        db = sat.synth.make_db(4, 4, 8)
        s.upload(db)
        with pytest.raises(sat.SatError, match="no query"):
            s.search()
        bad = sat.StructSet(np.array([200], np.int32), ["x"], np.array([0], np.int64),
                            np.zeros(20100, np.uint8), np.zeros(20100, np.float32))
        with pytest.raises(sat.SatError, match="order"):
            s.upload(bad)
        qt, qd, qtypes = sat.synth.make_query(6)
        s.upload(db)
        s.set_query(qt, qd, qtypes)
        with pytest.raises(sat.SatError, match="maxstart"):
            s.search(maxstart=0)
    with pytest.raises(sat.SatError, match="out of range"):
        sat.Searcher(4096)


def test_results_belong_to_the_last_search():
    """The result buffers are only handed out for the search they were filled by: after a new query
    batch or a new upload, sat_results / sat_topk refuse until a search has run (the buffers may be
    too small for the new batch), and solution maps are only served after a search with lsoln."""
    db = sat.synth.make_db(40, 6, 12, seed=9)
    q = sat.synth.make_query(8)
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_query(*q, 0)
        with pytest.raises(sat.SatError, match="no search has run"):
            s.results()
        s.search_async(True, False, 64)
        one, _ = s.results()
        with pytest.raises(sat.SatError, match="without lsoln"):
            s.results(lsoln=True)
        s.set_queries([q, q, q], 0)                    # three times the rows: the old buffer is too small
        with pytest.raises(sat.SatError, match="no search has run"):
            s.results()
        with pytest.raises(sat.SatError, match="no search has run"):
            s.topk(3)
        s.search_async(True, True, 64)
        three, maps = s.results(lsoln=True)
        assert three.shape == (3, 40) and np.array_equal(three[0], one)
        s.upload(db)
        with pytest.raises(sat.SatError, match="no search has run"):
            s.results()


def test_device_score_buffer_is_the_one_the_search_fills():
    """sat_device_scores() after a queued search aliases that search's results (what bench.py hands
    to the RCCL gather), also right after an upload, when the first search must not re-allocate."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")                   # the runtime the library itself is linked with
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    db = sat.synth.make_db(3000, 8, 24, seed=4)
    q = sat.synth.make_query(16)
    with sat.Searcher(0) as s:
        for _ in range(2):
            s.upload(db)
            s.set_query(*q, 0)
            before = s.device_scores_ptr()
            s.search_async(True, False, 64)
            s.sync()
            assert s.device_scores_ptr() == before        # one query: the buffer allocated by the upload is used
            dev = np.empty(len(db), np.int32)
            assert hip.hipMemcpy(dev.ctypes.data, s.device_scores_ptr(), dev.nbytes, 2) == 0     # device -> host
            host, _ = s.results()
            assert np.array_equal(dev, host)


@pytest.mark.parametrize("lsoln", [True, False])
@pytest.mark.parametrize("pieces", [0, 1, 3, 8])
def test_overlapped_upload_and_first_search(monkeypatch, pieces, lsoln):
    """sat_db_upload_search = sat_db_upload_packed + sat_search, bit for bit, whatever the number of
    pieces the shard goes up in (0: the library's own choice - one piece at this size): a size-sorted
    mixed database (several order buckets per piece, pieces cut inside a bucket), a query batch of two
    size classes, scores and solution maps; the context then serves later searches as after a plain
    upload; a sample is checked against the oracle."""
    if pieces:
        monkeypatch.setenv("SAT_EXP_UPLOAD_PIECES", str(pieces))
    db = sat.synth.make_db(6000, 4, 70, seed=21, sort=True)
    queries = [sat.synth.make_query(12, seed=5), sat.synth.make_query(40, seed=6)]
    ordinal = np.arange(len(db)) + 1000
    with sat.Searcher(0) as a, sat.Searcher(0) as b:
        a.upload(db, db_ordinal=ordinal)
        a.set_queries(queries, 3)
        want, want_maps, _ = a.search(True, lsoln, 64)
        b.set_queries(queries, 3)
        b.upload_search(db, True, lsoln, 64, db_ordinal=ordinal)
        got, got_maps = b.results(lsoln=lsoln)
        assert np.array_equal(got, want) and (not lsoln or np.array_equal(got_maps, want_maps))
        # the resident shard is a normal one: other options, another search
        want2, _, _ = a.search(False, False, 64)
        got2, _, _ = b.search(False, False, 64)
        assert np.array_equal(got2, want2)
    sample = np.random.default_rng(1).choice(len(db), 24, replace=False)
    qt, qd, qtypes = queries[0]
    ref, ref_maps, _ = oracle_lib.search(db, qt, qd, qtypes, True, True, 64, entries=sample, query_ordinal=3,
                                         db_ordinal=ordinal)
    assert np.array_equal(got[0][sample], ref)
    assert not lsoln or np.array_equal(got_maps[0][sample], ref_maps)


def test_overlapped_upload_rejects_what_the_plain_upload_rejects(monkeypatch):
    """A bad cell in a late piece fails the whole call (the searches queued before it are thrown away)
    and leaves the context without a database; entries not in ascending cell order take the
    one-piece path and give the same results."""
    monkeypatch.setenv("SAT_EXP_UPLOAD_PIECES", "4")
    db = sat.synth.make_db(4000, 6, 20, seed=8)
    q = sat.synth.make_query(10, seed=2)
    tri = lambda e, i, j: int(db.cell_off[e]) + i * (i + 1) // 2 + j
    with sat.Searcher(0) as s:
        with pytest.raises(sat.SatError, match="no query"):
            s.upload_search(db, True, False, 64)
        s.set_query(*q, 0)
        tab = db.tab.copy()
        tab[tri(3900, 3, 1)] = 0x99
        with pytest.raises(sat.SatError, match="entry 3900: tableau code"):
            s.upload_search(sat.StructSet(db.orders, db.names, db.cell_off, tab, db.dist), True, False, 64)
        with pytest.raises(sat.SatError, match="no database"):
            s.search()
        with pytest.raises(sat.SatError, match="maxstart"):
            s.upload_search(db, True, False, 0)
        s.upload_search(db, True, False, 64)
        want, _ = s.results()
        # the same entries stored back to front: offsets descend, one piece
        order = np.arange(len(db))[::-1]
        cells = db.orders.astype(np.int64) * (db.orders + 1) // 2
        off = np.zeros(len(db), np.int64)
        off[order] = np.concatenate(([0], np.cumsum(cells[order])[:-1]))
        tab2 = np.empty_like(db.tab); dist2 = np.empty_like(db.dist)
        for e in range(len(db)):
            tab2[off[e]:off[e] + cells[e]] = db.tab[db.cell_off[e]:db.cell_off[e] + cells[e]]
            dist2[off[e]:off[e] + cells[e]] = db.dist[db.cell_off[e]:db.cell_off[e] + cells[e]]
        s.upload_search(sat.StructSet(db.orders, db.names, off, tab2, dist2), True, False, 64)
        got, _ = s.results()
        assert np.array_equal(got, want)


# ---------------------------------------------------------------- randomized soak, time-boxed
def test_randomized_soak_with_a_fixed_seed():
    """scripts/fuzz_parity.py inside the suite: 30 seconds of random databases (1..111 SSEs, '?' codes, exact 4.0 A
    differences), planted queries, LORDER / LSOLN, restart counts 1..300, forced lanes per chain / compaction / entries
    per workgroup and best-k rows, from a fixed seed - GPU against the oracle, bit for bit; stops at the first mismatch.
    (Longer soaks of other seeds are run by hand, profiles/*_logs/fuzz_*.)"""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAT_EXP_")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_parity.py"), "30", "20251005"], capture_output=True,
                       text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    last = p.stdout.strip().splitlines()[-1]
    assert last.startswith("fuzz ok:"), last
    assert int(last.split()[2]) >= 50, last          # ~10 cases a second on an idle box
    print("\n" + last)


# ---------------------------------------------------------------- the reference's in-kernel self-check
@pytest.mark.parametrize("lpc", ["", "1", "2"])
def test_every_move_passes_the_references_self_check(lpc):
    """The reference kernel, built with TESTING, asserts on EVERY move that score + delta equals the full score of
    the moved map (K.cu:1105-1134).  The same assertion lives in a diagnostic build of the device library
    (tests/native/libsat_selfcheck.so = the product sources + -DSAT_DIAG_SELFCHECK, csrc/diag/sat_diag.hpp; the
    shipped library contains none of it): after every proposal the proposed map's score is recomputed from the
    map bytes and the cell matrix and compared with score + delta.  Entries of 1..111 SSEs x queries of every
    size class x LORDER / LSOLN, one and several lanes per chain: millions of checked moves, no mismatch, and the
    diagnostic build's scores equal the oracle's."""
    import json
    import subprocess
    import sys
    lib = os.path.join(ROOT, "tests", "native", "libsat_selfcheck.so")
    assert os.path.exists(lib), "build with python -m cuda_satabsearch_amd.build --oracle"
    env = dict(os.environ, SAT_DEVICE_LIB=lib)
    if lpc:
        env["SAT_EXP_LPC"] = lpc
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "native", "selfcheck_run.py")], capture_output=True,
                       text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    cases = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(cases) == 18
    total = 0
    for c in cases:
        assert c["mismatches"] == 0 and c["scores_equal_oracle"], c
        # every (entry, restart, step) proposes exactly one move: 40 entries x 70 restarts x 100 steps
        assert c["checks"] == 40 * 70 * 100, c
        total += c["checks"]
    print(f"\n{total} moves checked against a full recomputation (lanes per chain: {lpc or 'default'})")


# ---------------------------------------------------------------- reference -c stream (T3)
@pytest.mark.parametrize("job", ["c1_d1ubia_small.r128", "d2phlb1.r4096", "d1twfa_.r128", "d2phlb1_TFT.r128", "multiquery.r128"])
def test_statistically_consistent_with_reference_host_output(searcher, small_db, golden_dir, job):
    """The reference's `-c` run draws from ONE sequential drand48 stream, which no parallel run can
    replay (its own GPU path does not either).  Against its golden stdout the GPU result must look
    like one more seed of the SAME algorithm: tests/golden/expected/seed_spread.json holds the
    entry-by-entry comparison of every pair of 8 drand48 seeds of the `-c` semantics on five jobs
    (tests/golden/make_seed_spread.py) - the 8-SSE query of BASELINE configs[0] / [1], the 19-SSE query at
    r = 4096 against the stdout the reference recorded in 2013, the 101-SSE query (large-query path), LORDER = F
    with solution maps, and a three-query stream - and the GPU-vs-golden figures must lie inside the measured
    ranges (tests/t3_band.py): fraction of entries that differ within [min - 0.03, max + 0.03], largest
    |difference| at most the largest seen + 2, |mean difference| at most the largest seen + 0.05, rank
    correlation at least the smallest seen - 0.01, and with LSOLN the fraction of identical solution maps."""
    import t3_band
    stdin_file, _, restarts, lorder, lsoln = t3_band.JOBS[job]
    qs = sat.StructSet.read(os.path.join(golden_dir, stdin_file), "query", skip_header_lines=2)
    searcher.upload(small_db)
    searcher.set_queries([(*qs.dense(k), qs.ssetypes(k)) for k in range(len(qs))], 0)
    scores, maps, _ = searcher.search(lorder, lsoln, restarts)
    run_maps = [[t3_band.map_pairs(maps[q, e]) for e in range(len(small_db))] for q in range(len(qs))] if lsoln else None
    t3_band.check(job, small_db.names, scores, run_maps)


# ---------------------------------------------------------------- full benchmark size
def test_full_size_properties():
    """BASELINE configs[2]/[3] scale on one GPU: 100k entries, 32-SSE query, r=128.  The
    oracle cannot run this in test time, so: (a) a random sample of entries is compared
    with the oracle bit for bit, (b) two runs are identical, (c) the planted source entry
    is the top hit, (d) every score is within the bounds the scoring function allows."""
    n = 100_000
    db = sat.synth.make_db(n, 32)
    q = sat.synth.planted_query(db, 54_321, keep=1.0, jitter=0.5)
    n1 = len(q[2])
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_query(*q, 0)
        a, _, ms = s.search(True, False, 128)
        b, _, _ = s.search(True, False, 128)
    assert np.array_equal(a, b)
    assert a.argmax() == 54_321
    assert a.max() <= 2 * n1 * (n1 - 1) // 2 and a.min() >= -2 * n1 * (n1 - 1) // 2
    sample = np.random.default_rng(0).choice(n, 48, replace=False)
    osc, _, _ = oracle_lib.search(db, *q, True, False, 128, entries=sample)
    assert np.array_equal(a[sample], osc)
    print(f"100k x 32-SSE: {ms:.1f} ms -> {n / ms * 1e3:.0f} scorings/s")


# ---------------------------------------------------------------- the hardware fact the launch sizing uses
def test_lds_is_handed_out_in_128_granules_of_1280_bytes():
    """resident_by_lds, which pick_epw and size_workgroup of cuda_satabsearch_amd/csrc/sat_launch.hip size launches
    with, counts resident entries per CU as 128 / ceil(bytes / 1280): the CU hands
    out its 160 KB of LDS in 1280-byte granules.  Measured here with workgroups that count themselves
    in and out (tests/native/lds_residency.hip): the workgroups resident on a CU drop exactly where a
    workgroup needs one more granule or the 128 are used up.  If a driver or firmware changes this, the
    sizing loses throughput (never correctness) and this test says why."""
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "liblds_residency.so"))
    lib.lds_resident_per_cu.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.lds_resident_per_cu.restype = ctypes.c_int
    expect = {(128, 11_520): 14, (128, 11_521): 12,        # 9 granules x 14 = 126 | 10 x 12 = 120
              (128, 12_800): 12, (128, 12_801): 11,        # 10 granules | 11 x 11 = 121
              (128, 14_080): 11, (128, 14_081): 10,        # 11 granules | 12 x 10 = 120
              (256, 26_880): 6, (256, 26_881): 5,          # 21 granules x 6 = 126 | 22 x 5 = 110
              (256, 32_000): 5, (256, 32_001): 4}          # 25 granules x 5 = 125 | 26 x 4 = 104
    got = {k: lib.lds_resident_per_cu(*k) for k in expect}
    assert got == expect


# ---------------------------------------------------------------- the random stream and rocRAND
def test_philox_block_is_rocrands_block():
    """The kernel writes its Philox4x32-10 block out by hand (sat_sa_kernel.hpp, philox_block); the
    claim that it is the block rocRAND's device API returns for rocrand_init(seed, subsequence,
    4 * block) + rocrand4() - and that its uniform conversion is rocrand_uniform's - is checked here on
    the device, both sides in one kernel (tests/native/rocrand_check.hip), for random and edge-case
    (seed, subsequence, block) triples, including the ones the search uses: seed + (query << 32),
    subsequence = db ordinal | restart << 32, block = SSE group or 32 + step pair."""
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "librocrand_check.so"))
    rng = np.random.default_rng(7)
    n = 20_000
    seed = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    sub = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    block = rng.integers(0, 2 ** 30, n, dtype=np.uint64).astype(np.uint32)
    # the search's own addressing
    k = n // 2
    seed[:k] = 1234 + (rng.integers(0, 300, k).astype(np.uint64) << np.uint64(32))
    sub[:k] = rng.integers(0, 1_000_000, k).astype(np.uint64) | (rng.integers(0, 4096, k).astype(np.uint64) << np.uint64(32))
    block[:k] = rng.integers(0, 82, k).astype(np.uint32)
    # edges
    seed[-4:] = [0, 2 ** 64 - 1, 1234, 1234]
    sub[-4:] = [0, 2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32]
    block[-4:] = [0, 2 ** 30 - 1, 0, 81]
    ours = (ctypes.c_uint32 * 4)()
    theirs = (ctypes.c_uint32 * 4)()
    bad = lib.sat_test_philox_vs_rocrand(n, seed.ctypes.data_as(ctypes.c_void_p), sub.ctypes.data_as(ctypes.c_void_p),
                                         block.ctypes.data_as(ctypes.c_void_p), ours, theirs)
    assert bad == 0, f"{bad} of {n} blocks differ from rocRAND's; first: ours {list(ours)} rocRAND {list(theirs)}"


# ---------------------------------------------------------------- multi-GPU entry points (one GPU here)
@pytest.mark.parametrize("gather", ["", "rccl", "peer"], ids=["direct", "rccl", "peer"])
def test_multi_gpu_entry_points_on_one_device(monkeypatch, gather, golden_dir, small_db):
    """sat_multi_*: cost-balanced shards, search on every GPU, ONE gather to device 0.  A box with one
    GPU can only run one shard, but every code path is exercised: SAT_MULTI_GATHER=rccl sends the
    shard through a one-rank RCCL communicator (ncclCommInitAll + ncclGather, the padded fixed-size
    gather and the row re-ordering included), =peer through hipMemcpyPeerAsync; results must equal the
    single-context search bit for bit, with solution maps and for the best-k rows.  (More than one
    GPU: unmeasured on hardware, see DESIGN.md.)"""
    if gather:
        monkeypatch.setenv("SAT_MULTI_GATHER", gather)
    qs = [load_query(golden_dir, "d2phlb1.input"), load_query(golden_dir, "multiquery.input", 0),
          load_query(golden_dir, "multiquery.input", 2)]
    with sat.Searcher(0) as s:
        s.upload(small_db)
        s.set_queries(qs, 3)
        ref, refmaps, _ = s.search(True, True, 64)
        refhits, refhitmaps = s.topk_hits(9, lsoln=True)
    with sat.MultiSearcher(1) as m:
        assert m.ndev == 1 and m.gather_kind == (gather or "none")
        m.upload(small_db)
        assert list(m.shards()) == [0, len(small_db)]
        m.set_queries(qs, 3)
        scores, maps, ms = m.search(True, True, 64)
        assert np.array_equal(scores, ref) and np.array_equal(maps, refmaps)
        hits, hitmaps, _ = m.search_topk(9, True, True, 64)
        assert np.array_equal(hits, refhits) and np.array_equal(hitmaps, refhitmaps)
        plain, none, _ = m.search(True, False, 64)
        assert np.array_equal(plain, ref) and none is None


@pytest.mark.parametrize("nshards", [2, 3, 5])
def test_multi_shard_path_with_several_contexts_on_one_gpu(nshards, golden_dir):
    """The multi-GPU code path with REAL shards on a one-GPU box: an explicit device list that names GPU
    0 several times gives one context per shard (peer-copy gather: RCCL refuses duplicate devices).
    Cost-balanced cuts of a size-sorted database, padded fixed-size gather, rows put back in database
    order, solution maps, and the merge of the per-shard best-k rows: all equal to the one-context search."""
    db = sat.synth.make_db(700, 4, 70, sort=True, seed=31)
    qs = [sat.synth.planted_query(db, 650, keep=0.6), load_query(golden_dir, "d2phlb1.input"), sat.synth.make_query(8)]
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(qs, 2)
        ref, refmaps, _ = s.search(True, True, 64)
        refhits, refhitmaps = s.topk_hits(20, lsoln=True)
    with sat.MultiSearcher(nshards, devices=[0] * nshards) as m:
        assert m.ndev == nshards and m.gather_kind == "peer"
        m.upload(db)
        b = m.shards()
        assert b[0] == 0 and b[-1] == len(db) and (np.diff(b) > 0).all()
        cost = sat.sharding.entry_cost(db.orders)
        shard_cost = [cost[b[g]:b[g + 1]].sum() for g in range(nshards)]
        assert max(shard_cost) / min(shard_cost) < 1.25              # 700 entries: coarse, but far from the 5x of equal counts
        assert len(set(np.diff(b).tolist())) > 1                      # unequal shard lengths: the gather pads
        m.set_queries(qs, 2)
        scores, maps, _ = m.search(True, True, 64)
        assert np.array_equal(scores, ref) and np.array_equal(maps, refmaps)
        hits, hitmaps, _ = m.search_topk(20, True, True, 64)
        assert np.array_equal(hits, refhits) and np.array_equal(hitmaps, refhitmaps)
        plain, _, _ = m.search(True, False, 64)
        assert np.array_equal(plain, ref)
