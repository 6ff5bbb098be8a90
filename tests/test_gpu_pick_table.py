"""The LORDER step of the launches with one-word db sets (entries of up to 32 SSEs) reads its candidate from a rank
table in LDS (sat_sa_kernel.hpp: pos, qbase) instead of stripping `pick` bits off the candidate mask: the candidates
of a window are all the SSEs of the type above the predecessor's image A, so the pick-th is the
(SSEs of the type up to A) + pick -th entry of the type's run.  Every score and every map must stay the oracle's, bit
for bit, where the table can go wrong: deep picks (entries of one type under a short query), a type that is absent,
SSE 31 as the image below the window, entries of one and two SSEs, query SSEs without a counterpart, several entry
orders in one upload under both small query classes, two entry slots side by side in a workgroup (each with a table of
its own), partial waves and lanes that loop over restarts, and the match and pair modes, which share the kernel body."""
import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import matches_lib
import oracle_lib

pytestmark = pytest.mark.gpu

TYPE = 0          # the type the one-type entries and the short query are made of


def retyped(db, new_types):
    """`db` with the SSE types of entry s replaced by new_types(s, types)"""
    tabs, dmats = [], []
    for s in range(len(db)):
        t, d = db.dense(s)
        idx = np.arange(t.shape[0])
        ty = np.asarray(new_types(s, t[idx, idx].copy()), np.uint8)
        t[idx, idx] = ty
        d[idx, idx] = ty.astype(np.float32)
        tabs.append(t)
        dmats.append(d)
    return sat.StructSet.from_dense(db.orders, tabs, dmats)


def query_of_type(n, seed, types):
    t, d, _ = sat.synth.make_query(n, seed=seed)
    ty = np.asarray(types, np.uint8)
    idx = np.arange(n)
    t[idx, idx] = ty
    d[idx, idx] = ty.astype(np.float32)
    return t, d, ty


@pytest.fixture(scope="module")
def searcher():
    assert sat.device_count() >= 1, "GPU tests need a HIP device (no CPU path exists)"
    s = sat.Searcher(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def base16():
    return sat.synth.make_db(16, 32, 32, seed=511)


@pytest.fixture(scope="module")
def db_one_type(base16):
    """(a): 16 entries of 32 SSEs, every SSE of type TYPE - a window holds up to 31 candidates"""
    return retyped(base16, lambda s, ty: np.full_like(ty, TYPE))


@pytest.fixture(scope="module")
def db_type_absent(base16):
    """(b): the same entries without a single SSE of type TYPE"""
    return retyped(base16, lambda s, ty: np.where(ty == TYPE, 1, ty))


@pytest.fixture(scope="module")
def q3():
    return query_of_type(3, 512, [TYPE] * 3)


@pytest.fixture(scope="module")
def q32():
    return sat.synth.make_query(32, seed=513)


@pytest.fixture(scope="module")
def ref_q3(db_one_type, q3):
    """the oracle on (a) under the 3-SSE query at r = 128 with maps: shared by the plain and the pair-mode test"""
    return oracle_lib.search(db_one_type, *q3, True, True, 128)[:2]


def compare(searcher, db, q, lsoln, maxstart, ref=None):
    searcher.upload(db)
    searcher.set_query(*q, 0)
    scores, maps, _ = searcher.search(True, lsoln, maxstart)
    oscores, omaps = ref if ref is not None else oracle_lib.search(db, *q, True, lsoln, maxstart)[:2]
    bad = np.nonzero(scores != oscores)[0]
    assert bad.size == 0, f"{bad.size} score mismatches, first at entries {bad[:5]}: gpu {scores[bad[:5]]} oracle {oscores[bad[:5]]}"
    if lsoln:
        assert np.array_equal(maps, omaps), f"SSE maps differ at entries {np.nonzero((maps != omaps).any(axis=1))[0][:5]}"
    return scores, maps


def test_deep_picks_under_a_short_query(searcher, db_one_type, q3, ref_q3):
    """(a) 3-SSE query of one type x 32-SSE entries of that type, r = 128, LSOLN = T: a pick of 16 and more occurs in
    12 % of the wave-steps (counted with the oracle), where the strip loop never went beyond a few"""
    scores, maps = compare(searcher, db_one_type, q3, True, 128, ref_q3)
    assert (maps[:, :3] >= 16).any()                       # images from deep inside a window came back


def test_one_type_entries_under_the_32_sse_query(searcher, db_one_type, q32):
    """(a) the same entries under a 32-SSE query of mixed types: a query SSE finds all 32 db SSEs or none"""
    compare(searcher, db_one_type, q32, True, 128)


def test_type_absent(searcher, db_type_absent, q3, q32):
    """(b) no db SSE of the query's type: every run of the table is empty, nothing is ever matched"""
    scores, maps = compare(searcher, db_type_absent, q3, True, 128)
    assert (maps[:, :3] == -1).all() and (scores == 0).all()
    compare(searcher, db_type_absent, q32, True, 128)


def test_sse_31_below_the_window(searcher, base16, q32):
    """(b) n2 = 32 where only the last one to three SSEs have the type of the query's last SSE: once SSE 31 is an image
    (A = 31) nothing lies above it, and the index formed from the whole mask is the run's end"""
    rare = int(q32[2][-1])

    def types(s, ty):
        ty = np.where(ty == rare, (rare + 1) & 3, ty)
        ty[31 - s % 3:] = rare                              # SSE 31 alone, or the last two or three
        return ty

    db = retyped(base16, types)
    _, maps = compare(searcher, db, q32, True, 128)
    assert (maps[:, :32] == 31).any()


def test_entries_of_one_and_two_sses(searcher, q3, q32):
    """(b) n2 = 1 and 2: a table of one or two bytes, the rest padding"""
    base = sat.synth.make_db(32, orders=[1] * 16 + [2] * 16, seed=514)
    db = retyped(base, lambda s, ty: np.where(np.arange(ty.size) == s % 2, TYPE, ty))
    compare(searcher, db, q3, True, 128)
    compare(searcher, db, q32, True, 128)


def test_query_sses_without_a_counterpart(searcher, base16):
    """(b) the first three query SSEs are of a type no entry has: steps that move a later SSE before any SSE at or
    below it is mapped (`none`) read the table at an index they do not use"""
    db = retyped(base16, lambda s, ty: np.where(ty == 2, 0, ty))
    _, _, types = sat.synth.make_query(12, seed=515)
    q = query_of_type(12, 515, np.concatenate([[2, 2, 2], np.where(types[3:] == 2, 1, types[3:])]))
    _, maps = compare(searcher, db, q, True, 128)
    assert (maps[:, :3] == -1).all() and (maps[:, 3:12] >= 0).any()


@pytest.mark.parametrize("n1", [32, 16, 8])
def test_mixed_orders_in_one_upload(searcher, n1):
    """(c) entries of 5, 17 and 31 SSEs in one upload (a slot's table is sized for 32 whatever its entry's order), under
    a 32-SSE query and under the small query class"""
    db = sat.synth.make_db(60, orders=[5] * 20 + [17] * 20 + [31] * 20, seed=516)
    compare(searcher, db, sat.synth.make_query(n1, seed=520 + n1), True, 128)


def test_two_entry_slots_per_workgroup(monkeypatch, db_one_type, db_type_absent, q3, q32):
    """(d) two entry slots in a workgroup, one-type and type-absent entries alternating: a slot that read its
    neighbour's table would find candidates where it has none, and none where it has 32"""
    monkeypatch.setenv("SAT_EXP_EPW", "2")
    tabs, dmats = [], []
    for s in range(16):
        for src in (db_one_type, db_type_absent):
            t, d = src.dense(s)
            tabs.append(t)
            dmats.append(d)
    db = sat.StructSet.from_dense([32] * 32, tabs, dmats)
    with sat.Searcher(0) as s2:
        compare(s2, db, q3, True, 128)
        assert "block 2 x " in s2.last_launch_info()
        compare(s2, db, q32, True, 128)
        assert "block 2 x " in s2.last_launch_info()


@pytest.mark.parametrize("maxstart", [1, 100, 300])
def test_restart_counts(searcher, db_one_type, q3, q32, maxstart):
    """(e) r = 1 and 100 (partial waves), r = 300 (256 chains: lanes that run a second restart)"""
    compare(searcher, db_one_type, q3, True, maxstart)
    compare(searcher, db_one_type, q32, True, maxstart)


def test_match_mode(searcher, db_one_type, q3):
    """(f) two matches per entry: the record and replay passes run the same step"""
    searcher.upload(db_one_type)
    searcher.set_query(*q3, 0)
    counts, scores, restarts, maps, _ = searcher.search_matches(2, True, 128)
    for e in range(len(db_one_type)):
        oc, osc, ors, omp = matches_lib.matches(db_one_type, e, q3, True, 128, 2)
        assert counts[0, e] == oc, f"entry {e}: count"
        assert np.array_equal(scores[0, e], osc), f"entry {e}: scores"
        assert np.array_equal(restarts[0, e], ors), f"entry {e}: restarts"
        assert np.array_equal(maps[0, e][:, :3], omp[:, :3]), f"entry {e}: maps"


def test_pair_mode(searcher, db_one_type, q3, ref_q3):
    """(f) the pair mode: score pass and map pass of chosen rows"""
    searcher.upload(db_one_type)
    searcher.set_query(*q3, 0)
    entries = np.random.default_rng(9).permutation(len(db_one_type))[:11].astype(np.int32)
    scores, maps = searcher.search_pairs(np.zeros(len(entries), np.int32), entries, True, True, 128)
    assert np.array_equal(scores, ref_q3[0][entries])
    assert np.array_equal(maps, ref_q3[1][entries])
