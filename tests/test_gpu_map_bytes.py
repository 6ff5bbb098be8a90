"""The chain-map byte encoding of the launches with 8-byte cells (entries of up to 32 SSEs; sat_sa_kernel.hpp,
map_bytes_scaled): a map byte holds the byte offset of its cell in a row, l << 3, and 0x04 stands for "unmatched".
Nothing outside the kernel sees it, so every score and every map must still be the oracle's, bit for bit - at the
shapes where the encoding can go wrong: image 31 (byte 0xF8) and the flag where index 32 used to be, several entry
orders below 32 in one upload, both query classes of the rows-in-step score, the dense per-lane loops of LORDER = F,
the match and pair modes' copy-outs, dense maps with few unmatched bytes, and partial waves."""
import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import matches_lib
import oracle_lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def searcher():
    assert sat.device_count() >= 1, "GPU tests need a HIP device (no CPU path exists)"
    s = sat.Searcher(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def db32():
    """(a): 64 entries of exactly 32 SSEs"""
    return sat.synth.make_db(64, 32, 32, seed=411)


@pytest.fixture(scope="module")
def q32():
    return sat.synth.make_query(32, seed=412)


@pytest.fixture(scope="module")
def db_orders():
    """(b): 5, 17 and 31 SSEs in one upload"""
    return sat.synth.make_db(60, orders=[5] * 20 + [17] * 20 + [31] * 20, seed=413)


@pytest.fixture(scope="module")
def ref32(db32, q32):
    """the oracle on (a) at r = 128, LORDER = T, with maps: shared by the plain, the pair-mode and the sanity tests"""
    scores, maps, _ = oracle_lib.search(db32, *q32, True, True, 128)
    return scores, maps


def compare(searcher, db, q, lorder, lsoln, maxstart, ref=None):
    searcher.upload(db)
    searcher.set_query(*q, 0)
    scores, maps, _ = searcher.search(lorder, lsoln, maxstart)
    oscores, omaps = ref if ref is not None else oracle_lib.search(db, *q, lorder, lsoln, maxstart)[:2]
    bad = np.nonzero(scores != oscores)[0]
    assert bad.size == 0, f"{bad.size} score mismatches, first at entries {bad[:5]}: gpu {scores[bad[:5]]} oracle {oscores[bad[:5]]}"
    if lsoln:
        assert np.array_equal(maps, omaps), f"SSE maps differ at entries {np.nonzero((maps != omaps).any(axis=1))[0][:5]}"
    return scores, maps


@pytest.mark.parametrize("lsoln", [False, True])
def test_32_sse_entries_carry_image_31_and_the_flag(searcher, db32, q32, ref32, lsoln):
    """(a) 32-SSE query x 32-SSE entries, r = 128, LORDER = T: the compacted rounds; with LSOLN the decoded maps"""
    _, maps = compare(searcher, db32, q32, True, lsoln, 128, ref32)
    if lsoln:
        n1 = q32[0].shape[0]
        assert (maps[:, :n1] == 31).any() and (maps[:, :n1] == -1).any()      # byte 0xF8 and the flag came back decoded


@pytest.mark.parametrize("lsoln", [False, True])
@pytest.mark.parametrize("n1", [32, 8, 16])
def test_entry_orders_below_32_and_the_small_query_class(searcher, db_orders, n1, lsoln):
    """(b) entries of 5, 17 and 31 SSEs (several order buckets, n2 < 32: the row pitch is no power of two), under the
    32-SSE query and under an 8- and a 16-SSE query (N1P = 16: the initial score walks the rows in step)"""
    compare(searcher, db_orders, sat.synth.make_query(n1, seed=420 + n1), True, lsoln, 128)


def test_lorder_off_takes_the_dense_loops(searcher, db32, q32):
    """(c) LORDER = F: every lane scores its own two rows (move_group), proposals read their own map byte"""
    compare(searcher, db32, q32, False, True, 128)


def test_match_mode_copies_decoded_maps_out(searcher, db32, q32):
    """(d) two matches per entry: the replay pass writes the picked restarts' own-best maps"""
    searcher.upload(db32)
    searcher.set_query(*q32, 0)
    counts, scores, restarts, maps, _ = searcher.search_matches(2, True, 128)
    n1 = q32[0].shape[0]
    for e in range(len(db32)):
        oc, osc, ors, omp = matches_lib.matches(db32, e, q32, True, 128, 2)
        assert counts[0, e] == oc, f"entry {e}: count"
        assert np.array_equal(scores[0, e], osc), f"entry {e}: scores"
        assert np.array_equal(restarts[0, e], ors), f"entry {e}: restarts"
        assert np.array_equal(maps[0, e][:, :n1], omp[:, :n1]), f"entry {e}: maps"


def test_pair_mode_copies_decoded_maps_out(searcher, db32, q32, ref32):
    """(d) the pair mode (the re-scoring of candidates runs on it): score pass and map pass of chosen rows"""
    searcher.upload(db32)
    searcher.set_query(*q32, 0)
    entries = np.random.default_rng(7).permutation(len(db32))[:40].astype(np.int32)
    scores, maps = searcher.search_pairs(np.zeros(len(entries), np.int32), entries, True, True, 128)
    assert np.array_equal(scores, ref32[0][entries])
    assert np.array_equal(maps, ref32[1][entries])


def test_near_copies_of_the_query_give_dense_maps(searcher):
    """(e) every entry a near copy of the query: thinit matches half the SSEs (the rows form of the initial score) and
    the maps end with few unmatched bytes"""
    base = sat.synth.make_db(1, 32, 32, seed=431)
    t, d = base.dense(0)
    db = sat.StructSet.from_dense([32] * 32, [t] * 32, [d] * 32)
    q = sat.synth.planted_query(base, 0, keep=1.0, jitter=0.5)
    scores, maps = compare(searcher, db, q, True, True, 128)
    assert scores.min() > 4 * 32
    assert (maps[:, :32] >= 0).mean() > 0.75


@pytest.mark.parametrize("maxstart", [1, 200])
def test_partial_waves_take_the_uncompacted_path(searcher, db32, q32, maxstart):
    """(f) r = 1 and r = 200: waves with idle lanes score their rows per lane"""
    compare(searcher, db32, q32, True, True, maxstart)
