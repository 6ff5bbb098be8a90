"""The initial full score of the 32-SSE class with one-word sets, one lane per chain and LSOLN = F walks the wave's
matched pairs in ONE order, dealt to the 64 lanes in equal chunks (sat_sa_body.inc: FS_FLAT; the chunk functions of
sat_sa_kernel.hpp).  The initial score is the base of every score a chain reports, so every score must stay the oracle's,
bit for bit, where the deal can go wrong: full waves of every entry order, a partial wave (the older loop) beside a full
one, waves with fewer pairs than lanes and with none at all, waves on both sides of the ballot that sends dense initial
maps to the rows-in-step form, two entry slots side by side in a workgroup (the sums of a wave live in ITS item table
and nowhere else), and the build with the walk compiled out (-DSAT_FS_FLAT=0: the team walk), which must give the same
bytes.  LORDER = F has no item table (no work compaction, satk::lds_layout) and keeps the team walk: the first version
took the walk there too and wrote its sums past the slot's LDS - into the neighbouring slot of a workgroup with two,
which the single-slot launches of small tests never showed; both LORDER settings run here with two slots as well."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import oracle_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESTARTS = (64, 128, 192, 100)          # one, two and three full waves; at 100 a full wave and a partial one


@pytest.fixture(scope="module")
def searcher():
    assert sat.device_count() >= 1, "GPU tests need a HIP device (no CPU path exists)"
    s = sat.Searcher(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def q32():
    return sat.synth.make_query(32, seed=611)


@pytest.fixture(scope="module")
def db_orders():
    """64 entries of 1..32 SSEs, two of each order"""
    return sat.synth.make_db(64, orders=np.repeat(np.arange(1, 33), 2), seed=612)


ORDINAL = 1000 + 7 * np.arange(64)      # stream keys that are not the entries' positions

_refs = {}


def reference(tag, db, q, lorder, maxstart, ordinal):
    """the oracle's scores, computed once per case and shared"""
    key = (tag, lorder, maxstart)
    if key not in _refs:
        _refs[key] = oracle_lib.search(db, *q, lorder, False, maxstart, db_ordinal=ordinal)[0]
        _refs[key].setflags(write=False)
    return _refs[key]


def compare(searcher, tag, db, q, lorder, maxstart, ordinal=None):
    ordinal = np.arange(len(db)) if ordinal is None else ordinal
    searcher.upload(db, db_ordinal=ordinal)
    searcher.set_query(*q, 0)
    scores, _, _ = searcher.search(lorder, False, maxstart)
    oscores = reference(tag, db, q, lorder, maxstart, ordinal)
    bad = np.nonzero(scores != oscores)[0]
    assert bad.size == 0, f"{bad.size} score mismatches, first at entries {bad[:5]}: gpu {scores[bad[:5]]} oracle {oscores[bad[:5]]}"
    return scores


@pytest.mark.parametrize("maxstart", RESTARTS)
def test_every_entry_order(searcher, db_orders, q32, maxstart):
    """32-SSE query x entries of 1..32 SSEs: full waves at r = 64, 128 and 192; at r = 100 the second wave is partial and
    takes the loop that was there, beside a full one on the walk"""
    compare(searcher, "orders", db_orders, q32, True, maxstart, ORDINAL[:len(db_orders)])
    # the instantiations that hold the walk: <N1P = 32, M2W = 1, QLDS, OPT = 1 (LORDER, one lane per chain, no maps), ...>
    names = re.findall(r"sat_sa_kernel<([^>]*)>", searcher.last_launch_info())
    assert names, searcher.last_launch_info()
    for name in names:
        args = [a.strip() for a in name.split(",")]
        assert (args[0], args[1], args[3]) == ("32", "1", "1"), name


@pytest.mark.parametrize("n1", [17, 32])
def test_fewer_pairs_than_lanes(searcher, n1):
    """entries of 2..4 SSEs: a chain matches at most 4 SSEs and most match fewer than two - most waves hold fewer
    than 64 pairs (chunks of one pair, lanes without any), some none at all"""
    db = sat.synth.make_db(32, orders=np.tile([2, 3, 4, 2], 8), seed=613)
    compare(searcher, f"short{n1}", db, sat.synth.make_query(n1, seed=614 + n1), True, 128)


def matched_per_chain(qtypes, dtypes, ordinal, restarts, seed=1234):
    """matched SSEs of every restart's initial map (thinit, restated from the Philox streams: block i >> 2, word i & 3
    decides query SSE i; the next db SSE of its type; the first failed search ends the map)"""
    out = []
    for r in range(restarts):
        m = j = 0
        stopped = False
        for i0 in range(0, len(qtypes), 4):
            blk = oracle_lib.philox4x32_10((i0 >> 2, 0, ordinal, r), (seed, 0))
            for i in range(i0, min(i0 + 4, len(qtypes))):
                if stopped or blk[i - i0] >= 0x7FFFFFC0:
                    continue
                jj = next((x for x in range(j, len(dtypes)) if dtypes[x] == qtypes[i]), -1)
                stopped = jj < 0
                if not stopped:
                    m, j = m + 1, jj + 1
        out.append(m)
    return out


def test_both_sides_of_the_dense_map_ballot(searcher):
    """a 32-SSE query against 16 near-copies of the structure it was taken from (distances jittered, e of entry e's
    SSEs retyped): thinit matches 9 to 16 SSEs on average, and a wave with one chain of 18 matched SSEs or more scores
    its initial maps by the rows in step, the others by the walk, with up to 136 pairs per chain"""
    base = sat.synth.make_db(1, 32, 32, seed=615)
    q = sat.synth.planted_query(base, 0, keep=1.0)
    t, d = base.dense(0)
    pick, rng = np.random.default_rng(616), np.random.default_rng(618)
    idx = np.arange(32)
    tabs, dmats, sides = [], [], []
    for e in range(16):
        noise = np.tril(rng.uniform(-0.5, 0.5, size=d.shape).astype(np.float32), -1)
        de = np.round(np.abs(d + noise + noise.T), 3).astype(np.float32)
        te = t.copy()
        ty = t[idx, idx].copy()
        sel = pick.choice(32, size=e, replace=False)
        ty[sel] = (ty[sel] + 1) & 3
        te[idx, idx] = ty
        de[idx, idx] = ty.astype(np.float32)
        tabs.append(te)
        dmats.append(de)
        ms = matched_per_chain([int(x) & 3 for x in q[2]], [int(x) & 3 for x in ty], e, 128)
        sides += [max(ms[:64]) >= 18, max(ms[64:]) >= 18]
    assert 8 <= sum(sides) <= 24, sides                          # waves on both sides, by the kernel's own rule
    db = sat.StructSet.from_dense([32] * 16, tabs, dmats)
    scores = compare(searcher, "copies", db, q, True, 128)
    assert scores[0] > 100                                       # the copy is found


def test_no_pairs_anywhere(searcher, db_orders):
    """a query of a type no entry has: nothing is ever matched, every wave deals out nothing"""
    tabs, dmats = [], []
    for s in range(len(db_orders)):
        t, d = db_orders.dense(s)
        idx = np.arange(t.shape[0])
        ty = np.where(t[idx, idx] == 0, 1, t[idx, idx]).astype(np.uint8)
        t[idx, idx] = ty
        d[idx, idx] = ty.astype(np.float32)
        tabs.append(t)
        dmats.append(d)
    db = sat.StructSet.from_dense(db_orders.orders, tabs, dmats)
    t, d, _ = sat.synth.make_query(32, seed=617)
    idx = np.arange(32)
    t[idx, idx] = 0
    d[idx, idx] = 0.0
    scores = compare(searcher, "absent", db, (t, d, np.zeros(32, np.uint8)), True, 128)
    assert (scores == 0).all()


def test_lorder_f(searcher, db_orders, q32):
    """LORDER = F: its static step loops follow the same initial score (by the team walk: no item table there)"""
    compare(searcher, "orders", db_orders, q32, False, 128, ORDINAL[:len(db_orders)])


@pytest.mark.parametrize("lorder", [True, False])
def test_two_entry_slots_per_workgroup(monkeypatch, q32, lorder):
    """the bench launch's shape, two 32-SSE entries per workgroup: whatever a slot's walk writes outside its own carve
    lands in its neighbour's cells or maps"""
    monkeypatch.setenv("SAT_EXP_EPW", "2")
    db = sat.synth.make_db(48, 32, 32, seed=619)
    with sat.Searcher(0) as s2:
        compare(s2, "slots", db, q32, lorder, 128)
        assert "block 2 x " in s2.last_launch_info()


CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import numpy as np
import cuda_satabsearch_amd as sat
db = sat.synth.make_db(64, orders=np.repeat(np.arange(1, 33), 2), seed=612)
out = {}
with sat.Searcher(0) as s:
    s.upload(db, db_ordinal=1000 + 7 * np.arange(64))
    s.set_query(*sat.synth.make_query(32, seed=611), 0)
    for r in %r:
        out[str(r)] = s.search(True, False, r)[0].tolist()
print(json.dumps(out))
"""


def test_the_build_without_the_walk_gives_the_same_bytes(searcher, db_orders, q32):
    """tests/native/libsat_teamwalk.so = the product sources with -DSAT_FS_FLAT=0, loaded by a fresh process: the first
    case's scores, byte for byte"""
    lib = os.path.join(ROOT, "tests", "native", "libsat_teamwalk.so")
    assert os.path.exists(lib), "build with python -m cuda_satabsearch_amd.build --oracle"
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, RESTARTS)], capture_output=True, text=True,
                       env=dict(os.environ, SAT_DEVICE_LIB=lib), timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    other = json.loads(p.stdout.strip().splitlines()[-1])
    searcher.upload(db_orders, db_ordinal=ORDINAL)
    searcher.set_query(*q32, 0)
    for r in RESTARTS:
        scores = searcher.search(True, False, r)[0]
        assert scores.tobytes() == np.asarray(other[str(r)], scores.dtype).tobytes(), f"r = {r}"
