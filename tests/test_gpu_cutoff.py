"""The p-value cutoff on the GPU (-m gpu): sat_hits_cutoff against the filtered sat_topk_hits list at every boundary,
the row cap, the capacity contract and the bytes copied back, a mixed-size database, the multi-GPU merge and the
command line's -p - all byte for byte."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import _native

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
MAXDIM = 111
HIT = 32                                   # sizeof(sat_hit)
SMALL_QUERIES = ("d1ubia_", "d2phlb1", "1qlp_sheetbc", "d1ae6h1", "d1twfa_")


def load_query(golden_dir, name, index=0):
    qs = sat.StructSet.read(os.path.join(golden_dir, name), "query", skip_header_lines=2)
    t, d = qs.dense(index)
    return t, d, qs.ssetypes(index)


def expected(ref, ref_maps, p, k=None):
    """query q's rows: sat_topk_hits(N) without the rows whose p-value exceeds p, cut to k"""
    rows, maps = [], []
    for q in range(ref.shape[0]):
        keep = np.nonzero(ref[q]["pvalue"] <= p)[0]
        if k:
            keep = keep[:k]
        rows.append(ref[q][keep])
        maps.append(ref_maps[q][keep] if ref_maps is not None else None)
    return rows, maps


def assert_rows(got, want, got_maps=None, want_maps=None):
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, f"query {q}: {g.shape} rows, want {w.shape}"
        assert g.tobytes() == w.tobytes(), f"query {q}: rows differ"
        if want_maps is not None:
            assert got_maps[q].dtype == np.int32 and got_maps[q].shape == (len(w), MAXDIM)
            assert np.array_equal(got_maps[q], want_maps[q]), f"query {q}: maps differ"


@pytest.fixture(scope="module")
def small_db(golden_dir):
    return sat.StructSet.read(os.path.join(golden_dir, "tableauxdistmatrixdb.small.ascii"))


@pytest.fixture(scope="module")
def small_searcher(golden_dir, small_db):
    assert sat.device_count() >= 1, "GPU tests need a HIP device (no CPU path exists)"
    s = sat.Searcher(0)
    s.upload(small_db)
    s.set_queries([load_query(golden_dir, n + ".input") for n in SMALL_QUERIES])
    yield s
    s.close()


# ---------------------------------------------------------------- 1. the filtered sat_topk_hits list, every boundary
@pytest.mark.parametrize("lsoln", [True, False])
def test_cutoff_is_the_filtered_topk_list(small_searcher, small_db, lsoln):
    s, n = small_searcher, len(small_db)
    s.search(True, lsoln, 128)
    ref = s.topk_hits(n, lsoln=lsoln)
    ref, ref_maps = ref if lsoln else (ref, None)
    distinct = np.unique(ref["pvalue"])
    assert len(distinct) > 3
    cuts = {0.0, 1e-12, 0.05, 1.0}
    for p in distinct:
        cuts.update({float(p), float(np.nextafter(p, 0.0))})
    for p in sorted(cuts):
        got = s.hits_cutoff(p, lsoln=lsoln)
        got, got_maps = got if lsoln else (got, None)
        want, want_maps = expected(ref, ref_maps, p)
        assert_rows(got, want, got_maps, want_maps if lsoln else None)
    # p >= 1: every row, sat_topk_hits(N) itself
    got = s.hits_cutoff(1.0, lsoln=lsoln)
    rows = got[0] if lsoln else got
    assert np.concatenate(rows).tobytes() == ref.tobytes()


def test_row_cap_gives_the_prefixes(small_searcher, small_db):
    s, n = small_searcher, len(small_db)
    s.search(True, True, 128)
    ref, ref_maps = s.topk_hits(n, lsoln=True)
    for p in (0.0, 0.05, 1.0):
        for k in (1, 3, n + 5):
            got, got_maps = s.hits_cutoff(p, k=k, lsoln=True)
            want, want_maps = expected(ref, ref_maps, p, k)
            assert_rows(got, want, got_maps, want_maps)
            assert all(len(g) <= k for g in got)


# ---------------------------------------------------------------- 2. the capacity contract and the bytes copied back
def test_capacity_contract(small_searcher, small_db):
    s, n, nq = small_searcher, len(small_db), len(SMALL_QUERIES)
    lib = _native.device_lib()
    s.search(True, True, 128)
    info = s.last_launch_info()
    ref, ref_maps = s.topk_hits(n, lsoln=True)
    p = 0.05
    want, want_maps = expected(ref, ref_maps, p)
    want_counts = np.array([len(w) for w in want], np.int32)
    total = int(want_counts.sum())
    assert total > 1
    counts = np.full(nq, -7, np.int32)

    # short capacity: T returned, counts written, the rows untouched; only the counts crossed
    hits = np.frombuffer(b"\xab" * (HIT * (total - 1)), np.uint8).copy()
    maps = np.full((total - 1) * MAXDIM, 0x5a5a5a5a, np.int32)
    before = s.d2h_bytes()
    r = lib.sat_hits_cutoff(s._ctx, p, 0, counts.ctypes.data, total - 1, hits.ctypes.data, maps.ctypes.data)
    assert r == total
    assert np.array_equal(counts, want_counts)
    assert (hits == 0xab).all() and (maps == 0x5a5a5a5a).all()
    assert s.d2h_bytes() - before == 4 * nq

    # no buffer at all
    counts[:] = -7
    before = s.d2h_bytes()
    assert lib.sat_hits_cutoff(s._ctx, p, 0, counts.ctypes.data, 0, None, None) == total
    assert np.array_equal(counts, want_counts)
    assert s.d2h_bytes() - before == 4 * nq

    # capacity T: the rows, and exactly 4 nq + 32 T + 444 T bytes
    for with_maps in (True, False):
        rows = np.zeros(total, sat.search._HIT_DTYPE)
        rmaps = np.full((total, MAXDIM), -1, np.int32)
        before = s.d2h_bytes()
        r = lib.sat_hits_cutoff(s._ctx, p, 0, counts.ctypes.data, total, rows.ctypes.data,
                                rmaps.ctypes.data if with_maps else None)
        assert r == total
        assert s.d2h_bytes() - before == 4 * nq + HIT * total + (4 * MAXDIM * total if with_maps else 0)
        assert rows.tobytes() == np.concatenate(want).tobytes()
        if with_maps:
            assert np.array_equal(rmaps, np.concatenate(want_maps))

    # another cutoff from the same search: no search ran, and it equals a fresh search's
    again = s.hits_cutoff(1e-3, lsoln=True)
    assert s.last_launch_info() == info
    s.search(True, True, 128)
    fresh = s.hits_cutoff(1e-3, lsoln=True)
    assert_rows(again[0], fresh[0], again[1], fresh[1])


def test_argument_checks(small_searcher, golden_dir, small_db):
    s, nq = small_searcher, len(SMALL_QUERIES)
    lib = _native.device_lib()
    counts = np.zeros(nq, np.int32)
    s.search(True, False, 128)
    for bad in (float("nan"), float("inf"), -1e-9):
        assert lib.sat_hits_cutoff(s._ctx, bad, 0, counts.ctypes.data, 0, None, None) == -1          # SAT_EINVAL
    assert lib.sat_hits_cutoff(s._ctx, 0.05, 0, None, 0, None, None) == -1
    maps = np.zeros(MAXDIM, np.int32)
    hits = np.zeros(1, sat.search._HIT_DTYPE)
    assert lib.sat_hits_cutoff(s._ctx, 0.05, 0, counts.ctypes.data, 1, hits.ctypes.data, maps.ctypes.data) == -5  # no lsoln
    with sat.Searcher(0) as fresh:
        fresh.upload(small_db)
        fresh.set_queries([load_query(golden_dir, "d1ubia_.input")])
        assert lib.sat_hits_cutoff(fresh._ctx, 0.05, 0, counts.ctypes.data, 0, None, None) == -5    # no search yet


# ---------------------------------------------------------------- 3. a mixed database with planted copies
def _append(db, extra):
    return sat.StructSet(np.concatenate([db.orders, extra.orders]).astype(np.int32), list(db.names) + list(extra.names),
                         np.concatenate([db.cell_off, extra.cell_off + len(db.tab)]).astype(np.int64),
                         np.concatenate([db.tab, extra.tab]), np.concatenate([db.dist, extra.dist]))


def _jittered(q, seed):
    t, d, ty = q
    rng = np.random.default_rng(seed)
    m = t.shape[0]
    noise = np.tril(rng.uniform(-0.3, 0.3, size=(m, m)).astype(np.float32), -1)
    d2 = np.round(np.abs(d + noise + noise.T), 3).astype(np.float32)
    d2[np.arange(m), np.arange(m)] = d[np.arange(m), np.arange(m)]
    return t, d2


def test_mixed_database_with_planted_copies(golden_dir):
    base = sat.synth.make_db(20_000 - 6, 8, 96, sort=False, seed=4242)
    queries = [sat.synth.make_query(8, seed=801), sat.synth.make_query(32, seed=3201),
               load_query(golden_dir, "d1twfa_.input")]
    assert [q[0].shape[0] for q in queries] == [8, 32, 101]
    # two near-copies of every query, in the middle of the database
    planted = []
    for i, q in enumerate(queries):
        for j in range(2):
            planted.append(_jittered(q, 10 * i + j))
    pad = max(q[0].shape[0] for q in queries)
    tabs = np.zeros((len(planted), pad, pad), np.uint8)
    dmats = np.zeros((len(planted), pad, pad), np.float32)
    for i, (t, d) in enumerate(planted):
        m = t.shape[0]
        tabs[i, :m, :m], dmats[i, :m, :m] = t, d
    extra = sat.StructSet.from_dense(np.array([t.shape[0] for t, _ in planted], np.int32), tabs, dmats,
                                     ["planted%d" % i for i in range(len(planted))])
    half = len(base) // 2
    db = _append(_append(base.subset(np.arange(half)), extra), base.subset(np.arange(half, len(base))))
    assert len(db) == 20_000
    copies = {qi: [half + 2 * qi, half + 2 * qi + 1] for qi in range(3)}
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries)
        s.search(True, True, 128)
        ref, ref_maps = s.topk_hits(len(db), lsoln=True)
        for p in (1e-6, 1e-3, 1.0):
            got, got_maps = s.hits_cutoff(p, lsoln=True)
            want, want_maps = expected(ref, ref_maps, p)
            assert_rows(got, want, got_maps, want_maps)
            if p == 1e-6:
                for qi in range(3):
                    assert set(copies[qi]) <= set(int(e) for e in got[qi]["entry"]), f"query {qi}: planted copies missing"
        got = s.hits_cutoff(1e-6, k=1)
        assert [len(g) for g in got] == [1, 1, 1]


# ---------------------------------------------------------------- 4. multi-GPU: three shards on one GPU
def test_multi_cutoff_equals_one_context(golden_dir):
    db = sat.synth.make_db(700, 4, 70, sort=True, seed=31)
    qs = [sat.synth.planted_query(db, 650, keep=0.6), load_query(golden_dir, "d2phlb1.input"),
          sat.synth.planted_query(db, 230, keep=0.7)]
    cases = [(p, k) for p in (1e-3, 0.05, 1.0) for k in (None, 3)]
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(qs, 2)
        s.search(True, True, 64)
        ref = {c: s.hits_cutoff(c[0], k=c[1], lsoln=True) for c in cases}
    lib = _native.device_lib()
    with sat.MultiSearcher(3, devices=[0, 0, 0]) as m:
        m.upload(db)
        m.set_queries(qs, 2)
        begin = m.shards()
        for c in cases:
            rows, maps, _ = m.search_cutoff(c[0], k=c[1], lorder=True, lsoln=True, maxstart=64)
            assert_rows(rows, ref[c][0], maps, ref[c][1])
        # the rows straddle the shard edges
        shard = np.searchsorted(np.asarray(begin[1:-1]), np.concatenate(ref[(1.0, None)][0])["entry"], side="right")
        assert len(np.unique(shard)) == 3
        # a short capacity: the counts, then the rows from every shard's last search
        counts = np.zeros(3, np.int32)
        ms = C.c_double(0.0)
        total = sum(len(r) for r in ref[(0.05, None)][0])
        one = np.zeros(1, sat.search._HIT_DTYPE)
        r = lib.sat_multi_search_cutoff(m._m, 1, 0, 64, 0.05, 0, counts.ctypes.data, 1, one.ctypes.data, None, C.byref(ms))
        assert r == total and one.tobytes() == bytes(HIT)
        assert list(counts) == [len(x) for x in ref[(0.05, None)][0]]
        before = m.d2h_bytes()
        rows = np.zeros(total, sat.search._HIT_DTYPE)
        assert lib.sat_multi_hits_cutoff(m._m, 0.05, 0, counts.ctypes.data, total, rows.ctypes.data, None) == total
        assert rows.tobytes() == np.concatenate(ref[(0.05, None)][0]).tobytes()
        # per shard: its counts and its own rows, nothing proportional to the database
        assert m.d2h_bytes() - before < 3 * 4 * 3 + HIT * total * 3
        again = m.hits_cutoff(0.05, lsoln=False)
        assert_rows(again, ref[(0.05, None)][0])


# ---------------------------------------------------------------- 5. the command line
ROW = re.compile(r"^\S+ +-?\d+ \S+ \S+ +(\S+)\n$")


def _pvalues_of_the_table():
    h = _native.host_lib()
    return [h.sat_pv_gumbel(h.sat_z_gumbel_trunc(float(x))) for x in range(-128, 128)]


def _filter(text, p, k=None):
    """-k output with the rows whose p-value is above p (and their map lines) removed, each query cut to k rows"""
    out, keep, kept = [], True, 0
    for line in text.splitlines(keepends=True):
        if line.startswith("#"):
            out.append(line)
            if line.startswith("# cudaSaTabsearch"):
                kept = 0
            continue
        m = ROW.match(line)
        if m:
            keep = float(m.group(1)) <= p and (k is None or kept < k)
            kept += keep
        if keep:
            out.append(line)
    return "".join(out)


def _copied(stderr):
    return int(re.search(rb"copied (\d+) bytes", stderr).group(1))


@pytest.mark.parametrize("name", ["d2phlb1_TTT", "multiquery", "qmode", "mixed"])
def test_cli_cutoff(golden_dir, tmp_path, name):
    cwd, args = golden_dir, []
    if name == "qmode":
        stdin = open(os.path.join(golden_dir, "qmode_sids.txt"), "rb").read()
        args = ["-q", "tableauxdistmatrixdb.small.ascii"]
    elif name == "mixed":
        # both size classes, inline LSOLN queries: one query from each class
        db = sat.synth.make_db(60, 70, 111, sort=False, seed=11)
        sat.synth.write_ascii(db, tmp_path / "mix.ascii")
        db.subset([int(np.argmax(db.orders <= 96)), int(np.argmax(db.orders > 96))]).write_ascii(tmp_path / "q.body")
        stdin, cwd = b"mix.ascii\nT T T\n" + (tmp_path / "q.body").read_bytes(), str(tmp_path)
    else:
        stdin = open(os.path.join(golden_dir, name + ".input"), "rb").read()

    def run(*extra):
        p = subprocess.run([CLI, *args, *extra], input=stdin, cwd=cwd, capture_output=True)
        assert p.returncode == 0, p.stderr.decode()[-400:]
        return p

    full = run("-k", "1000000")
    text = full.stdout.decode()
    assert text.count("\n") > 100
    table = _pvalues_of_the_table()
    for cut in (1e-3, 0.05):
        # away from every p-value a row can have: the %g text filters exactly as the double does
        assert all(abs(v - cut) > 1e-4 * cut for v in table)
        p = run("-p", repr(cut))
        assert p.stdout.decode() == _filter(text, cut)
        assert _copied(p.stderr) < _copied(full.stderr)
    assert any(ROW.match(l) for l in _filter(text, 1e-3).splitlines(keepends=True)), "nothing qualifies at 1e-3"
    assert run("-p", "1").stdout == full.stdout
    assert run("-p", "0.05", "-k", "3").stdout.decode() == _filter(text, 0.05, 3)
    assert run("-p", "0.05", "-G", "0,0").stdout == run("-p", "0.05").stdout
