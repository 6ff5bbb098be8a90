"""Fitted Gumbel statistics on the GPU (-m gpu): the device histogram against the host's, planted scores at every edge
of the binning, sat_stats_fit / sat_stats_set through every row path (best-k rows, the p-value cutoff), the life of a
fit, three shards on one GPU, and the command line's -F with -k / -p / -M - all byte for byte.

2 500 entries are no multiple of a histogram block's or a cutoff block's rows, and the queries of 8, 19 and 101 SSEs
lie in three size classes."""
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import _native
from cuda_satabsearch_amd.search import _HIT_DTYPE
from select_lib import expected_rows, fit_table, host_fits, host_histogram

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
BINS, PER_UNIT, MAXDIM = 4096, 256, 111
GUMBEL_A, GUMBEL_B = 0.3780327676087335, 0.3582596175507505
N1S = (8, 19, 101)
R = 8


@pytest.fixture(scope="module")
def db():
    return sat.synth.make_db(2500, 4, 40)


@pytest.fixture(scope="module")
def queries():
    return [sat.synth.make_query(n1, seed=100 + n1) for n1 in N1S]


@pytest.fixture(scope="module")
def searcher(db, queries):
    assert sat.device_count() >= 1, "GPU tests need a HIP device (no CPU path exists)"
    s = sat.Searcher(0)
    s.upload(db)
    s.set_queries(queries)
    yield s
    s.close()


def planted(db, rng):
    """scores [3][N] that reach what no search produces on demand: negatives, zeros, exact bin edges, the first
    overflowing score of several entries, and (query 2) one bin hit by every row"""
    n = len(db)
    tot = [n1 + db.orders.astype(np.int64) for n1 in N1S]
    sc = np.zeros((3, n), np.int64)
    sc[0] = rng.integers(0, 40, n)
    sc[0][::7] = -rng.integers(1, 9, len(sc[0][::7]))                 # negatives
    sc[0][3::11] = 0
    sc[0][5::13] = tot[0][5::13] * 3                                  # norm2 = 6: an exact bin edge
    sc[0][6::17] = tot[0][6::17]                                      # norm2 = 2
    first_over = -(-(BINS - 1) * tot[0] // 512)                       # smallest score of the overflow bin
    sc[0][8::19] = first_over[8::19]
    sc[0][9::19] = first_over[9::19] - 1                              # ... and the largest below it
    sc[1] = rng.integers(0, 25, n)
    sc[1][::5] = tot[1][::5] // 2                                     # norm2 just under or at 1
    sc[1][1::29] = 12210                                              # the largest legal score: overflow
    sc[2] = tot[2]                                                    # norm2 = 2, bin 512, for every row
    assert ((512 * sc[2]) // tot[2] == 2 * PER_UNIT).all()
    return sc.astype(np.int32)


# ---------------------------------------------------------------- 1. the histogram
@pytest.mark.parametrize("lorder", [True, False])
def test_device_histogram_equals_host_histogram(searcher, db, lorder):
    s = searcher
    s.search(lorder, False, R)
    scores, _ = s.results()
    before = s.d2h_bytes()
    counts, below = s.score_histogram()
    assert s.d2h_bytes() - before == 3 * (BINS + 1) * 4
    want, want_below = host_histogram(scores, N1S, db.orders)
    assert np.array_equal(counts, want) and np.array_equal(below, want_below)
    assert (counts.sum(axis=1) + below == len(db)).all()
    assert ((counts > 0).sum(axis=1) >= 2).all()


def test_planted_scores_reach_every_edge_of_the_binning(searcher, db):
    s = searcher
    s.search(True, False, R)
    sc = planted(db, np.random.default_rng(3))
    s.debug_set_scores(sc)
    got, _ = s.results()
    assert np.array_equal(got, sc)
    counts, below = s.score_histogram()
    want, want_below = host_histogram(sc, N1S, db.orders)
    assert np.array_equal(counts, want) and np.array_equal(below, want_below)
    assert below[0] > 0 and below[1] == 0 and counts[0][0] > 0 and counts[0][6 * PER_UNIT] > 0 and counts[0][2 * PER_UNIT] > 0
    assert counts[0][BINS - 1] > 0 and counts[1][BINS - 1] > 0
    assert counts[2][2 * PER_UNIT] == len(db) and counts[2].sum() == len(db)


# ---------------------------------------------------------------- 2. the fit through every row path
@pytest.mark.parametrize("lsoln", [True, False])
def test_fit_statistics_and_the_rows_it_gives(searcher, db, lsoln):
    s, n = searcher, len(db)
    s.search(True, lsoln, R)
    scores, _ = s.results(False)
    plain = s.topk_hits(50, lsoln=lsoln)
    plain, plain_maps = plain if lsoln else (plain, None)
    counts, below = s.score_histogram()
    fits = s.fit_statistics(0.01)
    want_fits = host_fits(counts, below, 0.01)
    assert fits.tobytes() == want_fits.tobytes()
    assert fits["fitted"].all() and (fits["censored"] > 0).all() and (fits["censored"] <= 25).all()
    want = expected_rows(scores, N1S, db.orders, fits)
    got = s.topk_hits(50, lsoln=lsoln)
    got, got_maps = got if lsoln else (got, None)
    for f in ("entry", "score", "norm2"):
        assert np.array_equal(got[f], plain[f])
    if lsoln:
        assert np.array_equal(got_maps, plain_maps)
    for q in range(3):
        assert got[q].tobytes() == want[q][:50].tobytes(), f"query {q}"
    assert not np.array_equal(got["pvalue"], plain["pvalue"])
    # the cutoff: P between two occupied bins' p-values of query 0
    pv = np.unique(want[0]["pvalue"])
    assert len(pv) > 4
    P = float((pv[len(pv) // 2 - 1] + pv[len(pv) // 2]) / 2)
    rows = s.hits_cutoff(P, lsoln=lsoln)
    rows, maps = rows if lsoln else (rows, None)
    full = s.topk_hits(n, lsoln=lsoln)
    full, full_maps = full if lsoln else (full, None)
    for q in range(3):
        keep = np.nonzero(want[q]["pvalue"] <= P)[0]
        assert rows[q].tobytes() == want[q][keep].tobytes(), f"query {q}"
        assert full[q].tobytes() == want[q].tobytes()
        if lsoln:
            assert np.array_equal(maps[q], full_maps[q][keep])
    assert 0 < len(rows[0]) < n
    # counts only, with a short capacity
    lib = _native.device_lib()
    c = np.zeros(3, np.int32)
    one = np.zeros(1, _HIT_DTYPE)
    total = lib.sat_hits_cutoff(s._ctx, P, 0, c.ctypes.data, 1, one.ctypes.data, None)
    assert total == sum(len(r) for r in rows) and list(c) == [len(r) for r in rows] and one.tobytes() == bytes(32)


# ---------------------------------------------------------------- 3. the life of a fit
def test_a_fit_is_dropped_with_the_scores_it_was_made_from(searcher, db):
    s = searcher
    s.search(True, False, R)
    plain = s.topk_hits(40)
    fits = s.fit_statistics(0.0)
    assert fits["fitted"].all() and not np.array_equal(s.topk_hits(40)["pvalue"], plain["pvalue"])
    s.set_statistics(None)
    assert s.topk_hits(40).tobytes() == plain.tobytes()
    s.set_statistics(fits)
    fitted = s.topk_hits(40)
    assert fitted.tobytes() != plain.tobytes()
    s.search_pairs([0, 1], [3, 4], True, False, R)                     # a pair search keeps it
    assert s.topk_hits(40).tobytes() == fitted.tobytes()
    s.search(True, False, R)                                           # a new search drops it
    assert s.topk_hits(40).tobytes() == plain.tobytes()
    # a query whose scores leave one occupied bin has no fit and keeps the built-in rows
    sc = planted(db, np.random.default_rng(5))
    s.debug_set_scores(sc)
    builtin = s.topk_hits(len(db))
    fits = s.fit_statistics(0.01)
    assert list(fits["fitted"]) == [1, 1, 0]
    assert (fits[2]["a"], fits[2]["b"]) == (GUMBEL_A, GUMBEL_B) and fits[2]["rows"] == len(db)
    assert fits[0]["below"] == int((sc[0] < 0).sum())
    after = s.topk_hits(len(db))
    assert after[2].tobytes() == builtin[2].tobytes()
    want = expected_rows(sc, N1S, db.orders, fits)
    for q in range(3):
        assert after[q].tobytes() == want[q].tobytes(), f"query {q}"      # negative scores use bin 0
    # parameters that cannot be used are refused, and nothing is installed
    bad = fits.copy()
    bad[0]["b"] = 0.0
    with pytest.raises(sat.SatError):
        s.set_statistics(bad)
    with pytest.raises(sat.SatError):
        s.fit_statistics(0.6)


def test_builtin_constants_installed_as_a_fit(searcher, db):
    s, n = searcher, len(db)
    s.search(True, False, R)
    sc, _ = s.results()
    sc = sc.copy()
    for q, n1 in enumerate(N1S):
        sc[q][q::9] = (n1 + db.orders[q::9]) * (1 + q)                 # norm2 = 2, 4, 6 exactly
    s.debug_set_scores(sc)
    plain = s.topk_hits(n)
    s.set_statistics([(GUMBEL_A, GUMBEL_B)] * 3)
    ranked = s.topk_hits(n)
    rows = s.hits_cutoff(1.0)
    exact = 0
    for q in range(3):
        assert len(rows[q]) == n and rows[q].tobytes() == ranked[q].tobytes()
        at_int = ranked[q]["norm2"] == np.floor(ranked[q]["norm2"])
        exact += int(at_int.sum())
        assert ranked[q][at_int].tobytes() == plain[q][at_int].tobytes()
        assert (ranked[q]["pvalue"] <= plain[q]["pvalue"]).all()       # 1/256 steps under the built-ins' steps of 1
    assert exact >= 3 * (n // 9)


# ---------------------------------------------------------------- 4. shards
def test_search_fit_is_the_same_for_any_sharding(db, queries):
    ref = None
    for ndev in (1, 2, 3):
        with sat.MultiSearcher(ndev, devices=[0] * ndev) as m:
            m.upload(db)
            m.set_queries(queries)
            before = m.d2h_bytes()
            fits, _ = m.search_fit(0.01, lorder=True, lsoln=False, maxstart=R)
            assert m.d2h_bytes() - before == ndev * 3 * (BINS + 1) * 4
            counts, below = m.score_histogram()
            rows = m.hits_cutoff(0.05)
            best = m.hits_cutoff(1.0, k=7)
            got = (fits.tobytes(), counts.tobytes(), below.tobytes(), [r.tobytes() for r in rows], [r.tobytes() for r in best])
            assert fits["fitted"].all() and [len(r) for r in best] == [7, 7, 7]
            m.set_statistics(None)
            assert [r.tobytes() for r in m.hits_cutoff(1.0, k=7)] != got[4]
        if ref is None:
            ref = got
        assert got == ref, f"{ndev} shards"
    with sat.Searcher(0) as s:                                          # ... and one plain context
        s.upload(db)
        s.set_queries(queries)
        s.search(True, False, R)
        assert s.fit_statistics(0.01).tobytes() == ref[0]
        assert [r.tobytes() for r in s.hits_cutoff(0.05)] == ref[3]


# ---------------------------------------------------------------- 5. the command line
MULTI_N1 = (8, 13, 101)                                                  # multiquery.input: D1UBIA_, D1AE6H1, d1twfa_


def blocks_of(stdout):
    blocks = []
    for line in stdout.split(b"\n")[:-1]:
        if line.startswith(b"# cudaSaTabsearch"):
            blocks.append(([], []))
        (blocks[-1][0] if line.startswith(b"#") else blocks[-1][1]).append(line)
    return blocks


@pytest.fixture(scope="module")
def cli(golden_dir):
    stdin = open(os.path.join(golden_dir, "multiquery.input"), "rb").read()
    cache = {}

    def run(*args):
        if args not in cache:
            # (64 restarts: at 16 none of the three queries' five best rows has a second, disjoint match; from 64 on the
            # same random streams give three of them one - tests/matches_lib.py on the CPU says which)
            p = subprocess.run([CLI, "-r", "64", *args], input=stdin, cwd=golden_dir, capture_output=True)
            assert p.returncode == 0, p.stderr.decode()[-400:]
            cache[args] = p.stdout
        return cache[args]
    return run


def ranked(rows, k=None, pmax=None):
    """a listing block's rows as -k prints them: by descending score, ties in database order"""
    order = sorted(range(len(rows)), key=lambda i: (-int(rows[i].split()[1]), i))
    out = [rows[i] for i in order if pmax is None or float(rows[i].split()[4]) <= pmax]
    return out[:k] if k else out


@pytest.mark.parametrize("censor", ["0.01", "0"])
def test_cli_listing_carries_each_querys_fit(cli, censor):
    plain, fitted = blocks_of(cli()), blocks_of(cli("-F", censor))
    assert len(plain) == len(fitted) == 3
    heads = []
    for (h0, r0), (h1, r1) in zip(plain, fitted):
        assert h1[:3] == h0 and len(h1) == 4 and h1[3].startswith(b"# GUMBEL a = ")
        heads.append(h1[3])
        assert [r.rsplit(b" ", 2)[0] for r in r1] == [r.rsplit(b" ", 2)[0] for r in r0]
        assert len({r.split()[4] for r in r1 if int(float(r.split()[2])) == 0}) >= 2
    assert len(set(heads)) == 3


def test_cli_best_k_rows_under_a_fit(cli):
    listing, top = blocks_of(cli("-F", "0.01")), blocks_of(cli("-F", "0.01", "-k", "10"))
    for (h, rows), (hk, rk) in zip(listing, top):
        assert hk == h and rk == ranked(rows, 10)
    assert cli("-F", "0.01", "-k", "10", "-G", "0,0") == cli("-F", "0.01", "-k", "10")


def test_cli_cutoff_under_a_fit(cli):
    listing = blocks_of(cli("-F", "0.01"))
    # a cutoff away from every p-value printed: the %g text then filters exactly as the double does
    pv = sorted({float(r.split()[4]) for r in listing[0][1]})
    gaps = [(b / a, (a + b) / 2) for a, b in zip(pv, pv[1:]) if a > 0 and b < 0.5]
    P = max(gaps)[1]
    assert all(abs(float(r.split()[4]) - P) > 1e-4 * P for _, rows in listing for r in rows)
    cut = blocks_of(cli("-F", "0.01", "-p", repr(P)))
    for (h, rows), (hp, rp) in zip(listing, cut):
        assert hp == h and rp == ranked(rows, pmax=P)
    assert 0 < len(cut[0][1]) < len(listing[0][1])
    assert cli("-F", "0.01", "-p", repr(P), "-G", "0,0") == cli("-F", "0.01", "-p", repr(P))


def test_cli_matches_of_the_printed_rows_under_a_fit(cli, golden_dir):
    small = sat.StructSet.read(os.path.join(golden_dir, "tableauxdistmatrixdb.small.ascii"))
    order_of = {n.encode(): int(o) for n, o in zip(small.names, small.orders)}
    listing, both = blocks_of(cli("-F", "0")), blocks_of(cli("-F", "0", "-k", "5", "-M", "2"))
    seconds = 0
    for (h, rows), (hm, rm), n1 in zip(listing, both, MULTI_N1):
        assert hm == h
        assert [r for r in rm if b":" not in r.split()[0]] == ranked(rows, 5)
        m = re.match(rb"# GUMBEL a = (\S+) b = (\S+) ", h[3])
        z, p = fit_table(float(m.group(1)), float(m.group(2)))
        for r in rm:
            name, score = r.split()[0], int(r.split()[1])
            if not name.endswith(b":2"):
                continue
            seconds += 1
            k = 0 if score < 0 else min((512 * score) // (n1 + order_of[name[:-2]]), BINS - 1)
            assert r.split()[3:] == [b"%g" % z[k], b"%g" % p[k]], r
    assert seconds > 0, "no printed row had a second match"
    assert cli("-F", "0", "-k", "5", "-M", "2", "-G", "0,0") == cli("-F", "0", "-k", "5", "-M", "2")
