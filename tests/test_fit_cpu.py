"""Gumbel statistics fitted to a search's own scores, host side (not gpu): the binning shared with the device, the
host histogram, the censored maximum-likelihood fit of csrc/host/sat_gumbel.c against scipy, its fallbacks, the
per-bin z / p table, and the same code as a stand-alone program under AddressSanitizer + UBSan.

Expected values come from numpy / scipy; the histograms are made of the score columns of committed goldens with the
orders of the 586-entry database."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy import optimize, stats

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_satabsearch_amd", "csrc", "host")
EXPECTED = os.path.join(ROOT, "tests", "golden", "expected")
BINS, PER_UNIT = 4096, 256
GUMBEL_A, GUMBEL_B = 0.3780327676087335, 0.3582596175507505      # sat_gumbel.h
SAT_EINVAL = -1
BOUND = 1e-6          # absolute, on a and b: two independent optimisers agree to 2e-8; the rest is scipy's stopping rule

# golden -> the orders of its query blocks (the queries' SSE counts; None: a SID of the database)
GOLDENS = {
    "d2phlb1.r128.out": [19],
    "d2phlb1_TFT.r128.out": [19],
    "recorded_2013_d2phlb1.r4096.out": [19],
    "multiquery.r128.out": [8, 13, 101],
    "qmode_small.r16.out": [None, None, None],
}


def host():
    return _native.host_lib()


def fit_binned(counts, censor):
    f = _native.Fit()
    counts = np.ascontiguousarray(counts, np.uint32)
    rc = host().sat_gumbel_fit_binned(counts.ctypes.data, float(censor), C.byref(f))
    return rc, f


def golden_blocks(name):
    """[(query id, [(entry name, score)])] of a golden listing (map lines of LSOLN goldens are skipped)"""
    blocks = []
    for line in open(os.path.join(EXPECTED, name)):
        if line.startswith("# QUERY ID ="):
            blocks.append((line.split("=")[1].strip(), []))
        elif not line.startswith("#"):
            f = line.split()
            if len(f) == 5:
                blocks[-1][1].append((f[0], int(f[1])))
    return blocks


@pytest.fixture(scope="module")
def small_db(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, "tableauxdistmatrixdb.small.ascii"))
    return {n: int(o) for n, o in zip(db.names, db.orders)}


@pytest.fixture(scope="module")
def histograms(small_db):
    """{(golden, block): (counts uint32[4096], below)} through numpy"""
    upper = {k.upper(): v for k, v in small_db.items()}
    out = {}
    for name, n1s in GOLDENS.items():
        blocks = golden_blocks(name)
        assert len(blocks) >= len(n1s), name
        for b, n1 in enumerate(n1s):
            qid, rows = blocks[b]
            n1 = upper[qid.upper()] if n1 is None else n1
            # (the 2013 recording split the database into 556 + 30 entries: its first block is fitted, as DESIGN 6g's table has it)
            assert len(rows) == (556 if name.startswith("recorded_2013") else 586)
            s = np.array([r[1] for r in rows], np.int64)
            tot = n1 + np.array([small_db[r[0]] for r in rows], np.int64)
            ok = s >= 0
            bins = np.minimum((512 * s[ok]) // tot[ok], BINS - 1)
            out[(name, b)] = (np.bincount(bins, minlength=BINS).astype(np.uint32), int((~ok).sum()))
    return out


def censoring(counts, censor):
    """(hi, n_c): the highest uncensored bin and the censored rows, by the rule of sat_gumbel.h restated"""
    counts = counts.astype(np.int64)
    n = int(counts.sum())
    n_c = int(counts[BINS - 1])
    limit = max(int(np.floor(censor * n)), n_c)
    hi = BINS - 2
    while hi >= 0 and n_c + counts[hi] <= limit:
        n_c += int(counts[hi])
        hi -= 1
    return hi, n_c


def neg_loglik(theta, counts, hi, n_c):
    a, b = theta[0], np.exp(theta[1])
    k = np.nonzero(counts[:hi + 1])[0]
    t = ((k + 0.5) / PER_UNIT - a) / b
    l = np.sum(counts[k] * (-np.log(b) - t - np.exp(-t)))
    if n_c:
        tc = ((hi + 1) / PER_UNIT - a) / b
        l += n_c * np.log(-np.expm1(-np.exp(-tc)))
    return -l


def score_equations(a, b, counts, hi, n_c):
    """d/da and d/db of the censored log-likelihood"""
    k = np.nonzero(counts[:hi + 1])[0]
    c = counts[k].astype(np.float64)
    t = ((k + 0.5) / PER_UNIT - a) / b
    e = np.exp(-t)
    da = np.sum(c * (1.0 - e)) / b
    db = np.sum(c * (-1.0 + t * (1.0 - e))) / b
    if n_c:
        tc = ((hi + 1) / PER_UNIT - a) / b
        u = np.exp(-tc)
        h = u / np.expm1(u)                       # -d/dt log(1 - exp(-exp(-t)))
        da += n_c * h / b
        db += n_c * h * tc / b
    return da, db


# ---- binning

def test_bin_is_floor_of_norm2_times_256_for_every_size():
    h = host()
    for tot in range(2, 223):
        n1 = tot // 2
        n2 = tot - n1
        first_over = -(-(BINS - 1) * tot // 512)                     # the first score whose bin is the overflow bin
        edges = [(k * tot) // 512 for k in range(0, BINS, 97)]        # around exact bin edges (512 s = k tot)
        sweep = set(range(0, 60)) | {first_over - 1, first_over, first_over + 1, 12210, 1 << 22, (1 << 22) + 5, 2 ** 31 - 1}
        for e in edges:
            sweep |= {e - 1, e, e + 1}
        for s in sorted(x for x in sweep if x >= 0):
            want = min(int(np.floor(2.0 * s / tot * 256)), BINS - 1)
            assert h.sat_stat_bin(s, n1, n2) == want, (s, tot)
        assert h.sat_stat_bin(first_over, n1, n2) == BINS - 1 and h.sat_stat_bin(first_over - 1, n1, n2) < BINS - 1
        for s in (-1, -7, -(2 ** 31)):
            assert h.sat_stat_bin(s, n1, n2) == -1


def test_host_histogram_equals_numpy():
    rng = np.random.default_rng(11)
    n, n1 = 5000, 19
    orders = rng.integers(1, 112, n).astype(np.int32)
    scores = rng.integers(-3, 60, n).astype(np.int32)
    scores[::97] = 0
    scores[5::211] = 4000                                            # overflow
    scores[7::301] = (n1 + orders[7::301]) * 3                       # norm2 = 6 exactly: a bin edge
    counts = np.zeros(BINS, np.uint32)
    below = C.c_int32(0)
    host().sat_stat_histogram(scores.ctypes.data, n, n1, orders.ctypes.data, counts.ctypes.data, C.byref(below))
    ok = scores >= 0
    bins = np.minimum((512 * scores[ok].astype(np.int64)) // (n1 + orders[ok]), BINS - 1)
    assert np.array_equal(counts, np.bincount(bins, minlength=BINS).astype(np.uint32))
    assert below.value == int((~ok).sum()) and counts[BINS - 1] > 0 and counts[6 * PER_UNIT] > 0
    # it ADDS: a second call doubles everything (shards are summed this way)
    host().sat_stat_histogram(scores.ctypes.data, n, n1, orders.ctypes.data, counts.ctypes.data, C.byref(below))
    assert np.array_equal(counts, 2 * np.bincount(bins, minlength=BINS).astype(np.uint32)) and below.value == 2 * int((~ok).sum())


# ---- the fit

CASES = [(name, b) for name, n1s in GOLDENS.items() for b in range(len(n1s))]


@pytest.mark.parametrize("name,block", CASES)
def test_plain_mle_agrees_with_scipy(histograms, name, block):
    counts, _ = histograms[(name, block)]
    rc, f = fit_binned(counts, 0.0)
    assert rc == 0 and f.fitted == 1
    hi, n_c = censoring(counts, 0.0)
    assert f.rows == int(counts.sum()) and f.censored == n_c == int(counts[BINS - 1])
    k = np.nonzero(counts[:hi + 1])[0]
    mid = np.repeat((k + 0.5) / PER_UNIT, counts[k])
    a, b = stats.gumbel_r.fit(mid)
    print("%s[%d] censor 0: a %.17g b %.17g  |da| %.3g |db| %.3g" % (name, block, f.a, f.b, abs(f.a - a), abs(f.b - b)))
    assert abs(f.a - a) <= BOUND and abs(f.b - b) <= BOUND
    da, db = score_equations(f.a, f.b, counts, hi, n_c)
    assert abs(da) <= 1e-9 * f.rows and abs(db) <= 1e-9 * f.rows


@pytest.mark.parametrize("censor", [0.01, 0.05])
@pytest.mark.parametrize("name,block", CASES)
def test_censored_mle_agrees_with_scipy_minimize(histograms, name, block, censor):
    counts, _ = histograms[(name, block)]
    rc, f = fit_binned(counts, censor)
    assert rc == 0 and f.fitted == 1
    hi, n_c = censoring(counts, censor)
    assert f.censored == n_c and n_c <= max(int(np.floor(censor * f.rows)), int(counts[BINS - 1]))
    a0, b0 = stats.gumbel_r.fit(np.repeat((np.arange(hi + 1) + 0.5) / PER_UNIT, counts[:hi + 1]))
    r = optimize.minimize(neg_loglik, [a0, np.log(b0)], args=(counts.astype(np.float64), hi, n_c), method="Nelder-Mead",
                          options={"xatol": 1e-11, "fatol": 1e-13, "maxiter": 4000, "maxfev": 8000})
    a, b = r.x[0], np.exp(r.x[1])
    print("%s[%d] censor %g: a %.17g b %.17g  |da| %.3g |db| %.3g" % (name, block, censor, f.a, f.b, abs(f.a - a), abs(f.b - b)))
    assert abs(f.a - a) <= BOUND and abs(f.b - b) <= BOUND
    da, db = score_equations(f.a, f.b, counts, hi, n_c)
    assert abs(da) <= 1e-9 * f.rows and abs(db) <= 1e-9 * f.rows


def test_issue_table_values(histograms):
    """the parameters the histograms of the goldens give, to the three decimals they were reported with"""
    for key, (a, b) in {("d2phlb1.r128.out", 0): (0.471, 0.359), ("recorded_2013_d2phlb1.r4096.out", 0): (0.616, 0.486),
                        ("d2phlb1_TFT.r128.out", 0): (1.059, 0.796), ("multiquery.r128.out", 2): (0.074, 0.058),
                        ("multiquery.r128.out", 1): (0.562, 0.634)}.items():
        rc, f = fit_binned(histograms[key][0], 0.0)
        assert rc == 0 and f.fitted == 1
        assert abs(f.a - a) < 6e-4 and abs(f.b - b) < 6e-4, (key, f.a, f.b)


def one_bin(k, c):
    h = np.zeros(BINS, np.uint32)
    h[k] = c
    return h


def two_bins():
    h = np.zeros(BINS, np.uint32)
    h[100] = h[200] = 500
    return h


@pytest.mark.parametrize("what,counts,censor", [
    ("empty", np.zeros(BINS, np.uint32), 0.0),
    ("one bin", one_bin(300, 586), 0.01),
    ("overflow only", one_bin(BINS - 1, 1000), 0.0),
    ("censor 0.5 leaves one bin", two_bins(), 0.5),
])
def test_fallbacks_keep_the_builtin_constants(what, counts, censor):
    rc, f = fit_binned(counts, censor)
    assert rc == 0 and f.fitted == 0, what
    assert f.a == GUMBEL_A and f.b == GUMBEL_B
    assert f.rows == int(counts.sum())


def test_two_bins_fit_without_censoring():
    rc, f = fit_binned(two_bins(), 0.0)
    assert rc == 0 and f.fitted == 1 and f.censored == 0 and f.b > 0


@pytest.mark.parametrize("censor", [-1e-9, -1.0, 0.5000001, 2.0, float("nan"), float("inf")])
def test_censor_outside_the_range_is_einval(histograms, censor):
    rc, _ = fit_binned(histograms[("d2phlb1.r128.out", 0)][0], censor)
    assert rc == SAT_EINVAL


# ---- the table

def fit_table(a, b):
    z, p = np.empty(BINS), np.empty(BINS)
    host().sat_gumbel_fit_table(float(a), float(b), z.ctypes.data, p.ctypes.data)
    return z, p


@pytest.mark.parametrize("a,b", [(GUMBEL_A, GUMBEL_B), (1.059, 0.796), (0.074, 0.058)])
def test_table_is_monotone_and_p_is_pv_of_z(a, b):
    z, p = fit_table(a, b)
    assert np.all(np.diff(z) > 0) and np.all(np.diff(p) <= 0)
    h = host()
    for k in range(BINS):
        assert np.float64(h.sat_pv_gumbel(float(z[k]))).tobytes() == p[k].tobytes(), k


def test_builtin_table_meets_the_truncated_statistics_at_the_integers():
    z, _ = fit_table(GUMBEL_A, GUMBEL_B)
    for x in range(16):
        assert z[PER_UNIT * x].tobytes() == np.float64(host().sat_z_gumbel_trunc(float(x))).tobytes()


def test_report_stats_fitted():
    z, p = fit_table(0.5, 0.4)
    n2, zz, pp = sat.report.stats_fitted(11, 19, 12, 0.5, 0.4)
    k = (512 * 11) // 31
    assert (n2, zz, pp) == (2.0 * 11 / 31.0, z[k], p[k])
    assert sat.report.stats_fitted(-3, 19, 12, 0.5, 0.4)[1:] == (z[0], p[0])


# ---- the same code under the host sanitizers, as a program of its own

def test_fit_driver_under_sanitizers(histograms, tmp_path):
    src = [os.path.join(ROOT, "tests", "native", "fit_driver.c"), os.path.join(HOST, "sat_gumbel.c")]
    plain, asan = str(tmp_path / "fit_driver"), str(tmp_path / "fit_driver_asan")
    common = ["gcc", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-I", HOST]
    subprocess.run(common + ["-O2", "-o", plain] + src + ["-lm"], check=True)
    subprocess.run(common + ["-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                             "-o", asan] + src + ["-lm"], check=True)
    counts, _ = histograms[("d2phlb1_TFT.r128.out", 0)]
    hist = tmp_path / "hist.txt"
    hist.write_text("".join("%d %d\n" % (k, counts[k]) for k in np.nonzero(counts)[0]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    ref = subprocess.run([plain, str(hist)], capture_output=True, env=env)
    chk = subprocess.run([asan, str(hist)], capture_output=True, env=env)
    err = chk.stderr.decode(errors="replace")
    assert "ERROR: AddressSanitizer" not in err and "runtime error:" not in err and "LeakSanitizer" not in err, err[-3000:]
    assert ref.returncode == 0 and chk.returncode == 0, err[-1000:]
    assert chk.stdout == ref.stdout and b"file censor 0.05: rc 0 fitted 1" in ref.stdout
    out = ref.stdout.decode()
    for what in ("empty", "one bin", "overflow only"):
        assert out.count(what + " censor") == 4 and (what + " censor 0: rc 0 fitted 0") in out
    assert "two bins censor 0.5: rc 0 fitted 0" in out and out.count("bad censor") == 3 and "rc -1" in out
    rc, f = fit_binned(counts, 0.05)
    assert ("file censor 0.05: rc 0 fitted 1 a %.17g b %.17g rows %d censored %d" % (f.a, f.b, f.rows, f.censored)) in out
