"""-F censor on the command line without a GPU: the host mode's listing with statistics fitted to its own scores (the
"# GUMBEL" header line, rows from the query's table), the option checks and the refusals.  The GPU side is
tests/test_gpu_fit.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import stats

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
EXPECTED = os.path.join(ROOT, "tests", "golden", "expected")
BINS, PER_UNIT = 4096, 256
BOUND = 1e-6                                   # as tests/test_fit_cpu.py
GUMBEL = re.compile(rb"^# GUMBEL a = (\S+) b = (\S+) rows = (\d+) censored = (\d+) below = (\d+)$")


def run(golden_dir, args, stdin=b""):
    return subprocess.run([CLI] + args, input=stdin, cwd=golden_dir, capture_output=True)


def blocks_of(stdout):
    """[(header lines, row lines)] of a listing; a block starts at "# cudaSaTabsearch" """
    blocks = []
    for line in stdout.split(b"\n")[:-1]:
        if line.startswith(b"# cudaSaTabsearch"):
            blocks.append(([], []))
        (blocks[-1][0] if line.startswith(b"#") else blocks[-1][1]).append(line)
    return blocks


def fit_table(a, b):
    z, p = np.empty(BINS), np.empty(BINS)
    _native.host_lib().sat_gumbel_fit_table(float(a), float(b), z.ctypes.data, p.ctypes.data)
    return z, p


@pytest.fixture(scope="module")
def db_orders(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, "tableauxdistmatrixdb.small.ascii"))
    return {n.encode(): int(o) for n, o in zip(db.names, db.orders)}


@pytest.mark.parametrize("name,golden", [("d2phlb1", "d2phlb1.r128.out"), ("d2phlb1_TFT", "d2phlb1_TFT.r128.out")])
def test_host_listing_with_fitted_statistics(golden_dir, db_orders, name, golden):
    p = run(golden_dir, ["-c", "-F", "0", "-r", "128"], open(os.path.join(golden_dir, name + ".input"), "rb").read())
    assert p.returncode == 0, p.stderr[-400:]
    (head, rows), = blocks_of(p.stdout)
    (ghead, grows), = blocks_of(open(os.path.join(EXPECTED, golden), "rb").read())
    # three header lines as ever, then the fit; every row keeps name, score and norm2
    assert head[:3] == ghead and len(head) == 4
    m = GUMBEL.match(head[3])
    assert m, head[3]
    entry = [r for r in rows if len(r.split()) == 5]                # (LSOLN map lines have two fields)
    gentry = [r for r in grows if len(r.split()) == 5]
    assert len(entry) == len(gentry) == 586
    assert [r.rsplit(b" ", 2)[0] for r in entry] == [r.rsplit(b" ", 2)[0] for r in gentry]
    assert [r for r in rows if len(r.split()) != 5] == [r for r in grows if len(r.split()) != 5]
    # the printed parameters against scipy on the golden's scores
    n1 = 19
    scores = np.array([int(r.split()[1]) for r in gentry])
    tot = n1 + np.array([db_orders[r.split()[0]] for r in gentry])
    assert (scores >= 0).all()
    bins = np.minimum((512 * scores) // tot, BINS - 1)
    a, b = stats.gumbel_r.fit((bins[bins < BINS - 1] + 0.5) / PER_UNIT)
    pa, pb = float(m.group(1)), float(m.group(2))
    assert abs(pa - a) <= BOUND and abs(pb - b) <= BOUND
    assert (int(m.group(3)), int(m.group(4)), int(m.group(5))) == (586, int((bins == BINS - 1).sum()), 0)
    # every row's z and p: the table of the PRINTED a, b at the row's bin
    z, pv = fit_table(pa, pb)
    for r, k in zip(entry, bins):
        assert r.split()[3:] == [b"%g" % z[k], b"%g" % pv[k]], r
    # not the built-in statistics: rows the int-truncated table cannot tell apart differ here
    low = {r.split()[4] for r in entry if int(float(r.split()[2])) == 0}
    assert len(low) >= 2


def test_query_list_gets_one_fit_per_block(golden_dir):
    sids = open(os.path.join(golden_dir, "qmode_sids.txt"), "rb").read()
    p = run(golden_dir, ["-c", "-r", "16", "-q", "tableauxdistmatrixdb.small.ascii", "-F", "0.01"], sids)
    assert p.returncode == 0, p.stderr[-400:]
    blocks = blocks_of(p.stdout)
    gblocks = blocks_of(open(os.path.join(EXPECTED, "qmode_small.r16.out"), "rb").read())
    assert len(blocks) == len(gblocks) == len(sids.split())
    params = []
    for (head, rows), (ghead, grows) in zip(blocks, gblocks):
        assert head[:3] == ghead and len(head) == 4
        m = GUMBEL.match(head[3])
        assert m, head[3]
        params.append((m.group(1), m.group(2)))
        assert int(m.group(3)) == 586 and 0 < int(m.group(4)) <= 5          # floor(0.01 * 586) = 5
        assert [r.rsplit(b" ", 2)[0] for r in rows] == [r.rsplit(b" ", 2)[0] for r in grows]
        z, pv = fit_table(float(m.group(1)), float(m.group(2)))
        texts = {(b"%g" % z[k], b"%g" % pv[k]) for k in range(BINS)}
        assert all(tuple(r.split()[3:]) in texts for r in rows)
    assert len(set(params)) == len(params)                                   # each block its own parameters


def assert_refused_early(p, message):
    assert p.returncode == 1, p.stderr
    assert message in p.stderr, p.stderr
    assert p.stdout == b""
    assert b"MAXDIM" not in p.stderr and b"HIP device" not in p.stderr


def test_usage_lists_the_fit(golden_dir):
    p = run(golden_dir, ["-x"])
    assert p.returncode == 1 and b"[-F censor]" in p.stderr and b"  -F censor : fit each query's Gumbel parameters" in p.stderr


def test_fit_and_refine_or_matches_do_not_combine(golden_dir):
    assert_refused_early(run(golden_dir, ["-F", "0.01", "-k", "5", "-R", "256"]), b"ERROR: -F cannot be combined with -R")
    assert_refused_early(run(golden_dir, ["-F", "0.01", "-m", "2"]), b"ERROR: -F cannot be combined with -m")
    # the existing refusals come first
    assert_refused_early(run(golden_dir, ["-F", "0.01", "-R", "256"]), b"ERROR: -R needs -k K")
    assert_refused_early(run(golden_dir, ["-F", "0", "-k", "5", "-R", "256", "-m", "2"]), b"ERROR: -R cannot be combined with -m")


@pytest.mark.parametrize("arg", ["x", "", "0.6", "-0.1", "nan", "inf", "0.1x"])
def test_fit_values_are_checked(golden_dir, arg):
    p = run(golden_dir, ["-F", arg])
    assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""
    assert ("ERROR: -F needs a censored fraction in [0, 0.5] (got '%s')" % arg).encode() in p.stderr
    assert b"MAXDIM" not in p.stderr


@pytest.mark.parametrize("arg", ["0", "0.01", "0.5", "5e-2"])
def test_good_fractions_pass_the_option_checks(golden_dir, arg):
    p = run(golden_dir, ["-c", "-F", arg])                                    # no stdin: stops at the database name
    assert b"-F " not in p.stderr and b"Usage:" not in p.stderr and b"MAXDIM" in p.stderr
