"""The p-value cutoff (-p), command-line side without a GPU: the usage text, the value checks, and the refusals made
right after the option parsing, before the banner or any device call (the GPU side is tests/test_gpu_cutoff.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")


def run(golden_dir, args, stdin=b""):
    return subprocess.run([CLI] + args, input=stdin, cwd=golden_dir, capture_output=True)


def assert_refused_early(p, message):
    assert p.returncode == 1, p.stderr
    assert message in p.stderr, p.stderr
    assert p.stdout == b""
    # nothing after the option checks ran: no banner, no device query
    assert b"MAXDIM" not in p.stderr and b"HIP device" not in p.stderr


def test_usage_lists_the_cutoff(golden_dir):
    p = run(golden_dir, ["-x"])
    assert p.returncode == 1
    assert b"[-p P]" in p.stderr
    assert b"  -p P : print only rows whose p-value is <= P, ranked as -k (GPU mode)" in p.stderr


def test_cutoff_needs_the_gpu_path(golden_dir):
    query = open(os.path.join(golden_dir, "d1ubia_.input"), "rb").read()
    assert_refused_early(run(golden_dir, ["-c", "-p", "1e-3"], query), b"ERROR: -p needs the GPU path")


def test_cutoff_and_matches_do_not_combine(golden_dir):
    assert_refused_early(run(golden_dir, ["-p", "1e-3", "-m", "2"]), b"ERROR: -p cannot be combined with -m")


def test_cutoff_and_refine_do_not_combine(golden_dir):
    # refused as -p, not as -R without -k
    assert_refused_early(run(golden_dir, ["-p", "1e-3", "-R", "4096"]), b"ERROR: -p cannot be combined with -R")
    assert_refused_early(run(golden_dir, ["-R", "4096", "-k", "5", "-p", "0.05"]), b"ERROR: -p cannot be combined with -R")


@pytest.mark.parametrize("arg", ["x", "", "-1", "nan", "inf", "1e-3x"])
def test_cutoff_values_are_checked(golden_dir, arg):
    p = run(golden_dir, ["-p", arg])
    assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""
    assert ("ERROR: -p needs a p-value >= 0 (got '%s')" % arg).encode() in p.stderr
    assert b"MAXDIM" not in p.stderr


@pytest.mark.parametrize("arg", ["1e-3", "0", "1", "0.05"])
def test_good_cutoffs_pass_the_option_checks(golden_dir, arg):
    # no stdin: the run stops later (no database name, or no device), never at -p
    p = run(golden_dir, ["-p", arg])
    assert b"-p " not in p.stderr, p.stderr
    assert b"Usage:" not in p.stderr and b"MAXDIM" in p.stderr
