"""Refine (-R / -C), command-line side without a GPU: the usage text, and every refusal made right after the option
parsing, before the database is read or a device is asked for (the GPU side is tests/test_gpu_refine.py)."""
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


def test_usage_lists_refine_options(golden_dir):
    p = run(golden_dir, ["-x"])
    assert p.returncode == 1
    assert b"[-R restarts [-C C]]" in p.stderr
    assert b"  -R restarts :" in p.stderr and b"  -C C :" in p.stderr


def test_refine_needs_the_gpu_path(golden_dir):
    query = open(os.path.join(golden_dir, "d1ubia_.input"), "rb").read()
    assert_refused_early(run(golden_dir, ["-c", "-R", "4096", "-k", "5"], query), b"ERROR: -R needs the GPU path")


def test_refine_needs_k(golden_dir):
    assert_refused_early(run(golden_dir, ["-R", "4096"]), b"ERROR: -R needs -k K")


def test_k_above_candidates_is_refused(golden_dir):
    assert_refused_early(run(golden_dir, ["-R", "4096", "-C", "3", "-k", "5"]), b"ERROR: -k K (5) exceeds -C C (3)")


def test_refine_and_matches_do_not_combine(golden_dir):
    assert_refused_early(run(golden_dir, ["-R", "4096", "-k", "5", "-m", "2"]), b"ERROR: -R cannot be combined with -m")


def test_candidates_need_refine(golden_dir):
    assert_refused_early(run(golden_dir, ["-C", "40", "-k", "5"]), b"ERROR: -C needs -R")


@pytest.mark.parametrize("opt", ["-R", "-C"])
@pytest.mark.parametrize("arg", ["0", "-1", "x", "2x", ""])
def test_refine_counts_must_be_positive(golden_dir, opt, arg):
    # a valid -R first: the value check, not an unknown option, is what refuses
    p = run(golden_dir, ["-R", "64", "-k", "5", opt, arg])
    assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""
    assert ("ERROR: %s needs a positive integer (got '%s')" % (opt, arg)).encode() in p.stderr
