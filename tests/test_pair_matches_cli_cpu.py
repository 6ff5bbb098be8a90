"""Matches of the printed rows (-M), command-line side without a GPU: the usage text, and every refusal made right after
the option parsing, before the database is read or a device is asked for (the GPU side is
tests/test_gpu_pair_matches.py)."""
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


def test_usage_lists_the_option(golden_dir):
    p = run(golden_dir, ["-x"])
    assert p.returncode == 1
    assert b"[-M M]" in p.stderr and b"  -M M :" in p.stderr
    # -m keeps its own line
    assert b"[-m M]" in p.stderr and b"  -m M :" in p.stderr


@pytest.mark.parametrize("args", [["-M", "3"], ["-r", "64", "-M", "2"], ["-M", "2", "-C", "4"]])
def test_needs_a_ranked_mode(golden_dir, args):
    message = b"ERROR: -C needs -R" if "-C" in args else b"ERROR: -M needs -k K, -p P or -R restarts -k K"
    assert_refused_early(run(golden_dir, args), message)


@pytest.mark.parametrize("ranked", [["-k", "5"], ["-p", "0.01"]])
def test_does_not_combine_with_m(golden_dir, ranked):
    p = run(golden_dir, ranked + ["-m", "2", "-M", "2"])
    # (-p with -m is refused first, as before)
    message = b"ERROR: -p cannot be combined with -m" if ranked[0] == "-p" else b"ERROR: -M cannot be combined with -m"
    assert_refused_early(p, message)


def test_needs_the_gpu_path(golden_dir):
    query = open(os.path.join(golden_dir, "d1ubia_.input"), "rb").read()
    assert_refused_early(run(golden_dir, ["-c", "-k", "5", "-M", "2"], query), b"ERROR: -M needs the GPU path")
    assert_refused_early(run(golden_dir, ["-c", "-M", "2"], query), b"ERROR: -M needs the GPU path")


@pytest.mark.parametrize("arg", ["0", "9", "x", "-1", "2x", ""])
def test_count_must_be_1_to_8(golden_dir, arg):
    p = run(golden_dir, ["-k", "5", "-M", arg])
    assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""
    assert ("ERROR: -M needs an integer 1..8 (got '%s')" % arg).encode() in p.stderr
    assert b"MAXDIM" not in p.stderr


@pytest.mark.parametrize("args", [["-k", "5", "-M", "1"], ["-p", "0.5", "-M", "8"], ["-R", "256", "-k", "5", "-M", "3"]])
def test_accepted_combinations_get_past_the_option_checks(golden_dir, args):
    """With a ranked mode the option checks pass: the run goes on to its banner (and, without stdin, fails there)."""
    p = run(golden_dir, args)
    assert b"MAXDIM" in p.stderr and b"ERROR: -M" not in p.stderr
