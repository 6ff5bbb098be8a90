"""The whole-database polish (-P T -A, sat_polish_all_set) without a GPU: the command line's refusals and usage text,
and the four declarations of the public header."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")


def run(golden_dir, args, stdin=b""):
    return subprocess.run([CLI] + args, input=stdin, cwd=golden_dir, capture_output=True)


def assert_refused_early(p, message):
    assert p.returncode == 1, p.stderr
    assert message in p.stderr, p.stderr
    assert p.stderr.count(b"ERROR:") == 1 and p.stdout == b""
    # nothing after the option checks ran: no banner, no device query
    assert b"MAXDIM" not in p.stderr and b"HIP device" not in p.stderr


@pytest.mark.parametrize("args,message", [
    (["-A"], b"ERROR: -A needs -P T\n"),
    (["-A", "-k", "5"], b"ERROR: -A needs -P T\n"),
    (["-A", "-P", "4", "-c"], b"ERROR: -A cannot be combined with -c\n"),
    (["-A", "-P", "4", "-m", "2"], b"ERROR: -A cannot be combined with -m\n"),
    (["-A", "-P", "4", "-k", "5", "-M", "2"], b"ERROR: -A cannot be combined with -M\n"),
    (["-A", "-P", "4", "-k", "5", "-R", "512"], b"ERROR: -A cannot be combined with -R\n"),
    (["-A", "-P", "4", "-k", "5", "-C", "20"], b"ERROR: -A cannot be combined with -C\n"),
])
def test_cli_refusals_of_all_rows(golden_dir, args, message):
    query = open(os.path.join(golden_dir, "d1ubia_.input"), "rb").read()
    assert_refused_early(run(golden_dir, args, query), message)


@pytest.mark.parametrize("args,message", [
    (["-P", "4", "-p", "0.01"], b"ERROR: -P cannot be combined with -p\n"),
    (["-P", "4", "-F", "0.1"], b"ERROR: -P cannot be combined with -F\n"),
    (["-P", "4"], b"ERROR: -P needs -k K\n"),
])
def test_without_all_rows_the_refusals_of_polish_stand(golden_dir, args, message):
    query = open(os.path.join(golden_dir, "d1ubia_.input"), "rb").read()
    assert_refused_early(run(golden_dir, args, query), message)


def test_usage_names_all_rows(golden_dir):
    p = run(golden_dir, ["-x"])
    assert p.returncode == 1 and p.stdout == b""
    assert b"[-P T] [-A]" in p.stderr and b"  -A : with -P T: all rows" in p.stderr


def test_header_declares_the_mode():
    text = open(os.path.join(ROOT, "include", "satabsearch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for decl in ("int sat_polish_all_set(sat_ctx *ctx, int tops);", "int sat_polish_all_get(const sat_ctx *ctx);",
                 "int sat_results_base(sat_ctx *ctx, int32_t *base_scores);",
                 "int sat_multi_polish_all_set(sat_multi *m, int tops);"):
        assert decl in text, decl
    debug = open(os.path.join(ROOT, "include", "satabsearch_debug.h")).read()
    assert "SAT_EXP_POLISH_GROUP" in debug
