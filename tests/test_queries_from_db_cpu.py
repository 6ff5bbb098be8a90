"""Queries taken from the resident database (-Q, -a, sat_queries_from_db) without a GPU: the command line's refusals and
usage text, the declarations of the two headers, and the host mode's -q output, which the new options leave alone."""
import os
import re
import subprocess

import pytest

import edge_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")


def run(golden_dir, args, stdin=b""):
    return subprocess.run([CLI] + args, input=stdin, cwd=golden_dir, capture_output=True)


@pytest.mark.parametrize("args,message", [
    (["-Q", ec.EDGE_DB, "-c"], b"ERROR: -Q cannot be combined with -c\n"),
    (["-c", "-a", ec.EDGE_DB], b"ERROR: -a cannot be combined with -c\n"),
    (["-Q", ec.EDGE_DB, "-q", ec.EDGE_DB], b"ERROR: -Q cannot be combined with -q\n"),
    (["-q", ec.EDGE_DB, "-a", ec.EDGE_DB], b"ERROR: -a cannot be combined with -q\n"),
    (["-a", ec.EDGE_DB, "-Q", ec.EDGE_DB, "-k", "3"], b"ERROR: -a cannot be combined with -Q\n"),
])
def test_cli_refusals(golden_dir, args, message):
    p = run(golden_dir, args, ec.edge_sids()[1].encode())
    assert p.returncode == 1, p.stderr
    assert message in p.stderr, p.stderr
    assert p.stderr.count(b"ERROR:") == 1 and p.stdout == b""
    # nothing after the option checks ran: no banner, no device query
    assert b"MAXDIM" not in p.stderr and b"HIP device" not in p.stderr


def test_usage_names_both_options(golden_dir):
    p = run(golden_dir, ["-x"])
    assert p.returncode == 1 and p.stdout == b""
    assert b"[-q dbfile | -Q dbfile | -a dbfile]" in p.stderr
    assert b"  -Q dbfile : as -q dbfile" in p.stderr and b"  -a dbfile : all-vs-all" in p.stderr
    for opt in (b"-Q", b"-a"):                 # an option without its argument is a usage error too
        p = run(golden_dir, [opt.decode()])
        assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""


def test_headers_declare_the_calls():
    text = open(os.path.join(ROOT, "include", "satabsearch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for decl in ("int sat_queries_from_db(sat_ctx *ctx, int n_queries, const int32_t *entry, uint32_t first_query_ordinal);",
                 "int sat_multi_queries_from_db(sat_multi *m, int n_queries, const int32_t *entry, uint32_t first_query_ordinal);",
                 "unsigned long long sat_stat_query_h2d_bytes(const sat_ctx *ctx);"):
        assert decl in text, decl
    debug = open(os.path.join(ROOT, "include", "satabsearch_debug.h")).read()
    debug = re.sub(r"/\*.*?\*/", "", debug, flags=re.S)
    assert "long long sat_debug_query_blob(struct sat_ctx *ctx, void *out, size_t capacity);" in debug


def test_host_mode_q_output_is_unchanged(golden_dir):
    """-c -q over the edge database prints the committed bytes (the reference's own); -Q never reaches the host mode"""
    name, bodies, _, restarts = [j for j in ec.EDGE_JOBS if j[1] is None][0]
    args, stdin = ec.job_command((name, bodies, None, restarts), golden_dir)
    want = open(os.path.join(ROOT, "tests", "golden", "expected", name + ".out"), "rb").read()
    p = run(golden_dir, ["-c"] + args, stdin)
    assert p.returncode == 0, p.stderr[-400:]
    assert p.stdout == want
