"""Scoring a search against a classification (-E, sat_eval_*) without a GPU: the one reducing function of
csrc/host/sat_eval.h against pair counts made in Python (eval_lib), the host code under the sanitizers as a stand-alone
program, the command line's refusals and usage text, the declarations of the header, and the new translation unit in the
recorded build commands."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cuda_satabsearch_amd import _native, report

import edge_cases as ec
import eval_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
HOST = os.path.join(ROOT, "cuda_satabsearch_amd", "csrc", "host")


def expand(pos, neg):
    """the listing a table stands for: one score per counted row"""
    bins = np.arange(len(pos))
    return np.repeat(bins, pos), np.repeat(bins, neg)


def check(pos, neg, rocn):
    pos, neg = np.asarray(pos, np.uint32), np.asarray(neg, np.uint32)
    want = eval_lib.table_counts(pos, neg, rocn)
    if int(pos.sum()) * int(neg.sum()) <= 4_000_000:           # small enough to compare row against row
        assert eval_lib.pair_counts(*expand(pos, neg), rocn) == want
    assert report.eval_reduce(pos, neg, rocn) == want, (pos, neg, rocn)
    return want


# ---------------------------------------------------------------- 1. sat_eval_reduce
def test_random_tables():
    rng = np.random.default_rng(5)
    for _ in range(300):
        bins = int(rng.integers(1, 60))
        top = int(rng.choice([2, 4, 30]))                       # few values: many empty bins and many ties
        pos, neg = rng.integers(0, top, bins), rng.integers(0, top, bins)
        if rng.random() < 0.3:
            pos[rng.random(bins) < 0.7] = 0
        if rng.random() < 0.3:
            neg[rng.random(bins) < 0.7] = 0
        check(pos, neg, int(rng.choice([1, 2, 5, 50, 1000])))


@pytest.mark.parametrize("name,pos,neg,rocn,want", [
    ("one bin", [3], [4], 50, (12, 12, 3, 4, 4)),
    ("one bin, one negative counted", [3], [4], 1, (12, 3, 3, 4, 1)),
    ("all ties in a wider table", [0, 5, 0], [0, 7, 0], 3, (35, 15, 5, 7, 3)),
    ("tie-free", [0, 1, 0, 1, 0, 1], [1, 0, 1, 0, 1, 0], 2, (2 * 6, 2 * 3, 3, 3, 2)),
    ("all positives above", [0, 0, 2, 3], [4, 1, 0, 0], 50, (2 * 25, 2 * 25, 5, 5, 5)),
    ("all positives below", [2, 3, 0, 0], [0, 0, 4, 1], 50, (0, 0, 5, 5, 5)),
    ("rocn = 1", [1, 0, 1, 1], [0, 1, 0, 1], 1, (1 + 4, 1, 3, 2, 1)),
    ("rocn = negatives", [1, 0, 1, 1], [0, 1, 0, 1], 2, (5, 5, 3, 2, 2)),
    ("rocn > negatives", [1, 0, 1, 1], [0, 1, 0, 1], 9, (5, 5, 3, 2, 2)),
    # negatives by score from the top: 2 at bin 3 (1 positive tied: 1 each), 4 at bin 1 (2 positives above: 4 each);
    # the first 3 negatives take the whole first group and ONE of the second
    ("a tie group straddles the n-th negative", [0, 0, 1, 1], [0, 4, 0, 2], 3, (2 * 1 + 4 * 4, 2 * 1 + 1 * 4, 2, 6, 3)),
    ("no positive", [0, 0, 0], [1, 2, 3], 4, (0, 0, 0, 6, 4)),
    ("no negative", [1, 2, 3], [0, 0, 0], 4, (0, 0, 6, 0, 0)),
    ("nothing at all", [0], [0], 1, (0, 0, 0, 0, 0)),
])
def test_edge_tables(name, pos, neg, rocn, want):
    assert check(pos, neg, rocn) == want, name


def test_counts_near_2_to_31_need_the_64_bit_sums():
    big = 2**31 - 1
    want = check([0, big - 5, 5], [big - 7, 7, 0], 50)
    assert want[0] == 2 * big * (big - 7) + 7 * (2 * 5 + big - 5) and want[0] > 2**62 and want[2:4] == (big, big)
    want = check([big], [big], 2**31 - 1)
    assert want[:2] == (big * big, big * big)
    check([1, 0, big - 1], [0, big, 0], 2**30)
    # a side of 2^31 rows is no table of a search: refused, not wrapped
    with pytest.raises(ValueError):
        report.eval_reduce([big, 1], [1, 1])
    with pytest.raises(ValueError):
        report.eval_reduce([1], [1], 0)
    with pytest.raises(ValueError):
        report.eval_reduce([1, 1], [1])


def test_ratios_and_table_lines():
    rows = np.zeros(3, eval_lib.EVAL_DTYPE)
    rows[0] = (7, 1, 3, 2, 1, 1)
    rows[1] = (0, 0, 0, 6, 4, 0)
    rows[2]["query_class"] = -1
    assert report.eval_ratios(rows[0]) == (7 / 12.0, 1 / 6.0) and report.eval_ratios(rows[1]) == (None, None)
    lines = report.eval_table(["d1abca_", "d1abcb_", "x"], ["a.1", "b.2"], rows, "db", "cls", 10, 7, 128, 50, polish_all=2)
    assert lines == ["# EVAL dbfile = db classes = cls entries = 10 classified = 7 distinct = 2 restarts = 128 rocn = 50",
                     "# POLISH tops = 2 all rows",
                     "# MEAN queries = 1 auc = 0.583333 rocn = 0.166667",
                     "d1abca_  b.2 3 2 7 1 1 0.583333 0.166667",
                     "d1abcb_  a.1 0 6 0 0 4 NA NA",
                     "x        - 0 0 0 0 0 NA NA"]
    assert report.eval_table(["x"], [], rows[2:], "db", "cls", 1, 0, 1, 5)[1] == "# MEAN queries = 0 auc = NA rocn = NA"


# ---------------------------------------------------------------- 2. the host code under the sanitizers
def test_host_code_under_the_sanitizers(tmp_path):
    """the reducer on tie-free listings against the reference's definition (for every negative the positives ranked
    above it) and the class-file reader on good and bad files: a stand-alone program built with
    -fsanitize=address,undefined, run as a child; no report may appear"""
    exe = str(tmp_path / "eval_check")
    build = subprocess.run(["gcc", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-Wall", "-Wextra", "-I", HOST, "-o", exe, os.path.join(ROOT, "tests", "native", "eval_check.c"),
                            os.path.join(HOST, "sat_eval.c"), os.path.join(HOST, "sat_parse.c"), "-lm", "-lpthread"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    scratch = tmp_path / "files"
    scratch.mkdir()
    run = subprocess.run([exe, str(scratch)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == "eval_check: ok\n"
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr and run.stderr == ""


# ---------------------------------------------------------------- 3. command line
def run(golden_dir, args, stdin=b""):
    return subprocess.run([CLI] + args, input=stdin, cwd=golden_dir, capture_output=True)


@pytest.mark.parametrize("args,message", [
    (["-c", "-a", ec.EDGE_DB, "-E", "f"], b"ERROR: -E cannot be combined with -c\n"),
    (["-E", "f"], b"ERROR: -E needs -a dbfile or -Q dbfile\n"),
    (["-q", ec.EDGE_DB, "-E", "f"], b"ERROR: -E needs -a dbfile or -Q dbfile\n"),
    (["-a", ec.EDGE_DB, "-E", "f", "-k", "3"], b"ERROR: -E cannot be combined with -k\n"),
    (["-a", ec.EDGE_DB, "-E", "f", "-p", "0.5"], b"ERROR: -E cannot be combined with -p\n"),
    (["-a", ec.EDGE_DB, "-E", "f", "-m", "2"], b"ERROR: -E cannot be combined with -m\n"),
    (["-a", ec.EDGE_DB, "-E", "f", "-M", "2"], b"ERROR: -E cannot be combined with -M\n"),
    (["-a", ec.EDGE_DB, "-E", "f", "-R", "64"], b"ERROR: -E cannot be combined with -R\n"),
    (["-a", ec.EDGE_DB, "-E", "f", "-C", "5"], b"ERROR: -E cannot be combined with -C\n"),
    (["-a", ec.EDGE_DB, "-E", "f", "-F", "0.05"], b"ERROR: -E cannot be combined with -F\n"),
    (["-a", ec.EDGE_DB, "-E", "f", "-L", "0.001"], b"ERROR: -E cannot be combined with -L\n"),
    (["-a", ec.EDGE_DB, "-E", "f", "-H", "0.001,0.01"], b"ERROR: -E cannot be combined with -H\n"),
    (["-Q", ec.EDGE_DB, "-E", "f", "-k", "3"], b"ERROR: -E cannot be combined with -k\n"),
    (["-a", ec.EDGE_DB, "-E", "f", "-P", "2"], b"ERROR: -E takes -P T only with -A\n"),
    (["-a", ec.EDGE_DB, "-N", "5"], b"ERROR: -N needs -E classfile\n"),
    (["-a", ec.EDGE_DB, "-N", "5", "-L", "0.001"], b"ERROR: -N needs -E classfile\n"),
])
def test_cli_refusals(golden_dir, args, message):
    p = run(golden_dir, args, b"not read\n")
    assert p.returncode == 1, p.stderr
    assert message in p.stderr, p.stderr
    assert p.stderr.count(b"ERROR:") == 1 and p.stdout == b""
    # nothing after the option checks ran: no banner, no device query
    assert b"MAXDIM" not in p.stderr and b"HIP device" not in p.stderr


@pytest.mark.parametrize("value", ["0", "-3", "x", "5x", "", "1.5", "99999999999"])
def test_cli_refuses_a_bad_n(golden_dir, value):
    p = run(golden_dir, ["-a", ec.EDGE_DB, "-E", "f", "-N", value])
    assert p.returncode == 1 and p.stdout == b""
    assert b"ERROR: -N needs an integer >= 1 (got '" + value.encode() + b"')\n" in p.stderr
    assert b"Usage:" in p.stderr and b"MAXDIM" not in p.stderr


def test_usage_names_the_options(golden_dir):
    p = run(golden_dir, ["-x"])
    assert p.returncode == 1 and p.stdout == b""
    assert b"[-E classfile [-N n]]" in p.stderr
    assert b"  -E classfile : with -a dbfile or -Q dbfile: score the search against a classification on the GPU" in p.stderr
    assert b"name class positives negatives u2 t2 n_used auc rocn" in p.stderr
    assert b"  -N n : with -E: the negatives ROC-n counts up to (n >= 1). Default 50" in p.stderr
    assert b"[-A] [-L P] [-b]" in p.stderr                    # the older text stays
    for option in (["-E"], ["-a", ec.EDGE_DB, "-E", "f", "-N"]):    # an option without its argument is a usage error too
        p = run(golden_dir, option)
        assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""


def test_cli_reads_the_class_file_before_it_touches_a_gpu(golden_dir, tmp_path):
    """a class file that cannot be used ends the run after the database is loaded and before any device is asked for"""
    p = run(golden_dir, ["-a", ec.EDGE_DB, "-E", str(tmp_path / "missing")])
    assert p.returncode == 1 and p.stdout == b"" and b"ERROR: cannot open class file " in p.stderr and b"HIP device" not in p.stderr
    names = [line.split()[0] for line in open(os.path.join(golden_dir, ec.EDGE_DB)) if re.match(r"^\S+\s+\d+\s*$", line)]
    assert len(names) > 3
    twice = tmp_path / "twice"
    twice.write_text("%s a\n# comment\n%s b\n%s a\n" % (names[0], names[1], names[0].upper()))
    p = run(golden_dir, ["-a", ec.EDGE_DB, "-E", str(twice)])
    assert p.returncode == 1 and p.stdout == b"" and b"HIP device" not in p.stderr
    assert b" line 4: the name '" + names[0].upper().encode() + b"' is listed twice (first on line 1)\n" in p.stderr


# ---------------------------------------------------------------- 4. header, build
def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "satabsearch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for decl in ("int sat_eval_classes(sat_ctx *ctx, int n_nodes, const int32_t *node_class);",
                 "int sat_eval_rows(sat_ctx *ctx, const int32_t *query_node, int rocn, sat_eval *rows);",
                 "int sat_eval_tables(sat_ctx *ctx, const int32_t *query_node, uint32_t *counts, const int64_t *offset);",
                 "int sat_multi_eval_classes(sat_multi *m, const int32_t *node_class);",
                 "int sat_multi_eval_rows(sat_multi *m, const int32_t *query_node, int rocn, sat_eval *rows);"):
        assert decl in text, decl
        assert decl[4:decl.index("(")] in _native.ABI_SYMBOLS
    assert "typedef struct sat_eval { uint64_t u2, t2; int32_t positives, negatives, n_used, query_class; } sat_eval;" in text
    assert C.sizeof(_native.Eval) == 32 and eval_lib.EVAL_DTYPE.itemsize == 32
    host = open(os.path.join(HOST, "sat_eval.h")).read()
    assert host.count("void sat_eval_walk(") == 1                 # the one reducing function, in the header both sides include
    host = re.sub(r"/\*.*?\*/", "", host, flags=re.S)
    assert "int sat_eval_reduce(const uint32_t *pos, const uint32_t *neg, int32_t bins, int32_t rocn, sat_eval_row *out);" in host
    assert "sat_abi_version" in text and _native.EVAL_BLOCK_ROWS == 4096


def test_the_evaluation_is_a_translation_unit_of_the_device_library(monkeypatch):
    """sat_eval.hip is in build.DEVICE_SOURCES and build_device() compiles it once for gfx950 to an object the library
    links, with the host function's object beside it; libsathost.so holds the host function too (the commands are
    recorded, not run).  The kernels are that file's: sat_capi.hip keeps none, and both sides call the one function."""
    from cuda_satabsearch_amd import build
    assert "sat_eval.hip" in build.DEVICE_SOURCES
    cmds = []
    monkeypatch.setattr(build, "_run", cmds.append)
    build.build_device(force=True)
    build.build_host(force=True)
    compiles = [c for c in cmds if "-c" in c and c[-1] == os.path.join(build.CSRC, "sat_eval.hip")]
    assert len(compiles) == 1 and "--offload-arch=gfx950" in compiles[0]
    assert len([c for c in cmds if "-c" in c and c[0] == build.HIPCC]) == len(build.DEVICE_SOURCES)
    obj = compiles[0][compiles[0].index("-o") + 1]
    links = [c for c in cmds if "-shared" in c and c[c.index("-o") + 1] == build.DEVICE_LIB[0]]
    assert len(links) == 1 and "-Wl," + obj in links[0]
    assert "-Wl," + os.path.join(build.PKG, "sat_eval.o") in links[0] and obj != os.path.join(build.PKG, "sat_eval.o")
    host = [c for c in cmds if "-shared" in c and c[c.index("-o") + 1] == os.path.join(build.PKG, "libsathost.so")]
    assert len(host) == 1 and os.path.join(build.HOST, "sat_eval.c") in host[0]
    assert "sat_eval.hip" in open(os.path.join(ROOT, "Makefile")).read()
    text = open(os.path.join(build.CSRC, "sat_eval.hip")).read()
    assert '#include "host/sat_eval.h"' in text and "sat_eval_walk(&acc" in text
    assert "eval_histogram(" in text and "eval_reduce(" in text
    assert re.search(r"kEvalBlock = 1024, kEvalPasses = 4, kEvalRows = kEvalBlock \* kEvalPasses;", text)     # _native.EVAL_BLOCK_ROWS
    assert "constexpr int kEvalWindow = %d," % _native.EVAL_WINDOW_BINS in text
    assert "__global__" not in open(os.path.join(build.CSRC, "sat_capi.hip")).read()
    assert '#include "sat_eval.h"' in open(os.path.join(build.HOST, "sat_eval.c")).read()
    # the library exports the host function beside the device calls
    lib = C.CDLL(_native.DEVICE_LIB)
    assert hasattr(lib, "sat_eval_reduce") and hasattr(_native.host_lib(), "sat_eval_reduce")
