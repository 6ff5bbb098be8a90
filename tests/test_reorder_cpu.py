"""Hits out of sequence order (-X B, sat_reorder_hits) without a GPU: the order of a map - sat_map_kind of
csrc/host/sat_reorder.h through libsathost.so - against reorder_lib's restatement of its rule, the same C under the
sanitizers as a stand-alone program, the command line's refusals and its -x parser, the -c goldens through the new
binary, the table report.reorder_table renders, and the declarations and build lists."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from cuda_satabsearch_amd import _native, report, search

import edge_cases as ec
import reorder_lib as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
HOST = os.path.join(ROOT, "cuda_satabsearch_amd", "csrc", "host")
EXPECTED = os.path.join(ROOT, "tests", "golden", "expected")


def rotations():
    for n in range(2, 7):
        for c in range(1, n):
            yield list(range(c, n)) + list(range(c))


def named_cases():
    """(name, map, (kind, matched, descents, cut)) - the expected tuples are written out by hand"""
    yield "empty", [], (rl.SEQ, 0, 0, 0)
    yield "all unmatched", [-1] * 5, (rl.SEQ, 0, 0, 0)
    yield "one match", [-1, 7, -1], (rl.SEQ, 1, 0, 0)
    yield "identity", list(range(9)), (rl.SEQ, 9, 0, 0)
    yield "ascending with gaps", [-1, 2, -1, 5, 40], (rl.SEQ, 3, 0, 0)
    for m in rotations():
        c = m[0]
        yield "rotation %r" % m, m, (rl.CIRC, len(m), 1, len(m) - c + 1)
    yield "rotation with gaps", [-1, 6, 9, -1, -1, 0, 3, -1], (rl.CIRC, 4, 1, 6)
    yield "rotation, unmatched first of the second run", [4, 5, -1, 1, 2], (rl.CIRC, 4, 1, 4)
    yield "reversal", [4, 3, 2, 1, 0], (rl.PERM, 5, 4, 0)
    yield "swap", [1, 0], (rl.CIRC, 2, 1, 2)
    yield "two descents", [2, 3, 0, 4, -1, 1], (rl.PERM, 5, 2, 0)
    yield "two swaps", [1, 0, 3, 2], (rl.PERM, 4, 2, 0)
    yield "one descent, last above first", [1, 3, 2], (rl.PERM, 3, 1, 0)
    yield "one descent, last above first, gaps", [5, -1, 9, 7, -1], (rl.PERM, 3, 1, 0)
    big = list(range(60, 111)) + list(range(60))
    yield "n1 = 111 rotation", big, (rl.CIRC, 111, 1, 52)
    yield "n1 = 111 identity", list(range(111)), (rl.SEQ, 111, 0, 0)
    yield "n1 = 111 reversal", list(range(110, -1, -1)), (rl.PERM, 111, 110, 0)


CASES = list(named_cases())


# ---------------------------------------------------------------- 1. sat_map_kind
@pytest.mark.parametrize("name,m,want", CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_map_kind_named_cases(name, m, want):
    assert rl.kind(m) == want, "the restatement"
    assert report.map_kind(m) == want


def test_map_kind_every_small_map():
    """every map of up to 5 query SSEs into 5 db SSEs without a db SSE twice, unmatched places included"""
    count, kinds = 0, set()
    for n1 in range(0, 6):
        for m in itertools.product(range(-1, 5), repeat=n1):
            used = [j for j in m if j >= 0]
            if len(used) != len(set(used)):
                continue
            got = report.map_kind(list(m))
            assert got == rl.kind(m), m
            kinds.add(got[0])
            count += 1
    assert count > 2000 and kinds == {rl.SEQ, rl.CIRC, rl.PERM}


def test_map_kind_random_long_maps():
    rng = np.random.default_rng(7)
    for n1 in (16, 33, 64, 111):
        for _ in range(200):
            m = rng.permutation(111)[:n1].astype(np.int32)
            if rng.random() < 0.5:
                m = np.sort(m)
                m = np.roll(m, int(rng.integers(0, n1)))
            m[rng.random(n1) < 0.2] = -1
            assert report.map_kind(m) == rl.kind(m.tolist())


def test_map_kind_refuses_bad_arguments():
    host = _native.host_lib()
    assert host.sat_map_kind(None, 3, None, None, None) == -1
    assert host.sat_map_kind(None, -1, None, None, None) == -1
    assert host.sat_map_kind(None, 0, None, None, None) == rl.SEQ
    m = np.array([2, 0, 1], np.int32)
    assert host.sat_map_kind(m.ctypes.data, 3, None, None, None) == rl.CIRC          # the outputs are optional


# ---------------------------------------------------------------- 2. the host code under the sanitizers
def test_host_code_under_the_sanitizers(tmp_path):
    """sat_reorder.c and tests/native/reorder_check.c - a stand-alone program with its own main that reads maps on stdin
    and prints their order - built plainly and with -fsanitize=address,undefined; both run as children on the same maps.
    The outputs are equal, they are what reorder_lib computes, and no report appears.  Nothing is loaded into Python,
    nothing is preloaded."""
    maps = [c[1] for c in CASES]
    rng = np.random.default_rng(11)
    for n1 in (1, 2, 7, 64, 111):
        for _ in range(20):
            m = rng.permutation(111)[:n1]
            m[rng.random(n1) < 0.3] = -1
            maps.append(m.tolist())
    text = "".join("%d %s\n" % (len(m), " ".join(map(str, m))) for m in maps)
    want = ["%d %d %d %d" % rl.kind(m) for m in maps] + ["reorder_check: %d maps" % len(maps)]
    outputs = []
    for name, flags in (("plain", ["-O2"]),
                        ("sanitized", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / ("reorder_check_" + name))
        build = subprocess.run(["gcc"] + flags + ["-Wall", "-Wextra", "-I", HOST, "-o", exe, os.path.join(ROOT, "tests", "native", "reorder_check.c"),
                                                  os.path.join(HOST, "sat_reorder.c")], capture_output=True, text=True)
        assert build.returncode == 0, build.stderr
        run_ = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert run_.returncode == 0, run_.stderr[-2000:]
        assert "Sanitizer" not in run_.stderr and "runtime error" not in run_.stderr and run_.stderr == ""
        outputs.append(run_.stdout)
    assert outputs[0] == outputs[1]
    assert outputs[0].splitlines() == want


# ---------------------------------------------------------------- 3. command line
def run(golden_dir, args, stdin=b""):
    return subprocess.run([CLI] + args, input=stdin, cwd=golden_dir, capture_output=True)


X = ["-X", "0.01", "-p", "0.001"]


@pytest.mark.parametrize("args,message", [
    (["-c", "-q", ec.EDGE_DB] + X, b"ERROR: -X cannot be combined with -c\n"),
    (["-c"] + X, b"ERROR: -X cannot be combined with -c\n"),
    (["-q", ec.EDGE_DB] + X + ["-m", "2"], b"ERROR: -X cannot be combined with -m\n"),
    (["-q", ec.EDGE_DB] + X + ["-M", "2"], b"ERROR: -X cannot be combined with -M\n"),
    (["-q", ec.EDGE_DB] + X + ["-k", "3", "-R", "64"], b"ERROR: -X cannot be combined with -R\n"),
    (["-q", ec.EDGE_DB] + X + ["-C", "5"], b"ERROR: -X cannot be combined with -C\n"),
    (["-a", ec.EDGE_DB] + X + ["-L", "0.001"], b"ERROR: -X cannot be combined with -L\n"),
    (["-a", ec.EDGE_DB] + X + ["-H", "0.001,0.01"], b"ERROR: -X cannot be combined with -H\n"),
    (["-a", ec.EDGE_DB] + X + ["-D", "0.001"], b"ERROR: -X cannot be combined with -D\n"),
    (["-a", ec.EDGE_DB] + X + ["-E", "f"], b"ERROR: -X cannot be combined with -E\n"),
    (["-a", ec.EDGE_DB] + X + ["-N", "5"], b"ERROR: -X cannot be combined with -N\n"),
    (["-a", ec.EDGE_DB] + X + ["-W", "0.001"], b"ERROR: -X cannot be combined with -W\n"),
    (["-a", ec.EDGE_DB, "-X", "0.01", "-W", "0.001"], b"ERROR: -X cannot be combined with -W\n"),
    (["-a", ec.EDGE_DB, "-X", "0.01"], b"ERROR: -X needs -p P\n"),
    (["-a", ec.EDGE_DB, "-X", "0.01", "-k", "5"], b"ERROR: -X needs -p P\n"),
    (["-X", "0"], b"ERROR: -X needs -p P\n"),
    (["-q", ec.EDGE_DB] + X + ["-k", "3", "-P", "2"], b"ERROR: -X takes -P T only with -A\n"),
    (["-a", ec.EDGE_DB, "-x", "c"], b"ERROR: -x needs -X B\n"),
    (["-x", "scn"], b"ERROR: -x needs -X B\n"),
    (["-a", ec.EDGE_DB, "-p", "0.001", "-x", "n"], b"ERROR: -x needs -X B\n"),
])
def test_cli_refusals(golden_dir, args, message):
    p = run(golden_dir, args, b"not read\n")
    assert p.returncode == 1, p.stderr
    assert message in p.stderr, p.stderr
    assert p.stderr.count(b"ERROR:") == 1 and p.stdout == b""
    # nothing after the option checks ran: no banner, no device query
    assert b"MAXDIM" not in p.stderr and b"HIP device" not in p.stderr


@pytest.mark.parametrize("value", ["-0.1", "1.5", "nan", "inf", "1e-3x", ""])
def test_cli_refuses_a_baseline_cutoff_outside_0_1(golden_dir, value):
    p = run(golden_dir, ["-a", ec.EDGE_DB, "-p", "0.5", "-X", value])
    assert p.returncode == 1 and p.stdout == b""
    assert b"ERROR: -X needs a p-value in [0, 1] (got '" + value.encode() + b"')\n" in p.stderr
    assert b"Usage:" in p.stderr and b"MAXDIM" not in p.stderr


@pytest.mark.parametrize("value", ["", "q", "cq", "c,n", "S", "seq", "c n", "1"])
def test_kinds_parser_refuses(golden_dir, value):
    p = run(golden_dir, ["-a", ec.EDGE_DB, "-p", "0.5", "-X", "0", "-x", value])
    assert p.returncode == 1 and p.stdout == b""
    assert b"ERROR: -x needs letters of s, c, n (got '" + value.encode() + b"')\n" in p.stderr
    assert b"Usage:" in p.stderr and b"MAXDIM" not in p.stderr


@pytest.mark.parametrize("value", ["s", "c", "n", "cn", "nc", "scn", "ncs", "cc"])
def test_kinds_parser_accepts(golden_dir, value):
    """a good -x passes the parser: the run ends at the next refusal, which is not -x's"""
    p = run(golden_dir, ["-c", "-p", "0.5", "-X", "0", "-x", value])
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr == b"ERROR: -X cannot be combined with -c\n"


def test_usage_names_the_options(golden_dir):
    p = run(golden_dir, ["-Z"])
    assert p.returncode == 1 and p.stdout == b""
    assert b"       [-X B [-x kinds]]\n" in p.stderr
    assert b"  -X B : with -p P: only the hits that need a match out of sequence order" in p.stderr
    assert b"(not with -c, -m, -M, -R, -C, -L, -H, -D, -E, -N, -W)" in p.stderr
    assert b"use -F with it" in p.stderr
    assert b"  -x kinds : with -X: the kinds of map printed, letters of s (sequential), c (circular permutation)," in p.stderr
    # the older text stays, byte for byte
    for older in (b"       [-W P [-f F]]\n",
                  b"  -f F : with -W: every two SSEs of the core are matched together in at least F (0 < F <= 1) of the hits.",
                  b"  -b : cache the parsed database as dbfile.satbin\n"):
        assert older in p.stderr, older
    for option in ("-X", "-x"):                          # the option without its argument is a usage error too
        p = run(golden_dir, [option])
        assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""


@pytest.mark.parametrize("name", ["c1_d1ubia_small", "d2phlb1_TFT", "d2phlb1_TTT", "multiquery", "d1twfa_"])
def test_without_the_option_the_host_goldens_are_byte_identical(golden_dir, name):
    with open(os.path.join(golden_dir, name + ".input"), "rb") as f:
        p = run(golden_dir, ["-c", "-r", "128"], f.read())
    assert p.returncode == 0, p.stderr.decode()[-400:]
    assert p.stdout == open(os.path.join(EXPECTED, name + ".r128.out"), "rb").read()


# ---------------------------------------------------------------- 4. the table
def test_reorder_table_renders_the_block():
    rows = np.zeros(2, search._REORDER_DTYPE)
    rows[0] = ((2, 56, 7.0, 12.5, 1e-9), 0.25, 4, rl.CIRC, 8, 1, 5, 0)
    rows[1] = ((0, 9, 1.125, 0.5, 0.0625), 1.0, -3, rl.PERM, 3, 2, 0, 0)
    maps = np.full((2, 111), -1, np.int32)
    maps[0, :3] = [1, 2, 0]
    maps[1, :3] = [2, -1, 0]
    lines = report.reorder_table(["a", "b", "d1ubia_"], rows, maps, 3, 0.01, rl.CIRC | rl.PERM)
    assert lines == ["# REORDER ordered pvalue >= 0.01 kinds = cn",
                     "d1ubia_  56 7 12.5 1e-09 4 0.25 circ 8 1 5",
                     "  1   2", "  2   3", "  3   1",
                     "a        9 1.125 0.5 0.0625 -3 1 perm 3 2 0",
                     "  1   3", "  3   1"]
    fit = np.zeros(1, search._FIT_DTYPE)[0]
    fit["a"], fit["b"], fit["rows"], fit["censored"], fit["below"], fit["fitted"] = 1.5, 0.25, 14, 1, 2, 1
    lines = report.reorder_table(["a"], rows[:0], maps[:0], 3, 0, rl.SEQ | rl.CIRC | rl.PERM, base_fit=fit)
    assert lines == ["# REORDER ordered pvalue >= 0 kinds = scn", "# GUMBEL ordered a = 1.5 b = 0.25 rows = 14 censored = 1 below = 2"]
    fit["fitted"] = 0
    assert report.reorder_table(["a"], rows[:0], maps[:0], 3, 1, rl.SEQ, base_fit=fit)[1] == "# GUMBEL ordered not fitted"


# ---------------------------------------------------------------- 5. header, build
def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "satabsearch.h")).read()
    assert "12 bytes a row" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"\s+", " ", text)
    for decl in ("int sat_baseline_keep(sat_ctx *ctx);", "int sat_baseline_drop(sat_ctx *ctx);",
                 "int sat_baseline_results(sat_ctx *ctx, int32_t *scores, double *pvalues);",
                 "int sat_reorder_hits(sat_ctx *ctx, double max_pvalue, double min_base_pvalue, int kinds, int max_rows, int32_t *counts, "
                 "int capacity, sat_reorder_hit *rows, int32_t *ssemaps);",
                 "int sat_search_reordered(sat_ctx *ctx, int maxstart, double censor, double *kernel_ms);",
                 "int sat_multi_baseline_keep(sat_multi *m);",
                 "int sat_multi_reorder_hits(sat_multi *m, double max_pvalue, double min_base_pvalue, int kinds, int max_rows, int32_t *counts, "
                 "int capacity, sat_reorder_hit *rows, int32_t *ssemaps);",
                 "int sat_multi_search_reordered(sat_multi *m, int maxstart, double censor, double *wall_ms);"):
        assert decl in text, decl
        assert decl[4:decl.index("(")] in _native.ABI_SYMBOLS
    assert ("typedef struct sat_reorder_hit { sat_hit hit; double base_pvalue; int32_t base_score; int32_t kind; int32_t matched; "
            "int32_t descents; int32_t cut; int32_t pad; } sat_reorder_hit;") in text
    assert search._REORDER_DTYPE.itemsize == 64
    host = open(os.path.join(HOST, "sat_reorder.h")).read()
    host = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", host, flags=re.S))
    assert "int32_t sat_map_kind(const int32_t *map, int32_t n1, int32_t *matched, int32_t *descents, int32_t *cut);" in host
    for name, bit in (("SAT_KIND_SEQUENTIAL", 1), ("SAT_KIND_CIRCULAR", 2), ("SAT_KIND_PERMUTED", 4)):
        assert "#define %s %d" % (name, bit) in host and "#define %s %d" % (name, bit) in text


def test_the_selection_is_a_translation_unit_of_the_device_library(monkeypatch):
    """sat_reorder.hip is in build.DEVICE_SOURCES and build_device() compiles it once for gfx950 to an object the library
    links; libsathost.so holds the host file (the commands are recorded, not run).  The predicate, the block count and
    the chunk walk are shared, not copied, the map's order is the host header's text, and sat_topk.hip's kernels are
    left alone; the command line reaches the new calls through weak references."""
    from cuda_satabsearch_amd import build
    assert "sat_reorder.hip" in build.DEVICE_SOURCES
    cmds = []
    monkeypatch.setattr(build, "_run", cmds.append)
    build.build_device(force=True)
    build.build_host(force=True)
    compiles = [c for c in cmds if "-c" in c and c[-1] == os.path.join(build.CSRC, "sat_reorder.hip")]
    assert len(compiles) == 1 and "--offload-arch=gfx950" in compiles[0]
    obj = compiles[0][compiles[0].index("-o") + 1]
    links = [c for c in cmds if "-shared" in c and c[c.index("-o") + 1] == build.DEVICE_LIB[0]]
    assert len(links) == 1 and "-Wl," + obj in links[0]
    host = [c for c in cmds if "-shared" in c and c[c.index("-o") + 1] == os.path.join(build.PKG, "libsathost.so")]
    assert len(host) == 1 and os.path.join(build.HOST, "sat_reorder.c") in host[0]
    assert "sat_reorder.hip" in open(os.path.join(ROOT, "Makefile")).read()
    text = open(os.path.join(build.CSRC, "sat_reorder.hip")).read()
    assert '#include "sat_hitrow.hpp"' in text and '#include "sat_cutoff.hpp"' in text and '#include "host/sat_reorder.h"' in text
    assert "struct HitQuery {" not in text and "bool cutoff_row(" not in text and "cutoff_row(scores" in text
    assert "block_count(hit" in text and "sat_row_chunks(ctx, kCutoffBlock" in text
    assert "sat_map_walk_add(" in text and "descents++" not in text
    main = open(os.path.join(HOST, "sat_main.c")).read()
    assert "#pragma weak sat_multi_reorder_hits\n" in main and "#pragma weak sat_multi_baseline_keep\n" in main
    assert hasattr(_native.host_lib(), "sat_map_kind")
