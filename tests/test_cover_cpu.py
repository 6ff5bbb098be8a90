"""Clustering around representatives (-a -D P, sat_cover_*) without a GPU: the two host functions of
csrc/host/sat_cover.h against cover_lib's naive loop on random and named graphs, their bad arguments, the same code
under the sanitizers as a stand-alone program, the command line's refusals and usage text, the declarations of the
header, and the new translation unit in the recorded build commands."""
import os
import re
import subprocess

import numpy as np
import pytest

from cuda_satabsearch_amd import _native, report

import cover_lib
import edge_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
HOST = os.path.join(ROOT, "cuda_satabsearch_amd", "csrc", "host")


def check(n, a, b, what=""):
    """report.cover_greedy and report.cover_sizes against cover_lib on the pairs (a[i], b[i]); returns cover_lib's tuple"""
    want = cover_lib.cover(n, a, b)
    rep, degree, rounds = report.cover_greedy(n, a, b)
    assert rep.dtype == np.int32 and degree.dtype == np.int32
    cover_lib.same((rep, degree, int(degree.sum()) // 2, rounds), want, what)
    sizes, clusters = report.cover_sizes(rep)
    assert np.array_equal(sizes, want[1]), what
    assert clusters == int((want[0] == np.arange(n)).sum()) == rounds + int((want[1] == 1).sum()), what
    cover_lib.check_invariants(n, a, b, rep)
    return want


# ---------------------------------------------------------------- 1. sat_cover_greedy, sat_cover_sizes
def test_random_graphs():
    rng = np.random.default_rng(17)
    sizes = [1, 2, 3, 63, 64, 65, 128, 129, 300] + rng.integers(1, 301, size=41).tolist()
    assert len(sizes) == 50
    for n in sizes:
        # few distinct degrees, so that ties abound: about d / 2 pairs a node, d in 0 .. 3, self pairs and repeats among them
        pairs = int(n * rng.integers(0, 4) / 2)
        a, b = rng.integers(0, n, pairs), rng.integers(0, n, pairs)
        want = check(n, a, b, "n = %d, %d pairs" % (n, pairs))
        # the result is the edge set's: the pairs reversed, shuffled and repeated change nothing
        order = rng.permutation(2 * pairs)
        rep, degree, rounds = report.cover_greedy(n, np.concatenate([b, a])[order], np.concatenate([a, b])[order])
        cover_lib.same((rep, degree, int(degree.sum()) // 2, rounds), want, "n = %d, doubled" % n)


def test_path_of_4():
    """0 - 1 - 2 - 3: single linkage has one cluster.  The gains are 2 3 3 2; nodes 1 and 2 tie and the smaller index
    wins, so 1 takes {0, 1, 2}.  Node 3 is left with no unassigned neighbour: gain 1, its own representative."""
    want = check(4, [0, 1, 2], [1, 2, 3])
    assert want[0].tolist() == [1, 1, 1, 3] and want[1].tolist() == [3, 3, 3, 1] and want[4] == 1
    assert cover_lib.components(4, [0, 1, 2], [1, 2, 3]) == 1


def test_named_graphs():
    rng = np.random.default_rng(5)
    n = 200
    order = rng.permutation(n - 1)
    want = check(n, order + 1, order, "path of 200, dealt in shuffled order")
    assert want[0][:6].tolist() == [1, 1, 1, 4, 4, 4] and want[4] == 67 and want[0][198:].tolist() == [198, 198]
    want = check(n, np.full(n - 1, n - 1), np.arange(n - 1), "star")
    assert (want[0] == n - 1).all() and (want[1] == n).all() and want[4] == 1
    # two stars sharing leaves: hub 0 has the leaves 2 .. 50, hub 1 the leaves 30 .. 100.  Hub 1 has the larger gain, is
    # picked first and takes the shared leaves 30 .. 50
    a = np.concatenate([np.zeros(49, int), np.ones(71, int)])
    b = np.concatenate([np.arange(2, 51), np.arange(30, 101)])
    want = check(101, a, b, "two stars sharing leaves")
    assert (want[0][30:101] == 1).all() and (want[0][2:30] == 0).all() and want[0][:2].tolist() == [0, 1] and want[4] == 2
    clique = [(i, j) for i in range(70) for j in range(i)]
    want = check(70, [c[0] for c in clique], [c[1] for c in clique], "clique")
    assert not want[0].any() and (want[2] == 69).all() and want[4] == 1
    want = check(n, np.arange(1, n, 2), np.arange(0, n, 2), "perfect matching")
    assert want[4] == n // 2 and np.array_equal(want[0], np.arange(n) // 2 * 2)        # every representative the smaller end
    want = check(n, [], [], "no edges")
    assert np.array_equal(want[0], np.arange(n)) and want[4] == 0 and want[3] == 0 and (want[1] == 1).all()
    want = check(5, [2, 1, 0, 3, 0, 4], [2, 1, 3, 0, 3, 4], "self pairs and repeated pairs only")
    assert want[0].tolist() == [0, 1, 2, 0, 4] and want[2].tolist() == [1, 0, 0, 1, 0] and want[3] == 1


def test_bad_arguments_are_refused():
    host = _native.host_lib()
    a, b = np.array([0, 1], np.int32), np.array([1, 2], np.int32)
    rep, deg, size = np.empty(3, np.int32), np.empty(3, np.int32), np.empty(3, np.int32)
    assert host.sat_cover_greedy(3, 2, a.ctypes.data, b.ctypes.data, rep.ctypes.data, deg.ctypes.data) == 1
    assert host.sat_cover_greedy(3, 2, a.ctypes.data, b.ctypes.data, rep.ctypes.data, None) == 1      # degree may be NULL
    assert host.sat_cover_greedy(0, 0, a.ctypes.data, b.ctypes.data, rep.ctypes.data, deg.ctypes.data) == -1
    assert host.sat_cover_greedy(3, -1, a.ctypes.data, b.ctypes.data, rep.ctypes.data, deg.ctypes.data) == -1
    assert host.sat_cover_greedy(3, 2, None, b.ctypes.data, rep.ctypes.data, deg.ctypes.data) == -1
    assert host.sat_cover_greedy(3, 2, a.ctypes.data, None, rep.ctypes.data, deg.ctypes.data) == -1
    assert host.sat_cover_greedy(3, 2, a.ctypes.data, b.ctypes.data, None, deg.ctypes.data) == -1
    assert host.sat_cover_greedy(2, 2, a.ctypes.data, b.ctypes.data, rep.ctypes.data, deg.ctypes.data) == -1     # node 2 of 2
    bad = np.array([-1, 1], np.int32)
    assert host.sat_cover_greedy(3, 2, bad.ctypes.data, b.ctypes.data, rep.ctypes.data, deg.ctypes.data) == -1
    for table in ([1, 2, 2], [0, 3, 2], [0, -1, 2]):
        t = np.array(table, np.int32)
        assert host.sat_cover_sizes(3, t.ctypes.data, size.ctypes.data) == -1
        with pytest.raises(ValueError):
            report.cover_sizes(t)
    t = np.array([1, 1, 2], np.int32)
    assert host.sat_cover_sizes(0, t.ctypes.data, size.ctypes.data) == -1
    assert host.sat_cover_sizes(3, None, size.ctypes.data) == -1 and host.sat_cover_sizes(3, t.ctypes.data, None) == -1
    with pytest.raises(ValueError):
        report.cover_greedy(3, [0, 3], [1, 1])
    with pytest.raises(ValueError):
        report.cover_greedy(3, [0], [1, 1])


# ---------------------------------------------------------------- 2. the host code under the sanitizers
def test_host_code_under_the_sanitizers(tmp_path):
    """sat_cover.c and tests/native/cover_check.c - a stand-alone program with its own main that replays the named
    graphs against tables written out in its source - built with -fsanitize=address,undefined and run as a child; no
    report may appear.  Nothing is loaded into Python, nothing is preloaded."""
    exe = str(tmp_path / "cover_check")
    build = subprocess.run(["gcc", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-Wall", "-Wextra", "-I", HOST, "-o", exe, os.path.join(ROOT, "tests", "native", "cover_check.c"),
                            os.path.join(HOST, "sat_cover.c")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == "cover_check: ok\n"
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr and run.stderr == ""


# ---------------------------------------------------------------- 3. command line
def run(golden_dir, args, stdin=b""):
    return subprocess.run([CLI] + args, input=stdin, cwd=golden_dir, capture_output=True)


@pytest.mark.parametrize("args,message", [
    (["-c", "-a", ec.EDGE_DB, "-D", "0.001"], b"ERROR: -D cannot be combined with -c\n"),
    (["-D", "0.001"], b"ERROR: -D needs -a dbfile\n"),
    (["-q", ec.EDGE_DB, "-D", "0.001"], b"ERROR: -D needs -a dbfile\n"),
    (["-Q", ec.EDGE_DB, "-D", "0.001"], b"ERROR: -D needs -a dbfile\n"),
    (["-a", ec.EDGE_DB, "-D", "0.001", "-k", "3"], b"ERROR: -D cannot be combined with -k\n"),
    (["-a", ec.EDGE_DB, "-D", "0.001", "-p", "0.5"], b"ERROR: -D cannot be combined with -p\n"),
    (["-a", ec.EDGE_DB, "-D", "0.001", "-m", "2"], b"ERROR: -D cannot be combined with -m\n"),
    (["-a", ec.EDGE_DB, "-D", "0.001", "-M", "2"], b"ERROR: -D cannot be combined with -M\n"),
    (["-a", ec.EDGE_DB, "-D", "0.001", "-R", "64"], b"ERROR: -D cannot be combined with -R\n"),
    (["-a", ec.EDGE_DB, "-D", "0.001", "-C", "5"], b"ERROR: -D cannot be combined with -C\n"),
    (["-a", ec.EDGE_DB, "-D", "0.001", "-L", "0.001"], b"ERROR: -D cannot be combined with -L\n"),
    (["-a", ec.EDGE_DB, "-D", "0.001", "-H", "0.001,0.01"], b"ERROR: -D cannot be combined with -H\n"),
    (["-a", ec.EDGE_DB, "-D", "0.001", "-E", "f"], b"ERROR: -D cannot be combined with -E\n"),
])
def test_cli_refusals(golden_dir, args, message):
    p = run(golden_dir, args, b"not read\n")
    assert p.returncode == 1, p.stderr
    assert message in p.stderr, p.stderr
    assert p.stderr.count(b"ERROR:") == 1 and p.stdout == b""
    # nothing after the option checks ran: no banner, no device query
    assert b"MAXDIM" not in p.stderr and b"HIP device" not in p.stderr


@pytest.mark.parametrize("value", ["-0.1", "1.5", "nan", "inf", "1e-3x", ""])
def test_cli_refuses_a_cutoff_outside_0_1(golden_dir, value):
    p = run(golden_dir, ["-a", ec.EDGE_DB, "-D", value])
    assert p.returncode == 1 and p.stdout == b""
    assert b"ERROR: -D needs a p-value in [0, 1] (got '" + value.encode() + b"')\n" in p.stderr
    assert b"Usage:" in p.stderr and b"MAXDIM" not in p.stderr


def test_usage_names_the_option(golden_dir):
    p = run(golden_dir, ["-x"])
    assert p.returncode == 1 and p.stdout == b""
    assert b"       [-E classfile [-N n]] [-D P]\n" in p.stderr
    assert b"  -D P : with -a dbfile: cluster the database around representatives on the GPU" in p.stderr
    assert b"(not with -c, -k, -p, -m, -M, -R, -C, -L, -H, -E)" in p.stderr
    # the older text stays, byte for byte
    for older in (b"[-k K] [-p P] [-m M] [-M M] [-R restarts [-C C]] [-F censor] [-P T] [-A] [-L P] [-b] [-H P1,P2,...]\n",
                  b"  -L P : with -a dbfile: cluster the database on the GPU - single linkage over the rows whose p-value\n",
                  b"  -H P1,P2,... : with -a dbfile: cluster the database at 1..8 ascending p-values (each 0..1) in ONE run",
                  b"  -E classfile : with -a dbfile or -Q dbfile: score the search against a classification on the GPU",
                  b"  -N n : with -E: the negatives ROC-n counts up to (n >= 1). Default 50\n",
                  b"  -b : cache the parsed database as dbfile.satbin\n"):
        assert older in p.stderr, older
    p = run(golden_dir, ["-D"])                  # the option without its argument is a usage error too
    assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""


# ---------------------------------------------------------------- 4. header, build
def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "satabsearch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for decl in ("int sat_cover_begin(sat_ctx *ctx, int n_nodes);",
                 "int sat_cover_add(sat_ctx *ctx, double max_pvalue, const int32_t *query_node);",
                 "int sat_cover_solve(sat_ctx *ctx, int32_t *rep, int32_t *degree, unsigned long long *edges, int *rounds);",
                 "int sat_cover_end(sat_ctx *ctx);",
                 "int sat_multi_cover_begin(sat_multi *m);",
                 "int sat_multi_cover_add(sat_multi *m, double max_pvalue, const int32_t *query_node);",
                 "int sat_multi_cover_solve(sat_multi *m, int32_t *rep, int32_t *degree, unsigned long long *edges, int *rounds);"):
        assert decl in text, decl
        assert decl[4:decl.index("(")] in _native.ABI_SYMBOLS
    assert "#define SAT_COVER_ROUND_BATCH %d\n" % _native.COVER_ROUND_BATCH in text
    host = open(os.path.join(HOST, "sat_cover.h")).read()
    host = re.sub(r"/\*.*?\*/", "", host, flags=re.S)
    assert "int sat_cover_sizes(int n, const int32_t *rep, int32_t *size);" in host
    assert "int sat_cover_greedy(int n, long long n_pairs, const int32_t *a, const int32_t *b, int32_t *rep, int32_t *degree);" in host
    for inline in ("sat_cover_stride(", "sat_cover_word(", "sat_cover_bit(", "sat_cover_key("):
        assert host.count("SAT_COVER_FN") > 4 and inline in host


def test_the_cover_is_a_translation_unit_of_the_device_library(monkeypatch):
    """sat_cover.hip is in build.DEVICE_SOURCES and build_device() compiles it once for gfx950 to an object the library
    links, with the host file's object beside it; libsathost.so holds the host file too (the commands are recorded, not
    run).  The predicate and the chunk walk are shared, not copied, and so are the matrix layout and the key."""
    from cuda_satabsearch_amd import build
    assert "sat_cover.hip" in build.DEVICE_SOURCES
    cmds = []
    monkeypatch.setattr(build, "_run", cmds.append)
    build.build_device(force=True)
    build.build_host(force=True)
    compiles = [c for c in cmds if "-c" in c and c[-1] == os.path.join(build.CSRC, "sat_cover.hip")]
    assert len(compiles) == 1 and "--offload-arch=gfx950" in compiles[0]
    assert len([c for c in cmds if "-c" in c and c[0] == build.HIPCC]) == len(build.DEVICE_SOURCES)
    obj = compiles[0][compiles[0].index("-o") + 1]
    links = [c for c in cmds if "-shared" in c and c[c.index("-o") + 1] == build.DEVICE_LIB[0]]
    assert len(links) == 1 and "-Wl," + obj in links[0]
    assert "-Wl," + os.path.join(build.PKG, "sat_cover.o") in links[0] and obj != os.path.join(build.PKG, "sat_cover.o")
    host = [c for c in cmds if "-shared" in c and c[c.index("-o") + 1] == os.path.join(build.PKG, "libsathost.so")]
    assert len(host) == 1 and os.path.join(build.HOST, "sat_cover.c") in host[0]
    assert "sat_cover.hip" in open(os.path.join(ROOT, "Makefile")).read()
    text = open(os.path.join(build.CSRC, "sat_cover.hip")).read()
    assert '#include "sat_hitrow.hpp"' in text and '#include "sat_cutoff.hpp"' in text and '#include "host/sat_cover.h"' in text
    assert "struct HitQuery {" not in text and "bool cutoff_row(" not in text and "cutoff_row(scores" in text
    assert "sat_row_chunks(ctx, kCutoffBlock" in text and "sat_cover_key(" in text and "sat_cover_key_node(" in text
    # no cooperative launch, no grid-wide barrier: kernel boundaries only
    assert "hipLaunchCooperativeKernel" not in text and "cooperative_groups" not in text and "grid.sync" not in text
    assert "__global__" not in open(os.path.join(build.CSRC, "sat_capi.hip")).read()
    import ctypes as C
    lib = C.CDLL(_native.DEVICE_LIB)
    assert hasattr(lib, "sat_cover_sizes") and hasattr(_native.host_lib(), "sat_cover_greedy")
