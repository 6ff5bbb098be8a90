"""A query's SSEs profiled over its hits (-W P, sat_profile_rows) without a GPU: the conserved core of
csrc/host/sat_profile.h against profile_lib's restatement of its rule on random and hand-made matrices, the same C under
the sanitizers as a stand-alone program, the command line's refusals, the -c goldens through the new binary, the table
report.profile_table renders, and the declarations and build lists."""
import os
import re
import subprocess

import numpy as np
import pytest

from cuda_satabsearch_amd import _native, report

import edge_cases as ec
import profile_lib as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
HOST = os.path.join(ROOT, "cuda_satabsearch_amd", "csrc", "host")
EXPECTED = os.path.join(ROOT, "tests", "golden", "expected")
ORDERS = (1, 2, 3, 8, 32, 111)
FRACTIONS = (0.01, 0.5, 1.0)


def random_cases():
    """(hits, joint, fraction) of a few hundred seeded random map sets: joint <= the smaller diagonal by construction"""
    rng = np.random.default_rng(2024)
    for n1 in ORDERS:
        for rows in (0, 1, 2, 7, 40, 200) + ((1000,) if n1 <= 32 else ()):
            for _ in range(3):
                hits, joint = pl.matrices(pl.random_matched(rng, n1, rows))
                for fraction in FRACTIONS:
                    yield hits, joint, fraction


def check(hits, joint, fraction, what=""):
    want = pl.core(joint, hits, fraction)
    got = report.profile_core(joint, hits, fraction)
    assert got[0].tolist() == want[0].tolist() and got[1] == want[1], (what, hits, fraction, got, want)
    # what the core promises: every two members are matched together in at least `fraction` of the hits
    m = np.flatnonzero(got[0])
    for i in m:
        for k in m:
            assert float(joint[i][k]) >= fraction * hits
    return got


# ---------------------------------------------------------------- 1. sat_profile_core
def test_random_matrices():
    count = sizes = 0
    for hits, joint, fraction in random_cases():
        assert (joint <= np.minimum.outer(np.diag(joint), np.diag(joint))).all() and (joint == joint.T).all()
        core, _ = check(hits, joint, fraction)
        count += 1
        sizes += 0 < core.sum() < len(core)
    assert count >= 300 and sizes >= 30                 # a few hundred, and many of them neither empty nor everything


def test_no_hits_and_empty_start():
    j = np.zeros((4, 4), np.uint32)
    assert check(0, j, 0.5)[0].tolist() == [False] * 4 and check(0, j, 0.5)[1] == 0
    j = np.diag([1, 2, 1, 0]).astype(np.uint32)
    core, least = check(10, j, 0.5, "no SSE reaches half of the hits")
    assert not core.any() and least == 0


def test_one_sse():
    core, least = check(5, np.array([[3]], np.uint32), 0.5)
    assert core.tolist() == [True] and least == 3
    core, least = check(5, np.array([[2]], np.uint32), 0.5)
    assert core.tolist() == [False] and least == 0
    # one SSE left of several: joint_min is its diagonal count
    j = np.array([[6, 0], [0, 5]], np.uint32)
    core, least = check(10, j, 0.5)
    assert core.tolist() == [True, False] and least == 6


def test_chain_drops_one_end_by_the_tie_rule():
    """a-b and b-c are matched together, a-c never: the pair (a, c) falls below, the diagonals tie, the larger index goes"""
    j = np.array([[6, 6, 0], [6, 10, 6], [0, 6, 6]], np.uint32)
    core, least = check(10, j, 0.5)
    assert core.tolist() == [True, True, False] and least == 6
    # the smaller diagonal goes, whatever its index
    j = np.array([[5, 5, 0], [5, 10, 6], [0, 6, 6]], np.uint32)
    core, least = check(10, j, 0.5)
    assert core.tolist() == [False, True, True] and least == 6


def test_all_equal_counts_exercise_the_tie_order():
    """every diagonal 8, every pair 3 of 10 hits: the first pair in (i, k) order is (0, 1) and loses 1, then (0, 2)
    loses 2, ... - SSE 0 alone is left"""
    j = np.full((5, 5), 3, np.uint32)
    np.fill_diagonal(j, 8)
    core, least = check(10, j, 0.5)
    assert core.tolist() == [True, False, False, False, False] and least == 8
    # the smallest joint goes first, not the first pair: (2, 3) has the smallest count and the equal diagonals drop 3;
    # then the pairs at 3 go in (i, k) order: (0, 1) drops 1, (0, 2) drops 2, (0, 4) drops 4
    j[2, 3] = j[3, 2] = 1
    j[0, 4] = j[4, 0] = 3
    core, least = check(10, j, 0.5)
    assert core.tolist() == [True, False, False, False, False] and least == 8
    j[0, 1] = j[1, 0] = 5                                # now (0, 1) holds: (2, 3) drops 3, (0, 2) drops 2, (0, 4) drops 4
    core, least = check(10, j, 0.5)
    assert core.tolist() == [True, True, False, False, False] and least == 5


def test_fraction_one_and_refused_fractions():
    j = np.array([[4, 4, 3], [4, 4, 3], [3, 3, 4]], np.uint32)
    core, least = check(4, j, 1.0)
    assert core.tolist() == [True, True, False] and least == 4
    host = _native.host_lib()
    flags = np.zeros(3, np.uint8)
    for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert pl.core(j, 4, bad) is None
        assert host.sat_profile_core(3, 4, j.ctypes.data, bad, flags.ctypes.data, None) == -1
        with pytest.raises(ValueError):
            report.profile_core(j, 4, bad)
    assert host.sat_profile_core(0, 4, j.ctypes.data, 0.5, flags.ctypes.data, None) == -1
    assert host.sat_profile_core(3, 4, None, 0.5, flags.ctypes.data, None) == -1
    assert host.sat_profile_core(3, 4, j.ctypes.data, 0.5, None, None) == -1
    assert host.sat_profile_core(3, 4, j.ctypes.data, 0.5, flags.ctypes.data, None) == 3          # joint_min may be NULL
    with pytest.raises(ValueError):
        report.profile_core(np.zeros((2, 3), np.uint32), 1, 0.5)


# ---------------------------------------------------------------- 2. the host code under the sanitizers
def test_host_code_under_the_sanitizers(tmp_path):
    """sat_profile.c and tests/native/profile_check.c - a stand-alone program with its own main that reads cases on stdin
    and prints the results - built plainly and with -fsanitize=address,undefined; both run as children on the same cases.
    The outputs are equal, they are what profile_lib computes, and no report appears.  Nothing is loaded into Python,
    nothing is preloaded."""
    cases = list(random_cases())[::3]
    j = np.array([[4, 4, 3], [4, 4, 3], [3, 3, 4]], np.uint32)
    cases += [(4, j, bad) for bad in (0.0, -0.5, 1.5, float("nan"))] + [(0, j, 0.5), (4, j, 1.0)]
    text = "".join("%d %d %r\n%s\n" % (len(jt), hits, float(f), " ".join(map(str, jt.ravel().tolist()))) for hits, jt, f in cases)
    want = []
    for hits, jt, f in cases:
        w = pl.core(jt, hits, f)
        want.append("-1 0" if w is None else "%d %d %s" % (w[0].sum(), w[1], " ".join(str(int(x)) for x in w[0])))
    want.append("profile_check: %d cases" % len(cases))
    outputs = []
    for name, flags in (("plain", ["-O2"]),
                        ("sanitized", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / ("profile_check_" + name))
        build = subprocess.run(["gcc"] + flags + ["-Wall", "-Wextra", "-I", HOST, "-o", exe, os.path.join(ROOT, "tests", "native", "profile_check.c"),
                                                  os.path.join(HOST, "sat_profile.c")], capture_output=True, text=True)
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


@pytest.mark.parametrize("args,message", [
    (["-c", "-a", ec.EDGE_DB, "-W", "0.001"], b"ERROR: -W cannot be combined with -c\n"),
    (["-c", "-W", "0.001"], b"ERROR: -W cannot be combined with -c\n"),
    (["-a", ec.EDGE_DB, "-W", "0.001", "-k", "3"], b"ERROR: -W cannot be combined with -k\n"),
    (["-a", ec.EDGE_DB, "-W", "0.001", "-p", "0.5"], b"ERROR: -W cannot be combined with -p\n"),
    (["-a", ec.EDGE_DB, "-W", "0.001", "-m", "2"], b"ERROR: -W cannot be combined with -m\n"),
    (["-a", ec.EDGE_DB, "-W", "0.001", "-M", "2"], b"ERROR: -W cannot be combined with -M\n"),
    (["-a", ec.EDGE_DB, "-W", "0.001", "-R", "64"], b"ERROR: -W cannot be combined with -R\n"),
    (["-a", ec.EDGE_DB, "-W", "0.001", "-C", "5"], b"ERROR: -W cannot be combined with -C\n"),
    (["-a", ec.EDGE_DB, "-W", "0.001", "-L", "0.001"], b"ERROR: -W cannot be combined with -L\n"),
    (["-a", ec.EDGE_DB, "-W", "0.001", "-H", "0.001,0.01"], b"ERROR: -W cannot be combined with -H\n"),
    (["-a", ec.EDGE_DB, "-W", "0.001", "-D", "0.001"], b"ERROR: -W cannot be combined with -D\n"),
    (["-a", ec.EDGE_DB, "-W", "0.001", "-E", "f"], b"ERROR: -W cannot be combined with -E\n"),
    (["-a", ec.EDGE_DB, "-W", "0.001", "-N", "5"], b"ERROR: -W cannot be combined with -N\n"),
    (["-q", ec.EDGE_DB, "-W", "0.001", "-P", "2"], b"ERROR: -W takes -P T only with -A\n"),
    (["-a", ec.EDGE_DB, "-f", "0.5"], b"ERROR: -f needs -W P\n"),
    (["-f", "0.5"], b"ERROR: -f needs -W P\n"),
    (["-a", ec.EDGE_DB, "-L", "0.001", "-f", "0.5"], b"ERROR: -f needs -W P\n"),
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
    p = run(golden_dir, ["-a", ec.EDGE_DB, "-W", value])
    assert p.returncode == 1 and p.stdout == b""
    assert b"ERROR: -W needs a p-value in [0, 1] (got '" + value.encode() + b"')\n" in p.stderr
    assert b"Usage:" in p.stderr and b"MAXDIM" not in p.stderr


@pytest.mark.parametrize("value", ["0", "-0.1", "1.5", "nan", "inf", "0.5x", ""])
def test_cli_refuses_a_fraction_outside_0_1(golden_dir, value):
    p = run(golden_dir, ["-a", ec.EDGE_DB, "-W", "0.001", "-f", value])
    assert p.returncode == 1 and p.stdout == b""
    assert b"ERROR: -f needs a fraction in (0, 1] (got '" + value.encode() + b"')\n" in p.stderr
    assert b"Usage:" in p.stderr and b"MAXDIM" not in p.stderr


def test_usage_names_the_options(golden_dir):
    p = run(golden_dir, ["-x"])
    assert p.returncode == 1 and p.stdout == b""
    assert b"       [-W P [-f F]]\n" in p.stderr
    assert b"  -W P : which SSEs: profile each query's SSEs over its hits on the GPU" in p.stderr
    assert b"(not with -c, -k, -p, -m, -M, -R, -C, -L, -H, -D, -E, -N)" in p.stderr
    assert b"  -f F : with -W: every two SSEs of the core are matched together in at least F (0 < F <= 1) of the hits." in p.stderr
    # the older text stays, byte for byte
    for older in (b"       [-E classfile [-N n]] [-D P]\n",
                  b"  -D P : with -a dbfile: cluster the database around representatives on the GPU",
                  b"  -b : cache the parsed database as dbfile.satbin\n"):
        assert older in p.stderr, older
    for option in ("-W", "-f"):                          # the option without its argument is a usage error too
        p = run(golden_dir, [option])
        assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""


@pytest.mark.parametrize("name", ["c1_d1ubia_small", "d2phlb1_TFT", "d2phlb1_TTT", "multiquery", "d1twfa_"])
def test_without_the_option_the_host_goldens_are_byte_identical(golden_dir, name):
    with open(os.path.join(golden_dir, name + ".input"), "rb") as f:
        p = run(golden_dir, ["-c", "-r", "128"], f.read())
    assert p.returncode == 0, p.stderr.decode()[-400:]
    assert p.stdout == open(os.path.join(EXPECTED, name + ".r128.out"), "rb").read()


# ---------------------------------------------------------------- 4. the table
def test_profile_table_renders_the_block():
    j0 = np.array([[4, 3, 1], [3, 3, 0], [1, 0, 1]], np.uint32)
    # a motif of the source's SSEs 5, 1, 8: its second SSE is never matched with the others and goes
    j1 = np.array([[2, 0, 2], [0, 1, 0], [2, 0, 2]], np.uint32)
    j2 = np.zeros((2, 2), np.uint32)
    lines = report.profile_table(["d1ubia_", "d2phlb1", "d1twfa_"], [[0, 1, 0], [0, 3, 2], ["xa", "e"]], [4, 2, 0], [j0, j1, j2],
                                 "db.ascii", 1e-3, 0.5, 16, sses=[None, [4, 0, 7], None])
    assert lines == ["# PROFILE dbfile = db.ascii pvalue <= 0.001 fraction >= 0.5 restarts = 16 queries = 3",
                     "# QUERY d1ubia_ sses = 3 hits = 4",
                     "# CORE sses = 2 joint >= 3 d1ubia_@1,2",
                     "1 e 4 4 3 1",
                     "2 xa 3 3 3 0",
                     "3 e 1 1 0 1",
                     "# QUERY d2phlb1 sses = 3 hits = 2",
                     "# QUERY SSES = 5,1,8",
                     "# CORE sses = 2 joint >= 2 d2phlb1@5,8",
                     "1 e 2 2 0 2",
                     "2 xg 1 0 1 0",
                     "3 xi 2 2 0 2",
                     "# QUERY d1twfa_ sses = 2 hits = 0",
                     "# CORE none",
                     "1 xa 0 0 0",
                     "2 e 0 0 0"]
    lines = report.profile_table(["q"], [[0]], [7], [np.array([[7]], np.uint32)], "d", 1.0, 1.0, 128, polish_all=2, gumbel=(0.05, 1))
    assert lines == ["# PROFILE dbfile = d pvalue <= 1 fraction >= 1 restarts = 128 queries = 1",
                     "# POLISH tops = 2 all rows",
                     "# GUMBEL censor = 0.05 fitted = 1 of 1",
                     "# QUERY q sses = 1 hits = 7",
                     "# CORE sses = 1 joint >= 7 q@1",
                     "1 e 7 7"]


# ---------------------------------------------------------------- 5. header, build
def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "satabsearch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"\s+", " ", text)
    for decl in ("int sat_profile_rows(sat_ctx *ctx, double max_pvalue, const int32_t *query_node, uint32_t *hits, uint32_t *joint, "
                 "const int64_t *offset);",
                 "int sat_multi_profile_rows(sat_multi *m, double max_pvalue, const int32_t *query_node, uint32_t *hits, uint32_t *joint, "
                 "const int64_t *offset);"):
        assert decl in text, decl
        assert decl[4:decl.index("(")] in _native.ABI_SYMBOLS
    host = open(os.path.join(HOST, "sat_profile.h")).read()
    host = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", host, flags=re.S))
    assert ("int sat_profile_core(int n1, uint32_t hits, const uint32_t *joint, double fraction, uint8_t *in_core, "
            "uint32_t *joint_min);") in host


def test_the_profile_is_a_translation_unit_of_the_device_library(monkeypatch):
    """sat_profile.hip is in build.DEVICE_SOURCES and build_device() compiles it once for gfx950 to an object the library
    links; libsathost.so holds the host file (the commands are recorded, not run).  The predicate, the block count and
    the chunk walk are shared, not copied; the pass has no compare-and-swap and no unbounded loop; the command line
    reaches the new calls through weak references."""
    from cuda_satabsearch_amd import build
    assert "sat_profile.hip" in build.DEVICE_SOURCES
    cmds = []
    monkeypatch.setattr(build, "_run", cmds.append)
    build.build_device(force=True)
    build.build_host(force=True)
    compiles = [c for c in cmds if "-c" in c and c[-1] == os.path.join(build.CSRC, "sat_profile.hip")]
    assert len(compiles) == 1 and "--offload-arch=gfx950" in compiles[0]
    obj = compiles[0][compiles[0].index("-o") + 1]
    links = [c for c in cmds if "-shared" in c and c[c.index("-o") + 1] == build.DEVICE_LIB[0]]
    assert len(links) == 1 and "-Wl," + obj in links[0]
    host = [c for c in cmds if "-shared" in c and c[c.index("-o") + 1] == os.path.join(build.PKG, "libsathost.so")]
    assert len(host) == 1 and os.path.join(build.HOST, "sat_profile.c") in host[0]
    assert "sat_profile.hip" in open(os.path.join(ROOT, "Makefile")).read()
    text = open(os.path.join(build.CSRC, "sat_profile.hip")).read()
    assert '#include "sat_hitrow.hpp"' in text and '#include "sat_cutoff.hpp"' in text
    assert "struct HitQuery {" not in text and "bool cutoff_row(" not in text and "cutoff_row(scores" in text
    assert "block_count(counted" in text and "sat_row_chunks(ctx, kCutoffBlock" in text
    code = re.sub(r"//[^\n]*", "", text)
    assert "atomicCAS" not in code and "while" not in code and "for (;;)" not in code
    assert "atomicAdd" in code and "__ballot(" in code and "__popcll(" in code
    # the text of the state error is sat_cutoff.hpp's, once for the selection layer
    layer = {f: open(os.path.join(build.CSRC, f)).read() for f in ("sat_cutoff.hpp", "sat_topk.hip", "sat_multi.hip", "sat_profile.hip")}
    assert [f for f, t in layer.items() if "ran without lsoln" in t] == ["sat_cutoff.hpp"] and "sat_check_lsoln(" in layer["sat_profile.hip"]
    main = open(os.path.join(HOST, "sat_main.c")).read()
    assert "#pragma weak sat_multi_profile_rows\n" in main and "#pragma weak sat_profile_core\n" in main
    assert hasattr(_native.host_lib(), "sat_profile_core")
