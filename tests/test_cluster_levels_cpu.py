"""Clustering at several p-values in one pass (-a -H P1,..,PL, sat_cluster_*_levels) without a GPU: sat_cluster_nested of
csrc/host/sat_cluster.h against a Python check, report.cluster_levels_table against report.cluster_table per level, the
command line's refusals, list parsing and usage text, the declarations of the headers, the build commands - and the
planted score classes tests/test_gpu_cluster_levels.py uses, each strictly between its two neighbouring cutoffs."""
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import _native, report

import edge_cases as ec
from test_cluster_cpu import components

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")

# ---------------------------------------------------------------- the planted classes of the GPU tests
LEVELS = (1e-5, 1e-4, 1e-3, 0.05, 0.5)
CLASSES = (5, 4, 3, 2, 1, 0)                   # integer norm2; class k first qualifies at level 5 - k (0-based), class 0 nowhere
PLANTED_N, PLANTED_ORDERS = 1500, (8, 20)


def planted_score(k, n1, n2):
    """the smallest score whose norm2 = 2 * score / (n1 + n2) is >= k: the built-in table is indexed by int(norm2) = k"""
    return (k * (n1 + n2) + 1) // 2


def first_level(k):
    """the 0-based level at which class k first qualifies, len(LEVELS) for class 0"""
    return len(LEVELS) - k if k > 0 else len(LEVELS)


def test_planted_classes_lie_strictly_between_their_cutoffs():
    db = sat.synth.make_db(PLANTED_N, *PLANTED_ORDERS, sort=False)
    lo, hi = int(db.orders.min()), int(db.orders.max())
    assert (lo, hi) == PLANTED_ORDERS
    bounds = (0.0,) + LEVELS + (1.0,)
    for n1 in (lo, hi):
        for n2 in (lo, hi):
            for k in CLASSES:
                norm2, _, p = report.stats(planted_score(k, n1, n2), n1, n2)
                assert int(norm2) == k
                j = first_level(k)
                assert bounds[j] < p < bounds[j + 1], (k, n1, n2, p)


# ---------------------------------------------------------------- 1. sat_cluster_nested
def nested_by_definition(labels):
    """what sat_cluster_nested returns, by its definition: -1 unless every level is canonical, else the first level
    (from 1) whose clusters do not each lie inside one cluster of the next level, else 0"""
    levels, n = labels.shape
    for lab in labels:
        for v in range(n):
            if not 0 <= lab[v] <= v or lab[lab[v]] != lab[v]:
                return -1
    for j in range(levels - 1):
        for l in set(labels[j].tolist()):
            if len(set(labels[j + 1][labels[j] == l].tolist())) != 1:
                return j + 1
    return 0


def nested(labels):
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    return _native.host_lib().sat_cluster_nested(lab.shape[1], lab.shape[0], lab.ctypes.data)


def random_chain(rng, n, levels):
    """levels labellings of n nodes, each made from the one before by more edges: nested by construction"""
    edges, out = [], []
    for _ in range(levels):
        edges += rng.integers(0, n, size=(int(rng.integers(0, max(2, n // levels))), 2)).tolist()
        out.append(components(n, edges))
    return np.array(out, np.int32)


def test_nested_chains_and_broken_ones():
    rng = np.random.default_rng(5)
    sizes = [1, 2, 3, 64, 65, 300] + rng.integers(1, 301, size=34).tolist()
    broken_seen = 0
    for i, n in enumerate(sizes):
        levels = 1 + i % 8
        chain = random_chain(rng, n, levels)
        assert nested_by_definition(chain) == 0 and nested(chain) == 0
        if levels == 1:
            continue
        # one level replaced by a labelling of its own edges: in general not nested any more
        bad = chain.copy()
        j = int(rng.integers(0, levels))
        bad[j] = components(n, rng.integers(0, n, size=(max(1, n // 3), 2)).tolist())
        want = nested_by_definition(bad)
        assert nested(bad) == want
        broken_seen += want > 0
        # the chain upside down: the loosest level first
        want = nested_by_definition(chain[::-1])
        assert nested(chain[::-1]) == want
        broken_seen += want > 0
    assert broken_seen >= 20


def test_nested_reports_the_first_broken_pair():
    fine = np.array([0, 0, 2, 2, 4, 5], np.int32)
    coarse = np.array([0, 0, 0, 0, 4, 4], np.int32)
    other = np.array([0, 1, 1, 3, 3, 5], np.int32)              # cuts across `fine`
    assert nested([fine, coarse]) == 0 and nested([fine, fine, coarse, coarse]) == 0
    assert nested([coarse, fine]) == 1
    assert nested([fine, coarse, fine]) == 2
    assert nested([fine, other, coarse]) == 1
    assert nested([fine, coarse, coarse, other]) == 3
    assert nested([other]) == 0


def test_nested_refuses_non_canonical_labels_and_bad_arguments():
    host = _native.host_lib()
    ok = np.array([[0, 0, 2, 3], [0, 0, 2, 2]], np.int32)
    assert nested(ok) == 0
    # a label above its node, a label that is not its own label, a label outside the nodes - at either level
    for bad_level in ([1, 1, 2, 3], [0, 0, 1, 3], [0, -1, 2, 3], [0, 4, 2, 3]):
        for j in (0, 1):
            bad = ok.copy()
            bad[j] = bad_level
            assert nested(bad) == -1 == nested_by_definition(bad)
    assert host.sat_cluster_nested(0, 2, ok.ctypes.data) == -1
    assert host.sat_cluster_nested(4, 0, ok.ctypes.data) == -1
    assert host.sat_cluster_nested(-4, 2, ok.ctypes.data) == -1
    assert host.sat_cluster_nested(4, 2, None) == -1


# ---------------------------------------------------------------- 2. report.cluster_levels_table
def test_levels_table_is_cluster_table_per_level():
    rng = np.random.default_rng(8)
    for n, levels in ((1, 1), (7, 3), (300, 8), (129, 5)):
        chain = random_chain(rng, n, levels)
        degrees = rng.integers(0, 4, size=(levels, n)).astype(np.int32)
        reps, sizes = report.cluster_levels_table(chain, degrees)
        assert reps.shape == sizes.shape == (levels, n) and reps.dtype == sizes.dtype == np.int32
        for j in range(levels):
            want = report.cluster_table(chain[j], degrees[j])
            assert np.array_equal(reps[j], want[0]) and np.array_equal(sizes[j], want[1])


def test_levels_table_refuses_what_nested_refuses():
    fine = np.array([0, 0, 2, 2], np.int32)
    coarse = np.array([0, 0, 0, 0], np.int32)
    zeros = np.zeros((2, 4), np.int32)
    report.cluster_levels_table([fine, coarse], zeros)
    with pytest.raises(ValueError, match="not nested.*level 1"):
        report.cluster_levels_table([coarse, fine], zeros)
    with pytest.raises(ValueError, match="not canonical"):
        report.cluster_levels_table([fine, [1, 1, 1, 1]], zeros)
    with pytest.raises(ValueError, match=r"\[levels, n\]"):
        report.cluster_levels_table(fine, zeros)
    with pytest.raises(ValueError, match=r"\[levels, n\]"):
        report.cluster_levels_table([fine, coarse], zeros[:1])


# ---------------------------------------------------------------- 3. command line
def run(golden_dir, args, stdin=b""):
    return subprocess.run([CLI] + args, input=stdin, cwd=golden_dir, capture_output=True)


H = "1e-4,1e-3"


@pytest.mark.parametrize("args,message", [
    (["-c", "-a", ec.EDGE_DB, "-H", H], b"ERROR: -H cannot be combined with -c\n"),
    (["-H", H], b"ERROR: -H needs -a dbfile\n"),
    (["-q", ec.EDGE_DB, "-H", H], b"ERROR: -H needs -a dbfile\n"),
    (["-Q", ec.EDGE_DB, "-H", H], b"ERROR: -H needs -a dbfile\n"),
    (["-a", ec.EDGE_DB, "-H", H, "-L", "0.001"], b"ERROR: -H cannot be combined with -L\n"),
    (["-a", ec.EDGE_DB, "-L", "0.001", "-H", H], b"ERROR: -H cannot be combined with -L\n"),
    (["-a", ec.EDGE_DB, "-H", H, "-k", "3"], b"ERROR: -H cannot be combined with -k\n"),
    (["-a", ec.EDGE_DB, "-H", H, "-p", "0.5"], b"ERROR: -H cannot be combined with -p\n"),
    (["-a", ec.EDGE_DB, "-H", H, "-m", "2"], b"ERROR: -H cannot be combined with -m\n"),
    (["-a", ec.EDGE_DB, "-H", H, "-M", "2"], b"ERROR: -H cannot be combined with -M\n"),
    (["-a", ec.EDGE_DB, "-H", H, "-R", "64"], b"ERROR: -H cannot be combined with -R\n"),
    (["-a", ec.EDGE_DB, "-H", H, "-C", "5"], b"ERROR: -H cannot be combined with -C\n"),
])
def test_cli_refusals(golden_dir, args, message):
    p = run(golden_dir, args, b"not read\n")
    assert p.returncode == 1, p.stderr
    assert message in p.stderr, p.stderr
    assert p.stderr.count(b"ERROR:") == 1 and p.stdout == b""
    # nothing after the option checks ran: no banner, no device query
    assert b"MAXDIM" not in p.stderr and b"HIP device" not in p.stderr


@pytest.mark.parametrize("value", ["", "0.1,", ",0.1", "0.2,0.1", "0.1,0.1", "0.1,,0.2", "1e-9,1e-8,1e-7,1e-6,1e-5,1e-4,1e-3,1e-2,1e-1",
                                   "1.5", "0.1,1.5", "-0.1", "nan", "0.1,nan", "inf", "1e-3x", "0.1;0.2", "0.1, 0.2x"])
def test_cli_refuses_a_bad_list(golden_dir, value):
    p = run(golden_dir, ["-a", ec.EDGE_DB, "-H", value])
    assert p.returncode == 1 and p.stdout == b""
    assert b"ERROR: -H needs 1..8 ascending p-values in [0, 1] (got '" + value.encode() + b"')\n" in p.stderr
    assert b"Usage:" in p.stderr and b"MAXDIM" not in p.stderr and b"HIP device" not in p.stderr


def test_usage_names_the_option_and_keeps_the_older_text(golden_dir):
    p = run(golden_dir, ["-x"])
    assert p.returncode == 1 and p.stdout == b""
    assert b"[-A] [-L P] [-b] [-H P1,P2,...]" in p.stderr
    assert b"  -H P1,P2,... : with -a dbfile: cluster the database at 1..8 ascending p-values" in p.stderr
    assert b"(not with -c, -L, -k, -p, -m, -M, -R, -C)" in p.stderr
    # what the older tests pin
    assert b"[-A] [-L P] [-b]" in p.stderr
    assert b"  -L P : with -a dbfile: cluster the database on the GPU" in p.stderr
    assert b"name representative cluster_size degree" in p.stderr
    p = run(golden_dir, ["-H"])                  # the option without its argument is a usage error too
    assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""


# ---------------------------------------------------------------- 4. headers, build
def test_headers_declare_the_calls():
    text = open(os.path.join(ROOT, "include", "satabsearch.h")).read()
    assert re.search(r"^#define SAT_MAX_CLUSTER_LEVELS 8\b", text, re.M)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for decl in ("int sat_cluster_begin_levels(sat_ctx *ctx, int n_nodes, int n_levels, const double *max_pvalue);",
                 "int sat_cluster_add_levels(sat_ctx *ctx, const int32_t *query_node);",
                 "int sat_cluster_labels_levels(sat_ctx *ctx, int32_t *label, int32_t *degree, unsigned long long *edges);",
                 "int sat_multi_cluster_begin_levels(sat_multi *m, int n_levels, const double *max_pvalue);",
                 "int sat_multi_cluster_add_levels(sat_multi *m, const int32_t *query_node);",
                 "int sat_multi_cluster_labels_levels(sat_multi *m, int32_t *label, int32_t *degree, unsigned long long *edges);"):
        assert decl in text, decl
        assert decl[4:decl.index("(")] in _native.ABI_SYMBOLS
    assert _native.MAX_CLUSTER_LEVELS == 8
    host = open(os.path.join(ROOT, "cuda_satabsearch_amd", "csrc", "host", "sat_cluster.h")).read()
    host = re.sub(r"/\*.*?\*/", "", host, flags=re.S)
    assert "int sat_cluster_nested(int n, int n_levels, const int32_t *labels);" in host


def test_the_leveled_kernels_live_in_the_clustering_translation_unit(monkeypatch):
    """cluster_add_levels is a kernel of sat_cluster.hip, which is still ONE translation unit of the device library
    (the commands are recorded, not run), and takes the row's p-value from the shared header's functions without
    defining them again."""
    from cuda_satabsearch_amd import build
    cmds = []
    monkeypatch.setattr(build, "_run", cmds.append)
    build.build_device(force=True)
    build.build_host(force=True)
    compiles = [c for c in cmds if "-c" in c and c[-1] == os.path.join(build.CSRC, "sat_cluster.hip")]
    assert len(compiles) == 1 and "--offload-arch=gfx950" in compiles[0]
    assert len([c for c in cmds if "-c" in c and c[0] == build.HIPCC]) == len(build.DEVICE_SOURCES)      # no new unit
    host = [c for c in cmds if "-shared" in c and c[c.index("-o") + 1] == os.path.join(build.PKG, "libsathost.so")]
    assert len(host) == 1 and os.path.join(build.HOST, "sat_cluster.c") in host[0]
    text = open(os.path.join(build.CSRC, "sat_cluster.hip")).read()
    for kernel in ("cluster_add_levels(", "cluster_init_levels(", "cluster_labels_levels("):
        assert re.search(r"__global__ void (__launch_bounds__\(kCutoffBlock\) )?" + re.escape(kernel), text), kernel
    assert "hit_row(" in text and "sat_hit hit_row(" not in text and "bool cutoff_row(" not in text and "struct HitQuery {" not in text
    shared = open(os.path.join(build.CSRC, "sat_hitrow.hpp")).read()
    assert shared.count("struct HitQuery {") == 1 and shared.count("bool cutoff_row(") == 1 and shared.count("sat_hit hit_row(") == 1
