"""Clustering the database (-a -L P, sat_cluster_*) without a GPU: the two host functions of csrc/host/sat_cluster.h
against a small Python union-find, the command line's refusals and usage text, the declarations of the header, and the
new translation unit in the recorded build commands."""
import os
import re
import subprocess

import numpy as np
import pytest

from cuda_satabsearch_amd import _native, report

import edge_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")


# ---------------------------------------------------------------- the reference: union-find in Python
def components(n, edges):
    """label[v] = the smallest node of v's connected component under `edges` (pairs of nodes)"""
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for a, b in edges:
        a, b = find(int(a)), find(int(b))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(v) for v in range(n)], np.int32)


def table(labels, degrees):
    """(reps, sizes, clusters) by the definition: the member with the largest degree, ties to the smallest index"""
    n = len(labels)
    reps, sizes = np.empty(n, np.int32), np.empty(n, np.int32)
    for l in set(labels.tolist()):
        members = np.nonzero(labels == l)[0]
        best = members[np.argmax(degrees[members])]              # argmax returns the first of equal values
        reps[members], sizes[members] = best, len(members)
    return reps, sizes, len(set(labels.tolist()))


def scrambled(rng, labels):
    """the same partition with every component labelled by a random member instead of its smallest: what a join must
    accept too"""
    out = np.empty_like(labels)
    for l in set(labels.tolist()):
        members = np.nonzero(labels == l)[0]
        out[members] = rng.choice(members)
    return out


def check_join(n, edge_sets, rng=None):
    sets = [components(n, e) for e in edge_sets]
    want = components(n, [e for es in edge_sets for e in es])
    got = report.cluster_join(np.array(sets, np.int32))
    assert np.array_equal(got, want)
    if rng is not None:
        got = report.cluster_join(np.array([scrambled(rng, s) for s in sets], np.int32))
        assert np.array_equal(got, want)
    return want


# ---------------------------------------------------------------- 1. sat_cluster_join, sat_cluster_reps
def test_random_partitions():
    rng = np.random.default_rng(11)
    sizes = [1, 2, 3, 5, 17, 64, 65, 300] + rng.integers(1, 301, size=40).tolist()
    for n in sizes:
        nsets = int(rng.integers(1, 5))
        edge_sets = [rng.integers(0, n, size=(int(rng.integers(0, n + 1)), 2)).tolist() for _ in range(nsets)]
        labels = check_join(n, edge_sets, rng)
        degrees = rng.integers(0, 4, size=n).astype(np.int32)            # few values: many ties
        reps, sizes_, clusters = table(labels, degrees)
        got_reps, got_sizes = report.cluster_table(labels, degrees)
        assert np.array_equal(got_reps, reps) and np.array_equal(got_sizes, sizes_)
        host = _native.host_lib()
        out = np.empty((2, n), np.int32)
        assert host.sat_cluster_reps(n, labels.ctypes.data, degrees.ctypes.data, out[0].ctypes.data, out[1].ctypes.data) == clusters
        # no degrees: the representative is the cluster's smallest node, the label itself
        assert host.sat_cluster_reps(n, labels.ctypes.data, None, out[0].ctypes.data, out[1].ctypes.data) == clusters
        assert np.array_equal(out[0], labels) and np.array_equal(out[1], sizes_)


@pytest.mark.parametrize("shape", ["path", "star", "singletons", "one component"])
def test_named_graphs(shape):
    n = 200
    rng = np.random.default_rng(3)
    if shape == "path":
        edges = [(i + 1, i) for i in rng.permutation(n - 1)]
    elif shape == "star":
        edges = [(n - 1, i) for i in range(n - 1)]
    elif shape == "singletons":
        edges = []
    else:
        edges = [(int(a), int(b)) for a, b in rng.integers(0, n, size=(6 * n, 2))] + [(i, i + 1) for i in range(n - 1)]
    # the edges dealt to three sets, so that no set alone holds the partition
    sets = [edges[g::3] for g in range(3)]
    labels = check_join(n, sets, rng)
    assert len(set(labels.tolist())) == (n if shape == "singletons" else 1)
    degrees = np.zeros(n, np.int32)
    for a, b in edges:
        degrees[a] += 1
        degrees[b] += 1
    reps, sizes = report.cluster_table(labels, degrees)
    want = table(labels, degrees)
    assert np.array_equal(reps, want[0]) and np.array_equal(sizes, want[1])
    if shape == "star":
        assert (reps == n - 1).all() and (sizes == n).all()
    if shape == "path":
        assert (reps == 1).all()                  # the ends have degree 1, every inner node 2: the first inner node
    if shape == "singletons":
        assert np.array_equal(reps, np.arange(n)) and (sizes == 1).all()


def test_degree_ties_go_to_the_smallest_index():
    labels = np.array([0, 0, 2, 0, 2, 5, 2], np.int32)
    degrees = np.array([1, 7, 4, 7, 4, 0, 4], np.int32)
    reps, sizes = report.cluster_table(labels, degrees)
    assert reps.tolist() == [1, 1, 2, 1, 2, 5, 2] and sizes.tolist() == [3, 3, 3, 3, 3, 1, 3]
    reps, _ = report.cluster_table(labels, np.zeros(7, np.int32))
    assert reps.tolist() == labels.tolist()


def test_bad_arguments_are_refused():
    host = _native.host_lib()
    out = np.empty(4, np.int32)
    for bad in ([0, 4, 2, 3], [0, -1, 2, 3]):
        lab = np.array(bad, np.int32)
        assert host.sat_cluster_join(4, 1, lab.ctypes.data, out.ctypes.data) == -1
    ok = np.arange(4, dtype=np.int32)
    assert host.sat_cluster_join(0, 1, ok.ctypes.data, out.ctypes.data) == -1
    assert host.sat_cluster_join(4, 0, ok.ctypes.data, out.ctypes.data) == -1
    assert host.sat_cluster_join(4, 1, None, out.ctypes.data) == -1
    # a labelling that is not canonical: a label above its node, a label that is not its own label
    for bad in ([1, 1, 2, 3], [0, 0, 1, 3]):
        with pytest.raises(ValueError):
            report.cluster_table(np.array(bad, np.int32), np.zeros(4, np.int32))


# ---------------------------------------------------------------- 2. command line
def run(golden_dir, args, stdin=b""):
    return subprocess.run([CLI] + args, input=stdin, cwd=golden_dir, capture_output=True)


@pytest.mark.parametrize("args,message", [
    (["-c", "-a", ec.EDGE_DB, "-L", "0.001"], b"ERROR: -L cannot be combined with -c\n"),
    (["-L", "0.001"], b"ERROR: -L needs -a dbfile\n"),
    (["-q", ec.EDGE_DB, "-L", "0.001"], b"ERROR: -L needs -a dbfile\n"),
    (["-Q", ec.EDGE_DB, "-L", "0.001"], b"ERROR: -L needs -a dbfile\n"),
    (["-a", ec.EDGE_DB, "-L", "0.001", "-k", "3"], b"ERROR: -L cannot be combined with -k\n"),
    (["-a", ec.EDGE_DB, "-L", "0.001", "-p", "0.5"], b"ERROR: -L cannot be combined with -p\n"),
    (["-a", ec.EDGE_DB, "-L", "0.001", "-m", "2"], b"ERROR: -L cannot be combined with -m\n"),
    (["-a", ec.EDGE_DB, "-L", "0.001", "-M", "2"], b"ERROR: -L cannot be combined with -M\n"),
    (["-a", ec.EDGE_DB, "-L", "0.001", "-R", "64"], b"ERROR: -L cannot be combined with -R\n"),
    (["-a", ec.EDGE_DB, "-L", "0.001", "-C", "5"], b"ERROR: -L cannot be combined with -C\n"),
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
    p = run(golden_dir, ["-a", ec.EDGE_DB, "-L", value])
    assert p.returncode == 1 and p.stdout == b""
    assert b"ERROR: -L needs a p-value in [0, 1] (got '" + value.encode() + b"')\n" in p.stderr
    assert b"Usage:" in p.stderr and b"MAXDIM" not in p.stderr


def test_usage_names_the_option(golden_dir):
    p = run(golden_dir, ["-x"])
    assert p.returncode == 1 and p.stdout == b""
    assert b"[-A] [-L P] [-b]" in p.stderr
    assert b"  -L P : with -a dbfile: cluster the database on the GPU" in p.stderr
    assert b"name representative cluster_size degree" in p.stderr
    p = run(golden_dir, ["-L"])                  # the option without its argument is a usage error too
    assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""


# ---------------------------------------------------------------- 3. header, build
def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "satabsearch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for decl in ("int sat_cluster_begin(sat_ctx *ctx, int n_nodes);",
                 "int sat_cluster_add(sat_ctx *ctx, double max_pvalue, const int32_t *query_node);",
                 "int sat_cluster_labels(sat_ctx *ctx, int32_t *label, int32_t *degree, unsigned long long *edges);",
                 "int sat_cluster_end(sat_ctx *ctx);",
                 "int sat_multi_search_only(sat_multi *m, int lorder, int lsoln, int maxstart, double *wall_ms);",
                 "int sat_multi_cluster_begin(sat_multi *m);",
                 "int sat_multi_cluster_add(sat_multi *m, double max_pvalue, const int32_t *query_node);",
                 "int sat_multi_cluster_labels(sat_multi *m, int32_t *label, int32_t *degree, unsigned long long *edges);"):
        assert decl in text, decl
    host = open(os.path.join(ROOT, "cuda_satabsearch_amd", "csrc", "host", "sat_cluster.h")).read()
    host = re.sub(r"/\*.*?\*/", "", host, flags=re.S)
    assert "int sat_cluster_join(int n, int nsets, const int32_t *labels, int32_t *out);" in host
    assert "int sat_cluster_reps(int n, const int32_t *label, const int32_t *degree, int32_t *rep, int32_t *size);" in host


def test_the_clustering_is_a_translation_unit_of_the_device_library(monkeypatch):
    """sat_cluster.hip is in build.DEVICE_SOURCES and build_device() compiles it for gfx950 to an object the library
    links, with the host helper's object beside it; libsathost.so holds the helper too (the commands are recorded, not
    run).  The predicate is shared, not copied: one definition, in the header both files include."""
    from cuda_satabsearch_amd import build
    assert "sat_cluster.hip" in build.DEVICE_SOURCES
    cmds = []
    monkeypatch.setattr(build, "_run", cmds.append)
    build.build_device(force=True)
    build.build_host(force=True)
    compiles = [c for c in cmds if "-c" in c and c[-1] == os.path.join(build.CSRC, "sat_cluster.hip")]
    assert len(compiles) == 1 and "--offload-arch=gfx950" in compiles[0]
    obj = compiles[0][compiles[0].index("-o") + 1]
    links = [c for c in cmds if "-shared" in c and c[c.index("-o") + 1] == build.DEVICE_LIB[0]]
    assert len(links) == 1 and "-Wl," + obj in links[0]
    assert "-Wl," + os.path.join(build.PKG, "sat_cluster.o") in links[0]
    host = [c for c in cmds if "-shared" in c and c[c.index("-o") + 1] == os.path.join(build.PKG, "libsathost.so")]
    assert len(host) == 1 and os.path.join(build.HOST, "sat_cluster.c") in host[0]
    assert "sat_cluster.hip" in open(os.path.join(ROOT, "Makefile")).read()
    for f in ("sat_topk.hip", "sat_cluster.hip"):
        text = open(os.path.join(build.CSRC, f)).read()
        assert '#include "sat_hitrow.hpp"' in text and "struct HitQuery {" not in text and "bool cutoff_row(" not in text, f
    shared = open(os.path.join(build.CSRC, "sat_hitrow.hpp")).read()
    assert shared.count("struct HitQuery {") == 1 and shared.count("bool cutoff_row(") == 1 and shared.count("sat_hit hit_row(") == 1
