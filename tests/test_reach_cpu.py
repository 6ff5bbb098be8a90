"""Transitive search (sat_reach_*) without a GPU: the key's packing, the shard join and the rows of csrc/host/sat_reach.h
through libsathost against reach_lib's numpy restatement, the order of the packed keys, the bad arguments, the same code
under the sanitizers as a stand-alone program over the same cases, and report.reach_table / reach_path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cuda_satabsearch_amd import _native, report

import reach_lib as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_satabsearch_amd", "csrc", "host")
N = 10000
NSETS = 3
LARGEST_NODE = (1 << 27) - 2


def pack_cases():
    """(depth, parent, p) of N keys: the named edge cases first, random ones behind them"""
    rng = np.random.default_rng(5)
    depth = rng.integers(0, 63, N).astype(np.int32)
    parent = rng.integers(-1, LARGEST_NODE + 1, N).astype(np.int32)
    p = np.exp(rng.uniform(np.log(1e-300), 0.0, N))
    tenth = 0.1
    named = [
        (0, -1, 0.0),                                   # a seed
        (1, 0, 0.0),                                    # p = 0
        (1, 0, -0.0), (1, 0, -1e-3),                    # p <= 0 packs as 0
        (1, 5, 1e-40),                                  # a subnormal float
        (1, 5, float(np.float32(1.4e-45))),             # the smallest one
        (1, 5, 1e-50),                                  # rounds to the float 0
        (1, 5, 5e-324),                                 # a subnormal double
        (62, 7, 1.0),                                   # p = 1 at the largest depth
        (3, 9, tenth), (3, 9, np.nextafter(tenth, 1.0)), (3, 9, np.nextafter(tenth, 0.0)),       # one float from three doubles
        (2, LARGEST_NODE, 0.5),                         # the largest legal node
        (2, -1, 0.5),                                   # an external parent
        (2, 0, 1.0 + 2.0 ** -24), (2, 0, 1.0 + 2.0 ** -23),      # a tie to even, and the float above 1
    ]
    for i, (d, par, pv) in enumerate(named):
        depth[i], parent[i], p[i] = d, par, pv
    return depth, parent, p


def join_cases():
    """NSETS accumulators over N nodes (keys with parents below N, a third of the nodes unreached in each set) and their
    supports; returns (keys [NSETS, N], support [NSETS, N], joined keys, joined support)"""
    rng = np.random.default_rng(6)
    keys = rl.pack(rng.integers(0, 63, (NSETS, N)), np.exp(rng.uniform(-40.0, 0.0, (NSETS, N))), rng.integers(-1, N, (NSETS, N)))
    keys[rng.random((NSETS, N)) < 1 / 3] = rl.UNREACHED
    keys[:, 17] = rl.UNREACHED                          # unreached everywhere
    keys[1, 18] = keys[0, 18]                           # the same key twice
    keys[:, 19] = rl.pack([4, 2, 2], [0.5, 0.5, 0.25], [3, -1, -1])     # an external parent wins at the smaller p
    support = rng.integers(0, 1000, (NSETS, N)).astype(np.int32)
    return keys, support, keys.min(axis=0), support.sum(axis=0).astype(np.int32)


def lib_pack(lib, depth, parent, p):
    return np.array([lib.sat_reach_pack_key(int(d), float(x), int(par)) for d, par, x in zip(depth, parent, p)], np.uint64)


# ---------------------------------------------------------------- 1. pack, unpack
def test_pack_and_unpack_against_numpy():
    lib = _native.host_lib()
    depth, parent, p = pack_cases()
    want = rl.pack(depth, p, parent)
    got = lib_pack(lib, depth, parent, p)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    # the named cases say what they are meant to
    assert want[0] == 0x7FFFFFF and (want[1:4] == (np.uint64(1) << np.uint64(58))).all()
    assert rl.pbits(1e-40) > 0 and rl.pbits(1e-40) < rl.pbits(float(np.finfo(np.float32).tiny))
    assert rl.pbits(float(np.float32(1.4e-45))) == 1 and rl.pbits(1e-50) == 0 and rl.pbits(5e-324) == 0
    assert rl.pbits(1.0) == 0x3F800000 and want[9] == want[10] == want[11]
    assert int(want[12]) & 0x7FFFFFF == LARGEST_NODE and int(want[13]) & 0x7FFFFFF == 0x7FFFFFF
    assert rl.pbits(1.0 + 2.0 ** -24) == 0x3F800000 and rl.pbits(1.0 + 2.0 ** -23) == 0x3F800001
    assert (want < rl.UNREACHED).all()
    d, par, pv = C.c_int32(), C.c_int32(), C.c_float()
    wd, wpar, wpv = rl.unpack(want)
    for i in range(0, N, 7):
        lib.sat_reach_unpack_key(int(want[i]), C.byref(d), C.byref(par), C.byref(pv))
        assert (d.value, par.value) == (wd[i], wpar[i]) and np.float32(pv.value).view(np.uint32) == wpv[i].view(np.uint32)
        assert wd[i] == depth[i] and wpar[i] == max(parent[i], -1)
        assert wpv[i] == (np.float32(p[i]) if p[i] > 0 else np.float32(0))
    lib.sat_reach_unpack_key(0xFFFFFFFFFFFFFFFF, C.byref(d), C.byref(par), C.byref(pv))
    assert (d.value, par.value) == (63, -1)


def test_key_order_is_depth_then_float_p_then_parent():
    depth, parent, p = pack_cases()
    # many ties on every level of the order
    depth[100:4000] = depth[100:4000] % 3
    p[100:2000] = np.float32(0.25)
    parent[100:1000] = parent[100:1000] % 5 - 1
    keys = lib_pack(_native.host_lib(), depth, parent, p)
    pf = np.where(p > 0, p.astype(np.float32), np.float32(0)).astype(np.float64)
    par = np.where(parent < 0, 1 << 27, parent)                         # an external parent sorts last
    triples = list(zip(depth.tolist(), pf.tolist(), par.tolist()))
    order = np.argsort(keys, kind="stable")
    by_triple = sorted(range(N), key=lambda i: (triples[i], i))
    assert [triples[i] for i in order] == [triples[i] for i in by_triple]
    for i, j in zip(order[:-1], order[1:]):                              # equal keys are equal triples, and the reverse
        assert (keys[i] == keys[j]) == (triples[i] == triples[j])


# ---------------------------------------------------------------- 2. join, decode
def test_join_and_decode_against_numpy():
    lib = _native.host_lib()
    keys, support, want_keys, want_support = join_cases()
    out_keys, out_support = np.zeros(N, np.uint64), np.zeros(N, np.int32)
    assert lib.sat_reach_join(N, NSETS, keys.ctypes.data, support.ctypes.data, out_keys.ctypes.data, out_support.ctypes.data) == 0
    assert np.array_equal(out_keys, want_keys) and np.array_equal(out_support, want_support)
    assert out_keys[17] == rl.UNREACHED and out_keys[18] == min(keys[:, 18])
    # one set: a copy
    assert lib.sat_reach_join(N, 1, keys.ctypes.data, support.ctypes.data, out_keys.ctypes.data, out_support.ctypes.data) == 0
    assert np.array_equal(out_keys, keys[0]) and np.array_equal(out_support, support[0])
    want = rl.decode(want_keys, want_support)
    assert 0 < len(want) < N and (np.diff(want["node"]) > 0).all() and (want["parent"] == -1).any()
    rows = np.zeros(N, rl.ROW_DTYPE)
    assert lib.sat_reach_decode(N, want_keys.ctypes.data, want_support.ctypes.data, N, rows.ctypes.data) == len(want)
    rl.same_rows(rows[:len(want)], want, "decode")
    rows = np.zeros(N, rl.ROW_DTYPE)
    assert lib.sat_reach_decode(N, want_keys.ctypes.data, want_support.ctypes.data, 10, rows.ctypes.data) == len(want)
    rl.same_rows(rows[:10], want[:10], "capped decode")
    assert not rows[10:].view(np.uint8).any()
    assert lib.sat_reach_decode(N, want_keys.ctypes.data, want_support.ctypes.data, 0, None) == len(want)


def test_bad_arguments():
    lib = _native.host_lib()
    keys, support = np.full(4, rl.UNREACHED, np.uint64), np.zeros(4, np.int32)
    ok, os_ = np.zeros(4, np.uint64), np.zeros(4, np.int32)
    rows = np.zeros(4, rl.ROW_DTYPE)
    k, s, o, o2, r = keys.ctypes.data, support.ctypes.data, ok.ctypes.data, os_.ctypes.data, rows.ctypes.data
    assert lib.sat_reach_join(4, 1, k, s, o, o2) == 0
    for args in ((0, 1, k, s, o, o2), (4, 0, k, s, o, o2), (4, 1, None, s, o, o2), (4, 1, k, None, o, o2), (4, 1, k, s, None, o2),
                 (4, 1, k, s, o, None)):
        assert lib.sat_reach_join(*args) == -1, args
    assert lib.sat_reach_decode(4, k, s, 4, r) == 0
    for args in ((0, k, s, 0, None), (1 << 27, k, s, 0, None), (4, None, s, 0, None), (4, k, None, 0, None), (4, k, s, -1, r),
                 (4, k, s, 1, None)):
        assert lib.sat_reach_decode(*args) == -1, args
    keys[2] = rl.pack(1, 0.5, 4)                                        # a parent past the last node
    assert lib.sat_reach_decode(4, k, s, 4, r) == -1
    keys[2] = rl.pack(1, 0.5, 3)
    assert lib.sat_reach_decode(4, k, s, 4, r) == 1 and (rows[0]["node"], rows[0]["parent"]) == (2, 3)


# ---------------------------------------------------------------- 3. the host code under the sanitizers
def test_host_code_under_the_sanitizers(tmp_path):
    """sat_reach.c and tests/native/reach_check.c - a stand-alone program with its own main - built with
    -fsanitize=address,undefined and run as a child over the cases of the tests above, written to a file with numpy's
    expectations; no report may appear.  Nothing is loaded into Python, nothing is preloaded."""
    exe, cases = str(tmp_path / "reach_check"), str(tmp_path / "cases.bin")
    build = subprocess.run(["gcc", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-Wall", "-Wextra", "-I", HOST, "-o", exe, os.path.join(ROOT, "tests", "native", "reach_check.c"),
                            os.path.join(HOST, "sat_reach.c")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    depth, parent, p = pack_cases()
    keys, support, want_keys, want_support = join_cases()
    rows = rl.decode(want_keys, want_support)
    with open(cases, "wb") as f:
        for a in (np.array([N, NSETS], np.int32), depth, parent, p.astype(np.float64), rl.pack(depth, p, parent), keys, support, want_keys,
                  want_support, np.array([len(rows)], np.int32), rows):
            f.write(np.ascontiguousarray(a).tobytes())
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == "reach_check: ok\n"
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr and run.stderr == ""


# ---------------------------------------------------------------- 4. report
ROWS = np.array([(0, 0, -1, 0, 0.0), (2, 1, 0, 3, 1e-9), (3, 2, 2, 1, 2.5e-4), (5, 1, -1, 1, 0.5), (7, 3, 3, 2, 1e-3)], rl.ROW_DTYPE)
NAMES = ["seed", "x1", "near", "far", "x4", "outside", "x6", "last"]


def test_reach_table():
    assert report.reach_table(ROWS, NAMES) == [
        "# name depth parent pvalue support",
        "seed 0 - 0 0",
        "near 1 seed 1e-09 3",
        "far 2 near 0.00025 1",
        "outside 1 - 0.5 1",
        "last 3 far 0.001 2",
    ]
    assert report.reach_table(ROWS[:0], NAMES) == ["# name depth parent pvalue support"]


def test_reach_path():
    assert report.reach_path(ROWS, 7) == [7, 3, 2, 0]
    assert report.reach_path(ROWS, 0) == [0]
    assert report.reach_path(ROWS, 5) == [5]                            # reached from an external query: the chain ends there
    with pytest.raises(KeyError):
        report.reach_path(ROWS, 1)
    broken = ROWS.copy()
    broken["depth"][2] = 3                                               # node 3 no longer one level below node 7's ... above it
    with pytest.raises(ValueError, match="node 7 at depth 3 has its parent 3 at depth 3"):
        report.reach_path(broken, 7)
