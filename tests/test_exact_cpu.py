"""The exact search without a GPU: the host twin sat_exact_host (csrc/host/sat_exact.c, which compiles the walk, the
bound and the unit split the device compiles) against the brute-force reference of tests/exact_lib.py; its budget; the
sanitizer build; the ABI."""
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import _native, report

import exact_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_satabsearch_amd", "csrc", "host")


def _cases():
    """300 (pair, lorder, base score, base map): 200 ordered pairs (queries of 1..7 SSEs, entries of 1..14), 100
    unordered (1..5, 1..10).  Two thirds start from the plain search's row at one restart (the CPU oracle's), the others
    from the empty map."""
    out = []
    for lorder, nq, ne, n1max, n2max, seed in ((True, 10, 20, 7, 14, 501), (False, 10, 10, 5, 10, 502)):
        db = exact_lib.make_db([1 + (k * 5) % n2max for k in range(ne)], seed)
        queries = exact_lib.make_queries(db, [1 + k % n1max for k in range(nq)], seed + 7)
        sc, mp = exact_lib.sa_rows(db, queries, lorder, 1)
        for q in range(nq):
            for e in range(ne):
                pair = exact_lib.Pair(db, e, queries[q])
                if (q + e) % 3 == 0:
                    out.append((pair, lorder, 0, np.full(pair.n1, -1, np.int32)))
                else:
                    out.append((pair, lorder, int(sc[q, e]), mp[q, e, :pair.n1].copy()))
    return out


@pytest.fixture(scope="module")
def cases():
    got = _cases()
    assert len(got) == 300
    return got


@pytest.fixture(scope="module")
def optima(cases):
    return [pair.optimum(lorder) for pair, lorder, _, _ in cases]


def test_cases_cover_the_awkward_cells(cases, optima):
    pairs = [c[0] for c in cases]
    assert any((p.qt & 0x44).any() or (p.tab2 & 0x44 & ~np.eye(p.n2, dtype=np.uint8) * 255).any() for p in pairs)
    assert any((p.dmat2 >= 100).any() or (p.qd >= 100).any() for p in pairs)
    assert any(not np.isfinite(p.dmat2).all() or not np.isfinite(p.qd).all() for p in pairs)
    # an entry without any SSE of a type the query needs, and the optimum it leaves: 0 with the empty map
    none = [k for k, p in enumerate(pairs) if not set(p.qtypes.tolist()) & set(p.types2.tolist())]
    assert none and all(optima[k][0] == 0 and (optima[k][1] == -1).all() for k in none)
    assert max(p.n1 for p in pairs) == 7 and max(p.n2 for p in pairs) == 14 and min(p.n1 for p in pairs) == 1 and min(p.n2 for p in pairs) == 1


def test_host_twin_equals_brute_force(cases, optima):
    """with a budget above every walk (a unit's nodes are at most n1 x the pair's maps) no pair may be unproven"""
    improved = 0
    for (pair, lorder, base, bmap), (opt, _, maps) in zip(cases, optima):
        assert maps * pair.n1 < exact_lib.FULL_BUDGET // exact_lib.units(pair.n2)
        assert pair.feasible(bmap, lorder) and pair.full_score(bmap) == base
        score, m, unproven, nodes = pair.host(lorder, exact_lib.FULL_BUDGET, base, bmap)
        assert not unproven
        assert score == opt, (pair.n1, pair.n2, lorder, base, score, opt)
        assert pair.feasible(m, lorder) and pair.full_score(m) == score
        assert nodes <= maps * pair.n1 + exact_lib.units(pair.n2)
        if score == base:
            assert (m == bmap).all()                        # the incumbent's row, untouched
        else:
            assert score > base
            improved += 1
    assert improved >= 30


def test_bound_does_not_decide_the_result(cases, optima):
    """the optimum from the worst incumbent any feasible map beats: every improving map is then visited or pruned by
    the bound alone, and the first of the best ones in unit order is the same map from any start below it"""
    for (pair, lorder, base, bmap), (opt, _, _) in list(zip(cases, optima))[::7]:
        empty = np.full(pair.n1, -1, np.int32)
        low, mlow, _, _ = pair.host(lorder, exact_lib.FULL_BUDGET, -1000, empty)
        assert low == opt and pair.full_score(mlow) == opt
        if opt > base:
            score, m, _, _ = pair.host(lorder, exact_lib.FULL_BUDGET, base, bmap)
            assert score == opt and pair.full_score(m) == opt


def test_one_node_a_unit(cases, optima):
    """max_nodes = the number of units: every unit expands at most its root, the result is still a feasible map whose
    full score is the reported one, between the base score and the optimum"""
    flagged = 0
    for (pair, lorder, base, bmap), (opt, _, _) in zip(cases, optima):
        score, m, unproven, nodes = pair.host(lorder, exact_lib.units(pair.n2), base, bmap)
        assert nodes <= exact_lib.units(pair.n2)
        assert pair.feasible(m, lorder) and pair.full_score(m) == score
        assert base <= score <= opt
        again = pair.host(lorder, exact_lib.units(pair.n2), base, bmap)
        assert (score, unproven, nodes) == (again[0], again[2], again[3]) and (m == again[1]).all()
        flagged += unproven
    assert 0 < flagged < len(cases)


def test_budget_split(cases):
    """a budget below the units leaves the highest units nothing; the node count never exceeds the budget"""
    pair, lorder, base, bmap = next(c for c in cases if c[0].n2 >= 10 and c[0].n1 >= 4)
    for budget in (1, 2, 5, exact_lib.units(pair.n2) - 1, 64, 1000):
        score, m, unproven, nodes = pair.host(lorder, budget, base, bmap)
        assert nodes <= budget and score >= base and pair.full_score(m) == score


def test_host_twin_under_sanitizers(tmp_path):
    """sat_exact.c and a stand-alone driver under AddressSanitizer + UndefinedBehaviorSanitizer: no report, and the
    checksum of the plain build"""
    srcs = [os.path.join(HOST, "sat_exact.c"), os.path.join(ROOT, "tests", "native", "exact_driver.c")]
    outs = []
    for name, flags in (("plain", ["-O2"]), ("asan", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / ("exact_driver_" + name))
        subprocess.run(["gcc", "-ffp-contract=off", "-Wall", "-Wextra", "-I", HOST, "-o", exe] + flags + srcs + ["-lm"], check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe], capture_output=True, env=env)
        err = p.stderr.decode(errors="replace")
        assert "ERROR: AddressSanitizer" not in err and "runtime error:" not in err and "LeakSanitizer" not in err, err[-3000:]
        assert p.returncode == 0, (p.stdout, err[-400:])
        outs.append(p.stdout)
    assert outs[0] == outs[1] and b"bad 0" in outs[0]


def test_abi_has_the_exact_calls():
    header = open(os.path.join(ROOT, "include", "satabsearch.h")).read()
    names = ("sat_search_exact", "sat_exact_results", "sat_exact_stats", "sat_multi_search_exact", "sat_multi_exact_results",
             "sat_multi_exact_stats")
    import ctypes
    lib = ctypes.CDLL(_native.DEVICE_LIB)
    for name in names:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _native.ABI_SYMBOLS and hasattr(lib, name)
    assert re.search(r"#define SAT_ABI_VERSION\s+1\b", header)
    assert re.search(r"#define SAT_EXACT_MAX_QUERY\s+16\b", header) and _native.EXACT_MAX_QUERY == 16
    assert ctypes.sizeof(_native.ExactStat) == 40
    for cls in (sat.Searcher, sat.MultiSearcher):
        assert all(hasattr(cls, m) for m in ("search_exact", "exact_results", "exact_stats"))


def test_exact_table():
    stats = np.zeros(2, [("rows", np.int64), ("proven", np.int64), ("improved", np.int64), ("gain", np.int64), ("nodes", np.uint64)])
    stats[0] = (10, 9, 2, 5, 1234)
    lines = report.exact_table(stats, names=["d1ubia_", "motif"])
    assert lines[0].startswith("#") and lines[1] == "d1ubia_ 10 9 2 2.500 123.4" and lines[2] == "motif 0 0 0 0.000 0.0"
