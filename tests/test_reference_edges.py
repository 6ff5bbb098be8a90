"""oracle == reference and `satabsearch -c` == reference beyond the reference's example database, and the same
inputs through the GPU kernel.

The 586-entry example database behind test_oracle_golden.py has one entry above 64 SSEs, none above 96, no
half-unknown code and no distance >= 100 A: the reference's second ("large") pass, the upper set word of
sat_host_search.c, LORDER = F at step level and the mixed-class -q list never ran against the reference there.
tests/edge_cases.py builds inputs that do; this file pins both restatements to the reference on them:

* recorded (always): the stdout of oracle/_ref/ref_oracle on the edge jobs, committed under tests/golden/expected
  by tests/golden/make_edge_golden.py, byte for byte; two step traces of ref_oracle_debug;
* guard (always): the committed fixtures still hold the properties they were made for;
* live (where oracle/_ref is built, i.e. where the reference tree is present): the committed files are fresh,
  FUZZ_CASES seeded random cases give identical stdout from ref_oracle, oracle_cli -c and satabsearch -c, and four
  step traces (LORDER T / F x 8 / 97 SSEs) are equal;
* gpu: satabsearch == oracle_cli -p -G on every edge job, and Searcher.search == oracle_lib.search on one batch of
  every fixture query, which closes reference == oracle (drand48), oracle (Philox) == kernel on identical data.
"""
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import edge_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
ORACLE_CLI = os.path.join(ROOT, "oracle", "oracle_cli")
REF = os.path.join(ROOT, "oracle", "_ref", "ref_oracle")
REF_DEBUG = os.path.join(ROOT, "oracle", "_ref", "ref_oracle_debug")
EXPECTED = os.path.join(ROOT, "tests", "golden", "expected")

live = pytest.mark.skipif(not (os.path.exists(REF) and os.path.exists(REF_DEBUG)), reason="oracle/_ref not built")
JOB_IDS = [j[0] for j in ec.EDGE_JOBS]
QUERIES = ("EQ001", "EQ002", "EQ008", "EQ033", "EQ064", "EQ097", "EQ111", "EQFAR")


def run(binary, cwd, args, stdin):
    p = subprocess.run([binary, *args], input=stdin, cwd=cwd, capture_output=True)
    assert p.returncode == 0, "%s %s: exit %d: %s" % (os.path.basename(binary), args, p.returncode, p.stderr.decode()[-400:])
    return p.stdout


def expected(name):
    with open(os.path.join(EXPECTED, name), "rb") as f:
        return f.read()


def trace_stdin(golden_dir, query, options):
    return ec.stdin_of(golden_dir, ec.EDGE_SUB3_DB, options, (query,))


# ---------------------------------------------------------------------------------------------- recorded
@pytest.mark.parametrize("job", ec.EDGE_JOBS, ids=JOB_IDS)
def test_oracle_cli_prints_the_recorded_reference_output(golden_dir, job):
    args, stdin = ec.job_command(job, golden_dir)
    assert run(ORACLE_CLI, golden_dir, ["-c", *args], stdin) == expected(job[0] + ".out")


@pytest.mark.parametrize("job", ec.EDGE_JOBS, ids=JOB_IDS)
def test_host_mode_prints_the_recorded_reference_output(golden_dir, job):
    args, stdin = ec.job_command(job, golden_dir)
    assert run(CLI, golden_dir, ["-c", *args], stdin) == expected(job[0] + ".out")


@pytest.mark.parametrize("trace", [t for t in ec.EDGE_TRACES if t[3]], ids=lambda t: t[0])
def test_oracle_step_trace_equals_the_recorded_reference_trace(golden_dir, trace):
    """Every SA step (restart, iteration, ssei, startj, endj, newj) and map over a small entry and two above 96 SSEs,
    for LORDER = T and F: the small class, then the large class on the same drand48 stream."""
    name, query, options, _ = trace
    out = run(ORACLE_CLI, golden_dir, ["-c", "-r", "1", "-t"], trace_stdin(golden_dir, query, options))
    gold = expected(name + ".stdout")
    assert out == gold and gold.count(b"# QUERY ID") == 2


# ---------------------------------------------------------------------------------------------- fixture guard
def text_records(path):
    """[(name, order, tableau rows, distance rows)] of an ASCII file, by its text alone."""
    with open(path) as f:
        lines = f.read().split("\n")
    out, k = [], 0
    while k < len(lines):
        if not lines[k].strip():
            k += 1
            continue
        name, order = lines[k].split()
        n = int(order)
        out.append((name, n, lines[k + 1:k + 1 + n], lines[k + 1 + n:k + 1 + 2 * n]))
        k += 1 + 2 * n
    return out


def offdiag_codes(rec):
    return [row[3 * j:3 * j + 2] for i, row in enumerate(rec[2]) for j in range(i)]


def test_fixtures_still_hold_what_they_were_made_for(golden_dir):
    """Trimming a fixture must not drop coverage silently: asserted on the unpacked files' text."""
    recs = text_records(os.path.join(golden_dir, ec.EDGE_DB))
    orders = [r[1] for r in recs]
    names = [r[0] for r in recs]
    assert len(set(names)) == len(names) and all(len(n) <= 7 for n in names)
    assert set(ec.BOUNDARY_ORDERS) <= set(orders) and orders.count(111) >= 2
    large = [k for k, n in enumerate(orders) if n > ec.SMALL_MAX]
    assert len(large) >= 6
    between = [k for k in range(large[0], large[-1]) if orders[k] <= ec.SMALL_MAX]
    assert len(between) >= 5 and orders != sorted(orders)                      # small entries between the large ones
    assert 1 in orders[:large[-1]] and 2 in orders[:large[-1]]
    assert 1 in orders[large[-1] + 1:] and 2 in orders[large[-1] + 1:]          # orders 1 and 2 again after the last large
    # ?? and every half-unknown code in an entry above 96 SSEs, some in a row above 64
    unknown = [k for k in large if {"??", *ec.HALF_UNKNOWN} <= set(offdiag_codes(recs[k]))]
    assert unknown
    assert any("?" in row for k in unknown for row in recs[k][2][65:])
    # an entry of xi / xg helices only
    assert any(r[1] >= 4 and {row[3 * i:3 * i + 2] for i, row in enumerate(r[2])} == {"xi", "xg"} for r in recs)
    # 0.5 A grid on every second entry
    for r in recs[::2]:
        cells = np.array([float(v) for row in r[3] for v in row.split()])
        assert np.all(cells * 2 == np.round(cells * 2)) or r[0] == names[ec.EDGE_FAR_ENTRIES[1]]
    # 100.000, 123.456 and 99.999 in two entries, once in a row past column 64 (which needs an entry above 64 SSEs)
    far = [k for k, r in enumerate(recs) if all(any(v in row.split()[:-1] for row in r[3]) for v in ("100.000", "123.456", "99.999"))]
    assert len(far) >= 2
    assert any(v in row.split()[65:-1] for k in far for row in recs[k][3] for v in ("100.000", "123.456"))
    assert any(sum(v in ("100.000", "123.456") for v in row.split()) >= 2 for k in far for row in recs[k][3])   # the shift adds up

    # queries: the orders, ? cells, n1 above most entries, >= 100 A cells
    q = {name: text_records(os.path.join(golden_dir, ec.query_file(name)))[0] for name in QUERIES}
    assert sorted(r[1] for r in q.values()) == [1, 2, 8, 33, 40, 64, 97, 111]
    assert {"??"} < {c for c in offdiag_codes(q["EQ033"]) if "?" in c}          # ?? and at least one half-unknown code
    assert sum(n < 64 for n in orders) > len(orders) / 2                        # EQ064, EQ097, EQ111: n1 > n2 for most entries
    assert sum(v in ("100.000", "123.456") for row in q["EQFAR"][3] for v in row.split()[:-1]) >= 4
    multi = [j for j in ec.EDGE_JOBS if j[1] == ("EQ008", "EQ097", "EQ002")]
    assert sorted(j[2] for j in multi) == ["T F T", "T T F"]
    assert sorted({j[3] for j in ec.EDGE_JOBS}) == [16, 128]

    # the SID list: small, LARGE (upper case), small, large, large, small, the first again
    with open(os.path.join(golden_dir, ec.EDGE_SIDS)) as f:
        sids = f.read().split()
    order_of = {n.lower(): o for n, o in zip(names, orders)}
    assert ["L" if order_of[s.lower()] > ec.SMALL_MAX else "s" for s in sids] == list("sLsLLss")
    assert sids[6] == sids[0] and sids[1].isupper() and sids[1] not in names and sids[0] in names

    # the traces' database: one small entry, two above 96
    sub = text_records(os.path.join(golden_dir, ec.EDGE_SUB3_DB))
    assert sorted(r[1] > ec.SMALL_MAX for r in sub) == [False, True, True]


def test_fixture_sizes():
    """No edge file above the largest fixture there was before them, 700 KB in all."""
    sizes = [os.path.getsize(os.path.join(ROOT, "tests", "golden", sub, f)) for sub in ("inputs", "expected")
             for f in os.listdir(os.path.join(ROOT, "tests", "golden", sub)) if f.startswith("edge")]
    limit = os.path.getsize(os.path.join(ROOT, "tests", "golden", "inputs", "tableauxdistmatrixdb.small.ascii.gz"))
    assert max(sizes) <= limit and sum(sizes) < 700 * 1024


# ---------------------------------------------------------------------------------------------- live, against oracle/_ref
@live
def test_committed_expected_files_are_fresh(golden_dir):
    for job in ec.EDGE_JOBS:
        args, stdin = ec.job_command(job, golden_dir)
        assert run(REF, golden_dir, ["-c", *args], stdin) == expected(job[0] + ".out"), job[0]


@live
@pytest.mark.parametrize("trace", ec.EDGE_TRACES, ids=lambda t: t[0])
def test_oracle_step_trace_equals_the_reference_debug_build(golden_dir, trace):
    name, query, options, committed = trace
    stdin = trace_stdin(golden_dir, query, options)
    gold = run(REF_DEBUG, golden_dir, ["-c", "-r", "1"], stdin)
    assert run(ORACLE_CLI, golden_dir, ["-c", "-r", "1", "-t"], stdin) == gold
    assert gold.count(b"\n") > 300 and (not committed or gold == expected(name + ".stdout"))


FUZZ_BLOCK = 50
FUZZ_BLOCKS = 6
FUZZ_CASES = FUZZ_BLOCK * FUZZ_BLOCKS


@pytest.fixture(scope="module")
def pool():
    return ec.Pool()


def first_difference(a, b):
    la, lb = a.split(b"\n"), b.split(b"\n")
    for k in range(max(len(la), len(lb))):
        x, y = (la[k] if k < len(la) else None), (lb[k] if k < len(lb) else None)
        if x != y:
            return "line %d: %r != %r" % (k + 1, x, y)
    return "equal"


@live
@pytest.mark.parametrize("block", range(FUZZ_BLOCKS))
def test_live_differential_fuzz(pool, tmp_path, block):
    """Seeded random databases of 1-6 entries (orders half from the class / word boundaries, half uniform on 1..111;
    0.5 and 1.0 A grids; any of the 25 code combinations; cells of 0, 4, 100, 123.456 and 999.999 A; random helix
    types), one or two planted or foreign queries or a -q list, random options and restart counts: the reference,
    the oracle and `satabsearch -c` exit 0 with the same stdout.  A failing case keeps its files and names its seed."""
    t0 = time.time()
    failures = []
    for seed in range(block * FUZZ_BLOCK, (block + 1) * FUZZ_BLOCK):
        case = tmp_path / ("seed%04d" % seed)
        case.mkdir()
        args = ec.fuzz_case(seed, pool, str(case))
        with open(case / "stdin", "rb") as f:
            stdin = f.read()
        ref = run(REF, str(case), ["-c", *args], stdin)
        bad = []
        for binary in (ORACLE_CLI, CLI):
            out = run(binary, str(case), ["-c", *args], stdin)
            if out != ref:
                bad.append("%s: %s" % (os.path.basename(binary), first_difference(out, ref)))
        if bad:
            failures.append("seed %d (%s, files in %s): %s" % (seed, " ".join(args), case, "; ".join(bad)))
        else:
            shutil.rmtree(case)
    print("\nfuzz block %d: %d cases x 3 binaries in %.1f s" % (block, FUZZ_BLOCK, time.time() - t0))
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------- gpu
@pytest.mark.gpu
@pytest.mark.parametrize("job", ec.EDGE_JOBS, ids=JOB_IDS)
def test_gpu_mode_equals_the_oracle_on_the_edge_jobs(golden_dir, job):
    args, stdin = ec.job_command(job, golden_dir)
    gpu = run(CLI, golden_dir, args, stdin)
    assert gpu == run(ORACLE_CLI, golden_dir, ["-c", "-p", "-G", *args], stdin)
    assert len(re.findall(rb"^# QUERY ID", gpu, re.M)) == 2 * (7 if job[1] is None else len(job[1]))   # both classes


@pytest.fixture(scope="module")
def edge_batch(golden_dir):
    db = sat.StructSet.read(os.path.join(golden_dir, ec.EDGE_DB))
    queries = []
    for name in QUERIES:
        qs = sat.StructSet.read(os.path.join(golden_dir, ec.query_file(name)), "query")
        queries.append((*qs.dense(0), qs.ssetypes(0)))
    return db, queries


@pytest.mark.gpu
@pytest.mark.parametrize("lorder", [True, False], ids=["LORDER_T", "LORDER_F"])
def test_searcher_equals_the_oracle_on_the_edge_batch(edge_batch, lorder):
    """Every fixture query in one batch (1 to 111 SSEs, so the batch mixes query size classes) over the edge database
    (every order bucket in one upload), ordinals from 0, maxstart 100: scores and maps bit for bit."""
    import oracle_lib
    db, queries = edge_batch
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries, 0)
        scores, maps, _ = s.search(lorder, True, 100)
    for k, (qt, qd, qtypes) in enumerate(queries):
        oscores, omaps, _ = oracle_lib.search(db, qt, qd, qtypes, lorder, True, 100, query_ordinal=k)
        assert np.array_equal(scores[k], oscores), "query %s: entries %s differ" % (QUERIES[k], np.nonzero(scores[k] != oscores)[0])
        assert np.array_equal(maps[k], omaps), "maps of query %s differ" % QUERIES[k]
