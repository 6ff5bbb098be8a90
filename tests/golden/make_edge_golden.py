#!/usr/bin/env python3
"""tests/golden/make_edge_golden.py - regenerate the edge fixtures (tests/edge_cases.py describes them).

Like make_golden.sh this runs only where oracle/_ref holds the reference's own host path (oracle/Makefile,
`make ref`): it writes the synthetic edge database, its 3-entry sub-database, the query bodies and the SID list
under inputs/ (large files gzipped; the golden_dir fixture unpacks them), runs oracle/_ref/ref_oracle on every
job of edge_cases.EDGE_JOBS and ref_oracle_debug on the committed step traces, and stores their stdout under
expected/.  Deterministic: a second run rewrites every file byte for byte."""
import gzip
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import edge_cases as ec  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "ref_oracle")
REF_DEBUG = os.path.join(ROOT, "oracle", "_ref", "ref_oracle_debug")
GZIP_OVER = 4096


def store(work, name):
    """inputs/<name>, gzipped (no timestamp) when large."""
    src = os.path.join(work, name)
    dst = os.path.join(HERE, "inputs", name)
    for stale in (dst, dst + ".gz"):
        if os.path.exists(stale):
            os.remove(stale)
    if os.path.getsize(src) <= GZIP_OVER:
        shutil.copy(src, dst)
        return
    with open(src, "rb") as fi, open(dst + ".gz", "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=raw, mtime=0) as fo:
            shutil.copyfileobj(fi, fo)


def reference(binary, work, args, stdin, out_name):
    p = subprocess.run([binary, "-c", *args], input=stdin, cwd=work, capture_output=True)
    if p.returncode != 0:
        sys.exit("%s %s failed: %s" % (binary, args, p.stderr.decode()[-300:]))
    with open(os.path.join(HERE, "expected", out_name), "wb") as f:
        f.write(p.stdout)


def main():
    for b in (REF, REF_DEBUG):
        if not os.path.exists(b):
            sys.exit("%s is missing: run `make -C oracle ref` where the reference tree is present" % b)
    pool = ec.Pool()
    entries = ec.edge_entries(pool)
    queries = ec.edge_queries(pool, entries)
    with tempfile.TemporaryDirectory() as work:
        ec.write(entries, os.path.join(work, ec.EDGE_DB))
        ec.write([entries[k] for k in ec.EDGE_SUB3], os.path.join(work, ec.EDGE_SUB3_DB))
        for name, (t, d) in queries.items():
            ec.write([(name, t, d)], os.path.join(work, ec.query_file(name)))
        with open(os.path.join(work, ec.EDGE_SIDS), "w") as f:
            f.write(ec.edge_sids()[1])
        for name in [ec.EDGE_DB, ec.EDGE_SUB3_DB, ec.EDGE_SIDS] + [ec.query_file(q) for q in queries]:
            store(work, name)
        for job in ec.EDGE_JOBS:
            args, stdin = ec.job_command(job, work)
            reference(REF, work, args, stdin, job[0] + ".out")
        for name, query, options, committed in ec.EDGE_TRACES:
            if committed:
                reference(REF_DEBUG, work, ["-r", "1"], ec.stdin_of(work, ec.EDGE_SUB3_DB, options, (query,)), name + ".stdout")
    total = 0
    for sub in ("inputs", "expected"):
        for f in sorted(os.listdir(os.path.join(HERE, sub))):
            if f.startswith("edge"):
                size = os.path.getsize(os.path.join(HERE, sub, f))
                total += size
                print("%8d  %s/%s" % (size, sub, f))
    print("%8d  total" % total)


if __name__ == "__main__":
    main()
