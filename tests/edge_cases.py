"""Inputs that carry the reference to the places its 586-entry example database never reaches (test
infrastructure, shared by tests/golden/make_edge_golden.py and tests/test_reference_edges.py).

* both size classes in one database (orders 1..111, entries above 96 SSEs interleaved with small ones),
* `??` and half-unknown tableau codes (`P?`, `?E`, ...) in database and query,
* distances on a 0.5 A grid with query offsets of exactly 0, +-0.5 and +-4.0 A (MXSSED itself),
* distances >= 100 A, which the ASCII reader mis-columns (sat_parse.c, "7-column quirk"),
* entries of `xi` / `xg` helices only,
* query lists (-q) that mix the classes, repeat a SID and spell one in upper case.

Everything is built from cuda_satabsearch_amd.synth and deterministic in its seeds.  EDGE_* describe the
committed fixtures; fuzz_case() draws the inputs of the live differential test.
"""
import os

import numpy as np

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import synth

SMALL_MAX = 96                      # MAXDIM_GPU: the boundary of the reference's two passes
BOUNDARY_ORDERS = (1, 2, 3, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 98, 110, 111, 111)
ALL_CODES = np.array([(h << 4) | l for h in range(5) for l in range(5)], np.uint8)      # P R O L ? x E D S T ?
UNKNOWN = 0x44                                                                           # ??
HALF_UNKNOWN = {"P?": 0x04, "?E": 0x40, "R?": 0x14, "?T": 0x43}
OFFSETS = np.array([0.0, 0.5, -0.5, 4.0, -4.0], np.float32)

POOL_SEED = 0xED6E
POOL_SIZE = 64


class Pool:
    """POOL_SIZE synthetic 111-SSE structures; every entry of an edge input is the leading block of one."""

    def __init__(self, seed=POOL_SEED):
        db = synth.make_db(POOL_SIZE, orders=np.full(POOL_SIZE, sat.structures.MAXDIM, np.int32), seed=seed, sort=False)
        self.cells = [db.dense(s) for s in range(POOL_SIZE)]

    def leading(self, s, n):
        t, d = self.cells[s]
        return t[:n, :n].copy(), d[:n, :n].copy()


def put(a, i, j, v):
    a[i, j] = a[j, i] = v


def snap(d, grid):
    """Off-diagonal distances onto a grid (the diagonal holds the SSE types)."""
    diag = np.diagonal(d).copy()
    d[:] = np.round(d / grid) * grid
    np.fill_diagonal(d, diag)


def set_types(t, d, types):
    n = t.shape[0]
    idx = np.arange(n)
    t[idx, idx] = types
    d[idx, idx] = np.asarray(types, np.float32)


def sub_query(t, d, sel, rng):
    """The sub-structure `sel` of (t, d) with every distance moved by exactly 0, +-0.5 or +-4.0 A."""
    sel = np.asarray(sel)
    m = sel.size
    qt, qd = t[np.ix_(sel, sel)].copy(), d[np.ix_(sel, sel)].copy()
    off = np.tril(OFFSETS[rng.integers(0, OFFSETS.size, size=(m, m))], -1)
    types = np.diagonal(qt).copy()
    qd = np.abs(qd + off + off.T).astype(np.float32)
    set_types(qt, qd, types)
    return qt, qd


def struct_set(entries):
    """entries: list of (name, tab[n, n], dist[n, n])."""
    return sat.StructSet.from_dense([e[1].shape[0] for e in entries], [e[1] for e in entries],
                                    [e[2] for e in entries], [e[0] for e in entries])


def write(entries, path):
    synth.write_ascii(struct_set(entries), path)


# ---------------------------------------------------------------------------------------------- the committed fixtures
#            file order: small entries between the large ones, orders 1 and 2 again after the last large one
EDGE_ORDERS = (17, 1, 2, 97, 3, 111, 64, 33, 98, 16, 65, 110, 48, 32, 111, 49, 96, 100, 8, 24, 101, 1, 2, 12, 40, 9, 70, 5)
EDGE_UNKNOWN_ENTRY = 20        # 101 SSEs: ?? cells and half-unknown codes
EDGE_HELIX_ENTRY = 25          # 9 SSEs, xi / xg only
EDGE_FAR_ENTRIES = (17, 24)    # 100 and 40 SSEs: cells of 100.000, 123.456 and 99.999 A
EDGE_SUB3 = (0, 3, 8)          # the step traces' database: 17, 97 and 98 SSEs


def edge_name(k):
    return "e%02dn%03d" % (k, EDGE_ORDERS[k])          # 7 characters: -q cuts SIDs to 7


def edge_entries(pool):
    rng = np.random.default_rng([POOL_SEED, 1])
    out = []
    for k, n in enumerate(EDGE_ORDERS):
        t, d = pool.leading(k, n)
        if k % 2 == 0:
            snap(d, 0.5)
        if k == EDGE_UNKNOWN_ENTRY:
            for c in range(60):                         # ?? and half-unknown codes all over, rows above 64 included
                i = int(rng.integers(1, n))
                j = int(rng.integers(0, i))
                put(t, i, j, (UNKNOWN, *HALF_UNKNOWN.values())[c % 5])
            put(t, 100, 70, UNKNOWN)
            put(t, 99, 3, HALF_UNKNOWN["P?"])
        if k == EDGE_HELIX_ENTRY:
            set_types(t, d, np.array([2, 3, 3, 2, 2, 3, 2, 3, 3], np.uint8))
        if k == EDGE_FAR_ENTRIES[0]:                    # one, two and three long cells in a row; row 80 past column 64
            put(d, 80, 70, 100.0)
            put(d, 90, 10, 123.456); put(d, 90, 66, 100.0)
            put(d, 95, 2, 99.999); put(d, 95, 3, 100.0); put(d, 95, 40, 123.456); put(d, 95, 94, 100.0)
        if k == EDGE_FAR_ENTRIES[1]:
            put(d, 20, 4, 100.0); put(d, 21, 5, 123.456); put(d, 22, 6, 99.999)
            put(d, 30, 1, 123.456); put(d, 30, 2, 100.0); put(d, 30, 29, 100.0)
        out.append((edge_name(k), t, d))
    return out


def edge_queries(pool, entries):
    """name -> (tab, dist): planted queries are sub-structures of an entry, foreign ones are not."""
    rng = np.random.default_rng([POOL_SEED, 2])
    pick = lambda n, m: np.sort(rng.choice(n, size=m, replace=False))
    q = {}
    q["EQ001"] = pool.leading(40, 1)                                            # foreign
    q["EQ002"] = pool.leading(41, 2)                                            # foreign
    _, t, d = entries[6]
    q["EQ008"] = sub_query(t, d, pick(64, 8), rng)                              # planted in the 64-SSE entry
    _, t, d = entries[EDGE_UNKNOWN_ENTRY]
    unknown_rows = np.unique(np.nonzero(t >= 0x40)[0])[:12]
    sel = np.union1d(unknown_rows, pick(101, 33))[:33]
    q["EQ033"] = sub_query(t, d, np.sort(sel), rng)                             # planted, carries ? cells
    t, d = pool.leading(42, 64)
    snap(d, 1.0)
    q["EQ064"] = (t, d)                                                         # foreign, more SSEs than most entries
    _, t, d = entries[5]
    q["EQ097"] = sub_query(t, d, pick(111, 97), rng)                            # planted in the first 111-SSE entry
    _, t, d = entries[14]
    q["EQ111"] = sub_query(t, d, np.arange(111), rng)                           # the second 111-SSE entry, moved
    _, t, d = entries[EDGE_FAR_ENTRIES[1]]
    q["EQFAR"] = sub_query(t, d, np.arange(40), np.random.default_rng(0))       # keeps the >= 100 A cells
    for i, j, v in ((20, 4, 100.0), (21, 5, 123.456), (30, 1, 123.456), (30, 2, 100.0), (30, 29, 100.0)):
        put(q["EQFAR"][1], i, j, v)
    return q


def query_file(name):
    return "edge_%s.query" % name.lower()


# jobs: (name, bodies or None for -q, "LTYPE LORDER LSOLN", restarts); expected stdout in expected/<name>.out
EDGE_DB = "edge.ascii"
EDGE_SUB3_DB = "edge_sub3.ascii"
EDGE_SIDS = "edge_sids.txt"
EDGE_JOBS = []
for _q in ("EQ001", "EQ002", "EQ008", "EQ033", "EQ064", "EQ097", "EQ111", "EQFAR"):
    for _opt in ("T T T", "T F T"):
        EDGE_JOBS.append(("edge_%s_%s.r16" % (_q.lower(), _opt.replace(" ", "")), (_q,), _opt, 16))
EDGE_JOBS.append(("edge_eq033_TFT.r128", ("EQ033",), "T F T", 128))
EDGE_JOBS.append(("edge_multi_TFT.r16", ("EQ008", "EQ097", "EQ002"), "T F T", 16))
EDGE_JOBS.append(("edge_multi_TTF.r16", ("EQ008", "EQ097", "EQ002"), "T T F", 16))
EDGE_JOBS.append(("edge_qlist.r16", None, "T T F", 16))
# step traces over the 3-entry sub-database, one restart: (name, query, options, committed)
EDGE_TRACES = [("edge_sub3_eq008_TTT.r1.trace", "EQ008", "T T T", True), ("edge_sub3_eq008_TFT.r1.trace", "EQ008", "T F T", True),
               ("edge_sub3_eq097_TTT.r1.trace", "EQ097", "T T T", False), ("edge_sub3_eq097_TFT.r1.trace", "EQ097", "T F T", False)]


def edge_sids():
    """small, LARGE (upper case), small, large, large, small, and the first one again."""
    ks = (6, 3, 18, 5, 20, 21, 6)
    names = [edge_name(k) for k in ks]
    names[1] = names[1].upper()
    return ks, "".join(n + "\n" for n in names)


def job_command(job, golden_dir):
    """(argv tail, stdin bytes) of an edge job: `-r R` with header + query bodies on stdin, or `-r R -q db` with SIDs."""
    _, bodies, options, restarts = job
    if bodies is None:
        with open(os.path.join(golden_dir, EDGE_SIDS), "rb") as f:
            return ["-r", str(restarts), "-q", EDGE_DB], f.read()
    return ["-r", str(restarts)], stdin_of(golden_dir, EDGE_DB, options, bodies)


def stdin_of(golden_dir, db, options, bodies):
    data = (db + "\n" + options + "\n").encode()
    for b in bodies:
        with open(os.path.join(golden_dir, query_file(b)), "rb") as f:
            data += f.read()
    return data


# ---------------------------------------------------------------------------------------------- live differential fuzz
def mutate(t, d, rng):
    n = t.shape[0]
    grid = (None, 0.5, 1.0)[int(rng.integers(0, 3))]
    if grid:
        snap(d, grid)
    if n > 1 and rng.random() < 0.5:
        for _ in range(int(rng.integers(1, 2 * n))):
            i = int(rng.integers(1, n))
            put(t, i, int(rng.integers(0, i)), ALL_CODES[int(rng.integers(0, 25))])
    if n > 1 and rng.random() < 0.5:
        for _ in range(int(rng.integers(1, n + 1))):
            i = int(rng.integers(1, n))
            put(d, i, int(rng.integers(0, i)), (0.0, 4.0, 100.0, 123.456, 999.999)[int(rng.integers(0, 5))])
    if rng.random() < 0.3:
        set_types(t, d, rng.integers(0, 4, size=n).astype(np.uint8))


def draw_order(rng):
    if rng.random() < 0.5:
        return int(BOUNDARY_ORDERS[int(rng.integers(0, len(BOUNDARY_ORDERS)))])
    return int(rng.integers(1, sat.structures.MAXDIM + 1))


def fuzz_case(seed, pool, directory):
    """Writes db.ascii and stdin into `directory`; returns the argv tail shared by the three binaries."""
    rng = np.random.default_rng([POOL_SEED, 3, seed])
    entries = []
    for k in range(int(rng.integers(1, 7))):
        t, d = pool.leading(int(rng.integers(0, POOL_SIZE)), draw_order(rng))
        mutate(t, d, rng)
        entries.append(("f%04de%d" % (seed % 10000, k), t, d))
    write(entries, os.path.join(directory, "db.ascii"))
    restarts = (1, 2, 7, 16, 33)[int(rng.integers(0, 5))]
    if seed % 4 == 3:                                   # -q over its own database
        sids = []
        for _ in range(int(rng.integers(1, 6))):
            name = entries[int(rng.integers(0, len(entries)))][0]
            sids.append(name.upper() if rng.random() < 0.3 else name)
        with open(os.path.join(directory, "stdin"), "w") as f:
            f.write("".join(s + "\n" for s in sids))
        return ["-r", str(restarts), "-q", "db.ascii"]
    queries = []
    for k in range(int(rng.integers(1, 3))):
        if rng.random() < 0.6:                          # planted
            _, t, d = entries[int(rng.integers(0, len(entries)))]
            n = t.shape[0]
            m = int(rng.integers(1, n + 1))
            qt, qd = sub_query(t, d, np.sort(rng.choice(n, size=m, replace=False)), rng)
        else:                                           # foreign
            qt, qd = pool.leading(int(rng.integers(0, POOL_SIZE)), draw_order(rng))
            mutate(qt, qd, rng)
        queries.append(("Q%04dq%d" % (seed % 10000, k), qt, qd))
    write(queries, os.path.join(directory, "body"))
    options = " ".join("TF"[int(rng.integers(0, 2))] for _ in range(3))
    with open(os.path.join(directory, "stdin"), "w") as f, open(os.path.join(directory, "body")) as b:
        f.write("db.ascii\n" + options + "\n" + b.read())
    return ["-r", str(restarts)]
