"""Shared by the tests of the exact search (tests/test_exact_cpu.py, tests/test_gpu_exact.py): the brute-force reference
tests/native/exact_oracle.c (every feasible map of a pair, no pruning, the pinned oracle's full score) built with the
oracle's flags; the host twin sat_exact_host of libsathost.so on a StructSet's packed entries; seeded databases and
queries with the cells that need care - `?` codes, distances of 100 A and more, non-finite distances, entries without
an SSE of a needed type.  Test infrastructure only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "exact_oracle.c")
MAXDIM = 111
FULL_BUDGET = 1 << 32

_lib = None


def lib():
    """Compiles exact_oracle.c once per process into a private temp dir (-O3 -ffp-contract=off: oracle/Makefile)."""
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="exact_oracle_"), "libexact_oracle.so")
        subprocess.run([os.environ.get("CC") or "gcc", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                        os.path.join(ROOT, "oracle"), "-o", out, SRC, "-lm"], check=True)
        l = C.CDLL(out)
        l.exact_oracle_optimum.restype = C.c_longlong
        l.exact_oracle_optimum.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.exact_oracle_full_score.restype = C.c_int
        l.exact_oracle_full_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib = l
    return _lib


def units(n2):
    """the parallel units of a row (sat_exact_units): the image of query SSE 0"""
    return int(n2) + 1


class Pair:
    """One (query, entry e of db) pair in the layouts the oracle (dense) and the host twin (packed) read."""

    def __init__(self, db, e, q):
        self.qt, self.qd, self.qtypes = (np.ascontiguousarray(q[0], np.uint8), np.ascontiguousarray(q[1], np.float32),
                                         np.ascontiguousarray(q[2], np.uint8))
        self.n1, self.n2 = int(self.qt.shape[0]), int(db.orders[e])
        self.query = oracle_lib._Query(self.n1, self.qt.shape[1], self.qt.ctypes.data, self.qd.ctypes.data, self.qtypes.ctypes.data)
        t, d = db.dense(int(e))
        self.tab2, self.dmat2 = np.ascontiguousarray(t, np.uint8), np.ascontiguousarray(d, np.float32)
        self.types2 = db.ssetypes(int(e))
        o, cells = int(db.cell_off[e]), self.n2 * (self.n2 + 1) // 2
        self.tri_tab = np.ascontiguousarray(db.tab[o:o + cells])
        self.tri_dist = np.ascontiguousarray(db.dist[o:o + cells])

    def optimum(self, lorder):
        """(optimum, a map int32[n1] that has it, feasible maps) by brute force"""
        score, best = C.c_int(0), np.full(self.n1, -1, np.int32)
        maps = lib().exact_oracle_optimum(C.byref(self.query), self.n2, self.tab2.ctypes.data, self.dmat2.ctypes.data,
                                          self.tab2.shape[1], int(bool(lorder)), C.byref(score), best.ctypes.data)
        return int(score.value), best, int(maps)

    def full_score(self, m):
        m = np.ascontiguousarray(np.asarray(m)[:self.n1], np.int32)
        return int(lib().exact_oracle_full_score(C.byref(self.query), self.tab2.ctypes.data, self.dmat2.ctypes.data,
                                                 self.tab2.shape[1], m.ctypes.data))

    def feasible(self, m, lorder):
        m = [int(x) for x in np.asarray(m)[:self.n1]]
        on = [(i, j) for i, j in enumerate(m) if j >= 0]
        if any(j >= self.n2 or self.types2[j] != self.qtypes[i] for i, j in on):
            return False
        img = [j for _, j in on]
        return len(set(img)) == len(img) and (not lorder or img == sorted(img))

    def host(self, lorder, max_nodes, base_score, base_map):
        """sat_exact_host: (score, map int32[n1], unproven, nodes)"""
        import cuda_satabsearch_amd._native as native
        base_map = np.ascontiguousarray(np.asarray(base_map)[:self.n1], np.int32)
        score, flag, nodes = C.c_int32(0), C.c_uint8(0), C.c_uint32(0)
        out = np.full(self.n1, -1, np.int32)
        rc = native.host_lib().sat_exact_host(self.n1, self.qt.ctypes.data, self.qd.ctypes.data, self.qt.shape[1],
                                              self.qtypes.ctypes.data, self.n2, self.tri_tab.ctypes.data, self.tri_dist.ctypes.data,
                                              int(bool(lorder)), int(max_nodes), int(base_score), base_map.ctypes.data,
                                              C.byref(score), out.ctypes.data, C.byref(flag), C.byref(nodes))
        assert rc == 0
        return int(score.value), out, bool(flag.value), int(nodes.value)


def _spoil(t, d, rng, n):
    """a few cells of a dense symmetric structure made awkward, in place: `?` codes, far and non-finite distances"""
    if n < 2:
        return
    for _ in range(int(rng.integers(0, 4))):
        i, j = (int(x) for x in rng.choice(n, size=2, replace=False))
        kind = int(rng.integers(0, 5))
        if kind == 0:
            t[i, j] = t[j, i] = (int(t[i, j]) & 0x0F) | 0x40                 # `?` for the first letter
        elif kind == 1:
            t[i, j] = t[j, i] = (int(t[i, j]) & 0xF0) | 0x04                 # and for the second
        elif kind == 2:
            d[i, j] = d[j, i] = np.float32(100.0 + 60.0 * rng.random())
        elif kind == 3:
            d[i, j] = d[j, i] = np.float32(np.nan)
        else:
            d[i, j] = d[j, i] = np.float32(np.inf)


def make_db(orders, seed, spoil=True, uniform_types_from=64):
    """A database of the given orders (unsorted, as given).  Entries of `uniform_types_from` SSEs and more get SSE types
    spread over 0..3 (the two types queries mostly have a fifth each), so that every query SSE has about a fifth of them
    as candidates and brute force stays cheap."""
    import cuda_satabsearch_amd as sat
    orders = np.asarray(orders, np.int32)
    base = sat.synth.make_db(len(orders), orders=orders, seed=seed, sort=False)
    rng = np.random.Generator(np.random.Philox(key=seed ^ 0xE8AC7))
    tabs, dists = [], []
    for s, n in enumerate(orders):
        n = int(n)
        t, d = base.dense(s)
        if n >= uniform_types_from:
            types = rng.choice(4, size=n, p=(0.2, 0.2, 0.3, 0.3)).astype(np.uint8)
            t[np.arange(n), np.arange(n)] = types
            d[np.arange(n), np.arange(n)] = types.astype(np.float32)
        if spoil and s % 3 == 0:
            _spoil(t, d, rng, n)
        if spoil and s % 17 == 5:                               # one SSE type only: most queries find nothing to match
            t[np.arange(n), np.arange(n)] = 2
            d[np.arange(n), np.arange(n)] = 2.0
        tabs.append(t)
        dists.append(d)
    return sat.StructSet.from_dense(orders, tabs, dists)


def make_queries(db, orders, seed, spoil=True):
    """Queries of the given orders: every second one planted in an entry that is long enough (so that good maps exist),
    the others random; some with awkward cells."""
    import cuda_satabsearch_amd as sat
    rng = np.random.Generator(np.random.Philox(key=seed ^ 0x9E77))
    out = []
    for k, n1 in enumerate(orders):
        n1 = int(n1)
        hosts = np.nonzero(db.orders >= max(n1, 2))[0]
        if k % 2 == 0 and n1 >= 2 and len(hosts):
            s = int(hosts[int(rng.integers(0, len(hosts)))])
            t, d, types = sat.synth.planted_query(db, s, keep=n1 / float(db.orders[s]), seed=seed + k)
            if len(types) != n1:                                # (the rounding of keep: cut or fall back)
                t, d, types = (t[:n1, :n1].copy(), d[:n1, :n1].copy(), types[:n1].copy()) if len(types) > n1 else sat.synth.make_query(n1, seed=seed + k)
        else:
            t, d, types = sat.synth.make_query(n1, seed=seed + k)
        t, d = t.copy(), d.copy()
        if spoil and k % 3 == 1:
            _spoil(t, d, rng, n1)
        out.append((t, d, np.ascontiguousarray(types, np.uint8)))
    return out


def sa_rows(db, queries, lorder, maxstart, first_ordinal=0, seed=1234):
    """The plain search's rows by the CPU oracle, which reproduces the GPU's SA bit for bit: (scores [nq, N], maps [nq, N, 111])"""
    scores = np.zeros((len(queries), len(db)), np.int32)
    maps = np.full((len(queries), len(db), MAXDIM), -1, np.int32)
    for q, (t, d, types) in enumerate(queries):
        sc, mp, _ = oracle_lib.search(db, t, d, types, lorder=lorder, lsoln=True, maxstart=maxstart, seed=seed,
                                      query_ordinal=first_ordinal + q)
        scores[q], maps[q] = sc, mp
    return scores, maps


def host_rows(db, queries, lorder, max_nodes, base_scores, base_maps):
    """The host twin over every row: (scores, maps [nq, N, 111], unproven, nodes)"""
    nq, n = len(queries), len(db)
    scores, nodes = np.zeros((nq, n), np.int32), np.zeros((nq, n), np.uint32)
    maps, flags = np.full((nq, n, MAXDIM), -1, np.int32), np.zeros((nq, n), bool)
    for q in range(nq):
        n1 = len(queries[q][2])
        for e in range(n):
            s, m, f, nd = Pair(db, e, queries[q]).host(lorder, max_nodes, base_scores[q, e], base_maps[q, e])
            scores[q, e], flags[q, e], nodes[q, e] = s, f, nd
            maps[q, e, :n1] = m
    return scores, maps, flags, nodes


# ---- the database and the queries of tests/test_gpu_exact.py
GPU_QUERY_ORDERS = (1, 2, 3, 4, 5, 6, 7, 3, 5, 6)
GPU_FIRST = 3                                                       # ordinal of the first query
BUDGET_NODES = 64


def gpu_db():
    """200 entries of 1..14 SSEs in no order, then one of 111 SSEs (its types uniform over 0..3)"""
    return make_db([1 + (k * 11) % 14 for k in range(200)] + [111], 811)


def gpu_queries(db):
    return make_queries(db, GPU_QUERY_ORDERS, 823)


def budget_rows():
    """the rows of search_exact(lorder, maxstart 1, 64 nodes a row) of a fresh context, under the environment the process
    was started with: {name: array}"""
    import cuda_satabsearch_amd as sat
    db = gpu_db()
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(gpu_queries(db), GPU_FIRST)
        scores, maps, _ = s.search_exact(True, 1, BUDGET_NODES)
        base, flags, nodes = s.exact_results()
        return {"scores": scores, "maps": maps, "base": base, "flags": flags, "nodes": nodes,
                "info": np.frombuffer(s.last_launch_info().encode(), np.uint8)}


if __name__ == "__main__":
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    np.savez(sys.argv[1], **budget_rows())
