"""CPU reference of the several-matches mode (sat_search_matches): tests/native/chain_oracle.c (the pinned oracle's
helpers, one restart chain at a time, Philox streams) built with the oracle's flags, and select_matches(), the greedy
rule of include/satabsearch.h.  Test infrastructure only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "chain_oracle.c")
MAXDIM = 111
MAX_MATCHES = 8

_lib = None


def lib():
    """Compiles chain_oracle.c once per process into a private temp dir (-O3 -ffp-contract=off: oracle/Makefile)."""
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="chain_oracle_"), "libchain_oracle.so")
        subprocess.run([os.environ.get("CC") or "gcc", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                        os.path.join(ROOT, "oracle"), "-o", out, SRC, "-lm"], check=True)
        l = C.CDLL(out)
        l.chain_oracle_restart.restype = C.c_int
        l.chain_oracle_restart.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_int,
                                           C.c_uint64, C.c_uint32, C.c_int, C.c_void_p]
        l.chain_oracle_entry.restype = None
        l.chain_oracle_entry.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_int,
                                         C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def restarts(db, s, q, lorder, maxstart, query_ordinal=0, seed=1234, db_ordinal=None):
    """Own best of every restart of (query q, entry s): scores int32[maxstart], maps int32[maxstart, 111]."""
    qt, qd, qtypes = (np.ascontiguousarray(q[0], np.uint8), np.ascontiguousarray(q[1], np.float32),
                      np.ascontiguousarray(q[2], np.uint8))
    query = oracle_lib._Query(qt.shape[0], qt.shape[1], qt.ctypes.data, qd.ctypes.data, qtypes.ctypes.data)
    t, d = db.dense(int(s))
    t, d = np.ascontiguousarray(t, np.uint8), np.ascontiguousarray(d, np.float32)
    scores = np.empty(maxstart, np.int32)
    maps = np.empty((maxstart, MAXDIM), np.int32)
    ordinal = int(s if db_ordinal is None else db_ordinal)
    lib().chain_oracle_entry(C.byref(query), int(db.orders[s]), t.ctypes.data, d.ctypes.data, t.shape[1], ordinal,
                             int(bool(lorder)), seed, query_ordinal, int(maxstart), scores.ctypes.data, maps.ctypes.data)
    return scores, maps


def select_matches(scores, maps, max_matches):
    """The greedy rule: restarts by descending (score, -restart); the first is taken, each later one iff its score is
    positive and its db set misses the union of those taken, up to max_matches.  Returns (count, scores[M],
    restarts[M], maps[M, 111]) with the unused slots at 0, -1 and all -1."""
    order = sorted(range(len(scores)), key=lambda r: (-int(scores[r]), r))
    out_s = np.zeros(max_matches, np.int32)
    out_r = np.full(max_matches, -1, np.int32)
    out_m = np.full((max_matches, maps.shape[1]), -1, np.int32)
    used = set()
    count = 0
    for r in order:
        if count == max_matches:
            break
        dset = set(int(j) for j in maps[r] if j >= 0)
        if count > 0 and (scores[r] <= 0 or dset & used):
            continue
        out_s[count], out_r[count], out_m[count] = scores[r], r, maps[r]
        used |= dset
        count += 1
    return count, out_s, out_r, out_m


def matches(db, s, q, lorder, maxstart, max_matches, query_ordinal=0, seed=1234):
    sc, mp = restarts(db, s, q, lorder, maxstart, query_ordinal, seed)
    return select_matches(sc, mp, max_matches)
