"""CPU reference of the polish (sat_search_pairs_polish): tests/native/polish_oracle.c (the pinned oracle's move_delta,
one map at a time) built with the oracle's flags, and polish_pair(), the per-pair rule of include/satabsearch.h: rank the
restarts by (s_r, -r), polish the own-best maps of the first min(T, maxstart), the largest polished score wins, ties to
the lowest rank.  naive_moves() restates the neighbourhood with full scores only.  Test infrastructure only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import matches_lib
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "polish_oracle.c")
MAXDIM = 111

_lib = None


def lib():
    """Compiles polish_oracle.c once per process into a private temp dir (-O3 -ffp-contract=off: oracle/Makefile)."""
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="polish_oracle_"), "libpolish_oracle.so")
        subprocess.run([os.environ.get("CC") or "gcc", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                        os.path.join(ROOT, "oracle"), "-o", out, SRC, "-lm"], check=True)
        l = C.CDLL(out)
        l.polish_oracle_map.restype = C.c_int
        l.polish_oracle_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                        C.c_void_p]
        l.polish_oracle_full_score.restype = C.c_int
        l.polish_oracle_full_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib = l
    return _lib


class Pair:
    """One (query, dense entry) pair held in the layout the C side reads."""

    def __init__(self, q, tab2, dmat2, n2):
        self.qt, self.qd, self.qtypes = (np.ascontiguousarray(q[0], np.uint8), np.ascontiguousarray(q[1], np.float32),
                                         np.ascontiguousarray(q[2], np.uint8))
        self.n1 = int(self.qt.shape[0])
        self.query = oracle_lib._Query(self.n1, self.qt.shape[1], self.qt.ctypes.data, self.qd.ctypes.data,
                                       self.qtypes.ctypes.data)
        self.tab2, self.dmat2 = np.ascontiguousarray(tab2, np.uint8), np.ascontiguousarray(dmat2, np.float32)
        self.n2 = int(n2)
        self.types2 = np.diagonal(self.tab2)[:self.n2].copy()

    @classmethod
    def of(cls, db, s, q):
        t, d = db.dense(int(s))
        return cls(q, t, d, db.orders[s])

    def full_score(self, m):
        m = np.ascontiguousarray(m, np.int32)
        return int(lib().polish_oracle_full_score(C.byref(self.query), self.tab2.ctypes.data, self.dmat2.ctypes.data,
                                                  self.tab2.shape[1], m.ctypes.data))

    def polish(self, m, score, lorder):
        """Polish a copy of map m (int32[>= n1]) whose full score is `score`: (polished score, moves, map int32[111])."""
        out = np.full(MAXDIM, -1, np.int32)
        out[:self.n1] = np.asarray(m, np.int32)[:self.n1]
        moves = C.c_int(0)
        p = lib().polish_oracle_map(C.byref(self.query), self.n2, self.tab2.ctypes.data, self.dmat2.ctypes.data,
                                    self.tab2.shape[1], int(bool(lorder)), out.ctypes.data, int(score), C.byref(moves))
        return int(p), int(moves.value), out

    def naive_moves(self, m, lorder):
        """Every allowed move (i, j) of map m with its delta, from FULL scores of the moved map: [(delta, i, j)]."""
        m = np.asarray(m, np.int32)[:self.n1].copy()
        base = self.full_score(m)
        used = set(int(j) for j in m if j >= 0)
        out = []
        for i in range(self.n1):
            below = [int(m[k]) for k in range(i) if m[k] >= 0]
            above = [int(m[k]) for k in range(i + 1, self.n1) if m[k] >= 0]
            lo, hi = (max(below, default=-1), min(above, default=self.n2)) if lorder else (-1, self.n2)
            cands = [-1] if m[i] >= 0 else []
            cands += [j for j in range(lo + 1, hi) if j not in used and self.types2[j] == self.qtypes[i]]
            for j in cands:
                moved = m.copy()
                moved[i] = j
                out.append((self.full_score(moved) - base, i, j))
        return out


def rank(scores):
    """the restarts by descending key (s_r, -r), as sat_search_matches ranks them"""
    return sorted(range(len(scores)), key=lambda r: (-int(scores[r]), r))


def polish_ranked(pair, scores, maps, lorder, tops):
    """The per-pair rule on the restarts' own bests: (score, base_score, restart, moves, map int32[111])."""
    order = rank(scores)[:min(int(tops), len(scores))]
    best = None
    for r in order:                                           # ties keep the lowest rank
        p, mv, m = pair.polish(maps[r], int(scores[r]), lorder)
        if best is None or p > best[0]:
            best = (p, int(scores[order[0]]), int(r), mv, m)
    return best


def polish_pair(db, s, q, lorder, maxstart, tops, query_ordinal=0, seed=1234, db_ordinal=None):
    sc, mp = matches_lib.restarts(db, s, q, lorder, maxstart, query_ordinal, seed, db_ordinal)
    return polish_ranked(Pair.of(db, s, q), sc, mp, lorder, tops)
