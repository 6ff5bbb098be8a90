"""Helpers of the profile tests (-W P, sat_profile_rows): the conserved core restated in Python from the rule of
csrc/host/sat_profile.h - not from its C - and the matrices of a set of maps in numpy."""
import numpy as np


def core(joint, hits, fraction):
    """(in_core bool[n1], joint_min), or None where the fraction is refused.  The rule, step by step:
    S = the SSEs whose diagonal count reaches fraction * hits; while a pair of S lies below it, take such a pair with the
    smallest joint count (then the smallest i, then the smallest k) and drop its member with the smaller diagonal count,
    the larger index on a tie."""
    if not (fraction > 0.0 and fraction <= 1.0):
        return None
    j = np.asarray(joint, dtype=np.int64)
    n1 = len(j)
    t = float(fraction) * float(hits)
    members = set(i for i in range(n1) if hits > 0 and float(j[i, i]) >= t)
    while True:
        below = [(int(j[i, k]), i, k) for i in sorted(members) for k in sorted(members) if i < k and float(j[i, k]) < t]
        if not below:
            break
        _, i, k = min(below)
        members.discard(i if j[i, i] < j[k, k] else k)
    flags = np.array([i in members for i in range(n1)], bool)
    m = sorted(members)
    if len(m) == 0:
        least = 0
    elif len(m) == 1:
        least = int(j[m[0], m[0]])
    else:
        least = min(int(j[i, k]) for i in m for k in m if i < k)
    return flags, least


def matrices(matched):
    """(hits, joint uint32[n1, n1]) of a 0/1 array [rows, n1]: joint[i][k] = the rows that match both"""
    a = np.asarray(matched).astype(np.int64)
    assert a.ndim == 2
    return len(a), (a.T @ a).astype(np.uint32)


def random_matched(rng, n1, rows):
    """a random 0/1 array [rows, n1] whose columns have differing densities and some correlated blocks, so that cores of
    every size, ties and dropped pairs all occur"""
    density = rng.choice([0.05, 0.3, 0.5, 0.5, 0.8, 1.0], size=n1)
    a = rng.random((rows, n1)) < density
    if n1 >= 3 and rows:
        # two groups of columns that exclude each other: each is matched often, together they never are
        half = rng.random(rows) < 0.5
        g = rng.permutation(n1)[:max(2, n1 // 3)]
        a[:, g[: len(g) // 2]] &= half[:, None]
        a[:, g[len(g) // 2:]] &= ~half[:, None]
    return a.astype(np.uint8)


def expected(maps_rows, entries, n1, own=None):
    """(hits, joint) of the rows of one query: maps_rows int32[rows, >= n1], two-dimensional (a map per row, < 0 = unmatched), entries
    the rows' entry ordinals; the rows whose entry is `own` are dropped"""
    maps_rows = np.asarray(maps_rows)[:, :n1]
    keep = np.ones(len(entries), bool) if own is None or own < 0 else np.asarray(entries) != own
    return matrices(maps_rows[keep] >= 0)
