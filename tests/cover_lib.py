"""The greedy cover by its specification, in Python: sets of neighbours and the loop written naively.
The reference of the cover tests - never the code under test, and it shares nothing with it."""
import numpy as np


def neighbours(n, a, b):
    """adj[v] = the set of v's neighbours under the pairs (a[i], b[i]): a self pair is no edge, a pair seen twice or in
    both directions is one"""
    adj = [set() for _ in range(n)]
    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        if x != y:
            adj[x].add(y)
            adj[y].add(x)
    return adj


def cover(n, a, b):
    """(rep, size, degree, edges, rounds) of the pairs (a[i], b[i]) over n nodes:
        unassigned = all nodes
        repeat: gain(v) = 1 + |adj(v) & unassigned| for every unassigned v; v* = the largest gain, ties to the smallest
                index; gain(v*) == 1: stop; else v* and its unassigned neighbours get rep = v* and leave"""
    adj = neighbours(n, a, b)
    rep = np.arange(n, dtype=np.int32)
    unassigned = set(range(n))
    rounds = 0
    while unassigned:
        best, best_gain = -1, 0
        for v in sorted(unassigned):
            gain = 1 + len(adj[v] & unassigned)
            if gain > best_gain:                    # strictly: among equal gains the smallest index stays
                best, best_gain = v, gain
        if best_gain == 1:
            break
        members = (adj[best] & unassigned) | {best}
        rep[list(members)] = best
        unassigned -= members
        rounds += 1
    degree = np.array([len(s) for s in adj], np.int32)
    size = np.bincount(rep, minlength=n).astype(np.int32)[rep]
    assert int(degree.sum()) % 2 == 0
    return rep, size, degree, int(degree.sum()) // 2, rounds


def check_invariants(n, a, b, rep):
    """every member is adjacent to its representative (dominating), no two representatives are adjacent (independent)"""
    adj = neighbours(n, a, b)
    rep = np.asarray(rep)
    assert rep.shape == (n,) and (rep >= 0).all() and (rep < n).all()
    assert np.array_equal(rep[rep], rep), "a representative is not its own"
    for v in range(n):
        if rep[v] != v:
            assert int(rep[v]) in adj[v], "node %d is no neighbour of its representative %d" % (v, rep[v])
    reps = set(np.nonzero(rep == np.arange(n))[0].tolist())
    for r in reps:
        assert not (adj[r] & reps), "representatives %d and %s are adjacent" % (r, sorted(adj[r] & reps)[:4])


def components(n, a, b):
    """the number of connected components: what single linkage makes of the same edges"""
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        x, y = find(x), find(y)
        if x != y:
            parent[max(x, y)] = min(x, y)
    return len({find(v) for v in range(n)})


def same(got, want, what=""):
    """got = (rep, degree, edges, rounds) of the code under test against cover()'s tuple; the sizes through `sizes`"""
    rep, degree, edges, rounds = got
    assert np.array_equal(rep, want[0]), "%s: rep differs at %s" % (what, np.nonzero(np.asarray(rep) != want[0])[0][:8])
    assert np.array_equal(degree, want[2]), "%s: degree differs at %s" % (what, np.nonzero(np.asarray(degree) != want[2])[0][:8])
    assert edges == want[3], "%s: %d edges, expected %d" % (what, edges, want[3])
    assert rounds == want[4], "%s: %d rounds, expected %d" % (what, rounds, want[4])
