"""The transitive search restated for its tests (test_reach_cpu.py, test_gpu_reach.py): the key's packing in numpy, an
accumulator that takes rows by the definition, and the rows it decodes to.  Nothing here calls the code under test."""
import numpy as np

UNREACHED = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_PARENT = 0x7FFFFFF
ROW_DTYPE = np.dtype([("node", np.int32), ("depth", np.int32), ("parent", np.int32), ("support", np.int32),
                      ("pvalue", np.float32)])


def pbits(p):
    """the 31 bits p packs as: the IEEE bits of float32(p), round to nearest; p <= 0 gives 0"""
    p = np.asarray(p, np.float64)
    with np.errstate(under="ignore", over="ignore"):
        bits = p.astype(np.float32).view(np.uint32).astype(np.uint64) & np.uint64(0x7FFFFFFF)
    return np.where(p > 0, bits, np.uint64(0))


def pack(depth, p, parent):
    """depth in bits 63..58, pbits in 57..27, parent in 26..0 (a negative parent: 0x7FFFFFF)"""
    parent = np.asarray(parent, np.int64)
    par = np.where(parent < 0, NO_PARENT, parent).astype(np.uint64)
    return (np.asarray(depth, np.int64).astype(np.uint64) << np.uint64(58)) | (pbits(p) << np.uint64(27)) | par


def unpack(keys):
    """(depth int32, parent int32 with -1 for none, pvalue float32) of uint64 keys"""
    keys = np.asarray(keys, np.uint64)
    depth = (keys >> np.uint64(58)).astype(np.int32)
    par = (keys & np.uint64(0x7FFFFFF)).astype(np.int64)
    pv = ((keys >> np.uint64(27)) & np.uint64(0x7FFFFFFF)).astype(np.uint32).view(np.float32)
    return depth, np.where(par == NO_PARENT, -1, par).astype(np.int32), pv


def decode(keys, support):
    """the reached nodes as rows, ascending"""
    depth, parent, pv = unpack(keys)
    at = np.nonzero(depth != 63)[0]
    rows = np.zeros(len(at), ROW_DTYPE)
    rows["node"], rows["depth"], rows["parent"], rows["support"], rows["pvalue"] = at, depth[at], parent[at], np.asarray(support)[at], pv[at]
    return rows


class Accumulator:
    """keys and supports over n nodes by the definition: a seed is (0, 0, none); a step a -> b at depth d and p-value p
    lowers key[b] to pack(d, p, a) and adds 1 to support[b]; a step with a == b is none"""

    def __init__(self, n, seeds=()):
        self.keys = np.full(n, UNREACHED, np.uint64)
        self.support = np.zeros(n, np.int32)
        self.keys[np.asarray(seeds, np.int64)] = pack(0, 0.0, -1)

    def add(self, depth, a, b, p):
        a, b, p = np.asarray(a, np.int64).ravel(), np.asarray(b, np.int64).ravel(), np.asarray(p, np.float64).ravel()
        keep = a != b
        a, b, p = a[keep], b[keep], p[keep]
        np.minimum.at(self.keys, b, pack(np.full(len(a), depth), p, a))
        np.add.at(self.support, b, 1)

    def frontier(self, depth):
        return np.nonzero(unpack(self.keys)[0] == depth)[0].astype(np.int32)

    def rows(self):
        return decode(self.keys, self.support)


def same_rows(got, want, what=""):
    assert got.dtype == want.dtype, what
    assert len(got) == len(want), "%s: %d rows, expected %d" % (what, len(got), len(want))
    for f in ("node", "depth", "parent", "support"):
        assert np.array_equal(got[f], want[f]), "%s: %s differs at rows %s" % (what, f, np.nonzero(got[f] != want[f])[0][:8])
    assert np.array_equal(got["pvalue"].view(np.uint32), want["pvalue"].view(np.uint32)), "%s: pvalue bits differ" % what
