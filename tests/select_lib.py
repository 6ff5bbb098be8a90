"""What the selection passes must return, for tests only: the rows of best-k and of the p-value cutoff with their
statistics, the score histogram, the fit made of it and the clustering at a p-value, from a score matrix in plain numpy
and the host library's statistics (libsathost: sat_z_gumbel_trunc, sat_pv_gumbel, sat_gumbel_fit_table,
sat_stat_histogram, sat_gumbel_fit_binned - pinned to the reference by the CPU suite).  Nothing here calls the device
library: not sat_topk_hits, not sat_hits_cutoff."""
import ctypes as C

import numpy as np

from cuda_satabsearch_amd import _native
from cuda_satabsearch_amd.search import _FIT_DTYPE, _HIT_DTYPE

BINS, PER_UNIT, MAXDIM = 4096, 256, 111


def host():
    return _native.host_lib()


def host_histogram(scores, n1s, orders):
    counts = np.zeros((len(n1s), BINS), np.uint32)
    below = np.zeros(len(n1s), np.int32)
    orders = np.ascontiguousarray(orders, np.int32)
    for q, n1 in enumerate(n1s):
        row = np.ascontiguousarray(scores[q], np.int32)
        b = C.c_int32(0)
        host().sat_stat_histogram(row.ctypes.data, len(row), int(n1), orders.ctypes.data, counts[q].ctypes.data, C.byref(b))
        below[q] = b.value
    return counts, below


def host_fits(counts, below, censor):
    fits = np.zeros(len(counts), _FIT_DTYPE)
    for q in range(len(counts)):
        f = _native.Fit()
        assert host().sat_gumbel_fit_binned(counts[q].ctypes.data, float(censor), C.byref(f)) == 0
        fits[q] = (f.a, f.b, f.rows, f.censored, below[q], f.fitted)
    return fits


def fit_table(a, b):
    z, p = np.empty(BINS), np.empty(BINS)
    host().sat_gumbel_fit_table(float(a), float(b), z.ctypes.data, p.ctypes.data)
    return z, p


def builtin_stats(norm2):
    """(z, p) of the built-in constants for one norm2: at norm2 truncated toward zero and clamped to -128..127, as the
    device's row documents it (sat_hitrow.hpp; no legal score leaves that range, a planted one can)"""
    x = max(-128, min(127, int(norm2)))
    z = host().sat_z_gumbel_trunc(float(x))
    return z, host().sat_pv_gumbel(float(z))


def expected_rows(scores, n1s, orders, fits):
    """every query's rows in sat_topk_hits order with the statistics the host gives them: the fitted table at the
    row's bin for a query with a fit, else the built-in int-truncated ones"""
    out = []
    for q, n1 in enumerate(n1s):
        order = np.argsort(-scores[q].astype(np.int64), kind="stable")
        rows = np.zeros(len(order), _HIT_DTYPE)
        rows["entry"], rows["score"] = order, scores[q][order]
        tot = n1 + orders[order].astype(np.int64)
        rows["norm2"] = 2.0 * rows["score"] / tot.astype(np.float64)
        if fits is not None and fits[q]["fitted"]:
            z, p = fit_table(fits[q]["a"], fits[q]["b"])
            s = rows["score"].astype(np.int64)
            k = np.where(s < 0, 0, np.minimum((512 * np.maximum(s, 0)) // tot, BINS - 1))
            rows["zscore"], rows["pvalue"] = z[k], p[k]
        else:
            for i, n2 in enumerate(rows["norm2"]):
                rows["zscore"][i], rows["pvalue"][i] = builtin_stats(n2)
        out.append(rows)
    return out


def components(n, a, b):
    """label[v] = the smallest node of v's connected component under the edges (a[i], b[i]): a plain union-find"""
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
    return np.array([find(v) for v in range(n)], np.int32)


class Reference:
    """The selection passes over scores[nq][n]: queries of n1s[q] SSEs, entries of orders[e], fits a sat_fit record
    array (or None: the built-in statistics for every query), maps[q][n][>= n1s[q]] the solution maps of the search
    (or None)."""

    def __init__(self, scores, n1s, orders, fits=None, maps=None):
        self.scores = np.ascontiguousarray(scores, np.int32)
        self.n1s = [int(x) for x in n1s]
        self.orders = np.ascontiguousarray(orders, np.int32)
        self.nq, self.n = self.scores.shape
        assert len(self.n1s) == self.nq and len(self.orders) == self.n
        self.fits, self.maps = fits, maps
        self._rows = expected_rows(self.scores, self.n1s, self.orders, fits)

    def rows(self, q):
        """every row of query q, by (score descending, entry ascending)"""
        return self._rows[q]

    def row_maps(self, q, entries):
        """the int32[rows, 111] maps of the rows of query q against `entries`: the search's map, -1 from the query's
        order on"""
        out = np.full((len(entries), MAXDIM), -1, np.int32)
        n1 = self.n1s[q]
        out[:, :n1] = np.asarray(self.maps[q])[entries, :n1]
        return out

    def topk(self, k):
        """(rows [nq, k'], maps int32[nq, k', 111] or None), k' = min(k, n)"""
        k = min(int(k), self.n)
        rows = np.stack([self._rows[q][:k] for q in range(self.nq)])
        maps = None if self.maps is None else np.stack([self.row_maps(q, rows[q]["entry"]) for q in range(self.nq)])
        return rows, maps

    def cutoff(self, max_p, k=None):
        """(rows per query: those with pvalue <= max_p, cut to k; their maps per query or None; the counts returned)"""
        rows, maps = [], []
        for q in range(self.nq):
            keep = np.nonzero(self._rows[q]["pvalue"] <= max_p)[0]
            if k:
                keep = keep[:k]
            rows.append(self._rows[q][keep])
            maps.append(None if self.maps is None else self.row_maps(q, rows[-1]["entry"]))
        return rows, (None if self.maps is None else maps), np.array([len(r) for r in rows], np.int32)

    def histogram(self):
        """(counts uint32[nq, 4096], below int32[nq]) by the host's sat_stat_histogram"""
        return host_histogram(self.scores, self.n1s, self.orders)

    def fit(self, censor):
        """the sat_fit records sat_stats_fit makes of the histogram"""
        counts, below = self.histogram()
        return host_fits(counts, below, censor)

    def components(self, max_p, query_node, ordinal=None):
        """(labels, degrees, edges) over max(n, nodes named) nodes: every row with pvalue <= max_p whose two ends
        query_node[q] and ordinal[entry] differ is an edge; label[v] = the smallest node of v's component, degrees
        count every edge at both ends, edges all of them"""
        ordinal = np.arange(self.n) if ordinal is None else np.asarray(ordinal)
        a, b = [], []
        for q in range(self.nq):
            e = self._rows[q]["entry"][self._rows[q]["pvalue"] <= max_p]
            a.append(np.full(len(e), int(query_node[q]), np.int64))
            b.append(ordinal[e].astype(np.int64))
        a, b = np.concatenate(a), np.concatenate(b)
        keep = a != b
        a, b = a[keep], b[keep]
        nodes = self.n
        degrees = (np.bincount(a, minlength=nodes) + np.bincount(b, minlength=nodes)).astype(np.int32)
        return components(nodes, a, b), degrees, int(len(a))
