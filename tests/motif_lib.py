"""Motif queries (a chosen list of a resident entry's SSEs): what tests/test_motif_cpu.py and
tests/test_gpu_motif.py share - the host-cut dense arrays a motif must equal, the `packed` database with its non-finite
cells, and the spelling of a list on the command line."""
import numpy as np

import cuda_satabsearch_amd as sat

PACKED_ORDERS = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 111)      # both edges of the classes 16, 32, 64 and 112
# the non-finite cells of the packed database: (entry, i, j)
PACKED_NAN, PACKED_INF, PACKED_NEG_INF, PACKED_NAN2 = (4, 16, 3), (7, 32, 31), (10, 110, 0), (1, 1, 0)


def packed_db():
    """the packed upload of tests/test_gpu_queries_from_db.py, made again: the orders at the class edges, a NaN, a +inf
    and a -inf distance cell, every type code"""
    base = sat.synth.make_db(len(PACKED_ORDERS), orders=np.array(PACKED_ORDERS, np.int32), seed=77, sort=False)
    tab, dist = base.tab.copy(), base.dist.copy()

    def cell(s, i, j):
        return int(base.cell_off[s]) + i * (i + 1) // 2 + j

    dist[cell(*PACKED_NAN)] = np.nan             # 17 SSEs: the last row of the entry
    dist[cell(*PACKED_INF)] = np.inf             # 33 SSEs
    dist[cell(*PACKED_NEG_INF)] = -np.inf        # 111 SSEs
    dist[cell(*PACKED_NAN2)] = np.nan            # 2 SSEs: the only off-diagonal cell
    for i, ty in enumerate((0, 1, 2, 3, 3, 2, 1, 0)):
        tab[cell(3, i, i)] = ty                  # 16 SSEs
        tab[cell(10, 100 + i, 100 + i)] = ty
    db = sat.StructSet(base.orders, base.names, base.cell_off, tab, dist)
    assert tuple(db.orders) == PACKED_ORDERS and np.isnan(db.dist).sum() == 2 and np.isinf(db.dist).sum() == 2
    return db


def cut(db, e, sses):
    """the dense query (tab, dist, types) of entry e's SSEs `sses` (0-based, the order given; None or empty: the whole
    entry), cut on the host: cell (i, k) is the entry's cell (sses[i], sses[k])"""
    t, d = db.dense(int(e))
    if sses is None or len(sses) == 0:
        return t, d, db.ssetypes(int(e))
    l = np.asarray(sses, np.int64)
    assert len(set(l.tolist())) == l.size and l.min() >= 0 and l.max() < db.orders[int(e)]
    qt, qd = np.ascontiguousarray(t[np.ix_(l, l)]), np.ascontiguousarray(d[np.ix_(l, l)])
    return qt, qd, np.ascontiguousarray(np.diagonal(qt))


def dense_queries(db, entries, sses):
    return [cut(db, e, l) for e, l in zip(entries, sses)]


def spell(sses):
    """a 0-based list as the command line takes it: 1-based, comma separated"""
    return ",".join(str(int(v) + 1) for v in sses)


def stdin_lines(db, entries, sses):
    return "".join(db.names[int(e)] + ("@" + spell(l) if l is not None and len(l) else "") + "\n" for e, l in zip(entries, sses)).encode()
