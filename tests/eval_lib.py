"""The reference of the evaluation tests (test infrastructure, shared by tests/test_eval_cpu.py and tests/test_gpu_eval.py):
AUC and ROC-n sums by the definition, never through the code under test - every (positive, negative) pair of a query is
compared, and ROC-n expands each tie group of negatives into the share of it that the first n negatives take."""
import numpy as np

EVAL_DTYPE = np.dtype([("u2", np.uint64), ("t2", np.uint64), ("positives", np.int32), ("negatives", np.int32),
                       ("n_used", np.int32), ("query_class", np.int32)], align=True)


def pair_counts(pos, neg, rocn):
    """(u2, t2, positives, negatives, n_used) of a listing given as the scores of its positives and of its negatives.
    A pair (positive, negative) counts 2 when the positive scores higher and 1 on a tie: u2 sums it over all pairs, t2
    over the pairs of the first n_used = min(rocn, negatives) negatives from the top, where a tie group that does not
    fit gives only the share that does - its members are interchangeable, so any k of them count the same."""
    pos, neg = np.asarray(pos, np.int64).ravel(), np.asarray(neg, np.int64).ravel()
    if len(pos) and len(neg):
        w = 2 * (pos[:, None] > neg[None, :]).sum(0, dtype=np.int64) + (pos[:, None] == neg[None, :]).sum(0, dtype=np.int64)
    else:
        w = np.zeros(len(neg), np.int64)
    n_used = min(int(rocn), len(neg))
    order = np.argsort(-neg, kind="stable")
    t2, remaining, i = 0, n_used, 0
    while i < len(neg) and remaining > 0:
        j = i
        while j < len(neg) and neg[order[j]] == neg[order[i]]:
            j += 1
        k = min(j - i, remaining)
        t2 += k * int(w[order[i]])                     # the group's members share one score, so one pair count each
        remaining -= k
        i = j
    return int(w.sum()), t2, len(pos), len(neg), n_used


def table_counts(pos, neg, rocn):
    """pair_counts for a listing given as counts by score (bin 0 the lowest), in Python integers of any size: tie group
    against tie group instead of row against row, so that counts near 2^31 can be checked"""
    pos, neg = [int(x) for x in pos], [int(x) for x in neg]
    w = [sum(2 * pos[a] for a in range(b + 1, len(pos))) + pos[b] for b in range(len(neg))]
    n_used = min(int(rocn), sum(neg))
    t2, remaining = 0, n_used
    for b in range(len(neg) - 1, -1, -1):
        k = min(neg[b], remaining)
        t2 += k * w[b]
        remaining -= k
    return sum(neg[b] * w[b] for b in range(len(neg))), t2, sum(pos), sum(neg), n_used


def clamp(scores, n1):
    m = int(n1) * (int(n1) - 1)
    return np.clip(np.asarray(scores, np.int64), -m, m)


def expected_rows(scores, n1s, query_nodes, node_class, rocn, ordinals=None):
    """the records sat_eval_rows must return for the score matrix [nq, entries]: query q is node query_nodes[q], entry
    e is node ordinals[e] (default e); a row counts when its entry is classified and is not the query's own node"""
    scores = np.asarray(scores).reshape(len(query_nodes), -1)
    node_class = np.asarray(node_class, np.int32)
    ordinals = np.arange(scores.shape[1]) if ordinals is None else np.asarray(ordinals)
    entry_class = node_class[ordinals]
    rows = np.zeros(len(query_nodes), EVAL_DTYPE)
    for q, node in enumerate(query_nodes):
        c = int(node_class[node])
        if c < 0:
            rows[q]["query_class"] = -1
            continue
        counted = (entry_class >= 0) & (ordinals != node)
        s = clamp(scores[q], n1s[q])
        rows[q] = pair_counts(s[counted & (entry_class == c)], s[counted & (entry_class != c)], rocn) + (c,)
    return rows


def expected_tables(scores, n1s, query_nodes, node_class, ordinals=None):
    """the packed uint32 tables sat_eval_tables must return: per query pos[bins] then neg[bins], bins = 2 n1 (n1 - 1) + 1,
    bin = clamped score + n1 (n1 - 1); rows counted as in expected_rows; an unclassified query's table is zero"""
    scores = np.asarray(scores).reshape(len(query_nodes), -1)
    node_class = np.asarray(node_class, np.int32)
    ordinals = np.arange(scores.shape[1]) if ordinals is None else np.asarray(ordinals)
    entry_class = node_class[ordinals]
    out = []
    for q, node in enumerate(query_nodes):
        m = int(n1s[q]) * (int(n1s[q]) - 1)
        tab = np.zeros((2, 2 * m + 1), np.uint32)
        c = int(node_class[node])
        if c >= 0:
            counted = (entry_class >= 0) & (ordinals != node)
            s = clamp(scores[q], n1s[q]) + m
            for side, keep in enumerate((counted & (entry_class == c), counted & (entry_class != c))):
                np.add.at(tab[side], s[keep], 1)
        out.append(tab.ravel())
    return np.concatenate(out)


def same_rows(got, want, what=""):
    assert got.dtype == EVAL_DTYPE or got.dtype.itemsize == 32
    for f in EVAL_DTYPE.names:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, "%s: %s differs at queries %s: got %s, expected %s" % (what, f, bad[:6], got[f][bad[:6]], want[f][bad[:6]])
