"""Result rows: `name rawscore norm2score z-score p-value` exactly as the reference
prints them (nvcc_src_current/cudaSaTabsearch.cu:415-420 header, :445-453 rows), with
the statistics of csrc/host/sat_gumbel.c (reference gumbelstats.c)."""
from . import _native


def _g(x):
    """C printf("%g") formatting (Python's %g follows the same rules)."""
    return "%g" % x


def stats(score, n1, n2):
    host = _native.host_lib()
    norm2 = host.sat_norm2(int(score), int(n1), int(n2))
    z = host.sat_z_gumbel_trunc(norm2)
    p = host.sat_pv_gumbel(z)
    return norm2, z, p


def stats_fitted(score, n1, n2, a, b):
    """(norm2, z, p) of a row of a query whose Gumbel parameters were fitted to (a, b): z and p at the lower edge of
    the row's histogram bin (sat_gumbel_fit_table; a negative score uses bin 0), as the device and the command line
    print them under -F."""
    import numpy as np
    host = _native.host_lib()
    z = np.empty(_native.STAT_BINS)
    p = np.empty(_native.STAT_BINS)
    host.sat_gumbel_fit_table(float(a), float(b), z.ctypes.data, p.ctypes.data)
    k = max(host.sat_stat_bin(int(score), int(n1), int(n2)), 0)
    return host.sat_norm2(int(score), int(n1), int(n2)), float(z[k]), float(p[k])


def header_lines(qid, dbfile, ltype=True, lorder=True, lsoln=False):
    tf = lambda b: "T" if b else "F"
    return [f"# cudaSaTabsearch LTYPE = {tf(ltype)} LORDER = {tf(lorder)} LSOLN = {tf(lsoln)}",
            "# QUERY ID = %-8s" % qid,
            "# DBFILE = %-80s" % dbfile]


def result_lines(names, orders, scores, n1, ssemaps=None, wide_pvalue_gap=False):
    """wide_pvalue_gap reproduces the two blanks before the p-value that the reference's
    GPU path prints for the large-structure pass (cudaSaTabsearch.cu:1261)."""
    out = []
    gap = "  " if wide_pvalue_gap else " "
    for e, name in enumerate(names):
        norm2, z, p = stats(scores[e], n1, orders[e])
        out.append("%-8s %d %s %s%s%s" % (name, int(scores[e]), _g(norm2), _g(z), gap, _g(p)))
        if ssemaps is not None:
            for i in range(n1):
                j = int(ssemaps[e][i])
                if j >= 0:
                    out.append("%3d %3d" % (i + 1, j + 1))
    return out


def cluster_join(label_sets):
    """Join several labellings of the same nodes (int32[nsets, n], e.g. one per shard) into the canonical one:
    out[v] = the smallest node of v's component (sat_cluster_join of csrc/host/sat_cluster.h)."""
    import numpy as np
    sets = np.ascontiguousarray(label_sets, dtype=np.int32)
    if sets.ndim == 1:
        sets = sets[None, :]
    out = np.empty(sets.shape[1], np.int32)
    if _native.host_lib().sat_cluster_join(sets.shape[1], sets.shape[0], sets.ctypes.data, out.ctypes.data) != 0:
        raise ValueError("labels must lie in 0 .. n - 1 (and n, nsets >= 1)")
    return out


def cluster_table(labels, degrees):
    """(reps int32[n], sizes int32[n]) of the canonical labelling Searcher.cluster_labels returns: reps[v] = the member
    of v's cluster with the largest degree, ties to the smallest index; sizes[v] = the members of v's cluster
    (sat_cluster_reps of csrc/host/sat_cluster.h, which the command line's -L prints from).  The cluster count is
    len(set(labels))."""
    import numpy as np
    lab = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    deg = np.ascontiguousarray(degrees, dtype=np.int32).ravel()
    if lab.shape != deg.shape:
        raise ValueError("labels and degrees differ in length")
    reps = np.empty(len(lab), np.int32)
    sizes = np.empty(len(lab), np.int32)
    if _native.host_lib().sat_cluster_reps(len(lab), lab.ctypes.data, deg.ctypes.data, reps.ctypes.data, sizes.ctypes.data) < 0:
        raise ValueError("labels are not canonical: labels[v] must be the smallest node of v's cluster")
    return reps, sizes


def cluster_levels_table(labels, degrees):
    """(reps int32[L, n], sizes int32[L, n]) of the labellings Searcher.cluster_labels_levels returns (int32[L, n] each,
    tightest level first): cluster_table per level (sat_cluster_reps, which the command line's -H prints from).  Raises
    ValueError when a level is not canonical or a level's clusters do not lie inside the next level's
    (sat_cluster_nested of csrc/host/sat_cluster.h)."""
    import numpy as np
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    deg = np.ascontiguousarray(degrees, dtype=np.int32)
    if lab.ndim != 2 or lab.shape != deg.shape:
        raise ValueError("labels and degrees must both be [levels, n]")
    host = _native.host_lib()
    broken = host.sat_cluster_nested(lab.shape[1], lab.shape[0], lab.ctypes.data)
    if broken < 0:
        raise ValueError("labels are not canonical: labels[j][v] must be the smallest node of v's cluster at level j")
    if broken > 0:
        raise ValueError("the levels are not nested: a cluster of level %d lies in no one cluster of level %d" % (broken, broken + 1))
    reps, sizes = np.empty_like(lab), np.empty_like(lab)
    for j in range(lab.shape[0]):
        host.sat_cluster_reps(lab.shape[1], lab[j].ctypes.data, deg[j].ctypes.data, reps[j].ctypes.data, sizes[j].ctypes.data)
    return reps, sizes


def cover_greedy(n, a, b):
    """(rep int32[n], degrees int32[n], rounds) of the greedy cover of the graph on n nodes with the edges (a[i], b[i]):
    the specification of csrc/host/sat_cover.h in plain C (sat_cover_greedy), for rows that never saw a GPU - what
    Searcher.cover_solve returns for the same edges.  Self pairs are no edges; repeats and both directions are one."""
    import numpy as np
    ea = np.ascontiguousarray(a, dtype=np.int32).ravel()
    eb = np.ascontiguousarray(b, dtype=np.int32).ravel()
    if ea.shape != eb.shape:
        raise ValueError("a and b differ in length")
    n = int(n)
    rep = np.empty(max(n, 0), np.int32)
    deg = np.empty(max(n, 0), np.int32)
    rounds = _native.host_lib().sat_cover_greedy(n, len(ea), ea.ctypes.data, eb.ctypes.data, rep.ctypes.data, deg.ctypes.data)
    if rounds < 0:
        raise ValueError("n must be >= 1 and every node must lie in 0 .. n - 1")
    return rep, deg, rounds


def cover_sizes(rep):
    """(sizes int32[n], clusters) of a cover table: sizes[v] = the members of v's cluster (sat_cover_sizes of
    csrc/host/sat_cover.h, which the command line's -D prints from)."""
    import numpy as np
    r = np.ascontiguousarray(rep, dtype=np.int32).ravel()
    sizes = np.empty(len(r), np.int32)
    clusters = _native.host_lib().sat_cover_sizes(len(r), r.ctypes.data, sizes.ctypes.data)
    if clusters < 0:
        raise ValueError("rep is no cover table: rep[rep[v]] must be rep[v], in 0 .. n - 1")
    return sizes, clusters


def eval_reduce(pos, neg, rocn=50):
    """(u2, t2, positives, negatives, n_used) of one query's two score histograms (equal length, bin 0 the lowest
    score): the sums behind its AUC = u2 / (2 positives negatives) and ROC-n = t2 / (2 positives n_used), by the one
    reducing function of csrc/host/sat_eval.h that the device uses too (sat_eval_reduce)."""
    import ctypes as C
    import numpy as np
    p = np.ascontiguousarray(pos, dtype=np.uint32).ravel()
    g = np.ascontiguousarray(neg, dtype=np.uint32).ravel()
    if p.shape != g.shape:
        raise ValueError("pos and neg differ in length")
    row = _native.Eval()
    if _native.host_lib().sat_eval_reduce(p.ctypes.data, g.ctypes.data, len(p), int(rocn), C.byref(row)) != 0:
        raise ValueError("a table needs bins >= 1, rocn >= 1 and fewer than 2^31 rows a side")
    return int(row.u2), int(row.t2), int(row.positives), int(row.negatives), int(row.n_used)


def eval_ratios(row):
    """(auc, rocn) of a row of Searcher.eval_rows, None for both where the query has no positive or no negative"""
    if row["positives"] <= 0 or row["negatives"] <= 0:
        return None, None
    return (int(row["u2"]) / (2.0 * float(row["positives"]) * float(row["negatives"])),
            int(row["t2"]) / (2.0 * float(row["positives"]) * float(row["n_used"])))


def eval_table(names, class_tokens, rows, dbfile, classfile, entries, classified, restarts, rocn, polish_all=0):
    """The lines the command line's -E prints: names[q] the query's name, class_tokens[id] the token of a class id,
    rows the records of Searcher.eval_rows for all queries in order."""
    out = ["# EVAL dbfile = %s classes = %s entries = %d classified = %d distinct = %d restarts = %d rocn = %d"
           % (dbfile, classfile, entries, classified, len(class_tokens), restarts, rocn)]
    if polish_all:
        out.append("# POLISH tops = %d all rows" % polish_all)
    ratios = [eval_ratios(r) for r in rows]
    both = [r for r in ratios if r[0] is not None]
    auc_sum = rocn_sum = 0.0
    for a, r in both:                                    # summed in query order, as the command line does
        auc_sum += a
        rocn_sum += r
    out.append("# MEAN queries = %d auc = %.6f rocn = %.6f" % (len(both), auc_sum / len(both), rocn_sum / len(both)) if both
               else "# MEAN queries = 0 auc = NA rocn = NA")
    for name, row, (a, r) in zip(names, rows, ratios):
        cls = int(row["query_class"])
        out.append("%-8s %s %d %d %d %d %d %s %s" % (name, class_tokens[cls] if cls >= 0 else "-", row["positives"], row["negatives"],
                                                    int(row["u2"]), int(row["t2"]), row["n_used"],
                                                    "NA" if a is None else "%.6f" % a, "NA" if r is None else "%.6f" % r))
    return out


def profile_core(joint, hits, fraction=0.5):
    """(in_core bool[n1], joint_min) of one query's profile - its uint32[n1, n1] matrix and its hits from
    Searcher.profile_rows: the SSEs every two of which are matched together in at least `fraction` of the hits
    (sat_profile_core of csrc/host/sat_profile.h, which the command line's -W prints from); joint_min is the smallest
    joint count among them, 0 for an empty core."""
    import ctypes as C
    import numpy as np
    j = np.ascontiguousarray(joint, dtype=np.uint32)
    if j.ndim != 2 or j.shape[0] != j.shape[1] or j.shape[0] < 1:
        raise ValueError("joint must be a square matrix of at least one SSE")
    core = np.zeros(j.shape[0], np.uint8)
    least = C.c_uint32(0)
    if _native.host_lib().sat_profile_core(j.shape[0], int(hits), j.ctypes.data, float(fraction), core.ctypes.data, C.addressof(least)) < 0:
        raise ValueError("fraction must lie in (0, 1]")
    return core.astype(bool), int(least.value)


_SSE_TYPE_NAMES = ("e", "xa", "xi", "xg")


def profile_table(names, types, hits, joints, dbfile, pvalue, fraction, restarts, sses=None, polish_all=0, gumbel=None):
    """The lines the command line's -W prints: names[q] the query's name, types[q] its SSEs' type codes (the tableau's
    diagonal: 0 e, 1 xa, 2 xi, 3 xg, or their spellings), hits and joints what Searcher.profile_rows returned for all
    queries in order.  sses[q], where the query is a motif, is its 0-based list in the source entry's numbering (else
    None): the core is then written in that numbering, so that the text after "joint >= J " is a SID@list line.
    gumbel: (censor, fitted) under -F."""
    out = ["# PROFILE dbfile = %s pvalue <= %s fraction >= %s restarts = %d queries = %d" % (dbfile, _g(pvalue), _g(fraction), restarts, len(names))]
    if polish_all:
        out.append("# POLISH tops = %d all rows" % polish_all)
    if gumbel is not None:
        out.append("# GUMBEL censor = %s fitted = %d of %d" % (_g(gumbel[0]), gumbel[1], len(names)))
    for q, name in enumerate(names):
        joint, n1 = joints[q], len(joints[q])
        lst = None if sses is None else sses[q]
        out.append("# QUERY %s sses = %d hits = %d" % (name, n1, int(hits[q])))
        if lst is not None:
            out.append("# QUERY SSES = " + ",".join(str(int(l) + 1) for l in lst))
        core, least = profile_core(joint, hits[q], fraction)
        if not core.any():
            out.append("# CORE none")
        else:
            members = [(int(lst[i]) if lst is not None else i) + 1 for i in range(n1) if core[i]]
            out.append("# CORE sses = %d joint >= %d %s@%s" % (len(members), least, name, ",".join(map(str, members))))
        for i in range(n1):
            t = types[q][i]
            out.append("%d %s %d %s" % (i + 1, t if isinstance(t, str) else _SSE_TYPE_NAMES[int(t) & 3], int(joint[i][i]),
                                        " ".join(str(int(x)) for x in joint[i])))
    return out


KIND_NAMES = {1: "seq", 2: "circ", 4: "perm"}
_KIND_LETTERS = ((1, "s"), (2, "c"), (4, "n"))


def map_kind(ssemap):
    """(kind, matched, descents, cut) of one solution map - the images of the query's SSEs, -1 where unmatched: kind 1
    sequential (no descent among the images in query order), 2 circular (one descent and the last image below the
    first: a rotation; cut = the 1-based query SSE at which the second run starts), 4 permuted (sat_map_kind of
    csrc/host/sat_reorder.h, the definition the device's selection uses)."""
    import ctypes as C
    import numpy as np
    m = np.ascontiguousarray(ssemap, dtype=np.int32).ravel()
    out = (C.c_int32 * 3)()
    base = C.addressof(out)
    kind = _native.host_lib().sat_map_kind(m.ctypes.data if len(m) else None, len(m), base, base + 4, base + 8)
    if kind < 0:
        raise ValueError("bad map")
    return int(kind), int(out[0]), int(out[1]), int(out[2])


def reorder_table(names, rows, maps, n1, min_base_pvalue, kinds, base_fit=None):
    """The lines the command line's -X prints for one query behind its usual header lines: rows and maps what
    Searcher.reorder_hits(..., lsoln=True) returned for it, names the database's, n1 the query's order; base_fit: under
    -F the ordered search's fit record (a, b, rows, censored, below, fitted)."""
    out = ["# REORDER ordered pvalue >= %s kinds = %s" % (_g(min_base_pvalue), "".join(c for bit, c in _KIND_LETTERS if kinds & bit))]
    if base_fit is not None:
        f = base_fit
        out.append("# GUMBEL ordered a = %.17g b = %.17g rows = %d censored = %d below = %d" % (f["a"], f["b"], f["rows"], f["censored"], f["below"])
                   if f["fitted"] else "# GUMBEL ordered not fitted")
    for r, row in enumerate(rows):
        h = row["hit"]
        out.append("%-8s %d %s %s %s %d %s %s %d %d %d" % (names[int(h["entry"])], int(h["score"]), _g(h["norm2"]), _g(h["zscore"]),
                                                         _g(h["pvalue"]), int(row["base_score"]), _g(row["base_pvalue"]),
                                                         KIND_NAMES[int(row["kind"])], int(row["matched"]), int(row["descents"]),
                                                         int(row["cut"])))
        for i in range(n1):
            j = int(maps[r][i])
            if j >= 0:
                out.append("%3d %3d" % (i + 1, j + 1))
    return out


def exact_table(stats, names=None):
    """The statistics of an exact search (Searcher.exact_stats) as text lines: per query its rows, the rows proven
    optimal, the rows the proof pass improved, the mean gain of an improved row and the nodes a row.  names: the queries'
    names (default: their positions)."""
    lines = ["# query rows proven improved mean_gain nodes_per_row"]
    for q, s in enumerate(stats):
        rows, improved = int(s["rows"]), int(s["improved"])
        lines.append("%s %d %d %d %.3f %.1f" % (names[q] if names is not None else str(q), rows, int(s["proven"]), improved,
                                              int(s["gain"]) / improved if improved else 0.0,
                                              int(s["nodes"]) / rows if rows else 0.0))
    return lines


def reach_table(rows, names):
    """The reached nodes of a transitive search (Searcher.reach_rows / search_reach) as text lines `name depth parent_name
    pvalue support`, in the rows' order; a seed or a node reached from an external query has the parent `-`.  names: the
    names of the whole database's structures, by node."""
    lines = ["# name depth parent pvalue support"]
    for r in rows:
        parent = int(r["parent"])
        lines.append("%s %d %s %s %d" % (names[int(r["node"])], int(r["depth"]), names[parent] if parent >= 0 else "-",
                                         _g(float(r["pvalue"])), int(r["support"])))
    return lines


def reach_path(rows, node):
    """The chain of parents from `node` back to a seed (or to a node reached from an external query): the nodes, `node`
    first.  Every link goes one level up, so the chain has depth + 1 nodes.  Raises KeyError for a node the rows do not
    hold, ValueError for rows whose depths do not descend along the chain."""
    by_node = {int(r["node"]): r for r in rows}
    path, at = [int(node)], by_node[int(node)]
    while int(at["parent"]) >= 0:
        up = by_node[int(at["parent"])]
        if int(up["depth"]) != int(at["depth"]) - 1:
            raise ValueError("node %d at depth %d has its parent %d at depth %d" % (int(at["node"]), int(at["depth"]),
                                                                                   int(up["node"]), int(up["depth"])))
        path.append(int(up["node"]))
        at = up
    return path
