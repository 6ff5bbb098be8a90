/*
 * sat_cluster.h - the host side of the single-linkage clustering (plain C): joining the labels several shards give
 * the same nodes, and the table the command line prints, and the check that clusterings at several cutoffs are nested.  The graph itself
 * is built on the GPUs (sat_cluster_* of include/satabsearch.h); these functions are all the host
 * does, for the command line, sat_multi.hip and the Python package alike.
 *
 * A labelling of n nodes gives node v the label label[v] in 0 .. n - 1, a node of v's own component; nodes with one
 * label are one component.  It is CANONICAL when label[v] is the smallest node of v's component.
 */
#ifndef SAT_CLUSTER_H
#define SAT_CLUSTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Join nsets labellings of the same n nodes: labels[g * n + v] is node v's label in set g (any node of v's component
 * there, canonical or not).  Two nodes end in one component iff a chain of (v, labels[g][v]) links joins them.
 * out[v] (n entries, not overlapping labels) = the smallest node of v's component: the canonical labelling.
 * Returns 0, or -1 on a bad argument (n < 1, nsets < 1, a null array, a label outside 0 .. n - 1; out is then
 * unspecified).  Uses out as its only work space.
 */
int sat_cluster_join(int n, int nsets, const int32_t *labels, int32_t *out);

/*
 * The table of a canonical labelling: rep[v] = the member of v's cluster with the largest degree[] (ties: the smallest
 * index), size[v] = the members of v's cluster.  degree may be NULL (every degree 0: the representative is the
 * cluster's smallest node).  Returns the number of clusters, or -1 on a bad argument (n < 1, a null array, a labelling
 * that is not canonical).  No work space beyond rep and size.
 */
int sat_cluster_reps(int n, const int32_t *label, const int32_t *degree, int32_t *rep, int32_t *size);

/*
 * The check of a family of clusterings at several cutoffs (sat_cluster_*_levels): labels[j * n + v] is node
 * v's label at level j, tightest cutoff first.  Single linkage is monotone in the cutoff, so every level REFINES the
 * next: a cluster of level j lies inside one cluster of level j + 1, that is labels[j + 1][v] == labels[j + 1][labels[j][v]]
 * for every v.  Returns 0 iff every level is a canonical labelling and each refines the next; -1 on a bad argument
 * (n < 1, n_levels < 1, a null array) or a level that is no canonical labelling; k > 0 when levels k and k + 1 (counted
 * from 1) are the first pair whose nesting is broken.  Reads only: no work space at all.
 */
int sat_cluster_nested(int n, int n_levels, const int32_t *labels);

#ifdef __cplusplus
}
#endif
#endif
