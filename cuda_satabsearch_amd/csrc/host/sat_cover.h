/*
 * sat_cover.h - clustering the database around representatives (-a -D P, sat_cover_* of include/satabsearch.h, DESIGN.md
 * 6r): the layout of the adjacency bit matrix and the packing of a round's arg-max key, ONE definition each for the host
 * (sat_cover.c) and the device (sat_cover.hip), and the host side: the cover itself from an edge list in plain C, and
 * the table the command line prints.
 *
 * The graph: nodes 0 .. n - 1, undirected edges between DIFFERENT nodes; an edge seen twice or in both directions is one
 * edge.  degree[v] = the distinct neighbours of v.  The greedy cover:
 *     unassigned = all nodes
 *     repeat: gain(v) = 1 + |adj(v) & unassigned| for every unassigned v; v* = the largest gain, ties to the smallest
 *             index; gain(v*) == 1: stop - every node left is its own representative; else v* and its unassigned
 *             neighbours get rep = v* and leave unassigned
 * So every node is its representative or adjacent to it, and no two representatives are adjacent.
 */
#ifndef SAT_COVER_H
#define SAT_COVER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifdef __HIPCC__
#define SAT_COVER_FN __host__ __device__ static inline
#else
#define SAT_COVER_FN static inline
#endif

/* The bit matrix: row v is `stride` 64-bit words, node u is bit (u & 63) of word (u >> 6); the bits from n up are 0 */
SAT_COVER_FN size_t sat_cover_stride(int n) { return ((size_t)n + 63) >> 6; }
SAT_COVER_FN size_t sat_cover_word(int32_t v) { return (size_t)v >> 6; }
SAT_COVER_FN unsigned long long sat_cover_bit(int32_t v) { return 1ull << (v & 63); }
/* the bits of word w that are nodes below n (all of them but in the last word) */
SAT_COVER_FN unsigned long long sat_cover_valid(int n, size_t w)
{
    const size_t first = w << 6;
    if (first + 64 <= (size_t)n) return ~0ull;
    return first >= (size_t)n ? 0ull : (1ull << ((size_t)n - first)) - 1ull;
}

/* A round's key: the larger key wins, so the larger gain does and among equal gains the smaller node.  0 is below the
 * key of every gain >= 1 */
SAT_COVER_FN unsigned long long sat_cover_key(uint32_t gain, int32_t v) { return ((unsigned long long)gain << 32) | (0xffffffffu - (uint32_t)v); }
SAT_COVER_FN uint32_t sat_cover_key_gain(unsigned long long key) { return (uint32_t)(key >> 32); }
SAT_COVER_FN int32_t sat_cover_key_node(unsigned long long key) { return (int32_t)(0xffffffffu - (uint32_t)key); }

/*
 * The table of a cover: size[v] = the members of v's cluster.  Returns the number of clusters (the v with rep[v] == v),
 * or -1 on a bad argument: n < 1, a null array, or a rep that is no cover table (a rep[v] outside 0 .. n - 1, or
 * rep[rep[v]] != rep[v]).
 */
int sat_cover_sizes(int n, const int32_t *rep, int32_t *size);

/*
 * The specification above from the edge list (a[i], b[i]), i < n_pairs: self pairs are no edges, repeats and the two
 * directions of a pair are one edge.  rep[n]; degree[n] may be NULL.  Returns the number of rounds (the clusters of two or
 * more members), or -1 on a bad argument (n < 1, n_pairs < 0, a null array, a node outside 0 .. n - 1) or when the
 * n * ceil(n / 64) words of the matrix cannot be allocated.
 */
int sat_cover_greedy(int n, long long n_pairs, const int32_t *a, const int32_t *b, int32_t *rep, int32_t *degree);

#ifdef __cplusplus
}
#endif
#endif
