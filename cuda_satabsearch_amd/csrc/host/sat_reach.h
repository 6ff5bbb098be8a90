/*
 * sat_reach.h - the host side of the transitive search (sat_reach_* of include/satabsearch.h), plain C: ONE
 * definition of a node's 64-bit key, used by the host (sat_reach.c, the sharded calls of sat_multi.hip, the Python
 * package) and by the device (sat_reach.hip), the join of the arrays several shards keep over the same nodes, and the
 * rows a caller reads.
 *
 * A node's key, most significant first:
 *   depth   bits 63..58   0 .. SAT_REACH_MAX_DEPTH: the level the node was first reached at; 63: unreached
 *   pbits   bits 57..27   the IEEE bits of (float)p, round to nearest: monotone for p >= 0; p <= 0 packs as 0
 *   parent  bits 26..0    the node it was reached through; SAT_REACH_NO_PARENT: none (a seed) or an external query
 * so that unsigned order of the keys is the lexicographic order of (depth, float p, parent), an external parent last, and
 * an unreached node - all ones - is above every key that can be packed.  A seed is depth 0, pbits 0, no parent.
 */
#ifndef SAT_REACH_H
#define SAT_REACH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifdef __HIPCC__
#define SAT_REACH_FN __host__ __device__ static inline
#else
#define SAT_REACH_FN static inline
#endif

#define SAT_REACH_UNREACHED  0xFFFFFFFFFFFFFFFFull
#define SAT_REACH_NO_PARENT  0x7FFFFFF      /* also the largest node count: nodes are 0 .. 2^27 - 2 */
#define SAT_REACH_MAX_DEPTH  62
#define SAT_REACH_NO_DEPTH   63

/* a reached node as the caller reads it: the layout of struct sat_reach_row of include/satabsearch.h, 20 bytes */
typedef struct sat_reach_rec {
    int32_t node, depth, parent, support;
    float pvalue;
} sat_reach_rec;

/* the 31 bits p packs as */
SAT_REACH_FN uint32_t sat_reach_pbits(double p)
{
    union { float f; uint32_t u; } v;
    if (!(p > 0.0)) return 0u;
    v.f = (float)p;
    return v.u & 0x7FFFFFFFu;
}

/* the key of "reached at `depth` (0 .. 62) through `parent` (a node, or < 0: none / external) at p-value p" */
SAT_REACH_FN uint64_t sat_reach_pack(int32_t depth, double p, int32_t parent)
{
    const uint64_t par = parent < 0 ? (uint64_t)SAT_REACH_NO_PARENT : (uint64_t)parent & 0x7FFFFFFu;
    return ((uint64_t)(uint32_t)depth << 58) | ((uint64_t)sat_reach_pbits(p) << 27) | par;
}

/* a key's three fields: depth 63 for an unreached node, parent -1 for none / external, the float that was packed */
SAT_REACH_FN void sat_reach_unpack(uint64_t key, int32_t *depth, int32_t *parent, float *pvalue)
{
    union { float f; uint32_t u; } v;
    const uint32_t par = (uint32_t)(key & 0x7FFFFFFu);
    v.u = (uint32_t)((key >> 27) & 0x7FFFFFFFu);
    *depth = (int32_t)(key >> 58);
    *parent = par == SAT_REACH_NO_PARENT ? -1 : (int32_t)par;
    *pvalue = v.f;
}

/* the two inline functions above as symbols of the host library, for callers that cannot include this file */
uint64_t sat_reach_pack_key(int32_t depth, double p, int32_t parent);
void sat_reach_unpack_key(uint64_t key, int32_t *depth, int32_t *parent, float *pvalue);

/*
 * Join nsets accumulators over the same n nodes: keys[g * n + v] and support[g * n + v] are node v's in set g.
 * out_keys[v] = the smallest of v's keys, out_support[v] = the sum of its supports: what one accumulator holds after the
 * rows of all sets (atomicMin and atomicAdd commute).  Returns 0, or -1 on a bad argument (n < 1, nsets < 1, a null
 * array).  No work space beyond the outputs, which must not overlap the inputs.
 */
int sat_reach_join(int n, int nsets, const uint64_t *keys, const int32_t *support, uint64_t *out_keys, int32_t *out_support);

/*
 * The reached nodes of n keys and supports as rows, ascending by node: the first min(cap, count) of them to rows (may be
 * NULL when cap is 0).  Returns count, uncapped, or -1 on a bad argument: n < 1 or n > SAT_REACH_NO_PARENT, a null
 * array, cap < 0, rows null with cap > 0, or a reached node whose parent is neither a node below n nor none.
 */
int sat_reach_decode(int n, const uint64_t *keys, const int32_t *support, int cap, sat_reach_rec *rows);

#ifdef __cplusplus
}
#endif
#endif
