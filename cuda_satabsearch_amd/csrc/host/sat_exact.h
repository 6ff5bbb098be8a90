/*
 * sat_exact.h - exact search for small queries (sat_search_exact of include/satabsearch.h): ONE definition
 * of the unit split, the budget split, the bound and the depth-first walk of one unit, compiled by the device
 * (exact_pass of sat_exact.hip) and by the host twin (sat_exact_host of sat_exact.c), so that score, map, flag and node
 * count of a row are the same on either side, in any launch shape and on any number of shards.
 *
 * A feasible map of a query of n1 SSEs into an entry of n2 SSEs is a partial injective map with equal SSE types, under
 * lorder with images ascending in the query index.  Its score is the sum of the pair terms of its matched pairs i < k.
 * The walk assigns the query SSEs in index order; for SSE i it tries the allowed db SSEs in ascending order, then
 * "unmatched".  One such extension evaluated is a NODE.  A node is pruned when
 *     partial score + sat_exact_bound(...) <= max(incumbent, best found so far in this unit)
 * so only maps strictly better than the incumbent are ever recorded, and a unit keeps the first of its best ones.
 *
 * A row's parallel units are its top-level subtrees: unit u < n2 holds the maps with query SSE 0 on db SSE u, unit n2
 * those with SSE 0 unmatched - sat_exact_units(), a function of (n1, n2, lorder) alone.  A row's node budget is split
 * evenly over them (sat_exact_share); a unit that would exceed its share stops and the row is flagged unproven.  A unit
 * prunes with the incumbent and its own best only, never with what another unit found.
 */
#ifndef SAT_EXACT_H
#define SAT_EXACT_H

#include <stdint.h>
#include <string.h>
#include <math.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifdef __HIPCC__
#define SAT_EXACT_FN __host__ __device__ static inline
#else
#define SAT_EXACT_FN static inline
#endif

#define SAT_EXACT_QMAX    16             /* SAT_EXACT_MAX_QUERY of include/satabsearch.h: the levels of a walk      */
#define SAT_EXACT_QPITCH  16             /* cells per row of a query's dense cell array (size class 16)             */
#define SAT_EXACT_NONE    INT32_MIN      /* a unit that recorded no map                                              */
#define SAT_EXACT_QSENT   1.0e30f        /* the query side's "never within 4 A" distance (SAT_K_QSENT)               */
#define SAT_EXACT_DSENT   (-1.0e30f)     /* the db side's (SAT_K_DSENT)                                              */

/* the parallel units of a row, and unit u's share of the row's max_nodes (1 .. 2^32): even, the remainder one each to
 * the lowest units; units >= 2, so a share fits 32 bits */
SAT_EXACT_FN int32_t sat_exact_units(int32_t n1, int32_t n2, int32_t lorder)
{
    (void)n1;
    (void)lorder;
    return n2 + 1;
}
SAT_EXACT_FN uint32_t sat_exact_share(uint64_t max_nodes, int32_t units, int32_t u)
{
    return (uint32_t)(max_nodes / (uint64_t)units) + ((uint64_t)u < max_nodes % (uint64_t)units ? 1u : 0u);
}

/* What the SSEs still to assign can add at most: `matched` SSEs are matched so far, at most r more can be - r the
 * smaller of the query SSEs left whose type the entry has at all and of the db SSEs still free (under lorder: those
 * above the last image).  Every pair among the r and every pair of one of them with a matched one adds at most 2. */
SAT_EXACT_FN int32_t sat_exact_bound(int32_t matched, int32_t r) { return r * (2 * matched + r - 1); }

/* One pair term in plain C: 0 when the distances differ by more than 4 A, else 2 / 1 / -2 for both / one / no nibble of
 * the two code bytes equal - satk::pair_term of sat_sa_kernel.hpp for cleaned cells (no NaN, nibbles <= 7). */
SAT_EXACT_FN int32_t sat_exact_term_c(uint32_t qd_bits, uint32_t qc, uint32_t dd_bits, uint32_t dc)
{
    float qd, dd;
    memcpy(&qd, &qd_bits, sizeof qd);
    memcpy(&dd, &dd_bits, sizeof dd);
    if (!(fabsf(qd - dd) <= 4.0f)) return 0;
    const uint32_t x = qc ^ dc;
    const int hi = (x & 0xF0u) == 0u, lo = (x & 0x0Fu) == 0u;
    return hi && lo ? 2 : (hi || lo ? 1 : -2);
}

/* The device sets these to its own arithmetic before it includes this file. */
#ifndef SAT_EXACT_TERM
#define SAT_EXACT_TERM(qd, qc, dd, dc) sat_exact_term_c(qd, qc, dd, dc)
#endif
#ifndef SAT_EXACT_TRI
#define SAT_EXACT_TRI(j, l) ((j) > (l) ? (j) * ((j) + 1) / 2 + (l) : (l) * ((l) + 1) / 2 + (j))
#endif
#ifndef SAT_EXACT_WALK_FN
#define SAT_EXACT_WALK_FN static inline
#endif

/* A pair as the walk reads it: the query's dense cells {distance bits, code byte} with the sentinel on the diagonal and
 * for non-finite distances, its SSE types; the entry's packed lower triangle with non-finite distances replaced by the
 * sentinel, its SSE types, and `present`, bit t set when the entry has an SSE of type t. */
typedef struct sat_exact_view {
    int32_t n1, n2, lorder;
    uint32_t present;
    const uint32_t *qcell;              /* [n1][SAT_EXACT_QPITCH][2] */
    const uint8_t *qtypes;              /* [n1] */
    const float *dist;                  /* [n2 (n2 + 1) / 2] */
    const uint8_t *code;
    const uint8_t *type2;               /* [n2] */
} sat_exact_view;

typedef struct sat_exact_unit_result {
    int32_t score;                      /* the unit's best score above the incumbent, SAT_EXACT_NONE without one */
    uint32_t nodes;                     /* nodes it expanded, <= its share */
    int32_t exhausted;                  /* it stopped at its share with work left */
} sat_exact_unit_result;

/*
 * The walk of unit `unit` with `share` nodes.  stack: SAT_EXACT_QMAX words, level i at stack[i * stride] - the image of
 * query SSE i + 1 (0: unmatched) in bits 0-7, the largest image so far + 1 in bits 8-15, the matched SSEs so far in
 * bits 16-20, the partial score in bits 21-31.  bmap[0 .. n1): the recorded map as image + 1, written only with a map.
 */
SAT_EXACT_WALK_FN void sat_exact_unit(const sat_exact_view *v, int32_t unit, uint32_t share, int32_t incumbent,
                                      uint32_t *stack, int32_t stride, uint8_t *bmap, sat_exact_unit_result *out)
{
    const int32_t n1 = v->n1, n2 = v->n2, lorder = v->lorder;
    int32_t best = incumbent, found = 0, exhausted = 0;
    uint32_t nodes = 0;
    /* nibble i: the query SSEs behind i whose type the entry has (at most 15) */
    uint64_t remq = 0;
    {
        uint32_t cnt = 0;
        for (int32_t i = n1 - 1; i >= 0; i--) {
            remq |= (uint64_t)cnt << (4 * i);
            cnt += (v->present >> v->qtypes[i]) & 1u;
        }
    }
    int32_t i = 0, c = unit < n2 ? unit : n2;
    if (unit < n2 && v->type2[unit] != v->qtypes[0]) c = n2 + 1;       /* no such map: nothing to expand */
    for (;;) {
        int32_t last = -1, m = 0, ps = 0;
        if (i > 0) {
            const uint32_t w = stack[(i - 1) * stride];
            last = (int32_t)((w >> 8) & 0xFFu) - 1;
            m = (int32_t)((w >> 16) & 0x1Fu);
            ps = (int32_t)w >> 21;
        }
        /* the next candidate from the cursor: a db SSE of the type, free, under lorder above the last image; then n2 =
         * "unmatched"; the root's one candidate is the unit's own */
        int32_t j = c;
        if (i > 0 && j < n2) {
            const uint32_t qt = v->qtypes[i];
            if (lorder && j <= last) j = last + 1;
            for (; j < n2; j++) {
                if (v->type2[j] != qt) continue;
                int32_t used = 0;
                if (!lorder)
                    for (int32_t k = 0; k < i; k++) used |= (int32_t)(stack[k * stride] & 0xFFu) == j + 1;
                if (!used) break;
            }
        }
        if (j > n2) {                                        /* level i is done: back to the level above */
            if (i == 0) break;
            i--;
            const int32_t img1 = (int32_t)(stack[i * stride] & 0xFFu);
            c = (i == 0 || img1 == 0) ? n2 + 1 : img1;
            continue;
        }
        if (nodes >= share) {
            exhausted = 1;
            break;
        }
        nodes++;
        const int32_t on = j < n2;
        int32_t sc = ps;
        if (on)
            for (int32_t k = 0; k < i; k++) {
                const int32_t l1 = (int32_t)(stack[k * stride] & 0xFFu);
                if (l1) {
                    const int32_t cell = SAT_EXACT_TRI(j, l1 - 1);
                    const uint32_t *q = v->qcell + 2 * (i * SAT_EXACT_QPITCH + k);
                    uint32_t dd;
                    memcpy(&dd, &v->dist[cell], sizeof dd);
                    sc += SAT_EXACT_TERM(q[0], q[1], dd, (uint32_t)v->code[cell]);
                }
            }
        const int32_t m2 = m + on, last2 = (on && j > last) ? j : last;
        if (i == n1 - 1) {
            if (sc > best) {                                 /* strictly better: the first such map of its score stays */
                best = sc;
                found = 1;
                for (int32_t k = 0; k < i; k++) bmap[k] = (uint8_t)(stack[k * stride] & 0xFFu);
                bmap[i] = (uint8_t)(on ? j + 1 : 0);
            }
        } else {
            const int32_t rq = (int32_t)((remq >> (4 * i)) & 15u), room = lorder ? n2 - 1 - last2 : n2 - m2;
            if (sc + sat_exact_bound(m2, rq < room ? rq : room) > best) {
                stack[i * stride] = (uint32_t)(on ? j + 1 : 0) | ((uint32_t)(last2 + 1) << 8) | ((uint32_t)m2 << 16) | ((uint32_t)sc << 21);
                i++;
                c = 0;
                continue;
            }
        }
        c = i == 0 ? n2 + 1 : j + 1;
    }
    out->score = found ? best : SAT_EXACT_NONE;
    out->nodes = nodes;
    out->exhausted = exhausted;
}

/*
 * The host twin, one pair: the query as sat_queries_set takes it (dense n1 x n1 codes and distances of row pitch
 * `qpitch`, n1 <= SAT_EXACT_QMAX), the entry as a packed lower triangle (cell (i, j), j <= i, at i (i + 1) / 2 + j; SSE
 * types on the diagonal of tab_tri), the incumbent's score and map (base_map[0 .. n1), -1 = unmatched; may be NULL when
 * map is).  *score, map[0 .. n1): the incumbent's, or the strictly better map's of the lowest unit that found the best
 * score; *unproven: a unit exhausted its share; *nodes: the units' nodes summed, saturating.  Returns 0, or -1 on a bad
 * argument (orders out of range, max_nodes outside 1 .. 2^32, a null array).
 */
int sat_exact_host(int32_t n1, const uint8_t *qtab, const float *qdmat, int32_t qpitch, const uint8_t *qtypes, int32_t n2,
                   const uint8_t *tab_tri, const float *dist_tri, int32_t lorder, uint64_t max_nodes, int32_t base_score,
                   const int32_t *base_map, int32_t *score, int32_t *map, uint8_t *unproven, uint32_t *nodes);

#ifdef __cplusplus
}
#endif
#endif
