/*
 * sat_reorder.h - the order of a solution map (-X, sat_reorder_hits of include/satabsearch.h): ONE
 * definition of what makes a map sequential, a circular permutation or out of order, used by the host (sat_reorder.c,
 * the Python package, the command line) and by the device (the kernels of sat_reorder.hip), so that a row's kind is the
 * same on either side.
 *
 * A map m[0 .. n1) gives every query SSE its db SSE or -1; no db SSE twice.  With j_1 .. j_t the images of the matched
 * query SSEs in query order:
 *   matched  = t
 *   descents = #{ s : j_(s+1) < j_s }
 *   kind     = SAT_KIND_SEQUENTIAL  descents == 0 (t <= 1 too)
 *              SAT_KIND_CIRCULAR    descents == 1 and j_t < j_1: two ascending runs, the second wholly below the
 *                                   first - a rotation
 *              SAT_KIND_PERMUTED    everything else
 *   cut      = the 1-based query SSE at which the second run starts (kind circular), else 0
 * The walk takes one element at a time, so the same text reads the device's int8 maps and the host's int32 rows.
 */
#ifndef SAT_REORDER_H
#define SAT_REORDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifdef __HIPCC__
#define SAT_REORDER_FN __host__ __device__ static inline
#else
#define SAT_REORDER_FN static inline
#endif

#define SAT_KIND_SEQUENTIAL 1
#define SAT_KIND_CIRCULAR   2
#define SAT_KIND_PERMUTED   4
#define SAT_KIND_ALL        7

/* the walk over a map: what the elements so far gave; `cut` is that of the LAST descent until sat_map_walk_kind */
typedef struct sat_map_walk {
    int32_t matched, descents, first, last, cut;
} sat_map_walk;

SAT_REORDER_FN void sat_map_walk_begin(sat_map_walk *w)
{
    w->matched = w->descents = w->cut = 0;
    w->first = w->last = -1;
}

/* query SSE i (0-based, ascending from call to call) maps to db SSE j, or to nothing (j < 0) */
SAT_REORDER_FN void sat_map_walk_add(sat_map_walk *w, int32_t i, int32_t j)
{
    if (j < 0) return;
    if (w->matched == 0) w->first = j;
    else if (j < w->last) {
        w->descents++;
        w->cut = i + 1;
    }
    w->last = j;
    w->matched++;
}

/* behind the last element: the kind; cut is left 0 unless the map is circular */
SAT_REORDER_FN int32_t sat_map_walk_kind(sat_map_walk *w)
{
    if (w->descents == 1 && w->last < w->first) return SAT_KIND_CIRCULAR;
    w->cut = 0;
    return w->descents == 0 ? SAT_KIND_SEQUENTIAL : SAT_KIND_PERMUTED;
}

/*
 * A whole int32 map on the host: returns the kind, and matched / descents / cut where the pointers are not NULL.
 * n1 = 0 is the empty map (sequential).  -1 on a bad argument: n1 < 0, or map NULL with n1 > 0.
 */
int32_t sat_map_kind(const int32_t *map, int32_t n1, int32_t *matched, int32_t *descents, int32_t *cut);

#ifdef __cplusplus
}
#endif
#endif
