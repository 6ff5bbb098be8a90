/* sat_reorder.c - see sat_reorder.h */
#include "sat_reorder.h"

#include <stddef.h>

int32_t sat_map_kind(const int32_t *map, int32_t n1, int32_t *matched, int32_t *descents, int32_t *cut)
{
    if (n1 < 0 || (!map && n1 > 0))
        return -1;
    sat_map_walk w;
    sat_map_walk_begin(&w);
    for (int32_t i = 0; i < n1; i++)
        sat_map_walk_add(&w, i, map[i]);
    const int32_t kind = sat_map_walk_kind(&w);
    if (matched) *matched = w.matched;
    if (descents) *descents = w.descents;
    if (cut) *cut = w.cut;
    return kind;
}
