/* sat_reach.c - the host side of the transitive search: see sat_reach.h */
#include "sat_reach.h"

#include <stddef.h>

/* sat_reach_pack / sat_reach_unpack as symbols of the host library (the Python package and the tests call them) */
uint64_t sat_reach_pack_key(int32_t depth, double p, int32_t parent) { return sat_reach_pack(depth, p, parent); }
void sat_reach_unpack_key(uint64_t key, int32_t *depth, int32_t *parent, float *pvalue) { sat_reach_unpack(key, depth, parent, pvalue); }

int sat_reach_join(int n, int nsets, const uint64_t *keys, const int32_t *support, uint64_t *out_keys, int32_t *out_support)
{
    if (n < 1 || nsets < 1 || !keys || !support || !out_keys || !out_support) return -1;
    for (int v = 0; v < n; v++) {
        uint64_t k = keys[v];
        uint32_t s = (uint32_t)support[v];                  /* unsigned: the device's atomicAdd wraps, so does this */
        for (int g = 1; g < nsets; g++) {
            const uint64_t kg = keys[(size_t)g * (size_t)n + (size_t)v];
            if (kg < k) k = kg;
            s += (uint32_t)support[(size_t)g * (size_t)n + (size_t)v];
        }
        out_keys[v] = k;
        out_support[v] = (int32_t)s;
    }
    return 0;
}

int sat_reach_decode(int n, const uint64_t *keys, const int32_t *support, int cap, sat_reach_rec *rows)
{
    if (n < 1 || n > SAT_REACH_NO_PARENT || !keys || !support || cap < 0 || (cap > 0 && !rows)) return -1;
    int count = 0;
    for (int v = 0; v < n; v++) {
        sat_reach_rec r;
        sat_reach_unpack(keys[v], &r.depth, &r.parent, &r.pvalue);
        if (r.depth == SAT_REACH_NO_DEPTH) continue;
        if (r.parent >= n) return -1;
        if (count < cap) {
            r.node = v;
            r.support = support[v];
            rows[count] = r;
        }
        count++;
    }
    return count;
}
