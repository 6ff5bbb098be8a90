/*
 * sat_exact.c - the host twin of the exact search's proof pass (sat_exact.h; exact_pass of sat_exact.hip does the same
 * work on the device): one (query, entry) pair, its units walked one after the other in unit order.
 */
#include "sat_exact.h"

int sat_exact_host(int32_t n1, const uint8_t *qtab, const float *qdmat, int32_t qpitch, const uint8_t *qtypes, int32_t n2,
                   const uint8_t *tab_tri, const float *dist_tri, int32_t lorder, uint64_t max_nodes, int32_t base_score,
                   const int32_t *base_map, int32_t *score, int32_t *map, uint8_t *unproven, uint32_t *nodes)
{
    enum { MAXN2 = 111, CELLS = MAXN2 * (MAXN2 + 1) / 2 };
    if (n1 < 1 || n1 > SAT_EXACT_QMAX || n2 < 1 || n2 > MAXN2 || qpitch < n1 || max_nodes < 1 || max_nodes > ((uint64_t)1 << 32))
        return -1;
    if (!qtab || !qdmat || !qtypes || !tab_tri || !dist_tri || !score || (map && !base_map)) return -1;

    /* the pair as the device stages it: the query's cells as sat_queries_set lays them out, the entry's triangle cleaned */
    static const float qsent = SAT_EXACT_QSENT;
    uint32_t qcell[SAT_EXACT_QMAX * SAT_EXACT_QPITCH * 2];
    float dist[CELLS];
    uint8_t type2[MAXN2];
    for (int32_t i = 0; i < n1; i++)
        for (int32_t k = 0; k < n1; k++) {
            float d = qsent;
            uint32_t code = 0;
            if (k != i) {
                const float x = qdmat[(size_t)i * qpitch + k];
                if (isfinite(x)) d = x;
                code = qtab[(size_t)i * qpitch + k];
            }
            memcpy(&qcell[2 * (i * SAT_EXACT_QPITCH + k)], &d, sizeof d);
            qcell[2 * (i * SAT_EXACT_QPITCH + k) + 1] = code;
        }
    const int32_t ncell = n2 * (n2 + 1) / 2;
    for (int32_t c = 0; c < ncell; c++) dist[c] = fabsf(dist_tri[c]) <= 3.0e38f ? dist_tri[c] : SAT_EXACT_DSENT;
    sat_exact_view v = { n1, n2, lorder ? 1 : 0, 0u, qcell, qtypes, dist, tab_tri, type2 };
    for (int32_t j = 0; j < n2; j++) {
        type2[j] = tab_tri[j * (j + 1) / 2 + j] & 3u;
        v.present |= 1u << type2[j];
    }

    const int32_t units = sat_exact_units(n1, n2, v.lorder);
    uint32_t stack[SAT_EXACT_QMAX];
    uint8_t bmap[SAT_EXACT_QMAX], wmap[SAT_EXACT_QMAX];
    int32_t best = base_score, win = -1, flag = 0;
    uint64_t total = 0;
    for (int32_t u = 0; u < units; u++) {
        sat_exact_unit_result r;
        sat_exact_unit(&v, u, sat_exact_share(max_nodes, units, u), base_score, stack, 1, bmap, &r);
        total += r.nodes;
        flag |= r.exhausted;
        if (r.score != SAT_EXACT_NONE && r.score > best) {   /* equal scores: the lowest unit stays */
            best = r.score;
            win = u;
            memcpy(wmap, bmap, sizeof wmap);
        }
    }
    *score = best;
    if (map)
        for (int32_t i = 0; i < n1; i++) map[i] = win >= 0 ? (int32_t)wmap[i] - 1 : base_map[i];
    if (unproven) *unproven = (uint8_t)flag;
    if (nodes) *nodes = total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)total;
    return 0;
}
