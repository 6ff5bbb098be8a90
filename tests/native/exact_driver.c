/*
 * exact_driver.c - stand-alone driver of the exact search's host twin (csrc/host/sat_exact.c) for the sanitizer build of
 * tests/test_exact_cpu.py: seeded random pairs at the limits of the interface - queries of 1 and of 16 SSEs, entries of
 * 1 and of 111 SSEs, both orders, budgets of 1 node, one node a unit and 2^32 - with the invariants that need no
 * reference: base <= score, nodes <= max_nodes, a changed row has a map of the right types, the refused arguments.
 * Prints one checksum line; exits 1 on a broken invariant.
 */
#include <stdio.h>
#include <stdlib.h>
#include "sat_exact.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33) % n;
}

int main(void)
{
    enum { QP = 16, N2MAX = 111 };
    static const uint8_t codes[8] = { 0x00, 0x01, 0x11, 0x13, 0x23, 0x22, 0x32, 0x30 };
    uint64_t sum = 0;
    int bad = 0;
    for (int round = 0; round < 400; round++) {
        const int n1 = round % 7 == 0 ? 16 : 1 + (int)rnd(6), n2 = round % 11 == 0 ? N2MAX : 1 + (int)rnd(20);
        const int lorder = (int)rnd(2);
        uint8_t qtab[QP * QP], qtypes[QP];
        float qd[QP * QP];
        uint8_t *tri = malloc((size_t)n2 * (n2 + 1) / 2);          /* exact sizes: an overrun is the sanitizer's to see */
        float *dist = malloc(sizeof(float) * (size_t)n2 * (n2 + 1) / 2);
        if (!tri || !dist) return 2;
        for (int i = 0; i < n1; i++) {
            qtypes[i] = (uint8_t)rnd(3);
            for (int k = 0; k <= i; k++) {
                qtab[i * QP + k] = qtab[k * QP + i] = codes[rnd(8)];
                qd[i * QP + k] = qd[k * QP + i] = (float)rnd(30) + 0.5f * (float)rnd(2);
            }
        }
        if (n1 > 1 && round % 5 == 0) qd[1] = qd[QP] = NAN;
        for (int i = 0, c = 0; i < n2; i++)
            for (int k = 0; k <= i; k++, c++) {
                tri[c] = k == i ? (uint8_t)rnd(3) : codes[rnd(8)];
                dist[c] = k == i ? (float)tri[c] : (float)rnd(30);
            }
        if (n2 > 1 && round % 3 == 0) dist[1] = round % 2 ? INFINITY : 140.0f;
        int32_t base_map[QP], map[QP], score = 0;
        for (int i = 0; i < QP; i++) base_map[i] = -1;
        const int units = sat_exact_units(n1, n2, lorder);
        const uint64_t budgets[3] = { 1, (uint64_t)units, n1 == 16 || n2 == N2MAX ? 200000u : (uint64_t)1 << 32 };
        for (int b = 0; b < 3; b++) {
            uint8_t flag = 0;
            uint32_t nodes = 0;
            if (sat_exact_host(n1, qtab, qd, QP, qtypes, n2, tri, dist, lorder, budgets[b], 0, base_map, &score, map, &flag, &nodes) != 0)
                bad |= 1;
            if (score < 0 || nodes > budgets[b]) bad |= 2;
            for (int i = 0; i < n1; i++)
                if (map[i] >= 0 && (map[i] >= n2 || (tri[map[i] * (map[i] + 1) / 2 + map[i]] & 3u) != qtypes[i])) bad |= 4;
            if (score == 0)
                for (int i = 0; i < n1; i++)
                    if (map[i] != -1) bad |= 8;
            sum = sum * 1000003u + (uint64_t)(uint32_t)score * 7u + nodes + flag;
        }
        /* refusals */
        if (sat_exact_host(17, qtab, qd, QP, qtypes, n2, tri, dist, lorder, 10, 0, base_map, &score, map, NULL, NULL) != -1) bad |= 16;
        if (sat_exact_host(n1, qtab, qd, QP, qtypes, n2, tri, dist, lorder, 0, 0, base_map, &score, map, NULL, NULL) != -1) bad |= 16;
        if (sat_exact_host(n1, qtab, qd, QP, qtypes, 112, tri, dist, lorder, 10, 0, base_map, &score, map, NULL, NULL) != -1) bad |= 16;
        free(tri);
        free(dist);
    }
    printf("exact_driver checksum %llu bad %d\n", (unsigned long long)sum, bad);
    return bad ? 1 : 0;
}
