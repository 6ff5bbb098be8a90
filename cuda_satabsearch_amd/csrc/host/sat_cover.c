/* sat_cover.c - see sat_cover.h */
#include "sat_cover.h"

#include <stdlib.h>

int sat_cover_sizes(int n, const int32_t *rep, int32_t *size)
{
    if (n < 1 || !rep || !size)
        return -1;
    for (int32_t v = 0; v < n; v++)
        if (rep[v] < 0 || rep[v] >= n || rep[rep[v]] != rep[v])
            return -1;
    int clusters = 0;
    for (int32_t v = 0; v < n; v++)
        size[v] = 0;
    for (int32_t v = 0; v < n; v++) {
        size[rep[v]]++;
        clusters += rep[v] == v;
    }
    /* a member's representative holds the count; a representative is its own and keeps it */
    for (int32_t v = 0; v < n; v++)
        if (rep[v] != v)
            size[v] = size[rep[v]];
    return clusters;
}

/* the lowest set bit's index; x != 0 */
static int low_bit(unsigned long long x)
{
    int i = 0;
    while (!(x & 1ull)) {
        x >>= 1;
        i++;
    }
    return i;
}

int sat_cover_greedy(int n, long long n_pairs, const int32_t *a, const int32_t *b, int32_t *rep, int32_t *degree)
{
    if (n < 1 || n_pairs < 0 || !rep || (n_pairs > 0 && (!a || !b)))
        return -1;
    for (long long i = 0; i < n_pairs; i++)
        if (a[i] < 0 || a[i] >= n || b[i] < 0 || b[i] >= n)
            return -1;
    const size_t stride = sat_cover_stride(n);
    unsigned long long *adj = calloc((size_t)n * stride + stride, sizeof *adj), *un = adj ? adj + (size_t)n * stride : NULL;
    int32_t *gain = malloc(sizeof *gain * (size_t)n);
    if (!adj || !gain) {
        free(adj);
        free(gain);
        return -1;
    }
    for (long long i = 0; i < n_pairs; i++)
        if (a[i] != b[i]) {
            adj[(size_t)a[i] * stride + sat_cover_word(b[i])] |= sat_cover_bit(b[i]);
            adj[(size_t)b[i] * stride + sat_cover_word(a[i])] |= sat_cover_bit(a[i]);
        }
    for (size_t w = 0; w < stride; w++)
        un[w] = sat_cover_valid(n, w);
    /* gain[v] = 1 + |adj(v) & unassigned| for the unassigned v, kept up as nodes leave */
    for (int32_t v = 0; v < n; v++) {
        int32_t d = 0;
        for (size_t w = 0; w < stride; w++)
            for (unsigned long long x = adj[(size_t)v * stride + w]; x; x &= x - 1)
                d++;
        gain[v] = 1 + d;
        rep[v] = v;
        if (degree)
            degree[v] = d;
    }
    int rounds = 0;
    for (;;) {
        int32_t best = -1;
        for (int32_t v = 0; v < n; v++)
            if ((un[sat_cover_word(v)] & sat_cover_bit(v)) && (best < 0 || gain[v] > gain[best]))
                best = v;                               /* strictly larger only: ties stay with the smallest index */
        if (best < 0 || gain[best] == 1)
            break;
        rounds++;
        /* the cluster: best and its unassigned neighbours.  They leave first (the row of best is not its own
         * neighbour, so its bit goes by hand), then every unassigned neighbour of a leaver loses one gain per leaver */
        unsigned long long *row = adj + (size_t)best * stride;
        un[sat_cover_word(best)] &= ~sat_cover_bit(best);
        for (size_t w = 0; w < stride; w++) {
            const unsigned long long members = row[w] & un[w];
            un[w] &= ~members;
            for (unsigned long long x = members; x; x &= x - 1)
                rep[(int32_t)(w << 6) + low_bit(x)] = best;
        }
        for (int32_t u = 0; u < n; u++)
            if (rep[u] == best)
                for (size_t w = 0; w < stride; w++)
                    for (unsigned long long x = adj[(size_t)u * stride + w] & un[w]; x; x &= x - 1)
                        gain[(int32_t)(w << 6) + low_bit(x)]--;
    }
    free(adj);
    free(gain);
    return rounds;
}
