/*
 * exact_oracle.c - brute-force reference of the exact search (test infrastructure, like oracle/): EVERY feasible map of
 * one (query, dense entry) pair, no pruning, each scored with the pinned oracle's full score (its tmscord), and the
 * largest score returned.  Independent of csrc/host/sat_exact.h: no bound, no units, no budget, another visiting order
 * (recursion with "unmatched" first), the oracle's own distance test and pair score on the raw cells.
 * This file includes the pinned oracle unchanged, as chain_oracle.c and polish_oracle.c do.
 * Build flags as the oracle's: -O3 -ffp-contract=off.
 */
#include "../../oracle/sa_oracle.c"

typedef struct exact_walk {
    const sa_oracle_query *q;
    const uint8_t *tab2;
    const float *dmat2;
    int pitch2, n2, lorder;
    uint8_t types2[SA_MAXDIM];
    char used[SA_MAXDIM];
    int map[SA_MAXDIM], best_map[SA_MAXDIM];
    int best;
    long long maps;
} exact_walk;

static void exact_rec(exact_walk *w, int i, int last)
{
    if (i == w->q->n) {
        const int s = sa_oracle_full_score(w->q, w->tab2, w->dmat2, w->pitch2, w->map);
        if (w->maps++ == 0 || s > w->best) {
            w->best = s;
            memcpy(w->best_map, w->map, sizeof(int) * (size_t)w->q->n);
        }
        return;
    }
    w->map[i] = -1;
    exact_rec(w, i + 1, last);
    for (int j = w->lorder ? last + 1 : 0; j < w->n2; j++) {
        if (w->used[j] || w->types2[j] != w->q->ssetypes[i]) continue;
        w->used[j] = 1;
        w->map[i] = j;
        exact_rec(w, i + 1, j > last ? j : last);
        w->used[j] = 0;
    }
    w->map[i] = -1;
}

/* The optimum over every feasible map; best_map[0 .. n1) (may be NULL) one map that has it.  Returns the maps seen. */
long long exact_oracle_optimum(const sa_oracle_query *q, int n2, const uint8_t *tab2, const float *dmat2, int pitch2,
                               int lorder, int *best_score, int *best_map)
{
    exact_walk w;
    memset(&w, 0, sizeof w);
    w.q = q;
    w.tab2 = tab2;
    w.dmat2 = dmat2;
    w.pitch2 = pitch2;
    w.n2 = n2;
    w.lorder = lorder;
    for (int j = 0; j < n2; j++) w.types2[j] = tab2[(size_t)j * pitch2 + j];
    exact_rec(&w, 0, -1);
    *best_score = w.best;
    if (best_map) memcpy(best_map, w.best_map, sizeof(int) * (size_t)q->n);
    return w.maps;
}

/* The full score of a map (the oracle's tmscord). */
int exact_oracle_full_score(const sa_oracle_query *q, const uint8_t *tab2, const float *dmat2, int pitch2, const int *map)
{
    return sa_oracle_full_score(q, tab2, dmat2, pitch2, map);
}
