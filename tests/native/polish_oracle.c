/*
 * polish_oracle.c - CPU reference of the best-improvement polish of ONE map (test infrastructure, like oracle/).
 *
 * The rule of include/satabsearch.h (sat_search_pairs_polish): from a map m, a move (i, j) re-images query SSE i to the
 * free db SSE j of its type (inside the LORDER window) or to -1; delta = row(i, j | m) - row(i, m[i] | m); the allowed
 * move with the largest delta > 0 is applied, ties to the smallest i, then the smallest j (-1 first), until none is left.
 * This file includes the pinned oracle unchanged, as chain_oracle.c does, and scores with ITS move_delta - the oracle's
 * own tscord and distance test.  tests/polish_lib.py ranks the restarts and picks the winner.
 * Build flags as the oracle's: -O3 -ffp-contract=off.
 */
#include "../../oracle/sa_oracle.c"

/* row(i, j | m): the terms of query SSE i imaged to db SSE j against every other matched SSE; 0 for j = -1 */
static int polish_row(const sa_oracle_query *q, const uint8_t *tab2, const float *dmat2, int pitch2, const int *map,
                      int i, int j)
{
    return j < 0 ? 0 : move_delta(q, tab2, dmat2, pitch2, map, i, -1, j);
}

/* The full score of a map (the oracle's tmscord), for the tests' naive checks. */
int polish_oracle_full_score(const sa_oracle_query *q, const uint8_t *tab2, const float *dmat2, int pitch2, const int *map)
{
    return sa_oracle_full_score(q, tab2, dmat2, pitch2, map);
}

/* Polish map[0 .. n1) in place; `score` is its full score.  Returns the polished score, *moves = accepted moves.
 * The entry is dense with row pitch `pitch2`, its SSE types on the diagonal of tab2. */
int polish_oracle_map(const sa_oracle_query *q, int n2, const uint8_t *tab2, const float *dmat2, int pitch2, int lorder,
                      int *map, int score, int *moves)
{
    const int n1 = q->n;
    uint8_t types2[SA_MAXDIM];
    for (int j = 0; j < n2; j++) types2[j] = tab2[(size_t)j * pitch2 + j];
    *moves = 0;
    for (;;) {
        char used[SA_MAXDIM];
        memset(used, 0, sizeof used);
        for (int i = 0; i < n1; i++)
            if (map[i] >= 0) used[map[i]] = 1;
        int best = 0, bi = -1, bj = -1;
        for (int i = 0; i < n1; i++) {                      /* ascending i, then j from -1: strict > keeps the first */
            const int old = map[i];
            const int oldrow = polish_row(q, tab2, dmat2, pitch2, map, i, old);
            int lo = -1, hi = n2;
            if (lorder) {
                for (int k = 0; k < i; k++)
                    if (map[k] > lo) lo = map[k];
                for (int k = i + 1; k < n1; k++)
                    if (map[k] >= 0 && map[k] < hi) hi = map[k];
            }
            if (old >= 0 && -oldrow > best) {
                best = -oldrow;
                bi = i;
                bj = -1;
            }
            for (int j = lo + 1; j < hi; j++) {
                if (used[j] || types2[j] != q->ssetypes[i]) continue;
                const int d = polish_row(q, tab2, dmat2, pitch2, map, i, j) - oldrow;
                if (d > best) {
                    best = d;
                    bi = i;
                    bj = j;
                }
            }
        }
        if (best <= 0) break;
        map[bi] = bj;
        score += best;
        (*moves)++;
    }
    return score;
}
