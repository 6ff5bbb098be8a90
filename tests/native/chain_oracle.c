/*
 * chain_oracle.c - CPU reference for ONE restart chain (test infrastructure, like oracle/).
 *
 * Several matches per entry (sat_search_matches) are built from the own best of every restart: s_r = the largest of
 * the chain's initial full score and its 100 proposed scores, map_r = the state where s_r is first reached (strict
 * >, the proposed state).  The pinned oracle only keeps the best over all restarts, so this file includes it
 * unchanged and runs its helpers (chain_begin, random_initial_map, move_delta, pick_free_same_type, the bound
 * helpers) for one restart at a time, in Philox mode.  tests/matches_lib.py pins max_r (s_r, -r) to
 * sa_oracle_search's score and LSOLN map.  Build flags as the oracle's: -O3 -ffp-contract=off.
 */
#include "../../oracle/sa_oracle.c"

/* Own best of restart `restart` of (query, entry): returns s_r, writes map_r[0 .. n1) (-1 = unmatched).
 * The entry is dense with row pitch `pitch2` (types on the diagonal of tab2); streams keyed by
 * (seed, query_ordinal, db_ordinal, restart) exactly as sa_oracle_search's SA_RNG_PHILOX mode. */
int chain_oracle_restart(const sa_oracle_query *q, int n2, const uint8_t *tab2, const float *dmat2, int pitch2,
                         uint32_t db_ordinal, int lorder, uint64_t seed, uint32_t query_ordinal, int restart,
                         int *outmap)
{
    const int n1 = q->n;
    int ssemap[SA_MAXDIM], revmap[SA_MAXDIM];
    uint8_t types2[SA_MAXDIM];
    sa_oracle_rng rng;
    chain_draws draws;
    memset(&rng, 0, sizeof rng);
    rng.mode = SA_RNG_PHILOX;
    rng.seed = seed;
    rng.query_ordinal = query_ordinal;
    for (int j = 0; j < n2; j++) types2[j] = tab2[(size_t)j * pitch2 + j];

    chain_begin(&draws, &rng, db_ordinal, (uint32_t)restart);
    random_initial_map(q, types2, n2, ssemap, revmap, &draws);
    int score = sa_oracle_full_score(q, tab2, dmat2, pitch2, ssemap);
    int rbest = score;
    memcpy(outmap, ssemap, (size_t)n1 * sizeof(int));

    float temp = k_temp0;
    for (int iter = 0; iter < SA_MAXITER; iter++) {
        const int block = SA_PHILOX_STEP_BLOCK0 + (iter >> 1);
        const int word_a = 2 * (iter & 1), word_b = word_a + 1;
        float u = chain_draw16(&draws, block, word_a, 1);
        int ssei = (int)((u - SA_EPS) * n1);
        int startj = 0, endj = n2;
        if (lorder) {
            startj = lower_bound_image(ssemap, ssei, n2);
            endj = upper_bound_image(ssemap, ssei, n1, n2);
        }
        int newj = pick_free_same_type(types2, revmap, startj, endj, q->ssetypes[ssei], &draws, block, word_a);
        int oldj = ssemap[ssei];
        int delta = move_delta(q, tab2, dmat2, pitch2, ssemap, ssei, oldj, newj);
        int newscore = score + delta;
        if (newscore > rbest) {
            rbest = newscore;
            memcpy(outmap, ssemap, (size_t)n1 * sizeof(int));
            outmap[ssei] = newj >= 0 ? newj : -1;
        }
        u = chain_draw(&draws, block, word_b);
        if (expf((float)delta / temp) > u) {
            score = newscore;
            if (oldj >= 0) revmap[oldj] = -1;
            if (newj >= 0) revmap[newj] = ssei;
            ssemap[ssei] = newj >= 0 ? newj : -1;
        }
        temp *= k_alpha;
    }
    return rbest;
}

/* Every restart 0 .. maxstart-1 of one entry: scores[r], maps[r * SA_MAXDIM + i] (i < n1; the rest -1). */
void chain_oracle_entry(const sa_oracle_query *q, int n2, const uint8_t *tab2, const float *dmat2, int pitch2,
                        uint32_t db_ordinal, int lorder, uint64_t seed, uint32_t query_ordinal, int maxstart,
                        int *scores, int *maps)
{
    for (int r = 0; r < maxstart; r++) {
        int *m = maps + (size_t)r * SA_MAXDIM;
        for (int i = 0; i < SA_MAXDIM; i++) m[i] = -1;
        scores[r] = chain_oracle_restart(q, n2, tab2, dmat2, pitch2, db_ordinal, lorder, seed, query_ordinal, r, m);
    }
}
