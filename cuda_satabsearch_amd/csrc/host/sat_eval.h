/*
 * sat_eval.h - scoring a search against a classification (-E, sat_eval_* of include/satabsearch.h): ONE
 * definition of how a query's two score histograms become its AUC and ROC-n sums, used by the host (sat_eval.c, the
 * sharded call of sat_multi.hip, the Python package) and by the device (eval_reduce of sat_eval.hip), so that the five
 * integers are the same on either side, on any number of shards and in any launch shape.
 *
 * A query of order n1 has the scores -m .. m, m = n1 (n1 - 1), one bin each: bin = score + m (a score outside is
 * clamped in).  pos[bin] counts the counted rows of the query's own class at that score, neg[bin] those of the other
 * classes.  With Pabove(s) the positives at scores above s:
 *   u2 = sum over s of neg[s] * (2 * Pabove(s) + pos[s])          AUC   = u2 / (2 * positives * negatives)
 *   t2 = the same sum over the first n_used = min(n, negatives) negatives from the top, a tie group that straddles the
 *        n-th negative sharing what is left evenly                ROC-n = t2 / (2 * positives * n_used)
 * Mann-Whitney with ties counted half, doubled so that everything stays an integer.
 */
#ifndef SAT_EVAL_H
#define SAT_EVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifdef __HIPCC__
#define SAT_EVAL_FN __host__ __device__ static inline
#else
#define SAT_EVAL_FN static inline
#endif

/* a query's result: the layout of struct sat_eval of include/satabsearch.h, 32 bytes */
typedef struct sat_eval_row {
    uint64_t u2, t2;
    int32_t positives, negatives, n_used, query_class;
} sat_eval_row;

/* the bins of a query of order n1 >= 1, and the bin of a score */
SAT_EVAL_FN int32_t sat_eval_bins(int32_t n1) { return 2 * n1 * (n1 - 1) + 1; }
SAT_EVAL_FN int32_t sat_eval_bin_of(int32_t score, int32_t n1)
{
    const int32_t m = n1 * (n1 - 1);
    return (score < -m ? -m : (score > m ? m : score)) + m;
}

/*
 * The one reducing function: walk `bins` bins from the top (bin bins - 1) down, adding to *acc, which holds what the
 * bins ABOVE them gave - positives = Pabove, negatives = the negatives above, u2, t2 their sums - and leaves with
 * n_used = min(rocn, negatives).  A zeroed *acc and a query's whole table: its result (query_class is not touched).
 * The device hands every lane one bin and the counts above it from a wave-wide scan, and adds the lanes' u2 and t2.
 * The sums fit: positives and negatives are below 2^31, so a term is below 2^31 * 2^32 and so is their sum.
 */
SAT_EVAL_FN void sat_eval_walk(sat_eval_row *acc, const uint32_t *pos, const uint32_t *neg, int32_t bins, int32_t rocn)
{
    for (int32_t b = bins - 1; b >= 0; b--) {
        const uint64_t p = pos[b], g = neg[b];
        const uint64_t w = 2u * (uint64_t)(uint32_t)acc->positives + p;
        const uint64_t room = rocn > acc->negatives ? (uint64_t)(rocn - acc->negatives) : 0u;
        acc->u2 += g * w;
        acc->t2 += (g < room ? g : room) * w;
        acc->positives += (int32_t)p;
        acc->negatives += (int32_t)g;
    }
    acc->n_used = rocn < acc->negatives ? rocn : acc->negatives;
}

/*
 * A whole table on the host: out's five integers from pos[bins] and neg[bins] (bin 0 the lowest score), out's
 * query_class left alone.  Returns 0, or -1 on a bad argument: a null array, bins < 1, rocn < 1, or counts whose sum
 * per side exceeds 2^31 - 1 (out is then unspecified).
 */
int sat_eval_reduce(const uint32_t *pos, const uint32_t *neg, int32_t bins, int32_t rocn, sat_eval_row *out);

#ifdef __cplusplus
}
#endif
#endif
