/*
 * sat_gumbel.h - score normalisation and Gumbel tail statistics for the
 * "name rawscore norm2score z-score p-value" output row.
 *
 * Follows nvcc_src_current/gumbelstats.c:50-58 (z), :69-72 (p), :91-94 (norm2)
 * and the location/scale constants gumbelstats.h:22-23.
 */
#ifndef SAT_GUMBEL_H
#define SAT_GUMBEL_H
#include <stdint.h>
#include "sat_stats.h"
#ifdef __cplusplus
extern "C" {
#endif

#define SAT_GUMBEL_A 0.3780327676087335
#define SAT_GUMBEL_B 0.3582596175507505

/* norm2 = 2*score / (n1 + n2), in double */
double sat_norm2(int score, int n1, int n2);

/*
 * z of a Gumbel(a,b) variate.  The reference prototype takes an `int x`
 * (gumbelstats.h:26) and is called with the double norm2 score
 * (cudaSaTabsearch.cu:446), so the score is truncated toward zero first:
 * z only takes the values of x = ..., -1, 0, 1, 2, ...  Kept, because the
 * printed z and p columns depend on it.
 */
double sat_z_gumbel_trunc(double norm2score);

/* p = 1 - exp(-exp(-(pi/sqrt(6) * z + euler_gamma))) */
double sat_pv_gumbel(double z);

/*
 * ---- Gumbel parameters fitted to a search's own scores (-F).  The constants above were fitted once, to
 * one database, one restart count and one mix of queries (gumbelstats.h:21); the reference's workflow re-fits them to
 * the scores at hand (scripts/fitgumbeldist.r).  Here a query's norm2 scores are counted in the integer histogram of
 * sat_stats.h and the fit is a maximum-likelihood fit to the bin midpoints.
 */
#ifndef SAT_EINVAL
#define SAT_EINVAL -1
#endif

#ifndef SAT_FIT_DEFINED
#define SAT_FIT_DEFINED
typedef struct sat_fit {
    double  a, b;       /* location and scale; the built-in constants when fitted == 0                       */
    int32_t rows;       /* rows in the histogram's bins                                                      */
    int32_t censored;   /* of them, rows above the censoring point (the overflow bin included)               */
    int32_t below;      /* rows with a negative score: in no bin, not fitted (filled in by whoever counted)  */
    int32_t fitted;     /* 0: no fit exists, the query keeps the built-in statistics                         */
} sat_fit;
#endif

/* the bin of a row (sat_stats.h), -1 for score < 0 */
int sat_stat_bin(int score, int n1, int n2);

/* The host restatement of the device's histogram kernel: for e < n, the row (scores[e], n1, orders[e]) is ADDED to
 * counts[SAT_STAT_BINS] or, when its score is negative, to *below.  The caller zeroes both (shards add up). */
void sat_stat_histogram(const int32_t *scores, int n, int n1, const int32_t *orders, uint32_t *counts, int32_t *below);

/*
 * Maximum-likelihood Gumbel(a, b) of a histogram, right-censored.  Bin k stands for x_k = (k + 0.5) / 256.  With n the
 * rows of all bins, the overflow bin is always censored, and further whole bins are taken from the top while the
 * censored total stays <= max(floor(censor * n), overflow count); x_c is the upper edge of the highest uncensored bin,
 * n_c the censored rows.  Maximised over (a, log b), t = (x - a) / b:
 *     sum_k c_k * (-log b - t_k - exp(-t_k)) + n_c * log(1 - exp(-exp(-t_c)))
 * by Newton steps with analytic derivatives and step halving from the moments of the uncensored bins.  censor = 0 is
 * the plain MLE of fitgumbeldist.r on everything but the overflow bin.
 * Returns SAT_EINVAL for a censor outside [0, 0.5] (NaN included) or a null argument, else 0 - also when no fit exists
 * (fewer than 2 occupied uncensored bins, no convergence, a non-finite or non-positive b): then fitted = 0 and a, b
 * are the built-in constants.  out->below is set to 0.
 */
int sat_gumbel_fit_binned(const uint32_t *counts, double censor, sat_fit *out);

/*
 * The statistics of a fitted query, one entry per bin, evaluated at the bin's LOWER edge (conservative, as the
 * reference's truncation to an int is, at 1/256 instead of 1):
 *     z[k] = (k / 256.0 - (a + b * gamma)) / (pi / sqrt 6 * b),   p[k] = sat_pv_gumbel(z[k])
 * With the built-in (a, b), z[256 * x] is sat_z_gumbel_trunc(x) bit for bit.  Every place that needs a fitted row's z
 * and p - the device's tables, the multi-GPU host code, the command line - calls this with the same two doubles.
 */
void sat_gumbel_fit_table(double a, double b, double *z, double *p);

#ifdef __cplusplus
}
#endif
#endif
