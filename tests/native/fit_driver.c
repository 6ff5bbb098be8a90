/* fit_driver.c - the Gumbel fit of csrc/host/sat_gumbel.c as a stand-alone program, for the sanitizer run of
 * tests/test_fit_cpu.py: built once normally and once with -fsanitize=address,undefined, both builds must print the
 * same bytes and the second no report.
 *
 *   fit_driver [histogram.txt]
 *
 * Runs the edge histograms (empty, one bin, everything in the overflow bin, two bins with censor = 0.5, a spread with
 * negative rows counted through sat_stat_histogram) and, when given, a histogram file of "bin count" lines, each at
 * censor 0, 0.01, 0.05 and 0.5, then the bad censors; prints every result and the ends of its table. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sat_gumbel.h"

static void report(const char *what, const uint32_t *counts, double censor)
{
    sat_fit f;
    memset(&f, 0xA5, sizeof f);
    const int rc = sat_gumbel_fit_binned(counts, censor, &f);
    printf("%s censor %g: rc %d", what, censor, rc);
    if (rc != 0) {
        printf("\n");
        return;
    }
    printf(" fitted %d a %.17g b %.17g rows %d censored %d below %d\n", f.fitted, f.a, f.b, f.rows, f.censored, f.below);
    double *z = malloc(sizeof(double) * SAT_STAT_BINS), *p = malloc(sizeof(double) * SAT_STAT_BINS);
    if (!z || !p)
        exit(2);
    sat_gumbel_fit_table(f.a, f.b, z, p);
    int ordered = 1;
    for (int k = 1; k < SAT_STAT_BINS; k++)
        ordered &= z[k] > z[k - 1] && p[k] <= p[k - 1];
    printf("  table z %.17g .. %.17g p %.17g .. %.17g ordered %d\n", z[0], z[SAT_STAT_BINS - 1], p[0], p[SAT_STAT_BINS - 1],
           ordered);
    free(z);
    free(p);
}

static void all_censors(const char *what, const uint32_t *counts)
{
    static const double censors[] = { 0.0, 0.01, 0.05, 0.5 };
    for (size_t i = 0; i < sizeof censors / sizeof censors[0]; i++)
        report(what, counts, censors[i]);
}

int main(int argc, char **argv)
{
    uint32_t *counts = calloc(SAT_STAT_BINS, sizeof(uint32_t));
    if (!counts)
        return 2;
    all_censors("empty", counts);

    counts[300] = 586;
    all_censors("one bin", counts);

    memset(counts, 0, sizeof(uint32_t) * SAT_STAT_BINS);
    counts[SAT_STAT_BINS - 1] = 1000;
    all_censors("overflow only", counts);

    memset(counts, 0, sizeof(uint32_t) * SAT_STAT_BINS);
    counts[100] = 500;
    counts[200] = 500;
    all_censors("two bins", counts);

    /* a spread of scores through the host histogram: negatives, zeros, bin edges, the overflow bin */
    memset(counts, 0, sizeof(uint32_t) * SAT_STAT_BINS);
    enum { N = 2000 };
    int32_t *scores = malloc(sizeof(int32_t) * N), *orders = malloc(sizeof(int32_t) * N), below = 0;
    if (!scores || !orders)
        return 2;
    for (int e = 0; e < N; e++) {
        orders[e] = 1 + e % 111;
        scores[e] = e % 97 == 0 ? -1 - e % 5 : (e % 89 == 0 ? 4000 : (e * 7) % 40);
    }
    sat_stat_histogram(scores, N, 19, orders, counts, &below);
    printf("spread: below %d bin(-3) %d bin(0) %d bin(65 of 19+111) %d bin(1040 of 19+111) %d\n", (int)below,
           sat_stat_bin(-3, 19, 111), sat_stat_bin(0, 19, 111), sat_stat_bin(65, 19, 111), sat_stat_bin(1040, 19, 111));
    all_censors("spread", counts);
    free(scores);
    free(orders);

    report("bad censor", counts, -0.01);
    report("bad censor", counts, 0.51);
    report("bad censor", counts, NAN);

    if (argc > 1) {
        FILE *fp = fopen(argv[1], "r");
        if (!fp) {
            fprintf(stderr, "cannot open %s\n", argv[1]);
            return 2;
        }
        memset(counts, 0, sizeof(uint32_t) * SAT_STAT_BINS);
        int bin;
        unsigned c;
        while (fscanf(fp, "%d %u", &bin, &c) == 2)
            if (bin >= 0 && bin < SAT_STAT_BINS)
                counts[bin] = c;
        fclose(fp);
        all_censors("file", counts);
    }
    free(counts);
    return 0;
}
