/*
 * sat_stats.h - the score histogram behind the fitted Gumbel statistics (-F): ONE definition of a row's bin, used by
 * the host (sat_gumbel.c) and by the device (sat_topk.hip), so that a histogram made on either side, on any number of
 * shards and in any launch shape, is the same array of integers.
 *
 * A query's rows are counted by norm2 = 2 * score / (n1 + n2) in bins of 1 / SAT_STAT_BINS_PER_UNIT:
 *   score >= 0   bin = min((512 * score) / (n1 + n2), SAT_STAT_BINS - 1), an integer division; it equals
 *                floor(norm2 * 256): a norm2 off a bin edge is at least 1 / (256 * 222) away from it
 *   score <  0   no bin: counted apart ("below"), left out of the fit
 * The last bin takes every norm2 >= 16 - 1/256 (overflow).
 */
#ifndef SAT_STATS_H
#define SAT_STATS_H

#include <stdint.h>

#define SAT_STAT_BINS 4096
#define SAT_STAT_BINS_PER_UNIT 256

#ifdef __HIPCC__
#define SAT_STAT_FN __host__ __device__ static inline
#else
#define SAT_STAT_FN static inline
#endif

/* the bin of a score >= 0 for sum = n1 + n2 >= 1 (32-bit arithmetic: from 2^22 on the product would not fit, and such
 * a score lies far above the overflow edge for every legal sum) */
SAT_STAT_FN int sat_stat_bin_of(int32_t score, int32_t sum)
{
    if (score >= (1 << 22)) return SAT_STAT_BINS - 1;
    const uint32_t b = (512u * (uint32_t)score) / (uint32_t)sum;
    return b > (uint32_t)(SAT_STAT_BINS - 1) ? SAT_STAT_BINS - 1 : (int)b;
}

#endif
