// sat_hitrow.hpp - the device code the selection passes share: the row of one (query, entry) score (hit_row), its map as
// the caller's int32 row (row_map), the qualifying predicate of the p-value cutoff (cutoff_row) and the block's count of
// qualifying rows (block_count), for sat_topk.hip (best-k, sat_hits_cutoff) and sat_cluster.hip (sat_cluster_add), so that
// both read the same double from the same table index; and the queries' HitQuery rows on the device (hit_queries).  Not
// part of the public interface.
//
// Everything here stays in an unnamed namespace, as it was in sat_topk.hip: HitQuery is a parameter type of that file's
// kernels, so their symbols - and with them the file's device code - are what they were.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sat_ctx.hpp"
#include "host/sat_gumbel.h"

namespace {

struct HitQuery {
    int32_t n1;
    int32_t fitted;            // 1: the query's rows take their statistics from `fit`
    const int8_t *ssemaps;     // this query's [N][n1] maps, or null
    const double *fit;         // fitted: z[SAT_STAT_BINS] then p[SAT_STAT_BINS] of the query (sat_stats_set), else null
};

// the row of (entry, score) for a query of n1 SSEs against an entry of n2.  fit = null: the built-in statistics, z and p
// of norm2 truncated to an int; else the query's fitted tables at the row's histogram bin (a negative score: bin 0)
__device__ __forceinline__ sat_hit hit_row(int32_t entry, int32_t score, int n1, int n2, const double *ztab, const double *ptab,
                                           const double *fit)
{
    const double norm2 = 2.0 * score / ((double)(n1 + n2));            // sat_norm2
    sat_hit h;
    h.entry = entry;
    h.score = score;
    h.norm2 = norm2;
    if (fit) {
        const int bin = score < 0 ? 0 : sat_stat_bin_of(score, n1 + n2);
        h.zscore = fit[bin];
        h.pvalue = fit[SAT_STAT_BINS + bin];
        return h;
    }
    int x = (int)norm2;                                                // the reference's double -> int
    x = x < -128 ? -128 : (x > 127 ? 127 : x);                         // |norm2| <= 110 for every legal score
    h.zscore = ztab[x + 128];
    h.pvalue = ptab[x + 128];
    return h;
}

// the HitQuery rows sat_hitq_upload / sat_hitq_segments (sat_cutoff.hpp) left in the context
inline const HitQuery *hit_queries(const sat_ctx *ctx) { return reinterpret_cast<const HitQuery *>(ctx->d_hitq.get()); }

// a row's solution map as the caller's int32 row: the n1 images at src, -1 behind them; all -1 without maps (src null)
__device__ __forceinline__ void row_map(const int8_t *src, int n1, int32_t *out)
{
    for (int i = 0; i < SAT_MAXDIM; i++) out[i] = (src && i < n1) ? (int32_t)src[i] : -1;
}

// ---- p-value cutoff.  Blocks of 1024 rows, `bpq` blocks per query, so that a block holds rows of one query only.  A row
// qualifies iff the p-value hit_row gives it is <= max_p: the same double, from the same table index.
constexpr int kCutoffBlock = 1024, kCutoffWaves = kCutoffBlock / 64;

__device__ __forceinline__ bool cutoff_row(const int32_t *scores, int n, int bpq, const int32_t *orders, const HitQuery *queries,
                                           const double *ztab, const double *ptab, double max_p, int &q, int &e, int32_t &score)
{
    q = (int)(blockIdx.x / (unsigned)bpq);
    e = (int)(blockIdx.x - (unsigned)q * bpq) * kCutoffBlock + (int)threadIdx.x;
    if (e >= n) return false;
    score = scores[(size_t)q * n + e];
    return hit_row(e, score, queries[q].n1, orders[e], ztab, ptab, queries[q].fit).pvalue <= max_p;
}

// The block's count of threads with `flag`: a ballot per wave, the 16 counts through LDS, and thread 0 hands their sum
// - when it is not zero - to add(c): ONE atomic per block and counter (one per wave took 170 us)
template <typename F> __device__ __forceinline__ void block_count(bool flag, F add)
{
    __shared__ int32_t wave_count[kCutoffWaves];
    const unsigned long long mask = __ballot(flag);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = (int32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t c = 0;
        for (int w = 0; w < kCutoffWaves; w++) c += wave_count[w];
        if (c) add(c);
    }
}

}  // namespace
