// sat_reorder.hip - hits that match only out of sequence order, selected on the device (sat_baseline_*, sat_reorder_hits,
// sat_search_reordered).
//
// Two searches of one (database, query batch) are compared where their rows lie.  sat_baseline_keep copies the rows of
// the search at hand - score and p-value, 12 bytes a row - into buffers of the context; a later search (the unordered
// one, with lsoln) is then the searched state, and sat_reorder_hits selects its rows (q, e) that
//   - cutoff_row of sat_hitrow.hpp passes at max_pvalue: the predicate of sat_hits_cutoff, the same double from the same
//     table index,
//   - the baseline did not call a hit: base_pvalue >= min_base_pvalue,
//   - and whose map has one of the asked-for orders (host/sat_reorder.h: sequential, circular, permuted).
// The passes are those of sat_hits_cutoff with this predicate: count (one atomic per block), compact (each block claims
// a run of its query's segment), one segmented radix sort of (score, inverted entry) keys, finish (the rows, 64 bytes
// each, and their maps).  A thread reads its map - n1 bytes at stride n1 - only where both p-value tests pass.  Keys
// are integers and the sort order is total, so the rows do not depend on the launch shape, the chunks or the shards.
// The sort and the cub plumbing are this file's own instantiations: sat_topk.hip's are internal to it, and its code
// stays what it was.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "sat_pairs.hpp"
#include "sat_cutoff.hpp"
#include "sat_hitrow.hpp"
#include "host/sat_reorder.h"

namespace {

// ---- the baseline.  The queries of one launch ride in the kernel's arguments - order and "has a fit" of each - so
// that the call needs no host buffer that would have to outlive it: nothing waits.
constexpr int kBaselineQueries = 256;
struct BaselineQueries {
    uint8_t n1[kBaselineQueries];
    uint32_t fitted[kBaselineQueries / 32];
};

// One thread per row, blocks of 1024 rows of one query.  scores, fit_tabs, base_score and base_p are the launch's first query's.
__global__ void __launch_bounds__(kCutoffBlock) baseline_keep(const int32_t *scores, int n, int bpq, const int32_t *orders,
                                                               BaselineQueries bq, const double *fit_tabs, const double *ztab,
                                                               const double *ptab, int32_t *base_score, double *base_p)
{
    const int q = (int)(blockIdx.x / (unsigned)bpq);
    const int e = (int)(blockIdx.x - (unsigned)q * bpq) * kCutoffBlock + (int)threadIdx.x;
    if (e >= n) return;
    const size_t row = (size_t)q * n + e;
    const int32_t score = scores[row];
    const double *fit = ((bq.fitted[q >> 5] >> (q & 31)) & 1u) ? fit_tabs + (size_t)q * 2 * SAT_STAT_BINS : nullptr;
    base_score[row] = score;
    base_p[row] = hit_row(e, score, (int)bq.n1[q], orders[e], ztab, ptab, fit).pvalue;
}

// ---- the selection.  What a row must pass beyond cutoff_row.
struct ReorderTest {
    double min_base_p;         // <= 0: no condition
    int32_t kinds;             // SAT_KIND_* bits
};

// the order of the map of n1 bytes at `map`
__device__ __forceinline__ int32_t map_order(const int8_t *map, int n1, sat_map_walk &w)
{
    sat_map_walk_begin(&w);
    for (int i = 0; i < n1; i++) sat_map_walk_add(&w, i, (int32_t)map[i]);
    return sat_map_walk_kind(&w);
}

// cutoff_row, then the baseline's p-value, then - only where both pass, and only when some kind is excluded - the map
__device__ __forceinline__ bool reorder_row(const int32_t *scores, int n, int bpq, const int32_t *orders, const HitQuery *queries,
                                            const double *ztab, const double *ptab, double max_p, ReorderTest test,
                                            const double *base_p, int &q, int &e, int32_t &score)
{
    if (!cutoff_row(scores, n, bpq, orders, queries, ztab, ptab, max_p, q, e, score)) return false;
    if (test.min_base_p > 0.0 && !(base_p[(size_t)q * n + e] >= test.min_base_p)) return false;
    if (test.kinds == SAT_KIND_ALL) return true;
    const int n1 = queries[q].n1;
    sat_map_walk w;
    return (map_order(queries[q].ssemaps + (size_t)e * n1, n1, w) & test.kinds) != 0;      // e < n here
}

// counts[q] += qualifying rows of query q
__global__ void __launch_bounds__(kCutoffBlock) reorder_count(const int32_t *scores, int n, int bpq, const int32_t *orders,
                                                               const HitQuery *queries, const double *ztab, const double *ptab,
                                                               double max_p, ReorderTest test, const double *base_p, int32_t *counts)
{
    int q, e;
    int32_t score = 0;
    const bool hit = reorder_row(scores, n, bpq, orders, queries, ztab, ptab, max_p, test, base_p, q, e, score);
    block_count(hit, [&](int32_t c) { atomicAdd(counts + q, c); });
}

// the qualifying rows' keys into their query's segment seg[q] .. seg[q + 1], in any order (as cutoff_compact of
// sat_topk.hip): each block claims a run of its segment through cursor[q]; the predicate of reorder_count keeps it inside
__global__ void __launch_bounds__(kCutoffBlock) reorder_compact(const int32_t *scores, int n, int bpq, const int32_t *orders,
                                                                 const HitQuery *queries, const double *ztab, const double *ptab,
                                                                 double max_p, ReorderTest test, const double *base_p,
                                                                 const int32_t *seg, int32_t *cursor, unsigned long long *keys)
{
    int q, e;
    int32_t score = 0;
    const bool hit = reorder_row(scores, n, bpq, orders, queries, ztab, ptab, max_p, test, base_p, q, e, score);
    __shared__ int32_t wave_base[kCutoffWaves + 1];                     // each wave's offset in the block's run, the run
    const unsigned long long mask = __ballot(hit);
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    if (lane == 0) wave_base[wave] = (int32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t c = 0;
        for (int w = 0; w < kCutoffWaves; w++) {
            const int32_t v = wave_base[w];
            wave_base[w] = c;
            c += v;
        }
        wave_base[kCutoffWaves] = c ? atomicAdd(cursor + q, c) : 0;
    }
    __syncthreads();
    if (hit) {
        const int slot = seg[q] + wave_base[kCutoffWaves] + wave_base[wave] + (int)__popcll(mask & ((1ull << lane) - 1ull));
        keys[slot] = pair_key(score, (uint32_t)e);
    }
}

// one thread per output row t: query q holds rows out_off[q] .. out_off[q + 1] - 1, its rank r is sorted key seg[q] + r
__global__ void reorder_finish(const unsigned long long *sorted, const int32_t *seg, const int32_t *out_off, int nq, int rows, int n,
                               const int32_t *orders, const HitQuery *queries, const double *ztab, const double *ptab,
                               const int32_t *base_score, const double *base_p, sat_reorder_hit *out, int32_t *maps)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows) return;
    int lo = 0, hi = nq - 1;                                            // the last q with out_off[q] <= t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (out_off[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    const int q = lo, r = t - out_off[q];
    const unsigned long long key = sorted[seg[q] + r];
    const int32_t entry = key_index(key), score = key_score(key);
    const int n1 = queries[q].n1;
    const int8_t *map = queries[q].ssemaps + (size_t)entry * n1;
    const size_t row = (size_t)q * n + entry;
    sat_map_walk w;
    sat_reorder_hit h;
    h.hit = hit_row(entry, score, n1, orders[entry], ztab, ptab, queries[q].fit);
    h.base_pvalue = base_p[row];
    h.base_score = base_score[row];
    h.kind = map_order(map, n1, w);
    h.matched = w.matched;
    h.descents = w.descents;
    h.cut = w.cut;
    h.pad = 0;
    out[t] = h;
    if (maps) row_map(map, n1, maps + (size_t)t * SAT_MAXDIM);
}

// hipCUB's two-phase call (as cub_run of sat_topk.hip): the space in ctx->d_sort_temp, grown behind the stream
template <typename F> int cub_run(sat_ctx *ctx, F run)
{
    size_t temp_bytes = 0;
    HIP_TRY(run(nullptr, temp_bytes));
    SAT_TRY(ctx->d_sort_temp.grow_after(ctx->stream, temp_bytes ? temp_bytes : 1));
    HIP_TRY(run(ctx->d_sort_temp.get(), temp_bytes));
    return SAT_OK;
}

bool has_baseline(const sat_ctx *ctx) { return ctx->baseline_nq != 0 && ctx->d_bl_score.get() && ctx->d_bl_pvalue.get(); }

int check_baseline(const sat_ctx *ctx)
{
    return has_baseline(ctx) ? SAT_OK : sat_fail(SAT_ESTATE, "no baseline kept (sat_baseline_keep has not been called since the last database upload / query change)");
}

}  // namespace

// sat_ctx.hpp: load this file's code object (an empty launch of a small kernel)
int sat_reorder_load_code(sat_ctx *ctx)
{
    hipLaunchKernelGGL(reorder_finish, dim3(1), dim3(64), 0, ctx->stream, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return SAT_OK;
}

// sat_cutoff.hpp: the checks of sat_reorder_hits, nothing else
int sat_reorder_check(sat_ctx *ctx, double max_pvalue, double min_base_pvalue, int kinds, const int32_t *counts)
{
    SAT_TRY(sat_check_searched(ctx));
    SAT_TRY(sat_check_lsoln(ctx->searched_lsoln));
    SAT_TRY(check_baseline(ctx));
    if (ctx->baseline_nq != ctx->queries.size() || ctx->baseline_n != ctx->n_entries)
        return sat_fail(SAT_ESTATE, "the baseline holds %zu x %d rows, the last search %zu x %d", ctx->baseline_nq, ctx->baseline_n,
                        ctx->queries.size(), ctx->n_entries);
    if (!counts) return sat_fail(SAT_EINVAL, "counts buffer is null");
    SAT_TRY(sat_check_pvalue(max_pvalue));
    if (!(std::isfinite(min_base_pvalue) && min_base_pvalue >= 0.0)) return sat_fail(SAT_EINVAL, "min_base_pvalue must be finite and >= 0");
    if (kinds < 1 || kinds > SAT_KIND_ALL) return sat_fail(SAT_EINVAL, "kinds must be 1..%d (got %d)", SAT_KIND_ALL, kinds);
    return SAT_OK;
}

// ---- the two halves of sat_reorder_hits, as sat_cutoff_count / sat_cutoff_rows (sat_cutoff.hpp): ctx->d_seg holds [nq]
// the count pass's counts, then for the chunk at hand its segment offsets [nqc + 1], output offsets [nqc + 1] and claim
// cursors [nqc]

int sat_reorder_count(sat_ctx *ctx, double max_pvalue, double min_base_pvalue, int kinds, int32_t *counts)
{
    const int n = ctx->n_entries, nq = (int)ctx->queries.size(), pc = std::min(sat_cutoff_chunk(ctx, n), nq);
    const ReorderTest test = { min_base_pvalue, kinds };
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(ctx->d_seg.grow((size_t)nq + 3 * (size_t)pc + 2));
    SAT_TRY(sat_hitq_upload(ctx, true));
    const HitQuery *hq = hit_queries(ctx);
    HIP_TRY(hipMemsetAsync(ctx->d_seg.get(), 0, (size_t)nq * sizeof(int32_t), ctx->stream));
    SAT_TRY(sat_row_chunks(ctx, kCutoffBlock, [&](int q0, int, int bpq, dim3 grid) -> int {
        hipLaunchKernelGGL(reorder_count, grid, dim3(kCutoffBlock), 0, ctx->stream, ctx->d_scores.get() + (size_t)q0 * n, n, bpq,
                           ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(), max_pvalue, test,
                           ctx->d_bl_pvalue.get() + (size_t)q0 * n, ctx->d_seg.get() + q0);
        HIP_TRY(hipGetLastError());
        return SAT_OK;
    }));
    SAT_TRY(sat_fetch(ctx, counts, ctx->d_seg.get(), (size_t)nq, true));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SAT_OK;
}

int sat_reorder_rows(sat_ctx *ctx, double max_pvalue, double min_base_pvalue, int kinds, int max_rows, const int32_t *counts,
                     sat_reorder_hit *rows_out, int32_t *ssemaps)
{
    const int n = ctx->n_entries, nq = (int)ctx->queries.size();
    const bool maps = ssemaps != nullptr;
    const ReorderTest test = { min_base_pvalue, kinds };
    // the row buffers hold every query's rows, the key buffers the keys of the largest chunk
    size_t rows_total = 0, keys_max = 0;
    for (int q = 0; q < nq; q++) rows_total += (size_t)sat_row_cap(counts[q], max_rows);
    if (rows_total == 0) return SAT_OK;
    (void)sat_row_chunks(ctx, kCutoffBlock, [&](int q0, int nqc, int, dim3) {
        size_t keys = 0;
        for (int q = q0; q < q0 + nqc; q++) keys += (size_t)counts[q];
        if (keys > keys_max) keys_max = keys;
        return SAT_OK;
    });
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(ctx->d_keys.grow(keys_max));
    SAT_TRY(ctx->d_sorted.grow(keys_max));
    SAT_TRY(ctx->d_reorder_rows.grow(rows_total));
    if (maps) SAT_TRY(ctx->d_hit_maps.grow(rows_total * SAT_MAXDIM));
    const HitQuery *hq = hit_queries(ctx);                                    // as sat_reorder_count left them
    size_t out_row = 0;
    std::vector<int32_t> out_off;
    SAT_TRY(sat_row_chunks(ctx, kCutoffBlock, [&](int q0, int nqc, int bpq, dim3 grid) -> int {
        int32_t *seg = ctx->d_seg.get() + nq, *d_out = seg + nqc + 1, *cursor = d_out + nqc + 1;
        // the chunk's output offsets (each query cut to max_rows); its segment offsets: a scan of its counts
        out_off.assign((size_t)nqc + 1, 0);
        int keys = 0;
        for (int q = 0; q < nqc; q++) {
            keys += counts[q0 + q];
            out_off[(size_t)q + 1] = out_off[(size_t)q] + sat_row_cap(counts[q0 + q], max_rows);
        }
        const int rows = out_off[(size_t)nqc];
        if (rows == 0) return SAT_OK;
        const double *base_p = ctx->d_bl_pvalue.get() + (size_t)q0 * n;
        HIP_TRY(hipMemcpyAsync(d_out, out_off.data(), out_off.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemsetAsync(seg, 0, sizeof(int32_t), ctx->stream));
        HIP_TRY(hipMemsetAsync(cursor, 0, (size_t)nqc * sizeof(int32_t), ctx->stream));
        SAT_TRY(cub_run(ctx, [&](void *temp, size_t &temp_bytes) {
            return hipcub::DeviceScan::InclusiveSum(temp, temp_bytes, ctx->d_seg.get() + q0, seg + 1, nqc, ctx->stream);
        }));
        hipLaunchKernelGGL(reorder_compact, grid, dim3(kCutoffBlock), 0, ctx->stream, ctx->d_scores.get() + (size_t)q0 * n, n, bpq,
                           ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(), max_pvalue, test, base_p, seg,
                           cursor, ctx->d_keys.get());
        HIP_TRY(hipGetLastError());
        const unsigned long long *in = ctx->d_keys.get();
        unsigned long long *sorted = ctx->d_sorted.get();
        SAT_TRY(cub_run(ctx, [&](void *temp, size_t &temp_bytes) {
            if (nqc == 1) return hipcub::DeviceRadixSort::SortKeysDescending(temp, temp_bytes, in, sorted, keys, 0, 64, ctx->stream);
            return hipcub::DeviceSegmentedRadixSort::SortKeysDescending(temp, temp_bytes, in, sorted, keys, nqc, seg, seg + 1, 0, 64,
                                                                        ctx->stream);
        }));
        hipLaunchKernelGGL(reorder_finish, dim3((unsigned)((rows + 127) / 128)), dim3(128), 0, ctx->stream, ctx->d_sorted.get(), seg, d_out,
                           nqc, rows, n, ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(),
                           ctx->d_bl_score.get() + (size_t)q0 * n, base_p, ctx->d_reorder_rows.get() + out_row,
                           maps ? ctx->d_hit_maps.get() + out_row * SAT_MAXDIM : nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));                     // out_off is reused by the next chunk
        out_row += (size_t)rows;
        return SAT_OK;
    }));
    SAT_TRY(sat_fetch(ctx, rows_out, ctx->d_reorder_rows.get(), rows_total));
    if (maps) SAT_TRY(sat_fetch(ctx, ssemaps, ctx->d_hit_maps.get(), rows_total * SAT_MAXDIM));
    return SAT_OK;
}

extern "C" {

int sat_baseline_keep(sat_ctx *ctx)
{
    SAT_TRY(sat_check_searched(ctx));
    const int n = ctx->n_entries, nq = (int)ctx->queries.size(), bpq = (n + kCutoffBlock - 1) / kCutoffBlock;
    const size_t rows = (size_t)nq * n;
    HIP_TRY(hipSetDevice(ctx->device));
    ctx->baseline_nq = 0;                                               // (a failed allocation leaves none)
    SAT_TRY(ctx->d_bl_score.grow_after(ctx->stream, rows));
    SAT_TRY(ctx->d_bl_pvalue.grow_after(ctx->stream, rows));
    const int per = std::min(sat_cutoff_chunk(ctx, n), kBaselineQueries);
    SAT_TRY(sat_query_chunks(nq, per, [&](int q0, int nqc) -> int {
        BaselineQueries bq = {};
        for (int q = 0; q < nqc; q++) {
            bq.n1[q] = (uint8_t)ctx->queries[(size_t)(q0 + q)].n1;
            if (!ctx->fits.empty() && ctx->fits[(size_t)(q0 + q)].fitted) bq.fitted[q >> 5] |= 1u << (q & 31);
        }
        hipLaunchKernelGGL(baseline_keep, dim3((unsigned)nqc * (unsigned)bpq), dim3(kCutoffBlock), 0, ctx->stream,
                           ctx->d_scores.get() + (size_t)q0 * n, n, bpq, ctx->d_orders.get(), bq,
                           ctx->d_fit_tabs.get() ? ctx->d_fit_tabs.get() + (size_t)q0 * 2 * SAT_STAT_BINS : nullptr, ctx->d_gumbel_z.get(),
                           ctx->d_gumbel_p.get(), ctx->d_bl_score.get() + (size_t)q0 * n, ctx->d_bl_pvalue.get() + (size_t)q0 * n);
        HIP_TRY(hipGetLastError());
        return SAT_OK;
    }));
    ctx->baseline_nq = (size_t)nq;
    ctx->baseline_n = n;
    return SAT_OK;
}

int sat_baseline_drop(sat_ctx *ctx)
{
    SAT_TRY(sat_check_context(ctx));
    ctx->baseline_nq = 0;
    return SAT_OK;
}

// include/satabsearch_debug.h
int sat_debug_baseline_shape(sat_ctx *ctx, int n_queries, int n_entries)
{
    SAT_TRY(sat_check_context(ctx));
    SAT_TRY(check_baseline(ctx));
    if (n_queries < 1 || n_entries < 1) return sat_fail(SAT_EINVAL, "a baseline has at least one row");
    ctx->baseline_nq = (size_t)n_queries;
    ctx->baseline_n = n_entries;
    return SAT_OK;
}

int sat_baseline_results(sat_ctx *ctx, int32_t *scores, double *pvalues)
{
    SAT_TRY(sat_check_context(ctx));
    SAT_TRY(check_baseline(ctx));
    const size_t rows = ctx->baseline_nq * (size_t)ctx->baseline_n;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (scores) SAT_TRY(sat_fetch(ctx, scores, ctx->d_bl_score.get(), rows));
    if (pvalues) SAT_TRY(sat_fetch(ctx, pvalues, ctx->d_bl_pvalue.get(), rows));
    return SAT_OK;
}

int sat_reorder_hits(sat_ctx *ctx, double max_pvalue, double min_base_pvalue, int kinds, int max_rows, int32_t *counts,
                     int capacity, sat_reorder_hit *rows, int32_t *ssemaps)
{
    SAT_TRY(sat_check_context(ctx));
    SAT_TRY(sat_reorder_check(ctx, max_pvalue, min_base_pvalue, kinds, counts));
    const int nq = (int)ctx->queries.size();
    std::vector<int32_t> raw((size_t)nq);
    SAT_TRY(sat_reorder_count(ctx, max_pvalue, min_base_pvalue, kinds, raw.data()));
    size_t total = 0;
    for (int q = 0; q < nq; q++) total += (size_t)(counts[q] = sat_row_cap(raw[(size_t)q], max_rows));
    if (total > (size_t)INT_MAX) return sat_fail(SAT_EINVAL, "%zu rows qualify: more than one call can return", total);
    if (!rows || (long long)total > (long long)capacity) return (int)total;
    SAT_TRY(sat_reorder_rows(ctx, max_pvalue, min_base_pvalue, kinds, max_rows, raw.data(), rows, ssemaps));
    return (int)total;
}

int sat_search_reordered(sat_ctx *ctx, int maxstart, double censor, double *kernel_ms)
{
    SAT_TRY(sat_check_context(ctx));
    const bool fit = censor >= 0.0;
    if (fit) SAT_TRY(sat_check_censor(censor));
    double ms[2] = { 0.0, 0.0 };
    for (int pass = 0; pass < 2; pass++) {
        const int lorder = pass == 0, lsoln = pass == 1;            // the ordered search is the baseline
        SAT_TRY(timed(ctx, &ms[pass], [&] {
            return ctx->polish_all ? sat_polish_all_launch(ctx, lorder, lsoln, maxstart) : launch_search(ctx, lorder, lsoln, maxstart, ctx->stream);
        }));
        if (ctx->polish_all) SAT_TRY(sat_polish_all_check(ctx));
        if (fit) SAT_TRY(sat_stats_fit(ctx, censor, nullptr));      // each search fitted to its own scores
        if (pass == 0) SAT_TRY(sat_baseline_keep(ctx));
    }
    if (kernel_ms) *kernel_ms = ms[0] + ms[1];
    return SAT_OK;
}

}  // extern "C"
