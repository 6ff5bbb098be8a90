// sat_topk.hip - best-k hits of a finished search, selected, ranked and given their statistics
// on the device, so that only k rows per query leave the GPU.
//
// Users of the reference sort the full "name score norm2 z p" listing by raw score and keep the
// head (README_example_usage.txt:100, 256: `sort -k 2,2nr | head`).  Here: one pass packs every
// (score, entry index) of the query batch into 64-bit keys, one segmented radix sort (rocPRIM
// through hipCUB; one segment per query) orders them, and a last kernel turns the first k keys of
// each segment into rows {entry, score, norm2, z, p} (gumbelstats.c:50-94 via csrc/host/sat_gumbel.c)
// and gathers their solution maps when the search ran with LSOLN.  Ties keep database order.
//
// The statistics are bit-identical to the host's: norm2 = 2 * score / (n1 + n2) is one IEEE double
// division on either side, and z and p, which the reference computes from norm2 TRUNCATED TO AN
// INT (gumbelstats.h:26 vs cudaSaTabsearch.cu:446), are looked up in a 256-entry table the host
// fills with its own libm when the context is created - no device exp().
//
// All scratch (keys, sort space, rows) belongs to the context and only ever grows.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "sat_pairs.hpp"
#include "sat_cutoff.hpp"
#include "sat_hitrow.hpp"               // HitQuery, hit_row, cutoff_row: shared with sat_cluster.hip
#include "host/sat_gumbel.h"

namespace {

// key = biased score in the high word, inverted entry index in the low word: a descending
// sort lists higher scores first and, among equal scores, lower entry indices first (pair_key, spelled out here: through
// the helper this kernel compiles to other instructions, and its code stays what it was)
__global__ void pack_keys(const int32_t *scores, long long total, int n, unsigned long long *keys)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const uint32_t e = (uint32_t)(i % n);
        keys[i] = ((unsigned long long)(uint32_t)(scores[i] + 0x40000000) << 32) | (0xFFFFFFFFu - e);
    }
}

// one thread per (query, rank): decode the key, look the statistics up, gather the map
__global__ void finish_hits(const unsigned long long *sorted, int n, int k, int nq, const int32_t *orders,
                            const HitQuery *queries, const double *ztab, const double *ptab,
                            sat_hit *hits, int32_t *maps)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq * k) return;
    const int q = t / k, r = t - q * k;
    const unsigned long long key = sorted[(size_t)q * n + r];
    const int32_t entry = key_index(key), score = key_score(key);
    const int n1 = queries[q].n1, n2 = orders[entry];
    hits[t] = hit_row(entry, score, n1, n2, ztab, ptab, queries[q].fit);
    if (maps) {
        int32_t *out = maps + (size_t)t * SAT_MAXDIM;
        const int8_t *src = queries[q].ssemaps ? queries[q].ssemaps + (size_t)entry * n1 : nullptr;
        for (int i = 0; i < SAT_MAXDIM; i++) out[i] = (src && i < n1) ? (int32_t)src[i] : -1;
    }
}

// The HitQuery rows of queries [q0, q0 + nq) into ctx->d_hitq (maps: their solution maps of the last search; the fitted
// tables of the queries that have a fit), queued
// on the context's stream from `hq`, which the caller keeps until the stream has passed the copy.
int upload_hit_queries(sat_ctx *ctx, int q0, int nq, bool maps, std::vector<HitQuery> &hq)
{
    const int rc = ctx->d_hitq.grow((size_t)nq * sizeof(HitQuery));
    if (rc != SAT_OK) return rc;
    hq.resize((size_t)nq);
    for (int q = 0; q < nq; q++) {
        const auto &info = ctx->queries[(size_t)(q0 + q)];
        hq[(size_t)q].n1 = info.n1;
        const bool fitted = !ctx->fits.empty() && ctx->fits[(size_t)(q0 + q)].fitted;
        hq[(size_t)q].fitted = fitted ? 1 : 0;
        hq[(size_t)q].ssemaps = maps ? ctx->d_ssemaps.get() + info.ssemap_off : nullptr;
        hq[(size_t)q].fit = fitted ? ctx->d_fit_tabs.get() + (size_t)(q0 + q) * 2 * SAT_STAT_BINS : nullptr;
    }
    HIP_TRY(hipMemcpyAsync(ctx->d_hitq.get(), hq.data(), hq.size() * sizeof(HitQuery), hipMemcpyHostToDevice, ctx->stream));
    return SAT_OK;
}

const HitQuery *hit_queries(const sat_ctx *ctx) { return reinterpret_cast<const HitQuery *>(ctx->d_hitq.get()); }

// n keys sorted descending from `in` to `out` on `stream`: one segment, or nseg segments seg[s] .. seg[s + 1] - 1 (a
// device array).  temp = null: only sets temp_bytes to the space the sort needs (hipcub's two-phase call).
hipError_t sort_keys_desc(void *temp, size_t &temp_bytes, const unsigned long long *in, unsigned long long *out, int n, int nseg,
                          int *seg, hipStream_t stream)
{
    if (nseg == 1) return hipcub::DeviceRadixSort::SortKeysDescending(temp, temp_bytes, in, out, n, 0, 64, stream);
    return hipcub::DeviceSegmentedRadixSort::SortKeysDescending(temp, temp_bytes, in, out, n, nseg, seg, seg + 1, 0, 64, stream);
}

// rank queries [q0, q0 + nq) of the last search; rows land at row `out_row` of ctx->d_hits (and
// ctx->d_hit_maps), which hold `rows_total` rows
int select_hits(sat_ctx *ctx, int q0, int nq, int k, bool want_maps, size_t out_row, size_t rows_total)
{
    const int n = ctx->n_entries;
    const size_t total = (size_t)nq * n;
    HIP_TRY(hipSetDevice(ctx->device));
    int rc;
    if ((rc = ctx->d_keys.grow(total)) != SAT_OK) return rc;
    if ((rc = ctx->d_sorted.grow(total)) != SAT_OK) return rc;
    if (out_row == 0) {                                   // first chunk: size the row buffers for the whole batch
        if ((rc = ctx->d_hits.grow(rows_total)) != SAT_OK) return rc;
        if (want_maps && (rc = ctx->d_hit_maps.grow(rows_total * SAT_MAXDIM)) != SAT_OK) return rc;
    }
    if ((rc = ctx->d_seg.grow((size_t)nq + 1)) != SAT_OK) return rc;

    std::vector<int> seg((size_t)nq + 1);
    std::vector<HitQuery> hq;
    for (int q = 0; q <= nq; q++) seg[(size_t)q] = q * n;            // nq * n < 2^31: the callers cut the batch
    HIP_TRY(hipMemcpyAsync(ctx->d_seg.get(), seg.data(), seg.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = upload_hit_queries(ctx, q0, nq, want_maps, hq)) != SAT_OK) return rc;

    const int32_t *scores = ctx->d_scores.get() + (size_t)q0 * n;
    hipLaunchKernelGGL(pack_keys, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, scores, (long long)total, n,
                       ctx->d_keys.get());
    HIP_TRY(hipGetLastError());
    size_t temp_bytes = 0;
    HIP_TRY(sort_keys_desc(nullptr, temp_bytes, ctx->d_keys.get(), ctx->d_sorted.get(), (int)total, nq, ctx->d_seg.get(), ctx->stream));
    if ((rc = ctx->d_sort_temp.grow(temp_bytes ? temp_bytes : 1)) != SAT_OK) return rc;
    HIP_TRY(sort_keys_desc(ctx->d_sort_temp.get(), temp_bytes, ctx->d_keys.get(), ctx->d_sorted.get(), (int)total, nq, ctx->d_seg.get(),
                           ctx->stream));
    hipLaunchKernelGGL(finish_hits, dim3((unsigned)((nq * k + 127) / 128)), dim3(128), 0, ctx->stream, ctx->d_sorted.get(), n, k, nq,
                       ctx->d_orders.get(), hit_queries(ctx), ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(), ctx->d_hits.get() + out_row,
                       want_maps ? ctx->d_hit_maps.get() + out_row * SAT_MAXDIM : nullptr);
    HIP_TRY(hipGetLastError());
    // the host vectors die at return
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SAT_OK;
}

// every query of the last search ranked: its best k rows at row q * k of ctx->d_hits (and ctx->d_hit_maps).  One
// segmented sort handles up to 2^31 - 1 keys (ctx->tune.select_keys): long query lists over large databases go in chunks.
int select_all_hits(sat_ctx *ctx, int k, bool want_maps)
{
    const int nq = (int)ctx->queries.size(), n = ctx->n_entries;
    const int per_chunk = (int)(ctx->tune.select_keys / n) < 1 ? 1 : (int)(ctx->tune.select_keys / n);
    for (int q0 = 0; q0 < nq; q0 += per_chunk) {
        const int nqc = nq - q0 < per_chunk ? nq - q0 : per_chunk;
        const int rc = select_hits(ctx, q0, nqc, k, want_maps, (size_t)q0 * k, (size_t)nq * k);
        if (rc != SAT_OK) return rc;
    }
    return SAT_OK;
}

// refine: pair p = q * C + c is candidate c of query q (stage-1 row p of ctx->d_hits); its final key is the
// stage-2 score over the inverted entry index, as pack_keys builds them, its value the pair
__global__ void pack_refined(const unsigned long long *pkeys, const sat_hit *cand, int npairs, unsigned long long *keys, int32_t *vals)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npairs) return;
    keys[p] = pair_key(key_score(pkeys[p]), (uint32_t)cand[p].entry);
    vals[p] = p;
}

// one thread per (query, rank) of the refined rows: the statistics of the stage-2 score, the stage-1 score and map
__global__ void finish_refined(const unsigned long long *sorted, const int32_t *vals, int c, int k, int nq, const int32_t *orders,
                               const HitQuery *queries, const double *ztab, const double *ptab, const sat_hit *cand,
                               const int8_t *pmaps, sat_hit *hits, int32_t *first, int32_t *maps, const int32_t *pbase,
                               int32_t *base)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq * k) return;
    const int q = t / k, r = t - q * k;
    const unsigned long long key = sorted[(size_t)q * c + r];
    const int p = vals[(size_t)q * c + r];
    const int32_t entry = key_index(key), score = key_score(key);
    const int n1 = queries[q].n1;
    hits[t] = hit_row(entry, score, n1, orders[entry], ztab, ptab, queries[q].fit);
    first[t] = cand[p].score;
    if (base) base[t] = pbase[p];                        // polish: the pair's score before it
    if (maps) {
        int32_t *out = maps + (size_t)t * SAT_MAXDIM;
        const int8_t *src = pmaps + (size_t)p * SAT_MAXDIM;
        for (int i = 0; i < SAT_MAXDIM; i++) out[i] = i < n1 ? (int32_t)src[i] : -1;
    }
}

int check_searched(sat_ctx *ctx)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (ctx->n_entries <= 0 || ctx->queries.empty() || !ctx->d_scores.get() || ctx->searched_nq != ctx->queries.size())
        return sat_fail(SAT_ESTATE, "no search has run since the last database upload / query change");
    return SAT_OK;
}

// ---- p-value cutoff (sat_hits_cutoff).  Blocks of 1024 rows, `bpq` blocks per query, so that a block holds rows of
// one query only: each wave counts its qualifying rows with a ballot, the block sums its 16 waves' counts in LDS and
// counts (or claims) them with ONE atomic.  (Every query's counter sits in a few cache lines: at P = 1 one atomic per
// wave took 170 us of the q200 shape's flag pass)  A row qualifies iff the p-value hit_row gives it is
// <= max_p: the same double, from the same table index (cutoff_row, sat_hitrow.hpp).

// counts[q] += qualifying rows of query q
__global__ void __launch_bounds__(kCutoffBlock) cutoff_count(const int32_t *scores, int n, int bpq, const int32_t *orders,
                                                              const HitQuery *queries, const double *ztab, const double *ptab,
                                                              double max_p, int32_t *counts)
{
    int q, e;
    int32_t score = 0;
    const bool hit = cutoff_row(scores, n, bpq, orders, queries, ztab, ptab, max_p, q, e, score);
    __shared__ int32_t wave_count[kCutoffWaves];
    const unsigned long long mask = __ballot(hit);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = (int32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t c = 0;
        for (int w = 0; w < kCutoffWaves; w++) c += wave_count[w];
        if (c) atomicAdd(counts + q, c);
    }
}

// the qualifying rows' keys (pack_keys' layout) into their query's segment seg[q] .. seg[q + 1], in any order: each
// block claims a run of its segment through cursor[q], the same predicate as cutoff_count keeps it inside
__global__ void __launch_bounds__(kCutoffBlock) cutoff_compact(const int32_t *scores, int n, int bpq, const int32_t *orders,
                                                                const HitQuery *queries, const double *ztab, const double *ptab,
                                                                double max_p, const int32_t *seg, int32_t *cursor,
                                                                unsigned long long *keys)
{
    int q, e;
    int32_t score = 0;
    const bool hit = cutoff_row(scores, n, bpq, orders, queries, ztab, ptab, max_p, q, e, score);
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
__global__ void cutoff_finish(const unsigned long long *sorted, const int32_t *seg, const int32_t *out_off, int nq, int rows,
                              const int32_t *orders, const HitQuery *queries, const double *ztab, const double *ptab,
                              sat_hit *hits, int32_t *maps)
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
    hits[t] = hit_row(entry, score, n1, orders[entry], ztab, ptab, queries[q].fit);
    if (maps) {
        int32_t *out = maps + (size_t)t * SAT_MAXDIM;
        const int8_t *src = queries[q].ssemaps ? queries[q].ssemaps + (size_t)entry * n1 : nullptr;
        for (int i = 0; i < SAT_MAXDIM; i++) out[i] = (src && i < n1) ? (int32_t)src[i] : -1;
    }
}


// ---- score histogram (sat_score_histogram).  Blocks of kHistRows rows, `bpq` blocks per query, so that a block holds
// rows of one query only (as the cutoff kernels): the block counts its rows in a 16 KB LDS histogram with LDS integer
// atomics, then adds its NON-ZERO bins to counts[q][bin] with global integer atomics - a query's scores crowd into a
// few hundred bins, so a block of several thousand rows flushes a few hundred atomics.  Negative scores are summed
// with a ballot per pass and one atomic per block.  Integers only: the result does not depend on the launch shape.
constexpr int kHistBlock = 1024, kHistWaves = kHistBlock / 64, kHistPasses = 8, kHistRows = kHistBlock * kHistPasses;

__global__ void __launch_bounds__(kHistBlock) score_histogram(const int32_t *scores, int n, int bpq, const int32_t *orders,
                                                              const HitQuery *queries, uint32_t *counts, int32_t *below)
{
    __shared__ uint32_t hist[SAT_STAT_BINS];
    __shared__ int32_t wave_below[kHistWaves];
    const int q = (int)(blockIdx.x / (unsigned)bpq);
    const int e0 = (int)(blockIdx.x - (unsigned)q * bpq) * kHistRows;
    const int n1 = queries[q].n1;
    for (int k = (int)threadIdx.x; k < SAT_STAT_BINS; k += kHistBlock) hist[k] = 0u;
    __syncthreads();
    int32_t neg = 0;                                                    // (meaningful in lane 0 of each wave)
    for (int pass = 0; pass < kHistPasses; pass++) {
        const int e = e0 + pass * kHistBlock + (int)threadIdx.x;        // e0 + kHistRows <= n + kHistRows: no overflow, n < 2^31 - 2^13
        bool is_neg = false;
        if (e < n) {
            const int32_t score = scores[(size_t)q * n + e];
            is_neg = score < 0;
            if (!is_neg) atomicAdd(&hist[sat_stat_bin_of(score, n1 + orders[e])], 1u);
        }
        neg += (int32_t)__popcll(__ballot(is_neg));
    }
    if ((threadIdx.x & 63) == 0) wave_below[threadIdx.x >> 6] = neg;
    __syncthreads();
    uint32_t *out = counts + (size_t)q * SAT_STAT_BINS;
    for (int k = (int)threadIdx.x; k < SAT_STAT_BINS; k += kHistBlock) {
        const uint32_t c = hist[k];
        if (c) atomicAdd(out + k, c);
    }
    if (threadIdx.x == 0) {
        int32_t c = 0;
        for (int w = 0; w < kHistWaves; w++) c += wave_below[w];
        if (c) atomicAdd(below + q, c);
    }
}

// queries per chunk: under 2^31 keys per sort (as sat_topk_hits) and under 2^31 threads per launch - or under
// ctx->tune.select_keys of either
int cutoff_chunk(const sat_ctx *ctx, int n)
{
    const long long bpq = (n + kCutoffBlock - 1) / kCutoffBlock, keys = ctx->tune.select_keys;
    long long per = keys / n;
    if (keys / (bpq * kCutoffBlock) < per) per = keys / (bpq * kCutoffBlock);
    return per < 1 ? 1 : (int)per;
}

}  // namespace

// sat_cutoff.hpp, for sat_cluster.hip: the searched-state check, the chunking and the HitQuery rows of the cutoff pass
int sat_check_searched(sat_ctx *ctx) { return check_searched(ctx); }
int sat_cutoff_chunk(const sat_ctx *ctx, int n) { return cutoff_chunk(ctx, n); }
int sat_hitq_upload(sat_ctx *ctx)
{
    std::vector<HitQuery> hq_host;
    const int rc = upload_hit_queries(ctx, 0, (int)ctx->queries.size(), false, hq_host);
    if (rc != SAT_OK) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // hq_host dies at return
    return SAT_OK;
}

// The histogram of every query of the last search into ctx->d_hist (counts [nq][SAT_STAT_BINS], then below [nq]) and
// from there to the host.  The query lists go in cutoff_chunk's chunks: fewer blocks per query here, so a chunk that
// fits the cutoff kernels' grid fits this one.
extern "C" int sat_score_histogram(sat_ctx *ctx, uint32_t *counts, int32_t *below)
{
    int rc = check_searched(ctx);
    if (rc != SAT_OK) return rc;
    if (!counts || !below) return sat_fail(SAT_EINVAL, "histogram buffer is null");
    const int n = ctx->n_entries, nq = (int)ctx->queries.size();
    if (n > 0x7FFFFFFF - kHistRows) return sat_fail(SAT_EINVAL, "too many entries for the histogram pass");
    const int per_chunk = cutoff_chunk(ctx, n);
    const int bpq = (n + kHistRows - 1) / kHistRows;
    const size_t words = (size_t)nq * (SAT_STAT_BINS + 1);
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = ctx->d_hist.grow(words)) != SAT_OK) return rc;
    std::vector<HitQuery> hq_host;
    if ((rc = upload_hit_queries(ctx, 0, nq, false, hq_host)) != SAT_OK) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // hq_host dies at return
    const HitQuery *hq = hit_queries(ctx);
    uint32_t *d_counts = ctx->d_hist.get();
    int32_t *d_below = reinterpret_cast<int32_t *>(d_counts + (size_t)nq * SAT_STAT_BINS);
    HIP_TRY(hipMemsetAsync(d_counts, 0, words * sizeof(uint32_t), ctx->stream));
    for (int q0 = 0; q0 < nq; q0 += per_chunk) {
        const int nqc = nq - q0 < per_chunk ? nq - q0 : per_chunk;
        hipLaunchKernelGGL(score_histogram, dim3((unsigned)nqc * (unsigned)bpq), dim3(kHistBlock), 0, ctx->stream,
                           ctx->d_scores.get() + (size_t)q0 * n, n, bpq, ctx->d_orders.get(), hq + q0,
                           d_counts + (size_t)q0 * SAT_STAT_BINS, d_below + q0);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(counts, d_counts, (size_t)nq * SAT_STAT_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(below, d_below, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->d2h_bytes += words * sizeof(uint32_t);
    return SAT_OK;
}

extern "C" int sat_stats_set(sat_ctx *ctx, const sat_fit *fits)
{
    int rc = check_searched(ctx);
    if (rc != SAT_OK) return rc;
    ctx->fits.clear();
    if (!fits) return SAT_OK;
    const size_t nq = ctx->queries.size();
    bool any = false;
    for (size_t q = 0; q < nq; q++) {
        if (!fits[q].fitted) continue;
        if (!std::isfinite(fits[q].a) || !std::isfinite(fits[q].b) || !(fits[q].b > 0.0))
            return sat_fail(SAT_EINVAL, "query %zu: fitted parameters a = %g, b = %g are not usable", q, fits[q].a, fits[q].b);
        any = true;
    }
    if (any) {
        HIP_TRY(hipSetDevice(ctx->device));
        // (rows selected earlier may still be read through the old tables on the stream)
        if ((rc = ctx->d_fit_tabs.grow_after(ctx->stream, nq * 2 * SAT_STAT_BINS)) != SAT_OK) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        std::vector<double> tab(2 * SAT_STAT_BINS);
        for (size_t q = 0; q < nq; q++) {
            if (!fits[q].fitted) continue;
            sat_gumbel_fit_table(fits[q].a, fits[q].b, tab.data(), tab.data() + SAT_STAT_BINS);    // the host's libm
            HIP_TRY(hipMemcpy(ctx->d_fit_tabs.get() + q * 2 * SAT_STAT_BINS, tab.data(), tab.size() * sizeof(double),
                              hipMemcpyHostToDevice));
        }
    }
    ctx->fits.assign(fits, fits + nq);
    return SAT_OK;
}

extern "C" int sat_stats_fit(sat_ctx *ctx, double censor, sat_fit *fits)
{
    int rc = check_searched(ctx);
    if (rc != SAT_OK) return rc;
    if (!(censor >= 0.0 && censor <= 0.5)) return sat_fail(SAT_EINVAL, "censor must lie in [0, 0.5]");
    const size_t nq = ctx->queries.size();
    std::vector<uint32_t> counts(nq * SAT_STAT_BINS);
    std::vector<int32_t> below(nq);
    if ((rc = sat_score_histogram(ctx, counts.data(), below.data())) != SAT_OK) return rc;
    std::vector<sat_fit> fit(nq);
    for (size_t q = 0; q < nq; q++) {
        if (sat_gumbel_fit_binned(counts.data() + q * SAT_STAT_BINS, censor, &fit[q]) != 0)
            return sat_fail(SAT_EINVAL, "censor must lie in [0, 0.5]");
        fit[q].below = below[q];
    }
    if ((rc = sat_stats_set(ctx, fit.data())) != SAT_OK) return rc;
    if (fits) std::copy(fit.begin(), fit.end(), fits);
    return SAT_OK;
}

extern "C" int sat_debug_set_scores(sat_ctx *ctx, const int32_t *scores)
{
    int rc = check_searched(ctx);
    if (rc != SAT_OK) return rc;
    if (!scores) return sat_fail(SAT_EINVAL, "scores buffer is null");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(ctx->d_scores.get(), scores, ctx->queries.size() * (size_t)ctx->n_entries * sizeof(int32_t), hipMemcpyHostToDevice));
    ctx->fits.clear();
    return SAT_OK;
}

extern "C" int sat_topk(sat_ctx *ctx, int query, int k, int32_t *entry_index, int32_t *scores_out)
{
    int rc = check_searched(ctx);
    if (rc != SAT_OK) return rc;
    if (!entry_index || !scores_out || k < 1) return sat_fail(SAT_EINVAL, "bad top-k arguments");
    if (query < 0 || query >= (int)ctx->queries.size()) return sat_fail(SAT_EINVAL, "query %d out of range", query);
    if (k > ctx->n_entries) k = ctx->n_entries;
    if ((rc = select_hits(ctx, query, 1, k, false, 0, (size_t)k)) != SAT_OK) return rc;
    std::vector<sat_hit> rows((size_t)k);
    HIP_TRY(hipMemcpy(rows.data(), ctx->d_hits.get(), rows.size() * sizeof(sat_hit), hipMemcpyDeviceToHost));
    ctx->d2h_bytes += rows.size() * sizeof(sat_hit);
    for (int i = 0; i < k; i++) {
        entry_index[i] = rows[(size_t)i].entry;
        scores_out[i] = rows[(size_t)i].score;
    }
    return k;
}

extern "C" int sat_topk_hits(sat_ctx *ctx, int k, sat_hit *hits, int32_t *ssemaps)
{
    int rc = check_searched(ctx);
    if (rc != SAT_OK) return rc;
    if (!hits || k < 1) return sat_fail(SAT_EINVAL, "bad top-k arguments");
    if (ssemaps && !ctx->searched_lsoln) return sat_fail(SAT_ESTATE, "the last search ran without lsoln");
    if (k > ctx->n_entries) k = ctx->n_entries;
    const int nq = (int)ctx->queries.size();
    if ((rc = select_all_hits(ctx, k, ssemaps != nullptr)) != SAT_OK) return rc;
    HIP_TRY(hipMemcpy(hits, ctx->d_hits.get(), (size_t)nq * k * sizeof(sat_hit), hipMemcpyDeviceToHost));
    ctx->d2h_bytes += (size_t)nq * k * sizeof(sat_hit);
    if (ssemaps) {
        HIP_TRY(hipMemcpy(ssemaps, ctx->d_hit_maps.get(), (size_t)nq * k * SAT_MAXDIM * sizeof(int32_t), hipMemcpyDeviceToHost));
        ctx->d2h_bytes += (size_t)nq * k * SAT_MAXDIM * sizeof(int32_t);
    }
    return k;
}

// sat_search_refine (tops = 0) and sat_search_refine_polish (tops = maps polished per candidate): the stage-2 keys and
// maps come from the pair search or from the polish (sat_polish.hip), everything around them is shared
static int refine(sat_ctx *ctx, int lorder, int lsoln, int maxstart, int candidates, int refine_maxstart, int tops,
                  int k, sat_hit *hits, int32_t *ssemaps, int32_t *first_scores, int32_t *base_scores)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (!hits || k < 1) return sat_fail(SAT_EINVAL, "bad top-k arguments");
    if (candidates < 1) return sat_fail(SAT_EINVAL, "candidates must be >= 1 (got %d)", candidates);
    if (refine_maxstart < 1) return sat_fail(SAT_EINVAL, "refine_maxstart must be >= 1 (got %d)", refine_maxstart);
    if (k > candidates) return sat_fail(SAT_EINVAL, "k (%d) exceeds the candidates per query (%d)", k, candidates);
    HIP_TRY(hipSetDevice(ctx->device));
    // stage 1: the plain search at maxstart, without LSOLN
    int rc = launch_search(ctx, lorder, 0, maxstart, ctx->stream);
    if (rc != SAT_OK) return rc;
    const std::string stage1_info = ctx->last_launch_info;
    const int n = ctx->n_entries, nq = (int)ctx->queries.size();
    const int c = candidates < n ? candidates : n;
    if (k > c) k = c;
    if ((long long)nq * c > 0x7FFFFFFFll) return sat_fail(SAT_EINVAL, "queries x candidates exceed 2^31 - 1");
    const int npairs = nq * c;
    // the best c entries of every query, ranked on the device (rows stay there); only their indices come back
    if ((rc = select_all_hits(ctx, c, false)) != SAT_OK) return rc;
    std::vector<int32_t> query((size_t)npairs), entry((size_t)npairs);
    HIP_TRY(hipMemcpy2D(entry.data(), sizeof(int32_t), ctx->d_hits.get(), sizeof(sat_hit), sizeof(int32_t), (size_t)npairs,
                        hipMemcpyDeviceToHost));
    ctx->d2h_bytes += (size_t)npairs * sizeof(int32_t);
    for (int p = 0; p < npairs; p++) query[(size_t)p] = p / c;
    // stage 2: the candidates at refine_maxstart (and their maps)
    const bool maps = lsoln && ssemaps;
    rc = tops ? sat_pair_matches_launch(ctx, lorder, refine_maxstart, tops, true, query.data(), entry.data(), npairs, PairMode::Polish)
              : sat_pairs_launch(ctx, lorder, refine_maxstart, maps, query.data(), entry.data(), npairs);
    if (rc != SAT_OK) return rc;
    const unsigned long long *pkeys = tops ? ctx->d_polkeys.get() : ctx->d_pkeys.get();
    const int8_t *pmaps = tops ? ctx->d_polmaps.get() : ctx->d_pmaps.get();
    const std::string stage2_info = ctx->last_launch_info;
    // the final ranking: segments of c keys, one per query
    if ((rc = ctx->d_rkeys.grow((size_t)npairs)) != SAT_OK) return rc;
    if ((rc = ctx->d_rsorted.grow((size_t)npairs)) != SAT_OK) return rc;
    if ((rc = ctx->d_rvals.grow((size_t)npairs)) != SAT_OK) return rc;
    if ((rc = ctx->d_rvals_sorted.grow((size_t)npairs)) != SAT_OK) return rc;
    if ((rc = ctx->d_rhits.grow((size_t)nq * k)) != SAT_OK) return rc;
    if ((rc = ctx->d_rfirst.grow(2 * (size_t)nq * k)) != SAT_OK) return rc;      // stage-1 scores, then (polish) base scores
    if (maps && (rc = ctx->d_rmaps.grow((size_t)nq * k * SAT_MAXDIM)) != SAT_OK) return rc;
    if ((rc = ctx->d_seg.grow((size_t)nq + 1)) != SAT_OK) return rc;
    std::vector<int> seg((size_t)nq + 1);
    std::vector<HitQuery> hq;
    for (int q = 0; q <= nq; q++) seg[(size_t)q] = q * c;
    HIP_TRY(hipMemcpyAsync(ctx->d_seg.get(), seg.data(), seg.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = upload_hit_queries(ctx, 0, nq, false, hq)) != SAT_OK) return rc;
    hipLaunchKernelGGL(pack_refined, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, ctx->stream, pkeys, ctx->d_hits.get(),
                       npairs, ctx->d_rkeys.get(), ctx->d_rvals.get());
    HIP_TRY(hipGetLastError());
    size_t temp_bytes = 0;
    HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairsDescending(nullptr, temp_bytes, ctx->d_rkeys.get(), ctx->d_rsorted.get(),
                                                                 ctx->d_rvals.get(), ctx->d_rvals_sorted.get(), npairs, nq,
                                                                 ctx->d_seg.get(), ctx->d_seg.get() + 1, 0, 64, ctx->stream));
    if ((rc = ctx->d_sort_temp.grow(temp_bytes ? temp_bytes : 1)) != SAT_OK) return rc;
    HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairsDescending(ctx->d_sort_temp.get(), temp_bytes, ctx->d_rkeys.get(),
                                                                 ctx->d_rsorted.get(), ctx->d_rvals.get(), ctx->d_rvals_sorted.get(),
                                                                 npairs, nq, ctx->d_seg.get(), ctx->d_seg.get() + 1, 0, 64, ctx->stream));
    hipLaunchKernelGGL(finish_refined, dim3((unsigned)((nq * k + 127) / 128)), dim3(128), 0, ctx->stream, ctx->d_rsorted.get(),
                       ctx->d_rvals_sorted.get(), c, k, nq, ctx->d_orders.get(), hit_queries(ctx), ctx->d_gumbel_z.get(),
                       ctx->d_gumbel_p.get(), ctx->d_hits.get(), pmaps, ctx->d_rhits.get(), ctx->d_rfirst.get(),
                       maps ? ctx->d_rmaps.get() : nullptr, tops ? (const int32_t *)ctx->d_polout.get() + npairs : nullptr,
                       tops ? ctx->d_rfirst.get() + (size_t)nq * k : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t rows = (size_t)nq * k;
    if (tops) {
        // a pair whose polish did not finish carries moves = -1 (sat_polish.hip): one flag row, npairs ints
        std::vector<int32_t> mv((size_t)npairs);
        HIP_TRY(hipMemcpy(mv.data(), ctx->d_polout.get() + 3 * (size_t)npairs, mv.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        ctx->d2h_bytes += mv.size() * sizeof(int32_t);
        for (int p = 0; p < npairs; p++)
            if (mv[(size_t)p] < 0) return sat_fail(SAT_EDEVICE, "pair %d: the polish did not finish", p);
        if (base_scores) {
            HIP_TRY(hipMemcpy(base_scores, ctx->d_rfirst.get() + rows, rows * sizeof(int32_t), hipMemcpyDeviceToHost));
            ctx->d2h_bytes += rows * sizeof(int32_t);
        }
    }
    HIP_TRY(hipMemcpy(hits, ctx->d_rhits.get(), rows * sizeof(sat_hit), hipMemcpyDeviceToHost));
    ctx->d2h_bytes += rows * sizeof(sat_hit);
    if (first_scores) {
        HIP_TRY(hipMemcpy(first_scores, ctx->d_rfirst.get(), rows * sizeof(int32_t), hipMemcpyDeviceToHost));
        ctx->d2h_bytes += rows * sizeof(int32_t);
    }
    if (maps) {
        HIP_TRY(hipMemcpy(ssemaps, ctx->d_rmaps.get(), rows * SAT_MAXDIM * sizeof(int32_t), hipMemcpyDeviceToHost));
        ctx->d2h_bytes += rows * SAT_MAXDIM * sizeof(int32_t);
    }
    ctx->last_launch_info = "stage 1: " + stage1_info + " || stage 2: " + stage2_info;
    return k;
}

extern "C" int sat_search_refine(sat_ctx *ctx, int lorder, int lsoln, int maxstart, int candidates, int refine_maxstart,
                                 int k, sat_hit *hits, int32_t *ssemaps, int32_t *first_scores)
{
    return refine(ctx, lorder, lsoln, maxstart, candidates, refine_maxstart, 0, k, hits, ssemaps, first_scores, nullptr);
}

extern "C" int sat_search_refine_polish(sat_ctx *ctx, int lorder, int lsoln, int maxstart, int candidates, int refine_maxstart,
                                        int tops, int k, sat_hit *hits, int32_t *ssemaps, int32_t *first_scores,
                                        int32_t *base_scores)
{
    if (tops < 1 || tops > SAT_MAX_MATCHES) return sat_fail(SAT_EINVAL, "tops must be 1..%d (got %d)", SAT_MAX_MATCHES, tops);
    return refine(ctx, lorder, lsoln, maxstart, candidates, refine_maxstart, tops, k, hits, ssemaps, first_scores, base_scores);
}

// ---- p-value cutoff.  ctx->d_seg holds, in ints: [nq] the count pass's counts, then for the chunk at hand its
// segment offsets [nqc + 1], its output offsets [nqc + 1] and its claim cursors [nqc].

int sat_cutoff_count(sat_ctx *ctx, double max_pvalue, bool maps, int32_t *counts)
{
    int rc = check_searched(ctx);
    if (rc != SAT_OK) return rc;
    if (maps && !ctx->searched_lsoln) return sat_fail(SAT_ESTATE, "the last search ran without lsoln");
    const int n = ctx->n_entries, nq = (int)ctx->queries.size();
    const int per_chunk = cutoff_chunk(ctx, n), pc = per_chunk < nq ? per_chunk : nq;
    const int bpq = (n + kCutoffBlock - 1) / kCutoffBlock;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = ctx->d_seg.grow((size_t)nq + 3 * (size_t)pc + 2)) != SAT_OK) return rc;
    std::vector<HitQuery> hq_host;
    if ((rc = upload_hit_queries(ctx, 0, nq, maps, hq_host)) != SAT_OK) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // hq_host dies at return
    const HitQuery *hq = hit_queries(ctx);
    HIP_TRY(hipMemsetAsync(ctx->d_seg.get(), 0, (size_t)nq * sizeof(int32_t), ctx->stream));
    for (int q0 = 0; q0 < nq; q0 += per_chunk) {
        const int nqc = nq - q0 < per_chunk ? nq - q0 : per_chunk;
        hipLaunchKernelGGL(cutoff_count, dim3((unsigned)nqc * (unsigned)bpq), dim3(kCutoffBlock), 0, ctx->stream,
                           ctx->d_scores.get() + (size_t)q0 * n, n, bpq, ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(),
                           ctx->d_gumbel_p.get(), max_pvalue, ctx->d_seg.get() + q0);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(counts, ctx->d_seg.get(), (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->d2h_bytes += (size_t)nq * sizeof(int32_t);
    return SAT_OK;
}

int sat_cutoff_rows(sat_ctx *ctx, double max_pvalue, int max_rows, const int32_t *counts, sat_hit *hits, int32_t *ssemaps)
{
    const int n = ctx->n_entries, nq = (int)ctx->queries.size();
    const int per_chunk = cutoff_chunk(ctx, n);
    const int bpq = (n + kCutoffBlock - 1) / kCutoffBlock;
    const bool maps = ssemaps != nullptr;
    size_t rows_total = 0, keys_max = 0;
    for (int q0 = 0; q0 < nq; q0 += per_chunk) {
        const int nqc = nq - q0 < per_chunk ? nq - q0 : per_chunk;
        size_t keys = 0;
        for (int q = q0; q < q0 + nqc; q++) {
            keys += (size_t)counts[q];
            rows_total += (size_t)(max_rows > 0 && counts[q] > max_rows ? max_rows : counts[q]);
        }
        if (keys > keys_max) keys_max = keys;
    }
    if (rows_total == 0) return SAT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    int rc;
    if ((rc = ctx->d_keys.grow(keys_max)) != SAT_OK) return rc;
    if ((rc = ctx->d_sorted.grow(keys_max)) != SAT_OK) return rc;
    if ((rc = ctx->d_hits.grow(rows_total)) != SAT_OK) return rc;
    if (maps && (rc = ctx->d_hit_maps.grow(rows_total * SAT_MAXDIM)) != SAT_OK) return rc;
    const HitQuery *hq = hit_queries(ctx);                                    // as sat_cutoff_count left them
    size_t out_row = 0;
    std::vector<int32_t> out_off;
    for (int q0 = 0; q0 < nq; q0 += per_chunk) {
        const int nqc = nq - q0 < per_chunk ? nq - q0 : per_chunk;
        int32_t *seg = ctx->d_seg.get() + nq, *d_out = seg + nqc + 1, *cursor = d_out + nqc + 1;
        // the chunk's output offsets (each query cut to max_rows); its segment offsets: a scan of its counts
        out_off.assign((size_t)nqc + 1, 0);
        int keys = 0;
        for (int q = 0; q < nqc; q++) {
            const int c = counts[q0 + q];
            keys += c;
            out_off[(size_t)q + 1] = out_off[(size_t)q] + (max_rows > 0 && c > max_rows ? max_rows : c);
        }
        const int rows = out_off[(size_t)nqc];
        if (rows == 0) continue;
        HIP_TRY(hipMemcpyAsync(d_out, out_off.data(), out_off.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemsetAsync(seg, 0, sizeof(int32_t), ctx->stream));
        HIP_TRY(hipMemsetAsync(cursor, 0, (size_t)nqc * sizeof(int32_t), ctx->stream));
        size_t scan_bytes = 0, sort_bytes = 0;
        HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, ctx->d_seg.get() + q0, seg + 1, nqc, ctx->stream));
        HIP_TRY(sort_keys_desc(nullptr, sort_bytes, ctx->d_keys.get(), ctx->d_sorted.get(), keys, nqc, seg, ctx->stream));
        const size_t temp_bytes = scan_bytes > sort_bytes ? scan_bytes : sort_bytes;
        if ((rc = ctx->d_sort_temp.grow(temp_bytes ? temp_bytes : 1)) != SAT_OK) return rc;
        HIP_TRY(hipcub::DeviceScan::InclusiveSum(ctx->d_sort_temp.get(), scan_bytes, ctx->d_seg.get() + q0, seg + 1, nqc, ctx->stream));
        hipLaunchKernelGGL(cutoff_compact, dim3((unsigned)nqc * (unsigned)bpq), dim3(kCutoffBlock), 0, ctx->stream,
                           ctx->d_scores.get() + (size_t)q0 * n, n, bpq, ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(),
                           ctx->d_gumbel_p.get(), max_pvalue, seg, cursor, ctx->d_keys.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(sort_keys_desc(ctx->d_sort_temp.get(), sort_bytes, ctx->d_keys.get(), ctx->d_sorted.get(), keys, nqc, seg, ctx->stream));
        hipLaunchKernelGGL(cutoff_finish, dim3((unsigned)((rows + 127) / 128)), dim3(128), 0, ctx->stream, ctx->d_sorted.get(), seg, d_out,
                           nqc, rows, ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(),
                           ctx->d_hits.get() + out_row, maps ? ctx->d_hit_maps.get() + out_row * SAT_MAXDIM : nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));                     // out_off is reused by the next chunk
        out_row += (size_t)rows;
    }
    HIP_TRY(hipMemcpy(hits, ctx->d_hits.get(), rows_total * sizeof(sat_hit), hipMemcpyDeviceToHost));
    ctx->d2h_bytes += rows_total * sizeof(sat_hit);
    if (maps) {
        HIP_TRY(hipMemcpy(ssemaps, ctx->d_hit_maps.get(), rows_total * SAT_MAXDIM * sizeof(int32_t), hipMemcpyDeviceToHost));
        ctx->d2h_bytes += rows_total * SAT_MAXDIM * sizeof(int32_t);
    }
    return SAT_OK;
}

extern "C" int sat_hits_cutoff(sat_ctx *ctx, double max_pvalue, int max_rows, int32_t *counts, int capacity, sat_hit *hits,
                               int32_t *ssemaps)
{
    int rc = check_searched(ctx);
    if (rc != SAT_OK) return rc;
    if (!counts) return sat_fail(SAT_EINVAL, "counts buffer is null");
    if (!std::isfinite(max_pvalue) || max_pvalue < 0.0) return sat_fail(SAT_EINVAL, "max_pvalue must be finite and >= 0");
    const int nq = (int)ctx->queries.size();
    std::vector<int32_t> raw((size_t)nq);
    if ((rc = sat_cutoff_count(ctx, max_pvalue, ssemaps != nullptr, raw.data())) != SAT_OK) return rc;
    size_t total = 0;
    for (int q = 0; q < nq; q++) {
        counts[q] = max_rows > 0 && raw[(size_t)q] > max_rows ? max_rows : raw[(size_t)q];
        total += (size_t)counts[q];
    }
    if (total > (size_t)INT_MAX) return sat_fail(SAT_EINVAL, "%zu rows qualify: more than one call can return", total);
    if (!hits || (long long)total > (long long)capacity) return (int)total;
    if ((rc = sat_cutoff_rows(ctx, max_pvalue, max_rows, raw.data(), hits, ssemaps)) != SAT_OK) return rc;
    return (int)total;
}
