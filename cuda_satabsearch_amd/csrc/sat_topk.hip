// sat_topk.hip - the rows of a finished search, selected, ranked and given their statistics on the device, so that only
// the rows asked for leave the GPU: best-k (sat_topk, sat_topk_hits), the final ranking of the refine calls, every row
// under a p-value cutoff (sat_hits_cutoff and its two halves), the score histogram and the fit built on it.  One code
// object: the file's kernels and the hipCUB / rocPRIM instantiations they rank with.  What it shares with
// sat_cluster.hip and sat_multi.hip - the argument checks, the chunk walk, the counted copies - is in sat_cutoff.hpp, the
// device code of a row in sat_hitrow.hpp.
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
#include "sat_hitrow.hpp"               // HitQuery, hit_row, row_map, cutoff_row, block_count: shared with sat_cluster.hip
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
    if (maps) row_map(queries[q].ssemaps ? queries[q].ssemaps + (size_t)entry * n1 : nullptr, n1, maps + (size_t)t * SAT_MAXDIM);
}

// The HitQuery rows of queries [q0, q0 + nq) into ctx->d_hitq (maps: their solution maps of the last search; the fitted
// tables of the queries that have a fit), queued on the context's stream from `hq`, which the caller keeps until then.
int upload_hit_queries(sat_ctx *ctx, int q0, int nq, bool maps, std::vector<HitQuery> &hq)
{
    SAT_TRY(ctx->d_hitq.grow((size_t)nq * sizeof(HitQuery)));
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

// What a ranking of queries [q0, q0 + nq) reads from the host: the segment offsets q * stride, q = 0 .. nq, into
// ctx->d_seg (nq * stride < 2^31: the callers cut the batch) and the HitQuery rows, queued like those from `host`.
struct RankInput { std::vector<int> seg; std::vector<HitQuery> hq; };
int upload_rank_input(sat_ctx *ctx, int q0, int nq, int stride, bool maps, RankInput &host)
{
    SAT_TRY(ctx->d_seg.grow((size_t)nq + 1));
    host.seg.resize((size_t)nq + 1);
    for (int q = 0; q <= nq; q++) host.seg[(size_t)q] = q * stride;
    HIP_TRY(hipMemcpyAsync(ctx->d_seg.get(), host.seg.data(), host.seg.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    return upload_hit_queries(ctx, q0, nq, maps, host.hq);
}

// hipCUB's two-phase call: run(null, bytes) only sets bytes to the space the call needs, ctx->d_sort_temp grows to it
// (behind the stream: the call before may still work in it), run(space, bytes) does the work.
template <typename F> int cub_run(sat_ctx *ctx, F run)
{
    size_t temp_bytes = 0;
    HIP_TRY(run(nullptr, temp_bytes));
    SAT_TRY(ctx->d_sort_temp.grow_after(ctx->stream, temp_bytes ? temp_bytes : 1));
    HIP_TRY(run(ctx->d_sort_temp.get(), temp_bytes));
    return SAT_OK;
}

// n keys sorted descending from ctx->d_keys to ctx->d_sorted: one segment, or nseg segments seg[s] .. seg[s + 1] - 1 (device)
int sort_keys_desc(sat_ctx *ctx, int n, int nseg, int *seg)
{
    const unsigned long long *in = ctx->d_keys.get();
    unsigned long long *out = ctx->d_sorted.get();
    return cub_run(ctx, [&](void *temp, size_t &temp_bytes) {
        if (nseg == 1) return hipcub::DeviceRadixSort::SortKeysDescending(temp, temp_bytes, in, out, n, 0, 64, ctx->stream);
        return hipcub::DeviceSegmentedRadixSort::SortKeysDescending(temp, temp_bytes, in, out, n, nseg, seg, seg + 1, 0, 64, ctx->stream);
    });
}

// rank queries [q0, q0 + nq) of the last search; rows land at row `out_row` of ctx->d_hits (and
// ctx->d_hit_maps), which hold `rows_total` rows
int select_hits(sat_ctx *ctx, int q0, int nq, int k, bool want_maps, size_t out_row, size_t rows_total)
{
    const int n = ctx->n_entries;
    const size_t total = (size_t)nq * n;
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(ctx->d_keys.grow(total));
    SAT_TRY(ctx->d_sorted.grow(total));
    if (out_row == 0) {                                   // first chunk: size the row buffers for the whole batch
        SAT_TRY(ctx->d_hits.grow(rows_total));
        if (want_maps) SAT_TRY(ctx->d_hit_maps.grow(rows_total * SAT_MAXDIM));
    }
    RankInput host;
    SAT_TRY(upload_rank_input(ctx, q0, nq, n, want_maps, host));

    const int32_t *scores = ctx->d_scores.get() + (size_t)q0 * n;
    hipLaunchKernelGGL(pack_keys, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, scores, (long long)total, n,
                       ctx->d_keys.get());
    HIP_TRY(hipGetLastError());
    SAT_TRY(sort_keys_desc(ctx, (int)total, nq, ctx->d_seg.get()));
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
    return sat_query_chunks(nq, per_chunk, [&](int q0, int nqc) { return select_hits(ctx, q0, nqc, k, want_maps, (size_t)q0 * k, (size_t)nq * k); });
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
    if (maps) {                                          // (not row_map: without its null test this loop compiles to other code)
        int32_t *out = maps + (size_t)t * SAT_MAXDIM;
        const int8_t *src = pmaps + (size_t)p * SAT_MAXDIM;
        for (int i = 0; i < SAT_MAXDIM; i++) out[i] = i < n1 ? (int32_t)src[i] : -1;
    }
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
    block_count(hit, [&](int32_t c) { atomicAdd(counts + q, c); });
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
    if (maps) row_map(queries[q].ssemaps ? queries[q].ssemaps + (size_t)entry * n1 : nullptr, n1, maps + (size_t)t * SAT_MAXDIM);
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

}  // namespace

// ---- sat_cutoff.hpp: the searched state, for this file and for sat_cluster_add, which walks the same rows
int sat_check_searched(sat_ctx *ctx)
{
    SAT_TRY(sat_check_context(ctx));
    if (ctx->n_entries <= 0 || ctx->queries.empty() || !ctx->d_scores.get() || ctx->searched_nq != ctx->queries.size())
        return sat_fail(SAT_ESTATE, "no search has run since the last database upload / query change");
    return SAT_OK;
}

int sat_cutoff_chunk(const sat_ctx *ctx, int n)
{
    const long long bpq = (n + kCutoffBlock - 1) / kCutoffBlock, keys = ctx->tune.select_keys;
    long long per = keys / n;
    if (keys / (bpq * kCutoffBlock) < per) per = keys / (bpq * kCutoffBlock);
    return per < 1 ? 1 : (int)per;
}

int sat_hitq_upload(sat_ctx *ctx, bool maps)
{
    std::vector<HitQuery> hq_host;
    SAT_TRY(upload_hit_queries(ctx, 0, (int)ctx->queries.size(), maps, hq_host));
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // hq_host dies at return
    return SAT_OK;
}

// The histogram of every query of the last search into ctx->d_hist (counts [nq][SAT_STAT_BINS], then below [nq]) and
// from there to the host.  The query lists go in sat_cutoff_chunk's chunks: fewer blocks per query here, so a chunk that
// fits the cutoff kernels' grid fits this one.
extern "C" int sat_score_histogram(sat_ctx *ctx, uint32_t *counts, int32_t *below)
{
    SAT_TRY(sat_check_searched(ctx));
    if (!counts || !below) return sat_fail(SAT_EINVAL, "histogram buffer is null");
    const int n = ctx->n_entries, nq = (int)ctx->queries.size();
    if (n > 0x7FFFFFFF - kHistRows) return sat_fail(SAT_EINVAL, "too many entries for the histogram pass");
    const size_t words = (size_t)nq * (SAT_STAT_BINS + 1);
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(ctx->d_hist.grow(words));
    SAT_TRY(sat_hitq_upload(ctx, false));
    const HitQuery *hq = hit_queries(ctx);
    uint32_t *d_counts = ctx->d_hist.get();
    int32_t *d_below = reinterpret_cast<int32_t *>(d_counts + (size_t)nq * SAT_STAT_BINS);
    HIP_TRY(hipMemsetAsync(d_counts, 0, words * sizeof(uint32_t), ctx->stream));
    SAT_TRY(sat_row_chunks(ctx, kHistRows, [&](int q0, int, int bpq, dim3 grid) -> int {
        hipLaunchKernelGGL(score_histogram, grid, dim3(kHistBlock), 0, ctx->stream, ctx->d_scores.get() + (size_t)q0 * n, n, bpq,
                           ctx->d_orders.get(), hq + q0, d_counts + (size_t)q0 * SAT_STAT_BINS, d_below + q0);
        HIP_TRY(hipGetLastError());
        return SAT_OK;
    }));
    SAT_TRY(sat_fetch(ctx, counts, d_counts, (size_t)nq * SAT_STAT_BINS, true));
    SAT_TRY(sat_fetch(ctx, below, d_below, (size_t)nq, true));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SAT_OK;
}

extern "C" int sat_stats_set(sat_ctx *ctx, const sat_fit *fits)
{
    SAT_TRY(sat_check_searched(ctx));
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
        SAT_TRY(ctx->d_fit_tabs.grow_after(ctx->stream, nq * 2 * SAT_STAT_BINS));
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
    SAT_TRY(sat_check_searched(ctx));
    SAT_TRY(sat_check_censor(censor));
    return sat_fit_queries(ctx->queries.size(), censor, fits, [&](uint32_t *counts, int32_t *below) { return sat_score_histogram(ctx, counts, below); },
                           [&](const sat_fit *fit) { return sat_stats_set(ctx, fit); });
}

extern "C" int sat_debug_set_scores(sat_ctx *ctx, const int32_t *scores)
{
    SAT_TRY(sat_check_searched(ctx));
    if (!scores) return sat_fail(SAT_EINVAL, "scores buffer is null");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(ctx->d_scores.get(), scores, ctx->queries.size() * (size_t)ctx->n_entries * sizeof(int32_t), hipMemcpyHostToDevice));
    ctx->fits.clear();
    return SAT_OK;
}

extern "C" int sat_topk(sat_ctx *ctx, int query, int k, int32_t *entry_index, int32_t *scores_out)
{
    SAT_TRY(sat_check_searched(ctx));
    SAT_TRY(sat_check_topk(entry_index && scores_out, k));
    if (query < 0 || query >= (int)ctx->queries.size()) return sat_fail(SAT_EINVAL, "query %d out of range", query);
    if (k > ctx->n_entries) k = ctx->n_entries;
    SAT_TRY(select_hits(ctx, query, 1, k, false, 0, (size_t)k));
    std::vector<sat_hit> rows((size_t)k);
    SAT_TRY(sat_fetch(ctx, rows.data(), ctx->d_hits.get(), rows.size()));
    for (int i = 0; i < k; i++) {
        entry_index[i] = rows[(size_t)i].entry;
        scores_out[i] = rows[(size_t)i].score;
    }
    return k;
}

extern "C" int sat_topk_hits(sat_ctx *ctx, int k, sat_hit *hits, int32_t *ssemaps)
{
    SAT_TRY(sat_check_searched(ctx));
    SAT_TRY(sat_check_topk(hits != nullptr, k));
    if (ssemaps) SAT_TRY(sat_check_lsoln(ctx->searched_lsoln));
    if (k > ctx->n_entries) k = ctx->n_entries;
    const size_t rows = ctx->queries.size() * (size_t)k;
    SAT_TRY(select_all_hits(ctx, k, ssemaps != nullptr));
    SAT_TRY(sat_fetch(ctx, hits, ctx->d_hits.get(), rows));
    if (ssemaps) SAT_TRY(sat_fetch(ctx, ssemaps, ctx->d_hit_maps.get(), rows * SAT_MAXDIM));
    return k;
}

// sat_search_refine (tops = 0) and sat_search_refine_polish (tops = maps polished per candidate): the stage-2 keys and
// maps come from the pair search or from the polish (sat_polish.hip), everything around them is shared
static int refine(sat_ctx *ctx, int lorder, int lsoln, int maxstart, int candidates, int refine_maxstart, int tops,
                  int k, sat_hit *hits, int32_t *ssemaps, int32_t *first_scores, int32_t *base_scores)
{
    SAT_TRY(sat_check_refine(ctx, hits, k, candidates, refine_maxstart));
    HIP_TRY(hipSetDevice(ctx->device));
    // stage 1: the plain search at maxstart, without LSOLN
    SAT_TRY(launch_search(ctx, lorder, 0, maxstart, ctx->stream));
    const std::string stage1_info = ctx->last_launch_info;
    const int n = ctx->n_entries, nq = (int)ctx->queries.size();
    const int c = candidates < n ? candidates : n;
    if (k > c) k = c;
    if ((long long)nq * c > 0x7FFFFFFFll) return sat_fail(SAT_EINVAL, "queries x candidates exceed 2^31 - 1");
    const int npairs = nq * c;
    // the best c entries of every query, ranked on the device (rows stay there); only their indices come back
    SAT_TRY(select_all_hits(ctx, c, false));
    std::vector<int32_t> query((size_t)npairs), entry((size_t)npairs);
    SAT_TRY(sat_fetch_strided(ctx, entry.data(), ctx->d_hits.get(), sizeof(sat_hit), (size_t)npairs));     // sat_hit begins with its entry
    for (int p = 0; p < npairs; p++) query[(size_t)p] = p / c;
    // stage 2: the candidates at refine_maxstart (and their maps)
    const bool maps = lsoln && ssemaps;
    SAT_TRY(tops ? sat_pair_matches_launch(ctx, lorder, refine_maxstart, tops, true, query.data(), entry.data(), npairs, PairMode::Polish)
                 : sat_pairs_launch(ctx, lorder, refine_maxstart, maps, query.data(), entry.data(), npairs));
    const unsigned long long *pkeys = tops ? ctx->d_polkeys.get() : ctx->d_pkeys.get();
    const int8_t *pmaps = tops ? ctx->d_polmaps.get() : ctx->d_pmaps.get();
    const std::string stage2_info = ctx->last_launch_info;
    // the final ranking: segments of c keys, one per query
    const size_t rows = (size_t)nq * k;
    SAT_TRY(ctx->d_rkeys.grow((size_t)npairs));
    SAT_TRY(ctx->d_rsorted.grow((size_t)npairs));
    SAT_TRY(ctx->d_rvals.grow((size_t)npairs));
    SAT_TRY(ctx->d_rvals_sorted.grow((size_t)npairs));
    SAT_TRY(ctx->d_rhits.grow(rows));
    SAT_TRY(ctx->d_rfirst.grow(2 * rows));                               // stage-1 scores, then (polish) base scores
    if (maps) SAT_TRY(ctx->d_rmaps.grow(rows * SAT_MAXDIM));
    RankInput host;
    SAT_TRY(upload_rank_input(ctx, 0, nq, c, false, host));
    hipLaunchKernelGGL(pack_refined, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, ctx->stream, pkeys, ctx->d_hits.get(),
                       npairs, ctx->d_rkeys.get(), ctx->d_rvals.get());
    HIP_TRY(hipGetLastError());
    SAT_TRY(cub_run(ctx, [&](void *temp, size_t &temp_bytes) {
        return hipcub::DeviceSegmentedRadixSort::SortPairsDescending(temp, temp_bytes, ctx->d_rkeys.get(), ctx->d_rsorted.get(),
                                                                     ctx->d_rvals.get(), ctx->d_rvals_sorted.get(), npairs, nq,
                                                                     ctx->d_seg.get(), ctx->d_seg.get() + 1, 0, 64, ctx->stream);
    }));
    hipLaunchKernelGGL(finish_refined, dim3((unsigned)((nq * k + 127) / 128)), dim3(128), 0, ctx->stream, ctx->d_rsorted.get(),
                       ctx->d_rvals_sorted.get(), c, k, nq, ctx->d_orders.get(), hit_queries(ctx), ctx->d_gumbel_z.get(),
                       ctx->d_gumbel_p.get(), ctx->d_hits.get(), pmaps, ctx->d_rhits.get(), ctx->d_rfirst.get(),
                       maps ? ctx->d_rmaps.get() : nullptr, tops ? (const int32_t *)ctx->d_polout.get() + npairs : nullptr,
                       tops ? ctx->d_rfirst.get() + rows : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (tops) {
        // a pair whose polish did not finish carries moves = -1 (sat_polish.hip): one flag row, npairs ints
        std::vector<int32_t> mv((size_t)npairs);
        SAT_TRY(sat_fetch(ctx, mv.data(), ctx->d_polout.get() + 3 * (size_t)npairs, mv.size()));
        for (int p = 0; p < npairs; p++)
            if (mv[(size_t)p] < 0) return sat_fail(SAT_EDEVICE, "pair %d: the polish did not finish", p);
        if (base_scores) SAT_TRY(sat_fetch(ctx, base_scores, ctx->d_rfirst.get() + rows, rows));
    }
    SAT_TRY(sat_fetch(ctx, hits, ctx->d_rhits.get(), rows));
    if (first_scores) SAT_TRY(sat_fetch(ctx, first_scores, ctx->d_rfirst.get(), rows));
    if (maps) SAT_TRY(sat_fetch(ctx, ssemaps, ctx->d_rmaps.get(), rows * SAT_MAXDIM));
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
    SAT_TRY(sat_check_tops(tops));
    return refine(ctx, lorder, lsoln, maxstart, candidates, refine_maxstart, tops, k, hits, ssemaps, first_scores, base_scores);
}

// ---- p-value cutoff.  ctx->d_seg holds, in ints: [nq] the count pass's counts, then for the chunk at hand its
// segment offsets [nqc + 1], its output offsets [nqc + 1] and its claim cursors [nqc].

int sat_cutoff_count(sat_ctx *ctx, double max_pvalue, bool maps, int32_t *counts)
{
    SAT_TRY(sat_check_searched(ctx));
    if (maps) SAT_TRY(sat_check_lsoln(ctx->searched_lsoln));
    const int n = ctx->n_entries, nq = (int)ctx->queries.size(), pc = std::min(sat_cutoff_chunk(ctx, n), nq);
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(ctx->d_seg.grow((size_t)nq + 3 * (size_t)pc + 2));
    SAT_TRY(sat_hitq_upload(ctx, maps));
    const HitQuery *hq = hit_queries(ctx);
    HIP_TRY(hipMemsetAsync(ctx->d_seg.get(), 0, (size_t)nq * sizeof(int32_t), ctx->stream));
    SAT_TRY(sat_row_chunks(ctx, kCutoffBlock, [&](int q0, int, int bpq, dim3 grid) -> int {
        hipLaunchKernelGGL(cutoff_count, grid, dim3(kCutoffBlock), 0, ctx->stream, ctx->d_scores.get() + (size_t)q0 * n, n, bpq,
                           ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(), max_pvalue, ctx->d_seg.get() + q0);
        HIP_TRY(hipGetLastError());
        return SAT_OK;
    }));
    SAT_TRY(sat_fetch(ctx, counts, ctx->d_seg.get(), (size_t)nq, true));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SAT_OK;
}

int sat_cutoff_rows(sat_ctx *ctx, double max_pvalue, int max_rows, const int32_t *counts, sat_hit *hits, int32_t *ssemaps)
{
    const int n = ctx->n_entries, nq = (int)ctx->queries.size();
    const bool maps = ssemaps != nullptr;
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
    SAT_TRY(ctx->d_hits.grow(rows_total));
    if (maps) SAT_TRY(ctx->d_hit_maps.grow(rows_total * SAT_MAXDIM));
    const HitQuery *hq = hit_queries(ctx);                                    // as sat_cutoff_count left them
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
        HIP_TRY(hipMemcpyAsync(d_out, out_off.data(), out_off.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemsetAsync(seg, 0, sizeof(int32_t), ctx->stream));
        HIP_TRY(hipMemsetAsync(cursor, 0, (size_t)nqc * sizeof(int32_t), ctx->stream));
        SAT_TRY(cub_run(ctx, [&](void *temp, size_t &temp_bytes) {
            return hipcub::DeviceScan::InclusiveSum(temp, temp_bytes, ctx->d_seg.get() + q0, seg + 1, nqc, ctx->stream);
        }));
        hipLaunchKernelGGL(cutoff_compact, grid, dim3(kCutoffBlock), 0, ctx->stream, ctx->d_scores.get() + (size_t)q0 * n, n, bpq,
                           ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(), max_pvalue, seg, cursor,
                           ctx->d_keys.get());
        HIP_TRY(hipGetLastError());
        SAT_TRY(sort_keys_desc(ctx, keys, nqc, seg));
        hipLaunchKernelGGL(cutoff_finish, dim3((unsigned)((rows + 127) / 128)), dim3(128), 0, ctx->stream, ctx->d_sorted.get(), seg, d_out,
                           nqc, rows, ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(),
                           ctx->d_hits.get() + out_row, maps ? ctx->d_hit_maps.get() + out_row * SAT_MAXDIM : nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));                     // out_off is reused by the next chunk
        out_row += (size_t)rows;
        return SAT_OK;
    }));
    SAT_TRY(sat_fetch(ctx, hits, ctx->d_hits.get(), rows_total));
    if (maps) SAT_TRY(sat_fetch(ctx, ssemaps, ctx->d_hit_maps.get(), rows_total * SAT_MAXDIM));
    return SAT_OK;
}

extern "C" int sat_hits_cutoff(sat_ctx *ctx, double max_pvalue, int max_rows, int32_t *counts, int capacity, sat_hit *hits,
                               int32_t *ssemaps)
{
    SAT_TRY(sat_check_searched(ctx));
    if (!counts) return sat_fail(SAT_EINVAL, "counts buffer is null");
    SAT_TRY(sat_check_pvalue(max_pvalue));
    const int nq = (int)ctx->queries.size();
    std::vector<int32_t> raw((size_t)nq);
    SAT_TRY(sat_cutoff_count(ctx, max_pvalue, ssemaps != nullptr, raw.data()));
    size_t total = 0;
    for (int q = 0; q < nq; q++) total += (size_t)(counts[q] = sat_row_cap(raw[(size_t)q], max_rows));
    if (total > (size_t)INT_MAX) return sat_fail(SAT_EINVAL, "%zu rows qualify: more than one call can return", total);
    if (!hits || (long long)total > (long long)capacity) return (int)total;
    SAT_TRY(sat_cutoff_rows(ctx, max_pvalue, max_rows, raw.data(), hits, ssemaps));
    return (int)total;
}
