// sat_reach.hip - transitive search: follow hits of hits from a seed, on the device (sat_reach_*, sat_search_reach;
// DESIGN.md 6x).
//
// Nodes are the structures of the whole database in file order.  Row (q, e) of the last search is the DIRECTED step
// a -> b, a = query_node[q] (-1: an external query), b = ordinal[e], iff the p-value hit_row gives it is <= max_pvalue -
// the double sat_hits_cutoff and sat_cluster_add compare - and a != b.  The accumulator is one 64-bit key per node
// (host/sat_reach.h: depth | bits of (float)p | parent, unreached = all ones) and one support count.  reach_add walks the
// rows as cluster_add does; a step does atomicMin(key + b, pack(depth, p, a)) and atomicAdd(support + b, 1).  Both
// commute, so key[] and support[] are functions of the multiset of (depth, row) pairs added: nothing depends on the
// launch shape, the batch cut of a level, the order of the add calls or the sharding.
//
// key is written by the init and seed kernels - plain stores, each in a launch of its own, ordered on the stream before
// any add - and by atomicMin alone after that: a word only ever decreases.  reach_add reads it with a relaxed agent-scope
// atomic load (the eight XCDs have an L2 each; a plain load may be served from a stale line).  A stale value is an EARLIER
// value of the word, so at or above the current one: "loaded <= candidate" then holds for the current word too and the
// atomic is skipped rightly; "loaded > candidate" costs at worst one atomic that changes nothing.  A block's rows share
// their query and many queries share popular entries, so most steps past the first to a node skip the 64-bit atomic.
//
// The frontier and the rows leave through one ordered compaction: the count of every block of 1024 nodes, one block
// that turns the counts into running sums (and their total), and a scatter in which a node's place is its block's sum
// plus its rank in the block - three launches in stream order, no cooperative launch, no grid-wide barrier, and the
// order is ascending by construction.  These kernels run behind every add on the stream and load the keys plainly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "sat_ctx.hpp"
#include "sat_cutoff.hpp"
#include "sat_hitrow.hpp"
#include "host/sat_reach.h"

static_assert(sizeof(sat_reach_row) == 20 && sizeof(sat_reach_row) == sizeof(sat_reach_rec), "sat_reach_row is 20 bytes");

namespace {

// One thread per row, the grid of cluster_add (blocks of kCutoffBlock rows of one query)
__global__ void __launch_bounds__(kCutoffBlock) reach_add(const int32_t *scores, int n, int bpq, const int32_t *orders,
                                                           const HitQuery *queries, const double *ztab, const double *ptab,
                                                           double max_p, int depth, const int32_t *query_node, const uint32_t *ordinal,
                                                           unsigned long long *key, int32_t *support)
{
    const int q = (int)(blockIdx.x / (unsigned)bpq);
    const int e = (int)(blockIdx.x - (unsigned)q * bpq) * kCutoffBlock + (int)threadIdx.x;
    if (e >= n) return;
    const double p = hit_row(e, scores[(size_t)q * n + e], queries[q].n1, orders[e], ztab, ptab, queries[q].fit).pvalue;
    if (!(p <= max_p)) return;
    const int32_t a = query_node[q], b = (int32_t)ordinal[e];          // a is -1 or < nodes, b < nodes: checked on the host
    if (a == b) return;
    const unsigned long long cand = sat_reach_pack(depth, p, a);
    if (__hip_atomic_load(key + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > cand) atomicMin(key + b, cand);
    atomicAdd(support + b, 1);
}

// key[v] = unreached, support[v] = 0 for v < nodes
__global__ void reach_init(int nodes, unsigned long long *key, int32_t *support)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < nodes) {
        key[v] = SAT_REACH_UNREACHED;
        support[v] = 0;
    }
}

// the seeds (distinct, < nodes: checked on the host) at depth 0
__global__ void reach_seed(int n_seeds, const int32_t *seed, unsigned long long *key)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_seeds) key[seed[i]] = sat_reach_pack(0, 0.0, -1);
}

// want >= 0: the node's depth is `want`; want < 0: the node is reached
__device__ __forceinline__ bool wanted(unsigned long long key, int want)
{
    const int depth = (int)(key >> 58);
    return want >= 0 ? depth == want : depth != SAT_REACH_NO_DEPTH;
}

// the threads of the block with `flag` before this one, and (total) all of them: a ballot per wave, the 16 counts
// through LDS.  Every thread of the block calls it, once per kernel.
__device__ __forceinline__ int block_rank(bool flag, int &total)
{
    __shared__ int32_t wave_count[kCutoffWaves];
    const unsigned long long mask = __ballot(flag);
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    if (lane == 0) wave_count[wave] = (int32_t)__popcll(mask);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = 0; w < kCutoffWaves; w++) {
        const int c = wave_count[w];
        before += w < wave ? c : 0;
        total += c;
    }
    return before + (int)__popcll(mask & ((1ull << lane) - 1ull));
}

// counts[block] = the wanted nodes among the block's kCutoffBlock
__global__ void __launch_bounds__(kCutoffBlock) reach_count(int nodes, const unsigned long long *key, int want, int32_t *counts)
{
    const int v = (int)blockIdx.x * kCutoffBlock + (int)threadIdx.x;
    int total;
    (void)block_rank(v < nodes && wanted(key[v < nodes ? v : 0], want), total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// ONE block: offsets[i] = counts[0] + .. + counts[i - 1] for i < nb, *total = their sum.  kCutoffBlock counts at a time,
// an inclusive scan in LDS, the running sum carried from chunk to chunk.
__global__ void __launch_bounds__(kCutoffBlock) reach_scan(int nb, const int32_t *counts, int32_t *offsets, int32_t *total)
{
    __shared__ int32_t s[kCutoffBlock];
    const int t = (int)threadIdx.x;
    int32_t carry = 0;
    for (int base = 0; base < nb; base += kCutoffBlock) {
        const int i = base + t;
        const int32_t c = i < nb ? counts[i] : 0;
        s[t] = c;
        __syncthreads();
        for (int off = 1; off < kCutoffBlock; off <<= 1) {
            const int32_t below = t >= off ? s[t - off] : 0;
            __syncthreads();
            s[t] += below;
            __syncthreads();
        }
        if (i < nb) offsets[i] = carry + s[t] - c;
        carry += s[kCutoffBlock - 1];
        __syncthreads();                                               // every thread has read the chunk's sum
    }
    if (t == 0) *total = carry;
}

// the wanted node of rank r overall goes to place r, if r < cap: its number to out_nodes, or (out_rows not null) its row
__global__ void __launch_bounds__(kCutoffBlock) reach_scatter(int nodes, const unsigned long long *key, const int32_t *support, int want,
                                                               const int32_t *offsets, int cap, int32_t *out_nodes, sat_reach_row *out_rows)
{
    const int v = (int)blockIdx.x * kCutoffBlock + (int)threadIdx.x;
    const unsigned long long k = key[v < nodes ? v : 0];
    const bool flag = v < nodes && wanted(k, want);
    int total;
    const int rank = block_rank(flag, total);
    if (!flag) return;
    const int at = offsets[blockIdx.x] + rank;
    if (at >= cap) return;
    if (out_rows) {
        sat_reach_row r;
        sat_reach_unpack(k, &r.depth, &r.parent, &r.pvalue);
        r.node = v;
        r.support = support[v];
        out_rows[at] = r;
    } else {
        out_nodes[at] = v;
    }
}

int check_accumulator(const sat_ctx *ctx)
{
    SAT_TRY(sat_check_context(ctx));
    if (ctx->reach_nodes <= 0)
        return sat_fail(SAT_ESTATE, "no reach accumulator (sat_reach_begin has not been called since the last database upload)");
    return SAT_OK;
}

// The ordered compaction of the nodes `want` asks for (a depth, or -1: the reached nodes): *count = how many, uncapped,
// and the first min(cap, *count) to nodes, or as rows to rows.  Copies 4 bytes and those.
int compact(sat_ctx *ctx, int want, int cap, int32_t *nodes, sat_reach_row *rows, int32_t *count)
{
    const int n = ctx->reach_nodes, nb = (n + kCutoffBlock - 1) / kCutoffBlock, room = std::min(cap, n);
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(ctx->d_rc_scan.grow_after(ctx->stream, 2 * (size_t)nb + 1));
    if (rows) SAT_TRY(ctx->d_rc_rows.grow_after(ctx->stream, (size_t)room));
    else SAT_TRY(ctx->d_rc_out.grow_after(ctx->stream, (size_t)room));
    int32_t *counts = ctx->d_rc_scan.get(), *offsets = counts + nb, *total = offsets + nb;
    hipLaunchKernelGGL(reach_count, dim3((unsigned)nb), dim3(kCutoffBlock), 0, ctx->stream, n, ctx->d_rc_key.get(), want, counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(reach_scan, dim3(1), dim3(kCutoffBlock), 0, ctx->stream, nb, counts, offsets, total);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(reach_scatter, dim3((unsigned)nb), dim3(kCutoffBlock), 0, ctx->stream, n, ctx->d_rc_key.get(),
                       ctx->d_rc_support.get(), want, offsets, room, rows ? nullptr : ctx->d_rc_out.get(), rows ? ctx->d_rc_rows.get() : nullptr);
    HIP_TRY(hipGetLastError());
    SAT_TRY(sat_fetch(ctx, count, total, 1, true));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t got = (size_t)std::min(room, *count);
    if (got == 0) return SAT_OK;
    if (rows) SAT_TRY(sat_fetch(ctx, rows, ctx->d_rc_rows.get(), got, true));
    else SAT_TRY(sat_fetch(ctx, nodes, ctx->d_rc_out.get(), got, true));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SAT_OK;
}

// a search of the current batch between the context's timing events, as sat_search runs it, lsoln off
int timed_search(sat_ctx *ctx, int lorder, int maxstart, double *ms)
{
    SAT_TRY(timed(ctx, ms, [&] {
        return ctx->polish_all ? sat_polish_all_launch(ctx, lorder, 0, maxstart) : launch_search(ctx, lorder, 0, maxstart, ctx->stream);
    }));
    return ctx->polish_all ? sat_polish_all_check(ctx) : SAT_OK;
}

}  // namespace

// sat_ctx.hpp: load this file's code object (an empty launch of a small kernel)
int sat_reach_load_code(sat_ctx *ctx)
{
    hipLaunchKernelGGL(reach_init, dim3(1), dim3(64), 0, ctx->stream, 0, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return SAT_OK;
}

// sat_ctx.hpp: the accumulator goes (the caller has waited for the stream, or is about to free the database anyway)
void sat_reach_drop(sat_ctx *ctx)
{
    ctx->reach_nodes = 0;
    ctx->d_rc_key.reset();
    ctx->d_rc_support.reset();
}

int sat_reach_check_begin(int n_nodes, int n_seeds, const int32_t *seed_node)
{
    if (n_nodes > SAT_REACH_NO_PARENT) return sat_fail(SAT_EINVAL, "n_nodes = %d: a key holds nodes up to %d", n_nodes, SAT_REACH_NO_PARENT - 1);
    if (n_seeds < 0) return sat_fail(SAT_EINVAL, "n_seeds must be >= 0 (got %d)", n_seeds);
    if (n_seeds > 0 && !seed_node) return sat_fail(SAT_EINVAL, "seed list is null");
    std::vector<std::pair<int32_t, int>> seen((size_t)n_seeds);
    for (int i = 0; i < n_seeds; i++) {
        if (seed_node[i] < 0 || seed_node[i] >= n_nodes)
            return sat_fail(SAT_EINVAL, "seed %d: node %d outside 0..%d", i, seed_node[i], n_nodes - 1);
        seen[(size_t)i] = { seed_node[i], i };
    }
    std::sort(seen.begin(), seen.end());
    int twice = -1;                                                    // the first position that repeats an earlier one
    for (int i = 1; i < n_seeds; i++)
        if (seen[(size_t)i].first == seen[(size_t)i - 1].first && (twice < 0 || seen[(size_t)i].second < twice)) twice = seen[(size_t)i].second;
    if (twice >= 0) return sat_fail(SAT_EINVAL, "seed %d: node %d listed twice", twice, seed_node[twice]);
    return SAT_OK;
}

int sat_reach_check_add(int depth, double max_pvalue, int nq, const int32_t *query_node, int nodes)
{
    if (!query_node) return sat_fail(SAT_EINVAL, "query_node is null");
    if (depth < 1 || depth > SAT_REACH_MAX_DEPTH) return sat_fail(SAT_EINVAL, "depth must be 1..%d (got %d)", SAT_REACH_MAX_DEPTH, depth);
    SAT_TRY(sat_check_pvalue(max_pvalue));
    for (int q = 0; q < nq; q++)
        if (query_node[q] < -1 || query_node[q] >= nodes)
            return sat_fail(SAT_EINVAL, "query %d: node %d outside -1..%d", q, query_node[q], nodes - 1);
    return SAT_OK;
}

int sat_reach_check_fetch(int depth, int cap, const void *out, const int32_t *count)
{
    if (depth < 0 || depth > SAT_REACH_MAX_DEPTH) return sat_fail(SAT_EINVAL, "depth must be 0..%d (got %d)", SAT_REACH_MAX_DEPTH, depth);
    if (!count) return sat_fail(SAT_EINVAL, "count is null");
    if (cap < 0) return sat_fail(SAT_EINVAL, "cap must be >= 0 (got %d)", cap);
    if (cap > 0 && !out) return sat_fail(SAT_EINVAL, "cap = %d but the output buffer is null", cap);
    return SAT_OK;
}

int sat_reach_check_search(int n_seeds, const int32_t *seed_entry, int n_entries, int maxstart, double max_pvalue, int max_depth,
                           int max_queries, int batch, double censor, int cap, const void *rows, const int32_t *count, const void *info)
{
    if (n_seeds < 1 || !seed_entry) return sat_fail(SAT_EINVAL, "bad seed list (n_seeds=%d)", n_seeds);
    for (int i = 0; i < n_seeds; i++)
        if (seed_entry[i] < 0 || seed_entry[i] >= n_entries)
            return sat_fail(SAT_EINVAL, "seed %d: entry %d outside 0..%d", i, seed_entry[i], n_entries - 1);
    if (maxstart < 1) return sat_fail(SAT_EINVAL, "maxstart must be >= 1 (got %d)", maxstart);
    SAT_TRY(sat_check_pvalue(max_pvalue));
    if (max_depth < 1 || max_depth > SAT_REACH_MAX_DEPTH)
        return sat_fail(SAT_EINVAL, "max_depth must be 1..%d (got %d)", SAT_REACH_MAX_DEPTH, max_depth);
    if (max_queries < 1) return sat_fail(SAT_EINVAL, "max_queries must be >= 1 (got %d)", max_queries);
    if (batch < 1 || batch > 256) return sat_fail(SAT_EINVAL, "batch must be 1..256 (got %d)", batch);
    if (censor >= 0.0) SAT_TRY(sat_check_censor(censor));
    if (!info) return sat_fail(SAT_EINVAL, "info is null");
    return sat_reach_check_fetch(0, cap, rows, count);
}

int sat_reach_arrays_fetch(sat_ctx *ctx, unsigned long long *keys, int32_t *support)
{
    SAT_TRY(check_accumulator(ctx));
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(sat_fetch(ctx, keys, ctx->d_rc_key.get(), (size_t)ctx->reach_nodes, true));
    SAT_TRY(sat_fetch(ctx, support, ctx->d_rc_support.get(), (size_t)ctx->reach_nodes, true));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SAT_OK;
}

extern "C" {

int sat_reach_begin(sat_ctx *ctx, int n_nodes, int n_seeds, const int32_t *seed_node)
{
    SAT_TRY(sat_check_context(ctx));
    SAT_TRY(sat_check_uploaded(ctx->n_entries > 0));
    SAT_TRY(sat_check_nodes(n_nodes, ctx->max_ordinal));
    SAT_TRY(sat_reach_check_begin(n_nodes, n_seeds, seed_node));
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // an earlier accumulator may still be in use there
    ctx->reach_nodes = 0;
    SAT_TRY(ctx->d_rc_key.grow((size_t)n_nodes));
    SAT_TRY(ctx->d_rc_support.grow((size_t)n_nodes));
    SAT_TRY(ctx->d_rc_out.grow((size_t)n_seeds));
    // the caller's list may go at return: a synchronous copy (the stream is idle)
    if (n_seeds > 0) HIP_TRY(hipMemcpy(ctx->d_rc_out.get(), seed_node, (size_t)n_seeds * sizeof(int32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(reach_init, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, ctx->stream, n_nodes, ctx->d_rc_key.get(),
                       ctx->d_rc_support.get());
    HIP_TRY(hipGetLastError());
    if (n_seeds > 0) {
        hipLaunchKernelGGL(reach_seed, dim3((unsigned)((n_seeds + 255) / 256)), dim3(256), 0, ctx->stream, n_seeds, ctx->d_rc_out.get(),
                           ctx->d_rc_key.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));         // d_rc_out is the compaction's scratch from here on
    }
    ctx->reach_nodes = n_nodes;
    return SAT_OK;
}

int sat_reach_add(sat_ctx *ctx, int depth, double max_pvalue, const int32_t *query_node)
{
    SAT_TRY(check_accumulator(ctx));
    SAT_TRY(sat_check_searched(ctx));
    const int n = ctx->n_entries, nodes = ctx->reach_nodes, nq = (int)ctx->queries.size();
    SAT_TRY(sat_reach_check_add(depth, max_pvalue, nq, query_node, nodes));
    if (ctx->max_ordinal >= (uint32_t)nodes) return sat_fail(SAT_ESTATE, "the accumulator does not cover the resident database");
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(ctx->d_rc_qnode.grow_after(ctx->stream, (size_t)nq));
    // the caller's array may go at return: a synchronous copy, ordered behind the stream by sat_hitq_upload's wait
    SAT_TRY(sat_hitq_upload(ctx, false));
    HIP_TRY(hipMemcpy(ctx->d_rc_qnode.get(), query_node, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice));
    const HitQuery *hq = hit_queries(ctx);
    return sat_row_chunks(ctx, kCutoffBlock, [&](int q0, int, int bpq, dim3 grid) -> int {
        hipLaunchKernelGGL(reach_add, grid, dim3(kCutoffBlock), 0, ctx->stream, ctx->d_scores.get() + (size_t)q0 * n, n, bpq,
                           ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(), max_pvalue, depth,
                           ctx->d_rc_qnode.get() + q0, ctx->d_ordinal.get(), ctx->d_rc_key.get(), ctx->d_rc_support.get());
        HIP_TRY(hipGetLastError());
        return SAT_OK;
    });
}

int sat_reach_frontier(sat_ctx *ctx, int depth, int cap, int32_t *nodes, int32_t *count)
{
    SAT_TRY(check_accumulator(ctx));
    SAT_TRY(sat_reach_check_fetch(depth, cap, nodes, count));
    return compact(ctx, depth, cap, nodes, nullptr, count);
}

int sat_reach_rows(sat_ctx *ctx, int cap, sat_reach_row *rows, int32_t *count)
{
    SAT_TRY(check_accumulator(ctx));
    SAT_TRY(sat_reach_check_fetch(0, cap, rows, count));
    if (cap == 0) {                                         // rows may be null: count alone, through the node path
        return compact(ctx, -1, 0, nullptr, nullptr, count);
    }
    return compact(ctx, -1, cap, nullptr, rows, count);
}

int sat_reach_end(sat_ctx *ctx)
{
    SAT_TRY(sat_check_context(ctx));
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    sat_reach_drop(ctx);
    return SAT_OK;
}

int sat_search_reach(sat_ctx *ctx, int n_seeds, const int32_t *seed_entry, int lorder, int maxstart, double max_pvalue,
                     int max_depth, int max_queries, int batch, double censor, uint32_t first_query_ordinal, int cap,
                     sat_reach_row *rows, int32_t *count, sat_reach_info *info)
{
    SAT_TRY(sat_check_context(ctx));
    SAT_TRY(sat_check_uploaded(ctx->n_entries > 0));
    SAT_TRY(sat_reach_check_search(n_seeds, seed_entry, ctx->n_entries, maxstart, max_pvalue, max_depth, max_queries, batch, censor,
                                   cap, rows, count, info));
    // the nodes are the ordinals: the largest must fit a key's parent field - asked before anything is sized by it
    if (ctx->max_ordinal >= (uint32_t)SAT_REACH_NO_PARENT)
        return sat_fail(SAT_EINVAL, "a resident entry has ordinal %u in the whole database: a key holds nodes up to %d", ctx->max_ordinal,
                        SAT_REACH_NO_PARENT - 1);
    // nodes <-> resident entries: a node the walk reaches is the ordinal of a resident entry
    const int n_nodes = (int)ctx->max_ordinal + 1;
    std::vector<int32_t> entry_of((size_t)n_nodes, -1), seeds((size_t)n_seeds);
    for (int e = ctx->n_entries - 1; e >= 0; e--) entry_of[ctx->h_ordinal[(size_t)e]] = e;
    for (int i = 0; i < n_seeds; i++) seeds[(size_t)i] = (int32_t)ctx->h_ordinal[(size_t)seed_entry[i]];
    SAT_TRY(sat_reach_begin(ctx, n_nodes, n_seeds, seeds.data()));
    *info = sat_reach_info{ 0, 0, 0, SAT_REACH_EXHAUSTED, 0.0, 0.0 };
    std::vector<int32_t> frontier, entries((size_t)batch);
    for (int d = 1;; d++) {
        // no more than the budget's rest can be searched: a longer frontier ends the run, and its count says so
        frontier.resize((size_t)std::min(max_queries - info->queries, n_nodes));
        int32_t c = 0;
        SAT_TRY(sat_reach_frontier(ctx, d - 1, (int)frontier.size(), frontier.data(), &c));
        if (c == 0) { info->stop = SAT_REACH_EXHAUSTED; break; }
        if (d - 1 == max_depth) { info->stop = SAT_REACH_DEPTH; break; }
        if (c > max_queries - info->queries) { info->stop = SAT_REACH_BUDGET; break; }
        for (int at = 0; at < c; at += batch) {
            const int nb = std::min(batch, c - at);
            for (int i = 0; i < nb; i++) entries[(size_t)i] = entry_of[(size_t)frontier[(size_t)(at + i)]];
            SAT_TRY(sat_queries_from_db(ctx, nb, entries.data(), first_query_ordinal + (uint32_t)(info->queries + at)));
            double ms = 0.0;
            SAT_TRY(timed_search(ctx, lorder, maxstart, &ms));
            info->search_ms += ms;
            if (censor >= 0.0) SAT_TRY(sat_stats_fit(ctx, censor, nullptr));
            SAT_TRY(timed(ctx, &ms, [&] { return sat_reach_add(ctx, d, max_pvalue, frontier.data() + at); }));
            info->pass_ms += ms;
        }
        info->queries += c;
        info->levels++;
    }
    SAT_TRY(sat_reach_rows(ctx, cap, rows, count));
    info->reached = *count;
    return SAT_OK;
}

}  // extern "C"
