// sat_eval.hip - a finished search scored against a classification of the database, on the device (sat_eval_*,
// DESIGN.md 6q): per query the AUC and ROC-n sums of csrc/host/sat_eval.h, 32 bytes a query to the host.
//
// Nodes are the structures of the whole database in file order, node_class[v] >= 0 a node's class.  Row (q, e) of the
// last search is COUNTED for query q iff entry e is classified and is not the query's own node; it is a positive when
// its class is the query's, else a negative.  eval_histogram walks the rows as score_histogram does and counts them by
// raw score into the query's table [2][bins] (positives, then negatives; bins = 2 n1 (n1 - 1) + 1, sat_eval_bin_of);
// eval_reduce walks each table from the top and leaves one sat_eval.  Everything is an integer count or a sum of
// products of counts, so nothing depends on the launch shape, the LDS window, the chunks or the sharding: the shards'
// tables add up (sat_eval_tables, sat_multi_eval_rows).  The host side takes the searched-state check, the chunk walk
// and the counted copies from sat_cutoff.hpp.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

#include "sat_ctx.hpp"
#include "sat_cutoff.hpp"
#include "host/sat_eval.h"

static_assert(sizeof(sat_eval) == 32 && sizeof(sat_eval_row) == 32, "sat_eval is 32 bytes");
static_assert(offsetof(sat_eval, query_class) == offsetof(sat_eval_row, query_class), "sat_eval_row is sat_eval's layout");

namespace {

// what the kernels know of a query: where its table starts in the scratch (in words), its order, node and class
struct EvalQuery {
    long long off;
    int32_t n1, node, cls, pad;
};

// ---- eval_histogram.  Blocks of kEvalRows rows, `bpq` blocks per query, so that a block holds rows of one query only
// (as score_histogram).  A 111-SSE query has 24 421 bins a side: the LDS holds a WINDOW of kEvalWindow bins a side,
// from the bin of score kEvalWindowLow up (from bin 0 where the whole table fits: every query of at most 32 SSEs).  A
// row inside the window is counted with an LDS integer atomic, and the block then adds its NON-ZERO bins to the query's
// table with global integer atomics; a row outside goes straight to a global atomic.  The scores of a search crowd
// just above zero - an unrelated pair of structures scores a few tens - so the window starts a little below it.
constexpr int kEvalBlock = 1024, kEvalPasses = 4, kEvalRows = kEvalBlock * kEvalPasses;
constexpr int kEvalWindow = 2048, kEvalWindowLow = -256;

__global__ void __launch_bounds__(kEvalBlock) eval_histogram(const int32_t *scores, int n, int bpq, const EvalQuery *queries,
                                                             const int32_t *entry_class, const uint32_t *ordinal, uint32_t *tables)
{
    __shared__ uint32_t hist[2][kEvalWindow];
    const int q = (int)(blockIdx.x / (unsigned)bpq);
    const EvalQuery eq = queries[q];
    if (eq.cls < 0) return;                                             // an unclassified query: its table stays zero
    const int e0 = (int)(blockIdx.x - (unsigned)q * bpq) * kEvalRows;
    const int bins = sat_eval_bins(eq.n1);
    // the window's first bin: 0 when the table fits, else the bin of kEvalWindowLow (bins > kEvalWindow: it exists)
    const int lo = bins <= kEvalWindow ? 0 : sat_eval_bin_of(kEvalWindowLow, eq.n1);
    uint32_t *table = tables + eq.off;
    for (int k = (int)threadIdx.x; k < 2 * kEvalWindow; k += kEvalBlock) (&hist[0][0])[k] = 0u;
    __syncthreads();
    for (int pass = 0; pass < kEvalPasses; pass++) {
        const int e = e0 + pass * kEvalBlock + (int)threadIdx.x;        // e0 + kEvalRows <= n + kEvalRows: no overflow (checked on the host)
        if (e >= n) continue;
        const int32_t c = entry_class[e];
        if (c < 0 || (int32_t)ordinal[e] == eq.node) continue;         // unclassified, or the structure against itself
        const int side = c == eq.cls ? 0 : 1;
        const int bin = sat_eval_bin_of(scores[(size_t)q * n + e], eq.n1);      // 0 .. bins - 1
        const int w = bin - lo;
        if (w >= 0 && w < kEvalWindow) atomicAdd(&hist[side][w], 1u);
        else atomicAdd(table + (size_t)side * bins + bin, 1u);
    }
    __syncthreads();
    for (int k = (int)threadIdx.x; k < 2 * kEvalWindow; k += kEvalBlock) {
        const int side = k / kEvalWindow, w = k - side * kEvalWindow;
        const uint32_t c = hist[side][w];
        if (c) atomicAdd(table + (size_t)side * bins + lo + w, c);     // c != 0: a row was counted there, so lo + w < bins
    }
}

// entry_class[e] = node_class[ordinal[e]]: the pass reads a contiguous word per entry instead of gathering
__global__ void eval_entry_classes(int n, const uint32_t *ordinal, const int32_t *node_class, int32_t *entry_class)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) entry_class[e] = node_class[ordinal[e]];
}

// ---- eval_reduce.  One wave per query walks its table from the top, 64 bins a step, lane 0 the highest: a wave-wide
// scan gives every lane the positives and negatives above its bin, sat_eval_walk (the host's function) that bin's terms
// of u2 and t2, and the lanes' sums are added at the end.  A step whose 128 counts are all zero - most of a large
// query's table - is skipped.  The walk is bound by the latency of its loads, one wave a query: the counts of
// kReduceAhead steps are loaded before the first of them is worked on (one step at a time, a 111-SSE query's 382 steps
// took 122 us).  The row is written with plain vector stores by lane 0.
constexpr int kReduceAhead = 8;

__device__ __forceinline__ uint32_t wave_exclusive_sum(uint32_t v, int lane, uint32_t &total)
{
    uint32_t s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(s, d);
        if (lane >= d) s += up;
    }
    total = __shfl(s, 63);
    return s - v;
}

__global__ void __launch_bounds__(64) eval_reduce(const EvalQuery *queries, const uint32_t *tables, int rocn, sat_eval *rows)
{
    const int q = (int)blockIdx.x, lane = (int)threadIdx.x;
    const EvalQuery eq = queries[q];
    sat_eval_row out = { 0, 0, 0, 0, 0, eq.cls < 0 ? -1 : eq.cls };
    if (eq.cls >= 0) {
        const int bins = sat_eval_bins(eq.n1);
        const uint32_t *pos = tables + eq.off, *neg = pos + bins;
        uint32_t pabove = 0, nabove = 0;                                 // above this step's bins (wave-uniform)
        unsigned long long u2 = 0, t2 = 0;                               // this lane's terms
        for (int top = bins - 1; top >= 0; top -= 64 * kReduceAhead) {
            uint32_t p[kReduceAhead], g[kReduceAhead];
#pragma unroll
            for (int j = 0; j < kReduceAhead; j++) {
                const int b = top - 64 * j - lane;
                p[j] = b >= 0 ? pos[b] : 0u;
                g[j] = b >= 0 ? neg[b] : 0u;
            }
#pragma unroll
            for (int j = 0; j < kReduceAhead; j++) {
                if (!__any((p[j] | g[j]) != 0u)) continue;
                uint32_t ptotal, ntotal;
                sat_eval_row acc = { 0, 0, (int32_t)(pabove + wave_exclusive_sum(p[j], lane, ptotal)),
                                     (int32_t)(nabove + wave_exclusive_sum(g[j], lane, ntotal)), 0, 0 };
                sat_eval_walk(&acc, &p[j], &g[j], 1, rocn);
                u2 += acc.u2;
                t2 += acc.t2;
                pabove += ptotal;
                nabove += ntotal;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            u2 += __shfl_down(u2, d);
            t2 += __shfl_down(t2, d);
        }
        out.u2 = u2;
        out.t2 = t2;
        out.positives = (int32_t)pabove;
        out.negatives = (int32_t)nabove;
        out.n_used = rocn < out.negatives ? rocn : out.negatives;
    }
    if (lane == 0) {
        sat_eval *row = rows + q;
        row->u2 = out.u2;
        row->t2 = out.t2;
        row->positives = out.positives;
        row->negatives = out.negatives;
        row->n_used = out.n_used;
        row->query_class = out.query_class;
    }
}

// The checks of a call that reads the tables of the last search, in the order every such call makes them, and nothing
// else: the searched state, installed classes, rocn and the buffers (`buffers`: none is null), then the nodes' range
int check_rows(sat_ctx *ctx, const int32_t *query_node, int rocn, bool buffers)
{
    SAT_TRY(sat_check_searched(ctx));
    SAT_TRY(sat_check_eval_classes(ctx->eval_nodes > 0));
    SAT_TRY(sat_check_eval_args(rocn, buffers));
    SAT_TRY(sat_check_query_nodes((int)ctx->queries.size(), query_node, ctx->eval_nodes));
    if (ctx->max_ordinal >= (uint32_t)ctx->eval_nodes) return sat_fail(SAT_ESTATE, "the classes do not cover the resident database");
    if (ctx->n_entries > 0x7FFFFFFF - kEvalRows) return sat_fail(SAT_EINVAL, "too many entries for the evaluation pass");
    return SAT_OK;
}

// Behind check_rows: every query's table made in ctx->d_eval_tab - zeroed, then counted by eval_histogram, chunk after
// chunk of the queries - and the queries' EvalQuery rows in ctx->d_eval_q.  off: each query's first word, and the total
int make_tables(sat_ctx *ctx, const int32_t *query_node, std::vector<long long> &off)
{
    const int n = ctx->n_entries, nq = (int)ctx->queries.size();
    std::vector<EvalQuery> eq((size_t)nq);
    off.assign((size_t)nq + 1, 0);
    for (int q = 0; q < nq; q++) {
        const int n1 = ctx->queries[(size_t)q].n1;
        eq[(size_t)q] = { off[(size_t)q], n1, query_node[q], ctx->eval_class[(size_t)query_node[q]], 0 };
        off[(size_t)q + 1] = off[(size_t)q] + 2ll * sat_eval_bins(n1);
    }
    const size_t words = (size_t)off[(size_t)nq];
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(ctx->d_eval_tab.grow_after(ctx->stream, words));
    SAT_TRY(ctx->d_eval_q.grow_after(ctx->stream, (size_t)nq * sizeof(EvalQuery)));
    // the host rows die at return: a synchronous copy, behind whatever the stream still holds
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(ctx->d_eval_q.get(), eq.data(), eq.size() * sizeof(EvalQuery), hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(ctx->d_eval_tab.get(), 0, words * sizeof(uint32_t), ctx->stream));
    const EvalQuery *d_eq = reinterpret_cast<const EvalQuery *>(ctx->d_eval_q.get());
    return sat_row_chunks(ctx, kEvalRows, [&](int q0, int, int bpq, dim3 grid) -> int {
        hipLaunchKernelGGL(eval_histogram, grid, dim3(kEvalBlock), 0, ctx->stream, ctx->d_scores.get() + (size_t)q0 * n, n, bpq,
                           d_eq + q0, ctx->d_entry_class.get(), ctx->d_ordinal.get(), ctx->d_eval_tab.get());
        HIP_TRY(hipGetLastError());
        return SAT_OK;
    });
}

}  // namespace

// sat_ctx.hpp: load this file's code object (an empty launch of a small kernel)
int sat_eval_load_code(sat_ctx *ctx)
{
    hipLaunchKernelGGL(eval_entry_classes, dim3(1), dim3(64), 0, ctx->stream, 0, nullptr, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return SAT_OK;
}

// sat_ctx.hpp: the classes go (the caller has waited for the stream, or is about to free the database anyway)
void sat_eval_drop(sat_ctx *ctx)
{
    ctx->eval_nodes = 0;
    ctx->eval_class.clear();
    ctx->d_entry_class.reset();
}

extern "C" {

int sat_eval_classes(sat_ctx *ctx, int n_nodes, const int32_t *node_class)
{
    SAT_TRY(sat_check_context(ctx));
    if (!node_class) {
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        sat_eval_drop(ctx);
        return SAT_OK;
    }
    SAT_TRY(sat_check_uploaded(ctx->n_entries > 0));
    SAT_TRY(sat_check_nodes(n_nodes, ctx->max_ordinal));
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // an earlier class array may still be in use there
    ctx->eval_nodes = 0;
    const int n = ctx->n_entries;
    DevBuf<int32_t> d_node_class;
    SAT_TRY(d_node_class.alloc((size_t)n_nodes));
    SAT_TRY(ctx->d_entry_class.grow((size_t)n));
    HIP_TRY(hipMemcpy(d_node_class.get(), node_class, (size_t)n_nodes * sizeof(int32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(eval_entry_classes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, ctx->d_ordinal.get(),
                       d_node_class.get(), ctx->d_entry_class.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // d_node_class dies at return
    ctx->eval_class.assign(node_class, node_class + n_nodes);
    ctx->eval_nodes = n_nodes;
    return SAT_OK;
}

int sat_eval_rows(sat_ctx *ctx, const int32_t *query_node, int rocn, sat_eval *rows)
{
    SAT_TRY(sat_check_context(ctx));
    SAT_TRY(check_rows(ctx, query_node, rocn, query_node && rows));
    const int nq = (int)ctx->queries.size();
    std::vector<long long> off;
    SAT_TRY(make_tables(ctx, query_node, off));
    SAT_TRY(ctx->d_eval_rows.grow_after(ctx->stream, (size_t)nq));
    hipLaunchKernelGGL(eval_reduce, dim3((unsigned)nq), dim3(64), 0, ctx->stream, reinterpret_cast<const EvalQuery *>(ctx->d_eval_q.get()),
                       ctx->d_eval_tab.get(), rocn, ctx->d_eval_rows.get());
    HIP_TRY(hipGetLastError());
    SAT_TRY(sat_fetch(ctx, rows, ctx->d_eval_rows.get(), (size_t)nq, true));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SAT_OK;
}

int sat_eval_tables(sat_ctx *ctx, const int32_t *query_node, uint32_t *counts, const int64_t *offset)
{
    SAT_TRY(sat_check_context(ctx));
    SAT_TRY(check_rows(ctx, query_node, 1, query_node && counts));
    const int nq = (int)ctx->queries.size();
    std::vector<long long> off;
    SAT_TRY(make_tables(ctx, query_node, off));
    if (!offset) {
        SAT_TRY(sat_fetch(ctx, counts, ctx->d_eval_tab.get(), (size_t)off[(size_t)nq], true));
    } else {
        for (int q = 0; q < nq; q++)
            SAT_TRY(sat_fetch(ctx, counts + offset[q], ctx->d_eval_tab.get() + off[(size_t)q], (size_t)(off[(size_t)q + 1] - off[(size_t)q]), true));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SAT_OK;
}

}  // extern "C"
