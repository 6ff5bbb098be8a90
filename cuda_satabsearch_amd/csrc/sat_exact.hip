// sat_exact.hip - exact search for small queries (sat_search_exact and its results / statistics calls,
// include/satabsearch.h).
//
// The search the context's settings make (plain, or polished where sat_polish_all_set is on) gives every (query, entry)
// row an incumbent: a feasible map and its score.  Behind it exact_pass runs a depth-first branch and bound over the
// feasible maps of every row and replaces a row only by a strictly better map; a row whose walk finished within its
// node budget is proven optimal.  What a unit of the walk is, how the budget is split, the bound and the walk itself
// are host/sat_exact.h, which the host twin (host/sat_exact.c) compiles too.  The SA kernels are not touched: the
// incumbent search is launch_search / sat_polish_all_launch as every other mode calls them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#include "sat_cutoff.hpp"

// the walk with the SA kernel's arithmetic for one cell pair and its triangle index
#define SAT_EXACT_TERM(qd, qc, dd, dc) satk::pair_term(qd, qc, dd, dc)
#define SAT_EXACT_TRI(j, l) satk::tri_index(j, l)
#define SAT_EXACT_WALK_FN __device__ __forceinline__
#include "host/sat_exact.h"

static_assert(SAT_EXACT_QMAX == SAT_EXACT_MAX_QUERY, "the walk's levels are the public limit");
static_assert(sizeof(sat_exact_stat) == 40, "40 bytes a query leave the device");

namespace {

constexpr int kThreads = 128;          // lanes of a workgroup, each with a stack of its own
constexpr int kQueries = 4;            // queries a workgroup serves against its entry

struct ExactArgs {
    const int32_t *entry_list;    // entries of this launch (blockIdx.x)
    const SatQuery *desc;         // the launch's first query descriptor; blockIdx.y picks kQueries of them
    int32_t nq;                   // queries of this launch
    const int32_t *orders;
    const int64_t *cell_off;
    const uint8_t *tab_tri;
    const float *dist_tri;
    int32_t lorder, n2max;        // the LDS carve holds the triangle of an entry of up to n2max SSEs
    unsigned long long max_nodes;
    const int32_t *scores0;       // d_scores: a row's index is its score's
    int32_t *base;                // [rows] the incumbent's score
    uint8_t *unproven;            // [rows]
    uint32_t *nodes;              // [rows] saturating
};

__host__ __device__ inline uint32_t exact_cells(int n2) { return ((uint32_t)n2 * (uint32_t)(n2 + 1) / 2u + 15u) & ~15u; }
// LDS: distances [cells] f32 | query cells [kQueries][16][16] {distance bits, code} | stacks [16][kThreads] u32 (lane-minor) |
// unit scores, unit nodes (bit 31: exhausted) [kQueries * (n2max + 1)] each | codes [cells] | db types [112] |
// query types [kQueries][16] | unit maps [kQueries * (n2max + 1)][16]
__host__ __device__ inline uint32_t exact_lds_bytes(int n2max)
{
    const uint32_t items = (uint32_t)kQueries * (uint32_t)(n2max + 1);
    return exact_cells(n2max) * 5u + kQueries * SAT_EXACT_QMAX * SAT_EXACT_QPITCH * 8u + SAT_EXACT_QMAX * kThreads * 4u + items * 8u + 112u +
           kQueries * SAT_EXACT_QMAX + items * SAT_EXACT_QMAX;
}

// One workgroup per (entry, kQueries queries).  The entry's packed triangle is staged once and cleaned as pair_polish
// cleans it (non-finite distances become the sentinel that never passes the distance test); the queries' dense cells and
// types sit beside it.  The work items are (query slot, unit) in that order, item t on lane t mod kThreads: a lane walks
// its unit with sat_exact_unit - its stack in LDS, level-major and lane-minor, so that the lanes of a wave at one level
// hit different banks - and files the unit's score, nodes and map under the item's index.  Behind a barrier one lane per
// query slot folds the slot's units in unit order (the largest score, the lowest unit among equals) and writes the row:
// always its base score, flag and node count, score and map only where a unit found a strictly better map.  No float
// leaves the pair terms, no atomics: the row is a function of its inputs alone.
__global__ void __launch_bounds__(kThreads) exact_pass(const ExactArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = (int)threadIdx.x;
    const uint32_t cells = exact_cells(a.n2max), items_max = (uint32_t)kQueries * (uint32_t)(a.n2max + 1);
    float *distL = reinterpret_cast<float *>(lds);
    uint32_t *qcellL = reinterpret_cast<uint32_t *>(distL + cells);
    uint32_t *stackL = qcellL + kQueries * SAT_EXACT_QMAX * SAT_EXACT_QPITCH * 2;
    int32_t *uscoreL = reinterpret_cast<int32_t *>(stackL + SAT_EXACT_QMAX * kThreads);
    uint32_t *unodesL = reinterpret_cast<uint32_t *>(uscoreL + items_max);
    uint8_t *codeL = reinterpret_cast<uint8_t *>(unodesL + items_max);
    uint8_t *type2 = codeL + cells;
    uint8_t *qtypeL = type2 + 112;
    uint8_t *umapL = qtypeL + kQueries * SAT_EXACT_QMAX;

    const int e = a.entry_list[blockIdx.x], n2 = a.orders[e];
    const int q0 = (int)blockIdx.y * kQueries, nqs = min(kQueries, a.nq - q0);
    const bool sane = n2 >= 1 && n2 <= a.n2max && nqs >= 1;
    uint32_t present = 0;
    if (sane) {
        const uint8_t *tt = a.tab_tri + a.cell_off[e];
        const float *dd = a.dist_tri + a.cell_off[e];
        const int ncell = (n2 * (n2 + 1)) >> 1;
        for (int c = tid; c < ncell; c += kThreads) {
            const float v = dd[c];
            distL[c] = fabsf(v) <= 3.0e38f ? v : SAT_K_DSENT;
            codeL[c] = tt[c];
        }
        for (int j = tid; j < n2; j += kThreads) type2[j] = tt[((j * (j + 1)) >> 1) + j] & 3u;
        for (int s = 0; s < nqs; s++) {
            const SatQuery Q = a.desc[q0 + s];
            const int n1 = min(Q.n1, SAT_EXACT_QMAX);          // (the host refuses longer queries before any launch)
            for (int x = tid; x < n1 * n1; x += kThreads) {
                const int i = x / n1, k = x - i * n1;
                const uint2 cell = Q.qpair[i * SAT_EXACT_QPITCH + k];
                qcellL[2 * ((s * SAT_EXACT_QMAX + i) * SAT_EXACT_QPITCH + k)] = cell.x;
                qcellL[2 * ((s * SAT_EXACT_QMAX + i) * SAT_EXACT_QPITCH + k) + 1] = cell.y;
            }
            for (int i = tid; i < n1; i += kThreads) qtypeL[s * SAT_EXACT_QMAX + i] = Q.qtypes[i];
        }
    }
    __syncthreads();
    if (sane) {
        for (int j = 0; j < n2; j++) present |= 1u << type2[j];
        const int units = sat_exact_units(0, n2, a.lorder), items = nqs * units;
        for (int t = tid; t < items; t += kThreads) {
            const int s = t / units, u = t - s * units;
            const SatQuery Q = a.desc[q0 + s];
            sat_exact_view v;
            v.n1 = min(Q.n1, SAT_EXACT_QMAX);
            v.n2 = n2;
            v.lorder = a.lorder;
            v.present = present;
            v.qcell = qcellL + 2 * s * SAT_EXACT_QMAX * SAT_EXACT_QPITCH;
            v.qtypes = qtypeL + s * SAT_EXACT_QMAX;
            v.dist = distL;
            v.code = codeL;
            v.type2 = type2;
            sat_exact_unit_result r;
            sat_exact_unit(&v, u, sat_exact_share(a.max_nodes, units, u), Q.scores[e], stackL + tid, kThreads,
                           umapL + (size_t)t * SAT_EXACT_QMAX, &r);
            uscoreL[t] = r.score;
            // (bit 31 is free: a share reaches 2^31 only for an entry of one SSE, whose walks end after a few nodes)
            unodesL[t] = r.nodes | (r.exhausted ? 0x80000000u : 0u);
        }
    }
    __syncthreads();
    if (sane && tid < nqs) {
        const SatQuery Q = a.desc[q0 + tid];
        const int n1 = min(Q.n1, SAT_EXACT_QMAX), units = sat_exact_units(0, n2, a.lorder);
        const int32_t inc = Q.scores[e];
        int32_t best = inc, win = -1;
        uint32_t flag = 0;
        unsigned long long total = 0ull;
        for (int u = 0; u < units; u++) {
            const int t = tid * units + u;
            const int32_t sc = uscoreL[t];
            const uint32_t nd = unodesL[t];
            total += nd & 0x7FFFFFFFu;
            flag |= nd >> 31;
            if (sc != SAT_EXACT_NONE && sc > best) {
                best = sc;
                win = u;
            }
        }
        const size_t row = (size_t)(Q.scores - a.scores0) + (size_t)e;
        a.base[row] = inc;
        a.unproven[row] = (uint8_t)flag;
        a.nodes[row] = total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)total;
        if (win >= 0) {
            Q.scores[e] = best;
            if (Q.ssemaps) {
                const uint8_t *wm = umapL + (size_t)(tid * units + win) * SAT_EXACT_QMAX;
                int8_t *dst = Q.ssemaps + (size_t)e * (size_t)n1;
                for (int i = 0; i < n1; i++) dst[i] = (int8_t)((int)wm[i] - 1);
            }
        }
    }
}

// One workgroup per query: its rows' statistics summed with integer atomics in LDS, 40 bytes out.
__global__ void __launch_bounds__(256) exact_stats(int n, const int32_t *scores, const int32_t *base, const uint8_t *unproven,
                                                   const uint32_t *nodes, sat_exact_stat *out)
{
    __shared__ unsigned long long acc[4];
    const int q = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (tid < 4) acc[tid] = 0ull;
    __syncthreads();
    unsigned long long proven = 0ull, improved = 0ull, gain = 0ull, nd = 0ull;
    for (int e = tid; e < n; e += 256) {
        const size_t row = (size_t)q * (size_t)n + (size_t)e;
        const int32_t d = scores[row] - base[row];
        proven += unproven[row] ? 0u : 1u;
        improved += d > 0 ? 1u : 0u;
        gain += (unsigned long long)(d > 0 ? d : 0);
        nd += nodes[row];
    }
    atomicAdd(&acc[0], proven);
    atomicAdd(&acc[1], improved);
    atomicAdd(&acc[2], gain);
    atomicAdd(&acc[3], nd);
    __syncthreads();
    if (tid == 0 && out) {
        sat_exact_stat s;
        s.rows = n;
        s.proven = (int64_t)acc[0];
        s.improved = (int64_t)acc[1];
        s.gain = (int64_t)acc[2];
        s.nodes = acc[3];
        out[q] = s;
    }
}

bool exact_state(const sat_ctx *ctx)
{
    return ctx->n_entries > 0 && !ctx->queries.empty() && ctx->searched_exact && ctx->searched_nq == ctx->queries.size() &&
           ctx->d_xbase.get();
}

}  // namespace

// ---------------------------------------------------------------- launch code (sat_ctx.hpp)

// the refusals of sat_search_exact, all SAT_EINVAL, all before anything is queued or changed
int sat_exact_check(const sat_ctx *ctx, int maxstart, unsigned long long max_nodes)
{
    SAT_TRY(sat_check_context(ctx));
    if (ctx->n_entries <= 0) return sat_fail(SAT_EINVAL, "exact search: no database uploaded");
    if (ctx->queries.empty()) return sat_fail(SAT_EINVAL, "exact search: no query set");
    if (maxstart < 1) return sat_fail(SAT_EINVAL, "maxstart must be >= 1 (got %d)", maxstart);
    if (max_nodes < 1ull || max_nodes > (1ull << 32))
        return sat_fail(SAT_EINVAL, "max_nodes must be 1..2^32 (got %llu)", max_nodes);
    for (size_t q = 0; q < ctx->queries.size(); q++)
        if (ctx->queries[q].n1 > SAT_EXACT_MAX_QUERY)
            return sat_fail(SAT_EINVAL, "exact search: query %zu has %d SSEs, the limit is %d", q, ctx->queries[q].n1, SAT_EXACT_MAX_QUERY);
    return SAT_OK;
}

// Queue the incumbent search and the proof pass on the context's stream.  The pass is cut into launches by summed
// budget: the rows of a launch may expand at most `scratch budget in bytes` nodes together (2^30 unless SAT_EXP_SCRATCH_KB
// says otherwise: 4096 rows at the default max_nodes), and no launch crosses an order bucket, so that each sizes its LDS
// for its own bucket.  The cut cannot show in a row: rows share nothing.
int sat_exact_launch(sat_ctx *ctx, int lorder, int maxstart, unsigned long long max_nodes)
{
    SAT_TRY(sat_exact_check(ctx, maxstart, max_nodes));
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(ctx->polish_all ? sat_polish_all_launch(ctx, lorder, 1, maxstart) : launch_search(ctx, lorder, 1, maxstart, ctx->stream));
    if (ctx->polish_all) SAT_TRY(sat_polish_all_check(ctx));
    const std::string incumbent_info = ctx->last_launch_info;
    const size_t nq = ctx->queries.size(), N = (size_t)ctx->n_entries, rows = nq * N;
    SAT_TRY(ctx->d_xbase.grow_after(ctx->stream, std::max(rows, ctx->d_scores.capacity())));
    SAT_TRY(ctx->d_xflag.grow_after(ctx->stream, rows));
    SAT_TRY(ctx->d_xnodes.grow_after(ctx->stream, rows));

    ExactArgs a{};
    a.orders = ctx->d_orders.get();
    a.cell_off = ctx->d_cell_off.get();
    a.tab_tri = ctx->d_tab.get();
    a.dist_tri = ctx->d_dist.get();
    a.lorder = lorder ? 1 : 0;
    a.max_nodes = max_nodes;
    a.scores0 = ctx->d_scores.get();
    a.base = ctx->d_xbase.get();
    a.unproven = ctx->d_xflag.get();
    a.nodes = ctx->d_xnodes.get();
    // every query is of size class 16, so the descriptors stand in input order from class_begin[0]
    const SatQuery *desc = ctx->d_qdesc.get() + ctx->class_begin[0];
    const unsigned long long launch_nodes = std::max<unsigned long long>((unsigned long long)ctx->tune.scratch_bytes, 1ull);
    const size_t launch_rows = (size_t)std::max<unsigned long long>(launch_nodes / max_nodes, 1ull);
    const size_t qn_max = std::min<size_t>(std::min(nq, launch_rows), (size_t)65535 * kQueries);
    const size_t en_max = std::max<size_t>(launch_rows / qn_max, 1);
    size_t launches = 0;
    for (int b = 0; b < kNumBuckets; b++) {
        const int begin = ctx->bucket_begin[b], count = ctx->bucket_begin[b + 1] - begin;
        if (count == 0) continue;
        a.n2max = ctx->bucket_n2max[b];
        const uint32_t lds = exact_lds_bytes(a.n2max);
        for (size_t qa = 0; qa < nq; qa += qn_max) {
            const size_t qn = std::min(qn_max, nq - qa);
            for (size_t e0 = 0; e0 < (size_t)count; e0 += en_max, launches++) {
                const size_t en = std::min(en_max, (size_t)count - e0);
                a.entry_list = ctx->d_lists.get() + begin + e0;
                a.desc = desc + qa;
                a.nq = (int32_t)qn;
                hipLaunchKernelGGL(exact_pass, dim3((unsigned)en, (unsigned)((qn + kQueries - 1) / kQueries)), dim3(kThreads), lds, ctx->stream, a);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    ctx->searched_exact = true;                          // (the incumbent search set the rest of the searched state)
    char tail[160];
    snprintf(tail, sizeof tail, " | exact pass (%llu nodes a row, %zu launches of up to %zu rows)", max_nodes, launches, qn_max * en_max);
    ctx->last_launch_info = incumbent_info + tail;
    return SAT_OK;
}

// load this file's code object (an empty launch of a small kernel)
int sat_exact_load_code(sat_ctx *ctx)
{
    hipLaunchKernelGGL(exact_stats, dim3(1), dim3(256), 0, ctx->stream, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return SAT_OK;
}

int sat_exact_check_state(const sat_ctx *ctx)
{
    SAT_TRY(sat_check_context(ctx));
    return exact_state(ctx) ? SAT_OK : sat_fail(SAT_EINVAL, "the last search was not an exact one (sat_search_exact)");
}

extern "C" {

int sat_search_exact(sat_ctx *ctx, int lorder, int maxstart, unsigned long long max_nodes, double *kernel_ms)
{
    SAT_TRY(sat_exact_check(ctx, maxstart, max_nodes));
    return timed(ctx, kernel_ms, [&] { return sat_exact_launch(ctx, lorder, maxstart, max_nodes); });
}

int sat_exact_results(sat_ctx *ctx, int32_t *base_scores, uint8_t *unproven, uint32_t *nodes)
{
    SAT_TRY(sat_exact_check_state(ctx));
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t rows = ctx->queries.size() * (size_t)ctx->n_entries;
    if (base_scores) SAT_TRY(sat_fetch(ctx, base_scores, (const int32_t *)ctx->d_xbase.get(), rows));
    if (unproven) SAT_TRY(sat_fetch(ctx, unproven, (const uint8_t *)ctx->d_xflag.get(), rows));
    if (nodes) SAT_TRY(sat_fetch(ctx, nodes, (const uint32_t *)ctx->d_xnodes.get(), rows));
    return SAT_OK;
}

int sat_exact_stats(sat_ctx *ctx, sat_exact_stat *per_query)
{
    SAT_TRY(sat_exact_check_state(ctx));
    if (!per_query) return sat_fail(SAT_EINVAL, "per_query buffer is null");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t nq = ctx->queries.size();
    SAT_TRY(ctx->d_xstats.grow_after(ctx->stream, nq));
    hipLaunchKernelGGL(exact_stats, dim3((unsigned)nq), dim3(256), 0, ctx->stream, ctx->n_entries, (const int32_t *)ctx->d_scores.get(),
                       (const int32_t *)ctx->d_xbase.get(), (const uint8_t *)ctx->d_xflag.get(), (const uint32_t *)ctx->d_xnodes.get(),
                       ctx->d_xstats.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return sat_fetch(ctx, per_query, (const sat_exact_stat *)ctx->d_xstats.get(), nq);
}

}  // extern "C"
