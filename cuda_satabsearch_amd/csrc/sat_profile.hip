// sat_profile.hip - a query's SSEs profiled over its hits, on the device (sat_profile_rows).
//
// Row (q, e) of the last search COUNTS iff cutoff_row of sat_hitrow.hpp passes it - the predicate of sat_hits_cutoff,
// sat_cluster_add and sat_cover_add, the same double from the same table index - and the entry is not the query's own
// node.  For every query of order n1 the pass keeps hits[q], the counted rows, and joint[q][i][k], the counted rows
// whose map matches SSE i and SSE k (map[i] >= 0 and map[k] >= 0); the diagonal is the rows that match SSE i at all.
// Every counter is a uint32 that only integer atomic adds touch, so the numbers are a property of the row SET: the
// launch shape, the chunks of the query list, the batches, the order of the calls and the sharding cannot show in them.
//
// profile_add walks the rows as cluster_add does, a block of 1024 rows of one query.  The waves transpose their rows'
// maps with ballots - M[wave][i] is the 64-bit set of the wave's rows that match SSE i - and the block's threads then
// take the pairs i <= k, one popcount of an AND per wave and pair, ONE atomic per pair and block.  The device keeps the
// matrix full, [n1][n1] words a query, but profile_add writes its UPPER triangle only; profile_mirror copies it below
// the diagonal before the matrices leave.  No loop here has a bound other than n1, the 16 waves or the matrix size, and
// nothing waits for another thread but at the block's barriers, which every thread of a block reaches or none does.
#include <hip/hip_runtime.h>

#include <vector>

#include "sat_ctx.hpp"
#include "sat_cutoff.hpp"
#include "sat_hitrow.hpp"

namespace {

typedef unsigned long long u64;

// a query's row for the kernels: the first word of its matrix behind the hits in ctx->d_profile, its own node (< 0: none)
struct ProfileQuery {
    long long off;
    int32_t node;
    int32_t pad;
};

// One thread per row, the grid of cluster_add.  `queries`, `pq` and `hits` are the chunk's; `joint` is the whole call's.
__global__ void __launch_bounds__(kCutoffBlock) profile_add(const int32_t *scores, int n, int bpq, const int32_t *orders,
                                                             const HitQuery *queries, const double *ztab, const double *ptab,
                                                             double max_p, const ProfileQuery *pq, const uint32_t *ordinal,
                                                             uint32_t *hits, uint32_t *joint)
{
    __shared__ u64 wave_rows[kCutoffWaves];                     // the wave's counted rows
    __shared__ u64 M[kCutoffWaves][SAT_MAXDIM];                 // M[w][i]: those of them that match SSE i
    int q, e;
    int32_t score = 0;
    bool counted = cutoff_row(scores, n, bpq, orders, queries, ztab, ptab, max_p, q, e, score);
    if (counted) {
        const int32_t node = pq[q].node;
        counted = node < 0 || (int32_t)ordinal[e] != node;      // a structure is no hit of itself
    }
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const u64 rows = __ballot(counted);
    if (lane == 0) wave_rows[wave] = rows;
    block_count(counted, [&](int32_t c) { atomicAdd(hits + q, (uint32_t)c); });
    // behind block_count's barrier: every wave's set is there.  The same 16 words for every thread of the block, so the
    // whole block leaves here or none of it - the common case at a useful cutoff
    u64 any = 0ull;
#pragma unroll
    for (int w = 0; w < kCutoffWaves; w++) any |= wave_rows[w];
    if (!any) return;
    const int n1 = queries[q].n1;
    if (rows) {                                                 // the wave's own ballot: a wave with no counted row skips its maps
        const int8_t *map = queries[q].ssemaps + (size_t)e * n1;        // read only where counted: e < n there
        for (int i = 0; i < n1; i++) {
            const u64 matched = __ballot(counted && map[i] >= 0);
            if (lane == 0) M[wave][i] = matched;
        }
    }
    __syncthreads();
    uint32_t *mine = joint + pq[q].off;
    for (int cell = (int)threadIdx.x; cell < n1 * n1; cell += kCutoffBlock) {
        const int i = cell / n1, k = cell - i * n1;
        if (i > k) continue;
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < kCutoffWaves; w++)
            if (wave_rows[w]) c += (uint32_t)__popcll(M[w][i] & M[w][k]);   // a wave that skipped left its M unwritten
        if (c) atomicAdd(mine + cell, c);
    }
}

// One block per query, behind every profile_add of the call: the upper triangle copied below the diagonal
__global__ void profile_mirror(int nq, const HitQuery *queries, const ProfileQuery *pq, uint32_t *joint)
{
    const int q = (int)blockIdx.x;
    if (q >= nq) return;
    const int n1 = queries[q].n1;
    uint32_t *mine = joint + pq[q].off;
    for (int cell = (int)threadIdx.x; cell < n1 * n1; cell += (int)blockDim.x) {
        const int i = cell / n1, k = cell - i * n1;
        if (i > k) mine[cell] = mine[k * n1 + i];
    }
}

}  // namespace

// sat_ctx.hpp: load this file's code object (an empty launch of a small kernel)
int sat_profile_load_code(sat_ctx *ctx)
{
    hipLaunchKernelGGL(profile_mirror, dim3(1), dim3(64), 0, ctx->stream, 0, nullptr, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return SAT_OK;
}

// sat_cutoff.hpp: the checks of sat_profile_rows, nothing else
int sat_profile_check(sat_ctx *ctx, double max_pvalue, const uint32_t *hits, const uint32_t *joint)
{
    SAT_TRY(sat_check_searched(ctx));
    SAT_TRY(sat_check_lsoln(ctx->searched_lsoln));
    if (!hits || !joint) return sat_fail(SAT_EINVAL, "null array");
    return sat_check_pvalue(max_pvalue);
}

extern "C" int sat_profile_rows(sat_ctx *ctx, double max_pvalue, const int32_t *query_node, uint32_t *hits, uint32_t *joint,
                                const int64_t *offset)
{
    SAT_TRY(sat_check_context(ctx));
    SAT_TRY(sat_profile_check(ctx, max_pvalue, hits, joint));
    const int n = ctx->n_entries, nq = (int)ctx->queries.size();
    // d_profile: hits [nq], then the matrices packed in query order
    std::vector<ProfileQuery> pq((size_t)nq);
    long long words = nq;
    for (int q = 0; q < nq; q++) {
        const long long n1 = ctx->queries[(size_t)q].n1;
        pq[(size_t)q] = { words - nq, query_node ? query_node[q] : -1, 0 };
        words += n1 * n1;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(ctx->d_profile.grow_after(ctx->stream, (size_t)words));
    SAT_TRY(ctx->d_profile_q.grow_after(ctx->stream, (size_t)nq * sizeof(ProfileQuery)));
    // the host rows die at return: a synchronous copy, ordered behind the stream by sat_hitq_upload's wait
    SAT_TRY(sat_hitq_upload(ctx, true));
    HIP_TRY(hipMemcpy(ctx->d_profile_q.get(), pq.data(), pq.size() * sizeof(ProfileQuery), hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(ctx->d_profile.get(), 0, (size_t)words * sizeof(uint32_t), ctx->stream));
    const HitQuery *hq = hit_queries(ctx);
    const ProfileQuery *d_pq = reinterpret_cast<const ProfileQuery *>(ctx->d_profile_q.get());
    uint32_t *d_hits = ctx->d_profile.get(), *d_joint = d_hits + nq;
    SAT_TRY(sat_row_chunks(ctx, kCutoffBlock, [&](int q0, int, int bpq, dim3 grid) -> int {
        hipLaunchKernelGGL(profile_add, grid, dim3(kCutoffBlock), 0, ctx->stream, ctx->d_scores.get() + (size_t)q0 * n, n, bpq,
                           ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(), max_pvalue, d_pq + q0,
                           ctx->d_ordinal.get(), d_hits + q0, d_joint);
        HIP_TRY(hipGetLastError());
        return SAT_OK;
    }));
    hipLaunchKernelGGL(profile_mirror, dim3((unsigned)nq), dim3(256), 0, ctx->stream, nq, hq, d_pq, d_joint);
    HIP_TRY(hipGetLastError());
    SAT_TRY(sat_fetch(ctx, hits, d_hits, (size_t)nq, true));
    if (!offset) {
        SAT_TRY(sat_fetch(ctx, joint, d_joint, (size_t)(words - nq), true));
    } else {
        for (int q = 0; q < nq; q++) {
            const size_t n1 = (size_t)ctx->queries[(size_t)q].n1;
            SAT_TRY(sat_fetch(ctx, joint + offset[q], d_joint + pq[(size_t)q].off, n1 * n1, true));
        }
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SAT_OK;
}
