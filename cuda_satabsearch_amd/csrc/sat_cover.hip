// sat_cover.hip - clustering the database around representatives, on the device (sat_cover_*).
//
// Nodes are the structures of the whole database in file order.  Row (q, e) of the last search is the UNDIRECTED edge
// {query_node[q], ordinal[e]} iff cutoff_row of sat_hitrow.hpp passes it - the predicate of sat_hits_cutoff and
// sat_cluster_add - and the two differ.  cover_add walks the rows as cluster_add does and keeps the graph itself: an
// adjacency BIT matrix, nodes rows of `stride` 64-bit words (host/sat_cover.h has the layout), written by integer atomic
// OR only.  A bit is set or it is not, so the matrix is a property of the edge SET: the launch shape, the batches, the
// order of the calls, repeats, the two directions of a pair and the sharding cannot show in it.
//
// The solve is the greedy cover of host/sat_cover.h, a round at a time, two kernels a round:
//   cover_gain   one wave per unassigned row: gain = 1 + popcount(row & unassigned); a block's best, when it is above 1,
//                goes into ONE 64-bit atomicMax on the round's key (sat_cover_key: the tie rule is in the packing)
//   cover_apply  one block: reads the key; none posted - every gain is 1 - sets `done`; else the winner and its
//                unassigned neighbours get their rep and leave `unassigned`, the round is counted, the key re-armed
// Only kernel boundaries carry values between the phases: no kernel reads what another block of the same launch wrote,
// but for the atomic on the key itself, and nothing spins.  Rounds are queued kRoundBatch at a time; the host looks at
// `done` once per batch; a round after `done` is two launches that return at once.
#include <hip/hip_runtime.h>

#include <string>

#include "sat_ctx.hpp"
#include "sat_cutoff.hpp"
#include "sat_hitrow.hpp"
#include "host/sat_cover.h"

namespace {

typedef unsigned long long u64;

// the words of ctx->d_cv_state
enum { kKey = 0, kDone, kRounds, kDegreeSum, kBroken, kStateWords };
constexpr int kRoundBatch = SAT_COVER_ROUND_BATCH;
constexpr int kRowWaves = 4;                    // rows (waves) per block of the row kernels

__device__ __forceinline__ u64 wave_or(u64 x)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x |= __shfl_xor(x, d);
    return x;
}

__device__ __forceinline__ int32_t wave_sum(int32_t x)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// One thread per row, the grid of cluster_add.  A qualifying row that is no self row sets bit a of row b and bit b of
// row a, a = the query's node, b = the entry's.  Bit a of row b: the lanes' rows b differ, one atomic each.  Bit b of
// row a: a block holds rows of one query, so every lane of the wave writes row a, and entries next to each other mostly
// have ordinals next to each other: the lanes whose bits share a word are peeled off group by group (the first live
// lane's word, a ballot of the lanes that share it, a wave-wide OR of their bits) and ONE lane issues the group's atomic.
// After kPeel groups whatever is left goes lane by lane - ordinals in no order at all would otherwise cost 64 turns.
// -DSAT_COVER_PEEL=0 compiles the combining out (scripts/cover_cost.py measures both).
#ifndef SAT_COVER_PEEL
#define SAT_COVER_PEEL 4
#endif
constexpr int kPeel = SAT_COVER_PEEL;
__global__ void __launch_bounds__(kCutoffBlock) cover_add(const int32_t *scores, int n, int bpq, const int32_t *orders,
                                                           const HitQuery *queries, const double *ztab, const double *ptab,
                                                           double max_p, const int32_t *query_node, const uint32_t *ordinal,
                                                           size_t stride, u64 *adj)
{
    int q, e;
    int32_t score = 0;
    bool edge = cutoff_row(scores, n, bpq, orders, queries, ztab, ptab, max_p, q, e, score);
    const int32_t a = query_node[q];                                    // both < the accumulator's nodes: checked on the host
    int32_t b = 0;
    if (edge) {
        b = (int32_t)ordinal[e];
        edge = a != b;
    }
    if (edge) atomicOr(adj + (size_t)b * stride + sat_cover_word(a), sat_cover_bit(a));
    u64 *row = adj + (size_t)a * stride;
    const size_t word = sat_cover_word(b);
    const u64 bit = sat_cover_bit(b);
    const int lane = (int)(threadIdx.x & 63);
    u64 todo = __ballot(edge);
    for (int turn = 0; turn < kPeel && todo; turn++) {                  // todo is the wave's: every lane takes every turn
        const int lead = __ffsll((long long)todo) - 1;
        const size_t w = (size_t)__shfl((unsigned long long)word, lead);
        const bool mine = edge && ((todo >> lane) & 1ull) && word == w;
        const u64 bits = wave_or(mine ? bit : 0ull);
        if (lane == lead) atomicOr(row + w, bits);
        todo &= ~__ballot(mine);
    }
    if (edge && ((todo >> lane) & 1ull)) atomicOr(row + word, bit);
}

// a solve starts: every node unassigned and its own representative, the state words zero
__global__ void cover_reset(int nodes, size_t stride, u64 *un, int32_t *rep, u64 *state)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < kStateWords) state[i] = 0ull;
    if (i < stride) un[i] = sat_cover_valid(nodes, i);
    if (i < (size_t)nodes) rep[i] = (int32_t)i;
}

// One wave per row: degree[v] = popcount(row v); the block's sum into ONE atomic on the degree sum (twice the edges)
__global__ void __launch_bounds__(64 * kRowWaves) cover_degree(int nodes, size_t stride, const u64 *adj, int32_t *degree, u64 *state)
{
    __shared__ int32_t wave_deg[kRowWaves];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int v = (int)blockIdx.x * kRowWaves + wave;
    int32_t d = 0;
    if (v < nodes) {
        const u64 *row = adj + (size_t)v * stride;
        for (size_t w = (size_t)lane; w < stride; w += 64) d += __popcll(row[w]);
        d = wave_sum(d);
        if (lane == 0) degree[v] = d;
    }
    if (lane == 0) wave_deg[wave] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 sum = 0ull;
        for (int w = 0; w < kRowWaves; w++) sum += (u64)wave_deg[w];
        if (sum) atomicAdd(state + kDegreeSum, sum);
    }
}

// A round's first half.  One wave per row; a row that is assigned, or a round after `done`, does nothing.  `done` and
// `unassigned` were written by earlier launches, the key only through atomics
__global__ void __launch_bounds__(64 * kRowWaves) cover_gain(int nodes, size_t stride, const u64 *adj, const u64 *un, u64 *state)
{
    __shared__ u64 wave_key[kRowWaves];
    if (state[kDone]) return;                                           // the whole block: before any barrier
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int v = (int)blockIdx.x * kRowWaves + wave;
    u64 key = 0ull;
    if (v < nodes && (un[sat_cover_word(v)] & sat_cover_bit(v))) {
        const u64 *row = adj + (size_t)v * stride;
        int32_t c = 0;
        for (size_t w = (size_t)lane; w < stride; w += 64) c += __popcll(row[w] & un[w]);
        c = wave_sum(c);
        if (c > 0) key = sat_cover_key((uint32_t)c + 1u, v);            // gain 1 posts nothing: the key stays 0
    }
    if (lane == 0) wave_key[wave] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 best = 0ull;
        for (int w = 0; w < kRowWaves; w++) best = wave_key[w] > best ? wave_key[w] : best;
        if (best) atomicMax(state + kKey, best);
    }
}

// A round's second half, ONE block.  Thread t owns the words t, t + blockDim.x, ... of `unassigned`: no word has two
// writers.  Every thread has read the key before thread 0 re-arms it (the barrier)
constexpr int kApplyBlock = 1024;
__global__ void __launch_bounds__(kApplyBlock) cover_apply(size_t stride, const u64 *adj, u64 *un, int32_t *rep, u64 *state)
{
    if (state[kDone]) return;
    const u64 key = state[kKey];
    __syncthreads();
    if (key == 0ull) {
        if (threadIdx.x == 0) state[kDone] = 1ull;
        return;
    }
    const int32_t best = sat_cover_key_node(key);
    const u64 *row = adj + (size_t)best * stride;
    for (size_t w = threadIdx.x; w < stride; w += kApplyBlock) {
        u64 members = row[w] & un[w];
        if (w == sat_cover_word(best)) members |= sat_cover_bit(best);  // a row does not hold its own node
        if (!members) continue;
        un[w] &= ~members;
        for (u64 x = members; x; x &= x - 1ull) rep[(int32_t)(w << 6) + __ffsll((long long)x) - 1] = best;
    }
    if (threadIdx.x == 0) {
        state[kKey] = 0ull;
        state[kRounds] += 1ull;
    }
}

// After the rounds: the representatives as a bit mask (a node is one iff rep[v] == v) ...
__global__ void cover_rep_mask(int nodes, size_t stride, const int32_t *rep, u64 *mask)
{
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= stride) return;
    u64 m = 0ull;
    for (int i = 0; i < 64; i++) {
        const size_t v = (w << 6) + (size_t)i;
        if (v < (size_t)nodes && rep[v] == (int32_t)v) m |= 1ull << i;
    }
    mask[w] = m;
}

// ... and the two invariants, one wave per row: a member is adjacent to its representative, a representative to no
// representative.  Counts what breaks either; the host refuses a result whose count is not 0
__global__ void __launch_bounds__(64 * kRowWaves) cover_check(int nodes, size_t stride, const u64 *adj, const int32_t *rep, const u64 *mask,
                                                                u64 *state)
{
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int v = (int)blockIdx.x * kRowWaves + wave;
    if (v >= nodes) return;
    const u64 *row = adj + (size_t)v * stride;
    const int32_t r = rep[v];
    int32_t broken = 0;
    if (r == v) {
        for (size_t w = (size_t)lane; w < stride; w += 64) broken += __popcll(row[w] & mask[w]);
        broken = wave_sum(broken);
    } else if (lane == 0) {
        broken = r < 0 || r >= nodes || !(row[sat_cover_word(r)] & sat_cover_bit(r)) || rep[r] != r;
    }
    if (lane == 0 && broken) atomicAdd(state + kBroken, (u64)broken);
}

// rows |= more, `words` words: the shards' matrices onto one
__global__ void cover_or(size_t words, u64 *rows, const u64 *more)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words && more[i]) rows[i] |= more[i];
}

int check_accumulator(const sat_ctx *ctx)
{
    SAT_TRY(sat_check_context(ctx));
    if (ctx->cover_nodes <= 0)
        return sat_fail(SAT_ESTATE, "no cover accumulator (sat_cover_begin has not been called since the last database upload)");
    return SAT_OK;
}

unsigned row_blocks(int nodes) { return (unsigned)((nodes + kRowWaves - 1) / kRowWaves); }

}  // namespace

// sat_ctx.hpp: load this file's code object (an empty launch of a small kernel)
int sat_cover_load_code(sat_ctx *ctx)
{
    hipLaunchKernelGGL(cover_or, dim3(1), dim3(64), 0, ctx->stream, (size_t)0, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return SAT_OK;
}

// sat_ctx.hpp: the accumulator goes (the caller has waited for the stream, or is about to free the database anyway)
void sat_cover_drop(sat_ctx *ctx)
{
    ctx->cover_nodes = 0;
    ctx->d_cv_adj.reset();
    ctx->d_cv_mask.reset();
    ctx->d_cv_out.reset();
    ctx->d_cv_state.reset();
}

// sat_ctx.hpp, for sat_multi_cover_solve: rows row0 .. row0 + rows - 1 of the matrix to the host (counted) ...
int sat_cover_rows_fetch(sat_ctx *ctx, int row0, int rows, unsigned long long *host)
{
    SAT_TRY(check_accumulator(ctx));
    const size_t stride = sat_cover_stride(ctx->cover_nodes);
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(sat_fetch(ctx, host, ctx->d_cv_adj.get() + (size_t)row0 * stride, (size_t)rows * stride, true));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SAT_OK;
}

// ... and ORed into the same rows of this context's matrix.  The staging buffer lives for the call
int sat_cover_rows_or(sat_ctx *ctx, int row0, int rows, const unsigned long long *host)
{
    SAT_TRY(check_accumulator(ctx));
    const size_t stride = sat_cover_stride(ctx->cover_nodes), words = (size_t)rows * stride;
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<u64> staged;
    SAT_TRY(staged.alloc(words));
    HIP_TRY(hipMemcpyAsync(staged.get(), host, words * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(cover_or, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, ctx->stream, words,
                       ctx->d_cv_adj.get() + (size_t)row0 * stride, staged.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // `staged` and the caller's rows die at return
    return SAT_OK;
}

extern "C" {

int sat_cover_begin(sat_ctx *ctx, int n_nodes)
{
    SAT_TRY(sat_check_context(ctx));
    SAT_TRY(sat_check_uploaded(ctx->n_entries > 0));
    SAT_TRY(sat_check_nodes(n_nodes, ctx->max_ordinal));
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // an earlier accumulator may still be in use there
    ctx->cover_nodes = 0;
    const size_t stride = sat_cover_stride(n_nodes), words = (size_t)n_nodes * stride;
    // the matrix is the one buffer that may not fit: its failure says what was asked for
    const int rc = ctx->d_cv_adj.grow(words);
    if (rc != SAT_OK) {
        const std::string why = sat_last_error();
        return sat_fail(rc, "the adjacency matrix of %d nodes needs %zu bytes: %s", n_nodes, words * sizeof(u64), why.c_str());
    }
    SAT_TRY(ctx->d_cv_mask.grow(2 * stride));               // unassigned, then the representatives' mask
    SAT_TRY(ctx->d_cv_out.grow(2 * (size_t)n_nodes));       // rep [n_nodes], then degree [n_nodes]
    SAT_TRY(ctx->d_cv_state.grow(kStateWords));
    HIP_TRY(hipMemsetAsync(ctx->d_cv_adj.get(), 0, words * sizeof(u64), ctx->stream));
    ctx->cover_nodes = n_nodes;
    return SAT_OK;
}

int sat_cover_add(sat_ctx *ctx, double max_pvalue, const int32_t *query_node)
{
    SAT_TRY(check_accumulator(ctx));
    SAT_TRY(sat_check_searched(ctx));
    if (!query_node) return sat_fail(SAT_EINVAL, "query_node is null");
    SAT_TRY(sat_check_pvalue(max_pvalue));
    const int n = ctx->n_entries, nq = (int)ctx->queries.size(), nodes = ctx->cover_nodes;
    SAT_TRY(sat_check_query_nodes(nq, query_node, nodes));
    if (ctx->max_ordinal >= (uint32_t)nodes) return sat_fail(SAT_ESTATE, "the accumulator does not cover the resident database");
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(ctx->d_cv_qnode.grow_after(ctx->stream, (size_t)nq));
    // the caller's array may go at return: a synchronous copy, ordered behind the stream by sat_hitq_upload's wait
    SAT_TRY(sat_hitq_upload(ctx, false));
    HIP_TRY(hipMemcpy(ctx->d_cv_qnode.get(), query_node, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice));
    const HitQuery *hq = hit_queries(ctx);
    const size_t stride = sat_cover_stride(nodes);
    return sat_row_chunks(ctx, kCutoffBlock, [&](int q0, int, int bpq, dim3 grid) -> int {
        hipLaunchKernelGGL(cover_add, grid, dim3(kCutoffBlock), 0, ctx->stream, ctx->d_scores.get() + (size_t)q0 * n, n, bpq,
                           ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(), max_pvalue,
                           ctx->d_cv_qnode.get() + q0, ctx->d_ordinal.get(), stride, ctx->d_cv_adj.get());
        HIP_TRY(hipGetLastError());
        return SAT_OK;
    });
}

int sat_cover_solve(sat_ctx *ctx, int32_t *rep, int32_t *degree, unsigned long long *edges, int *rounds)
{
    SAT_TRY(check_accumulator(ctx));
    if (!rep) return sat_fail(SAT_EINVAL, "rep buffer is null");
    const int nodes = ctx->cover_nodes;
    const size_t stride = sat_cover_stride(nodes);
    u64 *adj = ctx->d_cv_adj.get(), *un = ctx->d_cv_mask.get(), *mask = un + stride, *state = ctx->d_cv_state.get();
    int32_t *d_rep = ctx->d_cv_out.get(), *d_degree = d_rep + nodes;
    const size_t most = std::max(std::max(stride, (size_t)nodes), (size_t)kStateWords);
    HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(cover_reset, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, ctx->stream, nodes, stride, un, d_rep, state);
    hipLaunchKernelGGL(cover_degree, dim3(row_blocks(nodes)), dim3(64 * kRowWaves), 0, ctx->stream, nodes, stride, adj, d_degree, state);
    HIP_TRY(hipGetLastError());
    // a round takes at least two nodes: nodes / 2 rounds at most, and one more that finds nothing left
    for (int queued = 0;; queued += kRoundBatch) {
        if (queued > nodes / 2 + 1) return sat_fail(SAT_EDEVICE, "the cover did not finish in %d rounds", queued);
        for (int r = 0; r < kRoundBatch; r++) {
            hipLaunchKernelGGL(cover_gain, dim3(row_blocks(nodes)), dim3(64 * kRowWaves), 0, ctx->stream, nodes, stride, adj, un, state);
            hipLaunchKernelGGL(cover_apply, dim3(1), dim3(kApplyBlock), 0, ctx->stream, stride, adj, un, d_rep, state);
        }
        HIP_TRY(hipGetLastError());
        u64 done = 0ull;
        SAT_TRY(sat_fetch(ctx, &done, state + kDone, 1, true));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (done) break;
    }
    hipLaunchKernelGGL(cover_rep_mask, dim3((unsigned)((stride + 255) / 256)), dim3(256), 0, ctx->stream, nodes, stride, d_rep, mask);
    hipLaunchKernelGGL(cover_check, dim3(row_blocks(nodes)), dim3(64 * kRowWaves), 0, ctx->stream, nodes, stride, adj, d_rep, mask, state);
    HIP_TRY(hipGetLastError());
    u64 counts[3] = { 0ull, 0ull, 0ull };                   // rounds, the degrees' sum, the broken invariants
    SAT_TRY(sat_fetch(ctx, rep, d_rep, (size_t)nodes, true));
    if (degree) SAT_TRY(sat_fetch(ctx, degree, d_degree, (size_t)nodes, true));
    SAT_TRY(sat_fetch(ctx, counts, state + kRounds, 3, true));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (counts[2] != 0ull)
        return sat_fail(SAT_EDEVICE, "the cover breaks its invariants at %llu places (a member off its representative, or two "
                        "representatives adjacent)", counts[2]);
    if (counts[1] & 1ull) return sat_fail(SAT_EDEVICE, "the adjacency matrix is not symmetric (its bits sum to %llu)", counts[1]);
    if (edges) *edges = counts[1] / 2ull;
    if (rounds) *rounds = (int)counts[0];
    return SAT_OK;
}

int sat_cover_end(sat_ctx *ctx)
{
    SAT_TRY(sat_check_context(ctx));
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    sat_cover_drop(ctx);
    return SAT_OK;
}

}  // extern "C"
