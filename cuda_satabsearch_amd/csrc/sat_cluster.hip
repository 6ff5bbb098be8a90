// sat_cluster.hip - single-linkage clustering of the database at a p-value, on the device (sat_cluster_*).
//
// Nodes are the structures of the whole database in file order.  Row (q, e) of the last search is an edge between
// query_node[q] and ordinal[e] iff the p-value hit_row gives it is <= max_pvalue - cutoff_row of sat_hitrow.hpp, the
// predicate of sat_hits_cutoff - and the two differ.  cluster_add walks the rows as cutoff_count does and keeps the graph
// as a lock-free union-find (parent) plus a degree per node and one edge counter; cluster_labels turns the forest into
// label[v] = the smallest node of v's component.  Everything is integers and the labels are a property of the edge SET,
// so nothing depends on the launch shape, the batches, the order of the calls or the sharding.  The host side takes the
// searched-state check, the chunk walk, the queries' HitQuery rows and the counted copies from sat_cutoff.hpp.
//
// The union-find links by index - the larger root goes under the smaller - and keeps, at every moment:
//   (1) parent[v] <= v;                     (3) parent[v] is a node of v's tree, so of v's component of the edges so far;
//   (2) parent[v] only ever decreases;      (4) a root (parent[r] == r) is the smallest node of its tree.
// parent is written by two operations only, both atomic and both lowering the word: atomicCAS(parent + hi, hi, lo) with
// lo < hi a node of the tree being joined to hi's, and atomicMin(parent + v, ancestor of v).  No plain store, no lock, no
// flag.  Off a root parent[v] < v, so the forest has no cycle.  Reads are relaxed agent-scope atomic loads: the eight
// XCDs have an L2 each and a plain load may be served from a stale line.  A stale value is an EARLIER value of the word:
// by (2) at or above the current one, by (3) a node of v's tree then and - trees only merge - ever after.  Following it
// is slower, never wrong.  The one place a stale read could matter is "x is a root"; that is decided by the CAS on x,
// which acts on the word itself, and on failure the walk goes on from the value the CAS returned - no loop re-reads a
// word until it changes.  Termination: find descends strictly, and every retry of unite replaces hi by a smaller node.
#include <hip/hip_runtime.h>

#include "sat_ctx.hpp"
#include "sat_cutoff.hpp"
#include "sat_hitrow.hpp"

namespace {

__device__ __forceinline__ int32_t load_parent(const int32_t *parent, int32_t v)
{
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of v's tree as the loads show it (a root of an earlier moment at worst: still a node of v's tree, <= v)
__device__ __forceinline__ int32_t find_root(const int32_t *parent, int32_t v)
{
    for (;;) {
        const int32_t p = load_parent(parent, v);
        if (p == v) return v;
        v = p;
    }
}

// join the components of a and b
__device__ __forceinline__ void unite(int32_t *parent, int32_t a, int32_t b)
{
    const int32_t a0 = a, b0 = b;
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) break;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) break;                   // hi was a root and now hangs under lo
        a = old;                                // hi had been hooked already: old < hi is its ancestor; go on from there
        b = lo;
    }
    // path compression for the two ends: the smaller of the nodes the walks ended at is now above both in their one
    // tree, and atomicMin only lowers.  Only where a load shows something to lower: the lanes of a block share their
    // query's node, and a thousand atomics on its one word cost more than the walks they save (a stale load here costs
    // one atomic that changes nothing)
    const int32_t r = a < b ? a : b;
    if (load_parent(parent, a0) > r) atomicMin(parent + a0, r);
    if (load_parent(parent, b0) > r) atomicMin(parent + b0, r);
}

// One thread per row, the grid of cutoff_count: a qualifying row that is no self row adds 1 to the degree of its entry's
// node and joins the two ends; the block's edges go through block_count into ONE 64-bit atomic on the edge counter (one
// word for the whole grid: one atomic per wave is DESIGN 6d's 170 us) and ONE atomic on the degree of the query's node -
// a block holds rows of one query only, so its edge count is what that node's degree gains.
__global__ void __launch_bounds__(kCutoffBlock) cluster_add(const int32_t *scores, int n, int bpq, const int32_t *orders,
                                                             const HitQuery *queries, const double *ztab, const double *ptab,
                                                             double max_p, const int32_t *query_node, const uint32_t *ordinal,
                                                             int32_t *parent, int32_t *degree, unsigned long long *edges)
{
    int q, e;
    int32_t score = 0;
    bool edge = cutoff_row(scores, n, bpq, orders, queries, ztab, ptab, max_p, q, e, score);
    if (edge) {
        const int32_t a = query_node[q], b = (int32_t)ordinal[e];      // both < the accumulator's nodes: checked on the host
        edge = a != b;
        if (edge) {
            atomicAdd(degree + b, 1);
            unite(parent, a, b);
        }
    }
    block_count(edge, [&](int32_t c) {
        atomicAdd(edges, (unsigned long long)c);
        atomicAdd(degree + query_node[q], c);
    });
}

// parent[v] = v, degree[v] = 0 for v < nodes; the edge counter 0
__global__ void cluster_init(int nodes, int32_t *parent, int32_t *degree, unsigned long long *edges)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v == 0) *edges = 0ull;
    if (v < nodes) {
        parent[v] = v;
        degree[v] = 0;
    }
}

// label[v] = the root of v; parent is only read, so further cluster_add launches may follow
__global__ void cluster_labels(int nodes, const int32_t *parent, int32_t *label)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < nodes) label[v] = find_root(parent, v);
}

int check_accumulator(const sat_ctx *ctx)
{
    SAT_TRY(sat_check_context(ctx));
    if (ctx->cluster_nodes <= 0)
        return sat_fail(SAT_ESTATE, "no cluster accumulator (sat_cluster_begin has not been called since the last database upload)");
    return SAT_OK;
}

}  // namespace

// sat_ctx.hpp: load this file's code object (an empty launch of a small kernel)
int sat_cluster_load_code(sat_ctx *ctx)
{
    hipLaunchKernelGGL(cluster_labels, dim3(1), dim3(64), 0, ctx->stream, 0, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return SAT_OK;
}

// sat_ctx.hpp: the accumulator goes (the caller has waited for the stream, or is about to free the database anyway)
void sat_cluster_drop(sat_ctx *ctx)
{
    ctx->cluster_nodes = 0;
    ctx->d_cl_parent.reset();
    ctx->d_cl_out.reset();
    ctx->d_cl_edges.reset();
}

extern "C" {

int sat_cluster_begin(sat_ctx *ctx, int n_nodes)
{
    SAT_TRY(sat_check_context(ctx));
    SAT_TRY(sat_check_uploaded(ctx->n_entries > 0));
    if (n_nodes < 1) return sat_fail(SAT_EINVAL, "n_nodes must be >= 1 (got %d)", n_nodes);
    if (ctx->max_ordinal >= (uint32_t)n_nodes)
        return sat_fail(SAT_EINVAL, "n_nodes = %d, but a resident entry has ordinal %u in the whole database", n_nodes, ctx->max_ordinal);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // an earlier accumulator may still be in use there
    ctx->cluster_nodes = 0;
    SAT_TRY(ctx->d_cl_parent.grow((size_t)n_nodes));
    SAT_TRY(ctx->d_cl_out.grow(2 * (size_t)n_nodes));
    SAT_TRY(ctx->d_cl_edges.grow(1));
    // d_cl_out: labels [n_nodes] (written by sat_cluster_labels), then degrees [n_nodes]
    hipLaunchKernelGGL(cluster_init, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, ctx->stream, n_nodes, ctx->d_cl_parent.get(),
                       ctx->d_cl_out.get() + n_nodes, ctx->d_cl_edges.get());
    HIP_TRY(hipGetLastError());
    ctx->cluster_nodes = n_nodes;
    return SAT_OK;
}

int sat_cluster_add(sat_ctx *ctx, double max_pvalue, const int32_t *query_node)
{
    SAT_TRY(check_accumulator(ctx));
    SAT_TRY(sat_check_searched(ctx));
    if (!query_node) return sat_fail(SAT_EINVAL, "query_node is null");
    SAT_TRY(sat_check_pvalue(max_pvalue));
    const int n = ctx->n_entries, nq = (int)ctx->queries.size(), nodes = ctx->cluster_nodes;
    for (int q = 0; q < nq; q++)
        if (query_node[q] < 0 || query_node[q] >= nodes)
            return sat_fail(SAT_EINVAL, "query %d: node %d outside 0..%d", q, query_node[q], nodes - 1);
    if (ctx->max_ordinal >= (uint32_t)nodes) return sat_fail(SAT_ESTATE, "the accumulator does not cover the resident database");
    HIP_TRY(hipSetDevice(ctx->device));
    SAT_TRY(ctx->d_cl_qnode.grow_after(ctx->stream, (size_t)nq));
    // the caller's array may go at return: a synchronous copy, ordered behind the stream by sat_hitq_upload's wait
    SAT_TRY(sat_hitq_upload(ctx, false));
    HIP_TRY(hipMemcpy(ctx->d_cl_qnode.get(), query_node, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice));
    const HitQuery *hq = hit_queries(ctx);
    return sat_row_chunks(ctx, kCutoffBlock, [&](int q0, int, int bpq, dim3 grid) -> int {
        hipLaunchKernelGGL(cluster_add, grid, dim3(kCutoffBlock), 0, ctx->stream, ctx->d_scores.get() + (size_t)q0 * n, n, bpq,
                           ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(), max_pvalue,
                           ctx->d_cl_qnode.get() + q0, ctx->d_ordinal.get(), ctx->d_cl_parent.get(), ctx->d_cl_out.get() + nodes,
                           ctx->d_cl_edges.get());
        HIP_TRY(hipGetLastError());
        return SAT_OK;
    });
}

int sat_cluster_labels(sat_ctx *ctx, int32_t *label, int32_t *degree, unsigned long long *edges)
{
    SAT_TRY(check_accumulator(ctx));
    if (!label) return sat_fail(SAT_EINVAL, "label buffer is null");
    const int nodes = ctx->cluster_nodes;
    HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(cluster_labels, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, ctx->stream, nodes, ctx->d_cl_parent.get(),
                       ctx->d_cl_out.get());
    HIP_TRY(hipGetLastError());
    SAT_TRY(sat_fetch(ctx, label, ctx->d_cl_out.get(), (size_t)nodes, true));
    if (degree) SAT_TRY(sat_fetch(ctx, degree, ctx->d_cl_out.get() + nodes, (size_t)nodes, true));
    if (edges) SAT_TRY(sat_fetch(ctx, edges, ctx->d_cl_edges.get(), 1, true));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SAT_OK;
}

int sat_cluster_end(sat_ctx *ctx)
{
    SAT_TRY(sat_check_context(ctx));
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    sat_cluster_drop(ctx);
    return SAT_OK;
}

}  // extern "C"
