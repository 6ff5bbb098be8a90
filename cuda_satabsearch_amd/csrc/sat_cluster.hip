// sat_cluster.hip - single-linkage clustering of the database at a p-value, on the device (sat_cluster_*),
// and at several p-values in one pass (sat_cluster_*_levels; below the plain kernels).
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
#include "host/sat_cluster.h"

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

// join the components of a and b; true iff this call made the hook that joined them (false: the walks met in one tree)
__device__ __forceinline__ bool unite(int32_t *parent, int32_t a, int32_t b)
{
    const int32_t a0 = a, b0 = b;
    bool hooked = false;
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) break;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicCAS(parent + hi, hi, lo);
        hooked = old == hi;
        if (hooked) break;                      // hi was a root and now hangs under lo
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
    return hooked;
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

// ---- Several cutoffs in one pass.  Level j of L has the cutoff cuts.p[j], ascending, a forest of its own
// at parent + j * nodes, and the same invariants (1) - (4) and the same termination argument as the one forest above: the
// levels share no word.  A row whose p-value first qualifies at level j0 is an edge of the levels j0 .. L - 1.  It is
// COUNTED once, at j0 - cluster_labels_levels sums the counts of the levels up to j into level j's degrees and edges - and
// UNITED in the forests j0 .. L - 1, tightest first, until a level where this thread made no hook: every hook of forest j
// was made by an edge that goes on to forest j + 1, where it hooks or finds its ends joined, so by induction over the
// hooks forest j + 1 ends up connecting whatever forest j connects, and two ends found in one tree of forest j need no
// help in the looser ones.  (Final connectivity only: nothing reads a forest before the launch has ended.)  Every edge of
// a context goes through that context's own forests, so the argument holds across add calls and per shard.
// -DSAT_CLUSTER_CLIMB_ALL compiles the early stop out (scripts/cluster_levels_cost.py measures both).

// the cutoffs as ONE kernel argument, by value: no upload, no constant memory
struct ClusterCuts {
    double p[SAT_MAX_CLUSTER_LEVELS];
    int32_t levels;
};

// The p-value of this thread's row: cutoff_row's block and row arithmetic, then the double hit_row gives - the one
// sat_hits_cutoff and cluster_add compare.  q is the block's query in any case; false: no row (past the query's last)
__device__ __forceinline__ bool row_pvalue(const int32_t *scores, int n, int bpq, const int32_t *orders, const HitQuery *queries,
                                           const double *ztab, const double *ptab, int &q, int &e, double &p)
{
    q = (int)(blockIdx.x / (unsigned)bpq);
    e = (int)(blockIdx.x - (unsigned)q * bpq) * kCutoffBlock + (int)threadIdx.x;
    if (e >= n) return false;
    p = hit_row(e, scores[(size_t)q * n + e], queries[q].n1, orders[e], ztab, ptab, queries[q].fit).pvalue;
    return true;
}

// One thread per row, the grid of cluster_add.  j0 = the first level with p <= cuts.p[j], by L compares of the double
// itself (a NaN passes none: j0 = L, no edge).  The block's count per level: a ballot per wave and level, the 16 counts
// through LDS, and thread j hands level j's sum - when it is not zero - to ONE atomic on the level's edge counter and ONE
// on the degree of the query's node at that level (a block holds rows of one query only).
__global__ void __launch_bounds__(kCutoffBlock) cluster_add_levels(const int32_t *scores, int n, int bpq, const int32_t *orders,
                                                                    const HitQuery *queries, const double *ztab, const double *ptab,
                                                                    ClusterCuts cuts, const int32_t *query_node, const uint32_t *ordinal,
                                                                    int nodes, int32_t *parent, int32_t *degree_at,
                                                                    unsigned long long *edges_at)
{
    __shared__ int32_t wave_count[SAT_MAX_CLUSTER_LEVELS][kCutoffWaves];
    const int levels = cuts.levels;
    int q, e, j0 = levels;
    int32_t a = 0, b = 0;
    double p;
    if (row_pvalue(scores, n, bpq, orders, queries, ztab, ptab, q, e, p)) {
        int above = 0;                                                  // the levels whose cutoff the row misses
#pragma unroll
        for (int j = 0; j < SAT_MAX_CLUSTER_LEVELS; j++) above += (j < levels && !(p <= cuts.p[j])) ? 1 : 0;
        a = query_node[q], b = (int32_t)ordinal[e];                     // both < nodes: checked on the host
        j0 = a != b ? above : levels;
    }
#pragma unroll
    for (int j = 0; j < SAT_MAX_CLUSTER_LEVELS; j++)
        if (j < levels) {
            const unsigned long long mask = __ballot(j0 == j);
            if ((threadIdx.x & 63) == 0) wave_count[j][threadIdx.x >> 6] = (int32_t)__popcll(mask);
        }
    if (j0 < levels) {
        atomicAdd(degree_at + (size_t)j0 * nodes + b, 1);
        for (int j = j0; j < levels; j++) {
            const bool hooked = unite(parent + (size_t)j * nodes, a, b);
#ifndef SAT_CLUSTER_CLIMB_ALL
            if (!hooked) break;
#else
            (void)hooked;
#endif
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < levels) {
        int32_t c = 0;
        for (int w = 0; w < kCutoffWaves; w++) c += wave_count[threadIdx.x][w];
        if (c) {
            atomicAdd(edges_at + threadIdx.x, (unsigned long long)c);
            atomicAdd(degree_at + (size_t)threadIdx.x * nodes + query_node[q], c);
        }
    }
}

// level blockIdx.y: parent[v] = v, degree_at[v] = 0 for v < nodes; the level's edge counter 0
__global__ void cluster_init_levels(int nodes, int32_t *parent, int32_t *degree_at, unsigned long long *edges_at)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t at = (size_t)blockIdx.y * nodes;
    if (v == 0) edges_at[blockIdx.y] = 0ull;
    if (v < nodes) {
        parent[at + v] = v;
        degree_at[at + v] = 0;
    }
}

// level j = blockIdx.y: label[j][v] = the root of v in forest j; degree[j][v] and edges[j] = the counts of the levels
// 0 .. j summed.  parent and the "at" counts are only read, so further cluster_add_levels launches may follow
__global__ void cluster_labels_levels(int nodes, const int32_t *parent, const int32_t *degree_at, const unsigned long long *edges_at,
                                      int32_t *label, int32_t *degree, unsigned long long *edges)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, j = (int)blockIdx.y;
    const size_t at = (size_t)j * nodes;
    if (v == 0) {
        unsigned long long sum = 0ull;
        for (int i = 0; i <= j; i++) sum += edges_at[i];
        edges[j] = sum;
    }
    if (v < nodes) {
        label[at + v] = find_root(parent + at, v);
        int32_t sum = 0;
        for (int i = 0; i <= j; i++) sum += degree_at[(size_t)i * nodes + v];
        degree[at + v] = sum;
    }
}

// an accumulator of the kind the call works on (leveled: the _levels calls)
int check_accumulator(const sat_ctx *ctx, bool leveled)
{
    SAT_TRY(sat_check_context(ctx));
    if (ctx->cluster_nodes <= 0)
        return sat_fail(SAT_ESTATE, "no cluster accumulator (sat_cluster_begin has not been called since the last database upload)");
    if (leveled && ctx->cluster_levels == 0)
        return sat_fail(SAT_ESTATE, "the cluster accumulator is a plain one (sat_cluster_begin): it takes sat_cluster_add and sat_cluster_labels");
    if (!leveled && ctx->cluster_levels > 0)
        return sat_fail(SAT_ESTATE, "the cluster accumulator is a leveled one (sat_cluster_begin_levels, %d levels): it takes sat_cluster_add_levels "
                        "and sat_cluster_labels_levels", ctx->cluster_levels);
    return SAT_OK;
}

// the checks both begin calls make
int check_begin(sat_ctx *ctx, int n_nodes)
{
    SAT_TRY(sat_check_context(ctx));
    SAT_TRY(sat_check_uploaded(ctx->n_entries > 0));
    if (n_nodes < 1) return sat_fail(SAT_EINVAL, "n_nodes must be >= 1 (got %d)", n_nodes);
    if (ctx->max_ordinal >= (uint32_t)n_nodes)
        return sat_fail(SAT_EINVAL, "n_nodes = %d, but a resident entry has ordinal %u in the whole database", n_nodes, ctx->max_ordinal);
    return SAT_OK;
}

// An add call behind its accumulator's check: the searched state, the queries' nodes (more(): the checks the call makes
// between the null list and the nodes' range), the nodes and the HitQuery rows to the device, then launch(q0, bpq, grid,
// hq) for every chunk of the queries
template <typename More, typename Launch> int add_rows(sat_ctx *ctx, const int32_t *query_node, More more, Launch launch)
{
    SAT_TRY(sat_check_searched(ctx));
    if (!query_node) return sat_fail(SAT_EINVAL, "query_node is null");
    SAT_TRY(more());
    const int nq = (int)ctx->queries.size(), nodes = ctx->cluster_nodes;
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
        launch(q0, bpq, grid, hq);
        HIP_TRY(hipGetLastError());
        return SAT_OK;
    });
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
    ctx->cluster_nodes = ctx->cluster_levels = 0;
    ctx->d_cl_parent.reset();
    ctx->d_cl_out.reset();
    ctx->d_cl_edges.reset();
}

extern "C" {

int sat_cluster_begin(sat_ctx *ctx, int n_nodes)
{
    SAT_TRY(check_begin(ctx, n_nodes));
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // an earlier accumulator may still be in use there
    ctx->cluster_nodes = ctx->cluster_levels = 0;
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
    SAT_TRY(check_accumulator(ctx, false));
    const int n = ctx->n_entries, nodes = ctx->cluster_nodes;
    return add_rows(ctx, query_node, [&] { return sat_check_pvalue(max_pvalue); }, [&](int q0, int bpq, dim3 grid, const HitQuery *hq) {
        hipLaunchKernelGGL(cluster_add, grid, dim3(kCutoffBlock), 0, ctx->stream, ctx->d_scores.get() + (size_t)q0 * n, n, bpq,
                           ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(), max_pvalue,
                           ctx->d_cl_qnode.get() + q0, ctx->d_ordinal.get(), ctx->d_cl_parent.get(), ctx->d_cl_out.get() + nodes,
                           ctx->d_cl_edges.get());
    });
}

int sat_cluster_labels(sat_ctx *ctx, int32_t *label, int32_t *degree, unsigned long long *edges)
{
    SAT_TRY(check_accumulator(ctx, false));
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

int sat_cluster_begin_levels(sat_ctx *ctx, int n_nodes, int n_levels, const double *max_pvalue)
{
    SAT_TRY(check_begin(ctx, n_nodes));
    SAT_TRY(sat_check_levels(n_levels, max_pvalue));
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // an earlier accumulator may still be in use there
    ctx->cluster_nodes = ctx->cluster_levels = 0;
    const size_t cells = (size_t)n_levels * (size_t)n_nodes;
    SAT_TRY(ctx->d_cl_parent.grow(cells));
    SAT_TRY(ctx->d_cl_out.grow(3 * cells));
    SAT_TRY(ctx->d_cl_edges.grow(2 * (size_t)n_levels));
    // d_cl_out: labels, degrees (written by sat_cluster_labels_levels), the degrees at each level; [n_levels][n_nodes] each
    hipLaunchKernelGGL(cluster_init_levels, dim3((unsigned)((n_nodes + 255) / 256), (unsigned)n_levels), dim3(256), 0, ctx->stream, n_nodes,
                       ctx->d_cl_parent.get(), ctx->d_cl_out.get() + 2 * cells, ctx->d_cl_edges.get());
    HIP_TRY(hipGetLastError());
    ctx->cluster_nodes = n_nodes;
    ctx->cluster_levels = n_levels;
    std::copy(max_pvalue, max_pvalue + n_levels, ctx->cluster_cut);
    return SAT_OK;
}

int sat_cluster_add_levels(sat_ctx *ctx, const int32_t *query_node)
{
    SAT_TRY(check_accumulator(ctx, true));
    const int n = ctx->n_entries, nodes = ctx->cluster_nodes, levels = ctx->cluster_levels;
    ClusterCuts cuts = {};
    cuts.levels = levels;
    std::copy(ctx->cluster_cut, ctx->cluster_cut + levels, cuts.p);
    int32_t *degree_at = ctx->d_cl_out.get() + 2 * (size_t)levels * nodes;
    return add_rows(ctx, query_node, [] { return SAT_OK; }, [&](int q0, int bpq, dim3 grid, const HitQuery *hq) {
        hipLaunchKernelGGL(cluster_add_levels, grid, dim3(kCutoffBlock), 0, ctx->stream, ctx->d_scores.get() + (size_t)q0 * n, n, bpq,
                           ctx->d_orders.get(), hq + q0, ctx->d_gumbel_z.get(), ctx->d_gumbel_p.get(), cuts,
                           ctx->d_cl_qnode.get() + q0, ctx->d_ordinal.get(), nodes, ctx->d_cl_parent.get(), degree_at,
                           ctx->d_cl_edges.get());
    });
}

int sat_cluster_labels_levels(sat_ctx *ctx, int32_t *label, int32_t *degree, unsigned long long *edges)
{
    SAT_TRY(check_accumulator(ctx, true));
    if (!label) return sat_fail(SAT_EINVAL, "label buffer is null");
    const int nodes = ctx->cluster_nodes, levels = ctx->cluster_levels;
    const size_t cells = (size_t)levels * (size_t)nodes;
    HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(cluster_labels_levels, dim3((unsigned)((nodes + 255) / 256), (unsigned)levels), dim3(256), 0, ctx->stream, nodes,
                       ctx->d_cl_parent.get(), ctx->d_cl_out.get() + 2 * cells, ctx->d_cl_edges.get(), ctx->d_cl_out.get(),
                       ctx->d_cl_out.get() + cells, ctx->d_cl_edges.get() + levels);
    HIP_TRY(hipGetLastError());
    SAT_TRY(sat_fetch(ctx, label, ctx->d_cl_out.get(), cells, true));
    if (degree) SAT_TRY(sat_fetch(ctx, degree, ctx->d_cl_out.get() + cells, cells, true));
    if (edges) SAT_TRY(sat_fetch(ctx, edges, ctx->d_cl_edges.get() + levels, (size_t)levels, true));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // single linkage is monotone in the cutoff: every level refines the next.  One walk of the labels, no allocation
    const int broken = sat_cluster_nested(nodes, levels, label);
    if (broken < 0) return sat_fail(SAT_EDEVICE, "a level's labels are no canonical labelling");
    if (broken > 0) return sat_fail(SAT_EDEVICE, "level %d's clusters do not lie inside level %d's", broken - 1, broken);
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
