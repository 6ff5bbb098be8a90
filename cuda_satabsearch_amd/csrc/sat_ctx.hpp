// sat_ctx.hpp - private definition of the C ABI's context (shared by the library's translation units except
// sat_launch.hip; not part of the public interface).  The pair modes' declarations are in sat_pairs.hpp, which includes it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <utility>
#include <vector>

#include "satabsearch.h"
#include "sat_sa_kernel.hpp"
#include "sat_launch.hpp"               // sat_fail, HIP_TRY; the launch code's part of the context

// A device array of T that owns its allocation: the pointer and its capacity in elements live and die together.
// Freed on destruction or reset(), on whatever device is current then (the owners make theirs current first).
template <typename T> class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(cap_, o.cap_);
        }
        return *this;
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }

    T *get() const { return p_; }
    size_t capacity() const { return cap_; }
    void reset()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // Room for `need` elements, contents not kept: when the capacity is smaller, the old allocation is replaced by
    // one of exactly `need`.  *moved tells whether the pointer changed.  A failed allocation leaves the buffer empty.
    int grow(size_t need, bool *moved = nullptr)
    {
        if (moved) *moved = need > cap_;
        if (need <= cap_) return SAT_OK;
        reset();
        T *p = nullptr;
        HIP_TRY(hipMalloc(&p, need * sizeof(T)));
        p_ = p;
        cap_ = need;
        return SAT_OK;
    }
    // grow() that waits for `stream` before replacing the allocation: work queued there may still use it
    int grow_after(hipStream_t stream, size_t need)
    {
        if (need > cap_) HIP_TRY(hipStreamSynchronize(stream));
        return grow(need);
    }
    // a fresh allocation of exactly `n` elements
    int alloc(size_t n)
    {
        reset();
        return grow(n);
    }

  private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

// A query's size class: its order padded to 16, 32, 64 or 112
__host__ __device__ inline int query_n1p(int n1) { return n1 <= 16 ? 16 : (n1 <= 32 ? 32 : (n1 <= 64 ? 64 : 112)); }

// One query of padded order n1p in the query blob: qdist | qcode | qtypes | qpair - the grouped cells (16 + 4 bytes per
// group of four and column), the SSE types, then from the next 16-byte boundary the dense pair cells of the full score.
// The offsets of the last three and the size of the whole.
struct QueryBlob { size_t qcode, qtypes, qpair, bytes; };
__host__ __device__ inline QueryBlob query_blob(int n1p)
{
    const size_t n = (size_t)n1p, groups = n / 4 * n;
    QueryBlob b;
    b.qcode = groups * 16;
    b.qtypes = groups * 20;
    b.qpair = (groups * 20 + n + 15) & ~(size_t)15;
    b.bytes = b.qpair + n * n * 8;
    return b;
}

// db entries are launched in classes of similar order so that every launch sizes its
// LDS for the largest member of the class only
constexpr int kNumBuckets = 7;
constexpr int kBucketMax[kNumBuckets] = { 16, 32, 48, 64, 80, 96, 111 };

struct sat_ctx {
    int device = 0;
    uint64_t seed = SAT_DEFAULT_SEED;
    hipStream_t own_stream = nullptr;   // created with the context
    hipStream_t stream = nullptr;       // where work is queued (own_stream unless sat_use_stream)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    // database shard
    int n_entries = 0;
    DevBuf<int32_t> d_orders;
    DevBuf<int64_t> d_cell_off;
    DevBuf<uint8_t> d_tab;
    DevBuf<float> d_dist;
    DevBuf<uint32_t> d_ordinal;
    uint32_t max_ordinal = 0;               // the largest of them (sat_cluster_begin sizes its nodes by it)
    std::vector<uint32_t> h_ordinal;        // the host's copy (sat_search_reach turns a frontier's nodes into entries)
    DevBuf<int32_t> d_lists;                // entry indices grouped by bucket
    int bucket_begin[kNumBuckets + 1] = { 0 };
    int bucket_n2max[kNumBuckets] = { 0 };
    std::vector<int32_t> h_orders;

    // queries (a batch; one query is a batch of 1), input order
    // cls, desc: the query's size class and descriptor index (the descriptors are grouped by class, input order
    // inside), set where the descriptors are built
    struct QueryInfo { int n1, n1p; uint32_t ordinal; size_t blob_off; size_t ssemap_off; int cls, desc; };
    std::vector<QueryInfo> queries;
    DevBuf<uint8_t> d_qblob;                // per query: qdist | qcode | qtypes | qpair (query_blob)
    // queries taken from the resident shard (sat_queries_from_db, sat_qfromdb.hip): the entry of each query as it came
    // from the host (with sat_queries_from_db_sses followed by the lists' offsets and the list bytes), each query's
    // offset in the blob as the device summed them; only grow
    DevBuf<int32_t> d_qentry;
    DevBuf<unsigned long long> d_qoff;
    DevBuf<SatQuery> d_qdesc;               // descriptors grouped by size class
    int class_begin[5] = { 0, 0, 0, 0, 0 };  // classes: n1p = 16, 32, 64, 112
    int class_n1max[4] = { 0, 0, 0, 0 };
    int class_wpl[4] = { 0, 0, 0, 0 };       // map words per lane shared by the class's queries, 0 = mixed
    bool desc_dirty = true;
    bool desc_lsoln = false;

    // Metropolis table
    DevBuf<float> d_ptab;
    DevBuf<int32_t> d_prow;

    // overrides (SAT_EXP_* in satabsearch_debug.h), read ONCE when the context is created: these of the search plan,
    // the upload and the pair split, the launch heuristics' in `sa`.  scratch_bytes: what the scratch in d_bmap_slabs may
    // take before a search is cut into several launches (every cut keeps at least one slab).  select_keys: the (query,
    // entry) keys a chunk of a selection pass may hold (select_all_hits, cutoff_chunk in sat_topk.hip)
    struct Tuning { int streams = -1, upload_threads = 0, upload_timing = 0, upload_pieces = 0, refine_split = 0, polish_group = 0;
                    size_t scratch_bytes = (size_t)1 << 30;
                    long long select_keys = 0x7FFFFFFFll; } tune;
    // what sat_launch.hip keeps per context: its overrides, the instantiations whose dynamic-LDS limit has been raised
    // on this device, the entries per workgroup chosen so far
    SaLaunchState sa;
    // side streams: the order buckets of one search run concurrently (each launch has a tail of
    // half-empty CUs; the next bucket's workgroups fill it), forked from / joined to `stream`
    hipStream_t side_stream[kNumBuckets] = { nullptr };
    hipEvent_t ev_fork = nullptr, ev_join[kNumBuckets] = { nullptr };

    // what the result buffers hold: set by a search, cleared by an upload or a new query batch
    size_t searched_nq = 0;                  // 0 = no search since the last upload / query change
    bool searched_lsoln = false;
    bool searched_polished = false;          // the last search was a polished one: d_base holds its rows' base scores
    bool searched_exact = false;             // the last search was an exact one (sat_search_exact): d_xbase, d_xflag, d_xnodes hold its rows'
    // whole-database polish (sat_polish_all_set): 0 = off, else the maps polished per row.  A setting of the context,
    // like its stream: uploads and query changes leave it alone.
    int polish_all = 0;

    // multi-GPU gather (sat_multi.hip): the result buffers are sized for at least this many rows per
    // query, so that a fixed-size gather may read a shard padded to the largest shard
    int min_rows = 0;

    // results: scores [nq][N]; ssemaps: query q's [N][n1_q] block at queries[q].ssemap_off
    DevBuf<int32_t> d_scores;
    DevBuf<int8_t> d_ssemaps;
    DevBuf<uint32_t> d_bmap_slabs;           // LSOLN scratch: one best-map slab per workgroup of a launch
    // several matches per entry (sat_search_matches): outputs by descriptor index d, rows d * n_entries + e
    DevBuf<int32_t> d_mcounts, d_mscores, d_mrestarts;
    DevBuf<int8_t> d_mmaps;                  // [ndesc][N][M][SAT_MAXDIM]

    // pair mode (sat_search_pairs): work items (host copy kept until the next pair search: the upload is
    // asynchronous), one 64-bit arg-max key and one map per pair, the scores the keys give
    std::vector<SatPairItem> h_pitems;
    DevBuf<SatPairItem> d_pitems;
    DevBuf<unsigned long long> d_pkeys;
    DevBuf<int8_t> d_pmaps;                  // [pairs][SAT_MAXDIM], -1 past n1
    DevBuf<int32_t> d_pscores;
    // pair-match mode (sat_search_pairs_matches): per pair the words of a db set in its launch; counts [pairs],
    // scores [pairs][M], restarts [pairs][M] in one array; the maps go to d_pmaps as [pairs][M][SAT_MAXDIM]
    std::vector<uint8_t> h_psetw;
    DevBuf<uint8_t> d_psetw;
    DevBuf<int32_t> d_pmout;
    // polish (sat_search_pairs_polish, sat_polish.hip): score, base score, restart, moves [4][pairs]; the polished score
    // as the high word of a pair key [pairs]; the winner's polished map [pairs][SAT_MAXDIM]
    DevBuf<int32_t> d_polout;
    DevBuf<unsigned long long> d_polkeys;
    DevBuf<int8_t> d_polmaps;
    // whole-database polish: the rows' scores before the polish, laid out as d_scores; the "did not finish" flag
    DevBuf<int32_t> d_base;
    DevBuf<int32_t> d_polerr;
    // refine (sat_search_refine, sat_topk.hip): the final ranking of the nq x C re-scored candidates
    DevBuf<unsigned long long> d_rkeys, d_rsorted;
    DevBuf<int32_t> d_rvals, d_rvals_sorted, d_rfirst, d_rmaps;
    DevBuf<sat_hit> d_rhits;

    // best-k selection (sat_topk.hip): context-owned scratch that only grows
    DevBuf<unsigned long long> d_keys, d_sorted;
    DevBuf<unsigned char> d_sort_temp, d_hitq;
    DevBuf<int> d_seg;
    DevBuf<sat_hit> d_hits;
    DevBuf<int32_t> d_hit_maps;
    // z and p of every truncated norm2 score -128 .. 127, computed by the HOST's libm (sat_gumbel.c)
    DevBuf<double> d_gumbel_z, d_gumbel_p;
    // Fitted statistics (sat_stats_fit / sat_stats_set, sat_topk.hip): fits[q] of the searched state, empty = every query
    // on the built-in constants.  They belong to the scores in d_scores: whatever replaces those (a search, an upload, a
    // query change) empties them.  d_fit_tabs: query q's z[SAT_STAT_BINS] then p[SAT_STAT_BINS] at q * 2 * SAT_STAT_BINS,
    // filled by the host's libm for the fitted queries; d_hist: the score histogram, counts [nq][SAT_STAT_BINS] then below [nq]
    std::vector<sat_fit> fits;
    DevBuf<double> d_fit_tabs;
    DevBuf<uint32_t> d_hist;

    // single-linkage clustering (sat_cluster_*, sat_cluster.hip): the accumulator over cluster_nodes nodes (0 = none) -
    // the union-find's parent [nodes]; labels [nodes] (written by sat_cluster_labels) then degrees [nodes] in one array;
    // the 64-bit edge counter; the batch's node of each query.  An upload drops it (free_db).
    // Leveled (sat_cluster_begin_levels; cluster_levels = L > 0, cutoffs cluster_cut[0 .. L - 1] ascending):
    // one forest per level in d_cl_parent [L][nodes]; d_cl_out holds labels [L][nodes], degrees [L][nodes] (both written
    // by sat_cluster_labels_levels) and then the degrees counted AT each level [L][nodes]; d_cl_edges the edges at each
    // level [L], then their running sums [L].
    int cluster_nodes = 0;
    int cluster_levels = 0;
    double cluster_cut[SAT_MAX_CLUSTER_LEVELS] = { 0 };
    DevBuf<int32_t> d_cl_parent, d_cl_out, d_cl_qnode;
    DevBuf<unsigned long long> d_cl_edges;

    // transitive search (sat_reach_*, sat_reach.hip): the accumulator over reach_nodes nodes (0 = none) -
    // a 64-bit key (host/sat_reach.h) and a support count per node; the batch's node of each query.  Scratch of the
    // ordered compaction, which only grows: the count of every block of 1024 nodes, then their running sums, then the
    // total; the compacted nodes, or rows, before they leave.  It shares no word with the other accumulators.  An upload
    // drops it (free_db).
    int reach_nodes = 0;
    DevBuf<unsigned long long> d_rc_key;
    DevBuf<int32_t> d_rc_support, d_rc_qnode, d_rc_scan, d_rc_out;
    DevBuf<sat_reach_row> d_rc_rows;

    // clustering around representatives (sat_cover_*, sat_cover.hip): the accumulator over cover_nodes nodes
    // (0 = none) - the adjacency bit matrix, [nodes] rows of sat_cover_stride(nodes) words (host/sat_cover.h); the
    // `unassigned` mask and then the representatives' mask, a row's words each; rep [nodes] then degree [nodes] in one
    // array; the solve's state words (the round's key, done, rounds, the degrees' sum, the broken invariants); the batch's
    // node of each query.  It shares no word with the single-linkage accumulator above: a context may hold both.  An
    // upload drops it (free_db).
    int cover_nodes = 0;
    DevBuf<unsigned long long> d_cv_adj, d_cv_mask, d_cv_state;
    DevBuf<int32_t> d_cv_out, d_cv_qnode;

    // evaluation against a classification (sat_eval_*, sat_eval.hip): the class of each of eval_nodes
    // nodes (0 = none installed) on the host, of each resident entry on the device; scratch that only grows - every
    // query's table [2][bins] of the call at hand, the queries' rows for the kernels, the results.  An upload drops the
    // classes (free_db).
    int eval_nodes = 0;
    std::vector<int32_t> eval_class;
    DevBuf<int32_t> d_entry_class;
    DevBuf<uint32_t> d_eval_tab;
    DevBuf<unsigned char> d_eval_q;
    DevBuf<sat_eval> d_eval_rows;

    // a query's SSEs profiled over its hits (sat_profile_rows, sat_profile.hip): scratch that only grows -
    // hits [nq] then every query's [n1][n1] matrix, packed in query order; the queries' rows for the kernels
    DevBuf<uint32_t> d_profile;
    DevBuf<unsigned char> d_profile_q;

    // the baseline of sat_reorder_hits (sat_baseline_keep, sat_reorder.hip): every row's score and p-value
    // of the search that was the last one when it was kept, laid out as d_scores - 12 bytes a row.  baseline_nq x
    // baseline_n rows, 0 = none kept: it belongs to (resident database, query batch), so an upload and a query change
    // drop it; searches, fits, the polish setting and the accumulators leave it alone.  The buffers only grow.
    size_t baseline_nq = 0;
    int baseline_n = 0;
    DevBuf<int32_t> d_bl_score;
    DevBuf<double> d_bl_pvalue;
    // the selection's rows (sat_reorder_hit) before they leave; scratch that only grows
    DevBuf<sat_reorder_hit> d_reorder_rows;

    // exact search (sat_search_exact, sat_exact.hip): every row's incumbent score, laid out as d_scores; its
    // "unproven" flag and its node count; the per-query statistics before they leave.  The buffers only grow.
    DevBuf<int32_t> d_xbase;
    DevBuf<uint8_t> d_xflag;
    DevBuf<uint32_t> d_xnodes;
    DevBuf<sat_exact_stat> d_xstats;

    // bytes copied device -> host by this context's result calls (sat_stat_d2h_bytes)
    unsigned long long d2h_bytes = 0;
    // bytes copied host -> device by sat_queries_set / sat_queries_from_db (sat_stat_query_h2d_bytes)
    unsigned long long query_h2d_bytes = 0;
    // kernel instantiations and launch geometry of the last search (sat_last_launch_info; one launch_info() of
    // sat_launch.hip per launch, from the SaKernel that was launched)
    std::string last_launch_info;
};

// ---- sat_db.hip.  (Re)build the device query descriptors - pointers into the query blob and into the result buffers,
// grouped by size class - where the batch, the result buffers or `lsoln` changed; load the file's code object.
int refresh_descriptors(sat_ctx *ctx, bool lsoln, hipStream_t stream);
int sat_db_load_code(sat_ctx *ctx);

// ---- sat_cluster.hip.  Load that file's code object (an empty launch of a small kernel); drop the accumulator.
int sat_cluster_load_code(sat_ctx *ctx);
void sat_cluster_drop(sat_ctx *ctx);

// ---- sat_reach.hip.  Load that file's code object (an empty launch of a small kernel); drop the accumulator; and for
// the sharded calls of sat_multi.hip: the argument checks of sat_reach_begin behind the context's and the database's, of
// sat_reach_add behind the accumulator's and the searched state's, of the frontier and rows calls; the context's keys
// and supports to the host (counted in its d2h bytes); the nodes at `depth` (-1: the reached nodes) of joined keys.
int sat_reach_load_code(sat_ctx *ctx);
void sat_reach_drop(sat_ctx *ctx);
int sat_reach_check_begin(int n_nodes, int n_seeds, const int32_t *seed_node);
int sat_reach_check_add(int depth, double max_pvalue, int nq, const int32_t *query_node, int nodes);
int sat_reach_check_fetch(int depth, int cap, const void *out, const int32_t *count);
int sat_reach_check_search(int n_seeds, const int32_t *seed_entry, int n_entries, int maxstart, double max_pvalue, int max_depth,
                           int max_queries, int batch, double censor, int cap, const void *rows, const int32_t *count, const void *info);
int sat_reach_arrays_fetch(sat_ctx *ctx, unsigned long long *keys, int32_t *support);

// ---- sat_cover.hip.  Load that file's code object (an empty launch of a small kernel); drop the accumulator; and for
// sat_multi_cover_solve: rows row0 .. row0 + rows - 1 of the context's adjacency matrix to the host (counted in its
// d2h bytes), and such rows ORed into the context's own.
int sat_cover_load_code(sat_ctx *ctx);
void sat_cover_drop(sat_ctx *ctx);
int sat_cover_rows_fetch(sat_ctx *ctx, int row0, int rows, unsigned long long *host);
int sat_cover_rows_or(sat_ctx *ctx, int row0, int rows, const unsigned long long *host);

// ---- sat_eval.hip.  Load that file's code object (an empty launch of a small kernel); drop the installed classes.
int sat_eval_load_code(sat_ctx *ctx);
void sat_eval_drop(sat_ctx *ctx);

// ---- sat_profile.hip.  Load that file's code object (an empty launch of a small kernel).
int sat_profile_load_code(sat_ctx *ctx);

// ---- sat_reorder.hip.  Load that file's code object (an empty launch of a small kernel).
int sat_reorder_load_code(sat_ctx *ctx);

// ---- sat_exact.hip.  Load that file's code object (an empty launch of a small kernel); and for sat_multi_search_exact:
// the refusals of sat_search_exact (all SAT_EINVAL, nothing queued or changed), the incumbent search and the proof pass
// queued on the context's stream, and the check that the last search was an exact one.
int sat_exact_load_code(sat_ctx *ctx);
int sat_exact_check(const sat_ctx *ctx, int maxstart, unsigned long long max_nodes);
int sat_exact_launch(sat_ctx *ctx, int lorder, int maxstart, unsigned long long max_nodes);
int sat_exact_check_state(const sat_ctx *ctx);

// ---- sat_qfromdb.hip, for sat_multi_queries_from_db.  sat_queries_from_db on one shard's context, every check made by
// the caller: query q has order n1s[q] and is entry code[q] >= 0 of this shard, or code[q] = -query_n1p(n1s[q]): a
// query whose entry another shard holds - it takes its room in the blob and the caller copies its bytes in afterwards.
// sse_begin, sse: null, or the lists of sat_queries_from_db_sses (n1s[q] is then the list's length where query q has
// one); only the lists of the shard's own queries are read, so the caller may leave the other ranges empty.
int sat_qfromdb_set(sat_ctx *ctx, int n_queries, const int32_t *code, const int32_t *n1s, const int32_t *sse_begin,
                    const uint8_t *sse, uint32_t first_query_ordinal);
// the checks of sat_queries_from_db_sses' lists, SAT_EINVAL with the message set: the offsets of the batch; the list of
// m SSEs of query q, which is entry `entry` of that order
int sat_qfromdb_check_offsets(int n_queries, const int32_t *sse_begin, const uint8_t *sse);
int sat_qfromdb_check_list(int q, int entry, int order, const uint8_t *list, int m);
// where query q lies in the context's blob, and its size
void sat_qfromdb_segment(const sat_ctx *ctx, int q, uint8_t **at, size_t *bytes);

// ---- sat_capi.hip, for the overlapped upload of sat_db.hip.  The entries a set of launches covers: indices into the
// resident shard grouped by order bucket.  A search covers the whole shard (the context's lists); the overlapped upload
// (sat_db_upload_search) searches the shard piece by piece, each piece with lists of its own.
struct ListView {
    const int32_t *d_list;       // device array the `begin` offsets index
    const int *begin;            // [kNumBuckets + 1]
    const int *n2max;            // [kNumBuckets] largest order per bucket, 0 = empty
    int n;                       // entries covered = begin[kNumBuckets] - begin[0]
};
// The preconditions of queuing a search, checked in this order: a context, a database (need_db), a query batch,
// maxstart >= 1.
int check_ready(const sat_ctx *ctx, bool need_db, int maxstart);
// Queue a search of `piece` (null: the whole shard) on `stream`.  mx: one pass of the match mode (sat_search_matches)
// instead of a plain search; lsoln is 0 then.
int launch_search(sat_ctx *ctx, int lorder, int lsoln, int maxstart, hipStream_t stream, const ListView *piece = nullptr,
                  const SatMatchArgs *mx = nullptr);

// The two halves of sat_search_matches (sat_capi.hip), for sat_multi_search_matches: queue both passes on the
// context's stream, then wait and copy query q's row of entry e to row q * total + offset + e of the caller's arrays
// (maps may be NULL: no replay pass, none copied).
int sat_matches_launch(sat_ctx *ctx, int lorder, int maxstart, int max_matches, bool maps);
int sat_matches_collect(sat_ctx *ctx, int max_matches, int32_t *counts, int32_t *scores, int32_t *restarts,
                        int32_t *ssemaps, size_t total, size_t offset);

#ifdef SAT_DIAG
// ---- sat_capi.hip, diagnostic builds only: satdiag::begin / end (diag/sat_diag.hpp, whose host side that file holds)
hipError_t sat_diag_begin(hipStream_t stream, unsigned long long *&arg);
hipError_t sat_diag_end(hipStream_t stream);
#endif
// ---- sat_capi.hip, shared with the pair modes (sat_pairs.hip).  prepare_sa (sat_launch.hpp) for queries of class c of
// the current batch, with the SatKernelArgs fields every launch shares (base_args)
int prepare_launch(sat_ctx *ctx, int mode, int lorder, int lsoln, int maxstart, int plan_starts, int c, int n2max, long long work,
                   bool pack, SaLaunch &out);
// The head of both match searches: a context, max_matches in range, then the SatMatchArgs fields they share (the record
// pass; maps of SAT_MAXDIM bytes).  The caller adds the row length and the outputs once its buffers stand.  (The
// descriptor table is taken before the caller's refresh_descriptors: only sat_set_queries reallocates it.)
int match_args(const sat_ctx *ctx, int max_matches, SatMatchArgs &mx);

// One map of the device's outputs (int8, SAT_MAXDIM bytes) as the caller's int32 row: the images of the query's n1
// SSEs, -1 behind them, all -1 for an unused match slot
inline void expand_map(const int8_t *in, int n1, bool used, int32_t *out)
{
    for (int i = 0; i < SAT_MAXDIM; i++) out[i] = (used && i < n1) ? in[i] : -1;
}

// queue `launch` on the context's stream between its two timing events, wait for it, *kernel_ms (may be null) = the
// time between the events
template <typename F> int timed(sat_ctx *ctx, double *kernel_ms, F launch)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    const int rc = launch();
    if (rc != SAT_OK) return rc;
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (kernel_ms) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        *kernel_ms = ms;
    }
    return SAT_OK;
}
