/*
 * satabsearch.h - C ABI of the MI355X tableau-search library (libsatabsearch.so).
 *
 * This is the drop-in boundary for ONE path of stivalaa/cuda_satabsearch: the
 * simulated-annealing scoring of one query against every database structure.
 * Plain C: pointers and sizes only, no HIP / torch / C++ types.  Each entry
 * point names the reference interface it stands in for (paths relative to the
 * reference tree, H.cu = nvcc_src_current/cudaSaTabsearch.cu,
 * K.cu = nvcc_src_current/cudaSaTabsearch_kernel.cu).
 *
 * Ownership: the caller owns every host buffer it passes; the context owns all
 * device memory.  Threading: one context per host thread; no globals.
 * Errors: every int-returning call yields 0 on success and a negative SAT_E*
 * code otherwise; sat_last_error() has the text.  Nothing in the library calls
 * exit() or abort().  (Tuning / test overrides of the launch heuristics: include/satabsearch_debug.h.)
 * There is no CPU fallback: without a usable HIP device sat_ctx_create() fails with
 * SAT_ENODEVICE.
 */
#ifndef SATABSEARCH_H
#define SATABSEARCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAT_ABI_VERSION   1
#define SAT_MAXDIM        111    /* saparams.h:15 (MAXDIM): largest structure order        */
#define SAT_MAXITER       100    /* saparams.h:33 (MAXITER): SA steps per restart           */
#define SAT_DEFAULT_SEED  1234   /* H.cu:263, :871                                           */
#define SAT_MAX_MATCHES   8      /* largest max_matches of sat_search_matches                */
#define SAT_MAX_CLUSTER_LEVELS 8 /* most p-value cutoffs of one leveled cluster accumulator  */

#define SAT_OK          0
#define SAT_EINVAL     -1   /* bad argument (order out of range, bad type code, ...)        */
#define SAT_ENODEVICE  -2   /* no HIP device / device index out of range                    */
#define SAT_ENOMEM     -3   /* host or device allocation failed                             */
#define SAT_EDEVICE    -4   /* a HIP call or the kernel launch failed (H.cu:1067-1073)      */
#define SAT_ESTATE     -5   /* call order violated (search before upload / query)           */

typedef struct sat_ctx sat_ctx;

/* Message of the most recent failure on this thread ("" if none). */
const char *sat_last_error(void);

/* Library ABI version (SAT_ABI_VERSION it was built with). */
int sat_abi_version(void);

/* Number of visible HIP devices; replaces cudaGetDeviceCount, H.cu:805-812. */
int sat_device_count(void);

/*
 * Create a context on HIP device `device` (the reference picks one device and
 * calls cudaSetDevice, H.cu:813-865, then allocates and seeds one RNG state per
 * thread with init_rng, H.cu:258-264, 896-922).  Here the random streams are
 * counter based, so `seed` is all the state there is: chain (query ordinal, db
 * ordinal, restart) draws from its own Philox4x32-10 stream.
 * Returns NULL on failure.
 */
sat_ctx *sat_ctx_create(int device, uint64_t seed);

/* Release every device and host resource of the context (H.cu:1117-1126, 1326-1337). */
void sat_ctx_destroy(sat_ctx *ctx);

/*
 * Upload a database shard given as packed lower triangles (the layout the
 * library's own reader produces, sat_parse.h):
 *   n_entries          structures in this shard
 *   orders[e]          number of SSEs of entry e, 1..SAT_MAXDIM
 *   cell_off[e]        index of entry e's first cell in tab_tri / dist_tri
 *   tab_tri, dist_tri  cell (i,j), j <= i, at cell_off[e] + i*(i+1)/2 + j;
 *                      diagonal of tab_tri = SSE type code 0..3, off-diagonal =
 *                      two-nibble tableau code (parsetableaux.c:13-33)
 *   db_ordinal[e]      position of entry e in the whole database's file order
 *                      (keys the random streams, so results do not depend on
 *                      how the database is sharded over GPUs); NULL = e
 * Replaces the cudaMalloc3D + cudaMemcpy3D of the dense 96x96 / 111x111 slots,
 * H.cu:924-967 and 1135-1177; both size classes go into the one packed store.
 */
int sat_db_upload_packed(sat_ctx *ctx, int n_entries, const int32_t *orders,
                         const int64_t *cell_off, const uint8_t *tab_tri,
                         const float *dist_tri, const int64_t *db_ordinal);

/*
 * Upload a shard AND run the first search of the current query (or query batch) over it, overlapped:
 * the shard goes up in a few pieces of whole entries, and each piece is checked and searched on the GPU
 * while the host copies the next one - a single query over a freshly read database then costs about
 * max(copy, search) instead of their sum (the reference copies the whole database, H.cu:924-967, then
 * launches, H.cu:1036).  Arguments as sat_db_upload_packed + sat_search_async; the query must be set
 * before.  On return the shard is resident and validated as after sat_db_upload_packed, and the search
 * has completed: collect with sat_results / sat_topk_hits / sat_device_scores.  Results are those of
 * sat_db_upload_packed followed by sat_search, bit for bit.  Entries laid out in ascending cell order
 * (as every reader here produces them) are needed for the overlap; otherwise, and for small shards,
 * the two steps simply run one after the other.  The copies are synchronous calls (the caller's buffers
 * may be pageable), so the overlap also needs the search on a stream they do not wait for: the context's
 * own (non-blocking) stream, or a non-blocking stream given to sat_use_stream; on the device's default
 * stream the pieces are copied and searched in turn - same results, no gain.
 */
int sat_db_upload_search(sat_ctx *ctx, int n_entries, const int32_t *orders,
                         const int64_t *cell_off, const uint8_t *tab_tri,
                         const float *dist_tri, const int64_t *db_ordinal,
                         int lorder, int lsoln, int maxstart);

/*
 * Same, from the reference's dense host layout: entry e occupies
 * pitch*pitch cells at tabs + e*pitch*pitch (row-major, symmetric), exactly the
 * arrays read_database() returns (parsetableaux.c:317-506; pitch 96 or 111).
 * Only the lower triangle is read.
 */
int sat_db_upload_dense(sat_ctx *ctx, int n_entries, const int32_t *orders,
                        const uint8_t *tabs, const float *dmats, int pitch,
                        const int64_t *db_ordinal);

/* Entries currently resident. */
int sat_db_size(const sat_ctx *ctx);

/*
 * Set the query: dense n1 x n1 code and distance matrices with row pitch
 * `pitch` (111 in the reference), SSE types in qssetypes[0..n1).  Replaces the
 * four cudaMemcpy to the c_qn / c_qtab / c_qdmat / c_qssetypes device symbols,
 * copyQueryToConstantMemory H.cu:486-558 and K.cu:118-121.  `query_ordinal` is
 * the query's index in the run (second key of the random streams).
 */
int sat_query_set(sat_ctx *ctx, int n1, const uint8_t *qtab, const float *qdmat,
                  int pitch, const uint8_t *qssetypes, uint32_t query_ordinal);

/*
 * Set a BATCH of queries that one sat_search scores together (grid = entries x queries
 * inside the launches): query q occupies pitch*pitch cells at qtabs + q*pitch*pitch and
 * qdmats + q*pitch*pitch, its SSE types pitch bytes at qssetypes + q*pitch, its order is
 * n1s[q]; its stream key is first_query_ordinal + q.  The reference loops over queries
 * with a sync, four cudaMemcpy and a launch each (H.cu:987-1115); query lists (-q) of
 * hundreds of SIDs are its main workload, and a small database alone cannot fill the GPU.
 * After this call every result buffer has one row per query, in the order given here.
 */
int sat_queries_set(sat_ctx *ctx, int n_queries, const int32_t *n1s, const uint8_t *qtabs,
                    const float *qdmats, int pitch, const uint8_t *qssetypes,
                    uint32_t first_query_ordinal);

/*
 * Set a batch of queries that are ENTRIES OF THE RESIDENT SHARD: query q is entry entry[q] (any order,
 * repeats allowed), its stream key first_query_ordinal + q.  The database is already on the device as packed triangles,
 * so nothing but the index list crosses from the host - 4 * n_queries bytes instead of up to 163 KB a query: a kernel
 * (one workgroup per query) reads the entry's raw uploaded cells and writes the query's part of the batch, byte for
 * byte what sat_queries_set builds on the host from the entry's dense arrays with the SSE types taken from the tableau
 * diagonal.  Afterwards the context is exactly as after that sat_queries_set call with the same ordinal - query count,
 * size classes, stream keys, no searched state, fitted statistics dropped, sat_polish_all_set kept - so every later
 * call returns bit-identical results.  An uploaded cell is a valid query cell by construction (the upload applies the
 * same rules), so there is nothing to reject beyond the indices.  Like sat_queries_set it first waits for the work
 * queued on the context's current stream; the kernel runs on that stream (sat_use_stream is honoured) and has finished
 * at return.  The batch is a copy: a later upload leaves it as it leaves any other batch.
 * n_queries < 1, entry == NULL and an index outside 0 .. n_entries - 1 (the message names its position) are SAT_EINVAL
 * and leave the previous batch intact; no database is SAT_ESTATE; a failed launch is SAT_EDEVICE.
 */
int sat_queries_from_db(sat_ctx *ctx, int n_queries, const int32_t *entry, uint32_t first_query_ordinal);

/*
 * MOTIF QUERIES: as sat_queries_from_db, but query q is a chosen list of entry[q]'s SSEs.  sse_begin
 * [n_queries + 1] is CSR into sse with sse_begin[0] == 0: query q's list l is sse[sse_begin[q] .. sse_begin[q + 1]), m
 * distinct 0-BASED SSE indices of the entry (order n), 1 <= m <= n, in ANY order; an empty range means the whole entry.
 * Query SSE i is entry SSE l[i]: an ascending list is a substructure, any other order a permuted one - under LORDER = T
 * the search then looks for that permuted topology.  (The reference's query builder, pytableaucreate.py -s, sorts its
 * list; the order is kept as given here.)  The query is exactly the structure of order m with
 *     tab[i][k]  = the entry's tab[max(l[i], l[k])][min(l[i], l[k])],
 *     dist[i][k] = the same cell of the entry's distances,
 *     SSE type i = the entry's tableau diagonal at l[i],
 * and its size class follows m, not n: five SSEs of a 101-SSE entry are a 16-wide query.  The kernel of
 * sat_queries_from_db gathers the list's packed sub-triangle from the entry's raw uploaded cells and expands that, so
 * afterwards the context is exactly as after sat_queries_set with these dense arrays and the same ordinal, and every
 * later call, in every mode, returns bit-identical results.
 * The call copies exactly 8 * n_queries + 4 + sse_begin[n_queries] bytes to the device - the indices, the offsets, the
 * list bytes, counted in sat_stat_query_h2d_bytes - and nothing comes back.
 * SAT_EINVAL, the previous batch intact: what sat_queries_from_db refuses; sse_begin or sse NULL; sse_begin[0] != 0 or
 * offsets that descend; a list longer than its entry's order; an index >= the order; an index twice in one list (the
 * message names the query's position and the offending SSE).  No database is SAT_ESTATE, a failed launch SAT_EDEVICE.
 */
int sat_queries_from_db_sses(sat_ctx *ctx, int n_queries, const int32_t *entry, const int32_t *sse_begin, const uint8_t *sse,
                             uint32_t first_query_ordinal);

/* Bytes sat_queries_set (the batch's whole blob), sat_queries_from_db (4 * n_queries) and sat_queries_from_db_sses
 * (8 * n_queries + 4 + the lists) have copied from the host to the device on this context since it was created. */
unsigned long long sat_stat_query_h2d_bytes(const sat_ctx *ctx);

/* Queries currently set (1 after sat_query_set). */
int sat_query_count(const sat_ctx *ctx);

/*
 * Run the search for the current query (or query batch) over the resident shard and wait.
 * With a batch of nq queries: scores is [nq][n_entries], ssemaps [nq][n_entries*SAT_MAXDIM].
 * Replaces the sa_tabsearch_gpu / sa_tabsearch_gpu_noshared launches, their
 * cudaDeviceSynchronize and the result cudaMemcpy, H.cu:1036-1087, 1219-1253
 * (kernel contract K.cu:756-802):
 *   lorder     keep sequence order of matched SSEs (LORDER)
 *   lsoln      also return the best SSE map (LSOLN)
 *   maxstart   restarts per db entry (-r, default 128)
 *   scores     [n_entries]            best score per entry, shard order
 *   ssemaps    [n_entries * SAT_MAXDIM] or NULL; entry e's map at e*SAT_MAXDIM,
 *              ssemaps[e*111 + i] = db SSE matched to query SSE i, or -1; only
 *              written when lsoln != 0 (same layout as K.cu:797-800, 1232)
 *   kernel_ms  (may be NULL) device time of the search kernels, launch -> sync,
 *              the window the reference times (H.cu:1036-1077)
 */
int sat_search(sat_ctx *ctx, int lorder, int lsoln, int maxstart,
               int32_t *scores, int32_t *ssemaps, double *kernel_ms);

/*
 * Several matches per entry: up to max_matches non-overlapping placements of the query in every database
 * structure (a motif that occurs twice in a chain is found twice).  Every (query, entry) runs the maxstart
 * restarts of sat_search, with the same streams.  Restart r's own best s_r is the largest of its initial
 * full score and its 100 proposed scores, map_r the state where s_r is first reached (strict >, the proposed
 * state, as for the LSOLN map), D_r the db SSEs map_r matches, key_r = (s_r, -r).  Walking the restarts by
 * descending key, the first is taken - exactly sat_search's score and LSOLN map - and each later r is taken
 * iff s_r > 0 and D_r is disjoint from the D of everything taken before, up to max_matches
 * (1..SAT_MAX_MATCHES, else SAT_EINVAL).  Results do not depend on the launch shape or the sharding.
 *   counts    [nq][n_entries]              matches found, 1..max_matches
 *   scores    [nq][n_entries][M]           s_r of match m; 0 past the count
 *   restarts  [nq][n_entries][M]           r of match m; -1 past the count
 *   ssemaps   [nq][n_entries][M][SAT_MAXDIM] map_r of match m as sat_search lays out a map, all -1 past
 *             the count; or NULL: the maps are not computed (their pass is skipped)
 *   kernel_ms as sat_search
 * Everything else sat_search rejects is rejected the same way.  The call leaves the buffers behind
 * sat_results / sat_topk / sat_topk_hits / sat_device_scores holding match 0's scores, as after
 * sat_search(lsoln = 0): ranking those gives the entries as a plain search ranks them.
 */
int sat_search_matches(sat_ctx *ctx, int lorder, int maxstart, int max_matches,
                       int32_t *counts, int32_t *scores, int32_t *restarts, int32_t *ssemaps,
                       double *kernel_ms);
/*
 * Pair search: one score per (query, entry) pair instead of the whole database.  query[p] is an index into the
 * current batch (sat_queries_set), entry[p] an index into the resident shard; pairs may come in any order, repeat,
 * and mix query size classes and entry sizes.  scores[p] is exactly what sat_search(lorder, lsoln, maxstart) writes
 * for row query[p], entry entry[p]; with lsoln, ssemaps[p * SAT_MAXDIM ..] is exactly that row's map (-1 past the
 * query's order).  Restart r of a pair is the same random stream wherever it runs, so the pair's restarts are cut
 * into ranges that run in parallel (SAT_EXP_REFINE_SPLIT in satabsearch_debug.h; results do not depend on the cut)
 * and their arg-max keys (score, -restart) are combined.  With lsoln the winning restart runs once more for its
 * map.  npairs == 0 does nothing.  kernel_ms as sat_search.  Leaves the buffers of sat_results / sat_topk /
 * sat_topk_hits untouched.
 */
int sat_search_pairs(sat_ctx *ctx, int lorder, int lsoln, int maxstart, int npairs, const int32_t *query,
                     const int32_t *entry, int32_t *scores, int32_t *ssemaps, double *kernel_ms);

/*
 * Pair-match search: the matches of sat_search_matches for a list of (query, entry) pairs instead of the whole
 * database.  query[p] / entry[p] as sat_search_pairs takes them (any order, repeats allowed, mixed size classes).
 *   counts    [npairs]                  \
 *   scores    [npairs][M]                | exactly what sat_search_matches(lorder, maxstart, max_matches) writes for
 *   restarts  [npairs][M]                | row (query[p], entry[p]): same greedy rule, same unused-slot values
 *   ssemaps   [npairs][M][SAT_MAXDIM]   /  (score 0, restart -1, map all -1); or NULL: no map pass
 * so slot 0 is sat_search's score and LSOLN map of the row.  Three passes: the pair kernel with the match mode's
 * per-restart record {s_r, D_r} (the restarts of a pair cut into items as in sat_search_pairs, SAT_EXP_REFINE_SPLIT;
 * the records go to the pair's slab in device memory), a selection kernel (one workgroup per pair: the greedy walk
 * over the pair's records), and with ssemaps a map pass that re-runs the picked restarts of each pair.  Results do not
 * depend on the cut into items, entries per workgroup, lanes per chain, cell layout, forced modes or sharding.  A slab
 * is (1 + set words) x 4 x maxstart bytes (set words: 1, 2 or 4 by the largest entry of the list); the list is cut
 * into launches whose slabs stay under 1 GiB.  npairs == 0 does nothing.  max_matches outside 1..SAT_MAX_MATCHES and
 * indices out of range are SAT_EINVAL, no database / no query SAT_ESTATE, as sat_search_matches and sat_search_pairs
 * reject them.  Leaves the buffers behind sat_results / sat_topk / sat_topk_hits / sat_hits_cutoff untouched: it runs
 * after them, on the rows they chose.  kernel_ms as sat_search.
 * Copies to the host exactly 4 * npairs * (1 + 2 * max_matches) bytes, + SAT_MAXDIM * npairs * max_matches with
 * ssemaps - nothing that depends on the database size.
 */
int sat_search_pairs_matches(sat_ctx *ctx, int lorder, int maxstart, int max_matches, int npairs, const int32_t *query,
                             const int32_t *entry, int32_t *counts, int32_t *scores, int32_t *restarts, int32_t *ssemaps,
                             double *kernel_ms);

/*
 * Pair search with a polish of the best restarts' maps.  The state sat_search reports for a pair is the
 * best one any restart VISITED, often not a local optimum of the search's own neighbourhood; this call climbs from the
 * own-best maps of the pair's `tops` best restarts to local optima and reports the best of them.
 *   Terms.  A map m gives every query SSE i an image m[i]: -1 or a db SSE, no db SSE twice.  term(i, j, k, l) is
 *     tscord(qtab[i][k], tab[j][l]) if fabsf(qd[i][k] - d[j][l]) <= 4.0f, else 0 - f32, exactly the search's arithmetic,
 *     and whatever the search scores 0 scores 0 here (NaN / inf cells, the sentinels).  row(i, j | m) is the sum of
 *     term(i, j, k, m[k]) over the k != i with m[k] >= 0; row(i, -1 | m) = 0.
 *   Moves from m.  (i, -1), unmatch, is allowed iff m[i] >= 0.  (i, j), j >= 0, is allowed iff type[j] == qtype[i] (type =
 *     the entry's tableau diagonal), j is no image of m and, under lorder, lo < j < hi with lo the largest image of a
 *     matched query SSE below i (-1 if none) and hi the smallest image of a matched query SSE above i (n2 if none).
 *     delta(i, j) = row(i, j | m) - row(i, m[i] | m).
 *   Polish of a map: apply the allowed move with the largest delta > 0 - ties to the smallest i, then the smallest j,
 *     -1 being the smallest j - until no allowed move has delta > 0.  The polished score is the map's score plus the
 *     deltas, i.e. the full score (tmscord) of the final map.  Every step gains at least 1 and scores are bounded, so it
 *     ends; the result is injective and type consistent, and under lorder still order preserving.
 *   Per pair: the maxstart restarts are ranked by the key (s_r, -r) exactly as sat_search_matches ranks them (s_r, map_r
 *     as defined there); the own-best maps of the first min(tops, maxstart) are polished to p_t; the winner is the
 *     largest p_t, ties to the lowest rank t.
 *   scores       [npairs]  p of the winner; always >= base_scores
 *   base_scores  [npairs]  s of rank 0: sat_search_pairs' score of the pair, bit for bit
 *   restarts     [npairs]  the winner's restart r
 *   moves        [npairs]  the moves its polish accepted
 *   ssemaps      [npairs][SAT_MAXDIM] its polished map, laid out as sat_search_pairs lays out a map
 * Every output except scores may be NULL.  tops is 1..SAT_MAX_MATCHES (the map pass runs at most that many chains per
 * pair).  Pairs as sat_search_pairs takes them (any order, repeats, mixed classes); npairs == 0 does nothing; what the
 * other pair searches reject is rejected the same way (SAT_EINVAL / SAT_ESTATE).  Passes per launch of the list (cut as
 * sat_search_pairs_matches cuts it): the pair-match record pass, a selection of the `tops` largest keys (no set test),
 * the pair-match map pass on those restarts, and the polish kernel - one workgroup per pair, one wave per map (in launches
 * of 16 384 maps or more a group of 16 or 32 lanes per map for entries of up to 16 / 32 SSEs, same results); a wave
 * that has not finished within 2 n1 (n1 - 1) + 1 rounds (which cannot happen: scores lie in [-n1 (n1 - 1), n1 (n1 - 1)])
 * makes the call fail with SAT_EDEVICE.  Nothing depends on the launch shape, cell layout, lanes per chain, entries per
 * workgroup, the cut into items or the sharding.  Leaves the buffers behind sat_results / sat_topk* / sat_hits_cutoff
 * alone and keeps an installed fit.  Copies 16 * npairs bytes to the host, + SAT_MAXDIM * npairs with ssemaps.
 */
int sat_search_pairs_polish(sat_ctx *ctx, int lorder, int maxstart, int tops, int npairs, const int32_t *query,
                            const int32_t *entry, int32_t *scores, int32_t *base_scores, int32_t *restarts, int32_t *moves,
                            int32_t *ssemaps, double *kernel_ms);

/*
 * Whole-database polish.  sat_polish_all_set(ctx, tops) with tops in 1..SAT_MAX_MATCHES turns every plain
 * whole-database search of the context - sat_search, sat_search_async, sat_db_upload_search, and through them
 * sat_multi_search, sat_multi_search_topk, sat_multi_search_cutoff and sat_multi_search_fit - into a polished search;
 * 0 (the default) turns it off again, after which not one bit of any result differs from a context that never had it
 * on; anything else is SAT_EINVAL.  It is a setting of the context, like its stream: uploads and query changes leave
 * it alone.  sat_polish_all_get returns it.
 *   Scores: the score of row (q, e) is exactly the scores[p] that sat_search_pairs_polish(lorder, maxstart, tops)
 *     returns for the pair (q, e) - same ranks, same tie-breaks, same min(tops, maxstart) -, and with lsoln the row's map
 *     is that pair's ssemaps row.
 *   The result buffers and the searched state are as after sat_search with these values: sat_results, sat_topk,
 *     sat_topk_hits, sat_hits_cutoff, sat_score_histogram, sat_stats_fit / sat_stats_set, sat_device_scores /
 *     sat_device_ssemaps and the multi-GPU gather work on polished rows.  An installed fit is dropped, as any new
 *     search drops it.  Without lsoln the maps are computed internally only: sat_results(lsoln = 1) is SAT_ESTATE.
 *   sat_results_base copies the rows' scores before the polish, [n_queries][n_entries]: rank 0's s, bit for bit what
 *     the plain search writes, from a device buffer the polished search fills.  SAT_ESTATE unless the last search of
 *     the context was a polished one.
 *   Not touched by the mode: sat_search_matches, the pair searches and stage 1 of every refine call stay plain.
 *     sat_search_timed is SAT_ESTATE while the mode is on (its window is defined for the plain search).
 *     sat_db_upload_search uploads, then searches, one after the other.
 *   The passes are sat_search_pairs_polish's over the pairs (q, e) in row order, cut into launches whose record slabs
 *     stay under 1 GiB and that hold at most 2^18 pairs; the polish runs a map on a group of 16 or 32 lanes for entries
 *     of up to 16 / 32 SSEs and on a wave above; the rows go from the polish's outputs straight into the result buffers
 *     on the device.  kernel_ms of sat_search covers all passes; sat_last_launch_info is "polish all (T tops, L launches
 *     of up to P pairs): " followed by the pair-match string of the last launch.  A row whose polish did not finish (it
 *     cannot happen, see above) fails sat_search, sat_sync and sat_results_base with SAT_EDEVICE.
 */
int sat_polish_all_set(sat_ctx *ctx, int tops);
int sat_polish_all_get(const sat_ctx *ctx);
int sat_results_base(sat_ctx *ctx, int32_t *base_scores);

/*
 * Queue all further work of this context on the caller's stream (`hip_stream` is a
 * hipStream_t passed as void*; NULL selects the device's default stream).  A context
 * starts on a private non-blocking stream; sat_use_own_stream() goes back to it.
 * Lets a caller order the search with its own copies / collectives (bench.py hands
 * over torch's current stream so that the RCCL gather follows the kernel).
 */
int sat_use_stream(sat_ctx *ctx, void *hip_stream);
int sat_use_own_stream(sat_ctx *ctx);

/*
 * Device-resident variant for callers that keep results on the GPU (bench.py,
 * torch.distributed gather over RCCL): launches on the context's current stream,
 * does not synchronise and does not copy.  Results land in the context's device
 * buffers:
 *   sat_device_scores()   int32 [n_queries][n_entries]
 *   sat_device_ssemaps()  int8, query q's [n_entries][n1_q] block after those of queries
 *                         0..q-1; -1 = unmatched; valid after a search with lsoln != 0
 * Pointer lifetime: ask for the pointers AFTER the search has been queued; they stay valid
 * (and keep that search's results) until the next database upload, the next query / query
 * batch change or a search with more queries or lsoln newly set - any of these may
 * re-allocate the buffers.
 * sat_query_order() is the order of query 0.
 */
int sat_search_async(sat_ctx *ctx, int lorder, int lsoln, int maxstart);
void *sat_device_scores(sat_ctx *ctx);
void *sat_device_ssemaps(sat_ctx *ctx);
int sat_query_order(const sat_ctx *ctx);

/* Wait for everything queued on the context's current stream. */
int sat_sync(sat_ctx *ctx);

/*
 * Wait for the queued search and copy its results to the host, same buffers and
 * layout as sat_search (ssemaps may be NULL when lsoln == 0).  SAT_ESTATE when no search
 * has run since the last upload / query change, or lsoln is asked of a search without it.  With sat_search_async
 * this lets one host thread keep several devices busy (one context per GPU, the
 * database sharded contiguously): launch on all, then collect from each - the
 * multi-GPU mode the reference left as a TODO (H.cu:790).
 */
int sat_results(sat_ctx *ctx, int lsoln, int32_t *scores, int32_t *ssemaps);

/*
 * Best-k hits of query `query` (0 for a single query) of the last search, selected and
 * sorted on the device: entry_index[i] / scores_out[i] for i < k, by descending score, ties
 * in database order - what `sort -k 2,2nr | head` does to the reference's output
 * (README_example_usage.txt:100).  Returns the number of hits written (min(k, n_entries))
 * or a negative SAT_E* code.  Waits for the queued search.
 */
int sat_topk(sat_ctx *ctx, int query, int k, int32_t *entry_index, int32_t *scores_out);

/*
 * One row of the reference's output, "name rawscore norm2score z-score p-value"
 * (cudaSaTabsearch.cu:445-453), for a best-k hit: the entry's index in the shard instead of its name.
 */
typedef struct sat_hit {
    int32_t entry;      /* index in the resident shard                                            */
    int32_t score;      /* raw score                                                              */
    double  norm2;      /* 2 * score / (n1 + n2)                         gumbelstats.c:91-94      */
    double  zscore;     /* Gumbel z of the norm2 score truncated to an int   gumbelstats.c:50-58  */
    double  pvalue;     /* 1 - exp(-exp(-(pi / sqrt 6 * z + gamma)))      gumbelstats.c:69-72     */
} sat_hit;

/*
 * Best-k rows of EVERY query of the last search, ranked and given their statistics on the device
 * (one segmented sort for the whole batch; the statistics are bit-identical to the host's
 * csrc/host/sat_gumbel.c): hits[q * k + r] is rank r of query q, by descending score, ties in
 * database order.  ssemaps (may be NULL): [n_queries * k * SAT_MAXDIM] solution maps of those rows,
 * laid out like sat_search's, after a search with lsoln.  Only these k rows per query are copied
 * to the host - what a user who pipes the reference's output through `sort -k 2,2nr | head`
 * wants (README_example_usage.txt:100, 256).  Returns min(k, n_entries) or a negative SAT_E* code.
 */
int sat_topk_hits(sat_ctx *ctx, int k, sat_hit *hits, int32_t *ssemaps);

/*
 * Every row of the last search whose p-value is <= max_pvalue (finite, >= 0; else SAT_EINVAL), selected on the
 * device.  A row qualifies iff the pvalue sat_topk_hits would give it - the same double, from the same table - is
 * <= max_pvalue; max_pvalue >= 1 takes every row.  Query q's rows are sat_topk_hits(n_entries)'s rows of q without
 * the ones that do not qualify (descending score, ties in database order, every field and map byte-equal), cut to
 * their first max_rows (max_rows <= 0: no cut).  The result is CSR:
 *   counts    [n_queries] rows of each query; always written (NULL is SAT_EINVAL)
 *   hits      query q's rows start at hits[counts[0] + .. + counts[q - 1]]
 *   ssemaps   (may be NULL) the rows' maps at the same row index times SAT_MAXDIM; after a search without lsoln
 *             SAT_ESTATE
 * Returns the total row count T or a negative SAT_E* code.  With hits == NULL or T > capacity only counts is written
 * (and T returned): grow the buffers and call again - that costs a selection, not a search, as does asking again with
 * another max_pvalue.  Never searches (SAT_ESTATE before the first search).  Cost: one flag / count pass over the
 * n_queries x n_entries scores, then compaction, a segmented sort and the rows of the qualifying rows only.  Copies
 * 4 * n_queries + 32 * T bytes (+ 444 * T with ssemaps) to the host; 4 * n_queries when only counts is written.
 */
int sat_hits_cutoff(sat_ctx *ctx, double max_pvalue, int max_rows, int32_t *counts, int capacity, sat_hit *hits,
                    int32_t *ssemaps);

/*
 * Refine: a cheap search of every entry, then a long search of each query's best candidates only.
 *   1. stage 1: sat_search(lorder, lsoln = 0, maxstart); the candidates of query q are its best C entries in
 *      sat_topk_hits order (descending score, ties in database order), C = min(candidates, n_entries)
 *   2. stage 2: sat_search_pairs over those candidates with refine_maxstart restarts (and lsoln)
 *   3. hits[q * K + r], K = min(k, C): the best K candidates of query q by stage-2 score, ties in database
 *      order, with norm2 / z / p of the stage-2 score from the same table as sat_topk_hits
 * ssemaps (may be NULL; written when lsoln): [n_queries * K * SAT_MAXDIM] the stage-2 maps of those rows.
 * first_scores (may be NULL): [n_queries * K] each row's stage-1 score.  Returns K or a negative SAT_E* code;
 * k < 1, candidates < 1, refine_maxstart < 1 and k > candidates are SAT_EINVAL.  Every stage-2 score is exactly
 * sat_search's at refine_maxstart, so refine_maxstart == maxstart gives exactly sat_topk_hits' rows.  Only the
 * K rows and the n_queries * C candidate indices are copied to the host.  The buffers of sat_results / sat_topk /
 * sat_topk_hits hold the stage-1 search afterwards.
 */
int sat_search_refine(sat_ctx *ctx, int lorder, int lsoln, int maxstart, int candidates, int refine_maxstart,
                      int k, sat_hit *hits, int32_t *ssemaps, int32_t *first_scores);

/*
 * sat_search_refine with stage 2 = sat_search_pairs_polish(refine_maxstart, tops) over the candidates:
 * refine_maxstart == maxstart polishes only.  The rows are ranked by polished score, ties in database order, with norm2 /
 * z / p of the polished score from the same table as sat_search_refine (the built-in constants: the statistics are not
 * calibrated to polished scores).  ssemaps (may be NULL; written when lsoln): the polished maps.  base_scores (may be
 * NULL) [n_queries * K]: each row's score before the polish, i.e. sat_search_refine's score of it.  Copies, beyond
 * sat_search_refine's rows, 4 bytes per candidate (the polish's completion flags).
 */
int sat_search_refine_polish(sat_ctx *ctx, int lorder, int lsoln, int maxstart, int candidates, int refine_maxstart,
                             int tops, int k, sat_hit *hits, int32_t *ssemaps, int32_t *first_scores, int32_t *base_scores);


/*
 * ---- Gumbel statistics fitted to the search's own scores.  Every z and p above comes from two
 * constants fitted once to one database, one restart count and one mix of queries (gumbelstats.h:21-23); the
 * reference's workflow re-fits them to the scores at hand (scripts/fitgumbeldist.r).  Here that happens on the
 * device, from a per-query integer histogram of the norm2 scores - integer counts do not depend on the order they
 * are added in and add up across shards, so the fit is identical for any launch shape and any sharding.
 *
 * Binning (one definition for host and device, csrc/host/sat_stats.h): a row with score >= 0 goes to bin
 * min((512 * score) / (n1 + n2), SAT_STAT_BINS - 1) = floor(norm2 * 256), the last bin taking every
 * norm2 >= 16 - 1/256; rows with score < 0 go into no bin and are counted in below[q].
 */
#define SAT_STAT_BINS           4096
#define SAT_STAT_BINS_PER_UNIT  256

#ifndef SAT_FIT_DEFINED
#define SAT_FIT_DEFINED
typedef struct sat_fit {
    double  a, b;       /* location and scale; the built-in constants when fitted == 0                       */
    int32_t rows;       /* rows in the histogram's bins                                                      */
    int32_t censored;   /* of them, rows above the censoring point (the overflow bin included)               */
    int32_t below;      /* rows with a negative score: in no bin, not fitted                                 */
    int32_t fitted;     /* 0: no fit exists, the query keeps the built-in statistics                         */
} sat_fit;
#endif

/*
 * The histogram of the last search's scores, made on the device (one LDS histogram per block of rows, integer
 * atomics only: bit-reproducible): counts [n_queries][SAT_STAT_BINS], below [n_queries].  As sat_hits_cutoff it
 * never searches (SAT_ESTATE before the first search).  Copies exactly n_queries * (SAT_STAT_BINS + 1) * 4 bytes.
 */
int sat_score_histogram(sat_ctx *ctx, uint32_t *counts, int32_t *below);

/*
 * Histogram, fit, install: each query's histogram goes through sat_gumbel_fit_binned of csrc/host/sat_gumbel.h (the
 * maximum-likelihood Gumbel of the bin midpoints, the top `censor` of the rows right-censored; censor in [0, 0.5],
 * else SAT_EINVAL) and the result is installed as by sat_stats_set.  fits (may be NULL) [n_queries] receives the
 * parameters; a query for which no fit exists (fewer than 2 occupied uncensored bins, no convergence) comes back
 * with fitted == 0 and keeps the built-in statistics.
 */
int sat_stats_fit(sat_ctx *ctx, double censor, sat_fit *fits);

/*
 * Install the caller's parameters for the current searched state: fits [n_queries]; queries with fitted == 0 keep the
 * built-ins, NULL puts every query back on them.  A query with a fit gets its own SAT_STAT_BINS-entry z / p tables on
 * the device, filled by the host's libm (sat_gumbel_fit_table: z and p at the LOWER edge of the row's bin), and every
 * row sat_topk_hits / sat_hits_cutoff give for it from then on - also the rows sat_hits_cutoff selects: a row still
 * qualifies iff the same double from the same table is <= max_pvalue - carries table entry clamp(bin, 0, 4095); a row
 * with score < 0 uses bin 0.  A fit belongs to the searched state: any new search (stage 1 of sat_search_refine and
 * sat_search_matches included), database upload or query change drops the context back to the built-in constants.  The
 * pair searches keep it: they leave the result buffers alone.  A fitted a or b that is not finite, or b <= 0, is
 * SAT_EINVAL; SAT_ESTATE before the first search.  (This is how sat_multi_search_fit installs the merged fit, and how
 * a calibration pooled over queries is installed.)
 */
int sat_stats_set(sat_ctx *ctx, const sat_fit *fits);

/*
 * ---- Single-linkage clustering of the database at a p-value, kept on the device.
 * Nodes are the structures of the WHOLE database in file order, 0 .. n_nodes - 1.  After a search, row (q, e) QUALIFIES
 * iff the p-value sat_hits_cutoff tests for it - the same double from the same table index, so a fit installed by
 * sat_stats_fit / sat_stats_set and the polished rows of sat_polish_all_set are followed - is <= max_pvalue.  A qualifying
 * row is an undirected EDGE between query_node[q] and the ordinal of entry e in the whole database (db_ordinal of the
 * upload); a row whose two ends are one node (a structure against itself) is no edge and is counted nowhere.
 *   label[v]   the smallest node of v's connected component: single linkage at the cutoff
 *   degree[v]  the edges with v at either end; repeats count each time (a pair that qualifies in both directions gives 2
 *              to each end)
 *   edges      the edges added, 64 bits
 * All three are integers and functions of the multiset of edges: nothing depends on the launch shape, the cut into
 * batches, the order of the sat_cluster_add calls or the sharding.
 *
 * sat_cluster_begin   start (or restart, emptied) the context's accumulator over n_nodes nodes.  Needs a resident database
 *                     (else SAT_ESTATE); n_nodes < 1 or a resident entry whose ordinal is >= n_nodes is SAT_EINVAL and
 *                     leaves an earlier accumulator as it was.
 * sat_cluster_add     add the qualifying rows of the last search (SAT_ESTATE before one, as sat_hits_cutoff, and without
 *                     an accumulator); query_node[q] is the node of query q of the batch.  query_node == NULL, a node
 *                     outside 0 .. n_nodes - 1 (the message names its position), a max_pvalue that is not finite or is
 *                     negative: SAT_EINVAL, nothing added.  Copies 4 * n_queries bytes (and the queries' table
 *                     pointers, as sat_hits_cutoff) to the device and NOTHING back: sat_stat_d2h_bytes does not move.  One
 *                     pass over the n_queries x n_entries scores on the context's current stream, behind the search; the
 *                     call does not wait for it.  Never searches, leaves the result buffers and an installed fit alone,
 *                     and may be called again: another batch, another cutoff.
 * sat_cluster_labels  wait, flatten the forest into labels (the accumulator stays as it is: more sat_cluster_add calls
 *                     may follow) and copy label[n_nodes], degree[n_nodes] and *edges: exactly 8 * n_nodes + 8 bytes.
 *                     degree and edges may be NULL: 4 * n_nodes, respectively 8, bytes fewer.  label == NULL is SAT_EINVAL.
 * sat_cluster_end     free the accumulator.
 * A database upload drops the accumulator (sat_cluster_add / sat_cluster_labels are then SAT_ESTATE until the next
 * sat_cluster_begin); query changes and searches keep it.
 */
int sat_cluster_begin(sat_ctx *ctx, int n_nodes);
int sat_cluster_add(sat_ctx *ctx, double max_pvalue, const int32_t *query_node);
int sat_cluster_labels(sat_ctx *ctx, int32_t *label, int32_t *degree, unsigned long long *edges);
int sat_cluster_end(sat_ctx *ctx);

/*
 * ---- The same clustering at several p-values in one pass: L = n_levels cutoffs max_pvalue[0] < ... <
 * max_pvalue[L - 1], 1 <= L <= SAT_MAX_CLUSTER_LEVELS, each finite and in [0, 1].  Nodes, rows and the double tested are
 * those above; row (q, e) is an edge of level j iff that double is <= max_pvalue[j] (a NaN qualifies nowhere) and its two
 * ends differ, so the edges of level j are among those of level j + 1.  Per level j, label[j][v], degree[j][v] and
 * edges[j] are exactly what the calls above return for the same add calls at max_pvalue[j] - integers, functions of the
 * multiset of edges - and the levels are NESTED: label[j + 1][v] == label[j + 1][label[j][v]].
 * A context holds ONE accumulator, plain (above) or leveled; the add and labels calls of the other kind are SAT_ESTATE,
 * with a message that names the kind that is active.  sat_cluster_end and a database upload drop either kind.
 *
 * The begin call      the checks of sat_cluster_begin, then the levels': n_levels outside 1 .. SAT_MAX_CLUSTER_LEVELS, a
 *                     null list, a cutoff that is not finite, lies outside [0, 1] or is not above the one before it
 *                     (the message names its position): SAT_EINVAL, and an earlier accumulator of either kind stays as it
 *                     was.  An accepted call replaces whatever accumulator there was.
 * The add call        sat_cluster_add for every level at once: its checks, copies, stream order and one pass over the
 *                     rows; each row's p-value is fetched once.  Nothing comes back: sat_stat_d2h_bytes does not move.
 * The labels call     wait, flatten every level's forest and copy label[L][n_nodes], degree[L][n_nodes] and edges[L],
 *                     tightest level first: exactly L * (8 * n_nodes + 8) bytes; degree and edges may be NULL (fewer
 *                     bytes).  The nesting is checked on the host (SAT_EDEVICE if it fails).  The forests stay usable
 *                     for more add calls.
 */
int sat_cluster_begin_levels(sat_ctx *ctx, int n_nodes, int n_levels, const double *max_pvalue);
int sat_cluster_add_levels(sat_ctx *ctx, const int32_t *query_node);
int sat_cluster_labels_levels(sat_ctx *ctx, int32_t *label, int32_t *degree, unsigned long long *edges);

/*
 * ---- Clustering the database around representatives: a greedy cover of the graph itself, kept on the device (DESIGN.md
 * 6r; the specification, the matrix layout and a plain-C restatement are in csrc/host/sat_cover.h).
 * Nodes, rows and the double tested are those of the single-linkage calls above.  A qualifying row whose two ends differ
 * is the UNDIRECTED edge {query_node[q], ordinal of e}: seen in both directions, or twice, it is ONE edge - unlike above,
 * where rows are counted.  The context keeps the adjacency as a bit matrix: n_nodes rows of ceil(n_nodes / 64) 64-bit
 * words, n_nodes^2 / 8 bytes (15 000 nodes: 28 MB).
 *   degree[v]  the DISTINCT neighbours of v
 *   edges      the distinct unordered pairs: the degrees' sum halved, 64 bits
 *   rep[v]     v's representative under the greedy cover: with every node unassigned, the unassigned node with the largest
 *              gain = 1 + its unassigned neighbours (ties: the smallest index) takes them as its cluster, and they leave;
 *              when the largest gain is 1 every node left is its own representative
 *   rounds     the clusters of two or more members
 * So every node is its representative or a neighbour of it, and no two representatives are neighbours; the solve checks
 * both on the device before it returns (SAT_EDEVICE if either is broken).  Everything is a function of the edge SET:
 * nothing depends on the launch shape, the batches, the order or repetition of the add calls, or the sharding.
 *
 * sat_cover_begin   start (or restart, emptied) the accumulator over n_nodes nodes; checks as sat_cluster_begin.  A matrix
 *                   that does not fit is SAT_ENOMEM, with the bytes it needs in the message.  It is an accumulator of its
 *                   own: the single-linkage one, plain or leveled, may live beside it on the context and neither sees the
 *                   other.
 * sat_cover_add     add the qualifying rows of the last search; arguments, checks, copies to the device and stream order
 *                   as sat_cluster_add.  NOTHING comes back: sat_stat_d2h_bytes does not move.
 * sat_cover_solve   wait, run the rounds and copy rep[n_nodes] (required: NULL is SAT_EINVAL), degree[n_nodes], *edges and
 *                   *rounds (each may be NULL).  The matrix is only read: more adds and another solve may follow.  The
 *                   rounds are queued SAT_COVER_ROUND_BATCH at a time and the host reads one 8-byte flag per batch, so
 *                   the call copies exactly 4 * n_nodes (+ 4 * n_nodes with degree) + 24 + 8 * (rounds /
 *                   SAT_COVER_ROUND_BATCH + 1) bytes, whether edges and rounds are asked for or not.
 * sat_cover_end     free the accumulator.  A database upload drops it too; query changes and searches keep it.
 */
#define SAT_COVER_ROUND_BATCH 64
int sat_cover_begin(sat_ctx *ctx, int n_nodes);
int sat_cover_add(sat_ctx *ctx, double max_pvalue, const int32_t *query_node);
int sat_cover_solve(sat_ctx *ctx, int32_t *rep, int32_t *degree, unsigned long long *edges, int *rounds);
int sat_cover_end(sat_ctx *ctx);

/* Bytes this context's result calls (sat_results, sat_search, sat_topk, sat_topk_hits, sat_hits_cutoff, the pair searches) have copied
 * from the device to the host since it was created (diagnostics: the best-k path moves O(k) rows). */
unsigned long long sat_stat_d2h_bytes(const sat_ctx *ctx);

/* Diagnostics: the kernel instantiations (template arguments as rocprofv3 prints them), grids, block
 * sizes and LDS bytes of the launches of this context's last search, "; "-separated.  After sat_search_matches:
 * "record pass: <launches>", followed by " | replay pass: <launches>" when maps were asked for.  After
 * sat_search_pairs: "score pass (R restarts, S per item): <launches>", followed by " | map pass: <launches>" with
 * lsoln; after sat_search_refine: "stage 1: <launches> || stage 2: <the pair search's>"; after sat_search_pairs_matches:
 * "record pass (R restarts, S per item, L launches of up to P pairs): <launches> | select", followed by
 * " | map pass: <launches>" when maps were asked for; after sat_search_pairs_polish the same with " | polish" at the end. */
const char *sat_last_launch_info(const sat_ctx *ctx);

/*
 * Diagnostics: the LDS carve of one entry slot of the SA kernel (csrc/sat_sa_kernel.hpp, lds_layout -
 * the one function both the kernel and the launch sizing use), byte offsets out[0..10] = code bytes,
 * query distances, query codes, chain maps, type masks, query types, LSOLN leader key, the waves'
 * arg-max keys, the byte stride between those keys (256: inside the item tables), item tables, total.
 * m2w = words of a db-side bit set in the launch's size class: 1 (entries up to 32 SSEs), 2 (64) or 4; its bits
 * 8-9 may name the cell layout, 1 + {0: full matrix of 8-byte cells, 1: full matrix in two arrays, 2: lower
 * triangle in two arrays} (0: the layout launches of such entries get).  With bit 16 of m2w set `out` has 14 words:
 * out[11..13] = per-query-SSE type masks, per-query-SSE run starts and the rank table of the LORDER pick (the three
 * arrays of launches with one-word db sets, between the query types and the leader key).
 * Lets tests assert alignment and monotonicity without a GPU.
 */
void sat_debug_lds_layout(int m2w, int n1, int n1p, int n2, int chains, int threads, int q_in_lds, int compact,
                          uint32_t out[11]);

/*
 * ---- one search over several GPUs of a node, driven from one host thread -------------------------
 * The reference is single-GPU (cudaSaTabsearch.cu:790 "TODO allow multiple GPUs").  A sat_multi
 * holds one context per GPU; the database is cut into contiguous shards of equal COST
 * (csrc/host/sat_shard.h: real databases are size sorted and a 96-SSE entry costs four 32-SSE
 * ones), each GPU holds its shard and the queries, a search is queued on all of them and ONE
 * gather (RCCL ncclGather over xGMI; SAT_MULTI_GATHER=peer: hipMemcpyPeerAsync; an RCCL gather that fails
 * at run time falls back to the peer copies for the rest of the context's life unless
 * SAT_MULTI_GATHER=rccl insists) brings the shard
 * rows to device 0, from where one copy takes them to the host in database file order.  Results
 * are identical for any number of GPUs (streams are keyed by the entry's ordinal in the database).
 *
 * sat_multi_create      ndev GPUs (<= 0: all visible; devices == NULL: 0 .. ndev-1; a list may name a GPU more
 *                       than once - several shards on one GPU, gathered by peer copies)
 * sat_multi_db_upload_packed   as sat_db_upload_packed for the WHOLE database (ordinals = file order), with ONE more
 *                       requirement: cell_off must ascend in file order without overlap (entry e + 1 starts at or
 *                       after the end of entry e - what every reader here produces), because a shard is uploaded
 *                       as a window of the packed arrays; anything else is SAT_EINVAL
 * sat_multi_shards      begin[ndev + 1]: shard g holds entries begin[g] .. begin[g+1]-1
 * sat_multi_queries_set as sat_queries_set, on every GPU
 * sat_multi_queries_from_db  as sat_queries_from_db with entry[q] an index into the WHOLE database: the shard that
 *                       holds the entry expands it, and that query's bytes go device to device into every other
 *                       shard's batch (a peer copy between GPUs, a plain copy where the list names one GPU twice);
 *                       each shard receives one 4-byte word per query from the host.  Every shard is then exactly as
 *                       after sat_multi_queries_set with the entries' dense arrays
 * sat_multi_queries_from_db_sses  as sat_queries_from_db_sses in the same way: the shard that holds the entry gathers and
 *                       expands the motif, the other shards keep room for a query of the list's length and take its
 *                       bytes device to device; each shard receives 8 * n_queries + 4 bytes and the lists of its OWN
 *                       queries from the host.  Every shard is then exactly as after sat_multi_queries_set with the
 *                       motifs' dense arrays
 * sat_multi_search      as sat_search: scores [nq][n_entries] (and ssemaps) in database order;
 *                       wall_ms = launch on all GPUs .. rows on the host
 * sat_multi_search_topk the best k rows per query, each GPU ranking its own shard (sat_topk_hits) and
 *                       the host merging ndev x k candidates; hits[q * k + r].entry is the index
 *                       in the whole database; ssemaps as in sat_topk_hits
 * sat_multi_gather_kind "rccl", "peer" or "none" (one GPU)
 */
typedef struct sat_multi sat_multi;
sat_multi *sat_multi_create(int ndev, const int *devices, uint64_t seed);
void sat_multi_destroy(sat_multi *m);
int sat_multi_device_count(const sat_multi *m);
const char *sat_multi_gather_kind(const sat_multi *m);
int sat_multi_db_upload_packed(sat_multi *m, int n_entries, const int32_t *orders, const int64_t *cell_off,
                               const uint8_t *tab_tri, const float *dist_tri);
int sat_multi_shards(const sat_multi *m, int32_t *begin);
int sat_multi_queries_set(sat_multi *m, int n_queries, const int32_t *n1s, const uint8_t *qtabs,
                          const float *qdmats, int pitch, const uint8_t *qssetypes, uint32_t first_query_ordinal);
int sat_multi_queries_from_db(sat_multi *m, int n_queries, const int32_t *entry, uint32_t first_query_ordinal);
int sat_multi_queries_from_db_sses(sat_multi *m, int n_queries, const int32_t *entry, const int32_t *sse_begin, const uint8_t *sse,
                                   uint32_t first_query_ordinal);
int sat_multi_search(sat_multi *m, int lorder, int lsoln, int maxstart, int32_t *scores, int32_t *ssemaps,
                     double *wall_ms);
int sat_multi_search_topk(sat_multi *m, int lorder, int lsoln, int maxstart, int k, sat_hit *hits,
                          int32_t *ssemaps, double *wall_ms);
/* sat_search_matches over every shard: counts [nq][n_entries], scores / restarts [nq][n_entries][M],
 * ssemaps [nq][n_entries][M][SAT_MAXDIM] or NULL, in database order; wall_ms as sat_multi_search.
 * Leaves every shard's context as sat_search_matches leaves it. */
int sat_multi_search_matches(sat_multi *m, int lorder, int maxstart, int max_matches, int32_t *counts,
                             int32_t *scores, int32_t *restarts, int32_t *ssemaps, double *wall_ms);
/* sat_search_refine over every shard, exactly what one context holding the whole database returns: each shard
 * ranks its own best C (as sat_multi_search_topk), the host merges them into the global best C of every query,
 * each shard re-scores the candidates in its range, the host merges the final rows (hits[].entry is the index in
 * the whole database).  wall_ms as sat_multi_search; stage2_ms (may be NULL) the part of it from the merged
 * candidates to the re-scored rows on the host.  Leaves every shard's context holding its stage-1 search. */
int sat_multi_search_refine(sat_multi *m, int lorder, int lsoln, int maxstart, int candidates, int refine_maxstart,
                            int k, sat_hit *hits, int32_t *ssemaps, int32_t *first_scores, double *wall_ms,
                            double *stage2_ms);
/* sat_search_pairs_matches with entry[p] an index into the WHOLE database, exactly what one context holding it returns:
 * the host routes every pair to the shard that holds its entry (sat_multi_shards), every shard runs its own pairs, the
 * host puts the rows back in the caller's order.  Only the pairs' rows cross to the host.  wall_ms as sat_multi_search.
 * Leaves every shard's last search as it was. */
int sat_multi_search_pairs_matches(sat_multi *m, int lorder, int maxstart, int max_matches, int npairs, const int32_t *query,
                                   const int32_t *entry, int32_t *counts, int32_t *scores, int32_t *restarts,
                                   int32_t *ssemaps, double *wall_ms);
/* sat_search_pairs_polish with entry[p] an index into the WHOLE database, and sat_search_refine_polish over every shard:
 * exactly what one context holding the whole database returns, routed and merged as sat_multi_search_pairs_matches and
 * sat_multi_search_refine do it.  wall_ms as sat_multi_search. */
int sat_multi_search_pairs_polish(sat_multi *m, int lorder, int maxstart, int tops, int npairs, const int32_t *query,
                                  const int32_t *entry, int32_t *scores, int32_t *base_scores, int32_t *restarts, int32_t *moves,
                                  int32_t *ssemaps, double *wall_ms);
int sat_multi_search_refine_polish(sat_multi *m, int lorder, int lsoln, int maxstart, int candidates, int refine_maxstart, int tops,
                                   int k, sat_hit *hits, int32_t *ssemaps, int32_t *first_scores, int32_t *base_scores,
                                   double *wall_ms);
/* sat_hits_cutoff over every shard, exactly what one context holding the whole database returns: each shard selects
 * its own rows (max_rows per query at most), the host merges them per query by score descending, then entry index in
 * the whole database ascending (hits[].entry), and cuts to max_rows.  Same CSR output, capacity contract and return
 * value; only counts and rows cross to the host, nothing proportional to n_entries.  sat_multi_search_cutoff searches
 * every shard first (wall_ms as sat_multi_search); sat_multi_hits_cutoff selects from every shard's last search again,
 * e.g. after a short capacity, without a new search. */
int sat_multi_search_cutoff(sat_multi *m, int lorder, int lsoln, int maxstart, double max_pvalue, int max_rows,
                            int32_t *counts, int capacity, sat_hit *hits, int32_t *ssemaps, double *wall_ms);
int sat_multi_hits_cutoff(sat_multi *m, double max_pvalue, int max_rows, int32_t *counts, int capacity, sat_hit *hits,
                          int32_t *ssemaps);
/* The fitted statistics over every shard, exactly what one context holding the whole database gives:
 * sat_multi_score_histogram sums the shards' integer histograms on the host (ndev * nq * (SAT_STAT_BINS + 1) * 4 bytes
 * cross to it), sat_multi_stats_set installs the same parameters on every shard, and sat_multi_search_fit searches
 * every shard WITHOUT a gather, sums the histograms, fits once (sat_stats_fit's censor) and installs the fit
 * everywhere; fits (may be NULL) [n_queries].  Afterwards sat_multi_hits_cutoff(P, K) returns the rows without a new
 * search; P >= 1 with max_rows = K is the best K rows of every query.  wall_ms as sat_multi_search. */
int sat_multi_score_histogram(sat_multi *m, uint32_t *counts, int32_t *below);
int sat_multi_stats_set(sat_multi *m, const sat_fit *fits);
int sat_multi_search_fit(sat_multi *m, int lorder, int lsoln, int maxstart, double censor, sat_fit *fits, double *wall_ms);
/* sat_polish_all_set with the same setting on every shard's context: sat_multi_search, sat_multi_search_topk,
 * sat_multi_search_cutoff and sat_multi_search_fit then work on polished rows, exactly those of one context holding
 * the whole database; the refine calls' stage 1, the match and the pair searches stay plain. */
int sat_multi_polish_all_set(sat_multi *m, int tops);
/* sat_multi_search_only searches every shard and waits - no gather, no copy: sat_multi_search_fit without the fit.
 * Afterwards sat_multi_hits_cutoff, sat_multi_score_histogram and sat_multi_cluster_add work on it.  wall_ms as
 * sat_multi_search.
 * The clustering over every shard, exactly what one context holding the whole database returns: every shard keeps an
 * accumulator over the WHOLE database's nodes (sat_multi_cluster_begin: n_nodes = the database size; SAT_ESTATE without
 * a database), into which sat_multi_cluster_add adds the edges that end at its own entries (query_node[q] a node of the
 * whole database; rejections as sat_cluster_add, checked before any shard adds).  sat_multi_cluster_labels brings every
 * shard's labels and degrees to the host (ndev * (8 * n_nodes + 8) bytes), joins the labels (sat_cluster_join of
 * csrc/host/sat_cluster.h) and sums degrees and edges; degree and edges may be NULL. */
int sat_multi_search_only(sat_multi *m, int lorder, int lsoln, int maxstart, double *wall_ms);
int sat_multi_cluster_begin(sat_multi *m);
int sat_multi_cluster_add(sat_multi *m, double max_pvalue, const int32_t *query_node);
int sat_multi_cluster_labels(sat_multi *m, int32_t *label, int32_t *degree, unsigned long long *edges);
/* The leveled accumulator over every shard (the calls of DESIGN.md 6p on each shard's context, n_nodes = the database
 * size): every shard keeps L forests over the whole database's nodes; the labels call brings every shard's arrays to
 * the host (ndev * L * (8 * n_nodes + 8) bytes), joins each level's labels with sat_cluster_join, sums degrees and edges
 * per level and checks the nesting.  Arguments, layouts and rejections as on one context. */
int sat_multi_cluster_begin_levels(sat_multi *m, int n_levels, const double *max_pvalue);
int sat_multi_cluster_add_levels(sat_multi *m, const int32_t *query_node);
int sat_multi_cluster_labels_levels(sat_multi *m, int32_t *label, int32_t *degree, unsigned long long *edges);
/* The cover over every shard, exactly what one context holding the whole database returns: every shard keeps a matrix
 * over the WHOLE database's nodes, into which sat_multi_cover_add adds the rows of its own entries (checks as
 * sat_multi_cluster_add, made before any shard adds).  sat_multi_cover_solve ORs the matrices of the shards 1 .. ndev - 1
 * into shard 0's, through the host - n_nodes * ceil(n_nodes / 64) * 8 bytes down and up again per extra shard, once per
 * solve - and solves there; an OR is idempotent, so shard 0's matrix stays a part of the whole graph and more adds and
 * solves may follow.  With one shard no matrix crosses. */
int sat_multi_cover_begin(sat_multi *m);
int sat_multi_cover_add(sat_multi *m, double max_pvalue, const int32_t *query_node);
int sat_multi_cover_solve(sat_multi *m, int32_t *rep, int32_t *degree, unsigned long long *edges, int *rounds);
/*
 * A search scored against a classification of the database, on the GPUs (the definitions and the one
 * reducing function are in csrc/host/sat_eval.h).  Nodes are the structures of the whole database in file order, as for
 * the clustering; node_class[v] >= 0 is node v's class, < 0 means unclassified.
 *
 * sat_eval_classes   installs the classes of n_nodes nodes: the class of every resident entry is kept on the device.
 *                    NULL removes them; a database upload drops them.  SAT_ESTATE without a database; SAT_EINVAL, and
 *                    nothing changes, for n_nodes < 1 or a resident entry whose ordinal is >= n_nodes.
 * sat_eval_rows      scores the LAST search (it never searches: SAT_ESTATE before one, and without installed classes):
 *                    query q is node query_node[q], of class c = node_class[query_node[q]].  Its counted rows are the
 *                    resident entries that are classified and are not the query's own node; a counted row is a positive
 *                    when its class is c, else a negative; rows are ranked by the raw score (polished where the search
 *                    was; an installed fit does not matter).  rows[q] is the struct below: with Pabove(s) the positives
 *                    above score s,
 *                        u2 = sum over s of neg[s] * (2 * Pabove(s) + pos[s]),   AUC   = u2 / (2 * positives * negatives)
 *                        t2 = the same sum over the first n_used = min(rocn, negatives) negatives from the top, a tie
 *                             group sharing what is left evenly,                 ROC-n = t2 / (2 * positives * n_used)
 *                    (both undefined when positives or negatives is 0).  A query whose own class is < 0 gets an all-zero
 *                    row with query_class = -1.  The tables are built and reduced on the device: 24 bytes a query go up
 *                    and exactly 32 come back.  The result buffers, an installed fit and a cluster accumulator are left
 *                    alone; a second call gives the same rows.  SAT_EINVAL, and nothing changes: rocn < 1, a null
 *                    pointer, a node outside 0 .. n_nodes - 1 (the message names its position).
 * sat_eval_tables    the raw tables instead of their reduction, for shards and tests: query q of order n1 has
 *                    bins = 2 * n1 * (n1 - 1) + 1 scores -n1 (n1 - 1) .. n1 (n1 - 1) (a score outside is clamped in);
 *                    its table is pos[bins] then neg[bins], bin = score + n1 (n1 - 1), and starts at counts[offset[q]].
 *                    offset = NULL packs the tables one after the other in query order (the sum of 2 * bins words).
 *                    Checks as sat_eval_rows.  Integer counts: the tables of the shards of a database add up.
 * sat_multi_eval_*   the same over every shard, exactly what one context holding the whole database returns, bit for
 *                    bit: n_nodes is the database size; each shard makes the tables of its own entries, the host sums
 *                    them and reduces (ndev * the tables' bytes cross to it); with one shard no table crosses.
 */
typedef struct sat_eval { uint64_t u2, t2; int32_t positives, negatives, n_used, query_class; } sat_eval; /* 32 bytes */
int sat_eval_classes(sat_ctx *ctx, int n_nodes, const int32_t *node_class);
int sat_eval_rows(sat_ctx *ctx, const int32_t *query_node, int rocn, sat_eval *rows);
int sat_eval_tables(sat_ctx *ctx, const int32_t *query_node, uint32_t *counts, const int64_t *offset);
int sat_multi_eval_classes(sat_multi *m, const int32_t *node_class);
int sat_multi_eval_rows(sat_multi *m, const int32_t *query_node, int rocn, sat_eval *rows);
/*
 * A query's SSEs profiled over its hits, on the GPUs (the core of a profile is csrc/host/sat_profile.h's).
 *
 * sat_profile_rows   profiles the LAST search (it never searches: SAT_ESTATE before one, and after one without lsoln -
 *                    the maps are what it reads).  A row (q, e) counts iff its p-value - the double sat_hits_cutoff
 *                    compares: an installed fit and a whole-database polish are followed - is <= max_pvalue and, where
 *                    query_node is not NULL and query_node[q] >= 0, the entry's ordinal in the whole database is not
 *                    query_node[q]: a structure is no hit of itself.  (No range check: a node no ordinal equals excludes
 *                    nothing.)  hits[q] is the number of counted rows; query q of order n1 has the n1 x n1 matrix, row-
 *                    major, full and symmetric, joint[offset[q] + i * n1 + k] = the counted rows whose map matches SSE i
 *                    and SSE k, the diagonal the rows that match SSE i at all.  offset = NULL packs the matrices one after
 *                    the other in query order (the sum of n1 * n1 words); words between the matrices are not written.
 *                    The counting is done on the device, in integers: exactly 4 * n_queries + 4 * sum(n1 * n1) bytes
 *                    come back, no row and no map.  The result buffers, an installed fit, the polish setting, a cluster
 *                    or cover accumulator and installed classes are left alone; a second call gives the same numbers.
 *                    SAT_EINVAL, and nothing changes: hits or joint NULL, max_pvalue negative or not finite.
 * sat_multi_profile_rows   the same over every shard, exactly what one context holding the whole database returns, bit
 *                    for bit: every check is made for every shard before the first one works; each shard profiles its
 *                    own entries and the host adds the matrices (ndev * the bytes above cross to it); with one shard
 *                    nothing is added.
 */
int sat_profile_rows(sat_ctx *ctx, double max_pvalue, const int32_t *query_node, uint32_t *hits, uint32_t *joint,
                     const int64_t *offset);
int sat_multi_profile_rows(sat_multi *m, double max_pvalue, const int32_t *query_node, uint32_t *hits, uint32_t *joint,
                           const int64_t *offset);
unsigned long long sat_multi_stat_d2h_bytes(const sat_multi *m);

/*
 * Hits that match only out of sequence order, on the GPUs (the order of a map is csrc/host/sat_reorder.h's).
 * Two searches of the same (database, query batch) are compared on the device: the first is KEPT as the baseline, the
 * second is the searched state every selection call works on; sat_reorder_hits reports the rows of the second that the
 * first does not call a hit and whose map has one of the asked-for orders.
 *
 * sat_baseline_keep   keeps the rows of the LAST search as the context's baseline: per row (q, e) its int32 score and
 *                    its p-value - the double sat_hits_cutoff compares at that moment, an installed fit and a whole-
 *                    database polish followed.  A small kernel on the context's stream; the call does not wait and
 *                    nothing crosses to the host (sat_stat_d2h_bytes does not move).  Costs 12 bytes a row of device
 *                    memory, kept until dropped.  SAT_ESTATE before a search.  The baseline belongs to (resident
 *                    database, query batch): a database upload and every query-setting call (sat_query_set, sat_queries_set,
 *                    sat_queries_from_db, sat_queries_from_db_sses - also with an unchanged shape) drop it; searches, the
 *                    pair searches, fits, sat_polish_all_set and the cluster, cover, eval and profile calls keep it.  A
 *                    second sat_baseline_keep replaces it.
 * sat_baseline_drop   forgets it (the memory stays with the context).
 * sat_baseline_results   the kept rows, [n_queries][n_entries] each; either array may be NULL.  Copies exactly 4 and /
 *                    or 8 bytes a row.  SAT_ESTATE without a baseline.
 * sat_reorder_hits   never searches.  Row (q, e) of the last search qualifies iff (1) sat_hits_cutoff's predicate passes
 *                    it at max_pvalue - the same double from the same table index -, (2) its kept base_pvalue is >=
 *                    min_base_pvalue (0: no condition) and (3) `kinds`, an OR of SAT_KIND_SEQUENTIAL (1),
 *                    SAT_KIND_CIRCULAR (2), SAT_KIND_PERMUTED (4), has the bit of its map's kind.  Output, order (score
 *                    descending, ties in database order), CSR layout, the cut to max_rows, the capacity contract (rows
 *                    NULL or T > capacity: only counts is written, T returned) and the return value are
 *                    sat_hits_cutoff's; rows[].hit is byte-equal to the sat_hit that call gives the row.  ssemaps (may
 *                    be NULL): the rows' maps, SAT_MAXDIM each.  Copies 4 * n_queries + 64 * T bytes (+ 444 * T with
 *                    ssemaps).  Integers and a fixed order throughout: the launch shape, the chunks of the query list
 *                    and the sharding cannot show in a byte.
 *                    SAT_ESTATE: no search has run; the last search ran without lsoln; no baseline; the baseline's shape
 *                    is not the current n_queries x n_entries.  SAT_EINVAL, nothing changed: counts NULL; a p-value
 *                    negative or not finite; kinds outside 1..7.
 * sat_search_reordered   the two searches in one call: the ordered search (lorder = 1, lsoln = 0), sat_stats_fit(censor)
 *                    when censor >= 0, sat_baseline_keep, the unordered search (lorder = 0, lsoln = 1), sat_stats_fit
 *                    again - each search fitted to its own scores.  Afterwards the searched state is the unordered
 *                    search's.  Both searches follow sat_polish_all_set as sat_search does: where it is on, the baseline
 *                    and the searched state hold polished rows, and sat_results_base works.  The baseline is kept behind
 *                    the first fit and before the second search: its p-values are the ordered search's under the ordered
 *                    search's own fit.  A censor outside [0, 0.5] is SAT_EINVAL before either search: nothing changes.
 *                    *kernel_ms (may be NULL): both searches' time on the stream.
 * sat_multi_*        the same over every shard; sat_multi_reorder_hits merges as sat_multi_hits_cutoff does (per query
 *                    by score, then by entry index in the whole database) and returns exactly what one context holding
 *                    the whole database returns; every check is made for every shard before the first one works.
 */
#define SAT_KIND_SEQUENTIAL 1   /* (as csrc/host/sat_reorder.h defines them) */
#define SAT_KIND_CIRCULAR   2
#define SAT_KIND_PERMUTED   4
#define SAT_KIND_ALL        7
typedef struct sat_reorder_hit {
    sat_hit hit;            /* the row sat_hits_cutoff gives                                             */
    double  base_pvalue;    /* the baseline's p-value of the row                                         */
    int32_t base_score;     /* and its raw score                                                         */
    int32_t kind;           /* SAT_KIND_* of the map                                                     */
    int32_t matched;        /* query SSEs the map matches                                                */
    int32_t descents;       /* places where the images step down                                         */
    int32_t cut;            /* circular: the 1-based query SSE at which the second run starts; else 0    */
    int32_t pad;            /* 0                                                                         */
} sat_reorder_hit;          /* 64 bytes */
int sat_baseline_keep(sat_ctx *ctx);
int sat_baseline_drop(sat_ctx *ctx);
int sat_baseline_results(sat_ctx *ctx, int32_t *scores, double *pvalues);
int sat_reorder_hits(sat_ctx *ctx, double max_pvalue, double min_base_pvalue, int kinds, int max_rows, int32_t *counts,
                     int capacity, sat_reorder_hit *rows, int32_t *ssemaps);
int sat_search_reordered(sat_ctx *ctx, int maxstart, double censor, double *kernel_ms);
int sat_multi_baseline_keep(sat_multi *m);
int sat_multi_baseline_drop(sat_multi *m);
int sat_multi_baseline_results(sat_multi *m, int32_t *scores, double *pvalues);
int sat_multi_reorder_hits(sat_multi *m, double max_pvalue, double min_base_pvalue, int kinds, int max_rows, int32_t *counts,
                           int capacity, sat_reorder_hit *rows, int32_t *ssemaps);
int sat_multi_search_reordered(sat_multi *m, int maxstart, double censor, double *wall_ms);

/*
 * Exact search for small queries: every row's score proven optimal, or improved, by a depth-first branch
 * and bound on the GPU behind the ordinary search.  No command-line option: the C ABI and the Python classes only.
 *
 * A feasible map of a query into an entry is a partial injective map between SSEs of equal type, under lorder with
 * images ascending in the query index; its score is the objective the search maximises (the reference's tmscord, K.cu:
 * 396-440): the sum of the pair terms of its matched pairs.  Every map the search or the polish reports is feasible; the
 * empty map scores 0.
 *
 * sat_search_exact   (1) the search the context's settings make, with lsoln (polished where sat_polish_all_set is on):
 *                    its rows are the incumbents, their scores the BASE scores.  (2) The proof pass: for every row a walk
 *                    over the feasible maps - query SSEs in index order, for each the allowed db SSEs ascending, then
 *                    "unmatched" -, a node (one such extension evaluated) pruned when its partial score plus an
 *                    admissible bound does not exceed max(incumbent, best found so far in its unit).  A row changes only
 *                    when a map STRICTLY better than the incumbent is found: otherwise its score and map are the
 *                    incumbent's byte for byte.  A row's parallel units are its top-level subtrees (the image of query SSE
 *                    0: n2 + 1 of them); among better maps of equal score each unit keeps its first, the lowest unit wins.
 *                    max_nodes, 1 .. 2^32 (SAT_EXACT_DEFAULT_NODES), bounds the nodes of one row: split evenly over its
 *                    units, a unit that spends its share stops and the row is flagged UNPROVEN - its score is then the
 *                    best feasible score known, a lower bound >= base.  A unit prunes with the incumbent and its own best
 *                    only, so score, map, flag and node count of a row depend on (query, entry, lorder, maxstart, seed,
 *                    polish setting, max_nodes) alone: not on the run, the launch cuts, SAT_EXP_* or the sharding.
 *                    Afterwards the context is in the state sat_search with lsoln leaves: scores and maps stand in the
 *                    ordinary buffers, fits are dropped, and sat_results, sat_topk_hits, sat_hits_cutoff,
 *                    sat_score_histogram / sat_stats_fit, the cluster, cover, eval and profile calls and
 *                    sat_baseline_keep work on the exact rows.  *kernel_ms (may be NULL): both parts' time on the stream.
 *                    Refusals, all SAT_EINVAL with a message, before anything is queued and with the searched state
 *                    unchanged: no database, no query, maxstart < 1, max_nodes outside 1 .. 2^32, a query of more than
 *                    SAT_EXACT_MAX_QUERY SSEs anywhere in the batch (either lorder).  Entries may have any order.
 * sat_exact_results  per row, laid out [n_queries][n_entries]; any pointer may be NULL: the base score, the unproven
 *                    flag (0 / 1), the nodes expanded (saturating at 2^32 - 1).  SAT_EINVAL unless the last search was
 *                    an exact one.
 * sat_exact_stats    per query, reduced on the device, 40 bytes a query back: rows, proven rows, improved rows
 *                    (score > base), the summed gain score - base, the summed nodes.
 * sat_multi_*        the same over every shard, rows left on the shards (as sat_multi_search_only); every refusal is made
 *                    for every shard before the first one works.  sat_multi_exact_results returns the whole database's
 *                    rows in file order - scores, ssemaps ([n_queries][n_entries][SAT_MAXDIM]) and the three arrays of
 *                    sat_exact_results, any pointer NULL - bit-equal to one context holding the whole database;
 *                    sat_multi_exact_stats sums the shards' statistics.
 */
#define SAT_EXACT_MAX_QUERY      16
#define SAT_EXACT_DEFAULT_NODES  (1ull << 18)
typedef struct sat_exact_stat {
    int64_t  rows;          /* rows of the query: the resident entries                 */
    int64_t  proven;        /* rows whose walk finished within max_nodes              */
    int64_t  improved;      /* rows with score > base                                  */
    int64_t  gain;          /* sum of score - base                                     */
    uint64_t nodes;         /* sum of the rows' node counts                            */
} sat_exact_stat;           /* 40 bytes */
int sat_search_exact(sat_ctx *ctx, int lorder, int maxstart, unsigned long long max_nodes, double *kernel_ms);
int sat_exact_results(sat_ctx *ctx, int32_t *base_scores, uint8_t *unproven, uint32_t *nodes);
int sat_exact_stats(sat_ctx *ctx, sat_exact_stat *per_query);
int sat_multi_search_exact(sat_multi *m, int lorder, int maxstart, unsigned long long max_nodes, double *wall_ms);
int sat_multi_exact_results(sat_multi *m, int32_t *scores, int32_t *ssemaps, int32_t *base_scores, uint8_t *unproven,
                            uint32_t *nodes);
int sat_multi_exact_stats(sat_multi *m, sat_exact_stat *per_query);

/*
 * ---- Transitive search: follow hits of hits from a seed, kept on the device (the key's layout and the
 * host-side functions are in csrc/host/sat_reach.h).  No command-line option: the C ABI and the Python classes only.
 * Nodes, qualifying rows and the double tested are those of sat_cluster_add.  A qualifying row (q, e) is the DIRECTED
 * step a -> b from a = query_node[q] to b = the ordinal of entry e; a row with a == b is none.  query_node[q] == -1 is an
 * EXTERNAL query, one not taken from the database: it has no self row and is recorded as parent -1.  Each node has one
 * 64-bit key - depth (63: unreached) above the bits of (float)p above the parent - and a support count; adding the rows
 * of a search at depth d does, for every step a -> b, atomicMin(key[b], pack(d, p, a)) and atomicAdd(support[b], 1).  So
 * a node keeps the shallowest depth it was ever reached at, within it the smallest float-rounded p, and of equal ones
 * the smallest parent node, external queries last.  Everything is integers and a function of the multiset of (depth,
 * row) pairs added: nothing depends on the launch shape, the cut of a level into batches, the order of the add calls or
 * the sharding.
 *
 * sat_reach_begin     start (or restart, emptied) the accumulator over n_nodes nodes with the n_seeds nodes of seed_node
 *                     at depth 0.  Checks as sat_cluster_begin; n_nodes above 2^27 - 1, n_seeds < 0, a null list with
 *                     n_seeds > 0, a seed outside 0 .. n_nodes - 1 or listed twice (the message names its position):
 *                     SAT_EINVAL, an earlier accumulator stays as it was.  n_seeds == 0 is allowed: an external start.
 * sat_reach_add       add the qualifying rows of the last search at `depth`; SAT_ESTATE as sat_cluster_add.  query_node
 *                     NULL, depth outside 1 .. 62, a max_pvalue that is not finite or negative, a node below -1 or above
 *                     n_nodes - 1 (the message names its position): SAT_EINVAL, nothing added.  Copies 4 * n_queries
 *                     bytes (and the queries' table pointers) to the device and NOTHING back.  One pass on the context's
 *                     stream behind the search; the call does not wait for it.
 * sat_reach_frontier  wait; *count = the nodes whose key has exactly `depth` (0 .. 62), and the first min(cap, *count) of
 *                     them, ascending, to `nodes` - compacted on the device.  Copies exactly 4 + 4 * min(cap, *count)
 *                     bytes.  count NULL, cap < 0, nodes NULL with cap > 0: SAT_EINVAL.
 * sat_reach_rows      the same for the REACHED nodes as rows: 4 + 20 * min(cap, *count) bytes; parent -1 for seeds and
 *                     external parents, pvalue 0 for seeds.  An unreached node never crosses to the host.
 * sat_reach_end       free the accumulator.  A database upload drops it too; query changes and searches keep it.
 *
 * sat_search_reach    the loop.  The seeds are entries of the resident database (outside it or listed twice: SAT_EINVAL);
 *                     the accumulator is restarted over max ordinal + 1 nodes (a resident ordinal of 2^27 - 1 or above:
 *                     SAT_EINVAL, before anything is allocated or changed).  Level d = 1, 2, ... takes the nodes at
 *                     depth d - 1 as queries, in ascending node order, in batches of `batch` (1 .. 256) built by
 *                     sat_queries_from_db, searches each batch with the context's ordinary search (lsoln off, polished
 *                     where sat_polish_all_set is on), installs sat_stats_fit(censor) if censor >= 0, and calls
 *                     sat_reach_add(d).  Query ordinals number the queries in the order searched, from
 *                     first_query_ordinal: a query's random stream does not depend on `batch`.  Before level d the loop
 *                     stops, in this order, when no node is at depth d - 1 (SAT_REACH_EXHAUSTED), when d - 1 ==
 *                     max_depth (1 .. 62; SAT_REACH_DEPTH), or when the level would take the queries searched past
 *                     max_queries (>= 1; SAT_REACH_BUDGET): a level is searched whole or not at all.  Then rows and
 *                     *count as sat_reach_rows(cap); the accumulator stays.  Between levels only the frontier list
 *                     crosses: 4 bytes a node up, and down again.  The result buffers afterwards hold the last batch.
 * sat_multi_*         every shard keeps keys and supports over the whole database's nodes and adds the rows of its own
 *                     entries; checks are made for every shard before the first one works; frontier and rows fetch the
 *                     shards' arrays and join them on the host (sat_reach_join: element-wise min and sum).  Bit-equal to
 *                     one context holding the whole database.  Seeds of sat_multi_search_reach are entries of the whole
 *                     database, which are its nodes.  sat_multi_reach_end frees every shard's
 *                     accumulator.
 */
#define SAT_REACH_EXHAUSTED 0
#define SAT_REACH_DEPTH     1
#define SAT_REACH_BUDGET    2
typedef struct sat_reach_row {
    int32_t node, depth, parent, support;
    float   pvalue;
} sat_reach_row;            /* 20 bytes */
typedef struct sat_reach_info {
    int32_t levels;         /* levels searched                                         */
    int32_t queries;        /* queries searched                                        */
    int32_t reached;        /* nodes reached, the seeds among them                     */
    int32_t stop;           /* SAT_REACH_EXHAUSTED / _DEPTH / _BUDGET                  */
    double  search_ms;      /* the searches' summed time (multi: wall clock)           */
    double  pass_ms;        /* the add passes' summed time                             */
} sat_reach_info;           /* 32 bytes */
int sat_reach_begin(sat_ctx *ctx, int n_nodes, int n_seeds, const int32_t *seed_node);
int sat_reach_add(sat_ctx *ctx, int depth, double max_pvalue, const int32_t *query_node);
int sat_reach_frontier(sat_ctx *ctx, int depth, int cap, int32_t *nodes, int32_t *count);
int sat_reach_rows(sat_ctx *ctx, int cap, sat_reach_row *rows, int32_t *count);
int sat_reach_end(sat_ctx *ctx);
int sat_search_reach(sat_ctx *ctx, int n_seeds, const int32_t *seed_entry, int lorder, int maxstart, double max_pvalue,
                     int max_depth, int max_queries, int batch, double censor, uint32_t first_query_ordinal, int cap,
                     sat_reach_row *rows, int32_t *count, sat_reach_info *info);
int sat_multi_reach_begin(sat_multi *m, int n_seeds, const int32_t *seed_node);
int sat_multi_reach_add(sat_multi *m, int depth, double max_pvalue, const int32_t *query_node);
int sat_multi_reach_frontier(sat_multi *m, int depth, int cap, int32_t *nodes, int32_t *count);
int sat_multi_reach_rows(sat_multi *m, int cap, sat_reach_row *rows, int32_t *count);
int sat_multi_reach_end(sat_multi *m);
int sat_multi_search_reach(sat_multi *m, int n_seeds, const int32_t *seed_entry, int lorder, int maxstart, double max_pvalue,
                           int max_depth, int max_queries, int batch, double censor, uint32_t first_query_ordinal, int cap,
                           sat_reach_row *rows, int32_t *count, sat_reach_info *info);

/*
 * Time `repeats` back-to-back searches with HIP events on the launch stream
 * (inputs resident, no copies inside the window).  Returns total milliseconds
 * in *total_ms and the dominant SA kernel's summed device time in *kernel_ms.
 * SAT_ESTATE while sat_polish_all_set is on.
 */
int sat_search_timed(sat_ctx *ctx, int lorder, int lsoln, int maxstart, int repeats,
                     double *total_ms, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* SATABSEARCH_H */
