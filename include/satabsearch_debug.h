/*
 * satabsearch_debug.h - what is NOT part of the drop-in boundary of satabsearch.h: environment overrides of the
 * library's launch heuristics, for tuning runs and tests.  Results never depend on them (the random streams are
 * keyed by query / db ordinal / restart, not by the launch shape); they are read ONCE by sat_ctx_create, never on
 * the search path.  Nothing here is needed to use the library.
 *
 *   SAT_EXP_LPC = 0|1|2          log2 lanes per restart chain (default: by LDS occupancy, size_workgroup in sat_launch.hip)
 *   SAT_EXP_LPC_WAVES = n        resident waves per CU at which that choice stops adding lanes (default 8; 12 for queries above 64 SSEs)
 *   SAT_EXP_CHAINS = 64|128|192 restart chains per workgroup (default: one per restart, at most 256)
 *   SAT_EXP_COMPACT = 0|1        wave-level work compaction of the SA step (default: exactly when LORDER)
 *   SAT_EXP_QLDS = 0|1           query cells staged in LDS (default: queries of up to 16 SSEs)
 *   SAT_EXP_LDS_PAD = bytes      unused LDS added per db entry (occupancy experiments)
 *   SAT_EXP_EPW = 1..8           db entries per workgroup (default: chosen per launch from the CU's LDS granules)
 *   SAT_EXP_GENERAL = 1          the general kernel instantiation instead of the option-specialised ones (prepare_sa in sat_launch.hip)
 *   SAT_EXP_REFINE_SPLIT = n     restarts per work item of a pair search (sat_search_pairs, sat_search_pairs_matches,
 *                                stage 2 of sat_search_refine; default: chosen so that the pairs x items fill the GPU,
 *                                whole rounds of the chains)
 *   SAT_EXP_POLISH_GROUP = 0|16|32|64  lanes a map of the polish runs on (sat_polish.hip; default 0: groups of 16 / 32 lanes for
 *                                entries of up to 16 / 32 SSEs in the whole-database mode and in large pair launches,
 *                                else a wave).  A forced width serves the entries it can hold; wider ones fall to the next
 *   SAT_EXP_SCRATCH_KB = n       scratch a search may take before it is cut into several launches, in KiB (default 0: 1 GiB; the
 *                                LSOLN best-map slabs of a plain or match search, the record slabs of a pair-match / polish
 *                                list, the map pass of the pair modes at most 256 MiB of it).  Every cut keeps one slab at least
 *   SAT_EXP_SELECT_KEYS = n      the most (query, entry) keys a chunk of a selection pass may hold (default 0: 2^31 - 1): best-k
 *                                (sat_topk_hits, stage 1 of the refine calls) cuts its query list into chunks of n / entries
 *                                queries, the p-value cutoff, the score histogram and sat_cluster_add into chunks of
 *                                n / (entries rounded up to whole blocks of 1024).  A chunk always holds one query at least
 *   SAT_EXP_STREAMS = 0           queue the order buckets of a search one after the other instead of concurrently
 *   SAT_EXP_UPLOAD_THREADS = n   host threads slicing the database copy (default 4)
 *   SAT_EXP_UPLOAD_TIMING = 1    per-phase upload times on stderr
 *   SAT_EXP_UPLOAD_PIECES = n    pieces of the overlapped upload + search (default by size, at most 8)
 *   SAT_MULTI_GATHER = rccl|peer the gather of sat_multi_* (default: RCCL, falling back to peer copies)
 *   SAT_PARSE_THREADS = n        threads of the mmap reader (libsathost; default: cores, at most 16)
 *   SAT_DEVICE_LIB = path        Python wrapper only: load another build of libsatabsearch.so (A/B runs)
 *
 * Diagnostic BUILDS (-DSAT_DIAG ..., cuda_satabsearch_amd/csrc/diag/sat_diag.hpp: phase timers, issue-sensitivity
 * perturbations, duplicated LDS accesses, the per-move self-check) are separate libraries made by
 * scripts/exp/variant_lib.sh and tests/native; the shipped library contains none of that code.  They export one
 * extra symbol:
 */
#ifndef SATABSEARCH_DEBUG_H
#define SATABSEARCH_DEBUG_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* diagnostic builds only: counters of the last search - [0..7] and [10] wave-cycles per phase of the kernel, [8] self-check
 * mismatches, [9] self-checks made */
void sat_diag_counters(unsigned long long out[16]);

/* Every build, a test hook: overwrite the device scores of the last search with the caller's [n_queries][n_entries]
 * array (and drop any fitted statistics, which belonged to the scores replaced).  Tests use it to reach negative
 * scores, the overflow bin and exact bin edges of the score histogram, which no real search produces on demand.
 * SAT_ESTATE before the first search. */
struct sat_ctx;
int sat_debug_set_scores(struct sat_ctx *ctx, const int32_t *scores);

/* Every build, a test hook: the instantiations of the SA kernel the library can launch - the distinct kernels its
 * dispatcher chooses over its whole argument domain (family, query class, set width and cell layout, query cells in
 * LDS or not, option code -1..11, words per lane 0..4) -, one name per line, each spelled exactly as
 * sat_last_launch_info spells it: "sat_sa_kernel<32, 1, false, 1, 4, 0>", "sat_sa_pair_kernel<...>", ...  Needs no
 * context and no device, and does not depend on the SAT_EXP_* environment.  The string lives as long as the library. */
const char *sat_debug_sa_instances(void);

/* Every build, a test hook: the current query batch as it lies on the device (per query qdist | qcode | qtypes |
 * qpair, input order).  Returns its size in bytes, or a negative SAT_E* code (SAT_ESTATE without a query batch); the
 * bytes are copied to `out` when it is not NULL and `capacity` holds them.  Tests compare the batches of
 * sat_queries_set and sat_queries_from_db with it. */
long long sat_debug_query_blob(struct sat_ctx *ctx, void *out, size_t capacity);

/* Every build, a test hook: the context of shard `shard` of a sat_multi (NULL outside 0 .. ndev - 1), for
 * sat_debug_query_blob and sat_stat_query_h2d_bytes - what each shard of sat_multi_queries_from_db(_sses) holds and was
 * sent.  The context stays the sat_multi's: read it with those two calls only, never set queries on it, search with it
 * or destroy it. */
struct sat_multi;
struct sat_ctx *sat_debug_multi_ctx(struct sat_multi *m, int shard);

/* Every build, a test hook: declare the kept baseline (sat_baseline_keep) to be of n_queries x n_entries rows, whatever
 * it holds.  An upload and every query change drop the baseline, so no sequence of public calls leaves one of another
 * shape than the searched state's; tests reach sat_reorder_hits' refusal of such a baseline with this.  The buffers are
 * not touched: put the true shape back before the baseline is read.  SAT_ESTATE without a baseline. */
int sat_debug_baseline_shape(struct sat_ctx *ctx, int n_queries, int n_entries);
#ifdef __cplusplus
}
#endif
#endif
