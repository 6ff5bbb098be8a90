// sat_cutoff.hpp - what the selection layer shares across sat_topk.hip, sat_cluster.hip and sat_multi.hip: the argument
// checks of its entry points (each text once), the walk over the chunks of a query list, the counted device-to-host
// copy, the fit of every query from a histogram, the searched-state functions sat_cluster_add uses too, and the two
// halves of sat_hits_cutoff.  Not part of the public interface.
#pragma once

#include <algorithm>
#include <cmath>
#include <stdint.h>
#include <vector>

#include "sat_pairs.hpp"                // the context, sat_fail - and sat_check_pairs, the pair lists' check of this kind
#include "host/sat_gumbel.h"

// a failed call of the library's own: its code goes up, the message stays what the call set
#define SAT_TRY(expr) do { const int rc__ = (expr); if (rc__ != SAT_OK) return rc__; } while (0)

// ---- Argument checks: SAT_OK, or the code and the text every entry point that takes the argument gives.  The entry
// points call them in the order their checks have always fired.
inline int sat_check_context(const void *ctx) { return ctx ? SAT_OK : sat_fail(SAT_EINVAL, "null context"); }
inline int sat_check_uploaded(bool uploaded) { return uploaded ? SAT_OK : sat_fail(SAT_ESTATE, "no database uploaded"); }
// a call that reads the solution maps of the last search (searched_lsoln: it kept them)
inline int sat_check_lsoln(bool searched_lsoln) { return searched_lsoln ? SAT_OK : sat_fail(SAT_ESTATE, "the last search ran without lsoln"); }
inline int sat_check_pvalue(double p) { return std::isfinite(p) && p >= 0.0 ? SAT_OK : sat_fail(SAT_EINVAL, "max_pvalue must be finite and >= 0"); }
// the cutoffs of a leveled cluster accumulator: 1 .. SAT_MAX_CLUSTER_LEVELS of them, each finite and in [0, 1], strictly ascending
inline int sat_check_levels(int n_levels, const double *max_pvalue)
{
    if (n_levels < 1 || n_levels > SAT_MAX_CLUSTER_LEVELS)
        return sat_fail(SAT_EINVAL, "n_levels must be 1..%d (got %d)", SAT_MAX_CLUSTER_LEVELS, n_levels);
    if (!max_pvalue) return sat_fail(SAT_EINVAL, "max_pvalue list is null");
    for (int j = 0; j < n_levels; j++) {
        if (!(std::isfinite(max_pvalue[j]) && max_pvalue[j] >= 0.0 && max_pvalue[j] <= 1.0))
            return sat_fail(SAT_EINVAL, "level %d: max_pvalue must be finite and lie in [0, 1]", j);
        if (j > 0 && !(max_pvalue[j] > max_pvalue[j - 1]))
            return sat_fail(SAT_EINVAL, "level %d: max_pvalue must be above level %d's (%g after %g)", j, j - 1, max_pvalue[j], max_pvalue[j - 1]);
    }
    return SAT_OK;
}
// (fit_rc: what sat_gumbel_fit_binned said to that censor - it refuses the same range)
inline int sat_check_censor(double c, int fit_rc = 0) { return c >= 0.0 && c <= 0.5 && !fit_rc ? SAT_OK : sat_fail(SAT_EINVAL, "censor must lie in [0, 0.5]"); }
inline int sat_check_tops(int tops)
{
    return tops >= 1 && tops <= SAT_MAX_MATCHES ? SAT_OK : sat_fail(SAT_EINVAL, "tops must be 1..%d (got %d)", SAT_MAX_MATCHES, tops);
}
// a best-k call's output buffers (`buffers`: none is null) and its k; the arguments of a refine call, on one context or sharded
inline int sat_check_topk(bool buffers, int k) { return buffers && k >= 1 ? SAT_OK : sat_fail(SAT_EINVAL, "bad top-k arguments"); }
inline int sat_check_refine(const void *ctx, const sat_hit *hits, int k, int candidates, int refine_maxstart)
{
    SAT_TRY(sat_check_context(ctx));
    SAT_TRY(sat_check_topk(hits != nullptr, k));
    if (candidates < 1) return sat_fail(SAT_EINVAL, "candidates must be >= 1 (got %d)", candidates);
    if (refine_maxstart < 1) return sat_fail(SAT_EINVAL, "refine_maxstart must be >= 1 (got %d)", refine_maxstart);
    if (k > candidates) return sat_fail(SAT_EINVAL, "k (%d) exceeds the candidates per query (%d)", k, candidates);
    return SAT_OK;
}

// The evaluation against a classification (sat_eval_*, sat_eval.hip; sat_multi_eval_* make the same checks for every
// shard before the first one works): the node count against the resident ordinals, installed classes, a call's rocn
// and buffers (`buffers`: none is null), the node of every query - the message names the first bad one's position
inline int sat_check_nodes(int n_nodes, uint32_t max_ordinal)
{
    if (n_nodes < 1) return sat_fail(SAT_EINVAL, "n_nodes must be >= 1 (got %d)", n_nodes);
    if (max_ordinal >= (uint32_t)n_nodes)
        return sat_fail(SAT_EINVAL, "n_nodes = %d, but a resident entry has ordinal %u in the whole database", n_nodes, max_ordinal);
    return SAT_OK;
}
inline int sat_check_eval_classes(bool installed)
{
    return installed ? SAT_OK : sat_fail(SAT_ESTATE, "no classes installed (sat_eval_classes has not been called since the last database upload)");
}
inline int sat_check_eval_args(int rocn, bool buffers)
{
    if (rocn < 1) return sat_fail(SAT_EINVAL, "rocn must be >= 1 (got %d)", rocn);
    return buffers ? SAT_OK : sat_fail(SAT_EINVAL, "null array");
}
inline int sat_check_query_nodes(int nq, const int32_t *query_node, int nodes)
{
    for (int q = 0; q < nq; q++)
        if (query_node[q] < 0 || query_node[q] >= nodes)
            return sat_fail(SAT_EINVAL, "query %d: node %d outside 0..%d", q, query_node[q], nodes - 1);
    return SAT_OK;
}

// the rows a query returns of the c that qualify: all of them when max_rows <= 0
inline int32_t sat_row_cap(int32_t c, int max_rows) { return max_rows > 0 && c > max_rows ? max_rows : c; }

// ---- The searched state (sat_topk.hip).  SAT_ESTATE unless a search has run since the last upload / query change.
int sat_check_searched(sat_ctx *ctx);
// queries per launch of a kernel shaped like the cutoff kernels (blocks of 1024 rows, whole blocks per query): under 2^31
// keys per sort and under 2^31 threads per launch - or under ctx->tune.select_keys of either
int sat_cutoff_chunk(const sat_ctx *ctx, int n);
// The HitQuery rows (sat_hitrow.hpp: hit_queries) of every query of the searched state into ctx->d_hitq - maps: with
// their solution maps of the last search; an installed fit is followed - and the wait for the context's stream: the
// rows' host copy dies there, and what the caller copies synchronously next is ordered behind the stream.
int sat_hitq_upload(sat_ctx *ctx, bool maps);

// ---- A query list in chunks of at most per_chunk queries: step(q0, nqc) for each in turn; the first error ends it.
template <typename F> int sat_query_chunks(int nq, int per_chunk, F step)
{
    for (int q0 = 0; q0 < nq; q0 += per_chunk) SAT_TRY(step(q0, std::min(nq - q0, per_chunk)));
    return SAT_OK;
}
// The searched state's queries for a pass of one thread per row, in blocks of block_rows rows of one query each:
// sat_cutoff_chunk's chunks, step(q0, nqc, bpq, grid) with bpq blocks per query and the chunk's grid of nqc * bpq blocks.
template <typename F> int sat_row_chunks(const sat_ctx *ctx, int block_rows, F step)
{
    const int n = ctx->n_entries, bpq = (n + block_rows - 1) / block_rows;
    return sat_query_chunks((int)ctx->queries.size(), sat_cutoff_chunk(ctx, n),
                            [&](int q0, int nqc) { return step(q0, nqc, bpq, dim3((unsigned)nqc * (unsigned)bpq)); });
}

// ---- Results to the host: `count` elements, and exactly their bytes added to what sat_stat_d2h_bytes reports.
// Synchronous, or (queued) on the context's stream, where the caller waits.  src_pitch: the leading T of `count` records
// of that many bytes each.
template <typename T> int sat_fetch(sat_ctx *ctx, T *dst, const T *src, size_t count, bool queued = false)
{
    if (queued) HIP_TRY(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    else HIP_TRY(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyDeviceToHost));
    ctx->d2h_bytes += count * sizeof(T);
    return SAT_OK;
}
template <typename T> int sat_fetch_strided(sat_ctx *ctx, T *dst, const void *src, size_t src_pitch, size_t count)
{
    HIP_TRY(hipMemcpy2D(dst, sizeof(T), src, src_pitch, sizeof(T), count, hipMemcpyDeviceToHost));
    ctx->d2h_bytes += count * sizeof(T);
    return SAT_OK;
}

// ---- sat_stats_fit and sat_multi_search_fit behind their checks and searches: histogram(counts, below) of the nq
// queries, each query fitted with the top `censor` of its rows censored, install(fit), and the fits to `fits` (may be null)
template <typename Hist, typename Install> int sat_fit_queries(size_t nq, double censor, sat_fit *fits, Hist histogram, Install install)
{
    std::vector<uint32_t> counts(nq * SAT_STAT_BINS);
    std::vector<int32_t> below(nq);
    SAT_TRY(histogram(counts.data(), below.data()));
    std::vector<sat_fit> fit(nq);
    for (size_t q = 0; q < nq; q++) {
        SAT_TRY(sat_check_censor(censor, sat_gumbel_fit_binned(counts.data() + q * SAT_STAT_BINS, censor, &fit[q])));
        fit[q].below = below[q];
    }
    SAT_TRY(install(fit.data()));
    if (fits) std::copy(fit.begin(), fit.end(), fits);
    return SAT_OK;
}

// ---- The two halves of sat_hits_cutoff (sat_topk.hip); sat_multi_hits_cutoff sums its shards' counts in between.
// After the checks sat_hits_cutoff makes on a context (a search has run; maps only after a search with LSOLN):
// the flag / count pass over every query of the last search.  counts[q] (host, n_queries entries) = rows of query q
// whose p-value is <= max_pvalue, uncapped.  Copies exactly 4 * n_queries bytes to the host.
int sat_cutoff_count(sat_ctx *ctx, double max_pvalue, bool maps, int32_t *counts);
// Right after sat_cutoff_count with the same max_pvalue and its counts: compaction, sort and finish, then the rows
// to the host in CSR order - query q's first min(max_rows, counts[q]) rows (all when max_rows <= 0) at the sum of
// the rows of the queries before it; maps (may be NULL) at the same row index times SAT_MAXDIM.
int sat_cutoff_rows(sat_ctx *ctx, double max_pvalue, int max_rows, const int32_t *counts, sat_hit *hits, int32_t *ssemaps);

// ---- The checks of sat_profile_rows (sat_profile.hip) behind the context's, in its order and nothing else: a search
// has run, with lsoln; the two arrays; the p-value.  sat_multi_profile_rows makes them for every shard before the first works.
int sat_profile_check(sat_ctx *ctx, double max_pvalue, const uint32_t *hits, const uint32_t *joint);

// ---- sat_reorder_hits (sat_reorder.hip) in three parts, for sat_multi_reorder_hits, which makes the checks for every
// shard before the first works and sums the shards' counts between the halves.  The checks behind the context's, in
// their order: a search has run, with lsoln; a baseline, of the searched shape; counts; the two p-values; kinds.  Then
// the halves, as sat_cutoff_count / sat_cutoff_rows above with the wider predicate and rows: counts[q] uncapped,
// 4 * n_queries bytes; the rows (64 bytes each) and maps (may be NULL) in CSR order.
int sat_reorder_check(sat_ctx *ctx, double max_pvalue, double min_base_pvalue, int kinds, const int32_t *counts);
int sat_reorder_count(sat_ctx *ctx, double max_pvalue, double min_base_pvalue, int kinds, int32_t *counts);
int sat_reorder_rows(sat_ctx *ctx, double max_pvalue, double min_base_pvalue, int kinds, int max_rows, const int32_t *counts,
                     sat_reorder_hit *rows, int32_t *ssemaps);
