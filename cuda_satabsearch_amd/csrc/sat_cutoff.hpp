// sat_cutoff.hpp - the two halves of sat_hits_cutoff (sat_topk.hip), shared with sat_multi.hip; not part of the
// public interface.
#pragma once

#include <stdint.h>

#include "satabsearch.h"

// After the checks sat_hits_cutoff makes on a context (a search has run; maps only after a search with LSOLN):
// the flag / count pass over every query of the last search.  counts[q] (host, n_queries entries) = rows of query q
// whose p-value is <= max_pvalue, uncapped.  Copies exactly 4 * n_queries bytes to the host.
int sat_cutoff_count(sat_ctx *ctx, double max_pvalue, bool maps, int32_t *counts);

// Right after sat_cutoff_count with the same max_pvalue and its counts: compaction, sort and finish, then the rows
// to the host in CSR order - query q's first min(max_rows, counts[q]) rows (all when max_rows <= 0) at the sum of
// the rows of the queries before it; maps (may be NULL) at the same row index times SAT_MAXDIM.
int sat_cutoff_rows(sat_ctx *ctx, double max_pvalue, int max_rows, const int32_t *counts, sat_hit *hits, int32_t *ssemaps);

// ---- for sat_cluster.hip (sat_cluster_add walks the same rows through the same predicate, cutoff_row of sat_hitrow.hpp).
// sat_hits_cutoff's state check: SAT_ESTATE unless a search has run since the last upload / query change.
int sat_check_searched(sat_ctx *ctx);
// queries per launch of a kernel shaped like the cutoff kernels (blocks of 1024 rows, whole blocks per query)
int sat_cutoff_chunk(const sat_ctx *ctx, int n);
// The HitQuery rows (sat_hitrow.hpp) of every query of the searched state into ctx->d_hitq, without maps, as
// sat_cutoff_count leaves them: an installed fit is followed.  Waits for the context's stream.
int sat_hitq_upload(sat_ctx *ctx);
