// sat_pairs.hpp - the pair modes (sat_pairs.hip, sat_polish.hip) as the other translation units see them: a pair list
// is queued on a context, its rows are collected.  Not part of the public interface.
#pragma once

#include "sat_ctx.hpp"

// The 64-bit arg-max key of a restart or an entry: the biased score over the inverted index, so that the largest key is
// the highest score and, among equal scores, the lowest index (the SA kernels fold theirs into ctx->d_pkeys likewise).
__host__ __device__ inline unsigned long long pair_key(int32_t score, uint32_t index)
{
    return ((unsigned long long)(uint32_t)(score + 0x40000000) << 32) | (0xFFFFFFFFu - index);
}
__host__ __device__ inline int32_t key_score(unsigned long long key) { return (int32_t)(uint32_t)(key >> 32) - 0x40000000; }
__host__ __device__ inline int32_t key_index(unsigned long long key) { return (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu)); }

// Pair mode (sat_pairs.hip).  sat_pairs_launch queues both passes of a pair search on the context's stream (pair p:
// batch query query[p], shard entry entry[p], restarts 0 .. maxstart - 1; maps: also the map pass); the keys land in
// ctx->d_pkeys, the maps in ctx->d_pmaps.  sat_pairs_collect waits and copies scores (and maps, -1 past the query's
// order) to the host.  sat_check_pairs: a pair list as the pair searches take it - indices below nq queries and
// n_entries entries -, or SAT_EINVAL with the text that names the first bad pair.
int sat_check_pairs(int nq, int n_entries, const int32_t *query, const int32_t *entry, int npairs);
int sat_pairs_launch(sat_ctx *ctx, int lorder, int maxstart, bool maps, const int32_t *query, const int32_t *entry, int npairs);
int sat_pairs_collect(sat_ctx *ctx, int npairs, int32_t *scores, int32_t *ssemaps, const int32_t *query);
// The maps half of the three collects: M maps of SAT_MAXDIM bytes per pair from d_maps to the caller's int32 rows (pair
// p is of query query[p], goes to row where[p]; counts[p], when given: the slots of p that hold a map, the others all -1)
int sat_collect_maps(sat_ctx *ctx, const int8_t *d_maps, size_t P, size_t M, const int32_t *query, const int32_t *counts,
                     const int32_t *where, int32_t *ssemaps);

// Pair-match mode (sat_pairs.hip), the two halves of sat_search_pairs_matches: queue the record pass, the selection and
// (maps, and always in the polish modes) the map pass of every launch of the pair list on the context's stream; then
// wait and copy the row of pair p to row where[p] of the caller's arrays (NULL: row p; ssemaps may be NULL).  What the
// selection keeps of a pair's restarts is the mode:
enum class PairMode {
    Matches,        // up to `per_pair` non-overlapping matches (pair_match_select)
    Polish,         // the `per_pair` best restarts, each polished behind the map pass (sat_polish.hip)
    PolishPacked    // the whole-database mode: Polish with the lane-group kernel wherever the entries fit a group, and
                    // each launch's rows scattered to where a plain search puts them (`maps`: with their maps)
};
// per_pair: sat_search_pairs_matches' max_matches, sat_search_pairs_polish's tops - the rows of ranks a pair has.
int sat_pair_matches_launch(sat_ctx *ctx, int lorder, int maxstart, int per_pair, bool maps, const int32_t *query,
                            const int32_t *entry, int npairs, PairMode mode = PairMode::Matches);
int sat_pair_matches_collect(sat_ctx *ctx, int max_matches, int npairs, int32_t *counts, int32_t *scores, int32_t *restarts,
                             int32_t *ssemaps, const int32_t *query, const int32_t *where = nullptr);

// Polish (sat_polish.hip), the hooks of a polishing sat_pair_matches_launch and the second half of
// sat_search_pairs_polish: room for the outputs of `npairs` pairs; behind the selection (pair_polish_select: the ranks
// go to counts / scores / restarts as pair_match_select lays them out) and the map pass, the polish of the n pairs
// named by the launch's map items, entries of up to n2max SSEs (outputs in ctx->d_polout / d_polkeys / d_polmaps, rows
// indexed by the pair); wait and copy the rows, as sat_pair_matches_collect (every output but scores may be NULL).
// width: the lanes a map runs on, 16 or 32 (every entry of the items must fit) or 64; sat_polish_width chooses it for
// an item group (packed: PairMode::PolishPacked).
int sat_polish_reserve(sat_ctx *ctx, int npairs);
int sat_polish_run(sat_ctx *ctx, int lorder, const SatPairItem *d_map_items, int n, int tops, int n2max, int npairs,
                   const int32_t *counts, const int32_t *scores, const int32_t *restarts, const int8_t *maps, int width = 64);
int sat_polish_width(const sat_ctx *ctx, int launch_pairs, int tops, int n2max, bool packed);
int sat_polish_collect(sat_ctx *ctx, int npairs, int32_t *scores, int32_t *base_scores, int32_t *restarts, int32_t *moves,
                       int32_t *ssemaps, const int32_t *query, const int32_t *where = nullptr);

// Whole-database polish (sat_polish_all_set).  sat_polish_all_launch (sat_pairs.hip) is the polished form
// of launch_search over the whole shard on the context's stream: the pairs (q, e) in row order, in PolishPacked lists
// of at most kPolishAllPairs pairs, none longer than one launch of its plan, so that a list's scratch beyond the slabs
// - tops x SAT_MAXDIM map bytes, 16 x (1 + tops) bytes of ranks and rows and its items per pair - stays under 0.3 GiB.
// sat_polish_scatter (sat_polish.hip) puts a launch's rows (its n map items, rows of `npairs` pairs) into d_scores,
// d_base and, with maps, d_ssemaps.  sat_polish_all_check waits and fails with SAT_EDEVICE when a polish did not finish.
constexpr int kPolishAllPairs = 1 << 18;
int sat_polish_all_launch(sat_ctx *ctx, int lorder, int lsoln, int maxstart);
int sat_polish_scatter(sat_ctx *ctx, const SatPairItem *d_map_items, int n, int npairs, bool maps);
int sat_polish_all_check(sat_ctx *ctx);
// sat_pairs.hip's code object loaded now, not by the first pair search (sat_ctx_create)
int sat_pairs_load_code(sat_ctx *ctx);
