// sat_pairs.hip - the pair modes (sat_search_pairs, sat_search_pairs_matches and, with sat_polish.hip, the polish;
// DESIGN.md 6c, 6e, 6h, 6j, 6l): chosen (query, entry) pairs instead of whole rows.  A pair list becomes work items of
// the SA kernels' pair instantiations: a score or record pass over every pair's restarts, their selection by the small
// kernels here, a map pass that re-runs the chosen ones for their maps.  Declared in sat_pairs.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sat_pairs.hpp"

namespace {

int order_bucket(int n2)
{
    int b = 0;
    while (b < kNumBuckets - 1 && n2 > kBucketMax[b]) b++;
    return b;
}

// the map pass's items name the winning restart of their pair: the low word of its key
__global__ void __launch_bounds__(256) pair_winners(SatPairItem *items, int n, const unsigned long long *keys)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = key_index(keys[items[i].pair]);
    items[i].r0 = r;
    items[i].r1 = r + 1;
}

__global__ void __launch_bounds__(256) pair_scores(const unsigned long long *keys, int n, int32_t *scores)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) scores[i] = key_score(keys[i]);
}

// Pair-match mode, the selection over the records of one pair (one workgroup per pair of a launch): the
// pair's slab holds, restart-major, the own best s_r of each of its R restarts and behind them the `setw[pair]` words
// of its db set D_r (the layout of the match kernel's slab; the items of the pair wrote them from several workgroups).
// Round 0 takes the largest key (s_r, ~r) - the pair's arg-max, which the record pass also folded into keys[pair]; a
// count of -1 reports a disagreement -, each later round the largest key with s_r > 0 whose set misses the union of
// the sets taken so far.  Writes counts[pair], scores / restarts [pair][M] (0 / -1 past the count).
__global__ void __launch_bounds__(256) pair_match_select(int pair0, int R, int M, const uint32_t *slabs, uint32_t slab_words,
                                                         const uint8_t *setw, const unsigned long long *keys, int32_t *counts,
                                                         int32_t *scores, int32_t *restarts)
{
    __shared__ unsigned long long red[4];
    __shared__ uint32_t uni[4];
    const int p = pair0 + (int)blockIdx.x;
    const uint32_t *rec = slabs + (size_t)blockIdx.x * slab_words;
    const int W = setw[p];
    const int t = (int)threadIdx.x, wave = t >> 6;
    if (t < 4) uni[t] = 0u;
    int m = 0;
    unsigned long long first = 0ull;
    for (int round = 0; round < M; round++) {
        __syncthreads();                               // the union of the round before; `red` is free again
        unsigned long long k = 0ull;
        for (int r = t; r < R; r += 256) {
            const int s = (int)rec[r];
            uint32_t hit = 0u;
            for (int w = 0; w < W; w++) hit |= rec[(size_t)(w + 1) * (size_t)R + (size_t)r] & uni[w];
            const unsigned long long rk = pair_key(s, (uint32_t)r);
            k = ((round == 0 || (s > 0 && hit == 0u)) && rk > k) ? rk : k;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long other = __shfl_xor(k, off, 64);
            k = other > k ? other : k;
        }
        if ((t & 63) == 0) red[wave] = k;
        __syncthreads();
        unsigned long long cur = red[0];
        for (int w = 1; w < 4; w++) cur = red[w] > cur ? red[w] : cur;
        if (cur == 0ull) break;                        // (the same for every thread: nothing left to take)
        if (round == 0) first = cur;
        const uint32_t r = (uint32_t)key_index(cur);
        if (t == 0) {
            scores[(size_t)p * M + m] = key_score(cur);
            restarts[(size_t)p * M + m] = (int32_t)r;
        }
        if (t < W) uni[t] |= rec[(size_t)(t + 1) * (size_t)R + (size_t)r];
        m++;
    }
    if (t == 0) {
        counts[p] = first == keys[p] ? m : -1;
        for (int x = m; x < M; x++) {
            scores[(size_t)p * M + x] = 0;
            restarts[(size_t)p * M + x] = -1;
        }
    }
}

// The polish modes' selection: pair_match_select without the set test.  One workgroup per pair of a
// launch, over the pair's record slab (restart-major: the R own bests first; the set words behind them are not read).  Round t takes the largest key below the one taken before - keys are distinct, their low
// word is the restart - so rank t holds the t-th restart by descending (s_r, -r).  Same outputs as pair_match_select:
// counts[pair] = min(T, R), or -1 when rank 0 is not the arg-max key the record pass folded into keys[pair]; scores /
// restarts [pair][T], 0 / -1 past the count.  (The keys are pair_key's, spelled out: through the helpers the compiler
// schedules this kernel differently, and its code stays what it was.)
__global__ void __launch_bounds__(256) pair_polish_select(int pair0, int R, int T, const uint32_t *slabs, uint32_t slab_words,
                                                          const unsigned long long *keys, int32_t *counts, int32_t *scores,
                                                          int32_t *restarts)
{
    __shared__ unsigned long long red[4];
    const int p = pair0 + (int)blockIdx.x;
    const uint32_t *rec = slabs + (size_t)blockIdx.x * slab_words;
    const int t = (int)threadIdx.x, wave = t >> 6;
    unsigned long long prev = ~0ull, first = 0ull;
    int m = 0;
    for (int round = 0; round < T; round++) {
        __syncthreads();                               // `red` is free again
        unsigned long long k = 0ull;
        for (int r = t; r < R; r += 256) {
            const int s = (int)rec[r];
            const unsigned long long rk = (((unsigned long long)(uint32_t)(s + 0x40000000)) << 32) | (0xFFFFFFFFu - (uint32_t)r);
            k = (rk < prev && rk > k) ? rk : k;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long other = __shfl_xor(k, off, 64);
            k = other > k ? other : k;
        }
        if ((t & 63) == 0) red[wave] = k;
        __syncthreads();
        unsigned long long cur = red[0];
        for (int w = 1; w < 4; w++) cur = red[w] > cur ? red[w] : cur;
        if (cur == 0ull) break;                        // (the same for every thread: fewer than T restarts)
        if (round == 0) first = cur;
        if (t == 0) {
            scores[(size_t)p * T + m] = (int32_t)(uint32_t)(cur >> 32) - 0x40000000;
            restarts[(size_t)p * T + m] = (int32_t)(0xFFFFFFFFu - (uint32_t)(cur & 0xFFFFFFFFu));
        }
        prev = cur;
        m++;
    }
    if (t == 0) {
        counts[p] = first == keys[p] ? m : -1;
        for (int x = m; x < T; x++) {
            scores[(size_t)p * T + x] = 0;
            restarts[(size_t)p * T + x] = -1;
        }
    }
}

// The two passes of the pair-match mode that run the SA kernel (launch_pair_pass): the match arguments and the
// restarts of a pair (the row length of its record slab).
struct PairMatchPass { SatMatchArgs mx; int maxstart; };

// The item groups of a pair list or of one chunk of it (build_pair_items): score items [goff[g], goff[g + 1]) and, with
// maps, map items [moff[g], moff[g + 1]) of the item table hold queries of class gcls[g] and entries of up to gn2[g] SSEs.
struct PairGroups { std::vector<size_t> goff, moff; std::vector<int> gcls, gn2; };

// One pass of the pair mode over the item groups of `grp` in d_items: its score items (map_pass = false) or its map
// items.  Score pass: the option-specialised LSOLN-off kernels, restarts per item at most `starts`.  Map pass: one restart per
// item, the general kernel with LSOLN, cut into launches whose best-map slabs stay under 256 MiB or the scratch budget,
// whichever is less (one stream: a launch reuses the region).
// pm: the pair-match mode's kernel instead (options from the arguments).  Its record pass (map_pass = false) is a score
// pass that also files the records (pm->mx.rec_slabs, set by the caller); its map pass runs the picked restarts of a
// pair as the chains of one item (workgroups sized for max_matches chains).
int launch_pair_pass(sat_ctx *ctx, int lorder, bool map_pass, int starts, const SatPairItem *d_items, const PairGroups &grp,
                     std::string &info, const PairMatchPass *pm = nullptr)
{
    hipStream_t stream = ctx->stream;
    const std::vector<size_t> &off = map_pass ? grp.moff : grp.goff;
    SatPairArgs px;
    px.items = nullptr;
    px.keys = ctx->d_pkeys.get();
    px.maps = ctx->d_pmaps.get();
    SatMatchArgs mpart = pm ? pm->mx : SatMatchArgs{};
    mpart.replay = map_pass ? 1 : 0;
    for (size_t g = 0; g < grp.gcls.size(); g++) {
        const int count = (int)(off[g + 1] - off[g]);
        if (count == 0) continue;
        // (the arguments' maxstart is unused by the pair mode's restart loop; the pair-match mode's records are laid out
        // by it.)  Entries per workgroup: the score pass as a plain launch; the map pass keeps one item per workgroup (its
        // one restart per item gains nothing from packing, and its best-map slabs are counted per item)
        SaLaunch l;
        int rc = prepare_launch(ctx, pm ? kPairMatch : kPair, lorder, map_pass && !pm, pm ? pm->maxstart : starts,
                            map_pass ? (pm ? pm->mx.max_matches : 1) : starts, grp.gcls[g], grp.gn2[g], count, !map_pass, l);
        if (rc != SAT_OK) return rc;
        SatKernelArgs &a = l.args;
        a.entry_list = nullptr;
        a.queries = ctx->d_qdesc.get();                 // items carry descriptor indices
#ifdef SAT_DIAG
        HIP_TRY(sat_diag_begin(stream, a.diag));
#endif
        int per_launch = count;
        if (map_pass) {
            const size_t slab_words = (size_t)((ctx->class_n1max[grp.gcls[g]] + 3) / 4) * (size_t)l.w.chains;
            const size_t budget = std::min(ctx->tune.scratch_bytes, (size_t)1 << 28) / 4;
            per_launch = (int)std::min<size_t>((size_t)count, std::max<size_t>(1, budget / slab_words));
            // one slab per entry slot of a launch, the spare slots of its last workgroup included (the kernel indexes
            // the slab by slot; with epw = 1 there are none)
            const size_t slabs = (size_t)per_launch + (size_t)l.epw - 1;
            if ((rc = ctx->d_bmap_slabs.grow_after(stream, slab_words * slabs)) != SAT_OK) return rc;
            a.bmap_slabs = ctx->d_bmap_slabs.get();
            a.bmap_slab_words = (uint32_t)slab_words;
        }
        for (int i0 = 0; i0 < count; i0 += per_launch) {
            const int n = count - i0 < per_launch ? count - i0 : per_launch;
            a.n_list = n;
            px.items = d_items + off[g] + (size_t)i0;
            HIP_TRY(launch_sa(l.k, dim3((n + l.epw - 1) / l.epw, 1), dim3(l.w.threads * l.epw), l.lds_launch, stream, a, &px, &mpart));
        }
        if (!info.empty()) info += "; ";
        info += launch_info(l.k, count, (count + l.epw - 1) / l.epw, 1, l.epw, l.w.threads, l.w.lds);
#ifdef SAT_DIAG
        HIP_TRY(sat_diag_end(stream));
#endif
    }
    return SAT_OK;
}

// Restarts per item.  A pair's R restarts on one workgroup of T chains take ceil(R / T) rounds at the latency
// of one workgroup: a few hundred pairs cannot fill the GPU that way.  Cut each pair into about
// kTargetItems / pairs items of whole rounds, never below one round (and no more items than rounds).
int pair_split(const sat_ctx *ctx, int maxstart, int npairs)
{
    if (ctx->tune.refine_split > 0) return ctx->tune.refine_split < maxstart ? ctx->tune.refine_split : maxstart;
    constexpr long long kTargetItems = 2048;        // 256 CUs x 8 workgroups
    const int t0 = std::min(256, (maxstart + 63) / 64 * 64);
    const long long rounds = (maxstart + t0 - 1) / t0;
    long long items = (kTargetItems + npairs - 1) / npairs;
    if (items > rounds) items = rounds;
    if (items < 1) items = 1;
    const long long per = (rounds + items - 1) / items;
    return (int)std::min<long long>(maxstart, per * t0);
}

// Append the items of pairs p0 .. p0 + n - 1 to `items`, grouped by (query class, entry order bucket) - a launch's LDS
// is sized for the class and the group's largest entry: the score items, each pair cut into items of `split` restarts,
// then (maps) one map item per pair in the same groups, its restarts filled in on the device.  SatPairItem::slab, read
// by the pair-match kernel only, numbers the pairs from p0.  setw (pair-match mode, else null): setw[p] = the set
// words of pair p's launch.
PairGroups build_pair_items(const sat_ctx *ctx, const int32_t *query, const int32_t *entry, int p0, int n, int maxstart, int split,
                            bool maps, std::vector<SatPairItem> &items, uint8_t *setw)
{
    std::vector<std::vector<int>> members(4 * kNumBuckets);
    std::vector<int> n2max(4 * kNumBuckets, 0);
    for (int p = p0; p < p0 + n; p++) {
        const int n2 = ctx->h_orders[(size_t)entry[p]];
        const int g = ctx->queries[(size_t)query[p]].cls * kNumBuckets + order_bucket(n2);
        members[(size_t)g].push_back(p);
        n2max[(size_t)g] = std::max(n2max[(size_t)g], n2);
    }
    auto item_of = [&](int p, int r0, int r1) {
        SatPairItem it{};
        it.pair = p;
        it.desc = ctx->queries[(size_t)query[p]].desc;
        it.entry = entry[p];
        it.r0 = r0;
        it.r1 = r1;
        it.slab = p - p0;
        return it;
    };
    PairGroups grp;
    grp.goff.push_back(items.size());
    for (int g = 0; g < 4 * kNumBuckets; g++) {
        if (members[(size_t)g].empty()) continue;
        for (int p : members[(size_t)g]) {
            if (setw) setw[p] = (uint8_t)satk::set_words(n2max[(size_t)g]);
            for (int r0 = 0; r0 < maxstart; r0 += split) items.push_back(item_of(p, r0, maxstart - r0 < split ? maxstart : r0 + split));
        }
        grp.goff.push_back(items.size());
        grp.gcls.push_back(g / kNumBuckets);
        grp.gn2.push_back(n2max[(size_t)g]);
    }
    if (maps) {
        grp.moff.push_back(items.size());
        for (int g = 0; g < 4 * kNumBuckets; g++) {
            if (members[(size_t)g].empty()) continue;
            for (int p : members[(size_t)g]) items.push_back(item_of(p, 0, 0));
            grp.moff.push_back(items.size());
        }
    }
    return grp;
}

}  // namespace

// sat_pairs.hpp
int sat_check_pairs(int nq, int n_entries, const int32_t *query, const int32_t *entry, int npairs)
{
    if (npairs < 0 || (npairs > 0 && (!query || !entry))) return sat_fail(SAT_EINVAL, "bad pair list");
    for (int p = 0; p < npairs; p++) {
        if (query[p] < 0 || query[p] >= nq) return sat_fail(SAT_EINVAL, "pair %d: query %d out of range", p, query[p]);
        if (entry[p] < 0 || entry[p] >= n_entries) return sat_fail(SAT_EINVAL, "pair %d: entry %d out of range", p, entry[p]);
    }
    return SAT_OK;
}

// sat_pairs.hpp: queue a pair search (both passes) on the context's stream
int sat_pairs_launch(sat_ctx *ctx, int lorder, int maxstart, bool maps, const int32_t *query, const int32_t *entry, int npairs)
{
    int rc = check_ready(ctx, true, maxstart);
    if (rc != SAT_OK) return rc;
    if ((rc = sat_check_pairs((int)ctx->queries.size(), ctx->n_entries, query, entry, npairs)) != SAT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = refresh_descriptors(ctx, false, ctx->stream)) != SAT_OK) return rc;
    ctx->last_launch_info.clear();
    if (npairs == 0) return SAT_OK;

    const int split = pair_split(ctx, maxstart, npairs);
    std::vector<SatPairItem> &items = ctx->h_pitems;
    HIP_TRY(hipStreamSynchronize(ctx->stream));      // the previous pair search's upload has read the table
    items.clear();
    const PairGroups grp = build_pair_items(ctx, query, entry, 0, npairs, maxstart, split, maps, items, nullptr);
    if ((rc = ctx->d_pitems.grow_after(ctx->stream, items.size())) != SAT_OK) return rc;
    if ((rc = ctx->d_pkeys.grow_after(ctx->stream, (size_t)npairs)) != SAT_OK) return rc;
    if (maps && (rc = ctx->d_pmaps.grow_after(ctx->stream, (size_t)npairs * SAT_MAXDIM)) != SAT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->d_pitems.get(), items.data(), items.size() * sizeof(SatPairItem), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->d_pkeys.get(), 0, (size_t)npairs * sizeof(unsigned long long), ctx->stream));
    std::string info;
    rc = launch_pair_pass(ctx, lorder, false, split, ctx->d_pitems.get(), grp, info);
    if (rc != SAT_OK) return rc;
    char head[96];
    snprintf(head, sizeof head, "score pass (%d restarts, %d per item): ", maxstart, split);
    ctx->last_launch_info = head + info;
    if (maps) {
        // the map items name the winning restart of their pair
        const size_t n_score = grp.moff[0];
        const int n_map = (int)(items.size() - n_score);
        HIP_TRY(hipMemsetAsync(ctx->d_pmaps.get(), 0xFF, (size_t)npairs * SAT_MAXDIM, ctx->stream));
        hipLaunchKernelGGL(pair_winners, dim3((unsigned)((n_map + 255) / 256)), dim3(256), 0, ctx->stream,
                           ctx->d_pitems.get() + n_score, n_map, ctx->d_pkeys.get());
        HIP_TRY(hipGetLastError());
        info.clear();
        rc = launch_pair_pass(ctx, lorder, true, 1, ctx->d_pitems.get(), grp, info);
        if (rc != SAT_OK) return rc;
        ctx->last_launch_info += " | map pass: " + info;
    }
    return SAT_OK;
}

int sat_pairs_collect(sat_ctx *ctx, int npairs, int32_t *scores, int32_t *ssemaps, const int32_t *query)
{
    HIP_TRY(hipSetDevice(ctx->device));
    if (npairs == 0) return SAT_OK;
    const int rc = ctx->d_pscores.grow_after(ctx->stream, (size_t)npairs);
    if (rc != SAT_OK) return rc;
    hipLaunchKernelGGL(pair_scores, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_pkeys.get(), npairs,
                       ctx->d_pscores.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(scores, ctx->d_pscores.get(), (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost));
    ctx->d2h_bytes += (size_t)npairs * sizeof(int32_t);
    return ssemaps ? sat_collect_maps(ctx, ctx->d_pmaps.get(), (size_t)npairs, 1, query, nullptr, nullptr, ssemaps) : SAT_OK;
}

// sat_pairs.hpp
int sat_collect_maps(sat_ctx *ctx, const int8_t *d_maps, size_t P, size_t M, const int32_t *query, const int32_t *counts,
                     const int32_t *where, int32_t *ssemaps)
{
    std::vector<int8_t> mp(P * M * SAT_MAXDIM);
    HIP_TRY(hipMemcpy(mp.data(), d_maps, mp.size(), hipMemcpyDeviceToHost));
    ctx->d2h_bytes += mp.size();
    for (size_t p = 0; p < P; p++)
        for (size_t m = 0; m < M; m++)
            expand_map(mp.data() + (p * M + m) * SAT_MAXDIM, ctx->queries[(size_t)query[p]].n1, !counts || (int32_t)m < counts[p],
                       ssemaps + ((where ? (size_t)where[p] : p) * M + m) * SAT_MAXDIM);
    return SAT_OK;
}

namespace {

// The plan of a pair-match list.  A pair's record slab holds the scores and the set words of its
// restarts, as wide as the widest set of the list (n2max: its largest entry); the list is cut into launches of as many
// pairs as the scratch budget holds slabs, at least one.  Once the items are built, what each launch covers: pairs
// p0 .. p0 + n - 1 and their item groups - grp.moff[0] is where its map items, one per pair, start in the item table.
struct PairMatchPlan {
    size_t slab_words;
    int per_launch, split;               // pairs of a launch; restarts per score item (pair_split)
    struct Launch { int p0, n; PairGroups grp; };
    std::vector<Launch> launches;
    PairMatchPlan(const sat_ctx *ctx, int n2max, int maxstart, size_t npairs)
        : slab_words((size_t)(1 + satk::set_words(n2max)) * (size_t)maxstart),
          per_launch((int)std::min(npairs, std::max<size_t>(1, ctx->tune.scratch_bytes / 4 / slab_words))),
          split(pair_split(ctx, maxstart, (int)npairs)) {}
};

}  // namespace

// sat_pairs.hpp.  Each launch of the plan runs its record pass, the selection, its map pass and what its mode adds
// (sat_polish.hip: a selection without the set test; behind the map pass the polish, then the scatter of the launch's
// rows) before the next one reuses the scratch, so no caller needs to know how the list was cut.
int sat_pair_matches_launch(sat_ctx *ctx, int lorder, int maxstart, int per_pair, bool maps, const int32_t *query,
                            const int32_t *entry, int npairs, PairMode mode)
{
    const bool polish = mode != PairMode::Matches, map_pass = maps || polish;      // (the polish works on the maps)
    PairMatchPass pm{};
    int rc = match_args(ctx, per_pair, pm.mx);
    if (rc != SAT_OK) return rc;
    if ((rc = check_ready(ctx, true, maxstart)) != SAT_OK) return rc;
    if ((rc = sat_check_pairs((int)ctx->queries.size(), ctx->n_entries, query, entry, npairs)) != SAT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = refresh_descriptors(ctx, false, ctx->stream)) != SAT_OK) return rc;
    ctx->last_launch_info.clear();
    if (npairs == 0) return SAT_OK;
    const size_t M = (size_t)per_pair;
    int n2_all = 0;
    for (int p = 0; p < npairs; p++) n2_all = std::max(n2_all, ctx->h_orders[(size_t)entry[p]]);
    PairMatchPlan plan(ctx, n2_all, maxstart, (size_t)npairs);

    // the items of every launch, one behind the other in the table
    std::vector<SatPairItem> &items = ctx->h_pitems;
    std::vector<uint8_t> &setw = ctx->h_psetw;
    HIP_TRY(hipStreamSynchronize(ctx->stream));      // the previous pair search's uploads have read the tables
    items.clear();
    setw.assign((size_t)npairs, 0);
    for (int p0 = 0; p0 < npairs; p0 += plan.per_launch) {
        const int n = std::min(plan.per_launch, npairs - p0);
        plan.launches.push_back({ p0, n, build_pair_items(ctx, query, entry, p0, n, maxstart, plan.split, map_pass, items, setw.data()) });
    }
    // outputs: counts [pairs], scores [pairs][M], restarts [pairs][M] in one array (one copy to the host), the maps
    if ((rc = ctx->d_pitems.grow_after(ctx->stream, items.size())) != SAT_OK ||
        (rc = ctx->d_pkeys.grow_after(ctx->stream, (size_t)npairs)) != SAT_OK ||
        (rc = ctx->d_psetw.grow_after(ctx->stream, (size_t)npairs)) != SAT_OK ||
        (rc = ctx->d_pmout.grow_after(ctx->stream, (size_t)npairs * (1 + 2 * M))) != SAT_OK ||
        (rc = ctx->d_bmap_slabs.grow_after(ctx->stream, plan.slab_words * (size_t)plan.per_launch)) != SAT_OK ||
        (map_pass && (rc = ctx->d_pmaps.grow_after(ctx->stream, (size_t)npairs * M * SAT_MAXDIM)) != SAT_OK) ||
        (polish && (rc = sat_polish_reserve(ctx, npairs)) != SAT_OK))
        return rc;
    HIP_TRY(hipMemcpyAsync(ctx->d_pitems.get(), items.data(), items.size() * sizeof(SatPairItem), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->d_psetw.get(), setw.data(), setw.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->d_pkeys.get(), 0, (size_t)npairs * sizeof(unsigned long long), ctx->stream));
    if (map_pass) HIP_TRY(hipMemsetAsync(ctx->d_pmaps.get(), 0xFF, (size_t)npairs * M * SAT_MAXDIM, ctx->stream));

    pm.maxstart = maxstart;
    pm.mx.n_entries = 0;                                 // (rows are pairs)
    pm.mx.rec_slab_words = (uint32_t)plan.slab_words;
    pm.mx.counts = ctx->d_pmout.get();
    pm.mx.scores = pm.mx.counts + npairs;
    pm.mx.restarts = pm.mx.scores + (size_t)npairs * M;
    pm.mx.maps = ctx->d_pmaps.get();
    std::string rec_info, map_info;
    for (const PairMatchPlan::Launch &ch : plan.launches) {
        // (the map pass of the launch before may have replaced the scratch with a larger one)
        pm.mx.rec_slabs = ctx->d_bmap_slabs.get();
        if ((rc = launch_pair_pass(ctx, lorder, false, plan.split, ctx->d_pitems.get(), ch.grp, rec_info, &pm)) != SAT_OK)
            return rc;
        const uint32_t *slabs = ctx->d_bmap_slabs.get();
        const unsigned long long *keys = ctx->d_pkeys.get();
        if (polish)
            hipLaunchKernelGGL(pair_polish_select, dim3((unsigned)ch.n), dim3(256), 0, ctx->stream, ch.p0, maxstart, per_pair, slabs,
                               (uint32_t)plan.slab_words, keys, pm.mx.counts, pm.mx.scores, pm.mx.restarts);
        else
            hipLaunchKernelGGL(pair_match_select, dim3((unsigned)ch.n), dim3(256), 0, ctx->stream, ch.p0, maxstart, per_pair, slabs,
                               (uint32_t)plan.slab_words, (const uint8_t *)ctx->d_psetw.get(), keys, pm.mx.counts, pm.mx.scores, pm.mx.restarts);
        HIP_TRY(hipGetLastError());
        if (map_pass && (rc = launch_pair_pass(ctx, lorder, true, 1, ctx->d_pitems.get(), ch.grp, map_info, &pm)) != SAT_OK)
            return rc;
        // the polish walks the launch's map items: one per pair, with its descriptor and entry.  An item group's entries
        // share an order bucket, and with it the width the polish runs at; neighbouring groups of one width go in one
        // launch (every launch ends on its slowest maps: fewer launches, fewer tails)
        if (polish)
            for (size_t g = 0; g < ch.grp.gcls.size();) {
                auto width_of = [&](size_t x) { return sat_polish_width(ctx, ch.n, per_pair, ch.grp.gn2[x], mode == PairMode::PolishPacked); };
                const int width = width_of(g);
                int n2max = ch.grp.gn2[g];
                size_t h = g + 1;
                for (; h < ch.grp.gcls.size() && width_of(h) == width; h++) n2max = std::max(n2max, ch.grp.gn2[h]);
                const int n = (int)(ch.grp.moff[h] - ch.grp.moff[g]);
                if (n > 0 && (rc = sat_polish_run(ctx, lorder, ctx->d_pitems.get() + ch.grp.moff[g], n, per_pair, n2max, npairs,
                                                  pm.mx.counts, pm.mx.scores, pm.mx.restarts, pm.mx.maps, width)) != SAT_OK)
                    return rc;
                g = h;
            }
        if (mode == PairMode::PolishPacked &&
            (rc = sat_polish_scatter(ctx, ctx->d_pitems.get() + ch.grp.moff[0], ch.n, npairs, maps)) != SAT_OK)
            return rc;
    }
    char head[128];
    snprintf(head, sizeof head, "record pass (%d restarts, %d per item, %zu launches of up to %d pairs): ", maxstart, plan.split,
             plan.launches.size(), plan.per_launch);
    ctx->last_launch_info = head + rec_info + " | select";
    if (map_pass) ctx->last_launch_info += " | map pass: " + map_info;
    if (polish) ctx->last_launch_info += " | polish";
    return SAT_OK;
}

// sat_pairs.hpp: wait for the pair-match search and copy its rows: 4 * npairs * (1 + 2 M) bytes, + 111 * npairs * M
// with maps
int sat_pair_matches_collect(sat_ctx *ctx, int max_matches, int npairs, int32_t *counts, int32_t *scores, int32_t *restarts,
                             int32_t *ssemaps, const int32_t *query, const int32_t *where)
{
    HIP_TRY(hipSetDevice(ctx->device));
    if (npairs == 0) return SAT_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t P = (size_t)npairs, M = (size_t)max_matches;
    std::vector<int32_t> out(P * (1 + 2 * M));
    HIP_TRY(hipMemcpy(out.data(), ctx->d_pmout.get(), out.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    ctx->d2h_bytes += out.size() * sizeof(int32_t);
    for (size_t p = 0; p < P; p++)
        if (out[p] < 1 || out[p] > (int32_t)M)
            return sat_fail(SAT_EDEVICE, "pair %zu: the records and the arg-max key of the record pass disagree", p);
    const int32_t *const src[3] = { out.data(), out.data() + P, out.data() + P + P * M };
    int32_t *const dst[3] = { counts, scores, restarts };
    for (size_t k = 0; k < 3; k++) {                     // (in place: one copy an array, as before there was a `where`)
        const size_t w = k ? M : 1;
        if (!where) memcpy(dst[k], src[k], P * w * sizeof(int32_t));
        for (size_t p = 0; where && p < P; p++) memcpy(dst[k] + (size_t)where[p] * w, src[k] + p * w, w * sizeof(int32_t));
    }
    return ssemaps ? sat_collect_maps(ctx, ctx->d_pmaps.get(), P, M, query, out.data(), where, ssemaps) : SAT_OK;
}

// sat_pairs.hpp: the polished form of a plain whole-shard search (the context's polish_all maps per row)
int sat_polish_all_launch(sat_ctx *ctx, int lorder, int lsoln, int maxstart)
{
    int rc = check_ready(ctx, true, maxstart);
    if (rc != SAT_OK) return rc;
    const int tops = ctx->polish_all;
    HIP_TRY(hipSetDevice(ctx->device));
    // the descriptors carry the rows' destinations: the score rows and, with lsoln, the map blocks
    if ((rc = refresh_descriptors(ctx, lsoln != 0, ctx->stream)) != SAT_OK) return rc;
    const size_t N = (size_t)ctx->n_entries, nq = ctx->queries.size(), rows = nq * N;
    if ((rc = ctx->d_base.grow_after(ctx->stream, ctx->d_scores.capacity())) != SAT_OK ||
        (rc = ctx->d_polerr.grow_after(ctx->stream, 1)) != SAT_OK)
        return rc;
    HIP_TRY(hipMemsetAsync(ctx->d_polerr.get(), 0, sizeof(int32_t), ctx->stream));
    // a launch: as many rows as the pair-match plan puts in one launch of its own, at most kPolishAllPairs
    int n2_all = 0;
    for (size_t e = 0; e < N; e++) n2_all = std::max(n2_all, ctx->h_orders[e]);
    const size_t chunk = (size_t)PairMatchPlan(ctx, n2_all, maxstart, std::min<size_t>(rows, (size_t)kPolishAllPairs)).per_launch;
    std::vector<int32_t> query, entry;
    size_t launches = 0;
    for (size_t r0 = 0; r0 < rows; r0 += chunk, launches++) {
        const size_t n = std::min(chunk, rows - r0);
        query.resize(n);
        entry.resize(n);
        for (size_t x = 0; x < n; x++) {
            query[x] = (int32_t)((r0 + x) / N);
            entry[x] = (int32_t)((r0 + x) % N);
        }
        // (the call waits for the launch before it: its tables and outputs are this launch's alone; it scatters its rows)
        if ((rc = sat_pair_matches_launch(ctx, lorder, maxstart, tops, lsoln != 0, query.data(), entry.data(), (int)n,
                                          PairMode::PolishPacked)) != SAT_OK)
            return rc;
    }
    char head[96];
    snprintf(head, sizeof head, "polish all (%d tops, %zu launches of up to %zu pairs): ", tops, launches, chunk);
    ctx->last_launch_info = head + ctx->last_launch_info;
    ctx->searched_nq = nq;
    ctx->searched_lsoln = lsoln != 0;
    ctx->searched_polished = true;
    ctx->searched_exact = false;
    ctx->fits.clear();                                   // a fit belongs to the scores it was made from
    return SAT_OK;
}

int sat_polish_all_check(sat_ctx *ctx)
{
    if (!ctx->searched_polished || ctx->searched_nq != ctx->queries.size()) return SAT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int32_t err = 0;
    HIP_TRY(hipMemcpy(&err, ctx->d_polerr.get(), sizeof err, hipMemcpyDeviceToHost));
    if (err)
        return sat_fail(SAT_EDEVICE, "a row's polish did not finish (records and arg-max key disagree, or the move cap was reached)");
    return SAT_OK;
}

// sat_pairs.hpp: load this file's code object (an empty launch of a small kernel)
int sat_pairs_load_code(sat_ctx *ctx)
{
    hipLaunchKernelGGL(pair_scores, dim3(1), dim3(256), 0, ctx->stream, nullptr, 0, nullptr);
    HIP_TRY(hipGetLastError());
    return SAT_OK;
}

extern "C" {

int sat_search_pairs(sat_ctx *ctx, int lorder, int lsoln, int maxstart, int npairs, const int32_t *query,
                     const int32_t *entry, int32_t *scores, int32_t *ssemaps, double *kernel_ms)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (npairs > 0 && !scores) return sat_fail(SAT_EINVAL, "scores buffer is null");
    if (lsoln && npairs > 0 && !ssemaps) return sat_fail(SAT_EINVAL, "lsoln set but ssemaps buffer is null");
    const int rc = timed(ctx, kernel_ms, [&] { return sat_pairs_launch(ctx, lorder, maxstart, lsoln != 0, query, entry, npairs); });
    if (rc != SAT_OK) return rc;
    return sat_pairs_collect(ctx, npairs, scores, lsoln ? ssemaps : nullptr, query);
}

int sat_search_pairs_matches(sat_ctx *ctx, int lorder, int maxstart, int max_matches, int npairs, const int32_t *query,
                             const int32_t *entry, int32_t *counts, int32_t *scores, int32_t *restarts, int32_t *ssemaps,
                             double *kernel_ms)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (npairs > 0 && (!counts || !scores || !restarts)) return sat_fail(SAT_EINVAL, "counts / scores / restarts buffer is null");
    const int rc = timed(ctx, kernel_ms, [&] {
        return sat_pair_matches_launch(ctx, lorder, maxstart, max_matches, ssemaps != nullptr, query, entry, npairs);
    });
    if (rc != SAT_OK) return rc;
    return sat_pair_matches_collect(ctx, max_matches, npairs, counts, scores, restarts, ssemaps, query);
}

}  // extern "C"
