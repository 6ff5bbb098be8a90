// sat_capi.hip - C ABI (include/satabsearch.h) over the gfx950 SA kernel.
//
// Host side of the drop-in boundary: the context, the Metropolis table, the search modes' plans and launches, results.
// What goes up - the packed database store, the query buffer - is sat_db.hip; which SA kernel a launch runs and with
// which workgroup is sat_launch.hip, reached through sat_launch.hpp only.  Together they replace the device glue of
// nvcc_src_current/cudaSaTabsearch.cu (init_rng :258-264, copyQueryToConstantMemory :486-558, alloc/upload :896-984,
// launch/sync/download :1036-1087 and :1128-1270).  No CPU search path exists in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "satabsearch.h"
#ifdef SAT_DIAG
#define SAT_DIAG_HOST 1           // diagnostic builds only: the counters' host side (diag/sat_diag.hpp)
#endif
#include "sat_sa_kernel.hpp"
#include "sat_ctx.hpp"
#include "host/sat_gumbel.h"

namespace {

thread_local char g_err[512] = "";

}  // namespace

int sat_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

namespace {

int build_metropolis_table(sat_ctx *ctx)
{
    // P[iter][nd] = expf((float)(-nd) / temp_iter), temp_0 = 10, temp *= 0.95f per step
    // (saparams.h:34-37, K.cu:1030, 1166, 1189), computed with the host libm.  A draw
    // u is never below 2^-32 (rocrand_uniform.h:65-68), so entries <= 2^-32 can never
    // accept and each row is cut after its last entry above that bound.
    const int max_nd = 4 * (SAT_MAXDIM - 1);     // |delta| <= 4 per other query SSE
    const float umin = 2.3283064e-10f;
    std::vector<float> tab;
    std::vector<int32_t> rows(2 * SAT_MAXITER);
    volatile float temp = 10.0f;
    for (int it = 0; it < SAT_MAXITER; it++) {
        int last = 0;
        std::vector<float> row(max_nd + 1);
        for (int nd = 0; nd <= max_nd; nd++) {
            volatile float x = (float)(-nd) / temp;
            row[nd] = expf(x);
            if (row[nd] > umin) last = nd;
        }
        rows[2 * it] = (int32_t)tab.size();
        rows[2 * it + 1] = last;
        // stored times 2^32 (exact): the kernel compares with 2^32 * u.  The row is indexed by
        // 1 - delta clamped to [0, last + 2]: a leading 2^33 for every delta > 0 (expf(x > 0) > 1 >= u)
        // and a trailing 0.0 for "can never be accepted"
        tab.push_back(8589934592.0f);
        for (int nd = 0; nd <= last; nd++) tab.push_back(ldexpf(row[nd], 32));
        tab.push_back(0.0f);
        temp = temp * 0.95f;
    }
    int rc;
    if ((rc = ctx->d_ptab.grow(tab.size())) != SAT_OK || (rc = ctx->d_prow.grow(rows.size())) != SAT_OK) return rc;
    HIP_TRY(hipMemcpy(ctx->d_ptab.get(), tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->d_prow.get(), rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return SAT_OK;
}

int build_gumbel_tables(sat_ctx *ctx)
{
    // the reference computes z from the norm2 score TRUNCATED TO AN INT (gumbelstats.h:26 vs H.cu:446),
    // so z and p take one value per integer: tabulated here with the host's libm for x = -128 .. 127
    // (|norm2| <= 110), the device's best-k rows look them up (sat_topk.hip)
    double z[256], p[256];
    for (int x = -128; x < 128; x++) {
        z[x + 128] = sat_z_gumbel_trunc((double)x);
        p[x + 128] = sat_pv_gumbel(z[x + 128]);
    }
    int rc;
    if ((rc = ctx->d_gumbel_z.grow(256)) != SAT_OK || (rc = ctx->d_gumbel_p.grow(256)) != SAT_OK) return rc;
    HIP_TRY(hipMemcpy(ctx->d_gumbel_z.get(), z, sizeof z, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->d_gumbel_p.get(), p, sizeof p, hipMemcpyHostToDevice));
    return SAT_OK;
}

// the SatKernelArgs fields every launch shares: the database shard, the options, the Metropolis table; no slabs
SatKernelArgs base_args(const sat_ctx *ctx, int lorder, int lsoln, int maxstart)
{
    SatKernelArgs a;
    a.orders = ctx->d_orders.get();
    a.cell_off = ctx->d_cell_off.get();
    a.tab_tri = ctx->d_tab.get();
    a.dist_tri = ctx->d_dist.get();
    a.ordinal = ctx->d_ordinal.get();
    a.lorder = lorder ? 1 : 0;
    a.lsoln = lsoln ? 1 : 0;
    a.maxstart = maxstart;
    a.ptab = ctx->d_ptab.get();
    a.prow = ctx->d_prow.get();
    a.bmap_slabs = nullptr;
    a.bmap_slab_words = 0;
    return a;
}

// prepare_sa (sat_launch.hpp) for queries of class c of the current batch, with the arguments every launch shares
int prepare_launch(sat_ctx *ctx, int mode, int lorder, int lsoln, int maxstart, int plan_starts, int c, int n2max, long long work,
               bool pack, SaLaunch &out)
{
    out.args = base_args(ctx, lorder, lsoln, maxstart);
    return prepare_sa(ctx->sa, mode, lorder, lsoln, plan_starts, c, ctx->class_n1max[c], ctx->class_wpl[c], n2max, work, pack, out);
}

}  // namespace

// sat_ctx.hpp
int check_ready(const sat_ctx *ctx, bool need_db, int maxstart)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (need_db && ctx->n_entries <= 0) return sat_fail(SAT_ESTATE, "no database uploaded");
    if (ctx->queries.empty()) return sat_fail(SAT_ESTATE, "no query set");
    if (maxstart < 1) return sat_fail(SAT_EINVAL, "maxstart must be >= 1 (got %d)", maxstart);
    return SAT_OK;
}

// sat_ctx.hpp.  mx: one pass of the match mode (sat_search_matches) instead of a plain search; lsoln is 0 then.  Its record pass
// keeps one record slab per entry slot (scores and db sets of every restart) in the best-map scratch, its replay
// pass a best-map slab per slot there and runs max_matches restarts per entry (workgroups sized for that).
int launch_search(sat_ctx *ctx, int lorder, int lsoln, int maxstart, hipStream_t stream, const ListView *piece, const SatMatchArgs *mx)
{
    int rc = check_ready(ctx, true, maxstart);
    if (rc != SAT_OK) return rc;
    const ListView whole = { ctx->d_lists.get(), ctx->bucket_begin, ctx->bucket_n2max, ctx->n_entries };
    const ListView &view = piece ? *piece : whole;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = refresh_descriptors(ctx, lsoln != 0, stream)) != SAT_OK) return rc;
#ifdef SAT_DIAG
    unsigned long long *diag = nullptr;
    HIP_TRY(satdiag::begin(stream, diag));
#endif

    const bool replay = mx && mx->replay;
    struct Planned { SaLaunch l; int count, nqc, n2max, max_entries; size_t slab_words; };
    std::vector<Planned> plan;
    for (int c = 0; c < 4; c++) {
        const int nqc = ctx->class_begin[c + 1] - ctx->class_begin[c];
        if (nqc == 0) continue;
        // A small problem cannot fill the GPU: its run time is the latency of one workgroup per
        // launch, so all order buckets go into ONE launch sized for the largest entry instead of
        // one launch per bucket queued behind each other.
        const bool one_launch = (long long)view.n * nqc <= 4096;
        int overall_n2max = 0;
        for (int b = 0; b < kNumBuckets; b++)
            if (view.n2max[b] > overall_n2max) overall_n2max = view.n2max[b];
        for (int b = 0; b < kNumBuckets; b++) {
            Planned pl;
            pl.count = view.begin[b + 1] - view.begin[b];
            pl.n2max = view.n2max[b];
            if (one_launch) {
                if (b > 0) break;
                pl.count = view.n;
                pl.n2max = overall_n2max;
            }
            if (pl.count == 0) continue;
            pl.nqc = nqc;
            rc = prepare_launch(ctx, mx ? kMatch : kPlain, lorder, lsoln, maxstart, replay ? mx->max_matches : maxstart, c, pl.n2max,
                            (long long)pl.count * nqc, true, pl.l);
            if (rc != SAT_OK) return rc;
            pl.l.args.queries = ctx->d_qdesc.get() + ctx->class_begin[c];
            pl.l.args.entry_list = view.d_list + (one_launch ? view.begin[0] : view.begin[b]);
#ifdef SAT_DIAG
            pl.l.args.diag = diag;
#endif
            pl.slab_words = (lsoln || replay) ? (size_t)((ctx->class_n1max[c] + 3) / 4) * pl.l.w.chains
                          : (mx ? (size_t)(1 + pl.l.k.m2w) * (size_t)maxstart : 0);
            plan.push_back(pl);
        }
    }

    // The launches of one search (order buckets x query classes) are independent.  Queued on ONE stream
    // each would wait for the last workgroups of the one before it (a tail of half-empty CUs per
    // launch); forked over side streams they run concurrently and the next bucket's workgroups fill
    // the tail.  Largest entries first: their workgroups run longest.  One launch needs no fork.
    std::stable_sort(plan.begin(), plan.end(), [](const Planned &x, const Planned &y) { return x.n2max > y.n2max; });
    const bool fork = plan.size() > 1 && ctx->tune.streams != 0 && ctx->side_stream[0] != nullptr;
    const int nlanes = fork ? (int)(plan.size() < (size_t)kNumBuckets ? plan.size() : (size_t)kNumBuckets) : 1;
    if (fork) HIP_TRY(hipEventRecord(ctx->ev_fork, stream));
    // LSOLN: every workgroup of a launch owns a slab of best maps in global memory; launches are cut so
    // that the slabs of all concurrent launches stay under 1 GiB together (a lane of launches reuses
    // its region launch after launch).  grid.y is limited to 65535: very long query lists are split too.
    const size_t lane_budget_words = ((size_t)1 << 30) / 4 / (size_t)nlanes;
    const bool slabs = lsoln || mx;
    if (slabs) {
        size_t need_total = 0;
        for (size_t i = 0; i < plan.size(); i++) {
            Planned &pl = plan[i];
            size_t fit = lane_budget_words / pl.slab_words;           // workgroups per launch
            if (fit < 1) fit = 1;
            const int qn_cap = pl.nqc < 65535 ? pl.nqc : 65535;
            pl.max_entries = (int)(fit / (size_t)qn_cap);
            if (pl.max_entries < 1) pl.max_entries = 1;
            if (pl.max_entries > pl.count) pl.max_entries = pl.count;
            // (the spare slots of a launch's last workgroup have slabs too)
            const size_t need = pl.slab_words * (size_t)(pl.max_entries + pl.l.epw - 1) * (size_t)qn_cap;
            if (need > need_total) need_total = need;
        }
        need_total *= (size_t)nlanes;                                  // one region per lane of launches
        if ((rc = ctx->d_bmap_slabs.grow_after(stream, need_total)) != SAT_OK) return rc;
    }
    const size_t lane_region_words = slabs ? ctx->d_bmap_slabs.capacity() / (size_t)nlanes : 0;
    for (size_t i = 0; i < plan.size(); i++) {
        const Planned &pl = plan[i];
        const int lane = fork ? (int)(i % (size_t)nlanes) : 0;
        hipStream_t s = fork ? ctx->side_stream[lane] : stream;
        if (fork && i < (size_t)nlanes) HIP_TRY(hipStreamWaitEvent(s, ctx->ev_fork, 0));
        const int max_entries = slabs ? pl.max_entries : pl.count, epw = pl.l.epw;
        for (int q0 = 0; q0 < pl.nqc; q0 += 65535) {
            const int qn = pl.nqc - q0 < 65535 ? pl.nqc - q0 : 65535;
            for (int e0 = 0; e0 < pl.count; e0 += max_entries) {
                const int en = pl.count - e0 < max_entries ? pl.count - e0 : max_entries;
                SatKernelArgs part = pl.l.args;
                part.queries += q0;
                part.entry_list += e0;
                part.n_list = en;
                // the lane's scratch region: best maps (LSOLN, replay pass) or the record pass's records
                SatMatchArgs mpart = mx ? *mx : SatMatchArgs{};
                if (lsoln || replay) {
                    part.bmap_slabs = ctx->d_bmap_slabs.get() + (size_t)lane * lane_region_words;
                    part.bmap_slab_words = (uint32_t)pl.slab_words;
                } else if (mx) {
                    mpart.rec_slabs = ctx->d_bmap_slabs.get() + (size_t)lane * lane_region_words;
                    mpart.rec_slab_words = (uint32_t)pl.slab_words;
                }
                HIP_TRY(launch_sa(pl.l.k, dim3((en + epw - 1) / epw, qn), dim3(pl.l.w.threads * epw), pl.l.lds_launch, s, part, nullptr,
                                  &mpart));
            }
        }
    }
    if (fork)
        for (int lane = 0; lane < nlanes; lane++) {
            HIP_TRY(hipEventRecord(ctx->ev_join[lane], ctx->side_stream[lane]));
            HIP_TRY(hipStreamWaitEvent(stream, ctx->ev_join[lane], 0));
        }
    ctx->searched_nq = ctx->queries.size();
    ctx->searched_lsoln = lsoln != 0;
    ctx->searched_polished = false;
    ctx->fits.clear();                                   // a fit belongs to the scores it was made from
    ctx->last_launch_info.clear();
    for (size_t i = 0; i < plan.size(); i++) {
        const Planned &pl = plan[i];
        if (i) ctx->last_launch_info += "; ";
        ctx->last_launch_info += launch_info(pl.l.k, 0, (pl.count + pl.l.epw - 1) / pl.l.epw, pl.nqc, pl.l.epw, pl.l.w.threads, pl.l.w.lds);
    }
#ifdef SAT_DIAG
    HIP_TRY(satdiag::end(stream));
#endif
    return SAT_OK;
}

// ---------------------------------------------------------------- pair mode (sat_search_pairs)

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
    const int r = (int)(0xFFFFFFFFu - (uint32_t)(keys[items[i].pair] & 0xFFFFFFFFu));
    items[i].r0 = r;
    items[i].r1 = r + 1;
}

__global__ void __launch_bounds__(256) pair_scores(const unsigned long long *keys, int n, int32_t *scores)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) scores[i] = (int32_t)(uint32_t)(keys[i] >> 32) - 0x40000000;
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
            const unsigned long long rk = (((unsigned long long)(uint32_t)(s + 0x40000000)) << 32) | (0xFFFFFFFFu - (uint32_t)r);
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
        const uint32_t r = 0xFFFFFFFFu - (uint32_t)(cur & 0xFFFFFFFFu);
        if (t == 0) {
            scores[(size_t)p * M + m] = (int32_t)(uint32_t)(cur >> 32) - 0x40000000;
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

// The two passes of the pair-match mode that run the SA kernel (launch_pair_pass): the match arguments and the
// restarts of a pair (the row length of its record slab).
struct PairMatchPass { SatMatchArgs mx; int maxstart; };

// The item groups of a pair list or of one chunk of it (build_pair_items): score items [goff[g], goff[g + 1]) and, with
// maps, map items [moff[g], moff[g + 1]) of the item table hold queries of class gcls[g] and entries of up to gn2[g] SSEs.
struct PairGroups { std::vector<size_t> goff, moff; std::vector<int> gcls, gn2; };

// One pass of the pair mode over the item groups of `grp` in d_items: its score items (map_pass = false) or its map
// items.  Score pass: the option-specialised LSOLN-off kernels, restarts per item at most `starts`.  Map pass: one restart per
// item, the general kernel with LSOLN, cut into launches whose best-map slabs stay under 256 MiB (one stream: a launch
// reuses the region).
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
        HIP_TRY(satdiag::begin(stream, a.diag));
#endif
        int per_launch = count;
        if (map_pass) {
            const size_t slab_words = (size_t)((ctx->class_n1max[grp.gcls[g]] + 3) / 4) * (size_t)l.w.chains;
            const size_t budget = ((size_t)1 << 28) / 4;
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
        HIP_TRY(satdiag::end(stream));
#endif
    }
    return SAT_OK;
}

// a pair list as sat_search_pairs takes it: indices into the current batch and the resident shard
int check_pairs(const sat_ctx *ctx, const int32_t *query, const int32_t *entry, int npairs)
{
    if (npairs < 0 || (npairs > 0 && (!query || !entry))) return sat_fail(SAT_EINVAL, "bad pair list");
    const int nq = (int)ctx->queries.size();
    for (int p = 0; p < npairs; p++) {
        if (query[p] < 0 || query[p] >= nq) return sat_fail(SAT_EINVAL, "pair %d: query %d out of range", p, query[p]);
        if (entry[p] < 0 || entry[p] >= ctx->n_entries) return sat_fail(SAT_EINVAL, "pair %d: entry %d out of range", p, entry[p]);
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

// the items build_pair_items makes of a whole pair list (the callers reserve their table once)
size_t pair_item_count(int npairs, int maxstart, int split, bool maps)
{
    return (size_t)npairs * (size_t)((maxstart + split - 1) / split) + (maps ? (size_t)npairs : 0);
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

// One map of the device's outputs (int8, SAT_MAXDIM bytes) as the caller's int32 row: the images of the query's n1
// SSEs, -1 behind them, all -1 for an unused match slot
void expand_map(const int8_t *in, int n1, bool used, int32_t *out)
{
    for (int i = 0; i < SAT_MAXDIM; i++) out[i] = (used && i < n1) ? in[i] : -1;
}

// The head of both match searches: a context, max_matches in range, then the SatMatchArgs fields they share (the record
// pass; maps of SAT_MAXDIM bytes).  The caller adds the row length and the outputs once its buffers stand.  (The
// descriptor table is taken before the caller's refresh_descriptors: only sat_set_queries reallocates it.)
int match_args(const sat_ctx *ctx, int max_matches, SatMatchArgs &mx)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (max_matches < 1 || max_matches > SAT_MAX_MATCHES)
        return sat_fail(SAT_EINVAL, "max_matches must be 1..%d (got %d)", SAT_MAX_MATCHES, max_matches);
    mx = SatMatchArgs{};
    mx.desc_base = ctx->d_qdesc.get();
    mx.max_matches = max_matches;
    mx.map_pitch = SAT_MAXDIM;
    return SAT_OK;
}

}  // namespace

// sat_ctx.hpp: queue a pair search (both passes) on the context's stream
int sat_pairs_launch(sat_ctx *ctx, int lorder, int maxstart, bool maps, const int32_t *query, const int32_t *entry, int npairs)
{
    int rc = check_ready(ctx, true, maxstart);
    if (rc != SAT_OK) return rc;
    if ((rc = check_pairs(ctx, query, entry, npairs)) != SAT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = refresh_descriptors(ctx, false, ctx->stream)) != SAT_OK) return rc;
    ctx->last_launch_info.clear();
    if (npairs == 0) return SAT_OK;

    const int split = pair_split(ctx, maxstart, npairs);
    std::vector<SatPairItem> &items = ctx->h_pitems;
    HIP_TRY(hipStreamSynchronize(ctx->stream));      // the previous pair search's upload has read the table
    items.clear();
    items.reserve(pair_item_count(npairs, maxstart, split, maps));
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

int sat_launch_plain(sat_ctx *ctx, int lorder, int maxstart)
{
    return launch_search(ctx, lorder, 0, maxstart, ctx->stream);
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
    if (ssemaps) {
        std::vector<int8_t> mp((size_t)npairs * SAT_MAXDIM);
        HIP_TRY(hipMemcpy(mp.data(), ctx->d_pmaps.get(), mp.size(), hipMemcpyDeviceToHost));
        ctx->d2h_bytes += mp.size();
        for (size_t p = 0; p < (size_t)npairs; p++)
            expand_map(mp.data() + p * SAT_MAXDIM, ctx->queries[(size_t)query[p]].n1, true, ssemaps + p * SAT_MAXDIM);
    }
    return SAT_OK;
}

// sat_ctx.hpp: queue a pair-match search on the context's stream.  The pair list is cut into launches of at most
// `chunk` pairs whose record slabs stay under the 1 GiB scratch budget; each runs its record pass, the selection and
// (maps) its map pass before the next one reuses the scratch.
// polish (sat_polish.hip): the selection without the set test, and behind the map pass the polish of the picked maps.
int sat_pair_matches_launch(sat_ctx *ctx, int lorder, int maxstart, int max_matches, bool maps, const int32_t *query,
                            const int32_t *entry, int npairs, bool polish, bool packed)
{
    PairMatchPass pm{};
    int rc = match_args(ctx, max_matches, pm.mx);
    if (rc != SAT_OK) return rc;
    if ((rc = check_ready(ctx, true, maxstart)) != SAT_OK) return rc;
    if ((rc = check_pairs(ctx, query, entry, npairs)) != SAT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = refresh_descriptors(ctx, false, ctx->stream)) != SAT_OK) return rc;
    ctx->last_launch_info.clear();
    if (npairs == 0) return SAT_OK;
    const size_t M = (size_t)max_matches;
    const int split = pair_split(ctx, maxstart, npairs);

    // a pair's slab: the scores and the set words of its restarts, as wide as the widest set of the list
    int n2_all = 0;
    for (int p = 0; p < npairs; p++) n2_all = std::max(n2_all, ctx->h_orders[(size_t)entry[p]]);
    const size_t slab_words = (size_t)(1 + satk::set_words(n2_all)) * (size_t)maxstart;
    const size_t budget_words = ((size_t)1 << 30) / 4;
    const int chunk = (int)std::min<size_t>((size_t)npairs, std::max<size_t>(1, budget_words / slab_words));

    // the items of every launch of `chunk` pairs, one behind the other in the table
    struct Chunk { int p0, n; PairGroups grp; };
    std::vector<Chunk> chunks;
    std::vector<SatPairItem> &items = ctx->h_pitems;
    std::vector<uint8_t> &setw = ctx->h_psetw;
    HIP_TRY(hipStreamSynchronize(ctx->stream));      // the previous pair search's uploads have read the tables
    items.clear();
    items.reserve(pair_item_count(npairs, maxstart, split, maps));
    setw.assign((size_t)npairs, 0);
    for (int p0 = 0; p0 < npairs; p0 += chunk) {
        const int n = std::min(chunk, npairs - p0);
        chunks.push_back({ p0, n, build_pair_items(ctx, query, entry, p0, n, maxstart, split, maps, items, setw.data()) });
    }
    // outputs: counts [pairs], scores [pairs][M], restarts [pairs][M] in one array (one copy to the host), the maps
    if ((rc = ctx->d_pitems.grow_after(ctx->stream, items.size())) != SAT_OK ||
        (rc = ctx->d_pkeys.grow_after(ctx->stream, (size_t)npairs)) != SAT_OK ||
        (rc = ctx->d_psetw.grow_after(ctx->stream, (size_t)npairs)) != SAT_OK ||
        (rc = ctx->d_pmout.grow_after(ctx->stream, (size_t)npairs * (1 + 2 * M))) != SAT_OK ||
        (rc = ctx->d_bmap_slabs.grow_after(ctx->stream, slab_words * (size_t)chunk)) != SAT_OK ||
        (maps && (rc = ctx->d_pmaps.grow_after(ctx->stream, (size_t)npairs * M * SAT_MAXDIM)) != SAT_OK) ||
        (polish && (rc = sat_polish_reserve(ctx, npairs)) != SAT_OK))
        return rc;
    HIP_TRY(hipMemcpyAsync(ctx->d_pitems.get(), items.data(), items.size() * sizeof(SatPairItem), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->d_psetw.get(), setw.data(), setw.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->d_pkeys.get(), 0, (size_t)npairs * sizeof(unsigned long long), ctx->stream));
    if (maps) HIP_TRY(hipMemsetAsync(ctx->d_pmaps.get(), 0xFF, (size_t)npairs * M * SAT_MAXDIM, ctx->stream));

    pm.maxstart = maxstart;
    pm.mx.n_entries = 0;                                 // (rows are pairs)
    pm.mx.rec_slab_words = (uint32_t)slab_words;
    pm.mx.counts = ctx->d_pmout.get();
    pm.mx.scores = pm.mx.counts + npairs;
    pm.mx.restarts = pm.mx.scores + (size_t)npairs * M;
    pm.mx.maps = ctx->d_pmaps.get();
    std::string rec_info, map_info;
    for (const Chunk &ch : chunks) {
        // (the map pass of the launch before may have replaced the scratch with a larger one)
        pm.mx.rec_slabs = ctx->d_bmap_slabs.get();
        if ((rc = launch_pair_pass(ctx, lorder, false, split, ctx->d_pitems.get(), ch.grp, rec_info, &pm)) != SAT_OK)
            return rc;
        if (polish) {
            if ((rc = sat_polish_select(ctx, ch.p0, ch.n, maxstart, max_matches, (uint32_t)slab_words, pm.mx.counts, pm.mx.scores,
                                        pm.mx.restarts)) != SAT_OK)
                return rc;
        } else {
            hipLaunchKernelGGL(pair_match_select, dim3((unsigned)ch.n), dim3(256), 0, ctx->stream, ch.p0, maxstart, max_matches,
                               (const uint32_t *)ctx->d_bmap_slabs.get(), (uint32_t)slab_words, (const uint8_t *)ctx->d_psetw.get(),
                               (const unsigned long long *)ctx->d_pkeys.get(), pm.mx.counts, pm.mx.scores, pm.mx.restarts);
            HIP_TRY(hipGetLastError());
        }
        if (maps && (rc = launch_pair_pass(ctx, lorder, true, 1, ctx->d_pitems.get(), ch.grp, map_info, &pm)) != SAT_OK)
            return rc;
        // the polish walks the launch's map items: one per pair, with its descriptor and entry.  An item group's entries
        // share an order bucket, and with it the width the polish runs at; neighbouring groups of one width go in one
        // launch (every launch ends on its slowest maps: fewer launches, fewer tails)
        if (polish)
            for (size_t g = 0; g < ch.grp.gcls.size();) {
                const int width = sat_polish_width(ctx, ch.n, max_matches, ch.grp.gn2[g], packed);
                int n2max = ch.grp.gn2[g];
                size_t h = g + 1;
                for (; h < ch.grp.gcls.size() && sat_polish_width(ctx, ch.n, max_matches, ch.grp.gn2[h], packed) == width; h++)
                    n2max = std::max(n2max, ch.grp.gn2[h]);
                const int n = (int)(ch.grp.moff[h] - ch.grp.moff[g]);
                if (n > 0 && (rc = sat_polish_run(ctx, lorder, ctx->d_pitems.get() + ch.grp.moff[g], n, max_matches, n2max, npairs,
                                                  pm.mx.counts, pm.mx.scores, pm.mx.restarts, pm.mx.maps, width)) != SAT_OK)
                    return rc;
                g = h;
            }
    }
    char head[128];
    snprintf(head, sizeof head, "record pass (%d restarts, %d per item, %zu launches of up to %d pairs): ", maxstart, split,
             chunks.size(), chunk);
    ctx->last_launch_info = head + rec_info + " | select";
    if (maps) ctx->last_launch_info += " | map pass: " + map_info;
    if (polish) ctx->last_launch_info += " | polish";
    return SAT_OK;
}

// sat_ctx.hpp: wait for the pair-match search and copy its rows: 4 * npairs * (1 + 2 M) bytes, + 111 * npairs * M
// with maps
int sat_pair_matches_collect(sat_ctx *ctx, int max_matches, int npairs, int32_t *counts, int32_t *scores, int32_t *restarts,
                             int32_t *ssemaps, const int32_t *query)
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
    memcpy(counts, out.data(), P * sizeof(int32_t));
    memcpy(scores, out.data() + P, P * M * sizeof(int32_t));
    memcpy(restarts, out.data() + P + P * M, P * M * sizeof(int32_t));
    if (ssemaps) {
        std::vector<int8_t> mp(P * M * SAT_MAXDIM);
        HIP_TRY(hipMemcpy(mp.data(), ctx->d_pmaps.get(), mp.size(), hipMemcpyDeviceToHost));
        ctx->d2h_bytes += mp.size();
        for (size_t p = 0; p < P; p++)
            for (size_t m = 0; m < M; m++)
                expand_map(mp.data() + (p * M + m) * SAT_MAXDIM, ctx->queries[(size_t)query[p]].n1, (int32_t)m < counts[p],
                           ssemaps + (p * M + m) * SAT_MAXDIM);
    }
    return SAT_OK;
}

// sat_ctx.hpp: the polished form of a plain whole-shard search (the context's polish_all maps per row)
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
    // a launch: as many rows as sat_pair_matches_launch takes in one launch of its own, at most kPolishAllPairs
    int n2_all = 0;
    for (size_t e = 0; e < N; e++) n2_all = std::max(n2_all, ctx->h_orders[e]);
    const size_t slab_words = (size_t)(1 + satk::set_words(n2_all)) * (size_t)maxstart;
    const size_t chunk = std::min<size_t>(std::min<size_t>(rows, (size_t)kPolishAllPairs), std::max<size_t>(1, (((size_t)1 << 30) / 4) / slab_words));
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
        // (the call waits for the launch before it: its tables and outputs are this launch's alone)
        if ((rc = sat_pair_matches_launch(ctx, lorder, maxstart, tops, true, query.data(), entry.data(), (int)n, true, true)) != SAT_OK)
            return rc;
        const size_t n_score = ctx->h_pitems.size() - n;          // the map items, one per pair, stand behind the score items
        if ((rc = sat_polish_scatter(ctx, ctx->d_pitems.get() + n_score, (int)n, (int)n, lsoln != 0)) != SAT_OK) return rc;
    }
    char head[96];
    snprintf(head, sizeof head, "polish all (%d tops, %zu launches of up to %zu pairs): ", tops, launches, chunk);
    ctx->last_launch_info = head + ctx->last_launch_info;
    ctx->searched_nq = nq;
    ctx->searched_lsoln = lsoln != 0;
    ctx->searched_polished = true;
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

namespace {

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

}  // namespace

extern "C" {

const char *sat_last_error(void) { return g_err; }

int sat_abi_version(void) { return SAT_ABI_VERSION; }

int sat_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

sat_ctx *sat_ctx_create(int device, uint64_t seed)
{
    int n = sat_device_count();
    if (n <= 0) {
        sat_fail(SAT_ENODEVICE, "no HIP device available (this library has no CPU path)");
        return nullptr;
    }
    if (device < 0 || device >= n) {
        sat_fail(SAT_ENODEVICE, "device %d out of range (0..%d)", device, n - 1);
        return nullptr;
    }
    sat_ctx *ctx = new (std::nothrow) sat_ctx();
    if (!ctx) {
        sat_fail(SAT_ENOMEM, "out of host memory");
        return nullptr;
    }
    ctx->device = device;
    ctx->seed = seed;
    auto init = [&]() -> int {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
        ctx->stream = ctx->own_stream;
        HIP_TRY(hipEventCreate(&ctx->ev0));
        HIP_TRY(hipEventCreate(&ctx->ev1));
        // launch-heuristic overrides: read once here, never on the search path
        auto env_int = [](const char *name, int dflt) { const char *v = getenv(name); return v && *v ? atoi(v) : dflt; };
        ctx->sa.compact = env_int("SAT_EXP_COMPACT", -1);
        ctx->sa.qlds = env_int("SAT_EXP_QLDS", -1);
        ctx->sa.lpc = env_int("SAT_EXP_LPC", -1);
        ctx->sa.general = env_int("SAT_EXP_GENERAL", 0);
        ctx->tune.streams = env_int("SAT_EXP_STREAMS", -1);
        ctx->tune.upload_threads = env_int("SAT_EXP_UPLOAD_THREADS", 0);
        ctx->tune.upload_timing = env_int("SAT_EXP_UPLOAD_TIMING", 0);
        ctx->tune.upload_pieces = env_int("SAT_EXP_UPLOAD_PIECES", 0);
        ctx->sa.epw = env_int("SAT_EXP_EPW", 0);
        ctx->sa.lpc_waves = env_int("SAT_EXP_LPC_WAVES", 0);
        ctx->sa.chains = env_int("SAT_EXP_CHAINS", 0);
        ctx->tune.refine_split = env_int("SAT_EXP_REFINE_SPLIT", 0);
        ctx->tune.polish_group = env_int("SAT_EXP_POLISH_GROUP", 0);
        const int pad = env_int("SAT_EXP_LDS_PAD", 0);
        ctx->sa.lds_pad = pad > 0 ? (size_t)pad : 0;
        if (ctx->tune.streams != 0) {
            for (int b = 0; b < kNumBuckets; b++) {
                HIP_TRY(hipStreamCreateWithFlags(&ctx->side_stream[b], hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&ctx->ev_join[b], hipEventDisableTiming));
            }
            HIP_TRY(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
        }
        const int rc_tab = build_metropolis_table(ctx);
        if (rc_tab != SAT_OK) return rc_tab;
        // load the code objects of the upload, the SA kernels and this file now (an empty launch of a small kernel, or
        // a question about one): the ~5 ms the first launch of a process pays for them belong to context creation, not
        // to the first upload or search
        int rc_load;
        if ((rc_load = sat_db_load_code(ctx)) != SAT_OK || (rc_load = sa_load_code()) != SAT_OK) return rc_load;
        hipLaunchKernelGGL(pair_scores, dim3(1), dim3(256), 0, ctx->stream, nullptr, 0, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return build_gumbel_tables(ctx);
    };
    if (init() != SAT_OK) {
        sat_ctx_destroy(ctx);
        return nullptr;
    }
    return ctx;
}

void sat_ctx_destroy(sat_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    // the device buffers go with the context, freed with its device current; then its events and streams
    std::vector<hipEvent_t> events = { ctx->ev0, ctx->ev1, ctx->ev_fork };
    events.insert(events.end(), ctx->ev_join, ctx->ev_join + kNumBuckets);
    std::vector<hipStream_t> streams(ctx->side_stream, ctx->side_stream + kNumBuckets);
    streams.push_back(ctx->own_stream);
    delete ctx;
    for (hipEvent_t e : events)
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t st : streams)
        if (st) (void)hipStreamDestroy(st);
}

int sat_query_count(const sat_ctx *ctx) { return ctx ? (int)ctx->queries.size() : 0; }

int sat_use_stream(sat_ctx *ctx, void *hip_stream)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->stream = static_cast<hipStream_t>(hip_stream);
    return SAT_OK;
}

int sat_use_own_stream(sat_ctx *ctx)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->stream = ctx->own_stream;
    return SAT_OK;
}

int sat_search_async(sat_ctx *ctx, int lorder, int lsoln, int maxstart)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (ctx->polish_all) return sat_polish_all_launch(ctx, lorder, lsoln, maxstart);
    return launch_search(ctx, lorder, lsoln, maxstart, ctx->stream);
}

int sat_polish_all_set(sat_ctx *ctx, int tops)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (tops < 0 || tops > SAT_MAX_MATCHES) return sat_fail(SAT_EINVAL, "tops must be 0..%d (got %d)", SAT_MAX_MATCHES, tops);
    ctx->polish_all = tops;
    return SAT_OK;
}

int sat_polish_all_get(const sat_ctx *ctx) { return ctx ? ctx->polish_all : 0; }

int sat_results_base(sat_ctx *ctx, int32_t *base_scores)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (!base_scores) return sat_fail(SAT_EINVAL, "base_scores buffer is null");
    if (ctx->n_entries <= 0) return sat_fail(SAT_ESTATE, "no database uploaded");
    if (ctx->queries.empty() || ctx->searched_nq != ctx->queries.size() || !ctx->searched_polished || !ctx->d_base.get())
        return sat_fail(SAT_ESTATE, "the last search was not a polished one (sat_polish_all_set)");
    const int rc = sat_polish_all_check(ctx);
    if (rc != SAT_OK) return rc;
    const size_t n = ctx->queries.size() * (size_t)ctx->n_entries;
    HIP_TRY(hipMemcpy(base_scores, ctx->d_base.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost));
    ctx->d2h_bytes += n * sizeof(int32_t);
    return SAT_OK;
}

void *sat_device_scores(sat_ctx *ctx) { return ctx ? ctx->d_scores.get() : nullptr; }
void *sat_device_ssemaps(sat_ctx *ctx) { return ctx ? ctx->d_ssemaps.get() : nullptr; }
int sat_query_order(const sat_ctx *ctx) { return (ctx && !ctx->queries.empty()) ? ctx->queries[0].n1 : 0; }

unsigned long long sat_stat_d2h_bytes(const sat_ctx *ctx) { return ctx ? ctx->d2h_bytes : 0ull; }

const char *sat_last_launch_info(const sat_ctx *ctx) { return ctx ? ctx->last_launch_info.c_str() : ""; }

int sat_sync(sat_ctx *ctx)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return sat_polish_all_check(ctx);
}

int sat_results(sat_ctx *ctx, int lsoln, int32_t *scores, int32_t *ssemaps)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (!scores) return sat_fail(SAT_EINVAL, "scores buffer is null");
    if (lsoln && !ssemaps) return sat_fail(SAT_EINVAL, "lsoln set but ssemaps buffer is null");
    if (ctx->n_entries <= 0) return sat_fail(SAT_ESTATE, "no database uploaded");
    if (ctx->queries.empty() || !ctx->d_scores.get() || ctx->searched_nq != ctx->queries.size())
        return sat_fail(SAT_ESTATE, "no search has run since the last database upload / query change");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t nq = ctx->queries.size(), N = (size_t)ctx->n_entries;
    HIP_TRY(hipMemcpy(scores, ctx->d_scores.get(), nq * N * sizeof(int32_t), hipMemcpyDeviceToHost));
    ctx->d2h_bytes += nq * N * sizeof(int32_t);
    if (lsoln) {
        if (!ctx->d_ssemaps.get() || !ctx->searched_lsoln) return sat_fail(SAT_ESTATE, "the last search ran without lsoln");
        std::vector<int8_t> packed;
        for (size_t qi = 0; qi < nq; qi++) {
            const auto &q = ctx->queries[qi];
            packed.resize(N * q.n1);
            HIP_TRY(hipMemcpy(packed.data(), ctx->d_ssemaps.get() + q.ssemap_off, packed.size(), hipMemcpyDeviceToHost));
            ctx->d2h_bytes += packed.size();
            int32_t *out = ssemaps + qi * N * SAT_MAXDIM;
            for (size_t e = 0; e < N; e++)
                for (int i = 0; i < q.n1; i++)
                    out[e * SAT_MAXDIM + i] = packed[e * q.n1 + i];
        }
    }
    return SAT_OK;
}

int sat_search(sat_ctx *ctx, int lorder, int lsoln, int maxstart,
               int32_t *scores, int32_t *ssemaps, double *kernel_ms)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (!scores) return sat_fail(SAT_EINVAL, "scores buffer is null");
    if (lsoln && !ssemaps) return sat_fail(SAT_EINVAL, "lsoln set but ssemaps buffer is null");
    int rc = timed(ctx, kernel_ms, [&] {
        return ctx->polish_all ? sat_polish_all_launch(ctx, lorder, lsoln, maxstart) : launch_search(ctx, lorder, lsoln, maxstart, ctx->stream);
    });
    if (rc != SAT_OK) return rc;
    if (ctx->polish_all && (rc = sat_polish_all_check(ctx)) != SAT_OK) return rc;
    return sat_results(ctx, lsoln, scores, ssemaps);
}

}  // extern "C"

int sat_matches_launch(sat_ctx *ctx, int lorder, int maxstart, int max_matches, bool maps)
{
    SatMatchArgs mx;
    int rc = match_args(ctx, max_matches, mx);
    if (rc != SAT_OK) return rc;
    if ((rc = check_ready(ctx, true, maxstart)) != SAT_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    // counts: one per row, scores / restarts: M per row, maps: M x SAT_MAXDIM bytes per row
    const size_t rows = ctx->queries.size() * (size_t)ctx->n_entries, slots = rows * (size_t)max_matches;
    if ((rc = ctx->d_mcounts.grow_after(ctx->stream, rows)) != SAT_OK || (rc = ctx->d_mscores.grow_after(ctx->stream, slots)) != SAT_OK ||
        (rc = ctx->d_mrestarts.grow_after(ctx->stream, slots)) != SAT_OK ||
        (rc = ctx->d_mmaps.grow_after(ctx->stream, maps ? slots * SAT_MAXDIM : 0)) != SAT_OK)
        return rc;
    mx.n_entries = ctx->n_entries;
    mx.counts = ctx->d_mcounts.get();
    mx.scores = ctx->d_mscores.get();
    mx.restarts = ctx->d_mrestarts.get();
    mx.maps = ctx->d_mmaps.get();
    rc = launch_search(ctx, lorder, 0, maxstart, ctx->stream, nullptr, &mx);
    if (rc != SAT_OK) return rc;
    // sat_last_launch_info names both passes
    const std::string record_info = ctx->last_launch_info;
    ctx->last_launch_info = "record pass: " + record_info;
    if (!maps) return SAT_OK;
    // the replay pass reads the record pass's counts and restarts: same stream, and the order buckets of one pass
    // are joined back onto it before the next pass forks
    mx.replay = 1;
    rc = launch_search(ctx, lorder, 0, maxstart, ctx->stream, nullptr, &mx);
    if (rc == SAT_OK) ctx->last_launch_info = "record pass: " + record_info + " | replay pass: " + ctx->last_launch_info;
    return rc;
}

int sat_matches_collect(sat_ctx *ctx, int max_matches, int32_t *counts, int32_t *scores, int32_t *restarts,
                        int32_t *ssemaps, size_t total, size_t offset)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t nq = ctx->queries.size(), N = (size_t)ctx->n_entries, M = (size_t)max_matches;
    std::vector<int32_t> c(nq * N), sc(nq * N * M), rs(nq * N * M);
    std::vector<int8_t> mp(ssemaps ? nq * N * M * SAT_MAXDIM : 0);
    HIP_TRY(hipMemcpy(c.data(), ctx->d_mcounts.get(), c.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sc.data(), ctx->d_mscores.get(), sc.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rs.data(), ctx->d_mrestarts.get(), rs.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (ssemaps) HIP_TRY(hipMemcpy(mp.data(), ctx->d_mmaps.get(), mp.size(), hipMemcpyDeviceToHost));
    ctx->d2h_bytes += (c.size() + sc.size() + rs.size()) * sizeof(int32_t) + mp.size();
    // device rows are by descriptor index: the queries grouped by size class (refresh_descriptors)
    for (size_t qi = 0; qi < nq; qi++) {
        const size_t d = (size_t)ctx->queries[qi].desc;
        const int n1 = ctx->queries[qi].n1;
        for (size_t e = 0; e < N; e++) {
            const size_t src = d * N + e, dst = qi * total + offset + e;
            counts[dst] = c[src];
            for (size_t m = 0; m < M; m++) {
                scores[dst * M + m] = sc[src * M + m];
                restarts[dst * M + m] = rs[src * M + m];
                if (ssemaps) expand_map(mp.data() + (src * M + m) * SAT_MAXDIM, n1, (int)m < c[src], ssemaps + (dst * M + m) * SAT_MAXDIM);
            }
        }
    }
    return SAT_OK;
}

extern "C" {

int sat_search_matches(sat_ctx *ctx, int lorder, int maxstart, int max_matches, int32_t *counts, int32_t *scores,
                       int32_t *restarts, int32_t *ssemaps, double *kernel_ms)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (!counts || !scores || !restarts) return sat_fail(SAT_EINVAL, "counts / scores / restarts buffer is null");
    const int rc = timed(ctx, kernel_ms, [&] { return sat_matches_launch(ctx, lorder, maxstart, max_matches, ssemaps != nullptr); });
    if (rc != SAT_OK) return rc;
    return sat_matches_collect(ctx, max_matches, counts, scores, restarts, ssemaps, (size_t)ctx->n_entries, 0);
}

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

int sat_search_timed(sat_ctx *ctx, int lorder, int lsoln, int maxstart, int repeats,
                     double *total_ms, double *kernel_ms)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (repeats < 1) return sat_fail(SAT_EINVAL, "repeats must be >= 1");
    if (ctx->polish_all) return sat_fail(SAT_ESTATE, "sat_search_timed times the plain search: not while sat_polish_all_set is on");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    for (int r = 0; r < repeats; r++) {
        int rc = launch_search(ctx, lorder, lsoln, maxstart, ctx->stream);
        if (rc != SAT_OK) return rc;
    }
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (total_ms) *total_ms = ms;
    if (kernel_ms) *kernel_ms = ms;
    return SAT_OK;
}

}  // extern "C"
