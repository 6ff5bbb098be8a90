// sat_capi.hip - C ABI (include/satabsearch.h) over the gfx950 SA kernel.
//
// Host side of the drop-in boundary: device memory, the packed database store, the
// query buffer, the Metropolis table, size-class dispatch and launches.  Replaces
// the device glue of nvcc_src_current/cudaSaTabsearch.cu (init_rng :258-264,
// copyQueryToConstantMemory :486-558, alloc/upload :896-984, launch/sync/download
// :1036-1087 and :1128-1270).  No CPU search path exists in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <set>
#include <string>
#include <thread>
#include <type_traits>
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

// db entries are launched in classes of similar order so that every launch sizes its
// LDS for the largest member of the class only
const int kBucketMax[kNumBuckets] = { 16, 32, 48, 64, 80, 96, 111 };
constexpr size_t kLdsLimit = 160 * 1024;

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

void free_db(sat_ctx *ctx)
{
    ctx->d_orders.reset();
    ctx->d_cell_off.reset();
    ctx->d_tab.reset();
    ctx->d_dist.reset();
    ctx->d_ordinal.reset();
    ctx->d_lists.reset();
    ctx->d_scores.reset();
    ctx->d_ssemaps.reset();
    ctx->desc_dirty = true;
    ctx->n_entries = 0;
    ctx->min_rows = 0;
    ctx->searched_nq = 0;
    ctx->fits.clear();
    ctx->h_orders.clear();
}

// ---- kernel choice.  The four kernel families are instantiated over the same size classes and db layouts: the
// dispatch below calls f with std::integral_constant arguments, so that one walk of the tree (pick_sa_kernel) names every
// instantiation once.
template <int V> using Int = std::integral_constant<int, V>;

// f(Int<N1P>) for a query size class
template <typename F> auto by_class(int n1p, F f)
{
    switch (n1p) {
    case 16: return f(Int<16>{});
    case 32: return f(Int<32>{});
    case 64: return f(Int<64>{});
    default: return f(Int<112>{});
    }
}

// f(std::bool_constant<b>)
template <typename F> auto by_flag(bool b, F f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// f(Int<V>) for v in First .. Last, Last for anything above
template <int First, int Last, typename F> auto by_value(int v, F f)
{
    if constexpr (First == Last) return f(Int<Last>{});
    else return v == First ? f(Int<First>{}) : by_value<First + 1, Last>(v, f);
}

// f(Int<M2W>, Int<CELLS>): db-side set width and cell layout (satk::cell_layout of the launch's largest entry).
// One-word sets go with the 8-byte cells, two-word sets with either split layout (entries of up to 48 SSEs: full
// matrix, above: triangle), four-word sets with the triangle.
template <typename F> auto by_layout(int m2w, int cells, F f)
{
    if (m2w == 1) return f(Int<1>{}, Int<SAT_CELLS_FULL8>{});
    if (m2w == 2) return cells == SAT_CELLS_FULL5 ? f(Int<2>{}, Int<SAT_CELLS_FULL5>{}) : f(Int<2>{}, Int<SAT_CELLS_TRI5>{});
    return f(Int<4>{}, Int<SAT_CELLS_TRI5>{});
}

// The four kernel families (sat_sa_kernel.hpp): bit 0 = the match arguments, bit 1 = the pair arguments
enum SaMode { kPlain = 0, kMatch = 1, kPair = 2, kPairMatch = 3 };

// A chosen SA kernel: the instantiation's address and the template arguments it was instantiated with (opt = -1, wpl = 0:
// the general instantiation).  What is launched (launch_sa) and what sat_last_launch_info names (launch_info) both come
// from this one record.
struct SaKernel { const void *fn; int mode, n1p, m2w, cells; bool qlds; int opt, wpl; };

// the instantiation of family MODE; only the plain family has WPL, only the plain and the pair family have OPT
template <int MODE, int N1P, int M2W, bool QLDS, int OPT, int WPL, int CELLS> const void *sa_instance()
{
    static_assert(MODE == kPlain || WPL == 0, "words per lane are an argument of the plain kernel only");
    static_assert(MODE == kPlain || MODE == kPair || OPT == -1, "the match families read their options from the arguments");
    if constexpr (MODE == kPlain) return reinterpret_cast<const void *>(sat_sa_kernel<N1P, M2W, QLDS, OPT, WPL, CELLS>);
    else if constexpr (MODE == kPair) return reinterpret_cast<const void *>(sat_sa_pair_kernel<N1P, M2W, QLDS, OPT, CELLS>);
    else if constexpr (MODE == kMatch) return reinterpret_cast<const void *>(sat_sa_match_kernel<N1P, M2W, QLDS, CELLS>);
    else return reinterpret_cast<const void *>(sat_sa_pair_match_kernel<N1P, M2W, QLDS, CELLS>);
}

// The kernel of a launch's family, size class and layout.  opt >= 0 asks for an instantiation with the options as
// compile-time facts (bit 0 LORDER, bit 1 LSOLN, bits 2-3 log2 of the lanes per chain; compaction tables exactly when
// LORDER); these exist for the default placement of the query cells only (LDS for the 16 class, L1/L2 for the others):
//   plain       opt 0-3, and with LORDER also `wpl`, the words per lane of the compacted rounds when every query of the
//               launch has the same, for the values a class can have (satk::compaction_shape), else 0 (see the kernel's
//               OPT and WPL parameters); opt 4-11 (several lanes per chain) for the largest entries only (M2W = 4, words
//               per lane read per query);
//   pair        opt 0 / 1 (LSOLN off, one lane per chain, words per lane read per query);
//   match, pair-match   none.
// Anything else runs the general instantiation.
SaKernel pick_sa_kernel(int mode, int n1p, int m2w, int cells, bool qlds, int opt, int wpl)
{
    SaKernel k = { nullptr, mode, n1p, m2w, cells, qlds, -1, 0 };
    by_value<kPlain, kPairMatch>(mode, [&](auto md) {
        by_class(n1p, [&](auto c) {
            constexpr int MODE = decltype(md)::value, N1P = decltype(c)::value;
            constexpr bool kQ = N1P < 32;
            // the instantiation <q, o, w> for the launch's layout
            auto take = [&](auto q, auto o, auto w) {
                k.opt = decltype(o)::value;
                k.wpl = decltype(w)::value;
                k.fn = by_layout(m2w, cells, [](auto m, auto l) {
                    return sa_instance<MODE, N1P, decltype(m)::value, decltype(q)::value, decltype(o)::value, decltype(w)::value,
                                       decltype(l)::value>();
                });
            };
            const std::bool_constant<kQ> q{};
            if constexpr (MODE == kPlain) {
                if (opt >= 4 && qlds == kQ && m2w == 4)
                    return by_value<4, 11>(opt, [&](auto o) {
                        k.opt = decltype(o)::value;
                        k.fn = sa_instance<kPlain, N1P, 4, kQ, decltype(o)::value, 0, SAT_CELLS_TRI5>();
                    });
                if (opt >= 0 && opt < 4 && qlds == kQ)
                    return by_value<0, 3>(opt, [&](auto o) {
                        if constexpr ((decltype(o)::value & 1) == 0) take(q, o, Int<0>{});     // no compaction: wpl unused
                        else {
                            if (wpl == 4) return take(q, o, Int<4>{});
                            if constexpr (N1P <= 64)
                                if (wpl == 3) return take(q, o, Int<3>{});
                            if constexpr (N1P == 16) {
                                if (wpl == 2) return take(q, o, Int<2>{});
                                if (wpl == 1) return take(q, o, Int<1>{});
                            }
                            take(q, o, Int<0>{});               // queries of different shapes: wpl read per query
                        }
                    });
            }
            if constexpr (MODE == kPair)
                if ((opt == 0 || opt == 1) && qlds == kQ) return by_value<0, 1>(opt, [&](auto o) { take(q, o, Int<0>{}); });
            by_flag(qlds, [&](auto qg) { take(qg, Int<-1>{}, Int<0>{}); });
        });
    });
    return k;
}

// Launch `k`: the kernel's parameters are the SatKernelArgs, then the pair arguments (pair families), then the match
// arguments (match families).  The only place that knows which family takes which.
hipError_t launch_sa(const SaKernel &k, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const SatKernelArgs &a,
                     const SatPairArgs *px, const SatMatchArgs *mx)
{
    void *args[3] = { const_cast<SatKernelArgs *>(&a), nullptr, nullptr };
    int n = 1;
    if (k.mode & kPair) args[n++] = const_cast<SatPairArgs *>(px);
    if (k.mode & kMatch) args[n++] = const_cast<SatMatchArgs *>(mx);
    (void)hipLaunchKernel(k.fn, grid, block, args, lds, stream);
    return hipGetLastError();
}

// An instantiation by name, "kernel<template arguments>" as the source spells it: the one formatter of
// sat_last_launch_info (launch_info) and of the list of instantiations (sat_debug_sa_instances).
std::string sa_kernel_name(const SaKernel &k)
{
    static const char *const kName[4] = { "sat_sa_kernel", "sat_sa_match_kernel", "sat_sa_pair_kernel", "sat_sa_pair_match_kernel" };
    char targs[48] = "", buf[128];
    if (k.mode == kPlain) snprintf(targs, sizeof targs, "%d, %d, ", k.opt, k.wpl);
    if (k.mode == kPair) snprintf(targs, sizeof targs, "%d, ", k.opt);
    snprintf(buf, sizeof buf, "%s<%d, %d, %s, %s%d>", kName[k.mode], k.n1p, k.m2w, k.qlds ? "true" : "false", targs, k.cells);
    return buf;
}

// One launch as sat_last_launch_info names it: "kernel<template arguments> [items N] grid X x Y block E x T lds B"
// (items: the pair families' item count; E entry slots of T threads; B the LDS bytes of one slot).
std::string launch_info(const SaKernel &k, int items, int grid_x, int grid_y, int epw, int threads, size_t lds)
{
    char count[32] = "", buf[128];
    if (k.mode & kPair) snprintf(count, sizeof count, " items %d", items);
    snprintf(buf, sizeof buf, "%s grid %d x %d block %d x %d lds %zu", count, grid_x, grid_y, epw, threads, lds);
    return sa_kernel_name(k) + buf;
}

const int kClassN1P[4] = { 16, 32, 64, 112 };

// (re)build the device query descriptors: pointers into the query blob and into the result
// buffers, grouped by size class
int refresh_descriptors(sat_ctx *ctx, bool lsoln, hipStream_t stream)
{
    const size_t nq = ctx->queries.size();
    const size_t rows = (size_t)(ctx->n_entries > ctx->min_rows ? ctx->n_entries : ctx->min_rows);    // capacity only
    bool moved = false;
    int rc = ctx->d_scores.grow(nq * rows, &moved);
    if (rc != SAT_OK) return rc;
    if (moved) ctx->desc_dirty = true;
    if (lsoln) {
        size_t need = 0, n1sum = 0;
        for (auto &q : ctx->queries) {
            q.ssemap_off = need;
            need += (size_t)ctx->n_entries * q.n1;
            n1sum += (size_t)q.n1;
        }
        if (rows * n1sum > need) need = rows * n1sum;
        if ((rc = ctx->d_ssemaps.grow(need, &moved)) != SAT_OK) return rc;
        if (moved || !ctx->desc_lsoln) ctx->desc_dirty = true;
    }
    if (!ctx->desc_dirty) return SAT_OK;

    std::vector<SatQuery> desc;
    desc.reserve(nq);
    for (int c = 0; c < 4; c++) {
        ctx->class_begin[c] = (int)desc.size();
        ctx->class_n1max[c] = 0;
        ctx->class_wpl[c] = -1;                       // -1: no query yet, 0: mixed
        for (size_t qi = 0; qi < nq; qi++) {
            auto &q = ctx->queries[qi];
            if (q.n1p != kClassN1P[c]) continue;
            q.cls = c;
            q.desc = (int)desc.size();
            const uint8_t *blob = ctx->d_qblob.get() + q.blob_off;
            const size_t groups = (size_t)q.n1p / 4 * q.n1p;
            SatQuery d;
            d.qdist = reinterpret_cast<const float4 *>(blob);
            d.qcode = reinterpret_cast<const uint32_t *>(blob + groups * 16);
            d.qtypes = blob + groups * 20;
            d.qpair = reinterpret_cast<const uint2 *>(blob + ((groups * 20 + (size_t)q.n1p + 15) & ~(size_t)15));
            d.n1 = q.n1;
            d.pad_ = 0;
            d.seed_q = ctx->seed + ((uint64_t)q.ordinal << 32);
            d.scores = ctx->d_scores.get() + qi * (size_t)ctx->n_entries;
            d.ssemaps = lsoln ? ctx->d_ssemaps.get() + q.ssemap_off : nullptr;
            desc.push_back(d);
            if (q.n1 > ctx->class_n1max[c]) ctx->class_n1max[c] = q.n1;
            int lpi, wpl;
            satk::compaction_shape((q.n1 + 3) >> 2, lpi, wpl);
            ctx->class_wpl[c] = ctx->class_wpl[c] < 0 ? wpl : (ctx->class_wpl[c] == wpl ? wpl : 0);
        }
        if (ctx->class_wpl[c] < 0) ctx->class_wpl[c] = 0;
    }
    ctx->class_begin[4] = (int)desc.size();
    // ordered after earlier launches on the stream; the host vector dies at return, so wait
    HIP_TRY(hipMemcpyAsync(ctx->d_qdesc.get(), desc.data(), desc.size() * sizeof(SatQuery), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    ctx->desc_dirty = false;
    ctx->desc_lsoln = lsoln;
    return SAT_OK;
}

// Entries per workgroup.  A CU hands out its LDS in 128 granules of 1280 bytes (measured,
// scripts/exp/lds_probe.hip: 128-thread workgroups drop from 12 to 11 to 10 per CU at 12 800 and 14 080
// bytes, 384-thread ones from 4 to 3 at 40 960), so a workgroup of one entry wastes up to a granule plus
// what is left over at the end of the CU.  k entries side by side round up once: the bench entry's
// 13 320 bytes fit 11 times alone (11 granules each) and 6 x 2 times in pairs (21 granules a pair).
// Picks the smallest k with the most resident entries, the register file's wave limit included.  Only
// workgroups of a multiple of 4 waves and at most 512 threads are considered: measured on the bench,
// 6-wave workgroups do not spread evenly over the 4 SIMDs (8.5 M scorings/s against 10.6 M), and 12-wave
// ones lose to their own start-up and drain phases what the extra residency gains (10.4 M).
int resident_by_lds(size_t bytes) { return (int)(128 / ((bytes + 1279) / 1280)); }

int pick_epw(const void *fn, int threads, size_t lds_stride)
{
    int best = 1, best_entries = 0;
    for (int k = 1; k * threads <= 512 && (size_t)k * lds_stride <= kLdsLimit; k++) {
        if (k > 1 && (k * threads / 64) % 4 != 0) continue;
        int by_regs = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&by_regs, fn, k * threads, 0) != hipSuccess) {
            (void)hipGetLastError();
            return 1;
        }
        const int by_lds = resident_by_lds((size_t)k * lds_stride);
        const int entries = (by_regs < by_lds ? by_regs : by_lds) * k;
        if (entries > best_entries) { best_entries = entries; best = k; }
    }
    return best;
}

// Before a launch of `fn` with `threads` per entry slot and `lds_stride` LDS bytes per slot: raise the
// instantiation's dynamic-LDS limit (once per context), then *epw = its entries per workgroup (see pick_epw; asked
// once per shape).  Launches of under 8192 entry-query pairs (`work`) keep one, for the most workgroups;
// SAT_EXP_EPW overrides where it fits.  epw = null: the caller keeps one entry per workgroup.
int launch_setup(sat_ctx *ctx, const void *fn, int threads, size_t lds_stride, long long work, int *epw)
{
    if (ctx->lds_attr_done.insert(fn).second)
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
    if (!epw) return SAT_OK;
    *epw = 1;
    if (work >= 8192) {
        const auto key = std::make_tuple(fn, threads, lds_stride);
        auto it = ctx->epw_choice.find(key);
        if (it == ctx->epw_choice.end()) it = ctx->epw_choice.emplace(key, pick_epw(fn, threads, lds_stride)).first;
        *epw = it->second;
    }
    if (ctx->tune.epw >= 1 && (size_t)ctx->tune.epw * lds_stride <= kLdsLimit && ctx->tune.epw * threads <= 1024)
        *epw = ctx->tune.epw;
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

// The preconditions of queuing a search, checked in this order: a context, a database (need_db), a query batch,
// maxstart >= 1.
int check_ready(const sat_ctx *ctx, bool need_db, int maxstart)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (need_db && ctx->n_entries <= 0) return sat_fail(SAT_ESTATE, "no database uploaded");
    if (ctx->queries.empty()) return sat_fail(SAT_ESTATE, "no query set");
    if (maxstart < 1) return sat_fail(SAT_EINVAL, "maxstart must be >= 1 (got %d)", maxstart);
    return SAT_OK;
}

// The workgroup of one launch: restart chains (one per restart up to 256, fewer where the LDS would not fit them),
// lanes per chain, where the query cells live, whether the SA step compacts its work, and the LDS bytes of one
// entry slot.  plan_starts = the most restarts one entry slot runs.
struct WgShape { int chains, lpc_shift, threads; bool qlds, compact; size_t lds; };
int size_workgroup(const sat_ctx *ctx, int plan_starts, int n1max, int n1p, int n2max, bool lsoln, bool lorder, WgShape &out)
{
    // chains: one per restart up to 256; shrink until the workgroup fits the LDS.
    // query cells: through L1/L2 for 32-SSE-class queries and up (frees 8+ KB of LDS per
    // workgroup: more resident waves), in LDS for the small class
    int chains = (plan_starts + 63) / 64 * 64;
    if (chains > 256) chains = 256;
    if (ctx->tune.chains >= 64 && ctx->tune.chains < chains) chains = ctx->tune.chains / 64 * 64;
    // work compaction needs sparse maps: with LORDER = F almost every step proposes a real
    // new image, the static loops win and the tables would only cost LDS
    bool compact = lorder != 0;
    if (ctx->tune.compact >= 0) compact = ctx->tune.compact != 0;
    bool qlds = n1p < 32;
    if (ctx->tune.qlds >= 0) qlds = ctx->tune.qlds != 0 || n1p < 32;
    size_t lds = 0;
    for (;;) {
        lds = satk::lds_bytes(n1max, n1p, n2max, chains, chains, lsoln, qlds, compact);
        if (lds <= kLdsLimit) break;
        if (chains > 64) { chains -= 64; continue; }
        if (qlds) {                                    // query cells stay in L1/L2 instead
            qlds = false;
            chains = (plan_starts + 63) / 64 * 64;
            if (chains > 256) chains = 256;
            continue;
        }
        return sat_fail(SAT_EINVAL, "workgroup does not fit in LDS (n1=%d n2=%d)", n1max, n2max);
    }
    // lanes per chain: when LDS leaves fewer than 2 waves per SIMD, let 2 or 4 adjacent lanes
    // share a chain (same cells in LDS, 2-4x the waves; they split the pair loops).  Measured:
    // the smallest sharing that reaches 8 waves per CU wins (one lane per chain also runs the
    // option-specialised kernels); beyond that, sharing only adds redundant bookkeeping.
    int lpc_shift = 0;
    for (int l = 0; l <= 2; l++) {
        if ((chains << l) > 1024 || (l > 0 && n1max <= (8 << (l - 1)))) break;
        const size_t lds_l = satk::lds_bytes(n1max, n1p, n2max, chains, chains << l, lsoln, qlds, compact);
        if (lds_l > kLdsLimit) break;
        lpc_shift = l;
        // (target: 8 resident waves per CU; 12 for the 101-SSE query class, whose steps are the longest
        // dependent chains - measured with the triangle cells: configs[4] 2.31 -> 2.45 M scorings/s, the
        // 101-SSE probe 2.48 -> 2.65 M, while 96-SSE entries under a 32-SSE query lose 5 % at 12)
        const int want_waves = ctx->tune.lpc_waves > 0 ? ctx->tune.lpc_waves : (n1p == 112 ? 12 : 8);
        if (resident_by_lds(lds_l) * ((chains << l) / 64) >= want_waves) break;
    }
    if (ctx->tune.lpc >= 0 && ctx->tune.lpc <= 2 && (chains << ctx->tune.lpc) <= 1024) lpc_shift = ctx->tune.lpc;
    // the per-wave tables grow with the lanes: re-size, backing off if that no longer fits
    for (;; lpc_shift--) {
        lds = satk::lds_bytes(n1max, n1p, n2max, chains, chains << lpc_shift, lsoln, qlds, compact);
        if (lds <= kLdsLimit || lpc_shift == 0) break;
    }
    const int threads = chains << lpc_shift;
    // experiment knob: extra (unused) LDS bytes per workgroup, to lower the occupancy
    if (ctx->tune.lds_pad && lds + ctx->tune.lds_pad <= kLdsLimit) lds += ctx->tune.lds_pad;
    out.chains = chains;
    out.lpc_shift = lpc_shift;
    out.threads = threads;
    out.qlds = qlds;
    out.compact = compact;
    out.lds = lds;
    return SAT_OK;
}

// What a launch of the SA kernel needs beyond its work list: the workgroup, the kernel, the entry slots per workgroup
// (epw), the LDS bytes between two slots and of the whole workgroup, and the arguments with the shape fields filled
// (the caller adds the work list, the queries and the slabs).
struct SaLaunch { WgShape w; SaKernel k; int epw; size_t lds_stride, lds_launch; SatKernelArgs args; };

// Prepare the launches of family `mode` for queries of class c and entries of up to n2max SSEs: the workgroup sized for
// plan_starts restarts, the kernel - option-specialised when the workgroup has the default layout for these options
// (which of them exist is pick_sa_kernel's business) -, its LDS limit and, with `pack`, the entry slots per workgroup
// for `work` entry-query pairs (else one).
int prepare_sa(sat_ctx *ctx, int mode, int lorder, int lsoln, int maxstart, int plan_starts, int c, int n2max, long long work,
               bool pack, SaLaunch &out)
{
    const int n1p = kClassN1P[c], m2w = satk::set_words(n2max);
    WgShape &w = out.w;                       // (lds_bytes sizes it for the same set width and cell layout)
    int rc = size_workgroup(ctx, plan_starts, ctx->class_n1max[c], n1p, n2max, lsoln != 0, lorder != 0, w);
    if (rc != SAT_OK) return rc;
    const bool special = (w.lpc_shift == 0 || m2w == 4) && w.compact == (lorder != 0) && !ctx->tune.general && !(mode & kMatch);
    const int opt = special ? (lorder ? 1 : 0) | (lsoln ? 2 : 0) | (w.lpc_shift << 2) : -1;
    out.k = pick_sa_kernel(mode, n1p, m2w, satk::cell_layout(n2max), w.qlds, opt, ctx->class_wpl[c]);
    if (!out.k.fn) return sat_fail(SAT_EDEVICE, "no kernel variant for n1p=%d m2w=%d", n1p, m2w);
    out.lds_stride = (w.lds + 15) & ~(size_t)15;
    out.epw = 1;
    if ((rc = launch_setup(ctx, out.k.fn, w.threads, out.lds_stride, work, pack ? &out.epw : nullptr)) != SAT_OK) return rc;
    out.lds_launch = out.epw > 1 ? (size_t)out.epw * out.lds_stride : w.lds;
    out.args = base_args(ctx, lorder, lsoln, maxstart);
    out.args.epw = out.epw;
    out.args.tpe = w.threads;
    out.args.lds_stride = (uint32_t)out.lds_stride;
    out.args.lpc_shift = w.lpc_shift;
    out.args.compact = w.compact ? 1 : 0;
    return SAT_OK;
}

// The entries a set of launches covers: indices into the resident shard grouped by order bucket.  A search
// covers the whole shard (the context's lists); the overlapped upload (sat_db_upload_search) searches the
// shard piece by piece, each piece with lists of its own.
struct ListView {
    const int32_t *d_list;       // device array the `begin` offsets index
    const int *begin;            // [kNumBuckets + 1]
    const int *n2max;            // [kNumBuckets] largest order per bucket, 0 = empty
    int n;                       // entries covered = begin[kNumBuckets] - begin[0]
};

// mx: one pass of the match mode (sat_search_matches) instead of a plain search; lsoln is 0 then.  Its record pass
// keeps one record slab per entry slot (scores and db sets of every restart) in the best-map scratch, its replay
// pass a best-map slab per slot there and runs max_matches restarts per entry (workgroups sized for that).
int launch_search(sat_ctx *ctx, int lorder, int lsoln, int maxstart, hipStream_t stream, const ListView *piece = nullptr,
                  const SatMatchArgs *mx = nullptr)
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
            rc = prepare_sa(ctx, mx ? kMatch : kPlain, lorder, lsoln, maxstart, replay ? mx->max_matches : maxstart, c, pl.n2max,
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
        int rc = prepare_sa(ctx, pm ? kPairMatch : kPair, lorder, map_pass && !pm, pm ? pm->maxstart : starts,
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
                            const int32_t *entry, int npairs, bool polish)
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
        // the polish walks the launch's map items: one per pair, with its descriptor and entry
        if (polish && (rc = sat_polish_run(ctx, lorder, ctx->d_pitems.get() + ch.grp.moff.front(), ch.n, max_matches, n2_all, npairs,
                                           pm.mx.counts, pm.mx.scores, pm.mx.restarts, pm.mx.maps)) != SAT_OK)
            return rc;
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

namespace {

// Upload validation: one wave per db entry reads the entry's packed triangle where the search will
// read it and flags cells outside the kernel's domain; the lowest flagged entry index survives.
// (entries e_begin .. e_end - 1: the overlapped upload checks the shard piece by piece)
__global__ void __launch_bounds__(256) validate_cells(int e_begin, int e_end, const int32_t *orders, const int64_t *cell_off,
                                                      const uint8_t *tab, const float *dist, int32_t *first_bad)
{
    const int e = e_begin + blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= e_end) return;
    const int n = orders[e];
    const int64_t base = cell_off[e];
    const int cells = n * (n + 1) / 2;
    bool bad = false;
    for (int c = lane; c < cells; c += 64) {
        // row i of cell c: the largest i with i (i + 1) / 2 <= c; diagonal cells hold the SSE type
        int i = (int)((sqrtf(8.0f * (float)c + 1.0f) - 1.0f) * 0.5f);
        while ((i + 1) * (i + 2) / 2 <= c) i++;
        while (i * (i + 1) / 2 > c) i--;
        const bool diagonal = c == i * (i + 1) / 2 + i;
        const uint8_t t = tab[base + c];
        if (diagonal) {
            bad |= t > 3;
        } else {
            const float ad = fabsf(dist[base + c]);
            bad |= (t & 0x88u) != 0 || (ad >= 1.0e29f && ad <= 3.4028234e38f);      // finite and out of range
        }
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0) atomicMin(first_bad, e);
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
        ctx->tune.compact = env_int("SAT_EXP_COMPACT", -1);
        ctx->tune.qlds = env_int("SAT_EXP_QLDS", -1);
        ctx->tune.lpc = env_int("SAT_EXP_LPC", -1);
        ctx->tune.general = env_int("SAT_EXP_GENERAL", 0);
        ctx->tune.streams = env_int("SAT_EXP_STREAMS", -1);
        ctx->tune.upload_threads = env_int("SAT_EXP_UPLOAD_THREADS", 0);
        ctx->tune.upload_timing = env_int("SAT_EXP_UPLOAD_TIMING", 0);
        ctx->tune.upload_pieces = env_int("SAT_EXP_UPLOAD_PIECES", 0);
        ctx->tune.epw = env_int("SAT_EXP_EPW", 0);
        ctx->tune.lpc_waves = env_int("SAT_EXP_LPC_WAVES", 0);
        ctx->tune.chains = env_int("SAT_EXP_CHAINS", 0);
        ctx->tune.refine_split = env_int("SAT_EXP_REFINE_SPLIT", 0);
        const int pad = env_int("SAT_EXP_LDS_PAD", 0);
        ctx->tune.lds_pad = pad > 0 ? (size_t)pad : 0;
        if (ctx->tune.streams != 0) {
            for (int b = 0; b < kNumBuckets; b++) {
                HIP_TRY(hipStreamCreateWithFlags(&ctx->side_stream[b], hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&ctx->ev_join[b], hipEventDisableTiming));
            }
            HIP_TRY(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
        }
        const int rc_tab = build_metropolis_table(ctx);
        if (rc_tab != SAT_OK) return rc_tab;
        // load the library's code object now (an empty launch of its smallest kernel): the ~5 ms the
        // first launch of a process pays for it belong to context creation, not to the first upload
        hipLaunchKernelGGL(validate_cells, dim3(1), dim3(256), 0, ctx->stream, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
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

// What sat_db_upload_search asks of the upload: the first search of the current query batch, queued piece
// by piece behind the copies.
struct FirstSearch { int lorder, lsoln, maxstart; };

// Counting sort of entries e_begin .. e_end - 1 by order into `out` (appended at position `pos`): bucket after
// bucket, inside a bucket the LARGEST entries first (file order among equals) - workgroups are dispatched in
// list order and a larger entry runs longer, so a launch ends on its cheapest workgroups instead of its dearest
// (real databases are sorted ascending).  begin[kNumBuckets + 1] / n2max[kNumBuckets] describe the result.
// (two passes over the entries: seven filtered passes and a stable sort per bucket took 3 ms of an 11 ms
// upload of the bench shard)
static void bucket_lists(const int32_t *orders, int e_begin, int e_end, int32_t *out, int pos, int *begin, int *n2max)
{
    int count[SAT_MAXDIM + 1] = { 0 }, start[SAT_MAXDIM + 1] = { 0 };
    for (int e = e_begin; e < e_end; e++) count[orders[e]]++;
    for (int b = 0; b < kNumBuckets; b++) {
        begin[b] = pos;
        n2max[b] = 0;
        const int lo = b == 0 ? 0 : kBucketMax[b - 1];
        for (int n = kBucketMax[b] < SAT_MAXDIM ? kBucketMax[b] : SAT_MAXDIM; n > lo; n--) {
            start[n] = pos;
            pos += count[n];
            if (count[n] && n2max[b] == 0) n2max[b] = n;
        }
    }
    begin[kNumBuckets] = pos;
    for (int e = e_begin; e < e_end; e++) out[(size_t)start[orders[e]]++] = e;
}

static int upload_impl(sat_ctx *ctx, int n_entries, const int32_t *orders,
                       const int64_t *cell_off, const uint8_t *tab_tri,
                       const float *dist_tri, const int64_t *db_ordinal, const FirstSearch *first)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (n_entries <= 0 || !orders || !cell_off || !tab_tri || !dist_tri)
        return sat_fail(SAT_EINVAL, "empty database or null array");
    if (first) {
        const int rc = check_ready(ctx, false, first->maxstart);
        if (rc != SAT_OK) return rc;
    }
    // header pass on the host (orders, offsets, ordinals: a few bytes per entry).  The CELLS - every
    // code byte and distance, 331 MB for the bench shard - are checked on the GPU after the copy, at
    // HBM speed (validate_cells): a host scan of them cost as much as the copy itself.
    int64_t cells_end = 0;
    bool ascending = true;                     // entry e + 1 starts at or after the end of entry e
    for (int e = 0; e < n_entries; e++) {
        const int n = orders[e];
        if (n < 1 || n > SAT_MAXDIM)
            return sat_fail(SAT_EINVAL, "entry %d: order %d outside 1..%d", e, n, SAT_MAXDIM);
        if (cell_off[e] < 0) return sat_fail(SAT_EINVAL, "entry %d: negative cell offset", e);
        if (cell_off[e] < cells_end) ascending = false;
        int64_t end = cell_off[e] + (int64_t)n * (n + 1) / 2;
        if (end > cells_end) cells_end = end;
        if (db_ordinal && (db_ordinal[e] < 0 || db_ordinal[e] > 0xFFFFFFFFll))
            return sat_fail(SAT_EINVAL, "entry %d: db ordinal out of range", e);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    free_db(ctx);
    const bool timing = ctx->tune.upload_timing != 0;
    auto now_ms = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_mark = now_ms();
    auto lap = [&](const char *what) {
        if (timing) { const double t = now_ms(); fprintf(stderr, "upload: %-18s %7.3f ms\n", what, t - t_mark); t_mark = t; }
    };

    const size_t dist_bytes = (size_t)cells_end * sizeof(float), tab_bytes = (size_t)cells_end;
    // Pieces: with a first search to overlap, the shard goes up in `npieces` runs of whole entries of about
    // equal cell count, and every piece is checked and searched as soon as it has landed - the GPU works on
    // piece c while the host threads copy piece c + 1 (the copies are synchronous calls out of the caller's
    // pageable memory; the kernels run on the context's non-blocking stream).  Needs entries laid out in
    // ascending order (a piece is then one contiguous cell range); small shards go up in one piece.
    int npieces = 1;
    if (first && ascending) {
        // at least 24 MB of distances per piece (each host thread's slice of it is then still a copy of a
        // useful size), at most 8: measured on the 331 MB bench shard, 19.4 ms for upload-then-search,
        // 16.3 / 14.6 / 14.2 / 15.2 / 16.8 ms overlapped in 2 / 4 / 8 / 12 / 16 pieces
        const size_t by_size = dist_bytes / ((size_t)24 << 20);
        npieces = ctx->tune.upload_pieces > 0 ? ctx->tune.upload_pieces : (int)(by_size < 8 ? by_size : 8);
        if (npieces > n_entries) npieces = n_entries;
        if (npieces < 1) npieces = 1;
    }
    std::vector<int> piece_e((size_t)npieces + 1, n_entries);        // piece c = entries piece_e[c] .. piece_e[c+1]-1
    piece_e[0] = 0;
    for (int c = 1, e = 0; c < npieces; c++) {
        const int64_t target = cells_end * c / npieces;
        while (e < n_entries && cell_off[e] < target) e++;
        piece_e[(size_t)c] = e > piece_e[(size_t)c - 1] ? e : piece_e[(size_t)c - 1];
    }
    auto piece_cell = [&](int c) -> int64_t { return c >= npieces || piece_e[(size_t)c] >= n_entries ? cells_end : (c == 0 ? 0 : cell_off[piece_e[(size_t)c]]); };

    // bucket lists of the whole shard (every later search) and, behind them, of each piece
    std::vector<int32_t> lists((size_t)n_entries * (npieces > 1 ? 2 : 1));
    bucket_lists(orders, 0, n_entries, lists.data(), 0, ctx->bucket_begin, ctx->bucket_n2max);
    std::vector<int> piece_begin((size_t)npieces * (kNumBuckets + 1)), piece_n2max((size_t)npieces * kNumBuckets);
    if (npieces > 1) {
        int pos = n_entries;
        for (int c = 0; c < npieces; c++) {
            bucket_lists(orders, piece_e[(size_t)c], piece_e[(size_t)c + 1], lists.data(), pos,
                         &piece_begin[(size_t)c * (kNumBuckets + 1)], &piece_n2max[(size_t)c * kNumBuckets]);
            pos += piece_e[(size_t)c + 1] - piece_e[(size_t)c];
        }
    }

    std::vector<uint32_t> ord(n_entries);
    for (int e = 0; e < n_entries; e++) ord[e] = db_ordinal ? (uint32_t)db_ordinal[e] : (uint32_t)e;

    lap("host lists");
    DevBuf<int32_t> d_bad;
    const int32_t none = 0x7FFFFFFF;
    // any failure below leaves the context without a database
    auto body = [&]() -> int {
        const size_t n = (size_t)n_entries;
        int rc;
        // (scores: one row, so that the first search of one query does not re-allocate them - refresh_descriptors)
        if ((rc = ctx->d_orders.grow(n)) != SAT_OK || (rc = ctx->d_cell_off.grow(n)) != SAT_OK ||
            (rc = ctx->d_ordinal.grow(n)) != SAT_OK || (rc = ctx->d_lists.grow(lists.size())) != SAT_OK ||
            (rc = ctx->d_tab.grow((size_t)cells_end)) != SAT_OK || (rc = ctx->d_dist.grow((size_t)cells_end)) != SAT_OK ||
            (rc = ctx->d_scores.grow(n)) != SAT_OK || (rc = d_bad.grow(1)) != SAT_OK)
            return rc;
        lap("hipMalloc");
        // the headers first: the piece-wise checks and searches read them
        HIP_TRY(hipMemcpy(ctx->d_orders.get(), orders, n * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ctx->d_cell_off.get(), cell_off, n * sizeof(int64_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ctx->d_ordinal.get(), ord.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ctx->d_lists.get(), lists.data(), lists.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(ctx->d_scores.get(), 0, n * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(d_bad.get(), &none, sizeof none, hipMemcpyHostToDevice));
        lap("header copies");
        ctx->n_entries = n_entries;

        // The two big arrays go up in slices from a few host threads (each slice a synchronous copy out
        // of the caller's pageable memory: the runtime stages it through its pinned buffers, and several
        // copies in flight keep the link busy while one thread waits for its staging buffer).  The threads
        // walk the pieces together and count themselves off per piece; thread 0 queues the check of a
        // complete piece and (sat_db_upload_search) its search, and goes on copying.
        unsigned hw = std::thread::hardware_concurrency();
        int nthreads = (int)(hw ? (hw < 4 ? hw : 4) : 1);
        if (ctx->tune.upload_threads > 0) nthreads = ctx->tune.upload_threads;
        if (dist_bytes < ((size_t)32 << 20)) nthreads = 1;
        std::vector<hipError_t> err((size_t)nthreads, hipSuccess);
        std::vector<std::atomic<int>> landed((size_t)npieces);
        for (auto &x : landed) x.store(0);
        auto copy_piece = [&](int t, int c) {
            const size_t c0 = (size_t)piece_cell(c), c1 = (size_t)piece_cell(c + 1);
            auto part = [&](const void *src, void *dst, size_t unit) {
                const size_t bytes = (c1 - c0) * unit, base = c0 * unit;
                const size_t lo = (bytes * (size_t)t / (size_t)nthreads) & ~(size_t)255;
                const size_t hi = t + 1 == nthreads ? bytes : (bytes * (size_t)(t + 1) / (size_t)nthreads) & ~(size_t)255;
                if (hi > lo && err[(size_t)t] == hipSuccess)
                    err[(size_t)t] = hipMemcpy((char *)dst + base + lo, (const char *)src + base + lo, hi - lo, hipMemcpyHostToDevice);
            };
            part(dist_tri, ctx->d_dist.get(), sizeof(float));
            part(tab_tri, ctx->d_tab.get(), 1);
            landed[(size_t)c].fetch_add(1, std::memory_order_release);
        };
        // (the runtime takes the copies of all threads through one queue: a thread running ahead into piece
        // c + 1 would delay the last slice of piece c, and with it the piece's search, so nobody starts a
        // piece before the one before it is complete)
        auto piece_complete = [&](int c) {
            while (landed[(size_t)c].load(std::memory_order_acquire) < nthreads) std::this_thread::yield();
        };
        auto helper = [&](int t) {
            (void)hipSetDevice(ctx->device);
            for (int c = 0; c < npieces; c++) {
                copy_piece(t, c);
                if (c + 1 < npieces) piece_complete(c);
            }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < nthreads; t++) pool.emplace_back(helper, t);
        rc = SAT_OK;
        for (int c = 0; c < npieces; c++) {
            copy_piece(0, c);
            piece_complete(c);
            if (rc != SAT_OK) continue;                      // (the helpers still finish their copies)
            // ---- check every cell where it now lives: one wave per entry; the kernel's pair arithmetic needs
            // tableau nibbles 0..7 (the reader produces 0..4), SSE types 0..3 and |distance| < 1e29 or non-finite.
            // A search queued behind the check of a bad piece is memory-safe (orders and offsets were checked
            // above; bad cells only give wrong sums) and its results are thrown away below.
            const int e0 = piece_e[(size_t)c], e1 = piece_e[(size_t)c + 1];
            if (e1 <= e0) continue;
            hipLaunchKernelGGL(validate_cells, dim3((unsigned)((e1 - e0 + 3) / 4)), dim3(256), 0, ctx->stream,
                               e0, e1, ctx->d_orders.get(), ctx->d_cell_off.get(), ctx->d_tab.get(), ctx->d_dist.get(), d_bad.get());
            if (hipGetLastError() != hipSuccess) { rc = sat_fail(SAT_EDEVICE, "launch of the cell check failed"); continue; }
            if (first) {
                if (npieces > 1) {
                    const ListView piece = { ctx->d_lists.get(), &piece_begin[(size_t)c * (kNumBuckets + 1)],
                                             &piece_n2max[(size_t)c * kNumBuckets], e1 - e0 };
                    rc = launch_search(ctx, first->lorder, first->lsoln, first->maxstart, ctx->stream, &piece);
                } else {
                    rc = launch_search(ctx, first->lorder, first->lsoln, first->maxstart, ctx->stream);
                }
            }
        }
        for (auto &th : pool) th.join();
        if (rc != SAT_OK) return rc;
        for (int t = 0; t < nthreads; t++) HIP_TRY(err[(size_t)t]);
        lap(first ? "cell copies, checks and the search queued" : "cell copies");
        int32_t bad = none;
        HIP_TRY(hipStreamSynchronize(ctx->stream));          // a non-blocking stream: the copy below does not wait for it
        HIP_TRY(hipMemcpy(&bad, d_bad.get(), sizeof bad, hipMemcpyDeviceToHost));
        lap(first ? "search + validate on GPU" : "validate on GPU");
        if (bad != none) {
            // the earliest flagged entry is looked at again on the host, cell by cell, for the message
            const int e = bad, n = orders[e];
            for (int i = 0; i < n; i++) {
                const int64_t rowbase = cell_off[e] + (int64_t)i * (i + 1) / 2;
                uint8_t ty = tab_tri[rowbase + i];
                if (ty > 3) return sat_fail(SAT_EINVAL, "entry %d: SSE %d has type code %u (0..3 expected)", e, i, ty);
                for (int j = 0; j < i; j++) {
                    if (tab_tri[rowbase + j] & 0x88)
                        return sat_fail(SAT_EINVAL, "entry %d: tableau code 0x%02x at (%d,%d) has a nibble above 7", e, tab_tri[rowbase + j], i, j);
                    float d = dist_tri[rowbase + j];
                    if (std::isfinite(d) && std::fabs(d) >= 1.0e29f)
                        return sat_fail(SAT_EINVAL, "entry %d: distance %g at (%d,%d) out of range", e, d, i, j);
                }
            }
            return sat_fail(SAT_EINVAL, "entry %d: invalid cell", e);     // not reached: the scan and the re-check agree
        }
        return SAT_OK;
    };
    const int rc = body();
    d_bad.reset();
    if (rc != SAT_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        free_db(ctx);
        return rc;
    }
    ctx->h_orders.assign(orders, orders + n_entries);
    return SAT_OK;
}

int sat_db_upload_packed(sat_ctx *ctx, int n_entries, const int32_t *orders,
                         const int64_t *cell_off, const uint8_t *tab_tri,
                         const float *dist_tri, const int64_t *db_ordinal)
{
    return upload_impl(ctx, n_entries, orders, cell_off, tab_tri, dist_tri, db_ordinal, nullptr);
}

int sat_db_upload_search(sat_ctx *ctx, int n_entries, const int32_t *orders,
                         const int64_t *cell_off, const uint8_t *tab_tri,
                         const float *dist_tri, const int64_t *db_ordinal,
                         int lorder, int lsoln, int maxstart)
{
    const FirstSearch first = { lorder, lsoln, maxstart };
    return upload_impl(ctx, n_entries, orders, cell_off, tab_tri, dist_tri, db_ordinal, &first);
}

int sat_db_upload_dense(sat_ctx *ctx, int n_entries, const int32_t *orders,
                        const uint8_t *tabs, const float *dmats, int pitch,
                        const int64_t *db_ordinal)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (n_entries <= 0 || !orders || !tabs || !dmats || pitch < 1)
        return sat_fail(SAT_EINVAL, "empty database or null array");
    std::vector<int64_t> off(n_entries);
    int64_t cells = 0;
    for (int e = 0; e < n_entries; e++) {
        if (orders[e] < 1 || orders[e] > SAT_MAXDIM || orders[e] > pitch)
            return sat_fail(SAT_EINVAL, "entry %d: order %d outside 1..min(%d, pitch %d)", e, orders[e], SAT_MAXDIM, pitch);
        off[e] = cells;
        cells += (int64_t)orders[e] * (orders[e] + 1) / 2;
    }
    std::vector<uint8_t> tt((size_t)cells);
    std::vector<float> dd((size_t)cells);
    for (int e = 0; e < n_entries; e++) {
        const uint8_t *t = tabs + (size_t)e * pitch * pitch;
        const float *d = dmats + (size_t)e * pitch * pitch;
        int64_t c = off[e];
        for (int i = 0; i < orders[e]; i++)
            for (int j = 0; j <= i; j++, c++) {
                tt[(size_t)c] = t[(size_t)i * pitch + j];
                dd[(size_t)c] = d[(size_t)i * pitch + j];
            }
    }
    return sat_db_upload_packed(ctx, n_entries, orders, off.data(), tt.data(), dd.data(), db_ordinal);
}

int sat_db_size(const sat_ctx *ctx) { return ctx ? ctx->n_entries : 0; }

int sat_queries_set(sat_ctx *ctx, int n_queries, const int32_t *n1s, const uint8_t *qtabs,
                    const float *qdmats, int pitch, const uint8_t *qssetypes, uint32_t first_query_ordinal)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (n_queries < 1 || !n1s || !qtabs || !qdmats || !qssetypes || pitch < 1)
        return sat_fail(SAT_EINVAL, "bad query batch (n_queries=%d pitch=%d)", n_queries, pitch);
    std::vector<sat_ctx::QueryInfo> infos((size_t)n_queries);
    size_t blob_bytes = 0;
    for (int qi = 0; qi < n_queries; qi++) {
        const int n1 = n1s[qi];
        if (n1 < 1 || n1 > SAT_MAXDIM || n1 > pitch)
            return sat_fail(SAT_EINVAL, "query %d: order %d outside 1..min(%d, pitch %d)", qi, n1, SAT_MAXDIM, pitch);
        auto &q = infos[(size_t)qi];
        q.n1 = n1;
        q.n1p = n1 <= 16 ? 16 : (n1 <= 32 ? 32 : (n1 <= 64 ? 64 : 112));
        q.ordinal = first_query_ordinal + (uint32_t)qi;
        q.blob_off = blob_bytes;
        q.ssemap_off = 0;
        const size_t groups = (size_t)q.n1p / 4 * q.n1p;
        // grouped cells (16 + 4 bytes per group and column), SSE types, then the dense pair cells of the full score
        blob_bytes += ((groups * 20 + (size_t)q.n1p + 15) & ~(size_t)15) + (size_t)q.n1p * q.n1p * 8;
    }
    // grouped, transposed query: group kw, column i holds dmat1[i][4kw..4kw+3] and the four code
    // bytes tab1[i][4kw..4kw+3]; diagonal, padding and non-finite distances get the sentinel
    // so they never score (the reference excludes k == i, K.cu:524, and NaN never passes <= 4)
    std::vector<uint8_t> blob(blob_bytes, 0);
    for (int qi = 0; qi < n_queries; qi++) {
        const auto &q = infos[(size_t)qi];
        const int n1 = q.n1, n1p = q.n1p, groups = n1p / 4;
        const uint8_t *qtab = qtabs + (size_t)qi * pitch * pitch;
        const float *qdmat = qdmats + (size_t)qi * pitch * pitch;
        const uint8_t *types = qssetypes + (size_t)qi * pitch;
        float4 *qdist = reinterpret_cast<float4 *>(blob.data() + q.blob_off);
        uint32_t *qcode = reinterpret_cast<uint32_t *>(blob.data() + q.blob_off + (size_t)groups * n1p * 16);
        uint8_t *qtypes = blob.data() + q.blob_off + (size_t)groups * n1p * 20;
        // dense [i][k] cells {distance, code byte}: the same values as the grouped arrays, for the pair-by-pair
        // full score of an initial map
        uint32_t *qpair = reinterpret_cast<uint32_t *>(blob.data() + q.blob_off + (((size_t)groups * n1p * 20 + (size_t)n1p + 15) & ~(size_t)15));
        for (int i = 0; i < n1p; i++)
            for (int k = 0; k < n1p; k++) {
                float d = SAT_K_QSENT;
                uint32_t code = 0;
                if (k < n1 && i < n1 && k != i) {
                    const float v = qdmat[(size_t)i * pitch + k];
                    if (std::isfinite(v)) d = v;                  // (range and nibbles are checked below)
                    code = qtab[(size_t)i * pitch + k];
                }
                memcpy(&qpair[((size_t)i * n1p + k) * 2], &d, sizeof d);
                qpair[((size_t)i * n1p + k) * 2 + 1] = code;
            }
        for (int i = 0; i < n1; i++) {
            if (types[i] > 3)
                return sat_fail(SAT_EINVAL, "query %d: SSE %d has type code %u (0..3 expected)", qi, i, types[i]);
            qtypes[i] = types[i];
        }
        for (int kw = 0; kw < groups; kw++)
            for (int i = 0; i < n1p; i++) {
                float d[4];
                uint32_t codes = 0;
                for (int sidx = 0; sidx < 4; sidx++) {
                    const int k = 4 * kw + sidx;
                    d[sidx] = SAT_K_QSENT;
                    if (k < n1 && i < n1 && k != i) {
                        const float v = qdmat[(size_t)i * pitch + k];
                        const uint32_t code = qtab[(size_t)i * pitch + k];
                        if (code & 0x88)
                            return sat_fail(SAT_EINVAL, "query %d: tableau code 0x%02x at (%d,%d) has a nibble above 7", qi, code, i, k);
                        if (std::isfinite(v)) {
                            if (std::fabs(v) >= 1.0e29f)
                                return sat_fail(SAT_EINVAL, "query %d: distance %g at (%d,%d) out of range", qi, v, i, k);
                            d[sidx] = v;
                        }
                        codes |= code << (8 * sidx);
                    }
                }
                qdist[(size_t)kw * n1p + i] = float4{ d[0], d[1], d[2], d[3] };
                qcode[(size_t)kw * n1p + i] = codes;
            }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->d_qblob.reset();
    ctx->d_qdesc.reset();
    int rc;
    if ((rc = ctx->d_qblob.grow(blob_bytes)) != SAT_OK || (rc = ctx->d_qdesc.grow((size_t)n_queries)) != SAT_OK) return rc;
    HIP_TRY(hipMemcpy(ctx->d_qblob.get(), blob.data(), blob_bytes, hipMemcpyHostToDevice));
    ctx->queries.swap(infos);
    ctx->desc_dirty = true;
    ctx->searched_nq = 0;                     // the result buffers no longer belong to the current batch
    ctx->fits.clear();
    return SAT_OK;
}

int sat_query_set(sat_ctx *ctx, int n1, const uint8_t *qtab, const float *qdmat,
                  int pitch, const uint8_t *qssetypes, uint32_t query_ordinal)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (n1 < 1 || n1 > SAT_MAXDIM || !qtab || !qdmat || !qssetypes || pitch < n1)
        return sat_fail(SAT_EINVAL, "bad query (n1=%d pitch=%d)", n1, pitch);
    // a batch of one; the type vector is only read up to n1, so its stride does not matter
    const int32_t n1s[1] = { n1 };
    return sat_queries_set(ctx, 1, n1s, qtab, qdmat, pitch, qssetypes, query_ordinal);
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
    return launch_search(ctx, lorder, lsoln, maxstart, ctx->stream);
}

void *sat_device_scores(sat_ctx *ctx) { return ctx ? ctx->d_scores.get() : nullptr; }
void *sat_device_ssemaps(sat_ctx *ctx) { return ctx ? ctx->d_ssemaps.get() : nullptr; }
int sat_query_order(const sat_ctx *ctx) { return (ctx && !ctx->queries.empty()) ? ctx->queries[0].n1 : 0; }

unsigned long long sat_stat_d2h_bytes(const sat_ctx *ctx) { return ctx ? ctx->d2h_bytes : 0ull; }

const char *sat_last_launch_info(const sat_ctx *ctx) { return ctx ? ctx->last_launch_info.c_str() : ""; }

void sat_debug_lds_layout(int m2w, int n1, int n1p, int n2, int chains, int threads, int q_in_lds, int compact,
                          uint32_t out[11])
{
    // m2w: low byte = words of a db-side set; bits 8-9 = 1 + cell layout (SAT_CELLS_*), 0 = the layout launches of
    // such entries get (satk::cell_layout)
    const int cells = (m2w >> 8) ? ((m2w >> 8) & 3) - 1 : satk::cell_layout(n2);
    m2w &= 0xFF;
    const satk::LdsLayout L = satk::lds_layout(m2w, cells, n2, satk::map_words((n1 + 3) >> 2), n1p, chains, threads,
                                               q_in_lds != 0, compact != 0);
    const uint32_t v[11] = { L.code, L.qdist, L.qcode, L.smap, L.tmask, L.qtypes, L.leader, L.red, L.red_stride, L.items, L.total };
    for (int i = 0; i < 11; i++) out[i] = v[i];
}

// satabsearch_debug.h: every instantiation pick_sa_kernel can choose, named as sat_last_launch_info names it, one per
// line in the order of the walk (family, class, set width and layout, QLDS, OPT, WPL).  Host only: the walk takes the
// addresses of the kernels' host stubs, which also tell two instantiations apart.
const char *sat_debug_sa_instances(void)
{
    static const std::string list = [] {
        const int layouts[4][2] = { { 1, SAT_CELLS_FULL8 }, { 2, SAT_CELLS_FULL5 }, { 2, SAT_CELLS_TRI5 }, { 4, SAT_CELLS_TRI5 } };
        std::set<const void *> seen;
        std::string out;
        for (int mode = kPlain; mode <= kPairMatch; mode++)
            for (int n1p : kClassN1P)
                for (const auto &l : layouts)
                    for (int qlds = 0; qlds < 2; qlds++)
                        for (int opt = -1; opt <= 11; opt++)
                            for (int wpl = 0; wpl <= 4; wpl++) {
                                const SaKernel k = pick_sa_kernel(mode, n1p, l[0], l[1], qlds != 0, opt, wpl);
                                if (seen.insert(k.fn).second) out += sa_kernel_name(k) + "\n";
                            }
        return out;
    }();
    return list.c_str();
}

int sat_sync(sat_ctx *ctx)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SAT_OK;
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
    const int rc = timed(ctx, kernel_ms, [&] { return launch_search(ctx, lorder, lsoln, maxstart, ctx->stream); });
    if (rc != SAT_OK) return rc;
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
