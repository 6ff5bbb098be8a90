// sat_launch.hip - the SA kernels' translation unit: every instantiation of sat_sa_kernel.hpp and the code that picks
// one and sizes its workgroup (sat_launch.hpp).  Nothing here knows the context: the state a context keeps for it is a
// SaLaunchState, the facts of a query class are arguments.  build.kernel_source_hash() covers exactly this file, its
// header and the kernel's two sources.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <set>
#include <string>
#include <type_traits>

#include "satabsearch.h"
#include "sat_sa_kernel.hpp"
#include "sat_launch.hpp"

namespace {

constexpr size_t kLdsLimit = 160 * 1024;

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

}  // namespace

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

namespace {

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

}  // namespace

// One launch as sat_last_launch_info names it: "kernel<template arguments> [items N] grid X x Y block E x T lds B"
// (items: the pair families' item count; E entry slots of T threads; B the LDS bytes of one slot).
std::string launch_info(const SaKernel &k, int items, int grid_x, int grid_y, int epw, int threads, size_t lds)
{
    char count[32] = "", buf[128];
    if (k.mode & kPair) snprintf(count, sizeof count, " items %d", items);
    snprintf(buf, sizeof buf, "%s grid %d x %d block %d x %d lds %zu", count, grid_x, grid_y, epw, threads, lds);
    return sa_kernel_name(k) + buf;
}

namespace {

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
int launch_setup(SaLaunchState &st, const void *fn, int threads, size_t lds_stride, long long work, int *epw)
{
    if (st.lds_attr_done.insert(fn).second)
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
    if (!epw) return SAT_OK;
    *epw = 1;
    if (work >= 8192) {
        const auto key = std::make_tuple(fn, threads, lds_stride);
        auto it = st.epw_choice.find(key);
        if (it == st.epw_choice.end()) it = st.epw_choice.emplace(key, pick_epw(fn, threads, lds_stride)).first;
        *epw = it->second;
    }
    if (st.epw >= 1 && (size_t)st.epw * lds_stride <= kLdsLimit && st.epw * threads <= 1024)
        *epw = st.epw;
    return SAT_OK;
}

// plan_starts = the most restarts one entry slot runs.
int size_workgroup(const SaLaunchState &st, int plan_starts, int n1max, int n1p, int n2max, bool lsoln, bool lorder, WgShape &out)
{
    // chains: one per restart up to 256; shrink until the workgroup fits the LDS.
    // query cells: through L1/L2 for 32-SSE-class queries and up (frees 8+ KB of LDS per
    // workgroup: more resident waves), in LDS for the small class
    int chains = (plan_starts + 63) / 64 * 64;
    if (chains > 256) chains = 256;
    if (st.chains >= 64 && st.chains < chains) chains = st.chains / 64 * 64;
    // work compaction needs sparse maps: with LORDER = F almost every step proposes a real
    // new image, the static loops win and the tables would only cost LDS
    bool compact = lorder != 0;
    if (st.compact >= 0) compact = st.compact != 0;
    bool qlds = n1p < 32;
    if (st.qlds >= 0) qlds = st.qlds != 0 || n1p < 32;
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
        const int want_waves = st.lpc_waves > 0 ? st.lpc_waves : (n1p == 112 ? 12 : 8);
        if (resident_by_lds(lds_l) * ((chains << l) / 64) >= want_waves) break;
    }
    if (st.lpc >= 0 && st.lpc <= 2 && (chains << st.lpc) <= 1024) lpc_shift = st.lpc;
    // the per-wave tables grow with the lanes: re-size, backing off if that no longer fits
    for (;; lpc_shift--) {
        lds = satk::lds_bytes(n1max, n1p, n2max, chains, chains << lpc_shift, lsoln, qlds, compact);
        if (lds <= kLdsLimit || lpc_shift == 0) break;
    }
    const int threads = chains << lpc_shift;
    // experiment knob: extra (unused) LDS bytes per workgroup, to lower the occupancy
    if (st.lds_pad && lds + st.lds_pad <= kLdsLimit) lds += st.lds_pad;
    out.chains = chains;
    out.lpc_shift = lpc_shift;
    out.threads = threads;
    out.qlds = qlds;
    out.compact = compact;
    out.lds = lds;
    return SAT_OK;
}

}  // namespace

// Prepare the launches of family `mode` for queries of class c and entries of up to n2max SSEs: the workgroup sized for
// plan_starts restarts, the kernel - option-specialised when the workgroup has the default layout for these options
// (which of them exist is pick_sa_kernel's business) -, its LDS limit and, with `pack`, the entry slots per workgroup
// for `work` entry-query pairs (else one).  Of out.args only the shape fields are written: the rest is the caller's.
int prepare_sa(SaLaunchState &st, int mode, int lorder, int lsoln, int plan_starts, int c, int n1max, int wpl, int n2max,
               long long work, bool pack, SaLaunch &out)
{
    const int n1p = kClassN1P[c], m2w = satk::set_words(n2max);
    WgShape &w = out.w;                       // (lds_bytes sizes it for the same set width and cell layout)
    int rc = size_workgroup(st, plan_starts, n1max, n1p, n2max, lsoln != 0, lorder != 0, w);
    if (rc != SAT_OK) return rc;
    const bool special = (w.lpc_shift == 0 || m2w == 4) && w.compact == (lorder != 0) && !st.general && !(mode & kMatch);
    const int opt = special ? (lorder ? 1 : 0) | (lsoln ? 2 : 0) | (w.lpc_shift << 2) : -1;
    out.k = pick_sa_kernel(mode, n1p, m2w, satk::cell_layout(n2max), w.qlds, opt, wpl);
    if (!out.k.fn) return sat_fail(SAT_EDEVICE, "no kernel variant for n1p=%d m2w=%d", n1p, m2w);
    out.lds_stride = (w.lds + 15) & ~(size_t)15;
    out.epw = 1;
    if ((rc = launch_setup(st, out.k.fn, w.threads, out.lds_stride, work, pack ? &out.epw : nullptr)) != SAT_OK) return rc;
    out.lds_launch = out.epw > 1 ? (size_t)out.epw * out.lds_stride : w.lds;
    out.args.epw = out.epw;
    out.args.tpe = w.threads;
    out.args.lds_stride = (uint32_t)out.lds_stride;
    out.args.lpc_shift = w.lpc_shift;
    out.args.compact = w.compact ? 1 : 0;
    return SAT_OK;
}

int sa_load_code(void)
{
    // (asking for a kernel's attributes loads the code object it lives in)
    hipFuncAttributes attr;
    HIP_TRY(hipFuncGetAttributes(&attr, sa_instance<kPlain, 16, 1, true, -1, 0, SAT_CELLS_FULL8>()));
    return SAT_OK;
}

extern "C" {

void sat_debug_lds_layout(int m2w, int n1, int n1p, int n2, int chains, int threads, int q_in_lds, int compact,
                          uint32_t out[11])
{
    // m2w: low byte = words of a db-side set; bits 8-9 = 1 + cell layout (SAT_CELLS_*), 0 = the layout launches of
    // such entries get (satk::cell_layout); bit 16 = three more words: qmask, qbase, pos
    const int cells = ((m2w >> 8) & 3) ? ((m2w >> 8) & 3) - 1 : satk::cell_layout(n2);
    const bool more = (m2w >> 16) & 1;
    m2w &= 0xFF;
    const satk::LdsLayout L = satk::lds_layout(m2w, cells, n2, satk::map_words((n1 + 3) >> 2), n1p, chains, threads,
                                               q_in_lds != 0, compact != 0);
    const uint32_t v[11] = { L.code, L.qdist, L.qcode, L.smap, L.tmask, L.qtypes, L.leader, L.red, L.red_stride, L.items, L.total };
    for (int i = 0; i < 11; i++) out[i] = v[i];
    if (more) {
        out[11] = L.qmask;
        out[12] = L.qbase;
        out[13] = L.pos;
    }
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

}  // extern "C"
