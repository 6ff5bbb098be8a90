// sat_capi.hip - C ABI (include/satabsearch.h) over the gfx950 SA kernel.
//
// Host side of the drop-in boundary: the context, its tables, the plan and launches of the plain search and the match
// mode, results.  Host code only: this file holds no kernel.  What goes up - the packed database store, the query
// buffer - is sat_db.hip; which SA kernel a launch runs and with which workgroup is sat_launch.hip, reached through
// sat_launch.hpp only; the pair modes are sat_pairs.hip and sat_polish.hip.  Together they replace the device glue of
// nvcc_src_current/cudaSaTabsearch.cu (init_rng :258-264, copyQueryToConstantMemory :486-558, alloc/upload :896-984,
// launch/sync/download :1036-1087 and :1128-1270).  No CPU search path exists in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "satabsearch.h"
#ifdef SAT_DIAG
#define SAT_DIAG_HOST 1           // diagnostic builds only: the counters' host side (diag/sat_diag.hpp)
#endif
#include "sat_sa_kernel.hpp"
#include "sat_pairs.hpp"
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

}  // namespace

// sat_ctx.hpp
int prepare_launch(sat_ctx *ctx, int mode, int lorder, int lsoln, int maxstart, int plan_starts, int c, int n2max, long long work,
                   bool pack, SaLaunch &out)
{
    out.args = base_args(ctx, lorder, lsoln, maxstart);
    return prepare_sa(ctx->sa, mode, lorder, lsoln, plan_starts, c, ctx->class_n1max[c], ctx->class_wpl[c], n2max, work, pack, out);
}

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
    // that the slabs of all concurrent launches stay under the scratch budget (1 GiB) together (a lane of launches
    // reuses its region launch after launch).  grid.y is limited to 65535: very long query lists are split too.
    const size_t lane_budget_words = ctx->tune.scratch_bytes / 4 / (size_t)nlanes;
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
    ctx->searched_exact = false;
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

#ifdef SAT_DIAG
hipError_t sat_diag_begin(hipStream_t stream, unsigned long long *&arg) { return satdiag::begin(stream, arg); }
hipError_t sat_diag_end(hipStream_t stream) { return satdiag::end(stream); }
#endif

// sat_ctx.hpp
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
        const int scratch_kb = env_int("SAT_EXP_SCRATCH_KB", 0);
        if (scratch_kb > 0) ctx->tune.scratch_bytes = (size_t)scratch_kb << 10;
        const int select_keys = env_int("SAT_EXP_SELECT_KEYS", 0);
        if (select_keys > 0) ctx->tune.select_keys = select_keys;
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
        // load the code objects of the upload, the SA kernels, the pair modes and the clustering now (an empty launch of a small kernel, or
        // a question about one): the ~5 ms the first launch of a process pays for them belong to context creation, not
        // to the first upload or search
        int rc_load;
        if ((rc_load = sat_db_load_code(ctx)) != SAT_OK || (rc_load = sa_load_code()) != SAT_OK ||
            (rc_load = sat_pairs_load_code(ctx)) != SAT_OK || (rc_load = sat_cluster_load_code(ctx)) != SAT_OK ||
            (rc_load = sat_eval_load_code(ctx)) != SAT_OK || (rc_load = sat_cover_load_code(ctx)) != SAT_OK ||
            (rc_load = sat_profile_load_code(ctx)) != SAT_OK || (rc_load = sat_reorder_load_code(ctx)) != SAT_OK ||
            (rc_load = sat_exact_load_code(ctx)) != SAT_OK || (rc_load = sat_reach_load_code(ctx)) != SAT_OK)
            return rc_load;
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
