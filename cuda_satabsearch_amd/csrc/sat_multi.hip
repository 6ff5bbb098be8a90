// sat_multi.hip - one search over the GPUs of a node from ONE host thread (include/satabsearch.h,
// sat_multi_*): the database is cut into contiguous shards of equal cost (csrc/host/sat_shard.c),
// every GPU holds only its shard plus the queries, the search is queued on all of them, and ONE
// gather brings the per-shard score arrays (and the int8 solution maps) into device 0's memory, from
// where a single copy takes them to the host, in database file order.
//
// The reference is single-GPU (cudaSaTabsearch.cu:790 "TODO allow multiple GPUs"); SURVEY.md section
// 8e specifies this mode.  Every (query, entry) pair is independent and the random streams are keyed
// by the entry's ordinal in the whole database, so the result is the same for any number of shards.
//
// The gather is RCCL's ncclGather over xGMI (single-process communicators from ncclCommInitAll; the
// library is loaded with dlopen when a multi-GPU context is created, so single-GPU users never pay
// for it).  Shards are padded to the largest one: a fixed-size gather, the rows are put in order on
// the host after the one device-to-host copy.  SAT_MULTI_GATHER=peer selects hipMemcpyPeerAsync
// into device 0 instead (also what is used when librccl cannot be loaded).
//
// The selection calls (best-k, refine, cutoff, histogram and fit, clustering) do not gather: every shard selects its own
// rows and the host merges them (merge_shards, merge_rows) or sums them.  Their argument checks are those of the
// single-context calls, from sat_cutoff.hpp; what every sharded call repeats - the set's own two checks, the wall clock,
// the search on every shard, stage 1 of best-k and refine - is written once below.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>          // types and prototypes only: the entry points are resolved with dlsym

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

#include "satabsearch_debug.h"
#include "sat_pairs.hpp"
#include "sat_cutoff.hpp"
#include "host/sat_gumbel.h"
#include "host/sat_shard.h"
#include "host/sat_cluster.h"
#include "host/sat_cover.h"
#include "host/sat_eval.h"
#include "host/sat_reach.h"

namespace {

struct Rccl {
    void *handle = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGather) Gather = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;

    bool load()
    {
        if (handle) return true;
        handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!handle) handle = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!handle) return false;
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(handle, "ncclCommInitAll"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(handle, "ncclCommDestroy"));
        Gather = reinterpret_cast<decltype(Gather)>(dlsym(handle, "ncclGather"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(dlsym(handle, "ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(dlsym(handle, "ncclGroupEnd"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(handle, "ncclGetErrorString"));
        return CommInitAll && CommDestroy && Gather && GroupStart && GroupEnd && GetErrorString;
    }
};

Rccl g_rccl;      // process-wide: the library is loaded at most once

}  // namespace

struct sat_multi {
    int ndev = 0;
    std::vector<int> devices;
    std::vector<sat_ctx *> ctx;
    std::vector<int32_t> begin;                 // shard g = entries begin[g] .. begin[g+1]-1 of the database
    int n_entries = 0;
    int pad_rows = 0;                           // largest shard: every shard's rows are padded to it in the gather
    bool use_rccl = false;
    bool force_gather = false;                  // SAT_MULTI_GATHER set: gather also with one GPU (tests)
    bool rccl_required = false;                 // SAT_MULTI_GATHER=rccl: an RCCL failure is an error, no peer-copy fallback
    std::vector<ncclComm_t> comm;
    // gathered rows on device 0: [ndev][nq * pad_rows] scores, [ndev][pad_rows * sum(n1)] map bytes
    DevBuf<int32_t> d_all_scores;
    DevBuf<int8_t> d_all_maps;
    // pinned landing zone of the one device-to-host copy
    void *h_stage = nullptr;
    size_t h_stage_cap = 0;
    std::vector<hipEvent_t> done;               // peer-copy path: shard g's rows have arrived on device 0
    unsigned long long d2h_bytes = 0;
};

namespace {

int rccl_fail(ncclResult_t r, const char *what)
{
    return sat_fail(SAT_EDEVICE, "%s failed: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "RCCL error");
}

int grow_stage(sat_multi *m, size_t bytes)
{
    if (bytes <= m->h_stage_cap) return SAT_OK;
    if (m->h_stage) (void)hipHostFree(m->h_stage);
    m->h_stage = nullptr;
    m->h_stage_cap = 0;
    HIP_TRY(hipHostMalloc(&m->h_stage, bytes, hipHostMallocDefault));
    m->h_stage_cap = bytes;
    return SAT_OK;
}

// the peer-copy path signals "shard g's rows have arrived on device 0" with one event per sender; they are made
// when that path is first taken (at creation without RCCL, or when a gather falls back to it)
int ensure_peer_events(sat_multi *m)
{
    for (int g = 1; g < m->ndev; g++) {
        if (m->done[(size_t)g]) continue;
        HIP_TRY(hipSetDevice(m->devices[(size_t)g]));
        HIP_TRY(hipEventCreateWithFlags(&m->done[(size_t)g], hipEventDisableTiming));
        (void)hipDeviceEnablePeerAccess(m->devices[0], 0);     // best effort: the copy is staged without it
        (void)hipGetLastError();
    }
    return SAT_OK;
}

// wait for everything queued on every GPU of the set (before an error return: no search may still be writing
// result buffers the caller is about to re-use or free); errors of the waits themselves are dropped
void sync_all(sat_multi *m)
{
    for (int g = 0; g < m->ndev; g++) {
        if (hipSetDevice(m->devices[(size_t)g]) == hipSuccess) (void)hipStreamSynchronize(m->ctx[(size_t)g]->stream);
        (void)hipGetLastError();
    }
}

// the error return of a call that has queued work on the GPUs: wait for all of them, keep the message
int bail(sat_multi *m, int rc)
{
    const std::string msg = sat_last_error();
    sync_all(m);
    return sat_fail(rc, "%s", msg.c_str());
}

// step(g) for every shard g in turn (queue work on its GPU, or collect it); the first error bails
template <typename F> int each_shard(sat_multi *m, F step)
{
    for (int g = 0; g < m->ndev; g++) {
        const int rc = step(g);
        if (rc != SAT_OK) return bail(m, rc);
    }
    return SAT_OK;
}

// a set that holds a database: what most entry points ask first (those that check arguments in between call the halves)
int check_uploaded(const sat_multi *m) { return sat_check_uploaded(!m->begin.empty()); }
int check_multi(const sat_multi *m) { return m ? check_uploaded(m) : sat_check_context(m); }

// the wall clock of a call, from where this is made; stop(ms), on the success paths only: the milliseconds (ms may be null)
struct Stopwatch {
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void stop(double *ms) const { if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// a whole-database search queued on every shard (polished where sat_multi_polish_all_set says so)
int search_shards(sat_multi *m, int lorder, int lsoln, int maxstart)
{
    return each_shard(m, [&](int g) { return sat_search_async(m->ctx[(size_t)g], lorder, lsoln, maxstart); });
}

// The k-way merge of one query's per-shard runs, each ranked by score (descending): shard g's run is rows[g][lo] ..
// rows[g][hi - 1] with {lo, hi} = run(g).  take(g, row) receives the first `count` rows of the merged order.  Equal
// scores: the lower shard first - shards are contiguous, so that is database order.
template <typename Run, typename Take>
void merge_shards(const std::vector<std::vector<sat_hit>> &rows, size_t count, Run run, Take take)
{
    const size_t ndev = rows.size();
    std::vector<size_t> head(ndev), end(ndev);
    for (size_t g = 0; g < ndev; g++) std::tie(head[g], end[g]) = run((int)g);
    for (size_t r = 0; r < count; r++) {
        size_t bg = ndev;
        for (size_t g = 0; g < ndev; g++)
            if (head[g] < end[g] && (bg == ndev || rows[g][head[g]].score > rows[bg][head[bg]].score)) bg = g;
        take((int)bg, head[bg]++);
    }
}

// The shards' ranked rows merged into the caller's, query after query: the first count(q) rows of the merge of query q's
// runs run(q, g), every entry indexed in the whole database, and (ssemaps not null) each row's map of maps[g] along.
template <typename Count, typename Run>
void merge_rows(const sat_multi *m, int nq, const std::vector<std::vector<sat_hit>> &rows, const std::vector<std::vector<int32_t>> &maps,
                Count count, Run run, sat_hit *hits, int32_t *ssemaps)
{
    size_t out = 0;
    for (int q = 0; q < nq; q++)
        merge_shards(rows, count(q), [&](int g) { return run(q, g); }, [&](int g, size_t row) {
            hits[out] = rows[(size_t)g][row];
            hits[out].entry += m->begin[(size_t)g];
            if (ssemaps) memcpy(ssemaps + out * SAT_MAXDIM, maps[(size_t)g].data() + row * SAT_MAXDIM, sizeof(int32_t) * SAT_MAXDIM);
            out++;
        });
}

// Stage 1 of the sharded best-k and refine calls: search(g) queued on every shard, then each shard's best c rows of every
// query (maps: and their maps) into cand[g] (cmaps[g]): c rows per query leave each GPU, the host merges ndev x c
// candidates.  got[g]: the rows per query shard g gave - query q's run there is run(q, g).
struct ShardRows {
    std::vector<std::vector<sat_hit>> cand;
    std::vector<std::vector<int32_t>> cmaps;
    std::vector<size_t> got;
    std::pair<size_t, size_t> run(int q, int g) const { return { (size_t)q * got[(size_t)g], (size_t)(q + 1) * got[(size_t)g] }; }
};
template <typename Search> int stage1(sat_multi *m, Search search, int c, bool maps, ShardRows &s)
{
    SAT_TRY(each_shard(m, search));
    const size_t rows = m->ctx[0]->queries.size() * (size_t)c;
    s.cand.resize((size_t)m->ndev);
    s.cmaps.resize((size_t)m->ndev);
    s.got.assign((size_t)m->ndev, 0);
    return each_shard(m, [&](int g) {
        s.cand[(size_t)g].resize(rows);
        if (maps) s.cmaps[(size_t)g].resize(rows * SAT_MAXDIM);
        const int r = sat_topk_hits(m->ctx[(size_t)g], c, s.cand[(size_t)g].data(), maps ? s.cmaps[(size_t)g].data() : nullptr);
        s.got[(size_t)g] = r < 0 ? 0 : (size_t)r;
        return r < 0 ? r : SAT_OK;
    });
}

// hit_row (sat_hitrow.hpp) without a fit, on the host, bit for bit: the same division, the truncation to an int and the
// clamp to the table's -128 .. 127 explained there, z and p from the functions that filled the device's table
sat_hit host_hit_row(int32_t entry, int32_t score, int n1, int n2)
{
    const double norm2 = sat_norm2(score, n1, n2);
    const int x = std::max(-128, std::min(127, (int)norm2));
    const double z = sat_z_gumbel_trunc((double)x);
    return { entry, score, norm2, z, sat_pv_gumbel(z) };
}

// bring `count` elements of every device's `src(g)` into block g of `dst` on device 0
template <typename T, typename Src>
int gather_to_device0(sat_multi *m, T *dst, size_t count, ncclDataType_t type, Src src)
{
    sat_ctx *root = m->ctx[0];
    if (m->use_rccl) {
        ncclResult_t r = g_rccl.GroupStart();
        bool ok = r == ncclSuccess;
        for (int g = 0; ok && g < m->ndev; g++) {
            if (hipSetDevice(m->devices[(size_t)g]) != hipSuccess) {       // (never leave the group open)
                (void)g_rccl.GroupEnd();
                return sat_fail(SAT_EDEVICE, "hipSetDevice(%d) failed inside the gather", m->devices[(size_t)g]);
            }
            r = g_rccl.Gather(src(g), dst, count, type, 0, m->comm[(size_t)g], m->ctx[(size_t)g]->stream);
            ok = r == ncclSuccess;
        }
        const ncclResult_t rend = g_rccl.GroupEnd();
        if (ok && rend == ncclSuccess) return SAT_OK;
        // RCCL refused the gather at run time: unless the caller insisted on it, take the peer-copy path from
        // here on (the searches are queued and their rows sit in each GPU's memory; nothing is lost)
        if (m->rccl_required)
            return rccl_fail(ok ? rend : r, ok ? "ncclGroupEnd" : "ncclGather");
        fprintf(stderr, "satabsearch: RCCL gather failed (%s); falling back to peer copies\n",
                g_rccl.GetErrorString ? g_rccl.GetErrorString(ok ? rend : r) : "RCCL error");
        sync_all(m);
        (void)hipGetLastError();
        m->use_rccl = false;
        const int rc = ensure_peer_events(m);
        if (rc != SAT_OK) return rc;
    }
    for (int g = 0; g < m->ndev; g++) {
        sat_ctx *c = m->ctx[(size_t)g];
        HIP_TRY(hipSetDevice(m->devices[(size_t)g]));
        HIP_TRY(hipMemcpyPeerAsync(dst + (size_t)g * count, m->devices[0], src(g), m->devices[(size_t)g], count * sizeof(T), c->stream));
        if (g > 0) {
            HIP_TRY(hipEventRecord(m->done[(size_t)g], c->stream));
            HIP_TRY(hipStreamWaitEvent(root->stream, m->done[(size_t)g], 0));
        }
    }
    return SAT_OK;
}

// the shard that holds entry `entry` of the database
int shard_of(const sat_multi *m, int entry) { return (int)(std::upper_bound(m->begin.begin(), m->begin.end(), entry) - m->begin.begin()) - 1; }

// A sharded pair call behind its own argument checks: the checks every one shares (a database, a query batch, maxstart,
// the list and its index ranges), every pair filed with the shard that holds its entry, under the entry's index there;
// launch(shard context, queries, entries, pairs) queued on every GPU, then collect(shard context, pairs, queries, where)
// for each shard: row i of a shard goes to row where[i] of the caller's arrays, the one its pair came from.
template <typename Launch, typename Collect>
int sharded_pairs(sat_multi *m, int maxstart, int npairs, const int32_t *query, const int32_t *entry, double *wall_ms, Launch launch,
                  Collect collect)
{
    SAT_TRY(check_uploaded(m));
    if (m->ctx[0]->queries.empty()) return sat_fail(SAT_ESTATE, "no query set");
    if (maxstart < 1) return sat_fail(SAT_EINVAL, "maxstart must be >= 1 (got %d)", maxstart);
    int rc = sat_check_pairs((int)m->ctx[0]->queries.size(), m->n_entries, query, entry, npairs);
    if (rc != SAT_OK) return rc;
    const Stopwatch clock;
    std::vector<std::vector<int32_t>> pq((size_t)m->ndev), pe((size_t)m->ndev), where((size_t)m->ndev);
    for (int p = 0; p < npairs; p++) {
        const int g = shard_of(m, entry[p]);
        pq[(size_t)g].push_back(query[p]);
        pe[(size_t)g].push_back(entry[p] - m->begin[(size_t)g]);
        where[(size_t)g].push_back(p);
    }
    rc = each_shard(m, [&](int g) { return launch(m->ctx[(size_t)g], pq[(size_t)g].data(), pe[(size_t)g].data(), (int)pq[(size_t)g].size()); });
    if (rc != SAT_OK) return rc;
    rc = each_shard(m, [&](int g) { return collect(m->ctx[(size_t)g], (int)pq[(size_t)g].size(), pq[(size_t)g].data(), where[(size_t)g].data()); });
    if (rc != SAT_OK) return rc;
    clock.stop(wall_ms);
    return SAT_OK;
}

}  // namespace

extern "C" {

sat_multi *sat_multi_create(int ndev, const int *devices, uint64_t seed)
{
    const int visible = sat_device_count();
    if (ndev <= 0) ndev = visible;
    // an explicit device list may name a device more than once (several shards on one GPU: how the
    // multi-shard path is exercised on a one-GPU box; RCCL refuses duplicates, peer copies do not)
    bool listed_ok = devices != nullptr;
    for (int g = 0; listed_ok && g < ndev; g++) listed_ok = devices[g] >= 0 && devices[g] < visible;
    if (visible <= 0 || (devices ? !listed_ok : ndev > visible)) {
        sat_fail(SAT_ENODEVICE, "%d GPUs asked for, %d visible (this library has no CPU path)", ndev, visible);
        return nullptr;
    }
    sat_multi *m = new (std::nothrow) sat_multi();
    if (!m) {
        sat_fail(SAT_ENOMEM, "out of host memory");
        return nullptr;
    }
    m->ndev = ndev;
    for (int g = 0; g < ndev; g++) m->devices.push_back(devices ? devices[g] : g);
    for (int g = 0; g < ndev; g++) {
        sat_ctx *c = sat_ctx_create(m->devices[(size_t)g], seed);
        if (!c) {
            sat_multi_destroy(m);
            return nullptr;
        }
        m->ctx.push_back(c);
    }
    m->done.assign((size_t)ndev, nullptr);
    const char *how = getenv("SAT_MULTI_GATHER");
    const bool want_peer = how && !strcmp(how, "peer");
    const bool force_rccl = how && !strcmp(how, "rccl");            // also with one GPU (tests)
    m->force_gather = want_peer || force_rccl;
    bool duplicates = false;
    for (int g = 0; g < ndev; g++)
        for (int h = 0; h < g; h++) duplicates = duplicates || m->devices[(size_t)g] == m->devices[(size_t)h];
    if (!want_peer && !duplicates && (ndev > 1 || force_rccl) && g_rccl.load()) {
        m->comm.assign((size_t)ndev, nullptr);
        if (g_rccl.CommInitAll(m->comm.data(), ndev, m->devices.data()) == ncclSuccess) m->use_rccl = true;
        else m->comm.clear();
    }
    if (force_rccl && !m->use_rccl) {
        sat_fail(SAT_EDEVICE, "SAT_MULTI_GATHER=rccl but librccl could not be loaded / initialised");
        sat_multi_destroy(m);
        return nullptr;
    }
    m->rccl_required = force_rccl;
    if (!m->use_rccl && ensure_peer_events(m) != SAT_OK) {
        sat_multi_destroy(m);
        return nullptr;
    }
    return m;
}

void sat_multi_destroy(sat_multi *m)
{
    if (!m) return;
    for (size_t g = 0; g < m->comm.size(); g++)
        if (m->comm[g]) (void)g_rccl.CommDestroy(m->comm[g]);
    if (!m->devices.empty()) (void)hipSetDevice(m->devices[0]);
    m->d_all_scores.reset();
    m->d_all_maps.reset();
    if (m->h_stage) (void)hipHostFree(m->h_stage);
    for (size_t g = 0; g < m->done.size(); g++)
        if (m->done[g]) (void)hipEventDestroy(m->done[g]);
    for (sat_ctx *c : m->ctx) sat_ctx_destroy(c);
    delete m;
}

int sat_multi_device_count(const sat_multi *m) { return m ? m->ndev : 0; }

const char *sat_multi_gather_kind(const sat_multi *m)
{
    if (!m) return "";
    if (m->ndev == 1 && !m->force_gather) return "none";
    return m->use_rccl ? "rccl" : "peer";
}

int sat_multi_db_upload_packed(sat_multi *m, int n_entries, const int32_t *orders, const int64_t *cell_off,
                               const uint8_t *tab_tri, const float *dist_tri)
{
    SAT_TRY(sat_check_context(m));
    if (n_entries < m->ndev) return sat_fail(SAT_EINVAL, "%d entries cannot be cut into %d shards", n_entries, m->ndev);
    if (!orders || !cell_off || !tab_tri || !dist_tri) return sat_fail(SAT_EINVAL, "null array");
    // a shard is uploaded as a WINDOW of the packed arrays (from its first entry's first cell): the entries must lie
    // in file order, one after the other without overlap - what every reader here produces
    for (int e = 0; e + 1 < n_entries; e++) {
        const int64_t n = orders[e];
        if (n < 1 || n > SAT_MAXDIM) return sat_fail(SAT_EINVAL, "entry %d: order %lld outside 1..%d", e, (long long)n, SAT_MAXDIM);
        if (cell_off[e] < 0 || cell_off[e + 1] < cell_off[e] + n * (n + 1) / 2)
            return sat_fail(SAT_EINVAL, "entry %d: cell offsets must ascend in file order without overlap for a sharded upload "
                            "(entry %d starts at cell %lld, entry %d at %lld)", e + 1, e, (long long)cell_off[e], e + 1, (long long)cell_off[e + 1]);
    }
    m->begin.assign((size_t)m->ndev + 1, 0);
    if (sat_shard_cuts(n_entries, orders, m->ndev, m->begin.data()) != 0) return sat_fail(SAT_EINVAL, "bad database");
    m->n_entries = n_entries;
    m->pad_rows = 0;
    std::vector<int64_t> ordinal((size_t)n_entries);
    for (int e = 0; e < n_entries; e++) ordinal[(size_t)e] = e;
    // every GPU has its own link to the host: the shards go up concurrently, one host thread per GPU
    std::vector<int> rcs((size_t)m->ndev, SAT_OK);
    std::vector<std::string> errs((size_t)m->ndev);
    auto upload_shard = [&](int g) {
        const int b = m->begin[(size_t)g], n = m->begin[(size_t)g + 1] - b;
        // a shard is a window of the packed arrays: rebase its cell offsets to the window
        std::vector<int64_t> off((size_t)n);
        for (int e = 0; e < n; e++) off[(size_t)e] = cell_off[b + e] - cell_off[b];
        rcs[(size_t)g] = sat_db_upload_packed(m->ctx[(size_t)g], n, orders + b, off.data(), tab_tri + cell_off[b],
                                              dist_tri + cell_off[b], ordinal.data() + b);
        if (rcs[(size_t)g] != SAT_OK) errs[(size_t)g] = sat_last_error();      // the message is per thread
    };
    {
        std::vector<std::thread> pool;
        for (int g = 1; g < m->ndev; g++) pool.emplace_back(upload_shard, g);
        upload_shard(0);
        for (auto &th : pool) th.join();
    }
    for (int g = 0; g < m->ndev; g++) {
        if (rcs[(size_t)g] != SAT_OK) {
            // entry numbers in the message are relative to the shard: say which
            return sat_fail(rcs[(size_t)g], "shard %d (entries from %d): %s", g, m->begin[(size_t)g], errs[(size_t)g].c_str());
        }
        const int n = m->begin[(size_t)g + 1] - m->begin[(size_t)g];
        if (n > m->pad_rows) m->pad_rows = n;
    }
    for (int g = 0; g < m->ndev; g++) m->ctx[(size_t)g]->min_rows = m->pad_rows;     // result buffers hold a padded shard
    return SAT_OK;
}

int sat_multi_shards(const sat_multi *m, int32_t *begin)
{
    if (!m || !begin) return sat_fail(SAT_EINVAL, "null argument");
    SAT_TRY(check_uploaded(m));
    for (int g = 0; g <= m->ndev; g++) begin[g] = m->begin[(size_t)g];
    return SAT_OK;
}

int sat_multi_queries_set(sat_multi *m, int n_queries, const int32_t *n1s, const uint8_t *qtabs, const float *qdmats,
                          int pitch, const uint8_t *qssetypes, uint32_t first_query_ordinal)
{
    SAT_TRY(sat_check_context(m));
    for (int g = 0; g < m->ndev; g++) {
        int rc = sat_queries_set(m->ctx[(size_t)g], n_queries, n1s, qtabs, qdmats, pitch, qssetypes, first_query_ordinal);
        if (rc != SAT_OK) return rc;
    }
    return SAT_OK;
}

// sat_multi_queries_from_db (sse_begin null) and sat_multi_queries_from_db_sses: the lists are checked against the order
// of each query's entry on the shard that holds it, and every shard is sent the lists of its own queries alone - the
// others' ranges are empty there, their room in the blob follows from the code
static int multi_queries_from_db(sat_multi *m, int n_queries, const int32_t *entry, const int32_t *sse_begin, const uint8_t *sse,
                                 uint32_t first_query_ordinal)
{
    // every query goes to the shard that holds its entry, under the entry's index there; the other shards learn its
    // size class only (sat_qfromdb_set)
    std::vector<int> owner((size_t)n_queries);
    std::vector<int32_t> n1s((size_t)n_queries);
    std::vector<std::vector<int32_t>> code((size_t)m->ndev, std::vector<int32_t>((size_t)n_queries));
    std::vector<std::vector<int32_t>> begin((size_t)(sse_begin ? m->ndev : 0), std::vector<int32_t>((size_t)n_queries + 1, 0));
    std::vector<std::vector<uint8_t>> lists((size_t)(sse_begin ? m->ndev : 0));
    for (int q = 0; q < n_queries; q++) {
        if (entry[q] < 0 || entry[q] >= m->n_entries)
            return sat_fail(SAT_EINVAL, "query %d: entry %d outside 0..%d", q, entry[q], m->n_entries - 1);
        const int g = shard_of(m, entry[q]);
        const int32_t local = entry[q] - m->begin[(size_t)g];
        owner[(size_t)q] = g;
        n1s[(size_t)q] = m->ctx[(size_t)g]->h_orders[(size_t)local];
        if (sse_begin) {
            const int len = sse_begin[q + 1] - sse_begin[q];
            SAT_TRY(sat_qfromdb_check_list(q, entry[q], n1s[(size_t)q], sse + sse_begin[q], len));
            if (len > 0) n1s[(size_t)q] = len;
            lists[(size_t)g].insert(lists[(size_t)g].end(), sse + sse_begin[q], sse + sse_begin[q + 1]);
            for (int h = 0; h < m->ndev; h++) begin[(size_t)h][(size_t)q + 1] = (int32_t)lists[(size_t)h].size();
        }
        for (int h = 0; h < m->ndev; h++) code[(size_t)h][(size_t)q] = h == g ? local : -query_n1p(n1s[(size_t)q]);
    }
    // each shard expands its own entries (and has waited for its stream when that returns) ...
    for (int g = 0; g < m->ndev; g++) {
        const int rc = sat_qfromdb_set(m->ctx[(size_t)g], n_queries, code[(size_t)g].data(), n1s.data(),
                                       sse_begin ? begin[(size_t)g].data() : nullptr, sse_begin ? lists[(size_t)g].data() : nullptr,
                                       first_query_ordinal);
        if (rc != SAT_OK) return rc;
    }
    // ... and sends every run of queries it owns to the other shards' blobs (the same offsets on every shard), device to
    // device: a peer copy between GPUs, a plain copy where the list names one GPU twice
    for (int q0 = 0; q0 < n_queries;) {
        const int g = owner[(size_t)q0];
        int q1 = q0 + 1;
        while (q1 < n_queries && owner[(size_t)q1] == g) q1++;
        uint8_t *src, *last, *dst;
        size_t bytes, last_bytes;
        sat_qfromdb_segment(m->ctx[(size_t)g], q0, &src, &bytes);
        sat_qfromdb_segment(m->ctx[(size_t)g], q1 - 1, &last, &last_bytes);
        bytes = (size_t)(last - src) + last_bytes;
        HIP_TRY(hipSetDevice(m->devices[(size_t)g]));
        for (int h = 0; h < m->ndev; h++) {
            if (h == g) continue;
            sat_qfromdb_segment(m->ctx[(size_t)h], q0, &dst, &last_bytes);
            if (m->devices[(size_t)h] == m->devices[(size_t)g])
                HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, m->ctx[(size_t)g]->stream));
            else
                HIP_TRY(hipMemcpyPeerAsync(dst, m->devices[(size_t)h], src, m->devices[(size_t)g], bytes, m->ctx[(size_t)g]->stream));
        }
        q0 = q1;
    }
    for (int g = 0; g < m->ndev; g++) {
        HIP_TRY(hipSetDevice(m->devices[(size_t)g]));
        HIP_TRY(hipStreamSynchronize(m->ctx[(size_t)g]->stream));
    }
    return SAT_OK;
}

sat_ctx *sat_debug_multi_ctx(sat_multi *m, int shard) { return m && shard >= 0 && shard < m->ndev ? m->ctx[(size_t)shard] : nullptr; }

int sat_multi_queries_from_db(sat_multi *m, int n_queries, const int32_t *entry, uint32_t first_query_ordinal)
{
    SAT_TRY(sat_check_context(m));
    if (n_queries < 1 || !entry) return sat_fail(SAT_EINVAL, "bad query batch (n_queries=%d)", n_queries);
    SAT_TRY(check_uploaded(m));
    return multi_queries_from_db(m, n_queries, entry, nullptr, nullptr, first_query_ordinal);
}

int sat_multi_queries_from_db_sses(sat_multi *m, int n_queries, const int32_t *entry, const int32_t *sse_begin, const uint8_t *sse,
                                   uint32_t first_query_ordinal)
{
    SAT_TRY(sat_check_context(m));
    if (n_queries < 1 || !entry) return sat_fail(SAT_EINVAL, "bad query batch (n_queries=%d)", n_queries);
    SAT_TRY(sat_qfromdb_check_offsets(n_queries, sse_begin, sse));
    SAT_TRY(check_uploaded(m));
    return multi_queries_from_db(m, n_queries, entry, sse_begin, sse, first_query_ordinal);
}

int sat_multi_search(sat_multi *m, int lorder, int lsoln, int maxstart, int32_t *scores, int32_t *ssemaps, double *wall_ms)
{
    SAT_TRY(sat_check_context(m));
    if (!scores) return sat_fail(SAT_EINVAL, "scores buffer is null");
    if (lsoln && !ssemaps) return sat_fail(SAT_EINVAL, "lsoln set but ssemaps buffer is null");
    SAT_TRY(check_uploaded(m));
    const Stopwatch clock;
    // (an error below waits for the searches already queued on the other GPUs before it is returned)
    int rc = search_shards(m, lorder, lsoln, maxstart);
    if (rc != SAT_OK) return rc;
    sat_ctx *root = m->ctx[0];
    const size_t nq = root->queries.size(), N = (size_t)m->n_entries, pad = (size_t)m->pad_rows;
    if (m->ndev == 1 && !m->force_gather) {
        rc = sat_results(root, lsoln, scores, ssemaps);
        clock.stop(wall_ms);
        return rc;
    }
    // ---- one gather of the (padded) per-shard rows to device 0, one copy to the host
    size_t map_bytes_per_row = 0;
    for (const auto &q : root->queries) map_bytes_per_row += (size_t)q.n1;
    const size_t score_count = nq * pad, map_count = pad * map_bytes_per_row;
    if (hipSetDevice(m->devices[0]) != hipSuccess) return bail(m, sat_fail(SAT_EDEVICE, "hipSetDevice failed"));
    if ((rc = m->d_all_scores.grow(score_count * (size_t)m->ndev)) != SAT_OK) return bail(m, rc);
    if (lsoln && (rc = m->d_all_maps.grow(map_count * (size_t)m->ndev)) != SAT_OK) return bail(m, rc);
    const size_t stage_bytes = score_count * (size_t)m->ndev * sizeof(int32_t) + (lsoln ? map_count * (size_t)m->ndev : 0);
    if ((rc = grow_stage(m, stage_bytes)) != SAT_OK) return bail(m, rc);
    if ((rc = gather_to_device0(m, m->d_all_scores.get(), score_count, ncclInt32,
                                [&](int g) { return (const int32_t *)m->ctx[(size_t)g]->d_scores.get(); })) != SAT_OK)
        return bail(m, rc);
    if (lsoln && (rc = gather_to_device0(m, m->d_all_maps.get(), map_count, ncclInt8,
                                         [&](int g) { return (const int8_t *)m->ctx[(size_t)g]->d_ssemaps.get(); })) != SAT_OK)
        return bail(m, rc);
    int32_t *h_scores = static_cast<int32_t *>(m->h_stage);
    int8_t *h_maps = reinterpret_cast<int8_t *>(h_scores + score_count * (size_t)m->ndev);
    auto to_host = [&]() -> int {
        HIP_TRY(hipSetDevice(m->devices[0]));
        HIP_TRY(hipMemcpyAsync(h_scores, m->d_all_scores.get(), score_count * (size_t)m->ndev * sizeof(int32_t), hipMemcpyDeviceToHost, root->stream));
        if (lsoln) HIP_TRY(hipMemcpyAsync(h_maps, m->d_all_maps.get(), map_count * (size_t)m->ndev, hipMemcpyDeviceToHost, root->stream));
        HIP_TRY(hipStreamSynchronize(root->stream));
        for (int g = 1; g < m->ndev; g++) {                            // the senders' streams are done too
            HIP_TRY(hipSetDevice(m->devices[(size_t)g]));
            HIP_TRY(hipStreamSynchronize(m->ctx[(size_t)g]->stream));
        }
        return SAT_OK;
    };
    if ((rc = to_host()) != SAT_OK) return bail(m, rc);
    m->d2h_bytes += stage_bytes;
    // rows of shard g: scores [nq][n_g] at block g; maps: query q's [n_g][n1_q] block after those of queries 0..q-1
    for (int g = 0; g < m->ndev; g++) {
        const size_t b = (size_t)m->begin[(size_t)g], n = (size_t)m->begin[(size_t)g + 1] - b;
        const int32_t *src = h_scores + (size_t)g * score_count;
        for (size_t q = 0; q < nq; q++) memcpy(scores + q * N + b, src + q * n, n * sizeof(int32_t));
        if (lsoln) {
            const int8_t *msrc = h_maps + (size_t)g * map_count;
            size_t qoff = 0;
            for (size_t q = 0; q < nq; q++) {
                const size_t n1 = (size_t)root->queries[q].n1;
                int32_t *out = ssemaps + (q * N + b) * SAT_MAXDIM;
                for (size_t e = 0; e < n; e++) {
                    for (size_t i = 0; i < n1; i++) out[e * SAT_MAXDIM + i] = msrc[qoff + e * n1 + i];
                    for (size_t i = n1; i < SAT_MAXDIM; i++) out[e * SAT_MAXDIM + i] = -1;
                }
                qoff += n * n1;
            }
        }
    }
    clock.stop(wall_ms);
    return SAT_OK;
}

int sat_multi_search_topk(sat_multi *m, int lorder, int lsoln, int maxstart, int k, sat_hit *hits, int32_t *ssemaps, double *wall_ms)
{
    SAT_TRY(sat_check_context(m));
    SAT_TRY(sat_check_topk(hits != nullptr, k));
    SAT_TRY(check_uploaded(m));
    const Stopwatch clock;
    if (k > m->n_entries) k = m->n_entries;
    ShardRows s;
    SAT_TRY(stage1(m, [&](int g) { return sat_search_async(m->ctx[(size_t)g], lorder, lsoln, maxstart); }, k, ssemaps != nullptr, s));
    merge_rows(m, (int)m->ctx[0]->queries.size(), s.cand, s.cmaps, [&](int) { return (size_t)k; },
               [&](int q, int g) { return s.run(q, g); }, hits, ssemaps);
    clock.stop(wall_ms);
    return k;
}

int sat_multi_search_matches(sat_multi *m, int lorder, int maxstart, int max_matches, int32_t *counts,
                             int32_t *scores, int32_t *restarts, int32_t *ssemaps, double *wall_ms)
{
    SAT_TRY(sat_check_context(m));
    if (!counts || !scores || !restarts) return sat_fail(SAT_EINVAL, "counts / scores / restarts buffer is null");
    SAT_TRY(check_uploaded(m));
    const Stopwatch clock;
    // both passes queued on every GPU, then each shard's rows copied to its place in database order
    SAT_TRY(each_shard(m, [&](int g) { return sat_matches_launch(m->ctx[(size_t)g], lorder, maxstart, max_matches, ssemaps != nullptr); }));
    SAT_TRY(each_shard(m, [&](int g) {
        return sat_matches_collect(m->ctx[(size_t)g], max_matches, counts, scores, restarts, ssemaps, (size_t)m->n_entries,
                                   (size_t)m->begin[(size_t)g]);
    }));
    clock.stop(wall_ms);
    return SAT_OK;
}

int sat_multi_search_pairs_matches(sat_multi *m, int lorder, int maxstart, int max_matches, int npairs, const int32_t *query,
                                   const int32_t *entry, int32_t *counts, int32_t *scores, int32_t *restarts, int32_t *ssemaps,
                                   double *wall_ms)
{
    SAT_TRY(sat_check_context(m));
    if (npairs > 0 && (!counts || !scores || !restarts)) return sat_fail(SAT_EINVAL, "counts / scores / restarts buffer is null");
    if (max_matches < 1 || max_matches > SAT_MAX_MATCHES)
        return sat_fail(SAT_EINVAL, "max_matches must be 1..%d (got %d)", SAT_MAX_MATCHES, max_matches);
    return sharded_pairs(m, maxstart, npairs, query, entry, wall_ms,
        [&](sat_ctx *c, const int32_t *q, const int32_t *e, int np) {
            return sat_pair_matches_launch(c, lorder, maxstart, max_matches, ssemaps != nullptr, q, e, np);
        },
        [&](sat_ctx *c, int np, const int32_t *q, const int32_t *where) {
            return sat_pair_matches_collect(c, max_matches, np, counts, scores, restarts, ssemaps, q, where);
        });
}

int sat_multi_search_pairs_polish(sat_multi *m, int lorder, int maxstart, int tops, int npairs, const int32_t *query,
                                  const int32_t *entry, int32_t *scores, int32_t *base_scores, int32_t *restarts, int32_t *moves,
                                  int32_t *ssemaps, double *wall_ms)
{
    SAT_TRY(sat_check_context(m));
    if (npairs > 0 && !scores) return sat_fail(SAT_EINVAL, "scores buffer is null");
    SAT_TRY(sat_check_tops(tops));
    return sharded_pairs(m, maxstart, npairs, query, entry, wall_ms,
        [&](sat_ctx *c, const int32_t *q, const int32_t *e, int np) {
            return sat_pair_matches_launch(c, lorder, maxstart, tops, true, q, e, np, PairMode::Polish);
        },
        [&](sat_ctx *c, int np, const int32_t *q, const int32_t *where) {
            return sat_polish_collect(c, np, scores, base_scores, restarts, moves, ssemaps, q, where);
        });
}

}  // extern "C"

// sat_multi_search_refine (tops = 0) and sat_multi_search_refine_polish (tops = maps polished per candidate)
static int multi_refine(sat_multi *m, int lorder, int lsoln, int maxstart, int candidates, int refine_maxstart, int tops, int k,
                        sat_hit *hits, int32_t *ssemaps, int32_t *first_scores, int32_t *base_scores, double *wall_ms,
                        double *stage2_ms)
{
    SAT_TRY(sat_check_refine(m, hits, k, candidates, refine_maxstart));
    SAT_TRY(check_uploaded(m));
    const Stopwatch clock;
    // stage 1 on every shard, each ranking its own best C
    // (a plain search whatever sat_polish_all_set says: the mode is for whole-database searches, not for a refine's stage 1)
    const int c = candidates < m->n_entries ? candidates : m->n_entries;
    if (k > c) k = c;
    const int nq = (int)m->ctx[0]->queries.size();
    ShardRows s;
    SAT_TRY(stage1(m, [&](int g) { return launch_search(m->ctx[(size_t)g], lorder, 0, maxstart, m->ctx[(size_t)g]->stream); }, c, false, s));
    // the global best C of every query, filed by shard as pairs
    struct Cand { int g, local, first, second, base; };
    std::vector<std::vector<Cand>> per_q((size_t)nq);
    std::vector<std::vector<int32_t>> pq((size_t)m->ndev), pe((size_t)m->ndev);
    std::vector<std::vector<std::pair<int, int>>> slot((size_t)m->ndev);     // (query, index in per_q) of each pair
    for (int q = 0; q < nq; q++)
        merge_shards(s.cand, (size_t)c, [&](int g) { return s.run(q, g); },
                     [&](int g, size_t row) {
                         const sat_hit &h = s.cand[(size_t)g][row];
                         pq[(size_t)g].push_back(q);
                         pe[(size_t)g].push_back(h.entry);
                         slot[(size_t)g].push_back({ q, (int)per_q[(size_t)q].size() });
                         per_q[(size_t)q].push_back({ g, h.entry, h.score, 0, 0 });
                     });
    // stage 2: every shard re-scores its candidates (queued on all, then collected)
    const Stopwatch clock2;
    const bool maps = lsoln && ssemaps;
    SAT_TRY(each_shard(m, [&](int g) {
        if (tops)
            return sat_pair_matches_launch(m->ctx[(size_t)g], lorder, refine_maxstart, tops, true, pq[(size_t)g].data(),
                                           pe[(size_t)g].data(), (int)pq[(size_t)g].size(), PairMode::Polish);
        return sat_pairs_launch(m->ctx[(size_t)g], lorder, refine_maxstart, maps, pq[(size_t)g].data(), pe[(size_t)g].data(),
                                (int)pq[(size_t)g].size());
    }));
    std::vector<std::vector<int32_t>> cmaps((size_t)nq);
    if (maps)
        for (int q = 0; q < nq; q++) cmaps[(size_t)q].resize(per_q[(size_t)q].size() * SAT_MAXDIM);
    SAT_TRY(each_shard(m, [&](int g) {
        const size_t np = pq[(size_t)g].size();
        std::vector<int32_t> sc(np), bs(tops ? np : 0), mp(maps ? np * SAT_MAXDIM : 0);
        const int r = tops ? sat_polish_collect(m->ctx[(size_t)g], (int)np, sc.data(), bs.data(), nullptr, nullptr,
                                                maps ? mp.data() : nullptr, pq[(size_t)g].data())
                           : sat_pairs_collect(m->ctx[(size_t)g], (int)np, sc.data(), maps ? mp.data() : nullptr, pq[(size_t)g].data());
        if (r != SAT_OK) return r;
        for (size_t p = 0; p < np; p++) {
            const auto &sl = slot[(size_t)g][p];
            per_q[(size_t)sl.first][(size_t)sl.second].second = sc[p];
            if (tops) per_q[(size_t)sl.first][(size_t)sl.second].base = bs[p];
            if (maps) memcpy(cmaps[(size_t)sl.first].data() + (size_t)sl.second * SAT_MAXDIM, mp.data() + p * SAT_MAXDIM, sizeof(int32_t) * SAT_MAXDIM);
        }
        return SAT_OK;
    }));
    clock2.stop(stage2_ms);
    // the final rows: stage-2 score descending, ties in database order; statistics as the device table holds them
    for (int q = 0; q < nq; q++) {
        auto &v = per_q[(size_t)q];
        std::vector<int> order(v.size());
        for (size_t i = 0; i < v.size(); i++) order[i] = (int)i;
        auto gidx = [&](const Cand &x) { return m->begin[(size_t)x.g] + x.local; };
        std::sort(order.begin(), order.end(), [&](int a, int b) {
            if (v[(size_t)a].second != v[(size_t)b].second) return v[(size_t)a].second > v[(size_t)b].second;
            return gidx(v[(size_t)a]) < gidx(v[(size_t)b]);
        });
        const int n1 = m->ctx[0]->queries[(size_t)q].n1;
        for (int r = 0; r < k; r++) {
            const Cand &x = v[(size_t)order[(size_t)r]];
            hits[(size_t)q * k + r] = host_hit_row(gidx(x), x.second, n1, m->ctx[(size_t)x.g]->h_orders[(size_t)x.local]);
            if (first_scores) first_scores[(size_t)q * k + r] = x.first;
            if (base_scores) base_scores[(size_t)q * k + r] = x.base;
            if (maps) memcpy(ssemaps + ((size_t)q * k + r) * SAT_MAXDIM, cmaps[(size_t)q].data() + (size_t)order[(size_t)r] * SAT_MAXDIM,
                             sizeof(int32_t) * SAT_MAXDIM);
        }
    }
    clock.stop(wall_ms);
    return k;
}

extern "C" {

int sat_multi_search_refine(sat_multi *m, int lorder, int lsoln, int maxstart, int candidates, int refine_maxstart, int k,
                            sat_hit *hits, int32_t *ssemaps, int32_t *first_scores, double *wall_ms, double *stage2_ms)
{
    return multi_refine(m, lorder, lsoln, maxstart, candidates, refine_maxstart, 0, k, hits, ssemaps, first_scores, nullptr, wall_ms,
                        stage2_ms);
}

int sat_multi_search_refine_polish(sat_multi *m, int lorder, int lsoln, int maxstart, int candidates, int refine_maxstart, int tops,
                                   int k, sat_hit *hits, int32_t *ssemaps, int32_t *first_scores, int32_t *base_scores,
                                   double *wall_ms)
{
    SAT_TRY(sat_check_tops(tops));
    return multi_refine(m, lorder, lsoln, maxstart, candidates, refine_maxstart, tops, k, hits, ssemaps, first_scores, base_scores,
                        wall_ms, nullptr);
}

int sat_multi_hits_cutoff(sat_multi *m, double max_pvalue, int max_rows, int32_t *counts, int capacity, sat_hit *hits,
                          int32_t *ssemaps)
{
    SAT_TRY(check_multi(m));
    if (!counts) return sat_fail(SAT_EINVAL, "counts buffer is null");
    SAT_TRY(sat_check_pvalue(max_pvalue));
    const int nq = (int)m->ctx[0]->queries.size();
    // every shard counts its qualifying rows; a query's rows are the sum, cut to max_rows
    std::vector<std::vector<int32_t>> raw((size_t)m->ndev, std::vector<int32_t>((size_t)nq));
    for (int g = 0; g < m->ndev; g++) SAT_TRY(sat_cutoff_count(m->ctx[(size_t)g], max_pvalue, ssemaps != nullptr, raw[(size_t)g].data()));
    size_t total = 0;
    for (int q = 0; q < nq; q++) {
        long long c = 0;
        for (int g = 0; g < m->ndev; g++) c += raw[(size_t)g][(size_t)q];
        counts[q] = sat_row_cap(c > INT_MAX ? INT_MAX : (int32_t)c, max_rows);
        total += (size_t)counts[q];
    }
    if (total > (size_t)INT_MAX) return sat_fail(SAT_EINVAL, "%zu rows qualify: more than one call can return", total);
    if (!hits || (long long)total > (long long)capacity) return (int)total;
    // each shard's rows (max_rows per query at most), merged per query: score descending, ties in database order
    std::vector<std::vector<sat_hit>> rows((size_t)m->ndev);
    std::vector<std::vector<int32_t>> rmaps((size_t)m->ndev);
    std::vector<std::vector<size_t>> off((size_t)m->ndev, std::vector<size_t>((size_t)nq + 1, 0));
    for (int g = 0; g < m->ndev; g++) {
        for (int q = 0; q < nq; q++) off[(size_t)g][(size_t)q + 1] = off[(size_t)g][(size_t)q] + (size_t)sat_row_cap(raw[(size_t)g][(size_t)q], max_rows);
        rows[(size_t)g].resize(off[(size_t)g][(size_t)nq]);
        if (ssemaps) rmaps[(size_t)g].resize(off[(size_t)g][(size_t)nq] * SAT_MAXDIM);
        SAT_TRY(sat_cutoff_rows(m->ctx[(size_t)g], max_pvalue, max_rows, raw[(size_t)g].data(), rows[(size_t)g].data(),
                                ssemaps ? rmaps[(size_t)g].data() : nullptr));
    }
    merge_rows(m, nq, rows, rmaps, [&](int q) { return (size_t)counts[q]; },
               [&](int q, int g) { return std::make_pair(off[(size_t)g][(size_t)q], off[(size_t)g][(size_t)q + 1]); }, hits, ssemaps);
    return (int)total;
}

int sat_multi_search_cutoff(sat_multi *m, int lorder, int lsoln, int maxstart, double max_pvalue, int max_rows, int32_t *counts,
                            int capacity, sat_hit *hits, int32_t *ssemaps, double *wall_ms)
{
    SAT_TRY(check_multi(m));
    if (!counts) return sat_fail(SAT_EINVAL, "counts buffer is null");
    SAT_TRY(sat_check_pvalue(max_pvalue));
    const Stopwatch clock;
    SAT_TRY(search_shards(m, lorder, lsoln, maxstart));
    const int r = sat_multi_hits_cutoff(m, max_pvalue, max_rows, counts, capacity, hits, ssemaps);
    if (r < 0) return bail(m, r);
    clock.stop(wall_ms);
    return r;
}

int sat_multi_score_histogram(sat_multi *m, uint32_t *counts, int32_t *below)
{
    SAT_TRY(check_multi(m));
    if (!counts || !below) return sat_fail(SAT_EINVAL, "histogram buffer is null");
    const size_t nq = m->ctx[0]->queries.size();
    // integer counts add up across the shards, in any order
    std::vector<uint32_t> c(nq * SAT_STAT_BINS);
    std::vector<int32_t> b(nq);
    std::fill(counts, counts + nq * SAT_STAT_BINS, 0u);
    std::fill(below, below + nq, 0);
    for (int g = 0; g < m->ndev; g++) {
        SAT_TRY(sat_score_histogram(m->ctx[(size_t)g], c.data(), b.data()));
        for (size_t i = 0; i < c.size(); i++) counts[i] += c[i];
        for (size_t q = 0; q < nq; q++) below[q] += b[q];
    }
    return SAT_OK;
}

int sat_multi_polish_all_set(sat_multi *m, int tops)
{
    SAT_TRY(sat_check_context(m));
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_polish_all_set(c, tops));
    return SAT_OK;
}

int sat_multi_stats_set(sat_multi *m, const sat_fit *fits)
{
    SAT_TRY(check_multi(m));
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_stats_set(c, fits));
    return SAT_OK;
}

int sat_multi_search_fit(sat_multi *m, int lorder, int lsoln, int maxstart, double censor, sat_fit *fits, double *wall_ms)
{
    SAT_TRY(check_multi(m));
    SAT_TRY(sat_check_censor(censor));
    const Stopwatch clock;
    SAT_TRY(search_shards(m, lorder, lsoln, maxstart));
    // no gather: each shard's scores stay where they are, only the histograms cross to the host
    const int rc = sat_fit_queries(m->ctx[0]->queries.size(), censor, fits,
                                   [&](uint32_t *counts, int32_t *below) { return sat_multi_score_histogram(m, counts, below); },
                                   [&](const sat_fit *fit) { return sat_multi_stats_set(m, fit); });
    if (rc != SAT_OK) return bail(m, rc);
    clock.stop(wall_ms);
    return SAT_OK;
}

int sat_multi_search_only(sat_multi *m, int lorder, int lsoln, int maxstart, double *wall_ms)
{
    SAT_TRY(check_multi(m));
    const Stopwatch clock;
    SAT_TRY(search_shards(m, lorder, lsoln, maxstart));
    // no gather: each shard's scores stay where they are (sat_sync also reports a polished row that did not finish)
    SAT_TRY(each_shard(m, [&](int g) { return sat_sync(m->ctx[(size_t)g]); }));
    clock.stop(wall_ms);
    return SAT_OK;
}

int sat_multi_search_exact(sat_multi *m, int lorder, int maxstart, unsigned long long max_nodes, double *wall_ms)
{
    SAT_TRY(sat_check_context(m));
    if (m->begin.empty()) return sat_fail(SAT_EINVAL, "exact search: no database uploaded");
    // the refusals of sat_search_exact, made for all shards before the first one works
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_exact_check(c, maxstart, max_nodes));
    const Stopwatch clock;
    SAT_TRY(each_shard(m, [&](int g) { return sat_exact_launch(m->ctx[(size_t)g], lorder, maxstart, max_nodes); }));
    // no gather: each shard's rows stay where they are
    SAT_TRY(each_shard(m, [&](int g) { return sat_sync(m->ctx[(size_t)g]); }));
    clock.stop(wall_ms);
    return SAT_OK;
}

int sat_multi_exact_results(sat_multi *m, int32_t *scores, int32_t *ssemaps, int32_t *base_scores, uint8_t *unproven, uint32_t *nodes)
{
    SAT_TRY(sat_check_context(m));
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_exact_check_state(c));
    // each shard's [nq][its entries] rows into the columns of its entries
    const size_t nq = m->ctx[0]->queries.size(), total = (size_t)m->n_entries;
    std::vector<int32_t> s, mp, b;
    std::vector<uint8_t> f;
    std::vector<uint32_t> nd;
    for (int g = 0; g < m->ndev; g++) {
        const size_t ng = (size_t)(m->begin[(size_t)g + 1] - m->begin[(size_t)g]), at = (size_t)m->begin[(size_t)g];
        if (scores || ssemaps) s.resize(nq * ng);
        if (ssemaps) mp.resize(nq * ng * SAT_MAXDIM);
        if (base_scores) b.resize(nq * ng);
        if (unproven) f.resize(nq * ng);
        if (nodes) nd.resize(nq * ng);
        if (scores || ssemaps) {
            if (ssemaps) std::fill(mp.begin(), mp.end(), -1);
            SAT_TRY(sat_results(m->ctx[(size_t)g], ssemaps ? 1 : 0, s.data(), ssemaps ? mp.data() : nullptr));
        }
        SAT_TRY(sat_exact_results(m->ctx[(size_t)g], base_scores ? b.data() : nullptr, unproven ? f.data() : nullptr, nodes ? nd.data() : nullptr));
        for (size_t q = 0; q < nq; q++) {
            if (scores) std::copy(s.begin() + q * ng, s.begin() + (q + 1) * ng, scores + q * total + at);
            if (ssemaps) std::copy(mp.begin() + q * ng * SAT_MAXDIM, mp.begin() + (q + 1) * ng * SAT_MAXDIM, ssemaps + (q * total + at) * SAT_MAXDIM);
            if (base_scores) std::copy(b.begin() + q * ng, b.begin() + (q + 1) * ng, base_scores + q * total + at);
            if (unproven) std::copy(f.begin() + q * ng, f.begin() + (q + 1) * ng, unproven + q * total + at);
            if (nodes) std::copy(nd.begin() + q * ng, nd.begin() + (q + 1) * ng, nodes + q * total + at);
        }
    }
    return SAT_OK;
}

int sat_multi_exact_stats(sat_multi *m, sat_exact_stat *per_query)
{
    SAT_TRY(sat_check_context(m));
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_exact_check_state(c));
    if (!per_query) return sat_fail(SAT_EINVAL, "per_query buffer is null");
    const size_t nq = m->ctx[0]->queries.size();
    std::vector<sat_exact_stat> part(nq);
    std::fill(per_query, per_query + nq, sat_exact_stat{ 0, 0, 0, 0, 0 });
    for (int g = 0; g < m->ndev; g++) {
        SAT_TRY(sat_exact_stats(m->ctx[(size_t)g], part.data()));
        for (size_t q = 0; q < nq; q++) {                // integer sums: any order
            per_query[q].rows += part[q].rows;
            per_query[q].proven += part[q].proven;
            per_query[q].improved += part[q].improved;
            per_query[q].gain += part[q].gain;
            per_query[q].nodes += part[q].nodes;
        }
    }
    return SAT_OK;
}

int sat_multi_cluster_begin(sat_multi *m)
{
    SAT_TRY(check_multi(m));
    // every shard's nodes are the whole database's: its edges end at its own entries' ordinals, but start anywhere
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_cluster_begin(c, m->n_entries));
    return SAT_OK;
}

int sat_multi_cluster_add(sat_multi *m, double max_pvalue, const int32_t *query_node)
{
    SAT_TRY(check_multi(m));
    // the argument checks of sat_cluster_add, made for all shards before the first one adds anything
    if (!query_node) return sat_fail(SAT_EINVAL, "query_node is null");
    SAT_TRY(sat_check_pvalue(max_pvalue));
    const size_t nq = m->ctx[0]->queries.size();
    for (size_t q = 0; q < nq; q++)
        if (query_node[q] < 0 || query_node[q] >= m->n_entries)
            return sat_fail(SAT_EINVAL, "query %zu: node %d outside 0..%d", q, query_node[q], m->n_entries - 1);
    return each_shard(m, [&](int g) { return sat_cluster_add(m->ctx[(size_t)g], max_pvalue, query_node); });
}

int sat_multi_cluster_labels(sat_multi *m, int32_t *label, int32_t *degree, unsigned long long *edges)
{
    SAT_TRY(check_multi(m));
    if (!label) return sat_fail(SAT_EINVAL, "label buffer is null");
    const size_t n = (size_t)m->n_entries, ndev = (size_t)m->ndev;
    if (ndev == 1) return sat_cluster_labels(m->ctx[0], label, degree, edges);
    std::vector<int32_t> labels(ndev * n), deg(degree ? n : 0);
    if (degree) std::fill(degree, degree + n, 0);
    if (edges) *edges = 0ull;
    for (size_t g = 0; g < ndev; g++) {
        unsigned long long e = 0ull;
        const int rc = sat_cluster_labels(m->ctx[g], labels.data() + g * n, degree ? deg.data() : nullptr, edges ? &e : nullptr);
        if (rc != SAT_OK) return rc;
        for (size_t v = 0; degree && v < n; v++) degree[v] += deg[v];          // integer sums: any order
        if (edges) *edges += e;
    }
    if (sat_cluster_join((int)n, (int)ndev, labels.data(), label) != 0)
        return sat_fail(SAT_EDEVICE, "a shard returned a label outside 0..%d", m->n_entries - 1);
    return SAT_OK;
}

int sat_multi_cluster_begin_levels(sat_multi *m, int n_levels, const double *max_pvalue)
{
    SAT_TRY(check_multi(m));
    // every shard makes the same checks on the same arguments: the first one's refusal is every one's, before any began
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_cluster_begin_levels(c, m->n_entries, n_levels, max_pvalue));
    return SAT_OK;
}

int sat_multi_cluster_add_levels(sat_multi *m, const int32_t *query_node)
{
    SAT_TRY(check_multi(m));
    // the argument checks of sat_cluster_add_levels, made for all shards before the first one adds anything
    if (!query_node) return sat_fail(SAT_EINVAL, "query_node is null");
    const size_t nq = m->ctx[0]->queries.size();
    for (size_t q = 0; q < nq; q++)
        if (query_node[q] < 0 || query_node[q] >= m->n_entries)
            return sat_fail(SAT_EINVAL, "query %zu: node %d outside 0..%d", q, query_node[q], m->n_entries - 1);
    return each_shard(m, [&](int g) { return sat_cluster_add_levels(m->ctx[(size_t)g], query_node); });
}

int sat_multi_cluster_labels_levels(sat_multi *m, int32_t *label, int32_t *degree, unsigned long long *edges)
{
    SAT_TRY(check_multi(m));
    if (!label) return sat_fail(SAT_EINVAL, "label buffer is null");
    const size_t n = (size_t)m->n_entries, ndev = (size_t)m->ndev, levels = (size_t)m->ctx[0]->cluster_levels;
    // one shard, or no leveled accumulator (the shard's call says which state error that is)
    if (ndev == 1 || levels == 0) return sat_cluster_labels_levels(m->ctx[0], label, degree, edges);
    // the shards' labels as [level][shard][node], so that a level's sets lie together for the join
    std::vector<int32_t> labels(levels * ndev * n), shard(levels * n), deg(degree ? levels * n : 0);
    std::vector<unsigned long long> e(levels);
    if (degree) std::fill(degree, degree + levels * n, 0);
    if (edges) std::fill(edges, edges + levels, 0ull);
    for (size_t g = 0; g < ndev; g++) {
        const int rc = sat_cluster_labels_levels(m->ctx[g], shard.data(), degree ? deg.data() : nullptr, edges ? e.data() : nullptr);
        if (rc != SAT_OK) return rc;
        for (size_t j = 0; j < levels; j++) {
            std::copy(shard.begin() + j * n, shard.begin() + (j + 1) * n, labels.begin() + (j * ndev + g) * n);
            if (edges) edges[j] += e[j];
        }
        for (size_t i = 0; degree && i < levels * n; i++) degree[i] += deg[i];  // integer sums: any order
    }
    for (size_t j = 0; j < levels; j++)
        if (sat_cluster_join((int)n, (int)ndev, labels.data() + j * ndev * n, label + j * n) != 0)
            return sat_fail(SAT_EDEVICE, "a shard returned a label outside 0..%d", m->n_entries - 1);
    const int broken = sat_cluster_nested((int)n, (int)levels, label);
    if (broken != 0) return sat_fail(SAT_EDEVICE, "the joined labels of level %d do not lie inside level %d's", broken - 1, broken);
    return SAT_OK;
}

// ---- Transitive search (sat_reach_*).  Every shard keeps keys and supports over the whole database's
// nodes; a step a -> b is added by the shard that holds b's entry, so the element-wise min of the shards' keys and the
// sum of their supports (sat_reach_join) are what one context holding the whole database has.

// the shards' arrays joined on the host: keys [n], support [n]
static int reach_joined(sat_multi *m, std::vector<uint64_t> &keys, std::vector<int32_t> &support)
{
    const size_t n = (size_t)m->n_entries, ndev = (size_t)m->ndev;
    std::vector<uint64_t> k(ndev * n);
    std::vector<int32_t> s(ndev * n);
    for (size_t g = 0; g < ndev; g++)
        SAT_TRY(sat_reach_arrays_fetch(m->ctx[g], reinterpret_cast<unsigned long long *>(k.data() + g * n), s.data() + g * n));
    keys.resize(n);
    support.resize(n);
    if (sat_reach_join((int)n, (int)ndev, k.data(), s.data(), keys.data(), support.data()) != 0)
        return sat_fail(SAT_EDEVICE, "the shards' reach arrays could not be joined");
    return SAT_OK;
}

int sat_multi_reach_begin(sat_multi *m, int n_seeds, const int32_t *seed_node)
{
    SAT_TRY(check_multi(m));
    SAT_TRY(sat_reach_check_begin(m->n_entries, n_seeds, seed_node));
    // every shard's nodes are the whole database's, and every shard knows the seeds
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_reach_begin(c, m->n_entries, n_seeds, seed_node));
    return SAT_OK;
}

int sat_multi_reach_add(sat_multi *m, int depth, double max_pvalue, const int32_t *query_node)
{
    SAT_TRY(check_multi(m));
    // the checks of sat_reach_add, made for all shards before the first one adds anything
    for (sat_ctx *c : m->ctx) {
        if (c->reach_nodes <= 0)
            return sat_fail(SAT_ESTATE, "no reach accumulator (sat_reach_begin has not been called since the last database upload)");
        SAT_TRY(sat_check_searched(c));
    }
    SAT_TRY(sat_reach_check_add(depth, max_pvalue, (int)m->ctx[0]->queries.size(), query_node, m->n_entries));
    return each_shard(m, [&](int g) { return sat_reach_add(m->ctx[(size_t)g], depth, max_pvalue, query_node); });
}

int sat_multi_reach_frontier(sat_multi *m, int depth, int cap, int32_t *nodes, int32_t *count)
{
    SAT_TRY(check_multi(m));
    if (m->ndev == 1) return sat_reach_frontier(m->ctx[0], depth, cap, nodes, count);
    SAT_TRY(sat_reach_check_fetch(depth, cap, nodes, count));
    std::vector<uint64_t> keys;
    std::vector<int32_t> support;
    SAT_TRY(reach_joined(m, keys, support));
    int32_t c = 0;
    for (size_t v = 0; v < keys.size(); v++)
        if ((int)(keys[v] >> 58) == depth) {
            if (c < cap) nodes[c] = (int32_t)v;
            c++;
        }
    *count = c;
    return SAT_OK;
}

int sat_multi_reach_rows(sat_multi *m, int cap, sat_reach_row *rows, int32_t *count)
{
    SAT_TRY(check_multi(m));
    if (m->ndev == 1) return sat_reach_rows(m->ctx[0], cap, rows, count);
    SAT_TRY(sat_reach_check_fetch(0, cap, rows, count));
    std::vector<uint64_t> keys;
    std::vector<int32_t> support;
    SAT_TRY(reach_joined(m, keys, support));
    const int c = sat_reach_decode(m->n_entries, keys.data(), support.data(), cap, reinterpret_cast<sat_reach_rec *>(rows));
    if (c < 0) return sat_fail(SAT_EDEVICE, "a shard returned a key whose parent lies outside 0..%d", m->n_entries - 1);
    *count = c;
    return SAT_OK;
}

int sat_multi_reach_end(sat_multi *m)
{
    SAT_TRY(sat_check_context(m));
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_reach_end(c));
    return SAT_OK;
}

int sat_multi_search_reach(sat_multi *m, int n_seeds, const int32_t *seed_entry, int lorder, int maxstart, double max_pvalue,
                           int max_depth, int max_queries, int batch, double censor, uint32_t first_query_ordinal, int cap,
                           sat_reach_row *rows, int32_t *count, sat_reach_info *info)
{
    SAT_TRY(check_multi(m));
    SAT_TRY(sat_reach_check_search(n_seeds, seed_entry, m->n_entries, maxstart, max_pvalue, max_depth, max_queries, batch, censor,
                                   cap, rows, count, info));
    // the whole database's entries are its nodes
    SAT_TRY(sat_multi_reach_begin(m, n_seeds, seed_entry));
    *info = sat_reach_info{ 0, 0, 0, SAT_REACH_EXHAUSTED, 0.0, 0.0 };
    std::vector<int32_t> frontier;
    for (int d = 1;; d++) {
        frontier.resize((size_t)std::min(max_queries - info->queries, m->n_entries));
        int32_t c = 0;
        SAT_TRY(sat_multi_reach_frontier(m, d - 1, (int)frontier.size(), frontier.data(), &c));
        if (c == 0) { info->stop = SAT_REACH_EXHAUSTED; break; }
        if (d - 1 == max_depth) { info->stop = SAT_REACH_DEPTH; break; }
        if (c > max_queries - info->queries) { info->stop = SAT_REACH_BUDGET; break; }
        for (int at = 0; at < c; at += batch) {
            const int nb = std::min(batch, c - at);
            SAT_TRY(sat_multi_queries_from_db(m, nb, frontier.data() + at, first_query_ordinal + (uint32_t)(info->queries + at)));
            double ms = 0.0;
            SAT_TRY(sat_multi_search_only(m, lorder, 0, maxstart, &ms));
            info->search_ms += ms;
            if (censor >= 0.0) {
                const int rc = sat_fit_queries((size_t)nb, censor, nullptr,
                                               [&](uint32_t *counts, int32_t *below) { return sat_multi_score_histogram(m, counts, below); },
                                               [&](const sat_fit *fit) { return sat_multi_stats_set(m, fit); });
                if (rc != SAT_OK) return bail(m, rc);
            }
            const Stopwatch clock;
            SAT_TRY(sat_multi_reach_add(m, d, max_pvalue, frontier.data() + at));
            SAT_TRY(each_shard(m, [&](int g) { return sat_sync(m->ctx[(size_t)g]); }));
            clock.stop(&ms);
            info->pass_ms += ms;
        }
        info->queries += c;
        info->levels++;
    }
    SAT_TRY(sat_multi_reach_rows(m, cap, rows, count));
    info->reached = *count;
    return SAT_OK;
}

int sat_multi_cover_begin(sat_multi *m)
{
    SAT_TRY(check_multi(m));
    // every shard's nodes are the whole database's: its rows end at its own entries' ordinals, but start anywhere
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_cover_begin(c, m->n_entries));
    return SAT_OK;
}

int sat_multi_cover_add(sat_multi *m, double max_pvalue, const int32_t *query_node)
{
    SAT_TRY(check_multi(m));
    // the argument checks of sat_cover_add, made for all shards before the first one adds anything
    if (!query_node) return sat_fail(SAT_EINVAL, "query_node is null");
    SAT_TRY(sat_check_pvalue(max_pvalue));
    SAT_TRY(sat_check_query_nodes((int)m->ctx[0]->queries.size(), query_node, m->n_entries));
    return each_shard(m, [&](int g) { return sat_cover_add(m->ctx[(size_t)g], max_pvalue, query_node); });
}

int sat_multi_cover_solve(sat_multi *m, int32_t *rep, int32_t *degree, unsigned long long *edges, int *rounds)
{
    SAT_TRY(check_multi(m));
    if (!rep) return sat_fail(SAT_EINVAL, "rep buffer is null");
    // The other shards' matrices ORed into shard 0's, through the host, a slab of rows at a time (32 MB at most, or one
    // row).  An OR adds edges of the whole graph only and is idempotent: shard 0 may be added to and solved again
    const int n = m->n_entries;
    const size_t stride = sat_cover_stride(n);
    const int slab = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)32 << 20) / (stride * sizeof(unsigned long long))));
    std::vector<unsigned long long> rows(m->ndev > 1 ? (size_t)slab * stride : 0);
    for (int g = 1; g < m->ndev; g++)
        for (int row0 = 0; row0 < n; row0 += slab) {
            const int count = std::min(slab, n - row0);
            SAT_TRY(sat_cover_rows_fetch(m->ctx[(size_t)g], row0, count, rows.data()));
            SAT_TRY(sat_cover_rows_or(m->ctx[0], row0, count, rows.data()));
        }
    return sat_cover_solve(m->ctx[0], rep, degree, edges, rounds);
}

int sat_multi_eval_classes(sat_multi *m, const int32_t *node_class)
{
    SAT_TRY(check_multi(m));
    // every shard's nodes are the whole database's; the same checks on the same arguments: the first refusal is every one's
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_eval_classes(c, m->n_entries, node_class));
    return SAT_OK;
}

int sat_multi_eval_rows(sat_multi *m, const int32_t *query_node, int rocn, sat_eval *rows)
{
    SAT_TRY(check_multi(m));
    if (m->ndev == 1) return sat_eval_rows(m->ctx[0], query_node, rocn, rows);      // no table crosses
    // the checks of sat_eval_rows, made for all shards before the first one works
    for (sat_ctx *c : m->ctx) {
        SAT_TRY(sat_check_searched(c));
        SAT_TRY(sat_check_eval_classes(c->eval_nodes > 0));
    }
    SAT_TRY(sat_check_eval_args(rocn, query_node && rows));
    const int nq = (int)m->ctx[0]->queries.size();
    SAT_TRY(sat_check_query_nodes(nq, query_node, m->ctx[0]->eval_nodes));
    // each shard's tables of its own entries, packed in query order; integer counts add up, in any order
    std::vector<size_t> off((size_t)nq + 1, 0);
    for (int q = 0; q < nq; q++) off[(size_t)q + 1] = off[(size_t)q] + 2 * (size_t)sat_eval_bins(m->ctx[0]->queries[(size_t)q].n1);
    std::vector<uint32_t> sum(off[(size_t)nq], 0u), part(off[(size_t)nq]);
    for (int g = 0; g < m->ndev; g++) {
        SAT_TRY(sat_eval_tables(m->ctx[(size_t)g], query_node, part.data(), nullptr));
        for (size_t i = 0; i < sum.size(); i++) sum[i] += part[i];
    }
    for (int q = 0; q < nq; q++) {
        const int32_t bins = sat_eval_bins(m->ctx[0]->queries[(size_t)q].n1), cls = m->ctx[0]->eval_class[(size_t)query_node[q]];
        sat_eval_row row = { 0, 0, 0, 0, 0, cls < 0 ? -1 : cls };
        if (cls >= 0 && sat_eval_reduce(sum.data() + off[(size_t)q], sum.data() + off[(size_t)q] + bins, bins, rocn, &row) != 0)
            return sat_fail(SAT_EDEVICE, "query %d: the shards' tables do not add up to a table", q);
        memcpy(rows + q, &row, sizeof row);
    }
    return SAT_OK;
}

int sat_multi_profile_rows(sat_multi *m, double max_pvalue, const int32_t *query_node, uint32_t *hits, uint32_t *joint, const int64_t *offset)
{
    SAT_TRY(check_multi(m));
    if (m->ndev == 1) return sat_profile_rows(m->ctx[0], max_pvalue, query_node, hits, joint, offset);     // nothing is added
    // the checks of sat_profile_rows, made for all shards before the first one works
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_profile_check(c, max_pvalue, hits, joint));
    // each shard's counts of its own entries, packed in query order; integer counts add up, in any order
    const size_t nq = m->ctx[0]->queries.size();
    std::vector<size_t> off(nq + 1, 0);
    for (size_t q = 0; q < nq; q++) off[q + 1] = off[q] + (size_t)m->ctx[0]->queries[q].n1 * (size_t)m->ctx[0]->queries[q].n1;
    std::vector<uint32_t> part_hits(nq), part(off[nq]);
    std::fill(hits, hits + nq, 0u);
    for (size_t q = 0; q < nq; q++) {
        uint32_t *out = joint + (offset ? (size_t)offset[q] : off[q]);
        std::fill(out, out + (off[q + 1] - off[q]), 0u);
    }
    for (int g = 0; g < m->ndev; g++) {
        SAT_TRY(sat_profile_rows(m->ctx[(size_t)g], max_pvalue, query_node, part_hits.data(), part.data(), nullptr));
        for (size_t q = 0; q < nq; q++) {
            hits[q] += part_hits[q];
            uint32_t *out = joint + (offset ? (size_t)offset[q] : off[q]);
            for (size_t i = off[q]; i < off[q + 1]; i++) out[i - off[q]] += part[i];
        }
    }
    return SAT_OK;
}

int sat_multi_baseline_keep(sat_multi *m)
{
    SAT_TRY(check_multi(m));
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_check_searched(c));
    return each_shard(m, [&](int g) { return sat_baseline_keep(m->ctx[(size_t)g]); });
}

int sat_multi_baseline_drop(sat_multi *m)
{
    SAT_TRY(sat_check_context(m));
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_baseline_drop(c));
    return SAT_OK;
}

int sat_multi_baseline_results(sat_multi *m, int32_t *scores, double *pvalues)
{
    SAT_TRY(check_multi(m));
    for (sat_ctx *c : m->ctx)
        if (!c->baseline_nq) return sat_baseline_results(c, scores, pvalues);          // its SAT_ESTATE and text
    // each shard's [nq][its entries] rows into the columns of its entries
    const size_t nq = m->ctx[0]->baseline_nq, total = (size_t)m->n_entries;
    std::vector<int32_t> s;
    std::vector<double> p;
    for (int g = 0; g < m->ndev; g++) {
        const size_t ng = (size_t)(m->begin[(size_t)g + 1] - m->begin[(size_t)g]), at = (size_t)m->begin[(size_t)g];
        if (scores) s.resize(nq * ng);
        if (pvalues) p.resize(nq * ng);
        SAT_TRY(sat_baseline_results(m->ctx[(size_t)g], scores ? s.data() : nullptr, pvalues ? p.data() : nullptr));
        for (size_t q = 0; q < nq; q++) {
            if (scores) std::copy(s.begin() + q * ng, s.begin() + (q + 1) * ng, scores + q * total + at);
            if (pvalues) std::copy(p.begin() + q * ng, p.begin() + (q + 1) * ng, pvalues + q * total + at);
        }
    }
    return SAT_OK;
}

int sat_multi_reorder_hits(sat_multi *m, double max_pvalue, double min_base_pvalue, int kinds, int max_rows, int32_t *counts,
                           int capacity, sat_reorder_hit *rows, int32_t *ssemaps)
{
    SAT_TRY(check_multi(m));
    // the checks of sat_reorder_hits, made for all shards before the first one works
    for (sat_ctx *c : m->ctx) SAT_TRY(sat_reorder_check(c, max_pvalue, min_base_pvalue, kinds, counts));
    const int nq = (int)m->ctx[0]->queries.size();
    // every shard counts its qualifying rows; a query's rows are the sum, cut to max_rows
    std::vector<std::vector<int32_t>> raw((size_t)m->ndev, std::vector<int32_t>((size_t)nq));
    for (int g = 0; g < m->ndev; g++) SAT_TRY(sat_reorder_count(m->ctx[(size_t)g], max_pvalue, min_base_pvalue, kinds, raw[(size_t)g].data()));
    size_t total = 0;
    for (int q = 0; q < nq; q++) {
        long long c = 0;
        for (int g = 0; g < m->ndev; g++) c += raw[(size_t)g][(size_t)q];
        counts[q] = sat_row_cap(c > INT_MAX ? INT_MAX : (int32_t)c, max_rows);
        total += (size_t)counts[q];
    }
    if (total > (size_t)INT_MAX) return sat_fail(SAT_EINVAL, "%zu rows qualify: more than one call can return", total);
    if (!rows || (long long)total > (long long)capacity) return (int)total;
    // each shard's rows (max_rows per query at most), merged per query: score descending, ties in database order - the
    // lower shard first, as merge_shards has it for sat_multi_hits_cutoff
    std::vector<std::vector<sat_reorder_hit>> part((size_t)m->ndev);
    std::vector<std::vector<int32_t>> pmaps((size_t)m->ndev);
    std::vector<std::vector<size_t>> off((size_t)m->ndev, std::vector<size_t>((size_t)nq + 1, 0));
    for (int g = 0; g < m->ndev; g++) {
        for (int q = 0; q < nq; q++) off[(size_t)g][(size_t)q + 1] = off[(size_t)g][(size_t)q] + (size_t)sat_row_cap(raw[(size_t)g][(size_t)q], max_rows);
        part[(size_t)g].resize(off[(size_t)g][(size_t)nq]);
        if (ssemaps) pmaps[(size_t)g].resize(off[(size_t)g][(size_t)nq] * SAT_MAXDIM);
        SAT_TRY(sat_reorder_rows(m->ctx[(size_t)g], max_pvalue, min_base_pvalue, kinds, max_rows, raw[(size_t)g].data(), part[(size_t)g].data(),
                                 ssemaps ? pmaps[(size_t)g].data() : nullptr));
    }
    size_t out = 0;
    std::vector<size_t> head((size_t)m->ndev);
    for (int q = 0; q < nq; q++) {
        for (int g = 0; g < m->ndev; g++) head[(size_t)g] = off[(size_t)g][(size_t)q];
        for (int32_t r = 0; r < counts[q]; r++) {
            int bg = -1;
            for (int g = 0; g < m->ndev; g++)
                if (head[(size_t)g] < off[(size_t)g][(size_t)q + 1] &&
                    (bg < 0 || part[(size_t)g][head[(size_t)g]].hit.score > part[(size_t)bg][head[(size_t)bg]].hit.score))
                    bg = g;
            const size_t row = head[(size_t)bg]++;
            rows[out] = part[(size_t)bg][row];
            rows[out].hit.entry += m->begin[(size_t)bg];
            if (ssemaps) memcpy(ssemaps + out * SAT_MAXDIM, pmaps[(size_t)bg].data() + row * SAT_MAXDIM, sizeof(int32_t) * SAT_MAXDIM);
            out++;
        }
    }
    return (int)total;
}

int sat_multi_search_reordered(sat_multi *m, int maxstart, double censor, double *wall_ms)
{
    SAT_TRY(check_multi(m));
    const bool fit = censor >= 0.0;
    if (fit) SAT_TRY(sat_check_censor(censor));
    const Stopwatch clock;
    for (int pass = 0; pass < 2; pass++) {
        const int lorder = pass == 0, lsoln = pass == 1;            // the ordered search is the baseline
        SAT_TRY(fit ? sat_multi_search_fit(m, lorder, lsoln, maxstart, censor, nullptr, nullptr)
                    : sat_multi_search_only(m, lorder, lsoln, maxstart, nullptr));
        if (pass == 0) SAT_TRY(sat_multi_baseline_keep(m));
    }
    clock.stop(wall_ms);
    return SAT_OK;
}

unsigned long long sat_multi_stat_d2h_bytes(const sat_multi *m)
{
    if (!m) return 0ull;
    unsigned long long total = m->d2h_bytes;
    for (const sat_ctx *c : m->ctx) total += sat_stat_d2h_bytes(c);
    return total;
}

}  // extern "C"
