// sat_db.hip - what goes up to the device: the packed database shard (checked where it lands, bucketed by order) and
// the query batch (grouped and transposed into one blob), and the descriptors that point into both.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "satabsearch.h"
#include "sat_pairs.hpp"

namespace {

// The cells the kernel's pair arithmetic can take, database and query alike: SSE types 0..3, tableau nibbles 0..7 (the
// reader produces 0..4) and |distance| < 1e29 or non-finite (a non-finite distance never scores).
__host__ __device__ inline bool bad_type(uint32_t type) { return type > 3; }
__host__ __device__ inline bool bad_code(uint32_t code) { return (code & 0x88u) != 0; }
__host__ __device__ inline bool bad_distance(float d)
{
    const float ad = fabsf(d);
    return ad >= 1.0e29f && ad <= 3.4028234e38f;      // finite and out of range
}

void free_db(sat_ctx *ctx)
{
    ctx->d_orders.reset();
    ctx->d_cell_off.reset();
    ctx->d_tab.reset();
    ctx->d_dist.reset();
    ctx->d_ordinal.reset();
    ctx->max_ordinal = 0;
    ctx->h_ordinal.clear();
    sat_cluster_drop(ctx);                    // its nodes were this database's
    sat_cover_drop(ctx);                      // and the cover accumulator's
    sat_reach_drop(ctx);                      // and the transitive search's
    sat_eval_drop(ctx);                       // and so were the classes'
    ctx->d_lists.reset();
    ctx->d_scores.reset();
    ctx->d_ssemaps.reset();
    ctx->desc_dirty = true;
    ctx->n_entries = 0;
    ctx->min_rows = 0;
    ctx->searched_nq = 0;
    ctx->fits.clear();
    ctx->baseline_nq = 0;                     // the kept baseline was of this database's rows
    ctx->h_orders.clear();
}

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
            bad |= bad_type(t);
        } else {
            const float d = dist[base + c];
            bad |= bad_code(t) || bad_distance(d);
        }
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0) atomicMin(first_bad, e);
}

}  // namespace

// sat_ctx.hpp: (re)build the device query descriptors: pointers into the query blob and into the result
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
            const QueryBlob at = query_blob(q.n1p);
            SatQuery d;
            d.qdist = reinterpret_cast<const float4 *>(blob);
            d.qcode = reinterpret_cast<const uint32_t *>(blob + at.qcode);
            d.qtypes = blob + at.qtypes;
            d.qpair = reinterpret_cast<const uint2 *>(blob + at.qpair);
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

// sat_ctx.hpp: load this file's code object (an empty launch of its kernel)
int sat_db_load_code(sat_ctx *ctx)
{
    hipLaunchKernelGGL(validate_cells, dim3(1), dim3(256), 0, ctx->stream, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return SAT_OK;
}

extern "C" {

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
    const uint32_t max_ordinal = *std::max_element(ord.begin(), ord.end());

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
        ctx->max_ordinal = max_ordinal;
        ctx->h_ordinal = ord;

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
                if (bad_type(ty)) return sat_fail(SAT_EINVAL, "entry %d: SSE %d has type code %u (0..3 expected)", e, i, ty);
                for (int j = 0; j < i; j++) {
                    if (bad_code(tab_tri[rowbase + j]))
                        return sat_fail(SAT_EINVAL, "entry %d: tableau code 0x%02x at (%d,%d) has a nibble above 7", e, tab_tri[rowbase + j], i, j);
                    float d = dist_tri[rowbase + j];
                    if (bad_distance(d))
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
    // whole-database polish (sat_polish_all_set): the passes of a polished search follow one another over the whole
    // shard, so the upload and the search run one after the other
    if (ctx && ctx->polish_all) {
        const int rc = upload_impl(ctx, n_entries, orders, cell_off, tab_tri, dist_tri, db_ordinal, nullptr);
        return rc != SAT_OK ? rc : sat_polish_all_launch(ctx, lorder, lsoln, maxstart);
    }
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
        q.n1p = query_n1p(n1);
        q.ordinal = first_query_ordinal + (uint32_t)qi;
        q.blob_off = blob_bytes;
        q.ssemap_off = 0;
        blob_bytes += query_blob(q.n1p).bytes;
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
        const QueryBlob at = query_blob(n1p);
        float4 *qdist = reinterpret_cast<float4 *>(blob.data() + q.blob_off);
        uint32_t *qcode = reinterpret_cast<uint32_t *>(blob.data() + q.blob_off + at.qcode);
        uint8_t *qtypes = blob.data() + q.blob_off + at.qtypes;
        // dense [i][k] cells {distance, code byte}: the same values as the grouped arrays, for the pair-by-pair
        // full score of an initial map
        uint32_t *qpair = reinterpret_cast<uint32_t *>(blob.data() + q.blob_off + at.qpair);
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
            if (bad_type(types[i]))
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
                        if (bad_code(code))
                            return sat_fail(SAT_EINVAL, "query %d: tableau code 0x%02x at (%d,%d) has a nibble above 7", qi, code, i, k);
                        if (bad_distance(v))
                            return sat_fail(SAT_EINVAL, "query %d: distance %g at (%d,%d) out of range", qi, v, i, k);
                        if (std::isfinite(v)) d[sidx] = v;
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
    ctx->query_h2d_bytes += blob_bytes;
    ctx->queries.swap(infos);
    ctx->desc_dirty = true;
    ctx->searched_nq = 0;                     // the result buffers no longer belong to the current batch
    ctx->fits.clear();
    ctx->baseline_nq = 0;                     // nor does a kept baseline
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

}  // extern "C"
