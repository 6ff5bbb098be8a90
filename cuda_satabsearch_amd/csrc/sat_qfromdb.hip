// sat_qfromdb.hip - queries taken from the resident database (sat_queries_from_db): a kernel expands
// entries of the shard into the query blob, byte for byte what sat_queries_set (sat_db.hip) builds on the host from the
// same entries' dense arrays - only the list of entry indices crosses from the host.  A motif query
// (sat_queries_from_db_sses) is a chosen list of an entry's SSEs: the same kernel gathers the list's
// sub-triangle from the entry and expands that; the indices, the lists' offsets and the list bytes cross from the host.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "satabsearch.h"
#include "satabsearch_debug.h"
#include "sat_ctx.hpp"

namespace {

constexpr int kQThreads = 256;
constexpr int kTriCells = SAT_MAXDIM * (SAT_MAXDIM + 1) / 2;         // 6216: the largest packed triangle

// What the host sends per query: the entry's index in the shard, or for a query another shard expands (sat_multi)
// minus its padded order - such a query only takes its room in the blob.  With lists (sbeg not null: the CSR offsets of
// sat_queries_from_db_sses) query q of the shard is the sbeg[q + 1] - sbeg[q] listed SSEs of its entry, the whole entry
// where that range is empty: the order of a query is its list's length, not its entry's.
__device__ inline int code_n1p(int q, const int32_t *code, const int32_t *orders, const int32_t *sbeg)
{
    if (code[q] < 0) return -code[q];
    const int m = sbeg ? sbeg[q + 1] - sbeg[q] : 0;
    return query_n1p(m > 0 ? m : orders[code[q]]);
}

// Each query's offset in the blob: the exclusive sum of the queries' blob sizes, input order.  One workgroup; thread t
// sums the queries t * per .. t * per + per - 1, the threads' sums are added up, and each thread walks its run again.
__global__ void __launch_bounds__(kQThreads) qfromdb_offsets(int nq, const int32_t *code, const int32_t *orders, const int32_t *sbeg,
                                                             unsigned long long *qoff)
{
    __shared__ unsigned long long part[kQThreads];
    const int t = threadIdx.x, per = (nq + kQThreads - 1) / kQThreads;
    const int q0 = t * per < nq ? t * per : nq, q1 = q0 + per < nq ? q0 + per : nq;
    unsigned long long sum = 0;
    for (int q = q0; q < q1; q++) sum += query_blob(code_n1p(q, code, orders, sbeg)).bytes;
    part[t] = sum;
    __syncthreads();
    unsigned long long at = 0;
    for (int u = 0; u < t; u++) at += part[u];
    for (int q = q0; q < q1; q++) {
        qoff[q] = at;
        at += query_blob(code_n1p(q, code, orders, sbeg)).bytes;
    }
}

// Query cell (i, k) of an entry of order n whose packed triangle lies in LDS, as sat_queries_set fills it: the RAW
// uploaded cell (max, min); the sentinel and code 0 on the diagonal, in the padding and - the distance alone - where
// the distance is not finite.
__device__ inline void query_cell(int i, int k, int n, const float *sdist, const uint8_t *stab, float &d, uint32_t &c)
{
    d = SAT_K_QSENT;
    c = 0;
    if (i < n && k < n && i != k) {
        const int hi = i > k ? i : k, lo = i > k ? k : i, cell = hi * (hi + 1) / 2 + lo;
        const float v = sdist[cell];
        if ((__float_as_uint(v) & 0x7F800000u) != 0x7F800000u) d = v;         // finite
        c = stab[cell];
    }
}

// One workgroup per query: the entry's triangle into LDS (coalesced, at most 6216 cells x 5 bytes), then the blob.
// A motif query (a list l[0 .. m - 1] in sse at sbeg[q]) stages its OWN packed m-triangle instead: the list into LDS,
// then cell (i, k), k <= i, from the entry's cell (max, min) of (l[i], l[k]), rows i walked by the lane rows below and
// k along the lanes - nothing divides; an ascending list reads ascending addresses of row l[i] of the entry's triangle,
// and the LDS stores of a row are consecutive.  The writers then run on it with n = m, so the identity list gives the
// whole entry's bytes.
// Lanes run over the contiguous index of each array - column i of qdist / qcode, column k of qpair - in rows of
// 1 << wshift >= n1p lanes, the workgroup's 256 >> wshift rows side by side: 16-, 4- and 8-byte stores of consecutive
// lanes to consecutive addresses, and no lane divides.  In a row of the triangle read along i (fixed k < i) lane i is
// at dword i (i + 1) / 2 + k, and the triangular numbers of an aligned run of 32 i fall on 32 different banks.
__global__ void __launch_bounds__(kQThreads) queries_from_db(int nq, const int32_t *code, const int32_t *orders, const int64_t *cell_off,
                                                             const uint8_t *tab, const float *dist, const int32_t *sbeg,
                                                             const uint8_t *sse, const unsigned long long *qoff, uint8_t *blob,
                                                             unsigned long long blob_bytes)
{
    __shared__ float sdist[kTriCells];
    __shared__ uint8_t stab[(kTriCells + 15) & ~15];
    __shared__ uint8_t slist[(SAT_MAXDIM + 15) & ~15];
    const int q = blockIdx.x, t = threadIdx.x;
    if (q >= nq) return;
    const int e = code[q];
    if (e < 0) return;                                  // another shard's: it arrives by a device copy
    const int ne = orders[e], l0 = sbeg ? sbeg[q] : 0, m = sbeg ? sbeg[q + 1] - l0 : 0;
    const int n = m > 0 ? m : ne, n1p = query_n1p(n);
    const QueryBlob at = query_blob(n1p);
    // (checked at upload and by the host, which sized the blob)
    if (ne < 1 || ne > SAT_MAXDIM || m < 0 || m > ne || qoff[q] + at.bytes > blob_bytes) return;
    const int wshift = n1p == 16 ? 4 : (n1p == 32 ? 5 : (n1p == 64 ? 6 : 7));
    const int col = t & ((1 << wshift) - 1), row0 = t >> wshift, rows = kQThreads >> wshift;
    const int64_t base = cell_off[e];
    if (m == 0) {
        const int cells = n * (n + 1) / 2;
        for (int c = t; c < cells; c += kQThreads) {
            sdist[c] = dist[base + c];
            stab[c] = tab[base + c];
        }
    } else {
        if (t < m) {
            const int v = sse[l0 + t];
            slist[t] = (uint8_t)(v < ne ? v : ne - 1);          // (the host refused an index past the order)
        }
        __syncthreads();
        for (int i = row0; i < m; i += rows)
            if (col <= i) {
                const int li = slist[i], lk = slist[col], hi = li > lk ? li : lk, lo = li > lk ? lk : li;
                const int64_t src = base + hi * (hi + 1) / 2 + lo;
                const int dst = i * (i + 1) / 2 + col;
                sdist[dst] = dist[src];
                stab[dst] = tab[src];
            }
    }
    __syncthreads();

    uint8_t *out = blob + qoff[q];
    float4 *qdist = reinterpret_cast<float4 *>(out);
    uint32_t *qcode = reinterpret_cast<uint32_t *>(out + at.qcode);
    uint32_t *qtypes = reinterpret_cast<uint32_t *>(out + at.qtypes);
    uint2 *qpair = reinterpret_cast<uint2 *>(out + at.qpair);

    // grouped and transposed: group kw, column i holds cells (i, 4 kw .. 4 kw + 3)
    if (col < n1p)
        for (int kw = row0; kw < n1p / 4; kw += rows) {
            float d[4];
            uint32_t codes = 0;
            for (int s = 0; s < 4; s++) {
                uint32_t c;
                query_cell(col, 4 * kw + s, n, sdist, stab, d[s], c);
                codes |= c << (8 * s);
            }
            qdist[kw * n1p + col] = float4{ d[0], d[1], d[2], d[3] };
            qcode[kw * n1p + col] = codes;
        }
    // SSE types: the tableau diagonal, four to a lane, 0 past the order; then 0 up to the pair cells
    if (t < n1p / 4) {
        uint32_t types = 0;
        for (int s = 0; s < 4; s++) {
            const int i = 4 * t + s;
            if (i < n) types |= (uint32_t)stab[i * (i + 1) / 2 + i] << (8 * s);
        }
        qtypes[t] = types;
    }
    for (size_t b = at.qtypes + (size_t)n1p + (size_t)t; b < at.qpair; b += kQThreads) out[b] = 0;
    // dense [i][k] cells {distance, code}
    if (col < n1p)
        for (int i = row0; i < n1p; i += rows) {
            float d;
            uint32_t c;
            query_cell(i, col, n, sdist, stab, d, c);
            qpair[i * n1p + col] = uint2{ __float_as_uint(d), c };
        }
}

}  // namespace

// sat_ctx.hpp.  The batch of sat_queries_from_db on one context: query q is entry code[q] >= 0 of the shard, or (code[q]
// < 0, see code_n1p) a query of order n1s[q] whose blob segment the caller copies in from another context afterwards.
// With lists (sse_begin not null) query q is the listed SSEs of its entry, and one copy takes the indices, the offsets
// and the list bytes to the device, in that order.  Waits for the context's stream, replaces the blob, runs the kernels
// on the stream and waits again.
int sat_qfromdb_set(sat_ctx *ctx, int n_queries, const int32_t *code, const int32_t *n1s, const int32_t *sse_begin,
                    const uint8_t *sse, uint32_t first_query_ordinal)
{
    std::vector<sat_ctx::QueryInfo> infos((size_t)n_queries);
    size_t blob_bytes = 0;
    for (int qi = 0; qi < n_queries; qi++) {
        auto &q = infos[(size_t)qi];
        q.n1 = n1s[qi];
        q.n1p = query_n1p(q.n1);
        q.ordinal = first_query_ordinal + (uint32_t)qi;
        q.blob_off = blob_bytes;
        q.ssemap_off = 0;
        q.cls = q.desc = 0;
        blob_bytes += query_blob(q.n1p).bytes;
    }
    // what crosses: 4 bytes a query, and with lists 4 (n_queries + 1) of offsets and the lists
    const size_t nq = (size_t)n_queries, list_bytes = sse_begin ? (size_t)sse_begin[n_queries] : 0;
    const size_t h2d_bytes = nq * sizeof(int32_t) + (sse_begin ? (nq + 1) * sizeof(int32_t) + list_bytes : 0);
    std::vector<int32_t> staged;
    if (sse_begin) {
        staged.resize((h2d_bytes + 3) / 4);
        memcpy(staged.data(), code, nq * sizeof(int32_t));
        memcpy(staged.data() + nq, sse_begin, (nq + 1) * sizeof(int32_t));
        if (list_bytes) memcpy(staged.data() + 2 * nq + 1, sse, list_bytes);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // from here on the old batch is gone: a failure leaves the context without queries
    ctx->queries.clear();
    ctx->desc_dirty = true;
    ctx->searched_nq = 0;
    ctx->fits.clear();
    ctx->baseline_nq = 0;
    ctx->d_qblob.reset();
    ctx->d_qdesc.reset();
    int rc;
    if ((rc = ctx->d_qblob.grow(blob_bytes)) != SAT_OK || (rc = ctx->d_qdesc.grow((size_t)n_queries)) != SAT_OK ||
        (rc = ctx->d_qentry.grow((h2d_bytes + 3) / 4)) != SAT_OK || (rc = ctx->d_qoff.grow((size_t)n_queries)) != SAT_OK)
        return rc;
    HIP_TRY(hipMemcpy(ctx->d_qentry.get(), sse_begin ? staged.data() : code, h2d_bytes, hipMemcpyHostToDevice));
    ctx->query_h2d_bytes += h2d_bytes;
    const int32_t *d_sbeg = sse_begin ? ctx->d_qentry.get() + nq : nullptr;
    const uint8_t *d_sse = sse_begin ? reinterpret_cast<const uint8_t *>(ctx->d_qentry.get() + 2 * nq + 1) : nullptr;
    hipLaunchKernelGGL(qfromdb_offsets, dim3(1), dim3(kQThreads), 0, ctx->stream, n_queries, ctx->d_qentry.get(), ctx->d_orders.get(),
                       d_sbeg, ctx->d_qoff.get());
    if (hipGetLastError() != hipSuccess) return sat_fail(SAT_EDEVICE, "launch of the query offsets failed");
    hipLaunchKernelGGL(queries_from_db, dim3((unsigned)n_queries), dim3(kQThreads), 0, ctx->stream, n_queries, ctx->d_qentry.get(),
                       ctx->d_orders.get(), ctx->d_cell_off.get(), ctx->d_tab.get(), ctx->d_dist.get(), d_sbeg, d_sse,
                       ctx->d_qoff.get(), ctx->d_qblob.get(), (unsigned long long)blob_bytes);
    if (hipGetLastError() != hipSuccess) return sat_fail(SAT_EDEVICE, "launch of the query expansion failed");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->queries.swap(infos);
    return SAT_OK;
}

int sat_qfromdb_check_offsets(int n_queries, const int32_t *sse_begin, const uint8_t *sse)
{
    if (!sse_begin || !sse) return sat_fail(SAT_EINVAL, "null SSE list (sse_begin or sse)");
    if (sse_begin[0] != 0) return sat_fail(SAT_EINVAL, "sse_begin[0] is %d, not 0", sse_begin[0]);
    for (int q = 0; q < n_queries; q++)
        if (sse_begin[q + 1] < sse_begin[q])
            return sat_fail(SAT_EINVAL, "query %d: sse_begin descends from %d to %d", q, sse_begin[q], sse_begin[q + 1]);
    return SAT_OK;
}

int sat_qfromdb_check_list(int q, int entry, int order, const uint8_t *list, int m)
{
    if (m > order) return sat_fail(SAT_EINVAL, "query %d: %d SSEs listed, entry %d has %d", q, m, entry, order);
    bool seen[SAT_MAXDIM + 1] = { false };
    for (int i = 0; i < m; i++) {
        if (list[i] >= order) return sat_fail(SAT_EINVAL, "query %d: SSE %d outside 0..%d of entry %d", q, (int)list[i], order - 1, entry);
        if (seen[list[i]]) return sat_fail(SAT_EINVAL, "query %d: SSE %d listed twice", q, (int)list[i]);
        seen[list[i]] = true;
    }
    return SAT_OK;
}

void sat_qfromdb_segment(const sat_ctx *ctx, int q, uint8_t **at, size_t *bytes)
{
    const auto &info = ctx->queries[(size_t)q];
    *at = ctx->d_qblob.get() + info.blob_off;
    *bytes = query_blob(info.n1p).bytes;
}

extern "C" {

int sat_queries_from_db(sat_ctx *ctx, int n_queries, const int32_t *entry, uint32_t first_query_ordinal)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (n_queries < 1 || !entry) return sat_fail(SAT_EINVAL, "bad query batch (n_queries=%d)", n_queries);
    if (ctx->n_entries <= 0) return sat_fail(SAT_ESTATE, "no database uploaded");
    std::vector<int32_t> n1s((size_t)n_queries);
    for (int qi = 0; qi < n_queries; qi++) {
        if (entry[qi] < 0 || entry[qi] >= ctx->n_entries)
            return sat_fail(SAT_EINVAL, "query %d: entry %d outside 0..%d", qi, entry[qi], ctx->n_entries - 1);
        n1s[(size_t)qi] = ctx->h_orders[(size_t)entry[qi]];
    }
    return sat_qfromdb_set(ctx, n_queries, entry, n1s.data(), nullptr, nullptr, first_query_ordinal);
}

int sat_queries_from_db_sses(sat_ctx *ctx, int n_queries, const int32_t *entry, const int32_t *sse_begin, const uint8_t *sse,
                             uint32_t first_query_ordinal)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (n_queries < 1 || !entry) return sat_fail(SAT_EINVAL, "bad query batch (n_queries=%d)", n_queries);
    int rc = sat_qfromdb_check_offsets(n_queries, sse_begin, sse);
    if (rc != SAT_OK) return rc;
    if (ctx->n_entries <= 0) return sat_fail(SAT_ESTATE, "no database uploaded");
    std::vector<int32_t> n1s((size_t)n_queries);
    for (int qi = 0; qi < n_queries; qi++) {
        if (entry[qi] < 0 || entry[qi] >= ctx->n_entries)
            return sat_fail(SAT_EINVAL, "query %d: entry %d outside 0..%d", qi, entry[qi], ctx->n_entries - 1);
        const int order = ctx->h_orders[(size_t)entry[qi]], m = sse_begin[qi + 1] - sse_begin[qi];
        if ((rc = sat_qfromdb_check_list(qi, entry[qi], order, sse + sse_begin[qi], m)) != SAT_OK) return rc;
        n1s[(size_t)qi] = m > 0 ? m : order;
    }
    return sat_qfromdb_set(ctx, n_queries, entry, n1s.data(), sse_begin, sse, first_query_ordinal);
}

unsigned long long sat_stat_query_h2d_bytes(const sat_ctx *ctx) { return ctx ? ctx->query_h2d_bytes : 0ull; }

long long sat_debug_query_blob(sat_ctx *ctx, void *out, size_t capacity)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (ctx->queries.empty()) return sat_fail(SAT_ESTATE, "no query set");
    const auto &last = ctx->queries.back();
    const size_t bytes = last.blob_off + query_blob(last.n1p).bytes;
    if (out && capacity >= bytes) {
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipMemcpy(out, ctx->d_qblob.get(), bytes, hipMemcpyDeviceToHost));
    }
    return (long long)bytes;
}

}  // extern "C"
