// sat_qfromdb.hip - queries taken from the resident database (sat_queries_from_db): a kernel expands
// entries of the shard into the query blob, byte for byte what sat_queries_set (sat_db.hip) builds on the host from the
// same entries' dense arrays - only the list of entry indices crosses from the host.
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
// minus its padded order - such a query only takes its room in the blob.
__device__ inline int code_n1p(int code, const int32_t *orders) { return code >= 0 ? query_n1p(orders[code]) : -code; }

// Each query's offset in the blob: the exclusive sum of the queries' blob sizes, input order.  One workgroup; thread t
// sums the queries t * per .. t * per + per - 1, the threads' sums are added up, and each thread walks its run again.
__global__ void __launch_bounds__(kQThreads) qfromdb_offsets(int nq, const int32_t *code, const int32_t *orders, unsigned long long *qoff)
{
    __shared__ unsigned long long part[kQThreads];
    const int t = threadIdx.x, per = (nq + kQThreads - 1) / kQThreads;
    const int q0 = t * per < nq ? t * per : nq, q1 = q0 + per < nq ? q0 + per : nq;
    unsigned long long sum = 0;
    for (int q = q0; q < q1; q++) sum += query_blob(code_n1p(code[q], orders)).bytes;
    part[t] = sum;
    __syncthreads();
    unsigned long long at = 0;
    for (int u = 0; u < t; u++) at += part[u];
    for (int q = q0; q < q1; q++) {
        qoff[q] = at;
        at += query_blob(code_n1p(code[q], orders)).bytes;
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
// Lanes run over the contiguous index of each array - column i of qdist / qcode, column k of qpair - in rows of
// 1 << wshift >= n1p lanes, the workgroup's 256 >> wshift rows side by side: 16-, 4- and 8-byte stores of consecutive
// lanes to consecutive addresses, and no lane divides.  In a row of the triangle read along i (fixed k < i) lane i is
// at dword i (i + 1) / 2 + k, and the triangular numbers of an aligned run of 32 i fall on 32 different banks.
__global__ void __launch_bounds__(kQThreads) queries_from_db(int nq, const int32_t *code, const int32_t *orders, const int64_t *cell_off,
                                                             const uint8_t *tab, const float *dist, const unsigned long long *qoff,
                                                             uint8_t *blob, unsigned long long blob_bytes)
{
    __shared__ float sdist[kTriCells];
    __shared__ uint8_t stab[(kTriCells + 15) & ~15];
    const int q = blockIdx.x, t = threadIdx.x;
    if (q >= nq) return;
    const int e = code[q];
    if (e < 0) return;                                  // another shard's: it arrives by a device copy
    const int n = orders[e], n1p = query_n1p(n), cells = n * (n + 1) / 2;
    const QueryBlob at = query_blob(n1p);
    if (n < 1 || n > SAT_MAXDIM || qoff[q] + at.bytes > blob_bytes) return;      // (checked at upload, sized by the host)
    const int64_t base = cell_off[e];
    for (int c = t; c < cells; c += kQThreads) {
        sdist[c] = dist[base + c];
        stab[c] = tab[base + c];
    }
    __syncthreads();

    uint8_t *out = blob + qoff[q];
    float4 *qdist = reinterpret_cast<float4 *>(out);
    uint32_t *qcode = reinterpret_cast<uint32_t *>(out + at.qcode);
    uint32_t *qtypes = reinterpret_cast<uint32_t *>(out + at.qtypes);
    uint2 *qpair = reinterpret_cast<uint2 *>(out + at.qpair);
    const int wshift = n1p == 16 ? 4 : (n1p == 32 ? 5 : (n1p == 64 ? 6 : 7));
    const int col = t & ((1 << wshift) - 1), row0 = t >> wshift, rows = kQThreads >> wshift;

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
// Waits for the context's stream, replaces the blob, runs the kernels on the stream and waits again.
int sat_qfromdb_set(sat_ctx *ctx, int n_queries, const int32_t *code, const int32_t *n1s, uint32_t first_query_ordinal)
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
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // from here on the old batch is gone: a failure leaves the context without queries
    ctx->queries.clear();
    ctx->desc_dirty = true;
    ctx->searched_nq = 0;
    ctx->fits.clear();
    ctx->d_qblob.reset();
    ctx->d_qdesc.reset();
    int rc;
    if ((rc = ctx->d_qblob.grow(blob_bytes)) != SAT_OK || (rc = ctx->d_qdesc.grow((size_t)n_queries)) != SAT_OK ||
        (rc = ctx->d_qentry.grow((size_t)n_queries)) != SAT_OK || (rc = ctx->d_qoff.grow((size_t)n_queries)) != SAT_OK)
        return rc;
    HIP_TRY(hipMemcpy(ctx->d_qentry.get(), code, (size_t)n_queries * sizeof(int32_t), hipMemcpyHostToDevice));
    ctx->query_h2d_bytes += (size_t)n_queries * sizeof(int32_t);
    hipLaunchKernelGGL(qfromdb_offsets, dim3(1), dim3(kQThreads), 0, ctx->stream, n_queries, ctx->d_qentry.get(), ctx->d_orders.get(),
                       ctx->d_qoff.get());
    if (hipGetLastError() != hipSuccess) return sat_fail(SAT_EDEVICE, "launch of the query offsets failed");
    hipLaunchKernelGGL(queries_from_db, dim3((unsigned)n_queries), dim3(kQThreads), 0, ctx->stream, n_queries, ctx->d_qentry.get(),
                       ctx->d_orders.get(), ctx->d_cell_off.get(), ctx->d_tab.get(), ctx->d_dist.get(), ctx->d_qoff.get(),
                       ctx->d_qblob.get(), (unsigned long long)blob_bytes);
    if (hipGetLastError() != hipSuccess) return sat_fail(SAT_EDEVICE, "launch of the query expansion failed");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->queries.swap(infos);
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
    return sat_qfromdb_set(ctx, n_queries, entry, n1s.data(), first_query_ordinal);
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
