/*
 * reach_check.c - a stand-alone program for the sanitizers (tests/test_reach_cpu.py builds it together with
 * csrc/host/sat_reach.c under -fsanitize=address,undefined and runs it as a child): the cases the test wrote to the file
 * named on the command line - made by numpy, never by the code under test - through sat_reach_pack / unpack / join /
 * decode, and the bad arguments.  Prints "reach_check: ok" and exits 0, or says what differs and exits 1.
 *
 * The file, native byte order: int32 n, nsets; then for the n pack cases depth int32[n], parent int32[n], p double[n],
 * key uint64[n]; then the join case keys uint64[nsets][n], support int32[nsets][n], the joined keys uint64[n] and
 * support int32[n]; then int32 count and the count rows (20 bytes each) the joined arrays decode to.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sat_reach.h"

static int fail(const char *what, long at)
{
    fprintf(stderr, "reach_check: %s at %ld\n", what, at);
    return 1;
}

static void *take(FILE *f, size_t size, size_t count)
{
    void *p = malloc(size * count + 1);
    if (!p || fread(p, size, count, f) != count) {
        fprintf(stderr, "reach_check: short file\n");
        exit(2);
    }
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 2) return fail("usage: reach_check FILE", 0);
    FILE *f = fopen(argv[1], "rb");
    if (!f) return fail("cannot open the file", 0);
    int32_t head[2];
    if (fread(head, sizeof(int32_t), 2, f) != 2 || head[0] < 1 || head[1] < 1) return fail("bad header", 0);
    const int n = head[0], nsets = head[1];
    int32_t *depth = take(f, 4, (size_t)n), *parent = take(f, 4, (size_t)n);
    double *p = take(f, 8, (size_t)n);
    uint64_t *key = take(f, 8, (size_t)n);
    uint64_t *keys = take(f, 8, (size_t)n * (size_t)nsets);
    int32_t *support = take(f, 4, (size_t)n * (size_t)nsets);
    uint64_t *want_keys = take(f, 8, (size_t)n);
    int32_t *want_support = take(f, 4, (size_t)n);
    int32_t count;
    if (fread(&count, 4, 1, f) != 1 || count < 0 || count > n) return fail("bad count", 0);
    sat_reach_rec *want_rows = take(f, sizeof(sat_reach_rec), (size_t)count);
    fclose(f);

    for (int i = 0; i < n; i++) {
        const uint64_t k = sat_reach_pack(depth[i], p[i], parent[i]);
        if (k != key[i] || sat_reach_pack_key(depth[i], p[i], parent[i]) != k) return fail("pack", i);
        int32_t d, par;
        float pv;
        sat_reach_unpack(k, &d, &par, &pv);
        const float want_p = p[i] > 0.0 ? (float)p[i] : 0.0f;
        if (d != depth[i] || par != (parent[i] < 0 ? -1 : parent[i]) || memcmp(&pv, &want_p, 4) != 0) return fail("unpack", i);
        if (k >= SAT_REACH_UNREACHED) return fail("a packed key reaches the unreached one", i);
    }
    {
        int32_t d, par;
        float pv;
        sat_reach_unpack(SAT_REACH_UNREACHED, &d, &par, &pv);
        if (d != SAT_REACH_NO_DEPTH || par != -1) return fail("unpack of the unreached key", 0);
    }

    uint64_t *out_keys = malloc(8 * (size_t)n);
    int32_t *out_support = malloc(4 * (size_t)n);
    sat_reach_rec *rows = malloc(sizeof(sat_reach_rec) * (size_t)n);
    if (!out_keys || !out_support || !rows) return fail("malloc", 0);
    if (sat_reach_join(n, nsets, keys, support, out_keys, out_support) != 0) return fail("join returned an error", 0);
    for (int v = 0; v < n; v++)
        if (out_keys[v] != want_keys[v] || out_support[v] != want_support[v]) return fail("join", v);
    if (sat_reach_decode(n, out_keys, out_support, n, rows) != count) return fail("decode's count", 0);
    for (int r = 0; r < count; r++)
        if (memcmp(&rows[r], &want_rows[r], sizeof(sat_reach_rec)) != 0) return fail("decode", r);
    /* capped: the count stays, the rows past the cap are not written */
    const int cap = count / 2;
    memset(rows, 0x5A, sizeof(sat_reach_rec) * (size_t)n);
    if (sat_reach_decode(n, out_keys, out_support, cap, rows) != count) return fail("capped decode's count", 0);
    for (int r = 0; r < cap; r++)
        if (memcmp(&rows[r], &want_rows[r], sizeof(sat_reach_rec)) != 0) return fail("capped decode", r);
    for (size_t b = sizeof(sat_reach_rec) * (size_t)cap; b < sizeof(sat_reach_rec) * (size_t)n; b++)
        if (((unsigned char *)rows)[b] != 0x5A) return fail("capped decode wrote past the cap, byte", (long)b);
    if (sat_reach_decode(n, out_keys, out_support, 0, NULL) != count) return fail("decode without rows", 0);

    /* bad arguments */
    if (sat_reach_join(0, nsets, keys, support, out_keys, out_support) != -1 || sat_reach_join(n, 0, keys, support, out_keys, out_support) != -1 ||
        sat_reach_join(n, nsets, NULL, support, out_keys, out_support) != -1 || sat_reach_join(n, nsets, keys, NULL, out_keys, out_support) != -1 ||
        sat_reach_join(n, nsets, keys, support, NULL, out_support) != -1 || sat_reach_join(n, nsets, keys, support, out_keys, NULL) != -1)
        return fail("join accepted a bad argument", 0);
    if (sat_reach_decode(0, out_keys, out_support, 0, NULL) != -1 || sat_reach_decode(SAT_REACH_NO_PARENT + 1, out_keys, out_support, 0, NULL) != -1 ||
        sat_reach_decode(n, NULL, out_support, 0, NULL) != -1 || sat_reach_decode(n, out_keys, NULL, 0, NULL) != -1 ||
        sat_reach_decode(n, out_keys, out_support, -1, rows) != -1 || sat_reach_decode(n, out_keys, out_support, 1, NULL) != -1)
        return fail("decode accepted a bad argument", 0);
    out_keys[0] = sat_reach_pack(1, 0.5, n);                /* a parent past the last node */
    if (sat_reach_decode(n, out_keys, out_support, n, rows) != -1) return fail("decode accepted a parent outside the nodes", 0);

    free(depth), free(parent), free(p), free(key), free(keys), free(support), free(want_keys), free(want_support), free(want_rows);
    free(out_keys), free(out_support), free(rows);
    printf("reach_check: ok\n");
    return 0;
}
