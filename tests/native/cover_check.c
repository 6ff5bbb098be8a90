/*
 * cover_check.c - the host side of the greedy cover (csrc/host/sat_cover.c) under the sanitizers: tests/test_cover_cpu.py
 * builds this file and sat_cover.c with gcc -fsanitize=address,undefined and runs the program.  It replays the named
 * graphs of the tests against tables written out here, walks the word edges of the bit matrix (63, 64, 65, 129 nodes)
 * and hands the functions their bad arguments.  Prints "cover_check: ok" and returns 0, or says what differs.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sat_cover.h"

static int failures;

#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "cover_check: " __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

typedef struct {
    const char *name;
    int n, pairs;
    int32_t a[16], b[16];
    int rounds, clusters;
    int32_t rep[8], size[8], degree[8];
} named;

static const named graphs[] = {
    /* gains 2 3 3 2: nodes 1 and 2 tie, the smaller takes {0, 1, 2}; node 3 is left alone */
    { "path of 4", 4, 3, { 0, 1, 2 }, { 1, 2, 3 }, 1, 2, { 1, 1, 1, 3 }, { 3, 3, 3, 1 }, { 1, 2, 2, 1 } },
    { "star", 6, 5, { 5, 5, 5, 5, 5 }, { 0, 1, 2, 3, 4 }, 1, 1, { 5, 5, 5, 5, 5, 5 }, { 6, 6, 6, 6, 6, 6 }, { 1, 1, 1, 1, 1, 5 } },
    /* hubs 0 (leaves 2 3 4 5) and 1 (leaves 2 3 4 6 7): 1 has the larger gain, goes first and takes the shared leaves */
    { "two stars sharing leaves", 8, 9, { 0, 0, 0, 0, 1, 1, 1, 1, 1 }, { 2, 3, 4, 5, 2, 3, 4, 6, 7 }, 2, 2,
      { 0, 1, 1, 1, 1, 0, 1, 1 }, { 2, 6, 6, 6, 6, 2, 6, 6 }, { 4, 5, 2, 2, 2, 1, 1, 1 } },
    { "clique", 5, 10, { 0, 0, 0, 0, 1, 1, 1, 2, 2, 3 }, { 1, 2, 3, 4, 2, 3, 4, 3, 4, 4 }, 1, 1,
      { 0, 0, 0, 0, 0 }, { 5, 5, 5, 5, 5 }, { 4, 4, 4, 4, 4 } },
    { "perfect matching", 6, 3, { 1, 3, 5 }, { 0, 2, 4 }, 3, 3, { 0, 0, 2, 2, 4, 4 }, { 2, 2, 2, 2, 2, 2 }, { 1, 1, 1, 1, 1, 1 } },
    { "no edges", 3, 0, { 0 }, { 0 }, 0, 3, { 0, 1, 2 }, { 1, 1, 1 }, { 0, 0, 0 } },
    { "self pairs and repeated pairs only", 4, 5, { 2, 1, 0, 3, 0 }, { 2, 1, 3, 0, 3 }, 1, 3, { 0, 1, 2, 0 }, { 2, 1, 1, 2 }, { 1, 0, 0, 1 } },
};

static void replay(const named *g)
{
    int32_t rep[8], size[8], degree[8];
    const int rounds = sat_cover_greedy(g->n, g->pairs, g->a, g->b, rep, degree);
    CHECK(rounds == g->rounds, "%s: %d rounds, expected %d", g->name, rounds, g->rounds);
    CHECK(!memcmp(rep, g->rep, sizeof(int32_t) * (size_t)g->n), "%s: representatives differ", g->name);
    CHECK(!memcmp(degree, g->degree, sizeof(int32_t) * (size_t)g->n), "%s: degrees differ", g->name);
    const int clusters = sat_cover_sizes(g->n, rep, size);
    CHECK(clusters == g->clusters, "%s: %d clusters, expected %d", g->name, clusters, g->clusters);
    CHECK(!memcmp(size, g->size, sizeof(int32_t) * (size_t)g->n), "%s: sizes differ", g->name);
    /* the pairs reversed and dealt twice: the same edge set, the same result; no degrees asked for */
    int32_t a2[32], b2[32], rep2[8];
    for (int i = 0; i < g->pairs; i++) {
        a2[i] = g->b[i], b2[i] = g->a[i];
        a2[g->pairs + i] = g->a[i], b2[g->pairs + i] = g->b[i];
    }
    CHECK(sat_cover_greedy(g->n, 2 * g->pairs, a2, b2, rep2, NULL) == g->rounds, "%s: rounds differ for the doubled pairs", g->name);
    CHECK(!memcmp(rep2, g->rep, sizeof(int32_t) * (size_t)g->n), "%s: representatives differ for the doubled pairs", g->name);
}

/* n nodes: the last node against every other (its bit is the last valid one of the last word), then a path as well */
static void word_edges(int n)
{
    int32_t *a = malloc(sizeof(int32_t) * 2 * (size_t)n), *b = malloc(sizeof(int32_t) * 2 * (size_t)n);
    int32_t *rep = malloc(sizeof(int32_t) * (size_t)n), *degree = malloc(sizeof(int32_t) * (size_t)n), *size = malloc(sizeof(int32_t) * (size_t)n);
    if (!a || !b || !rep || !degree || !size)
        exit(2);
    int pairs = 0;
    for (int i = 0; i + 1 < n; i++)
        a[pairs] = n - 1, b[pairs++] = i;
    int rounds = sat_cover_greedy(n, pairs, a, b, rep, degree);
    CHECK(rounds == (n > 1), "star of %d: %d rounds", n, rounds);
    const int hub = n == 2 ? 0 : n - 1;                         /* two nodes tie: the smaller index */
    for (int v = 0; v < n; v++) {
        CHECK(rep[v] == hub, "star of %d: node %d has representative %d", n, v, rep[v]);
        CHECK(degree[v] == (v == n - 1 ? n - 1 : 1), "star of %d: node %d has degree %d", n, v, degree[v]);
    }
    CHECK(sat_cover_sizes(n, rep, size) == 1 && size[0] == n, "star of %d: sizes", n);
    /* the path 0 - 1 - ... - n - 1 alone: node 1 takes {0, 1, 2}, node 4 {3, 4, 5}, ...; the tail is a pair or a singleton */
    pairs = 0;
    for (int i = 0; i + 1 < n; i++)
        a[pairs] = i + 1, b[pairs++] = i;
    rounds = sat_cover_greedy(n, pairs, a, b, rep, degree);
    for (int v = 0; v < n; v++) {
        const int block = v / 3, left = n - 3 * block;          /* nodes from this block's first one on */
        const int want = left >= 3 ? 3 * block + 1 : 3 * block;  /* a full block's middle; a tail's first node */
        CHECK(rep[v] == want, "path of %d: node %d has representative %d, expected %d", n, v, rep[v], want);
    }
    CHECK(rounds == n / 3 + (n % 3 == 2), "path of %d: %d rounds", n, rounds);
    free(a), free(b), free(rep), free(degree), free(size);
}

static void bad_arguments(void)
{
    int32_t a[2] = { 0, 1 }, b[2] = { 1, 2 }, rep[3], degree[3], size[3];
    CHECK(sat_cover_greedy(0, 0, a, b, rep, degree) == -1, "n = 0 accepted");
    CHECK(sat_cover_greedy(3, -1, a, b, rep, degree) == -1, "n_pairs < 0 accepted");
    CHECK(sat_cover_greedy(3, 2, NULL, b, rep, degree) == -1, "a = NULL accepted");
    CHECK(sat_cover_greedy(3, 2, a, NULL, rep, degree) == -1, "b = NULL accepted");
    CHECK(sat_cover_greedy(3, 2, a, b, NULL, degree) == -1, "rep = NULL accepted");
    CHECK(sat_cover_greedy(2, 2, a, b, rep, degree) == -1, "a node outside 0 .. n - 1 accepted");
    a[0] = -1;
    CHECK(sat_cover_greedy(3, 2, a, b, rep, degree) == -1, "a negative node accepted");
    CHECK(sat_cover_greedy(3, 0, NULL, NULL, rep, NULL) == 0 && rep[0] == 0 && rep[2] == 2, "no pairs, null lists refused");
    const int32_t good[3] = { 1, 1, 2 }, chain[3] = { 1, 2, 2 }, outside[3] = { 0, 3, 2 }, negative[3] = { 0, -1, 2 };
    CHECK(sat_cover_sizes(3, good, size) == 2 && size[0] == 2 && size[1] == 2 && size[2] == 1, "sizes of a good table");
    CHECK(sat_cover_sizes(3, chain, size) == -1, "rep[rep[v]] != rep[v] accepted");
    CHECK(sat_cover_sizes(3, outside, size) == -1, "a representative outside 0 .. n - 1 accepted");
    CHECK(sat_cover_sizes(3, negative, size) == -1, "a negative representative accepted");
    CHECK(sat_cover_sizes(0, good, size) == -1 && sat_cover_sizes(3, NULL, size) == -1 && sat_cover_sizes(3, good, NULL) == -1, "bad sizes arguments accepted");
    /* the layout and the key the device shares */
    CHECK(sat_cover_stride(1) == 1 && sat_cover_stride(64) == 1 && sat_cover_stride(65) == 2, "stride");
    CHECK(sat_cover_valid(65, 0) == ~0ull && sat_cover_valid(65, 1) == 1ull && sat_cover_valid(64, 1) == 0ull && sat_cover_valid(63, 0) == ~0ull >> 1, "valid bits");
    CHECK(sat_cover_key(3, 7) > sat_cover_key(3, 8) && sat_cover_key(4, 8) > sat_cover_key(3, 7) && sat_cover_key(1, 2147483647) > 0ull, "key order");
    CHECK(sat_cover_key_gain(sat_cover_key(5, 9)) == 5 && sat_cover_key_node(sat_cover_key(5, 9)) == 9, "key fields");
}

int main(void)
{
    for (size_t i = 0; i < sizeof graphs / sizeof graphs[0]; i++)
        replay(&graphs[i]);
    const int sizes[] = { 1, 2, 3, 63, 64, 65, 128, 129, 200 };
    for (size_t i = 0; i < sizeof sizes / sizeof sizes[0]; i++)
        word_edges(sizes[i]);
    bad_arguments();
    if (failures)
        return 1;
    printf("cover_check: ok\n");
    return 0;
}
