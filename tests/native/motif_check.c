/*
 * motif_check.c - sat_parse_sse_list (csrc/host/sat_parse.c) against results written out here: the lists
 * tests/test_motif_cpu.py accepts and refuses, replayed by a stand-alone program so that the parser runs under
 * -fsanitize=address,undefined (the test builds this file with sat_parse.c and runs it as a child process).  The output
 * buffer is exactly `order` bytes of the heap, so a write past it is a report.  Prints "motif_check: ok" or the first
 * difference and exits 1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sat_parse.h"

typedef struct {
    const char *text;
    int order;
    int m;                  /* the list's length, -1: refused */
    const char *want;       /* accepted: the 1-based list, expanded, "2,1,8"; refused: a piece of the message */
} list_case;

static const list_case CASES[] = {
    { "1", 8, 1, "1" },
    { "2,1,8,5,3", 8, 5, "2,1,8,5,3" },
    { "3-7", 8, 5, "3,4,5,6,7" },
    { "1-3,9,5-6", 9, 6, "1,2,3,9,5,6" },
    { "1-8", 8, 8, "1,2,3,4,5,6,7,8" },
    { "1", 1, 1, "1" },
    { "7-7", 8, 1, "7" },
    { "0", 8, -1, "SSE 0 out of range 1..8" },
    { "9", 8, -1, "SSE 9 out of range 1..8" },
    { "3,3", 8, -1, "SSE 3 twice" },
    { "2-4,3", 8, -1, "SSE 3 twice" },
    { "5-2", 8, -1, "range 5-2 descends" },
    { "1,,2", 8, -1, "empty item" },
    { "1,", 8, -1, "empty item" },
    { "-3", 8, -1, "empty item" },
    { "1x", 8, -1, "trailing text 'x'" },
    { "", 8, -1, "empty item" },
    { "1-", 8, -1, "without its end" },
    { " 1", 8, -1, "trailing text" },
    { "1 ,2", 8, -1, "trailing text" },
    { "+1", 8, -1, "trailing text" },
    { "99999999999999999999", 8, -1, "out of range 1..8" },
    { "1-99999999999999999999", 8, -1, "SSE 9 out of range 1..8" },
};

static int fail(const list_case *c, const char *what, const char *got)
{
    printf("motif_check: '%s' (order %d): %s, got '%s', want '%s'\n", c->text, c->order, what, got, c->want);
    return 1;
}

static int check(const list_case *c)
{
    uint8_t *out = malloc((size_t)c->order);
    char err[128] = "", text[1024] = "";
    const int m = sat_parse_sse_list(c->text, c->order, out, err, sizeof err);
    int bad = 0;
    if (m != c->m) {
        snprintf(text, sizeof text, "%d", m);
        bad = fail(c, "the length", text);
    } else if (m < 0) {
        if (!strstr(err, c->want))
            bad = fail(c, "the message", err);
    } else {
        size_t len = 0;
        for (int i = 0; i < m; i++)
            len += (size_t)snprintf(text + len, sizeof text - len, i ? ",%d" : "%d", out[i] + 1);
        if (strcmp(text, c->want))
            bad = fail(c, "the list", text);
    }
    free(out);
    return bad;
}

int main(void)
{
    for (size_t k = 0; k < sizeof CASES / sizeof CASES[0]; k++)
        if (check(&CASES[k]))
            return 1;
    /* the whole of the largest order as one range, and as 111 numbers back to front */
    char text[1024];
    size_t len = 0;
    for (int v = SAT_MAXDIM; v >= 1; v--)
        len += (size_t)snprintf(text + len, sizeof text - len, v < SAT_MAXDIM ? ",%d" : "%d", v);
    uint8_t *out = malloc(SAT_MAXDIM);
    char err[128];
    if (sat_parse_sse_list("1-111", SAT_MAXDIM, out, err, sizeof err) != SAT_MAXDIM || out[0] != 0 || out[110] != 110 ||
        sat_parse_sse_list(text, SAT_MAXDIM, out, err, sizeof err) != SAT_MAXDIM || out[0] != 110 || out[110] != 0) {
        printf("motif_check: the full lists of order %d\n", SAT_MAXDIM);
        return 1;
    }
    /* 112 numbers: one more than any entry has - the 112th is out of range, or one of 1..111 is there twice */
    snprintf(text + len, sizeof text - len, ",112");
    if (sat_parse_sse_list(text, SAT_MAXDIM, out, err, sizeof err) != -1 || !strstr(err, "SSE 112 out of range 1..111")) {
        printf("motif_check: 112 numbers: %s\n", err);
        return 1;
    }
    snprintf(text + len, sizeof text - len, ",57");
    if (sat_parse_sse_list(text, SAT_MAXDIM, out, err, sizeof err) != -1 || !strstr(err, "SSE 57 twice")) {
        printf("motif_check: 112 numbers: %s\n", err);
        return 1;
    }
    if (sat_parse_sse_list("1", 0, out, err, sizeof err) != -1 || sat_parse_sse_list("1", SAT_MAXDIM + 1, out, err, sizeof err) != -1) {
        printf("motif_check: an order outside 1..%d was taken\n", SAT_MAXDIM);
        return 1;
    }
    free(out);
    printf("motif_check: ok\n");
    return 0;
}
