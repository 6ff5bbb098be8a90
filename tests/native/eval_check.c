/*
 * eval_check.c - a stand-alone check of the host side of -E under the sanitizers (tests/test_eval_cpu.py builds it with
 * gcc -fsanitize=address,undefined from this file, csrc/host/sat_eval.c and csrc/host/sat_parse.c, and runs it with a
 * scratch directory as its argument):
 *   - sat_eval_reduce on tie-free listings against the definition the reference's evaluation states for them - for
 *     every negative the number of positives ranked above it, summed - counted here pair by pair, and ROC-n as the same
 *     count over the first n negatives from the top;
 *   - sat_read_classes on good files, a duplicated name, over-long tokens, a file without a trailing newline, an
 *     empty file and a missing one.
 * Prints "eval_check: ok" and returns 0, or says what differed and returns 1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sat_eval.h"
#include "sat_parse.h"

static int failures = 0;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "eval_check: " __VA_ARGS__); fprintf(stderr, "\n"); failures++; } } while (0)

/* a small generator of its own: the check needs no particular stream */
static uint32_t rng_state = 12345u;
static uint32_t rng(void)
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static void check_tie_free(int bins, int rocn)
{
    /* every score 0 .. bins - 1 is taken by at most one row, a positive or a negative */
    uint32_t *pos = calloc((size_t)bins, sizeof *pos), *neg = calloc((size_t)bins, sizeof *neg);
    for (int b = 0; b < bins; b++) {
        const uint32_t kind = rng() % 3;
        pos[b] = kind == 1;
        neg[b] = kind == 2;
    }
    unsigned long long above_all = 0, above_first = 0;
    int negatives = 0, positives = 0, seen = 0;
    for (int b = bins - 1; b >= 0; b--) {
        positives += (int)pos[b];
        if (!neg[b])
            continue;
        negatives++;
        unsigned long long above = 0;
        for (int a = b + 1; a < bins; a++)
            above += pos[a];
        above_all += above;
        if (seen++ < rocn)
            above_first += above;
    }
    sat_eval_row row;
    row.query_class = 77;
    CHECK(sat_eval_reduce(pos, neg, bins, rocn, &row) == 0, "reduce failed (bins %d)", bins);
    CHECK(row.u2 == 2 * above_all, "bins %d: u2 = %llu, pair count %llu", bins, (unsigned long long)row.u2, above_all);
    CHECK(row.t2 == 2 * above_first, "bins %d rocn %d: t2 = %llu, pair count %llu", bins, rocn, (unsigned long long)row.t2, above_first);
    CHECK(row.positives == positives && row.negatives == negatives, "bins %d: %d / %d rows", bins, row.positives, row.negatives);
    CHECK(row.n_used == (rocn < negatives ? rocn : negatives), "bins %d: n_used = %d", bins, row.n_used);
    CHECK(row.query_class == 77, "query_class was touched");
    free(pos);
    free(neg);
}

static void write_file(const char *path, const char *text, size_t len)
{
    FILE *fp = fopen(path, "w");
    if (!fp || fwrite(text, 1, len, fp) != len) {
        fprintf(stderr, "eval_check: cannot write %s\n", path);
        exit(2);
    }
    fclose(fp);
}

int main(int argc, char *argv[])
{
    if (argc != 2) {
        fprintf(stderr, "usage: eval_check scratch-directory\n");
        return 2;
    }
    for (int round = 0; round < 200; round++)
        check_tie_free(1 + (int)(rng() % 300), 1 + (int)(rng() % 60));
    check_tie_free(1, 1);
    check_tie_free(24421, 50);
    {
        uint32_t one = 1;
        sat_eval_row row;
        CHECK(sat_eval_reduce(NULL, &one, 1, 1, &row) == -1 && sat_eval_reduce(&one, &one, 0, 1, &row) == -1 &&
              sat_eval_reduce(&one, &one, 1, 0, &row) == -1 && sat_eval_reduce(&one, &one, 1, 1, NULL) == -1, "bad arguments pass");
        uint32_t big[2] = { 0x7FFFFFFFu, 1u };
        CHECK(sat_eval_reduce(big, big, 2, 1, &row) == -1, "2^31 rows a side pass");
    }

    /* a database of six one-SSE structures; d1abca_ twice */
    sat_struct_set db;
    sat_set_init(&db);
    const char *names[6] = { "d1abca_", "d1abcb_", "D2XYZA1", "d3foo__", "d1abca_", "d9zzzz_" };
    const uint8_t tab = 0;
    const float dist = 0.0f;
    for (int s = 0; s < 6; s++)
        if (sat_set_append(&db, names[s], 1, &tab, &dist) != s)
            return 2;
    char path[4096], err[512];
    sat_classes cl;

    snprintf(path, sizeof path, "%s/good.classes", argv[1]);
    const char *good = "# a comment\n\n  d1abcb_   a.1.1\t trailing words\nd2xyza1\tb.2\n   # another\nd1abca_ a.1.1\nnobody c.3\n\r\nd9zzzz_ b.2\n";
    write_file(path, good, strlen(good));
    CHECK(sat_read_classes(path, &db, &cl, err, sizeof err) == 0, "good file refused: %s", err);
    CHECK(cl.entries == 6 && cl.distinct == 2 && cl.classified == 5 && cl.unknown == 1, "good file: %d %d %d %d", cl.entries, cl.distinct,
          cl.classified, cl.unknown);
    if (cl.node_class) {
        const int32_t want[6] = { 0, 0, 1, -1, 0, 1 };
        CHECK(memcmp(cl.node_class, want, sizeof want) == 0, "good file: classes differ");
        CHECK(!strcmp(cl.token[0], "a.1.1") && !strcmp(cl.token[1], "b.2"), "good file: tokens differ");
    }
    sat_classes_free(&cl);

    /* the same without the last newline; then many classes, so that the token table grows */
    write_file(path, good, strlen(good) - 1);
    CHECK(sat_read_classes(path, &db, &cl, err, sizeof err) == 0 && cl.classified == 5 && cl.node_class[5] == 1, "no trailing newline: %s", err);
    sat_classes_free(&cl);
    {
        sat_struct_set many;
        sat_set_init(&many);
        char name[16], *text = malloc(1000 * 32);
        size_t len = 0;
        for (int s = 0; s < 1000; s++) {
            snprintf(name, sizeof name, "s%06d", s);
            if (sat_set_append(&many, name, 1, &tab, &dist) != s)
                return 2;
            len += (size_t)sprintf(text + len, "%s class%d\n", name, s % 333);
        }
        write_file(path, text, len);
        CHECK(sat_read_classes(path, &many, &cl, err, sizeof err) == 0 && cl.distinct == 333 && cl.classified == 1000 &&
              cl.node_class[999] == 0 && cl.node_class[332] == 332 && !strcmp(cl.token[332], "class332"), "many classes: %s", err);
        sat_classes_free(&cl);
        sat_set_free(&many);
        free(text);
    }

    snprintf(path, sizeof path, "%s/twice.classes", argv[1]);
    const char *twice = "d1abcb_ a\nd3foo__ b\nD1ABCB_ c\n";
    write_file(path, twice, strlen(twice));
    CHECK(sat_read_classes(path, &db, &cl, err, sizeof err) == -1, "a name listed twice passes");
    CHECK(strstr(err, "line 3") && strstr(err, "listed twice") && strstr(err, "line 1"), "a name listed twice: '%s'", err);
    CHECK(cl.node_class == NULL && cl.token == NULL && cl.distinct == 0, "a refused file leaves something behind");

    snprintf(path, sizeof path, "%s/noclass.classes", argv[1]);
    write_file(path, "d1abcb_ a\nd3foo__   \n", 21);
    CHECK(sat_read_classes(path, &db, &cl, err, sizeof err) == -1 && strstr(err, "line 2"), "a line without a class: '%s'", err);

    /* tokens far longer than any buffer: a name of 100 000 characters is no entry's, a class of 100 000 is a class */
    snprintf(path, sizeof path, "%s/long.classes", argv[1]);
    {
        const size_t big = 100000;
        char *text = malloc(3 * big + 64);
        size_t len = 0;
        memset(text + len, 'n', big); len += big;
        len += (size_t)sprintf(text + len, " a.1\nd3foo__ ");
        memset(text + len, 'c', big); len += big;
        len += (size_t)sprintf(text + len, "\nd9zzzz_ a.1\n");
        memset(text + len, 'x', big); len += big;              /* and a last line that is one long name without a class */
        write_file(path, text, len - big);
        CHECK(sat_read_classes(path, &db, &cl, err, sizeof err) == 0 && cl.unknown == 1 && cl.classified == 2 && cl.distinct == 2 &&
              strlen(cl.token[0]) == big && cl.node_class[3] == 0 && cl.node_class[5] == 1, "over-long tokens: %s", err);
        sat_classes_free(&cl);
        write_file(path, text, len);
        CHECK(sat_read_classes(path, &db, &cl, err, sizeof err) == -1 && strstr(err, "line 4") && strlen(err) < sizeof err - 1,
              "an over-long name without a class: '%s'", err);
        free(text);
    }

    snprintf(path, sizeof path, "%s/empty.classes", argv[1]);
    write_file(path, "", 0);
    CHECK(sat_read_classes(path, &db, &cl, err, sizeof err) == 0 && cl.distinct == 0 && cl.classified == 0 && cl.unknown == 0 &&
          cl.node_class && cl.node_class[0] == -1 && cl.node_class[5] == -1, "empty file: %s", err);
    sat_classes_free(&cl);

    snprintf(path, sizeof path, "%s/missing.classes", argv[1]);
    CHECK(sat_read_classes(path, &db, &cl, err, sizeof err) == -1 && strstr(err, "cannot open"), "a missing file: '%s'", err);

    sat_set_free(&db);
    if (failures)
        return 1;
    printf("eval_check: ok\n");
    return 0;
}
