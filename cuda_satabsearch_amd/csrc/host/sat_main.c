/*
 * sat_main.c - the `satabsearch` command line: drop-in for `cudaSaTabsearch`.
 *
 * Same options, stdin grammar and stdout bytes as the reference's main
 * (nvcc_src_current/cudaSaTabsearch.cu): options -c -q -r :605-626; "-q" SID list
 * :631-664 (SIDs cut to 7 chars, options fixed T T F); inline mode header :667-694;
 * LTYPE forced to T :696-700; SID lookup small class first :746-780; output = all
 * queries over the small class (order <= 96), then all queries over the large class
 * (97..111), three '#' header lines per (query, class) :1027-1030, rows :1102-1114 and
 * :1255-1268 (the large pass of the GPU path prints two blanks before the p-value).
 *
 * Host code is plain C; the search itself goes through the C ABI of
 * include/satabsearch.h (HIP kernel).  The reference is single-GPU (its TODO, :790);
 * here the database is sharded contiguously, by cost, over the visible GPUs (-g N) behind
 * the sat_multi_* entry points: launch on all, one RCCL gather to device 0, one copy to
 * the host, rows in file order.  Results do not depend on N (the random streams are keyed
 * by db ordinal).
 *
 * -c selects the host mode (csrc/host/sat_host_search.c): one CPU thread, one
 * sequential drand48 stream, byte-identical to the reference's -c.  It is never a
 * fallback: without -c a missing GPU is an error.
 *
 * Extensions: -g N (GPUs to use; default 1 as the reference, 0 = all visible), -G 0,2,3 (which GPUs; a GPU named twice
 * holds two shards), -s SEED (Philox seed, default 1234),
 * -k K (print only the K best rows per query, ranked on the GPU by raw score, ties in
 * database order - the `sort -k 2,2nr | head` users run on the reference's output),
 * -b (keep a binary image `dbfile.satbin` beside the database and load it instead of
 * parsing when it is newer than the ASCII file), -p P (print only the rows whose p-value is <= P, selected on the
 * GPU and ranked as -k; with -k K at most K of them per query), -M M (matches 2..M of the rows that -k / -p / -R print,
 * in -m's format: a pair-match search of those rows only, after the search that chose them), -F censor (fit each
 * query's Gumbel parameters to its own scores and print z and p from the fit: a fourth header line "# GUMBEL ...", see
 * sat_gumbel.h; the listing fits on the host, -k / -p on the GPUs from a histogram, so that still only the printed rows
 * leave them), -P T (polish: the rows of -k K are the K best of each query's C best entries after the own-best maps of
 * every candidate's T best restarts were climbed to local optima of the search's neighbourhood on the GPU; a fourth header
 * line "# POLISH ..."), -A (with -P T: polish EVERY row of the search - the whole-database mode of the library - and take
 * the ordinary route of the other options on the polished rows: the listing, -k, -p, -F; "# POLISH tops = T all rows"),
 * -Q dbfile (as -q dbfile, same stdout: the queries are entries of the database, which is resident on the GPUs, so each
 * batch is set from its entry indices and built there - sat_multi_queries_from_db - instead of being expanded on the host
 * and copied), -a dbfile (all-vs-all: every entry of the database is a query, in file order, set as -Q sets them; stdin
 * is not read; prints what -q dbfile prints for a stdin that lists every SID in file order), -L P (with -a dbfile: cluster
 * the database - single linkage over the rows whose p-value is <= P, the graph kept on the GPUs, sat_cluster.h - and print
 * one line per structure, "name representative cluster_size degree", under a "# CLUSTER ..." header instead of any rows),
 * -H P1,..,PL (-L at 1..8 ascending cutoffs from ONE all-vs-all run: a "# LEVEL j ..." line per cutoff and, per structure,
 * -L Pj's three columns for every j side by side; the clusterings are nested), -E classfile [-N n] (with -a dbfile or
 * -Q dbfile: score the search against a classification - per query the AUC and the ROC-n, default n = 50, of its ranking
 * of the classified structures, from two score histograms made and reduced on the GPUs, sat_eval.h: 32 bytes a query come
 * back, and one line per query is printed, "name class positives negatives u2 t2 n_used auc rocn", under "# EVAL ..." and
 * "# MEAN ..." instead of any rows), -D P (with -a dbfile: cluster the database around representatives - a greedy cover of
 * the graph of the rows whose p-value is <= P, kept as a bit matrix and solved on the GPUs, sat_cover.h: every structure is
 * a direct hit of its representative - and print -L's four columns, the degree counting distinct neighbours, under a
 * "# COVER ..." header), -W P [-f F] (profile each query's SSEs over its hits: every batch is searched with LSOLN on,
 * its rows and maps stay on the GPUs, and sat_multi_profile_rows counts there, per query, the rows whose p-value is <= P
 * - the query's own entry apart - and for every pair of the query's SSEs those whose map matches both; 4 + 4 n1 n1 bytes a
 * query come back.  Under a "# PROFILE ..." header each query gets "# QUERY name sses = n1 hits = H", its conserved core
 * "# CORE sses = c joint >= J name@list" - sat_profile.h: SSEs every two of which are matched together in at least F,
 * default 0.5, of the hits; the text after J is a SID@list line for -q / -Q - and n1 lines "i type matched joint_i1 ..
 * joint_in1" instead of any rows), -X B [-x kinds] with -p P (hits out of sequence order: every batch is searched twice on
 * the GPUs, in order without maps and - kept on the device as the baseline - out of order with maps, whatever the input's
 * LORDER and LSOLN say; sat_multi_reorder_hits then selects, of -p P's rows of the second search, those whose ordered
 * p-value is >= B and whose map is of one of the kinds - s sequential, c circular, n not sequential otherwise; default
 * cn, sat_reorder.h - and each block, under one more header line "# REORDER ordered pvalue >= B kinds = cn", lists only
 * those rows, with six more columns: ordered_raw ordered_pvalue kind(seq|circ|perm) matched descents cut).
 * Motif queries: with -q dbfile and -Q dbfile a stdin line may be SID@list, the list (sat_parse_sse_list: 2,1,8,5,3 or
 * 1-3,9 - 1-based, as pytableaucreate.py -s takes it, but kept in the order given) naming the SSEs of that entry the
 * query is made of.  The block gets a header line "# QUERY SSES = 2,1,8,5,3" after "# DBFILE" and is otherwise printed
 * as for a stand-alone query structure of the list's length; -Q builds such a batch on the GPUs
 * (sat_multi_queries_from_db_sses), -q cuts the sub-arrays on the host.
 */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include "satabsearch.h"
#include "sat_cluster.h"
#include "sat_cover.h"
#include "sat_gumbel.h"
#include "sat_host_search.h"
#include "sat_parse.h"
#include "sat_profile.h"


static double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

/* The sanitizer build of the host code links this file against stubs of the device library
 * (tests/native/gpu_stubs.c) that have no several-matches, refine, cutoff or pair-match entry point: weak references
 * keep that link working, and -m / -R / -p / -M report the missing entry point instead of calling it. */
#pragma weak sat_multi_search_matches
#pragma weak sat_multi_search_refine
#pragma weak sat_multi_search_cutoff
#pragma weak sat_multi_hits_cutoff
#pragma weak sat_multi_search_pairs_matches
#pragma weak sat_multi_search_fit
#pragma weak sat_multi_search_refine_polish
#pragma weak sat_multi_polish_all_set
#pragma weak sat_multi_queries_from_db
#pragma weak sat_multi_queries_from_db_sses
#pragma weak sat_multi_search_only
#pragma weak sat_multi_cluster_begin
#pragma weak sat_multi_cluster_add
#pragma weak sat_multi_cluster_labels
#pragma weak sat_cluster_reps
#pragma weak sat_multi_cluster_begin_levels
#pragma weak sat_multi_cluster_add_levels
#pragma weak sat_multi_cluster_labels_levels
#pragma weak sat_cluster_nested
#pragma weak sat_multi_cover_begin
#pragma weak sat_multi_cover_add
#pragma weak sat_multi_cover_solve
#pragma weak sat_cover_sizes
#pragma weak sat_multi_eval_classes
#pragma weak sat_multi_eval_rows
#pragma weak sat_multi_profile_rows
#pragma weak sat_profile_core
#pragma weak sat_multi_baseline_keep
#pragma weak sat_multi_reorder_hits

static void usage(const char *prog)
{
    fprintf(stderr, "Usage: %s [-c] [-q dbfile | -Q dbfile | -a dbfile] [-r restarts] [-g gpus] [-G gpu,gpu,...] [-s seed]\n"
                    "       [-k K] [-p P] [-m M] [-M M] [-R restarts [-C C]] [-F censor] [-P T] [-A] [-L P] [-b] [-H P1,P2,...]\n"
                    "       [-E classfile [-N n]] [-D P]\n"
                    "       [-W P [-f F]]\n"
                    "       [-X B [-x kinds]]\n", prog);
    fprintf(stderr, "  -c : run on host CPU not GPU card\n");
    fprintf(stderr, "  -q dbfile : database is read from dbfile, list of query\n"
                    "              ids is read from stdin\n");
    fprintf(stderr, "  -Q dbfile : as -q dbfile, same output; the queries are built on the GPU from the resident\n"
                    "              database instead of on the host (GPU mode)\n");
    fprintf(stderr, "  SID@list : (-q, -Q) a stdin line may name a motif: the listed SSEs of the entry, 1-based, commas and\n"
                    "              ranges, in the order given, e.g. d1ubia_@2,1,8,5,3 or d1ubia_@1-3,5 (header line # QUERY SSES);\n"
                    "              such a line holds at most %d characters, and may end in CR LF\n", SAT_MAX_LINE_LEN - 2);
    fprintf(stderr, "  -a dbfile : all-vs-all: every entry of dbfile is a query, in file order, built as with -Q;\n"
                    "              stdin is not read (GPU mode)\n");
    fprintf(stderr, "  -r restarts : number of restarts. Default %d\n", 128);
    fprintf(stderr, "  -g gpus : number of GPUs to shard the database over (0 = all visible). Default 1\n");
    fprintf(stderr, "  -G list : the GPUs to use, e.g. 0,2,3 (a GPU named twice holds two shards)\n");
    fprintf(stderr, "  -s seed : seed of the GPU random streams. Default %d\n", SAT_DEFAULT_SEED);
    fprintf(stderr, "  -k K : print only the K best rows per query (GPU mode)\n");
    fprintf(stderr, "  -p P : print only rows whose p-value is <= P, ranked as -k (GPU mode)\n");
    fprintf(stderr, "  -m M : up to M (1..%d) non-overlapping matches per structure: after an entry's row,\n"
                    "         matches 2..M as rows named name:k (GPU mode)\n", SAT_MAX_MATCHES);
    fprintf(stderr, "  -M M : as -m for the rows that -k, -p or -R print only: matches 2..M (1..%d) of each printed\n"
                    "         row as rows named name:k, found by a search of those rows alone; with -R at its\n"
                    "         restarts (GPU mode, needs -k or -p)\n", SAT_MAX_MATCHES);
    fprintf(stderr, "  -R restarts : re-score each query's C best entries (by -r) with this many restarts;\n"
                    "                rows as -k, with the new scores (GPU mode, needs -k)\n");
    fprintf(stderr, "  -C C : candidates per query re-scored by -R. Default K\n");
    fprintf(stderr, "  -F censor : fit each query's Gumbel parameters to its own scores, the top `censor` (0..0.5) of them\n"
                    "              right-censored; z and p come from the fit (header line # GUMBEL)\n");
    fprintf(stderr, "  -P T : polish: rank each query's C best entries (-C, default K) after the maps of their T (1..%d)\n"
                    "         best restarts (of -R restarts, default -r) were climbed to local optima; rows as -k, with\n"
                    "         the polished scores and maps (GPU mode, needs -k)\n", SAT_MAX_MATCHES);
    fprintf(stderr, "  -A : with -P T: all rows - polish every row of the search instead of C candidates; the listing, -k, -p\n"
                    "       and -F then work on the polished scores and maps (not with -c, -m, -M, -R, -C)\n");
    fprintf(stderr, "  -L P : with -a dbfile: cluster the database on the GPU - single linkage over the rows whose p-value\n"
                    "         is <= P (0..1); prints one line per structure: name representative cluster_size degree\n"
                    "         (not with -c, -k, -p, -m, -M, -R, -C)\n");
    fprintf(stderr, "  -H P1,P2,... : with -a dbfile: cluster the database at 1..%d ascending p-values (each 0..1) in ONE run - the\n"
                    "         clusterings of -L P1, -L P2, ... from one all-vs-all search, nested; prints a line per cutoff\n"
                    "         (# LEVEL j pvalue <= Pj clusters singletons edges) and one line per structure:\n"
                    "         name, then representative cluster_size degree for every level\n"
                    "         (not with -c, -L, -k, -p, -m, -M, -R, -C)\n", SAT_MAX_CLUSTER_LEVELS);
    fprintf(stderr, "  -E classfile : with -a dbfile or -Q dbfile: score the search against a classification on the GPU - classfile\n"
                    "         lists 'name class' per line (# comments; unlisted structures are unclassified); prints one line\n"
                    "         per query: name class positives negatives u2 t2 n_used auc rocn, where auc = u2 / (2 positives\n"
                    "         negatives) and rocn = t2 / (2 positives n_used) rank the classified structures other than the\n"
                    "         query itself by raw score, ties counted half (not with -c, -k, -p, -m, -M, -R, -C, -F, -L, -H)\n");
    fprintf(stderr, "  -N n : with -E: the negatives ROC-n counts up to (n >= 1). Default 50\n");
    fprintf(stderr, "  -D P : with -a dbfile: cluster the database around representatives on the GPU - a greedy cover of the graph\n"
                    "         of the rows whose p-value is <= P (0..1): every structure is a direct hit of its representative\n"
                    "         and no two representatives are hits of each other; prints one line per structure:\n"
                    "         name representative cluster_size degree, the degree counting distinct neighbours\n"
                    "         (not with -c, -k, -p, -m, -M, -R, -C, -L, -H, -E)\n");
    fprintf(stderr, "  -W P : which SSEs: profile each query's SSEs over its hits on the GPU - the rows whose p-value is <= P\n"
                    "         (0..1), the query's own entry apart; prints per query its hits, its conserved core as a SID@list\n"
                    "         line (# CORE) and one line per SSE: i type matched joint_i1 .. joint_in1, the hits that match SSE i\n"
                    "         and those that match SSE i and SSE k together; no rows, no maps\n"
                    "         (not with -c, -k, -p, -m, -M, -R, -C, -L, -H, -D, -E, -N)\n");
    fprintf(stderr, "  -f F : with -W: every two SSEs of the core are matched together in at least F (0 < F <= 1) of the hits.\n"
                    "         Default 0.5\n");
    fprintf(stderr, "  -X B : with -p P: only the hits that need a match out of sequence order - every query is searched in order\n"
                    "         and out of order (whatever LORDER and LSOLN say), and of -p's rows of the second search those are\n"
                    "         printed whose ordered p-value is >= B (0..1) and whose map is of one of -x's kinds; six more columns\n"
                    "         a row: ordered_raw ordered_pvalue kind(seq|circ|perm) matched descents cut; use -F with it\n"
                    "         (not with -c, -m, -M, -R, -C, -L, -H, -D, -E, -N, -W)\n");
    fprintf(stderr, "  -x kinds : with -X: the kinds of map printed, letters of s (sequential), c (circular permutation),\n"
                    "         n (not sequential otherwise). Default cn\n");
    fprintf(stderr, "  -b : cache the parsed database as dbfile.satbin\n");
    exit(1);
}

/* ---- stdout.  A query list against a database is millions of rows "name score norm2 z p": formatted with
 * printf they take several times the GPU search (3 M rows: 1.5 s against 0.25 s).  The rows are assembled
 * in a buffer instead, from pieces that printf itself produced: the "%g %g" text of (z, p) is cached per
 * truncated norm2 score (z and p are functions of that integer, sat_gumbel.h), the "%g" text of norm2 per
 * (score, n1 + n2) - byte-identical to printf("%-8s %d %g %g %g\n") by construction. */
static char out_buf[1 << 20];
static size_t out_len = 0;

static void out_flush(void)
{
    if (out_len) fwrite(out_buf, 1, out_len, stdout);
    out_len = 0;
    fflush(stdout);
}

static inline void out_bytes(const char *p, size_t n)
{
    if (out_len + n > sizeof(out_buf)) out_flush();
    if (n > sizeof(out_buf)) { fwrite(p, 1, n, stdout); return; }
    memcpy(out_buf + out_len, p, n);
    out_len += n;
}

/* cached printf("%g") texts */
#define ZP_SLOTS 512                       /* truncated norm2 score -256 .. 255 */
#define N2_SCORE_LO (-256)
#define N2_SCORE_N 1280                    /* scores -256 .. 1023 */
#define N2_SUM_N (2 * SAT_MAXDIM + 1)      /* n1 + n2 */
/* (a text that does not fit its slot is never cached - len stays 0 - and is formatted again row by row) */
typedef struct { unsigned char len; char text[23]; } g_text;          /* "%g" of a double: at most 13 characters */
typedef struct { unsigned char len; char text[47]; } zp_text;         /* " %g  %g\n": at most 30 */
static zp_text zp_cache[2][ZP_SLOTS];      /* [wide gap]["z p" of the integer] */
static g_text *norm2_cache = NULL;         /* [score - lo][n1 + n2], allocated on first use */

/* -F: the statistics of the query whose block is being printed - z and p of every histogram bin from the query's
 * fitted (a, b) (sat_gumbel_fit_table, as the device's tables), and the cached " z p" text per bin.  They are a
 * query's own: begin_query_stats sets them up afresh at each header. */
typedef struct {
    double z[SAT_STAT_BINS], p[SAT_STAT_BINS];
    zp_text text[2][SAT_STAT_BINS];        /* [wide gap][bin] */
} fit_stats;
static fit_stats *fit_store = NULL;        /* allocated on first use */
static fit_stats *fit_cur = NULL;          /* NULL: the built-in constants */

static inline void out_int(int v)
{
    char tmp[12];
    int n = 0;
    unsigned u = v < 0 ? 0u - (unsigned)v : (unsigned)v;
    do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
    if (v < 0) tmp[n++] = '-';
    if (out_len + 12 > sizeof(out_buf)) out_flush();
    while (n) out_buf[out_len++] = tmp[--n];
}

/* c: where the row's " z p" text is cached (a function of the truncated norm2 score or, with a fit, of the bin), or
 * NULL: formatted from zscore and pvalue */
static void out_row(const char *name, int score, double norm2score, double zscore, double pvalue, int sum, int wide_gap,
                    zp_text *c)
{
    /* "%-8s " */
    char nm[9];
    size_t ln = strlen(name);
    if (ln > 8) {                                          /* not produced by the reader; printf prints it whole */
        out_bytes(name, ln);
    } else {
        memset(nm, ' ', 8);
        memcpy(nm, name, ln);
        out_bytes(nm, 8);
    }
    out_bytes(" ", 1);
    out_int(score);
    out_bytes(" ", 1);
    /* norm2 */
    const int si = score - N2_SCORE_LO;
    if (si >= 0 && si < N2_SCORE_N && sum >= 0 && sum < N2_SUM_N) {
        if (!norm2_cache) norm2_cache = (g_text *)calloc((size_t)N2_SCORE_N * N2_SUM_N, sizeof(g_text));
        g_text *c = norm2_cache ? &norm2_cache[(size_t)si * N2_SUM_N + sum] : NULL;
        if (c && !c->len) {
            const int n = snprintf(c->text, sizeof c->text, "%g", norm2score);
            if (n > 0 && (size_t)n < sizeof c->text) c->len = (unsigned char)n;
        }
        if (c && c->len) out_bytes(c->text, c->len);
        else { char t[32]; out_bytes(t, (size_t)snprintf(t, sizeof t, "%g", norm2score)); }
    } else {
        char t[32];
        out_bytes(t, (size_t)snprintf(t, sizeof t, "%g", norm2score));
    }
    /* " z p\n" */
    if (c) {
        if (!c->len) {
            const int n = snprintf(c->text, sizeof c->text, wide_gap ? " %g  %g\n" : " %g %g\n", zscore, pvalue);
            if (n > 0 && (size_t)n < sizeof c->text) c->len = (unsigned char)n;
        }
        if (c->len) out_bytes(c->text, c->len);
        else { char t[64]; out_bytes(t, (size_t)snprintf(t, sizeof t, wide_gap ? " %g  %g\n" : " %g %g\n", zscore, pvalue)); }
    } else {
        char t[64];
        out_bytes(t, (size_t)snprintf(t, sizeof t, wide_gap ? " %g  %g\n" : " %g %g\n", zscore, pvalue));
    }
}

static inline void out_map_line(int a, int b)
{
    /* "%3d %3d\n" for 1 <= a, b <= 999 */
    char t[8];
    t[0] = a >= 100 ? (char)('0' + a / 100) : ' ';
    t[1] = a >= 10 ? (char)('0' + a / 10 % 10) : ' ';
    t[2] = (char)('0' + a % 10);
    t[3] = ' ';
    t[4] = b >= 100 ? (char)('0' + b / 100) : ' ';
    t[5] = b >= 10 ? (char)('0' + b / 10 % 10) : ' ';
    t[6] = (char)('0' + b % 10);
    t[7] = '\n';
    out_bytes(t, 8);
}

/* Report to stderr and end the run with status 1 */
__attribute__((format(printf, 1, 2), noreturn))
static void die(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    exit(1);
}

#define SAT_STR_(x) #x
#define SAT_STR(x) SAT_STR_(x)             /* a numeric macro as text, for the messages */

static void *checked(void *p)
{
    if (!p)
        die("malloc failed\n");
    return p;
}

/* A header or table line (never a row of a listing: those are assembled, above).  A text that does not fit ends the run */
__attribute__((format(printf, 1, 2)))
static void out_fmt(const char *fmt, ...)
{
    char line[SAT_MAX_LINE_LEN + 256];
    va_list ap;
    va_start(ap, fmt);
    const int n = vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    if (n < 0 || (size_t)n >= sizeof line)
        die("ERROR: an output line of %d characters does not fit its buffer\n", n);
    out_bytes(line, (size_t)n);
}

/* What the user wrote: the letters given and their parsed values.  Only the getopt loop of parse_options writes it */
typedef struct {
    uint64_t seen;                    /* the letters given, letter_bit() of each (-k 0 is no -k: it prints the listing) */
    int maxstart, want_gpus, topk, nmatch, refine, ncand;
    int rowmatch;                     /* -M: matches of each printed row */
    int tops;                         /* -P: the restarts whose maps are polished */
    double censor;                    /* -F: the right-censored fraction of the rows */
    double pmax;                      /* -p: the largest p-value printed */
    double lmax;                      /* -L: the largest p-value of an edge */
    int nlevels;                      /* -H: the cutoffs' count */
    double levels[SAT_MAX_CLUSTER_LEVELS];  /* -H: the largest p-value of an edge of each level, ascending */
    double dmax;                      /* -D: the largest p-value of an edge */
    const char *classfile;            /* -E: the classification the search is scored against */
    int rocn;                         /* -N: the negatives ROC-n counts up to */
    double wmax;                      /* -W: the largest p-value of a hit */
    double bmin;                      /* -X: the smallest ordered p-value of a row */
    int kinds;                        /* -x: SAT_KIND_* bits of the maps printed */
    double core;                      /* -f: the fraction of the hits every pair of the core is matched together in */
    unsigned long long seed;
    const char *qfile, *from_db, *all;  /* -q, -Q, -a: the database */
    int dev_list[64], ndev_list;
} given;

static uint64_t letter_bit(int c)
{
    return c >= 'a' && c <= 'z' ? (uint64_t)1 << (c - 'a') : c >= 'A' && c <= 'Z' ? (uint64_t)1 << (26 + c - 'A') : 0;
}

static int has(const given *g, int letter)
{
    return (g->seen & letter_bit(letter)) != 0;
}

/* What the run does: all of it derived from what was given, in plan_run, once every rule has passed */
typedef enum { FROM_STDIN, FROM_SIDS, FROM_DB_SIDS, FROM_DB_ALL } query_source;
typedef enum { OUT_LISTING, OUT_RANKED, OUT_NONE } row_output;
typedef enum { NO_CONSUMER, CLUSTER, CLUSTER_LEVELS, COVER, EVAL, PROFILE } row_consumer;
typedef enum { NO_POLISH, POLISH_CANDIDATES, POLISH_ALL } polish_mode;
typedef struct {
    const given *g;                   /* the values as given */
    query_source source;              /* inline structures on stdin; -q: SIDs, built on the host; -Q: SIDs, built on the GPUs
                                       * from the resident database; -a: every entry, built there */
    const char *dbfile;               /* -q, -Q, -a: the database; NULL: stdin names it */
    row_output out;                   /* what leaves the GPUs: the listing in class order; -k / -p / -R: each query's ranked
                                       * rows; nothing: a consumer reads the rows where they are */
    row_consumer consumer;            /* -L, -H, -D, -E, -W: which */
    polish_mode polish;               /* -P T: the maps of each candidate's T best restarts; with -A: of every row's */
    int tops;                         /* T */
    int ncand;                        /* -R, -P: candidates per query, C of -C, else K */
    int csr;                          /* -p, and -k with -F: a row count per query (pcounts) instead of K rows each */
    int nm;                           /* slots per entry: M of -m, else 1 */
    int kinds;                        /* -X: SAT_KIND_* bits of the maps printed, -x's, else c and n */
    double core;                      /* -W: -f's fraction, else 0.5 */
    int rocn;                         /* -E: -N's count, else 50 */
} options;

/* -Q, -a: the batches are set from entry indices on the GPUs */
static int queries_from_db(const options *o)
{
    return o->source == FROM_DB_SIDS || o->source == FROM_DB_ALL;
}

typedef struct {
    char dbfile[SAT_MAX_LINE_LEN];
    int ltype, lorder, lsoln;
    sat_struct_set queries, db;
    char *sids;                       /* -q: num_queries SIDs of SAT_LABELSIZE + 1 bytes */
    int num_queries;
    const sat_struct_set *qsrc;       /* where the queries' structures are: queries, or db with -q */
    int *qindex;                      /* query i is structure qindex[i] of qsrc */
    /* motif queries (SID@list with -q / -Q): query i is the listed SSEs of that structure, in the list's order */
    int motifs;                       /* how many of the queries are motifs; 0: qsub, sse_begin and sse are NULL */
    char **qlist;                     /* [num_queries] with -q / -Q: the list's text as read, NULL for a whole structure */
    int *qsub;                        /* the motif's own structure - the sub-arrays - in `queries`, -1 for a whole one */
    int32_t *sse_begin;               /* [num_queries + 1] CSR into sse; an empty range is a whole structure */
    uint8_t *sse;                     /* the lists, 0-based */
    int *cls_index[2], cls_count[2];  /* db entries of the small (order <= 96) and the large class, file order */
} input;

/* Where query qi's structure is: its set and (*s) its index there - a motif's sub-structure, else the entry itself */
static const sat_struct_set *query_set(const input *in, int qi, int *s)
{
    const int motif = in->motifs && in->qsub[qi] >= 0;
    *s = motif ? in->qsub[qi] : in->qindex[qi];
    return motif ? &in->queries : in->qsrc;
}

static int query_order(const input *in, int qi)
{
    int s;
    const sat_struct_set *set = query_set(in, qi, &s);
    return set->order[s];
}

/* Per-entry results on the host: slot m of row r at r * nm + m (nm = M of -m, else 1).  counts: each row's matches
 * (-m), or NULL: one.  maps: SAT_MAXDIM ints a slot with LSOLN, else NULL. */
typedef struct {
    int nm;
    int32_t *counts, *scores, *maps;
} slots;

/* Database entry e's row and map lines, then with -m its matches 2..count as rows "name:k" with theirs, from row r of
 * s.  A ranked row h (statistics from the device, map hmap) stands in for slot 0; the other rows get the host's. */
static void print_entry(const input *in, int e, int n1, const sat_hit *h, const int32_t *hmap, const slots *s,
                        size_t r, int wide_gap)
{
    const char *name = sat_set_name(&in->db, e);
    const int n2 = in->db.order[e], count = s->counts ? s->counts[r] : 1;
    char mname[SAT_MAX_LINE_LEN + 16];
    for (int m = 0; m < count; m++) {
        const size_t slot = r * (size_t)s->nm + (size_t)m;
        const int32_t *map = hmap;
        if (m == 0 && h) {
            out_row(name, h->score, h->norm2, h->zscore, h->pvalue, n1 + n2, wide_gap, NULL);
        } else {
            const int score = s->scores[slot];
            const double norm2score = sat_norm2(score, n1, n2);
            const int x = (int)norm2score;
            double zscore = 0.0, pvalue = 0.0;
            zp_text *c = NULL;
            if (fit_cur) {
                /* the query's fitted table at the row's bin, as the device indexes it */
                const int bin = score < 0 ? 0 : sat_stat_bin_of(score, n1 + n2);
                zscore = fit_cur->z[bin];
                pvalue = fit_cur->p[bin];
                c = &fit_cur->text[wide_gap ? 1 : 0][bin];
            } else {
                /* z and p only when their cached text is missing */
                if (x >= -256 && x < 256)
                    c = &zp_cache[wide_gap ? 1 : 0][x + 256];
                if (!(c && c->len)) {
                    zscore = sat_z_gumbel_trunc(norm2score);
                    pvalue = sat_pv_gumbel(zscore);
                }
            }
            if (m)
                snprintf(mname, sizeof mname, "%s:%d", name, m + 1);
            out_row(m ? mname : name, score, norm2score, zscore, pvalue, n1 + n2, wide_gap, c);
            map = s->maps ? s->maps + slot * SAT_MAXDIM : NULL;
        }
        if (map)
            for (int k = 0; k < n1; k++)
                if (map[k] >= 0)
                    out_map_line(k + 1, map[k] + 1);
    }
}

/* -F: the rows that follow are query `f`'s - its tables and an empty text cache; no fit (or NULL): the built-ins */
static char polish_header[128];      /* -P: the fourth header line of every block, else empty */

static void begin_query_stats(const sat_fit *f)
{
    fit_cur = NULL;
    if (!f || !f->fitted)
        return;
    if (!fit_store)
        fit_store = checked(malloc(sizeof *fit_store));
    fit_cur = fit_store;
    sat_gumbel_fit_table(f->a, f->b, fit_cur->z, fit_cur->p);
    memset(fit_cur->text, 0, sizeof fit_cur->text);
}

/* A motif query's "# QUERY SSES" line: the list as numbers, 1-based, ranges expanded, in the order given */
static void out_query_sses(const input *in, int qi)
{
    if (!in->motifs || in->qsub[qi] < 0)
        return;
    out_bytes("# QUERY SSES = ", 15);
    for (int32_t k = in->sse_begin[qi]; k < in->sse_begin[qi + 1]; k++)
        out_fmt(k > in->sse_begin[qi] ? ",%d" : "%d", in->sse[k] + 1);
    out_bytes("\n", 1);
}

/* A query's "# GUMBEL" line; which: "", or "ordered " for the fit of -X's ordered search */
static void out_gumbel(const sat_fit *f, const char *which)
{
    if (f->fitted)
        out_fmt("# GUMBEL %sa = %.17g b = %.17g rows = %d censored = %d below = %d\n", which, f->a, f->b, f->rows, f->censored,
                f->below);
    else
        out_fmt("# GUMBEL %snot fitted\n", which);
}

/* A table's "# GUMBEL" line: how many of its n queries were fitted; nothing without -F */
static void out_fitted(const options *o, const sat_fit *fits, int n)
{
    int fitted = 0;
    if (!fits)
        return;
    for (int v = 0; v < n; v++)
        fitted += fits[v].fitted != 0;
    out_fmt("# GUMBEL censor = %g fitted = %d of %d\n", o->g->censor, fitted, n);
}

/* The three '#' lines that open a block of query qi; with -F (f: the query's fit) a fourth, and the statistics of the
 * rows that follow are f's */
static void print_header(const input *in, int qi, const sat_fit *f)
{
    out_fmt("# cudaSaTabsearch LTYPE = %c LORDER = %c LSOLN = %c\n", in->ltype ? 'T' : 'F', in->lorder ? 'T' : 'F',
            in->lsoln ? 'T' : 'F');
    out_fmt("# QUERY ID = %-8s\n", sat_set_name(in->qsrc, in->qindex[qi]));
    out_fmt("# DBFILE = %-80s\n", in->dbfile);
    out_query_sses(in, qi);
    out_bytes(polish_header, strlen(polish_header));
    begin_query_stats(f);
    if (!f)
        return;
    if (!f->fitted)
        fprintf(stderr, "WARNING: no Gumbel fit for query %s: its rows keep the built-in statistics\n",
                sat_set_name(in->qsrc, in->qindex[qi]));
    out_gumbel(f, "");
}

/* -H's list into g->levels / g->nlevels; 0: not 1 .. SAT_MAX_CLUSTER_LEVELS numbers in [0, 1], strictly ascending, the
 * whole argument */
static int parse_levels(const char *arg, given *o)
{
    o->nlevels = 0;
    for (const char *at = arg;; ) {
        char *end = NULL;
        const double p = strtod(at, &end);
        if (end == at || (*end != ',' && *end != '\0') || !isfinite(p) || p < 0.0 || p > 1.0)
            return 0;
        if (o->nlevels == SAT_MAX_CLUSTER_LEVELS || (o->nlevels > 0 && !(p > o->levels[o->nlevels - 1])))
            return 0;
        o->levels[o->nlevels++] = p;
        if (*end == '\0')
            return 1;
        at = end + 1;
    }
}

/* -x's letters as SAT_KIND_* bits; 0: empty, or another character */
static int parse_kinds(const char *arg)
{
    int kinds = 0;
    for (const char *c = arg; *c; c++) {
        if (*c == 's') kinds |= SAT_KIND_SEQUENTIAL;
        else if (*c == 'c') kinds |= SAT_KIND_CIRCULAR;
        else if (*c == 'n') kinds |= SAT_KIND_PERMUTED;
        else return 0;
    }
    return kinds;
}

/* the bits as -x's letters, in the order s, c, n */
static const char *kinds_text(int kinds, char text[4])
{
    int n = 0;
    if (kinds & SAT_KIND_SEQUENTIAL) text[n++] = 's';
    if (kinds & SAT_KIND_CIRCULAR) text[n++] = 'c';
    if (kinds & SAT_KIND_PERMUTED) text[n++] = 'n';
    text[n] = '\0';
    return text;
}

/* "ERROR: -L needs WHAT (got 'ARG')", then the usage; without `what` the usage alone */
__attribute__((noreturn))
static void bad_arg(const char *prog, int letter, const char *what)
{
    if (what)
        fprintf(stderr, "ERROR: -%c needs %s (got '%s')\n", letter, what, optarg);
    usage(prog);
    exit(1);
}

/* optarg as a real number: the whole argument, finite, >= lo (open: > lo) and <= hi */
static double real_arg(const char *prog, int letter, const char *what, double lo, int open, double hi)
{
    char *end = NULL;
    const double v = strtod(optarg, &end);
    if (end == optarg || *end != '\0' || !isfinite(v) || (open ? !(v > lo) : v < lo) || v > hi)
        bad_arg(prog, letter, what);
    return v;
}

/* optarg as an integer 1 .. max: the whole argument, digits only (0, a sign, text are refused) */
static int int_arg(const char *prog, int letter, const char *what, long max)
{
    char *end = NULL;
    const long v = strtol(optarg, &end, 10);
    if (end == optarg || *end != '\0' || v < 1 || v > max)
        bad_arg(prog, letter, what);
    return (int)v;
}

/* "-OWNER cannot be combined with -x" for the first letter of `letters` that was given beside -OWNER */
static void forbid(const given *g, int owner, const char *letters)
{
    for (const char *c = letters; has(g, owner) && *c; c++)
        if (has(g, *c))
            die("ERROR: -%c cannot be combined with -%c\n", owner, *c);
}

/* -R, -P: the candidates per query */
static int candidates(const given *g)
{
    return has(g, 'C') ? g->ncand : g->topk;
}

/* The refusals, in a fixed order (tests/golden/cli_rules pins which one a command line gets that breaks several).  A mode
 * is a forbid() line of its own, its "needs" lines and the entry points it calls; nothing here changes what was given,
 * so where a block stands decides only which of several refusals is reported */
static void check_rules(const given *g)
{
    const int gpu = !has(g, 'c'), fit = has(g, 'F');
    const int each = has(g, 'P') && !has(g, 'A');            /* -P T without -A: polish per candidate, -k's rows */
    const int ranked = g->topk > 0 || has(g, 'p');           /* (-R needs -k) */
    if (has(g, 'x') && !has(g, 'X')) die("ERROR: -x needs -X B\n");
    if (has(g, 'X')) {
        /* hits out of sequence order: -p's run, searched twice, with another selection */
        forbid(g, 'X', "cmMRCLHDENW");
        if (!has(g, 'p')) die("ERROR: -X needs -p P\n");
        if (each) die("ERROR: -X takes -P T only with -A\n");
        if (!sat_multi_search_only || !sat_multi_search_fit || !sat_multi_baseline_keep || !sat_multi_reorder_hits)
            die("ERROR: this library has no sat_multi_reorder_hits\n");
    }
    if (has(g, 'f') && !has(g, 'W')) die("ERROR: -f needs -W P\n");
    if (has(g, 'W')) {
        /* profile: a run whose rows and maps stay on the GPUs; -q, -Q, -a and the stdin queries all feed it */
        forbid(g, 'W', "ckpmMRCHDLEN");
        if (each) die("ERROR: -W takes -P T only with -A\n");
        if (!sat_multi_search_only || !sat_multi_profile_rows || !sat_profile_core)
            die("ERROR: this library has no sat_multi_profile_rows\n");
        if (fit && !sat_multi_search_fit) die("ERROR: this library has no sat_multi_search_fit\n");
    }
    if (has(g, 'N') && !has(g, 'E')) die("ERROR: -N needs -E classfile\n");
    if (has(g, 'D')) {
        /* clustering around representatives: -L's run with another accumulator and another table */
        forbid(g, 'D', "c");
        if (!has(g, 'a')) die("ERROR: -D needs -a dbfile\n");
        forbid(g, 'D', "kpmMRCLHE");
        if (!sat_multi_search_only || !sat_multi_cover_begin || !sat_multi_cover_add || !sat_multi_cover_solve || !sat_cover_sizes)
            die("ERROR: this library has no sat_multi_cover_add\n");
        if (fit && !sat_multi_search_fit) die("ERROR: this library has no sat_multi_search_fit\n");
    }
    if (has(g, 'E')) {
        /* evaluation: a run over queries of the database whose rows stay on the GPUs */
        forbid(g, 'E', "c");
        if (!has(g, 'a') && !has(g, 'Q')) die("ERROR: -E needs -a dbfile or -Q dbfile\n");
        forbid(g, 'E', "kpmMRCFLH");
        if (each) die("ERROR: -E takes -P T only with -A\n");
        if (!sat_multi_search_only || !sat_multi_eval_classes || !sat_multi_eval_rows)
            die("ERROR: this library has no sat_multi_eval_rows\n");
    }
    if (has(g, 'H')) {
        /* clustering at several cutoffs: -L's run with another add call and another table */
        forbid(g, 'H', "c");
        if (!has(g, 'a')) die("ERROR: -H needs -a dbfile\n");
        forbid(g, 'H', "LkpmMRC");
        if (!sat_multi_search_only || !sat_multi_cluster_begin_levels || !sat_multi_cluster_add_levels ||
            !sat_multi_cluster_labels_levels || !sat_cluster_reps || !sat_cluster_nested)
            die("ERROR: this library has no sat_multi_cluster_add_levels\n");
        if (fit && !sat_multi_search_fit) die("ERROR: this library has no sat_multi_search_fit\n");
    } else if (has(g, 'L')) {
        /* clustering: an all-vs-all run whose rows stay on the GPUs */
        forbid(g, 'L', "c");
        if (!has(g, 'a')) die("ERROR: -L needs -a dbfile\n");
        forbid(g, 'L', "kpmMRC");
        if (!sat_multi_search_only || !sat_multi_cluster_begin || !sat_multi_cluster_add || !sat_multi_cluster_labels ||
            !sat_cluster_reps)
            die("ERROR: this library has no sat_multi_cluster_add\n");
        if (fit && !sat_multi_search_fit) die("ERROR: this library has no sat_multi_search_fit\n");
    }
    /* queries from the resident database */
    forbid(g, 'Q', "c");
    forbid(g, 'a', "c");
    forbid(g, 'Q', "q");
    forbid(g, 'a', "qQ");
    if ((has(g, 'Q') || has(g, 'a')) && !sat_multi_queries_from_db) die("ERROR: this library has no sat_multi_queries_from_db\n");
    if (has(g, 'A')) {
        /* all rows: the mode of the library; the run is an ordinary one on polished rows */
        if (!has(g, 'P')) die("ERROR: -A needs -P T\n");
        forbid(g, 'A', "cmMRC");
        if (!sat_multi_polish_all_set) die("ERROR: this library has no sat_multi_polish_all_set\n");
    }
    if (each) {
        if (!gpu) die("ERROR: -P needs the GPU path\n");
        forbid(g, 'P', "mMpF");
        if (g->topk <= 0) die("ERROR: -P needs -k K\n");
        if (!sat_multi_search_refine_polish) die("ERROR: this library has no sat_multi_search_refine_polish\n");
    }
    if (has(g, 'p')) {
        if (!gpu) die("ERROR: -p needs the GPU path\n");
        forbid(g, 'p', "mR");
        if (!sat_multi_search_cutoff || !sat_multi_hits_cutoff) die("ERROR: this library has no sat_multi_search_cutoff\n");
    }
    if (has(g, 'R')) {
        if (!gpu) die("ERROR: -R needs the GPU path\n");
        forbid(g, 'R', "m");
        if (g->topk <= 0) die("ERROR: -R needs -k K\n");
    }
    if (has(g, 'C') && !has(g, 'R') && !each) die("ERROR: -C needs -R\n");
    if ((has(g, 'R') || each) && g->topk > candidates(g)) die("ERROR: -k K (%d) exceeds -C C (%d)\n", g->topk, candidates(g));
    if (has(g, 'R') && !sat_multi_search_refine) die("ERROR: this library has no sat_multi_search_refine\n");
    if (has(g, 'm')) {
        if (!gpu) die("ERROR: -m needs the GPU path\n");
        if (!sat_multi_search_matches) die("ERROR: this library has no sat_multi_search_matches\n");
    }
    if (has(g, 'M')) {
        if (!gpu) die("ERROR: -M needs the GPU path\n");
        forbid(g, 'M', "m");
        if (!ranked) die("ERROR: -M needs -k K, -p P or -R restarts -k K\n");
        if (!sat_multi_search_pairs_matches) die("ERROR: this library has no sat_multi_search_pairs_matches\n");
    }
    forbid(g, 'F', "Rm");
    if (fit && ranked && (!sat_multi_search_fit || !sat_multi_hits_cutoff)) die("ERROR: this library has no sat_multi_search_fit\n");
}

/* The options into *g - only this loop writes it - and the refusals, all before the banner and any device call */
static void parse_options(int argc, char *argv[], given *g)
{
    const char *prog = argv[0];
    *g = (given){ .maxstart = 128, .want_gpus = 1, .seed = SAT_DEFAULT_SEED };
    int c;
    while ((c = getopt(argc, argv, "cq:Q:a:r:g:G:s:bk:p:m:M:R:C:F:P:AL:H:E:N:D:W:f:X:x:")) != -1) {
        g->seen |= letter_bit(c);
        switch (c) {
        case 'c': case 'b': case 'A': break;
        case 'q': g->qfile = optarg; break;
        case 'Q': g->from_db = optarg; break;
        case 'a': g->all = optarg; break;
        case 'E': g->classfile = optarg; break;
        case 'r': g->maxstart = atoi(optarg); break;
        case 'g': g->want_gpus = atoi(optarg); break;
        case 'G':
            for (char *tok = strtok(optarg, ","); tok && g->ndev_list < 64; tok = strtok(NULL, ","))
                g->dev_list[g->ndev_list++] = atoi(tok);
            break;
        case 's': g->seed = strtoull(optarg, NULL, 0); break;
        case 'k':
            g->topk = atoi(optarg);
            if (!g->topk) g->seen &= ~letter_bit('k');
            break;
        case 'p': g->pmax = real_arg(prog, c, "a p-value >= 0", 0.0, 0, INFINITY); break;
        case 'L': g->lmax = real_arg(prog, c, "a p-value in [0, 1]", 0.0, 0, 1.0); break;
        case 'D': g->dmax = real_arg(prog, c, "a p-value in [0, 1]", 0.0, 0, 1.0); break;
        case 'W': g->wmax = real_arg(prog, c, "a p-value in [0, 1]", 0.0, 0, 1.0); break;
        case 'X': g->bmin = real_arg(prog, c, "a p-value in [0, 1]", 0.0, 0, 1.0); break;
        case 'f': g->core = real_arg(prog, c, "a fraction in (0, 1]", 0.0, 1, 1.0); break;
        case 'F': g->censor = real_arg(prog, c, "a censored fraction in [0, 0.5]", 0.0, 0, 0.5); break;
        case 'm': g->nmatch = int_arg(prog, c, NULL, SAT_MAX_MATCHES); break;
        case 'M': g->rowmatch = int_arg(prog, c, "an integer 1.." SAT_STR(SAT_MAX_MATCHES), SAT_MAX_MATCHES); break;
        case 'P': g->tops = int_arg(prog, c, "an integer 1.." SAT_STR(SAT_MAX_MATCHES), SAT_MAX_MATCHES); break;
        case 'N': g->rocn = int_arg(prog, c, "an integer >= 1", 0x7FFFFFFFL); break;
        case 'R': g->refine = int_arg(prog, c, "a positive integer", 0x7FFFFFFFL); break;
        case 'C': g->ncand = int_arg(prog, c, "a positive integer", 0x7FFFFFFFL); break;
        case 'x':
            /* the whole argument, one or more of the letters s, c, n */
            g->kinds = parse_kinds(optarg);
            if (!g->kinds)
                bad_arg(prog, c, "letters of s, c, n");
            break;
        case 'H':
            /* the whole argument: 1 .. SAT_MAX_CLUSTER_LEVELS numbers, each as -L's, with commas between, strictly ascending */
            if (!parse_levels(optarg, g))
                bad_arg(prog, c, "1.." SAT_STR(SAT_MAX_CLUSTER_LEVELS) " ascending p-values in [0, 1]");
            break;
        default: usage(prog);
        }
    }
    check_rules(g);
}

/* What the run does, from what was given */
static void plan_run(const given *g, options *o)
{
    *o = (options){ .g = g, .tops = g->tops, .ncand = candidates(g) };
    o->source = has(g, 'a') ? FROM_DB_ALL : has(g, 'Q') ? FROM_DB_SIDS : has(g, 'q') ? FROM_SIDS : FROM_STDIN;
    o->dbfile = has(g, 'a') ? g->all : has(g, 'Q') ? g->from_db : g->qfile;
    o->consumer = has(g, 'L') ? CLUSTER : has(g, 'H') ? CLUSTER_LEVELS : has(g, 'D') ? COVER : has(g, 'E') ? EVAL
                  : has(g, 'W') ? PROFILE : NO_CONSUMER;
    o->out = o->consumer != NO_CONSUMER ? OUT_NONE : g->topk > 0 || has(g, 'p') ? OUT_RANKED : OUT_LISTING;
    o->polish = !has(g, 'P') ? NO_POLISH : has(g, 'A') ? POLISH_ALL : POLISH_CANDIDATES;
    o->csr = has(g, 'p') || (has(g, 'F') && g->topk > 0);
    o->nm = g->nmatch > 0 ? g->nmatch : 1;
    o->kinds = has(g, 'x') ? g->kinds : SAT_KIND_CIRCULAR | SAT_KIND_PERMUTED;
    o->core = has(g, 'f') ? g->core : 0.5;
    o->rocn = has(g, 'N') ? g->rocn : 50;
}

/* -q, -Q: query SIDs on stdin, one a line (cut to 7 characters), options T T F; -a: the same options and nothing read -
 * the queries are the database's entries, counted when it is loaded; else the database name, the options and the query
 * structures on stdin */
static void read_queries(const options *o, input *in)
{
    if (o->dbfile) {
        strncpy(in->dbfile, o->dbfile, sizeof in->dbfile - 1);
        in->ltype = in->lorder = 1;
        char buf[SAT_MAX_LINE_LEN];
        while (o->source != FROM_DB_ALL && !feof(stdin) && fgets(buf, SAT_MAX_LINE_LEN, stdin)) {
            in->sids = checked(realloc(in->sids, (size_t)(in->num_queries + 1) * (SAT_LABELSIZE + 1)));
            char *sid = in->sids + (size_t)in->num_queries++ * (SAT_LABELSIZE + 1);
            memset(sid, 0, SAT_LABELSIZE + 1);
            /* SID@list: the SID is what stands before the first '@', the list the rest of the line */
            char *list = strchr(buf, '@');
            in->qlist = checked(realloc(in->qlist, sizeof(char *) * (size_t)in->num_queries));
            in->qlist[in->num_queries - 1] = NULL;
            if (list) {
                /* a list is never cut in two: a line that fills the buffer would go on as the next query */
                if (strlen(buf) == SAT_MAX_LINE_LEN - 1 && buf[SAT_MAX_LINE_LEN - 2] != '\n')
                    die("ERROR: query line with a list is longer than %d characters\n", SAT_MAX_LINE_LEN - 2);
                *list++ = '\0';
                list[strcspn(list, "\n")] = '\0';
                if (*list && list[strlen(list) - 1] == '\r')         /* a CRLF line: as a 7-character SID's is cut off */
                    list[strlen(list) - 1] = '\0';
                in->qlist[in->num_queries - 1] = checked(strdup(list));
                in->motifs++;
            }
            strncpy(sid, buf, SAT_LABELSIZE);
            sid[SAT_LABELSIZE - 1] = '\0';
            size_t len = strlen(sid);
            if (len && sid[len - 1] == '\n') sid[len - 1] = '\0';
        }
    } else {
        char cltype, clorder, clsoln;
        if (fscanf(stdin, "%s\n", in->dbfile) != 1)
            die("ERROR reading dbfilename from stdin\n");
        if (fscanf(stdin, "%c %c %c\n", &cltype, &clorder, &clsoln) != 3)
            die("ERROR reading options from stdin\n");
        in->ltype = cltype == 'T';
        in->lorder = clorder == 'T';
        in->lsoln = clsoln == 'T';
        in->num_queries = sat_read_structures(stdin, &in->queries, "query");
        if (in->num_queries < 0)
            die("ERROR loading query structures from stdin\n");
        if (in->num_queries == 0)
            die("ERROR: no query structures found on stdin\n");
        fprintf(stderr, "Read %d query structures\n", in->num_queries);
    }
    if (!in->ltype) {
        fprintf(stderr, "WARNING: LTYPE is always set to T\n");
        in->ltype = 1;
    }
    if (has(o->g, 'X')) {
        /* -X runs both searches itself, whatever the input says; its rows are the unordered search's, with their maps */
        in->lorder = 0;
        in->lsoln = 1;
    }
}

/* Motif queries, once every query's entry is known: each list checked against its entry's order (a bad one ends the run
 * here, before any search), and the motif's own structure - packed cell (i, k) is the entry's cell (max, min) of (l[i],
 * l[k]) - appended to in->queries under the entry's name: what -q and -c search and what every mode prints from */
static void cut_motifs(input *in)
{
    uint8_t list[SAT_MAXDIM], *tab = checked(malloc(SAT_MAXDIM * (SAT_MAXDIM + 1) / 2));
    float *dist = checked(malloc(sizeof(float) * SAT_MAXDIM * (SAT_MAXDIM + 1) / 2));
    in->qsub = checked(malloc(sizeof(int) * (size_t)in->num_queries));
    in->sse_begin = checked(calloc((size_t)in->num_queries + 1, sizeof(int32_t)));
    in->sse = checked(malloc((size_t)in->motifs * SAT_MAXDIM));
    for (int q = 0; q < in->num_queries; q++) {
        const int e = in->qindex[q];
        in->qsub[q] = -1;
        in->sse_begin[q + 1] = in->sse_begin[q];
        if (!in->qlist[q])
            continue;
        char err[128];
        const int m = sat_parse_sse_list(in->qlist[q], in->db.order[e], list, err, sizeof err);
        if (m < 0)
            die("ERROR: query %s@%s: %s\n", in->sids + (size_t)q * (SAT_LABELSIZE + 1), in->qlist[q], err);
        const int64_t base = in->db.cell_off[e];
        for (int i = 0; i < m; i++)
            for (int k = 0; k <= i; k++) {
                const int hi = list[i] > list[k] ? list[i] : list[k], lo = list[i] > list[k] ? list[k] : list[i];
                tab[i * (i + 1) / 2 + k] = in->db.tab[base + hi * (hi + 1) / 2 + lo];
                dist[i * (i + 1) / 2 + k] = in->db.dist[base + hi * (hi + 1) / 2 + lo];
            }
        in->qsub[q] = sat_set_append(&in->queries, sat_set_name(&in->db, e), m, tab, dist);
        if (in->qsub[q] < 0)
            die("ERROR: no memory for query %s@%s\n", in->sids + (size_t)q * (SAT_LABELSIZE + 1), in->qlist[q]);
        memcpy(in->sse + in->sse_begin[q], list, (size_t)m);
        in->sse_begin[q + 1] += m;
    }
    free(tab);
    free(dist);
}

/* The database (-b: its binary image when that is newer than the file), split into the two size classes; then each
 * query's structure: the inline ones in turn, with -q / -Q the database entry of its SID (small class first), with -a
 * every entry in file order */
static void load_database(const options *o, input *in)
{
    FILE *dbfp = fopen(in->dbfile, "r");
    if (!dbfp)
        die("ERROR opening db file %s\n", in->dbfile);
    fclose(dbfp);
    fprintf(stderr, "Loading database...\n");
    const double t0 = now_ms();
    int total = -1;
    char binpath[SAT_MAX_LINE_LEN + 16];
    snprintf(binpath, sizeof(binpath), "%s.satbin", in->dbfile);
    if (has(o->g, 'b')) {
        struct stat sa, sb;
        if (stat(in->dbfile, &sa) == 0 && stat(binpath, &sb) == 0 && sb.st_mtime >= sa.st_mtime &&
            sat_set_load_binary(binpath, &in->db) == 0) {
            total = in->db.count;
            fprintf(stderr, "(binary image %s)\n", binpath);
        }
    }
    if (total < 0) {
        total = sat_read_structures_file(in->dbfile, &in->db, "database");     /* mmap reader, same semantics */
        if (total >= 0 && has(o->g, 'b') && sat_set_save_binary(&in->db, binpath) != 0)
            fprintf(stderr, "WARNING: could not write %s\n", binpath);
    }
    if (total < 0)
        die("ERROR loading database\n");
    /* the two passes of the reference: small class then large class, file order inside */
    for (int k = 0; k < 2; k++)
        in->cls_index[k] = checked(malloc(sizeof(int) * (size_t)(total + 1)));
    for (int s = 0; s < in->db.count; s++) {
        const int k = in->db.order[s] > SAT_MAXDIM_SMALL;
        in->cls_index[k][in->cls_count[k]++] = s;
    }
    fprintf(stderr, "Loaded %d db entries (%d order > %d) in %f ms\n",
            total, in->cls_count[1], SAT_MAXDIM_SMALL, now_ms() - t0);
    if (total == 0)
        die("ERROR: empty database\n");

    in->qsrc = o->dbfile ? &in->db : &in->queries;
    if (o->source == FROM_DB_ALL)
        in->num_queries = in->db.count;
    in->qindex = checked(malloc(sizeof(int) * (size_t)(in->num_queries + 1)));
    for (int i = 0; i < in->num_queries; i++) {
        in->qindex[i] = i;
        if (o->source != FROM_SIDS && o->source != FROM_DB_SIDS)
            continue;
        const char *sid = in->sids + (size_t)i * (SAT_LABELSIZE + 1);
        int found = -1;
        for (int k = 0; k < 2 && found < 0; k++)
            for (int d = 0; d < in->cls_count[k]; d++)
                if (!strcasecmp(sid, sat_set_name(&in->db, in->cls_index[k][d]))) {
                    found = in->cls_index[k][d];
                    break;
                }
        if (found < 0)
            die("ERROR: query %s not found\n", sid);
        in->qindex[i] = found;
    }
    if (in->motifs)
        cut_motifs(in);
}

static void free_input(input *in)
{
    free(in->qindex);
    free(in->sids);
    for (int i = 0; in->qlist && i < in->num_queries; i++)
        free(in->qlist[i]);
    free(in->qlist);
    free(in->qsub);
    free(in->sse_begin);
    free(in->sse);
    free(in->cls_index[0]);
    free(in->cls_index[1]);
    sat_set_free(&in->queries);
    sat_set_free(&in->db);
}

/* -F where every score is on the host: the histogram and the fit of one query's n rows */
static sat_fit fit_scores(const int32_t *scores, int n, int n1, const int32_t *orders, double censor)
{
    uint32_t *counts = checked(calloc(SAT_STAT_BINS, sizeof(uint32_t)));
    int32_t below = 0;
    sat_fit f;
    sat_stat_histogram(scores, n, n1, orders, counts, &below);
    if (sat_gumbel_fit_binned(counts, censor, &f) != 0)
        die("ERROR: -F censor out of range\n");
    f.below = below;
    free(counts);
    return f;
}

/* ---- host mode: class by class, query by query, ONE stream for everything */
static int run_host(const options *o, const input *in)
{
    const size_t total = (size_t)in->db.count;
    const int fit = has(o->g, 'F');
    slots one = { 1, NULL, checked(malloc(sizeof(int32_t) * total)),
                  in->lsoln ? checked(malloc(sizeof(int32_t) * SAT_MAXDIM * total)) : NULL };
    int32_t *fit_orders = fit ? checked(malloc(sizeof(int32_t) * (total + 1))) : NULL;
    sat_host_stream stream;
    sat_host_stream_seed(&stream, 1234);
    const int passes = in->cls_count[1] > 0 ? 2 : 1;
    for (int k = 0; k < passes; k++)
        for (int qi = 0; qi < in->num_queries; qi++) {
            int qs;
            const sat_struct_set *qset = query_set(in, qi, &qs);
            if (!fit)
                print_header(in, qi, NULL);
            fprintf(stderr, "Executing simulated annealing tableaux match kernel on host for query %s...\n",
                    sat_set_name(qset, qs));
            double t1 = now_ms();
            if (sat_host_search(&in->db, in->cls_index[k], in->cls_count[k], qset, qs, in->lorder, in->lsoln,
                                o->g->maxstart, &stream, one.scores, one.maps) != 0)
                die("malloc failed in host search\n");
            double ms = now_ms() - t1;
            fprintf(stderr, "host execution time %f ms\n", ms);
            fprintf(stderr, "%f million iterations/sec\n",
                    ((double)in->cls_count[k] * ((double)o->g->maxstart * SAT_MAXITER) / (ms / 1000)) / 1.0e6);
            if (fit) {
                /* the block's own rows: the one stream runs class after class, so a block is fitted when it is printed */
                for (int d = 0; d < in->cls_count[k]; d++)
                    fit_orders[d] = in->db.order[in->cls_index[k][d]];
                sat_fit f = fit_scores(one.scores, in->cls_count[k], qset->order[qs], fit_orders, o->g->censor);
                print_header(in, qi, &f);
            }
            for (int d = 0; d < in->cls_count[k]; d++)
                print_entry(in, in->cls_index[k][d], qset->order[qs], NULL, NULL, &one, (size_t)d, 0);
        }
    free(one.scores);
    free(one.maps);
    free(fit_orders);
    return 0;
}

/* ---- GPU mode */

/* -W: the solution maps a batch may hold on the GPUs (batch x entries x the largest query's SSEs bytes) */
#define PROFILE_MAP_BYTES ((size_t)4 << 30)

/* The host side of the GPU path, sized once for the mode */
typedef struct {
    int batch;                        /* queries a search scores */
    int kk;                           /* -k: rows per query, min(K, entries) */
    int32_t *n1s;                     /* the batch's queries: orders, codes, types and distances at pitch SAT_MAXDIM */
                                      /* (-Q, -a: the orders alone - the GPUs build the rest from their entries) */
    uint8_t *qtabs, *qtypes;
    float *qdmats;
    slots all;                        /* listing, -m: every entry's slots, row b * entries + e */
    int32_t *restarts;                /* -m: each slot's restart (asked for, not printed) */
    slots large;                      /* listing: the large class's slots of every query, row qi * large + d */
    sat_hit *hits;                    /* -k / -p / -R: the batch's ranked rows, and with LSOLN their maps */
    int32_t *hit_maps;
    int32_t *pcounts;                 /* -p: rows of each query of the batch */
    int hits_cap;                     /* -p: rows hits holds */
    int reorder;                      /* -X: the rows come as rhits, hits holds their sat_hit part */
    sat_reorder_hit *rhits;           /* -X: hits_cap of them */
    sat_fit *base_fits;               /* -X with -F: the batch's fits of the ordered search */
    slots rowm;                       /* -M: the slots of the batch's ranked rows, row r of hits */
    int32_t *rowm_restarts, *pair_q, *pair_e;   /* -M: each slot's restart; the rows as (query, entry) pairs */
    size_t rowm_cap;                  /* -M: rows they hold */
    int32_t *sse_begin;               /* -Q with motif queries: the batch's list offsets, batch + 1 of them */
    int32_t *qnode;                   /* -W: the batch's queries as database entries, -1 for a query that is none */
    uint32_t *phits, *pjoint;         /* -W: every query's hits; the matrices, query qi's at poff[qi] */
    size_t *poff;                     /* -W: num_queries + 1 of them */
    sat_classes classes;              /* -E: the classification */
    sat_eval *evals;                  /* -E: every query's row as the GPUs reduced it */
} gpu_bufs;

static void alloc_slots(slots *s, size_t rows, int nm, int with_counts, int lsoln)
{
    s->nm = nm;
    s->counts = with_counts ? checked(malloc(sizeof(int32_t) * rows)) : NULL;
    s->scores = checked(malloc(sizeof(int32_t) * rows * (size_t)nm));
    s->maps = lsoln ? checked(malloc(sizeof(int32_t) * SAT_MAXDIM * rows * (size_t)nm)) : NULL;
}

static void alloc_hits(gpu_bufs *B, size_t rows, int lsoln)
{
    free(B->hits);
    free(B->hit_maps);
    B->hits = checked(malloc(sizeof(sat_hit) * rows));
    if (B->reorder) {
        free(B->rhits);
        B->rhits = checked(malloc(sizeof(sat_reorder_hit) * rows));
    }
    B->hit_maps = lsoln ? checked(malloc(sizeof(int32_t) * SAT_MAXDIM * rows)) : NULL;
}

static void alloc_gpu_bufs(const options *o, const input *in, gpu_bufs *B)
{
    const given *g = o->g;
    const int total = in->db.count, nm = o->nm, lsoln = in->lsoln;
    const int entry_slots = o->out == OUT_LISTING || g->nmatch;          /* every entry's slots come to the host */
    *B = (gpu_bufs){ .batch = 256, .kk = g->topk < total ? g->topk : total, .reorder = has(g, 'X') };
    if (o->consumer == EVAL) {
        /* the classification, read before any GPU is touched: a bad file ends the run here */
        char err[SAT_MAX_LINE_LEN + 256];
        if (sat_read_classes(g->classfile, &in->db, &B->classes, err, sizeof err) != 0)
            die("ERROR: %s\n", err);
        if (B->classes.unknown)
            fprintf(stderr, "WARNING: %d names of %s are not in the database\n", B->classes.unknown, g->classfile);
        fprintf(stderr, "Read %d classes of %d of %d structures from %s\n", B->classes.distinct, B->classes.classified, total,
                g->classfile);
        B->evals = checked(calloc((size_t)in->num_queries + 1, sizeof(sat_eval)));
    }
    /* Queries go to the GPUs in batches: one set of launches scores a whole batch (grid = entries x queries), which
     * is what fills the machine when the database is small and the query list long (-q).  The batch size is bounded
     * by the host slots of every entry: score and map, with -m also count and restarts (the device holds the same
     * slots, maps as bytes). */
    if (entry_slots) {
        const size_t per_entry = (size_t)nm * (lsoln ? SAT_MAXDIM + 1 : 1) + (g->nmatch ? 1 + (size_t)nm : 0);
        const size_t per_query = (size_t)total * per_entry * sizeof(int32_t);
        const size_t budget = (size_t)1 << 30;
        if ((size_t)B->batch * per_query > budget) B->batch = (int)(budget / per_query);
    }
    if (o->consumer == PROFILE) {
        /* the batch's maps stay on the GPUs, a byte per entry and query SSE: at most PROFILE_MAP_BYTES of them, sized by
         * the run's largest query.  The counters are a query's own: nothing depends on the cut.  And every query's
         * result until the table is printed: 4 + 4 n1 n1 bytes */
        size_t n1max = 1;
        B->poff = checked(calloc((size_t)in->num_queries + 1, sizeof(size_t)));
        for (int qi = 0; qi < in->num_queries; qi++) {
            const size_t n1 = (size_t)query_order(in, qi);
            n1max = n1 > n1max ? n1 : n1max;
            B->poff[qi + 1] = B->poff[qi] + n1 * n1;
        }
        if ((size_t)B->batch * (size_t)total * n1max > PROFILE_MAP_BYTES) B->batch = (int)(PROFILE_MAP_BYTES / ((size_t)total * n1max));
        B->phits = checked(malloc(sizeof(uint32_t) * ((size_t)in->num_queries + 1)));
        B->pjoint = checked(malloc(sizeof(uint32_t) * (B->poff[in->num_queries] + 1)));
    }
    if (B->batch < 1) B->batch = 1;
    if (B->batch > in->num_queries) B->batch = in->num_queries;
    if (o->consumer == PROFILE)
        B->qnode = checked(malloc(sizeof(int32_t) * (size_t)B->batch));
    const size_t rows = (size_t)total * B->batch;
    if (entry_slots)
        alloc_slots(&B->all, rows, nm, g->nmatch, lsoln);
    if (g->nmatch)
        B->restarts = checked(malloc(sizeof(int32_t) * rows * nm));
    if (o->out == OUT_LISTING && in->cls_count[1] > 0)
        alloc_slots(&B->large, (size_t)in->cls_count[1] * in->num_queries, nm, g->nmatch, lsoln);
    if (o->csr) {
        B->hits_cap = has(g, 'p') ? 1024 : B->kk * B->batch;
        B->pcounts = checked(malloc(sizeof(int32_t) * (size_t)B->batch));
        alloc_hits(B, (size_t)B->hits_cap, lsoln);
    } else if (g->topk > 0) {
        alloc_hits(B, (size_t)B->kk * B->batch, lsoln);  /* only K rows per query (and GPU) ever leave the GPUs */
    }
    B->n1s = checked(malloc(sizeof(int32_t) * (size_t)B->batch));
    if (has(g, 'X') && has(g, 'F'))
        B->base_fits = checked(calloc((size_t)B->batch, sizeof(sat_fit)));
    if (queries_from_db(o) && in->motifs)
        B->sse_begin = checked(malloc(sizeof(int32_t) * ((size_t)B->batch + 1)));
    if (queries_from_db(o))
        return;
    B->qtabs = checked(calloc((size_t)B->batch * SAT_MAXDIM * SAT_MAXDIM, 1));
    B->qdmats = checked(calloc((size_t)B->batch * SAT_MAXDIM * SAT_MAXDIM, sizeof(float)));
    B->qtypes = checked(calloc((size_t)B->batch * SAT_MAXDIM, 1));
}

static void free_slots(slots *s)
{
    free(s->counts);
    free(s->scores);
    free(s->maps);
}

/* -M: room for the slots of `rows` ranked rows */
static void alloc_rowm(gpu_bufs *B, size_t rows, int nm, int lsoln)
{
    if (rows <= B->rowm_cap)
        return;
    free_slots(&B->rowm);
    free(B->rowm_restarts);
    free(B->pair_q);
    free(B->pair_e);
    alloc_slots(&B->rowm, rows, nm, 1, lsoln);
    B->rowm_restarts = checked(malloc(sizeof(int32_t) * rows * (size_t)nm));
    B->pair_q = checked(malloc(sizeof(int32_t) * rows));
    B->pair_e = checked(malloc(sizeof(int32_t) * rows));
    B->rowm_cap = rows;
}

static void free_gpu_bufs(gpu_bufs *B)
{
    free(B->n1s);
    free(B->sse_begin);
    free(B->qnode);
    free(B->phits);
    free(B->pjoint);
    free(B->poff);
    free(B->qtabs);
    free(B->qtypes);
    free(B->qdmats);
    free_slots(&B->all);
    free(B->restarts);
    free_slots(&B->large);
    free(B->hits);
    free(B->rhits);
    free(B->base_fits);
    free(B->hit_maps);
    free(B->pcounts);
    free_slots(&B->rowm);
    free(B->rowm_restarts);
    free(B->pair_q);
    free(B->pair_e);
    free(B->evals);
    sat_classes_free(&B->classes);
}

/* One multi-GPU context holding the database: it is cut into contiguous shards of equal COST (entries of a
 * size-sorted database differ several-fold in cost, sat_shard.h), every GPU holds its shard, a search is queued on
 * all of them and one gather (RCCL over xGMI) brings the rows to device 0. */
static sat_multi *open_multi(const options *o, const input *in)
{
    const int total = in->db.count, ndev = sat_device_count(), nlist = o->g->ndev_list;
    if (ndev <= 0)
        die("There is no usable HIP device (use -c for the host mode).\n");
    fprintf(stderr, "found %d HIP devices\n", ndev);
    int ngpu = o->g->want_gpus > 0 ? o->g->want_gpus : ndev;
    if (ngpu > ndev) ngpu = ndev;
    if (nlist > 0) ngpu = nlist;
    if (ngpu > total) ngpu = total;
    const double t0 = now_ms();
    sat_multi *multi = sat_multi_create(ngpu, nlist > 0 ? o->g->dev_list : NULL, o->g->seed);
    if (!multi)
        die("sat_multi_create(%d) failed: %s\n", ngpu, sat_last_error());
    if (sat_multi_db_upload_packed(multi, total, in->db.order, in->db.cell_off, in->db.tab, in->db.dist) != SAT_OK)
        die("database upload failed: %s\n", sat_last_error());
    fprintf(stderr, "Copied %d entries to %d GPU(s) in %f ms (gather: %s)\n", total, ngpu, now_ms() - t0,
            sat_multi_gather_kind(multi));
    if (ngpu > 1) {
        int32_t *begin = checked(malloc(sizeof(int32_t) * (size_t)(ngpu + 1)));
        if (sat_multi_shards(multi, begin) == SAT_OK)
            for (int g = 0; g < ngpu; g++)
                fprintf(stderr, "  GPU %d: entries %d .. %d\n", g, begin[g], begin[g + 1] - 1);
        free(begin);
    }
    return multi;
}

/* -X, and -p / -k with -F: the rows of the search just made whose p-value is <= pmax, selected on the GPUs into the
 * buffers as they are.  Returns the rows there are */
static int select_rows(const options *o, sat_multi *multi, gpu_bufs *B, double pmax)
{
    const given *g = o->g;
    if (has(g, 'X'))
        return sat_multi_reorder_hits(multi, pmax, g->bmin, o->kinds, g->topk, B->pcounts, B->hits_cap, B->rhits, B->hit_maps);
    return sat_multi_hits_cutoff(multi, pmax, g->topk, B->pcounts, B->hits_cap, B->hits, B->hit_maps);
}

/* rc rows were selected: where the buffers were short of them, they are grown and the rows selected again */
static int grow_and_select(const options *o, const input *in, sat_multi *multi, gpu_bufs *B, double pmax, int rc)
{
    if (rc <= B->hits_cap)
        return rc;
    B->hits_cap = rc;
    alloc_hits(B, (size_t)rc, in->lsoln);
    return select_rows(o, multi, B, pmax);
}

/* The mode's search of the batch set last.  Returns rows per query (-k, -R), the batch's rows (-p), 0 (listing, -m)
 * or a negative SAT_E* code. */
static int search_batch(const options *o, const input *in, sat_multi *multi, gpu_bufs *B, sat_fit *fits, double *ms,
                        double *ms_stage2)
{
    const given *g = o->g;
    const int lorder = in->lorder, lsoln = in->lsoln, maxstart = g->maxstart, fit = has(g, 'F');
    if (o->out == OUT_NONE) {
        /* -L, -H, -D, -E: the rows stay on the GPUs (no gather, no LSOLN: no map is printed); with -F the fit is installed
         * there.  -W: the same with LSOLN on, whatever the input says - the maps are what it counts, where they are */
        const int maps = o->consumer == PROFILE;
        if (fit)
            return sat_multi_search_fit(multi, lorder, maps, maxstart, g->censor, fits, ms);
        return sat_multi_search_only(multi, lorder, maps, maxstart, ms);
    }
    if (has(g, 'X')) {
        /* -X: the ordered search without maps, fitted (-F) and kept on the GPUs as the baseline; the unordered search with
         * maps, fitted to its own scores; then of -p's rows those the baseline does not call a hit and whose map is of
         * one of the kinds */
        double ms2 = 0.0;
        int rc = fit ? sat_multi_search_fit(multi, 1, 0, maxstart, g->censor, B->base_fits, ms)
                     : sat_multi_search_only(multi, 1, 0, maxstart, ms);
        if (rc == SAT_OK)
            rc = sat_multi_baseline_keep(multi);
        if (rc == SAT_OK)
            rc = fit ? sat_multi_search_fit(multi, 0, 1, maxstart, g->censor, fits, &ms2)
                     : sat_multi_search_only(multi, 0, 1, maxstart, &ms2);
        *ms += ms2;
        if (rc != SAT_OK)
            return rc;
        rc = grow_and_select(o, in, multi, B, g->pmax, select_rows(o, multi, B, g->pmax));
        for (int r = 0; r < rc; r++)
            B->hits[r] = B->rhits[r].hit;
        return rc;
    }
    if (fit && o->out == OUT_RANKED) {
        /* search, histogram and fit on the GPUs (fits: the batch's), then the rows by the fitted p-values: those under
         * -p's cutoff, or with -k alone (every p-value is <= 1) the K best */
        const int rc = sat_multi_search_fit(multi, lorder, lsoln, maxstart, g->censor, fits, ms);
        if (rc != SAT_OK)
            return rc;
        const double pmax = has(g, 'p') ? g->pmax : 1.0;
        return grow_and_select(o, in, multi, B, pmax, select_rows(o, multi, B, pmax));
    }
    if (has(g, 'p')) {
        /* every row of the batch under the cutoff, selected with the search */
        const int rc = sat_multi_search_cutoff(multi, lorder, lsoln, maxstart, g->pmax, g->topk, B->pcounts, B->hits_cap, B->hits,
                                               B->hit_maps, ms);
        return grow_and_select(o, in, multi, B, g->pmax, rc);
    }
    if (o->polish == POLISH_CANDIDATES)
        return sat_multi_search_refine_polish(multi, lorder, lsoln, maxstart, o->ncand, g->refine ? g->refine : maxstart, o->tops,
                                              B->kk, B->hits, B->hit_maps, NULL, NULL, ms);
    if (g->refine)
        return sat_multi_search_refine(multi, lorder, lsoln, maxstart, o->ncand, g->refine, B->kk, B->hits,
                                       B->hit_maps, NULL, ms, ms_stage2);
    if (g->nmatch) {
        /* match 0 of every entry is the plain search's score and map: the listing's rows come from the match slots;
         * -k ranks the entries as without -m (its own search), the extra rows from the slots */
        int rc = sat_multi_search_matches(multi, lorder, maxstart, o->nm, B->all.counts, B->all.scores, B->restarts,
                                          B->all.maps, ms);
        if (rc == SAT_OK && g->topk > 0) {
            double ms2 = 0.0;
            rc = sat_multi_search_topk(multi, lorder, lsoln, maxstart, B->kk, B->hits, B->hit_maps, &ms2);
            *ms += ms2;
        }
        return rc;
    }
    if (g->topk > 0)
        return sat_multi_search_topk(multi, lorder, lsoln, maxstart, B->kk, B->hits, B->hit_maps, ms);
    return sat_multi_search(multi, lorder, lsoln, maxstart, B->all.scores, B->all.maps, ms);
}

/* -M: the matches of the batch's ranked rows and of nothing else - a pair-match search of the rows search_batch chose
 * (rc of them per query, with -p pcounts[b]), at the restarts their scores come from (-R: stage 2's), so that slot 0 of
 * a row is the row itself.  Only these rows' slots come to the host. */
static int match_ranked_rows(const options *o, const input *in, sat_multi *multi, gpu_bufs *B, int nqb, int rc,
                             double *ms)
{
    size_t rows = 0;
    for (int b = 0; b < nqb; b++)
        rows += (size_t)(o->csr ? B->pcounts[b] : rc);
    alloc_rowm(B, rows ? rows : 1, o->g->rowmatch, in->lsoln);
    size_t r = 0;
    for (int b = 0; b < nqb; b++)
        for (size_t n = (size_t)(o->csr ? B->pcounts[b] : rc); n > 0; n--, r++) {
            B->pair_q[r] = b;
            B->pair_e[r] = B->hits[r].entry;
        }
    return sat_multi_search_pairs_matches(multi, in->lorder, o->g->refine ? o->g->refine : o->g->maxstart, o->g->rowmatch, (int)rows,
                                          B->pair_q, B->pair_e, B->rowm.counts, B->rowm.scores, B->rowm_restarts,
                                          B->rowm.maps, ms);
}

/* The blocks of queries q0 .. q0 + nqb - 1.  Ranked: each query's rows (-p: pcounts[b] rows of query b after those of
 * the queries before it, else rc a query).  Listing: each query's small-class rows; its large-class slots are kept
 * for the deferred block. */
static void print_batch(const options *o, const input *in, gpu_bufs *B, const sat_fit *fits, int q0, int nqb, int rc)
{
    const slots *all = &B->all, *large = &B->large;
    const size_t nm = (size_t)all->nm;
    size_t first = 0;
    for (int b = 0; b < nqb; b++) {
        const size_t row0 = (size_t)b * in->db.count;
        print_header(in, q0 + b, fits ? &fits[q0 + b] : NULL);
        if (has(o->g, 'X')) {
            /* -X: one more header line (two with -F: the ordered search's fit), then the rows with their six columns,
             * each followed by the unordered map's lines.  Few rows: printf formats them. */
            char kt[4];
            const int n1 = B->n1s[b];
            out_fmt("# REORDER ordered pvalue >= %g kinds = %s\n", o->g->bmin, kinds_text(o->kinds, kt));
            if (B->base_fits)
                out_gumbel(&B->base_fits[b], "ordered ");
            for (size_t r = first; r < first + (size_t)B->pcounts[b]; r++) {
                const sat_reorder_hit *h = &B->rhits[r];
                const char *kind = h->kind == SAT_KIND_SEQUENTIAL ? "seq" : h->kind == SAT_KIND_CIRCULAR ? "circ" : "perm";
                out_fmt("%-8s %d %g %g %g %d %g %s %d %d %d\n", sat_set_name(&in->db, h->hit.entry), h->hit.score, h->hit.norm2,
                        h->hit.zscore, h->hit.pvalue, h->base_score, h->base_pvalue, kind, h->matched, h->descents, h->cut);
                const int32_t *map = B->hit_maps + r * SAT_MAXDIM;
                for (int k = 0; k < n1; k++)
                    if (map[k] >= 0)
                        out_map_line(k + 1, map[k] + 1);
            }
            first += (size_t)B->pcounts[b];
            continue;
        }
        if (o->out == OUT_RANKED) {
            const size_t nrows = (size_t)(o->csr ? B->pcounts[b] : rc);
            for (size_t r = first; r < first + nrows; r++)
                print_entry(in, B->hits[r].entry, B->n1s[b], &B->hits[r],
                            B->hit_maps ? B->hit_maps + r * SAT_MAXDIM : NULL, o->g->rowmatch ? &B->rowm : all,
                            o->g->rowmatch ? r : row0 + B->hits[r].entry, 0);
            first += nrows;
            continue;
        }
        for (int d = 0; d < in->cls_count[0]; d++)
            print_entry(in, in->cls_index[0][d], B->n1s[b], NULL, NULL, all, row0 + in->cls_index[0][d], 0);
        for (int d = 0; d < in->cls_count[1]; d++) {
            const size_t to = (size_t)(q0 + b) * in->cls_count[1] + d, from = row0 + in->cls_index[1][d];
            memcpy(large->scores + to * nm, all->scores + from * nm, sizeof(int32_t) * nm);
            if (all->counts)
                large->counts[to] = all->counts[from];
            if (all->maps)
                memcpy(large->maps + to * nm * SAT_MAXDIM, all->maps + from * nm * SAT_MAXDIM,
                       sizeof(int32_t) * SAT_MAXDIM * nm);
        }
    }
}

static int count_singletons(const int32_t *size, int n)
{
    int singletons = 0;
    for (int v = 0; v < n; v++)
        singletons += size[v] == 1;
    return singletons;
}

/* -L, -D: the table of the clustering the GPUs hold, "name representative size degree" a structure.  -L: labels, degrees
 * and the edge count cross to the host (8 bytes a structure and shard), the representatives and sizes are
 * sat_cluster_reps'.  -D: the cover the GPUs solved - representatives and degrees (8 bytes a structure), the edge and
 * round counts; the sizes are sat_cover_sizes', and the library has checked the cover's two invariants before it returned */
static int print_clusters(const options *o, const input *in, sat_multi *multi, const sat_fit *fits)
{
    const int n = in->db.count, cover = o->consumer == COVER;
    int32_t *label = checked(malloc(sizeof(int32_t) * (size_t)n * 4)), *degree = label + n, *rep = degree + n, *size = rep + n;
    unsigned long long edges = 0;
    int rounds = 0;
    if ((cover ? sat_multi_cover_solve(multi, rep, degree, &edges, &rounds)
               : sat_multi_cluster_labels(multi, label, degree, &edges)) != SAT_OK) {
        fprintf(stderr, "clustering failed: %s\n", sat_last_error());
        free(label);
        return 1;
    }
    const int clusters = cover ? sat_cover_sizes(n, rep, size) : sat_cluster_reps(n, label, degree, rep, size);
    if (clusters < 0)
        die(cover ? "ERROR: the GPUs returned representatives that are no cover\n"
                  : "ERROR: the GPUs returned labels that are no clustering\n");
    out_fmt("# %s dbfile = %s entries = %d pvalue <= %g restarts = %d clusters = %d singletons = %d edges = %llu",
            cover ? "COVER" : "CLUSTER", in->dbfile, n, cover ? o->g->dmax : o->g->lmax, o->g->maxstart, clusters,
            count_singletons(size, n), edges);
    if (cover)
        out_fmt(" rounds = %d", rounds);
    out_bytes("\n", 1);
    out_bytes(polish_header, strlen(polish_header));
    out_fitted(o, fits, n);
    for (int v = 0; v < n; v++)
        out_fmt("%-8s %-8s %d %d\n", sat_set_name(&in->db, v), sat_set_name(&in->db, rep[v]), size[v], degree[v]);
    free(label);
    return 0;
}

/* -H: the tables of the L clusterings the GPUs hold, side by side - per level what print_clusters prints for it: 8 bytes
 * a structure, level and shard cross to the host; the levels must be nested (sat_cluster_nested) */
static int print_cluster_levels(const options *o, const input *in, sat_multi *multi, const sat_fit *fits)
{
    const int n = in->db.count, nl = o->g->nlevels;
    const size_t cells = (size_t)n * (size_t)nl;
    int32_t *label = checked(malloc(sizeof(int32_t) * cells * 4)), *degree = label + cells, *rep = degree + cells, *size = rep + cells;
    unsigned long long edges[SAT_MAX_CLUSTER_LEVELS] = { 0 };
    if (sat_multi_cluster_labels_levels(multi, label, degree, edges) != SAT_OK) {
        fprintf(stderr, "clustering failed: %s\n", sat_last_error());
        free(label);
        return 1;
    }
    const int broken = sat_cluster_nested(n, nl, label);
    if (broken < 0)
        die("ERROR: the GPUs returned labels that are no clustering\n");
    if (broken > 0)
        die("ERROR: the clusters of level %d do not lie inside those of level %d\n", broken, broken + 1);
    out_fmt("# CLUSTER dbfile = %s entries = %d levels = %d restarts = %d\n", in->dbfile, n, nl, o->g->maxstart);
    for (int j = 0; j < nl; j++) {
        const size_t at = (size_t)j * (size_t)n;
        const int clusters = sat_cluster_reps(n, label + at, degree + at, rep + at, size + at);
        if (clusters < 0)
            die("ERROR: the GPUs returned labels that are no clustering\n");
        out_fmt("# LEVEL %d pvalue <= %g clusters = %d singletons = %d edges = %llu\n", j + 1, o->g->levels[j], clusters,
                count_singletons(size + at, n), edges[j]);
    }
    out_bytes(polish_header, strlen(polish_header));
    out_fitted(o, fits, n);
    for (int v = 0; v < n; v++) {
        out_fmt("%-8s", sat_set_name(&in->db, v));
        for (int j = 0; j < nl; j++) {
            const size_t at = (size_t)j * (size_t)n + (size_t)v;
            out_fmt(" %-8s %d %d", sat_set_name(&in->db, rep[at]), size[at], degree[at]);
        }
        out_bytes("\n", 1);
    }
    free(label);
    return 0;
}

/* -E: the table of the evaluation - the queries' rows as the GPUs reduced them (32 bytes a query crossed to the host);
 * the two ratios are taken here, and their means over the queries where both are defined */
static void print_eval(const options *o, const input *in, const gpu_bufs *B)
{
    const sat_classes *cl = &B->classes;
    /* (the class file's name and the class tokens are of any length: they go out as they are, not through out_fmt) */
    out_fmt("# EVAL dbfile = %s classes = ", in->dbfile);
    out_bytes(o->g->classfile, strlen(o->g->classfile));
    out_fmt(" entries = %d classified = %d distinct = %d restarts = %d rocn = %d\n", in->db.count, cl->classified, cl->distinct,
            o->g->maxstart, o->rocn);
    out_bytes(polish_header, strlen(polish_header));
    int defined = 0;
    double auc_sum = 0.0, rocn_sum = 0.0;
    for (int qi = 0; qi < in->num_queries; qi++) {
        const sat_eval *e = &B->evals[qi];
        if (e->positives > 0 && e->negatives > 0) {
            auc_sum += (double)e->u2 / (2.0 * (double)e->positives * (double)e->negatives);
            rocn_sum += (double)e->t2 / (2.0 * (double)e->positives * (double)e->n_used);
            defined++;
        }
    }
    if (defined)
        out_fmt("# MEAN queries = %d auc = %.6f rocn = %.6f\n", defined, auc_sum / defined, rocn_sum / defined);
    else
        out_fmt("# MEAN queries = 0 auc = NA rocn = NA\n");
    for (int qi = 0; qi < in->num_queries; qi++) {
        const sat_eval *e = &B->evals[qi];
        const char *token = e->query_class >= 0 && e->query_class < cl->distinct ? cl->token[e->query_class] : "-";
        out_fmt("%-8s ", sat_set_name(&in->db, in->qindex[qi]));
        out_bytes(token, strlen(token));
        out_fmt(" %d %d %llu %llu %d", e->positives, e->negatives, (unsigned long long)e->u2, (unsigned long long)e->t2, e->n_used);
        if (e->positives > 0 && e->negatives > 0)
            out_fmt(" %.6f %.6f\n", (double)e->u2 / (2.0 * (double)e->positives * (double)e->negatives),
                    (double)e->t2 / (2.0 * (double)e->positives * (double)e->n_used));
        else
            out_fmt(" NA NA\n");
    }
}

/* -W: the table of the profiles - every query's hits and matrix as the GPUs counted them (4 + 4 n1 n1 bytes a query
 * crossed to the host); the core is sat_profile_core's.  A motif's core is written in its source entry's numbering */
static void print_profiles(const options *o, const input *in, const gpu_bufs *B, const sat_fit *fits)
{
    static const char *tname[4] = { "e", "xa", "xi", "xg" };
    out_fmt("# PROFILE dbfile = %s pvalue <= %g fraction >= %g restarts = %d queries = %d\n", in->dbfile, o->g->wmax, o->core,
            o->g->maxstart, in->num_queries);
    out_bytes(polish_header, strlen(polish_header));
    out_fitted(o, fits, in->num_queries);
    uint8_t in_core[SAT_MAXDIM];
    for (int qi = 0; qi < in->num_queries; qi++) {
        int qs;
        const sat_struct_set *qset = query_set(in, qi, &qs);
        const int n1 = qset->order[qs], motif = in->motifs && in->qsub[qi] >= 0;
        const char *name = sat_set_name(in->qsrc, in->qindex[qi]);
        const uint32_t *joint = B->pjoint + B->poff[qi];
        out_fmt("# QUERY %s sses = %d hits = %u\n", name, n1, B->phits[qi]);
        out_query_sses(in, qi);
        uint32_t joint_min = 0;
        const int core = sat_profile_core(n1, B->phits[qi], joint, o->core, in_core, &joint_min);
        if (core < 0)
            die("ERROR: no core for query %s\n", name);
        if (core == 0) {
            out_bytes("# CORE none\n", 12);
        } else {
            out_fmt("# CORE sses = %d joint >= %u %s@", core, joint_min, name);
            for (int i = 0, first = 1; i < n1; i++)
                if (in_core[i]) {
                    out_fmt(first ? "%d" : ",%d", motif ? in->sse[in->sse_begin[qi] + i] + 1 : i + 1);
                    first = 0;
                }
            out_bytes("\n", 1);
        }
        const uint8_t *tab = qset->tab + qset->cell_off[qs];
        for (int i = 0; i < n1; i++) {
            out_fmt("%d %s %u", i + 1, tname[tab[(size_t)i * (i + 1) / 2 + i] & 3], joint[(size_t)i * n1 + i]);
            for (int k = 0; k < n1; k++)
                out_fmt(" %u", joint[(size_t)i * n1 + k]);
            out_bytes("\n", 1);
        }
    }
}

/* The on-GPU consumer of the run's rows (-L, -H, -D, -E, -W; none: nothing to do), in three steps.  Before the first
 * batch: its accumulator on the GPUs */
static int consumer_begin(const options *o, sat_multi *multi, const gpu_bufs *B)
{
    switch (o->consumer) {
    case CLUSTER: return sat_multi_cluster_begin(multi);
    case CLUSTER_LEVELS: return sat_multi_cluster_begin_levels(multi, o->g->nlevels, o->g->levels);
    case COVER: return sat_multi_cover_begin(multi);
    case EVAL: return sat_multi_eval_classes(multi, B->classes.node_class);
    default: return SAT_OK;
    }
}

/* After each batch's search: its rows of queries q0 .. q0 + nqb - 1 taken in where they are.  Query b is structure
 * qindex[q0 + b] of the database; for -W when it was taken from there (a motif: its source entry), else no structure of it */
static int consumer_add(const options *o, const input *in, sat_multi *multi, gpu_bufs *B, int q0, int nqb)
{
    const int *entries = in->qindex + q0;
    switch (o->consumer) {
    case CLUSTER: return sat_multi_cluster_add(multi, o->g->lmax, entries);
    case CLUSTER_LEVELS: return sat_multi_cluster_add_levels(multi, entries);
    case COVER: return sat_multi_cover_add(multi, o->g->dmax, entries);
    case EVAL: return sat_multi_eval_rows(multi, entries, o->rocn, B->evals + q0);
    case PROFILE:
        for (int b = 0; b < nqb; b++)
            B->qnode[b] = o->dbfile ? entries[b] : -1;
        return sat_multi_profile_rows(multi, o->g->wmax, B->qnode, B->phits + q0, B->pjoint + B->poff[q0], NULL);
    default: return SAT_OK;
    }
}

/* After the last batch: its table.  Returns the run's status */
static int consumer_print(const options *o, const input *in, sat_multi *multi, const gpu_bufs *B, const sat_fit *fits)
{
    switch (o->consumer) {
    case CLUSTER: case COVER: return print_clusters(o, in, multi, fits);
    case CLUSTER_LEVELS: return print_cluster_levels(o, in, multi, fits);
    case EVAL: print_eval(o, in, B); return 0;
    case PROFILE: print_profiles(o, in, B, fits); return 0;
    default: return 0;
    }
}

/* -Q, -a: the batch q0 .. q0 + nqb - 1 from its entries' indices in the database the GPUs hold; where the run has a motif,
 * with the batch's lists, their offsets counted from the batch's first.  Else the structures expanded here and copied */
static int set_queries(const options *o, const input *in, sat_multi *multi, gpu_bufs *B, int q0, int nqb)
{
    if (!queries_from_db(o))
        return sat_multi_queries_set(multi, nqb, B->n1s, B->qtabs, B->qdmats, SAT_MAXDIM, B->qtypes, (uint32_t)q0);
    if (!in->motifs)
        return sat_multi_queries_from_db(multi, nqb, in->qindex + q0, (uint32_t)q0);
    for (int b = 0; b <= nqb; b++)
        B->sse_begin[b] = in->sse_begin[q0 + b] - in->sse_begin[q0];
    return sat_multi_queries_from_db_sses(multi, nqb, in->qindex + q0, B->sse_begin, in->sse + in->sse_begin[q0], (uint32_t)q0);
}

static int run_gpu(const options *o, const input *in)
{
    const given *g = o->g;
    const int total = in->db.count, fit = has(g, 'F'), stage2 = g->refine ? g->refine : g->maxstart;
    int status = 0;
    gpu_bufs B;
    alloc_gpu_bufs(o, in, &B);
    if (queries_from_db(o) && in->motifs && !sat_multi_queries_from_db_sses)
        die("ERROR: this library has no sat_multi_queries_from_db_sses\n");
    sat_multi *multi = open_multi(o, in);
    if (o->polish == POLISH_CANDIDATES)
        snprintf(polish_header, sizeof polish_header, "# POLISH tops = %d restarts = %d candidates = %d\n", o->tops, stage2, o->ncand);
    if (o->polish == POLISH_ALL) {
        snprintf(polish_header, sizeof polish_header, "# POLISH tops = %d all rows\n", o->tops);
        if (sat_multi_polish_all_set(multi, o->tops) != SAT_OK)
            die("ERROR: %s\n", sat_last_error());
    }
    /* -F: every query's fit - from the GPUs with -k / -p, else made here from the listing's scores (the whole
     * database's, both size classes: a query's two blocks carry the same line) */
    sat_fit *fits = fit ? checked(calloc((size_t)in->num_queries, sizeof(sat_fit))) : NULL;
    if (consumer_begin(o, multi, &B) != SAT_OK)
        die("ERROR: %s\n", sat_last_error());
    for (int q0 = 0; q0 < in->num_queries; q0 += B.batch) {
        const int nqb = in->num_queries - q0 < B.batch ? in->num_queries - q0 : B.batch;
        for (int b = 0; b < nqb; b++) {
            int qs;
            const sat_struct_set *qset = query_set(in, q0 + b, &qs);
            B.n1s[b] = qset->order[qs];
            if (queries_from_db(o))
                continue;
            uint8_t *tab = B.qtabs + (size_t)b * SAT_MAXDIM * SAT_MAXDIM;
            sat_set_expand(qset, qs, SAT_MAXDIM, tab, B.qdmats + (size_t)b * SAT_MAXDIM * SAT_MAXDIM);
            for (int i = 0; i < B.n1s[b]; i++)
                B.qtypes[(size_t)b * SAT_MAXDIM + i] = tab[i * SAT_MAXDIM + i];
        }
        fprintf(stderr, "Executing simulated annealing tableaux match kernel on GPU for %d quer%s (from %s)...\n",
                nqb, nqb == 1 ? "y" : "ies", sat_set_name(in->qsrc, in->qindex[q0]));
        double ms = 0.0, ms_stage2 = 0.0;
        /* the library calls of a batch, in this order: queries set, search, consumer add, then -M */
        int rc = set_queries(o, in, multi, &B, q0, nqb);
        if (rc == SAT_OK)
            rc = search_batch(o, in, multi, &B, fits ? fits + q0 : NULL, &ms, &ms_stage2);
        if (rc == SAT_OK)
            rc = consumer_add(o, in, multi, &B, q0, nqb);
        if (rc < 0) {
            fprintf(stderr, "kernel launch failed: %s\n", sat_last_error());
            status = 1;
            break;
        }
        if (g->rowmatch) {
            double ms_rows = 0.0;
            if (match_ranked_rows(o, in, multi, &B, nqb, rc, &ms_rows) != SAT_OK) {
                fprintf(stderr, "kernel launch failed: %s\n", sat_last_error());
                status = 1;
                break;
            }
            fprintf(stderr, "matches of the printed rows: %f ms\n", ms_rows);
        }
        fprintf(stderr, "GPU execution time %f ms\n", ms);
        if (o->polish == POLISH_CANDIDATES)
            fprintf(stderr, "polish: %d candidates per query x %d restarts, %d maps each\n", o->ncand < total ? o->ncand : total,
                    stage2, o->tops);
        else if (o->polish == POLISH_ALL)
            fprintf(stderr, "polish: every row, %d maps each\n", o->tops);
        else if (g->refine)
            fprintf(stderr, "refine: stage 2 %f ms, %d candidates per query x %d restarts\n", ms_stage2,
                    o->ncand < total ? o->ncand : total, g->refine);
        fprintf(stderr, "%f million iterations/sec\n",
                ((double)total * nqb * ((double)g->maxstart * SAT_MAXITER) / (ms / 1000)) / 1.0e6);
        if (o->out == OUT_NONE)
            continue;
        if (fit && o->out == OUT_LISTING)
            for (int b = 0; b < nqb; b++)
                fits[q0 + b] = fit_scores(B.all.scores + (size_t)b * total, total, B.n1s[b], in->db.order, g->censor);
        print_batch(o, in, &B, fits, q0, nqb, rc);
    }
    if (!status)
        status = consumer_print(o, in, multi, &B, fits);
    /* the listing's deferred block: every query's large-class rows, after all small-class blocks, with the reference
     * GPU path's two blanks before the p-value */
    if (!status && o->out == OUT_LISTING && in->cls_count[1] > 0)
        for (int qi = 0; qi < in->num_queries; qi++) {
            print_header(in, qi, fits ? &fits[qi] : NULL);
            for (int d = 0; d < in->cls_count[1]; d++)
                print_entry(in, in->cls_index[1][d], query_order(in, qi), NULL, NULL, &B.large,
                            (size_t)qi * in->cls_count[1] + d, 1);
        }
    fprintf(stderr, "copied %llu bytes of results from the GPU(s)\n", sat_multi_stat_d2h_bytes(multi));
    sat_multi_destroy(multi);
    free_gpu_bufs(&B);
    free(fits);
    return status;
}

int main(int argc, char *argv[])
{
    given g;
    options o;
    parse_options(argc, argv, &g);
    plan_run(&g, &o);
    fprintf(stderr, "MAXDIM = %d\n", SAT_MAXDIM);
    atexit(out_flush);                                   /* every exit path, exit(1) included */
    input in;
    memset(&in, 0, sizeof in);
    sat_set_init(&in.queries);
    sat_set_init(&in.db);
    read_queries(&o, &in);
    load_database(&o, &in);
    fprintf(stderr, "maxstart = %d\n", g.maxstart);
    const int status = has(&g, 'c') ? run_host(&o, &in) : run_gpu(&o, &in);
    free_input(&in);
    free(norm2_cache);
    free(fit_store);
    return status;
}
