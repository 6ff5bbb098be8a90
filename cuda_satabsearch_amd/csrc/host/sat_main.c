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

static void *checked(void *p)
{
    if (!p)
        die("malloc failed\n");
    return p;
}

typedef struct {
    int use_gpu, maxstart, want_gpus, bincache, topk, nmatch, refine, ncand, cutoff;
    int rowmatch;                     /* -M: matches of each printed row */
    int fit;                          /* -F: statistics fitted to each query's own scores */
    int polish;                       /* -P: maps polished per candidate */
    int polish_all;                   /* -P T -A: maps polished per row of every search (then polish is 0) */
    double censor;                    /* -F: the right-censored fraction of the rows */
    double pmax;                      /* -p: the largest p-value printed */
    int cluster;                      /* -L: cluster the database instead of printing rows */
    double lmax;                      /* -L: the largest p-value of an edge */
    int nlevels;                      /* -H: the cutoffs' count (then cluster is set too: the run is -L's but for its adds and its table) */
    double levels[SAT_MAX_CLUSTER_LEVELS];  /* -H: the largest p-value of an edge of each level, ascending */
    int cover;                        /* -D: cluster around representatives (then cluster is set too: the run is -L's but for its adds and its table) */
    double dmax;                      /* -D: the largest p-value of an edge */
    const char *classfile;            /* -E: score the search against this classification instead of printing rows */
    int rocn;                         /* -N: the negatives ROC-n counts up to (0: not given) */
    int profile;                      /* -W: profile each query's SSEs over its hits instead of printing rows */
    double wmax;                      /* -W: the largest p-value of a hit */
    int reorder;                      /* -X: only the rows that are hits out of sequence order alone */
    double bmin;                      /* -X: the smallest ordered p-value of such a row */
    int kinds;                        /* -x: SAT_KIND_* bits of the maps printed (0: not given) */
    int core_given;                   /* -f was given */
    double core;                      /* -f: the fraction of the hits every pair of the core is matched together in */
    unsigned long long seed;
    const char *qfile;                /* -q, -Q, -a: the database; stdin lists the query SIDs (not with -a) */
    const char *from_db;              /* -Q, -a: the database again - the batches are set from entry indices on the GPUs */
    const char *all;                  /* -a: the database again - every entry is a query */
    int dev_list[64], ndev_list;
    /* what the run prints, derived once the options are checked */
    int ranked;                       /* -k / -p / -R: each query's ranked rows; else the listing in class order */
    int csr;                          /* -p, and -k with -F: a row count per query (pcounts) instead of K rows each */
    int nm;                           /* slots per entry: M of -m, else 1 */
} options;

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

/* The three '#' lines that open a block of query qi; with -F (f: the query's fit) a fourth, and the statistics of the
 * rows that follow are f's */
static void print_header(const input *in, int qi, const sat_fit *f)
{
    char line[SAT_MAX_LINE_LEN + 64];
    int n = snprintf(line, sizeof line, "# cudaSaTabsearch LTYPE = %c LORDER = %c LSOLN = %c\n",
                     in->ltype ? 'T' : 'F', in->lorder ? 'T' : 'F', in->lsoln ? 'T' : 'F');
    out_bytes(line, (size_t)n);
    n = snprintf(line, sizeof line, "# QUERY ID = %-8s\n", sat_set_name(in->qsrc, in->qindex[qi]));
    out_bytes(line, (size_t)n);
    n = snprintf(line, sizeof line, "# DBFILE = %-80s\n", in->dbfile);
    out_bytes(line, (size_t)n);
    if (in->motifs && in->qsub[qi] >= 0) {
        /* the list as numbers, 1-based, ranges expanded, in the order given */
        out_bytes("# QUERY SSES = ", 15);
        for (int32_t k = in->sse_begin[qi]; k < in->sse_begin[qi + 1]; k++) {
            n = snprintf(line, sizeof line, k > in->sse_begin[qi] ? ",%d" : "%d", in->sse[k] + 1);
            out_bytes(line, (size_t)n);
        }
        out_bytes("\n", 1);
    }
    out_bytes(polish_header, strlen(polish_header));
    begin_query_stats(f);
    if (!f)
        return;
    if (f->fitted) {
        n = snprintf(line, sizeof line, "# GUMBEL a = %.17g b = %.17g rows = %d censored = %d below = %d\n", f->a, f->b,
                     f->rows, f->censored, f->below);
    } else {
        n = snprintf(line, sizeof line, "# GUMBEL not fitted\n");
        fprintf(stderr, "WARNING: no Gumbel fit for query %s: its rows keep the built-in statistics\n",
                sat_set_name(in->qsrc, in->qindex[qi]));
    }
    out_bytes(line, (size_t)n);
}

/* -H's list into o->levels / o->nlevels; 0: not 1 .. SAT_MAX_CLUSTER_LEVELS numbers in [0, 1], strictly ascending, the
 * whole argument */
static int parse_levels(const char *arg, options *o)
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

/* The options, then the refusals in a fixed order (the tests pin it), all before the banner and any device call */
static void parse_options(int argc, char *argv[], options *o)
{
    *o = (options){ .use_gpu = 1, .maxstart = 128, .want_gpus = 1, .seed = SAT_DEFAULT_SEED };
    int c;
    while ((c = getopt(argc, argv, "cq:Q:a:r:g:G:s:bk:p:m:M:R:C:F:P:AL:H:E:N:D:W:f:X:x:")) != -1) {
        char *end = NULL;
        long v;
        switch (c) {
        case 'c': o->use_gpu = 0; break;
        case 'q': o->qfile = optarg; break;
        case 'Q': o->from_db = optarg; break;
        case 'a': o->all = optarg; break;
        case 'r': o->maxstart = atoi(optarg); break;
        case 'g': o->want_gpus = atoi(optarg); break;
        case 'G':
            for (char *tok = strtok(optarg, ","); tok && o->ndev_list < 64; tok = strtok(NULL, ","))
                o->dev_list[o->ndev_list++] = atoi(tok);
            break;
        case 's': o->seed = strtoull(optarg, NULL, 0); break;
        case 'b': o->bincache = 1; break;
        case 'A': o->polish_all = 1; break;
        case 'k': o->topk = atoi(optarg); break;
        case 'p':
            /* the whole argument, a finite number >= 0 */
            o->pmax = strtod(optarg, &end);
            if (end == optarg || *end != '\0' || !isfinite(o->pmax) || o->pmax < 0.0) {
                fprintf(stderr, "ERROR: -p needs a p-value >= 0 (got '%s')\n", optarg);
                usage(argv[0]);
            }
            o->cutoff = 1;
            break;
        case 'L':
            /* the whole argument, a finite number in [0, 1] */
            o->lmax = strtod(optarg, &end);
            if (end == optarg || *end != '\0' || !isfinite(o->lmax) || o->lmax < 0.0 || o->lmax > 1.0) {
                fprintf(stderr, "ERROR: -L needs a p-value in [0, 1] (got '%s')\n", optarg);
                usage(argv[0]);
            }
            o->cluster = 1;
            break;
        case 'D':
            /* the whole argument, a finite number in [0, 1] */
            o->dmax = strtod(optarg, &end);
            if (end == optarg || *end != '\0' || !isfinite(o->dmax) || o->dmax < 0.0 || o->dmax > 1.0) {
                fprintf(stderr, "ERROR: -D needs a p-value in [0, 1] (got '%s')\n", optarg);
                usage(argv[0]);
            }
            o->cover = 1;
            break;
        case 'W':
            /* the whole argument, a finite number in [0, 1] */
            o->wmax = strtod(optarg, &end);
            if (end == optarg || *end != '\0' || !isfinite(o->wmax) || o->wmax < 0.0 || o->wmax > 1.0) {
                fprintf(stderr, "ERROR: -W needs a p-value in [0, 1] (got '%s')\n", optarg);
                usage(argv[0]);
            }
            o->profile = 1;
            break;
        case 'X':
            /* the whole argument, a finite number in [0, 1] */
            o->bmin = strtod(optarg, &end);
            if (end == optarg || *end != '\0' || !isfinite(o->bmin) || o->bmin < 0.0 || o->bmin > 1.0) {
                fprintf(stderr, "ERROR: -X needs a p-value in [0, 1] (got '%s')\n", optarg);
                usage(argv[0]);
            }
            o->reorder = 1;
            break;
        case 'x':
            /* the whole argument, one or more of the letters s, c, n */
            o->kinds = parse_kinds(optarg);
            if (!o->kinds) {
                fprintf(stderr, "ERROR: -x needs letters of s, c, n (got '%s')\n", optarg);
                usage(argv[0]);
            }
            break;
        case 'f':
            /* the whole argument, a number in (0, 1] */
            o->core = strtod(optarg, &end);
            if (end == optarg || *end != '\0' || !(o->core > 0.0 && o->core <= 1.0)) {
                fprintf(stderr, "ERROR: -f needs a fraction in (0, 1] (got '%s')\n", optarg);
                usage(argv[0]);
            }
            o->core_given = 1;
            break;
        case 'H':
            /* the whole argument: 1 .. SAT_MAX_CLUSTER_LEVELS numbers, each as -L's, with commas between, strictly ascending */
            if (!parse_levels(optarg, o)) {
                fprintf(stderr, "ERROR: -H needs 1..%d ascending p-values in [0, 1] (got '%s')\n", SAT_MAX_CLUSTER_LEVELS, optarg);
                usage(argv[0]);
            }
            break;
        case 'F':
            /* the whole argument, a number in [0, 0.5] */
            o->censor = strtod(optarg, &end);
            if (end == optarg || *end != '\0' || !(o->censor >= 0.0 && o->censor <= 0.5)) {
                fprintf(stderr, "ERROR: -F needs a censored fraction in [0, 0.5] (got '%s')\n", optarg);
                usage(argv[0]);
            }
            o->fit = 1;
            break;
        case 'm':
            /* 1 .. SAT_MAX_MATCHES, digits only: anything else (0, a sign, text) is a usage error */
            v = strtol(optarg, &end, 10);
            if (end == optarg || *end != '\0' || v < 1 || v > SAT_MAX_MATCHES) usage(argv[0]);
            o->nmatch = (int)v;
            break;
        case 'M':
            /* 1 .. SAT_MAX_MATCHES, digits only */
            v = strtol(optarg, &end, 10);
            if (end == optarg || *end != '\0' || v < 1 || v > SAT_MAX_MATCHES) {
                fprintf(stderr, "ERROR: -M needs an integer 1..%d (got '%s')\n", SAT_MAX_MATCHES, optarg);
                usage(argv[0]);
            }
            o->rowmatch = (int)v;
            break;
        case 'P':
            /* 1 .. SAT_MAX_MATCHES, digits only */
            v = strtol(optarg, &end, 10);
            if (end == optarg || *end != '\0' || v < 1 || v > SAT_MAX_MATCHES) {
                fprintf(stderr, "ERROR: -P needs an integer 1..%d (got '%s')\n", SAT_MAX_MATCHES, optarg);
                usage(argv[0]);
            }
            o->polish = (int)v;
            break;
        case 'E': o->classfile = optarg; break;
        case 'N':
            /* positive, digits only */
            v = strtol(optarg, &end, 10);
            if (end == optarg || *end != '\0' || v < 1 || v > 0x7FFFFFFFL) {
                fprintf(stderr, "ERROR: -N needs an integer >= 1 (got '%s')\n", optarg);
                usage(argv[0]);
            }
            o->rocn = (int)v;
            break;
        case 'R':
        case 'C':
            /* positive, digits only */
            v = strtol(optarg, &end, 10);
            if (end == optarg || *end != '\0' || v < 1 || v > 0x7FFFFFFFL) {
                fprintf(stderr, "ERROR: -%c needs a positive integer (got '%s')\n", c, optarg);
                usage(argv[0]);
            }
            if (c == 'R') o->refine = (int)v;
            else o->ncand = (int)v;
            break;
        default: usage(argv[0]);
        }
    }
    if (o->kinds && !o->reorder) die("ERROR: -x needs -X B\n");
    if (o->reorder) {
        /* hits out of sequence order: -p's run, searched twice, with another selection */
        if (!o->use_gpu) die("ERROR: -X cannot be combined with -c\n");
        if (o->nmatch) die("ERROR: -X cannot be combined with -m\n");
        if (o->rowmatch) die("ERROR: -X cannot be combined with -M\n");
        if (o->refine) die("ERROR: -X cannot be combined with -R\n");
        if (o->ncand) die("ERROR: -X cannot be combined with -C\n");
        if (o->cluster) die("ERROR: -X cannot be combined with -L\n");
        if (o->nlevels) die("ERROR: -X cannot be combined with -H\n");
        if (o->cover) die("ERROR: -X cannot be combined with -D\n");
        if (o->classfile) die("ERROR: -X cannot be combined with -E\n");
        if (o->rocn) die("ERROR: -X cannot be combined with -N\n");
        if (o->profile) die("ERROR: -X cannot be combined with -W\n");
        if (!o->cutoff) die("ERROR: -X needs -p P\n");
        if (o->polish && !o->polish_all) die("ERROR: -X takes -P T only with -A\n");
        if (!sat_multi_search_only || !sat_multi_search_fit || !sat_multi_baseline_keep || !sat_multi_reorder_hits)
            die("ERROR: this library has no sat_multi_reorder_hits\n");
        if (!o->kinds) o->kinds = SAT_KIND_CIRCULAR | SAT_KIND_PERMUTED;
    }
    if (o->core_given && !o->profile) die("ERROR: -f needs -W P\n");
    if (o->profile) {
        /* profile: a run whose rows and maps stay on the GPUs; -q, -Q, -a and the stdin queries all feed it */
        if (!o->use_gpu) die("ERROR: -W cannot be combined with -c\n");
        if (o->topk) die("ERROR: -W cannot be combined with -k\n");
        if (o->cutoff) die("ERROR: -W cannot be combined with -p\n");
        if (o->nmatch) die("ERROR: -W cannot be combined with -m\n");
        if (o->rowmatch) die("ERROR: -W cannot be combined with -M\n");
        if (o->refine) die("ERROR: -W cannot be combined with -R\n");
        if (o->ncand) die("ERROR: -W cannot be combined with -C\n");
        if (o->nlevels) die("ERROR: -W cannot be combined with -H\n");
        if (o->cover) die("ERROR: -W cannot be combined with -D\n");
        if (o->cluster) die("ERROR: -W cannot be combined with -L\n");
        if (o->classfile) die("ERROR: -W cannot be combined with -E\n");
        if (o->rocn) die("ERROR: -W cannot be combined with -N\n");
        if (o->polish && !o->polish_all) die("ERROR: -W takes -P T only with -A\n");
        if (!sat_multi_search_only || !sat_multi_profile_rows || !sat_profile_core)
            die("ERROR: this library has no sat_multi_profile_rows\n");
        if (o->fit && !sat_multi_search_fit) die("ERROR: this library has no sat_multi_search_fit\n");
        if (!o->core_given) o->core = 0.5;
    }
    if (o->rocn && !o->classfile) die("ERROR: -N needs -E classfile\n");
    if (o->cover) {
        /* clustering around representatives: -L's run with another accumulator and another table */
        if (!o->use_gpu) die("ERROR: -D cannot be combined with -c\n");
        if (!o->all) die("ERROR: -D needs -a dbfile\n");
        if (o->topk) die("ERROR: -D cannot be combined with -k\n");
        if (o->cutoff) die("ERROR: -D cannot be combined with -p\n");
        if (o->nmatch) die("ERROR: -D cannot be combined with -m\n");
        if (o->rowmatch) die("ERROR: -D cannot be combined with -M\n");
        if (o->refine) die("ERROR: -D cannot be combined with -R\n");
        if (o->ncand) die("ERROR: -D cannot be combined with -C\n");
        if (o->cluster) die("ERROR: -D cannot be combined with -L\n");
        if (o->nlevels) die("ERROR: -D cannot be combined with -H\n");
        if (o->classfile) die("ERROR: -D cannot be combined with -E\n");
        if (!sat_multi_search_only || !sat_multi_cover_begin || !sat_multi_cover_add || !sat_multi_cover_solve || !sat_cover_sizes)
            die("ERROR: this library has no sat_multi_cover_add\n");
        if (o->fit && !sat_multi_search_fit) die("ERROR: this library has no sat_multi_search_fit\n");
        o->cluster = 1;                              /* (-L's own checks below ask nothing these have not) */
    }
    if (o->classfile) {
        /* evaluation: a run over queries of the database whose rows stay on the GPUs */
        if (!o->use_gpu) die("ERROR: -E cannot be combined with -c\n");
        if (!o->all && !o->from_db) die("ERROR: -E needs -a dbfile or -Q dbfile\n");
        if (o->topk) die("ERROR: -E cannot be combined with -k\n");
        if (o->cutoff) die("ERROR: -E cannot be combined with -p\n");
        if (o->nmatch) die("ERROR: -E cannot be combined with -m\n");
        if (o->rowmatch) die("ERROR: -E cannot be combined with -M\n");
        if (o->refine) die("ERROR: -E cannot be combined with -R\n");
        if (o->ncand) die("ERROR: -E cannot be combined with -C\n");
        if (o->fit) die("ERROR: -E cannot be combined with -F\n");
        if (o->cluster) die("ERROR: -E cannot be combined with -L\n");
        if (o->nlevels) die("ERROR: -E cannot be combined with -H\n");
        if (o->polish && !o->polish_all) die("ERROR: -E takes -P T only with -A\n");
        if (!sat_multi_search_only || !sat_multi_eval_classes || !sat_multi_eval_rows)
            die("ERROR: this library has no sat_multi_eval_rows\n");
        if (!o->rocn) o->rocn = 50;
    }
    if (o->nlevels) {
        /* clustering at several cutoffs: -L's run with another add call and another table */
        if (!o->use_gpu) die("ERROR: -H cannot be combined with -c\n");
        if (!o->all) die("ERROR: -H needs -a dbfile\n");
        if (o->cluster) die("ERROR: -H cannot be combined with -L\n");
        if (o->topk) die("ERROR: -H cannot be combined with -k\n");
        if (o->cutoff) die("ERROR: -H cannot be combined with -p\n");
        if (o->nmatch) die("ERROR: -H cannot be combined with -m\n");
        if (o->rowmatch) die("ERROR: -H cannot be combined with -M\n");
        if (o->refine) die("ERROR: -H cannot be combined with -R\n");
        if (o->ncand) die("ERROR: -H cannot be combined with -C\n");
        if (!sat_multi_search_only || !sat_multi_cluster_begin_levels || !sat_multi_cluster_add_levels ||
            !sat_multi_cluster_labels_levels || !sat_cluster_reps || !sat_cluster_nested)
            die("ERROR: this library has no sat_multi_cluster_add_levels\n");
        if (o->fit && !sat_multi_search_fit) die("ERROR: this library has no sat_multi_search_fit\n");
        o->cluster = 1;
    } else if (o->cluster) {
        /* clustering: an all-vs-all run whose rows stay on the GPUs */
        if (!o->use_gpu) die("ERROR: -L cannot be combined with -c\n");
        if (!o->all) die("ERROR: -L needs -a dbfile\n");
        if (o->topk) die("ERROR: -L cannot be combined with -k\n");
        if (o->cutoff) die("ERROR: -L cannot be combined with -p\n");
        if (o->nmatch) die("ERROR: -L cannot be combined with -m\n");
        if (o->rowmatch) die("ERROR: -L cannot be combined with -M\n");
        if (o->refine) die("ERROR: -L cannot be combined with -R\n");
        if (o->ncand) die("ERROR: -L cannot be combined with -C\n");
        if (!sat_multi_search_only || !sat_multi_cluster_begin || !sat_multi_cluster_add || !sat_multi_cluster_labels ||
            !sat_cluster_reps)
            die("ERROR: this library has no sat_multi_cluster_add\n");
        if (o->fit && !sat_multi_search_fit) die("ERROR: this library has no sat_multi_search_fit\n");
    }
    if (o->from_db || o->all) {
        /* queries from the resident database: from here on the run is a -q run over that file */
        if (o->from_db && !o->use_gpu) die("ERROR: -Q cannot be combined with -c\n");
        if (o->all && !o->use_gpu) die("ERROR: -a cannot be combined with -c\n");
        if (o->from_db && o->qfile) die("ERROR: -Q cannot be combined with -q\n");
        if (o->all && o->qfile) die("ERROR: -a cannot be combined with -q\n");
        if (o->all && o->from_db) die("ERROR: -a cannot be combined with -Q\n");
        if (!sat_multi_queries_from_db) die("ERROR: this library has no sat_multi_queries_from_db\n");
        o->qfile = o->from_db = o->all ? o->all : o->from_db;
    }
    if (o->polish_all) {
        /* all rows: the mode of the library; from here on the run is an ordinary one on polished rows */
        if (!o->polish) die("ERROR: -A needs -P T\n");
        if (!o->use_gpu) die("ERROR: -A cannot be combined with -c\n");
        if (o->nmatch) die("ERROR: -A cannot be combined with -m\n");
        if (o->rowmatch) die("ERROR: -A cannot be combined with -M\n");
        if (o->refine) die("ERROR: -A cannot be combined with -R\n");
        if (o->ncand) die("ERROR: -A cannot be combined with -C\n");
        if (!sat_multi_polish_all_set) die("ERROR: this library has no sat_multi_polish_all_set\n");
        o->polish_all = o->polish;
        o->polish = 0;
    }
    if (o->polish && !o->use_gpu) die("ERROR: -P needs the GPU path\n");
    if (o->polish && o->nmatch) die("ERROR: -P cannot be combined with -m\n");
    if (o->polish && o->rowmatch) die("ERROR: -P cannot be combined with -M\n");
    if (o->polish && o->cutoff) die("ERROR: -P cannot be combined with -p\n");
    if (o->polish && o->fit) die("ERROR: -P cannot be combined with -F\n");
    if (o->polish && o->topk <= 0) die("ERROR: -P needs -k K\n");
    if (o->polish && !sat_multi_search_refine_polish) die("ERROR: this library has no sat_multi_search_refine_polish\n");
    if (o->cutoff && !o->use_gpu) die("ERROR: -p needs the GPU path\n");
    if (o->cutoff && o->nmatch) die("ERROR: -p cannot be combined with -m\n");
    if (o->cutoff && o->refine) die("ERROR: -p cannot be combined with -R\n");
    if (o->cutoff && (!sat_multi_search_cutoff || !sat_multi_hits_cutoff))
        die("ERROR: this library has no sat_multi_search_cutoff\n");
    if (o->refine && !o->use_gpu) die("ERROR: -R needs the GPU path\n");
    if (o->refine && o->nmatch) die("ERROR: -R cannot be combined with -m\n");
    if (o->refine && o->topk <= 0) die("ERROR: -R needs -k K\n");
    if (o->ncand && !o->refine && !o->polish) die("ERROR: -C needs -R\n");
    if ((o->refine || o->polish) && !o->ncand) o->ncand = o->topk;
    if ((o->refine || o->polish) && o->topk > o->ncand) die("ERROR: -k K (%d) exceeds -C C (%d)\n", o->topk, o->ncand);
    if (o->refine && !sat_multi_search_refine) die("ERROR: this library has no sat_multi_search_refine\n");
    if (o->nmatch && !o->use_gpu) die("ERROR: -m needs the GPU path\n");
    if (o->nmatch && !sat_multi_search_matches) die("ERROR: this library has no sat_multi_search_matches\n");
    o->ranked = o->topk > 0 || o->cutoff;                /* (-R needs -k) */
    if (o->rowmatch && !o->use_gpu) die("ERROR: -M needs the GPU path\n");
    if (o->rowmatch && o->nmatch) die("ERROR: -M cannot be combined with -m\n");
    if (o->rowmatch && !o->ranked) die("ERROR: -M needs -k K, -p P or -R restarts -k K\n");
    if (o->rowmatch && !sat_multi_search_pairs_matches)
        die("ERROR: this library has no sat_multi_search_pairs_matches\n");
    if (o->fit && o->refine) die("ERROR: -F cannot be combined with -R\n");
    if (o->fit && o->nmatch) die("ERROR: -F cannot be combined with -m\n");
    if (o->fit && o->ranked && (!sat_multi_search_fit || !sat_multi_hits_cutoff))
        die("ERROR: this library has no sat_multi_search_fit\n");
    o->csr = o->cutoff || (o->fit && o->topk > 0);
    o->nm = o->nmatch > 0 ? o->nmatch : 1;
}

/* -q, -Q: query SIDs on stdin, one a line (cut to 7 characters), options T T F; -a: the same options and nothing read -
 * the queries are the database's entries, counted when it is loaded; else the database name, the options and the query
 * structures on stdin */
static void read_queries(const options *o, input *in)
{
    if (o->qfile) {
        strncpy(in->dbfile, o->qfile, sizeof in->dbfile - 1);
        in->ltype = in->lorder = 1;
        char buf[SAT_MAX_LINE_LEN];
        while (!o->all && !feof(stdin) && fgets(buf, SAT_MAX_LINE_LEN, stdin)) {
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
    if (o->bincache) {
        struct stat sa, sb;
        if (stat(in->dbfile, &sa) == 0 && stat(binpath, &sb) == 0 && sb.st_mtime >= sa.st_mtime &&
            sat_set_load_binary(binpath, &in->db) == 0) {
            total = in->db.count;
            fprintf(stderr, "(binary image %s)\n", binpath);
        }
    }
    if (total < 0) {
        total = sat_read_structures_file(in->dbfile, &in->db, "database");     /* mmap reader, same semantics */
        if (total >= 0 && o->bincache && sat_set_save_binary(&in->db, binpath) != 0)
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

    in->qsrc = o->qfile ? &in->db : &in->queries;
    if (o->all)
        in->num_queries = in->db.count;
    in->qindex = checked(malloc(sizeof(int) * (size_t)(in->num_queries + 1)));
    for (int i = 0; i < in->num_queries; i++) {
        in->qindex[i] = i;
        if (!o->qfile || o->all)
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
    slots one = { 1, NULL, checked(malloc(sizeof(int32_t) * total)),
                  in->lsoln ? checked(malloc(sizeof(int32_t) * SAT_MAXDIM * total)) : NULL };
    int32_t *fit_orders = o->fit ? checked(malloc(sizeof(int32_t) * (total + 1))) : NULL;
    sat_host_stream stream;
    sat_host_stream_seed(&stream, 1234);
    const int passes = in->cls_count[1] > 0 ? 2 : 1;
    for (int k = 0; k < passes; k++)
        for (int qi = 0; qi < in->num_queries; qi++) {
            int qs;
            const sat_struct_set *qset = query_set(in, qi, &qs);
            if (!o->fit)
                print_header(in, qi, NULL);
            fprintf(stderr, "Executing simulated annealing tableaux match kernel on host for query %s...\n",
                    sat_set_name(qset, qs));
            double t1 = now_ms();
            if (sat_host_search(&in->db, in->cls_index[k], in->cls_count[k], qset, qs, in->lorder, in->lsoln,
                                o->maxstart, &stream, one.scores, one.maps) != 0)
                die("malloc failed in host search\n");
            double ms = now_ms() - t1;
            fprintf(stderr, "host execution time %f ms\n", ms);
            fprintf(stderr, "%f million iterations/sec\n",
                    ((double)in->cls_count[k] * ((double)o->maxstart * SAT_MAXITER) / (ms / 1000)) / 1.0e6);
            if (o->fit) {
                /* the block's own rows: the one stream runs class after class, so a block is fitted when it is printed */
                for (int d = 0; d < in->cls_count[k]; d++)
                    fit_orders[d] = in->db.order[in->cls_index[k][d]];
                sat_fit f = fit_scores(one.scores, in->cls_count[k], qset->order[qs], fit_orders, o->censor);
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
    const int total = in->db.count, nm = o->nm, lsoln = in->lsoln;
    const int entry_slots = (!o->ranked && !o->cluster && !o->classfile && !o->profile) || o->nmatch;     /* every entry's slots come to the host */
    *B = (gpu_bufs){ .batch = 256, .kk = o->topk < total ? o->topk : total, .reorder = o->reorder };
    /* Queries go to the GPUs in batches: one set of launches scores a whole batch (grid = entries x queries), which
     * is what fills the machine when the database is small and the query list long (-q).  The batch size is bounded
     * by the host slots of every entry: score and map, with -m also count and restarts (the device holds the same
     * slots, maps as bytes). */
    if (entry_slots) {
        const size_t per_entry = (size_t)nm * (lsoln ? SAT_MAXDIM + 1 : 1) + (o->nmatch ? 1 + (size_t)nm : 0);
        const size_t per_query = (size_t)total * per_entry * sizeof(int32_t);
        const size_t budget = (size_t)1 << 30;
        if ((size_t)B->batch * per_query > budget) B->batch = (int)(budget / per_query);
    }
    if (o->profile) {
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
    if (o->profile)
        B->qnode = checked(malloc(sizeof(int32_t) * (size_t)B->batch));
    const size_t rows = (size_t)total * B->batch;
    if (entry_slots)
        alloc_slots(&B->all, rows, nm, o->nmatch, lsoln);
    if (o->nmatch)
        B->restarts = checked(malloc(sizeof(int32_t) * rows * nm));
    if (!o->ranked && !o->cluster && !o->classfile && !o->profile && in->cls_count[1] > 0)
        alloc_slots(&B->large, (size_t)in->cls_count[1] * in->num_queries, nm, o->nmatch, lsoln);
    if (o->csr) {
        B->hits_cap = o->cutoff ? 1024 : B->kk * B->batch;
        B->pcounts = checked(malloc(sizeof(int32_t) * (size_t)B->batch));
        alloc_hits(B, (size_t)B->hits_cap, lsoln);
    } else if (o->topk > 0) {
        alloc_hits(B, (size_t)B->kk * B->batch, lsoln);  /* only K rows per query (and GPU) ever leave the GPUs */
    }
    B->n1s = checked(malloc(sizeof(int32_t) * (size_t)B->batch));
    if (o->reorder && o->fit)
        B->base_fits = checked(calloc((size_t)B->batch, sizeof(sat_fit)));
    if (o->from_db && in->motifs)
        B->sse_begin = checked(malloc(sizeof(int32_t) * ((size_t)B->batch + 1)));
    if (o->from_db)
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
}

/* One multi-GPU context holding the database: it is cut into contiguous shards of equal COST (entries of a
 * size-sorted database differ several-fold in cost, sat_shard.h), every GPU holds its shard, a search is queued on
 * all of them and one gather (RCCL over xGMI) brings the rows to device 0. */
static sat_multi *open_multi(const options *o, const input *in)
{
    const int total = in->db.count, ndev = sat_device_count();
    if (ndev <= 0)
        die("There is no usable HIP device (use -c for the host mode).\n");
    fprintf(stderr, "found %d HIP devices\n", ndev);
    int ngpu = o->want_gpus > 0 ? o->want_gpus : ndev;
    if (ngpu > ndev) ngpu = ndev;
    if (o->ndev_list > 0) ngpu = o->ndev_list;
    if (ngpu > total) ngpu = total;
    const double t0 = now_ms();
    sat_multi *multi = sat_multi_create(ngpu, o->ndev_list > 0 ? o->dev_list : NULL, o->seed);
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

/* The mode's search of the batch set last.  Returns rows per query (-k, -R), the batch's rows (-p), 0 (listing, -m)
 * or a negative SAT_E* code. */
static int search_batch(const options *o, const input *in, sat_multi *multi, gpu_bufs *B, sat_fit *fits, double *ms,
                        double *ms_stage2)
{
    const int lorder = in->lorder, lsoln = in->lsoln, maxstart = o->maxstart;
    if (o->cluster || o->classfile || o->profile) {
        /* -L, -H, -D, -E: the rows stay on the GPUs (no gather, no LSOLN: no map is printed); with -F the fit is installed
         * there.  -W: the same with LSOLN on, whatever the input says - the maps are what it counts, where they are */
        if (o->fit)
            return sat_multi_search_fit(multi, lorder, o->profile, maxstart, o->censor, fits, ms);
        return sat_multi_search_only(multi, lorder, o->profile, maxstart, ms);
    }
    if (o->reorder) {
        /* -X: the ordered search without maps, fitted (-F) and kept on the GPUs as the baseline; the unordered search with
         * maps, fitted to its own scores; then of -p's rows those the baseline does not call a hit and whose map is of one
         * of the kinds.  A short buffer is grown and the rows selected again. */
        double ms2 = 0.0;
        int rc = o->fit ? sat_multi_search_fit(multi, 1, 0, maxstart, o->censor, B->base_fits, ms)
                        : sat_multi_search_only(multi, 1, 0, maxstart, ms);
        if (rc == SAT_OK)
            rc = sat_multi_baseline_keep(multi);
        if (rc == SAT_OK)
            rc = o->fit ? sat_multi_search_fit(multi, 0, 1, maxstart, o->censor, fits, &ms2)
                        : sat_multi_search_only(multi, 0, 1, maxstart, &ms2);
        *ms += ms2;
        if (rc != SAT_OK)
            return rc;
        rc = sat_multi_reorder_hits(multi, o->pmax, o->bmin, o->kinds, o->topk, B->pcounts, B->hits_cap, B->rhits, B->hit_maps);
        if (rc > B->hits_cap) {
            B->hits_cap = rc;
            alloc_hits(B, (size_t)rc, 1);
            rc = sat_multi_reorder_hits(multi, o->pmax, o->bmin, o->kinds, o->topk, B->pcounts, B->hits_cap, B->rhits, B->hit_maps);
        }
        for (int r = 0; r < rc; r++)
            B->hits[r] = B->rhits[r].hit;
        return rc;
    }
    if (o->fit && o->ranked) {
        /* search, histogram and fit on the GPUs (fits: the batch's), then the rows by the fitted p-values: those under
         * -p's cutoff, or with -k alone (every p-value is <= 1) the K best */
        int rc = sat_multi_search_fit(multi, lorder, lsoln, maxstart, o->censor, fits, ms);
        if (rc != SAT_OK)
            return rc;
        const double pmax = o->cutoff ? o->pmax : 1.0;
        rc = sat_multi_hits_cutoff(multi, pmax, o->topk, B->pcounts, B->hits_cap, B->hits, B->hit_maps);
        if (rc > B->hits_cap) {
            B->hits_cap = rc;
            alloc_hits(B, (size_t)rc, lsoln);
            rc = sat_multi_hits_cutoff(multi, pmax, o->topk, B->pcounts, B->hits_cap, B->hits, B->hit_maps);
        }
        return rc;
    }
    if (o->cutoff) {
        /* every row of the batch under the cutoff; a short buffer is grown and the rows selected again */
        int rc = sat_multi_search_cutoff(multi, lorder, lsoln, maxstart, o->pmax, o->topk, B->pcounts, B->hits_cap,
                                         B->hits, B->hit_maps, ms);
        if (rc > B->hits_cap) {
            B->hits_cap = rc;
            alloc_hits(B, (size_t)rc, lsoln);
            rc = sat_multi_hits_cutoff(multi, o->pmax, o->topk, B->pcounts, B->hits_cap, B->hits, B->hit_maps);
        }
        return rc;
    }
    if (o->polish)
        return sat_multi_search_refine_polish(multi, lorder, lsoln, maxstart, o->ncand, o->refine ? o->refine : maxstart, o->polish,
                                              B->kk, B->hits, B->hit_maps, NULL, NULL, ms);
    if (o->refine)
        return sat_multi_search_refine(multi, lorder, lsoln, maxstart, o->ncand, o->refine, B->kk, B->hits,
                                       B->hit_maps, NULL, ms, ms_stage2);
    if (o->nmatch) {
        /* match 0 of every entry is the plain search's score and map: the listing's rows come from the match slots;
         * -k ranks the entries as without -m (its own search), the extra rows from the slots */
        int rc = sat_multi_search_matches(multi, lorder, maxstart, o->nm, B->all.counts, B->all.scores, B->restarts,
                                          B->all.maps, ms);
        if (rc == SAT_OK && o->topk > 0) {
            double ms2 = 0.0;
            rc = sat_multi_search_topk(multi, lorder, lsoln, maxstart, B->kk, B->hits, B->hit_maps, &ms2);
            *ms += ms2;
        }
        return rc;
    }
    if (o->topk > 0)
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
    alloc_rowm(B, rows ? rows : 1, o->rowmatch, in->lsoln);
    size_t r = 0;
    for (int b = 0; b < nqb; b++)
        for (size_t n = (size_t)(o->csr ? B->pcounts[b] : rc); n > 0; n--, r++) {
            B->pair_q[r] = b;
            B->pair_e[r] = B->hits[r].entry;
        }
    return sat_multi_search_pairs_matches(multi, in->lorder, o->refine ? o->refine : o->maxstart, o->rowmatch, (int)rows,
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
        if (o->reorder) {
            /* -X: one more header line (two with -F: the ordered search's fit), then the rows with their six columns,
             * each followed by the unordered map's lines.  Few rows: printf formats them. */
            char line[256], kt[4];
            const int n1 = B->n1s[b];
            int n = snprintf(line, sizeof line, "# REORDER ordered pvalue >= %g kinds = %s\n", o->bmin, kinds_text(o->kinds, kt));
            out_bytes(line, (size_t)n);
            if (B->base_fits) {
                const sat_fit *f = &B->base_fits[b];
                n = f->fitted ? snprintf(line, sizeof line, "# GUMBEL ordered a = %.17g b = %.17g rows = %d censored = %d below = %d\n",
                                         f->a, f->b, f->rows, f->censored, f->below)
                              : snprintf(line, sizeof line, "# GUMBEL ordered not fitted\n");
                out_bytes(line, (size_t)n);
            }
            for (size_t r = first; r < first + (size_t)B->pcounts[b]; r++) {
                const sat_reorder_hit *h = &B->rhits[r];
                const char *kind = h->kind == SAT_KIND_SEQUENTIAL ? "seq" : h->kind == SAT_KIND_CIRCULAR ? "circ" : "perm";
                n = snprintf(line, sizeof line, "%-8s %d %g %g %g %d %g %s %d %d %d\n", sat_set_name(&in->db, h->hit.entry), h->hit.score,
                             h->hit.norm2, h->hit.zscore, h->hit.pvalue, h->base_score, h->base_pvalue, kind, h->matched, h->descents,
                             h->cut);
                out_bytes(line, (size_t)n);
                const int32_t *map = B->hit_maps + r * SAT_MAXDIM;
                for (int k = 0; k < n1; k++)
                    if (map[k] >= 0)
                        out_map_line(k + 1, map[k] + 1);
            }
            first += (size_t)B->pcounts[b];
            continue;
        }
        if (o->ranked) {
            const size_t nrows = (size_t)(o->csr ? B->pcounts[b] : rc);
            for (size_t r = first; r < first + nrows; r++)
                print_entry(in, B->hits[r].entry, B->n1s[b], &B->hits[r],
                            B->hit_maps ? B->hit_maps + r * SAT_MAXDIM : NULL, o->rowmatch ? &B->rowm : all,
                            o->rowmatch ? r : row0 + B->hits[r].entry, 0);
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

/* -L: the table of the clustering the GPUs hold - labels, degrees and the edge count cross to the host (8 bytes a
 * structure and shard), the representatives and sizes are sat_cluster_reps' */
static int print_clusters(const options *o, const input *in, sat_multi *multi, const sat_fit *fits)
{
    const int n = in->db.count;
    int32_t *label = checked(malloc(sizeof(int32_t) * (size_t)n * 4)), *degree = label + n, *rep = degree + n, *size = rep + n;
    unsigned long long edges = 0;
    if (sat_multi_cluster_labels(multi, label, degree, &edges) != SAT_OK) {
        fprintf(stderr, "clustering failed: %s\n", sat_last_error());
        free(label);
        return 1;
    }
    const int clusters = sat_cluster_reps(n, label, degree, rep, size);
    if (clusters < 0)
        die("ERROR: the GPUs returned labels that are no clustering\n");
    int singletons = 0, fitted = 0;
    for (int v = 0; v < n; v++)
        singletons += size[v] == 1;
    char line[SAT_MAX_LINE_LEN + 256];
    int len = snprintf(line, sizeof line, "# CLUSTER dbfile = %s entries = %d pvalue <= %g restarts = %d clusters = %d singletons = %d "
                       "edges = %llu\n", in->dbfile, n, o->lmax, o->maxstart, clusters, singletons, edges);
    out_bytes(line, (size_t)len);
    out_bytes(polish_header, strlen(polish_header));
    if (fits) {
        for (int v = 0; v < n; v++)
            fitted += fits[v].fitted != 0;
        len = snprintf(line, sizeof line, "# GUMBEL censor = %g fitted = %d of %d\n", o->censor, fitted, n);
        out_bytes(line, (size_t)len);
    }
    for (int v = 0; v < n; v++) {
        len = snprintf(line, sizeof line, "%-8s %-8s %d %d\n", sat_set_name(&in->db, v), sat_set_name(&in->db, rep[v]), size[v],
                       degree[v]);
        out_bytes(line, (size_t)len);
    }
    free(label);
    return 0;
}

/* -D: the table of the cover the GPUs solved - representatives and degrees (8 bytes a structure), the edge and round
 * counts; the sizes are sat_cover_sizes'.  The library has checked the cover's two invariants before it returned */
static int print_cover(const options *o, const input *in, sat_multi *multi, const sat_fit *fits)
{
    const int n = in->db.count;
    int32_t *rep = checked(malloc(sizeof(int32_t) * (size_t)n * 3)), *degree = rep + n, *size = degree + n;
    unsigned long long edges = 0;
    int rounds = 0;
    if (sat_multi_cover_solve(multi, rep, degree, &edges, &rounds) != SAT_OK) {
        fprintf(stderr, "clustering failed: %s\n", sat_last_error());
        free(rep);
        return 1;
    }
    const int clusters = sat_cover_sizes(n, rep, size);
    if (clusters < 0)
        die("ERROR: the GPUs returned representatives that are no cover\n");
    int singletons = 0, fitted = 0;
    for (int v = 0; v < n; v++)
        singletons += size[v] == 1;
    char line[SAT_MAX_LINE_LEN + 256];
    int len = snprintf(line, sizeof line, "# COVER dbfile = %s entries = %d pvalue <= %g restarts = %d clusters = %d singletons = %d "
                       "edges = %llu rounds = %d\n", in->dbfile, n, o->dmax, o->maxstart, clusters, singletons, edges, rounds);
    out_bytes(line, (size_t)len);
    out_bytes(polish_header, strlen(polish_header));
    if (fits) {
        for (int v = 0; v < n; v++)
            fitted += fits[v].fitted != 0;
        len = snprintf(line, sizeof line, "# GUMBEL censor = %g fitted = %d of %d\n", o->censor, fitted, n);
        out_bytes(line, (size_t)len);
    }
    for (int v = 0; v < n; v++) {
        len = snprintf(line, sizeof line, "%-8s %-8s %d %d\n", sat_set_name(&in->db, v), sat_set_name(&in->db, rep[v]), size[v],
                       degree[v]);
        out_bytes(line, (size_t)len);
    }
    free(rep);
    return 0;
}

/* -H: the tables of the L clusterings the GPUs hold, side by side - per level what print_clusters prints for it: 8 bytes
 * a structure, level and shard cross to the host; the levels must be nested (sat_cluster_nested) */
static int print_cluster_levels(const options *o, const input *in, sat_multi *multi, const sat_fit *fits)
{
    const int n = in->db.count, nl = o->nlevels;
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
    char line[SAT_MAX_LINE_LEN + 256];
    int len = snprintf(line, sizeof line, "# CLUSTER dbfile = %s entries = %d levels = %d restarts = %d\n", in->dbfile, n, nl, o->maxstart);
    out_bytes(line, (size_t)len);
    for (int j = 0; j < nl; j++) {
        const size_t at = (size_t)j * (size_t)n;
        const int clusters = sat_cluster_reps(n, label + at, degree + at, rep + at, size + at);
        if (clusters < 0)
            die("ERROR: the GPUs returned labels that are no clustering\n");
        int singletons = 0;
        for (int v = 0; v < n; v++)
            singletons += size[at + v] == 1;
        len = snprintf(line, sizeof line, "# LEVEL %d pvalue <= %g clusters = %d singletons = %d edges = %llu\n", j + 1, o->levels[j], clusters,
                       singletons, edges[j]);
        out_bytes(line, (size_t)len);
    }
    out_bytes(polish_header, strlen(polish_header));
    if (fits) {
        int fitted = 0;
        for (int v = 0; v < n; v++)
            fitted += fits[v].fitted != 0;
        len = snprintf(line, sizeof line, "# GUMBEL censor = %g fitted = %d of %d\n", o->censor, fitted, n);
        out_bytes(line, (size_t)len);
    }
    for (int v = 0; v < n; v++) {
        len = snprintf(line, sizeof line, "%-8s", sat_set_name(&in->db, v));
        out_bytes(line, (size_t)len);
        for (int j = 0; j < nl; j++) {
            const size_t at = (size_t)j * (size_t)n + (size_t)v;
            len = snprintf(line, sizeof line, " %-8s %d %d", sat_set_name(&in->db, rep[at]), size[at], degree[at]);
            out_bytes(line, (size_t)len);
        }
        out_bytes("\n", 1);
    }
    free(label);
    return 0;
}

/* -E: the table of the evaluation - the queries' rows as the GPUs reduced them (32 bytes a query crossed to the host);
 * the two ratios are taken here, and their means over the queries where both are defined */
static void print_eval(const options *o, const input *in, const sat_classes *cl, const sat_eval *ev)
{
    /* (the class file's name and the class tokens are of any length: they go out as they are, not through `line`) */
    char line[SAT_MAX_LINE_LEN + 256];
    int len = snprintf(line, sizeof line, "# EVAL dbfile = %s classes = ", in->dbfile);
    out_bytes(line, (size_t)len);
    out_bytes(o->classfile, strlen(o->classfile));
    len = snprintf(line, sizeof line, " entries = %d classified = %d distinct = %d restarts = %d rocn = %d\n", in->db.count, cl->classified,
                   cl->distinct, o->maxstart, o->rocn);
    out_bytes(line, (size_t)len);
    out_bytes(polish_header, strlen(polish_header));
    int defined = 0;
    double auc_sum = 0.0, rocn_sum = 0.0;
    for (int qi = 0; qi < in->num_queries; qi++)
        if (ev[qi].positives > 0 && ev[qi].negatives > 0) {
            auc_sum += (double)ev[qi].u2 / (2.0 * (double)ev[qi].positives * (double)ev[qi].negatives);
            rocn_sum += (double)ev[qi].t2 / (2.0 * (double)ev[qi].positives * (double)ev[qi].n_used);
            defined++;
        }
    if (defined)
        len = snprintf(line, sizeof line, "# MEAN queries = %d auc = %.6f rocn = %.6f\n", defined, auc_sum / defined, rocn_sum / defined);
    else
        len = snprintf(line, sizeof line, "# MEAN queries = 0 auc = NA rocn = NA\n");
    out_bytes(line, (size_t)len);
    for (int qi = 0; qi < in->num_queries; qi++) {
        const sat_eval *e = &ev[qi];
        const char *token = e->query_class >= 0 && e->query_class < cl->distinct ? cl->token[e->query_class] : "-";
        len = snprintf(line, sizeof line, "%-8s ", sat_set_name(&in->db, in->qindex[qi]));
        out_bytes(line, (size_t)len);
        out_bytes(token, strlen(token));
        len = snprintf(line, sizeof line, " %d %d %llu %llu %d", e->positives, e->negatives, (unsigned long long)e->u2,
                       (unsigned long long)e->t2, e->n_used);
        out_bytes(line, (size_t)len);
        if (e->positives > 0 && e->negatives > 0)
            len = snprintf(line, sizeof line, " %.6f %.6f\n", (double)e->u2 / (2.0 * (double)e->positives * (double)e->negatives),
                           (double)e->t2 / (2.0 * (double)e->positives * (double)e->n_used));
        else
            len = snprintf(line, sizeof line, " NA NA\n");
        out_bytes(line, (size_t)len);
    }
}

/* -W: the table of the profiles - every query's hits and matrix as the GPUs counted them (4 + 4 n1 n1 bytes a query
 * crossed to the host); the core is sat_profile_core's.  A motif's core is written in its source entry's numbering */
static void print_profiles(const options *o, const input *in, const gpu_bufs *B, const sat_fit *fits)
{
    static const char *tname[4] = { "e", "xa", "xi", "xg" };
    char line[SAT_MAX_LINE_LEN + 256];
    int len = snprintf(line, sizeof line, "# PROFILE dbfile = %s pvalue <= %g fraction >= %g restarts = %d queries = %d\n", in->dbfile,
                       o->wmax, o->core, o->maxstart, in->num_queries);
    out_bytes(line, (size_t)len);
    out_bytes(polish_header, strlen(polish_header));
    if (fits) {
        int fitted = 0;
        for (int qi = 0; qi < in->num_queries; qi++)
            fitted += fits[qi].fitted != 0;
        len = snprintf(line, sizeof line, "# GUMBEL censor = %g fitted = %d of %d\n", o->censor, fitted, in->num_queries);
        out_bytes(line, (size_t)len);
    }
    uint8_t in_core[SAT_MAXDIM];
    for (int qi = 0; qi < in->num_queries; qi++) {
        int qs;
        const sat_struct_set *qset = query_set(in, qi, &qs);
        const int n1 = qset->order[qs], motif = in->motifs && in->qsub[qi] >= 0;
        const char *name = sat_set_name(in->qsrc, in->qindex[qi]);
        const uint32_t *joint = B->pjoint + B->poff[qi];
        len = snprintf(line, sizeof line, "# QUERY %s sses = %d hits = %u\n", name, n1, B->phits[qi]);
        out_bytes(line, (size_t)len);
        if (motif) {
            out_bytes("# QUERY SSES = ", 15);
            for (int32_t k = in->sse_begin[qi]; k < in->sse_begin[qi + 1]; k++) {
                len = snprintf(line, sizeof line, k > in->sse_begin[qi] ? ",%d" : "%d", in->sse[k] + 1);
                out_bytes(line, (size_t)len);
            }
            out_bytes("\n", 1);
        }
        uint32_t joint_min = 0;
        const int core = sat_profile_core(n1, B->phits[qi], joint, o->core, in_core, &joint_min);
        if (core < 0)
            die("ERROR: no core for query %s\n", name);
        if (core == 0) {
            out_bytes("# CORE none\n", 12);
        } else {
            len = snprintf(line, sizeof line, "# CORE sses = %d joint >= %u %s@", core, joint_min, name);
            out_bytes(line, (size_t)len);
            for (int i = 0, first = 1; i < n1; i++)
                if (in_core[i]) {
                    len = snprintf(line, sizeof line, first ? "%d" : ",%d", motif ? in->sse[in->sse_begin[qi] + i] + 1 : i + 1);
                    out_bytes(line, (size_t)len);
                    first = 0;
                }
            out_bytes("\n", 1);
        }
        const uint8_t *tab = qset->tab + qset->cell_off[qs];
        for (int i = 0; i < n1; i++) {
            len = snprintf(line, sizeof line, "%d %s %u", i + 1, tname[tab[(size_t)i * (i + 1) / 2 + i] & 3], joint[(size_t)i * n1 + i]);
            out_bytes(line, (size_t)len);
            for (int k = 0; k < n1; k++) {
                len = snprintf(line, sizeof line, " %u", joint[(size_t)i * n1 + k]);
                out_bytes(line, (size_t)len);
            }
            out_bytes("\n", 1);
        }
    }
}

static int run_gpu(const options *o, const input *in)
{
    /* -E: the classification, read before any GPU is touched: a bad file ends the run here */
    sat_classes classes;
    memset(&classes, 0, sizeof classes);
    if (o->classfile) {
        char err[SAT_MAX_LINE_LEN + 256];
        if (sat_read_classes(o->classfile, &in->db, &classes, err, sizeof err) != 0)
            die("ERROR: %s\n", err);
        if (classes.unknown)
            fprintf(stderr, "WARNING: %d names of %s are not in the database\n", classes.unknown, o->classfile);
        fprintf(stderr, "Read %d classes of %d of %d structures from %s\n", classes.distinct, classes.classified, in->db.count, o->classfile);
    }
    if (o->from_db && in->motifs && !sat_multi_queries_from_db_sses)
        die("ERROR: this library has no sat_multi_queries_from_db_sses\n");
    sat_eval *evals = o->classfile ? checked(calloc((size_t)in->num_queries + 1, sizeof(sat_eval))) : NULL;
    sat_multi *multi = open_multi(o, in);
    gpu_bufs B;
    alloc_gpu_bufs(o, in, &B);
    const int total = in->db.count;
    int status = 0;
    if (o->polish)
        snprintf(polish_header, sizeof polish_header, "# POLISH tops = %d restarts = %d candidates = %d\n", o->polish,
                 o->refine ? o->refine : o->maxstart, o->ncand);
    if (o->polish_all) {
        snprintf(polish_header, sizeof polish_header, "# POLISH tops = %d all rows\n", o->polish_all);
        if (sat_multi_polish_all_set(multi, o->polish_all) != SAT_OK)
            die("ERROR: %s\n", sat_last_error());
    }
    /* -F: every query's fit - from the GPUs with -k / -p, else made here from the listing's scores (the whole
     * database's, both size classes: a query's two blocks carry the same line) */
    sat_fit *fits = o->fit ? checked(calloc((size_t)in->num_queries, sizeof(sat_fit))) : NULL;
    if (o->cluster && (o->cover ? sat_multi_cover_begin(multi) : o->nlevels ? sat_multi_cluster_begin_levels(multi, o->nlevels, o->levels)
                                                               : sat_multi_cluster_begin(multi)) != SAT_OK)
        die("ERROR: %s\n", sat_last_error());
    if (o->classfile && sat_multi_eval_classes(multi, classes.node_class) != SAT_OK)
        die("ERROR: %s\n", sat_last_error());
    for (int q0 = 0; q0 < in->num_queries; q0 += B.batch) {
        const int nqb = in->num_queries - q0 < B.batch ? in->num_queries - q0 : B.batch;
        for (int b = 0; b < nqb; b++) {
            int qs;
            const sat_struct_set *qset = query_set(in, q0 + b, &qs);
            B.n1s[b] = qset->order[qs];
            if (o->from_db)
                continue;
            uint8_t *tab = B.qtabs + (size_t)b * SAT_MAXDIM * SAT_MAXDIM;
            sat_set_expand(qset, qs, SAT_MAXDIM, tab, B.qdmats + (size_t)b * SAT_MAXDIM * SAT_MAXDIM);
            for (int i = 0; i < B.n1s[b]; i++)
                B.qtypes[(size_t)b * SAT_MAXDIM + i] = tab[i * SAT_MAXDIM + i];
        }
        fprintf(stderr, "Executing simulated annealing tableaux match kernel on GPU for %d quer%s (from %s)...\n",
                nqb, nqb == 1 ? "y" : "ies", sat_set_name(in->qsrc, in->qindex[q0]));
        double ms = 0.0, ms_stage2 = 0.0;
        /* -Q, -a: the batch from its entries' indices in the database the GPUs hold; where the run has a motif, with
         * the batch's lists, their offsets counted from the batch's first */
        if (o->from_db && in->motifs)
            for (int b = 0; b <= nqb; b++)
                B.sse_begin[b] = in->sse_begin[q0 + b] - in->sse_begin[q0];
        int rc = o->from_db && in->motifs ? sat_multi_queries_from_db_sses(multi, nqb, in->qindex + q0, B.sse_begin,
                                                                           in->sse + in->sse_begin[q0], (uint32_t)q0)
                 : o->from_db ? sat_multi_queries_from_db(multi, nqb, in->qindex + q0, (uint32_t)q0)
                            : sat_multi_queries_set(multi, nqb, B.n1s, B.qtabs, B.qdmats, SAT_MAXDIM, B.qtypes, (uint32_t)q0);
        if (rc == SAT_OK)
            rc = search_batch(o, in, multi, &B, fits ? fits + q0 : NULL, &ms, &ms_stage2);
        /* -L, -H, -D: the batch's edges into the graph(s) on the GPUs; query b is structure qindex[q0 + b] of the database */
        if (rc == SAT_OK && o->cluster)
            rc = o->cover ? sat_multi_cover_add(multi, o->dmax, in->qindex + q0)
                 : o->nlevels ? sat_multi_cluster_add_levels(multi, in->qindex + q0) : sat_multi_cluster_add(multi, o->lmax, in->qindex + q0);
        /* -E: the batch's rows scored where they are; query b is structure qindex[q0 + b] of the database */
        if (rc == SAT_OK && o->classfile)
            rc = sat_multi_eval_rows(multi, in->qindex + q0, o->rocn, evals + q0);
        /* -W: the batch's rows and maps counted where they are; query b is structure qindex[q0 + b] of the database when
         * it was taken from there (a motif: its source entry), else no structure of it */
        if (rc == SAT_OK && o->profile) {
            for (int b = 0; b < nqb; b++)
                B.qnode[b] = o->qfile ? in->qindex[q0 + b] : -1;
            rc = sat_multi_profile_rows(multi, o->wmax, B.qnode, B.phits + q0, B.pjoint + B.poff[q0], NULL);
        }
        if (rc < 0) {
            fprintf(stderr, "kernel launch failed: %s\n", sat_last_error());
            status = 1;
            break;
        }
        if (o->rowmatch) {
            double ms_rows = 0.0;
            if (match_ranked_rows(o, in, multi, &B, nqb, rc, &ms_rows) != SAT_OK) {
                fprintf(stderr, "kernel launch failed: %s\n", sat_last_error());
                status = 1;
                break;
            }
            fprintf(stderr, "matches of the printed rows: %f ms\n", ms_rows);
        }
        fprintf(stderr, "GPU execution time %f ms\n", ms);
        if (o->polish)
            fprintf(stderr, "polish: %d candidates per query x %d restarts, %d maps each\n", o->ncand < total ? o->ncand : total,
                    o->refine ? o->refine : o->maxstart, o->polish);
        else if (o->polish_all)
            fprintf(stderr, "polish: every row, %d maps each\n", o->polish_all);
        else if (o->refine)
            fprintf(stderr, "refine: stage 2 %f ms, %d candidates per query x %d restarts\n", ms_stage2,
                    o->ncand < total ? o->ncand : total, o->refine);
        fprintf(stderr, "%f million iterations/sec\n",
                ((double)total * nqb * ((double)o->maxstart * SAT_MAXITER) / (ms / 1000)) / 1.0e6);
        if (o->cluster || o->classfile || o->profile)
            continue;
        if (o->fit && !o->ranked)
            for (int b = 0; b < nqb; b++)
                fits[q0 + b] = fit_scores(B.all.scores + (size_t)b * total, total, B.n1s[b], in->db.order, o->censor);
        print_batch(o, in, &B, fits, q0, nqb, rc);
    }
    /* the listing's deferred block: every query's large-class rows, after all small-class blocks, with the reference
     * GPU path's two blanks before the p-value */
    if (!status && o->cluster)
        status = o->cover ? print_cover(o, in, multi, fits) : o->nlevels ? print_cluster_levels(o, in, multi, fits) : print_clusters(o, in, multi, fits);
    if (!status && o->classfile)
        print_eval(o, in, &classes, evals);
    if (!status && o->profile)
        print_profiles(o, in, &B, fits);
    if (!status && !o->ranked && !o->cluster && !o->classfile && !o->profile && in->cls_count[1] > 0)
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
    free(evals);
    sat_classes_free(&classes);
    return status;
}

int main(int argc, char *argv[])
{
    options o;
    parse_options(argc, argv, &o);
    fprintf(stderr, "MAXDIM = %d\n", SAT_MAXDIM);
    atexit(out_flush);                                   /* every exit path, exit(1) included */
    input in;
    memset(&in, 0, sizeof in);
    sat_set_init(&in.queries);
    sat_set_init(&in.db);
    read_queries(&o, &in);
    load_database(&o, &in);
    if (o.reorder) {
        /* -X runs both searches itself; its rows are the unordered search's, with their maps */
        in.lorder = 0;
        in.lsoln = 1;
    }
    fprintf(stderr, "maxstart = %d\n", o.maxstart);
    const int status = o.use_gpu ? run_gpu(&o, &in) : run_host(&o, &in);
    free_input(&in);
    free(norm2_cache);
    free(fit_store);
    return status;
}
