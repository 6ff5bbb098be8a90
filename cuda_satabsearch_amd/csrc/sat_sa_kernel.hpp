// sat_sa_kernel.hpp - the simulated-annealing tableau search kernel for gfx950 (CDNA4).
//
// One ENTRY SLOT of a workgroup scores ONE database structure against the query; every lane runs
// an independent restart chain (lane = restart, as the reference maps threadIdx to restarts,
// K.cu:1012-1015), 100 Metropolis steps each.  A workgroup is one slot, or several side by side
// (own threads, own LDS carve, shared barriers only) where that packs more entries into the CU's
// 128 LDS granules of 1280 bytes - the host decides per launch (sat_capi.hip: prepare_sa, pick_epw).  Written from scratch for
// 64-wide wavefronts and the 160 KB LDS; what it computes follows the reference
// kernel body K.cu:924-1233 (K.cu = nvcc_src_current/cudaSaTabsearch_kernel.cu).
//
// Data layout
//   Dc   (LDS) the db entry's cells {f32 distance, code byte}.  Entries of up to 32 SSEs: the full
//        n2 x (n2+1) matrix of 8-byte cells, expanded from the packed lower triangle in HBM (one
//        ds_read_b64 per pair); larger entries: the lower triangle as it is, distances and codes in two
//        arrays, addressed by (max, min) of the pair - half the LDS where the cells limit the
//        workgroups per CU (DbRow).  Column n2 (full matrix) / row n2 (triangle) is a "null"
//        SSE whose distance is the sentinel -1e30: an unmatched query SSE
//        is represented as matched to the null SSE, so |d1 - d2| <= 4 is false and the
//        pair scores 0 without any branch or predicate in the hot loop (the reference
//        tests l >= 0, old_j >= 0, k != sse_i per pair, K.cu:521-531).  The null SSE is never the
//        ROW of an evaluation: a null image contributes 0, the compacted rounds never list it, and the two
//        loops that may meet one (full score, static loops) walk row 0 and drop the sum.  (Launches with 8-byte
//        cells keep the column but no longer read it: their map bytes carry "unmatched" as a flag that switches
//        the pair off in the selector, see map_bytes_scaled below.)
//   Q    query, grouped by 4 consecutive query SSEs k (one "word" of the map) and
//        TRANSPOSED: qdist[kw*N1P + i] = float4 of dmat1[i][4kw..4kw+3],
//        qcode[kw*N1P + i] = the four code bytes tab1[i][4kw..4kw+3] packed in a dword.
//        The hot loop reads column i = the moved SSE (different per lane) of group kw
//        (same for all lanes): 16-byte and 4-byte loads from consecutive addresses.
//        Diagonal and padding distances are the sentinel +1e30, which removes the k == i
//        term (K.cu:524,530).  Read through L1/L2 (32+-SSE queries) or staged in LDS.
//        Behind the grouped arrays the blob holds the same cells once more as a dense
//        qpair[i * N1P + k] = {distance, code byte} (8 bytes): the full score of an initial map
//        walks the matched pairs (i, k) of each chain and fetches one such cell per pair.
//   qmask (LDS, launches with one-word db sets) per query SSE the db SSEs of its type,
//        tmask[qtypes[i]]: one read on the path of every SA step instead of two dependent ones.
//   pos, qbase (LDS, the same launches) the entry's SSEs sorted by (type, index), one byte each, and per query
//        SSE the start of its type's run in it.  Under LORDER a step's candidates are all the free SSEs of the
//        type between the predecessor's image A and the next occupied SSE, so the pick-th of them is the
//        (SSEs of the type at or below A) + pick -th of the run: one table read instead of stripping `pick` bits.
//   smap (LDS) per-chain SSE map, one byte per query SSE (the image's index, or with 8-byte cells its cell's
//        byte offset in a row, l << 3, and 0x04 for "unmatched": map_bytes_scaled), stored word-interleaved
//        smap[w*(T+1) + chain]: word w of every chain is contiguous, so a loop over a
//        uniform word reads it conflict free; the odd row stride T+1 spreads the words of
//        ONE chain over different banks for the compacted loop, where the lanes serving
//        a row read that chain's words in the same instruction.
//   bmap (LSOLN only) best map so far of every chain, same word-interleaved layout but in
//        GLOBAL memory (one slab per entry slot of the launch): it is written on improvements
//        only and read once by the winner, the resident slabs (~4 KB x a few thousand
//        slots) live in L2, and keeping it out of LDS keeps 12 entries per CU.
//
// Work compaction in the SA step (the db-scan regime is sparse: on random pairs ~25 % of
// the query SSEs are matched, the moved SSE has a real old image in 25 % and a real new
// one in 27 % of the steps, both in 10 %, neither in 58 %): instead of every lane scoring
// 2 rows x n1/4 map words for its own chain, the lanes of a wave list the rows that are real
// (ballot + mbcnt prefix -> a per-wave item table in LDS: row, moved SSE, owner chain,
// sign), then the WHOLE wave works through them in rounds: a row is served by lpi =
// ceil(n1w / 4) lanes, each taking up to four map words (word kw, kw + lpi, ...) whose loads
// are issued together, a round holds 64 / lpi rows, and each lane adds its signed sum to the
// row's accumulator (the item slot itself) with an LDS atomic.  The last few rows of a step
// go to a tail shape with one or two words per lane (more lanes per row) rather than a mostly
// empty full round.  Maps are padded to lpi * wpl words (padding = unmatched SSEs, which meet
// the query's sentinel cells), so the rounds carry no validity tests.  A wave-step then costs
// ~S*n1w/64 packed evaluations (S = real rows in the wave, ~37 of 128) instead of 2*n1w per
// lane.  With LORDER = F most rows are real and the static per-lane loops run instead.
//
// Lanes per chain (lpc = 1, 2 or 4): when the cells of a large db entry leave room for
// only a few workgroups per CU, lpc adjacent lanes run ONE chain together - every lane
// does the cheap per-step bookkeeping redundantly (same stream, same decisions), each
// takes every lpc-th map word of the pair loops and the partial sums are added across
// the lanes - so a workgroup has lpc x the waves for the same LDS.
//
// Pair scores, four at a time (quad_terms): gfx950 issues and/or/xor/add/sub/lshr/
// bitop3/f32 add at one wave64 op per ~2.4 clk and everything else (cmp, cndmask, bcnt,
// perm, shifts left, SDWA, mad) at ~4.2 clk (profiles/r01_gfx950_valu_opcode_cost.txt), so
// the four pairs of a map word are evaluated with packed byte arithmetic:
//   * code bytes are (hi << 4) | lo with hi, lo <= 7 (parsetableaux.c:13-33 uses 0..4):
//     bits 3 and 7 are free guard bits;  X = codes(db, 4 bytes) ^ codes(query, 4 bytes);
//     (X + 0x77777777) & 0x88888888 has bit 3 / bit 7 of byte s set iff the low / high
//     nibble of pair s differs;
//   * distance test: t = 4 - |d1 - d2| is >= 0 exactly when |d1 - d2| <= 4 in f32 (the
//     reference's test K.cu:432, 524, 530); the four sign bytes are gathered by v_perm;
//   * the 3-bit index (lo differs, hi differs, too far) of every pair selects one of
//     {2, 1, 1, -2, 0, 0, 0, 0} = tscord (K.cu:306-332) gated by distance, all four with
//     ONE v_perm_b32, and v_dot4_i32_i8 adds the four signed bytes to the running sum.
//
// Free-SSE bookkeeping uses bit masks instead of the reference's int revmap[] and
// 111-int candidate list (K.cu:677-714): occ = occupied db SSEs, mapped = matched
// query SSEs, tmask[t] = db SSEs of type t.
//
// Random numbers: Philox4x32-10 with rocRAND's counter layout (rocrand_init(seed, subsequence,
// offset) + rocrand4), written out in philox_block; one 4x32-bit block per TWO SA steps, addressed
// by (seed, query, db ordinal, restart, step pair): a step takes two words - one split into two
// 16-bit draws (which query SSE moves, which candidate is taken), one whole for the Metropolis
// test - see oracle/sa_oracle.h for the slot layout, which the CPU oracle restates bit for bit.
//
// Metropolis test: the reference evaluates expf((float)delta / temp) > u with glibc
// expf on the host path (K.cu:1166).  temp takes 100 values and delta is a small
// integer, so the host tabulates P[iter][-delta] = expf(-nd / temp_iter) with ITS
// libm and the kernel compares table entries: accept decisions are those of the
// host's expf, bit for bit.
#pragma once

#ifndef SAT_FS_CHUNKS_ONLY
#include <hip/hip_runtime.h>
#include <type_traits>
#endif
#include <stdint.h>

// ---------------------------------------------------------------- chunk arithmetic of the flat pair walk
// (initial full score, sat_sa_body.inc: FS_FLAT).  Plain C++ without a device intrinsic, so that a host program runs
// the very functions the kernel runs: tests/native/fs_chunks_check.cpp defines SAT_FS_CHUNKS_ONLY and gets this
// section alone.
//
// A wave holds 64 chains; chain c has the matched query SSEs `mapped` and their images `occ` (thinit's maps are order
// preserving: the a-th set bit of one belongs to the a-th of the other) and owns the pairs (a, b), a < b, of its
// matched SSEs: p = m (m - 1) / 2 of them, ordered by a, then b.  The chains that own a pair are numbered 0 .. NZ - 1
// in lane order ("compacted": lane r holds the sets of the r-th of them), the wave's P pairs are ordered by chain,
// then inside the chain, and lane t takes the pairs [t q, min((t + 1) q, P)) with q = ceil(P / 64).
#if defined(__HIPCC__)
#define SAT_FS_HD __host__ __device__ __forceinline__
#else
#define SAT_FS_HD inline
#endif

namespace satk {

// the sets a compacted lane at or past NZ holds: a chain of one pair, never counted, so that a lane that has
// finished its chunk (or has none) always stands on a pair it can address
#define SAT_FS_DUMMY_SET 3u

SAT_FS_HD int fs_pairs(uint32_t mapped)
{
    const int m = __builtin_popcount(mapped);
    return (m * (m - 1)) >> 1;
}
SAT_FS_HD int fs_chunk(int P) { return (P + 63) >> 6; }
// pairs of lane t's chunk
SAT_FS_HD int fs_chunk_pairs(int P, int q, int t)
{
    const int left = P - t * q;
    return left < 0 ? 0 : (left < q ? left : q);
}

// Where a lane stands: rm / ro = the chain's two sets from the current row on (lowest bits: the row's SSE i and its
// image), rk / rl = the row's partners not yet visited (lowest bits: the pair's SSE k and its image).  rk is never
// empty between two calls.
struct FsCursor { uint32_t rm, ro, rk, rl; };

// the cursor on pair `off` (0 <= off < fs_pairs(mapped)) of a chain: rows are stripped while the pair lies behind
// them, then partners
SAT_FS_HD FsCursor fs_seek(uint32_t mapped, uint32_t occ, int off)
{
    FsCursor c;
    c.rm = mapped;
    c.ro = occ;
    int len = __builtin_popcount(mapped) - 1;          // partners of row 0
    while (off >= len && len > 1) {
        off -= len;
        len--;
        c.rm &= c.rm - 1u;
        c.ro &= c.ro - 1u;
    }
    c.rk = c.rm & (c.rm - 1u);
    c.rl = c.ro & (c.ro - 1u);
    while (off > 0 && (c.rk & (c.rk - 1u)) != 0u) {
        off--;
        c.rk &= c.rk - 1u;
        c.rl &= c.rl - 1u;
    }
    return c;
}

// Leaves the pair the cursor is on (go = 1; go = 0 leaves the cursor alone): the next partner, behind the row's last
// one the next row, behind the chain's last row the first pair of the chain with the sets (nm, no).  All by selects.
// Returns whether the chain was left.
SAT_FS_HD bool fs_advance(FsCursor &c, uint32_t go, uint32_t nm, uint32_t no)
{
    c.rk &= c.rk - go;
    c.rl &= c.rl - go;
    const bool row_end = c.rk == 0u;
    const uint32_t e = row_end ? 1u : 0u;
    uint32_t rm = c.rm & (c.rm - e), ro = c.ro & (c.ro - e);
    const bool chain_end = row_end && (rm & (rm - 1u)) == 0u;
    rm = chain_end ? nm : rm;
    ro = chain_end ? no : ro;
    c.rm = rm;
    c.ro = ro;
    c.rk = row_end ? rm & (rm - 1u) : c.rk;
    c.rl = row_end ? ro & (ro - 1u) : c.rl;
    return chain_end;
}

}   // namespace satk

#ifndef SAT_FS_CHUNKS_ONLY

// Hook points of the diagnostic builds (phase timers, perturbations, duplicated LDS accesses, the per-move
// self-check): their code lives in diag/sat_diag.hpp, which the shipped library does not include - every hook is
// nothing here.
#ifdef SAT_DIAG
#include "diag/sat_diag.hpp"
#endif
#ifndef SAT_DIAG_ARGS
#define SAT_DIAG_ARGS
#endif
#ifndef SAT_PHASE_INIT
#define SAT_PHASE_INIT
#define SAT_PHASE(k)
#define SAT_PHASE_FLUSH
#endif
#ifndef SAT_DIAG_FS_ROWS_ONLY
#define SAT_DIAG_FS_ROWS_ONLY 0
#endif
#ifndef SAT_DIAG_DUP_CELLS
#define SAT_DIAG_DUP_CELLS(row, o0, o1, o2, o3)
#endif
#ifndef SAT_DIAG_DUP_MAPWORD
#define SAT_DIAG_DUP_MAPWORD(p)
#endif
#ifndef SAT_DIAG_DUP_ATOMIC
#define SAT_DIAG_DUP_ATOMIC(p)
#endif
#ifndef SAT_DIAG_DUP_MAPBYTE
#define SAT_DIAG_DUP_MAPBYTE(p)
#endif
#ifndef SAT_DIAG_PERTURB_INIT
#define SAT_DIAG_PERTURB_INIT
#define SAT_DIAG_PERTURB_STEP
#define SAT_DIAG_PERTURB_END
#endif
#ifndef SAT_DIAG_SELFCHECK_STEP
#define SAT_DIAG_SELFCHECK_STEP
#endif

// Cell layouts of a launch, chosen from its largest entry (satk::cell_layout)
#define SAT_CELLS_FULL8 0             // full matrix, 8-byte cells {f32 distance, code}
#define SAT_CELLS_FULL5 1             // full matrix, distances and code bytes in two arrays
#define SAT_CELLS_TRI5  2             // lower triangle, distances and code bytes in two arrays
// register budget of the option-specialised kernels with one lane per chain, as resident waves per SIMD
#ifndef SAT_FAST_WAVES
#define SAT_FAST_WAVES 6
#endif
// the initial full score of two chains walked by a pair of lanes together (one-word sets, one lane per chain)
#ifndef SAT_FS_TEAMS
#define SAT_FS_TEAMS 1
#endif
// ... or, where that applies, the wave's matched pairs in ONE order dealt to the 64 lanes in equal chunks (0: the team
// walk, for A/B builds)
#ifndef SAT_FS_FLAT
#define SAT_FS_FLAT 1
#endif
// the LORDER step's candidate of one-word db sets read from the rank table `pos` (0: the strip loop, for A/B builds)
#ifndef SAT_PICK_TABLE
#define SAT_PICK_TABLE 1
#endif
#define SAT_K_MAXITER 100
#define SAT_K_MAXDIM 111              // SAT_MAXDIM of satabsearch.h: the pitch of a pair's map
#define SAT_FS_UNROLL 2               // pairs per lane and round of the full score of an initial map
#define SAT_K_STEP_BLOCK0 32          // Philox block of SA step 0 (oracle/sa_oracle.h)
#define SAT_K_EPS 1.1e-7              // K.cu:67
#define SAT_K_NO_SCORE (-99999)       // K.cu:1009
#define SAT_K_QSENT 1.0e30f            // query-side "never within 4 A" distance
#define SAT_K_DSENT (-1.0e30f)         // db-side sentinel (null SSE, non-finite input)

// One query of a batch; a launch covers (db entries of one size bucket) x (queries of one
// size class): blockIdx.x picks the entry, blockIdx.y the query.
struct SatQuery {
    const float4   *qdist;        // [N1P/4][N1P] distances of 4 consecutive query SSEs (transposed)
    const uint32_t *qcode;        // [N1P/4][N1P] their 4 code bytes
    const uint8_t  *qtypes;       // [N1P]
    const uint2    *qpair;        // [N1P][N1P] dense cells {distance, code byte} for the full score of an initial map
    int32_t         n1;
    uint32_t        pad_;
    uint64_t        seed_q;       // seed + (query ordinal << 32)
    int32_t        *scores;       // [N] this query's score row
    int8_t         *ssemaps;      // [N][n1] this query's maps, -1 = unmatched
};

struct SatKernelArgs {
    // database shard (HBM)
    const int32_t  *orders;       // [N]
    const int64_t  *cell_off;     // [N] first packed cell
    const uint8_t  *tab_tri;      // packed lower triangles, code bytes
    const float    *dist_tri;     // packed lower triangles, distances
    const uint32_t *ordinal;      // [N] db file-order ordinal (stream key)
    const int32_t  *entry_list;   // entries handled by this launch
    int32_t         n_list;       // how many
    // A workgroup holds `epw` entries side by side: entry slot s = threads [s * tpe, (s + 1) * tpe) with its
    // own LDS carve at s * lds_stride.  The slots share nothing but the three workgroup barriers; the
    // host picks epw so that the CU's 128 LDS granules of 1280 bytes hold the most entries.
    int32_t         epw, tpe;
    uint32_t        lds_stride;   // bytes, a multiple of 16
    // queries of this launch's size class
    const SatQuery *queries;
    // options
    int32_t         lorder, lsoln, maxstart;
    int32_t         lpc_shift;    // log2(lanes per chain): 0, 1 or 2
    int32_t         compact;      // 1: the SA step may use the wave-level work compaction (its LDS tables exist)
    uint32_t       *bmap_slabs;   // LSOLN: best-map slab of workgroup g at g * bmap_slab_words
    uint32_t        bmap_slab_words;
    // Metropolis table
    const float    *ptab;         // ragged rows { 2^33, 2^32 * expf(-nd / temp) for nd = 0 .. last, 0.0 }
    const int32_t  *prow;         // [100][2] = {row offset, largest tabulated -delta}
    SAT_DIAG_ARGS                 // diagnostic builds only (diag/sat_diag.hpp): their counters
};

// Several matches per entry (sat_search_matches, sat_sa_match_kernel; DESIGN.md "Several matches per entry").
// Record pass: every chain keeps the own best of its current restart (score and the db set of the state that
// first reached it) and files it per restart in a scratch slab of its entry slot; the epilogue picks up to M
// restarts greedily (descending key, disjoint db sets).  Replay pass: chain c re-runs the c-th picked restart
// of its entry and writes that restart's own-best map.  Outputs are indexed by the query's descriptor index
// d (its position in the context's descriptor array) and the entry e: row d * n_entries + e.
struct SatMatchArgs {
    const SatQuery *desc_base;    // the descriptor array a.queries points into
    int32_t         n_entries;    // row length of the outputs
    int32_t         max_matches;  // M, 1 .. SAT_MAX_MATCHES
    int32_t         replay;       // 0: record pass, 1: replay pass (maps)
    int32_t         map_pitch;    // bytes per map in `maps`
    uint32_t       *rec_slabs;    // record pass: slab of workgroup slot g at g * rec_slab_words (like bmap_slabs)
    uint32_t        rec_slab_words;
    uint32_t        pad_;
    int32_t        *counts;       // [ndesc][N]           matches found, 1 .. M
    int32_t        *scores;       // [ndesc][N][M]        0 past the count
    int32_t        *restarts;     // [ndesc][N][M]        -1 past the count
    int8_t         *maps;         // [ndesc][N][M][map_pitch] replay pass: the picked restarts' own-best maps
};

// Pair mode (sat_search_pairs, sat_sa_pair_kernel; DESIGN.md "Re-scoring candidates").  A work item is one
// (query descriptor, entry) pair and a range [r0, r1) of its restarts; the launch's entry slots take items in
// turn (the slot's n_list bounds the table).  Restart r of a pair is the same Philox stream wherever it runs,
// so the items of one pair fold their arg-max keys (score, ~restart) into keys[pair] by atomicMax and the
// largest is exactly sat_search's.  The map pass re-runs each pair's winning restart as one item with LSOLN.
// Pair-match mode (sat_search_pairs_matches, sat_sa_pair_match_kernel): the same items with the match
// mode's per-restart records.  Record pass: an item files {s_r, D_r} of its restarts in its PAIR's slab (slab index
// `slab`, restart-major over all maxstart restarts, as the match kernel lays a slab out) and folds its key into
// keys[pair]; the selection over a pair's records is a kernel of its own (pair_match_select, sat_capi.hip), because
// the records of one pair come from several workgroups.  Map pass: one item per pair, chain c re-runs the pair's c-th
// picked restart; the match outputs are then indexed by the pair (row = item.pair).
struct SatPairItem {
    int32_t pair;                 // output index
    int32_t desc;                 // descriptor index (into SatKernelArgs::queries) of the query
    int32_t entry;                // index in the resident shard
    int32_t r0, r1;               // restarts r0 .. r1 - 1
    int32_t slab;                 // pair-match record pass: the pair's record slab in its launch (SatMatchArgs::rec_slabs)
    int32_t pad_[2];
};
struct SatPairArgs {
    const SatPairItem   *items;   // [n_list]
    unsigned long long  *keys;    // [pairs] zeroed before the score pass
    int8_t              *maps;    // [pairs][SAT_K_MAXDIM] map pass: the winning restart's map (bytes past n1 untouched)
};

namespace satk {

// ---------------------------------------------------------------- small bit sets
template <int W> struct Bits { uint32_t w[W]; };

template <int W> __device__ __forceinline__ Bits<W> bits_zero()
{
    Bits<W> b;
#pragma unroll
    for (int i = 0; i < W; i++) b.w[i] = 0u;
    return b;
}
// bits [0, pos) set; pos may be <= 0 or >= 32*W
template <int W> __device__ __forceinline__ Bits<W> bits_below(int pos)
{
    Bits<W> b;
    if constexpr (W == 1) {
        // one word, full-rate ops only: all-ones shifted right by 32 - clamp(pos, 0, 32), done as
        // two shifts of at most 16 so that a total of 32 really empties the word
        const int s = 32 - min(max(pos, 0), 32);          // v_med3_i32
        const int h = s >> 1;
        b.w[0] = (0xFFFFFFFFu >> h) >> (s - h);
        return b;
    }
    // several words: the word that holds `pos` gets the bits below it, the words under it are full, the rest
    // empty (pos < 0: no word is under or at it; pos >= 32 W: every word is under it) - two compares and two
    // selects per word where a clamped 64-bit shift per word cost twice that
    const int wi = pos >> 5;                                   // arithmetic shift: negative for pos < 0
    const uint32_t part = (1u << (pos & 31)) - 1u;
#pragma unroll
    for (int i = 0; i < W; i++) b.w[i] = i < wi ? 0xFFFFFFFFu : (i == wi ? part : 0u);
    return b;
}
template <int W> __device__ __forceinline__ void bits_set(Bits<W> &b, int pos)
{
#pragma unroll
    for (int i = 0; i < W; i++) b.w[i] |= ((pos >> 5) == i) ? (1u << (pos & 31)) : 0u;
}
template <int W> __device__ __forceinline__ void bits_clear(Bits<W> &b, int pos)
{
#pragma unroll
    for (int i = 0; i < W; i++) b.w[i] &= ~(((pos >> 5) == i) ? (1u << (pos & 31)) : 0u);
}
template <int W> __device__ __forceinline__ int bits_count(const Bits<W> &b)
{
    int c = 0;
#pragma unroll
    for (int i = 0; i < W; i++) c += __popc(b.w[i]);
    return c;
}
template <int W> __device__ __forceinline__ bool bits_any(const Bits<W> &b)
{
    uint32_t o = 0u;
#pragma unroll
    for (int i = 0; i < W; i++) o |= b.w[i];
    return o != 0u;
}
// clears the lowest set bit (no-op on an empty set)
template <int W> __device__ __forceinline__ void bits_drop_lowest(Bits<W> &b)
{
    bool done = false;
#pragma unroll
    for (int i = 0; i < W; i++) {
        const bool here = !done && b.w[i] != 0u;
        b.w[i] = here ? b.w[i] & (b.w[i] - 1u) : b.w[i];
        done = done || here;
    }
}
template <int W> __device__ __forceinline__ int bits_lowest(const Bits<W> &b)   // -1 if empty
{
    int r = -1;
#pragma unroll
    for (int i = W - 1; i >= 0; i--) r = b.w[i] ? 32 * i + (__ffs(b.w[i]) - 1) : r;
    return r;
}
template <int W> __device__ __forceinline__ int bits_highest(const Bits<W> &b)  // -1 if empty
{
    int r = -1;
#pragma unroll
    for (int i = 0; i < W; i++) r = b.w[i] ? 32 * i + (31 - __clz(b.w[i])) : r;
    return r;
}
// position of the r-th (0-based, ascending) set bit of a non-zero word with > r bits
__device__ __forceinline__ int word_select(uint32_t v, int r)
{
    // branch-free rank select by halving: counts of the low half decide the side
    uint32_t a = v - ((v >> 1) & 0x55555555u);
    uint32_t b = (a & 0x33333333u) + ((a >> 2) & 0x33333333u);
    uint32_t c = (b + (b >> 4)) & 0x0F0F0F0Fu;
    uint32_t d = (c + (c >> 8)) & 0x00FF00FFu;
    int pos = 0;
    int t = (int)(d & 0xFFu);
    if (r >= t) { pos = 16; r -= t; }
    t = (int)((c >> pos) & 0xFu);
    if (r >= t) { pos += 8; r -= t; }
    t = (int)((b >> pos) & 0x7u);
    if (r >= t) { pos += 4; r -= t; }
    t = (int)((a >> pos) & 0x3u);
    if (r >= t) { pos += 2; r -= t; }
    t = (int)((v >> pos) & 0x1u);
    if (r >= t) { pos += 1; }
    return pos;
}
template <int W> __device__ __forceinline__ int bits_select(const Bits<W> &b, int r)
{
    // the word that holds the r-th bit and the rank inside it first (popcounts), then ONE rank select
    uint32_t word = b.w[0];
    int base = 0, rr = r;
    bool found = false;
#pragma unroll
    for (int i = 0; i < W; i++) {
        const int c = __popc(b.w[i]);
        const bool here = !found && r < c;
        word = here ? b.w[i] : word;
        base = here ? 32 * i : base;
        rr = here ? r : rr;
        found = found || here;
        r -= c;
    }
    // (r beyond the set: callers never ask; an empty word would select position 31 of nothing)
    return found ? base + word_select(word, rr) : 0;
}

// p = the highest set bit of `mapped` at or below position `upto` (0 when there is none: `none`).  One and two
// words as 32- and 64-bit arithmetic, more words word by word.
template <int W> __device__ __forceinline__ void highest_mapped_upto(const Bits<W> &mapped, int upto, int &p, bool &none)
{
    if constexpr (W == 1) {
        const uint32_t low = mapped.w[0] & (0xFFFFFFFFu >> (31 - upto));
        p = 31 ^ __builtin_clz(low | 1u);
        none = low == 0u;
    } else if constexpr (W == 2) {
        const unsigned long long m = (unsigned long long)mapped.w[0] | ((unsigned long long)mapped.w[1] << 32);
        const unsigned long long low = m & (~0ull >> (63 - upto));
        p = 63 ^ __builtin_clzll(low | 1ull);
        none = low == 0ull;
    } else {
        Bits<W> lowpart, below = bits_below<W>(upto + 1);
#pragma unroll
        for (int w = 0; w < W; w++) lowpart.w[w] = mapped.w[w] & below.w[w];
        p = bits_highest<W>(lowpart);
        none = p < 0;
        p = none ? 0 : p;
    }
}

// ---------------------------------------------------------------- pair scores
// Sum of the four pair scores of one map word: query SSEs 4kw..4kw+3 against the db SSEs
// in `word` (one byte each), all on db row `row` (the image of the moved / anchor SSE).
//   qd, qc   the query group's distances and code bytes for this lane's column
//   force    0x04 in byte s forces pair s to score 0 (used by the full score for k <= i)
// Returns acc + sum.  See the file header for the arithmetic.
// A row of the db entry's cell matrix in LDS, in one of three layouts picked per LAUNCH from its largest entry
// (cell_layout):
//   FULL8  entries of up to 32 SSEs: the full matrix of 8-byte cells {f32 distance, code byte}, one ds_read_b64 per
//          pair at row base + image;
//   FULL5  up to 48 SSEs: the full matrix, distances and code bytes in two arrays (5 bytes per cell, two reads per
//          pair): 37 % less LDS where the cells start to limit the workgroups per CU;
//   TRI5   above 48 SSEs: only the lower TRIANGLE (the matrix is symmetric), two arrays: a 96-SSE entry takes 23.8 KB
//          where the full split matrix took 46.6 KB, i.e. 4-5 resident workgroups per CU instead of 2-3, for ~17 cycles
//          of index arithmetic per pair (tri_index).  Measured per entry order (profiles/r03_cost_by_order.txt): the
//          triangle loses 10-19 % at 40 and 48 SSEs, where the LDS does not limit the occupancy and the index
//          arithmetic is pure cost, and wins from 56 SSEs on (-5 % at 64, -12 % at 88, -21 % at 111 under a 32-SSE
//          query; up to -44 % under an 8-SSE query).  The null SSE is row n2 of the triangle (n2 + 1 sentinel
//          cells): an unmatched image l = n2 is the larger index of every pair it appears in.
template <int CELLS> struct DbRow;
template <> struct DbRow<SAT_CELLS_FULL8> { const uint2 *cells; };
template <> struct DbRow<SAT_CELLS_FULL5> { const float *dist; const uint8_t *code; };
template <> struct DbRow<SAT_CELLS_TRI5> { const float *dist; const uint8_t *code; int j; };
__host__ __device__ inline int cell_layout(int n2max) { return n2max <= 32 ? SAT_CELLS_FULL8 : (n2max <= 48 ? SAT_CELLS_FULL5 : SAT_CELLS_TRI5); }
// 32-bit words of a db-side bit set (the kernels' M2W) for entries of up to n2 SSEs: the launch's template argument, the
// record slabs' row count and the selection kernel's set width all come from here
__host__ __device__ inline int set_words(int n2) { return n2 <= 32 ? 1 : (n2 <= 64 ? 2 : 4); }
// cell (j, l) of the lower triangle: row max(j, l), column min(j, l)
__device__ __forceinline__ int tri_index(int j, int l)
{
    const int mx = max(j, l), mn = min(j, l);
    return (int)((__umul24((uint32_t)mx, (uint32_t)mx) + (uint32_t)mx) >> 1) + mn;
}
__host__ __device__ inline uint32_t tri_cells(int n2) { return (uint32_t)(n2 + 1) * (uint32_t)(n2 + 2) / 2u; }   // rows 0 .. n2
// the distance bits and the code byte of cell (row, l)
template <int CELLS> __device__ __forceinline__ uint2 db_cell(const DbRow<CELLS> row, int l)
{
    if constexpr (CELLS == SAT_CELLS_FULL8) return row.cells[l];
    else if constexpr (CELLS == SAT_CELLS_FULL5) return uint2{ __float_as_uint(row.dist[l]), row.code[l] };
    else { const int c = tri_index(row.j, l); return uint2{ __float_as_uint(row.dist[c]), row.code[c] }; }
}

// Chain-map bytes of the FULL8 launches (entries of up to 32 SSEs, one-word db sets) hold the BYTE OFFSET of the
// image's cell inside a row of the cell matrix, l << 3 for the images l = 0..31, and 0x04 for "unmatched": the address
// of a pair's cell is then row base + one byte of the map word, a single v_add_u32_sdwa per pair where the plain
// index took a byte extract and a shift-add, the row pitch (8 (n2 + 1) bytes) needs no power of two, and the
// unmatched flag sits where the selector of quad_terms has its "scores 0" bit.  An unmatched byte addresses cell 0 of
// the row (a real cell, in the bank of the sentinel column of a 32-SSE entry) and the flag drops the term.  Only the
// kernel sees the encoding: its outputs, the items of the compaction tables and every other layout keep plain indices
// with the null SSE n2 for "unmatched".
#define SAT_MAP_UNMATCHED 0x04u
// Bytes of the rank table `pos` of a launch with one-word db sets: up to 32 SSEs, and one byte more for the lanes of
// a step that have no candidate - they read at up to (SSEs of the type) past its run's start and drop the byte.
#define SAT_POS_BYTES 36u
__host__ __device__ constexpr bool map_bytes_scaled(int m2w, int cells) { return cells == SAT_CELLS_FULL8 && m2w == 1; }
template <bool SCALED> __device__ __forceinline__ uint32_t map_encode(int j, int nullj)
{
    if constexpr (SCALED) return j == nullj ? SAT_MAP_UNMATCHED : (uint32_t)j << 3;
    else return (uint32_t)j;
}
template <bool SCALED> __device__ __forceinline__ int map_decode(uint32_t b, int nullj)
{
    if constexpr (SCALED) return (b & SAT_MAP_UNMATCHED) ? nullj : (int)(b >> 3);
    else return (int)b;
}

template <int CELLS>
__device__ __forceinline__ int quad_terms(const float4 qd, const uint32_t qc, const DbRow<CELLS> row,
                                          const uint32_t word, const uint32_t force, const int acc)
{
    uint2 d0, d1, d2, d3;
    if constexpr (CELLS == SAT_CELLS_FULL8) {
        // scaled map bytes (map_bytes_scaled): cell address = row base + byte s of the word without its flag bits.  The
        // masked word is formed once and kept opaque, so that each byte extract stays next to its add and the two
        // become one v_add_u32_sdwa (left to itself the compiler masks every byte on its own again)
        uint32_t offs = word & 0xF8F8F8F8u;
        asm("" : "+v"(offs));
        const uint32_t o0 = offs & 0xFFu, o1 = (offs >> 8) & 0xFFu, o2 = (offs >> 16) & 0xFFu, o3 = offs >> 24;
        SAT_DIAG_DUP_CELLS(row, o0, o1, o2, o3);
        const unsigned char *const base = reinterpret_cast<const unsigned char *>(row.cells);
        d0 = *reinterpret_cast<const uint2 *>(base + o0);
        d1 = *reinterpret_cast<const uint2 *>(base + o1);
        d2 = *reinterpret_cast<const uint2 *>(base + o2);
        d3 = *reinterpret_cast<const uint2 *>(base + o3);
    } else {
        const uint32_t l0 = word & 0xFFu, l1 = (word >> 8) & 0xFFu, l2 = (word >> 16) & 0xFFu, l3 = word >> 24;
        d0 = db_cell<CELLS>(row, (int)l0);
        d1 = db_cell<CELLS>(row, (int)l1);
        d2 = db_cell<CELLS>(row, (int)l2);
        d3 = db_cell<CELLS>(row, (int)l3);
    }
    // sign bit of t = "distances differ by more than 4 A"
    const float t0 = 4.0f - fabsf(qd.x - __uint_as_float(d0.x));
    const float t1 = 4.0f - fabsf(qd.y - __uint_as_float(d1.x));
    const float t2 = 4.0f - fabsf(qd.z - __uint_as_float(d2.x));
    const float t3 = 4.0f - fabsf(qd.w - __uint_as_float(d3.x));
    // v_perm_b32(S0, S1, sel): selector 0-3 = byte of S1, 4-7 = byte of S0, 0x0C = zero
    const uint32_t x = __builtin_amdgcn_perm(d1.y, d0.y, 0x0C0C0400u) ^
                       __builtin_amdgcn_perm(d3.y, d2.y, 0x04000C0Cu) ^ qc;
    const uint32_t z = (x + 0x77777777u) & 0x88888888u;             // bit 3: low nibbles differ, bit 7: high
    uint32_t sel;
    if constexpr (CELLS == SAT_CELLS_FULL8) {
        // selectors 0x09 / 0x0B give 0xFF or 0x00 by the SIGN of S1 / S0: the "too far" bytes come out clean, without
        // the shift that moved bit 7 to bit 2.  z >> 3 and z >> 6 hold bits 0, 1, 4 and 5 of a byte and a map byte
        // bits 2 (unmatched) and 3-7 (offset), so ONE or-or joins the code bits with the unmatched flag, and the
        // and-or that merged the distance bit now also strips everything above bit 2: an unmatched SSE costs no
        // instruction of its own.
        const uint32_t far = __builtin_amdgcn_perm(__float_as_uint(t1), __float_as_uint(t0), 0x0C0C0B09u) |
                             __builtin_amdgcn_perm(__float_as_uint(t3), __float_as_uint(t2), 0x0B090C0Cu);
        sel = __builtin_amdgcn_bitop3_b32(z >> 3, z >> 6, word, 0xFE);                        // a | b | c
        sel = __builtin_amdgcn_bitop3_b32(sel, far, 0x07070707u, 0xA8);                       // (a | b) & c
    } else {
        const uint32_t far = __builtin_amdgcn_perm(__float_as_uint(t1), __float_as_uint(t0), 0x0C0C0703u) |
                             __builtin_amdgcn_perm(__float_as_uint(t3), __float_as_uint(t2), 0x07030C0Cu);
        // ((z >> 3) | (z >> 6)) & 0x03030303 and the merge of the distance bits as two v_bitop3_b32 (full
        // rate; the and-or / or3 forms the compiler picks for the plain expression issue at half rate)
        sel = __builtin_amdgcn_bitop3_b32(z >> 3, z >> 6, 0x03030303u, 0xA8);        // (a | b) & c
        sel = __builtin_amdgcn_bitop3_b32(far >> 5, 0x04040404u, sel, 0xEA);          // (a & b) | c
    }
    sel |= force;
    const uint32_t terms = __builtin_amdgcn_perm(0u, 0xFE010102u, sel);   // {2, 1, 1, -2 | 0, 0, 0, 0}
    return __builtin_amdgcn_sdot4((int)terms, 0x01010101, acc, false);
}

// One pair score (the full score of an initial map walks the matched pairs one by one): query cell
// {distance, code byte}, db cell likewise; same arithmetic as one byte lane of quad_terms.
__device__ __forceinline__ int pair_term(const uint32_t qd_bits, const uint32_t qc, const uint32_t dd_bits, const uint32_t dc)
{
    const float t = 4.0f - fabsf(__uint_as_float(qd_bits) - __uint_as_float(dd_bits));   // sign bit: more than 4 A apart
    const uint32_t z = ((qc ^ dc) + 0x77u) & 0x88u;                      // bit 3: low nibbles differ, bit 7: high
    uint32_t sel = __builtin_amdgcn_bitop3_b32(z >> 3, z >> 6, 0x3u, 0xA8);                  // (a | b) & c
    sel = __builtin_amdgcn_bitop3_b32(__float_as_uint(t) >> 29, 0x4u, sel, 0xEA);             // (a & b) | c
    const uint32_t terms = __builtin_amdgcn_perm(0u, 0xFE010102u, sel);  // byte 0 = {2, 1, 1, -2 | 0, 0, 0, 0}[sel]
    return (int)(int8_t)(terms & 0xFFu);
}

// ---------------------------------------------------------------- random streams
// Block `block` of the chain's Philox stream, written out by hand (NOT a call into rocRAND), laid out as rocRAND's:
// key = seed_q, counter = (block, 0, subsequence lo, subsequence hi).
__device__ __forceinline__ uint4 philox_block(uint64_t seed_q, uint64_t subsequence, uint32_t block)
{
    // Philox4x32-10 written out (same words as rocrand_init(seed_q, subsequence, 4 * block) +
    // rocrand4 - checked on the device against rocRAND's own device API by
    // tests/test_gpu_parity.py::test_philox_block_is_rocrands_block): in every use here the block and the low
    // subsequence word are wave-uniform, so rounds 1-3 are left to the compiler (it keeps the
    // uniform half on the scalar unit); from round 4 on all four words are per lane and the two
    // three-way XORs of a round are one v_bitop3_b32 each.
    uint32_t c0 = block, c1 = 0u, c2 = (uint32_t)subsequence, c3 = (uint32_t)(subsequence >> 32);
    uint32_t k0 = (uint32_t)seed_q, k1 = (uint32_t)(seed_q >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0, n2;
        if (r < 3) {
            n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
            n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        } else {
            n0 = __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c1, k0, 0x96);
            n2 = __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c3, k1, 0x96);
        }
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return uint4{ c0, c1, c2, c3 };
}
// 2^32 * (uniform draw of word v): rocRAND's uniform_distribution is 2^-32 + float(v) * 2^-32
// in (0, 1] (rocrand_uniform.h:65-68); scaling by a power of two is exact, so float(v) + 1.0f is
// that value times 2^32 with the same two roundings.
__device__ __forceinline__ float draw32(uint32_t v)
{
    return (float)v + 1.0f;
}
__device__ __forceinline__ float to_uniform(uint32_t v)
{
    return draw32(v) * 2.3283064365386963e-10f;
}
// Index draw from a 16-bit value v: u = (v + 1) * 2^-16 in (0, 1] (exact in float), index =
// (int)((u - EPS) * n) evaluated in double, as K.cu:1042 and K.cu:710 do.  For n <= 111 that equals the integer
// ((v + 1) * n - 1) >> 16: when (v + 1) * n is a multiple of 2^16 the EPS term drops the index by
// one, otherwise the fractional part is at least 2^-16 > EPS * n and nothing changes
// (tests/test_oracle_units.py checks all 65536 x 111 cases against the double expression).
// nm1 = max(n - 1, 0); n = 0 gives 0.
__device__ __forceinline__ int scaled_index16(uint32_t v16, int n, int nm1)
{
    return (int)(__umul24(v16, (uint32_t)n) + (uint32_t)nm1) >> 16;
}

// Work compaction (SA step): a listed row is served by `lpi` lanes, each taking `wpl` <= 4 map
// words (word kw, kw + lpi, ...), so the map of a chain is padded to wpl * lpi >= n1w words.
__host__ __device__ inline void compaction_shape(int n1w, int &lpi, int &wpl)
{
    lpi = (n1w + 3) >> 2;
    wpl = lpi > 0 ? (n1w + lpi - 1) / lpi : 1;
    if (lpi < 1) lpi = 1;
}
__host__ __device__ inline int map_words(int n1w)
{
    int lpi, wpl;
    compaction_shape(n1w, lpi, wpl);
    return lpi * wpl;
}

// LDS carve of one workgroup, byte offsets from the dynamic-LDS base.  ONE function for the kernel
// (its own entry's n2, its own query's padded map words) and for the host (the launch's largest):
// the two cannot disagree, every offset keeps the alignment its users need (cells 16, query cells
// 16, 64-bit reduction keys / the LSOLN leader key 8: a 64-bit LDS atomic on a 4-byte aligned
// address faults), and the total grows with n2 and with the map words, so a workgroup sized for
// the launch's largest member holds every member.
struct LdsLayout {
    uint32_t code;        // split cells only: the code bytes (distances start at 0)
    uint32_t qdist;       // query cells staged in LDS (QLDS): float4 groups ...
    uint32_t qcode;       // ... and their code dwords
    uint32_t smap;        // chain maps, word-interleaved [word][chain], row stride chains + 1
    uint32_t tmask;       // [4 types][4 words] db SSEs of a type
    uint32_t qtypes;      // query SSE types
    uint32_t qmask;       // one-word db sets only: per query SSE the mask of the db SSEs of its type (tmask[qtypes[i]])
    uint32_t qbase;       // one-word db sets only: per query SSE the first byte of its type's run in `pos`
    uint32_t pos;         // one-word db sets only: the entry's SSEs sorted by (type, index), SAT_POS_BYTES bytes
    uint32_t leader;      // the LSOLN leader key (64-bit)
    uint32_t red;         // the waves' arg-max keys (64-bit), red_stride bytes apart
    uint32_t red_stride;
    uint32_t items;       // per-wave item tables of the work compaction
    uint32_t total;
};
// m2w = 32-bit words of a db-side bit set in this launch's size class (1, 2 or 4); cells = its cell layout
// (SAT_CELLS_*: DbRow).
__host__ __device__ inline LdsLayout lds_layout(int m2w, int cells, int n2, int words, int n1p, int chains, int threads,
                                                 bool q_in_lds, bool compact)
{
    LdsLayout L;
    const bool split = cells != SAT_CELLS_FULL8;
    // full matrix: rows 0 .. n2-1, columns 0 .. n2: the null SSE (index n2) has a column - map bytes
    // of unmatched query SSEs point at it - but no row: a null image scores 0 and its row is never summed
    uint32_t dcells = (uint32_t)n2 * (uint32_t)(n2 + 1);
    uint32_t off;
    if (split) {                                              // 4-byte distances + 1-byte codes; TRI5: lower triangle incl. the null row
        if (cells == SAT_CELLS_TRI5) dcells = tri_cells(n2);
        dcells = (dcells + 3u) & ~3u;
        L.code = dcells * 4u;
        off = L.code + ((dcells + 15u) & ~15u);
    } else {                                                  // 8-byte cells
        dcells = (dcells + 1u) & ~1u;
        L.code = 0u;
        off = dcells * 8u;
    }
    L.qdist = off;                                            // 16-byte aligned in both layouts
    if (q_in_lds) off += (uint32_t)words * (uint32_t)n1p * 16u;
    L.qcode = off;
    if (q_in_lds) off += (uint32_t)words * (uint32_t)n1p * 4u;
    L.smap = off;
    // an even word count keeps what follows 8-byte aligned
    off += (((uint32_t)words * (uint32_t)(chains + 1) + 1u) & ~1u) * 4u;
    L.tmask = off;
    off += 4u * (uint32_t)m2w * 4u;                           // [4 types][m2w words]
    L.qtypes = off;
    off += ((uint32_t)n1p + 15u) & ~15u;
    L.qmask = off;
    if (m2w == 1) off += (uint32_t)n1p * 4u;
    L.qbase = off;
    if (m2w == 1) off += (uint32_t)n1p;                       // (n1p is a multiple of 4)
    L.pos = off;
    if (m2w == 1) off += SAT_POS_BYTES;
    off = (off + 7u) & ~7u;
    L.leader = off;
    off += 8u;
    // the arg-max key of wave w: with item tables, the first 8 bytes of the wave's own table (it is done
    // with the table by then, and no other wave touches it); without, an array of 16 keys
    L.red = off;
    L.red_stride = compact ? 256u : 8u;
    if (!compact) off += 16u * 8u;
    L.items = off;
    if (compact) off += (uint32_t)((threads + 63) / 64) * 64u * 4u;      // compaction handles <= 64 rows per wave
    L.total = off;
    return L;
}

// LDS byte size of one workgroup (host side: the launch's largest query and entry)
__host__ __device__ inline size_t lds_bytes(int n1, int n1p, int n2, int chains, int threads, bool lsoln, bool q_in_lds,
                                             bool compact)
{
    (void)lsoln;                                              // the best maps live in global memory
    return lds_layout(set_words(n2), cell_layout(n2), n2, map_words((n1 + 3) >> 2), n1p, chains, threads, q_in_lds, compact).total;
}

}  // namespace satk


// N1P: pitch of the query cell matrix (>= 4*ceil(n1/4)); M2W: 32-bit words of a db-side
// bit set (n2 <= 32*M2W); QLDS: query cells staged in LDS (else read through L1/L2).
// OPT: >= 0: bit 0 LORDER, bit 1 LSOLN, bits 2-3 log2(lanes per chain) as compile-time facts (lanes per
// chain above one only instantiated for the largest entries, M2W = 4, where that layout is the default).
// -1 = every option is read from the arguments (the general instantiation: forced layouts, several lanes
// per chain, forced layouts); otherwise the options are compile-time facts - bit 0 LORDER, bit 1
// LSOLN, one lane per chain, work compaction exactly when LORDER - and their tests leave the SA
// step loop (the general kernel spills ~90 SGPRs and is ~9 % slower on the bench shape).
// WPL: map words per lane in the compacted rounds (satk::compaction_shape) when every query of
// the launch has the same; 0 = read it from the query (a four-way switch per step).
// CELLS: the launch's cell layout (SAT_CELLS_*, satk::cell_layout of its largest entry).
// MATCH: the match mode (SatMatchArgs), only in sat_sa_match_kernel; PAIRS: the pair mode (SatPairArgs), only in
// sat_sa_pair_kernel; both: sat_sa_pair_match_kernel; the plain kernels compile without any of it.
template <int N1P, int M2W, bool QLDS, int OPT, int WPL, int CELLS>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu((OPT < 0 || OPT >= 4) ? 4 : SAT_FAST_WAVES)))
sat_sa_kernel(const SatKernelArgs a)
{
    constexpr bool MATCH = false, PAIRS = false;
    const SatMatchArgs mx{};
    const SatPairArgs px{};
#include "sat_sa_body.inc"
}

// The match mode's two passes (SatMatchArgs): options read from the arguments, as in the general instantiation.
template <int N1P, int M2W, bool QLDS, int CELLS>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4)))
sat_sa_match_kernel(const SatKernelArgs a, const SatMatchArgs mx)
{
    constexpr bool MATCH = true, PAIRS = false;
    constexpr int OPT = -1, WPL = 0;
    const SatPairArgs px{};
#include "sat_sa_body.inc"
}

// The pair mode's kernel (SatPairArgs): grid.x covers the item table, grid.y is 1.  OPT as in sat_sa_kernel, with
// LSOLN off in the option-specialised instantiations (the map pass runs the general one); map words per lane read
// per query.
template <int N1P, int M2W, bool QLDS, int OPT, int CELLS>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu((OPT < 0 || OPT >= 4) ? 4 : SAT_FAST_WAVES)))
sat_sa_pair_kernel(const SatKernelArgs a, const SatPairArgs px)
{
    constexpr bool MATCH = false, PAIRS = true;
    constexpr int WPL = 0;
    const SatMatchArgs mx{};
#include "sat_sa_body.inc"
}

// The pair-match mode's record and map passes (SatPairArgs items, SatMatchArgs records and outputs): options read from
// the arguments, one instantiation per query class / db set width / cell layout, as the match kernel.
template <int N1P, int M2W, bool QLDS, int CELLS>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4)))
sat_sa_pair_match_kernel(const SatKernelArgs a, const SatPairArgs px, const SatMatchArgs mx)
{
    constexpr bool MATCH = true, PAIRS = true;
    constexpr int OPT = -1, WPL = 0;
#include "sat_sa_body.inc"
}

#endif   // SAT_FS_CHUNKS_ONLY
