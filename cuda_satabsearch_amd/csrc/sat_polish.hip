// sat_polish.hip - polish of the best restarts' maps (sat_search_pairs_polish and its refine / multi-GPU forms,
// include/satabsearch.h).
//
// The pair-match mode's record pass files the own best s_r of every restart of a pair; its map pass re-runs chosen
// restarts for their own-best maps.  Between the two, pair_polish_select (sat_pairs.hip, beside pair_match_select, which
// it is without the set test) takes the T largest keys (s_r, ~r) of a pair, and behind them pair_polish climbs from each
// of the T maps to a local optimum of the search's neighbourhood by best improvement and reports the best of the T
// results.  The polish kernels and their launch code live here; sat_pair_matches_launch calls them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "sat_pairs.hpp"

namespace {

// ---------------------------------------------------------------- polish
struct PolishArgs {
    const SatPairItem *items;     // the launch's map items: one per pair (pair, descriptor, entry)
    const SatQuery *desc;
    const int32_t *orders;
    const int64_t *cell_off;
    const uint8_t *tab_tri;
    const float *dist_tri;
    const int32_t *counts;        // [pairs]        ranks the selection filled
    const int32_t *scores;        // [pairs][T]     s_r of rank t
    const int32_t *restarts;      // [pairs][T]
    const int8_t *maps;           // [pairs][T][SAT_MAXDIM] own-best map of rank t (the map pass)
    int32_t T, lorder;
    int32_t n2max;                // the LDS carve holds the triangle of an entry of up to n2max SSEs
    int32_t npairs;               // row length of `out`
    int32_t nitems;               // pair_polish_group: items of the launch (a workgroup holds several)
    int32_t *out;                 // [4][npairs]: score, base score, restart, moves (-1: error)
    unsigned long long *okeys;    // [pairs] pair_key(score, ~0): the high word of a pair key, low word 0 (the refine ranking's)
    int8_t *omaps;                // [pairs][SAT_MAXDIM] the winner's polished map, -1 = unmatched
};

constexpr int kListStride = 112;   // entries of a wave's map / matched list in LDS (SAT_MAXDIM rounded up)

__host__ __device__ inline uint32_t polish_cells(int n2) { return ((uint32_t)n2 * (uint32_t)(n2 + 1) / 2u + 15u) & ~15u; }
// LDS: distances [cells] f32 | codes [cells] | db types [112] | query types [112] | per wave: matched list, query
// distances and query codes of the row in hand [3][112] u32 | per wave: map [112] i8 | per wave: polished score, moves
__host__ __device__ inline uint32_t polish_lds_bytes(int n2max, int T)
{
    return polish_cells(n2max) * 5u + 2u * kListStride + (uint32_t)T * (kListStride * 13u + 8u);
}

// the lanes of a wave exchange data through LDS (DS operations of one wave execute in order)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One workgroup per pair, wave t polishes the map of rank t: the T maps of a pair share the entry, whose packed
// triangle is staged once (cleaned as the SA kernel cleans it: NaN / inf become the sentinel that never passes the
// distance test).  A round of a wave walks the query SSEs i (wave-uniform); the lanes are the db SSEs j (two trips
// above 64) and sum row(i, j | m) over the matched list with satk::pair_term - the SA kernel's arithmetic for one
// cell pair.  The query cells {distance, code} of row i against the matched list come from the blob's dense array: lane x
// loads the cell of the list's x-th SSE one row ahead (the load of row i + 1 flies under the sums of row i) and files it
// in LDS beside the list, so the sum reads three broadcast words per term and no load depends on another.  Every round
// recomputes every row: a map costs (moves + 1) x n1 x matched terms per lane, and the waves of the slowest maps are
// what a launch waits for (DESIGN.md 6h has the figures and the row table that would make later rounds cheap).
// The diagonal cell of the dense array is the query's sentinel, so the list's own entry for i adds 0 and needs no test.
// The old row is the lane j = m[i].  Each lane keeps its largest key (delta, ~i, ~(j + 1)) over the round, one
// butterfly reduces them, the move is applied and the matched list rebuilt by ballot compaction.  No atomics, no 64-bit
// LDS values.  Scores lie in [-n1 (n1 - 1), n1 (n1 - 1)] and every move gains at least 1, so 2 n1 (n1 - 1) + 1 rounds
// always reach a round without a move; a wave that does not is reported (moves = -1) instead of spinning.
__global__ void __launch_bounds__(64 * SAT_MAX_MATCHES) pair_polish(const PolishArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, nthreads = (int)blockDim.x;
    const int T = a.T;
    const uint32_t cells = polish_cells(a.n2max);
    float *distL = reinterpret_cast<float *>(lds);
    uint8_t *codeL = lds + (size_t)cells * 4u;
    uint8_t *type2 = codeL + cells;
    uint8_t *qtypeL = type2 + kListStride;
    uint32_t *listL = reinterpret_cast<uint32_t *>(qtypeL + kListStride) + (size_t)w * 3u * kListStride;
    uint32_t *qdL = listL + kListStride, *qcL = qdL + kListStride;
    int8_t *mapsL = reinterpret_cast<int8_t *>(qtypeL + kListStride + (size_t)T * kListStride * 12u);
    int8_t *mapL = mapsL + (size_t)w * kListStride;
    int32_t *resL = reinterpret_cast<int32_t *>(mapsL + (size_t)T * kListStride);       // [T] scores, [T] moves

    const SatPairItem it = a.items[blockIdx.x];
    const int p = it.pair;
    const SatQuery Q = a.desc[it.desc];
    const int n1 = Q.n1, n1p = n1 <= 16 ? 16 : (n1 <= 32 ? 32 : (n1 <= 64 ? 64 : 112));
    const int e = it.entry, n2 = a.orders[e];
    const int count = a.counts[p];
    const bool sane = n2 >= 1 && n2 <= a.n2max && n1 >= 1 && n1 <= SAT_K_MAXDIM && count >= 1 && count <= T;

    if (sane) {
        const uint8_t *tt = a.tab_tri + a.cell_off[e];
        const float *dd = a.dist_tri + a.cell_off[e];
        const int ncell = (n2 * (n2 + 1)) >> 1;
        for (int c = tid; c < ncell; c += nthreads) {
            const float v = dd[c];
            distL[c] = fabsf(v) <= 3.0e38f ? v : SAT_K_DSENT;
            codeL[c] = tt[c];
        }
        for (int j = tid; j < n2; j += nthreads) type2[j] = tt[((j * (j + 1)) >> 1) + j] & 3u;
        for (int i = tid; i < n1; i += nthreads) qtypeL[i] = Q.qtypes[i];
    }
    __syncthreads();

    if (sane && w < count) {
        const uint2 *qpair = Q.qpair;
        const int8_t *src = a.maps + ((size_t)p * T + w) * SAT_MAXDIM;
        for (int i = lane; i < kListStride; i += 64) mapL[i] = i < n1 ? src[i] : (int8_t)-1;
        wave_sync();
        // occupied db SSEs (wave-uniform): bit j of occ[j >> 6]
        unsigned long long occ[2] = { 0ull, 0ull };
        for (int i = 0; i < n1; i++) {
            const int j = mapL[i];
            if (j >= 0 && j < n2) occ[j >> 6] |= 1ull << (j & 63);
        }
        int score = a.scores[(size_t)p * T + w], moves = 0;
        const int cap = 2 * n1 * (n1 - 1) + 1;
        const bool two = n2 > 64;
        const int j0 = lane, j1 = lane + 64;
        const int a0 = min(j0, n2 - 1), a1 = min(j1, n2 - 1);              // addressing only: lanes past n2 are masked
        const uint32_t t0 = type2[a0], t1 = type2[a1];
        bool done = false;
        for (int round = 0; round < cap && !done; round++) {
            // the matched list (k, m[k]), ascending k
            int nm = 0;
            for (int trip = 0; trip < 2; trip++) {
                const int k = lane + 64 * trip;
                const int l = min((int)mapL[min(k, kListStride - 1)], n2 - 1);      // (an image is below n2: the clamp guards the cell index)
                const bool on = k < n1 && l >= 0;
                const unsigned long long mask = __builtin_amdgcn_ballot_w64(on);
                const int pos = nm + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                if (on) listL[pos] = (uint32_t)k | ((uint32_t)l << 8);
                nm += __popcll(mask);
            }
            wave_sync();
            // lane x serves the list's x-th and (x + 64)-th SSE: their cells of row 0 are on the way
            const bool has0 = lane < nm, has1 = lane + 64 < nm;
            const int kx0 = has0 ? (int)(listL[lane] & 0xFFu) : 0, kx1 = has1 ? (int)(listL[lane + 64] & 0xFFu) : 0;
            uint2 nxt0 = qpair[kx0], nxt1 = qpair[kx1];
            unsigned long long best = 0ull;
            for (int i = 0; i < n1; i++) {
                wave_sync();                               // the sums of the row before have read its cells
                if (has0) { qdL[lane] = nxt0.x; qcL[lane] = nxt0.y; }
                if (has1) { qdL[lane + 64] = nxt1.x; qcL[lane + 64] = nxt1.y; }
                const int inext = min(i + 1, n1 - 1) * n1p;
                nxt0 = qpair[inext + kx0];
                nxt1 = qpair[inext + kx1];
                wave_sync();
                const int old = mapL[i];
                const uint32_t qt = qtypeL[i];
                int row0 = 0, row1 = 0, lo = -1, hi = n2;
#pragma unroll 4
                for (int x = 0; x < nm; x++) {
                    const uint32_t ent = listL[x], qd = qdL[x], qc = qcL[x];
                    const int k = (int)(ent & 0xFFu), l = (int)(ent >> 8);
                    lo = k < i ? max(lo, l) : lo;
                    hi = k > i ? min(hi, l) : hi;
                    const int c0 = satk::tri_index(a0, l);
                    row0 += satk::pair_term(qd, qc, __float_as_uint(distL[c0]), codeL[c0]);
                    if (two) {
                        const int c1 = satk::tri_index(a1, l);
                        row1 += satk::pair_term(qd, qc, __float_as_uint(distL[c1]), codeL[c1]);
                    }
                }
                const int from0 = __shfl(row0, old & 63, 64), from1 = __shfl(row1, old & 63, 64);
                const int oldrow = old < 0 ? 0 : (old < 64 ? from0 : from1);
                const bool window0 = !a.lorder || (j0 > lo && j0 < hi), window1 = !a.lorder || (j1 > lo && j1 < hi);
                const bool ok0 = j0 < n2 && t0 == qt && !((occ[0] >> lane) & 1ull) && window0;
                const bool ok1 = two && j1 < n2 && t1 == qt && !((occ[1] >> lane) & 1ull) && window1;
                const unsigned long long ikey = (unsigned long long)(0xFFFFu - (uint32_t)i) << 16;
                const int d0 = row0 - oldrow, d1 = row1 - oldrow, du = -oldrow;
                unsigned long long key = 0ull;
                if (old >= 0 && du > 0) key = ((unsigned long long)(uint32_t)du << 32) | ikey | 0xFFFFull;            // j = -1
                if (ok0 && d0 > 0) {
                    const unsigned long long k0 = ((unsigned long long)(uint32_t)d0 << 32) | ikey | (0xFFFFull - (unsigned)(j0 + 1));
                    key = k0 > key ? k0 : key;
                }
                if (ok1 && d1 > 0) {
                    const unsigned long long k1 = ((unsigned long long)(uint32_t)d1 << 32) | ikey | (0xFFFFull - (unsigned)(j1 + 1));
                    key = k1 > key ? k1 : key;
                }
                best = key > best ? key : best;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long other = __shfl_xor(best, off, 64);
                best = other > best ? other : best;
            }
            if (best == 0ull) {
                done = true;
            } else {
                const int bi = (int)(0xFFFFu - (uint32_t)((best >> 16) & 0xFFFFu));
                const int bj = (int)(0xFFFFu - (uint32_t)(best & 0xFFFFu)) - 1;
                const int old = mapL[bi];
                if (old >= 0) occ[old >> 6] &= ~(1ull << (old & 63));
                if (bj >= 0) occ[bj >> 6] |= 1ull << (bj & 63);
                wave_sync();                               // every lane has read the old image
                if (lane == 0) mapL[bi] = (int8_t)bj;
                wave_sync();
                score += (int)(uint32_t)(best >> 32);
                moves++;
            }
        }
        if (lane == 0) {
            resL[w] = score;
            resL[T + w] = done ? moves : -1;
        }
    }
    __syncthreads();

    // the pair's winner: the largest polished score, ties to the lowest rank
    if (w == 0) {
        int win = -1, bad = sane ? 0 : 1;
        if (sane) {
            win = 0;
            for (int t = 0; t < count; t++) {
                if (resL[T + t] < 0) bad = 1;
                if (resL[t] > resL[win]) win = t;
            }
        }
        const bool ok = !bad;
        if (lane == 0) {
            const int32_t s = ok ? resL[win] : 0;
            a.out[p] = s;
            a.out[(size_t)a.npairs + p] = ok ? a.scores[(size_t)p * T] : 0;
            a.out[2 * (size_t)a.npairs + p] = ok ? a.restarts[(size_t)p * T + win] : -1;
            a.out[3 * (size_t)a.npairs + p] = ok ? resL[T + win] : -1;
            a.okeys[p] = pair_key(s, 0xFFFFFFFFu);
        }
        const int8_t *wm = mapsL + (size_t)(ok ? win : 0) * kListStride;
        for (int i = lane; i < SAT_MAXDIM; i += 64) a.omaps[(size_t)p * SAT_MAXDIM + i] = (ok && i < n1) ? wm[i] : (int8_t)-1;
    }
}

// ---------------------------------------------------------------- polish, lane groups (entries of up to 32 SSEs)
// pair_polish with a map on a GROUP of G lanes instead of a wave: G = 16 serves entries of up to 16 SSEs, G = 32 those
// of up to 32, so a wave64 carries 4 or 2 maps and a workgroup of 256 threads 256 / G groups = (256 / G) / T pairs with
// their T ranks (groups left over idle).  The threads of a pair stage its entry's triangle once for all of its ranks.
// What the groups of a wave share is control flow only: the walk over the query SSEs i runs to the longest query of
// the wave, the matched-list loop to its longest list, the round loop until its last group has no move left; a group
// past its own bound is masked (its list entries add 0, its rows give no key).  Map, occupied set (one 32-bit word),
// matched list, the row's query cells and the move cap are the group's own.  The list compaction takes ceil(n1 / G)
// trips of the group, each a ballot of the wave cut down to the group's bits; the key butterfly stops at the group
// (offsets below G).  Lane x of a group serves the list's x-th and (x + G)-th SSE one row ahead, as pair_polish does;
// a list longer than 2 G (queries above 32 / 64 SSEs) loads the rest inside the row.  Same arithmetic
// (satk::pair_term), same keys (delta, ~i, ~(j + 1)), same sentinels, same outputs as pair_polish; no atomics, no
// 64-bit LDS values.
constexpr uint32_t kGroupBytes = kListStride * 13u;            // a group's list, query distances, query codes, map

template <int G> __host__ __device__ constexpr uint32_t group_slot_bytes()
{
    return (((uint32_t)G * (uint32_t)(G + 1) / 2u + 15u) & ~15u) * 5u + (uint32_t)G + (uint32_t)kListStride;   // (a multiple of 16)
}
template <int G> __host__ __device__ inline uint32_t group_lds_bytes(int T)
{
    const uint32_t ng = 256u / (uint32_t)G;
    return (ng / (uint32_t)T) * group_slot_bytes<G>() + ng * (kGroupBytes + 8u);
}

template <int G>
__global__ void __launch_bounds__(256) pair_polish_group(const PolishArgs a)
{
    static_assert(G == 16 || G == 32, "a group is 16 or 32 lanes");
    constexpr int NG = 256 / G;
    constexpr uint32_t cells = ((uint32_t)G * (uint32_t)(G + 1) / 2u + 15u) & ~15u;
    constexpr uint32_t GMASK = G == 32 ? 0xFFFFFFFFu : 0xFFFFu;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = (int)threadIdx.x, lane = tid & 63, gl = tid & (G - 1), g = tid / G, gbase = lane & ~(G - 1);
    const int T = a.T, PPW = NG / T;
    const int slot = g / T, rank = g - slot * T;
    const int item = (int)blockIdx.x * PPW + slot;
    const bool valid = slot < PPW && item < a.nitems;

    unsigned char *slotL = lds + (size_t)min(slot, PPW - 1) * group_slot_bytes<G>();
    float *distL = reinterpret_cast<float *>(slotL);
    uint8_t *codeL = slotL + (size_t)cells * 4u;
    uint8_t *type2 = codeL + cells;
    uint8_t *qtypeL = type2 + G;
    unsigned char *groupL = lds + (size_t)PPW * group_slot_bytes<G>() + (size_t)g * kGroupBytes;
    uint32_t *listL = reinterpret_cast<uint32_t *>(groupL);
    uint32_t *qdL = listL + kListStride, *qcL = qdL + kListStride;
    int8_t *mapL = reinterpret_cast<int8_t *>(groupL + (size_t)kListStride * 12u);
    int32_t *resL = reinterpret_cast<int32_t *>(lds + (size_t)PPW * group_slot_bytes<G>() + (size_t)NG * kGroupBytes);   // [NG] scores, [NG] moves

    // the pair of this thread's slot (the same for the T * G threads of the slot)
    int p = 0, n1 = 0, n1p = 16, n2 = 1, count = 0;
    const uint2 *qpair = nullptr;
    bool sane = false;
    if (valid) {
        const SatPairItem it = a.items[item];
        p = it.pair;
        const SatQuery Q = a.desc[it.desc];
        const int e = it.entry, qn1 = Q.n1, en2 = a.orders[e];
        count = a.counts[p];
        sane = en2 >= 1 && en2 <= G && en2 <= a.n2max && qn1 >= 1 && qn1 <= SAT_K_MAXDIM && count >= 1 && count <= T;
        if (sane) {
            n1 = qn1;
            n2 = en2;
            n1p = n1 <= 16 ? 16 : (n1 <= 32 ? 32 : (n1 <= 64 ? 64 : 112));
            qpair = Q.qpair;
            const uint8_t *tt = a.tab_tri + a.cell_off[e];
            const float *dd = a.dist_tri + a.cell_off[e];
            const int ncell = (n2 * (n2 + 1)) >> 1, st = rank * G + gl, nst = T * G;
            for (int c = st; c < ncell; c += nst) {
                const float v = dd[c];
                distL[c] = fabsf(v) <= 3.0e38f ? v : SAT_K_DSENT;
                codeL[c] = tt[c];
            }
            for (int j = st; j < n2; j += nst) type2[j] = tt[((j * (j + 1)) >> 1) + j] & 3u;
            for (int i = st; i < n1; i += nst) qtypeL[i] = Q.qtypes[i];
        }
    }
    __syncthreads();

    // From here to the next barrier every lane of a wave runs the same instructions (the shuffles, ballots and wave
    // barriers need all of them); what a lane may do is decided by its group's flags.
    const bool active = sane && rank < count;
    if (!active) n1 = 0;
    {
        const int8_t *src = a.maps + ((size_t)p * T + rank) * SAT_MAXDIM;
        for (int i = gl; i < kListStride; i += G) mapL[i] = (active && i < n1) ? src[i] : (int8_t)-1;
    }
    int n1w = n1;                                          // the longest query of the wave
#pragma unroll
    for (int off = 32; off >= G; off >>= 1) n1w = max(n1w, __shfl_xor(n1w, off, 64));
    n1w = __builtin_amdgcn_readfirstlane(n1w);
    const int trips = (n1w + G - 1) / G;
    wave_sync();
    uint32_t occ = 0u;                                     // occupied db SSEs of the group's map: bit j
    for (int i = 0; i < n1w; i++) {
        const int j = mapL[i];
        if (j >= 0 && j < n2) occ |= 1u << j;
    }
    int score = active ? a.scores[(size_t)p * T + rank] : 0, moves = 0, rounds = 0;
    const int cap = 2 * n1 * (n1 - 1) + 1;
    const int j0 = gl, a0 = min(j0, n2 - 1);               // addressing only: lanes past n2 are masked
    const uint32_t t0 = type2[a0];
    bool done = !active, capped = false;
    while (__builtin_amdgcn_ballot_w64(!done) != 0ull) {
        const bool live = !done;
        // the matched list (k, m[k]) of the group, ascending k
        int nm = 0;
        for (int trip = 0; trip < trips; trip++) {
            const int k = gl + G * trip;
            const int l = min((int)mapL[min(k, kListStride - 1)], n2 - 1);      // (an image is below n2: the clamp guards the cell index)
            const bool on = live && k < n1 && l >= 0;
            const uint32_t mask = (uint32_t)(__builtin_amdgcn_ballot_w64(on) >> gbase) & GMASK;
            const int pos = nm + __popc(mask & ((1u << gl) - 1u));
            if (on) listL[pos] = (uint32_t)k | ((uint32_t)l << 8);
            nm += __popc(mask);
        }
        int nmw = nm;                                      // the longest list of the wave
#pragma unroll
        for (int off = 32; off >= G; off >>= 1) nmw = max(nmw, __shfl_xor(nmw, off, 64));
        nmw = __builtin_amdgcn_readfirstlane(nmw);
        wave_sync();
        // lane x serves the list's x-th and (x + G)-th SSE: their cells of row 0 are on the way
        const bool has0 = gl < nm, has1 = gl + G < nm;
        const int kx0 = has0 ? (int)(listL[gl] & 0xFFu) : 0, kx1 = has1 ? (int)(listL[gl + G] & 0xFFu) : 0;
        uint2 nxt0 = uint2{ 0u, 0u }, nxt1 = uint2{ 0u, 0u };
        if (has0) nxt0 = qpair[kx0];
        if (has1) nxt1 = qpair[kx1];
        unsigned long long best = 0ull;
        for (int i = 0; i < n1w; i++) {
            wave_sync();                                   // the sums of the row before have read its cells
            const int irow = min(i, n1 - 1) * n1p, inext = min(i + 1, n1 - 1) * n1p;
            if (has0) { qdL[gl] = nxt0.x; qcL[gl] = nxt0.y; nxt0 = qpair[inext + kx0]; }
            if (has1) { qdL[gl + G] = nxt1.x; qcL[gl + G] = nxt1.y; nxt1 = qpair[inext + kx1]; }
            for (int x = gl + 2 * G; x < nmw; x += G)      // (a list longer than 2 G: not loaded ahead)
                if (x < nm) {
                    const uint2 c = qpair[irow + (int)(listL[x] & 0xFFu)];
                    qdL[x] = c.x;
                    qcL[x] = c.y;
                }
            wave_sync();
            const bool rowon = live && i < n1;
            const int old = rowon ? (int)mapL[i] : -1;
            const uint32_t qt = qtypeL[i];
            int row0 = 0, lo = -1, hi = n2;
#pragma unroll 4
            for (int x = 0; x < nmw; x++) {
                const bool xin = x < nm;
                const uint32_t ent = listL[x], qd = qdL[x], qc = qcL[x];
                const int k = (int)(ent & 0xFFu), l = xin ? (int)(ent >> 8) : 0;
                lo = (xin && k < i) ? max(lo, l) : lo;
                hi = (xin && k > i) ? min(hi, l) : hi;
                const int c0 = satk::tri_index(a0, l);
                const int term = satk::pair_term(qd, qc, __float_as_uint(distL[c0]), codeL[c0]);
                row0 += xin ? term : 0;
            }
            const int from0 = __shfl(row0, gbase + (old & (G - 1)), 64);
            const int oldrow = old < 0 ? 0 : from0;
            const bool window0 = !a.lorder || (j0 > lo && j0 < hi);
            const bool ok0 = rowon && j0 < n2 && t0 == qt && !((occ >> gl) & 1u) && window0;
            const unsigned long long ikey = (unsigned long long)(0xFFFFu - (uint32_t)i) << 16;
            const int d0 = row0 - oldrow, du = -oldrow;
            unsigned long long key = 0ull;
            if (rowon && old >= 0 && du > 0) key = ((unsigned long long)(uint32_t)du << 32) | ikey | 0xFFFFull;            // j = -1
            if (ok0 && d0 > 0) {
                const unsigned long long k0 = ((unsigned long long)(uint32_t)d0 << 32) | ikey | (0xFFFFull - (unsigned)(j0 + 1));
                key = k0 > key ? k0 : key;
            }
            best = key > best ? key : best;
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            const unsigned long long other = __shfl_xor(best, off, 64);
            best = other > best ? other : best;
        }
        const bool mv = live && best != 0ull;
        const int bi = mv ? (int)(0xFFFFu - (uint32_t)((best >> 16) & 0xFFFFu)) : 0;
        const int bj = (int)(0xFFFFu - (uint32_t)(best & 0xFFFFu)) - 1;
        const int was = mapL[bi];
        wave_sync();                                       // every lane has read the old image
        if (mv && gl == 0) mapL[bi] = (int8_t)bj;
        wave_sync();
        if (mv) {
            if (was >= 0) occ &= ~(1u << was);
            if (bj >= 0) occ |= 1u << bj;
            score += (int)(uint32_t)(best >> 32);
            moves++;
        }
        rounds++;
        if (live && !mv) done = true;
        if (live && mv && rounds >= cap) { done = true; capped = true; }   // (a cap that cannot bind: reported, not spun on)
    }
    if (active && gl == 0) {
        resL[g] = score;
        resL[NG + g] = capped ? -1 : moves;
    }
    __syncthreads();

    // the pair's winner: the largest polished score, ties to the lowest rank (the lanes of the pair's rank-0 group)
    if (valid && rank == 0) {
        int win = 0, bad = sane ? 0 : 1;
        if (sane)
            for (int t = 0; t < count; t++) {
                if (resL[NG + g + t] < 0) bad = 1;
                if (resL[g + t] > resL[g + win]) win = t;
            }
        const bool ok = !bad;
        if (gl == 0) {
            const int32_t s = ok ? resL[g + win] : 0;
            a.out[p] = s;
            a.out[(size_t)a.npairs + p] = ok ? a.scores[(size_t)p * T] : 0;
            a.out[2 * (size_t)a.npairs + p] = ok ? a.restarts[(size_t)p * T + win] : -1;
            a.out[3 * (size_t)a.npairs + p] = ok ? resL[NG + g + win] : -1;
            a.okeys[p] = pair_key(s, 0xFFFFFFFFu);
        }
        const int8_t *wm = reinterpret_cast<const int8_t *>(groupL + (size_t)(ok ? win : 0) * kGroupBytes + (size_t)kListStride * 12u);
        for (int i = gl; i < SAT_MAXDIM; i += G) a.omaps[(size_t)p * SAT_MAXDIM + i] = (ok && i < n1) ? wm[i] : (int8_t)-1;
    }
}

// ---------------------------------------------------------------- whole-database mode: the rows of a launch
// One thread per map item of a launch: the pair's polished score, its base score and (maps) its polished map go where a
// plain search puts the row of (query, entry) - the descriptor's score row, the base buffer at the same offset, the
// query's [N][n1] map block.  A pair whose polish did not finish raises the flag (every writer stores the same 1).
__global__ void __launch_bounds__(256) polish_scatter(const SatPairItem *items, int n, const SatQuery *desc, int npairs,
                                                      const int32_t *out, const int8_t *omaps, const int32_t *scores0,
                                                      int32_t *base0, int maps, int32_t *err)
{
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (x >= n) return;
    const SatPairItem it = items[x];
    const SatQuery Q = desc[it.desc];
    const int p = it.pair, e = it.entry, n1 = Q.n1;
    Q.scores[e] = out[p];
    base0[(Q.scores - scores0) + e] = out[(size_t)npairs + p];
    if (out[3 * (size_t)npairs + p] < 0) *err = 1;
    if (maps && Q.ssemaps) {
        const int8_t *src = omaps + (size_t)p * SAT_MAXDIM;
        int8_t *dst = Q.ssemaps + (size_t)e * (size_t)n1;
        for (int i = 0; i < n1; i++) dst[i] = src[i];
    }
}

}  // namespace

// ---------------------------------------------------------------- launch code (sat_pairs.hpp)

int sat_polish_reserve(sat_ctx *ctx, int npairs)
{
    int rc;
    if ((rc = ctx->d_polout.grow_after(ctx->stream, 4 * (size_t)npairs)) != SAT_OK ||
        (rc = ctx->d_polkeys.grow_after(ctx->stream, (size_t)npairs)) != SAT_OK ||
        (rc = ctx->d_polmaps.grow_after(ctx->stream, (size_t)npairs * SAT_MAXDIM)) != SAT_OK)
        return rc;
    return SAT_OK;
}

// The width the polish of an item group runs at (entries of up to n2max SSEs, in a launch of `launch_pairs` pairs): lane
// groups of 16 or 32 for entries they can hold - always in the whole-database mode (`packed`), in a pair search where the
// launch has maps enough to fill the GPU with packed waves -, else 64, pair_polish's wave per map.
// SAT_EXP_POLISH_GROUP forces a width for the entries it can hold; wider entries fall to the next width.
int sat_polish_width(const sat_ctx *ctx, int launch_pairs, int tops, int n2max, bool packed)
{
    const int fit = n2max <= 16 ? 16 : (n2max <= 32 ? 32 : 64);
    const int forced = ctx->tune.polish_group;
    if (forced == 16 || forced == 32 || forced == 64) return fit > forced ? fit : forced;
    constexpr long long kEnoughMaps = 16384;             // 256 CUs x 16 waves x 4 maps
    return (packed || (long long)launch_pairs * tops >= kEnoughMaps) ? fit : 64;
}

int sat_polish_run(sat_ctx *ctx, int lorder, const SatPairItem *d_map_items, int n, int tops, int n2max, int npairs,
                   const int32_t *counts, const int32_t *scores, const int32_t *restarts, const int8_t *maps, int width)
{
    PolishArgs a{};
    a.items = d_map_items;
    a.desc = ctx->d_qdesc.get();
    a.orders = ctx->d_orders.get();
    a.cell_off = ctx->d_cell_off.get();
    a.tab_tri = ctx->d_tab.get();
    a.dist_tri = ctx->d_dist.get();
    a.counts = counts;
    a.scores = scores;
    a.restarts = restarts;
    a.maps = maps;
    a.T = tops;
    a.lorder = lorder ? 1 : 0;
    a.n2max = n2max;
    a.npairs = npairs;
    a.nitems = n;
    a.out = ctx->d_polout.get();
    a.okeys = ctx->d_polkeys.get();
    a.omaps = ctx->d_polmaps.get();
    if (width == 16) {
        const int ppw = 16 / tops;
        hipLaunchKernelGGL(pair_polish_group<16>, dim3((unsigned)((n + ppw - 1) / ppw)), dim3(256), group_lds_bytes<16>(tops), ctx->stream, a);
    } else if (width == 32) {
        const int ppw = 8 / tops;
        hipLaunchKernelGGL(pair_polish_group<32>, dim3((unsigned)((n + ppw - 1) / ppw)), dim3(256), group_lds_bytes<32>(tops), ctx->stream, a);
    } else {
        hipLaunchKernelGGL(pair_polish, dim3((unsigned)n), dim3(64u * (unsigned)tops), polish_lds_bytes(n2max, tops), ctx->stream, a);
    }
    HIP_TRY(hipGetLastError());
    return SAT_OK;
}

int sat_polish_scatter(sat_ctx *ctx, const SatPairItem *d_map_items, int n, int npairs, bool maps)
{
    hipLaunchKernelGGL(polish_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_map_items, n,
                       (const SatQuery *)ctx->d_qdesc.get(), npairs, (const int32_t *)ctx->d_polout.get(),
                       (const int8_t *)ctx->d_polmaps.get(), (const int32_t *)ctx->d_scores.get(), ctx->d_base.get(), maps ? 1 : 0,
                       ctx->d_polerr.get());
    HIP_TRY(hipGetLastError());
    return SAT_OK;
}

// wait for the polish and copy its rows: 16 * npairs bytes, + SAT_MAXDIM * npairs with maps
int sat_polish_collect(sat_ctx *ctx, int npairs, int32_t *scores, int32_t *base_scores, int32_t *restarts, int32_t *moves,
                       int32_t *ssemaps, const int32_t *query, const int32_t *where)
{
    HIP_TRY(hipSetDevice(ctx->device));
    if (npairs == 0) return SAT_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t P = (size_t)npairs;
    std::vector<int32_t> out(4 * P);
    HIP_TRY(hipMemcpy(out.data(), ctx->d_polout.get(), out.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    ctx->d2h_bytes += out.size() * sizeof(int32_t);
    for (size_t p = 0; p < P; p++)
        if (out[3 * P + p] < 0)
            return sat_fail(SAT_EDEVICE, "pair %zu: the polish did not finish (records and arg-max key disagree, or the move cap was reached)", p);
    int32_t *const dst[4] = { scores, base_scores, restarts, moves };
    for (size_t k = 0; k < 4; k++) {
        if (dst[k] && !where) memcpy(dst[k], out.data() + k * P, P * sizeof(int32_t));
        for (size_t p = 0; dst[k] && where && p < P; p++) dst[k][where[p]] = out[k * P + p];
    }
    return ssemaps ? sat_collect_maps(ctx, ctx->d_polmaps.get(), P, 1, query, nullptr, where, ssemaps) : SAT_OK;
}

extern "C" int sat_search_pairs_polish(sat_ctx *ctx, int lorder, int maxstart, int tops, int npairs, const int32_t *query,
                                       const int32_t *entry, int32_t *scores, int32_t *base_scores, int32_t *restarts,
                                       int32_t *moves, int32_t *ssemaps, double *kernel_ms)
{
    if (!ctx) return sat_fail(SAT_EINVAL, "null context");
    if (npairs > 0 && !scores) return sat_fail(SAT_EINVAL, "scores buffer is null");
    const int rc = timed(ctx, kernel_ms, [&] {
        return sat_pair_matches_launch(ctx, lorder, maxstart, tops, true, query, entry, npairs, PairMode::Polish);
    });
    if (rc != SAT_OK) return rc;
    return sat_polish_collect(ctx, npairs, scores, base_scores, restarts, moves, ssemaps, query);
}
