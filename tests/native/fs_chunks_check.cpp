// fs_chunks_check.cpp - the flat pair walk of the initial full score (sat_sa_body.inc: FS_FLAT) run on the host, lane by
// lane, with the kernel's own chunk functions (the SAT_FS_CHUNKS_ONLY section of csrc/sat_sa_kernel.hpp: fs_pairs,
// fs_chunk, fs_chunk_pairs, fs_seek, fs_advance); what the kernel does with wave instructions (the compaction, the scan,
// the search over it, the fetch of another lane's sets) is restated here step by step.  Checks that every pair (chain, a, b) of a wave is visited exactly
// once, in order, by the lane the deal gives it to, with the right images, and that no visit addresses a sum slot
// past the owners.  Built with -fsanitize=address,undefined by tests/test_fs_chunks.py; prints one line, exits 0 / 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#define SAT_FS_CHUNKS_ONLY
#include "sat_sa_kernel.hpp"

using namespace satk;

struct Visit { int chain, i, ji, k, l, lane; };

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
// a set of m distinct positions below 32
static uint32_t random_set(int m)
{
    uint32_t s = 0;
    while (__builtin_popcount(s) < m) s |= 1u << (rnd() & 31u);
    return s;
}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 10) { printf("FAIL %s: ", name); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void run_wave(const char *name, const int *ms)
{
    uint32_t mapped[64], occ[64];
    for (int c = 0; c < 64; c++) { mapped[c] = random_set(ms[c]); occ[c] = random_set(ms[c]); }
    // what is expected: chain by chain, row by row
    std::vector<Visit> want;
    for (int c = 0; c < 64; c++) {
        int iv[32], jv[32], m = 0;
        for (int b = 0; b < 32; b++) if (mapped[c] >> b & 1u) iv[m++] = b;
        m = 0;
        for (int b = 0; b < 32; b++) if (occ[c] >> b & 1u) jv[m++] = b;
        for (int a = 0; a < m; a++)
            for (int b = a + 1; b < m; b++) want.push_back(Visit{ c, iv[a], jv[a], iv[b], jv[b], 0 });
    }
    // compaction: owners to 0 .. NZ - 1 in lane order; what a lane at or past NZ holds
    uint32_t cm[64], co[64];
    int chain_of[64], NZ = 0;
    for (int c = 0; c < 64; c++)
        if ((mapped[c] & (mapped[c] - 1u)) != 0u) { cm[NZ] = mapped[c]; co[NZ] = occ[c]; chain_of[NZ++] = c; }
    for (int r = NZ; r < 64; r++) { cm[r] = co[r] = SAT_FS_DUMMY_SET; chain_of[r] = -1; }
    int S[64], P = 0;                                  // exclusive scan
    for (int r = 0; r < 64; r++) { S[r] = P; P += r < NZ ? fs_pairs(cm[r]) : 0; }
    CHECK(P == (int)want.size(), "P = %d, %d pairs expected", P, (int)want.size());
    const int q = fs_chunk(P);
    CHECK(q * 64 >= P && (q - 1) * 64 < P, "q = %d for P = %d", q, P);
    std::vector<Visit> got;
    for (int t = 0; t < 64; t++) {
        const int first = t * q, mine = fs_chunk_pairs(P, q, t);
        int r = 0;
        for (int d = 32; d > 0; d >>= 1) r = S[r + d] <= first ? r + d : r;
        FsCursor cur = fs_seek(cm[r], co[r], mine > 0 ? first - S[r] : 0);
        for (int it = 0; it < ((q + 1) & ~1); it++) {           // two pairs per trip
            const bool valid = it < mine;
            CHECK(cur.rm != 0u && cur.ro != 0u && cur.rk != 0u && cur.rl != 0u, "lane %d trip %d stands on an empty set", t, it);
            if (failures) return;
            if (valid) {
                CHECK(r < NZ, "lane %d adds to slot %d of %d owners", t, r, NZ);
                got.push_back(Visit{ chain_of[r & 63], __builtin_ctz(cur.rm), __builtin_ctz(cur.ro), __builtin_ctz(cur.rk), __builtin_ctz(cur.rl), t });
            }
            r += fs_advance(cur, valid ? 1u : 0u, cm[(r + 1) & 63], co[(r + 1) & 63]) ? 1 : 0;
        }
    }
    CHECK(got.size() == want.size(), "%d pairs visited, %d expected", (int)got.size(), (int)want.size());
    // lanes take ascending chunks, so the visits come out in the wave's order: equal lists = every pair exactly once
    for (size_t g = 0; g < got.size() && g < want.size(); g++) {
        const Visit &a = got[g], &b = want[g];
        CHECK(a.chain == b.chain && a.i == b.i && a.ji == b.ji && a.k == b.k && a.l == b.l,
              "pair %d is (chain %d, %d -> %d, %d -> %d), expected (chain %d, %d -> %d, %d -> %d)", (int)g, a.chain, a.i, a.ji, a.k,
              a.l, b.chain, b.i, b.ji, b.k, b.l);
        CHECK(a.lane == (int)g / q, "pair %d visited by lane %d, dealt to lane %d", (int)g, a.lane, (int)g / q);
    }
}

int main()
{
    int ms[64], waves = 0;
    auto fill = [&](int v) { for (int c = 0; c < 64; c++) ms[c] = v; };
    fill(0); run_wave("all zeros", ms); waves++;
    fill(1); run_wave("all ones", ms); waves++;
    for (int c = 0; c < 64; c += 21) { fill(0); ms[c] = 2; run_wave("one chain, m = 2", ms); waves++; }
    fill(1); ms[63] = 2; run_wave("one chain, m = 2, last lane", ms); waves++;
    fill(2); ms[17] = 1; run_wave("P = 63", ms); waves++;
    fill(2); run_wave("P = 64", ms); waves++;
    fill(2); ms[40] = 1; ms[5] = 3; run_wave("P = 65", ms); waves++;
    for (int c = 0; c < 64; c += 9) { fill(c & 1); ms[c] = 16; run_wave("one chain holds every pair", ms); waves++; }
    fill(16); run_wave("m = 16 everywhere", ms); waves++;
    fill(32); run_wave("m = 32 everywhere", ms); waves++;
    // matched SSEs per chain on the bench inputs (profiles/r06_logs/fs_walk_model.txt: chains by m = 0 .. 19), capped at 16
    static const int hist[17] = { 34, 197, 512, 746, 523, 344, 201, 244, 326, 500, 568, 570, 466, 365, 279, 144, 125 };
    int total = 0;
    for (int m = 0; m < 17; m++) total += hist[m];
    for (int v = 0; v < 2000; v++) {
        for (int c = 0; c < 64; c++) {
            int x = (int)(rnd() % (uint32_t)total), m = 0;
            while (x >= hist[m]) x -= hist[m++];
            ms[c] = m;
        }
        // every tenth wave sparse, as beside short entries: most chains own nothing
        if (v % 10 == 9) for (int c = 0; c < 64; c++) if (rnd() % 4u) ms[c] = (int)(rnd() % 2u);
        run_wave("random", ms);
        waves++;
    }
    printf("%s: %d waves, %d failures\n", failures ? "FAILED" : "ok", waves, failures);
    return failures ? 1 : 0;
}
