// sat_sa_body.inc - the body of the SA kernel (sat_sa_kernel.hpp), included by its four kernels: the plain one
// (sat_sa_kernel: MATCH = PAIRS = false, the option-specialised and general instantiations), the match mode's
// (sat_sa_match_kernel: MATCH = true, options from the arguments), the pair mode's (sat_sa_pair_kernel:
// PAIRS = true) and the pair-match mode's (sat_sa_pair_match_kernel: both).  Kept as ONE text inside each kernel rather
// than a device function the kernels call: an inlined callee reads the kernel arguments through a reference and
// came out as different code for the plain kernels.  Not a header: it expects the kernel's own scope (template
// parameters N1P, M2W, QLDS, OPT, WPL, CELLS, the arguments `a`, `mx` and `px`, MATCH and PAIRS).
    using namespace satk;
    constexpr int M1W = (N1P + 31) / 32;
    extern __shared__ __align__(16) unsigned char lds_raw[];

    // entry slot of this wave (wave-uniform: tpe is a multiple of 64) and the lane inside it
    const int nthreads = a.tpe;
    const int wave_wg = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int slot = a.epw > 1 ? wave_wg / (nthreads >> 6) : 0;
    const int wlane = (int)(threadIdx.x & 63u);
    const int lane_id = ((wave_wg - slot * (nthreads >> 6)) << 6) | wlane;
    __builtin_assume(lane_id >= 0 && lane_id < 1024);
    const uint32_t lds_base = (uint32_t)slot * a.lds_stride;
    unsigned char *const lds_slot = lds_raw + lds_base;
    // chain = restart slot of this lane; `part` of `lpc` adjacent lanes share one chain
    constexpr bool FAST = OPT >= 0;
    const int lpc_shift = FAST ? (OPT >> 2) : a.lpc_shift;      // OPT bits 2-3: log2(lanes per chain), 0..2
    const bool opt_lorder = FAST ? (OPT & 1) != 0 : a.lorder != 0;
    const bool opt_compact = FAST ? (OPT & 1) != 0 : a.compact != 0;
    const int lpc = 1 << lpc_shift;
    const int tid = lane_id >> lpc_shift;         // chain index inside the workgroup
    const int part = lane_id & (lpc - 1);
    const int T = nthreads >> lpc_shift;          // chains per workgroup
    // the last workgroup's spare slots repeat the last entry (same result, written twice).  Pair mode: the slot's
    // work item names the query (a descriptor of the launch's class), the entry and the restarts; spare slots
    // repeat the last item (the same key folded in twice)
    const int list_pos = (int)blockIdx.x * a.epw + slot;
    SatPairItem pit{};
    if constexpr (PAIRS) pit = px.items[min(list_pos, a.n_list - 1)];
    const int e = PAIRS ? pit.entry : a.entry_list[min(list_pos, a.n_list - 1)];
    const SatQuery Q = PAIRS ? a.queries[pit.desc] : a.queries[blockIdx.y];
    const int n1 = Q.n1;
    const int n2 = a.orders[e];
    const int n2p = n2 + 1;
    const int n1w = (n1 + 3) >> 2;
    const int NULLJ = n2;                       // the null db SSE
    // (the match mode captures maps only in its replay pass, without the leader gate)
    const bool lsoln = MATCH ? false : (FAST ? (OPT & 2) != 0 : a.lsoln != 0);
    const bool replay = MATCH && mx.replay != 0;

    int cmp_lpi_q, cmp_wpl_q;
    compaction_shape(n1w, cmp_lpi_q, cmp_wpl_q);
    // lanes per listed row = ceil(n1w / 4): a compile-time fact in the two small query classes (1 for up to
    // 16 SSEs, 2 for 17..32), which turns the word strides of the rounds into instruction offsets
    constexpr int LPI_CT = N1P == 16 ? 1 : (N1P == 32 ? 2 : 0);
    const int cmp_lpi = LPI_CT ? LPI_CT : cmp_lpi_q;
    const int cmp_wpl = WPL > 0 ? WPL : cmp_wpl_q;           // the host launches WPL > 0 only where it matches
    const int cmp_words = cmp_lpi * cmp_wpl;                 // words n1w .. cmp_words - 1 stay "unmatched"
    // ---- carve LDS: satk::lds_layout, the function the host sizes the workgroup with.  The cell layout
    // goes by the launch's size class, not by this entry's order (n2max > 32 <=> M2W > 1).
    constexpr bool SPLIT = CELLS != SAT_CELLS_FULL8;
    // chain-map bytes as cell byte offsets with an "unmatched" flag (sat_sa_kernel.hpp: map_bytes_scaled); quad_terms
    // goes by the cell layout alone, and the 8-byte cells are launched with one-word sets only
    constexpr bool MAPOFF = map_bytes_scaled(M2W, CELLS);
    static_assert(MAPOFF == (CELLS == SAT_CELLS_FULL8), "8-byte cells go with one-word db sets");
    const LdsLayout lay = lds_layout(M2W, CELLS, n2, cmp_words, N1P, T, nthreads, QLDS, opt_compact);
    uint2 *Dc = reinterpret_cast<uint2 *>(lds_slot);                          // !SPLIT: 8-byte cells
    float *distL = reinterpret_cast<float *>(lds_slot);                       // SPLIT: distances ...
    uint8_t *codeL = lds_slot + lay.code;                                     // ... and code bytes
    auto db_row = [&](int j) -> DbRow<CELLS> {
        if constexpr (CELLS == SAT_CELLS_TRI5) return DbRow<SAT_CELLS_TRI5>{ distL, codeL, j };
        else if constexpr (CELLS == SAT_CELLS_FULL5) return DbRow<SAT_CELLS_FULL5>{ distL + __mul24(j, n2p), codeL + __mul24(j, n2p) };
        else return DbRow<SAT_CELLS_FULL8>{ Dc + __mul24(j, n2p) };
    };
    // query groups in LDS cover the padding words too (sentinel cells, like every group past n1w)
    float4 *qdistL = reinterpret_cast<float4 *>(lds_slot + lay.qdist);
    uint32_t *qcodeL = reinterpret_cast<uint32_t *>(lds_slot + lay.qcode);
    uint32_t *smap = reinterpret_cast<uint32_t *>(lds_slot + lay.smap);
    // map word w of chain c lives at w*TP + c with TP = T + 1: the odd stride puts the words of
    // one chain in different banks (the compacted loop reads them from several lanes at once) and
    // keeps word w of all chains contiguous for the static loops
    const int TP = T + 1;
    uint32_t *tmask = reinterpret_cast<uint32_t *>(lds_slot + lay.tmask);
    // best maps: word w of chain c at w*T + c of this workgroup's slab (global memory)
    uint32_t *bmap = (lsoln || replay) ? a.bmap_slabs + ((size_t)blockIdx.y * gridDim.x * a.epw + list_pos) * a.bmap_slab_words : nullptr;
    uint8_t *qtypes = lds_slot + lay.qtypes;
    // M2W == 1: the candidate mask of query SSE i by ONE LDS read (tmask[qtypes[i]] is two, one after the other,
    // on the path of every SA step)
    uint32_t *qmask = reinterpret_cast<uint32_t *>(lds_slot + lay.qmask);
    // ... and the rank table of the LORDER step's pick: the entry's SSEs sorted by (type, index), and per query SSE
    // where its type's run starts (read next to qmask, so the table read is the only dependent one)
    uint8_t *qbase = lds_slot + lay.qbase;
    uint8_t *pos = lds_slot + lay.pos;
    constexpr bool PICK_TABLE = SAT_PICK_TABLE && M2W == 1;
    unsigned char *red_b = lds_slot + lay.red;
    auto red_key = [&](int w) -> unsigned long long * { return reinterpret_cast<unsigned long long *>(red_b + (uint32_t)w * lay.red_stride); };
    constexpr int TMS = M2W;                                  // words per type of the type masks
    // explicit LDS address space: these two are written by some lanes and read by others of the
    // same wave between wavefront-scope fences, and must stay ds_* instructions
    typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
    typedef __attribute__((address_space(3))) int32_t lds_i32_t;
    const uint32_t items_off = lds_base + lay.items;
    // LSOLN: key (score, restart) of the best proposal any chain of the workgroup has recorded so
    // far, same form as the final arg-max key.  A chain copies its map out only when its new best
    // beats this leader: the map that is finally output belongs to the chain with the largest key,
    // and that chain's last own-best proposal always beats every key recorded before it (a stale,
    // lower leader only causes a spare copy).  ~1150 copies per workgroup become ~20.
    typedef __attribute__((address_space(3))) unsigned long long lds_u64_t;
    lds_u64_t *leader = (lds_u64_t *)(uintptr_t)(lds_base + lay.leader);
    auto beats_leader = [&](int sc, int restart_) -> bool {
        const unsigned long long key = (((unsigned long long)(uint32_t)(sc + 0x40000000)) << 32) | (0xFFFFFFFFu - (uint32_t)restart_);
        if (key <= *leader) return false;
        __hip_atomic_fetch_max(leader, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return true;
    };
    lds_u32_t *items = (lds_u32_t *)(uintptr_t)(uint32_t)(items_off + (uint32_t)(lane_id >> 6) * 256u);
    // query group (4 distances, 4 code bytes) of column `col`: from LDS, or from global memory
    // through L1 - the descriptor's pointers are cast to the global address space so that the
    // loads are global_load (a pointer read from memory is otherwise a generic "flat" pointer)
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) f32x4_t *gptr_f4;
    typedef const __attribute__((address_space(1))) uint32_t *gptr_u32;
    const gptr_f4 qdistG = (gptr_f4)(uintptr_t)Q.qdist;
    const gptr_u32 qcodeG = (gptr_u32)(uintptr_t)Q.qcode;
    typedef const __attribute__((address_space(1))) char *gptr_c;
    typedef const __attribute__((address_space(4))) int32_t *cptr_i32;
    const cptr_i32 prowC = (cptr_i32)(uintptr_t)a.prow;
    typedef const __attribute__((address_space(1))) float *gptr_f32;
    const gptr_f32 ptabG = (gptr_f32)(uintptr_t)a.ptab;
    // uniform 64-bit base + 32-bit byte offset: the saddr form of global_load, no 64-bit VALU math
    // (byte offsets: off16 = 16 * group index, off4 = 4 * group index.  The callers build them from a
    // per-lane base plus constants, so that the words of a round differ by instruction offsets only.)
    auto load_qdist = [&](uint32_t off16) -> float4 {
        if constexpr (QLDS) return *reinterpret_cast<const float4 *>(reinterpret_cast<const unsigned char *>(qdistL) + off16);
        else {
            const f32x4_t v = *(gptr_f4)((gptr_c)qdistG + off16);
            return float4{ v.x, v.y, v.z, v.w };
        }
    };
    auto load_qcode = [&](uint32_t off4) -> uint32_t {
        if constexpr (QLDS) return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const unsigned char *>(qcodeL) + off4);
        else return *(gptr_u32)((gptr_c)qcodeG + off4);
    };
    // the same cells for a wave-uniform index (the full score walks the query in step for all
    // chains): through the constant address space these are scalar loads into scalar registers
    typedef const __attribute__((address_space(4))) f32x4_t *cptr_f4;
    typedef const __attribute__((address_space(4))) uint32_t *cptr_u32;
    const cptr_f4 qdistC = (cptr_f4)(uintptr_t)Q.qdist;
    const cptr_u32 qcodeC = (cptr_u32)(uintptr_t)Q.qcode;
    auto load_qdist_uniform = [&](uint32_t idx) -> float4 {
        if constexpr (QLDS) return qdistL[idx];
        else {
            const f32x4_t v = qdistC[idx];
            return float4{ v.x, v.y, v.z, v.w };
        }
    };
    auto load_qcode_uniform = [&](uint32_t idx) -> uint32_t {
        if constexpr (QLDS) return qcodeL[idx];
        else return qcodeC[idx];
    };

    SAT_PHASE_INIT;
    // ---- stage the db entry: packed lower triangle (HBM) -> full cell matrix (LDS).  Row r of the triangle (r + 1
    // cells) and row n2 - 1 - r (n2 - r cells) are n2 + 1 cells together: the waves take such row pairs in turn
    // and the lanes the n2 + 1 positions, so consecutive lanes read consecutive triangle cells, every triangle cell
    // is read ONCE and written to both mirror positions, and no lane divides (the first version walked the
    // n2 (n2 + 1) cells of the full matrix: a division, and a gather of the mirrored triangle cell, per cell).
    // Launches with the triangle layout (DbRow) keep the triangle as it is: a straight copy.
    {
        const uint8_t *tt = a.tab_tri + a.cell_off[e];
        const float *dd = a.dist_tri + a.cell_off[e];
        // NaN / inf never pass the reference's |d1 - d2| <= 4 either: same as the sentinel
        auto clean = [](float v) -> uint32_t { return __float_as_uint(fabsf(v) <= 3.0e38f ? v : SAT_K_DSENT); };
        auto put = [&](int c, uint32_t dist_bits, uint32_t code) {
            if constexpr (SPLIT) {
                distL[c] = __uint_as_float(dist_bits);
                codeL[c] = (uint8_t)code;
            } else {
                Dc[c] = uint2{ dist_bits, code };
            }
        };
        if constexpr (CELLS == SAT_CELLS_TRI5) {
            // the triangle as it lies in HBM, then the null row: n2 + 1 cells that never pass the distance test
            // (four cells per lane and trip: the entry's first cell sits at any cell index, so the 16 bytes of
            // distances are only dword aligned and the 4 code bytes not at all - global memory takes both; their
            // LDS images start 16-byte aligned)
            const int ncell = (n2 * n2p) >> 1;
            typedef float f32x4u_t __attribute__((ext_vector_type(4), aligned(4)));
            typedef uint32_t u32u_t __attribute__((aligned(1)));
            for (int t = lane_id << 2; t + 3 < ncell; t += nthreads << 2) {
                const f32x4u_t v = *reinterpret_cast<const f32x4u_t *>(dd + t);
                const uint32_t c4 = *reinterpret_cast<const u32u_t *>(tt + t);
                *reinterpret_cast<uint4 *>(distL + t) = uint4{ clean(v.x), clean(v.y), clean(v.z), clean(v.w) };
                *reinterpret_cast<uint32_t *>(codeL + t) = c4;
            }
            for (int t = (ncell & ~3) + lane_id; t < ncell; t += nthreads) put(t, clean(dd[t]), tt[t]);
            for (int x = lane_id; x <= n2; x += nthreads) put(ncell + x, __float_as_uint(SAT_K_DSENT), 0u);
        } else {
            const int swave = lane_id >> 6, swaves = nthreads >> 6;
            const int pairs = (n2 + 1) >> 1;               // an odd order's middle row pairs with itself: taken once
            for (int r = swave; r < pairs; r += swaves) {
                const int rb = n2 - 1 - r;
                for (int x = wlane; x <= n2; x += 64) {
                    const bool first = x <= r;
                    if (!first && rb == r) continue;
                    const int hi = first ? r : rb, lo = first ? x : x - r - 1;
                    const int t = ((hi * (hi + 1)) >> 1) + lo;
                    const uint32_t dist_bits = clean(dd[t]), code = tt[t];
                    put(__mul24(hi, n2p) + lo, dist_bits, code);
                    if (lo != hi) put(__mul24(lo, n2p) + hi, dist_bits, code);
                }
            }
            // the null SSE's column: never passes the distance test
            for (int j = lane_id; j < n2; j += nthreads) put(__mul24(j, n2p) + n2, __float_as_uint(SAT_K_DSENT), 0u);
        }
        if (lane_id < 4 * TMS) tmask[lane_id] = 0u;
        if (lane_id == 0) *reinterpret_cast<unsigned long long *>(lds_slot + lay.leader) = 0ull;   // LSOLN leader key
        for (int i = lane_id; i < N1P; i += nthreads) qtypes[i] = Q.qtypes[i];
        if (QLDS) {
            const int groups = cmp_words * N1P;
            for (int c = lane_id; c < groups; c += nthreads) {
                qdistL[c] = Q.qdist[c];
                qcodeL[c] = Q.qcode[c];
            }
        }
    }
    __syncthreads();
    for (int j = lane_id; j < n2; j += nthreads) {
        int t = a.tab_tri[a.cell_off[e] + (int64_t)j * (j + 1) / 2 + j] & 3;   // diagonal = SSE type
        atomicOr(&tmask[t * TMS + (j >> 5)], 1u << (j & 31));
    }
    __syncthreads();
    if constexpr (M2W == 1) {
        // db SSEs of the types below each type: where a type's run starts in `pos`
        const uint32_t tm0 = tmask[0], tm1 = tmask[1], tm2 = tmask[2], tm3 = tmask[3];
        const int b1 = __popc(tm0), b2 = b1 + __popc(tm1), b3 = b2 + __popc(tm2);
        for (int i = lane_id; i < N1P; i += nthreads) {
            const int t = qtypes[i] & 3;
            qmask[i] = t == 0 ? tm0 : (t == 1 ? tm1 : (t == 2 ? tm2 : tm3));
            qbase[i] = (uint8_t)(t == 0 ? 0 : (t == 1 ? b1 : (t == 2 ? b2 : b3)));
        }
        // db SSE j goes to its rank among the SSEs of its type, behind the types below; the bytes past the last
        // SSE are read (and dropped) by steps without a candidate.  (A slot has at least 64 lanes.)
        if (lane_id < (int)SAT_POS_BYTES) {
            const int j = lane_id;
            const uint32_t bit = j < n2 ? 1u << j : 0u, below = bit - 1u;
            int rank = j;
            if (tm0 & bit) rank = __popc(tm0 & below);
            if (tm1 & bit) rank = b1 + __popc(tm1 & below);
            if (tm2 & bit) rank = b2 + __popc(tm2 & below);
            if (tm3 & bit) rank = b3 + __popc(tm3 & below);
            pos[rank] = (uint8_t)j;
        }
        __syncthreads();
    }

    uint8_t *smap_b = reinterpret_cast<uint8_t *>(smap);
    uint8_t *bmap_b = reinterpret_cast<uint8_t *>(bmap);
    auto bmap_byte_addr = [&](int k) -> int { return (__mul24(k >> 2, T) + tid) * 4 + (k & 3); };
    // byte k of this lane's map lives at ((k>>2)*T + tid)*4 + (k&3)
    const int T4 = TP << 2, tid4 = tid << 2;
    auto map_byte_addr = [&](int k) -> int { return __mul24(k >> 2, T4) + tid4 + (k & 3); };

    // Full score of this lane's chain in the rows-in-step form (tmscord, K.cu:396-440): every lane walks all n1 rows of
    // its chain, the wave reads the query cells with scalar loads; lanes that share a chain split the words and
    // the caller adds their sums.
    auto score_rows = [&]() -> int {
        int total = 0;
        for (int i = 0; i < n1 - 1; i++) {
            // an unmatched SSE has no row in LDS: its lane walks row 0 and drops the sum (scaled bytes: the flag
            // byte 0x04 decodes to row 0 by the shift alone)
            const uint32_t jb = smap_b[map_byte_addr(i)];
            const int j = MAPOFF ? (int)(jb >> 3) : (int)jb;
            const bool jreal = MAPOFF ? (jb & SAT_MAP_UNMATCHED) == 0u : j != NULLJ;
            const DbRow<CELLS> drow = db_row(jreal ? j : 0);
            int rowsum = 0;
            auto row_group = [&](int kw) {
                // pairs with k <= i inside the first word are switched off (mask from i and kw)
                const int below = i + 1 - 4 * kw;
                const uint32_t force = below <= 0 ? 0u : (0x04040404u >> (8 * (4 - below)));
                const uint32_t qi = (uint32_t)(kw * N1P + i);
                rowsum = quad_terms(load_qdist(qi << 4), load_qcode(qi << 2), drow, smap[kw * TP + tid], force, rowsum);
            };
            // one lane per chain: the group index stays in scalar registers, and so do the query cells
            if (lpc == 1) {
                for (int kw = (i + 1) >> 2; kw < n1w; kw++) {
                    const int below = i + 1 - 4 * kw;
                    const uint32_t force = below <= 0 ? 0u : (0x04040404u >> (8 * (4 - below)));
                    const uint32_t qi = (uint32_t)(kw * N1P + i);
                    rowsum = quad_terms(load_qdist_uniform(qi), load_qcode_uniform(qi), drow, smap[kw * TP + tid], force, rowsum);
                }
            } else {
                for (int kw = ((i + 1) >> 2) + part; kw < n1w; kw += lpc) row_group(kw);
            }
            total += jreal ? rowsum : 0;
        }
        return total;
    };

    const uint64_t subseq_lo = (uint64_t)a.ordinal[e];
    int best = SAT_K_NO_SCORE;
    uint32_t best_restart = 0xFFFFFFFFu;
    bool any = false;

    // ---- work compaction constants (see the SA step).  A listed row is served by cmp_lpi lanes,
    // each taking cmp_wpl <= 4 map words: the loads of a lane's words are in flight together and a
    // round holds 64 / cmp_lpi rows, so a typical step is one or two rounds.  lane / cmp_lpi by a
    // 16-bit reciprocal (exact for lane <= 64); lane -> (item of the round, first map word).
    const int cmp_recip = (65536 + cmp_lpi - 1) / cmp_lpi;
    const int per_round = (64 * cmp_recip) >> 16;
    const int sub = __mul24(wlane, cmp_recip) >> 16, kw = wlane - __mul24(sub, cmp_lpi);
    const bool lane_ok = sub < per_round;
    // tail shapes: one word per lane (n1w lanes per row) and two words per lane, used for the last
    // rows of a step when they fit one round of that shape; the two-word shape only if its padded
    // word count stays inside the map's
    const int tail1_recip = (65536 + n1w - 1) / n1w, tail1_rows = (64 * tail1_recip) >> 16;
    const int tail2_lpi = (n1w + 1) >> 1;
    const int tail2_recip = (65536 + tail2_lpi - 1) / tail2_lpi;
    const int tail2_rows = 2 * tail2_lpi <= cmp_words ? (64 * tail2_recip) >> 16 : 0;
    const uint32_t nullword = map_encode<MAPOFF>(NULLJ, NULLJ) * 0x01010101u;     // a map word of unmatched SSEs
    SAT_PHASE(7);                         // staging (and, in the restart loop, its own overhead)
    SAT_DIAG_PERTURB_INIT;
    // match mode: the output row of (query, entry), this slot's record slab, the restarts this chain runs (the
    // replay pass: the tid-th picked restart of the entry, once) and the own best of the current restart
    size_t mrow = 0;
    uint32_t *mrec = nullptr;
    int r_begin = tid, r_end = a.maxstart;
    if constexpr (PAIRS) {
        r_begin = pit.r0 + tid;
        r_end = pit.r1;
    }
    int rbest = SAT_K_NO_SCORE;
    Bits<M2W> rset = bits_zero<M2W>();
    if constexpr (MATCH) {
        if constexpr (PAIRS) {
            // pair-match mode: the outputs' row is the pair, the records go to the pair's slab (the items of one pair
            // run in several workgroups); the record pass keeps the item's restarts [r0, r1) set above
            mrow = (size_t)pit.pair;
            mrec = mx.rec_slabs + (size_t)pit.slab * mx.rec_slab_words;
        } else {
            mrow = (size_t)(&a.queries[blockIdx.y] - mx.desc_base) * (size_t)mx.n_entries + (size_t)e;
            mrec = mx.rec_slabs + ((size_t)blockIdx.y * gridDim.x * a.epw + list_pos) * mx.rec_slab_words;
        }
        if (replay) {
            const int cnt = mx.counts[mrow];
            r_begin = tid < cnt ? mx.restarts[mrow * mx.max_matches + tid] : 0;
            r_end = tid < cnt ? r_begin + 1 : 0;
        }
    }
    for (int restart = r_begin; restart < r_end; restart += T) {
        any = true;
        SAT_PHASE(7);
        const uint64_t subseq = subseq_lo | ((uint64_t)(uint32_t)restart << 32);

        // ---- random initial map (thinit, K.cu:588-648): order preserving, types respected
        Bits<M1W> mapped = bits_zero<M1W>();
        Bits<M2W> occ = bits_zero<M2W>();
        {
            {
                // (the word addresses are formed again every restart: kept, they are loop invariants that sit in
                // registers through the step loop - one of them ended up in scratch)
                int wa = tid;
                asm volatile("" : "+v"(wa));
                for (int w = 0; w < cmp_words; w++, wa += TP) smap[wa] = nullword;
            }
            int j = 0;
            bool stopped = false;
            for (int i0 = 0; i0 < n1; i0 += 4) {
                // a chain whose type search failed draws no more (K.cu:633-638): once that holds for every lane of
                // the wave the rest of the query is skipped - for long queries against short entries (the scan
                // position runs off the entry after ~2 n2 query SSEs) that is most of the loop and of its Philox blocks
                if constexpr (N1P > 32)
                    if (__builtin_amdgcn_ballot_w64(!stopped) == 0ull) break;
                uint4 r = philox_block(Q.seed_q, subseq, (uint32_t)(i0 >> 2));
                uint32_t rv[4] = { r.x, r.y, r.z, r.w };
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    const int i = i0 + s;
                    if (i < n1) {
                        // u < 0.5 for u = 2^-32 + float(v) * 2^-32 (K.cu:625): float(v) < 2^31, i.e. v below the
                        // first value that rounds up to 2^31 (24-bit mantissa, ties to even)
                        if (!stopped && rv[s] < 0x7FFFFFC0u) {
                            Bits<M2W> cand, below = bits_below<M2W>(j);
                            if constexpr (M2W == 1) {
                                cand.w[0] = qmask[i] & ~below.w[0];
                            } else {
                                const int t = qtypes[i];
#pragma unroll
                                for (int w = 0; w < M2W; w++) cand.w[w] = tmask[t * TMS + w] & ~below.w[w];
                            }
                            int jj = bits_lowest<M2W>(cand);
                            if (jj < 0) {
                                stopped = true;              // K.cu:633-638: give up, no more draws used
                            } else {
                                smap_b[map_byte_addr(i)] = (uint8_t)(MAPOFF ? jj << 3 : jj);
                                bits_set<M1W>(mapped, i);
                                bits_set<M2W>(occ, jj);
                                j = jj + 1;
                            }
                        }
                    }
                }
            }
        }

        SAT_PHASE(10);                    // thinit
        // ---- full score of the initial map (tmscord, K.cu:396-440): pairs i < k, both matched
        int score = 0;
        constexpr bool FS_PAIRS = N1P > 16 && !SAT_DIAG_FS_ROWS_ONLY;
        // The pair walk below costs the wave what its busiest lane costs, m (m - 1) / 2 single pairs for m matched
        // SSEs (~27 instructions each), the rows-in-step form n1w * n1 / 2 packed evaluations (~31 each) whatever
        // the maps hold: a wave whose densest initial map would make the walk the dearer of the two takes the rows
        // (all-hit databases, where thinit matches 16+ of 32 SSEs: 5.7 -> 6.6 M scorings/s on scripts/exp/
        // dense_hits.py, its all-miss leg 7.6 -> 8.3 M).  With sets of several words a pop costs more, but pricing
        // the pair at 60 there sent the 101-SSE-query launches to the rows too early (-4 %): one price for all.
        bool walk_pairs = FS_PAIRS;
        if constexpr (FS_PAIRS) {
            constexpr int PAIR_COST = 27;
            const int m = bits_count<M1W>(mapped);
            walk_pairs = __builtin_amdgcn_ballot_w64(__mul24(__mul24(m, m - 1), PAIR_COST) > __mul24(__mul24(n1w, n1), 31)) == 0ull;
        }
        if (walk_pairs) {
            // Every lane walks the matched pairs of ITS chain (set bits of `mapped`: i ascending, k above i)
            // and the wave loops until its last lane is done.  An initial map matches ~8 query SSEs whatever
            // the query's size, so this is ~30-90 single pair evaluations per restart where walking the rows
            // in step for all lanes costs n1w * n1 / 2 packed ones: 136 for a 32-SSE query, 1313 for 101 SSEs
            // (half the run time of the 101-SSE query class before this loop).  Measured against the rows-in-step
            // form below: 101-SSE query x entries of 8..96 SSEs 1.66 -> 2.1 M scorings/s, BASELINE configs[4]
            // 1.60 -> 2.0 M, configs[2] 310 -> 443 k, 32-SSE query x entries of 8..32 SSEs +7 %, x 32-SSE
            // entries +-0; queries of up to 16 SSEs keep the rows in step (at most 32 packed evaluations: 1.5 %
            // faster there).
            typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
            typedef const __attribute__((address_space(1))) u32x2_t *gptr_u2;
            const gptr_c qpairG = (gptr_c)(uintptr_t)Q.qpair;
            // thinit's maps are order preserving whatever LORDER says (K.cu:588-648), so the c-th matched query
            // SSE has the c-th occupied db SSE as its image: with a one-word db set the two bit sets are popped
            // in step and the map bytes are never read (with more words the byte read is cheaper than the pop)
            constexpr bool POP_IMAGES = M2W == 1;
            static_assert(POP_IMAGES || !MAPOFF, "the walk's map-byte reads take plain indices");
            Bits<M1W> ri = mapped;
            Bits<M2W> rj = occ;
            // pops the lowest set bit: its position (0 when the set is empty) and whether there was one
            auto pop = [](auto &b, bool &valid) -> int {
                constexpr int W = sizeof(b.w) / sizeof(b.w[0]);
                valid = bits_any<W>(b);
                const int pos = max(bits_lowest<W>(b), 0);
                bits_drop_lowest<W>(b);
                return pos;
            };
            // One-word sets on both sides, one lane per chain, full wave: the two lanes of a PAIR walk their two chains
            // together.  A walk costs the wave what its busiest lane costs, and the busiest chain of 64 has ~13
            // matched SSEs (78 pairs) where the mean has 7.7 (26): the rows of the pair's two chains (row a of a chain
            // with m matched SSEs = its a-th matched SSE against the m - 1 - a above it) are merged in order of
            // decreasing length and dealt to the two lanes alternately, so both lanes of the pair meet rows of nearly
            // equal length in the same trip and each does half of the pair's work.  A lane needs its partner's two
            // sets (two shuffles) and hands the partner's share of the sums back at the end (one more).  Bench shape
            // 10.85 -> 10.71 ms (+1.3 %): the walk's ~2300 VALU instructions per restart become ~1800 - the kernel is
            // issue bound, so that, not the shorter dependent chain of loads, is what the gain is.
            // (not with LSOLN: four more live registers there end up in scratch)
            constexpr bool FS_TEAMS = SAT_FS_TEAMS && M1W == 1 && M2W == 1 && FAST && (OPT == 0 || OPT == 1);
            bool teamed = false;
            if constexpr (FS_TEAMS) teamed = __builtin_amdgcn_ballot_w64(true) == ~0ull;
            // The wave's matched pairs in ONE order, dealt evenly (sat_sa_kernel.hpp: fs_seek, fs_advance; DESIGN §4 (32)).  The team walk
            // still pays every row trip for its busiest team and every inner trip for the wave's longest row: counted
            // on the bench inputs (scripts/exp/fs_walk_model.py) 12 row trips and 47 inner trips of two pairs per
            // wave where the pairs, dealt evenly, are 18 trips.  Here the chains that own a pair are compacted to the
            // first lanes (one ds_permute per set), a wave scan of their pair counts gives every chain its first
            // pair's number, lane t takes the pairs [t q, (t + 1) q) with q = ceil(P / 64): it finds the chain that
            // holds pair t q by a search over the scan (6 ds_bpermute), the row and partner inside it by stripping
            // bits (fs_seek), and then walks ONE flat loop of q pairs for the whole wave - next partner, next row,
            // next chain (its sets from the lane that holds them) all by selects (fs_advance).  A pair's term goes
            // to its chain's sum with an LDS atomic: the wave's item table, idle until the first SA step, one dword
            // per compacted chain; the chain's own lane reads it back.  Only launches with the work compaction HAVE that
            // table (satk::lds_layout): LORDER = F (OPT 0) keeps the team walk.
            constexpr bool FS_FLAT = SAT_FS_FLAT && FS_TEAMS && OPT == 1;
            if (FS_FLAT && teamed) {
                const uint32_t mp = mapped.w[0], oc = occ.w[0];
                const bool owns = (mp & (mp - 1u)) != 0u;                              // two matched SSEs or more
                const unsigned long long nzb = __builtin_amdgcn_ballot_w64(owns);
                const int NZ = __popcll(nzb);                                           // wave-uniform
                const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(nzb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)nzb, 0));
                // a permutation of the lanes: owners to 0 .. NZ - 1 in lane order, the rest behind them
                const int dest = (owns ? rank : NZ + wlane - rank) << 2;
                uint32_t cm = (uint32_t)__builtin_amdgcn_ds_permute(dest, (int)mp), co = (uint32_t)__builtin_amdgcn_ds_permute(dest, (int)oc);
                cm = wlane < NZ ? cm : SAT_FS_DUMMY_SET;
                co = wlane < NZ ? co : SAT_FS_DUMMY_SET;
                const int p = wlane < NZ ? fs_pairs(cm) : 0;
                // inclusive wave scan: inside the rows of 16 lanes by row_shr 1, 2, 4, 8 (a lane without a source adds
                // the 0 given as the old value), then lane 15 of rows 0 and 2 to rows 1 and 3 (row_bcast:15, row mask
                // 0xA), then lane 31 to rows 2 and 3 (row_bcast:31, row mask 0xC)
                int incl = p;
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xF, 0xF, false);
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xF, 0xF, false);
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xF, 0xF, false);
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xF, 0xF, false);
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xA, 0xF, false);
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xC, 0xF, false);
                const int P = __builtin_amdgcn_readlane(incl, 63);
                const int q = fs_chunk(P);
                const int first = __mul24(wlane, q), mine = fs_chunk_pairs(P, q, wlane);
                // the last compacted chain whose first pair is at or below this lane's (only owners come before P)
                int r = 0;
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) {
                    const int s = __builtin_amdgcn_ds_bpermute((r + d) << 2, incl - p);
                    r = s <= first ? r + d : r;
                }
                const int s0 = __builtin_amdgcn_ds_bpermute(r << 2, incl - p);
                FsCursor cur = fs_seek((uint32_t)__builtin_amdgcn_ds_bpermute(r << 2, (int)cm),
                                       (uint32_t)__builtin_amdgcn_ds_bpermute(r << 2, (int)co), mine > 0 ? first - s0 : 0);
                items[wlane] = 0u;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                for (int it = 0; it < q; it += SAT_FS_UNROLL) {
                    int ll[SAT_FS_UNROLL], rr[SAT_FS_UNROLL];
                    bool vv[SAT_FS_UNROLL];
                    DbRow<CELLS> drow[SAT_FS_UNROLL];
                    u32x2_t qcell[SAT_FS_UNROLL];
#pragma unroll
                    for (int u = 0; u < SAT_FS_UNROLL; u++) {
                        vv[u] = it + u < mine;
                        const int i = __builtin_ctz(cur.rm), k = __builtin_ctz(cur.rk);
                        drow[u] = db_row(__builtin_ctz(cur.ro));
                        ll[u] = __builtin_ctz(cur.rl);
                        rr[u] = r;
                        qcell[u] = *(gptr_u2)(qpairG + ((uint32_t)__mul24(i, N1P * 8) + ((uint32_t)k << 3)));
                        // (a lane that leaves the last chain fetches from lane 0 and stands there, its chunk done)
                        const uint32_t nm = (uint32_t)__builtin_amdgcn_ds_bpermute((r + 1) << 2, (int)cm);
                        const uint32_t no = (uint32_t)__builtin_amdgcn_ds_bpermute((r + 1) << 2, (int)co);
                        r += fs_advance(cur, vv[u] ? 1u : 0u, nm, no) ? 1 : 0;
                    }
#pragma unroll
                    for (int u = 0; u < SAT_FS_UNROLL; u++) {
                        const uint2 c = db_cell<CELLS>(drow[u], ll[u]);
                        int term = pair_term(qcell[u].x, qcell[u].y, c.x, c.y);
                        // (opaque: left to itself the compiler sinks a pair's cell reads and its term under the lane
                        // mask of its atomic, one pair's loads waiting behind the other's)
                        asm volatile("" : "+v"(term));
                        if (vv[u]) __hip_atomic_fetch_add((lds_i32_t *)(items + rr[u]), term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                score = owns ? (int)items[rank] : 0;
            } else if (FS_TEAMS && teamed) {
                const int pl = wlane & 1;
                const uint32_t om = (uint32_t)__shfl_xor((int)mapped.w[0], 1, 64), oo = (uint32_t)__shfl_xor((int)occ.w[0], 1, 64);
                const uint32_t m0 = pl ? om : mapped.w[0], o0 = pl ? oo : occ.w[0];       // chain 0: the even lane's
                const uint32_t m1 = pl ? mapped.w[0] : om, o1 = pl ? occ.w[0] : oo;
                const int c0n = __popc(m0), c1n = __popc(m1);
                const bool big1 = c1n > c0n;                                             // the longer chain leads the merged order
                const uint32_t mb = big1 ? m1 : m0, ob = big1 ? o1 : o0, msm = big1 ? m0 : m1, osm = big1 ? o0 : o1;
                const int rb = max((big1 ? c1n : c0n) - 1, 0), rs = max((big1 ? c0n : c1n) - 1, 0);   // rows with partners
                const int dlead = rb - rs, etot = rb + rs;
                uint32_t rm = mb, ro = ob;                 // the stream this lane is on: its sets with the rows below `cur` stripped
                int cur = 0, acc_b = 0, acc_s = 0;
                bool on_small = false;
                // element e of the merged order: the first dlead are rows 0 .. of the longer chain (lengths rb .. rs + 1),
                // then lengths rs .. 1 twice each, longer chain first.  This lane takes e = pl, pl + 2, ...: the leading
                // rows of the longer chain two apart, then ONE of the two chains row after row (e - dlead keeps its parity).
                for (int e = pl; __builtin_amdgcn_ballot_w64(e < etot) != 0ull; e += 2) {
                    const bool act = e < etot;
                    const int e2 = e - dlead;
                    const bool small = e2 >= 0 && (e2 & 1) != 0;
                    const int len = e2 < 0 ? rb - e : rs - (e2 >> 1);
                    const int a = (small ? rs : rb) - len;
                    if (small && !on_small) { rm = msm; ro = osm; cur = 0; on_small = true; }
#pragma unroll
                    for (int q = 0; q < 2; q++) {                           // at most two rows further on
                        const uint32_t go = (act && cur < a) ? 1u : 0u;
                        rm &= rm - go;
                        ro &= ro - go;
                        cur += (int)go;
                    }
                    const int i = act ? __ffs(rm) - 1 : 0, ji = act ? __ffs(ro) - 1 : 0;
                    Bits<1> rk, rl;
                    rk.w[0] = act ? rm & (rm - 1u) : 0u;
                    rl.w[0] = act ? ro & (ro - 1u) : 0u;
                    const DbRow<CELLS> drow = db_row(ji);
                    const uint32_t qrow = (uint32_t)__mul24(i, N1P * 8);
                    int rowsum = 0;
                    while (__builtin_amdgcn_ballot_w64(rk.w[0] != 0u) != 0ull) {
                        int ll[SAT_FS_UNROLL];
                        bool vv[SAT_FS_UNROLL];
                        u32x2_t qcell[SAT_FS_UNROLL];
#pragma unroll
                        for (int u = 0; u < SAT_FS_UNROLL; u++) {
                            bool vl;
                            const int k = pop(rk, vv[u]);
                            ll[u] = pop(rl, vl);
                            qcell[u] = *(gptr_u2)(qpairG + (qrow + ((uint32_t)k << 3)));
                        }
#pragma unroll
                        for (int u = 0; u < SAT_FS_UNROLL; u++) {
                            const uint2 c = db_cell<CELLS>(drow, ll[u]);
                            const int term = pair_term(qcell[u].x, qcell[u].y, c.x, c.y);
                            rowsum += vv[u] ? term : 0;
                        }
                    }
                    acc_s += small ? rowsum : 0;
                    acc_b += small ? 0 : rowsum;
                }
                const int acc0 = big1 ? acc_s : acc_b, acc1 = big1 ? acc_b : acc_s;          // by chain
                score = (pl ? acc1 : acc0) + __shfl_xor(pl ? acc0 : acc1, 1, 64);
            } else
            while (__builtin_amdgcn_ballot_w64(bits_any<M1W>(ri)) != 0ull) {
                bool ai, aj;
                // The lanes that share a chain take its ROWS in turn: every trip pops lpc matched SSEs, lane `part`
                // keeps the part-th as its row - with the matched SSEs above THAT one as the row's partners - and each
                // lane then walks its own row's partners alone.  (The first version shared every row: all lanes popped
                // the same partner sequence and kept every lpc-th, i.e. every lane paid every pop - and the pops of a
                // four-word set are most of a pair's instructions.)
                int i = 0, ji = 0;                                         // (a lane that is done walks row 0, sums nothing)
                ai = false;
                Bits<M1W> rk = bits_zero<M1W>();                           // the matched SSEs above i ...
                Bits<M2W> rl = bits_zero<M2W>();                           // ... and their images
                for (int p = 0; p < lpc; p++) {
                    bool v;
                    const int pos = pop(ri, v);
                    int img = 0;
                    if constexpr (POP_IMAGES) { bool vj; img = pop(rj, vj); }
                    if (p == part) {
                        i = pos;
                        ai = v;
                        ji = img;
                        rk = ri;
                        rl = rj;
                    }
                }
                (void)aj;
                if constexpr (!POP_IMAGES) { ji = smap_b[map_byte_addr(i)]; ji = ai ? ji : 0; }
                const DbRow<CELLS> drow = db_row(ji);
                const uint32_t qrow = (uint32_t)__mul24(i, N1P * 8);
                int rowsum = 0;
                // SAT_FS_UNROLL pairs per lane and round, their loads in flight together
                while (__builtin_amdgcn_ballot_w64(bits_any<M1W>(rk)) != 0ull) {
                    int ll[SAT_FS_UNROLL];
                    bool vv[SAT_FS_UNROLL];
                    u32x2_t qcell[SAT_FS_UNROLL];
#pragma unroll
                    for (int u = 0; u < SAT_FS_UNROLL; u++) {
                        const int ku = pop(rk, vv[u]);
                        ll[u] = 0;
                        if constexpr (POP_IMAGES) { bool vl; ll[u] = pop(rl, vl); }
                        // (none left: SSE 0's image, possibly the null column - it exists, and the term is dropped)
                        if constexpr (!POP_IMAGES) ll[u] = smap_b[map_byte_addr(ku)];
                        qcell[u] = *(gptr_u2)(qpairG + (qrow + ((uint32_t)ku << 3)));
                    }
#pragma unroll
                    for (int u = 0; u < SAT_FS_UNROLL; u++) {
                        const uint2 c = db_cell<CELLS>(drow, ll[u]);
                        const int term = pair_term(qcell[u].x, qcell[u].y, c.x, c.y);
                        rowsum += vv[u] ? term : 0;
                    }
                }
                score += rowsum;
            }
        } else {
            score = score_rows();
        }
        if (lpc >= 2) score += __shfl_xor(score, 1, 64);
        if (lpc == 4) score += __shfl_xor(score, 2, 64);
        const int best_before = best;
        if (score > best) {
            best = score;
            if (lsoln && beats_leader(score, restart))
                for (int w = 0; w < n1w; w++) bmap[w * T + tid] = smap[w * TP + tid];
        }
        if constexpr (MATCH) {
            rbest = score;
            rset = occ;
            if (replay && part == 0)
                for (int w = 0; w < n1w; w++) bmap[w * T + tid] = smap[w * TP + tid];
        }

        // ---- 100 Metropolis steps, temperature 10 * 0.95^iter (K.cu:1030-1191)
        SAT_PHASE(6);                     // full score of the initial map
        uint4 blk = uint4{ 0u, 0u, 0u, 0u };
        for (int iter = 0; iter < SAT_K_MAXITER; iter++) {
            // this step's row of the Metropolis table.  The directory is read-only for the kernel's
            // lifetime: through the constant address space these are scalar loads (a plain global
            // pointer gets a vector load, whose latency would sit in front of the table load), asked
            // for here so that they are back long before the test at the end of the step
            const int rowoff = prowC[2 * iter], rowmax = prowC[2 * iter + 1];
            // The first 64 entries of this step's row, one per lane: a coalesced load asked for here, a whole step
            // before the test needs it; the test then fetches its entry from the lane that holds it (ds_bpermute)
            // instead of waiting for a dependent global load at the very end of the step's chain.  Bench shape +3 %
            // in same-box A/B runs, the other LORDER launches of the 32-SSE classes and up with one-word db sets
            // 0 .. +0.7 %; not where it measured slower: the 16 class (-5 %), the static loops of LORDER = F
            // (-1.6 %), 64-SSE entries (-0.8 %).
            constexpr bool ROW_IN_LANES = N1P >= 32 && M2W == 1 && (OPT < 0 || (OPT & 1) != 0);
            float rowv = 0.0f;
            if constexpr (ROW_IN_LANES)
                rowv = *(gptr_f32)((gptr_c)ptabG + (((uint32_t)rowoff + (uint32_t)min(wlane, rowmax + 2)) << 2));
            // one Philox block per two steps: the even step draws it and uses words 0, 1, the odd step
            // uses words 2, 3 (moved down).  Word a = two 16-bit draws (moved SSE: high half, candidate:
            // low half), word b = the Metropolis draw.
            if ((iter & 1) == 0) {
                blk = philox_block(Q.seed_q, subseq, (uint32_t)(SAT_K_STEP_BLOCK0 + (iter >> 1)));
            } else {
                blk.x = blk.z;
                blk.y = blk.w;
            }
            const uint32_t word_a = blk.x, word_b = blk.y;
            SAT_DIAG_PERTURB_STEP;

            // which query SSE moves (K.cu:1037-1042)
            const int ssei = scaled_index16(word_a >> 16, n1, n1 - 1);

            // candidate db SSEs: free, same type, inside the order window (K.cu:1053-1086)
            int oldj;
            Bits<M2W> cand;
            int rank_base = 0;            // PICK_TABLE: where the window's first candidate stands in `pos`
            if (M2W == 1 && opt_lorder) {
                // LORDER maps are order preserving (thinit builds them so and every move stays
                // inside its window), so the images of the mapped query SSEs are the set bits of
                // `occ` in the same order.  With p = highest mapped query SSE <= ssei and A its
                // image, the window [startj, endj) of K.cu:1053-1077 is the run of free bits
                // between A and the next occupied bit above it: no second and third map read, no
                // range masks.  p == ssei exactly when ssei is mapped, so A is also its old image.
                int p;
                bool none;
                highest_mapped_upto(mapped, ssei, p, none);
                // (scaled bytes: with no mapped SSE at or below ssei the byte of SSE 0 is read, p is 0 and may equal
                // ssei: the plain byte was the null SSE by itself there, the scaled one is the flag and shifts to 0, so
                // `none` says "unmatched"; A is then not used: `empty`)
                const int A = MAPOFF ? smap_b[map_byte_addr(p)] >> 3 : smap_b[map_byte_addr(p)];
                SAT_DIAG_DUP_MAPBYTE(&smap_b[map_byte_addr(p)]);
                oldj = (p == ssei && !(MAPOFF && none)) ? A : NULLJ;
                const uint32_t above = 0xFFFFFFFEu << (A & 31);          // bits A+1 .. 31
                const uint32_t y = occ.w[0] & above;                     // occupied above A
                const uint32_t gap = (y - 1u) & ~y & above;              // free run up to the next occupied bit
                // no mapped SSE at or below ssei: startj = n2, empty (K.cu:1060-1063); no mapped
                // successor: endj = -1, empty, unless ssei is the last query SSE (K.cu:1064-1077)
                const bool empty = none || (y == 0u && ssei != n1 - 1);
                const uint32_t qm = qmask[ssei];
                cand.w[0] = empty ? 0u : (qm & gap);
                // Everything in the window is free, so its candidates are simply the SSEs of the type above A, in
                // order: the first of them stands in the type's run of `pos` behind the SSEs of the type up to A.
                // (No candidate - `empty`, or A = 31 - leaves an index of at most the run's end: read, not used.)
                if constexpr (PICK_TABLE) rank_base = qbase[ssei] + __popc(qm & ~above);
            } else if (M2W == 2 && FAST && opt_lorder) {
                // The same for entries of 33..64 SSEs with the two words of the db-side sets taken as ONE 64-bit
                // word: p, A and the old image as above, the window is the run of free bits between A and the next
                // occupied bit - (y - 1) & ~y on 64 bits - where the general path below reads three map bytes (two of
                // them behind the first) and builds four range masks word by word.
                int p;
                bool none;
                highest_mapped_upto(mapped, ssei, p, none);
                const int t = qtypes[ssei];
                const int A = smap_b[map_byte_addr(p)];
                oldj = p == ssei ? A : NULLJ;
                const unsigned long long occ64 = (unsigned long long)occ.w[0] | ((unsigned long long)occ.w[1] << 32);
                const unsigned long long above = (~1ull) << (A & 63);             // bits A+1 .. 63 (A = 64: no mapped SSE, `empty`)
                const unsigned long long y = occ64 & above;                       // occupied above A
                const unsigned long long gap = (y - 1ull) & ~y & above;           // free run up to the next occupied bit
                const unsigned long long tm = *reinterpret_cast<const unsigned long long *>(&tmask[t * TMS]);
                const bool empty = none || (y == 0ull && ssei != n1 - 1);
                const unsigned long long c64 = empty ? 0ull : (tm & gap);
                cand.w[0] = (uint32_t)c64;
                cand.w[M2W - 1] = (uint32_t)(c64 >> 32);
            } else if (M2W == 4 && FAST && opt_lorder) {
                // ... and for entries above 64 SSEs as two 64-bit halves: y - 1 borrows from the upper half exactly
                // when no bit of the lower half is occupied above A.
                int p;
                bool none;
                highest_mapped_upto(mapped, ssei, p, none);
                const int t = qtypes[ssei];
                const int A = smap_b[map_byte_addr(p)];
                oldj = p == ssei ? A : NULLJ;
                const unsigned long long occ_lo = (unsigned long long)occ.w[0] | ((unsigned long long)occ.w[1] << 32),
                                         occ_hi = (unsigned long long)occ.w[2] | ((unsigned long long)occ.w[3] << 32);
                const unsigned long long base = (~1ull) << (A & 63);               // (A & 63 = 63: nothing above it in its half)
                const bool a_hi = A >= 64;
                const unsigned long long above_lo = a_hi ? 0ull : base, above_hi = a_hi ? base : ~0ull;
                const unsigned long long y_lo = occ_lo & above_lo, y_hi = occ_hi & above_hi;      // occupied above A
                const unsigned long long gap_lo = (y_lo - 1ull) & ~y_lo & above_lo;
                const unsigned long long gap_hi = (y_hi - (y_lo == 0ull ? 1ull : 0ull)) & ~y_hi & above_hi;
                const unsigned long long *tm = reinterpret_cast<const unsigned long long *>(&tmask[t * TMS]);
                const bool empty = none || ((y_lo | y_hi) == 0ull && ssei != n1 - 1);
                const unsigned long long c_lo = empty ? 0ull : (tm[0] & gap_lo), c_hi = empty ? 0ull : (tm[1] & gap_hi);
                cand.w[0] = (uint32_t)c_lo;
                cand.w[1 % M2W] = (uint32_t)(c_lo >> 32);
                cand.w[2 % M2W] = (uint32_t)c_hi;
                cand.w[3 % M2W] = (uint32_t)(c_hi >> 32);
            } else {
                oldj = map_decode<MAPOFF>(smap_b[map_byte_addr(ssei)], NULLJ);
                int startj = 0, endj = n2;
                if (opt_lorder) {
                    Bits<M1W> upto = bits_below<M1W>(ssei + 1), lowpart, highpart;
#pragma unroll
                    for (int w = 0; w < M1W; w++) {
                        lowpart.w[w] = mapped.w[w] & upto.w[w];
                        highpart.w[w] = mapped.w[w] & ~upto.w[w];
                    }
                    const int p = bits_highest<M1W>(lowpart);
                    const int q = bits_lowest<M1W>(highpart);
                    const int pimg = map_decode<MAPOFF>(smap_b[map_byte_addr(p < 0 ? 0 : p)], NULLJ);
                    const int qimg = map_decode<MAPOFF>(smap_b[map_byte_addr(q < 0 ? 0 : q)], NULLJ);
                    startj = p < 0 ? n2 : pimg;                      // no mapped predecessor: empty window
                    endj = (ssei == n1 - 1) ? n2 : (q < 0 ? -1 : qimg);   // K.cu:1064-1077
                }
                const int t = qtypes[ssei];
                Bits<M2W> lo = bits_below<M2W>(startj), hi = bits_below<M2W>(endj);
#pragma unroll
                for (int w = 0; w < M2W; w++)
                    cand.w[w] = tmask[t * TMS + w] & ~occ.w[w] & hi.w[w] & ~lo.w[w];
            }
            // no candidate: the SSE becomes unmatched; one: it is taken without a draw
            // (K.cu:701-702); several: the draw picks the (u - EPS) * cnt -th (K.cu:705-711).
            // Branch-free: in a 64-lane wave every case occurs anyway.
            const int cnt = bits_count<M2W>(cand);
            const int pick = scaled_index16(word_a & 0xFFFFu, cnt, max(cnt - 1, 0));   // 0 for cnt <= 1: no draw used
            int sel;
            if (PICK_TABLE && opt_lorder) {
                // the pick-th candidate by its rank: one table read whatever the largest pick of the wave (stripping
                // `pick` bits cost every lane of the wave what its deepest pick cost, ~4 trips for a mean pick of 0.15)
                sel = pos[rank_base + pick];
            } else if (M2W == 1 && opt_lorder) {
                // inside an order window the picked rank is small (few free same-type SSEs): strip
                // the lowest set bit `pick` times, looping while any lane of the wave still has to
                uint32_t c = cand.w[0];
                int left = pick;
                {
                    // the first strip without the wave-level test (a ballot, a scalar branch and its wait per trip of
                    // the loop below; most waves need one or two strips): 32-SSE bench shape +1.5 %
                    const uint32_t go = left > 0 ? 1u : 0u;
                    c &= c - go;
                    left -= (int)go;
                }
                while (__builtin_amdgcn_ballot_w64(left > 0) != 0ull) {
                    const uint32_t go = left > 0 ? 1u : 0u;
                    c &= c - go;                                   // c & (c - 1) clears the lowest set bit
                    left -= (int)go;
                }
                sel = __ffs(c) - 1;
            } else if (M2W == 2 && FAST && opt_lorder && __builtin_amdgcn_ballot_w64(pick > 2) == 0ull) {
                // (wide windows - a short query against a long entry - hold many candidates: the strip loop runs as
                // often as the largest pick of the wave, so it is taken only while every pick is small; else the rank select)
                unsigned long long c = (unsigned long long)cand.w[0] | ((unsigned long long)cand.w[M2W - 1] << 32);
                int left = pick;
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const unsigned long long go = left > 0 ? 1ull : 0ull;
                    c &= c - go;
                    left -= (int)go;
                }
                sel = __ffsll((long long)c) - 1;
            } else if (M2W == 4 && FAST && opt_lorder && __builtin_amdgcn_ballot_w64(pick > 2) == 0ull) {
                unsigned long long c_lo = (unsigned long long)cand.w[0] | ((unsigned long long)cand.w[1 % M2W] << 32),
                                   c_hi = (unsigned long long)cand.w[2 % M2W] | ((unsigned long long)cand.w[3 % M2W] << 32);
                int left = pick;
                // strips the lowest candidate: of the lower half while it has one, else of the upper half
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const bool go = left > 0, in_lo = c_lo != 0ull;
                    c_lo &= c_lo - ((go && in_lo) ? 1ull : 0ull);
                    c_hi &= c_hi - ((go && !in_lo) ? 1ull : 0ull);
                    left -= go ? 1 : 0;
                }
                sel = c_lo != 0ull ? __ffsll((long long)c_lo) - 1 : 63 + __ffsll((long long)c_hi);
            } else {
                sel = bits_select<M2W>(cand, pick);
            }
            const bool nreal = cnt != 0;
            const int newj = nreal ? sel : NULLJ;
            const uint8_t newbyte = (uint8_t)(MAPOFF ? (nreal ? (uint32_t)sel << 3 : SAT_MAP_UNMATCHED) : (uint32_t)newj);   // its map byte

            SAT_PHASE(0);                 // draw + proposal
            // score change (deltasd, K.cu:502-535)
            int delta;
            {
                // rows of this step that are real, listed once per chain (part 0 of its lanes)
                const bool oreal = oldj != NULLJ;
                const bool lists = part == 0;
                const int nitems = lists ? (int)oreal + (int)nreal : 0;
                // (two plain ballots and scalar logic: a ballot of a combined predicate goes through
                // a select and a compare per lane)
                const unsigned long long bo = __builtin_amdgcn_ballot_w64(lists && oreal),
                                         bn = __builtin_amdgcn_ballot_w64(lists && nreal);
                const unsigned long long m1 = bo | bn, m2 = bo & bn;
                const int total_items = __popcll(m1) + __popcll(m2);           // wave-uniform
                // only full waves compact (a wave's last lanes may have no restart left), so a lane's
                // rank among the consumers is its lane number; see cmp_* above the restart loop
                if (opt_compact && __builtin_amdgcn_ballot_w64(true) == ~0ull && total_items <= 64) {
                    const int pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0)) +
                                    __builtin_amdgcn_mbcnt_hi((uint32_t)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m2, 0));
                    // item = row | moved SSE << 8 | owner chain << 16 | negate << 24.  The slot doubles as
                    // the row's accumulator: the lanes that serve an item all read it in one instruction,
                    // then add their signed sums to it; the owner subtracts what it wrote.
                    const uint32_t item1 = (uint32_t)(oreal ? oldj : newj) | ((uint32_t)ssei << 8) | ((uint32_t)tid << 16) |
                                           (oreal ? 1u << 24 : 0u);
                    const uint32_t item2 = (uint32_t)newj | ((uint32_t)ssei << 8) | ((uint32_t)tid << 16);
                    if (nitems >= 1) items[pre] = item1;
                    if (nitems == 2) items[pre + 1] = item2;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    SAT_PHASE(1);         // compaction set-up
                    // one round: the rows first .. first + 64 / lpi - 1 of the table, `lpi` lanes per row
                    // (lane `rsub` of the round serves row first + rsub, words rkw, rkw + lpi, ...)
                    auto one_round = [&](auto wtag, int first, int lpi, int rsub, int rkw, bool rlane_ok) {
                        constexpr int W = decltype(wtag)::value;
                        const int idx = first + rsub;
                        bool ok = rlane_ok && idx < total_items;
                        int v = 0;
                        if (ok) {
                            const uint32_t it = items[idx];
                            const int row = it & 0xFF, si = (it >> 8) & 0xFF, owner = (it >> 16) & 0xFF;
                            const DbRow<CELLS> drow = db_row(row);
                            float4 qd[W];
                            uint32_t qc[W], wd[W];
                            // byte offsets of (word rkw, column si) in the two query arrays; word rkw + u * lpi is
                            // u * lpi * N1P groups further on (an instruction offset where lpi is a constant)
                            const uint32_t qoff4 = (uint32_t)(rkw * N1P + si) << 2, qoff16 = qoff4 << 2;
#pragma unroll
                            for (int u = 0; u < W; u++) {
                                // words past the map (a lane's last one, when lpi does not divide n1w)
                                // are padding: unmatched SSEs against the query's sentinel cells
                                const int kwu = rkw + u * lpi;
                                wd[u] = smap[kwu * TP + owner];
                                SAT_DIAG_DUP_MAPWORD(&smap[kwu * TP + owner]);
                                qd[u] = load_qdist(qoff16 + (uint32_t)(u * lpi * N1P * 16));
                                qc[u] = load_qcode(qoff4 + (uint32_t)(u * lpi * N1P * 4));
                            }
#pragma unroll
                            for (int u = 0; u < W; u++) v = quad_terms(qd[u], qc[u], drow, wd[u], 0u, v);
                            v = (it >> 24) ? -v : v;
                        }
                        // signed sum of a lane's words -> the row's accumulator (its item slot)
                        if ((lpi & 3) == 0) {
                            // rows are aligned groups of 4m lanes: add up each quad of lanes with two
                            // DPP moves, so that a quarter of the lanes hit the accumulator
                            v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
                            v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
                            ok = ok && (rkw & 3) == 0;
                        }
                        if (ok)
                            __hip_atomic_fetch_add((lds_i32_t *)(items + idx), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        if (ok) SAT_DIAG_DUP_ATOMIC((lds_i32_t *)(items + idx));
                    };
                    auto main_round = [&](int first) {
                        if constexpr (WPL > 0) one_round(std::integral_constant<int, WPL>{}, first, cmp_lpi, sub, kw, lane_ok);
                        else switch (cmp_wpl) {
                        case 1: one_round(std::integral_constant<int, 1>{}, first, cmp_lpi, sub, kw, lane_ok); break;
                        case 2: one_round(std::integral_constant<int, 2>{}, first, cmp_lpi, sub, kw, lane_ok); break;
                        case 3: one_round(std::integral_constant<int, 3>{}, first, cmp_lpi, sub, kw, lane_ok); break;
                        default: one_round(std::integral_constant<int, 4>{}, first, cmp_lpi, sub, kw, lane_ok); break;
                        }
                    };
                    // full rounds of the main shape while more rows remain than one round holds; the
                    // last rows go to the shape with the fewest words per lane that still takes them in
                    // one round (a step lists ~0.6 rows per chain: the tail is usually a few rows)
                    int first = 0;
                    for (; total_items - first > per_round; first += per_round) main_round(first);
                    const int rest = total_items - first;
                    if (rest > 0) {
                        if (cmp_wpl > 1 && rest <= tail1_rows) {
                            // (lane -> (row, word) of a tail shape is worked out here every time: hoisted out
                            // of the step loop these values would sit in registers the main shape needs)
                            int l = wlane;
                            asm volatile("" : "+v"(l));
                            const int rsub = __mul24(l, tail1_recip) >> 16;
                            one_round(std::integral_constant<int, 1>{}, first, n1w, rsub, l - __mul24(rsub, n1w), rsub < tail1_rows);
                        } else if (cmp_wpl > 2 && rest <= tail2_rows) {
                            int l = wlane;
                            asm volatile("" : "+v"(l));
                            const int rsub = __mul24(l, tail2_recip) >> 16;
                            one_round(std::integral_constant<int, 2>{}, first, tail2_lpi, rsub, l - __mul24(rsub, tail2_lpi), rsub < tail2_rows);
                        } else {
                            main_round(first);
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    SAT_PHASE(2);         // compacted rounds
                    delta = 0;
                    if (nitems >= 1) delta = (int)(items[pre] - item1);
                    if (nitems == 2) delta += (int)(items[pre + 1] - item2);
                    // with several lanes per chain only part 0 listed rows: hand its sum to the others
                    if (lpc > 1) delta = __shfl(delta, wlane & ~(lpc - 1), 64);
                } else {
                    // dense regime: every lane scores its own two rows
                    // (a null image has no row: row 0 stands in and the sum is dropped)
                    const DbRow<CELLS> orow = db_row(oreal ? oldj : 0), nrow = db_row(nreal ? newj : 0);
                    int sum_new = 0, sum_old = 0;
                    auto move_group = [&](int kw) {
                        const uint32_t word = smap[kw * TP + tid];
                        const uint32_t qi = (uint32_t)(kw * N1P + ssei);      // 32-bit offsets from uniform bases
                        const float4 qd = load_qdist(qi << 4);
                        const uint32_t qc = load_qcode(qi << 2);
                        sum_new = quad_terms(qd, qc, nrow, word, 0u, sum_new);
                        sum_old = quad_terms(qd, qc, orow, word, 0u, sum_old);
                    };
                    if (lpc == 1) for (int kw = 0; kw < n1w; kw++) move_group(kw);
                    else for (int kw = part; kw < n1w; kw += lpc) move_group(kw);
                    delta = (nreal ? sum_new : 0) - (oreal ? sum_old : 0);
                    if (lpc >= 2) delta += __shfl_xor(delta, 1, 64);
                    if (lpc == 4) delta += __shfl_xor(delta, 2, 64);
                }
            }
            const int newscore = score + delta;
            SAT_PHASE(3);                 // read-back (compacted) or the static loops
            SAT_DIAG_SELFCHECK_STEP;

            // best-so-far from the PROPOSED state, before the accept test (K.cu:1136-1155)
            // (which restart holds the best is settled once per restart, below the step loop)
            if (lsoln && newscore > best) {
                if (beats_leader(newscore, restart)) {
                    for (int w = 0; w < n1w; w++) bmap[w * T + tid] = smap[w * TP + tid];
                    bmap_b[bmap_byte_addr(ssei)] = newbyte;
                }
            }
            best = max(best, newscore);
            if constexpr (MATCH) {
                // the restart's own best, from the proposed state: occ without the old image, with the new one
                if (newscore > rbest) {
                    rbest = newscore;
                    rset = occ;
                    if (oldj != NULLJ) bits_clear<M2W>(rset, oldj);
                    if (nreal) bits_set<M2W>(rset, newj);
                    if (replay && part == 0) {
                        for (int w = 0; w < n1w; w++) bmap[w * T + tid] = smap[w * TP + tid];
                        bmap_b[bmap_byte_addr(ssei)] = newbyte;
                    }
                }
            }

            SAT_PHASE(4);                 // best tracking
            // Metropolis: accept iff expf(delta / temp) > u, via the host-built table
            // the table holds 2^32 * expf(.), compared with 2^32 * u: same decision, one multiply less
            const float u = draw32(word_b);
            // row = { 2^33 (any delta > 0: expf(x > 0) > 1 >= u), P[0], ..., P[rowmax], 0.0 (a larger
            // -delta can never be accepted) }, indexed by 1 - delta clamped to the row
            const uint32_t nd = (uint32_t)min(max(1 - delta, 0), rowmax + 2);
            float p;
            // (full waves only: a lane without a restart has not loaded its entry of the row; -delta beyond 62
            // anywhere in the wave: the load after all)
            if (ROW_IN_LANES && __builtin_amdgcn_ballot_w64(true) == ~0ull && __builtin_amdgcn_ballot_w64(nd >= 64u) == 0ull)
                p = __int_as_float(__builtin_amdgcn_ds_bpermute((int)(nd << 2), __float_as_int(rowv)));
            else
                p = *(gptr_f32)((gptr_c)ptabG + (((uint32_t)rowoff + nd) << 2));
            const bool accept = p > u;
            if (accept) smap_b[map_byte_addr(ssei)] = newbyte;
            score = accept ? newscore : score;
            {
                // an accepted move toggles the old image's bit (set) and the new image's bit (clear) of `occ`, and
                // the moved SSE's bit of `mapped` when it changes between matched and unmatched; the accept
                // decision is folded into the bits, the word index picks the word
                const bool oreal_ = oldj != NULLJ;
                if constexpr (M2W == 1) {
                    // bit n2 (the null SSE) must not be touched; n2 may be 32: mask by comparison.
                    const uint32_t oldbit = (accept && oreal_) ? (1u << (oldj & 31)) : 0u;
                    const uint32_t newbit = (accept && nreal) ? (1u << (newj & 31)) : 0u;
                    occ.w[0] = (occ.w[0] & ~oldbit) | newbit;
                } else {
                    const uint32_t oldbit = (accept && oreal_) ? (1u << (oldj & 31)) : 0u;
                    const uint32_t newbit = (accept && nreal) ? (1u << (newj & 31)) : 0u;
                    const int ow = oldj >> 5, nw = newj >> 5;
#pragma unroll
                    for (int w = 0; w < M2W; w++) occ.w[w] ^= (ow == w ? oldbit : 0u) ^ (nw == w ? newbit : 0u);
                }
                if constexpr (M1W == 1) {
                    const uint32_t ibit = 1u << ssei;
                    const uint32_t setbit = (accept && nreal) ? ibit : 0u, clrbit = (accept && !nreal) ? ibit : 0u;
                    mapped.w[0] = (mapped.w[0] & ~clrbit) | setbit;
                } else {
                    const uint32_t ibit = (accept && oreal_ != nreal) ? (1u << (ssei & 31)) : 0u;
                    const int iw = ssei >> 5;
#pragma unroll
                    for (int w = 0; w < M1W; w++) mapped.w[w] ^= iw == w ? ibit : 0u;
                }
            }
            SAT_PHASE(5);                 // Metropolis + state update
        }
        if (best > best_before) best_restart = (uint32_t)restart;
        if constexpr (MATCH) {
            // record pass: the restart's record {own best, db set}, scores first, then the set words (restart-major:
            // the lanes of a wave write consecutive words); read back only by this lane, in the epilogue
            if (!replay && part == 0) {
                mrec[restart] = (uint32_t)rbest;
#pragma unroll
                for (int w = 0; w < M2W; w++) mrec[(size_t)(w + 1) * a.maxstart + restart] = rset.w[w];
            }
        }
    }
    SAT_PHASE_FLUSH;
    SAT_DIAG_PERTURB_END;

    if constexpr (MATCH) {
        // replay pass: the own-best map of the tid-th picked restart (pitch map_pitch; the host fills the rest)
        if (replay) {
            if (any && part == 0) {
                int8_t *out = mx.maps + (mrow * mx.max_matches + tid) * (size_t)mx.map_pitch;
                for (int i = 0; i < n1; i++) {
                    const int j = map_decode<MAPOFF>(bmap_b[bmap_byte_addr(i)], NULLJ);
                    out[i] = (int8_t)(j == NULLJ ? -1 : j);
                }
            }
            return;
        }
    }

    // ---- arg-max over restarts; ties go to the lowest restart index, which is the
    // first restart that reaches the maximum in the reference's sequential order
    // (strict '>' at K.cu:1024, 1137, 1211)
    unsigned long long key = any
        ? (((unsigned long long)(uint32_t)(best + 0x40000000)) << 32) | (0xFFFFFFFFu - best_restart)
        : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long other = __shfl_xor(key, off, 64);
        key = other > key ? other : key;
    }
    const int wave = lane_id >> 6, nwaves = (nthreads + 63) >> 6;
    if (wlane == 0) *red_key(wave) = key;
    __syncthreads();
    unsigned long long win = *red_key(0);
    for (int w = 1; w < nwaves; w++) win = *red_key(w) > win ? *red_key(w) : win;

    const uint32_t win_restart = 0xFFFFFFFFu - (uint32_t)(win & 0xFFFFFFFFu);
    // pair mode: the item's key folds into its pair's (restart ranges of one pair in any order, any workgroups);
    // its map pass re-runs the pair's winning restart alone and writes only the map
    if constexpr (PAIRS) {
        if (lane_id == 0 && !lsoln) atomicMax(px.keys + pit.pair, win);
    } else {
        if (lane_id == 0) Q.scores[e] = (int)(uint32_t)(win >> 32) - 0x40000000;
    }
    if (lsoln && any && part == 0 && best_restart == win_restart &&
        ((((unsigned long long)(uint32_t)(best + 0x40000000)) << 32) | (0xFFFFFFFFu - best_restart)) == win) {
        int8_t *out = PAIRS ? px.maps + (size_t)pit.pair * SAT_K_MAXDIM : Q.ssemaps + (size_t)e * n1;
        for (int i = 0; i < n1; i++) {
            const int j = map_decode<MAPOFF>(bmap_b[bmap_byte_addr(i)], NULLJ);
            out[i] = (int8_t)(j == NULLJ ? -1 : j);
        }
    }

    // (pair-match mode: the records of a pair are complete only when all its items have run - pair_match_select)
    if constexpr (MATCH && !PAIRS) {
        // ---- greedy selection: match 0 is the arg-max above; each further round takes the largest key among the
        // records with a positive score whose db set misses the union of the sets taken so far.  The union lives in
        // the type masks' LDS words (no wave reads those after the barrier above); only the lane that ran a restart
        // reads its records.
        uint32_t *uni = tmask;
        const int M = mx.max_matches;
        // appends key `k` as match m: its score and restart, and (the lane that ran it) its db set to the union
        int m = 0;
        auto take = [&](unsigned long long k) {
            const uint32_t r = 0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFu);
            if (lane_id == 0) {
                mx.scores[mrow * M + m] = (int)(uint32_t)(k >> 32) - 0x40000000;
                mx.restarts[mrow * M + m] = (int)r;
            }
            if (part == 0 && (int)(r % (uint32_t)T) == tid) {
#pragma unroll
                for (int w = 0; w < M2W; w++) {
                    const uint32_t s = mrec[(size_t)(w + 1) * a.maxstart + r];
                    uni[w] = m == 0 ? s : (uni[w] | s);
                }
            }
            m++;
        };
        take(win);
        // every slot of the workgroup runs all M - 1 rounds (the barriers are the workgroup's); a slot whose round
        // found nothing is done
        bool done = false;
        for (int round = 1; round < M; round++) {
            __syncthreads();
            unsigned long long k = 0ull;
            if (!done && part == 0) {
                for (int r = tid; r < a.maxstart; r += T) {
                    const int s = (int)mrec[r];
                    uint32_t hit = 0u;
#pragma unroll
                    for (int w = 0; w < M2W; w++) hit |= mrec[(size_t)(w + 1) * a.maxstart + r] & uni[w];
                    const unsigned long long rk = (((unsigned long long)(uint32_t)(s + 0x40000000)) << 32) | (0xFFFFFFFFu - (uint32_t)r);
                    k = (s > 0 && hit == 0u && rk > k) ? rk : k;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                unsigned long long other = __shfl_xor(k, off, 64);
                k = other > k ? other : k;
            }
            if (wlane == 0) *red_key(wave) = k;
            __syncthreads();
            unsigned long long cur = *red_key(0);
            for (int w = 1; w < nwaves; w++) cur = *red_key(w) > cur ? *red_key(w) : cur;
            if (done || cur == 0ull) done = true;
            else take(cur);
        }
        if (lane_id == 0) {
            mx.counts[mrow] = m;
            for (int x = m; x < M; x++) {
                mx.scores[mrow * M + x] = 0;
                mx.restarts[mrow * M + x] = -1;
            }
        }
    }
