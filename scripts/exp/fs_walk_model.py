"""VALU instructions of the initial full score's pair walk on the bench inputs, per wave, under three schedules:
    python scripts/exp/fs_walk_model.py [ENTRIES] > profiles/r06_logs/fs_walk_model.txt
  (a) the team walk of DESIGN §4 (25): two lanes share the rows of their two chains, the wave pays every row trip
      for its busiest team and every inner trip for its longest row;
  (b) the flat walk of §4 (32): the wave's matched pairs in one order (chain, row, partner), dealt to the lanes in
      contiguous chunks of q = ceil(P / 64), one flat loop of ceil(q / 2) trips behind a seek;
  (c) the ideal: sum of pairs / 64 at the single-pair price, nothing else.
No GPU: thinit's initial maps are rebuilt from the kernel's Philox streams (the oracle's Philox block through
tests/oracle_lib.py: key = seed, counter = (block, 0, db ordinal, restart), block i >> 2 word i & 3 decides query SSE i),
for the 32-SSE bench query against the first ENTRIES (default 48) entries of the bench database, r = 128; a wave is
restarts 0-63 or 64-127 of one entry.  The per-block instruction counts are read off the assembly of the bench
instantiation (scripts/exp/isa_one.sh) and stand below as constants: the dynamic trip counts are what is modelled."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (a) team walk, <32,1,false,1,4,0> built with -DSAT_FS_FLAT=0: set-up (two shuffles, the merged order), one row
# trip (strip to the row, its sets and bases, the inner loop's first test, the sums behind it), one inner trip of two
# pairs with its test, hand-back
TEAM = dict(setup=29, row=45 + 2 + 6, inner=47 + 2, tail=5)
# (b) flat walk, same instantiation: scan + deal + chain search (fixed), one trip of the row seek, one trip of the
# partner seek, one trip of two pairs (pops, cells, terms, row and chain advance by selects), read-back
FLAT = dict(fixed=60 + 6, row_seek=9, partner_seek=8, trip=71 + 22, tail=2)
PAIR = 24.5            # (c): one pair of the team walk's inner trip


def initial_maps(qtypes, dtypes, ordinal, restarts, seed=1234):
    """thinit (sat_sa_body.inc): (mapped, occ) bit sets of every restart's initial map."""
    import oracle_lib
    n1, n2 = len(qtypes), len(dtypes)
    out = []
    for r in range(restarts):
        mapped = occ = 0
        j = 0
        for i0 in range(0, n1, 4):
            blk = oracle_lib.philox4x32_10((i0 >> 2, 0, ordinal, r), (seed & 0xFFFFFFFF, seed >> 32))
            stop = False
            for s in range(4):
                i = i0 + s
                if i >= n1 or blk[s] >= 0x7FFFFFC0:
                    continue
                jj = next((x for x in range(j, n2) if dtypes[x] == qtypes[i]), -1)
                if jj < 0:
                    stop = True
                    break
                mapped |= 1 << i
                occ |= 1 << jj
                j = jj + 1
            if stop:
                break
        out.append((mapped, occ))
    return out


def team_cost(ms):
    """ms: matched SSEs of the wave's 64 chains, lane order."""
    rows_of = []                  # per lane: the row lengths it meets, trip by trip
    for t in range(32):
        c0, c1 = ms[2 * t], ms[2 * t + 1]
        rb, rs = max(max(c0, c1) - 1, 0), max(min(c0, c1) - 1, 0)
        dlead, etot = rb - rs, rb + rs
        for pl in (0, 1):
            lens = []
            for e in range(pl, etot, 2):
                e2 = e - dlead
                lens.append(rb - e if e2 < 0 else rs - (e2 >> 1))
            rows_of.append(lens)
    row_trips = max(len(l) for l in rows_of)
    inner = 0
    for t in range(row_trips):
        inner += max((-(-l[t] // 2) for l in rows_of if t < len(l)), default=0)
    return TEAM["setup"] + row_trips * TEAM["row"] + inner * TEAM["inner"] + TEAM["tail"], row_trips, inner


def flat_cost(ms):
    ps = [m * (m - 1) // 2 for m in ms]
    P = sum(ps)
    q = -(-P // 64)
    trips = -(-q // 2)
    # the seeks loop to the wave's deepest start: rows below the chunk's first row, partners below its first partner
    row_seek = partner_seek = 0
    starts = np.concatenate([[0], np.cumsum(ps)])
    for t in range(64):
        g = t * q
        if g >= P:
            break
        c = int(np.searchsorted(starts, g, side="right")) - 1
        off, m, a = g - int(starts[c]), ms[c], 0
        while off >= m - 1 - a:
            off -= m - 1 - a
            a += 1
        row_seek, partner_seek = max(row_seek, a), max(partner_seek, off)
    cost = FLAT["fixed"] + row_seek * FLAT["row_seek"] + partner_seek * FLAT["partner_seek"] + trips * FLAT["trip"] + FLAT["tail"]
    return cost, P, trips, row_seek, partner_seek


def main():
    import cuda_satabsearch_amd as sat
    entries = int(sys.argv[1]) if len(sys.argv) > 1 else 48
    q = sat.synth.make_query(32)
    db = sat.synth.make_db(entries, 32, 32, total=125_000)
    qtypes = [int(t) & 3 for t in q[2]]
    rows = []
    mall = []
    for e in range(entries):
        dtypes = [int(t) & 3 for t in db.ssetypes(e)]
        maps = initial_maps(qtypes, dtypes, e, 128)
        for w in range(2):
            ms = [bin(m).count("1") for m, _ in maps[64 * w:64 * w + 64]]
            mall += ms
            a, row_trips, inner = team_cost(ms)
            b, P, trips, rseek, pseek = flat_cost(ms)
            rows.append((a, b, P / 64 * PAIR, P, row_trips, inner, trips, rseek, pseek, max(ms)))
    r = np.array(rows, dtype=np.float64)
    mall = np.array(mall)
    print(f"bench inputs: 32-SSE query x first {entries} entries, r = 128: {len(rows)} waves, {len(mall)} chains")
    print(f"matched SSEs per chain m = {mall.mean():.2f} +- {mall.std():.2f} (max {mall.max()}), pairs per chain {np.mean(mall * (mall - 1) / 2):.1f}")
    print("chains by m = 0, 1, ...:", " ".join(str(int(x)) for x in np.bincount(mall)))
    print(f"pairs per wave P = {r[:, 3].mean():.0f} +- {r[:, 3].std():.0f}, busiest chain of a wave m = {r[:, 9].mean():.1f}")
    print(f"team walk: row trips {r[:, 4].mean():.1f}, inner trips {r[:, 5].mean():.1f} per wave")
    print(f"flat walk: trips {r[:, 6].mean():.1f}, row-seek trips {r[:, 7].mean():.1f}, partner-seek trips {r[:, 8].mean():.1f} per wave")
    print("block counts (VALU): team", TEAM, " flat", FLAT, " ideal pair", PAIR)
    print("| schedule | VALU per wave (mean) | min | max |")
    print("|---|---|---|---|")
    for k, name in enumerate(("(a) team walk", "(b) flat walk", "(c) ideal, sum of pairs / 64")):
        print(f"| {name} | {r[:, k].mean():.0f} | {r[:, k].min():.0f} | {r[:, k].max():.0f} |")
    print(f"(a) - (b) = {r[:, 0].mean() - r[:, 1].mean():.0f} VALU per wave (go on only at 500 or more)")


if __name__ == "__main__":
    main()
