"""The LDS carve of the rank table of the LORDER pick (sat_sa_kernel.hpp: lds_layout, qbase and pos; launches with
one-word db sets): where the three per-slot arrays behind the query types lie, that what follows them keeps its
alignment, and that the bench shape's slot still pairs up in 21 LDS granules."""
import ctypes

from cuda_satabsearch_amd import _native

MORE = 1 << 16          # sat_debug_lds_layout: 14 words, out[11..13] = qmask, qbase, pos
GRANULE = 1280


def layout(m2w, n1, n1p, n2, chains, threads, qlds, compact):
    out = (ctypes.c_uint32 * 14)()
    _native.device_lib().sat_debug_lds_layout(m2w | MORE, n1, n1p, n2, chains, threads, qlds, compact, out)
    names = ("code", "qdist", "qcode", "smap", "tmask", "qtypes", "leader", "red", "red_stride", "items", "total",
             "qmask", "qbase", "pos")
    return dict(zip(names, out))


def test_pick_table_offsets_and_alignment():
    """one-word sets: qmask (dwords, 4-byte aligned), then a byte per query SSE, then 33+ bytes of table - the most a
    step reads is byte 32 - and the 64-bit leader key behind them on an 8-byte boundary; wider sets carry none of the
    three.  The offsets do not depend on the entry's order beyond the cells in front (a slot sized for the launch's
    largest entry holds every entry's table)."""
    for n1p, n1s in ((16, (1, 7, 16)), (32, (17, 30, 32)), (64, (33, 64)), (112, (65, 111))):
        for n1 in n1s:
            for chains in (64, 128, 192, 256):
                for qlds in (0, 1):
                    for compact in (0, 1):
                        for n2 in (1, 2, 5, 17, 31, 32):
                            L = layout(1, n1, n1p, n2, chains, chains, qlds, compact)
                            assert L["qmask"] % 4 == 0 and L["qmask"] >= L["qtypes"] + n1p
                            assert L["qbase"] == L["qmask"] + 4 * n1p
                            assert L["pos"] == L["qbase"] + n1p
                            assert L["leader"] >= L["pos"] + 33 and L["leader"] - L["pos"] < 33 + 8 + 3
                            assert L["leader"] % 8 == 0 and L["red"] % 8 == 0 and L["items"] % 4 == 0
                            assert L["leader"] + 8 <= L["red"] <= L["total"]
                        for m2w, n2 in ((2, 33), (2, 64), (4, 65), (4, 111)):
                            L = layout(m2w, n1, n1p, n2, chains, chains, qlds, compact)
                            assert L["qmask"] == L["qbase"] == L["pos"]
                            assert L["leader"] == (L["pos"] + 7) // 8 * 8


def test_bench_slot_still_pairs_in_21_granules():
    """32-SSE query x 32-SSE entries, 128 chains, query cells through L1, compacted: the slot was 13 272 bytes and two
    of them share a workgroup of 21 granules - at most 13 440 bytes each"""
    L = layout(1, 32, 32, 32, 128, 128, 0, 1)
    assert L["total"] <= 13440
    stride = (L["total"] + 15) // 16 * 16
    assert (2 * stride + GRANULE - 1) // GRANULE <= 21
