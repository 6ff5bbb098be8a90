"""Resident entries per CU of the LORDER launches with one-word db sets, with and without the pick's rank table
(sat_sa_kernel.hpp: qbase, pos):
    python scripts/exp/lds_sweep.py
Slot sizes from the library's own carve (sat_debug_lds_layout; "without" = the same carve with the leader key right
behind qmask), the choice of entries per workgroup as pick_epw makes it (sat_launch.hip) - LDS granules of 1280 bytes, 128
per CU, k x threads <= 512, k > 1 only with a multiple of 4 waves - with the register file's limit taken as 6 waves
per SIMD (SAT_FAST_WAVES) instead of the occupancy call, so it runs without a GPU.  Prints every (chains, n1, n2) whose
resident entries change."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from cuda_satabsearch_amd import _native


def resident(threads, stride):
    best = 0
    k = 1
    while k * threads <= 512 and k * stride <= 160 * 1024:
        waves = k * threads // 64
        if k == 1 or waves % 4 == 0:
            by_regs = 24 // waves
            by_lds = 128 // ((k * stride + 1279) // 1280)
            best = max(best, min(by_regs, by_lds) * k)
        k += 1
    return best


def main():
    lib = _native.device_lib()
    out = (ctypes.c_uint32 * 14)()
    lost = {}
    shapes = 0
    for chains in (64, 128, 256):
        for n1 in range(1, 33):
            n1p = 16 if n1 <= 16 else 32
            for n2 in range(1, 33):
                lib.sat_debug_lds_layout(1 | 1 << 16, n1, n1p, n2, chains, chains, int(n1p < 32), 1, out)
                total, leader, qbase = out[10], out[6], out[12]
                old_total = total - (leader - (qbase + 7) // 8 * 8)
                new, old = resident(chains, (total + 15) // 16 * 16), resident(chains, (old_total + 15) // 16 * 16)
                shapes += 1
                if new != old:
                    lost.setdefault((chains, old, new), []).append((n1, n2))
    print("%d shapes, %d change" % (shapes, sum(len(v) for v in lost.values())))
    for (chains, old, new), v in sorted(lost.items()):
        print("chains %3d: %2d -> %2d entries per CU at (n1, n2) = %s" % (chains, old, new, " ".join("%dx%d" % s for s in v)))


if __name__ == "__main__":
    main()
