// sat_launch.hpp - which SA kernel instantiation a launch runs and with which workgroup (sat_launch.hip, the only
// translation unit that instantiates the SA kernels).  The rest of the library reaches the kernels through this header
// only: prepare_sa sizes and picks, launch_sa launches, launch_info names what ran.  Private, not part of the public
// interface; it knows nothing of the context beyond the SaLaunchState member defined here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <map>
#include <string>
#include <tuple>
#include <unordered_set>

#include "satabsearch.h"
#include "sat_sa_kernel.hpp"

// sets sat_last_error() text and returns `code`
int sat_fail(int code, const char *fmt, ...);

// a failed HIP call: sat_fail with its text, SAT_ENOMEM or SAT_EDEVICE
#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t err__ = (expr);                                                          \
        if (err__ != hipSuccess)                                                            \
            return sat_fail(err__ == hipErrorOutOfMemory ? SAT_ENOMEM : SAT_EDEVICE,        \
                            "%s failed: %s", #expr, hipGetErrorString(err__));              \
    } while (0)

// What the launch code keeps per context (sat_ctx::sa).
struct SaLaunchState {
    // launch-heuristic overrides (SAT_EXP_* in satabsearch_debug.h), read ONCE when the context is created
    int compact = -1, qlds = -1, lpc = -1, general = 0, epw = 0, lpc_waves = 0, chains = 0;
    size_t lds_pad = 0;
    // kernel instantiations whose dynamic-LDS limit has been raised on this device
    std::unordered_set<const void *> lds_attr_done;
    // entries per workgroup chosen for (instantiation, threads per entry, LDS bytes per entry): asked once
    std::map<std::tuple<const void *, int, size_t>, int> epw_choice;
};

// the padded order of the four query size classes
constexpr int kClassN1P[4] = { 16, 32, 64, 112 };

// The four kernel families (sat_sa_kernel.hpp): bit 0 = the match arguments, bit 1 = the pair arguments
enum SaMode { kPlain = 0, kMatch = 1, kPair = 2, kPairMatch = 3 };

// A chosen SA kernel: the instantiation's address and the template arguments it was instantiated with (opt = -1, wpl = 0:
// the general instantiation).  What is launched (launch_sa) and what sat_last_launch_info names (launch_info) both come
// from this one record.
struct SaKernel { const void *fn; int mode, n1p, m2w, cells; bool qlds; int opt, wpl; };

// The workgroup of one launch: restart chains (one per restart up to 256, fewer where the LDS would not fit them),
// lanes per chain, where the query cells live, whether the SA step compacts its work, and the LDS bytes of one
// entry slot.
struct WgShape { int chains, lpc_shift, threads; bool qlds, compact; size_t lds; };

// What a launch of the SA kernel needs beyond its work list: the workgroup, the kernel, the entry slots per workgroup
// (epw), the LDS bytes between two slots and of the whole workgroup, and the arguments with the shape fields filled
// (the caller adds the rest: the database and the options before prepare_sa, the work list, the queries and the slabs
// after).
struct SaLaunch { WgShape w; SaKernel k; int epw; size_t lds_stride, lds_launch; SatKernelArgs args; };

// The three calls a search makes (described where they are defined).  prepare_sa: the workgroup, the kernel and the
// entry slots per workgroup for queries of class c - the largest of n1max SSEs, `wpl` the map words per lane they share
// (0 = mixed) - and entries of up to n2max SSEs; it fills the shape fields of out.args and leaves the others alone.
int prepare_sa(SaLaunchState &st, int mode, int lorder, int lsoln, int plan_starts, int c, int n1max, int wpl, int n2max,
               long long work, bool pack, SaLaunch &out);
hipError_t launch_sa(const SaKernel &k, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const SatKernelArgs &a,
                     const SatPairArgs *px, const SatMatchArgs *mx);
std::string launch_info(const SaKernel &k, int items, int grid_x, int grid_y, int epw, int threads, size_t lds);

// Load the code object of the SA kernels on the current device (context creation: the first launch of a process
// would pay for it otherwise).
int sa_load_code(void);
