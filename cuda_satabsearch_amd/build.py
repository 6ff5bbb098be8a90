"""Build the native pieces of cuda_satabsearch_amd in-tree.

    python -m cuda_satabsearch_amd.build [--oracle] [--ref]

* libsatabsearch.so   HIP kernels + C ABI (include/satabsearch.h), hipcc --offload-arch=gfx950
* libsathost.so       host-only C: ASCII reader, Gumbel statistics, shard cuts, cluster tables, AUC / ROC-n, greedy cover, profile core, map order, exact-search twin, reach keys (csrc/host/)
* bin/satabsearch     the command line (csrc/host/sat_main.c), links both

`--oracle` additionally runs oracle/Makefile (test infrastructure, never linked into
the product), `--ref` also its `ref` target when /root/reference is mounted.
hipcc cross-compiles gfx950 code objects without a GPU present.
"""
import os
import re
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
HOST = os.path.join(CSRC, "host")
INC = os.path.join(ROOT, "include")

HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CC = os.environ.get("CC") or "gcc"


def _run(cmd):
    print("+", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


# The device library's translation units, sat_launch.hip (every SA kernel instantiation: minutes) first.  The one list
# of them: the library, its diagnostic twin, the Makefile and scripts/exp/variant_lib.sh all build from it.
DEVICE_SOURCES = ("sat_launch.hip", "sat_capi.hip", "sat_pairs.hip", "sat_db.hip", "sat_topk.hip", "sat_multi.hip",
                  "sat_polish.hip", "sat_qfromdb.hip", "sat_cluster.hip", "sat_eval.hip", "sat_cover.hip", "sat_profile.hip",
                  "sat_reorder.hip", "sat_exact.hip", "sat_reach.hip")
# sat_launch.hip and what it includes from csrc/ (diag/ apart, which only -DSAT_DIAG builds read)
KERNEL_SOURCES = ("sat_sa_kernel.hpp", "sat_sa_body.inc", "sat_launch.hpp", "sat_launch.hip")
HIPFLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fPIC", "-I", INC, "-I", CSRC]
# (library, directory of its objects, flags beyond HIPFLAGS).  The twin is the device library once more with the
# reference's TESTING assertion compiled in (diag/sat_diag.hpp, -DSAT_DIAG_SELFCHECK: every proposed move's score against
# a full recomputation) - loaded only by tests/test_gpu_parity.py::test_every_move_passes_the_references_self_check,
# through SAT_DEVICE_LIB
DEVICE_LIB = (os.path.join(PKG, "libsatabsearch.so"), os.path.join(PKG, "obj", "lib"), [])
SELFCHECK_LIB = (os.path.join(ROOT, "tests", "native", "libsat_selfcheck.so"), os.path.join(PKG, "obj", "selfcheck"),
                 ["-DSAT_DIAG", "-DSAT_DIAG_SELFCHECK"])
# ... and once more with the initial full score's flat pair walk compiled out (-DSAT_FS_FLAT=0: the team walk it replaced):
# tests/test_gpu_flat_walk.py asks both builds for the same bytes, and A/B runs load it through SAT_DEVICE_LIB
TEAMWALK_LIB = (os.path.join(ROOT, "tests", "native", "libsat_teamwalk.so"), os.path.join(PKG, "obj", "teamwalk"),
                ["-DSAT_FS_FLAT=0"])
JOBS = 16       # compile commands running at once, all libraries together


def kernel_source_hash():
    """sha256 over the sources of the SA kernels and of the code that picks one and sizes its workgroup - the translation
    unit sat_launch.hip: profiles/bench_traffic.json carries it, so that bench.py only reports committed counter figures
    that were measured on the kernel it is running."""
    import hashlib
    h = hashlib.sha256()
    for f in KERNEL_SOURCES:
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def include_closure(src):
    """`src` and every file it reaches through #include "..." lines (the conditional ones too), each looked up beside
    the including file, then in csrc/ and include/"""
    seen, todo = [], [src]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.append(f)
        with open(f) as fh:
            names = re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', fh.read(), re.M)
        for name in names:
            hits = [p for p in (os.path.normpath(os.path.join(d, name)) for d in (os.path.dirname(f), CSRC, INC)) if os.path.exists(p)]
            todo += hits[:1]
    return seen


def build_host(force=False):
    out = os.path.join(PKG, "libsathost.so")
    srcs = [os.path.join(HOST, f) for f in ("sat_parse.c", "sat_gumbel.c", "sat_shard.c", "sat_cluster.c", "sat_eval.c", "sat_cover.c",
                                            "sat_profile.c", "sat_reorder.c", "sat_exact.c", "sat_reach.c")]
    deps = srcs + [os.path.join(HOST, f) for f in ("sat_parse.h", "sat_gumbel.h", "sat_stats.h", "sat_shard.h", "sat_cluster.h", "sat_eval.h",
                                                "sat_cover.h", "sat_profile.h", "sat_reorder.h", "sat_exact.h", "sat_reach.h")]
    if force or _stale(out, deps):
        _run([CC, "-O2", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", HOST, "-o", out] + srcs + ["-lm", "-lpthread"])
    return out


def _host_objects(force=False):
    """plain-C host pieces linked into the device library (and its diagnostic twin): the Gumbel statistics (the
    context tabulates them with the host libm for the device-side best-k rows), the shard cost model and the join of the
    shards' cluster labels, the reduction of the shards' summed evaluation tables, the cover's table and its plain-C
    restatement, the join and the rows of the shards' reach arrays"""
    host_c = [os.path.join(HOST, "sat_gumbel.c"), os.path.join(HOST, "sat_shard.c"), os.path.join(HOST, "sat_cluster.c"),
              os.path.join(HOST, "sat_eval.c"), os.path.join(HOST, "sat_cover.c"), os.path.join(HOST, "sat_reach.c")]
    host_o = [os.path.join(PKG, "sat_gumbel.o"), os.path.join(PKG, "sat_shard.o"), os.path.join(PKG, "sat_cluster.o"),
              os.path.join(PKG, "sat_eval.o"), os.path.join(PKG, "sat_cover.o"), os.path.join(PKG, "sat_reach.o")]
    for c, o in zip(host_c, host_o):
        if force or _stale(o, [c] + [os.path.join(HOST, h) for h in ("sat_gumbel.h", "sat_stats.h", "sat_shard.h", "sat_cluster.h", "sat_eval.h",
                                                                      "sat_cover.h", "sat_reach.h")]):
            _run([CC, "-O2", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-I", HOST, "-c", "-o", o, c])
    return host_o


def build_device_libs(libs, force=False):
    """Each (library, object directory, flags) of `libs` from DEVICE_SOURCES: every translation unit to an object of its
    own, re-made only when it or a file it includes is newer, all of them side by side; then the link.  A library newer
    than everything it is made from is left alone, objects or not."""
    host_c = [os.path.join(HOST, f) for f in ("sat_gumbel.c", "sat_shard.c", "sat_cluster.c", "sat_eval.c", "sat_cover.c",
                                              "sat_reach.c", "sat_gumbel.h", "sat_stats.h", "sat_shard.h", "sat_cluster.h",
                                              "sat_eval.h", "sat_cover.h", "sat_reach.h")]
    srcs = [os.path.join(CSRC, f) for f in DEVICE_SOURCES]
    deps = [include_closure(src) for src in srcs]
    todo = [lib for lib in libs if force or _stale(lib[0], host_c + sum(deps, []))]
    if not todo:
        return
    host_o = _host_objects(force)
    compiles = []
    for out, objdir, flags in todo:
        os.makedirs(objdir, exist_ok=True)
    for src, dep in zip(srcs, deps):
        for out, objdir, flags in todo:
            obj = os.path.join(objdir, os.path.splitext(os.path.basename(src))[0] + ".o")
            if force or _stale(obj, dep):
                compiles.append([HIPCC] + HIPFLAGS + flags + ["-c", "-o", obj, src])
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(JOBS) as ex:
        list(ex.map(_run, compiles))
    for out, objdir, flags in todo:
        objs = [os.path.join(objdir, os.path.splitext(f)[0] + ".o") for f in DEVICE_SOURCES]
        # -Wl,: hipcc would compile a bare .o as HIP source.  librccl is NOT linked: sat_multi.hip loads it on demand
        _run([HIPCC, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", out] + ["-Wl," + o for o in objs + host_o] + ["-lm", "-ldl"])


def build_device(force=False):
    build_device_libs([DEVICE_LIB], force)
    return DEVICE_LIB[0]


def build_cli(force=False):
    src = os.path.join(HOST, "sat_main.c")
    if not os.path.exists(src):
        return None
    bindir = os.path.join(PKG, "bin")
    os.makedirs(bindir, exist_ok=True)
    out = os.path.join(bindir, "satabsearch")
    host_search = os.path.join(HOST, "sat_host_search.c")
    deps = [src, host_search, os.path.join(HOST, "sat_host_search.h"), os.path.join(HOST, "sat_cluster.h"),
            os.path.join(HOST, "sat_cover.h"), os.path.join(HOST, "sat_profile.h"), os.path.join(HOST, "sat_reorder.h"),
            os.path.join(PKG, "libsatabsearch.so"), os.path.join(PKG, "libsathost.so")]
    if force or _stale(out, deps):
        # -O3 without fast-math or fma contraction: the host mode must round like the reference's
        _run([CC, "-O3", "-ffp-contract=off", "-Wall", "-Wextra", "-I", INC, "-I", HOST, "-o", out, src, host_search,
              "-L", PKG, "-lsatabsearch", "-lsathost", "-lm", "-Wl,-rpath,$ORIGIN/.."])
    return out


def build_test_native(force=False, twin=True):
    """tests/native/*.hip: GPU-side TEST helpers (e.g. the rocRAND device API beside the kernel's own
    Philox block) and (twin) the device library's diagnostic twin.  Test infrastructure like oracle/: never loaded by
    the product."""
    tdir = os.path.join(ROOT, "tests", "native")
    src = os.path.join(tdir, "rocrand_check.hip")
    if not os.path.exists(src):
        return None
    out = os.path.join(tdir, "librocrand_check.so")
    if force or _stale(out, [src, os.path.join(CSRC, "sat_sa_kernel.hpp"), os.path.join(CSRC, "sat_sa_body.inc")]):
        _run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", INC, "-I", CSRC, "-o", out, src])
    if twin:
        build_device_libs([SELFCHECK_LIB], force)
    src2, out2 = os.path.join(tdir, "lds_residency.hip"), os.path.join(tdir, "liblds_residency.so")
    if os.path.exists(src2) and (force or _stale(out2, [src2])):
        _run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out2, src2])
    # the caller's side of a stream (tests/stream_lib.py)
    src3, out3 = os.path.join(tdir, "stream_probe.hip"), os.path.join(tdir, "libstream_probe.so")
    if os.path.exists(src3) and (force or _stale(out3, [src3])):
        _run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out3, src3])
    return out


def build_oracle(ref=False):
    odir = os.path.join(ROOT, "oracle")
    _run(["make", "-s", "-C", odir, "all"])
    if ref and os.path.isdir("/root/reference/nvcc_src_current"):
        _run(["make", "-s", "-C", odir, "ref"])


def build_all(force=False, oracle=False, ref=False):
    build_host(force)
    if oracle:
        # the device library and its twins: their translation units compile side by side
        build_device_libs([DEVICE_LIB, SELFCHECK_LIB, TEAMWALK_LIB], force)
        build_test_native(force, twin=False)
        build_cli(force)
        build_oracle(ref)
    else:
        build_device(force)
        build_cli(force)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv, oracle="--oracle" in sys.argv or "--ref" in sys.argv,
              ref="--ref" in sys.argv)
