"""The flat pair walk of the initial full score (sat_sa_body.inc: FS_FLAT) deals a wave's matched pairs to its 64 lanes
in equal contiguous chunks; where a chunk starts and how a lane steps from pair to pair, row to row and chain to chain
is plain C++ shared by the kernel and the host (a section of csrc/sat_sa_kernel.hpp that a host compiler can take
alone).  tests/native/fs_chunks_check.cpp - a stand-alone program with its own main - walks whole waves with those
functions and checks that every pair is visited exactly once, in order, by the lane it was dealt to: no pairs at all,
a single pair, P = 63 / 64 / 65, one chain that holds every pair, 16 and 32 matched SSEs everywhere, and 2 000 random
waves drawn from the bench inputs' distribution of matched SSEs.  Built here with the address and undefined-behaviour sanitizers, by the C++ compiler that $CXX names
(g++ without it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda_satabsearch_amd", "csrc")


def test_chunk_walk_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "fs_chunks_check")
    build = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-I", CSRC, "-o", exe,
                            os.path.join(ROOT, "tests", "native", "fs_chunks_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert build.stderr == "", build.stderr                     # no warnings either
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok: 2020 waves, 0 failures"), run.stdout
