"""The polish of the best restarts' maps, CPU side (no GPU): the reference of tests/polish_lib.py (the pinned oracle's
move_delta under the rule of include/satabsearch.h) checked against full scores and a naive restatement of the
neighbourhood, the tie-break on hand-made pairs, what the polish is worth against twice the restarts, and the command
line's -P refusals."""
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import matches_lib
import oracle_lib
import polish_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")


def load_query(golden_dir, name, index=0):
    qs = sat.StructSet.read(os.path.join(golden_dir, name), "query", skip_header_lines=2)
    t, d = qs.dense(index)
    return t, d, qs.ssetypes(index)


@pytest.fixture(scope="module")
def small_db(golden_dir):
    return sat.StructSet.read(os.path.join(golden_dir, "tableauxdistmatrixdb.small.ascii"))


def assert_valid_map(pair, m, lorder):
    """injective, type consistent, and under LORDER order preserving"""
    img = [(i, int(j)) for i, j in enumerate(m[:pair.n1]) if j >= 0]
    assert (np.asarray(m[pair.n1:]) == -1).all()
    assert all(0 <= j < pair.n2 for _, j in img)
    assert len(set(j for _, j in img)) == len(img)
    assert all(pair.types2[j] == pair.qtypes[i] for i, j in img)
    if lorder:
        assert [j for _, j in img] == sorted(j for _, j in img)


@pytest.mark.parametrize("qfile,lorder,maxstart,tops,step", [
    ("d1ubia_.input", True, 128, 4, 41),
    ("d2phlb1.input", True, 128, 8, 37),
    ("d2phlb1.input", True, 16, 2, 53),
    ("d2phlb1_TFT.input", False, 128, 4, 43),
    ("d1twfa_.input", True, 32, 2, 97),
    ("d1twfa_.input", False, 32, 1, 131),
])
def test_polished_maps_are_local_optima_with_their_full_score(small_db, golden_dir, qfile, lorder, maxstart, tops, step):
    q = load_query(golden_dir, qfile)
    entries = np.arange(3, len(small_db), step)
    oscores, _, _ = oracle_lib.search(small_db, *q, lorder, False, maxstart, entries=entries)
    moved = 0
    for k, s in enumerate(entries):
        pair = polish_lib.Pair.of(small_db, int(s), q)
        score, base, restart, moves, m = polish_lib.polish_pair(small_db, int(s), q, lorder, maxstart, tops)
        assert base == oscores[k], f"entry {s}: base score"
        assert score >= base and 0 <= restart < maxstart and moves >= 0
        assert score == pair.full_score(m), f"entry {s}: the polished score is not the map's full score"
        assert_valid_map(pair, m, lorder)
        # the second, naive loop: every allowed move scored by two full scores
        assert max((d for d, _, _ in pair.naive_moves(m, lorder)), default=0) <= 0, f"entry {s}: an improving move is left"
        moved += moves > 0
    assert moved, "no sampled pair was moved by the polish"


def test_every_step_is_the_best_move_of_the_naive_neighbourhood(small_db, golden_dir):
    """Step by step: the reference's accepted move is the naive list's largest delta, smallest i, smallest j."""
    q = load_query(golden_dir, "d2phlb1.input")
    steps = 0
    for s, lorder in ((10, True), (200, True), (77, False), (431, False)):
        pair = polish_lib.Pair.of(small_db, s, q)
        sc, mp = matches_lib.restarts(small_db, s, q, lorder, 8)
        for r in range(8):
            m, score = mp[r].copy(), int(sc[r])
            final, moves, fm = pair.polish(m, score, lorder)
            for _ in range(moves):
                d, i, j = min(pair.naive_moves(m, lorder), key=lambda x: (-x[0], x[1], x[2]))
                assert d > 0
                m[i] = j
                score += d
                steps += 1
            assert score == final and np.array_equal(m[:pair.n1], fm[:pair.n1])
    assert steps >= 8


def flat_pair(n1, n2, code=0x00, dist=10.0):
    """every SSE of type 0, every cell the same code and distance: every placement of a pair scores 2"""
    qt = np.full((n1, n1), code, np.uint8)
    qd = np.full((n1, n1), dist, np.float32)
    np.fill_diagonal(qt, 0)
    np.fill_diagonal(qd, 0.0)
    t = np.full((n2, n2), code, np.uint8)
    d = np.full((n2, n2), dist, np.float32)
    np.fill_diagonal(t, 0)
    np.fill_diagonal(d, 0.0)
    return (qt, qd, np.zeros(n1, np.uint8)), t, d


@pytest.mark.parametrize("lorder", [True, False])
def test_ties_go_to_the_smallest_i_then_the_smallest_j(lorder):
    q, t, d = flat_pair(3, 4)
    pair = polish_lib.Pair(q, t, d, 4)
    # from [0, -1, -1] the six moves (1, 1..3), (2, 1..3) all gain 2: (1, 1) is taken, then (2, 2) gains 4
    score, moves, m = pair.polish(np.array([0, -1, -1], np.int32), 0, lorder)
    assert (score, moves, list(m[:3])) == (6, 2, [0, 1, 2])
    # from [-1, 2, -1] every move of SSE 0 or 2 to a free db SSE gains 2: (0, 0) wins; then SSE 2 gains 4 on db SSE 3 and,
    # with LORDER off, just as much on db SSE 1: the smaller j
    score, moves, m = pair.polish(np.array([-1, 2, -1], np.int32), 0, lorder)
    assert list(m[:3]) == ([0, 2, 3] if lorder else [0, 2, 1]) and (score, moves) == (6, 2)


def test_unmatching_wins_a_tie_against_a_new_image():
    """[0, 1] scores -2; unmatching SSE 0 and moving it to db SSE 2 (too far from everything: 0) both gain 2"""
    q, t, d = flat_pair(2, 3)
    t[0, 1] = t[1, 0] = 0x11                       # both nibbles differ from the query's 0x00, within 4 A: -2
    d[2, :2] = d[:2, 2] = 50.0
    pair = polish_lib.Pair(q, t, d, 3)
    assert pair.full_score([0, 1]) == -2
    gains = sorted(pair.naive_moves(np.array([0, 1], np.int32), False), key=lambda x: (-x[0], x[1], x[2]))
    assert gains[:2] == [(2, 0, -1), (2, 0, 2)]
    score, moves, m = pair.polish(np.array([0, 1], np.int32), -2, False)
    assert (score, moves, list(m[:2])) == (0, 1, [-1, 1])


def test_fewer_restarts_than_tops_uses_them_all(small_db, golden_dir):
    q = load_query(golden_dir, "d2phlb1.input")
    for s in (5, 300):
        sc, mp = matches_lib.restarts(small_db, s, q, True, 3)
        pair = polish_lib.Pair.of(small_db, s, q)
        got = polish_lib.polish_ranked(pair, sc, mp, True, 8)
        same = polish_lib.polish_ranked(pair, sc, mp, True, 3)
        assert got[:4] == same[:4] and np.array_equal(got[4], same[4])
        assert got[0] == max(pair.polish(mp[r], int(sc[r]), True)[0] for r in range(3)) and 0 <= got[2] < 3
        one = polish_lib.polish_ranked(pair, sc, mp, True, 1)
        assert one[2] == polish_lib.rank(sc)[0] and one[0] <= got[0]


# (job, LORDER, every step-th entry of the 586): the three jobs of DESIGN.md 6h, a few seconds together
QUALITY_JOBS = [("d2phlb1.input", True, 2), ("d2phlb1_TFT.input", False, 4), ("d1twfa_.input", True, 8)]


@pytest.mark.parametrize("qfile,lorder,step", QUALITY_JOBS)
def test_polishing_one_map_beats_twice_the_restarts(small_db, golden_dir, qfile, lorder, step):
    """Mean polished score with T = 1 at r = 128 >= mean plain score at r = 256 (the same streams continued): twice the
    search cost against a few percent.  DESIGN.md 6h gives the mean gains over plain r = 128 on these rows as 1.89 /
    1.45 / 2.96 (polish) against 0.85 / 1.03 / 0.92 (r = 256)."""
    q = load_query(golden_dir, qfile)
    polished, plain256, plain128 = [], [], []
    for s in range(0, len(small_db), step):
        sc, mp = matches_lib.restarts(small_db, s, q, lorder, 256)
        p = polish_lib.polish_ranked(polish_lib.Pair.of(small_db, s, q), sc[:128], mp[:128], lorder, 1)
        assert p[1] == sc[:128].max()
        polished.append(p[0])
        plain128.append(int(sc[:128].max()))
        plain256.append(int(sc.max()))
    print("%s: rows %d, mean gain over plain r=128: polish T=1 %.2f, plain r=256 %.2f" % (
        qfile, len(polished), np.mean(polished) - np.mean(plain128), np.mean(plain256) - np.mean(plain128)))
    assert np.mean(polished) >= np.mean(plain256)


# ---------------------------------------------------------------- command line
def run(golden_dir, args, stdin=b""):
    return subprocess.run([CLI] + args, input=stdin, cwd=golden_dir, capture_output=True)


def assert_refused_early(p, message):
    assert p.returncode == 1, p.stderr
    assert message in p.stderr, p.stderr
    assert p.stderr.count(b"ERROR:") == 1 and p.stdout == b""
    # nothing after the option checks ran: no banner, no device query
    assert b"MAXDIM" not in p.stderr and b"HIP device" not in p.stderr


def test_usage_lists_the_option(golden_dir):
    p = run(golden_dir, ["-x"])
    assert p.returncode == 1 and b"[-P T]" in p.stderr and b"  -P T : polish" in p.stderr


@pytest.mark.parametrize("args,message", [
    (["-c", "-P", "2", "-k", "5"], b"ERROR: -P needs the GPU path"),
    (["-P", "2", "-k", "5", "-m", "2"], b"ERROR: -P cannot be combined with -m"),
    (["-P", "2", "-k", "5", "-M", "2"], b"ERROR: -P cannot be combined with -M"),
    (["-P", "2", "-k", "5", "-p", "0.01"], b"ERROR: -P cannot be combined with -p"),
    (["-P", "2", "-k", "5", "-F", "0.1"], b"ERROR: -P cannot be combined with -F"),
    (["-P", "2", "-R", "512", "-k", "5", "-F", "0.1"], b"ERROR: -P cannot be combined with -F"),
    (["-P", "2"], b"ERROR: -P needs -k K"),
    (["-P", "2", "-C", "3", "-k", "5"], b"ERROR: -k K (5) exceeds -C C (3)"),
])
def test_cli_refusals(golden_dir, args, message):
    query = open(os.path.join(golden_dir, "d1ubia_.input"), "rb").read()
    assert_refused_early(run(golden_dir, args, query), message)


@pytest.mark.parametrize("arg", ["0", "9", "-1", "x", "2x", ""])
def test_cli_rejects_tops_outside_1_to_8(golden_dir, arg):
    p = run(golden_dir, ["-k", "5", "-P", arg])
    assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""
    assert ("ERROR: -P needs an integer 1..8 (got '%s')" % arg).encode() in p.stderr


def test_candidates_without_polish_still_need_refine(golden_dir):
    assert_refused_early(run(golden_dir, ["-C", "40", "-k", "5"]), b"ERROR: -C needs -R")
