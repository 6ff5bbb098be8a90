"""Several matches per entry, CPU side (no GPU): the single-chain reference (tests/native/chain_oracle.c) pinned to
the pinned oracle, the greedy selection on a planted repeat, and the command line's refusal of -m in host mode."""
import os
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import matches_lib
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")


def load_query(golden_dir, name, index=0):
    qs = sat.StructSet.read(os.path.join(golden_dir, name), "query", skip_header_lines=2)
    t, d = qs.dense(index)
    return t, d, qs.ssetypes(index)


@pytest.fixture(scope="module")
def small_db(golden_dir):
    return sat.StructSet.read(os.path.join(golden_dir, "tableauxdistmatrixdb.small.ascii"))


@pytest.mark.parametrize("qfile,lorder,maxstart,step", [
    ("d1ubia_.input", True, 128, 9),
    ("d2phlb1.input", True, 1, 5),
    ("d2phlb1.input", True, 7, 5),
    ("d2phlb1.input", True, 128, 11),
    ("d2phlb1.input", False, 7, 7),
    ("d2phlb1.input", False, 128, 17),
    ("d1twfa_.input", True, 7, 23),
])
def test_chain_oracle_argmax_is_the_oracles_search(small_db, golden_dir, qfile, lorder, maxstart, step):
    """max_r (s_r, -r) of the per-restart own bests is sa_oracle_search's score, and map_r of that restart its LSOLN map."""
    q = load_query(golden_dir, qfile)
    entries = np.arange(0, len(small_db), step)
    oscores, omaps, _ = oracle_lib.search(small_db, *q, lorder, True, maxstart, entries=entries)
    for k, s in enumerate(entries):
        sc, mp = matches_lib.restarts(small_db, int(s), q, lorder, maxstart)
        best = int(np.lexsort((np.arange(maxstart), -sc.astype(np.int64)))[0])
        assert sc[best] == oscores[k], f"entry {s}"
        assert np.array_equal(mp[best], omaps[k]), f"map of entry {s}"


def planted_repeat(seed=5):
    """An 8-SSE query and one entry holding two perturbed copies of it one after the other (SSEs 0..7 and 8..15,
    the copies 40 A apart), plus the query's plain source as a second entry."""
    rng = np.random.default_rng(seed)
    qt, qd, qtypes = sat.synth.make_query(8, seed=seed)
    n = 16
    t = np.zeros((n, n), np.uint8)
    d = np.zeros((n, n), np.float32)
    t[:] = rng.choice(np.unique(qt[np.triu_indices(8, 1)]), size=(n, n))
    t = np.tril(t, -1)
    t = t + t.T
    d[:] = rng.uniform(35.0, 60.0, size=(n, n)).astype(np.float32)
    d = np.tril(d, -1)
    d = d + d.T
    for c in (0, 8):
        noise = np.tril(rng.uniform(-0.5, 0.5, size=(8, 8)).astype(np.float32), -1)
        t[c:c + 8, c:c + 8] = qt
        d[c:c + 8, c:c + 8] = np.abs(qd + noise + noise.T)
    idx = np.arange(n)
    t[idx, idx] = np.concatenate([qtypes, qtypes])
    d[idx, idx] = t[idx, idx].astype(np.float32)
    pitch = n
    tabs = np.zeros((2, pitch, pitch), np.uint8)
    dmats = np.zeros((2, pitch, pitch), np.float32)
    tabs[0], dmats[0] = t, d
    tabs[1, :8, :8], dmats[1, :8, :8] = qt, qd
    db = sat.StructSet.from_dense(np.array([n, 8], np.int32), tabs, dmats)
    return db, (qt, qd, qtypes)


def test_planted_repeat_gives_both_copies():
    db, q = planted_repeat()
    count, scores, restarts, maps = matches_lib.matches(db, 0, q, True, 128, 2)
    assert count == 2
    sets = [set(int(j) for j in maps[m] if j >= 0) for m in range(2)]
    assert sets[0].isdisjoint(sets[1])
    # one match in each copy, each scoring most of what the query scores against itself
    assert sorted(min(s) // 8 for s in sets) == [0, 1] and all(max(s) // 8 == min(s) // 8 for s in sets)
    self_score = oracle_lib.search(db, *q, True, False, 128, entries=[1])[0][0]
    assert scores[1] >= 0.7 * self_score and scores[0] >= scores[1] > 0
    # M = 1 is the plain search; the single copy of entry 1 gives one match only
    assert matches_lib.matches(db, 0, q, True, 128, 1)[0] == 1
    c1, s1, r1, m1 = matches_lib.matches(db, 1, q, True, 128, 4)
    assert c1 == 1 and list(s1[1:]) == [0, 0, 0] and list(r1[1:]) == [-1, -1, -1] and (m1[1:] == -1).all()


def test_select_matches_rule():
    maps = np.full((5, 111), -1, np.int32)
    maps[0, :3] = [0, 1, 2]
    maps[1, :3] = [3, 4, 5]
    maps[2, :3] = [2, 6, 7]     # overlaps restart 0
    maps[3, :2] = [8, 9]
    maps[4, :2] = [10, 11]
    scores = np.array([10, 9, 9, 0, 9], np.int32)
    count, s, r, m = matches_lib.select_matches(scores, maps, 8)
    assert count == 3 and list(r[:3]) == [0, 1, 4] and list(s[:3]) == [10, 9, 9]      # ties: lowest restart first
    assert list(r[3:]) == [-1] * 5 and list(s[3:]) == [0] * 5
    assert matches_lib.select_matches(np.array([-3, -5], np.int32), maps[:2], 4)[0] == 1


def test_cli_refuses_matches_in_host_mode(golden_dir):
    p = subprocess.run([CLI, "-c", "-m", "2"], input=open(os.path.join(golden_dir, "d1ubia_.input"), "rb").read(),
                       cwd=golden_dir, capture_output=True)
    assert p.returncode == 1
    assert b"ERROR: -m needs the GPU path" in p.stderr


@pytest.mark.parametrize("arg", ["0", "9", "-1", "x", "2x", ""])
def test_cli_rejects_match_counts_outside_1_to_8(golden_dir, arg):
    p = subprocess.run([CLI, "-m", arg], input=b"", cwd=golden_dir, capture_output=True)
    assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""
