"""tests/history_lib.py without a GPU: the schedules cover what tests/test_gpu_history.py says they cover, the model
follows a hand-written table of the state each call drops, and the references are not vacuous - every world a kind is
used with shows, on the CPU reference alone, a cutoff that is neither empty nor everything, a polish that moves a map and
one whose winner is not the best restart, an entry with several matches and one with fewer than asked for, a cluster edge
with at least two components, and a query the fit fits."""
import collections
import time

import numpy as np
import pytest

import history_lib as hl

ALL_DIMENSIONS = ("entries", "queries", "n1", "n2", "pairs", "m", "tops", "k", "nodes")


def sequences():
    """every sequence of operations the GPU module runs, as (multi, ops)"""
    out = [(False, w) for w in hl.schedule(hl.SEED)] + [(True, w) for w in hl.schedule(hl.SEED, True)]
    out += [(False, hl.grow_shrink_grow(k)) for k in hl.DATA_KINDS]
    out += [(True, hl.grow_shrink_grow(k, True)) for k in hl.DATA_KINDS if k in hl.MULTI_KINDS]
    return out + [(True, hl.shard_sequence())]


# ---------------------------------------------------------------- the schedules
@pytest.mark.parametrize("multi,count", [(False, hl.WALKS), (True, hl.MULTI_WALKS)], ids=["one_context", "shards"])
def test_schedule_covers_every_allowed_pair(multi, count):
    walks = hl.schedule(hl.SEED, multi)
    kinds = hl.MULTI_KINDS if multi else hl.KINDS
    assert len(walks) == count and all(hl.WALK_STEPS <= len(w) <= hl.WALK_STEPS + 5 for w in walks)
    followed = set()
    for walk in walks:
        m = hl.Model(multi)
        for o in walk:
            assert m.legal(o.kind), o
            m.apply(o)
        followed |= set(zip([o.kind for o in walk], [o.kind for o in walk][1:]))
    allowed = hl.allowed_pairs(multi)
    assert followed == allowed, sorted(allowed - followed)[:10]
    # the model allows something after every kind, forbids something (results before any search, ...), and every kind occurs
    assert {a for a, _ in allowed} == set(kinds) and len(allowed) < len(kinds) ** 2
    assert ("upload", "hits_cutoff") not in allowed and ("search", "hits_cutoff") in allowed
    if not multi:
        assert ("search_pairs_polish", "results_base") in allowed and ("search_matches", "results_base") not in allowed
    assert ("upload", "cluster_labels") not in allowed and ("set_queries", "cluster_labels") in allowed
    # the same seed gives the same walks: the schedule is code, not data
    hl._cache.pop(("schedule", hl.SEED, multi))
    assert hl.schedule(hl.SEED, multi) == walks


def test_every_dimension_rises_and_falls_twice_on_one_context():
    best = collections.defaultdict(lambda: (0, 0))
    for walk in hl.schedule(hl.SEED):
        for name, (up, down) in hl.rises_and_falls(walk).items():
            if min(up, down) > min(best[name]):
                best[name] = (up, down)
    for name in ALL_DIMENSIONS:
        assert min(best[name]) >= 2, "%s rises and falls %s times at best" % (name, best[name])


def test_walks_refuse_what_an_earlier_search_left_behind():
    """the refusals that depend on history: a plain search while the base scores of an earlier polished one are still on
    the device, a search without LSOLN while an earlier one's maps are - each with no upload or query change between"""
    found = collections.Counter()
    for walk in hl.schedule(hl.SEED):
        m, base, maps, need = hl.Model(), False, False, 0
        for o in walk:
            m.apply(o)
            if o.kind in ("search", "search_async_results", "upload_search") and m.searched.lsoln:
                now = len(hl.db(m.db)) * sum(hl.n1s_of(m.batch))
                found["a larger map buffer behind a smaller one"] += 0 < need < now
                need = max(need, now)
            if m.searched is None:
                base = maps = False
                continue
            found["plain after polished"] += base and not m.searched.tops
            found["no maps after maps"] += maps and not m.searched.lsoln
            base, maps = base or m.searched.tops > 0, maps or m.searched.lsoln
    assert found["plain after polished"] >= 3 and found["no maps after maps"] >= 3, found
    assert found["a larger map buffer behind a smaller one"] >= 3, found      # d_ssemaps moves under live descriptors


def test_grow_shrink_grow_differs_in_every_dimension():
    for kind in hl.DATA_KINDS:
        ops, m, seen = hl.grow_shrink_grow(kind), hl.Model(), []
        for o in ops:
            assert m.legal(o.kind), (kind, o)
            m.apply(o)
            if o.kind == kind:
                seen.append((hl.dimensions(o, m), dict(o.args)))
        assert len(seen) == 3, kind
        (big, big_args), (small, _), (again, again_args) = seen
        assert big == again and big_args == again_args, kind
        for name in big:
            assert big[name] > small[name], (kind, name)
        assert {"entries", "queries", "n1", "n2"} <= set(big)
        for name in ("pairs", "m", "tops", "k"):
            assert (name in big) == (name in big_args), (kind, name)       # the kind's own count, where it has one
        at = [i for i, o in enumerate(ops) if o.kind == kind]
        assert any(o.kind in hl.DATA_KINDS for o in ops[at[0] + 1:at[1]])  # another family in between


# ---------------------------------------------------------------- the model
FLAGS = ("db", "batch", "searched", "lsoln", "polished", "fit", "cluster", "tops")
SEARCH = dict(lorder=True, r=3)
# what each call drops from a context that has everything: a polished LSOLN search of the batch, a fit, an accumulator,
# polish-all on (include/satabsearch.h)
DROPS = {
    hl.op("upload", db="d32"): {"searched", "lsoln", "polished", "fit", "cluster"},
    hl.op("upload_dense", db="d32"): {"searched", "lsoln", "polished", "fit", "cluster"},
    hl.op("upload_search", db="d32", lsoln=True, **SEARCH): {"fit", "cluster"},
    hl.op("upload_search", db="d32", lsoln=False, **SEARCH): {"lsoln", "fit", "cluster"},
    hl.op("set_queries", batch="q2"): {"searched", "lsoln", "polished", "fit"},
    hl.op("set_query", batch="q1"): {"searched", "lsoln", "polished", "fit"},
    hl.op("set_queries_from_db", batch=("db", "d16")): {"searched", "lsoln", "polished", "fit"},
    hl.op("set_polish_all", tops=1): set(),
    hl.op("polish_all_off"): {"tops"},
    hl.op("search", lsoln=True, **SEARCH): {"fit"},
    hl.op("search", lsoln=False, **SEARCH): {"lsoln", "fit"},
    hl.op("search_async_results", lsoln=False, **SEARCH): {"lsoln", "fit"},
    hl.op("search_matches", m=3, maps=True, **SEARCH): {"lsoln", "polished", "fit"},
    hl.op("search_refine", k=1, cand=4, big_r=8, lsoln=True, **SEARCH): {"lsoln", "polished", "fit"},
    hl.op("search_refine_polish", k=1, cand=4, big_r=8, tops=3, lsoln=True, **SEARCH): {"lsoln", "polished", "fit"},
    hl.op("search_pairs", pairs=7, lsoln=True, **SEARCH): set(),
    hl.op("search_pairs_matches", pairs=7, m=3, maps=True, **SEARCH): set(),
    hl.op("search_pairs_polish", pairs=7, tops=3, **SEARCH): set(),
    hl.op("results", lsoln=True): set(),
    hl.op("results_base"): set(),
    hl.op("topk_hits", k=3, maps=True): set(),
    hl.op("hits_cutoff", frac=0.5, k=None, maps=False): set(),
    hl.op("score_histogram"): set(),
    hl.op("fit_statistics", censor=0.1): set(),
    hl.op("set_statistics", fit="ab"): set(),
    hl.op("set_statistics", fit="none"): {"fit"},
    hl.op("cluster_begin"): set(),
    hl.op("cluster_add", frac=0.1): set(),
    hl.op("cluster_labels"): set(),
    hl.op("cluster_end"): {"cluster"},
}


def full_model(multi=False):
    m = hl.Model(multi)
    for o in (hl.op("upload", db="d16"), hl.op("set_queries", batch="q5"), hl.op("set_polish_all", tops=3),
              hl.op("search", lsoln=True, **SEARCH), hl.op("fit_statistics", censor=0.0), hl.op("cluster_begin")):
        assert m.legal(o.kind)
        m.apply(o)
    assert m.flags() == (True,) * len(FLAGS)
    return m


def test_model_follows_the_table_of_dropped_state():
    assert {o.kind for o in DROPS} == set(hl.KINDS)
    for o, drops in DROPS.items():
        m = full_model()
        assert m.legal(o.kind), o
        m.apply(o)
        assert {name for name, on in zip(FLAGS, m.flags()) if not on} == drops, o
    # what is installed afterwards
    m = full_model()
    m.apply(hl.op("search_matches", m=3, maps=True, lorder=False, r=1))
    assert m.searched == hl.Searched(False, 1, False, 0) and m.tops == 3
    m.apply(hl.op("search", lorder=True, lsoln=False, r=3))
    assert m.searched == hl.Searched(True, 3, False, 3) and m.legal("results_base")
    m.apply(hl.op("cluster_add", frac=0.1))
    m.apply(hl.op("set_queries", batch="q1"))
    assert len(m.cluster[1]) == 1 and m.legal("cluster_labels") and not m.legal("cluster_add")
    # sat_multi: search_topk searches again, so the fit goes; what it does not have is never legal
    m = full_model(True)
    m.apply(hl.op("topk_hits", k=3, maps=False))
    assert m.fit is None and m.searched is not None
    assert not any(m.legal(k) for k in hl.KINDS if k not in hl.MULTI_KINDS)
    # nothing but the settings is legal on a new context
    assert sorted(k for k in hl.KINDS if hl.Model().legal(k)) == ["polish_all_off", "set_polish_all", "set_queries", "set_query",
                                                                 "upload", "upload_dense"]


# ---------------------------------------------------------------- the worlds and their references
def test_worlds_have_the_shapes_the_kernels_branch_on():
    largest = {name: int(hl.db(name).orders.max()) for name in hl.COMBOS}
    assert largest == {"d16": 16, "d32": 32, "d48": 48, "d111": 111, "d150": 48, "d1100": 32}
    assert [len(hl.db(n)) for n in ("d16", "d32", "d48", "d111", "d150", "d1100")] == [5, 40, 18, 12, 150, 1100]
    assert {1, 2, 32} <= set(hl.db("d32").orders.tolist()) and {65, 97, 111} <= set(hl.db("d111").orders.tolist())
    for name in hl.COMBOS:
        o = hl.db(name).orders
        assert (np.diff(o) < 0).any() and (np.diff(o) > 0).any(), "%s is sorted" % name
    assert [hl.n1s_of(b) for b in ("q1", "q5", "q2")] == [[8], [3, 16, 17, 40, 111], [24, 32]]
    assert len(hl.n1s_of("q4")) == 4 and max(hl.n1s_of("q4")) <= 32 and min(hl.n1s_of("q4")) > 16
    assert len(hl.db("d1100")) * len(hl.n1s_of("q4")) > 4096               # leaves the single-launch plan
    assert hl.FIRST["q5"] != 0
    assert sorted(hl.RMAX.values()) == [8, 16, 16, 32, 64, 100] and len(hl.db(hl.LARGEST[0])) > len(hl.db(hl.SMALLEST[0]))


FAMILY = {"hits_cutoff": "cutoff", "cluster_labels": "cluster", "fit_statistics": "fit", "search_matches": "matches",
          "search_pairs_matches": "matches", "search_pairs_polish": "polish", "search_refine_polish": "polish",
          "results_base": "polish"}


def worlds_used():
    """{family: worlds (database, batch) it is used with anywhere in the GPU module}"""
    used = collections.defaultdict(set)
    for multi, ops in sequences():
        m = hl.Model(multi)
        for o in ops:
            if o.kind in FAMILY:
                if o.kind == "cluster_labels":
                    used["cluster"] |= {(add[0], add[1]) for add in m.cluster[1]}
                else:
                    used[FAMILY[o.kind]].add((m.db, m.batch))
            m.apply(o)
    return used


def test_references_are_not_vacuous():
    used = worlds_used()
    assert set(used) == set(FAMILY.values()) and all(len(v) >= 2 for v in used.values())
    for dbname, bkey in sorted(used["cutoff"], key=str):
        w = hl.world_ref(dbname, bkey)
        sd = hl.Searched(True, w.rmax, False, 0)
        counts = w.select(sd, None).cutoff(w.pcut(sd, None, 0.6))[2]
        assert ((counts > 0) & (counts < w.n)).any(), (dbname, bkey, counts)
    for dbname, bkey in sorted(used["fit"], key=str):
        w = hl.world_ref(dbname, bkey)
        assert w.fits(hl.Searched(True, w.rmax, False, 0), ("fit", 0.0))["fitted"].any(), (dbname, bkey)
    for dbname, bkey in sorted(used["matches"], key=str):
        w = hl.world_ref(dbname, bkey)
        q, e = np.divmod(np.arange(w.nq * min(w.n, 40), dtype=np.int32), np.int32(min(w.n, 40)))
        counts = np.concatenate([w.match_rows(q, e, lorder, w.rmax, 8)[0] for lorder in (True, False)])
        assert (counts > 1).any() and (counts < 8).any(), (dbname, bkey)
    for dbname, bkey in sorted(used["polish"], key=str):
        w = hl.world_ref(dbname, bkey)
        q, e = np.divmod(np.arange(w.nq * min(w.n, 40), dtype=np.int32), np.int32(min(w.n, 40)))
        moved = other = False
        for lorder, r in ((True, 3), (False, 3), (True, w.rmax), (False, w.rmax)):      # restart counts the walks use
            sc, base, rs, moves, _ = w.polish_rows(q, e, lorder, r, 8)
            best = w.match_rows(q, e, lorder, r, 1)[2][:, 0]
            moved |= bool(((moves > 0) & (sc > base)).any())
            other |= bool((rs != best).any())
        assert moved and other, (dbname, bkey, moved, other)
    for dbname, bkey in sorted(used["cluster"], key=str):
        w = hl.world_ref(dbname, bkey)
        m = hl.Model()
        m.db, m.batch = dbname, bkey
        sd = hl.Searched(True, w.rmax, False, 0)
        labels, _, edges = w.select(sd, None).components(w.pcut(sd, None, 0.4, m.query_nodes()), m.query_nodes())
        assert edges >= 1 and len(set(labels.tolist())) >= 2, (dbname, bkey, edges)


def test_the_reference_cache_keeps_the_cpu_side_short():
    """every reference of every walk, computed once: about the sum of one reference per (world, parameters); a walk that
    comes back to a state costs nothing"""
    started, steps = time.time(), 0
    for walk in hl.schedule(hl.SEED):
        m = hl.Model()
        for o in walk:
            if o.kind in hl.DATA_KINDS:
                got = hl.expect(o, m)
                assert hl.expect(o, m) is got
                steps += 1
            m.apply(o)
    print("%d references of %d walks in %.1f s" % (steps, hl.WALKS, time.time() - started))
    assert steps == sum(1 for w in hl.schedule(hl.SEED) for o in w if o.kind in hl.DATA_KINDS) and steps > 500
