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
    kinds = hl.kinds_of(multi)                                                   # the 27 kinds, or the 19 sat_multi has of them
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
FLAGS = ("db", "batch", "searched", "lsoln", "polished", "fit", "cluster", "tops", "leveled", "cover", "classes", "baseline")
SEARCH = dict(lorder=True, r=3)
# what each call drops from a context that has everything: a polished LSOLN search of the batch, a fit, an accumulator
# (plain, or leveled: "leveled" goes with "cluster"), polish-all on, a cover accumulator, classes, a baseline
# (include/satabsearch.h)
DROPS = {
    hl.op("upload", db="d32"): {"searched", "lsoln", "polished", "fit", "cluster", "cover", "classes", "baseline"},
    hl.op("upload_dense", db="d32"): {"searched", "lsoln", "polished", "fit", "cluster", "cover", "classes", "baseline"},
    hl.op("upload_search", db="d32", lsoln=True, **SEARCH): {"fit", "cluster", "cover", "classes", "baseline"},
    hl.op("upload_search", db="d32", lsoln=False, **SEARCH): {"lsoln", "fit", "cluster", "cover", "classes", "baseline"},
    hl.op("set_queries", batch="q2"): {"searched", "lsoln", "polished", "fit", "baseline"},
    hl.op("set_query", batch="q1"): {"searched", "lsoln", "polished", "fit", "baseline"},
    hl.op("set_queries_from_db", batch=("db", "d16")): {"searched", "lsoln", "polished", "fit", "baseline"},
    hl.op("set_queries_motif", batch=("motif", "d16")): {"searched", "lsoln", "polished", "fit", "baseline"},
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
    hl.op("cluster_begin_levels", levels=3): set(),
    hl.op("cluster_add_levels"): set(),
    hl.op("cluster_labels_levels"): set(),
    hl.op("cover_begin"): set(),
    hl.op("cover_add", frac=0.1): set(),
    hl.op("cover_solve"): set(),
    hl.op("cover_end"): {"cover"},
    hl.op("set_eval_classes"): set(),
    hl.op("eval_classes_off"): {"classes"},
    hl.op("eval_rows", rocn=3): set(),
    hl.op("eval_tables"): set(),
    hl.op("profile_rows", frac=0.5, gaps=True): set(),
    hl.op("baseline_keep"): set(),
    hl.op("baseline_drop"): {"baseline"},
    hl.op("baseline_results"): set(),
    hl.op("reorder_hits", frac=0.5, base_frac=None, kinds=7, k=None, maps=True): set(),
    hl.op("search_reordered", r=3, censor=0.0): set(),               # polished (the setting is honoured), LSOLN, fitted
    hl.op("search_reordered", r=3, censor=None): {"fit"},
}
# a begin replaces the accumulator of the other kind: the one flag a call of the table turns ON, and the one a plain begin
# turns off on a context whose accumulator is leveled
TURNS_ON = {hl.op("cluster_begin_levels", levels=3): {"leveled"}}
LEVELED_DROPS = {hl.op("cluster_begin"): {"leveled"}}


def full_model(multi=False, leveled=False):
    """a context with everything; its accumulator is plain or leveled, and "leveled" says which"""
    m = hl.Model(multi)
    for o in (hl.op("upload", db="d16"), hl.op("set_queries", batch="q5"), hl.op("set_polish_all", tops=3),
              hl.op("search", lsoln=True, **SEARCH), hl.op("fit_statistics", censor=0.0),
              hl.op("cluster_begin_levels", levels=3) if leveled else hl.op("cluster_begin"), hl.op("cover_begin"),
              hl.op("set_eval_classes"), hl.op("baseline_keep")):
        assert m.legal(o.kind)
        m.apply(o)
    assert m.flags() == tuple(name != "leveled" or leveled for name in FLAGS)
    return m


def test_model_follows_the_table_of_dropped_state():
    assert {o.kind for o in DROPS} == set(hl.ALL_KINDS) and set(hl.KINDS) < set(hl.ALL_KINDS)
    for o, drops in DROPS.items():
        checked = 0
        for leveled in (False, True):
            m = full_model(leveled=leveled)
            if not m.legal(o.kind):                    # the add and labels calls of the other accumulator kind
                assert o.kind in ("cluster_add", "cluster_labels", "cluster_add_levels", "cluster_labels_levels"), o
                assert leveled != o.kind.endswith("_levels"), o
                continue
            m.apply(o)
            off = set(drops) | ({"leveled"} if not leveled else set())
            if leveled:
                off |= LEVELED_DROPS.get(o, set()) | ({"leveled"} if "cluster" in drops else set())
            off -= TURNS_ON.get(o, set())
            assert {name for name, on in zip(FLAGS, m.flags()) if not on} == off, (o, leveled)
            checked += 1
        assert checked >= 1, o
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
    assert not any(m.legal(k) for k in hl.ALL_KINDS if k not in hl.MULTI_KINDS)
    assert set(hl.ALL_KINDS) - set(hl.MULTI_KINDS) == {"upload_dense", "set_query", "upload_search", "search_async_results", "search_pairs",
                                                     "results", "results_base", "cluster_end", "cover_end", "eval_tables"}
    # nothing but the settings (and the two calls that only forget) is legal on a new context
    assert sorted(k for k in hl.ALL_KINDS if hl.Model().legal(k)) == ["baseline_drop", "eval_classes_off", "polish_all_off", "set_polish_all",
                                                                     "set_queries", "set_query", "upload", "upload_dense"]
    # what is installed afterwards, the new state: the baseline is the rows as they were kept
    m = full_model()
    kept = (m.searched, m.fit)
    assert m.baseline == kept and kept == (hl.Searched(True, 3, True, 3), ("fit", 0.0))
    for o in (hl.op("search", lorder=False, lsoln=True, r=1), hl.op("fit_statistics", censor=0.1), hl.op("polish_all_off"),
              hl.op("search_pairs", pairs=7, lsoln=True, **SEARCH), hl.op("cluster_begin"), hl.op("cover_add", frac=0.1),
              hl.op("eval_rows", rocn=3), hl.op("profile_rows", frac=0.5, gaps=False), hl.op("set_statistics", fit="none")):
        assert m.legal(o.kind), o
        m.apply(o)
        assert m.baseline == kept and m.legal("reorder_hits") and m.legal("baseline_results"), o
    m.apply(hl.op("search", lorder=False, lsoln=False, r=1))
    assert m.baseline == kept and not m.legal("reorder_hits") and not m.legal("profile_rows") and m.legal("eval_rows")
    m.apply(hl.op("set_polish_all", tops=1))
    m.apply(hl.op("search_reordered", r=3, censor=0.1))
    assert m.baseline == (hl.Searched(True, 3, False, 1), ("fit", 0.1)) and m.fit == ("fit", 0.1)
    assert m.searched == hl.Searched(False, 3, True, 1) and m.legal("reorder_hits") and m.legal("results_base")
    # the accumulators: one of a kind, the cover beside it; an upload drops the three and the classes
    m = full_model()
    assert m.legal("cluster_add") and not m.legal("cluster_add_levels") and not m.legal("cluster_labels_levels")
    m.apply(hl.op("cluster_add", frac=0.1))
    m.apply(hl.op("cluster_begin_levels", levels=3))
    assert m.cluster[1] == [] and m.legal("cluster_add_levels") and not m.legal("cluster_add") and not m.legal("cluster_labels")
    assert m.legal("cover_add") and m.legal("cover_solve")
    m.apply(hl.op("cluster_end"))
    assert m.cluster is None and m.cover is not None and not m.legal("cluster_labels_levels")
    m.apply(hl.op("upload", db="d16"))
    assert not any(m.legal(k) for k in ("cover_solve", "cover_add", "eval_rows", "baseline_results", "cluster_labels"))


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


# ---------------------------------------------------------------- the second schedule: old and new kinds
def states(walk, multi=False):
    """(operation, the model before it) along one walk"""
    m = hl.Model(multi)
    for o in walk:
        assert m.legal(o.kind), o
        yield o, m
        m = hl._clone(m)
        m.apply(o)


@pytest.mark.parametrize("multi,count,pairs", [(False, hl.NEW_WALKS, 1198), (True, hl.NEW_MULTI_WALKS, 807)], ids=["one_context", "shards"])
def test_new_schedule_covers_every_allowed_pair_with_a_new_kind(multi, count, pairs):
    walks = hl.schedule(hl.SEED, multi, True)
    kinds = hl.kinds_of(multi, True)
    assert len(walks) == count and all(len(w) <= hl.WALK_STEPS + 10 for w in walks)
    followed = set()
    for walk in walks:
        names = [o.kind for o, _ in states(walk, multi)]
        followed |= set(zip(names, names[1:]))
    allowed = hl.allowed_pairs(multi, True)
    assert len(allowed) == pairs and allowed <= followed, sorted(allowed - followed)[:10]
    assert all(a in hl.NEW_KINDS or b in hl.NEW_KINDS for a, b in allowed) and {k for p in allowed for k in p} == set(kinds)
    # the goal is every pair of the model over all kinds that has a new kind in it - not a subset of it
    everything = hl.allowed_pairs(multi, False) | allowed
    assert len(everything) == len(hl.allowed_pairs(multi, False)) + pairs
    for a, b in (("cluster_begin_levels", "cluster_add"), ("cluster_begin", "cluster_labels_levels"), ("upload", "cover_solve"),
                 ("upload", "eval_rows"), ("set_queries", "baseline_results"), ("set_queries_motif", "reorder_hits"),
                 ("search_matches", "profile_rows"), ("baseline_drop", "reorder_hits")):
        assert (a, b) not in allowed, (a, b)
    for a, b in (("search_reordered", "reorder_hits"), ("search", "reorder_hits"), ("search_pairs_matches", "eval_rows"),
                 ("set_queries", "cover_solve"), ("set_queries", "cluster_labels_levels"), ("fit_statistics", "baseline_results"),
                 ("cluster_begin_levels", "cover_add"), ("polish_all_off", "baseline_keep")):
        assert (a, b) in allowed, (a, b)
    hl._cache.pop(("schedule", hl.SEED, multi, True))
    assert hl.schedule(hl.SEED, multi, True) == walks
    # the first schedule is what it was: its kinds only
    assert all(o.kind in hl.kinds_of(multi) for w in hl.schedule(hl.SEED, multi) for o in w)


def rows_of(m):
    return len(hl.n1s_of(m.batch)) * len(hl.db(m.db))


@pytest.mark.parametrize("multi", [False, True], ids=["one_context", "shards"])
def test_new_walks_contain_the_named_sequences(multi):
    found, up, down = collections.Counter(), set(), set()
    for walk in hl.schedule(hl.SEED, multi, True):
        since_reordered = since_keep = None             # the kinds run since search_reordered / since a keep under a polished search
        added, last_rows, since_pairs = {}, {}, False
        for o, m in states(walk, multi):
            k = o.kind
            if k == "reorder_hits":
                found["a baseline kept across a search"] += since_reordered is not None and "search" in since_reordered
                found["a baseline of a polished search, the polish then off"] += since_keep is not None and "polish_all_off" in since_keep
            if k in hl.QUERY_SETTING or k.startswith("upload") or k in ("baseline_drop", "baseline_keep", "search_reordered"):
                since_reordered = since_keep = None
            if k == "search_reordered":
                since_reordered = []
            elif since_reordered is not None:
                since_reordered.append(k)
            if k == "baseline_keep" and m.searched.tops and m.tops:
                since_keep = []
            elif since_keep is not None:
                since_keep.append(k)
            found["a leveled begin over a live plain accumulator"] += k == "cluster_begin_levels" and m.cluster is not None and not m.leveled()
            found["a plain begin over a live leveled accumulator"] += k == "cluster_begin" and m.leveled()
            if k in ("cover_add", "cluster_add_levels"):
                other = "cluster_add_levels" if k == "cover_add" else "cover_add"
                found["a cover add and a leveled add from one search"] += added.get(other) == (m.db, m.batch, m.searched, m.fit)
                added[k] = (m.db, m.batch, m.searched, m.fit)
            if k in hl.SEARCHES or k in hl.QUERY_SETTING or k.startswith("upload") or k == "search_reordered":
                since_pairs, added = False, {}
            if k in hl.PAIR_SEARCHES:
                since_pairs = True
            found["eval_rows after a pair search"] += k == "eval_rows" and since_pairs
            found["profile_rows after a pair search"] += k == "profile_rows" and since_pairs
            if k in hl.NEW_DATA and m.batch is not None:
                after = hl._clone(m)
                after.apply(o)
                now = rows_of(after)
                if k in last_rows and now > last_rows[k]:
                    up.add(k)
                if k in last_rows and now < last_rows[k]:
                    down.add(k)
                last_rows[k] = now
    for name in ("a baseline kept across a search", "a baseline of a polished search, the polish then off",
                 "a leveled begin over a live plain accumulator", "a plain begin over a live leveled accumulator",
                 "a cover add and a leveled add from one search", "eval_rows after a pair search", "profile_rows after a pair search"):
        assert found[name] >= 1, (name, found)
    data = {k for k in hl.NEW_DATA if not multi or k in hl.MULTI_KINDS}
    assert up == data and down == data, (data - up, data - down)      # each on a larger batch behind a smaller one, and the reverse


def new_references(kind, multi=False):
    """(operation, model before it, its reference) of every `kind` step of the two hand-made walks of the second schedule"""
    for walk in hl.schedule(hl.SEED, multi, True)[-2:]:
        for o, m in states(walk, multi):
            if o.kind == kind:
                yield o, m, hl.expect(o, m)


def test_new_references_are_not_vacuous():
    """conditions on the CPU references alone, of steps the GPU module runs (the hand-made walks: the permutant world and
    25 / 200 / 25 rows)"""
    reorder_lib, select_lib = hl.reorder_lib, hl.select_lib
    # reorder_hits: one reference with sequential, circular and permuted rows, a query with none, and a min_base_pvalue that
    # removes some of the rows the same call returns without it, but not all
    shown = False
    for o, m, (counts, rows, *_) in new_references("reorder_hits"):
        a = dict(o.args)
        if a["base_frac"] is None or a["k"] or a["kinds"] != 7:
            continue
        w = m.world()
        free = sum(len(r) for r in w.reorder(m.searched, m.fit, m.baseline, w.pcut(m.searched, m.fit, a["frac"]), 0.0, 7, None)[0])
        shown |= (set(rows["kind"].tolist()) == {reorder_lib.SEQ, reorder_lib.CIRC, reorder_lib.PERM} and (counts == 0).any()
                  and 0 < len(rows) < free and bool((rows["base_pvalue"] > rows["hit"]["pvalue"]).any()))
    assert shown
    # eval_rows: positives and negatives, an unclassified query, and a tie group of negatives that straddles the rocn cut
    shown = False
    for o, m, (rows,) in new_references("eval_rows"):
        w, rocn, cl, nodes = m.world(), dict(o.args)["rocn"], hl.classes(m.db), m.query_nodes()
        straddles = False
        for q, node in enumerate(nodes):
            if cl[node] >= 0:
                counted = (cl >= 0) & (np.arange(w.n) != node) & (cl != cl[node])
                neg = np.sort(w.matrix(m.searched)[0][q][counted])[::-1]
                straddles |= len(neg) > rocn and neg[rocn - 1] == neg[rocn]
        shown |= (straddles and bool(((rows["positives"] > 0) & (rows["negatives"] > 0)).any()) and bool((rows["query_class"] == -1).any())
                  and bool((rows["t2"] > 0).any()))
    assert shown
    # cover_solve: two rounds at least, and representatives that are not the single-linkage labels of the same edges
    shown = False
    for o, m, (rep, deg, counts) in new_references("cover_solve"):
        ea, eb = hl._added_edges(m.cover[1])
        shown |= counts[1] >= 2 and not np.array_equal(rep, select_lib.components(m.cover[0], ea, eb))
    assert shown
    # cluster_labels_levels: two levels with different labels; the cutoffs ascend strictly
    shown = False
    for o, m, (labels, deg, edges) in new_references("cluster_labels_levels"):
        cuts = hl.level_cuts(*m.cluster[2])
        assert len(cuts) == len(labels) and all(a < b for a, b in zip(cuts, cuts[1:])) and 0.0 < cuts[0] and cuts[-1] < 1.0
        shown |= len(labels) >= 2 and any(not np.array_equal(labels[j], labels[j + 1]) for j in range(len(labels) - 1)) and edges[0] < edges[-1]
    assert shown
    assert {len(hl.level_cuts("d32", n)) for n in (1, 3, hl.MAX_LEVELS)} == {1, 3, hl.MAX_LEVELS}
    # profile_rows: hits, and a pair of SSEs matched together less often than either alone; packed and with gaps
    shown, gaps = False, set()
    for o, m, (hits, packed) in new_references("profile_rows"):
        w = m.world()
        offset, words = hl.profile_offsets(w.n1s, dict(o.args)["gaps"])
        gaps.add(dict(o.args)["gaps"])
        assert len(packed) == words and (not dict(o.args)["gaps"] or (packed == hl.PROFILE_FILL).sum() >= 5 * w.nq)
        for q, n1 in enumerate(w.n1s):
            j = packed[offset[q]:offset[q] + n1 * n1].reshape(n1, n1)
            shown |= hits[q] > 0 and bool((j < np.diag(j)[:, None]).any())
    assert shown and gaps == {False, True}
    # a motif batch whose list is not ascending, one that is the whole entry, and every n1 is the list's length
    lists = hl.motif_lists("dperm")
    assert any(l is not None and list(l) != sorted(l) for l in lists) and any(l is None for l in lists)
    assert [len(q[2]) for q in hl.batch(("motif", "dperm"))[0]] == [
        len(l) if l is not None else int(hl.db("dperm").orders[e]) for l, e in zip(lists, hl.db_indices("dperm"))]
    # the classification: implants by their source, unclassified entries, and both in every database
    for name in hl.NEW_COMBOS:
        c = hl.classes(name)
        assert (c == -1).any() and all(c[e] == s[1] for e, s in hl.IMPLANTS[name].items()) and len(set(c.tolist())) >= 4
    assert len(hl.db("dperm")) == 30 and int(hl.db("dperm").orders.max()) == 32
    # search_reordered: its baseline differs from its searched state, and a fitted p-value differs from the built-in one
    for o, m, ref in new_references("search_reordered"):
        sc, base_sc, base_p, rows = ref[0], ref[2], ref[3], ref[4]
        assert (sc != base_sc).any()
    # baseline_results as kept under one fit and read under another: the p-values are those of keep time
    assert any(m.baseline[1] != m.fit or m.baseline[0] != m.searched for _, m, _ in new_references("baseline_results"))


def test_the_reference_cache_keeps_the_new_cpu_side_short():
    """every reference of every walk of the second schedule, computed once (the figure is printed, not asserted)"""
    started, steps = time.time(), 0
    for walk in hl.schedule(hl.SEED, False, True):
        for o, m in states(walk):
            if o.kind in hl.DATA_KINDS:
                got = hl.expect(o, m)
                assert hl.expect(o, m) is got
                steps += 1
    print("%d references of %d walks in %.1f s" % (steps, hl.NEW_WALKS, time.time() - started))
    assert steps == sum(1 for w in hl.schedule(hl.SEED, False, True) for o in w if o.kind in hl.DATA_KINDS) and steps > 800
    assert {o.kind for w in hl.schedule(hl.SEED, False, True) for o in w} == set(hl.ALL_KINDS)


def test_caller_stream_walks_cover_every_kind():
    """the ten walks tests/test_gpu_caller_stream.py runs on every kind of caller's stream: four of the first schedule,
    four of the second, its two hand-made ones - every kind of call occurs among them, and each walk is legal from a
    fresh context"""
    walks = hl.caller_stream_walks()
    names = [name for name, _ in walks]
    assert len(walks) == 10 and len(set(names)) == 10 and names[-2:] == ["named", "sizes"]
    assert sum(n.startswith("walk") for n in names) == 4 and sum(n.startswith("new_walk") for n in names) == 4
    first, second = hl.schedule(hl.SEED), hl.schedule(hl.SEED, False, True)
    for name, ops in walks:
        assert any(ops == w for w in (first[:-1] if name.startswith("walk") else second)), name
        m = hl.Model()
        for o in ops:
            assert m.legal(o.kind), (name, o)
            m.apply(o)
    seen = {o.kind for _, ops in walks for o in ops}
    assert seen == set(hl.ALL_KINDS), sorted(set(hl.ALL_KINDS) - seen)
