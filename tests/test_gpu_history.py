"""What a context carries from one call to the next (-m gpu): sequences of calls of every family on ONE Searcher (or
MultiSearcher), each result compared byte for byte with its CPU reference (tests/history_lib.py: oracle_lib, matches_lib,
polish_lib, select_lib - never another GPU context).  1. every data-returning kind at its largest world, another family at
the smallest, the kind at its smallest, then at the largest again; 2. seeded walks that between them follow every ordered
pair of kinds the model of the documented state allows, with entries, queries, n1, n2, pairs, M, T, k and nodes going up
and down on one context; 3. at every step of every walk every result call the model says is not available returns its
documented error and changes nothing; 4. walks under a 16 KB scratch budget and a small selection-key budget, which make
the launch cuts depend on what the buffers were sized for before; 5. the same on 2 and 3 shards on device 0, with shard
sizes that move the padded rows up and down.
The kinds added since (the leveled accumulator, the cover, the evaluation, motif batches, the profile, the baseline and the
reordered hits) run through the same five: scenario 1 by DATA_KINDS, and the walks of the second schedule (NEW_WALKS: every
allowed pair with a new kind in it) through 2 to 5."""
import numpy as np
import pytest

import cuda_satabsearch_amd as sat
import cover_lib
import history_lib as hl

pytestmark = pytest.mark.gpu


def text(o):
    return "%s(%s)" % (o.kind, ", ".join("%s=%s" % kv for kv in o.args))


def follow(s, ops, multi=False, after_step=None, before_step=None):
    """run `ops` on `s`, comparing every data-returning step with its reference; returns the number compared.
    before_step(s, m) runs in front of every step (tests/test_gpu_caller_stream.py queues the caller's work there)"""
    m, compared = hl.Model(multi), 0
    for step, o in enumerate(ops):
        assert m.legal(o.kind), "step %d: the model does not allow %s" % (step, text(o))
        if before_step:
            before_step(s, m)
        got = hl.run(s, o, m)
        if o.kind in hl.DATA_KINDS:
            diff = hl.same(got, hl.expect(o, m))
            assert diff is None, "step %d, %s on (%s, %s) after %s: %s" % (
                step, text(o), dict(o.args).get("db", m.db), m.batch, [text(x) for x in ops[max(0, step - 4):step]], diff)
            compared += 1
            properties(o, m, got)
        m.apply(o)
        if after_step:
            after_step(s, m)
    return compared


def properties(o, m, got):
    """what the header promises of a result beyond its bytes: the nesting of the levels, the cover's two invariants"""
    if o.kind == "cluster_labels_levels":
        labels = got[0]
        for j in range(len(labels) - 1):
            assert np.array_equal(labels[j + 1][labels[j]], labels[j + 1]), "levels %d and %d are not nested" % (j, j + 1)
    if o.kind == "cover_solve":
        cover_lib.check_invariants(m.cover[0], *hl._added_edges(m.cover[1]), got[0])


def data_steps(ops):
    return sum(1 for o in ops if o.kind in hl.DATA_KINDS)


def shards(count):
    return sat.MultiSearcher(count, devices=[0] * count)


# ---------------------------------------------------------------- 1. grow, shrink, grow
@pytest.mark.parametrize("kind", hl.DATA_KINDS)
def test_grow_shrink_grow(kind):
    ops = hl.grow_shrink_grow(kind)
    assert [o.kind for o in ops].count(kind) >= 3
    with sat.Searcher(0) as s:
        assert follow(s, ops) == data_steps(ops)


# ---------------------------------------------------------------- 2. scheduled walks
@pytest.mark.parametrize("walk", range(hl.WALKS))
def test_walk(walk):
    walks = hl.schedule(hl.SEED)
    assert len(walks) == hl.WALKS
    with sat.Searcher(0) as s:
        assert follow(s, walks[walk]) == data_steps(walks[walk])


@pytest.mark.parametrize("walk", range(hl.NEW_WALKS))
def test_new_walk(walk):
    walks = hl.schedule(hl.SEED, False, True)
    assert len(walks) == hl.NEW_WALKS
    with sat.Searcher(0) as s:
        assert follow(s, walks[walk]) == data_steps(walks[walk])


# ---------------------------------------------------------------- 3. refusals
def refused(call, code):
    with pytest.raises(sat.SatError, match=r"^\[%d\]" % code):
        call()


def refusals(s, m):
    """every result call the model says is not available: SAT_ESTATE (-5); where it is available, a bad argument:
    SAT_EINVAL (-1).  Neither may change what the next legal call returns - the walk goes on comparing."""
    sd = m.searched
    nq = len(hl.n1s_of(m.batch)) if m.batch is not None else 1
    nodes = np.zeros(nq, np.int32)
    if sd is None:
        for call in (s.results, lambda: s.topk_hits(1), lambda: s.hits_cutoff(0.5), s.score_histogram):
            refused(call, -5)
    else:
        refused(lambda: s.hits_cutoff(-1.0), -1)
    if sd is None or not sd.lsoln:
        for call in (lambda: s.results(True), lambda: s.topk_hits(1, True), lambda: s.hits_cutoff(0.5, None, True)):
            refused(call, -5)
    if sd is None or not sd.tops:
        refused(s.results_base, -5)
    if sd is None or m.cluster is None or m.leveled():               # (the other accumulator kind: SAT_ESTATE)
        refused(lambda: s.cluster_add(0.5, nodes), -5)
    else:
        refused(lambda: s.cluster_add(0.5, nodes + m.cluster[0]), -1)
    if m.cluster is None or m.leveled():
        refused(s.cluster_labels, -5)
    refused(lambda: s.set_polish_all(9), -1)
    # the calls added since: no leveled accumulator (none, or the plain one), no cover, no classes, no lsoln, no baseline
    if sd is None or not m.leveled():
        refused(lambda: s.cluster_add_levels(nodes), -5)
    else:
        refused(lambda: s.cluster_add_levels(nodes + m.cluster[0]), -1)
    if not m.leveled():
        refused(s.cluster_labels_levels, -5)
    if m.db is not None:                                              # an earlier accumulator of either kind stays as it was
        refused(lambda: s.cluster_begin_levels([0.5, 0.1]), -1)
        refused(lambda: s.cluster_begin_levels(np.linspace(0.1, 0.9, hl.MAX_LEVELS + 1)), -1)
        refused(lambda: s.cover_begin(0), -1)
        refused(lambda: s.set_eval_classes(hl.classes(m.db)[:-1]), -1)
    else:
        for call in (lambda: s.cluster_begin_levels([0.5], 5), lambda: s.cover_begin(5), lambda: s.set_eval_classes(np.zeros(5, np.int32))):
            refused(call, -5)
    if sd is None or m.cover is None:
        refused(lambda: s.cover_add(0.5, nodes), -5)
    else:
        refused(lambda: s.cover_add(0.5, nodes + m.cover[0]), -1)
        refused(lambda: s.cover_add(-0.5, nodes), -1)
    if m.cover is None:
        refused(s.cover_solve, -5)
    if sd is None or not m.classes:
        refused(lambda: s.eval_rows(nodes), -5)
        refused(lambda: s.eval_tables(nodes) if m.batch is not None else s.eval_rows(nodes, 1), -5)
    else:
        refused(lambda: s.eval_rows(nodes, 0), -1)
        refused(lambda: s.eval_rows(nodes + len(hl.db(m.db))), -1)
        refused(lambda: s.eval_tables(nodes - 1), -1)
    if m.batch is not None:                                           # (the wrapper sizes the matrices by the batch)
        if sd is None or not sd.lsoln:
            refused(lambda: s.profile_rows(0.5), -5)
        else:
            refused(lambda: s.profile_rows(-0.5), -1)
            refused(lambda: s.profile_rows(float("nan"), nodes), -1)
    if sd is None:
        refused(s.baseline_keep, -5)
    if m.baseline is None:
        refused(s.baseline_results, -5)
    if m.baseline is None or sd is None or not sd.lsoln:
        refused(lambda: s.reorder_hits(0.5), -5)
        refused(lambda: s.reorder_hits(0.5, 0.0, 7, None, True), -5)
    else:
        refused(lambda: s.reorder_hits(0.5, 0.0, 0), -1)
        refused(lambda: s.reorder_hits(0.5, 0.0, 8), -1)
        refused(lambda: s.reorder_hits(-0.5), -1)
        refused(lambda: s.reorder_hits(0.5, -0.5), -1)
    if m.db is not None and m.batch is not None:
        refused(lambda: s.search_reordered(3, 1.5), -1)               # before either search: nothing changes


@pytest.mark.parametrize("walk", range(hl.WALKS))
def test_refusals_at_every_step(walk):
    """every walk once more with the refusals behind every step: which call is refused depends on what the context has
    held before - sat_results_base after a plain search that follows a polished one, maps after a search without LSOLN
    that follows one with (tests/test_history_cpu.py: the walks contain both)"""
    ops = hl.schedule(hl.SEED)[walk]
    with sat.Searcher(0) as s:
        refusals(s, hl.Model())
        assert follow(s, ops, after_step=refusals) == data_steps(ops)


@pytest.mark.parametrize("walk", range(hl.NEW_WALKS))
def test_refusals_at_every_step_of_a_new_walk(walk):
    """the same over the second schedule: which accumulator kind is live, whether a baseline or classes are, depends on
    what the context has been through"""
    ops = hl.schedule(hl.SEED, False, True)[walk]
    with sat.Searcher(0) as s:
        refusals(s, hl.Model())
        assert follow(s, ops, after_step=refusals) == data_steps(ops)


# ---------------------------------------------------------------- 4. budgets that make sizing history-sensitive
@pytest.mark.parametrize("name,value,walk", [("SAT_EXP_SCRATCH_KB", "16", 1), ("SAT_EXP_SELECT_KEYS", "100", 2),
                                             ("SAT_EXP_SCRATCH_KB", "16", 13), ("SAT_EXP_SELECT_KEYS", "100", 14),
                                             ("SAT_EXP_SELECT_KEYS", "100", -1), ("SAT_EXP_SELECT_KEYS", "100", -2),
                                             ("SAT_EXP_SCRATCH_KB", "16", -2)])
def test_walk_under_a_small_budget(monkeypatch, name, value, walk):
    """16 KB of scratch cuts every LSOLN, match and polish pass into launches whose size depends on the slab buffer's
    capacity; 100 selection keys cut the query list of the selection passes into chunks of 100 / entries queries - the
    new result calls go through the same chunk walk (walk < 0: the hand-made walks of the second schedule)"""
    ops = hl.schedule(hl.SEED)[walk] if walk >= 0 else hl.schedule(hl.SEED, False, True)[walk]
    monkeypatch.setenv(name, value)                                     # read when the context is created
    with sat.Searcher(0) as s:
        assert follow(s, ops) == data_steps(ops)


# ---------------------------------------------------------------- 5. shards
MULTI_DATA_KINDS = [k for k in hl.DATA_KINDS if k in hl.MULTI_KINDS]


@pytest.mark.parametrize("count", [2, 3])
@pytest.mark.parametrize("kind", MULTI_DATA_KINDS)
def test_shards_grow_shrink_grow(kind, count):
    ops = hl.grow_shrink_grow(kind, multi=True)
    with shards(count) as s:
        assert follow(s, ops, multi=True) == data_steps(ops)


@pytest.mark.parametrize("count,walk", [(2, 0), (3, 1), (2, hl.MULTI_WALKS - 1), (3, hl.MULTI_WALKS - 1)])
def test_shards_walk(count, walk):
    walks = hl.schedule(hl.SEED, multi=True)
    assert len(walks) == hl.MULTI_WALKS
    with shards(count) as s:
        assert follow(s, walks[walk], multi=True) == data_steps(walks[walk])


@pytest.mark.parametrize("count,walk", [(2, 0), (3, 1), (2, hl.NEW_MULTI_WALKS - 2), (3, hl.NEW_MULTI_WALKS - 1)])
def test_shards_new_walk(count, walk):
    walks = hl.schedule(hl.SEED, True, True)
    assert len(walks) == hl.NEW_MULTI_WALKS
    with shards(count) as s:
        assert follow(s, walks[walk], multi=True) == data_steps(walks[walk])


@pytest.mark.parametrize("count", [2, 3])
def test_shards_padded_rows_rise_and_fall(count):
    """150 -> 12 -> 40 -> 5 -> 150 entries: the gathers read a padded shard out of buffers an earlier, larger search sized"""
    ops = hl.shard_sequence()
    with shards(count) as s:
        assert follow(s, ops, multi=True) == data_steps(ops)
