"""The argument checks of the selection calls (-m gpu): what one context refuses, three shards refuse with the same code
and the same text - best-k, the refine calls, the p-value cutoff, the fit, sat_cluster_add - and both texts are those of
tests/golden/select_args.json, recorded once from the build before the checks were given one home (sat_cutoff.hpp).
Where that build's single and sharded texts differed, the file holds both and both stay.  Every case is an argument the
library refuses before it queues anything: the rows selected after the refusals are those selected before them.  The
same file pins the bytes each selection call copies back (Searcher.d2h_bytes)."""
import json
import os

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd._native import SatError

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "select_args.json")
R = 2                                                                   # maxstart of every search here
NAN, INF = float("nan"), float("inf")


def refusal(call):
    """"[code] text" of the SatError the call raises (ValueError: the binding's own refusal)"""
    try:
        call()
    except SatError as e:
        return str(e)
    except ValueError as e:
        return "ValueError: %s" % e
    return "no error"


def raw(obj, rc):
    """a C entry point called past the binding's own checks: its code and text as the binding would raise them"""
    if rc < 0:
        raise SatError("[%d] %s" % (rc, obj._lib.sat_last_error().decode()))


def refused_calls(s, m):
    """name -> (the call on one context, the call on three shards or None)"""
    nodes = [0, 1]
    calls = {}
    for p in (-1.0, NAN, INF):
        calls["hits_cutoff(%r)" % p] = (lambda p=p: s.hits_cutoff(p), lambda p=p: m.hits_cutoff(p))
        calls["search_cutoff(%r)" % p] = (None, lambda p=p: m.search_cutoff(p, maxstart=R))
        calls["cluster_add(%r)" % p] = (lambda p=p: s.cluster_add(p, nodes), lambda p=p: m.cluster_add(p, nodes))
    for c in (-0.1, 0.6, NAN):
        calls["fit(%r)" % c] = (lambda c=c: s.fit_statistics(c), lambda c=c: m.search_fit(c, maxstart=R))
    for tops in (0, 9):
        calls["refine_polish(tops=%d)" % tops] = (lambda t=tops: s.search_refine_polish(2, 3, 4, t, maxstart=R),
                                                  lambda t=tops: m.search_refine_polish(2, 3, 4, t, maxstart=R))
    calls["topk(k=0)"] = (lambda: s.topk(0), None)
    calls["topk_hits(k=0)"] = (lambda: s.topk_hits(0), lambda: m.search_topk(0, maxstart=R))
    for name, (k, c, r2) in {"k=0": (0, 3, 4), "candidates=0": (2, 0, 4), "refine_maxstart=0": (2, 3, 0),
                             "k>candidates": (4, 3, 4)}.items():
        calls["refine(%s)" % name] = (lambda a=(k, c, r2): s.search_refine(*a, maxstart=R),
                                      lambda a=(k, c, r2): m.search_refine(*a, maxstart=R))
        calls["refine_polish(%s)" % name] = (lambda a=(k, c, r2): s.search_refine_polish(*a, 2, maxstart=R),
                                             lambda a=(k, c, r2): m.search_refine_polish(*a, 2, maxstart=R))
    calls["cluster_add(NULL nodes)"] = (lambda: raw(s, s._lib.sat_cluster_add(s._ctx, 1.0, None)),
                                        lambda: raw(m, m._lib.sat_multi_cluster_add(m._m, 1.0, None)))
    calls["cluster_add(short nodes)"] = (lambda: s.cluster_add(1.0, nodes[:1]), lambda: m.cluster_add(1.0, nodes[:1]))
    calls["cluster_add(node out of range)"] = (lambda: s.cluster_add(1.0, [0, 5]), lambda: m.cluster_add(1.0, [0, 5]))
    return calls


def unsearched_calls(s, m):
    """the selection calls on a state no search has produced"""
    return {
        "unsearched topk": (lambda: s.topk(3), None),
        "unsearched topk_hits": (lambda: s.topk_hits(3), None),
        "unsearched hits_cutoff": (lambda: s.hits_cutoff(1.0), lambda: m.hits_cutoff(1.0)),
        "unsearched score_histogram": (s.score_histogram, m.score_histogram),
        "unsearched fit": (lambda: s.fit_statistics(0.0), None),
        "unsearched cluster_add": (lambda: s.cluster_add(1.0, [0, 1]), lambda: m.cluster_add(1.0, [0, 1])),
    }


def moved(obj, call):
    before = obj.d2h_bytes()
    call()
    return obj.d2h_bytes() - before


def good_rows(s, m):
    """one good best-3 and one good cutoff at P = 1, as bytes: one context, then three shards"""
    hits, maps = s.topk_hits(3, lsoln=True)
    rows, rmaps = s.hits_cutoff(1.0, lsoln=True)
    mhits, mmaps, _ = m.search_topk(3, lsoln=True, maxstart=R)
    mrows, mrmaps = m.hits_cutoff(1.0, lsoln=True)
    one = [hits.tobytes(), maps.tobytes()] + [x.tobytes() for x in rows + rmaps]
    three = [mhits.tobytes(), mmaps.tobytes()] + [x.tobytes() for x in mrows + mrmaps]
    return one, three


def observe():
    """everything the test compares: {"errors": name -> {"single", "multi"}, "d2h": {"single", "multi"}: call -> bytes},
    and the good rows before and after the refusals"""
    db = sat.synth.make_db(5, orders=np.array([4, 5, 6, 7, 8], np.int32), sort=False)
    queries = [sat.synth.make_query(5, seed=31), sat.synth.make_query(7, seed=32)]
    errors, d2h = {}, {"single": {}, "multi": {}}
    with sat.Searcher(0) as s, sat.MultiSearcher(3, devices=[0, 0, 0]) as m:
        for x in (s, m):
            x.upload(db)
            x.set_queries(queries)
            x.cluster_begin()

        def refuse(calls):
            for name, (one, three) in calls.items():
                errors[name] = {"single": refusal(one) if one else None, "multi": refusal(three) if three else None}

        refuse(unsearched_calls(s, m))
        s.search(True, True, R)
        m.search(True, True, R)
        before = good_rows(s, m)
        refuse(refused_calls(s, m))
        after = good_rows(s, m)
        # the bytes each good call copies back
        for name, call in {
            "topk(3)": lambda: s.topk(3), "topk_hits(3)": lambda: s.topk_hits(3), "topk_hits(3, maps)": lambda: s.topk_hits(3, lsoln=True),
            "hits_cutoff(1.0)": lambda: s.hits_cutoff(1.0), "hits_cutoff(1.0, maps)": lambda: s.hits_cutoff(1.0, lsoln=True),
            "score_histogram()": s.score_histogram, "fit_statistics()": s.fit_statistics,
            "search_refine(2, 3, 4)": lambda: s.search_refine(2, 3, 4, maxstart=R),
            "search_refine(2, 3, 4, maps)": lambda: s.search_refine(2, 3, 4, lsoln=True, maxstart=R),
            "search_refine_polish(2, 3, 4, 2)": lambda: s.search_refine_polish(2, 3, 4, 2, maxstart=R),
            "cluster_add(1.0)": lambda: s.cluster_add(1.0, [0, 1]), "cluster_labels()": s.cluster_labels,
        }.items():
            d2h["single"][name] = moved(s, call)
        for name, call in {
            "search_topk(3)": lambda: m.search_topk(3, maxstart=R), "search_topk(3, maps)": lambda: m.search_topk(3, lsoln=True, maxstart=R),
            "hits_cutoff(1.0)": lambda: m.hits_cutoff(1.0), "hits_cutoff(1.0, maps)": lambda: m.hits_cutoff(1.0, lsoln=True),
            "score_histogram()": m.score_histogram, "search_fit()": lambda: m.search_fit(maxstart=R),
            "search_refine(2, 3, 4)": lambda: m.search_refine(2, 3, 4, maxstart=R),
            "search_refine_polish(2, 3, 4, 2)": lambda: m.search_refine_polish(2, 3, 4, 2, maxstart=R),
            "cluster_add(1.0)": lambda: m.cluster_add(1.0, [0, 1]), "cluster_labels()": m.cluster_labels,
        }.items():
            d2h["multi"][name] = moved(m, call)
    return {"errors": errors, "d2h": d2h}, before, after


@pytest.fixture(scope="module")
def observed():
    assert sat.device_count() >= 1, "GPU tests need a HIP device (no CPU path exists)"
    return observe()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_is_refused_with_the_recorded_code_and_text(observed, golden):
    got, want = observed[0]["errors"], golden["errors"]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
        for text in got[name].values():
            assert text is None or text.startswith(("[-", "ValueError: ")), "%s was not refused: %s" % (name, text)


def test_one_context_and_three_shards_refuse_alike(observed, golden):
    """the same code and text in every case that has both calls: the recorded build's two texts differed nowhere (a case
    where they had would keep both in the fixture, and the first test would hold each to its own)"""
    recorded_apart = {n for n, e in golden["errors"].items() if e["single"] and e["multi"] and e["single"] != e["multi"]}
    assert recorded_apart == set()
    both = [e for e in observed[0]["errors"].values() if e["single"] and e["multi"]]
    assert len(both) == 26
    for e in both:
        assert e["single"] == e["multi"]


def test_the_state_is_usable_after_the_refusals(observed):
    _, before, after = observed
    assert before == after
    assert before[0] == before[1]                                       # and three shards select what one context selects
    assert len(before[0][0]) == 2 * 3 * 32                              # 2 queries x 3 rows of sat_hit


def test_bytes_copied_back_are_the_recorded_ones(observed, golden):
    assert observed[0]["d2h"] == golden["d2h"]
    assert observed[0]["d2h"]["single"]["cluster_add(1.0)"] == 0 and observed[0]["d2h"]["multi"]["cluster_add(1.0)"] == 0
