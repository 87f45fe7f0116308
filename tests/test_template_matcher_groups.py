"""CPU: TemplateMatcher.match_groups against the loop of match() it restates -- the returned lists, the roi / transform
writes and the cache -- around fake scorers, and database.similar's batched=False route with params.templateMatch."""
import copy

import numpy as np
import pytest


class FakeMedia:
    def __init__(self, tag, md5=None, image=True):
        self.tag = tag
        self.md5 = f"md5-{tag}" if md5 is None else md5
        self.score, self.roi, self.transform = -1, None, None
        self.image = np.full((4, 4), tag, np.uint8) if image is True else image

    def clone(self):
        return copy.copy(self)


def row(status, score, tag):
    """one result record; the roi and the transform carry the pair's tags so that a write from the wrong pair shows"""
    from cbird_amd.hashing import TEMPLATE_IMAGE_RESULT_DTYPE

    r = np.zeros(1, TEMPLATE_IMAGE_RESULT_DTYPE)[0]
    r["status"], r["r"]["score"] = status, score
    r["r"]["roi"] = np.arange(8) + tag
    r["r"]["tx"], r["r"]["tx_found"] = np.arange(6) + tag, 1
    return r


def scorers(table):
    """table: {(template's first pixel, candidate's first pixel): (status, score)} -> a per-template scorer, a pair scorer
    that answers the same, and the list of calls each has seen"""
    from cbird_amd.hashing import TEMPLATE_IMAGE_RESULT_DTYPE

    calls, pair_calls = [], []

    def answer(t, c):
        key = (int(t.flat[0]), int(c.flat[0]))
        return row(*table[key], tag=100 * key[0] + key[1])

    def scorer(tmpl, cands, params):
        calls.append(len(cands))
        return np.array([answer(tmpl, c) for c in cands], TEMPLATE_IMAGE_RESULT_DTYPE).reshape(len(cands))

    def pair_scorer(images, pt, pc, params):
        pair_calls.append(len(pt))
        assert len(set(zip(pt.tolist(), pc.tolist()))) == len(pt)  # every ordered pair once
        return np.array([answer(images[t], images[c]) for t, c in zip(pt, pc)], TEMPLATE_IMAGE_RESULT_DTYPE).reshape(len(pt))

    return scorer, pair_scorer, calls, pair_calls


def state(out):
    return [[(m.tag, m.score, None if m.roi is None else m.roi.tolist(),
              None if m.transform is None else m.transform.tolist()) for m in g] for g in out]


def both_ways(table, tmpls, groups, cache=None, expect_pair_calls=None):
    """match_groups on one matcher, the loop of match() on another, on clones of the same media"""
    from cbird_amd.index import SearchParams
    from cbird_amd.templatematcher import TemplateMatcher

    p = SearchParams()
    scorer, pair_scorer, calls, pair_calls = scorers(table)
    a, b = TemplateMatcher(pair_scorer=pair_scorer), TemplateMatcher(scorer)
    a._cache.update(cache or {}), b._cache.update(cache or {})
    ta, ga = [t.clone() for t in tmpls], [[m.clone() for m in g] for g in groups]
    tb, gb = [t.clone() for t in tmpls], [[m.clone() for m in g] for g in groups]
    got = a.match_groups(ta, ga, p)
    want = [b.match(t, g, p) for t, g in zip(tb, gb)]
    assert state(got) == state(want)
    assert [[ga[i].index(m) for m in g] for i, g in enumerate(got)] == [[gb[i].index(m) for m in g] for i, g in enumerate(want)]
    assert state(ga) == state(gb)  # the members that were dropped got the same writes too
    assert a._cache == b._cache
    assert len(pair_calls) <= 1 and (expect_pair_calls is None or pair_calls == expect_pair_calls)
    assert bool(calls) == bool(pair_calls)  # no call at all where the cache answers everything
    return got, a, pair_calls


def test_match_groups_equals_the_loop_of_match():
    import cbird_amd.hashing as H
    from cbird_amd.templatematcher import INT_MAX

    A, B, C_, D = (FakeMedia(k) for k in (1, 2, 3, 4))
    S = H.TM_SCORED
    # (A, B) in group 1, (B, A) in group 2: the second takes the first's cached score, not its own
    table = {(1, 2): (S, 3), (2, 1): (S, 5), (1, 3): (S, 9), (2, 3): (S, 1), (1, 4): (H.TM_NO_MATCHES, INT_MAX)}
    got, tm, _ = both_ways(table, [A, B], [[B, C_, D], [A, C_]], expect_pair_calls=[5])
    assert [m.score for m in got[1]] == [1, 3] and [m.score for m in got[0]] == [3]
    assert tm._cache == {"md5-2md5-1": 3, "md5-3md5-1": 9, "md5-4md5-1": INT_MAX, "md5-3md5-2": 1}
    # the same where the first ends NO_KEYPOINTS, which is not cached: the second uses its own result
    table[(1, 2)] = (H.TM_NO_KEYPOINTS, INT_MAX)
    got, tm, _ = both_ways(table, [A, B], [[B, C_, D], [A, C_]], expect_pair_calls=[5])
    assert [m.score for m in got[1]] == [1, 5] and "md5-1md5-2" in tm._cache and "md5-2md5-1" not in tm._cache
    # ... and a template without keypoints, an empty resize
    table[(1, 2)], table[(1, 3)] = (H.TM_NO_TEMPLATE_KEYPOINTS, INT_MAX), (H.TM_EMPTY_RESIZE, INT_MAX)
    both_ways(table, [A, B], [[B, C_], [A, C_]], expect_pair_calls=[4])


def test_match_groups_keeps_the_quirks_of_match():
    import cbird_amd.hashing as H

    S = H.TM_SCORED
    A, B, C_ = (FakeMedia(k) for k in (1, 2, 3))
    table = {(t, c): (S, (t * 3 + c) % 7) for t in range(1, 6) for c in range(1, 6)}
    # a group with one missing md5: nothing of it is looked up, everything is written under "invalid-cache-key"
    nomd5 = FakeMedia(4, md5="")
    got, tm, _ = both_ways(table, [A, B, A], [[B, nomd5], [A, C_], [B, C_]])
    assert "invalid-cache-key" in tm._cache
    # a template whose image does not load: its group comes back empty, the others go on
    broken = FakeMedia(5, image=lambda: None)
    got, tm, calls = both_ways(table, [broken, B], [[A, C_], [A, C_]], expect_pair_calls=[2])
    assert got[0] == [] and len(got[1]) == 2
    # a candidate whose image does not load is skipped, nothing is cached for it
    got, tm, calls = both_ways(table, [A, B], [[broken, B], [broken]], expect_pair_calls=[1])
    assert [m.tag for m in got[0]] == [2] and got[1] == [] and set(tm._cache) == {"md5-2md5-1"}
    # an empty group, and no groups
    both_ways(table, [A, B], [[], [A]], expect_pair_calls=[1])


def test_match_groups_with_a_cache_from_before():
    import cbird_amd.hashing as H
    from cbird_amd.index import SearchParams
    from cbird_amd.templatematcher import TemplateMatcher

    S = H.TM_SCORED
    A, B, C_ = (FakeMedia(k) for k in (1, 2, 3))
    table = {(1, 2): (S, 3), (2, 1): (S, 5), (1, 3): (S, 6), (2, 3): (S, 1)}
    cache = {"md5-1md5-2": 4, "md5-3md5-1": 100}  # (B, A) in the other order; (A, C) above the threshold
    got, tm, calls = both_ways(table, [A, B], [[B, C_], [A, C_]], cache=cache, expect_pair_calls=[1])
    assert [m.score for m in got[0]] == [4] and [m.score for m in got[1]] == [1, 4]
    # the cache answers everything: the pair scorer is not called at all
    got, tm, calls = both_ways(table, [A, B], [[B, C_], [A]], cache=dict(cache, **{"md5-2md5-1": 2}), expect_pair_calls=[])
    assert calls == []
    # scorer= alone keeps its meaning: match_groups goes through it once per distinct template
    scorer, _, seen, _ = scorers(table)
    tm = TemplateMatcher(scorer)
    out = tm.match_groups([A.clone(), B.clone()], [[B.clone(), C_.clone()], [A.clone(), C_.clone()]], SearchParams())
    assert seen == [2, 2] and [[m.score for m in g] for g in out] == [[3, 6], [1, 3]]
    with pytest.raises(ValueError):
        tm.match_groups([A], [], SearchParams())


# ---- database.similar's batched=False route ----------------------------------------------------------------------------
class StubIndex:
    """find() from a table: {needle id: [(media id, score)]}"""

    def __init__(self, table):
        self.table = table

    def find(self, needle, params):
        from cbird_amd.index import Match

        return [Match(mediaId=i, score=s) for i, s in self.table.get(needle.id, [])]


class RecordingMatcher:
    """drops every candidate with an odd id, scores the others 10 - id"""

    def __init__(self):
        self.calls = []

    def match(self, tmpl, group, params):
        self.calls.append((tmpl.id, [m.id for m in group]))
        keep = [m for m in group if m.id % 2 == 0]
        for m in keep:
            m.score = 10 - m.id
        return sorted(keep, key=lambda m: m.score)


def test_similar_sends_every_result_group_through_the_matcher():
    from cbird_amd import Media, SearchParams
    from cbird_amd.database import filter_results, similar

    media = [Media(id=i, dctHash=i, path=f"/img/{i:03d}.jpg") for i in range(1, 7)]
    table = {1: [(2, 1), (3, 2), (4, 3)], 2: [(1, 1)], 3: [], 4: [(6, 0), (2, 2)], 5: [(3, 1)]}
    idx = StubIndex(table)
    p = SearchParams(templateMatch=True)
    tm = RecordingMatcher()
    got = similar(idx, media, p, batched=False, matcher=tm)
    # once per needle that has results; the needle is the template, searchIndex's group the candidates
    assert tm.calls == [(1, [2, 3, 4]), (2, [1]), (4, [6, 2]), (5, [3])]
    by_id = {m.id: m for m in media}
    want = []
    for i, rows in table.items():
        kept = sorted((10 - j, j) for j, _ in rows if j % 2 == 0)
        group = [by_id[i]]
        for s, j in kept:
            m = Media(id=j, dctHash=j, path=by_id[j].path)
            m.score = s
            group.append(m)
        want.append(group)
    want = filter_results(p, want)
    assert [[(m.id, m.score) for m in g[1:]] for g in got] == [[(m.id, m.score) for m in g[1:]] for g in want]
    assert [g[0].id for g in got] == [g[0].id for g in want] == [1, 4]
    # without the flag nothing changes and the matcher is not asked
    tm2 = RecordingMatcher()
    plain = similar(idx, media, SearchParams(), batched=False, matcher=tm2)
    assert tm2.calls == []
    assert [[m.id for m in g] for g in plain] == [[m.id for m in g]
                                                  for g in similar(idx, media, SearchParams(), batched=False)]
