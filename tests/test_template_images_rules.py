"""CPU half of the suite for cbird_amd/csrc/tmimages.hip: the model of tests/template_images_rules.py on its own (the
conditions that keep the GPU comparison from passing on an all-empty fixture), the candScale arithmetic on truncation
boundaries, TemplateMatcher's cache / threshold / sort around an injected scorer, and SearchParams' defaults."""
import numpy as np
import pytest

import template_images_rules as M


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_model_status_mix(ch):
    tmpl, cands, model = M.chain_fixture(ch)
    assert tmpl.shape[:2] == (M.TH, M.TW) and len(cands) == len(M.NAMES) == len(model)
    print([(n, m["status"], m["n_keypoints"], m["n_matches"]) for n, m in zip(M.NAMES, model)])
    assert M.chain_conditions(model) == []
    by = dict(zip(M.NAMES, model))
    assert by["flat"]["status"] == M.NO_KEYPOINTS and by["inside_border"]["status"] == M.NO_KEYPOINTS
    assert by["enlarged_2_5"]["resized"] and by["enlarged_2_5"]["scale"] < 1 and by["enlarged_2_5"]["status"] == M.SCORED
    assert (by["enlarged_2_5"]["w"], by["enlarged_2_5"]["h"]) == (320, 259)  # 420 x 340 at float32(320) / 420
    assert not by["shifted"]["resized"] and by["shifted"]["scale"] == 1


def test_a_flat_template_has_no_keypoints():
    tmpl, cands, _ = M.chain_fixture(3)
    model = M.template_match_images(np.full_like(tmpl, 100), cands[:3])
    assert [m["status"] for m in model] == [M.NO_TEMPLATE_KEYPOINTS] * 3
    assert [(m["w"], m["h"]) for m in model] == [c.shape[1::-1] for c in cands[:3]]


def test_cand_scale_truncates_where_the_reference_does():
    assert M.max_size(333, 150) == 499          # 499.5 truncated, not rounded
    assert M.max_size(160, 200) == 320 and M.max_size(7, 15) == 1 and M.max_size(3, 30) == 0
    # not larger in area: never resized, whatever its longest side
    assert M.cand_target(160, 128, 1000, 20, 200) == (np.float32(1), 1000, 20, False)
    # larger in area but within maxSize
    assert M.cand_target(160, 128, 320, 300, 200) == (np.float32(1), 320, 300, False)
    s, w, h, r = M.cand_target(160, 128, 420, 340, 200)
    assert r and s == np.float32(320) / np.float32(420) and (w, h) == (320, 259)
    # int(w * factor) in float: 321 * (320 / 321) is 319.99997 in float32 and 320 exactly in double
    s, w, h, r = M.cand_target(160, 128, 321, 300, 200)
    assert r and w == int(np.float32(321) * s) and w in (319, 320) and h == int(np.float32(300) * s)
    # a side that truncates to 0: the reference's cv::resize throws
    s, w, h, r = M.cand_target(10, 10, 3000, 100, 200)
    assert r and (w, h) == (20, 0)
    s, w, h, r = M.cand_target(10, 10, 2000, 30, 3)  # maxSize 0: candScale 0
    assert r and s == 0 and (w, h) == (0, 0)


def test_radius_match_orders_by_distance_then_train_row():
    train = np.zeros((4, 32), np.uint8)
    train[1, 0] = 1      # distance 1 from the zero row
    train[3, 5] = 0x80   # another one at distance 1; rows 0 and 2 are duplicates at distance 0
    q = np.zeros((2, 32), np.uint8)
    q[1] = 0xFF
    assert M.radius_match(train, q, 1).tolist() == [[0, 0, 0], [0, 2, 0], [0, 1, 1], [0, 3, 1]]
    assert M.radius_match(train, q, 0).tolist() == [[0, 0, 0], [0, 2, 0]]
    assert len(M.radius_match(train, q, 256)) == 8 and len(M.radius_match(train[:0], q, 256)) == 0


@pytest.mark.parametrize("n_train,max_dist", [(1, 0), (63, 25), (100, 25), (257, 0), (100, 256)])
def test_match_fixture_plants_what_it_says(n_train, max_dist):
    train, txy, desc, xy, counts = M.match_case(n_train, max_dist)
    first, rec, a, b = M.match_model(train, txy, desc, xy, counts, max_dist)
    per = np.diff(first.astype(np.int64))
    if max_dist == 256:
        assert (per == counts.astype(np.int64) * n_train).all()
        return
    assert per[0] == 0 and per[1] >= 1 and per[4] >= 70          # every other planted query is within the radius
    if n_train >= 6:
        assert per[5:].tolist() == [0, 1, 2, 3]
    assert (rec[:, 2] <= max_dist).all() and (rec[:, 2] == max_dist).any()
    if n_train >= 3:  # a query next to a duplicated train row: equal distances, ordered by train row
        ties = 0
        for lo, hi in zip(first[:-1].astype(int), first[1:].astype(int)):
            r = rec[lo:hi]
            same = np.flatnonzero((r[1:, 0] == r[:-1, 0]) & (r[1:, 2] == r[:-1, 2]))
            ties += len(same)
            assert all(r[i + 1, 1] > r[i, 1] for i in same)
        assert ties >= 1


# ---- TemplateMatcher ---------------------------------------------------------------------------------------------------
class FakeMedia:
    def __init__(self, md5, image=None):
        self.md5, self.score, self.roi = md5, -1, None
        self.image = np.zeros((4, 4), np.uint8) if image is None else image


def scorer_returning(rows):
    """rows: {candidate's first pixel: (status, score)}; counts the calls and the candidates it was handed"""
    from cbird_amd.hashing import TEMPLATE_IMAGE_RESULT_DTYPE

    calls = []

    def scorer(tmpl, cands, params):
        calls.append(len(cands))
        out = np.zeros(len(cands), TEMPLATE_IMAGE_RESULT_DTYPE)
        for i, c in enumerate(cands):
            out[i]["status"], out[i]["r"]["score"] = rows[int(c.flat[0])]
        return out

    return scorer, calls


def media(tag, md5=None):
    return FakeMedia(f"md5-{tag}" if md5 is None else md5, np.full((4, 4), tag, np.uint8))


def test_template_matcher_threshold_sort_and_cache():
    from cbird_amd import hashing as H
    from cbird_amd.index import SearchParams
    from cbird_amd.templatematcher import INT_MAX, TemplateMatcher

    p = SearchParams()
    rows = {1: (H.TM_SCORED, 6), 2: (H.TM_SCORED, 7), 3: (H.TM_SCORED, 0), 4: (H.TM_NO_MATCHES, INT_MAX),
            5: (H.TM_FEW_POINTS, INT_MAX), 6: (H.TM_NO_TRANSFORM, INT_MAX), 7: (H.TM_NO_KEYPOINTS, INT_MAX)}
    scorer, calls = scorer_returning(rows)
    tm = TemplateMatcher(scorer)
    tmpl = media(0, "md5-t")
    group = [media(k) for k in rows]
    out = tm.match(tmpl, group, p)
    assert [m.md5 for m in out] == ["md5-3", "md5-1"] and [m.score for m in out] == [0, 6]  # 7 < 7 is false: strict
    assert calls == [7]
    # the INT_MAX exits and the scores are cached, NO_KEYPOINTS is not
    assert tm._cache == {"md5-1md5-t": 6, "md5-2md5-t": 7, "md5-3md5-t": 0, "md5-4md5-t": INT_MAX, "md5-5md5-t": INT_MAX,
                         "md5-6md5-t": INT_MAX}
    out = tm.match(tmpl, [media(k) for k in rows], p)
    assert [m.md5 for m in out] == ["md5-3", "md5-1"] and calls == [7, 1]  # only the one without keypoints is scored again
    # the other key order hits as well: the roles swapped
    scorer2, calls2 = scorer_returning({0: (H.TM_SCORED, 3)})
    tm._scorer = scorer2
    out = tm.match(media(1), [media(0, "md5-t")], p)
    assert [m.score for m in out] == [6] and calls2 == []
    # all cached: returns sorted without a call; an empty group returns at once
    assert tm.match(tmpl, [], p) == [] and calls2 == []
    p.tmThresh = 8
    assert [m.score for m in tm.match(tmpl, [media(2), media(1), media(3)], p)] == [0, 6, 7]


def test_template_matcher_without_md5_does_not_cache():
    from cbird_amd import hashing as H
    from cbird_amd.index import SearchParams
    from cbird_amd.templatematcher import TemplateMatcher

    scorer, calls = scorer_returning({1: (H.TM_SCORED, 2), 2: (H.TM_SCORED, 1)})
    tm = TemplateMatcher(scorer)
    group = [media(1), media(2, "")]
    out = tm.match(media(0, "md5-t"), group, SearchParams())
    assert [m.score for m in out] == [1, 2] and calls == [2]
    assert set(tm._cache) == {"invalid-cache-key"}  # (:164) no pair's key was written
    tm.match(media(0, "md5-t"), [media(1), media(2, "")], SearchParams())
    assert calls == [2, 2]
    tm.match(media(0, ""), [media(1)], SearchParams())  # the template's md5 is empty
    assert calls == [2, 2, 1]
    # an image that does not load: the candidate is skipped and nothing is cached; a template that does not: empty
    tm2 = TemplateMatcher(scorer)
    broken = FakeMedia("md5-9", image=lambda: None)
    assert [m.md5 for m in tm2.match(media(0, "md5-t"), [broken, media(1)], SearchParams())] == ["md5-1"]
    assert set(tm2._cache) == {"md5-1md5-t"}
    assert tm2.match(FakeMedia("md5-t", image=lambda: None), [media(2)], SearchParams()) == []


def test_search_params_defaults_are_the_reference_s():
    from cbird_amd.hashing import tm_params
    from cbird_amd.index import SearchParams

    p = SearchParams()
    assert (p.needleFeatures, p.haystackFeatures, p.tmThresh, p.tmScalePct, p.templateMatch) == (100, 1000, 7, 200, False)
    assert (p.cvThresh, p.dctThresh, p.mirrorMask) == (25, 5, 0)  # (what was there stays)
    assert tm_params().tolist() == [(100, 1000, 25, 200)] and tm_params(p).tobytes() == tm_params().tobytes()
    assert tuple(M.DEFAULTS.values()) == (100, 1000, 25, 200)
