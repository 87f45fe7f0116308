"""SearchParams.turnMask in cbird_amd.database, on the stub index of tests/test_query_compose.py: the quarter turns and
transposes of a needle are searched after its reflections, in flag order, as needles with id 0 and the needle's path,
and compose like them; similar() and the on-device sort-similar leave them to query().  No device needed."""
import warnings

import pytest

from cbird_amd.database import _sort_similar_on_device, query, similar
from cbird_amd.index import DctHashIndex, Media, SearchParams
from cbird_amd.scanner import IndexResult

from test_query_compose import ID_MAP, NEEDLE, StubIndex, pairs

VIEWS = {f: IndexResult(dctHash=100 + f) for f in (1, 2, 4, 8, 16, 32, 64)}


def test_turn_flags_and_default():
    assert (SearchParams.TurnRight, SearchParams.TurnLeft, SearchParams.Transpose, SearchParams.AntiTranspose) == (8, 16, 32, 64)
    assert SearchParams().turnMask == 0
    # disjoint from the reflections: mirrorMask | turnMask is one view mask
    assert (SearchParams.MirrorHorizontal | SearchParams.MirrorVertical | SearchParams.MirrorBoth) & 120 == 0


def test_turned_views_follow_the_reflections_in_flag_order_with_id_0_and_the_needles_path():
    idx = StubIndex({})
    query(idx, NEEDLE, SearchParams(mirrorMask=5, turnMask=72), ID_MAP, VIEWS)
    assert idx.asked == [(1, 100, "/d/1.jpg")] + [(0, 100 + f, "/d/1.jpg") for f in (1, 4, 8, 64)]
    idx = StubIndex({})
    query(idx, NEEDLE, SearchParams(turnMask=120), ID_MAP, VIEWS)
    assert [a[1] for a in idx.asked] == [100, 108, 116, 132, 164]


def test_turned_lists_compose_like_reflected_ones():
    idx = StubIndex({100: [(1, 0), (2, 3)], 108: [(1, 0), (3, 2)], 116: [(3, 2), (2, 2)]})
    got = query(idx, NEEDLE, SearchParams(turnMask=24), ID_MAP, VIEWS)
    # filterSelf drops id 1 from the needle's own list only (a turned needle has id 0); ties go by id, then by view
    assert pairs(got) == [(1, 0), (2, 2), (3, 2), (3, 2), (2, 3)]
    assert [id(m) for m in got if m.id == 3][0] != [id(m) for m in got if m.id == 3][1]


def test_a_set_turn_bit_without_its_view_raises():
    idx = StubIndex({})
    with pytest.raises(ValueError):
        query(idx, NEEDLE, SearchParams(turnMask=16), ID_MAP, {8: VIEWS[8]})
    with pytest.raises(ValueError):
        query(idx, NEEDLE, SearchParams(turnMask=8), ID_MAP, None)
    with pytest.raises(ValueError):
        query(idx, NEEDLE, SearchParams(mirrorMask=1, turnMask=8), ID_MAP, {1: VIEWS[1]})


def test_query_without_turn_mask_asks_what_it_asked_before():
    for mask, want in ((0, [100]), (7, [100, 101, 102, 104]), (2, [100, 102])):
        idx = StubIndex({})
        query(idx, NEEDLE, SearchParams(mirrorMask=mask, turnMask=0), ID_MAP, VIEWS)
        assert [a[1] for a in idx.asked] == want
        assert [a[0] for a in idx.asked] == [1] + [0] * (len(want) - 1)
    assert query(StubIndex({}), NEEDLE, SearchParams(), ID_MAP, None) == []


def test_similar_ignores_turn_mask_with_a_warning():
    hay = [Media(id=i, dctHash=100, path=f"/d/{i}.jpg") for i in (1, 2)]
    idx = StubIndex({100: [(1, 0), (2, 0)]})
    p = SearchParams(turnMask=120)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = similar(idx, hay, p, batched=False)
    assert len(w) == 1 and "turned images unsupported" in str(w[0].message)
    p.turnMask = 0
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        want = similar(idx, hay, p, batched=False)
    assert not w
    assert [pairs(g) for g in got] == [pairs(g) for g in want]


def test_sort_similar_leaves_turned_views_to_the_loop_route():
    index = DctHashIndex.__new__(DctHashIndex)  # (only its type is looked at)
    assert _sort_similar_on_device(index, SearchParams()) is True
    assert _sort_similar_on_device(index, SearchParams(turnMask=8)) is False
