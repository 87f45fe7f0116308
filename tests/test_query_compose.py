"""Engine::query's composition of a reflection search (src/engine.cpp:421-438) in cbird_amd.database, on a stub index
whose find() returns canned matches: the view order, similarTo's per-list minMatches clearing, the id-0 filterSelf rule
of a mirrored needle, duplicates kept across lists, the tie key of the final sort, and a missing view for a set bit.
No device needed; the kernel's resource check cross-compiles."""
import os
import subprocess
import sys
import warnings

import pytest

from cbird_amd.database import query, similar, similar_to
from cbird_amd.index import Match, Media, SearchParams
from cbird_amd.scanner import IndexResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StubIndex:
    """find() answers by the needle's dctHash; it records the needles it was asked about"""

    def __init__(self, table):
        self.table, self.asked = table, []

    def find(self, needle, params):
        self.asked.append((needle.id, needle.dctHash, needle.path))
        return [Match(mediaId=i, score=s) for i, s in self.table.get(needle.dctHash, [])]


ID_MAP = {i: Media(id=i, path=f"/d/{i}.jpg") for i in range(1, 10)}
NEEDLE = Media(id=1, dctHash=100, path="/d/1.jpg")
VIEWS = {1: IndexResult(dctHash=101), 2: IndexResult(dctHash=102), 4: IndexResult(dctHash=104)}


def pairs(g):
    return [(m.id, m.score) for m in g]


def test_views_are_searched_in_engine_order_with_id_0_and_the_needles_path():
    idx = StubIndex({})
    query(idx, NEEDLE, SearchParams(mirrorMask=7), ID_MAP, VIEWS)
    assert idx.asked == [(1, 100, "/d/1.jpg"), (0, 101, "/d/1.jpg"), (0, 102, "/d/1.jpg"), (0, 104, "/d/1.jpg")]
    idx = StubIndex({})
    query(idx, NEEDLE, SearchParams(mirrorMask=SearchParams.MirrorBoth | SearchParams.MirrorHorizontal), ID_MAP, VIEWS)
    assert [a[1] for a in idx.asked] == [100, 101, 104]
    assert (SearchParams.MirrorNone, SearchParams.MirrorHorizontal, SearchParams.MirrorVertical,
            SearchParams.MirrorBoth) == (0, 1, 2, 4)
    assert SearchParams().mirrorMask == 0


def test_filter_self_drops_the_needles_id_only_from_its_own_list():
    idx = StubIndex({100: [(1, 0), (2, 3)], 101: [(1, 0), (3, 2)]})
    got = query(idx, NEEDLE, SearchParams(mirrorMask=1), ID_MAP, VIEWS)
    assert pairs(got) == [(1, 0), (3, 2), (2, 3)]  # the H view finds the needle itself: its needle has id 0
    got = query(idx, NEEDLE, SearchParams(mirrorMask=1, filterSelf=False), ID_MAP, VIEWS)
    assert pairs(got) == [(1, 0), (1, 0), (3, 2), (2, 3)]


def test_each_list_is_cleared_on_its_own_by_min_matches():
    idx = StubIndex({100: [(2, 1), (3, 2)], 101: [(4, 1)], 102: [(5, 0), (6, 4)], 104: []})
    p = SearchParams(mirrorMask=7, minMatches=2)
    assert pairs(similar_to(idx, NEEDLE, p, ID_MAP)) == [(2, 1), (3, 2)]
    got = query(idx, NEEDLE, p, ID_MAP, VIEWS)
    assert pairs(got) == [(5, 0), (2, 1), (3, 2), (6, 4)]  # the H list (one match) is dropped whole
    p.minMatches = 1
    assert pairs(query(idx, NEEDLE, p, ID_MAP, VIEWS)) == [(5, 0), (2, 1), (4, 1), (3, 2), (6, 4)]


def test_duplicates_are_kept_and_ties_go_by_id_then_view():
    idx = StubIndex({100: [(7, 2), (3, 2)], 101: [(3, 2), (2, 2)], 102: [(7, 1)], 104: [(3, 2)]})
    got = query(idx, NEEDLE, SearchParams(mirrorMask=7), ID_MAP, VIEWS)
    assert pairs(got) == [(7, 1), (2, 2), (3, 2), (3, 2), (3, 2), (7, 2)]
    # the three (3, 2): identity list first, then H, then both -- the view order breaks the tie
    order = [id(m) for m in got if m.id == 3]
    assert len(set(order)) == 3


def test_path_filters_see_the_needles_path_in_every_list():
    media = dict(ID_MAP)
    media[4] = Media(id=4, path="/d/sub/4.jpg")
    idx = StubIndex({100: [(4, 1), (2, 2)], 101: [(4, 0), (3, 1)]})
    p = SearchParams(mirrorMask=1, path="/d/sub", inPath=True, minMatches=0)
    assert pairs(query(idx, NEEDLE, p, media, VIEWS)) == [(4, 0), (4, 1)]
    p = SearchParams(mirrorMask=1, filterParent=True, minMatches=0)
    assert pairs(query(idx, NEEDLE, p, media, VIEWS)) == [(4, 0), (4, 1)]  # /d is the needle's directory in both lists


def test_a_set_bit_without_its_view_raises():
    idx = StubIndex({})
    with pytest.raises(ValueError):
        query(idx, NEEDLE, SearchParams(mirrorMask=2), ID_MAP, {1: VIEWS[1]})
    with pytest.raises(ValueError):
        query(idx, NEEDLE, SearchParams(mirrorMask=1), ID_MAP, None)
    assert query(idx, NEEDLE, SearchParams(mirrorMask=0), ID_MAP, None) == []


def test_similar_ignores_mirror_mask_with_a_warning():
    hay = [Media(id=i, dctHash=100, path=f"/d/{i}.jpg") for i in (1, 2)]
    idx = StubIndex({100: [(1, 0), (2, 0)]})
    p = SearchParams(mirrorMask=7)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = similar(idx, hay, p, batched=False)
    assert [str(x.message) for x in w] == ["reflected images unsupported, use -similar-to"]
    p.mirrorMask = 0
    assert [pairs(g) for g in got] == [pairs(g) for g in similar(idx, hay, p, batched=False)]


def test_mirror_kernel_neither_spills_nor_uses_scratch():
    import shutil

    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "mirror.hip"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = [l for l in r.stdout.splitlines() if "k_gray_views" in l]
    assert len(lines) == 6 and all(" scratch   0 " in l for l in lines), r.stdout
