"""CPU: the NumPy model of the video coverage map (tests/video_coverage_rules.py) against results written down by hand
for every rule, and against a restated findVideo on the 12-clip set; the host-only Python layer (VideoCoverage.ranges /
contains, database.video_coverage) on a stub index."""
import numpy as np
import pytest

import video_coverage_rules as VR
from cbird_amd import Media, SearchParams
from cbird_amd.database import video_coverage
from cbird_amd.video import VideoCoverage, VideoIndex


@pytest.mark.parametrize("name", list(VR.HAND))
def test_model_reproduces_the_hand_vectors(name):
    src, dst, thresh, skip, want = VR.HAND[name]
    s, frames, dframes, dist = VR.coverage(src, dst, thresh, skip)
    got = dict(s, frames=frames.tolist(), dst_frames=dframes.tolist(), distances=dist.tolist())
    for key, value in want.items():
        assert got[key] == value, (name, key, got[key], value)
    assert len(frames) == len(dframes) == len(dist) == s["n_src"]
    assert s["n_covered"] == int((dist < thresh).sum())


def test_trim_rules_differ_on_both_sides_of_the_boundary():
    """the source trim never asks about the length; the destination trim holds only when last / 2 > skip"""
    frames = np.array([0, 10, 20, 30, 40], np.int32)
    for last, trimmed in ((40, False), (41, False), (42, True), (43, True)):
        f = frames.copy()
        f[-1] = last
        assert len(VR.dest_view(f, VR.FAR[:5], 20)) == (1 if trimmed else 5), last
        assert VR.source_view(f, VR.FAR[:5], 20)[0].tolist() == [2], last
    assert len(VR.dest_view(frames, VR.FAR[:5], 0)) == 5  # `skip &&`


@pytest.mark.parametrize("skip", [0, 20])
def test_model_equals_find_video_on_the_clips(skip):
    """(n_covered, near_percent, src_in, dst_in, len) is findVideo's (num, percentNear, srcIn, dstIn, len) for all 144
    ordered pairs; a pair without a covered frame is a video findVideo does not report"""
    clips = VR.clips()
    contained = 0
    for a, needle in enumerate(clips):
        found = VR.find_video(needle, clips, 5, skip)
        for b, other in enumerate(clips):
            s = VR.coverage(needle, other, 5, skip)[0]
            if s["n_covered"] == 0:
                assert b not in found, (a, b)
            else:
                assert found[b] == (s["n_covered"], s["near_percent"], s["src_in"], s["dst_in"], s["len"]), (a, b)
            if a != b and a >= 8 and s["n_src"] and s["src_frames_covered"] == s["src_frames_total"]:
                contained += 1
    # the four sub-clips lie whole inside their sources
    assert contained >= 4


def test_sub_clips_are_contained_and_their_sources_are_not():
    clips = VR.clips()
    for sub, source in ((8, 6), (9, 1), (10, 4), (11, 2)):  # ids 9-12 inside 7, 2, 5, 3
        s = VR.coverage(clips[sub], clips[source], 5, 0)[0]
        assert s["src_frames_covered"] == s["src_frames_total"] > 0 and s["gap_len"] == 0, (sub, source)
        back = VR.coverage(clips[source], clips[sub], 5, 0)[0]
        assert 0 < back["src_frames_covered"] < back["src_frames_total"] and back["gap_len"] > 0, (sub, source)


# ---- the Python layer without a device ------------------------------------------------------------------------------------
def _coverage_of(src, dst, thresh, skip):
    s, frames, dframes, dist = VR.coverage(src, dst, thresh, skip)
    return VideoCoverage(thresh, **s, frames=frames, dst_frames=dframes, distances=dist)


def test_ranges_and_contains():
    src, dst, thresh, skip, _ = VR.HAND["gap_is_measured_in_frame_numbers"]
    c = _coverage_of(src, dst, thresh, skip)
    assert c.ranges() == [(0, 1), (3, 1), (11, 2)]
    assert c.ranges(covered=False) == [(1, 2), (4, 7)]
    assert sum(n for _, n in c.ranges()) == c.src_frames_covered == 4
    assert sum(n for _, n in c.ranges(False)) == c.src_frames_total - c.src_frames_covered == 9
    assert not c.contains() and c.contains(30) and not c.contains(31) and c.percent() == 30
    # the span of the last considered frame comes from src_frames_total: it may reach into the trim
    src, dst, thresh, skip, _ = VR.HAND["span_reaches_into_the_trim"]
    c = _coverage_of(src, dst, thresh, skip)
    assert c.ranges() == [(5, 4)] and c.ranges(False) == [(9, 21)]
    whole = _coverage_of(*VR.HAND["span_of_the_last_frame"][:4])
    assert whole.contains() and whole.ranges() == [(0, 10)] and whole.ranges(False) == []
    empty = _coverage_of(*VR.HAND["source_trimmed_to_nothing"][:4])
    assert empty.ranges() == [] and empty.contains() and empty.percent() == 0
    with pytest.raises(ValueError):
        VideoCoverage(5, src_frames_total=3).ranges()
    for src, dst, thresh, skip, _ in VR.HAND.values():  # the model's own run lengths
        s, frames, _, dist = VR.coverage(src, dst, thresh, skip)
        spans = VR.source_view(src[0], src[1], skip)[1]
        c = _coverage_of(src, dst, thresh, skip)
        assert c.ranges() == VR.ranges(frames, spans, dist < thresh)
        assert c.ranges(False) == VR.ranges(frames, spans, dist >= thresh)


class _StubIndex:
    """DctVideoIndex.coverage from the model"""

    def __init__(self, videos):
        self.videos, self.calls = videos, []

    def coverage(self, pairs, p, maps=True):
        self.calls.append((list(pairs), maps))
        return [_coverage_of(self.videos[a], self.videos[b], p.dctThresh, p.skipFrames) for a, b in pairs]


def test_database_video_coverage_sets_two_attributes():
    clips = VR.clips()
    videos = {i + 1: c for i, c in enumerate(clips)}

    def media(i):
        m = Media(id=i, path=f"{i}.mp4")
        m.videoIndex = VideoIndex(videos[i][0].tolist(), [int(x) for x in videos[i][1]])
        return m

    image = Media(id=99, path="still.jpg")  # an image needle of findFrame: no video, skipped
    groups = [[media(9), media(7)], [media(7), media(9), media(3)], [image, media(2)], [media(4)]]
    before = [[dict(vars(m)) for m in g] for g in groups]
    index = _StubIndex(videos)
    p = SearchParams(algo=SearchParams.AlgoVideo, dctThresh=5)
    p.skipFrames = 0
    assert video_coverage(index, groups, p) is groups
    assert index.calls == [([(9, 7), (7, 9), (7, 9), (9, 7), (7, 3), (3, 7)], False)]  # one call, summaries only
    m = groups[0][1]  # clip 9 is a cut of clip 7
    assert m.coverage == 100 and 0 < m.coveredBy < 100
    m = groups[1][1]
    assert m.coveredBy == 100 and 0 < m.coverage < 100
    assert groups[1][2].coverage == 0 and groups[1][2].coveredBy == 0
    for g, b in zip(groups, before):
        for k, (m, was) in enumerate(zip(g, b)):
            now = dict(vars(m))
            if k > 0 and g[0] is not image:
                assert set(now) - set(was) == {"coverage", "coveredBy"}
                now.pop("coverage"), now.pop("coveredBy")
            assert now == was
    with pytest.raises(ValueError):
        video_coverage(index, groups, SearchParams(algo=SearchParams.AlgoDCT))
    with pytest.raises(ValueError):
        video_coverage(object(), groups, p)
