"""CPU: the NumPy model of the video segments (tests/video_segments_rules.py) against results written down by hand for
every rule -- ties, interval gaps, peeling, the stop rules, tol 0, direction, trimming, the empty cases, the monotone flag
-- on synthetic clips with known answers, and the host-only Python layer (VideoSegments.match_range / cut_list,
database.video_segments) on a stub index."""
import numpy as np
import pytest

import video_coverage_rules as VR
import video_segments_rules as SR
from cbird_amd import Media, SearchParams
from cbird_amd.database import video_segments
from cbird_amd.video import VSEGMENT_DTYPE, VSEGMENT_FRAME_DTYPE, VSEGMENTS_DTYPE, VideoIndex, VideoSegment, VideoSegments


@pytest.mark.parametrize("name", list(SR.HAND))
def test_model_reproduces_the_hand_vectors(name):
    src, dst, par, want, segs, columns = SR.hand(name)
    s, got_segs, frames, dframes, dist, seg = SR.run(src, dst, par)
    for key, value in want.items():
        assert s[key] == value, (name, key, s[key], value)
    assert got_segs == segs, name
    got = dict(frames=frames.tolist(), dst_frames=dframes.tolist(), distances=dist.tolist(), segments=seg.tolist())
    for key, value in columns.items():
        assert got[key] == value, (name, key)
    # what holds for every result
    assert len(frames) == len(dframes) == len(dist) == len(seg) == s["n_src"]
    assert s["n_segments"] == len(got_segs) <= par["max_segments"]
    assert [g["n_frames"] for g in got_segs] == sorted((g["n_frames"] for g in got_segs), reverse=True)  # supports never rise
    assert all(g["n_frames"] >= par["min_frames"] for g in got_segs)
    assert s["n_aligned"] == sum(g["n_frames"] for g in got_segs) == int((seg >= 0).sum())
    assert s["src_frames_aligned"] == sum(g["span_sum"] for g in got_segs) <= s["src_frames_total"]
    assert ((seg < 0) == (dframes < 0)).all() and ((seg < 0) == (dist == 65)).all()
    for r, g in enumerate(got_segs):
        apart = dframes[seg == r].astype(np.int64) - frames[seg == r] - g["offset"]
        assert len(apart) == g["n_frames"] and (np.abs(apart) <= par["tol"]).all() and (dist[seg == r] < par["thresh"]).all()


def test_plateau_of_a_copy_is_the_tolerance_window():
    src, dst, par, *_ = SR.hand("copy_plateau_centre")
    fs = np.asarray(src[0], np.int64)
    rows = [(np.array([i]), np.array([0])) for i in range(len(fs))]  # every frame matches its own copy alone
    omin = int(fs.min() - fs.max() - par["tol"])
    sup = SR.support(fs, fs, rows, np.ones(len(fs), bool), par["tol"], omin, int(fs.max() - fs.min() + par["tol"]) - omin + 1)
    at = np.nonzero(sup == 10)[0] + omin
    assert at.tolist() == [-2, -1, 0, 1, 2] and SR.pick(sup, omin) == (10, 0)


def test_pick_tie_rules_on_bare_supports():
    """rule 2 without videos: the centre of the run, floor toward minus infinity, the smaller |c|, the negative of two"""
    assert SR.pick(np.array([0, 3, 3, 3, 0]), 10) == (3, 12)
    assert SR.pick(np.array([0, 3, 3, 3, 3, 0]), 10) == (3, 12)  # [11, 14]: floor(12.5)
    assert SR.pick(np.array([2, 2, 0, 0]), -8) == (2, -8)  # [-8, -7]: floor(-7.5) = -8, not -7
    assert SR.pick(np.array([1, 0, 0, 0, 1]), -2) == (1, -2)  # runs at -2 and 2: the negative
    assert SR.pick(np.array([1, 1, 0, 0, 0, 1, 1]), -3) == (1, 2)  # [-3, -2] and [2, 3]: floor(-2.5) = -3, floor(2.5) = 2
    assert SR.pick(np.array([1, 0, 1, 0, 0]), 0) == (1, 0)
    assert SR.pick(np.array([0, 0, 0]), 5) == (0, 6)  # no support: the stop rule's business


def _walk_clip(rng, n, max_gap=11):
    step = np.zeros(n, np.uint64)
    for _ in range(2):
        step ^= np.uint64(1) << rng.integers(0, 64, n).astype(np.uint64)
    step[0] = rng.integers(0, 2**63, dtype=np.uint64)
    return np.cumsum(rng.integers(1, max_gap + 1, n)).astype(np.int32) - 1, np.bitwise_xor.accumulate(step)


def test_known_answers_on_random_walk_clips():
    """a sub-clip comes out as one segment at its true offset with every frame in it; a source cut from two stretches
    gives two segments at the two true offsets; an unrelated clip gives none"""
    rng = np.random.default_rng(3)
    f, h = _walk_clip(rng, 160)
    sub = (f[40:100] - f[40], h[40:100])
    s, segs, *_ = SR.segments(sub, (f, h), 5, 0, 15, 3, 4)
    assert segs[0]["offset"] == int(f[40]) and segs[0]["n_frames"] == 60 and s["n_aligned"] == 60
    assert (s["src_in"], s["dst_in"]) == (0, int(f[40]))
    # frames 20..59 then 100..139, renumbered to follow each other
    two_f = np.concatenate([f[20:60] - f[20], f[100:140] - f[100] + (f[60] - f[20])])
    s, segs, *_ = SR.segments((two_f, np.concatenate([h[20:60], h[100:140]])), (f, h), 5, 0, 15, 3, 4)
    offsets = sorted(g["offset"] for g in segs[:2])
    assert offsets == sorted([int(f[20]), int(f[100] - (f[60] - f[20]))]) and s["monotone"] == 1
    assert [g["n_frames"] for g in segs[:2]] == [40, 40]
    other = _walk_clip(rng, 60)
    assert SR.segments(other, (f, h), 5, 0, 15, 3, 4)[0]["n_segments"] == 0
    # destination frame numbers jittered by +-3: the plateau centre is still the true offset
    jit = (f + rng.integers(-3, 4, len(f))).astype(np.int32)
    jit.sort()
    s, segs, *_ = SR.segments(sub, (jit, h), 5, 0, 15, 3, 4)
    assert abs(segs[0]["offset"] - int(f[40])) <= 3 and segs[0]["n_frames"] == 60


def test_sub_clips_of_the_clip_set_align_whole():
    clips = VR.clips()
    for sub, source in ((8, 6), (9, 1), (10, 4), (11, 2)):
        s, segs, *_ = SR.segments(clips[sub], clips[source], 5, 0, 15, 3, 4)
        assert s["n_segments"] >= 1 and s["src_frames_aligned"] == s["src_frames_total"] > 0, (sub, source)
        assert s["monotone"] == 1 and segs[0]["offset"] > 0
        back = SR.segments(clips[source], clips[sub], 5, 0, 15, 3, 4)
        # (the plateau of the longer clip is cut by its other frames, so its centre is the mirror image only within tol)
        assert abs(back[1][0]["offset"] + segs[0]["offset"]) <= 15 and back[1][0]["offset"] < 0
        assert back[0]["src_frames_aligned"] < back[0]["src_frames_total"]


# ---- the Python layer without a device ------------------------------------------------------------------------------------
def test_record_layouts_match_the_header():
    assert VSEGMENT_DTYPE.itemsize == 32 and VSEGMENTS_DTYPE.itemsize == 48 and VSEGMENT_FRAME_DTYPE.itemsize == 16
    assert VSEGMENT_DTYPE.names == SR.SEGMENT_FIELDS and VSEGMENTS_DTYPE.names == SR.SUMMARY_FIELDS
    from cbird_amd import _lib
    import ctypes as C
    for struct, dtype in ((_lib.cbh_vsegment, VSEGMENT_DTYPE), (_lib.cbh_vsegments, VSEGMENTS_DTYPE),
                          (_lib.cbh_vsegment_frame, VSEGMENT_FRAME_DTYPE)):
        assert C.sizeof(struct) == dtype.itemsize
        assert [(n, getattr(struct, n).offset) for n, _ in struct._fields_] == [(n, dtype.fields[n][1]) for n in dtype.names]


def _segments_of(src, dst, par):
    s, segs, frames, dframes, dist, seg = SR.run(src, dst, par)
    return VideoSegments(**s, segments=[VideoSegment(**g) for g in segs], frames=frames, dst_frames=dframes, distances=dist,
                         segment_of=seg)


def test_match_range_and_cut_list():
    src, dst, par, *_ = SR.hand("swapped_scenes_not_monotone")
    r = _segments_of(src, dst, par)
    assert r.match_range() == (30, 0, 21)  # segment 0, the first found -- not the first in the source
    assert [(g.src_first, g.offset) for g in r.segments] == [(30, -30), (0, 100)]
    assert [(g.src_first, g.offset) for g in r.cut_list()] == [(0, 100), (30, -30)]
    assert r.segments[0].offset == -30  # cut_list sorts a copy
    assert r.percent() == 100 and r.monotone == 0
    middle = _segments_of(*SR.hand("trimmed_middle_is_monotone")[:3])
    assert [g.src_first for g in middle.cut_list()] == [0, 60] and middle.percent() == 51 * 100 // 81
    none = _segments_of(*SR.hand("no_match")[:3])
    assert none.match_range() == (-1, -1, 0) and none.cut_list() == [] and none.percent() == 0
    assert VideoSegments().match_range() == (-1, -1, 0) and VideoSegments().percent() == 0


class _StubIndex:
    """DctVideoIndex.segments from the model"""

    def __init__(self, videos):
        self.videos, self.calls = videos, []

    def segments(self, pairs, p, tol=15, min_frames=None, max_segments=4, maps=True):
        self.calls.append((list(pairs), tol, min_frames, max_segments, maps))
        par = dict(thresh=p.dctThresh, skip=p.skipFrames, tol=tol, min_frames=min_frames or 1, max_segments=max_segments)
        return [_segments_of(self.videos[a], self.videos[b], par) for a, b in pairs]


def test_database_video_segments_sets_two_attributes():
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
    assert video_segments(index, groups, p, min_frames=3) is groups
    assert index.calls == [([(9, 7), (7, 9), (7, 3)], 15, 3, 4, False)]  # one call, no maps
    m = groups[0][1]  # clip 9 is a cut of clip 7
    assert m.aligned == 100 and m.segments.n_segments >= 1 and m.segments.match_range()[0] == 0
    assert 0 < groups[1][1].aligned < 100 and groups[1][2].aligned == 0
    for g, b in zip(groups, before):
        for k, (m, was) in enumerate(zip(g, b)):
            now = dict(vars(m))
            if k > 0 and g[0] is not image:
                assert set(now) - set(was) == {"segments", "aligned"}
                now.pop("segments"), now.pop("aligned")
            assert now == was
    with pytest.raises(ValueError):
        video_segments(index, groups, SearchParams(algo=SearchParams.AlgoDCT))
    with pytest.raises(ValueError):
        video_segments(object(), groups, p)
