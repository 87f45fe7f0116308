"""The rules of the video segments (include/cbird_hip.h, cbh_video_segments) as a NumPy model on the two views of
tests/video_coverage_rules.py, and hand-made pairs for every rule.  Imported by tests/test_video_segments_rules.py (CPU)
and tests/test_video_segments.py / test_video_segments_cpp.py (GPU): the model is the reference of every one of them."""
import numpy as np

import video_coverage_rules as VR
from video_coverage_rules import B, FAR, OTHER, flip, popcount, source_view, dest_view  # noqa: F401

SUMMARY_FIELDS = ("src_frames_total", "src_frames_aligned", "n_src", "n_dst", "n_segments", "n_aligned", "monotone",
                  "src_in", "dst_in", "len")
SEGMENT_FIELDS = ("span_sum", "offset", "n_frames", "src_first", "src_last", "dst_first", "dst_last")


def matches(hs, hd, thresh):
    """per source hash the entries under thresh and their distances, 512 source frames at a time"""
    rows = []
    for a in range(0, len(hs), 512):
        d = popcount(hs[a:a + 512, None] ^ hd[None, :])
        for row in d:
            js = np.nonzero(row < thresh)[0]
            rows.append((js, row[js]))
    return rows


def support(fs, fd, rows, live, tol, omin, n_off):
    """rule 1: per offset of the domain the live source frames with a match within tol of it, each counted once -- a
    frame's windows [o - tol, o + tol] are united before they are counted"""
    d = np.zeros(n_off + 1, np.int64)
    for i in np.nonzero(live)[0]:
        offs = np.unique(fd[rows[i][0]] - fs[i])
        if len(offs) == 0:
            continue
        lo, hi = offs - tol, offs + tol
        first = np.r_[True, lo[1:] > hi[:-1]]  # a window that does not overlap the one before it starts a new stretch
        last = np.r_[first[1:], True]
        np.add.at(d, lo[first] - omin, 1)
        np.add.at(d, hi[last] + 1 - omin, -1)
    return np.cumsum(d)[:n_off]


def pick(sup, omin):
    """rule 2: (max support, the centre of the plateau of it nearest to 0, the negative one of two equally near)"""
    m = int(sup.max())
    at = np.nonzero(sup == m)[0]
    cut = np.nonzero(np.diff(at) > 1)[0]
    los, his = at[np.r_[0, cut + 1]] + omin, at[np.r_[cut, len(at) - 1]] + omin
    centres = [int(lo + hi) // 2 for lo, hi in zip(los, his)]  # // floors toward minus infinity
    return m, min(centres, key=lambda c: (abs(c), c >= 0))


def segments(src, dst, thresh, skip, tol=15, min_frames=1, max_segments=4):
    """(summary dict, [segment dict], src_frame[], dst_frame[], distance[], segment[]) of one ordered pair"""
    sfr, shs = np.asarray(src[0], np.int64), np.asarray(src[1], np.uint64)
    dfr, dhs = np.asarray(dst[0], np.int64), np.asarray(dst[1], np.uint64)
    si, spans = source_view(sfr, shs, skip)
    di = dest_view(dfr, dhs, skip)
    fs, hs, fd, hd = sfr[si], shs[si], dfr[di], dhs[di]
    n = len(fs)
    dst_frame, distance, segment = np.full(n, -1, np.int64), np.full(n, 65, np.int64), np.full(n, -1, np.int64)
    segs = []
    if n and len(fd):
        rows = matches(hs, hd, thresh)
        omin, omax = int(fd.min() - fs.max() - tol), int(fd.max() - fs.min() + tol)
        live = np.ones(n, bool)
        while len(segs) < max_segments:
            m, c = pick(support(fs, fd, rows, live, tol, omin, omax - omin + 1), omin)
            if m < min_frames or m == 0:
                break
            members = []
            for i in np.nonzero(live)[0]:
                js, ds = rows[i]
                delta = np.abs(fd[js] - fs[i] - c)
                near = delta <= tol
                if not near.any():
                    continue
                _, d, j = min(zip(delta[near].tolist(), ds[near].tolist(), js[near].tolist()))  # rule 3
                members.append(i)
                dst_frame[i], distance[i], segment[i], live[i] = fd[j], d, len(segs), False
            assert len(members) == m
            a, b = members[0], members[-1]
            segs.append(dict(span_sum=int(spans[members].sum()), offset=c, n_frames=m, src_first=int(fs[a]),
                             src_last=int(fs[b]), dst_first=int(dst_frame[a]), dst_last=int(dst_frame[b])))
    order = sorted(range(len(segs)), key=lambda r: segs[r]["src_first"])  # (stable: the earlier segment of two equals)
    placed = [segs[r]["src_first"] + segs[r]["offset"] for r in order]
    s = dict(src_frames_total=int(spans.sum()), src_frames_aligned=int(spans[segment >= 0].sum()), n_src=n, n_dst=len(fd),
             n_segments=len(segs), n_aligned=int((segment >= 0).sum()),
             monotone=int(all(x <= y for x, y in zip(placed, placed[1:]))), src_in=-1, dst_in=-1, len=0)
    if segs:
        s.update(src_in=segs[0]["src_first"], dst_in=segs[0]["dst_first"],
                 len=segs[0]["dst_last"] - segs[0]["dst_first"] + 1)
    return s, segs, fs.astype(np.int32), dst_frame.astype(np.int32), distance.astype(np.int32), segment.astype(np.int32)


def cut_list(segs):
    """VideoSegments.cut_list: the segments in source order"""
    return sorted(segs, key=lambda g: g["src_first"])


# ---- hand-made pairs ------------------------------------------------------------------------------------------------------
def _v(frames, hashes):
    return np.asarray(frames, np.int32), np.asarray(hashes, np.uint64)


def _far(ks):
    return [FAR[k] for k in ks]


def _seg(offset, n_frames, src_first, src_last, dst_first, dst_last, span_sum):
    return dict(span_sum=span_sum, offset=offset, n_frames=n_frames, src_first=src_first, src_last=src_last,
                dst_first=dst_first, dst_last=dst_last)


_TEN = list(range(0, 100, 10))
# name -> (source, destination, dict(thresh, skip, tol, min_frames, max_segments), the summary fields, the segments and the
# map columns written down by hand)
HAND = {
    # every frame matches its own copy only: offsets 0, support 10 on [-2, 2], the centre 0
    "copy_plateau_centre": (_v(_TEN, FAR[:10]), _v(_TEN, FAR[:10]), dict(tol=2),
                            dict(n_segments=1, n_aligned=10, src_frames_total=91, src_frames_aligned=91, monotone=1, src_in=0,
                                 dst_in=0, len=91),
                            [_seg(0, 10, 0, 90, 0, 90, 91)], dict(dst_frames=_TEN, segments=[0] * 10)),
    # shifted by 100: the plateau is [98, 102]; its edge 98 would be the first offset of the maximum
    "shifted_copy_centre_not_edge": (_v(_TEN, FAR[:10]), _v([f + 100 for f in _TEN], FAR[:10]), dict(tol=2),
                                     dict(src_in=0, dst_in=100, len=91), [_seg(100, 10, 0, 90, 100, 190, 91)], {}),
    # destination frames jittered: offsets 7, 9, 10, 11, 13 with tol 3 -> all five only at 10
    "jitter_gives_the_true_offset": (_v([0, 10, 20, 30, 40], FAR[:5]), _v([7, 19, 30, 41, 53], FAR[:5]), dict(tol=3),
                                     {}, [_seg(10, 5, 0, 40, 7, 53, 41)], {}),
    # two frames, each found at -7 and at +7: support 2 on [-9, -5] and on [5, 9]; centres -7 and 7, the negative wins
    "equal_support_negative_wins": (_v([100, 200], FAR[:2]), _v([93, 107, 193, 207], _far([0, 0, 1, 1])), dict(tol=2), {},
                                    [_seg(-7, 2, 100, 200, 93, 193, 101)], dict(dst_frames=[93, 193])),
    # runs [-12, -8] (centre -10) and [3, 7] (centre 5): the smaller |c|
    "two_runs_smaller_centre": (_v([100, 200], FAR[:2]), _v([90, 105, 190, 205], _far([0, 0, 1, 1])), dict(tol=2), {},
                                [_seg(5, 2, 100, 200, 105, 205, 101)], {}),
    # runs [-8, -5] (centre floor(-6.5) = -7) and [5, 8] (centre floor(6.5) = 6): floor is toward minus infinity, 6 is nearer
    "floor_is_toward_minus_infinity": (_v([100, 200], FAR[:2]), _v([93, 94, 106, 107, 193, 194, 206, 207],
                                                                   _far([0, 0, 0, 0, 1, 1, 1, 1])), dict(tol=1), {},
                                       [_seg(6, 2, 100, 200, 106, 206, 101)], dict(dst_frames=[106, 206])),
    # one frame, matches 2 tol + 1 = 5 apart: [8, 12] and [13, 17] touch, one run [8, 17], centre 12; the nearer match is 10
    "intervals_touch": (_v([0], [B]), _v([10, 15], [B, B]), dict(tol=2), {}, [_seg(12, 1, 0, 0, 10, 10, 1)], {}),
    # 2 tol + 2 = 6 apart: [8, 12] and [14, 18], offset 13 between them has support 0; two runs, centres 10 and 16
    "one_offset_between_intervals": (_v([0], [B]), _v([10, 16], [B, B]), dict(tol=2), {}, [_seg(10, 1, 0, 0, 10, 10, 1)],
                                     {}),
    # frames 0..40 lie at +100, frames 50..60 at +300; frame 20 is ALSO at +300: it goes to the first segment (offset 100)
    "peeling_earlier_segment_keeps_the_frame": (
        _v([0, 10, 20, 30, 40, 50, 60], FAR[:7]),
        _v([100, 110, 120, 130, 140, 320, 350, 360], _far([0, 1, 2, 3, 4, 2, 5, 6])), dict(tol=2),
        dict(n_segments=2, n_aligned=7, monotone=1),
        [_seg(100, 5, 0, 40, 100, 140, 50), _seg(300, 2, 50, 60, 350, 360, 11)],
        dict(dst_frames=[100, 110, 120, 130, 140, 350, 360], segments=[0, 0, 0, 0, 0, 1, 1])),
    "min_frames_at_the_support": ("peeling_earlier_segment_keeps_the_frame", dict(tol=2, min_frames=5),
                                  dict(n_segments=1, n_aligned=5, src_frames_aligned=50), 1),
    "min_frames_above_the_support": ("peeling_earlier_segment_keeps_the_frame", dict(tol=2, min_frames=6),
                                     dict(n_segments=0, n_aligned=0, src_in=-1, dst_in=-1, len=0, monotone=1), 0),
    "min_frames_below_the_support": ("peeling_earlier_segment_keeps_the_frame", dict(tol=2, min_frames=4),
                                     dict(n_segments=1), 1),
    "max_segments_cuts_the_list": ("peeling_earlier_segment_keeps_the_frame", dict(tol=2, max_segments=1),
                                   dict(n_segments=1, n_aligned=5), 1),
    # tol 0: offsets 10, 10, 11 -> support 2 at 10 alone, then frame 20 alone at 11
    "tol_0": (_v([0, 10, 20], FAR[:3]), _v([10, 20, 31], FAR[:3]), dict(tol=0), dict(n_segments=2),
              [_seg(10, 2, 0, 10, 10, 20, 20), _seg(11, 1, 20, 20, 31, 31, 1)], {}),
    # the source is the longer video: its frames 500.. are the destination's 0..
    "negative_offset": (_v([0, 250, 500, 510, 520, 530, 900], _far([10, 11, 0, 1, 2, 3, 12])), _v([0, 10, 20, 30], FAR[:4]),
                        dict(tol=2), dict(n_aligned=4, src_frames_total=901, src_frames_aligned=400, src_in=500, dst_in=0, len=31),
                        [_seg(-500, 4, 500, 530, 0, 30, 400)], dict(segments=[-1, -1, 0, 0, 0, 0, -1],
                                                                    distances=[65, 65, 0, 0, 0, 0, 65])),
    # skip 20, last 100: the source keeps 20..80; the destination (100 / 2 > 20) too, so frames 0, 10, 90, 100 never pair
    "trim_both_views": (_v(list(range(0, 101, 10)), FAR[:11]), _v(list(range(0, 101, 10)), FAR[:11]), dict(tol=2, skip=20),
                        dict(n_src=7, n_dst=7, n_aligned=7, src_frames_total=70), [_seg(0, 7, 20, 80, 20, 80, 70)], {}),
    # last 40: 40 / 2 is not above 20, the destination keeps all five entries; the source keeps frame 20 alone
    "trim_source_only": (_v([0, 10, 20, 30, 40], FAR[:5]), _v([0, 10, 20, 30, 40], FAR[:5]), dict(tol=2, skip=20),
                         dict(n_src=1, n_dst=5), [_seg(0, 1, 20, 20, 20, 20, 10)], {}),
    "empty_source_view": (_v([0, 10], FAR[:2]), _v([0, 10], FAR[:2]), dict(tol=2, skip=20),
                          dict(n_src=0, n_dst=2, n_segments=0, monotone=1, src_in=-1, dst_in=-1, len=0, src_frames_total=0),
                          [], dict(frames=[])),
    "empty_destination": (_v([0, 4], [B, B]), _v([0, 1], [0, (1 << 64) - 1]), dict(tol=2),
                          dict(n_src=2, n_dst=0, n_segments=0, src_frames_total=5, src_frames_aligned=0), [],
                          dict(dst_frames=[-1, -1], distances=[65, 65], segments=[-1, -1])),
    "no_match": (_v([0, 4], OTHER[:2]), _v([0, 4], FAR[:2]), dict(tol=2), dict(n_segments=0, n_aligned=0, monotone=1), [],
                 dict(dst_frames=[-1, -1], distances=[65, 65], segments=[-1, -1])),
    # scenes A = frames 0..20 and B = 30..50 of the source stand swapped in the destination: A at +100, B at -30
    "swapped_scenes_not_monotone": (_v([0, 10, 20, 30, 40, 50], FAR[:6]), _v([0, 10, 20, 100, 110, 120], _far([3, 4, 5, 0, 1, 2])),
                                    dict(tol=2), dict(n_segments=2, monotone=0, src_in=30, dst_in=0, len=21),
                                    [_seg(-30, 3, 30, 50, 0, 20, 21), _seg(100, 3, 0, 20, 100, 120, 30)], {}),
    # the destination lacks the middle: frames 0..20 at 0, frames 60..80 at -30
    "trimmed_middle_is_monotone": (_v([0, 10, 20, 30, 40, 50, 60, 70, 80], FAR[:9]), _v([0, 10, 20, 30, 40, 50], _far([0, 1, 2, 6, 7, 8])),
                                   dict(tol=2), dict(n_segments=2, monotone=1, n_aligned=6, src_frames_aligned=51),
                                   [_seg(0, 3, 0, 20, 0, 20, 30), _seg(-30, 3, 60, 80, 30, 50, 21)],
                                   dict(segments=[0, 0, 0, -1, -1, -1, 1, 1, 1])),
    # equal offset distance 1 on both sides of the centre: the smaller Hamming distance, then the lower entry
    "member_takes_nearest_then_distance_then_entry": (
        _v([0, 10, 20, 30], FAR[:4]),
        _v([100, 110, 119, 121, 129, 131], [FAR[0], FAR[1], flip(FAR[2], [0, 1]), flip(FAR[2], [2]), flip(FAR[3], [0]),
                                             flip(FAR[3], [1])]), dict(tol=2), {},
        [_seg(100, 4, 0, 30, 100, 129, 31)], dict(dst_frames=[100, 110, 121, 129], distances=[0, 0, 1, 1])),
}
DEFAULTS = dict(thresh=5, skip=0, tol=15, min_frames=1, max_segments=4)


def hand(name):
    """(source, destination, parameters, summary fields, segments or None, map columns) of one hand-made pair; an entry
    that names another one takes its videos and the first so many of its segments"""
    e = HAND[name]
    if isinstance(e[0], str):
        base = HAND[e[0]]
        e = (base[0], base[1], e[1], e[2], base[4][:e[3]], {})
    return e[0], e[1], {**DEFAULTS, **e[2]}, e[3], e[4], e[5]


def run(src, dst, par):
    return segments(src, dst, par["thresh"], par["skip"], par["tol"], par["min_frames"], par["max_segments"])


def sized_videos():
    """sources of 1, 63, 64, 65, 129 frames and destinations of 1, 255, 256, 257 and 600 entries (above the 256-entry LDS
    stage) cut from one random walk, the destinations with noise; every source against every destination"""
    rng = np.random.default_rng(11)
    n = 700
    step = np.zeros(n, np.uint64)
    for _ in range(2):
        step ^= np.uint64(1) << rng.integers(0, 64, n).astype(np.uint64)
    step[0] = rng.integers(0, 2**63, dtype=np.uint64)
    walk = np.bitwise_xor.accumulate(step)
    frames = np.cumsum(rng.integers(1, 6, n)).astype(np.int32) - 1
    src_lengths, dst_lengths = [1, 63, 64, 65, 129], [1, 255, 256, 257, 600]
    videos = []
    for m in src_lengths:
        a = int(rng.integers(0, 300))
        videos.append(((frames[a:a + m] - frames[a]).astype(np.int32), walk[a:a + m].copy()))
    for m in dst_lengths:
        a = int(rng.integers(0, n - m + 1))
        h = walk[a:a + m] ^ np.where(rng.random(m) < 0.3, np.uint64(1) << rng.integers(0, 64, m).astype(np.uint64), np.uint64(0))
        videos.append(((frames[a:a + m] - frames[a] + int(rng.integers(0, 3))).astype(np.int32), h))
    pairs = [(a, len(src_lengths) + b) for a in range(len(src_lengths)) for b in range(len(dst_lengths))]
    return videos, pairs


def static_videos():
    """a 300-frame static run on both sides, between moving stretches: every static frame matches 300 entries"""
    rng = np.random.default_rng(12)
    moving = rng.integers(0, 2**63, 80, dtype=np.uint64)
    still = np.full(300, moving[40], np.uint64)
    h = np.concatenate([moving[:40], still, moving[40:]])
    f = np.cumsum(rng.integers(1, 4, len(h))).astype(np.int32) - 1
    return [(f, h), ((f[20:] - f[20] + 500).astype(np.int32), h[20:].copy())], [(0, 1), (1, 0)]
