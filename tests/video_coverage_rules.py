"""The rules of the video coverage map (include/cbird_hip.h, cbh_video_coverage) as a NumPy model, a restated findVideo
(src/dctvideoindex.cpp:399-657) to hold the model against, and hand-made pairs for every rule.  Imported by
tests/test_video_coverage_rules.py (CPU) and tests/test_video_coverage.py / test_video_coverage_cpp.py (GPU): the model is
the reference of every one of them."""
import numpy as np

FIELDS = ("src_frames_total", "src_frames_covered", "gap_len", "gap_begin", "n_src", "n_dst", "n_covered", "n_low_detail",
          "near_percent", "src_in", "dst_in", "len", "dst_min", "dst_max")
FRAME_MARGIN = 15  # findVideo's frameMargin (:593)


def popcount(x):
    x = np.ascontiguousarray(x, np.uint64)
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x).astype(np.int64)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int64)


def flip(h, bits):
    for b in bits:
        h ^= 1 << b
    return h


def source_view(frames, hashes, skip):
    """the frames findVideo searches (:431): positions in the list, and the span of every one of them"""
    f = np.asarray(frames, np.int64)
    if len(f) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    last = f[-1]
    keep = ~((f < skip) | (f > last - skip))  # unconditional
    spans = np.append(np.diff(f), 1)  # up to the next stored frame of the UNTRIMMED list; 1 for the last
    return np.nonzero(keep)[0], spans[keep]


def dest_view(frames, hashes, skip):
    """the entries insertHashes stores (:61-111): positions in the list"""
    f = np.asarray(frames, np.int64)
    if len(f) == 0:
        return np.zeros(0, np.int64)
    pc = popcount(np.asarray(hashes, np.uint64))
    keep = (pc >= 5) & (64 - pc >= 5)
    last = int(f[-1])
    if skip and last // 2 > skip:  # the trim is conditional here
        keep &= ~((f < skip) | (f > last - skip))
    return np.nonzero(keep)[0]


def nearest(sh, dh):
    """per source hash (distance, entry) of the minimum of distance << 24 | entry; (65, -1) without entries"""
    if len(dh) == 0:
        return np.full(len(sh), 65, np.int64), np.full(len(sh), -1, np.int64)
    dist, entry = np.empty(len(sh), np.int64), np.empty(len(sh), np.int64)
    for a in range(0, len(sh), 512):
        d = popcount(sh[a:a + 512, None] ^ dh[None, :])
        key = (d << 24 | np.arange(len(dh), dtype=np.int64)[None, :]).min(axis=1)
        dist[a:a + 512], entry[a:a + 512] = key >> 24, key & 0xffffff
    return dist, entry


def coverage(src, dst, thresh, skip):
    """(summary dict, src_frame[], dst_frame[], distance[]) of one ordered pair of (frames, hashes) lists"""
    sfr, shs = np.asarray(src[0], np.int64), np.asarray(src[1], np.uint64)
    dfr, dhs = np.asarray(dst[0], np.int64), np.asarray(dst[1], np.uint64)
    si, spans = source_view(sfr, shs, skip)
    di = dest_view(dfr, dhs, skip)
    dist, entry = nearest(shs[si], dhs[di])
    frames = sfr[si]
    dframes = np.where(entry >= 0, dfr[di][np.maximum(entry, 0)] if len(di) else -1, -1)
    covered = dist < thresh
    pc = popcount(shs[si])
    s = dict.fromkeys(FIELDS, 0)
    s.update(n_src=len(si), n_dst=len(di), n_covered=int(covered.sum()),
             n_low_detail=int(((pc < 5) | (64 - pc < 5)).sum()), src_frames_total=int(spans.sum()),
             src_frames_covered=int(spans[covered].sum()), src_in=-1, dst_in=-1, dst_min=-1, dst_max=-1)
    if covered.any():
        cs, cd = frames[covered], dframes[covered]
        adjacent, last = 0, 0  # `int lastFrame = 0` (:608)
        for x in cd:
            adjacent += abs(int(x) - last) < FRAME_MARGIN
            last = int(x)
        s.update(near_percent=adjacent * 100 // len(cd), src_in=int(cs[0]), dst_in=int(cd[0]),
                 len=int(max(cs[-1] - cs[0], cd[-1] - cd[0])), dst_min=int(cd.min()), dst_max=int(cd.max()))
    # the longest run of uncovered frames, by the sum of its spans; the earliest among equals
    i = 0
    while i < len(frames):
        if covered[i]:
            i += 1
            continue
        j = i
        while j < len(frames) and not covered[j]:
            j += 1
        run = int(spans[i:j].sum())
        if run > s["gap_len"]:
            s["gap_len"], s["gap_begin"] = run, int(frames[i])
        i = j
    return s, frames.astype(np.int32), dframes.astype(np.int32), dist.astype(np.int32)


def find_video(needle, videos, thresh, skip):
    """findVideo with minFramesMatched 1, minFramesNear 0 and no self filter, restated from the reference and on its own
    feet (nothing of coverage() above but the two views): {video index: (num, percentNear, srcIn, dstIn, len)}"""
    nfr, nhs = np.asarray(needle[0], np.int64), np.asarray(needle[1], np.uint64)
    si, _ = source_view(nfr, nhs, skip)
    cand = {}
    for v, (vf, vh) in enumerate(videos):
        vf, vh = np.asarray(vf, np.int64), np.asarray(vh, np.uint64)
        di = dest_view(vf, vh, skip)
        for i in si:
            closest = None  # closestMatch[id] (:499-502): strictly nearer replaces, so the earliest among equals stays
            for e in di:
                d = bin(int(nhs[i]) ^ int(vh[e])).count("1")
                if d < thresh and (closest is None or d < closest[0]):
                    closest = (d, int(vf[e]))
            if closest is not None:
                cand.setdefault(v, []).append((int(nfr[i]), closest[1]))
    out = {}
    for v, ranges in cand.items():
        ranges.sort(key=lambda r: r[0])
        adjacent, last = 0, 0
        for _, frame in ranges:
            adjacent += abs(frame - last) < FRAME_MARGIN
            last = frame
        num = len(ranges)
        out[v] = (num, adjacent * 100 // num, ranges[0][0], ranges[0][1],
                  max(ranges[-1][0] - ranges[0][0], ranges[-1][1] - ranges[0][1]))
    return out


def ranges(frames, spans, flags):
    """VideoCoverage.ranges: runs of set flags as (first frame, sum of spans)"""
    out, i = [], 0
    while i < len(flags):
        if not flags[i]:
            i += 1
            continue
        j = i
        while j < len(flags) and flags[j]:
            j += 1
        out.append((int(frames[i]), int(np.sum(spans[i:j]))))
        i = j
    return out


# ---- hand-made pairs ------------------------------------------------------------------------------------------------------
B = 0x0123456789ABCDEF  # 32 bits set
_rng = np.random.default_rng(20)
FAR = [int(x) for x in _rng.integers(0, 2**63, 64, dtype=np.uint64)]  # pairwise some 32 bits apart
assert min(bin(a ^ b).count("1") for i, a in enumerate(FAR) for b in FAR[:i]) >= 12
OTHER = [int(x) for x in _rng.integers(0, 2**63, 64, dtype=np.uint64)]  # what an uncovered frame shows
assert min(bin(a ^ b).count("1") for a in OTHER for b in FAR) >= 12


def _v(frames, hashes):
    return np.asarray(frames, np.int32), np.asarray(hashes, np.uint64)


def _pattern(frames, covered, dst_frames=None):
    """a source whose frame k is an exact copy of destination frame k where covered[k], and far from all of it where not"""
    n = len(frames)
    src = _v(frames, [FAR[k] if covered[k] else OTHER[k] for k in range(n)])
    dst = _v(dst_frames if dst_frames is not None else frames, FAR[:n])
    return src, dst


_M = (1 << 64) - 1
_TRIM = [0, 10, 20, 30, 40]
# name -> (source, destination, thresh, skip, the fields and map columns written down by hand)
HAND = {
    # 3, 1, 1 bits away: the lowest entry of the two nearest
    "tie_takes_lowest_entry": (_v([0], [B]), _v([0, 10, 20], [flip(B, [0, 1, 2]), flip(B, [3]), flip(B, [4])]), 5, 0,
                               dict(dst_frames=[10], distances=[1], n_covered=1, dst_in=10)),
    "distance_0_and_64": (_v([0, 1], [B, B ^ _M]), _v([0], [B]), 64, 0,
                          dict(distances=[0, 64], n_covered=1, src_frames_covered=1, src_frames_total=2, gap_begin=1,
                               gap_len=1)),
    "distance_64_under_65": (_v([0, 1], [B, B ^ _M]), _v([0], [B]), 65, 0, dict(distances=[0, 64], n_covered=2, gap_len=0)),
    "thresh_minus_one_is_covered": (_v([0, 1], [flip(B, [1, 2, 3, 4]), flip(B, [1, 2, 3, 4, 5])]), _v([7], [B]), 5, 0,
                                    dict(distances=[4, 5], n_covered=1, src_in=0, dst_in=7, gap_begin=1, gap_len=1)),
    # last / 2 > skip: 40 / 2 = 20 is not above 20, the destination keeps all five; the source trim does not ask
    "trim_boundary_not_above": (_v(_TRIM, FAR[:5]), _v(_TRIM, FAR[:5]), 5, 20,
                                dict(n_src=1, n_dst=5, frames=[20], dst_frames=[20], distances=[0], src_frames_total=10)),
    "trim_boundary_odd_last": (_v([0, 10, 20, 30, 41], FAR[:5]), _v([0, 10, 20, 30, 41], FAR[:5]), 5, 20,
                               dict(n_src=1, n_dst=5, frames=[20], dst_frames=[20], distances=[0])),
    # 42 / 2 = 21 is above 20: only frame 20 stays an entry, frame 30 of the source finds it 30-odd bits away
    "trim_boundary_above": (_v([0, 10, 20, 22, 42], FAR[:5]), _v([0, 10, 20, 30, 42], FAR[:5]), 5, 20,
                            dict(n_src=2, n_dst=1, frames=[20, 22], dst_frames=[20, 20], n_covered=1,
                                 src_frames_total=22, src_frames_covered=2, gap_begin=22, gap_len=20)),
    "trim_skip_19": (_v(_TRIM, FAR[:5]), _v(_TRIM, FAR[:5]), 5, 19, dict(n_src=1, n_dst=1, frames=[20], dst_frames=[20])),
    # 4 and 60 set bits are no entries, 5 and 59 are; the source's own 4-bit hash is searched all the same
    "detail_rule_on_the_destination": (_v([0], [0xF]), _v([0, 1, 2, 3], [0xF, 0x1F, 0x1F ^ _M, 0xF ^ _M]), 5, 0,
                                       dict(n_dst=2, n_low_detail=1, dst_frames=[1], distances=[1], n_covered=1)),
    "empty_destination": (_v([0, 4], [B, B]), _v([0, 1], [0, _M]), 5, 0,
                          dict(n_src=2, n_dst=0, dst_frames=[-1, -1], distances=[65, 65], n_covered=0, near_percent=0,
                               src_in=-1, dst_in=-1, len=0, dst_min=-1, dst_max=-1, gap_begin=0, gap_len=5,
                               src_frames_total=5)),
    "no_destination_frames": (_v([3], [B]), _v([], []), 5, 0, dict(n_dst=0, dst_frames=[-1], distances=[65], gap_begin=3)),
    "source_trimmed_to_nothing": (_v([0, 10], FAR[:2]), _v([0, 10], FAR[:2]), 5, 20,
                                  dict(n_src=0, n_dst=2, n_covered=0, src_frames_total=0, gap_len=0, gap_begin=0, src_in=-1,
                                       frames=[], distances=[])),
    "no_source_frames": (_v([], []), _v([0], [B]), 5, 0, dict(n_src=0, n_dst=1, src_frames_total=0)),
    "span_of_the_last_frame": (*_pattern([0, 5, 9], [1, 1, 1]), 5, 0, dict(src_frames_total=10, src_frames_covered=10)),
    # the last considered frame's span reaches to the next STORED frame, which the trim dropped
    "span_reaches_into_the_trim": (*_pattern([0, 5, 9, 30], [1, 1, 0, 1]), 5, 5,
                                   dict(frames=[5, 9], n_src=2, src_frames_total=25, src_frames_covered=4, gap_begin=9,
                                        gap_len=21)),
    "gap_tie_takes_the_earliest": (*_pattern([0, 1, 2, 3, 4, 5, 6], [1, 0, 0, 1, 0, 0, 1]), 5, 0,
                                   dict(gap_begin=1, gap_len=2, n_covered=3)),
    # one frame that stands for seven beats two frames that stand for two
    "gap_is_measured_in_frame_numbers": (*_pattern([0, 1, 2, 3, 4, 11, 12], [1, 0, 0, 1, 0, 1, 1]), 5, 0,
                                         dict(gap_begin=4, gap_len=7)),
    "gap_at_the_end": (*_pattern([0, 1, 2, 9], [1, 1, 0, 0]), 5, 0, dict(gap_begin=2, gap_len=8)),
    # lastFrame starts at 0: the first match at 100 is not adjacent, 105 is, 300 is not
    "near_percent_starts_at_frame_0": (*_pattern([0, 1, 2], [1, 1, 1], [100, 105, 300]), 5, 0,
                                       dict(near_percent=33, src_in=0, dst_in=100, len=200, dst_min=100, dst_max=300)),
    "near_percent_first_match_near_0": (*_pattern([0, 1, 2], [1, 0, 1], [14, 20, 28]), 5, 0,
                                        dict(near_percent=100, dst_in=14, len=14, n_covered=2)),
    "near_percent_margin_is_strict": (*_pattern([0, 1], [1, 1], [15, 30]), 5, 0, dict(near_percent=0)),
}


def clips():
    """the set the rules were checked on: 12 clips of 70 frames, the last four sub-clips of earlier ones"""
    from cbird_amd import synth_video

    return synth_video.make_clips(12, n_frames=70, seed=7, subclip_frac=0.34, max_gap=9)
