"""The rules of the two per-needle reductions (cbird_amd/csrc/reduce.hip: K8 of findVideo, K5 of the keypoint vote), as
plain Python, and small fixtures that put a case on each rule's edge.

No GPU, no ctypes, no numpy: lists, dicts and Python integers.  Both models restate the reference text -- findVideo from
src/dctvideoindex.cpp (insertHashes :61-111, findVideo :399-657), the vote from src/dctfeaturesindex.cpp:291-358 -- and
not video.hip, reduce.hip or the C oracle, so that all of those can be held against them.  Candidates are every entry
with hamm64 < dctThresh (the exact search, vradix 0); their order is the entry order for findVideo (video by video in
_mediaId order, frame by frame inside one) and (distance, media id) for the vote: the project's fixed reading of the
trees' orders, pinned by the golden files.

Each model takes variant=: one rule switched to a plausible wrong form (VIDEO_VARIANTS, VOTE_VARIANTS).  A fixture that
gives another answer under a variant would catch a kernel with that mistake; KILLS names, per variant, fixtures that do
(tests/test_reduce_rules.py asserts it, without any kernel).

Hashes: base(i) are 126 words of popcount 32 that are pairwise 32 or 64 bits apart (the first-order Reed-Muller code of
length 64 under a fixed shuffle of the bit positions, so that the two 32-bit halves of a word are unrelated); flip(h,
bits...) makes a near copy.  A copy is its number of flipped bits from its base and at least 32 - 2 * 7 from anything
made from another base, so every distance in a fixture is known by construction.
"""
from __future__ import annotations

import dataclasses
import functools
import random
import struct

FRAME_MARGIN = 15  # `const int frameMargin = 15` (:593)
M64 = (1 << 64) - 1


def popc(x: int) -> int:
    return bin(x).count("1")


def hamm64(a: int, b: int) -> int:
    return popc(a ^ b)


# ---- findVideo ---------------------------------------------------------------------------------------------------
VIDEO_VARIANTS = (
    "margin_le",                 # abs(dst - last) <= 15
    "last_from_first",           # lastFrame starts at the first matched frame instead of 0
    "tie_last",                  # the last entry, not the first, wins a distance tie (<= for <, :501)
    "first_match_wins",          # the first entry under the threshold wins, whatever its distance
    "gate_matched_le",           # num <= minFramesMatched rejects
    "gate_near_le",              # percentNear <= minFramesNear rejects
    "len_src_only",              # len = srcLen
    "len_abs_dst",               # len = max(srcLen, abs(dstLen))
    "percent_rounded",           # percentNear rounded to nearest instead of truncated
    "group_by_video",            # closest match and candidates per video instead of per media id
    "index_trim_unconditional",  # index-side trim without `lastFrame / 2 > skip`
    "needle_trim_conditional",   # needle-side trim only when `lastFrame / 2 > skip`
    "detail_4_60",               # detail bounds 4/60 instead of 5/59
    "self_always_filtered",      # the needle's own media dropped even when filterSelf is off
    "order_by_video",            # results in _mediaId (video) order instead of ascending media id
)


@dataclasses.dataclass(frozen=True)
class VParams:
    thresh: int = 5  # dctThresh: a candidate has hamm64 < thresh
    skip: int = 0  # skipFrames
    vfm: int = 1  # minFramesMatched
    vfn: int = 0  # minFramesNear
    filter_self: bool = True


def video_entries(index, skip: int, variant: str | None = None):
    """insertHashes (:61-111) over every video of `index` = [(media id, frames, hashes)] in _mediaId order: the tree's
    values as (video index, frame, hash), in insertion order"""
    lo, hi = (4, 60) if variant == "detail_4_60" else (5, 59)
    out = []
    for vi, (_mid, frames, hashes) in enumerate(index):
        if not frames:
            continue  # (:73-75)
        last_frame = frames[-1]
        for frame, h in zip(frames, hashes):
            if popc(h) < lo or popc(h) > hi:  # hamm64(hash, 0) < 5 || hamm64(hash, ~0) < 5 (:89)
                continue
            trim = skip and (variant == "index_trim_unconditional" or last_frame // 2 > skip)  # (:93)
            if trim and (frame < skip or frame > last_frame - skip):
                continue
            out.append((vi, frame, h))
    return out


def find_video(index, needle, p: VParams, variant: str | None = None):
    """DctVideoIndex::findVideo of needle = (media id, frames, hashes): [(mediaId, score, srcIn, dstIn, len)]"""
    assert variant is None or variant in VIDEO_VARIANTS, variant
    needle_id, nframes, nhashes = needle
    if not nframes:
        return []  # "needle video index is empty" (:417-420)
    entries = video_entries(index, p.skip, variant)
    media_of = [mid for mid, _f, _h in index]
    last_frame = nframes[-1]
    trim = True
    if variant == "needle_trim_conditional":
        trim = bool(p.skip) and last_frame // 2 > p.skip
    cand = {}  # group -> [(srcIn, dstIn)]
    for src, q in zip(nframes, nhashes):
        if trim and (src < p.skip or src > last_frame - p.skip):  # (:431)
            continue
        closest = {}  # group -> (distance, frame), cleared per needle frame (:483)
        for vi, frame, h in entries:
            d = hamm64(q, h)
            if not d < p.thresh:
                continue
            mid = media_of[vi]
            if mid == needle_id and (p.filter_self or variant == "self_always_filtered"):  # (:494)
                continue
            key = vi if variant == "group_by_video" else mid
            if key not in closest:
                closest[key] = (d, frame)
            elif variant == "first_match_wins":
                pass
            elif d < closest[key][0] or (variant == "tie_last" and d == closest[key][0]):  # (:501)
                closest[key] = (d, frame)
        for key, (_d, frame) in closest.items():
            cand.setdefault(key, []).append((src, frame))  # (:507-508)
    results = []
    for key, ranges in cand.items():
        ranges = sorted(ranges, key=lambda r: r[0])  # MatchRange::operator< compares srcIn (:600)
        num_adjacent = 0
        last = ranges[0][1] if variant == "last_from_first" else 0  # `int lastFrame = 0` (:608)
        for _src, dst in ranges:
            gap = abs(dst - last)
            if gap < FRAME_MARGIN or (variant == "margin_le" and gap == FRAME_MARGIN):  # (:611)
                num_adjacent += 1
            last = dst
        num = len(ranges)
        percent_near = num_adjacent * 100 // num  # ints, both >= 0: C's division truncates like // (:616)
        if variant == "percent_rounded":
            percent_near = (num_adjacent * 200 + num) // (2 * num)
        if num < p.vfm or (variant == "gate_matched_le" and num == p.vfm):  # (:619)
            continue
        if percent_near < p.vfn or (variant == "gate_near_le" and percent_near == p.vfn):  # (:637)
            continue
        src_len = ranges[-1][0] - ranges[0][0]
        dst_len = ranges[-1][1] - ranges[0][1]
        length = max(src_len, dst_len)  # (:649-651)
        if variant == "len_src_only":
            length = src_len
        elif variant == "len_abs_dst":
            length = max(src_len, abs(dst_len))
        mid = media_of[key] if variant == "group_by_video" else key
        results.append((key, (mid, 100 - percent_near, ranges[0][0], ranges[0][1], length)))
    if variant == "order_by_video":
        first = {}
        for vi, mid in enumerate(media_of):
            first.setdefault(mid, vi)
        results.sort(key=lambda kr: first[kr[1][0]])
    elif variant == "group_by_video":
        results.sort(key=lambda kr: (kr[1][0], kr[0]))
    else:
        results.sort(key=lambda kr: kr[0])  # QMap<mediaid_t, ...>: ascending media id
    return [r for _k, r in results]


# ---- the keypoint vote -------------------------------------------------------------------------------------------
VOTE_VARIANTS = (
    "removed_take_no_place",  # removed entries dropped before the cut of 10
    "own_votes_count",        # the needle's own votes raise maxMatches
    "tie_highest_id",         # equal distances ordered by descending media id
    "branch_per_media",       # the `maxMatches == 1` branch taken where the MEDIA has one vote
)


def _f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


def find_features(rows, needle_hashes, needle_id: int, thresh: int, variant: str | None = None):
    """DctFeaturesIndex::find (:291-358) over rows = [(media id, hash)], id 0 = a removed entry: [(mediaId, score)]"""
    assert variant is None or variant in VOTE_VARIANTS, variant
    votes, sums = {}, {}
    max_matches = 0
    for q in needle_hashes:
        cand = [(hamm64(q, h), mid) for mid, h in rows if hamm64(q, h) < thresh]
        if variant == "removed_take_no_place":
            cand = [c for c in cand if c[1] != 0]
        cand.sort(key=(lambda c: (c[0], -c[1])) if variant == "tie_highest_id" else None)
        for d, mid in cand[:10]:  # (:301)
            if mid <= 0:  # "zero index means deleted" (:307)
                continue
            votes[mid] = votes.get(mid, 0) + 1
            sums[mid] = sums.get(mid, 0) + d
            if mid != needle_id or variant == "own_votes_count":  # (:322)
                max_matches = max(max_matches, votes[mid])
    out = []
    for mid in sorted(votes):  # QMap keys
        if mid == needle_id:
            score = -1
        elif (votes[mid] if variant == "branch_per_media" else max_matches) == 1:
            avg = _f32(sums[mid] / votes[mid])  # `(float) scores / matches`: small integers, one rounding
            score = int(_f32(10 * avg))  # `match.score = 10 * avgScore` (:347)
        else:
            score = max_matches - votes[mid]
        out.append((mid, score))
    return out


# ---- hashes ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bases():
    perm = list(range(64))
    random.Random(64).shuffle(perm)
    out = []
    for a in range(1, 64):
        for a0 in (0, 1):
            w = 0
            for x in range(64):
                if a0 ^ (popc(a & x) & 1):
                    w |= 1 << perm[x]
            out.append(w)
    assert all(popc(w) == 32 for w in out)
    assert all(hamm64(out[i], out[j]) >= 24 for i in range(len(out)) for j in range(i))
    return tuple(out)


def base(i: int) -> int:
    return _bases()[i]


def flip(h: int, *bits: int) -> int:
    assert len(set(bits)) == len(bits) <= 7
    for b in bits:
        h ^= 1 << b
    return h


JUNK = 125  # base(JUNK) is in no index: the hash of needle frames that must match nothing
PAD = 124  # base(PAD) is in no needle: the hash of index frames that must match nothing


# ---- fixtures ----------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class VideoScene:
    """one index, one batch of needles, one parameter set.  `steps` is how the index comes about: ("add", [videos]) and
    ("remove", [media ids]); `index` is what they leave, in _mediaId order"""
    steps: list
    needles: list  # [(media id, frames, hashes)]
    params: VParams
    note: str = ""

    @property
    def index(self):
        return apply_steps(self.steps)


def apply_steps(steps):
    """DctVideoIndex::add (:256-260) appends, remove (:262-280) drops every video of a listed id"""
    index = []
    for op, arg in steps:
        if op == "add":
            index += list(arg)
        else:
            assert op == "remove"
            index = [v for v in index if v[0] not in arg]
    return index


@dataclasses.dataclass
class VideoFixture:
    name: str
    scenes: list
    target: dict


@dataclasses.dataclass
class VoteScene:
    rows: list  # [(media id, hash)] as added
    removed: list  # media ids removed afterwards (their entries keep their hashes, id 0)
    needles: list  # [(media id, [hashes])]
    thresh: int

    @property
    def live_rows(self):
        return [(0 if mid in self.removed else mid, h) for mid, h in self.rows]


@dataclasses.dataclass
class VoteFixture:
    name: str
    scenes: list
    target: dict


def video_results(fx: VideoFixture, variant: str | None = None):
    """the model's answer to a whole fixture: per scene, per needle, the result list"""
    return [[find_video(sc.index, nd, sc.params, variant) for nd in sc.needles] for sc in fx.scenes]


def vote_results(fx: VoteFixture, variant: str | None = None):
    return [[find_features(sc.live_rows, hs, nid, sc.thresh, variant) for nid, hs in sc.needles] for sc in fx.scenes]


def _video(mid, frame_hash):
    """(media id, frames, hashes) from [(frame, hash)] in ascending frame order"""
    frames = [f for f, _h in frame_hash]
    assert frames == sorted(set(frames))
    return (mid, frames, [h for _f, h in frame_hash])


def _scene(index, needles, note="", **params):
    return VideoScene([("add", index)], needles, VParams(**params), note)


def margin_edges():
    """destination gaps of exactly 14, 15 and 16 in both directions, and a first destination frame of 14 and of 15"""
    dsts = [14, 15, 28, 29, 43, 55, 59, 71, 86, 100]
    at = {d: base(i) for i, d in enumerate(dsts)}
    index = [_video(10, [(0, base(20))] + [(d, at[d]) for d in dsts])]
    walk_a = [14, 28, 43, 59, 100, 86, 71, 55]  # +14 +14 +15 +16 +41 -14 -15 -16
    walk_b = [15, 29]
    needles = [_video(1, [(i, at[d]) for i, d in enumerate(walk_a)]), _video(2, [(i, at[d]) for i, d in enumerate(walk_b)])]
    fx = VideoFixture("margin_edges", [_scene(index, needles)], {})
    # A: 14 from 0, +14, -14 are adjacent, the 15s and 16s are not: 3 of 8 -> 37.  B: 15 from 0 is not, +14 is: 1 of 2
    fx.target = {"results": [[[(10, 63, 0, 14, 41)], [(10, 50, 0, 15, 14)]]]}
    assert video_results(fx) == fx.target["results"]
    return fx


def gates_at_equality():
    """num == minFramesMatched and one below; percentNear == minFramesNear; 2 adjacent of 3 = 66 against 66 and 67"""
    near = _video(20, [(10 * i, base(i)) for i in range(10)])  # neighbours 10 apart: every match adjacent to the last
    hops = [0, 100, 110, 300, 310, 500]
    far = _video(21, [(f, base(10 + i)) for i, f in enumerate(hops)])  # 0 y, 100 n, 110 y, 300 n, 310 y, 500 n: 3 of 6
    third = _video(22, [(0, base(30)), (10, base(31)), (200, base(32))])  # y y n: 2 of 3
    index = [near, far, third]
    n5 = _video(1, [(i, base(i)) for i in range(5)])
    n4 = _video(2, [(i, base(i)) for i in range(4)])
    n50 = _video(3, [(i, base(10 + i)) for i in range(6)])
    n66 = _video(4, [(i, base(30 + i)) for i in range(3)])
    scenes = [_scene(index, [n5, n4, n50], "num 5 and 4 against 5; 50 against 50", vfm=5, vfn=50),
              _scene(index, [n50], "50 against 51", vfm=5, vfn=51),
              _scene(index, [n66], "66 against 66", vfm=3, vfn=66),
              _scene(index, [n66], "66 against 67", vfm=3, vfn=67)]
    fx = VideoFixture("gates_at_equality", scenes, {})
    fx.target = {"results": [[[(20, 0, 0, 0, 40)], [], [(21, 50, 0, 0, 500)]], [[]], [[(22, 34, 0, 0, 200)]], [[]]]}
    assert video_results(fx) == fx.target["results"]
    return fx


def distance_ties():
    """two frames of one video equally far from a needle frame, the first keeps the match adjacent and the needle above
    minFramesNear, the second would not; and a strictly closer frame later in entry order than a farther one"""
    x, y = base(3), base(4)
    index = [_video(30, [(0, base(0)), (5, flip(x, 0)), (10, base(1)), (20, flip(y, 1, 2)), (200, flip(x, 1)), (300, y)]),
             _video(31, [(0, base(9)), (7, base(8))])]
    needle = _video(1, [(0, base(0)), (1, x), (2, base(1)), (3, y)])
    fx = VideoFixture("distance_ties", [_scene(index, [needle], vfm=1, vfn=60)], {})
    # (0,0) (1,5) (2,10) (3,300): y y y n = 75.  With frame 200 for needle frame 1: y n n n = 25 < 60
    fx.target = {"results": [[[(30, 25, 0, 0, 300)]]], "tie_frames": (5, 200), "closer_later": (20, 300)}
    assert video_results(fx) == fx.target["results"]
    assert video_results(fx, "tie_last") == [[[]]]
    return fx


def descending_destination():
    """dstLen negative so that srcLen wins although it is the smaller number, and dstLen winning over srcLen"""
    index = [_video(40, [(10 * i, base(i)) for i in range(10)])]
    down = _video(1, [(0, base(9)), (2, base(8)), (4, base(7))])  # dst 90 80 70: srcLen 4, dstLen -20
    up = _video(2, [(0, base(0)), (1, base(1)), (2, base(5))])  # dst 0 10 50: srcLen 2, dstLen 50
    fx = VideoFixture("descending_destination", [_scene(index, [down, up])], {})
    fx.target = {"results": [[[(40, 34, 0, 90, 4)], [(40, 34, 0, 0, 50)]]]}
    assert video_results(fx) == fx.target["results"]
    return fx


def self_and_strangers():
    """the needle's own video in the index with filterSelf on and off; a needle whose id the index lacks"""
    own = _video(51, [(10 * i, base(i)) for i in range(6)])
    twin = _video(52, [(10 * i + 3, flip(base(i), i)) for i in range(6)])
    other = _video(50, [(10 * i, base(40 + i)) for i in range(6)])
    index = [other, own, twin]
    stranger = (999, own[1], own[2])
    scenes = [_scene(index, [own, stranger], "filterSelf on", filter_self=True),
              _scene(index, [own, stranger], "filterSelf off", filter_self=False)]
    fx = VideoFixture("self_and_strangers", scenes, {})
    both = [(51, 0, 0, 0, 50), (52, 0, 0, 3, 50)]
    fx.target = {"results": [[both[1:], both], [both, both]]}
    assert video_results(fx) == fx.target["results"]
    return fx


def _padded(mid, skip, frame_hash):
    """a needle whose listed frames are moved up by `skip` and survive the trim, between a frame 0 and a last frame that
    do not"""
    last = frame_hash[-1][0] + 2 * skip
    return _video(mid, [(0, base(JUNK))] + [(f + skip, h) for f, h in frame_hash] + [(last, base(JUNK))])


def batch_shapes():
    """one batch of: a short needle whose first surviving frame matches nothing, a needle without frames, a needle that
    the trim empties, a 100-frame needle, a needle with a zero hash among its frames, short needles, and last a needle
    whose last surviving frame matches nothing -- empty record segments at both ends of the batch's frame list"""
    skip = 10
    long_video = _video(60, [(0, base(PAD))] + [(10 + 3 * i, base(i)) for i in range(100)] + [(330, base(PAD))])
    five_ones = 0x1F  # popcount 5: kept by the index, 5 bits from a zero hash
    small = _video(61, [(0, base(PAD)), (20, five_ones), (30, base(100)), (40, base(101)), (400, base(PAD))])
    index = [long_video, small]
    needles = [
        _padded(1, skip, [(0, base(110)), (1, base(3)), (2, base(4))]),  # frame 10 matches nothing
        (2, [], []),
        _video(3, [(0, base(0)), (5, base(1)), (12, base(2))]),  # lastFrame 12: 0 and 5 < 10, 12 > 2
        _padded(4, skip, [(i, base(i)) for i in range(100)]),
        _padded(5, skip, [(0, base(100)), (1, 0), (2, base(101))]),
        _padded(6, skip, [(0, base(50)), (7, base(51))]),
        _padded(7, skip, [(0, base(99))]),
        _padded(8, skip, [(0, base(101)), (1, base(100)), (2, base(111))]),  # frame 12 matches nothing
    ]
    fx = VideoFixture("batch_shapes", [_scene(index, needles, thresh=6, skip=skip)], {})
    # needle 1: (11,19) (12,22), 19 from 0 is not adjacent.  needle 5: (10,30) (11,20) (12,40): n y n, the zero hash on 20
    fx.target = {"results": [[[(60, 50, 11, 19, 3)], [], [], [(60, 0, 10, 10, 297)], [(61, 67, 10, 30, 10)],
                             [(60, 50, 10, 160, 7)], [(60, 100, 10, 307, 0)], [(61, 50, 10, 40, 1)]]],
                 "zero_hash_matches_frame": 20}
    assert video_results(fx) == fx.target["results"]
    return fx


def trim_edges():
    """index side: lastFrame / 2 == skip (lastFrame 40 and, by truncation, 41) and skip + 1 (42), one needle per index
    frame; needle side: frames at skip - 1, skip, lastFrame - skip, lastFrame - skip + 1, and a needle with
    lastFrame / 2 == skip, which is trimmed all the same.  A fresh index per skip: 20, 21, 0"""
    frames = {70: [0, 5, 20, 35, 40], 71: [0, 19, 20, 21, 22, 23, 42], 72: [0, 10, 20, 21, 22, 41]}
    index, probes, b = [], [], 0
    for mid, fs in frames.items():
        index.append(_video(mid, [(f, base(b + i)) for i, f in enumerate(fs)]))
        probes += [_video(100 + b + i, [(0, base(JUNK)), (30, base(b + i)), (60, base(JUNK))]) for i in range(len(fs))]
        b += len(fs)
    steps = [0, 19, 20, 50, 80, 81, 100]
    index.append(_video(73, [(0, base(PAD))] + [(100 + 10 * i, base(b + i)) for i in range(7)] + [(400, base(PAD))]))
    walker = _video(1, [(f, base(b + i)) for i, f in enumerate(steps)])
    half = _video(2, [(f, base(b + i)) for i, f in enumerate([0, 10, 20, 30, 40])])  # lastFrame / 2 == 20
    needles = probes + [walker, half]
    scenes = [_scene(index, needles, f"skip {s}", skip=s) for s in (20, 21, 0)]
    fx = VideoFixture("trim_edges", scenes, {})

    def present(scene_results):
        got = {}
        for nd, res in zip(needles[:len(probes)], scene_results):
            for mid, _score, _src, dst, _len in res:
                got.setdefault(mid, []).append(dst)
        return got

    res = video_results(fx)
    fx.target = {"present": [present(r) for r in res], "walker": [r[-2] for r in res], "half": [r[-1] for r in res]}
    assert fx.target["present"] == [{70: frames[70], 71: [20, 21, 22], 72: frames[72]}, frames, frames]
    # walker: frames 20 50 80 (n y y), frame 50 alone (n), all seven (n and six y); half: frame 20 alone, none, all five
    assert fx.target["walker"] == [[(73, 34, 20, 120, 60)], [(73, 100, 50, 130, 0)], [(73, 15, 0, 100, 100)]]
    assert fx.target["half"] == [[(73, 100, 20, 120, 0)], [], [(73, 20, 0, 100, 40)]]
    return fx


def detail_edges():
    """index frames of popcount 4, 5, 59 and 60 that are exact copies of needle frames: 4 and 60 never enter the index"""
    words = {10: 0xF, 20: 0x1F00, 30: M64 ^ (0x1F << 20), 40: M64 ^ (0xF << 32)}
    assert [popc(words[f]) for f in (10, 20, 30, 40)] == [4, 5, 59, 60]
    video = _video(80, [(0, base(0))] + sorted(words.items()) + [(50, base(1))])
    copy = (81, video[1], video[2])
    probes = [_video(90 + i, [(0, base(JUNK)), (30, h), (60, base(JUNK))]) for i, h in enumerate(video[2])]
    fx = VideoFixture("detail_edges", [_scene([video], [copy] + probes, thresh=3)], {})
    res = video_results(fx)
    fx.target = {"results": res, "frames_found": [r[0][3] for r in res[0][1:] if r]}
    assert fx.target["frames_found"] == [0, 20, 30, 50]
    assert res[0][0] == [(80, 50, 0, 0, 50)]  # 0 y, 20 n, 30 y, 50 n
    return fx


def dense_static():
    """600 identical frames against 300 copies: 600 tied records per needle frame, the first entry wins each; three more
    needles whose record totals are one below, on and one above a multiple of 256"""
    h, h2 = base(0), base(1)
    index = [_video(90, [(i, h) for i in range(600)]), _video(92, [(0, h2)])]
    needles = [_video(91, [(i, h) for i in range(300)])]
    for k, extra in enumerate((7, 8, 9)):  # 29 * 600 = 67 * 256 + 248
        needles.append(_video(93 + k, [(i, h) for i in range(29)] + [(29 + i, h2) for i in range(extra)]))
    fx = VideoFixture("dense_static", [_scene(index, needles)], {})
    totals = [sum(600 if x == h else 1 for x in nd[2]) for nd in needles]
    fx.target = {"record_totals": totals,
                 "results": [[[(90, 0, 0, 0, 299)]] + [[(90, 0, 0, 0, 28), (92, 0, 29, 0, e - 1)] for e in (7, 8, 9)]]}
    assert [t % 256 for t in totals[1:]] == [255, 0, 1] and totals[0] == 180000
    assert video_results(fx) == fx.target["results"]
    return fx


def removed_middle():
    """a video removed from the middle and added again at the end: video indexes 0 1 2 are media 100 102 101"""
    vids = [_video(100 + k, [(0, base(PAD))] + [(10 * k + 5 + 10 * i, flip(base(i), k)) for i in range(4)]) for k in range(3)]
    steps = [("add", vids), ("remove", [101]), ("add", [vids[1]])]
    needle = _video(1, [(i, base(i)) for i in range(4)])
    fx = VideoFixture("removed_middle", [VideoScene(steps, [needle], VParams())], {})
    assert [v[0] for v in fx.scenes[0].index] == [100, 102, 101]
    fx.target = {"results": [[[(100, 0, 0, 5, 30), (101, 25, 0, 15, 30), (102, 25, 0, 25, 30)]]]}
    assert video_results(fx) == fx.target["results"]
    return fx


def media_id_twice():
    """media 110 added twice, another video between the two: needle frames 0 and 1 are closer to the first copy, 2 and 3
    to the second, 4 ties (the first copy wins it).  Per media id that is ONE result over both copies' frames; per video
    it is two results with the same id"""
    first = _video(110, [(0, flip(base(0), 0)), (10, flip(base(1), 0)), (20, flip(base(2), 0, 1, 2)),
                         (30, flip(base(3), 0, 1, 2)), (40, flip(base(4), 0))])
    between = _video(111, [(0, base(PAD)), (9, flip(base(2), 5, 6))])
    second = _video(110, [(0, base(PAD)), (100, flip(base(0), 3, 4, 5)), (110, flip(base(1), 3, 4, 5)),
                          (120, flip(base(2), 3)), (130, flip(base(3), 3)), (140, flip(base(4), 1))])
    needle = _video(1, [(i, base(i)) for i in range(5)])
    own = (110, needle[1], needle[2])
    fx = VideoFixture("media_id_twice", [_scene([first, between, second], [needle, own], filter_self=True)], {})
    # (0,0) (1,10) (2,120) (3,130) (4,40): y y n y n = 60
    fx.target = {"results": [[[(110, 40, 0, 0, 40), (111, 0, 2, 9, 0)], [(111, 0, 2, 9, 0)]]]}
    assert video_results(fx) == fx.target["results"]
    assert [r[0] for r in video_results(fx, "group_by_video")[0][0]] == [110, 110, 111]
    return fx


VIDEO_FIXTURES = (margin_edges, gates_at_equality, distance_ties, descending_destination, self_and_strangers,
                  batch_shapes, trim_edges, detail_edges, dense_static, removed_middle, media_id_twice)


def cut_of_ten():
    """12 candidates for one needle hash: two removed entries among the first 10, three candidates tied across the 10th
    place of which the lowest id gets it"""
    x = base(0)
    plan = [(5, 0), (7, 1), (6, 1), (13, 2), (8, 2), (9, 2), (10, 3), (11, 3), (12, 3), (22, 4), (20, 4), (21, 4)]
    rows, bit = [], 0
    for mid, d in plan:
        rows.append((mid, flip(x, *range(bit, bit + d))))  # distinct hashes, all d bits from x
        bit += d
    rows.append((30, base(1)))
    fx = VoteFixture("cut_of_ten", [VoteScene(rows, [7, 13], [(99, [x])], 6)], {})
    fx.target = {"results": [[[(5, 0), (6, 10), (8, 20), (9, 20), (10, 30), (11, 30), (12, 30), (20, 40)]]]}
    assert vote_results(fx) == fx.target["results"]
    return fx


def own_votes():
    """the needle's own media has the most votes: maxMatches is 2, not 3 -- and 1, not 2, for the second needle"""
    h = [base(i) for i in range(5)]
    rows = [(30, h[0]), (30, h[1]), (30, h[2]), (31, flip(h[0], 0)), (31, flip(h[1], 0)), (32, flip(h[0], 1, 2)),
            (40, h[3]), (40, h[4]), (41, flip(h[3], 0, 1, 2)), (42, flip(h[4], 0))]
    fx = VoteFixture("own_votes", [VoteScene(rows, [], [(30, h[:3]), (40, h[3:])], 5)], {})
    fx.target = {"results": [[[(30, -1), (31, 0), (32, 1)], [(40, -1), (41, 30), (42, 10)]]]}
    assert vote_results(fx) == fx.target["results"]
    return fx


def single_vote_scores():
    """maxMatches == 1 with distances 0, 1 and thresh - 1: 10 x the distance"""
    thresh = 7
    h = [base(i) for i in range(3)]
    rows = [(60, h[0]), (61, flip(h[1], 9)), (62, flip(h[2], *range(thresh - 1)))]
    fx = VoteFixture("single_vote_scores", [VoteScene(rows, [], [(1, h)], thresh)], {})
    fx.target = {"results": [[[(60, 0), (61, 10), (62, 60)]]]}
    assert vote_results(fx) == fx.target["results"]
    return fx


def batch_of_needles():
    """needles with maxMatches 1, 3 and 40 in one call, a needle without hashes between two others, a zero needle hash
    (three bits from an entry of popcount 3), a 40-hash needle all of whose hashes vote for one media, and needle id 0"""
    h = [base(i) for i in range(60)]
    rows = [(70, flip(h[0], 0, 1))]  # needle 1: one vote
    rows += [(71, flip(h[1 + i], 0)) for i in range(3)] + [(72, flip(h[1], 1)), (73, flip(h[2], 1)), (73, flip(h[3], 1))]
    rows += [(74, 0b111)]  # for the zero hash
    rows += [(75, flip(h[10 + i], i % 7)) for i in range(40)] + [(76, flip(h[10 + i], 8, 9)) for i in range(5)]
    rows += [(77, h[55]), (77, h[56]), (78, flip(h[55], 0))]
    needles = [(1, [h[0]]), (7777, []), (2, h[1:4]), (3, [h[5], 0]), (4, h[10:50]), (0, h[55:57])]
    fx = VoteFixture("batch_of_needles", [VoteScene(rows, [], needles, 7)], {})
    fx.target = {"results": [[[(70, 20)], [], [(71, 0), (72, 2), (73, 1)], [(74, 30)], [(75, 0), (76, 35)],
                              [(77, 0), (78, 1)]]]}
    assert vote_results(fx) == fx.target["results"]
    return fx


VOTE_FIXTURES = (cut_of_ten, own_votes, single_vote_scores, batch_of_needles)

# variant -> fixtures whose model answer it changes (each asserted by test_every_variant_is_killed)
KILLS = {
    "margin_le": ["margin_edges"],
    "last_from_first": ["margin_edges"],
    "tie_last": ["distance_ties", "dense_static"],
    "first_match_wins": ["distance_ties", "media_id_twice"],
    "gate_matched_le": ["gates_at_equality"],
    "gate_near_le": ["gates_at_equality"],
    "len_src_only": ["descending_destination"],
    "len_abs_dst": ["descending_destination"],
    "percent_rounded": ["gates_at_equality"],
    "group_by_video": ["media_id_twice"],
    "index_trim_unconditional": ["trim_edges"],
    "needle_trim_conditional": ["trim_edges", "batch_shapes"],
    "detail_4_60": ["detail_edges"],
    "self_always_filtered": ["self_and_strangers"],
    "order_by_video": ["removed_middle"],
    "removed_take_no_place": ["cut_of_ten"],
    "own_votes_count": ["own_votes"],
    "tie_highest_id": ["cut_of_ten"],
    "branch_per_media": ["own_votes", "batch_of_needles"],
}
