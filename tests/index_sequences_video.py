"""Sequences of mutations and searches on a DctVideoIndex with the host mirror that says what every search must answer
(the other kinds: tests/index_sequences.py, tests/index_sequences_cv.py; same op format).  Pure Python and NumPy.

The mirror is the list of videos in _mediaId order and the one piece of derived state the reference keeps: the search
structure is built by the first search after a mutation, with THAT search's skipFrames, and a later search with another
skipFrames does not rebuild it (src/dctvideoindex.cpp:116, video.hip build()).  Every expected answer is
oracle.VideoOracle.find_video / find_frame over VideoOracle.build_entries(videos, the built skip).  remove() drops every
video of an id; slice() keeps the FIRST video of each wanted id, in the order asked (cbh_vidx_slice); an id added twice
is two videos and one group (tests/reduce_rules.py::media_id_twice).

Ops (t = handle number):
  mutations  ("add", t, n, seed)   n clips of 60-300 frames cut from twelve source films, so that clips overlap
             ("add_dull", t)       a clip whose hashes all have "insufficient detail" (fewer than 5 ones)
             ("add_again", t, seed)  one more clip under a media id the handle already holds
             ("remove", t, spec), ("slice", t, seed, num, den)
  searches   ("find_video", t, seed, skip), ("find_videos_batch", t, seed, nn, skip), ("find_frame", t, seed, skip),
             ("find_frames_batch", t, seed, nn, skip), ("entries", t, skip)
             ("coverage", t, seed, n, skip), ("segments", t, seed, n, skip)  n ordered pairs of held media ids -- an id
             held twice and the all-dull clip among them when the handle has one -- against
             tests/video_coverage_rules.py / tests/video_segments_rules.py on the FIRST video of each id; and one more
             call with a pair that names an id the handle does not hold (a removed one when there is one): CBH_E_INVAL.
             Neither call reads or builds the search structure.
"""
import numpy as np

import index_sequences as S

MUTATIONS = ("add", "add_dull", "add_again", "remove", "slice")
ROUTES = ("find_video", "find_videos_batch", "find_frame", "find_frames_batch", "entries", "coverage", "segments")
TOL, MAX_SEGMENTS = 15, 4   # segments(): findVideo's frameMargin, and the default number of segments
SKIPS = (20, 100)   # a clip of 60 frames (lastFrame about 120) is trimmed at 20 and left whole at 100: lastFrame / 2 <= skip
THRESH, VFM, VFN = 6, 5, 30
RADIX = 10

_films = {}


def _film(k):
    """source film k: 700 frames, frame numbers 1..3 apart, a random-walk hash"""
    if k not in _films:
        rng = np.random.default_rng([k, 5150])
        h, cur = np.empty(700, np.uint64), int(rng.integers(0, 2**63)) * 2
        for i in range(700):
            for _ in range(int(rng.integers(0, 4))):
                cur ^= 1 << int(rng.integers(1, 64))
            h[i] = cur
        gaps = rng.integers(1, 4, 700)
        gaps[0] = 0
        _films[k] = (np.cumsum(gaps).astype(np.int32), h)
    return _films[k]


def gen_clips(seed, n):
    """n clips (frames int32 from 0, hashes): windows of 60..300 frames of a film, 30 % of the hashes with a bit flipped"""
    rng = np.random.default_rng([int(seed), int(n), 9])
    out = []
    for _ in range(n):
        f, h = _film(int(rng.integers(0, 12)))
        m = int(rng.choice([60, 61, 150, 300]))
        a = int(rng.integers(0, 700 - m))
        hh = h[a:a + m].copy()
        hh ^= np.where(rng.random(m) < 0.3, np.uint64(1) << rng.integers(1, 64, m).astype(np.uint64), np.uint64(0))
        out.append(((f[a:a + m] - f[a]).astype(np.int32), hh))
    return out


class MirrorVideo:
    def __init__(self, videos=()):
        self.videos = list(videos)  # (media id, frames, hashes)
        self.built, self.built_skip = False, 0
        self.builds = []            # (skip asked, rebuilt?) per search: what the conditions read

    def count(self):
        return len(self.videos)

    def live_ids(self):
        return np.unique(np.array([v[0] for v in self.videos], np.uint32))

    ids = property(live_ids)

    def search_with(self, skip):
        """the skip the structure answers with: built now if a mutation came before"""
        self.builds.append((skip, not self.built, self.built_skip))
        if not self.built:
            self.built, self.built_skip = True, skip
        return self.built_skip

    def slice(self, ids):
        first = {}
        for v in self.videos:
            first.setdefault(v[0], v)
        seen, out = set(), []
        for i in np.asarray(ids).tolist():
            if i in first and i not in seen:
                seen.add(i)
                out.append(first[i])
        return MirrorVideo(out)


class World:
    def __init__(self, kind="video"):
        self.kind = kind
        self.handles = [MirrorVideo()]
        self.next_id = 1

    def take_ids(self, n):
        first = self.next_id
        self.next_id += n
        return np.arange(first, first + n, dtype=np.uint32)


def is_search(op):
    return op[0] not in MUTATIONS


def _needle_video(m, seed):
    """(id, frames, hashes): a clip the index holds under its own id, a fresh cut of a film, or a stranger"""
    rng = np.random.default_rng([seed, 53])
    r = rng.random()
    if m.videos and r < 0.5:
        mid, f, h = m.videos[int(rng.integers(0, len(m.videos)))]
        return int(mid), f, h
    f, h = gen_clips(seed + 77, 1)[0]
    return 0, f, h


def _needle_frame(m, seed):
    """(hash, src_in): a frame of an indexed clip with up to two bits flipped, sometimes a stranger or 0"""
    rng = np.random.default_rng([seed, 59])
    r = rng.random()
    if r < 0.08:
        return 0, -1
    if m.videos and r < 0.85:
        _, f, h = m.videos[int(rng.integers(0, len(m.videos)))]
        x = int(h[int(rng.integers(0, len(h)))])
        for _ in range(int(rng.integers(0, 3))):
            x ^= 1 << int(rng.integers(0, 64))
        return x, int(rng.choice([-1, 0, 17]))
    return int(rng.integers(1, 1 << 63)), -1


def resolve(world, op):
    name, m = op[0], world.handles[op[1]]
    if name == "add":
        return {"ids": world.take_ids(op[2]), "clips": gen_clips(op[3], op[2])}
    if name == "add_dull":
        return {"ids": world.take_ids(1), "clips": [(np.arange(0, 160, 2, dtype=np.int32), np.full(80, 0xF, np.uint64))]}
    if name == "add_again":
        live = m.live_ids()
        mid = int(np.random.default_rng([op[2], 61]).choice(live)) if len(live) else int(world.take_ids(1)[0])
        return {"ids": np.array([mid], np.uint32), "clips": gen_clips(op[2], 1)}
    if name == "remove":
        return {"ids": S._remove_ids(world, m, op[2])}
    if name == "slice":  # in a drawn order, not ascending: the order of the ids is the order of the slice's videos
        ids = S._slice_ids(world, m, op)
        return {"ids": ids[np.random.default_rng([op[2], 67]).permutation(len(ids))]}
    if name == "find_video":
        return {"needle": _needle_video(m, op[2])}
    if name == "find_videos_batch":
        return {"needles": [_needle_video(m, op[2] + 3 * j) for j in range(op[3])]}
    if name == "find_frame":
        return {"needle": _needle_frame(m, op[2])}
    if name == "find_frames_batch":
        return {"needles": [_needle_frame(m, op[2] + 3 * j) for j in range(op[3])]}
    if name == "entries":
        return {}
    if name in ("coverage", "segments"):
        rng = np.random.default_rng([op[2], 71])
        ids = [v[0] for v in m.videos]
        held = list(dict.fromkeys(ids))
        doubled = [i for i in held if ids.count(i) > 1]
        dull = [v[0] for v in m.videos if len(v[2]) and (v[2] == 0xF).all()]
        rest = [i for i in held if i not in doubled[:1] + dull[:1]]
        pool = doubled[:1] + dull[:1] + [int(x) for x in rng.choice(rest, min(len(rest), max(2, op[3])), replace=False)] if rest \
            else doubled[:1] + dull[:1]
        pairs = [(pool[j % len(pool)], pool[(j + 1) % len(pool)]) for j in range(op[3])] if pool else []
        if pool:
            pairs[-1] = (pool[0], pool[0])  # a video meets itself
        gone = [i for i in range(1, world.next_id) if i not in held]
        kinds = {"doubled"} & {"doubled" if any(a in doubled or b in doubled for a, b in pairs) else ""}
        kinds |= {"dull"} & {"dull" if any(a in dull or b in dull for a, b in pairs) else ""}
        kinds |= {"removed"} & {"removed" if gone else ""}
        bad = (pool[0] if pool else world.next_id + 4, gone[0] if gone else world.next_id + 5)
        return {"pairs": pairs, "bad": bad, "kinds": kinds}
    raise ValueError(op)


def _first_videos(m):
    first = {}
    for v in m.videos:
        first.setdefault(v[0], (v[1], v[2]))
    return first


def expect_pairs(op, a, m):
    """coverage / segments of every pair from the rule modules, as plain lists; then "INVAL" for the call with the bad pair"""
    import video_coverage_rules as VR
    import video_segments_rules as SR

    first, out = _first_videos(m), []
    for src, dst in a["pairs"]:
        if op[0] == "coverage":
            s, frames, dframes, dist = VR.coverage(first[src], first[dst], THRESH, op[4])
            out.append([[s[k] for k in VR.FIELDS], frames, dframes, dist])
        else:
            s, segs, frames, dframes, dist, seg = SR.segments(first[src], first[dst], THRESH, op[4], TOL, VFM, MAX_SEGMENTS)
            out.append([[s[k] for k in SR.SUMMARY_FIELDS], [[g[k] for k in SR.SEGMENT_FIELDS] for g in segs], frames, dframes, dist, seg])
    return out + ["INVAL"]


def expect(world, op, a, vorc, radix=0):
    """the answer and, for the runner, the entry count of the structure that gave it: (answer, entries)"""
    name, m = op[0], world.handles[op[1]]
    skip = op[-1]
    if name in ("coverage", "segments"):
        return expect_pairs(op, a, m), None  # (host tables of the held videos: nothing is built, nothing built is read)
    if name == "find_frame" and a["needle"][0] == 0:
        return [], None  # "needle has no dct hash": returns before anything is built
    built = m.search_with(skip)
    entries = vorc.build_entries(m.videos, built)
    ne = len(entries[0])

    def video(n):
        mid, f, h = n
        return vorc.find_video(entries, f, h, mid, THRESH, skip, VFM, VFN, True, radix) if m.videos else []

    def frame(n):
        return vorc.find_frame(entries, n[0], THRESH, n[1], radix) if n[0] and m.videos else []

    if name == "find_video":
        return video(a["needle"]), ne
    if name == "find_videos_batch":
        return [video(n) for n in a["needles"]], ne
    if name == "find_frame":
        return frame(a["needle"]), ne
    if name == "find_frames_batch":
        return [frame(n) for n in a["needles"]], ne
    if name == "entries":
        return ne, ne
    raise ValueError(op)


def apply_mutation(world, op, a):
    name, m = op[0], world.handles[op[1]]
    if name in ("add", "add_dull", "add_again"):
        m.videos += [(int(i), f, h) for i, (f, h) in zip(a["ids"], a["clips"])]
    elif name == "remove":
        gone = set(int(x) for x in a["ids"])
        m.videos = [v for v in m.videos if v[0] not in gone]
    elif name == "slice":
        world.handles.append(m.slice(a["ids"]))
        return
    m.built = False


HAND = [
    ("add", 0, 40, 1),                      # 40 clips
    ("find_video", 0, 2, 20),               # builds with skip 20: the 60-frame clips are trimmed
    ("find_video", 0, 3, 100),              # another skip, no mutation in between: NOT rebuilt, answers from skip 20
    ("entries", 0, 100),                    # ... and says so
    ("find_frames_batch", 0, 4, 16, 20),    # the first batched image search after the build uploads entry -> video
    ("find_frames_batch", 0, 4, 16, 20),
    ("add", 0, 1, 5),                       # a mutation ...
    ("find_frames_batch", 0, 6, 16, 100),   # ... then a batched image search FIRST, with the other skip: rebuilt with 100
    ("find_video", 0, 7, 20),               # a find_video after add after a find with another skip
    ("entries", 0, 20),
    ("add_dull", 0),                        # every hash has four ones: the clip adds no entry
    ("find_videos_batch", 0, 8, 6, 20),
    ("find_videos_batch", 0, 8, 6, 20),
    ("add_again", 0, 9),                    # a second clip under an id the handle holds: two videos, one group
    ("coverage", 0, 28, 4, 20),             # pairs with the doubled id (its first video) and the all-dull clip
    ("coverage", 0, 28, 4, 20),
    ("segments", 0, 29, 3, 100),
    ("find_video", 0, 10, 20),
    ("find_frame", 0, 11, 20),
    ("find_frame", 0, 11, 20),
    ("slice", 0, 12, 1, 3),                 # handle 1: a third of the ids, in a drawn order
    ("find_frame", 0, 13, 20),              # the parent right after (its structure is still the one built before)
    ("find_video", 1, 14, 100),             # the slice builds its own
    ("add", 1, 2, 15),
    ("coverage", 1, 31, 3, 100),            # the slice's own videos
    ("find_frames_batch", 1, 16, 8, 20),
    ("remove", 0, ("draw", 17, 6)),         # held, absent and repeated ids; both clips of a doubled id go
    ("segments", 0, 30, 3, 20),             # pairs of what is left; a pair that names a removed id is refused
    ("segments", 0, 30, 3, 20),
    ("find_frames_batch", 0, 4, 16, 20),    # the needles of the start: removed videos are gone
    ("find_videos_batch", 0, 18, 6, 100),
    ("entries", 0, 100),
    ("entries", 0, 100),
    ("add_again", 0, 19),
    ("find_frames_batch", 0, 20, 16, 20),
    ("remove", 1, ("draw", 21, 3)),
    ("find_video", 1, 22, 20),
    ("find_video", 1, 22, 20),
    ("remove", 0, ("all",)),                # everything at once ...
    ("find_video", 0, 23, 20),              # ... nothing to find, nothing to build on
    ("entries", 0, 20),
    ("add", 0, 3, 24),
    ("entries", 0, 100),
    ("find_video", 0, 25, 100),
    ("find_frame", 0, 26, 100),
    ("add_dull", 0),
    ("find_frame", 0, 26, 100),
    ("find_videos_batch", 0, 27, 4, 20),
]


def _search(rng, t, route=None):
    route = route or ROUTES[int(rng.integers(0, len(ROUTES)))]
    s, skip = int(rng.integers(1, 1 << 20)), int(rng.choice(SKIPS))
    return {"find_video": ("find_video", t, s, skip), "find_videos_batch": ("find_videos_batch", t, s, int(rng.choice([1, 6])), skip),
            "find_frame": ("find_frame", t, s, skip), "find_frames_batch": ("find_frames_batch", t, s, int(rng.choice([1, 16])), skip),
            "entries": ("entries", t, skip), "coverage": ("coverage", t, s, int(rng.choice([1, 4])), skip),
            "segments": ("segments", t, s, int(rng.choice([1, 3])), skip)}[route]


def sequence(seed, steps=40):
    rng = np.random.default_rng(seed)
    sd = lambda: int(rng.integers(1, 1 << 20))  # noqa: E731

    def mut(t, name):
        return {"add": ("add", t, int(rng.choice([1, 3])), sd()), "add_dull": ("add_dull", t), "add_again": ("add_again", t, sd()),
                "remove": ("remove", t, ("draw", sd(), int(rng.integers(1, 6))))}[name]

    def other(skip):
        return SKIPS[1 - SKIPS.index(skip)]

    plain = ("add", "add_dull", "add_again", "remove")
    segs = []
    for r in ROUTES:
        segs.append(lambda t, new, r=r: [mut(t, plain[int(rng.integers(0, 4))]), _search(rng, t, r), _search(rng, t, r)])
    for name in plain:
        segs.append(lambda t, new, n=name: [mut(t, n), _search(rng, t)])

    def skips(t, new):  # build with one skip, ask with the other (no rebuild), mutate, ask with the other (rebuild)
        a = _search(rng, t, "find_video")
        b = _search(rng, t, "find_video")[:3] + (other(a[3]),)
        return [mut(t, "add"), a, b, ("entries", t, other(a[3])), mut(t, "add"), ("find_frames_batch", t, sd(), 16, other(a[3])),
                ("find_video", t, sd(), a[3])]

    segs.append(skips)
    # pairs with a doubled id and with the dull clip under both skips, then with a removed id to refuse
    segs.append(lambda t, new: [("add_again", 0, sd()), ("coverage", 0, sd(), 4, SKIPS[0]), ("segments", 0, sd(), 3, SKIPS[1]),
                                ("add_dull", 0), ("coverage", 0, sd(), 4, SKIPS[1]), ("segments", 0, sd(), 3, SKIPS[0]),
                                ("remove", 0, ("draw", sd(), 3)), ("coverage", 0, sd(), 4, SKIPS[0]), ("segments", 0, sd(), 3, SKIPS[1])])
    segs.append(lambda t, new: [("slice", t, sd(), 1, 3), _search(rng, t), ("add", t, 2, sd()), _search(rng, t),
                                ("add", new, 2, sd()), _search(rng, new), ("remove", new, ("draw", sd(), 2)), _search(rng, new)])
    segs.append(lambda t, new: [("remove", t, ("all",)), _search(rng, t), ("add", t, 3, sd()), _search(rng, t)])
    ops, handles = [("add", 0, 40, sd())], 1
    for i in rng.permutation(len(segs)):
        t = 0 if rng.random() < 0.7 else int(rng.integers(0, handles))
        for op in segs[int(i)](t, handles):
            handles += op[0] == "slice"
            ops.append(op)
    while len(ops) < steps:
        ops.append(_search(rng, 0))
    return ops


def coverage(ops):
    world = World()
    f = {"ops": len(ops), "route_after_mutation": set(), "route_second_in_row": set(), "mutation_then_search": set(),
         "slice_parent_used": False, "slice_itself_used": False, "remove_all_then_add": False, "skips": set(),
         "skip_change_without_rebuild": 0, "skip_change_with_rebuild": 0, "frames_batch_first_after_mutation": 0,
         "doubled_id": False, "dull": False, "short_clip_untrimmed": False, "max_needles": 0,
         "pairs": {"coverage": set(), "segments": set()}}

    class NoOracle:  # expect() only needs the bookkeeping here
        @staticmethod
        def build_entries(videos, skip):
            return ([],)

        find_video = find_frame = staticmethod(lambda *a, **k: [])

    prev, parents, touched, removed_all = None, {}, {}, set()
    for op in ops:
        t, m = op[1], world.handles[op[1]]
        a = resolve(world, op)
        if is_search(op):
            if prev is not None and prev[1] == t:
                if prev[0] in MUTATIONS:
                    f["mutation_then_search"].add(prev[0])
                    f["route_after_mutation"].add(op[0])
                else:
                    f["route_second_in_row"].add(op[0])
            f["max_needles"] = max(f["max_needles"], len(a.get("needles", [0])))
            if op[0] in ("coverage", "segments"):
                f["pairs"][op[0]] |= {(k, op[4]) for k in a["kinds"]} | ({("pair", op[4])} if a["pairs"] else set())
            n0 = len(m.builds)
            if op[0] not in ("coverage", "segments"):
                expect(world, op, a, NoOracle)
            if len(m.builds) > n0:
                skip, rebuilt, before = m.builds[-1]
                f["skips"].add(skip)
                if rebuilt and op[0] == "find_frames_batch":
                    f["frames_batch_first_after_mutation"] += 1
                if rebuilt and len(m.builds) > 1 and before != skip:
                    f["skip_change_with_rebuild"] += 1
                if not rebuilt and before != skip:
                    f["skip_change_without_rebuild"] += 1
                ids = [v[0] for v in m.videos]
                f["doubled_id"] |= len(set(ids)) < len(ids)
                f["dull"] |= any((v[2] == 0xF).all() for v in m.videos)
                f["short_clip_untrimmed"] |= m.built_skip and any(len(v[1]) and v[1][-1] // 2 <= m.built_skip for v in m.videos)
            if touched.get(t):
                f["slice_itself_used" if t in parents else "slice_parent_used"] = True
        else:
            if op[0] == "slice":
                touched[t], touched[len(world.handles)] = False, False
                parents[len(world.handles)] = t
            elif t in touched:
                touched[t] = True
            if op[0] == "add" and t in removed_all:
                f["remove_all_then_add"] = True
            removed_all.discard(t)
            if op[0] == "remove" and op[2] == ("all",):
                removed_all.add(t)
            apply_mutation(world, op, a)
        prev = op
    return f
