"""Sequences of mutations and searches on a CvFeaturesIndex (256-bit descriptors), plain and sharded, with the host mirror
that says what every search must answer; the 64-bit and colour kinds are in tests/index_sequences.py, whose op format,
remove specs and helpers this module shares.  Pure Python and NumPy.

The mirror is the reference's three structures (src/cvfeaturesindex.h:77): the descriptor matrix in add order, the map
first row -> mediaId (0 = removed; the rows stay and still take knn places, tests/test_cvfeatures.py) and the map
mediaId -> first row.  A slice holds the wanted media in ascending id (tests/test_slice_device.py: rows_of +
download_rows + add); the sequences only ask for live and absent ids.

Ops (t = handle number; at most 32 needle descriptors per search):
  mutations  ("add", t, m, per, seed)  m media of `per` descriptors each, one cbh_idx256_add per media
             ("add_refused", t), ("remove", t, spec), ("slice", t, seed, num, den)
  searches   ("knn", t, seed, nq, k, thresh), ("knn_media", t, seed, nq, k, thresh), ("radius_match", t, seed, nq, max_dist),
             ("find", t, seed, thresh), ("find_by_id", t, seed, thresh), ("find_batch", t, seed, nn, thresh),
             ("descriptors", t, seed)
"""
import numpy as np

import index_sequences as S

KINDS = ("cv", "cv_sharded")
MUTATIONS = ("add", "add_refused", "remove", "slice")
ROUTES = ("knn", "knn_media", "radius_match", "find", "find_by_id", "find_batch", "descriptors")
SHARDS = 3          # the sharded kind: shards=(1, 3)
SHARD_RUN = 16384   # Shards256::kShardRun
KNN = 10


def is_search(op):
    return op[0] not in MUTATIONS


def gen_rows(seed, n):
    return np.random.default_rng([int(seed), int(n), 3]).integers(0, 256, (n, 32), dtype=np.uint8)


class MirrorCv:
    def __init__(self, shards=0):
        self.rows = np.zeros((0, 32), np.uint8)
        self.first = np.zeros(0, np.uint32)   # first row of every media, in add order
        self.media = np.zeros(0, np.uint32)   # its id, 0 once removed
        self.where = {}                       # id -> position in first / media (the last add of that id)
        self.cap, self.crossings = 0, []      # Rows256::append of a plain handle
        self.shards = shards                  # Shards256::next_shard
        self.shard_rows, self.cur, self.cur_run, self.turns = [0] * shards, 0, 0, [1] + [0] * (shards - 1) if shards else []

    def count(self):
        return len(self.rows)

    def add(self, mid, rows):
        need = len(self.rows) + len(rows)
        if self.shards:
            if self.cur_run >= SHARD_RUN:
                self.cur = int(np.argmin(self.shard_rows))  # (the first of the emptiest)
                self.cur_run = 0
                self.turns[self.cur] += 1
            self.shard_rows[self.cur] += len(rows)
            self.cur_run += len(rows)
        elif need > self.cap:
            self.crossings.append(self.cap)
            self.cap = max(need, self.cap + self.cap // 2 + 65536)
        self.where[int(mid)] = len(self.first)
        self.first = np.append(self.first, np.uint32(len(self.rows)))
        self.media = np.append(self.media, np.uint32(mid))
        self.rows = np.concatenate([self.rows, rows])

    def remove(self, ids):
        for i in np.asarray(ids).tolist():
            if i in self.where:
                self.media[self.where[i]] = 0

    def rows_of(self, mid):
        if mid not in self.where:
            return self.rows[:0]
        p = self.where[mid]
        end = int(self.first[p + 1]) if p + 1 < len(self.first) else len(self.rows)
        return self.rows[int(self.first[p]):end]

    def slice(self, ids):
        out = MirrorCv(self.shards)
        for mid in sorted(set(int(x) for x in ids)):
            d = self.rows_of(mid)
            if len(d):
                out.add(mid, d)
        return out

    def live_ids(self):
        return np.unique(self.media[self.media != 0])

    def media_of_rows(self, r):
        """the id of the media a row belongs to (0: removed)"""
        return self.media[np.searchsorted(self.first, r, side="right") - 1]

    ids = property(lambda self: self.media)  # (what index_sequences._remove_ids reads)


class World:
    def __init__(self, kind):
        assert kind in KINDS, kind
        self.kind = kind
        self.handles = [MirrorCv(SHARDS if kind == "cv_sharded" else 0)]
        self.next_id = 1

    def take_ids(self, n):
        first = self.next_id
        self.next_id += n
        return np.arange(first, first + n, dtype=np.uint32)


def _needles(m, seed, nq):
    """nq needle descriptors: rows of the index with 0..30 bits flipped (a few exact), and strangers"""
    rng = np.random.default_rng([seed, 43])
    q = gen_rows(seed + 500009, nq)
    if m.count():
        take = rng.random(nq) < 0.75
        q[take] = m.rows[rng.integers(0, m.count(), int(take.sum()))]
        for j in np.flatnonzero(take):
            for b in rng.choice(256, int(rng.integers(0, 31)), replace=False):
                q[j, b >> 3] ^= 1 << (b & 7)
    return q


def _needle_media(m, seed):
    """(id, descriptors): up to 32 descriptors of an indexed media, some bits flipped; or a stranger with id 0"""
    rng = np.random.default_rng([seed, 47])
    live = m.live_ids()
    if not len(live) or seed % 4 == 3:
        return 0, gen_rows(seed + 11, 20)
    mid = int(rng.choice(live))
    d = m.rows_of(mid)[:32].copy()
    d[::3, int(rng.integers(0, 32))] ^= 0x24
    return mid, d


def resolve(world, op):
    name, m = op[0], world.handles[op[1]]
    if name == "add":
        return {"ids": world.take_ids(op[2]), "rows": gen_rows(op[4], op[2] * op[3]).reshape(op[2], op[3], 32)}
    if name == "add_refused":
        return {"id": 1 << 30, "rows": gen_rows(4242, m.count() // 2 + 70000)}  # past any capacity the growth rule leaves
    if name == "remove":
        return {"ids": S._remove_ids(world, m, op[2])}
    if name == "slice":
        return {"ids": S._slice_ids(world, m, op)}
    if name in ("knn", "knn_media", "radius_match"):
        return {"q": _needles(m, op[2], op[3])}
    if name == "find":
        mid, d = _needle_media(m, op[2])
        return {"id": mid, "d": d}
    if name == "find_by_id":
        live = m.live_ids()
        return {"id": int(np.random.default_rng([op[2], 23]).choice(live)) if len(live) else world.next_id + 3}
    if name == "find_batch":
        return {"needles": [_needle_media(m, op[2] + 4 * j) for j in range(op[3])]}
    if name == "descriptors":  # a live, a removed or an absent id
        ever = np.arange(1, max(world.next_id, 2) + 1)
        return {"id": int(np.random.default_rng([op[2], 29]).choice(ever))}
    raise ValueError(op)


def _cut(r, d, c, k):
    """per needle: the count and its first min(k, count) (row, distance) places"""
    return [[int(c[q]), r[q, :min(k, int(c[q]))].tolist(), d[q, :min(k, int(c[q]))].tolist()] for q in range(len(c))]


def expect(world, op, a, cvo):
    name, m = op[0], world.handles[op[1]]
    if name in ("knn", "knn_media"):
        k = op[4]
        if m.count() == 0:
            return [[0, [], []] + ([[]] if name == "knn_media" else []) for _ in a["q"]]
        r, d, c = cvo.knn(m.rows, a["q"], k, op[5])
        out = _cut(r, d, c, k)
        if name == "knn_media":
            for q, row in enumerate(out):
                row.append(m.media_of_rows(np.array(row[1], np.int64)).tolist())
        return out
    if name == "radius_match":  # every row within max_dist, per query in (distance, row) order
        if m.count() == 0:
            return [[] for _ in a["q"]]
        k = 256
        r, d, c = cvo.knn(m.rows, a["q"], k, op[4] + 1)
        assert c.max() <= k, "more matches than the model asks the oracle for"
        return [list(zip(r[q, :c[q]].tolist(), d[q, :c[q]].tolist())) for q in range(len(c))]

    def find(mid, d, thresh):
        if d is None or len(d) == 0:
            d = m.rows_of(mid)  # (cvfeaturesindex.cpp:443)
        if len(d) == 0 or m.count() == 0:
            return []
        return S._pairs(*cvo.find(m.rows, m.first, m.media, d, KNN, thresh))

    if name == "find":
        return find(a["id"], a["d"], op[3])
    if name == "find_by_id":
        return find(a["id"], None, op[3])
    if name == "find_batch":
        return [find(mid, d, op[4]) for mid, d in a["needles"]]
    if name == "descriptors":
        return m.rows_of(a["id"])
    raise ValueError(op)


def apply_mutation(world, op, a):
    name, m = op[0], world.handles[op[1]]
    if name == "add":
        for mid, rows in zip(a["ids"].tolist(), a["rows"]):
            m.add(mid, rows)
    elif name == "remove":
        m.remove(a["ids"])
    elif name == "slice":
        world.handles.append(m.slice(a["ids"]))


# ---- sequences --------------------------------------------------------------------------------------------------------
HAND = {
    "cv": [
        ("add", 0, 650, 100, 1),                # 65 000 rows, media by media: one block of 65 536
        ("knn", 0, 2, 32, 10, 40),
        ("knn", 0, 2, 32, 10, 40),
        ("slice", 0, 3, 1, 50),                 # handle 1: 13 media, before the parent grows
        ("find", 0, 4, 25),
        ("add", 0, 3, 100, 5),                  # 65 300: inside the block
        ("knn_media", 0, 6, 32, 4, 60),
        ("add", 0, 6, 100, 7),                  # 65 900: across 65 536 -> 163 840, the rows copied device to device
        ("descriptors", 0, 8),
        ("descriptors", 0, 8),
        ("knn", 0, 2, 32, 10, 40),              # the needles of the start: the same rows answer, plus nothing new
        ("radius_match", 0, 9, 32, 25),
        ("radius_match", 0, 9, 32, 25),
        ("remove", 0, ("draw", 10, 40)),        # map entries become 0, rows stay
        ("knn_media", 0, 6, 32, 4, 60),         # the same rows, their media gone
        ("knn_media", 0, 6, 32, 4, 60),
        ("find_batch", 0, 11, 4, 25),
        ("find_batch", 0, 11, 4, 25),
        ("remove", 0, ("draw", 10, 40)),        # the same ids again
        ("find_by_id", 0, 12, 25),
        ("find_by_id", 0, 12, 25),
        ("add", 1, 2, 100, 13),                 # the slice grows on its own
        ("knn", 1, 14, 32, 10, 40),
        ("remove", 1, ("draw", 15, 3)),
        ("find", 1, 16, 25),
        ("find", 1, 16, 25),
        ("add_refused", 0),                     # CBH_E_NOMEM: append() keeps the old rows, the maps are untouched
        ("knn", 0, 2, 32, 10, 40),
        ("add", 0, 1, 100, 17),
        ("knn_media", 0, 18, 32, 10, 40),
        ("descriptors", 0, 19),
        ("remove", 0, ("all",)),
        ("find_batch", 0, 11, 4, 25),           # every media removed: nobody to vote for
        ("add", 0, 2, 100, 20),
        ("find", 0, 21, 25),
        ("radius_match", 0, 22, 32, 25),
        ("slice", 0, 23, 1, 1),                 # handle 2: the two live media
        ("radius_match", 0, 22, 32, 25),
        ("knn", 2, 24, 32, 10, 60),
        ("descriptors", 2, 25),
    ],
    # 14 adds of 6 000 rows: every shard is the current one twice (runs of 16 384 rows), segment tables rebuilt in between
    "cv_sharded": [
        ("add", 0, 60, 100, 1),
        ("knn", 0, 2, 32, 10, 40),
        ("add", 0, 60, 100, 3),
        ("add", 0, 60, 100, 4),                 # 18 000: the first run is over, shard 1 is next
        ("knn", 0, 2, 32, 10, 40),
        ("add", 0, 60, 100, 5),                 # the first rows of shard 1: a search right after needs its segment table
        ("knn_media", 0, 6, 32, 10, 40),
        ("knn_media", 0, 6, 32, 10, 40),
        ("add", 0, 60, 100, 7),
        ("add", 0, 60, 100, 8),
        ("radius_match", 0, 9, 32, 25),
        ("add", 0, 60, 100, 10),                # shard 2
        ("find", 0, 11, 25),
        ("find", 0, 11, 25),
        ("slice", 0, 12, 1, 20),                # handle 1: sharded like its parent
        ("find_batch", 0, 13, 4, 25),
        ("add", 0, 60, 100, 14),
        ("add", 0, 60, 100, 15),
        ("descriptors", 0, 16),
        ("add", 0, 60, 100, 17),                # shard 0 again: a second segment on it
        ("knn", 0, 18, 32, 10, 40),
        ("remove", 0, ("draw", 19, 60)),
        ("find_by_id", 0, 20, 25),
        ("find_by_id", 0, 20, 25),
        ("knn_media", 0, 18, 32, 10, 40),
        ("add", 0, 60, 100, 21),
        ("add", 0, 60, 100, 22),
        ("radius_match", 0, 23, 32, 25),
        ("radius_match", 0, 23, 32, 25),
        ("add", 0, 60, 100, 24),                # shard 1 again
        ("knn", 0, 18, 32, 10, 40),
        ("add", 0, 60, 100, 25),
        ("add", 0, 60, 100, 26),                # 84 000 rows: shard 2 again
        ("knn_media", 0, 27, 32, 10, 60),
        ("descriptors", 0, 28),
        ("descriptors", 0, 28),
        ("add", 1, 3, 100, 29),                 # the slice is still alive and its own
        ("knn", 1, 30, 32, 10, 40),
        ("remove", 1, ("draw", 31, 5)),
        ("find_batch", 1, 32, 4, 25),
        ("find_batch", 1, 32, 4, 25),
        ("remove", 0, ("all",)),
        ("find", 0, 33, 25),
        ("add", 0, 2, 100, 34),
        ("find", 0, 35, 25),
        ("knn", 0, 36, 32, 10, 40),
    ],
}


def _search(rng, t, route=None):
    route = route or ROUTES[int(rng.integers(0, len(ROUTES)))]
    s = int(rng.integers(1, 1 << 20))
    k, th = int(rng.choice([1, 4, 10])), int(rng.choice([25, 40, 60]))
    return {"knn": ("knn", t, s, 32, k, th), "knn_media": ("knn_media", t, s, 32, k, th),
            "radius_match": ("radius_match", t, s, int(rng.choice([1, 32])), 25), "find": ("find", t, s, 25),
            "find_by_id": ("find_by_id", t, s, 25), "find_batch": ("find_batch", t, s, int(rng.choice([1, 4])), 25),
            "descriptors": ("descriptors", t, s)}[route]


def sequence(kind, seed, steps=40):
    """as index_sequences.sequence: segments in a drawn order; the large adds keep their own order (the capacity and the
    shards' runs are functions of the row count), the rest is shuffled between them"""
    rng = np.random.default_rng(seed)
    sd = lambda: int(rng.integers(1, 1 << 20))  # noqa: E731
    sharded = kind == "cv_sharded"

    def mut(t, name):
        return {"add": ("add", t, int(rng.choice([1, 3])), 100, sd()), "remove": ("remove", t, ("draw", sd(), int(rng.integers(1, 60)))),
                "add_refused": ("add_refused", t)}[name]

    plain = ("add", "remove") if sharded else ("add", "remove", "add_refused")
    small = []
    for r in ROUTES:
        small.append(lambda t, new, r=r: [mut(t, plain[int(rng.integers(0, len(plain)))]), _search(rng, t, r), _search(rng, t, r)])
    for name in plain:
        small.append(lambda t, new, n=name: [mut(t, n), _search(rng, t)])
    small.append(lambda t, new: [("slice", t, sd(), 1, 20), _search(rng, t), ("add", t, 2, 100, sd()), _search(rng, t),
                                 ("add", new, 2, 100, sd()), _search(rng, new), ("remove", new, ("draw", sd(), 3)), _search(rng, new)])
    if not sharded:
        small.append(lambda t, new: [("add_refused", t), ("add", t, 1, 100, sd()), _search(rng, t, "knn_media"), _search(rng, t, "descriptors")])
    if sharded:
        big = [[("add", 0, 60, 100, sd())] + ([_search(rng, 0)] if j % 2 else []) for j in range(14)]
    else:
        big = [[("add", 0, 650, 100, sd()), _search(rng, 0)], [("add", 0, 3, 100, sd()), _search(rng, 0)],
               [("add", 0, 6, 100, sd()), _search(rng, 0, "knn"), _search(rng, 0, "descriptors")]]
    last = [("remove", 0, ("all",)), _search(rng, 0), ("add", 0, 2, 100, sd()), _search(rng, 0)]
    ops, handles = list(big[0]), 1
    order = [int(i) for i in rng.permutation(len(small))]
    slots = sorted(int(x) for x in rng.integers(1, len(big) + 1, len(small)))  # after which big step a small segment runs
    for b in range(1, len(big) + 1):
        for i, at in zip(order, slots):
            if at == b:
                t = 0 if rng.random() < 0.7 else int(rng.integers(0, handles))
                for op in small[i](t, handles):
                    handles += op[0] == "slice"
                    ops.append(op)
        if b < len(big):
            ops += big[b]
    ops += last
    while len(ops) < steps:
        ops.append(_search(rng, 0))
    return ops


def coverage(kind, ops):
    world = World(kind)
    f = {"ops": len(ops), "route_after_mutation": set(), "route_second_in_row": set(), "mutation_then_search": set(),
         "slice_parent_used": False, "slice_itself_used": False, "remove_all_then_add": False, "refused_then_add": False,
         "max_needles": 0, "crossings0": None, "turns0": None, "rows0": 0, "searches_between_runs": 0}
    prev, parents, touched, removed_all, refused, after_refusal = None, {}, {}, set(), set(), set()
    seen_turns = 1
    for op in ops:
        t, m = op[1], world.handles[op[1]]
        a = resolve(world, op)
        if op[0] not in MUTATIONS:
            if prev is not None and prev[1] == t:
                if prev[0] in MUTATIONS:
                    f["mutation_then_search"].add(prev[0])
                    f["route_after_mutation"].add(op[0])
                else:
                    f["route_second_in_row"].add(op[0])
            n = len(a["q"]) if "q" in a else max([len(d) for _, d in a.get("needles", [])] + [len(a.get("d", []))])
            f["max_needles"] = max(f["max_needles"], n)
            if touched.get(t):
                f["slice_itself_used" if t in parents else "slice_parent_used"] = True
            if t in after_refusal:
                f["refused_then_add"] = True
            if t == 0 and m.shards and sum(m.turns) > seen_turns:  # the first search after a shard took over
                f["searches_between_runs"] += 1
                seen_turns = sum(m.turns)
        else:
            if op[0] == "slice":
                touched[t], touched[len(world.handles)] = False, False
                parents[len(world.handles)] = t
            elif op[0] in ("add", "remove") and t in touched:
                touched[t] = True
            if op[0] == "add_refused":
                refused.add(t)
            if op[0] == "add":
                if t in refused:
                    after_refusal.add(t)
                if t in removed_all:
                    f["remove_all_then_add"] = True
            removed_all.discard(t)
            if op[0] == "remove" and op[2] == ("all",):
                removed_all.add(t)
            apply_mutation(world, op, a)
        prev = op
    m0 = world.handles[0]
    f["crossings0"], f["turns0"], f["rows0"] = list(m0.crossings), list(m0.turns), m0.count()
    return f
