"""-merge A B (src/main.cpp:1582-1652): the reference's shape written with what exists (database.merge with
batched=False: multi_search per needle, the placement in Python), the DCT stage for all needles in one launch plus the
placement behind the C ABI (cbh_merge_find + cbh_merge_place, merge.hip), and a numpy model of the same rules in this file
that shares no code with either -- held against each other and against hand-checked vectors.

CPU: the loop over a tiny numpy index against the vectors, the cascade over stub indexes, cbh_merge_place against the
model's placement.  GPU: the device route against the vectors, the model and the loop on a real DctHashIndex -- wave and
workgroup edges, every rule of a query, the prefix rule, the error codes, refused allocations, the mixed route with a
real ColorDescIndex and the C++ drop-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cbird_amd import Media, SearchParams
from cbird_amd.database import merge, multi_search
from cbird_amd.index import Match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "test_merge")
PLACED, NO_MATCH, MATCH_UNPLACED = 0, 1, 2
NONE = 0xFFFFFFFF
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def popcount(x):
    return _POP8[np.ascontiguousarray(x, np.uint64).view(np.uint8).reshape(-1, 8)].sum(1).astype(np.int64)


# ---- the numpy model ----------------------------------------------------------------------------------------------------
def model_find(h, ids, n_a, thresh, max_thresh=0, min_matches=1, max_matches=2, in_index=None, dir_id=None, under=None,
               filter_parent=False, path_mode=0):
    """per needle (place of the answer in the arrays or -1, its distance or -1); the arrays hold A then B, so the set of
    needle k without the needle is every place in front of it"""
    h, ids = np.asarray(h, np.uint64), np.asarray(ids, np.int64)
    held = np.ones(len(h), bool) if in_index is None else np.asarray(in_index, bool)
    out = []
    for me in range(n_a, len(h)):
        if h[me] == 0:
            out.append((-1, -1))
            continue
        cand = np.flatnonzero(held[:me])
        d = popcount(h[cand] ^ h[me])
        t = thresh
        if max_thresh > 0:
            while int((d < t).sum()) + (1 if (held[me] and t > 0) else 0) <= min_matches and t + 1 <= max_thresh:
                t += 1
        hit, dh = cand[d < t], d[d < t]
        o = np.lexsort((ids[hit], dh))[:max_matches]
        hit, dh = hit[o], dh[o]
        keep = np.ones(len(hit), bool)
        if path_mode:
            keep &= (np.asarray(under)[hit] != 0) == (path_mode == 1)
        if filter_parent:
            keep &= np.asarray(dir_id)[hit] != dir_id[me]
        hit, dh = hit[keep], dh[keep]
        out.append((int(hit[0]), int(dh[0])) if len(hit) and 1 + len(hit) > min_matches else (-1, -1))
    return out


def model_place(h, n_a, match):
    """(places in merged order, status per needle) for match[k] = a place or -1"""
    h = [int(x) for x in h]
    dist = lambda a, b: bin(h[a] ^ h[b]).count("1")  # noqa: E731
    merged, status = list(range(n_a)), []
    for k, m in enumerate(match):
        me = n_a + k
        if m < 0:
            status.append(NO_MATCH)
        elif m not in merged:
            status.append(MATCH_UNPLACED)
        else:
            at = merged.index(m)
            if 0 < at < len(merged) - 1 and dist(me, merged[at + 1]) < dist(me, merged[at - 1]):
                at += 1
            merged.insert(at, me)
            status.append(PLACED)
    return merged, status


def model_merge(h, ids, n_a, **kw):
    """the DCT stage alone: (merged ids, statuses, [(place or -1, score)] after the limit of 12)"""
    found = [(m, s) if m >= 0 and s < 12 else (-1, -1) for m, s in model_find(h, ids, n_a, **kw)]
    order, status = model_place(h, n_a, [m for m, _ in found])
    return [int(ids[i]) for i in order], status, found


# ---- the vectors ---------------------------------------------------------------------------------------------------------
X = 0x0123456789ABCDEF
CH = [X]
for _k in range(1, 6):
    CH.append(CH[-1] ^ (0b11 << (2 * _k + 20)))  # hamm(CH[i], CH[j]) = 2 |i - j|
# name: (A hashes, A ids, B hashes, B ids, params of model_find, merged ids, statuses, scores of the placed needles);
# "dirs" / "under" are parallel to A then B
VECTORS = {
    # b0 ties between ids 1 and 2, takes 1, the first of the list: in front of it.  b1 takes id 2 at place 2,
    # after = 2 < before = 6: behind it
    "interleave": ([CH[0], CH[2], CH[4]], [1, 2, 3], [CH[1], CH[3]], [4, 5], dict(thresh=3), [4, 1, 2, 5, 3],
                   [PLACED, PLACED], [2, 2]),
    # the tie goes to id 2 = CH[2] at place 1: before = 2, after = 6
    "before_wins": ([CH[0], CH[2], CH[4]], [3, 2, 1], [CH[1]], [4], dict(thresh=3), [3, 4, 2, 1], [PLACED], [2]),
    "match_is_last": ([CH[0], CH[2]], [1, 2], [CH[3]], [3], dict(thresh=3), [1, 3, 2], [PLACED], [2]),
    "match_on_an_earlier_needle": ([CH[0]], [1], [CH[1], CH[2]], [2, 3], dict(thresh=3), [3, 2, 1], [PLACED, PLACED],
                                   [2, 2]),
    "unplaced_match": ([CH[0]], [1], [CH[3], CH[4]], [2, 3], dict(thresh=3), [1], [NO_MATCH, MATCH_UNPLACED], [2]),
    # escalation: the only candidate is 4 bits away -- found when t reaches max_thresh = 5, not at 4
    "escalate_reaches": ([CH[0]], [1], [CH[2]], [2], dict(thresh=3, max_thresh=5), [2, 1], [PLACED], [4]),
    "escalate_one_short": ([CH[0]], [1], [CH[2]], [2], dict(thresh=3, max_thresh=4), [1], [NO_MATCH], []),
    # the needle shares its directory with id 1 (2 bits away); id 2 is 4 bits away.  In the index the needle counts
    # itself, 1 + 1 > minMatches, no escalation, and filterParent removes the only match ...
    "needle_in_the_index": ([CH[0], CH[3]], [1, 2], [CH[1]], [3], dict(thresh=3, max_thresh=5, filter_parent=True,
                                                                       dirs=[0, 1, 0]), [1, 2], [NO_MATCH], []),
    # ... outside it 1 + 0 <= minMatches escalates up to 5, id 2 comes in and survives the filter; it is last in the list
    "needle_outside_the_index": ([CH[0], CH[3]], [1, 2], [CH[1]], [3],
                                 dict(thresh=3, max_thresh=5, filter_parent=True, dirs=[0, 1, 0], in_index=[1, 1, 0]),
                                 [1, 3, 2], [PLACED], [4]),
    "needle_hash_0": ([0b11], [1], [0], [2], dict(thresh=3), [1], [NO_MATCH], []),
    "haystack_hash_0": ([0], [1], [0b11], [2], dict(thresh=3), [2, 1], [PLACED], [2]),
    # minMatches 2 against multiSearch's maxMatches 2: accepted iff both places are taken
    "min2_two_candidates": ([CH[0], CH[2]], [1, 2], [CH[1]], [3], dict(thresh=3, min_matches=2), [3, 1, 2], [PLACED], [2]),
    "min2_one_candidate": ([CH[0], CH[4]], [1, 2], [CH[1]], [3], dict(thresh=3, min_matches=2), [1, 2], [NO_MATCH], []),
    # the needle shares its directory with id 1, the first of two matches: id 2 answers, and it is last in the list
    "filter_parent": ([CH[0], CH[2]], [1, 2], [CH[1]], [3], dict(thresh=3, filter_parent=True, dirs=[0, 1, 0]), [1, 3, 2],
                      [PLACED], [2]),
    "path_in": ([CH[0], CH[2]], [1, 2], [CH[1]], [3], dict(thresh=3, path_mode=1, under=[0, 1, 0]), [1, 3, 2], [PLACED],
                [2]),
    "path_out": ([CH[0], CH[2]], [1, 2], [CH[1]], [3], dict(thresh=3, path_mode=2, under=[1, 0, 0]), [1, 3, 2], [PLACED],
                 [2]),
}


def vector(name):
    """(h, ids, n_a, model_find's keywords, paths, wanted ids, statuses, scores)"""
    ha, ia, hb, ib, kw, want, status, scores = VECTORS[name]
    kw = dict(kw)
    n = len(ia) + len(ib)
    dirs, under = kw.pop("dirs", [0] * n), kw.get("under", [0] * n)
    if kw.get("filter_parent"):
        kw["dir_id"] = np.array(dirs, np.uint32)
    if "under" in kw:
        kw["under"] = np.array(under, np.uint8)
    ids = list(ia) + list(ib)
    paths = [f"/db/{'in' if under[k] else 'out'}/d{dirs[k]}/{ids[k]}.jpg" for k in range(n)]
    return np.array(list(ha) + list(hb), np.uint64), np.array(ids, np.uint32), len(ia), kw, paths, want, status, scores


def params_of(thresh, max_thresh=0, min_matches=1, filter_parent=False, path_mode=0, **_):
    return SearchParams(dctThresh=thresh, maxThresh=max_thresh, minMatches=min_matches, maxMatches=5,
                        filterParent=filter_parent, path="in" if path_mode else "", inPath=path_mode == 1)


def media_of(hashes, ids, paths=None):
    return [Media(id=int(i), dctHash=int(h), path=paths[k] if paths else f"/db/{int(i)}.jpg")
            for k, (h, i) in enumerate(zip(hashes, ids))]


class TinyIndex:
    """find and slice of a 64-bit hash index in numpy, for the loop on a machine without a device"""

    def __init__(self, hashes, ids):
        self.h, self.i = np.asarray(hashes, np.uint64), np.asarray(ids, np.int64)

    def find(self, m, p):
        if not m.dctHash or not len(self.h):
            return []
        d = popcount(self.h ^ np.uint64(m.dctHash))
        return [Match(int(self.i[k]), int(d[k])) for k in np.flatnonzero(d < p.dctThresh)]

    def slice(self, media_ids):
        keep = np.isin(self.i, np.array(sorted(set(media_ids)), np.int64))
        return TinyIndex(self.h[keep], self.i[keep])


def held_of(h, ids, in_index):
    keep = np.ones(len(ids), bool) if in_index is None else np.asarray(in_index, bool)
    return np.asarray(h, np.uint64)[keep], np.asarray(ids, np.uint32)[keep]


def check_vector(name, got, report):
    *_, want, status, scores = vector(name)
    assert [m.id for m in got] == want
    assert [r[0] for r in report] == status
    assert [r[2] for r in report if r[0] != NO_MATCH] == scores
    assert all(r[1] == 0 for r in report if r[0] != NO_MATCH) and all(r[1:] == (-1, -1, 0) for r in report if r[0] == NO_MATCH)


@pytest.mark.parametrize("name", list(VECTORS))
def test_loop_and_model_reproduce_the_vectors(name):
    h, ids, n_a, kw, paths, want, status, scores = vector(name)
    mo, ms, found = model_merge(h, ids, n_a, **kw)
    assert (mo, ms) == (want, status) and [s for m, s in found if m >= 0] == scores
    media = media_of(h, ids, paths)
    got, report = merge(TinyIndex(*held_of(h, ids, kw.get("in_index"))), media[:n_a], media[n_a:], params_of(**kw),
                        batched=False, db_path="/db")
    check_vector(name, got, report)
    assert all(any(m is x for x in media) for m in got)


# ---- the cascade ---------------------------------------------------------------------------------------------------------
class Stub:
    """an index whose find returns prescribed (id, score) pairs per needle id, inside the slice's ids"""

    def __init__(self, answers, ids=None):
        self.answers, self.ids, self.slices = answers, ids, []

    def find(self, m, p):
        return [Match(i, s) for i, s in self.answers.get(m.id, []) if self.ids is None or i in self.ids]

    def slice(self, media_ids):
        part = Stub(self.answers, set(media_ids))
        self.slices.append(part.ids)
        return part


def _cascade(indexes, algo=0, thresh=13):
    a, b = media_of([X], [1]), media_of([X ^ 1], [2])
    p = SearchParams(algo=algo, dctThresh=thresh, maxMatches=5)
    got = multi_search(indexes, b[0], p, {1: a[0], 2: b[0]}, [1, 2])
    merged, report = merge(indexes, a, b, p, batched=False)
    assert report == [(PLACED, got[1], got[0][0].score, 1) if got[0] else (NO_MATCH, -1, -1, 0)]
    assert [m.id for m in merged] == ([2, 1] if got[0] else [1])
    return [(m.id, m.score) for m in got[0]], got[1]


def test_cascade_thresholds():
    hit = lambda s: Stub({2: [(1, s)]})  # noqa: E731
    # DCT at distance 12 under dctThresh 13 is a match of the query and refused by the cascade: the next algo answers
    assert _cascade({0: hit(11)}) == ([(1, 11)], 0)
    assert _cascade({0: hit(12), 1: hit(999)}) == ([(1, 999)], 1)
    assert _cascade({0: hit(12)}) == ([], -1)
    # 999 is accepted and 1000 refused, at algos 1 and 2; any colour score is accepted
    assert _cascade({0: hit(12), 1: hit(1000), 2: hit(999)}) == ([(1, 999)], 2)
    assert _cascade({0: hit(12), 1: hit(1000), 2: hit(1000), 3: hit(2 ** 31 - 2)}) == ([(1, 2 ** 31 - 2)], 3)
    assert _cascade({0: hit(12), 1: hit(1000), 2: hit(1000)}) == ([], -1)
    # a start at algo 2 never asks algos 0 and 1; a missing index counts as no match
    early = hit(1)
    assert _cascade({0: early, 1: early, 2: hit(1000), 3: hit(5)}, algo=2) == ([(1, 5)], 3)
    assert early.slices == []
    assert _cascade({0: hit(12), 3: hit(7)}) == ([(1, 7)], 3)
    assert _cascade({}, algo=1) == ([], -1)
    # a bare index stands for {params.algo: index}
    assert _cascade(hit(3)) == ([(1, 3)], 0)
    assert _cascade(hit(3), algo=3) == ([(1, 3)], 3)


def test_cascade_sets_and_max_matches():
    """needle k is searched inside A + b_0 .. b_k whatever was placed, with maxMatches 2, and a needle without a DCT
    hash skips algo 0 (mediaReady, src/index.cpp:31-52)"""
    a = media_of([X, X], [1, 2])
    b = media_of([X, 0, X], [3, 4, 5])
    dct = Stub({3: [(1, 5), (2, 4), (4, 1), (5, 0)], 4: [(1, 0)], 5: [(1, 9), (2, 8), (3, 7), (4, 6)]})
    col = Stub({4: [(3, 70)]})
    merged, report = merge({0: dct, 3: col}, a, b, SearchParams(dctThresh=13), batched=False)
    assert dct.slices == [{1, 2, 3}, {1, 2, 3, 4, 5}] and col.slices == [{1, 2, 3, 4}]
    assert report == [(PLACED, 0, 4, 2), (PLACED, 3, 70, 3), (PLACED, 0, 6, 4)]
    assert [m.id for m in merged] == [1, 5, 4, 3, 2]
    got, algo = multi_search(dct, b[2], SearchParams(dctThresh=13), {m.id: m for m in a + b}, [1, 2, 3, 4, 5])
    assert [(m.id, m.score) for m in got] == [(4, 6), (3, 7)] and algo == 0


def test_value_errors():
    a, b = media_of([X], [1]), media_of([X ^ 1], [2])
    idx = TinyIndex([X, X ^ 1], [1, 2])
    for batched in (False, True):
        for kw in (dict(filterSelf=False), dict(mirrorMask=1), dict(turnMask=8), dict(algo=4)):
            with pytest.raises(ValueError):
                merge(idx, a, b, SearchParams(**kw), batched=batched)
        with pytest.raises(ValueError):
            merge(idx, a, media_of([X ^ 1], [1]), SearchParams(), batched=batched)
        with pytest.raises(ValueError):
            merge(idx, a + media_of([3], [1]), b, SearchParams(), batched=batched)
        with pytest.raises(ValueError):
            merge(idx, a, media_of([X ^ 1], [0]), SearchParams(), batched=batched)
    with pytest.raises(ValueError):
        multi_search(idx, b[0], SearchParams(algo=4), {1: a[0], 2: b[0]}, [1, 2])


# ---- the placement behind the C ABI: host code, no device -----------------------------------------------------------------
def place(L, h, n_a, match):
    """cbh_merge_place on match[k] = a place or -1: (rc, places in merged order, statuses)"""
    h = np.ascontiguousarray(h, np.uint64)
    n_b = len(h) - n_a
    m32 = np.ascontiguousarray([NONE if m < 0 else m for m in match] + [0], np.uint32)
    order = np.full(len(h) + 1, 0xdeadbeef, np.uint32)
    status = np.full(n_b + 1, 0xee, np.uint8)
    n_out = C.c_size_t(12345)
    rc = L.cbh_merge_place(h.ctypes.data, n_a, n_b, m32.ctypes.data, order.ctypes.data, status.ctypes.data, C.byref(n_out))
    if rc:
        return rc, None, None
    assert (order[n_out.value:] == 0xdeadbeef).all() and status[n_b] == 0xee
    return 0, [int(i) for i in order[:n_out.value]], [int(s) for s in status[:n_b]]


def test_place_equals_the_model():
    from cbird_amd import _lib

    L = _lib.lib()
    rng = np.random.default_rng(5)
    cases = [(0, 0, "random"), (0, 7, "random"), (7, 0, "random"), (5, 9, "none"), (1, 40, "chain"), (0, 6, "chain"),
             (3, 3, "self")]
    cases += [(int(rng.integers(1, 40)), int(rng.integers(1, 60)), "random") for _ in range(40)]
    for n_a, n_b, kind in cases:
        n = n_a + n_b
        h = rng.integers(0, 1 << 12, n, dtype=np.uint64)  # few bits: before / after ties happen
        if kind == "none":
            match = [-1] * n_b
        elif kind == "chain":  # every needle matches the previous one
            match = [n_a + k - 1 if n_a + k > 0 else -1 for k in range(n_b)]
        elif kind == "self":  # itself or a later needle: never placed yet
            match = [n_a + min(k + int(rng.integers(0, 2)), n_b - 1) for k in range(n_b)]
        else:
            match = [int(rng.integers(-1, n_a + k + 2)) if n else -1 for k in range(n_b)]
            match = [m if m < n else -1 for m in match]
        rc, order, status = place(L, h, n_a, match)
        assert rc == 0 and (order, status) == model_place(h, n_a, match), (n_a, n_b, kind)
        if kind == "chain" and n_a:
            assert status == [PLACED] * n_b
        if kind == "chain" and not n_a:
            assert status == [NO_MATCH] + [MATCH_UNPLACED] * (n_b - 1) and order == []
        if kind == "self":
            assert status == [MATCH_UNPLACED] * n_b
    assert place(L, [1, 2, 3], 2, [3])[0] == _lib.CBH_E_INVAL  # a match outside the arrays


@pytest.mark.parametrize("name", ["interleave", "before_wins", "match_is_last", "match_on_an_earlier_needle",
                                  "unplaced_match"])
def test_place_reproduces_the_vectors(name):
    from cbird_amd import _lib

    h, ids, n_a, kw, _, want, status, _ = vector(name)
    rc, order, st = place(_lib.lib(), h, n_a, [m for m, _ in model_find(h, ids, n_a, **kw)])
    assert rc == 0 and [int(ids[i]) for i in order] == want and st == status


def _build_cpp():
    """the rules of tests/cpp/Makefile for one more program"""
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbird_amd", "cpp"), "-I" + os.path.join(CPP, "mock"), "-o", EXE,
                           os.path.join(CPP, "test_merge.cpp"), "-L" + os.path.join(ROOT, "cbird_amd"),
                           "-lcbird_hip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "cbird_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])


def test_dropin_compiles():
    _build_cpp()
    src = open(os.path.join(ROOT, "cbird_amd", "cpp", "gpu_dcthashindex.h")).read()
    assert ("bool gpuMerge(MediaGroup& setA, const MediaGroup& setB, const SearchParams& p, QVector<int>* unanswered,"
            in src)


# ---- the device route ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(gpu):
    from cbird_amd import _lib

    return _lib.lib()


def _ptr(a):
    return None if a is None else a.ctypes.data


def find(L, h, ids, n_a, thresh, max_thresh=0, min_matches=1, max_matches=2, in_index=None, dir_id=None, under=None,
         filter_parent=False, path_mode=0):
    """cbh_merge_find: (rc, [(place or -1, score)])"""
    from cbird_amd import _lib

    h, ids = np.ascontiguousarray(h, np.uint64), np.ascontiguousarray(ids, np.uint32)
    n_b = len(h) - n_a
    arr = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)  # noqa: E731
    in_index, dir_id, under = arr(in_index, np.uint8), arr(dir_id, np.uint32), arr(under, np.uint8)
    mp = _lib.cbh_merge_params(thresh, max_thresh, min_matches, max_matches, int(filter_parent), path_mode)
    match = np.full(n_b + 1, 0xdeadbeef, np.uint32)
    score = np.full(n_b + 1, -77, np.int32)
    rc = L.cbh_merge_find(_ptr(h), _ptr(ids), _ptr(in_index), _ptr(dir_id), _ptr(under), n_a, n_b, C.byref(mp), _ptr(match),
                          _ptr(score), 0)
    if rc:
        return rc, None
    assert match[n_b] == 0xdeadbeef and score[n_b] == -77
    return 0, [(-1 if int(m) == NONE else int(m), int(s)) for m, s in zip(match[:n_b], score[:n_b])]


def found_of(L, h, ids, n_a, **kw):
    rc, got = find(L, h, ids, n_a, **kw)
    assert rc == 0
    return got


def walk(n, seed, flips=(2, 3)):
    """a random walk of hashes -- each item flips a few bits of the previous one -- shuffled, with shuffled ids"""
    rng = np.random.default_rng(seed)
    h = np.zeros(n, np.uint64)
    cur = int(rng.integers(1, 1 << 63))
    for k in range(n):
        for b in rng.choice(64, int(rng.integers(flips[0], flips[1] + 1)), replace=False):
            cur ^= 1 << int(b)
        h[k] = cur
    rng.shuffle(h)
    return h, (rng.permutation(n) + 1).astype(np.uint32)


def real_index(gpu, h, ids, in_index=None):
    idx = gpu.DctHashIndex()
    idx.load(*held_of(h, ids, in_index))
    return idx


def both_routes(gpu, h, ids, n_a, p, in_index=None, paths=None, loop=True):
    """merge() on a real DctHashIndex: the device route, and the loop when asked; (ids, report) of the device route"""
    idx = real_index(gpu, h, ids, in_index)
    media = media_of(h, ids, paths)
    got, report = merge(idx, media[:n_a], media[n_a:], p, batched=True, db_path="/db")
    assert all(any(m is x for x in media) for m in got)
    if loop:
        slow, slow_report = merge(idx, media[:n_a], media[n_a:], p, batched=False, db_path="/db")
        assert ([m.id for m in slow], slow_report) == ([m.id for m in got], report)
    return [m.id for m in got], report


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VECTORS))
def test_device_reproduces_the_vectors(gpu, lib, name):
    h, ids, n_a, kw, paths, want, status, scores = vector(name)
    found = found_of(lib, h, ids, n_a, **kw)
    assert found == model_find(h, ids, n_a, **kw)
    rc, order, st = place(lib, h, n_a, [m for m, _ in found])
    assert rc == 0 and ([int(ids[i]) for i in order], st) == (want, status)
    assert [s for m, s in found if m >= 0] == scores
    media = media_of(h, ids, paths)
    idx = real_index(gpu, h, ids, kw.get("in_index"))
    for batched in (True, False):
        got, report = merge(idx, media[:n_a], media[n_a:], params_of(**kw), batched=batched, db_path="/db")
        check_vector(name, got, report)


# (|A|, |B|): empty sides, one lane short of / at / past a wave, needle counts one below / at / above the kernel's 4 waves
# per workgroup (3, 4, 5; 130 = 32 workgroups and a half), several strides of the lanes (1000 + 257)
EDGES = [(0, 0), (0, 3), (3, 0), (1, 1), (63, 1), (64, 64), (65, 130), (1000, 257), (10, 4), (10, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_a,n_b", EDGES)
def test_wave_and_workgroup_edges(gpu, lib, n_a, n_b):
    """shuffled random walks dense enough that most needles match and some do not, against the model; up to 130 needles
    also against the loop on the real index"""
    h, ids = walk(n_a + n_b, 100 + n_a + n_b)
    kw = dict(thresh=4)
    found = found_of(lib, h, ids, n_a, **kw)
    assert found == model_find(h, ids, n_a, **kw)
    want, status, _ = model_merge(h, ids, n_a, **kw)
    rc, order, st = place(lib, h, n_a, [m for m, _ in found])
    assert rc == 0 and ([int(ids[i]) for i in order], st) == (want, status)
    if n_b >= 64:
        assert status.count(PLACED) > n_b // 2 and status.count(NO_MATCH) > 0
    got, report = both_routes(gpu, h, ids, n_a, params_of(**kw), loop=n_b <= 130)
    assert got == want and [r[0] for r in report] == status
    assert [(r[2], r[3]) for r in report] == [(s, int(ids[m])) if m >= 0 else (-1, 0) for m, s in found]


def _rule_case(seed=7, n_a=40, n_b=30):
    h, ids = walk(n_a + n_b, seed)
    n = n_a + n_b
    rng = np.random.default_rng(seed)
    dirs = rng.integers(0, 2, n).astype(np.uint32)
    under = rng.integers(0, 2, n).astype(np.uint8)
    paths = [f"/db/{'in' if under[k] else 'out'}/d{dirs[k]}/{int(ids[k])}.jpg" for k in range(n)]
    dir_id = np.array([dirs[k] + 2 * under[k] for k in range(n)], np.uint32)  # equal numbers <=> equal directories
    return h, ids, n_a, dir_id, under, paths


RULES = {
    "thresh0": dict(thresh=0),
    "thresh1": dict(thresh=1, copies=True),
    "thresh65": dict(thresh=65),
    "escalate": dict(thresh=2, max_thresh=9),
    "escalate_from_0": dict(thresh=0, max_thresh=7),
    "thresh_above_max": dict(thresh=7, max_thresh=3),
    "in_index": dict(thresh=7, max_thresh=9, holes=True),
    "filter_parent": dict(thresh=7, filter_parent=True),
    "filter_parent_escalate": dict(thresh=4, max_thresh=8, filter_parent=True, holes=True),
    "path_in": dict(thresh=7, path_mode=1),
    "path_out": dict(thresh=7, path_mode=2),
    "max1": dict(thresh=7, max_matches=1, filter_parent=True),
    "max55": dict(thresh=20, max_matches=55, min_matches=3, path_mode=1),
    "max55_escalate": dict(thresh=3, max_thresh=20, max_matches=55, min_matches=5),
    "min0": dict(thresh=7, min_matches=0),
    "min_above_max": dict(thresh=9, max_thresh=12, min_matches=3),
    "hash0": dict(thresh=7, zero=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("rule", list(RULES))
def test_rules_of_a_query(gpu, lib, rule):
    h, ids, n_a, dir_id, under, paths = _rule_case()
    kw = dict(RULES[rule])
    in_index = None
    if kw.pop("holes", False):
        in_index = np.ones(len(h), np.uint8)
        in_index[[0, 3, 11, 30, 41, 42, 55, 69]] = 0  # items of A, needles, the last needle
    if kw.pop("copies", False):
        h[[44, 60, 61]] = h[[7, 43, 43]]  # an item of A again, and a needle twice again
    if kw.pop("zero", False):
        h[[2, 45, 46]] = 0  # an item of A and two needles: no needle hash, and a haystack hash like any other ...
        h[50] = 0b111       # ... for this needle, three bits from all three
    if kw.get("filter_parent"):
        kw["dir_id"] = dir_id
    if kw.get("path_mode"):
        kw["under"] = under
    if in_index is not None:
        kw["in_index"] = in_index
    found = found_of(lib, h, ids, n_a, **kw)
    assert found == model_find(h, ids, n_a, **kw)
    answered = sum(m >= 0 for m, _ in found)
    assert (answered == 0) == (rule in ("thresh0", "min_above_max"))
    if rule == "thresh1":
        assert all(s == 0 for m, s in found if m >= 0)
    if rule == "thresh65":
        assert answered == len(found)  # everything is a candidate, the first needle's set is A
    if rule == "hash0":
        best = min((2, 45, 46), key=lambda k: ids[k])
        assert found[5] == found[6] == (-1, -1) and found[10] == (best, 3)
    if rule == "in_index":
        gone = set(np.flatnonzero(in_index == 0).tolist())
        assert not gone & {m for m, _ in found}
    if kw.get("max_matches", 2) == 2:  # multiSearch's own: the Python entry and the loop on a real index
        p = params_of(**kw)
        got, report = both_routes(gpu, h, ids, n_a, p, in_index, paths)
        want, status, _ = model_merge(h, ids, n_a, **kw)
        assert got == want and [r[0] for r in report] == status


@pytest.mark.gpu
def test_prefix_rule(gpu, lib):
    """B = copies of one hash, A far away: every needle's only candidates are other needles, and needle k may match
    b_j only for j < k -- the smallest id among them"""
    n_a, n_b = 70, 67
    rng = np.random.default_rng(3)
    a = rng.integers(1, 1 << 62, n_a, dtype=np.uint64) | np.uint64(0xFFFF << 48)
    h = np.concatenate([a, np.full(n_b, 0x1234, np.uint64)])
    ids = (rng.permutation(n_a + n_b) + 1).astype(np.uint32)
    found = found_of(lib, h, ids, n_a, thresh=3)
    assert found == model_find(h, ids, n_a, thresh=3)
    assert found[0] == (-1, -1)
    for k in range(1, n_b):
        m, s = found[k]
        assert n_a <= m < n_a + k and s == 0 and ids[m] == ids[n_a:n_a + k].min()
    # the first needle is dropped, the second matches it: unplaced; so is every later one
    got, report = both_routes(gpu, h, ids, n_a, params_of(3))
    assert got == [int(i) for i in ids[:n_a]]
    assert [r[0] for r in report] == [NO_MATCH] + [MATCH_UNPLACED] * (n_b - 1)
    # with the first needle inside reach of A every needle is placed
    h[5] = 0x1234 ^ 0b11
    got, report = both_routes(gpu, h, ids, n_a, params_of(3))
    assert len(got) == n_a + n_b and all(r[0] == PLACED for r in report)
    assert (got, [r[0] for r in report]) == model_merge(h, ids, n_a, thresh=3)[:2]


@pytest.mark.gpu
def test_error_codes(lib):
    from cbird_amd import _lib

    h, ids = walk(20, 1)
    zero = ids.copy()
    zero[13] = 0
    assert find(lib, h, zero, 10, 5)[0] == _lib.CBH_E_INVAL
    for a, b in ((2, 13), (2, 5), (12, 17)):  # A and B, inside A, inside B
        twice = ids.copy()
        twice[b] = twice[a]
        assert find(lib, h, twice, 10, 5)[0] == _lib.CBH_E_INVAL
    assert find(lib, h, ids, 10, 5, max_matches=0)[0] == find(lib, h, ids, 10, 5, max_matches=56)[0] == _lib.CBH_E_INVAL
    assert find(lib, h, ids, 10, 66)[0] == find(lib, h, ids, 10, -1)[0] == _lib.CBH_E_INVAL
    assert find(lib, h, ids, 10, 5, max_thresh=66)[0] == find(lib, h, ids, 10, 5, max_thresh=-1)[0] == _lib.CBH_E_INVAL
    assert find(lib, h, ids, 10, 5, path_mode=3)[0] == find(lib, h, ids, 10, 5, path_mode=-1)[0] == _lib.CBH_E_INVAL
    assert find(lib, h, ids, 10, 5, filter_parent=True)[0] == find(lib, h, ids, 10, 5, path_mode=1)[0] == _lib.CBH_E_INVAL
    assert find(lib, h, ids, 10, 65, max_thresh=65, max_matches=55)[0] == 0
    # 2^24 items: refused before anything is read
    mp = _lib.cbh_merge_params(5, 0, 1, 2, 0, 0)
    one = np.ones(1, np.uint64)
    assert lib.cbh_merge_find(one.ctypes.data, one.ctypes.data, None, None, None, (1 << 24) - 1, 1, C.byref(mp),
                              one.ctypes.data, one.ctypes.data, 0) == _lib.CBH_E_UNSUPPORTED
    assert find(lib, h[:0], ids[:0], 0, 5) == (0, [])


def _tuning(L, key):
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0
    return v.value


@pytest.mark.gpu
def test_every_allocation_may_be_refused(lib):
    """the walk of tests/test_error_paths.py: every refused call returns CBH_E_NOMEM, leaves no scratch handed out, and
    the next call gives the same results"""
    from cbird_amd import _lib

    L = lib
    h, ids = walk(90, 40)
    first = find(L, h, ids, 50, 7)
    assert first[0] == 0
    refused = 0
    for k in range(100):
        live0, fired0 = _tuning(L, b"arena_live_bytes"), _tuning(L, b"fault_fired")
        L.cbh_set_tuning(b"fault_alloc_after", k)
        try:
            rc, _ = find(L, h, ids, 50, 7)
        finally:
            L.cbh_set_tuning(b"fault_alloc_after", -1)
        if _tuning(L, b"fault_fired") == fired0:
            assert rc == 0
            break
        refused += 1
        assert rc == _lib.CBH_E_NOMEM, (k, rc)
        assert _tuning(L, b"arena_live_bytes") == live0, k
        assert find(L, h, ids, 50, 7) == first, k
    else:
        pytest.fail("the call never ran out of allocations to refuse")
    # staged: hashes, ids, match, score; scratch: keys, values, hashes, seen, attributes, needle places, status, and the
    # sort's two buffers and workspace
    assert refused == 4 + 7 + 3


@pytest.mark.gpu
def test_mixed_route_with_a_colour_index(gpu):
    """a DCT stage that refuses some needles (no candidate under dctThresh, or one at 12 bits or more) and a real
    ColorDescIndex as algo 3 answering them: the device route equals the loop"""
    import color_search_cases as CS
    from cbird_amd.colordesc import ColorDescIndex

    n_a, n_b = 60, 45
    h, ids = walk(n_a + n_b, 21, flips=(8, 12))
    descs, _ = CS.synth_descriptors(n_a + n_b, 8, dup_frac=0.9)
    media = media_of(h, ids)
    for m, d in zip(media, descs):
        m.colorDescriptor = d
    dct = real_index(gpu, h, ids)
    colour = ColorDescIndex()
    colour.add(media)
    p = SearchParams(dctThresh=14, maxThresh=0)
    fast, fast_report = merge({0: dct, 3: colour}, media[:n_a], media[n_a:], p, batched=True)
    slow, slow_report = merge({0: dct, 3: colour}, media[:n_a], media[n_a:], p, batched=False)
    assert ([m.id for m in fast], fast_report) == ([m.id for m in slow], slow_report)
    algos = [r[1] for r in fast_report]
    assert algos.count(0) > 5 and algos.count(3) > 0
    # the DCT answers are the model's; the needles it refused at a score of 12 or 13 went on to the colour index
    found = model_find(h, ids, n_a, thresh=14)
    assert any(s >= 12 for _, s in found)
    for (m, s), r in zip(found, fast_report):
        assert (r[1] == 0 and (r[2], r[3]) == (s, int(ids[m]))) if 0 <= s < 12 else r[1] != 0


@pytest.mark.gpu
def test_dropin_runs_on_gpu(gpu, tmp_path):
    """GpuDctHashIndex::gpuMerge on one vector and one random case: the merged ids and the unanswered needles"""
    h, ids = walk(150, 9)
    cases = [vector("interleave")[:3] + (3,), (h, ids, 100, 3)]
    path = tmp_path / "sets.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for ch, ci, n_a, thresh in cases:
            f.write(np.array([n_a, len(ci) - n_a, thresh], np.int32).tobytes())
            for x, i in zip(ch, ci):
                f.write(np.uint32(i).tobytes() + np.uint64(x).tobytes())
    _build_cpp()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    for c, (ch, ci, n_a, thresh) in enumerate(cases):
        media = media_of(ch, ci)
        got, report = merge(real_index(gpu, ch, ci), media[:n_a], media[n_a:], SearchParams(dctThresh=thresh))
        unanswered = [k for k, r in enumerate(report) if r[0] == NO_MATCH]
        assert lines[c] == (f"case {c} unanswered " + " ".join(str(k) for k in unanswered) + " : " +
                            " ".join(str(m.id) for m in got)).replace("  ", " ")
    assert len(unanswered) > 0
