"""-sort-similar (src/main.cpp:1523-1580): the reference's loop written with what exists (database.sort_similar with
batched=False), the whole chain in one kernel launch (cbh_sort_similar, sortsimilar.hip) and a vectorised numpy model of
the same rules in this file, held against each other and against hand-checked vectors.

CPU: the loop over a tiny numpy index against the vectors.  GPU: the device route against the loop on a real
DctHashIndex and against the model -- the vectors, wave and workgroup edges, a ragged batch, the LDS residency boundary,
every rule of a query, the error codes, the Python batch entry and the C++ drop-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cbird_amd import Media, SearchParams
from cbird_amd.database import sort_similar, sort_similar_batch
from cbird_amd.index import Match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "test_sort_similar")
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def popcount(x):
    return _POP8[np.ascontiguousarray(x, np.uint64).view(np.uint8).reshape(-1, 8)].sum(1).astype(np.int64)


# ---- the numpy model ----------------------------------------------------------------------------------------------------
def model(hashes, ids, thresh, max_thresh=0, min_matches=1, max_matches=5, in_index=None, dir_id=None, under=None,
          filter_parent=False, path_mode=0, look_behind=5):
    """(ids in sorted order, queries, notFound, behind) of one selection given in selection order; a query is one
    vectorised pass over the unsorted items; a whole i iteration without an insert ends the loop in closed form"""
    h, ids = np.asarray(hashes, np.uint64), np.asarray(ids, np.int64)
    n = len(h)
    if n < 2:
        return [int(i) for i in ids], 0, 0, 0
    held = np.ones(n, bool) if in_index is None else np.asarray(in_index, bool)
    avail = held.copy()
    avail[0] = False
    order, queries, not_found, behind = [0], 0, 0, 0

    def ask(needle):
        if h[needle] == 0:
            return None
        d = popcount(h ^ h[needle])
        cand = np.flatnonzero(avail)
        dc = d[cand]
        t = thresh
        if max_thresh > 0:
            while int((dc < t).sum()) + (1 if (held[needle] and t > 0) else 0) <= min_matches:
                if t + 1 > max_thresh:
                    break
                t += 1
        hit = cand[dc < t]
        hit = hit[np.lexsort((ids[hit], d[hit]))][:max_matches]
        if path_mode:
            hit = hit[(under[hit] != 0) == (path_mode == 1)]
        if filter_parent:
            hit = hit[dir_id[hit] != dir_id[needle]]
        return int(hit[0]) if len(hit) and 1 + len(hit) > min_matches else None

    for i in range(n - 1):
        inserted, j = False, 0
        while j < min(look_behind, len(order)):
            got = ask(order[len(order) - 1 - j])
            if got is None:
                not_found += 1
            else:
                order.insert(len(order) - j, got)
                avail[got] = False
                inserted = True
                behind += j > 0
            queries += 1
            j += 1
        if not inserted:
            rest = (n - 2 - i) * min(look_behind, len(order))
            queries, not_found = queries + rest, not_found + rest
            break
    return [int(ids[k]) for k in order], queries, not_found, int(behind)


# ---- the vectors ---------------------------------------------------------------------------------------------------------
X = 0x0123456789ABCDEF
NEIGHBOURS = [X ^ (0b111 << (3 * k)) for k in range(6)]
CHAIN = [X]
for _k in range(1, 6):
    CHAIN.append(CHAIN[-1] ^ (0b11 << (2 * _k + 20)))
STAR = [X] + NEIGHBOURS
AS1 = ([1, 6, 5, 4, 3, 2], 30, 25, 4)
# name: (hashes, ids, params, (order, queries, notFound, behind or None))
VECTORS = {
    "1": (STAR, [1, 2, 3, 4, 5, 6, 7], dict(thresh=4), AS1),
    "2_ids_reversed": (STAR, [1, 7, 6, 5, 4, 3, 2], dict(thresh=4), AS1),
    "3_escalate": (STAR, [1, 2, 3, 4, 5, 6, 7], dict(thresh=1, max_thresh=4), AS1),
    "4_escalate_short": (STAR, [1, 2, 3, 4, 5, 6, 7], dict(thresh=1, max_thresh=3), ([1], 6, 6, None)),
    "5_min2": (STAR, [1, 2, 3, 4, 5, 6, 7], dict(thresh=4, min_matches=2), AS1),
    "6_min2_max1": (STAR, [1, 2, 3, 4, 5, 6, 7], dict(thresh=4, min_matches=2, max_matches=1), ([1], 6, 6, None)),
    "7_min0": (STAR, [1, 2, 3, 4, 5, 6, 7], dict(thresh=4, min_matches=0), AS1),
    "8_chain": (CHAIN, [1, 2, 3, 4, 5, 6], dict(thresh=3), ([1, 2, 3, 4, 5, 6], 19, 14, None)),
    "9_chain_from_2": ([CHAIN[p] for p in (2, 0, 1, 3, 4, 5)], [3, 1, 2, 4, 5, 6], dict(thresh=3),
                       ([3, 4, 5, 6, 2, 1], 23, 18, 3)),
    "10_pair": ([X, X ^ 1], [8, 9], dict(thresh=2), ([8, 9], 2, 1, None)),
}


def params_of(thresh, max_thresh=0, min_matches=1, max_matches=5, filter_parent=False, path="", in_path=False):
    return SearchParams(dctThresh=thresh, maxThresh=max_thresh, minMatches=min_matches, maxMatches=max_matches,
                        filterParent=filter_parent, path=path, inPath=in_path)


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


@pytest.mark.parametrize("name", list(VECTORS))
def test_loop_reproduces_the_vectors(name):
    hashes, ids, kw, (order, queries, not_found, behind) = VECTORS[name]
    got, q, nf = sort_similar(TinyIndex(hashes, ids), media_of(hashes, ids), params_of(**kw), batched=False)
    assert ([m.id for m in got], q, nf) == (order, queries, not_found)
    mo, mq, mnf, mb = model(hashes, ids, **kw)
    assert (mo, mq, mnf) == (order, queries, not_found) and (behind is None or mb == behind)


def test_loop_degenerate_selections_and_the_self_filter():
    idx = TinyIndex([X], [1])
    assert sort_similar(idx, [], params_of(4), batched=False) == ([], 0, 0)
    one = media_of([X], [1])
    assert sort_similar(idx, one, params_of(4), batched=False) == (one, 0, 0)
    p = params_of(4)
    p.filterSelf = False
    for batched in (False, True):
        with pytest.raises(ValueError):
            sort_similar(idx, one, p, batched=batched)
    with pytest.raises(ValueError):
        sort_similar_batch(idx, [one], p)


def test_dropin_compiles():
    _build_cpp()
    src = open(os.path.join(ROOT, "cbird_amd", "cpp", "gpu_dcthashindex.h")).read()
    assert "bool gpuSortSimilar(MediaGroup& selection, const SearchParams& p, int* queries, int* notFound," in src


def _build_cpp():
    """the rules of tests/cpp/Makefile for one more program"""
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbird_amd", "cpp"), "-I" + os.path.join(CPP, "mock"), "-o", EXE,
                           os.path.join(CPP, "test_sort_similar.cpp"), "-L" + os.path.join(ROOT, "cbird_amd"),
                           "-lcbird_hip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "cbird_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])


# ---- the device route ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(gpu):
    from cbird_amd import _lib

    return _lib.lib()


def _ptr(a):
    return None if a is None else a.ctypes.data


def device(L, sets, thresh, max_thresh=0, min_matches=1, max_matches=5, filter_parent=False, path_mode=0, look_behind=5,
           front=0):
    """cbh_sort_similar on sets = [(hashes, ids, in_index | None, dir_id | None, under | None)]; `front` unused items
    in front of the first set (set_first need not start at 0).  (rc, [(order, queries, notFound, behind)])"""
    from cbird_amd import _lib

    cat = lambda k, dt, fill: np.ascontiguousarray(np.concatenate(  # noqa: E731
        [np.full(front, fill, dt)] + [np.asarray(s[k] if s[k] is not None else np.full(len(s[0]), fill), dt) for s in sets]))
    hashes, ids = cat(0, np.uint64, 0), cat(1, np.uint32, 0)
    in_index = cat(2, np.uint8, 1) if any(s[2] is not None for s in sets) else None
    dir_id = cat(3, np.uint32, 0) if any(s[3] is not None for s in sets) else None
    under = cat(4, np.uint8, 0) if any(s[4] is not None for s in sets) else None
    first = np.zeros(len(sets) + 1, np.uint64)
    first[0] = front
    np.cumsum([len(s[0]) for s in sets], out=first[1:])
    first[1:] += np.uint64(front)
    sp = _lib.cbh_sort_similar_params(thresh, max_thresh, min_matches, max_matches, int(filter_parent), path_mode,
                                      look_behind)
    out_ids = np.full(max(len(ids), 1), 0xdeadbeef, np.uint32)
    res = (_lib.cbh_sort_similar_result * max(len(sets), 1))()
    rc = L.cbh_sort_similar(_ptr(hashes), _ptr(ids), _ptr(in_index), _ptr(dir_id), _ptr(under), _ptr(first), len(sets),
                            C.byref(sp), _ptr(out_ids), res, 0)
    if rc:
        return rc, None
    assert (out_ids[:front] == 0xdeadbeef).all()
    out = []
    for s in range(len(sets)):
        a, b, k = int(first[s]), int(first[s + 1]), res[s].sorted
        assert k <= b - a and (out_ids[a + k:b] == 0).all()
        out.append(([int(i) for i in out_ids[a:a + k]], res[s].queries, res[s].not_found, res[s].behind))
    return 0, out


def one(L, hashes, ids, thresh, in_index=None, dir_id=None, under=None, **kw):
    rc, out = device(L, [(hashes, ids, in_index, dir_id, under)], thresh, **kw)
    assert rc == 0
    return out[0]


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


def real_index(gpu, hashes, ids, in_index=None):
    idx = gpu.DctHashIndex()
    keep = np.ones(len(ids), bool) if in_index is None else np.asarray(in_index, bool)
    idx.load(np.asarray(hashes, np.uint64)[keep], np.asarray(ids, np.uint32)[keep])
    return idx


def loop(gpu, hashes, ids, p, in_index=None, paths=None, db_path=""):
    got, q, nf = sort_similar(real_index(gpu, hashes, ids, in_index), media_of(hashes, ids, paths), p, batched=False,
                              db_path=db_path)
    return [m.id for m in got], q, nf


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VECTORS))
def test_device_reproduces_the_vectors(gpu, lib, name):
    hashes, ids, kw, (order, queries, not_found, behind) = VECTORS[name]
    o, q, nf, b = one(lib, hashes, ids, **kw)
    assert (o, q, nf) == (order, queries, not_found) and (behind is None or b == behind)
    assert (o, q, nf, b) == model(hashes, ids, **kw)
    got, q2, nf2 = sort_similar(real_index(gpu, hashes, ids), media_of(hashes, ids), params_of(**kw))
    assert ([m.id for m in got], q2, nf2) == (order, queries, not_found)


EDGES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025]


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGES)
def test_wave_and_workgroup_edges(gpu, lib, n):
    """one lane short of, at and one past a wave and the largest workgroup, against the model and against the loop; the
    walks are dense enough that look-behind inserts happen and sparse enough that the chain breaks off"""
    h, ids = walk(n, 100 + n)
    thresh = 6 + n % 4
    got = one(lib, h, ids, thresh)
    assert got == model(h, ids, thresh)
    assert got[:3] == loop(gpu, h, ids, params_of(thresh))
    if n >= 63:
        assert got[3] > 0 and len(got[0]) < n
    if n <= 1:
        assert got == ([int(i) for i in ids], 0, 0, 0)


@pytest.mark.gpu
def test_ragged_batch_equals_the_single_calls(lib):
    sets = [walk(n, 300 + k) + (None, None, None) for k, n in enumerate([0, 1, 2, 70, 1, 1025])]
    rc, out = device(lib, sets, 7, front=3)
    assert rc == 0
    for s, got in zip(sets, out):
        assert got == one(lib, s[0], s[1], 7) == model(s[0], s[1], 7)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16384, 16385])
def test_residency_boundary(lib, n):
    """the largest set whose hashes stay in LDS and the smallest that reads them from memory: random hashes, no two of
    them near each other, and a chain of 40 whose positions in id order are among the last 64"""
    rng = np.random.default_rng(n)
    h = rng.integers(1, 1 << 63, n, dtype=np.uint64) | np.uint64(1 << 63)
    ids = (rng.permutation(n - 64) + 1).astype(np.uint32)
    ids = np.concatenate([ids, rng.permutation(np.arange(n - 63, n + 1)).astype(np.uint32)])
    chain = [int(h[n - 64])]
    for k in range(1, 40):
        chain.append(chain[-1] ^ (0b11 << (k % 31 * 2)))
    h[n - 64:n - 24] = np.array(chain, np.uint64)
    # selection order: the chain's start first, everything else shuffled
    perm = np.concatenate([[n - 64], rng.permutation(np.delete(np.arange(n), n - 64))])
    h, ids = h[perm], ids[perm]
    assert sorted(ids.tolist()) == list(range(1, n + 1))
    want = model(h, ids, 3)
    got = one(lib, h, ids, 3)
    assert got == want
    by_hash = {int(x): int(i) for x, i in zip(h, ids)}
    assert got[0] == [by_hash[c] for c in chain] and min(got[0]) > n - 64


def _rule_case(seed=7, n=48):
    h, ids = walk(n, seed)
    rng = np.random.default_rng(seed)
    dirs = rng.integers(0, 2, n).astype(np.uint32)
    under = rng.integers(0, 2, n).astype(np.uint8)
    paths = [f"/db/{'in' if under[k] else 'out'}/d{dirs[k]}/{int(ids[k])}.jpg" for k in range(n)]
    dir_id = np.array([dirs[k] + 2 * under[k] for k in range(n)], np.uint32)  # equal numbers <=> equal directories
    return h, ids, dir_id, under, paths


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["thresh0", "thresh_above_max", "first_hash0", "haystack_hash0", "in_index",
                                  "filter_parent", "path_in", "path_out", "look_behind1", "look_behind8"])
def test_rules_of_a_query(gpu, lib, rule):
    h, ids, dir_id, under, paths = _rule_case()
    n = len(h)
    kw, in_index, cmp_loop = dict(thresh=7), None, True
    if rule == "thresh0":
        kw = dict(thresh=0)
    elif rule == "thresh_above_max":
        kw = dict(thresh=7, max_thresh=3)
    elif rule == "first_hash0":
        h[0] = 0
    elif rule == "haystack_hash0":
        h[5] = 0  # a neighbour of the start, three bits away
        h[0] = 0b111
    elif rule == "in_index":
        in_index = np.ones(n, np.uint8)
        in_index[[0, 3, 4, 11, 30]] = 0
    elif rule == "filter_parent":
        kw = dict(thresh=7, filter_parent=True)
    elif rule == "path_in":
        kw = dict(thresh=7, path_mode=1)
    elif rule == "path_out":
        kw = dict(thresh=7, path_mode=2)
    else:
        kw, cmp_loop = dict(thresh=7, look_behind=int(rule[len("look_behind"):])), False  # the loop's is fixed at 5
    got = one(lib, h, ids, in_index=in_index, dir_id=dir_id if kw.get("filter_parent") else None,
              under=under if kw.get("path_mode") else None, **kw)
    assert got == model(h, ids, in_index=in_index, dir_id=dir_id, under=under, **kw)
    if rule == "thresh0":
        assert got == ([int(ids[0])], n - 1, n - 1, 0)
    if rule == "first_hash0":
        assert got == ([int(ids[0])], n - 1, n - 1, 0)
    if rule == "haystack_hash0":
        assert got[0][:2] == [int(ids[0]), int(ids[5])]
    if rule == "in_index":
        assert not set(got[0][1:]) & {int(ids[k]) for k in (3, 4, 11, 30)} and len(got[0]) > 1
    if rule == "look_behind1":
        assert got[3] == 0
    if cmp_loop:
        mode = kw.get("path_mode", 0)
        p = params_of(kw["thresh"], kw.get("max_thresh", 0), filter_parent=kw.get("filter_parent", False),
                      path="in" if mode else "", in_path=mode == 1)
        assert got[:3] == loop(gpu, h, ids, p, in_index, paths, db_path="/db")
        # the Python entry derives in_index from the index and the attributes from the paths
        o, q, nf = sort_similar(real_index(gpu, h, ids, in_index), media_of(h, ids, paths), p, db_path="/db")
        assert ([m.id for m in o], q, nf) == got[:3]


@pytest.mark.gpu
@pytest.mark.parametrize("min_matches", [0, 1, 2, 3])
@pytest.mark.parametrize("max_matches", [1, 2, 5])
def test_min_and_max_matches(gpu, lib, min_matches, max_matches):
    """with and without escalation, with and without a filter, the needle in the index or not"""
    h, ids, dir_id, under, paths = _rule_case(seed=9, n=40)
    out_of_index = np.ones(len(h), np.uint8)
    out_of_index[[0, 7]] = 0
    seen = []
    for max_thresh, fp, in_index in ((0, False, None), (9, False, None), (9, True, None), (9, False, out_of_index)):
        kw = dict(thresh=5, max_thresh=max_thresh, min_matches=min_matches, max_matches=max_matches, filter_parent=fp)
        got = one(lib, h, ids, in_index=in_index, dir_id=dir_id if fp else None, **kw)
        assert got == model(h, ids, in_index=in_index, dir_id=dir_id, **kw)
        seen.append(got)
    p = params_of(5, 9, min_matches, max_matches, filter_parent=True)
    assert seen[2][:3] == loop(gpu, h, ids, p, None, paths, db_path="/db")
    if min_matches > max_matches:
        assert all(len(g[0]) == 1 for g in seen)


@pytest.mark.gpu
def test_error_codes(lib):
    from cbird_amd import _lib

    h, ids = walk(20, 1)
    zero = ids.copy()
    zero[13] = 0
    assert device(lib, [(h, zero, None, None, None)], 5)[0] == _lib.CBH_E_INVAL
    twice = ids.copy()
    twice[13] = twice[2]
    assert device(lib, [(h, twice, None, None, None)], 5)[0] == _lib.CBH_E_INVAL
    ok = [(h, ids, None, None, None)]
    assert device(lib, ok, 5, look_behind=0)[0] == device(lib, ok, 5, look_behind=9)[0] == _lib.CBH_E_INVAL
    assert device(lib, ok, 5, max_matches=0)[0] == device(lib, ok, 5, max_matches=56)[0] == _lib.CBH_E_INVAL
    assert device(lib, ok, 5, filter_parent=True)[0] == device(lib, ok, 5, path_mode=1)[0] == _lib.CBH_E_INVAL
    assert device(lib, ok, 66)[0] == device(lib, ok, -1)[0] == _lib.CBH_E_INVAL
    assert device(lib, ok, 5, max_matches=55, look_behind=8)[0] == 0
    big = np.arange(1, _lib.CBH_SORT_SIMILAR_MAX + 2, dtype=np.uint32)
    assert device(lib, [(big.astype(np.uint64), big, None, None, None)], 5)[0] == _lib.CBH_E_UNSUPPORTED
    assert device(lib, [], 5) == (0, [])


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
    sets = [walk(n, 40 + n) + (None, None, None) for n in (70, 3)]
    rc, first = device(L, sets, 7)
    assert rc == 0
    refused = 0
    for k in range(100):
        live0, fired0 = _tuning(L, b"arena_live_bytes"), _tuning(L, b"fault_fired")
        L.cbh_set_tuning(b"fault_alloc_after", k)
        try:
            rc, _ = device(L, sets, 7)
        finally:
            L.cbh_set_tuning(b"fault_alloc_after", -1)
        if _tuning(L, b"fault_fired") == fired0:
            assert rc == 0
            break
        refused += 1
        assert rc == _lib.CBH_E_NOMEM, (k, rc)
        assert _tuning(L, b"arena_live_bytes") == live0, k
        assert device(L, sets, 7) == (0, first), k
    else:
        pytest.fail("the call never ran out of allocations to refuse")
    # staged: hashes, ids, set_first, out_ids, out; scratch: keys, values, hashes, ids, attributes, first places, status,
    # and the sort's two buffers and workspace
    assert refused == 5 + 7 + 3


@pytest.mark.gpu
def test_batch_entry_equals_the_single_calls(gpu):
    h, ids = walk(300, 77)
    idx = real_index(gpu, h, ids)
    media = media_of(h, ids)
    selections = [media[:120], [], media[120:121], media[121:300], media[50:200]]
    p = params_of(7, max_thresh=9)
    got = sort_similar_batch(idx, selections, p)
    assert len(got) == len(selections)
    for sel, (o, q, nf) in zip(selections, got):
        o1, q1, nf1 = sort_similar(idx, sel, p)
        assert ([m.id for m in o], q, nf) == ([m.id for m in o1], q1, nf1)
        assert all(any(m is x for x in sel) for m in o)
    o, q, nf = got[4]
    assert ([m.id for m in o], q, nf) == model(h[50:200], ids[50:200], 7, 9)[:3]
    # an index that is no DctHashIndex, or reflections: the loop
    tiny = TinyIndex(h, ids)
    o2, q2, nf2 = sort_similar_batch(tiny, [selections[0]], params_of(7))[0]
    assert ([m.id for m in o2], q2, nf2) == model(h[:120], ids[:120], 7)[:3]


@pytest.mark.gpu
def test_dropin_runs_on_gpu(gpu, tmp_path):
    cases = ["1", "9_chain_from_2"]
    path = tmp_path / "sets.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for name in cases:
            hashes, ids, kw, _ = VECTORS[name]
            f.write(np.array([len(ids), kw["thresh"]], np.int32).tobytes())
            for h, i in zip(hashes, ids):
                f.write(np.uint32(i).tobytes() + np.uint64(h).tobytes())
    _build_cpp()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    for c, name in enumerate(cases):
        order, queries, not_found, _ = VECTORS[name][3]
        assert lines[c] == f"case {c} {queries} {not_found} : " + " ".join(str(i) for i in order)
