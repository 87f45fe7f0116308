"""-sort-similar over a table of scores on the device: cbh_sort_similar_table (sortsimilar_table.hip) against the plain
model of tests/sort_similar_table_rules.py and against cbh_sort_similar on Hamming tables; cbh_color_sort_similar
(color.hip) against the model fed with np_scores, and database.sort_similar(batched=True) against the loop on the same
ColorDescIndex.  Every comparison is exact: orders, queries, notFound, behind."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import color_search_cases as CS
import test_sort_similar as TS
import test_sort_similar_table_rules as TR
from cbird_amd.database import sort_similar, sort_similar_batch
from sort_similar_table_rules import NO_MATCH, hamming_table, table_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "test_sort_similar_color")


@pytest.fixture(scope="module")
def lib(gpu):
    from cbird_amd import _lib

    return _lib.lib()


def _ptr(a):
    return None if a is None else a.ctypes.data


def device(L, sets, min_matches=1, max_matches=5, filter_parent=False, path_mode=0, look_behind=5, front=0):
    """cbh_sort_similar_table on sets = [(table [n, n] in selection order, ids, in_index | None, dir_id | None, under |
    None)]; `front` unused items in front of the first set and 3 * front unused scores in front of every table (neither
    set_first nor table_first need start at 0, and tables need not be 16-byte aligned).
    (rc, [(order, queries, notFound, behind)])"""
    from cbird_amd import _lib

    cat = lambda k, dt, fill: np.ascontiguousarray(np.concatenate(  # noqa: E731
        [np.full(front, fill, dt)] + [np.asarray(s[k] if s[k] is not None else np.full(len(s[1]), fill), dt) for s in sets]))
    ids = cat(1, np.uint32, 0)
    in_index = cat(2, np.uint8, 1) if any(s[2] is not None for s in sets) else None
    dir_id = cat(3, np.uint32, 0) if any(s[3] is not None for s in sets) else None
    under = cat(4, np.uint8, 0) if any(s[4] is not None for s in sets) else None
    first = np.zeros(len(sets) + 1, np.uint64)
    first[0] = front
    np.cumsum([len(s[1]) for s in sets], out=first[1:])
    first[1:] += np.uint64(front)
    parts, table_first, at = [], np.zeros(max(len(sets), 1), np.uint64), 0
    for k, s in enumerate(sets):
        parts.append(np.full(3 * front, 7, np.uint16))  # (a score that would match, were it ever read)
        table_first[k] = at + 3 * front
        parts.append(np.asarray(s[0], np.uint16).reshape(-1))
        at += 3 * front + len(s[1]) ** 2
    scores = np.ascontiguousarray(np.concatenate(parts + [np.zeros(1, np.uint16)]))
    sp = _lib.cbh_sort_table_params(min_matches, max_matches, int(filter_parent), path_mode, look_behind)
    out_ids = np.full(max(len(ids), 1), 0xdeadbeef, np.uint32)
    res = (_lib.cbh_sort_similar_result * max(len(sets), 1))()
    rc = L.cbh_sort_similar_table(_ptr(scores), _ptr(table_first), _ptr(ids), _ptr(in_index), _ptr(dir_id), _ptr(under),
                                  _ptr(first), len(sets), C.byref(sp), _ptr(out_ids), res, 0)
    if rc:
        return rc, None
    assert (out_ids[:front] == 0xdeadbeef).all()
    out = []
    for s in range(len(sets)):
        a, b, k = int(first[s]), int(first[s + 1]), res[s].sorted
        assert k <= b - a and (out_ids[a + k:b] == 0).all()
        out.append(([int(i) for i in out_ids[a:a + k]], res[s].queries, res[s].not_found, res[s].behind))
    return 0, out


def one(L, table, ids, in_index=None, dir_id=None, under=None, **kw):
    rc, out = device(L, [(table, ids, in_index, dir_id, under)], **kw)
    assert rc == 0
    return out[0]


def random_table(n, seed, kind="half"):
    """(table, ids): few distinct scores, so that ties fall to the id; ids shuffled, so that the selection's order is
    not the id order.  half: about half the entries match; dense: all; empty: none"""
    rng = np.random.default_rng([seed, n])
    if kind == "empty":
        t = np.full((n, n), NO_MATCH, np.uint16)
    else:
        t = rng.integers(0, 12, (n, n), dtype=np.uint16)
    if kind == "half":
        t[rng.integers(0, 2, (n, n), dtype=np.uint8) == 1] = NO_MATCH
    return t, (rng.permutation(n) + 1 + int(rng.integers(0, 1000))).astype(np.uint32)


# wave (64 lanes x 8 scores = 512 items), workgroup (1024 lanes = 8192 items) and load-width (8 scores) edges
EDGES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 2047, 2049, 4097]


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGES)
def test_table_entry_equals_the_model(lib, n):
    t, ids = random_table(n, 1)
    got = one(lib, t, ids)
    assert got == table_model(t, ids)
    if n <= 1:
        assert got == ([int(i) for i in ids], 0, 0, 0)
    if n >= 63:
        assert len(got[0]) > n // 2 and got[3] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9, 513])
def test_dense_and_empty_tables(lib, n):
    t, ids = random_table(n, 2, "dense")
    assert one(lib, t, ids) == table_model(t, ids)
    t, ids = random_table(n, 3, "empty")
    # nothing matches: the first item alone, and every query of every iteration counted in closed form
    assert one(lib, t, ids) == ([int(ids[0])], n - 1, n - 1, 0) == table_model(t, ids)


@pytest.mark.gpu
def test_second_load_of_a_lane(lib):
    """8193 items, the smallest set in which a lane of the 1024 takes a second load: an empty table but for a chain of
    30 items, the second of which has the largest id -- the one score of lane 0's second load"""
    n = 8193
    t, ids = random_table(n, 4, "empty")
    rng = np.random.default_rng(8193)
    chain = np.concatenate([[0], 1 + rng.choice(n - 1, 29, replace=False)])
    ids[ids == ids.max()], ids[chain[1]] = ids[chain[1]], ids.max()
    t[chain[:-1], chain[1:]] = np.arange(5, 5 + 29)
    got = one(lib, t, ids)
    assert got == table_model(t, ids)
    assert got[0] == [int(i) for i in ids[chain]]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 65, 700, 1025])
def test_table_entry_equals_the_hamming_entry(lib, n):
    h, ids = TS.walk(n, 500 + n)
    rng = np.random.default_rng(n)
    in_index = (rng.random(n) < 0.9).astype(np.uint8)
    thresh = 6 + n % 4
    want = TS.one(lib, h, ids, thresh, in_index=in_index)
    assert one(lib, hamming_table(h, thresh), ids, in_index=in_index) == want
    if n >= 65:
        assert 1 < len(want[0]) < n


def _rule_case(seed=7, n=48):
    """a random table whose scores mostly differ, so that a cut or a filter changes WHICH item is first"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 400, (n, n)).astype(np.uint16)
    t[rng.random((n, n)) < 0.6] = NO_MATCH
    ids = (rng.permutation(n) + 1).astype(np.uint32)
    dir_id = rng.integers(0, 3, n).astype(np.uint32)
    under = rng.integers(0, 2, n).astype(np.uint8)
    return t, ids, dir_id, under


@pytest.mark.gpu
@pytest.mark.parametrize("min_matches", [0, 1, 2, 3])
@pytest.mark.parametrize("max_matches", [1, 2, 5])
def test_min_and_max_matches(lib, min_matches, max_matches):
    t, ids, dir_id, under = _rule_case(seed=9, n=40)
    kw = dict(min_matches=min_matches, max_matches=max_matches)
    plain = one(lib, t, ids, **kw)
    assert plain == table_model(t, ids, **kw)
    if min_matches > max_matches:
        assert plain == ([int(ids[0])], 39, 39, 0)
    else:
        assert len(plain[0]) > 1
    # with a filter the cut comes first: the max_matches nearest are taken, then filtered, then counted
    got = one(lib, t, ids, dir_id=dir_id, filter_parent=True, **kw)
    assert got == table_model(t, ids, dir_id=dir_id, filter_parent=True, **kw)
    # a sparse row decides acceptance: needles with fewer than min_matches candidates fail
    sparse = t.copy()
    sparse[np.random.default_rng(1).random(t.shape) < 0.85] = NO_MATCH
    assert one(lib, sparse, ids, **kw) == table_model(sparse, ids, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["filter_parent", "path_in", "path_out", "look_behind1", "look_behind5", "look_behind8",
                                  "first_row_empty", "needle_outside", "candidate_outside"])
def test_rules_of_a_query(lib, rule):
    t, ids, dir_id, under = _rule_case()
    n = len(ids)
    kw, in_index = {}, None
    plain = table_model(t, ids)
    if rule == "filter_parent":
        kw = dict(filter_parent=True)
    elif rule == "path_in":
        kw = dict(path_mode=1)
    elif rule == "path_out":
        kw = dict(path_mode=2)
    elif rule.startswith("look_behind"):
        kw = dict(look_behind=int(rule[len("look_behind"):]))
    elif rule == "first_row_empty":
        t[0, :] = NO_MATCH
    elif rule == "needle_outside":
        in_index = np.ones(n, np.uint8)
        in_index[0] = 0  # the start is no entry of the index: it still asks, with the row the caller gives it
    elif rule == "candidate_outside":
        in_index = np.ones(n, np.uint8)
        second = list(ids).index(plain[0][1])
        in_index[second] = 0  # the item the plain chain places first is no candidate
    want = table_model(t, ids, in_index=in_index, dir_id=dir_id, under=under, **kw)
    got = one(lib, t, ids, in_index=in_index, dir_id=dir_id if kw.get("filter_parent") else None,
              under=under if kw.get("path_mode") else None, **kw)
    assert got == want
    if rule in ("filter_parent", "path_in", "path_out", "look_behind1", "look_behind8", "candidate_outside"):
        assert got != plain  # the rule decided something
    if rule == "look_behind1":
        assert got[3] == 0
    if rule == "first_row_empty":
        assert got == ([int(ids[0])], n - 1, n - 1, 0)
    if rule == "needle_outside":
        assert got == plain and len(got[0]) > 1
    if rule == "candidate_outside":
        assert int(plain[0][1]) not in got[0]


@pytest.mark.gpu
def test_ragged_batch_equals_the_single_calls(lib):
    sets = [random_table(n, 300 + k) + (None, None, None) for k, n in enumerate([0, 1, 2, 70, 1, 1025, 0, 9])]
    rc, out = device(lib, sets, front=3)
    assert rc == 0
    for s, got in zip(sets, out):
        assert got == one(lib, s[0], s[1]) == table_model(s[0], s[1])


@pytest.mark.gpu
def test_error_codes(lib):
    from cbird_amd import _lib

    t, ids = random_table(20, 1)
    zero = ids.copy()
    zero[13] = 0
    assert device(lib, [(t, zero, None, None, None)])[0] == _lib.CBH_E_INVAL
    twice = ids.copy()
    twice[13] = twice[2]
    assert device(lib, [(t, twice, None, None, None)])[0] == _lib.CBH_E_INVAL
    ok = [(t, ids, None, None, None)]
    assert device(lib, ok, look_behind=0)[0] == device(lib, ok, look_behind=9)[0] == _lib.CBH_E_INVAL
    assert device(lib, ok, max_matches=0)[0] == device(lib, ok, max_matches=56)[0] == _lib.CBH_E_INVAL
    assert device(lib, ok, filter_parent=True)[0] == device(lib, ok, path_mode=1)[0] == _lib.CBH_E_INVAL
    assert device(lib, ok, path_mode=3)[0] == _lib.CBH_E_INVAL
    assert device(lib, ok, max_matches=55, look_behind=8)[0] == 0
    assert device(lib, []) == (0, [])
    # a set above CBH_SORT_SIMILAR_MAX is refused before its table is looked at
    big = np.arange(1, _lib.CBH_SORT_SIMILAR_MAX + 2, dtype=np.uint32)
    first = np.array([0, len(big)], np.uint64)
    sp = _lib.cbh_sort_table_params(1, 5, 0, 0, 5)
    res = (_lib.cbh_sort_similar_result * 1)()
    assert lib.cbh_sort_similar_table(t.ctypes.data, np.zeros(1, np.uint64).ctypes.data, big.ctypes.data, None, None, None,
                                      first.ctypes.data, 1, C.byref(sp), big.ctypes.data, res, 0) == _lib.CBH_E_UNSUPPORTED


def _tuning(L, key):
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0
    return v.value


def _refuse_every_allocation(L, call, first):
    """the walk of tests/test_error_paths.py: every refused call returns CBH_E_NOMEM, leaves no scratch handed out, and
    the next call gives the same results.  Returns how many allocations could be refused"""
    from cbird_amd import _lib

    refused = 0
    for k in range(100):
        live0, fired0 = _tuning(L, b"arena_live_bytes"), _tuning(L, b"fault_fired")
        L.cbh_set_tuning(b"fault_alloc_after", k)
        try:
            rc, _ = call()
        finally:
            L.cbh_set_tuning(b"fault_alloc_after", -1)
        if _tuning(L, b"fault_fired") == fired0:
            assert rc == 0
            return refused
        refused += 1
        assert rc == _lib.CBH_E_NOMEM, (k, rc)
        assert _tuning(L, b"arena_live_bytes") == live0, k
        assert call() == (0, first), k
    pytest.fail("the call never ran out of allocations to refuse")


@pytest.mark.gpu
def test_every_allocation_of_the_table_entry_may_be_refused(lib):
    sets = [random_table(n, 40 + n) + (None, None, None) for n in (70, 3)]
    rc, first = device(lib, sets)
    assert rc == 0
    refused = _refuse_every_allocation(lib, lambda: device(lib, sets), first)
    # staged: scores, ids, set_first + table_first, out_ids, out; scratch: keys, values, ids, attributes, first places,
    # status, the sorted tables and where they start, and the sort's two buffers and workspace
    assert refused == 5 + 8 + 3


# ---- the colour entry ----------------------------------------------------------------------------------------------------
def colour_index(gpu, idx_d, idx_i):
    """a ColorDescIndex holding the case's entries: added with their ids, the removed ones then removed"""
    from cbird_amd.colordesc import ColorDescIndex

    idx = ColorDescIndex()
    live = idx_i != 0
    fake = idx_i.copy()
    fake[~live] = 1_000_000 + np.flatnonzero(~live)  # entries that are then removed: id 0, descriptor cleared
    filler = idx_d.copy()
    filler[~live] = CS.synth_descriptors(int((~live).sum()) + 1, 99)[0][: int((~live).sum())]
    idx.add(TR.media_of(filler, fake))
    if (~live).any():
        idx.remove(fake[~live])
    return idx


_cases = {}


def colour_case(n, seed):
    if (n, seed) not in _cases:
        media, ids, idx_d, idx_i = TR.colour_case(n, seed)
        table, in_index = TR.colour_tables(media, ids, idx_d, idx_i)
        _cases[(n, seed)] = (media, ids, idx_d, idx_i, table, in_index)
    return _cases[(n, seed)]


def _paths(n, ids, seed=3):
    rng = np.random.default_rng(seed)
    dirs, under = rng.integers(0, 3, n), rng.integers(0, 2, n).astype(np.uint8)
    paths = [f"/db/{'in' if under[k] else 'out'}/d{dirs[k]}/{int(ids[k])}.jpg" for k in range(n)]
    return paths, (dirs + 3 * under).astype(np.uint32), under


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed", [(96, 5), (300, 6)])
@pytest.mark.parametrize("kw", [dict(), dict(minMatches=2, maxMatches=2), dict(filterParent=True),
                                dict(path="in", inPath=True, maxMatches=2)])
def test_colour_entry_equals_the_model_and_the_loop(gpu, lib, n, seed, kw):
    media, ids, idx_d, idx_i, table, in_index = colour_case(n, seed)
    assert in_index.sum() < n and (idx_i == 0).any() and (media["numColors"] == 0).any()
    paths, dir_id, under = _paths(n, ids)
    p = TR.colour_params(**kw)
    mode = 0 if p.path == "" else (1 if p.inPath else 2)
    want = table_model(table, ids, p.minMatches, p.maxMatches, in_index, dir_id, under, p.filterParent, mode)
    idx = colour_index(gpu, idx_d, idx_i)
    got = idx.sort_similar(ids, media, p, dir_id=dir_id if p.filterParent else None, under=under if mode else None,
                           path_mode=mode)
    assert got == [want]
    assert len(want[0]) > (1 if mode else 3)  # (the path filter leaves the 300-item case a chain of two)
    # the index's own descriptors as needles: another table, unless no Media differs
    own = idx.sort_similar(ids, None, p, dir_id=dir_id if p.filterParent else None, under=under if mode else None,
                           path_mode=mode)
    entry_media = media.copy()
    entry_media[:] = np.zeros((), CS.COLOR_DTYPE)
    t_own, _ = TR.colour_tables(entry_media, ids, idx_d, idx_i)
    assert own == [table_model(t_own, ids, p.minMatches, p.maxMatches, in_index, dir_id, under, p.filterParent, mode)]
    # the Python entry against the loop on the same index
    sel = TR.media_of(media, ids, paths)
    o, q, nf = sort_similar(idx, sel, p, batched=True, db_path="/db")
    assert ([m.id for m in o], q, nf) == want[:3] and all(any(m is x for x in sel) for m in o)
    o, q, nf = sort_similar(idx, TR.media_of(media, ids, paths), p, batched=False, db_path="/db")
    assert ([m.id for m in o], q, nf) == want[:3]


@pytest.mark.gpu
def test_colour_batch_groups_and_chunks(gpu, lib):
    """a ragged batch in one call equals the single calls -- also when the tables go in several groups
    ("color_sort_table_kb") and are filled in several row chunks ("color_chunk_scores"); a set whose own table does not fit
    the budget is refused"""
    from cbird_amd import _lib

    media, ids, idx_d, idx_i, table, in_index = colour_case(300, 6)
    idx = colour_index(gpu, idx_d, idx_i)
    p = TR.colour_params()
    cuts = [0, 120, 120, 121, 250, 300]
    first = np.array(cuts, np.uint64)
    singles = [idx.sort_similar(ids[a:b], media[a:b], p)[0] for a, b in zip(cuts, cuts[1:])]
    for a, b, got in zip(cuts, cuts[1:], singles):
        sub = np.ix_(range(a, b), range(a, b))
        assert got == table_model(table[sub], ids[a:b], in_index=in_index[a:b])
    assert idx.sort_similar(ids, media, p, set_first=first) == singles
    assert _tuning(lib, b"color_sort_groups") == 1
    try:
        assert lib.cbh_set_tuning(b"color_sort_table_kb", 36) == 0  # 120 x 120 and 129 x 136 scores fit, each alone
        assert lib.cbh_set_tuning(b"color_chunk_scores", 50 * 129) == 0
        assert idx.sort_similar(ids, media, p, set_first=first) == singles
        assert _tuning(lib, b"color_sort_groups") >= 3
        assert lib.cbh_set_tuning(b"color_sort_table_kb", 20) == 0
        with pytest.raises(_lib.CbhError) as e:
            idx.sort_similar(ids, media, p, set_first=first)
        assert e.value.code == _lib.CBH_E_UNSUPPORTED
        assert lib.cbh_set_tuning(b"color_sort_table_kb", -1) == _lib.CBH_E_INVAL
    finally:
        lib.cbh_set_tuning(b"color_sort_table_kb", 0)
        lib.cbh_set_tuning(b"color_chunk_scores", 0)
    sels = [TR.media_of(media[a:b], ids[a:b]) for a, b in zip(cuts, cuts[1:])]
    got = sort_similar_batch(idx, sels, p)
    assert [([m.id for m in o], q, nf) for o, q, nf in got] == [s[:3] for s in singles]


@pytest.mark.gpu
def test_colour_index_holding_an_id_twice_takes_the_loop(gpu, lib):
    from cbird_amd import _lib

    media, ids, idx_d, idx_i, table, in_index = colour_case(96, 5)
    idx = colour_index(gpu, idx_d, idx_i)
    dup = int(np.flatnonzero(in_index)[5])
    idx.add(TR.media_of(media[dup:dup + 1], ids[dup:dup + 1]))
    p = TR.colour_params()
    with pytest.raises(_lib.CbhError) as e:
        idx.sort_similar(ids, media, p)
    assert e.value.code == _lib.CBH_E_UNSUPPORTED
    o, q, nf = sort_similar(idx, TR.media_of(media, ids), p, batched=True)
    o2, q2, nf2 = sort_similar(idx, TR.media_of(media, ids), p, batched=False)
    assert ([m.id for m in o], q, nf) == ([m.id for m in o2], q2, nf2) and len(o) > 1


@pytest.mark.gpu
def test_colour_error_codes(gpu, lib):
    from cbird_amd import _lib

    media, ids, idx_d, idx_i, table, in_index = colour_case(96, 5)
    idx = colour_index(gpu, idx_d, idx_i)

    def code(ids_, **kw):
        try:
            idx.sort_similar(ids_, None, TR.colour_params(**kw.pop("params", {})), **kw)
        except _lib.CbhError as e:
            return e.code
        return 0

    zero, twice = ids.copy(), ids.copy()
    zero[13], twice[13] = 0, twice[2]
    assert code(zero) == code(twice) == _lib.CBH_E_INVAL
    assert code(ids, look_behind=0) == code(ids, look_behind=9) == _lib.CBH_E_INVAL
    assert code(ids, params=dict(maxMatches=0)) == code(ids, params=dict(maxMatches=56)) == _lib.CBH_E_INVAL
    assert code(ids, params=dict(filterParent=True)) == code(ids, path_mode=1) == _lib.CBH_E_INVAL
    assert code(ids, params=dict(maxMatches=55), look_behind=8) == 0
    big = np.arange(1, _lib.CBH_COLOR_SORT_SIMILAR_MAX + 2, dtype=np.uint32)
    assert code(big) == _lib.CBH_E_UNSUPPORTED
    assert idx.sort_similar(ids[:0], None, TR.colour_params()) == [([], 0, 0, 0)]
    assert idx.sort_similar(ids[:1], None, TR.colour_params()) == [([int(ids[0])], 0, 0, 0)]
    # an empty index: nothing is a candidate
    from cbird_amd.colordesc import ColorDescIndex

    assert ColorDescIndex().sort_similar(ids, media, TR.colour_params()) == [([int(ids[0])], 95, 95, 0)]
    # the Python entry leaves reflections, the template matcher and other algorithms to the loop
    from cbird_amd import SearchParams
    from cbird_amd.database import _sort_similar_on_device

    assert _sort_similar_on_device(idx, TR.colour_params()) is True
    assert _sort_similar_on_device(idx, TR.colour_params(mirrorMask=1)) is False
    assert _sort_similar_on_device(idx, TR.colour_params(maxMatches=56)) is False
    assert _sort_similar_on_device(idx, SearchParams()) is False


@pytest.mark.gpu
def test_every_allocation_of_the_colour_entry_may_be_refused(gpu, lib):
    from cbird_amd import _lib

    media, ids, idx_d, idx_i, table, in_index = colour_case(96, 5)
    idx = colour_index(gpu, idx_d, idx_i)
    first = np.array([0, 60, 63, 96], np.uint64)
    p = TR.colour_params(filterParent=True)
    _, dir_id, _ = _paths(96, ids)

    def call():
        try:
            return 0, idx.sort_similar(ids, media, p, set_first=first, dir_id=dir_id)
        except _lib.CbhError as e:
            return e.code, None

    idx.sort_similar(ids, media, p, set_first=first, dir_id=dir_id)  # (the index's stream exists from here on)
    rc, want = call()
    assert rc == 0
    refused = _refuse_every_allocation(lib, call, want)
    # ids, attributes, dir ids, first places, set_first, table firsts, index positions, needles, out_ids, out; per group
    # the tables, three planes, colour counts, ids, scores
    assert refused == 10 + 7


@pytest.mark.gpu
def test_dropin_runs_on_gpu(gpu, tmp_path):
    cases = [colour_case(96, 5), colour_case(300, 6)]
    path = tmp_path / "sets.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for media, ids, idx_d, idx_i, _, _ in cases:
            live = idx_i != 0  # (the drop-in adds the live entries only: a removed entry is no candidate either way)
            f.write(np.array([int(live.sum()), len(ids)], np.int32).tobytes())
            for d, i in zip(idx_d[live], idx_i[live]):
                f.write(np.uint32(i).tobytes() + d.tobytes())
            for d, i in zip(media, ids):
                f.write(np.uint32(i).tobytes() + d.tobytes())
    cxx = os.environ.get("CXX", "g++")  # the rules of tests/cpp/Makefile for one more program
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbird_amd", "cpp"), "-I" + os.path.join(CPP, "mock"), "-o", EXE,
                           os.path.join(CPP, "test_sort_similar_color.cpp"), "-L" + os.path.join(ROOT, "cbird_amd"),
                           "-lcbird_hip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "cbird_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    for c, (media, ids, idx_d, idx_i, table, in_index) in enumerate(cases):
        order, queries, not_found, _ = table_model(table, ids, in_index=in_index)
        assert lines[c] == f"case {c} {queries} {not_found} : " + " ".join(str(i) for i in order)


@pytest.mark.gpu
def test_residency_4097_items_through_the_colour_entry(gpu, lib):
    """the largest size that stays within a few seconds: the colour entry against the table entry fed with
    cbh_color_distances of the same descriptors, cast to int -- GPU against GPU, so 64 random rows of that table are also
    held against np_scores.  Colour counts 20..24: most pairs are finite, the chain runs to the end"""
    from cbird_amd.colordesc import ColorDescIndex

    n = 4097
    rng = np.random.default_rng(4097)
    d = np.zeros(n, CS.COLOR_DTYPE)
    d["colors"] = rng.integers(0, 65536, (n, CS.NC, 4))
    d["numColors"] = rng.integers(20, 25, n)
    d["numColors"][rng.random(n) < 0.02] = 0
    d["numColors"][0] = 22
    ids = (rng.permutation(n) + 1).astype(np.uint32)
    order = rng.permutation(n)
    idx = ColorDescIndex()
    idx.add(TR.media_of(d[order], ids[order]))
    dist = idx.distances(d)                      # [needle, entry in add order]
    back = np.empty(n, np.int64)
    back[order] = np.arange(n)
    dist = dist[:, back]                         # columns in selection order
    table = np.where(dist < CS.FLT_MAX, np.where(dist < CS.FLT_MAX, dist, 0).astype(np.int64), NO_MATCH).astype(np.uint16)
    rows = rng.choice(n, 64, replace=False)
    want_rows = CS.int_scores(CS.np_scores(d[rows], d))
    assert (np.where(want_rows < 0, NO_MATCH, want_rows) == table[rows]).all()
    p = TR.colour_params()
    got = idx.sort_similar(ids, d, p)[0]
    assert got == one(lib, table, ids)
    assert len(got[0]) > n // 2 and got[3] > 0
