"""The colour search on the device (cbird_amd/csrc/color.hip, cbh_color_search_index_batch) against
tests/color_search_cases.py: scores on integer boundaries from both distance kernels, waves that leave the colour loop
early, every route of cbh_color_find_batch's cut ("color_full_sorts" / "color_window_cuts" say which one a needle took),
the later chunks of the needle loops ("color_chunk_scores"), cbh_color_find_all_batch's contract, searchIndex's whole-list
branch, and what "color_fma" 1 promises.  Every comparison is exact, except under "color_fma" 1.

k_color_dist2 (what find, find_batch and find_all_batch run) hands out int scores only, and only for entries whose id is
not 0; k_color_dist3 (distances()) hands out the floats of every entry."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import color_search_cases as CS

pytestmark = pytest.mark.gpu

MATCH = np.dtype([("id", np.uint32), ("score", np.int32)])
SENTINEL = np.array((0xFFFFFFFF, -7), MATCH)


@pytest.fixture(scope="module")
def co():
    from oracle import ColorOracle

    return ColorOracle()


def _L():
    from cbird_amd import _lib

    return _lib.lib()


def _tuning(key):
    v = C.c_longlong(-2)
    assert _L().cbh_get_tuning(key, C.byref(v)) == 0, key
    return int(v.value)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def make_index(descs, ids, parts=1, remove=()):
    """a ColorDescIndex holding (ids[i], descs[i]) in that order, added in `parts` calls (ids may be 0)"""
    from cbird_amd import _lib
    from cbird_amd.colordesc import ColorDescIndex

    idx = ColorDescIndex()
    descs = np.ascontiguousarray(descs, CS.COLOR_DTYPE)
    ids = np.ascontiguousarray(ids, np.uint32)
    cuts = [len(ids) * p // parts for p in range(parts + 1)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        _lib.check(_L().cbh_color_add(idx.handle, ids[a:b].ctypes.data, descs[a:b].ctypes.data, b - a), "add")
    assert idx.count() == len(ids)
    if len(remove):
        idx.remove(remove)
    return idx


def find_all(idx, needles, cap=None, sentinel_tail=0):
    """cbh_color_find_all_batch -> (rc, matches MATCH[cap + sentinel_tail], offsets u64[nq + 1]); cap None: enough"""
    needles = np.ascontiguousarray(needles, CS.COLOR_DTYPE).reshape(-1)
    nq = len(needles)
    if cap is None:
        cap = nq * idx.count()
    out = np.full(cap + sentinel_tail, SENTINEL, MATCH)
    off = np.full(nq + 1, 12345, np.uint64)
    rc = _L().cbh_color_find_all_batch(idx.handle, needles.ctypes.data, nq, out.ctypes.data if len(out) else None, cap,
                                       off.ctypes.data)
    return rc, out, off


def find_one(idx, needle):
    """cbh_color_find -> MATCH[count]"""
    needle = np.ascontiguousarray(needle, CS.COLOR_DTYPE).reshape(1)
    cap = max(1, idx.count())
    out = np.full(cap, SENTINEL, MATCH)
    n = C.c_size_t(99)
    assert _L().cbh_color_find(idx.handle, needle.ctypes.data, out.ctypes.data, cap, C.byref(n)) == 0
    return out[: n.value]


def expected_matches(scores, ids):
    """what find() reports for every needle, concatenated, and the offsets: entries with a finite score and id != 0 in
    index order, int(score)"""
    s = CS.int_scores(scores)
    ids = np.asarray(ids, np.uint32)
    keep = (s >= 0) & (ids != 0)[None, :]
    out = np.zeros(int(keep.sum()), MATCH)
    q, i = np.nonzero(keep)
    out["id"], out["score"] = ids[i], s[q, i]
    off = np.zeros(s.shape[0] + 1, np.uint64)
    np.cumsum(keep.sum(axis=1), out=off[1:])
    return out, off


def check_three_ways(idx, needles, descs, ids, ref=None):
    """the three comparisons: k_color_dist2's ints (through find_all_batch, i.e. every entry whose id is not 0) against
    int(np_scores); k_color_dist3's floats against np_scores bit for bit; and int() of those floats against the dist2
    ints.  Returns the reference scores."""
    ref = CS.np_scores(needles, descs) if ref is None else ref
    want, want_off = expected_matches(ref, ids)
    rc, got, off = find_all(idx, needles)
    assert rc == 0 and (off == want_off).all()
    got = got[: int(off[-1])]
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (len(bad), got[bad[:5]], want[bad[:5]])
    fl = idx.distances(needles)
    assert fl.shape == ref.shape
    diff = np.argwhere(_bits(fl) != _bits(ref))
    assert not len(diff), (len(diff), [(q, i, fl[q, i], ref[q, i]) for q, i in diff[:5]])
    from_floats, _ = expected_matches(fl, ids)
    assert (from_floats == got).all()
    return ref


# ---- scores on boundaries ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def boundary_set(which):
    """(needles, descs, ids, np_scores) -- the reference is computed once and shared with the "color_fma" test"""
    nd, ds = {"single": CS.boundary_pairs, "multi": CS.boundary_pairs_multi,
              "multi_mirrored": lambda: CS.boundary_pairs_multi(mirrored=True)}[which]()
    ref = CS.np_scores(nd, ds)
    ref.setflags(write=False)
    return nd, ds, np.arange(1, len(ds) + 1, dtype=np.uint32), ref


@pytest.mark.parametrize("which", ["single", "multi", "multi_mirrored"])
def test_scores_on_integer_boundaries(gpu, co, which):
    """every needle of a boundary set against every entry of it: pair i (on the diagonal) scores an integer or one ulp
    less, where a contracted or reordered sum of squares moves int(score) -- tests/test_color_search_model.py counts how
    many.  "multi": the needle side sums (rowmin / rowacc); "multi_mirrored": the entry side (colmin / colacc)."""
    nd, ds, ids, ref = boundary_set(which)
    idx = make_index(ds, ids)
    check_three_ways(idx, nd, ds, ids, ref)
    # and through cbh_color_find, needle by needle, against the C oracle's find()
    s = CS.int_scores(ref)
    for q in range(0, len(nd), 7):
        got = find_one(idx, nd[q])
        wi, ws = co.find(ds, ids, nd[q])
        assert (got["id"] == wi).all() and (got["score"] == ws).all()
        assert got["score"][np.nonzero(got["id"] == ids[q])[0][0]] == s[q, q]


# ---- wave shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", CS.WAVE_SIZES)
def test_wave_shapes(gpu, n):
    """colour counts in runs: whole waves of k_color_dist3 (64 entries) and k_color_dist2 (128) whose largest count is 1,
    2, 3, 15, 16, 17, 31 or 32 leave the colour loop there (`__ballot(h < hn) == 0`), with run boundaries off the wave
    boundaries, grayscale and removed entries inside, needles on both sides of the swap, at sizes around the 256- and
    512-entry tiles.  Loaded in two add() calls; then again through a slice whose planes fit exactly, so that the second
    add() has to regrow them (below 4096 entries add() alone never does); after remove(); on a slice() of every third id."""
    descs, ids, needles, removable = CS.wave_shape_index(5, n)
    idx = make_index(descs, ids, parts=2)
    ref = check_three_ways(idx, needles, descs, ids)
    if n >= 2:
        half = n // 2
        first = make_index(descs[:half], ids[:half])
        grown = first.slice(np.unique(ids[:half]))      # (0 listed: the zeroed entries stay)
        assert grown.count() == half
        from cbird_amd import _lib
        _lib.check(_L().cbh_color_add(grown.handle, ids[half:].ctypes.data, descs[half:].ctypes.data, n - half), "add")
        check_three_ways(grown, needles, descs, ids, ref)
    if len(removable):
        idx.remove(removable)
        d2, i2 = CS.removed(descs, ids, removable)
        assert (i2 == 0).sum() == (ids == 0).sum() + len(removable)
        check_three_ways(idx, needles, d2, i2)
    else:
        d2, i2 = descs, ids
    third = np.unique(i2[i2 != 0])[::3]
    sub = idx.slice(third)
    keep = np.isin(i2, third)
    assert sub.count() == keep.sum()
    if keep.any():
        check_three_ways(sub, needles, d2[keep], i2[keep])


# ---- cut paths -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def select_ref(name):
    """(case, descs, ids, np_scores) of a select case as its index stands after case.remove"""
    case = CS.select_cases()[name]
    d, ids = CS.case_index(case)
    ref = CS.np_scores(case.needles, d)
    ref.setflags(write=False)
    return case, d, ids, ref


def run_find_batch(idx, case):
    """find_batch with the counters' deltas: (ids, scores, counts, full sorts, window cuts)"""
    f0, w0 = _tuning(b"color_full_sorts"), _tuning(b"color_window_cuts")
    gi, gs, gc = idx.find_batch(case.needles, case.k)
    return gi, gs, gc, _tuning(b"color_full_sorts") - f0, _tuning(b"color_window_cuts") - w0


def check_cut(got, ref, ids, k):
    gi, gs, gc, full, window = got
    wi, ws, wc = CS.reference_cut(ref, ids, k)
    assert (gc == wc).all(), (gc, wc)
    assert (gi == wi).all() and (gs == ws).all(), np.argwhere((gi != wi) | (gs != ws))[:5]
    assert (full, window) == CS.predicted_counters(ref, ids, k)


@pytest.mark.parametrize("name", CS.SELECT_NAMES)
def test_select_case(gpu, name):
    """cbh_color_find_batch against reference_cut -- ids, scores and counts -- and the route every needle took against the
    routing rule restated in the helper"""
    case, d, ids, ref = select_ref(name)
    idx = make_index(case.descs, case.ids, remove=case.remove)
    check_cut(run_find_batch(idx, case), ref, ids, case.k)


# ---- chunks ----------------------------------------------------------------------------------------------------------------
def test_needle_chunks(gpu):
    """"color_chunk_scores" at three needles per chunk: 8 needles go in chunks of 3, 3, 2, and the two that take the full
    sort are the second of the second chunk and the second of the third (color_full_sort_one's q_in_chunk).  find_batch,
    find_all_batch and distances answer as with the default chunk size, and as the reference."""
    case, d, ids, ref = select_ref("chunks8")
    assert CS.route(ref, ids, case.k) == ["window"] * 4 + ["full", "window", "window", "full"]
    idx = make_index(case.descs, case.ids, remove=case.remove)
    L = _L()
    assert _tuning(b"color_chunk_scores") == 0
    whole = run_find_batch(idx, case)
    whole_all = find_all(idx, case.needles)
    whole_fl = idx.distances(case.needles)
    try:
        assert L.cbh_set_tuning(b"color_chunk_scores", 3 * len(ids)) == 0
        assert _tuning(b"color_chunk_scores") == 3 * len(ids)
        parts = run_find_batch(idx, case)
        parts_all = find_all(idx, case.needles)
        parts_fl = idx.distances(case.needles)
        # one needle per chunk: a budget below one row of scores still takes a needle at a time
        assert L.cbh_set_tuning(b"color_chunk_scores", 1) == 0
        ones = run_find_batch(idx, case)
    finally:
        assert L.cbh_set_tuning(b"color_chunk_scores", 0) == 0
    for got in (whole, parts, ones):
        check_cut(got, ref, ids, case.k)
    want, want_off = expected_matches(ref, ids)
    for rc, out, off in (whole_all, parts_all):
        assert rc == 0 and (off == want_off).all() and (out[: len(want)] == want).all()
    assert (_bits(whole_fl) == _bits(ref)).all() and (_bits(parts_fl) == _bits(ref)).all()


# ---- find_all_batch --------------------------------------------------------------------------------------------------------
def test_find_all_batch_contract(gpu):
    from cbird_amd import _lib
    from cbird_amd.colordesc import ColorDescIndex

    descs, ids, needles, _ = CS.wave_shape_index(5, 513)
    idx = make_index(descs, ids)
    L, h, nq = _L(), idx.handle, len(needles)
    zero = int(np.nonzero(needles["numColors"] == 0)[0][0])
    needles = np.r_[needles[1:4], needles[zero: zero + 1], needles[4:]]   # the colourless needle inside the batch
    rc, out, off = find_all(idx, needles, sentinel_tail=8)
    total = int(off[-1])
    assert rc == 0 and off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all() and total > 1000
    assert off[3] == off[4] and (out[total:] == SENTINEL).all()
    for q in range(nq):                                  # each range is cbh_color_find of that needle
        assert (out[int(off[q]): int(off[q + 1])] == find_one(idx, needles[q])).all(), q
    want, want_off = expected_matches(CS.np_scores(needles, descs), ids)
    assert (off == want_off).all() and (out[:total] == want).all()
    # one place too few: CBH_E_OVERFLOW, the offsets complete, nothing written past cap
    rc, short, off2 = find_all(idx, needles, cap=total - 1, sentinel_tail=8)
    assert rc == _lib.CBH_E_OVERFLOW and (off2 == off).all()
    assert (short[: total - 1] == out[: total - 1]).all() and (short[total - 1:] == SENTINEL).all()
    # no buffer at all: the offsets alone
    off3 = np.full(nq + 1, 12345, np.uint64)
    assert L.cbh_color_find_all_batch(h, needles.ctypes.data, nq, None, 0, off3.ctypes.data) == _lib.CBH_E_OVERFLOW
    assert (off3 == off).all()
    # an exact fit
    rc, fit, off4 = find_all(idx, needles, cap=total, sentinel_tail=8)
    assert rc == 0 and (fit[:total] == out[:total]).all() and (fit[total:] == SENTINEL).all()
    # no needles; an empty index
    off5 = np.full(1, 12345, np.uint64)
    assert L.cbh_color_find_all_batch(h, None, 0, None, 0, off5.ctypes.data) == 0 and off5[0] == 0
    empty = ColorDescIndex()
    rc, none, off6 = find_all(empty, needles, cap=4, sentinel_tail=0)
    assert rc == 0 and (off6 == 0).all() and (none == SENTINEL).all()
    # bad arguments
    buf = np.full(4, SENTINEL, MATCH)
    E = _lib.CBH_E_INVAL
    assert L.cbh_color_find_all_batch(None, needles.ctypes.data, nq, buf.ctypes.data, 4, off3.ctypes.data) == E
    assert L.cbh_color_find_all_batch(h, needles.ctypes.data, nq, buf.ctypes.data, 4, None) == E
    assert L.cbh_color_find_all_batch(h, None, nq, buf.ctypes.data, 4, off3.ctypes.data) == E
    assert L.cbh_color_find_all_batch(h, needles.ctypes.data, nq, None, 4, off3.ctypes.data) == E
    assert (buf == SENTINEL).all()


# ---- searchIndex's whole-list branch ---------------------------------------------------------------------------------------
class _M:
    def __init__(self, id_, desc):
        self.id, self.colorDescriptor, self.path, self.score, self.matchRange = int(id_), desc, f"m{id_}", -1, None

    def isValid(self):
        return self.id != 0


@pytest.mark.parametrize("filter_self", [False, True])
def test_search_index_takes_the_whole_list_when_the_fetched_places_run_out(gpu, filter_self):
    """cbh_color_search_index_batch fetches maxMatches + 9 places per needle and falls back to the needle's whole list
    when fewer than maxMatches of them are usable.  The idMap lacks the 30 best ids of needles 2 and 5, so none of their
    fetched places is; others have enough and take the short way."""
    from cbird_amd import SearchParams
    from cbird_amd.database import search_index, search_index_batch

    mm = 5
    d, ids = CS.synth_descriptors(600, 11)
    ref = CS.np_scores(d, d)
    s = CS.int_scores(ref)
    counts = (s >= 0).sum(axis=1)
    chosen = [int(q) for q in np.nonzero(counts > 80)[0][:8]]
    assert len(chosen) == 8
    missing = set()
    for q in (chosen[2], chosen[5]):
        v = np.nonzero(s[q] >= 0)[0]
        order = v[np.lexsort((ids[v], s[q, v]))]
        missing |= {int(ids[i]) for i in order[:30]}
    id_map = {int(i): _M(i, x) for i, x in zip(ids, d) if int(i) not in missing}
    needles = [_M(ids[q], d[q]) for q in chosen]

    def expect(q):
        v = np.nonzero(s[q] >= 0)[0]
        order = v[np.lexsort((ids[v], s[q, v]))]
        ranked = [(int(ids[i]), int(s[q, i])) for i in order]
        usable = [(i, sc) for i, sc in ranked if not (filter_self and i == int(ids[q])) and i in id_map]
        return ranked, usable[:mm]

    # the branch is taken for the two (near-duplicate palettes share neighbours: for some others as well), not for all
    usable_first = {}
    for q in chosen:
        ranked, _ = expect(q)
        assert len(ranked) > mm + 9
        usable_first[q] = sum(1 for i, _ in ranked[: mm + 9] if not (filter_self and i == int(ids[q])) and i in id_map)
    assert usable_first[chosen[2]] == 0 and usable_first[chosen[5]] == 0
    assert sum(u >= mm for u in usable_first.values()) >= 2 and sum(u < mm for u in usable_first.values()) >= 2
    idx = make_index(d, ids)
    p = SearchParams(algo=SearchParams.AlgoColor, filterSelf=filter_self, maxMatches=mm)
    got = search_index_batch(idx, needles, p, id_map)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "no media with id"
        want = [search_index(idx, m, p, id_map) for m in needles]
    assert [[(x.id, x.score) for x in g] for g in got] == [[(x.id, x.score) for x in g] for g in want]
    assert [[(x.id, x.score) for x in g] for g in got] == [expect(q)[1] for q in chosen]
    assert all(len(g) == mm for g in got)


# ---- "color_fma" 1 ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_set():
    d, ids = CS.synth_descriptors(700, 5)
    nd = d[::41]
    ref = CS.np_scores(nd, d)
    ref.setflags(write=False)
    return nd, d, ids, ref


@pytest.mark.parametrize("which", ["single", "multi", "multi_mirrored", "random"])
def test_color_fma_keeps_its_stated_contract(gpu, which):
    """"color_fma" 1 (k_color_dist3 with fused squares, never the default): distances within 1e-5 relative of the
    reference's -- DESIGN.md's bound; the fused sum of squares is off by at most one rounding of each product, a few
    float32 ulps (6e-8 each) on the score --, FLT_MAX exactly where the reference has it, int scores within one.  Back at
    0 everything is bit-exact again."""
    nd, ds, ids, ref = random_set() if which == "random" else boundary_set(which)
    idx = make_index(ds, ids)
    L = _L()
    want, want_off = expected_matches(ref, ids)
    try:
        assert L.cbh_set_tuning(b"color_fma", 1) == 0
        fl = idx.distances(nd)
        rc, got, off = find_all(idx, nd)
        one = find_one(idx, nd[1])
    finally:
        assert L.cbh_set_tuning(b"color_fma", 0) == 0
    fin = ref < CS.FLT_MAX
    assert fin.any() and (_bits(fl[~fin]) == _bits(CS.FLT_MAX)).all() and (fl[fin] < CS.FLT_MAX).all()
    rel = np.abs(fl[fin].astype(np.float64) - ref[fin]) / ref[fin]
    assert rel.max() <= 1e-5, rel.max()
    assert rc == 0 and (off == want_off).all()
    got = got[: len(want)]
    assert (got["id"] == want["id"]).all()
    assert np.abs(got["score"].astype(np.int64) - want["score"]).max() <= 1
    assert (one == got[int(off[1]): int(off[2])]).all()
    check_three_ways(idx, nd, ds, ids, ref)   # the knob is back at 0: bit for bit
