"""tests/color_search_cases.py on the CPU: its float32 restatement of ColorDescriptor::distance against the C oracle bit
for bit, every case builder against the conditions it states, and the case sets against mutants -- a set that a fused or
reordered sum of squares, a dropped count rule or swapped sides cannot change would prove nothing on the GPU."""
import numpy as np
import pytest

import color_search_cases as CS
from color_search_cases import synth_descriptors


@pytest.fixture(scope="module")
def co():
    from oracle import ColorOracle

    return ColorOracle()


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_dtype_is_the_products():
    from cbird_amd.colordesc import COLOR_DTYPE

    assert CS.COLOR_DTYPE == COLOR_DTYPE and CS.COLOR_DTYPE.itemsize == 258


@pytest.mark.parametrize("which", ["single", "multi", "multi_mirrored"])
def test_np_scores_is_the_oracle_on_boundary_pairs(co, which):
    nd, ds = {"single": CS.boundary_pairs, "multi": CS.boundary_pairs_multi,
              "multi_mirrored": lambda: CS.boundary_pairs_multi(mirrored=True)}[which]()
    got = CS.diagonal(CS.np_scores(nd, ds))
    want = np.array([co.distance(a, b) for a, b in zip(nd, ds)], np.float32)
    assert (_bits(got) == _bits(want)).all()
    # off the diagonal too: a row and a column of the matrix the GPU tests compare
    row = np.array([co.distance(nd[3], b) for b in ds], np.float32)
    colm = np.array([co.distance(a, ds[5]) for a in nd], np.float32)
    full = CS.np_scores(nd, ds)
    assert (_bits(full[3]) == _bits(row)).all() and (_bits(full[:, 5]) == _bits(colm)).all()


def test_np_scores_is_the_oracle_on_random_pairs(co):
    d, _ = synth_descriptors(300, 1)
    rng = np.random.default_rng(2)
    i, j = rng.integers(0, 300, (2, 2000))
    full = CS.np_scores(d, d)
    want = np.array([co.distance(d[a], d[b]) for a, b in zip(i, j)], np.float32)
    assert (_bits(full[i, j]) == _bits(want)).all()
    assert 100 < (want < CS.FLT_MAX).sum() < 1900  # both outcomes
    # and find(): ids, int scores, index order
    ids = np.arange(1, 301, dtype=np.uint32)
    ids[::17] = 0
    for q in (0, 7, 150):
        wi, ws = co.find(d, ids, d[q])
        s = CS.int_scores(full[q])
        keep = (s >= 0) & (ids != 0)
        assert ids[keep].tolist() == wi.tolist() and s[keep].tolist() == ws.tolist()


def test_boundary_pairs_meet_their_conditions():
    nd, ds = CS.boundary_pairs()
    assert len(nd) == len(ds) >= 300
    assert (nd["numColors"] == 1).all() and (ds["numColors"] == 1).all()
    s = CS.diagonal(CS.np_scores(nd, ds))
    up = np.nextafter(s, np.float32(np.inf))
    assert ((s == np.floor(s)) | (up == np.floor(up))).all()
    assert (s == np.floor(s)).sum() >= 100 and (up == np.floor(up)).sum() >= 100  # both kinds
    # sensitivity: either mutant moves int scores (the counts the seed gives are in the helper's docstring)
    assert CS.flips(nd, ds, CS.np_scores_fused) >= 10
    assert CS.flips(nd, ds, CS.np_scores_reordered) >= 10
    assert (len(nd), CS.flips(nd, ds, CS.np_scores_fused), CS.flips(nd, ds, CS.np_scores_reordered)) == (469, 31, 22)


@pytest.mark.parametrize("mirrored", [False, True])
def test_boundary_pairs_multi_meet_their_conditions(mirrored):
    nd, ds = CS.boundary_pairs_multi(mirrored=mirrored)
    assert len(nd) == len(ds) >= 80
    assert (nd["numColors"] == (7 if mirrored else 8)).all() and (ds["numColors"] == (8 if mirrored else 7)).all()
    s = CS.diagonal(CS.np_scores(nd, ds))
    up = np.nextafter(s, np.float32(np.inf))
    assert ((s == np.floor(s)) | (up == np.floor(up))).all()
    assert CS.flips(nd, ds, CS.np_scores_fused) >= 3
    assert CS.flips(nd, ds, CS.np_scores_reordered) >= 3
    assert (len(nd), CS.flips(nd, ds, CS.np_scores_fused), CS.flips(nd, ds, CS.np_scores_reordered)) == (105, 10, 9)
    # the two orientations are the same pairs, and the sum runs over the 8-colour side in both
    a, b = CS.boundary_pairs_multi(mirrored=not mirrored)
    assert (_bits(CS.diagonal(CS.np_scores(a, b))) == _bits(s)).all()
    swapped = CS.diagonal(CS._scores(nd, ds, swap_sides=True))
    assert (CS.int_scores(swapped) != CS.int_scores(s)).sum() > len(nd) // 2


@pytest.mark.parametrize("n", CS.WAVE_SIZES)
def test_wave_shape_index_meets_its_conditions(n):
    d, ids, needles, removable = CS.wave_shape_index(5, n)
    num = d["numColors"].astype(int)
    c = CS.wave_runs(n)
    assert len(d) == len(ids) == n and (num <= c).all()
    # every whole wave of either kernel (64 entries; 128 = 64 lanes x 2 entries) has exactly its run's count as maximum
    for w in (64, 128):
        for j in range(n // w):
            assert num[w * j: w * (j + 1)].max() == c[w * (j + 1) - 1], (w, j)
    starts = np.nonzero(np.r_[False, c[1:] != c[:-1]])[0]
    assert all(s % 64 for s in starts) and len(starts) == (n - 1) // CS.RUN
    if n >= 255:
        assert ((num == 0) & (ids != 0)).sum() >= 5            # grayscale entries
        gone = ids == 0
        assert gone.sum() >= 5 and (num[gone] == 0).all() and not d["colors"][gone].any()   # as remove() leaves them
        assert len(removable) >= 10 and np.isin(removable, ids).all() and (removable != 0).all()
    nn = set(needles["numColors"].tolist())
    assert 0 in nn
    for cc in set(c.tolist()):
        assert {k for k in range(cc - 3, cc + 4) if 1 <= k <= 32} <= nn
    if n == 1025:
        assert set(c.tolist()) == set(CS.WAVE_COLOURS)
        # every wave maximum occurs for both kernels
        assert {int(num[64 * j: 64 * j + 64].max()) for j in range(16)} == set(CS.WAVE_COLOURS)
        assert {int(num[128 * j: 128 * j + 128].max()) for j in range(8)} == set(CS.WAVE_COLOURS)
    if n >= 255:
        # sensitivity: without the count rule, and with the sides swapped, results change
        ref = CS.np_scores(needles, d)
        assert (_bits(CS._scores(needles, d, count_rule=False)) != _bits(ref)).sum() > n
        assert (CS.int_scores(CS._scores(needles, d, swap_sides=True)) != CS.int_scores(ref)).sum() > n // 4
        fin = ref < CS.FLT_MAX
        diff = np.abs(needles["numColors"].astype(int)[:, None] - num[None, :])
        assert (fin == ((diff <= 2) & (num[None, :] > 0) & (needles["numColors"][:, None] > 0))).all()
        assert (fin & (diff == 2)).any() and (~fin & (diff == 3) & (num[None, :] > 0)).any()


def test_wave_sizes_together_cover_every_colour_count():
    assert {int(x) for n in CS.WAVE_SIZES[2:-1] for x in CS.wave_runs(n)} >= {1, 2, 3, 15, 16, 17, 31}


def _case_scores(case):
    d, ids = CS.case_index(case)
    return d, ids, CS.np_scores(case.needles, d)


def _valid_sorted(scores, ids, q=0):
    s = CS.int_scores(scores)[q]
    return np.sort(s[(s >= 0) & (ids != 0)])


def test_select_cases_are_all_there_and_routed_as_named():
    cases = CS.select_cases()
    assert tuple(cases) == CS.SELECT_NAMES
    assert set(cases) >= {"typical", "kth_last_bin", "kth_outside_window", "kth_outside_many", "fewer_valid_than_k",
                          "ties_4096", "ties_4097", "k0", "k1", "k4096", "k4097", "k_gt_n", "min_has_id0",
                          "zero_needle_between", "nq65", "chunks8"}
    assert {len(c.needles) for c in cases.values()} >= {1, 65}
    assert {c.k for c in cases.values()} >= {0, 1, 4096, 4097}
    for c in cases.values():
        d, ids, sc = _case_scores(c)
        assert len(ids) <= 9000 and len(d) == len(ids)
        r = CS.route(sc, ids, c.k)
        assert r[0] == c.expect_path, c.name
        assert CS.predicted_counters(sc, ids, c.k) == (r.count("full"), r.count("window"))


def test_select_cases_sit_where_their_names_say():
    cases = CS.select_cases()
    W, CAP = CS.WIN, CS.CAND_CAP

    def v(name):
        c = cases[name]
        d, ids, sc = _case_scores(c)
        return c, ids, sc, _valid_sorted(sc, ids)

    c, ids, sc, s = v("typical")
    assert len(s) == 3000 and s[c.k - 1] - s[0] < 100
    c, ids, sc, s = v("kth_last_bin")
    assert s[c.k - 1] == s[0] + W - 1 and s[c.k] > s[c.k - 1]
    c, ids, sc, s = v("kth_outside_window")
    assert s[c.k - 1] == s[0] + W and s[c.k - 2] < s[0] + W and len(s) <= CAP
    c, ids, sc, s = v("kth_outside_many")
    assert s[c.k - 1] == s[0] + W and len(s) > CAP
    c, ids, sc, s = v("fewer_valid_than_k")
    assert 0 < len(s) < c.k and len(ids) > c.k
    for name, ties in (("ties_4096", CAP), ("ties_4097", CAP + 1)):
        c, ids, sc, s = v(name)
        assert (s <= s[c.k - 1]).sum() == ties and len(s) > ties and s[c.k - 1] - s[0] < W
    for k in (0, 1, CAP, CAP + 1):
        c, ids, sc, s = v(f"k{k}")
        assert c.k == k and len(s) == 5000 > CAP + 1
    c, ids, sc, s = v("k4096")
    assert (s <= s[CAP - 1]).sum() == CAP and s[CAP - 1] - s[0] < W
    c, ids, sc, s = v("k_gt_n")
    assert c.k > len(ids) == len(s)
    # the id-0 entry and the removed one are the two lowest of the index as loaded, and counting either into the
    # minimum would change the route
    c = cases["min_has_id0"]
    raw = CS.int_scores(CS.np_scores(c.needles, c.descs))[0]
    lowest = np.argsort(raw, kind="stable")[:2]
    assert sorted([int(c.ids[lowest[0]]), int(c.ids[lowest[1]])]) == [0, int(c.remove[0])]
    d, ids, sc = _case_scores(c)
    s = _valid_sorted(sc, ids)
    assert s[c.k - 1] == s[0] + W - 1 and len(s) > CAP
    assert CS.route(sc, ids, c.k) == ["window"]
    low = int(raw[raw >= 0].min())                          # the minimum, if the id test were forgotten
    assert c.ids[lowest[0]] == 0 and s[c.k - 1] - low >= W  # ... the k-th outside its window: everything, the full sort
    assert c.ids[lowest[1]] == c.remove[0] and s[c.k - 1] - int(raw[lowest[1]]) >= W   # the same for the removed one
    c = cases["zero_needle_between"]
    assert c.needles["numColors"].tolist() == [32, 0, 31]
    d, ids, sc = _case_scores(c)
    assert CS.route(sc, ids, c.k) == ["window", "none", "window"] and (CS.int_scores(sc)[0] != CS.int_scores(sc)[2]).any()
    c = cases["chunks8"]
    d, ids, sc = _case_scores(c)
    assert CS.route(sc, ids, c.k) == ["window"] * 4 + ["full", "window", "window", "full"]  # chunks of 3: 2nd and 3rd
    c = cases["nq65"]
    d, ids, sc = _case_scores(c)
    r = CS.route(sc, ids, c.k)
    assert len(r) == 65 and r.count("none") == 14 and r.count("window") == 51


def test_reference_cut_orders_by_score_then_id():
    ids = np.array([7, 0, 3, 9, 5, 4], np.uint32)
    sc = np.array([[5.5, 1.0, 5.0, CS.FLT_MAX, 2.9, 5.99]], np.float32)
    oi, os_, cnt = CS.reference_cut(sc, ids, 3)
    assert cnt.tolist() == [4] and oi.tolist() == [[5, 3, 4]] and os_.tolist() == [[2, 5, 5]]
    oi, os_, cnt = CS.reference_cut(sc, ids, 6)
    assert oi.tolist() == [[5, 3, 4, 7, 0, 0]] and os_.tolist() == [[2, 5, 5, 5, 0, 0]]
    oi, os_, cnt = CS.reference_cut(sc, ids, 0)
    assert oi.shape == (1, 0) and cnt.tolist() == [4]
    assert CS.route(sc, ids, 3) == ["window"] and CS.route(sc, ids, 0) == ["none"] and CS.route(sc, ids, 4097) == ["full"]


def test_color_chunk_scores_refuses_negative_values_and_the_counters_are_read_only():
    """"color_chunk_scores": 0 (the default budgets) or a positive number of score elements; a negative value is refused
    and leaves the knob as it was.  "color_full_sorts" / "color_window_cuts" can be read and never written."""
    import ctypes as C

    from cbird_amd import _lib

    L = _lib.lib()

    def get(key):
        v = C.c_longlong(-2)
        assert L.cbh_get_tuning(key, C.byref(v)) == _lib.CBH_OK, key
        return int(v.value)

    try:
        assert get(b"color_chunk_scores") == 0
        for good in (1, 3 * 4796, (1 << 31) - 1, 0, 77):
            assert L.cbh_set_tuning(b"color_chunk_scores", good) == _lib.CBH_OK and get(b"color_chunk_scores") == good
        for bad in (-1, -77, -(1 << 31)):
            assert L.cbh_set_tuning(b"color_chunk_scores", bad) == _lib.CBH_E_INVAL and get(b"color_chunk_scores") == 77
        for key in (b"color_full_sorts", b"color_window_cuts"):
            before = get(key)
            assert before >= 0
            for v in (0, 1):
                assert L.cbh_set_tuning(key, v) == _lib.CBH_E_INVAL
            assert get(key) == before
    finally:
        assert L.cbh_set_tuning(b"color_chunk_scores", 0) == _lib.CBH_OK
