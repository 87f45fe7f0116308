"""CPU: the numpy model of the difference image (tests/difference_rules.py) against values worked out by hand, and the
library's cut rule (cbh_gray_cuts, host code, no device) against the model where float32 rounds the running sum."""
import numpy as np
import pytest

import difference_rules as R


@pytest.mark.parametrize("s, bgr", [(0, (0, 0, 0)), (31, (248, 0, 0)), (32, (0, 8, 0)), (1023, (248, 248, 0)),
                                    (1024, (0, 0, 2)), (131071, (248, 248, 254)), (131072, (0, 0, 0)),
                                    (195075, (24, 128, 124))])
def test_colour_map(s, bgr):
    """r = ((s >> 10) << 1) & 255 wraps above 131071; 195075 = 3 * 255^2 is the largest sum"""
    assert tuple(int(v) for v in R.colour(s)) == bgr


def test_stretch_table_ties_round_to_even():
    """(0, 170): alpha = 1.5 exactly, so every odd s lands on a half"""
    t = R.stretch_table(0, 170)
    assert [int(t[s]) for s in (0, 1, 2, 3, 4, 5, 6, 7, 169, 170, 171, 255)] == [0, 2, 3, 4, 6, 8, 9, 10, 254, 255, 255, 255]
    for s in range(1, 170, 2):  # 1.5 s = k + 0.5 -> the even one of k, k + 1
        k = (3 * s - 1) // 2
        assert int(t[s]) == (k if k % 2 == 0 else k + 1)


def test_stretch_table_extremes():
    t = R.stretch_table(10, 11)  # alpha = 255
    assert (t[:11] == 0).all() and (t[11:] == 255).all()
    assert (R.stretch_table(0, 255) == np.arange(256)).all()
    t = R.stretch_table(254, 255)
    assert (t[:255] == 0).all() and t[255] == 255
    for lo, hi in [(5, 5), (9, 3), (256, -1), (77, 76)]:  # min >= max: copied
        assert (R.stretch_table(lo, hi) == np.arange(256)).all()


def _hist(**bins):
    h = np.zeros(256, np.uint32)
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


def test_cuts_by_hand():
    one = _hist(b77=54)
    assert R.gray_cuts(one, 5) == (77, 76)  # clip 1.35: the only level is both cuts' stop -> no stretch
    assert R.gray_cuts(one, 0) == (77, 77)
    two = _hist(b40=26, b200=51)
    assert R.gray_cuts(two, 5) == (40, 199)  # clip 1.925, max - clip 75.075: acc[199] = 26 is the first below it
    assert R.gray_cuts(two, 0) == (40, 200)
    # total 100, clip_pct 50: clip = 25 = acc[10] exactly (not < clip: the cut), max - clip = 75 = acc[20] exactly (>=: passed)
    exact = _hist(b10=25, b20=50, b30=25)
    assert R.gray_cuts(exact, 50) == (10, 19)
    assert R.gray_cuts(np.zeros(256, np.uint32), 0) == (256, -1)


def test_model_on_a_pair_by_hand():
    """2 x 1 against 1 x 1, no clip: left {10, 20} stretches to {0, 255}, the right pixel is its own range (copied) and
    is scaled to both positions"""
    left = np.array([[10, 20]], np.uint8)
    right = np.array([[[3, 0, 255]]], np.uint8)  # grey (3 * 1868 + 255 * 4899 + 8192) >> 14 = 77
    pic, rec = R.difference_image(left, right, clip_pct=0)
    s0 = 3 * 3 + 0 + 255 * 255            # left 0 against (3, 0, 255)
    s1 = 252 * 252 + 255 * 255 + 0        # left 255
    assert (rec["w"], rec["h"], rec["warped"]) == (2, 1, 0)
    assert (rec["left_min"], rec["left_max"], rec["right_min"], rec["right_max"]) == (10, 20, 77, 77)
    assert rec["sum_total"] == s0 + s1 and rec["sum_max"] == s1 and rec["n_ge32"] == 2 and rec["n_ge1024"] == 2
    for x, s in enumerate((s0, s1)):
        assert tuple(pic[0, x]) == ((s & 31) << 3, ((s >> 5) & 31) << 3, ((s >> 10) << 1) & 255, 255)


def test_the_pair_cases_are_what_they_claim():
    """the groups tests/test_difference.py runs on the device, here through the model alone, with the workgroup's portion
    the library was built with (a read-only figure that needs no device)"""
    import ctypes as C

    from cbird_amd import _lib

    v = C.c_longlong(0)
    assert _lib.lib().cbh_get_tuning(b"diff_block_pixels", C.byref(v)) == 0
    block_pixels = int(v.value)
    by = {}
    for grp in R.pair_groups(block_pixels):
        left, rights = R.group_in_channels(grp, 3, 3)
        by[grp["name"]] = (grp, left, rights, R.model_group(left, rights, grp))
    _, left, rights, want = by["sizes"]
    assert want[0][1]["sum_total"] == 0  # identical
    same = want[1][1]  # identical up to brightness: small, where an unrelated picture of the same size is not
    assert 0 < same["sum_total"] < same["w"] * same["h"] * 300 and same["n_ge1024"] == 0
    assert [w[1]["w"] for w in want] == [23, 23, 23, 31, 17, 23, 23]  # smaller rights grow, larger ones make the left grow
    ex = by["extremes"][3]
    assert ex[0][1]["sum_max"] == 195075 and (ex[0][0][..., 2] == 124).all()  # r wrapped in a real picture
    assert ex[1][1]["sum_total"] == 0
    assert (by["10x2_vs_4x6"][3][0][1]["w"], by["10x2_vs_4x6"][3][0][1]["h"]) == (4, 6)
    assert (by["1x1_vs_7x5"][3][0][1]["w"], by["1x1_vs_7x5"][3][0][1]["h"]) == (7, 5)
    assert [(w[1]["w"], w[1]["h"]) for w in by["equal_areas"][3]] == [(4, 6), (8, 3)]  # equal areas: the left is scaled
    dy = by["dyadic"][3]
    assert [w[1]["warped"] for w in dy] == [0] + [1] * 10 + [0]
    assert all((w[1]["w"], w[1]["h"]) == (24, 18) for w in dy[1:11]) and (dy[0][1]["w"], dy[0][1]["h"]) == (30, 22)
    assert dy[8][1]["right_min"] >= dy[8][1]["right_max"]  # nothing covered: a constant canvas
    assert dy[9][0].tobytes() == dy[10][0].tobytes()  # both singular matrices draw through the identity
    ge = by["general"]
    assert ge[1].shape[0] * ge[1].shape[1] > block_pixels and [w[1]["warped"] for w in ge[3]] == [1, 0, 1, 0]


def test_library_cut_rule_is_the_models_where_float32_rounds():
    """counts whose float32 running sum is not the integer sum (single counts above 2^24 that are odd, and sums that
    pass 2^24 on the way): cbh_gray_cuts, the function the device runs, against the loops of the model"""
    from cbird_amd.difference import gray_cuts

    rng = np.random.default_rng(5)
    hists = []
    h = np.zeros(256, np.uint32)
    h[3], h[4:200], h[250] = (1 << 24) + 1, 3, (1 << 25) + 3
    hists.append(h)
    hists.append(rng.integers((1 << 24) - 50, (1 << 24) + 50, 256).astype(np.uint32))
    hists.append(rng.integers(0, 1 << 22, 256).astype(np.uint32))
    hists.append((rng.integers(0, 2, 256) * rng.integers(1, 1 << 26, 256)).astype(np.uint32))
    hists.append(_hist(b10=25, b20=50, b30=25))
    hists.append(_hist(b0=(1 << 30), b255=1))
    hists.append(np.zeros(256, np.uint32))
    rounded = 0
    for h in hists:
        acc = np.float32(0)
        for c in h:
            acc = np.float32(acc + np.float32(c))
        rounded += int(acc) != int(h.astype(np.uint64).sum())
    assert rounded >= 4
    hs = np.stack(hists)
    for clip in (0, 0.5, 1, 5, 50, 99.5, 200):
        lo, hi = gray_cuts(hs, clip)
        for k, h in enumerate(hists):
            assert (int(lo[k]), int(hi[k])) == R.gray_cuts(h, clip), (k, clip)


def test_library_cut_rule_refuses_a_negative_clip():
    from cbird_amd import CbhError
    from cbird_amd.difference import gray_cuts

    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(CbhError):
            gray_cuts(np.zeros((1, 256), np.uint32), bad)
