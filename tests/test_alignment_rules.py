"""CPU: the numpy model of the alignment searches (tests/alignment_rules.py) against facts that do not come from it:
planted shifts, constant and periodic images, the 0 / 255 extreme, the window's borders, planted clip offsets, the two
tie rules of the temporal search, and alignment_transform through the difference image's own warp."""
import numpy as np
import pytest

import alignment_rules as A
import difference_rules as R


@pytest.mark.parametrize("dx,dy", [(-8, -8), (-8, 8), (8, -8), (8, 8), (0, 0), (3, -5)])
def test_a_planted_shift_is_found_with_sad_zero(dx, dy):
    left, right = A.planted(dx, dy, seed=3)
    table, rec = A.align_spatial(left, right)
    assert rec["min_x"] == dx and rec["min_y"] == dy and rec["min_sad"] == 0
    assert (table == 0).sum() == 1 and table[dx + 8, dy + 8] == 0
    assert rec["sad_at_zero"] == table[8, 8] and (rec["sad_at_zero"] == 0) == ((dx, dy) == (0, 0))


def test_constant_images_keep_the_first_shift():
    table, rec = A.align_spatial(np.full((5, 7, 3), 90, np.uint8), np.full((9, 4), 100, np.uint8))
    assert (table == 240 * 240 * 3 * 10).all()
    assert (rec["min_x"], rec["min_y"], rec["min_sad"]) == (-8, -8, 240 * 240 * 30)


def test_a_4_periodic_pattern_against_itself_keeps_the_first_of_its_zeros():
    row = np.array([10, 80, 160, 250], np.uint8)[np.arange(256) % 4]
    img = np.repeat(np.repeat(row[None, :], 256, axis=0)[:, :, None], 3, axis=2)
    table, rec = A.align_spatial(img, img)
    zeros = np.argwhere(table == 0)
    assert sorted({int(x) - 8 for x, _ in zeros}) == [-8, -4, 0, 4, 8] and len(zeros) == 5 * 17
    assert (rec["min_x"], rec["min_y"], rec["min_sad"], rec["sad_at_zero"]) == (-8, -8, 0, 0)


def test_black_against_white_is_the_largest_sad_everywhere():
    table, rec = A.align_spatial(np.zeros((2, 2), np.uint8), np.full((3, 3, 4), 255, np.uint8))
    assert A.MAX_SAD == 44064000 and (table == 44064000).all()
    assert (rec["min_x"], rec["min_y"], rec["min_sad"], rec["sad_at_zero"]) == (-8, -8, 44064000, 44064000)


def test_the_right_image_outside_rows_and_columns_8_to_247_takes_no_part():
    left, right = A.noise(256, 256, 5), A.noise(256, 256, 6)
    other = A.noise(256, 256, 7)
    other[8:248, 8:248] = right[8:248, 8:248]
    assert (other != right).any()
    assert (A.align_spatial(left, right)[0] == A.align_spatial(left, other)[0]).all()
    inside = right.copy()
    inside[8, 8, 0] ^= 1  # (and the corner of the window does)
    assert (A.align_spatial(left, right)[0] != A.align_spatial(left, inside)[0]).all()


def test_a_641_by_479_pair_is_scaled_by_the_pixel_centre_rule():
    left, right = R.textured(641, 479, 1), R.textured(641, 479, 2, 1)
    p = A.plane(right, 256)
    assert p.shape == (256, 256, 3) and (p[..., 0] == p[..., 2]).all()
    assert p[0, 0, 0] == right[0, 1] and p[255, 255, 0] == right[478, 639]  # (1 * 641) // 512 = 1, (511 * 641) // 512 = 639
    table, rec = A.align_spatial(left, right)
    assert table.max() <= A.MAX_SAD and rec["min_sad"] == table.min()
    assert A.align_spatial(left, left)[1]["min_sad"] == 0


# ---- temporal ---------------------------------------------------------------------------------------------------------
def _frames(n, seed=0):
    return [A.noise(6, 9, seed + k) for k in range(n)]


@pytest.mark.parametrize("where", ["first", "start", "last"])
def test_a_window_cut_from_the_left_clip_is_found_there(where):
    left = _frames(64)
    p, start = 60, 30
    assert A.default_start(p) == start
    d0 = {"first": 0, "start": start, "last": p - 1}[where]
    cells, means, rec = A.align_temporal(left, left[d0:d0 + 5], start)
    assert cells.shape == (60, 5) and (cells[d0] == 0).all() and means[d0] == 0 and (np.delete(means, d0) > 0).all()
    assert rec == dict(placement=d0, offset=d0 - start, min_mean=0, start_mean=int(means[start]))
    assert cells.max() <= A.MAX_CELL == 12533760


def test_a_static_clip_stays_at_start():
    f = A.noise(5, 5, 1)
    g = A.noise(5, 5, 2)
    cells, means, rec = A.align_temporal([f] * 12, [g] * 3, 4)
    assert (means == means[0]).all() and means[0] > 0
    assert rec == dict(placement=4, offset=0, min_mean=int(means[0]), start_mean=int(means[0]))


def _ones(count):
    f = np.zeros((128, 128, 3), np.uint8)
    f.reshape(-1)[:count] = 1
    return f  # against a black frame its cell is `count`


@pytest.mark.parametrize("counts,start,want", [
    ([10, 10, 11, 30], 2, 0),  # sums 20, 21, 41: means 10, 10, 20 -- the earlier of the equal means
    ([11, 10, 10, 30], 2, 0),  # sums 21, 20, 40: the larger sum comes first and still wins
    ([10, 10, 11, 30], 1, 1),  # start's mean equals the best: it stays
    ([30, 11, 10, 10], 0, 1),  # sums 41, 21, 20: means 20, 10, 10
])
def test_equal_integer_means_keep_the_earlier_placement_and_never_beat_start(counts, start, want):
    black = np.zeros((128, 128, 3), np.uint8)
    cells, means, rec = A.align_temporal([_ones(c) for c in counts], [black, black], start)
    assert [int(a) + int(b) for a, b in cells] == [counts[d] + counts[d + 1] for d in range(3)]
    assert list(means) == [(counts[d] + counts[d + 1]) // 2 for d in range(3)]
    assert rec["placement"] == want and rec["offset"] == want - start and rec["start_mean"] == means[start]


def test_default_start():
    from cbird_amd.alignment import default_start

    assert [default_start(p) for p in (1, 2, 3, 60, 61)] == [0, 1, 1, 30, 30]
    assert all(default_start(p) == A.default_start(p) for p in range(1, 200))


# ---- alignment_transform ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx,dy", [(3, -5), (-8, 8), (0, 0)])
def test_alignment_transform_redraws_the_right_image_on_the_left(dx, dy):
    from cbird_amd.alignment import alignment_transform

    left, right = A.planted(dx, dy, seed=9)
    rec = A.align_spatial(left, right)[1]
    m = alignment_transform(rec["min_x"], rec["min_y"], left.shape, right.shape)
    assert m.shape == (2, 3) and m.dtype == np.float64
    assert (m == np.array([[1, 0, -dx], [0, 1, -dy]], np.float64)).all()
    canvas = R.warp_canvas(right, m.reshape(6), 256, 256)
    ys, xs = np.mgrid[0:256, 0:256]
    covered = (xs - dx >= 0) & (xs - dx < 256) & (ys - dy >= 0) & (ys - dy < 256)
    assert covered.sum() == (256 - abs(dx)) * (256 - abs(dy))
    assert (canvas[covered] == left[covered]).all() and (canvas[~covered] == 0).all()
    # other sizes: the scale of both sides and the shift in the right image's pixels
    m = alignment_transform(4, -2, (100, 200, 3), (50, 512))
    assert (m == np.array([[2.56, 0, -8.0], [0, 0.5, 0.390625]])).all()
