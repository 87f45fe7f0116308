"""CPU: tests/demosaic_rules.py, the model of demosaicHough the device is held to, against hand-computed values; the
library's host-only steps 6 and 7 (cbh_grid_select, cbh_grid_rects: no device) against the same values and the model;
and the condition the model meets on synthetic contact sheets."""
import numpy as np
import pytest

import demosaic_rules as M

F = np.float32


# ---- step 2 ----------------------------------------------------------------------------------------------------------------
def test_gauss3_on_3x3_and_1xn():
    a = np.array([[0, 16, 32], [48, 64, 80], [96, 112, 128]], np.uint8)
    g = M.gauss3(a)
    assert g[1, 1] == 64  # S = 1024
    # the corner: rows and columns -1 reflect onto 1: S = 64 + 2*48 + 64 + 2*16 + 0 + 2*16 + 64 + 2*48 + 64 = 512
    assert g[0, 0] == (512 + 8) >> 4
    # one row reflects onto itself: S = 4 * (left + 2 * centre + right), the ends reflecting onto their one neighbour
    row = np.array([[10, 20, 40, 80]], np.uint8)
    assert M.gauss3(row).tolist() == [[15, 23, 45, 60]]
    assert M.gauss3(row.T).tolist() == [[15], [23], [45], [60]]
    assert M.gauss3(np.array([[77]], np.uint8)).tolist() == [[77]]


# ---- step 3 ----------------------------------------------------------------------------------------------------------------
def test_suppression_on_a_vertical_and_a_horizontal_step():
    g = np.zeros((8, 8), np.uint8)
    g[:, 4:] = 100
    dx, dy = M.sobel(g)
    assert (dy == 0).all() and (dx[:, 3] == 400).all() and (dx[:, 4] == 400).all() and (dx[:, :3] == 0).all()
    # m = 400 in columns 3 and 4: column 3 has m > left (0) and m >= right (400); column 4 fails m > left (400)
    cls = M.class_map(g, 50, 0)
    want = np.zeros((8, 8), np.uint8)
    want[:, 3] = 2
    assert (cls == want).all()
    assert (M.class_map(g.T.copy(), 50, 0) == want.T).all()  # m > up, m >= down: row 3
    # thresholds: strong needs m > high, a candidate m > low
    assert (M.class_map(g, 400, 0)[:, 3] == 1).all() and (M.class_map(g, 399, 0)[:, 3] == 2).all()
    assert (M.class_map(g, 400, 400) == 0).all() and (M.class_map(g, 0, 399)[:, 3] == 2).all()


def test_suppression_on_both_diagonal_steps():
    y, x = np.mgrid[0:8, 0:8]
    g = np.where(x + y >= 8, 100, 0).astype(np.uint8)
    dx, dy = M.sobel(g)
    # along the normal (1, 1): x + y = 6, 7, 8, 9 have dx = dy = 100, 300, 300, 100, so m = 200, 600, 600, 200; both
    # comparisons of the diagonal class are strict, against x + y - 2 and x + y + 2: the two middle lines stay
    assert dx[3, 3] == 100 and dx[3, 4] == 300 and dx[4, 4] == 300 and dx[4, 5] == 100 and (dx[2:6, 2:6] == dy[2:6, 2:6]).all()
    cls = M.class_map(g, 50, 0)
    inner = (slice(2, 6), slice(2, 6))
    want = np.where((x + y == 7) | (x + y == 8), 2, 0)
    assert (cls[inner] == want[inner]).all()
    # the other diagonal: dx changes sign, so s = -1 and the neighbours are up-right and down-left
    mirrored = M.class_map(g[:, ::-1].copy(), 50, 0)
    assert (mirrored[inner] == want[:, ::-1][inner]).all()
    # (dx ^ dy) < 0 picks them: a one-pixel-wide ridge along the other diagonal would be cut by the wrong pair
    dxm, dym = M.sobel(g[:, ::-1].copy())
    on = dxm[inner] != 0  # (the flat corners have dx = dy = 0)
    assert ((dxm[inner] ^ dym[inner]) < 0)[on].all() and ((dx[inner] ^ dy[inner]) >= 0).all()


def test_hysteresis_is_the_flood_fill():
    cls = np.zeros((5, 7), np.uint8)
    cls[0, 0] = 2
    cls[1, 1] = cls[2, 2] = cls[1, 3] = 1   # a diagonal chain from the seed, winding up again
    cls[4, 6] = cls[4, 5] = 1               # touches no seed
    e = M.hysteresis(cls)
    want = np.zeros((5, 7), np.uint8)
    want[0, 0] = want[1, 1] = want[2, 2] = want[1, 3] = 255
    assert (e == want).all()


# ---- step 5 ----------------------------------------------------------------------------------------------------------------
def test_rows_and_columns_vote_at_even_bins_and_the_line_position():
    tc, ts = M.hough_tables()
    assert tc[0] == F(2) and ts[0] == F(0) and ts[2] == F(2) and abs(tc[2]) < 1e-6
    i = np.arange(32768)
    for j in (0, 1, 32766):
        assert (M.vote_bins(i, np.full_like(i, j), 2, tc, ts) == 2 * i).all()   # a row is one bin whatever the column
        assert (M.vote_bins(np.full_like(i, j), i, 0, tc, ts) == 2 * i).all()   # and a column whatever the row
    for w, h in ((32767, 32767), (1, 32767), (600, 400)):
        numrho = 4 * (w + h) + 2
        for k in range(max(w, h)):
            assert M.line_position(2 * k + (numrho - 1) // 2, numrho) == max(k - 1, 0)


def test_local_maximum_rule():
    acc = np.zeros((4, 50), np.int64)
    acc[2, 5] = 24                   # not above the threshold
    acc[2, 10] = acc[2, 11] = 30     # acc > acc(r - 1) but acc >= acc(r + 1): the first of two equal bins
    acc[2, 20] = acc[1, 20] = 30     # equal to the 45 degree bin: rejected (acc > acc(n - 1))
    acc[2, 30] = acc[3, 30] = 30     # equal to the 135 degree bin: kept (acc >= acc(n + 1))
    acc[2, 40], acc[3, 40] = 30, 31  # below the 135 degree bin
    acc[0, 7] = acc[1, 7] = 30       # a column equal to the 45 degree bin: kept, there is no angle -1
    acc[0, 9], acc[1, 9] = 30, 31
    lm = M.local_maxima(acc, 24)
    assert np.nonzero(lm[2])[0].tolist() == [10, 30]
    assert np.nonzero(lm[0])[0].tolist() == [7]
    # (the diagonals' own lines, which the angle test drops: bin (1, 20) is >= its equal at angle 2)
    assert np.nonzero(lm[3])[0].tolist() == [40] and np.nonzero(lm[1])[0].tolist() == [9, 20]


def test_grid_lines_counts_and_thresholds():
    e = np.zeros((40, 50), np.uint8)
    e[36, :40] = 255      # threshold int(50 * 0.8) = 40: exactly 40 is not enough
    e[38, :41] = 255
    e[:32, 45] = 255      # int(40 * 0.8) = 32: exactly 32 is not enough
    e[:33, 47] = 255
    hor, ver = M.grid_lines(e, 0.8)
    assert hor == [37] and ver == [46]
    e[:, :] = 0
    e[0, :] = e[1, :] = 255
    assert M.grid_lines(e, 0.8)[0] == [0, 0]  # rows 0 and 1 both give 0: duplicates kept
    assert M.grid_lines(e, 0.8, h_margin=1)[0] == []


# ---- step 6 ----------------------------------------------------------------------------------------------------------------
SELECT_CASES = [  # (lines with 0 and the side, cols, min spacing, tolerance, the grid)
    ([0, 100, 200, 300, 400], 400, 96, 4, [0, 100, 200, 300, 400]),  # spacing N
    ([0, 100, 200, 400], 400, 96, 4, [0, 100, 200, 400]),            # a step of 2 N
    ([0, 100, 150, 200], 400, 40, 4, [0, 100, 150, 200]),            # steps of N / 2
    # 2 N = 200 > cols = 150 is not accepted from spacing 100, which leaves [0, 100, 200]; spacing 200 accepts 200 / 1
    # and 200 / 2 and gives [0, 200, 400]: as many lines, the larger span wins
    ([0, 100, 200, 400], 150, 96, 4, [0, 200, 400]),
    ([0, 100, 204], 300, 96, 4, [0, 100, 204]),  # s >= d - margin
    ([0, 100, 196], 300, 96, 4, [0, 100]),       # s < d + margin fails at d = s - margin: the pair alone is the grid
    ([0, 0, 100, 100, 200, 200], 200, 96, 4, [0, 100, 200]),  # duplicates: d2 stays 0, nothing is dropped
    ([0, 50, 100], 100, 96, 4, []),              # no spacing of at least 96 among the pairs the loops visit
    ([0, 300], 300, 96, 4, []),                  # fewer than 3 entries
]


@pytest.mark.parametrize("lines,cols,min_size,margin,want", SELECT_CASES)
def test_select_lines(lines, cols, min_size, margin, want):
    assert M.select_lines(lines, cols, min_size, margin) == want


def test_grid_rects_rules():
    assert M.grid_rects([0, 100], [], 150, 100) == [(0, 0, 150, 100)]          # fewer than 3 lines both ways
    assert M.grid_rects([], [], 150, 100) == [(0, 0, 150, 100)]
    assert M.grid_rects([0, 100, 200], [], 150, 200) == [(2, 2, 146, 96), (2, 102, 146, 96)]  # an empty grid is {0, side}
    assert M.grid_rects([10, 110], [0, 100, 200, 300], 300, 120, 3) == [(3, 13, 94, 94), (103, 13, 94, 94), (203, 13, 94, 94)]
    assert M.grid_rects([0, 3, 100], [0, 100], 100, 100) == [(2, 2, 96, -1), (2, 5, 96, 93)]  # a side below 1 comes out
    assert not M.subdivides((2, 2, 96, -1), M.DEFAULTS) and not M.subdivides((0, 0, 0, 5), M.DEFAULTS)
    assert M.subdivides((0, 0, 251, 100), M.DEFAULTS) and not M.subdivides((0, 0, 250, 100), M.DEFAULTS)
    # a cell that leaves its image or is all of it is not subdivided either
    assert M.subdivides((0, 0, 300, 100), M.DEFAULTS, (300, 101)) and not M.subdivides((0, 0, 300, 100), M.DEFAULTS, (300, 100))
    assert not M.subdivides((-2, 0, 300, 100), M.DEFAULTS, (400, 400)) and not M.subdivides((0, 1, 300, 100), M.DEFAULTS, (400, 100))
    assert M.subdivides((0, 0, 49, 100), M.DEFAULTS) and not M.subdivides((0, 0, 50, 100), M.DEFAULTS)


def test_library_grid_select_and_rects_on_the_host():
    """cbh_grid_select / cbh_grid_rects need no device: the hand-made cases, then random lists against the model"""
    from cbird_amd import _lib
    from cbird_amd.demosaic import grid_rects, grid_select

    for lines, cols, min_size, margin, want in SELECT_CASES:
        side = lines[-1]
        inner = list(lines[1:-1])  # the entry appends 0 and the side itself
        assert grid_select(inner[::-1], side, cols, min_size, margin).tolist() == want
    rng = np.random.default_rng(5)
    for _ in range(200):
        side = int(rng.integers(1, 700))
        step = int(rng.integers(20, 160))
        pos = [int(v) for v in rng.integers(0, side + 1, rng.integers(0, 12))]
        pos += [int(np.clip(k * step + rng.integers(-5, 6), 0, side)) for k in range(1, side // step + 1) if rng.random() < 0.8]
        cols = int(rng.integers(1, 700))
        min_size, margin = int(rng.integers(0, 120)), int(rng.integers(0, 8))
        want = M.select_lines(sorted(pos + [0, side]), cols, min_size, margin)
        assert grid_select(pos, side, cols, min_size, margin).tolist() == want
    for hg, vg, w, h, crop in [([0, 100], [], 150, 100, 2), ([], [], 150, 100, 2), ([0, 100, 200], [], 150, 200, 2),
                               ([10, 110], [0, 100, 200, 300], 300, 120, 3), ([0, 3, 100], [0, 100], 100, 100, 2)]:
        assert [tuple(r) for r in grid_rects(hg, vg, w, h, crop).tolist()] == M.grid_rects(hg, vg, w, h, crop)
    L = _lib.lib()
    n = np.zeros(1, np.uint64)
    out = np.full(8, -7, np.int32)
    hg, vg = np.array([0, 100, 200], np.int32), np.array([0, 50, 100], np.int32)
    assert L.cbh_grid_rects(hg.ctypes.data, 3, vg.ctypes.data, 3, 100, 200, 2, out.ctypes.data, 1, n.ctypes.data) == _lib.CBH_E_OVERFLOW
    assert n[0] == 4 and (out == -7).all()  # the needed count, nothing written
    assert L.cbh_grid_select(None, 1, 10, 10, 96, 4, out.ctypes.data, n.ctypes.data) == _lib.CBH_E_INVAL
    bad = np.array([11], np.int32)
    assert L.cbh_grid_select(bad.ctypes.data, 1, 10, 10, 96, 4, out.ctypes.data, n.ctypes.data) == _lib.CBH_E_INVAL


def test_default_params_match_the_model():
    from cbird_amd.demosaic import default_params

    p = default_params()
    for k, v in M.DEFAULTS.items():
        assert getattr(p, k) == F(v) if isinstance(v, float) else getattr(p, k) == v


# ---- the model on sheets ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", M.LAYOUTS, ids=lambda l: "x".join(map(str, l[0])))
def test_model_finds_every_planted_cell(layout):
    img, cells = M.sheet(*layout, seed=1)
    rects = M.demosaic(img)
    assert M.sheet_meets_condition(rects, cells, layout[2]), (rects, cells)
    if len(set(layout[0])) > 1:  # staggered: the top level finds the strips, every strip is subdivided
        top = M.stages(img, M.DEFAULTS)["rects"]
        assert len(top) == len(layout[0]) and all(M.subdivides(r, M.DEFAULTS) for r in top)


def test_textured_sheets_load_the_line_lists():
    for seed in (1, 2):
        st = M.stages(M.textured_sheet(seed), M.DEFAULTS)
        assert len(st["hor"]) > 50 and len(st["ver"]) > 20
