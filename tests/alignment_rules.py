"""The numpy restatement of alignSpatially (src/gui/videocomparewidget.cpp:590-627) and alignTemporally with sad128
(:629-680) as include/cbird_hip.h states them, written from the rules in vector code.  Everything is an integer, so the
device is held to this with no tolerance.  tests/test_alignment_rules.py holds this file to facts that do not come from it."""
import numpy as np

from difference_rules import rgb32, scale_nearest

SPATIAL, TEMPORAL, REACH = 256, 128, 8
SHIFTS = 2 * REACH + 1
INNER = SPATIAL - 2 * REACH  # 240 rows and columns take part
MAX_SAD = INNER * INNER * 3 * 255
MAX_CELL = TEMPORAL * TEMPORAL * 3 * 255


def plane(img, side):
    """the packed side x side x 3 plane of an image: grey replicated or alpha dropped, then QImage::scaled's rule"""
    return np.ascontiguousarray(scale_nearest(rgb32(img), side, side))


def absdiff_sum(a, b):
    """sum of |a - b| over uint8 arrays, along the last two axes"""
    d = np.maximum(a, b) - np.minimum(a, b)
    return d.sum(axis=(-2, -1), dtype=np.uint64)


def spatial_table_of_planes(a, b):
    """uint32 [17, 17] indexed [xo + 8, yo + 8]: sum over the right plane's interior of |A[y + yo][x + xo] - B[y][x]|"""
    a2 = a.reshape(SPATIAL, SPATIAL * 3)
    inner = b[REACH:REACH + INNER, REACH:REACH + INNER].reshape(INNER, INNER * 3)
    # win[xi, y, k] = a2[y, 3 * xi + k]: the 17 horizontal windows of every row, without copying
    win = np.lib.stride_tricks.as_strided(a2, (SHIFTS, SPATIAL, INNER * 3), (3, SPATIAL * 3, 1), writeable=False)
    table = np.zeros((SHIFTS, SHIFTS), np.uint32)
    for yi in range(SHIFTS):
        table[:, yi] = absdiff_sum(win[:, yi:yi + INNER], inner[None])
    return table


def spatial_pick(table):
    """the record of a table: the first entry in scan order (xo outer, yo inner) below every earlier one"""
    flat = table.reshape(-1)
    k = int(np.argmin(flat))  # (the first of equal minima)
    return dict(min_x=k // SHIFTS - REACH, min_y=k % SHIFTS - REACH, min_sad=int(flat[k]),
                sad_at_zero=int(table[REACH, REACH]))


def align_spatial(left, right):
    """-> (table uint32 [17, 17], record)"""
    table = spatial_table_of_planes(plane(left, SPATIAL), plane(right, SPATIAL))
    return table, spatial_pick(table)


def temporal_cells(left_frames, right_frames):
    """uint32 [P, W]: cell(d, i) = the SAD of all bytes of F[d + i] and G[i] at 128 x 128"""
    f = [plane(x, TEMPORAL).reshape(TEMPORAL, -1) for x in left_frames]
    g = [plane(x, TEMPORAL).reshape(TEMPORAL, -1) for x in right_frames]
    p = len(f) - len(g) + 1
    assert len(g) >= 1 and p >= 1
    cells = np.zeros((p, len(g)), np.uint32)
    memo = {}
    for d in range(p):
        for i in range(len(g)):
            key = (id(left_frames[d + i]), id(right_frames[i]))  # (clips repeat frames: a pair is worked out once)
            if key not in memo:
                memo[key] = int(absdiff_sum(f[d + i], g[i]))
            cells[d, i] = memo[key]
    return cells


def temporal_pick(cells, start):
    """-> (means uint32 [P], record): best = start; for d ascending a strictly smaller mean replaces it"""
    p, w = cells.shape
    assert 0 <= start < p
    means = (cells.astype(np.uint64).sum(axis=1) // np.uint64(w)).astype(np.uint32)
    d = int(np.argmin(means))  # (the earliest of the smallest)
    best = d if means[d] < means[start] else start
    return means, dict(placement=best, offset=best - start, min_mean=int(means[best]), start_mean=int(means[start]))


def align_temporal(left_frames, right_frames, start):
    """-> (cells, means, record)"""
    cells = temporal_cells(left_frames, right_frames)
    means, rec = temporal_pick(cells, start)
    return cells, means, rec


def default_start(p):
    return min(max((p - 1) // 2 + (p - 1) % 2, 0), p - 1)


# ---- case builders -----------------------------------------------------------------------------------------------------
def noise(h, w, seed, ch=3):
    """white noise: no two windows of it agree, so a planted shift is the only zero of its table"""
    shape = (h, w) if ch == 1 else (h, w, ch)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def planted(dx, dy, seed=1, ch=3):
    """(left, right), both 256 x 256, cut from one noise field so that left (x + dx, y + dy) = right (x, y) everywhere
    both exist"""
    t = noise(SPATIAL + 2 * REACH, SPATIAL + 2 * REACH, seed, ch)
    right = t[REACH:REACH + SPATIAL, REACH:REACH + SPATIAL]
    left = t[REACH - dy:REACH - dy + SPATIAL, REACH - dx:REACH - dx + SPATIAL]
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


SOURCE_SIZES = [(1, 1), (3, 5), (256, 256), (257, 255), (641, 479), (32767, 1), (1, 32767)]  # (w, h)
