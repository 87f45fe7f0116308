"""The numpy restatement of demosaicHough (src/cvutil.cpp:1445-1688) as include/cbird_hip.h states it, steps 1-8, and
the builders of the cases the tests run.  The contrast stage and the grey view come from tests/difference_rules.py.
Integer arithmetic everywhere but the Hough tables and votes (float32, every product and sum rounded, nothing fused);
plain loops where the rule is a loop (selectLines, the rectangles, the subdivision), a flood fill for the hysteresis.
Every output is an integer, so the device is held to this with no tolerance.
tests/test_demosaic_rules.py holds this file to hand-computed values."""
import numpy as np

from difference_rules import as_channels, auto_contrast, gray_view, textured

F = np.float32
DEFAULTS = dict(clip_pct=10.0, pre_blur=3, canny1=50, canny2=0, post_blur=3, h_margin=0, v_margin=0, hough_rho=0.5,
                hough_theta=45.0, hough_thresh_factor=0.8, min_grid_spacing=96, grid_tolerance=4, crop_margin=2,
                max_aspect=2.5, min_aspect=0.5)
SUB_FACTOR = 0.95  # houghThreshFactor of every subdivision (:1677)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ---- step 2: the 3 x 3 Gaussian on bytes --------------------------------------------------------------------------------
def reflect101(i, n):
    if n == 1:
        return 0
    return -i if i < 0 else 2 * n - 2 - i if i >= n else i


def gauss3(img):
    """(S + 8) >> 4, S = the (1,2,1) x (1,2,1) sum of the nine bytes, border REFLECT_101"""
    a = np.asarray(img).astype(np.int64)
    h, w = a.shape
    p = a[[reflect101(y, h) for y in range(-1, h + 1)]][:, [reflect101(x, w) for x in range(-1, w + 1)]]
    s = np.zeros((h, w), np.int64)
    for dy, wy in enumerate((1, 2, 1)):
        for dx, wx in enumerate((1, 2, 1)):
            s += wy * wx * p[dy:dy + h, dx:dx + w]
    return ((s + 8) >> 4).astype(np.uint8)


# ---- step 3: Canny --------------------------------------------------------------------------------------------------------
def sobel(g):
    """(dx, dy) of the 3 x 3 Sobel, border REPLICATE"""
    h, w = g.shape
    p = np.pad(np.asarray(g).astype(np.int64), 1, mode="edge")
    dx = (p[0:h, 2:] + 2 * p[1:h + 1, 2:] + p[2:, 2:]) - (p[0:h, 0:w] + 2 * p[1:h + 1, 0:w] + p[2:, 0:w])
    dy = (p[2:, 0:w] + 2 * p[2:, 1:w + 1] + p[2:, 2:]) - (p[0:h, 0:w] + 2 * p[0:h, 1:w + 1] + p[0:h, 2:])
    return dx, dy


def class_map(g, t1, t2):
    """0 none, 1 candidate, 2 strong"""
    low, high = min(t1, t2), max(t1, t2)
    h, w = g.shape
    dx, dy = sobel(g)
    m = np.abs(dx) + np.abs(dy)
    mp = np.pad(m, 1)  # 0 outside the image
    c = lambda oy, ox: mp[1 + oy:1 + oy + h, 1 + ox:1 + ox + w]
    x, y = np.abs(dx), np.abs(dy) << 15
    t22 = x * 13573
    t67 = t22 + (x << 16)
    horiz = (m > c(0, -1)) & (m >= c(0, 1))
    vert = (m > c(-1, 0)) & (m >= c(1, 0))
    neg = (dx ^ dy) < 0  # s = -1: up-right and down-left
    diag = np.where(neg, (m > c(-1, 1)) & (m > c(1, -1)), (m > c(-1, -1)) & (m > c(1, 1)))
    keep = np.where(y < t22, horiz, np.where(y > t67, vert, diag))
    cand = (m > low) & keep
    return (cand.astype(np.uint8) + (cand & (m > high)).astype(np.uint8))


def hysteresis(cls):
    """255 on every candidate 8-connected, through candidates, to a strong pixel: a flood fill from the strong ones"""
    h, w = cls.shape
    p = np.pad(cls, 1)
    out = np.zeros((h + 2, w + 2), np.uint8)
    stack = [(int(y) + 1, int(x) + 1) for y, x in zip(*np.nonzero(cls == 2))]
    for y, x in stack:
        out[y, x] = 255
    while stack:
        y, x = stack.pop()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                yy, xx = y + dy, x + dx
                if p[yy, xx] and not out[yy, xx]:
                    out[yy, xx] = 255
                    stack.append((yy, xx))
    return out[1:-1, 1:-1].copy()


def edge_map(img, p):
    """steps 1-4 -> (edges, class map before hysteresis)"""
    adjusted, _, _ = auto_contrast(img, p["clip_pct"])
    g = gray_view(adjusted)
    if p["pre_blur"]:
        g = gauss3(g)
    cls = class_map(g, p["canny1"], p["canny2"])
    e = hysteresis(cls)
    if p["post_blur"]:
        e = gauss3(e)
    return e, cls


# ---- step 5: Hough votes -----------------------------------------------------------------------------------------------------
def hough_tables(theta_deg=45.0):
    """(tabCos, tabSin) of the four angles: float32 accumulation of theta, the tables through f64 cos / sin, times 1 / rho"""
    theta = F(np.float64(F(theta_deg)) * np.pi / 180)
    ang, tc, ts = F(0), [], []
    for _ in range(4):
        tc.append(F(np.cos(np.float64(ang)) * 2.0))
        ts.append(F(np.sin(np.float64(ang)) * 2.0))
        ang = F(ang + theta)
    return np.array(tc, F), np.array(ts, F)


def vote_bins(i, j, n, tc, ts):
    """r - (numrho - 1) / 2 of pixels (row i, column j) at angle n: float32 products, a float32 sum, half to even"""
    a = (np.asarray(j).astype(F) * tc[n]).astype(F)
    b = (np.asarray(i).astype(F) * ts[n]).astype(F)
    return np.rint((a + b).astype(F)).astype(np.int64)


def accumulator(edges):
    h, w = edges.shape
    numrho = 4 * (w + h) + 2
    tc, ts = hough_tables()
    acc = np.zeros((4, numrho), np.int64)
    i, j = np.nonzero(edges)
    for n in range(4):
        np.add.at(acc[n], vote_bins(i, j, n, tc, ts) + (numrho - 1) // 2, 1)
    return acc


def local_maxima(acc, threshold):
    """bool [4, numrho]: the bins that are lines; missing neighbours count 0"""
    a = np.pad(acc, 1)
    b = a[1:-1, 1:-1]
    return (b > threshold) & (b > a[1:-1, 0:-2]) & (b >= a[1:-1, 2:]) & (b > a[0:-2, 1:-1]) & (b >= a[2:, 1:-1])


def line_position(r, numrho):
    """int(rho) of bin r, the long way"""
    rho = F(F(F(r) - F(F(numrho - 1) * F(0.5))) * F(0.5))
    return int(rho)


def grid_lines(edges, factor, h_margin=0, v_margin=0):
    """-> (horizontal positions, vertical positions), ascending, duplicates kept"""
    h, w = edges.shape
    numrho = 4 * (w + h) + 2
    acc = accumulator(edges)
    hor = [line_position(int(r), numrho) for r in np.nonzero(local_maxima(acc, int(F(w) * F(factor)))[2])[0]]
    ver = [line_position(int(r), numrho) for r in np.nonzero(local_maxima(acc, int(F(h) * F(factor)))[0])[0]]
    hor = [y for y in hor if y >= h_margin and y < h - h_margin]
    ver = [x for x in ver if x >= v_margin and x < w - v_margin]
    return hor, ver


# ---- step 6: selectLines (:1552-1617) --------------------------------------------------------------------------------------
def select_lines(lines, cols, min_size=96, margin=4):
    lines = [int(v) for v in lines]
    max_grid = []
    for k in range(len(lines) - 2):
        for i in range(k + 1, len(lines) - 1):
            grid_size = lines[i] - lines[k]
            if grid_size < min_size:
                continue
            grid = [lines[k], lines[i]]
            accepted = []
            for n in range(1, 3):
                s = n * grid_size
                if s > cols:
                    break
                accepted.append(s)
            for n in range(1, 3):
                s = grid_size // n
                if s < min_size:
                    break
                accepted.append(s)
            prev = i
            while True:
                last = prev
                found = False
                for j in range(prev + 1, len(lines)):
                    d = lines[j] - lines[prev]
                    for s in accepted:
                        if s >= d - margin and s < d + margin:
                            d2 = grid[-1] - lines[prev]
                            if d2 > 0:
                                if abs(d2 - grid_size) < abs(d - grid_size):
                                    continue
                                grid.pop()
                            grid.append(lines[j])
                            prev = j
                            found = True
                            break
                    if found:
                        break
                if not prev > last:
                    break
            if not max_grid or len(grid) > len(max_grid) or (len(grid) == len(max_grid) and
                                                             grid[-1] - grid[0] > max_grid[-1] - max_grid[0]):
                max_grid = grid
    return max_grid


def grid_of(positions, side, cols, p):
    return select_lines(sorted(list(positions) + [0, side]), cols, p["min_grid_spacing"], p["grid_tolerance"])


# ---- step 7: the rectangles (:1629-1664) -------------------------------------------------------------------------------------
def grid_rects(hgrid, vgrid, w, h, crop=2):
    hgrid = list(hgrid) or [0, h]
    vgrid = list(vgrid) or [0, w]
    if len(hgrid) < 3 and len(vgrid) < 3:
        return [(0, 0, w, h)]
    out = []
    y0 = hgrid[0]
    for y1 in hgrid[1:]:
        x0 = vgrid[0]
        for x1 in vgrid[1:]:
            out.append((x0 + crop, y0 + crop, x1 - x0 - 2 * crop, y1 - y0 - 2 * crop))
            x0 = x1
        y0 = y1
    return out


# ---- step 8 and the whole ------------------------------------------------------------------------------------------------------
def stages(img, p, factor=None):
    """one image, no subdivision -> dict(cls, edges, hor, ver, hgrid, vgrid, rects)"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    factor = p["hough_thresh_factor"] if factor is None else factor
    edges, cls = edge_map(img, p)
    hor, ver = grid_lines(edges, factor, p["h_margin"], p["v_margin"])
    hgrid, vgrid = grid_of(hor, h, w, p), grid_of(ver, w, w, p)
    return dict(cls=cls, edges=edges, hor=hor, ver=ver, hgrid=hgrid, vgrid=vgrid,
                rects=grid_rects(hgrid, vgrid, w, h, p["crop_margin"]))


def subdivides(r, p, node=None):
    """node = (w, h) of the image r is a cell of"""
    x, y, w, h = r
    if w < 1 or h < 1:  # the reference would assert or throw; not subdivided
        return False
    if node is not None:  # nor a cell that leaves its image (it would throw) or is all of it (it would never end)
        if x < 0 or y < 0 or x + w > node[0] or y + h > node[1] or (w, h) == tuple(node):
            return False
    aspect = F(w) / F(h)
    return bool(aspect > F(p["max_aspect"]) or aspect < F(p["min_aspect"]))


def demosaic(img, p=None, factor=None):
    """-> [(x, y, w, h)] in the reference's order"""
    p = p or DEFAULTS
    img = np.asarray(img, np.uint8)
    rects = stages(img, p, factor)["rects"]
    if len(rects) < 2:
        return rects
    final = []
    for r in rects:
        sub = []
        if subdivides(r, p, (img.shape[1], img.shape[0])):
            x, y, w, h = r
            sub = demosaic(img[y:y + h, x:x + w], p, SUB_FACTOR)
        if sub:
            final += [(r[0] + s[0], r[1] + s[1], s[2], s[3]) for s in sub]
        else:
            final.append(r)
    return final


# ---- case builders ---------------------------------------------------------------------------------------------------------
def smooth_tile(w, h, seed):
    """per channel 128 + 30 * the sum of three cosines with periods of 40 .. 120 px"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    t = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(3):
            px, py = rng.uniform(40, 120, 2)
            ph = rng.uniform(0, 2 * np.pi)
            t[:, :, c] += np.cos(2 * np.pi * (x / px + y / py) + ph)
    return np.clip(128 + 30 * t, 0, 255).astype(np.uint8)


def sheet(cols_per_row, tile_h, gap, bg, width, seed=0, tile=smooth_tile):
    """a contact sheet as BGR: row k holds cols_per_row[k] tiles of tile_h rows, `gap` pixels of background `bg` around
    every tile -> (image, the planted cells as (x, y, w, h) row by row)"""
    rows = len(cols_per_row)
    height = rows * tile_h + (rows + 1) * gap
    img = np.full((height, width, 3), bg, np.uint8)
    cells = []
    for k, n in enumerate(cols_per_row):
        y = gap + k * (tile_h + gap)
        free = width - (n + 1) * gap
        x = gap
        for c in range(n):
            tw = free // n + (1 if c < free % n else 0)
            img[y:y + tile_h, x:x + tw] = tile(tw, tile_h, seed * 100 + k * 10 + c)
            cells.append((x, y, tw, tile_h))
            x += tw + gap
    return img, cells


# (tile columns per row, tile height, gap, background, sheet width); the first and the last are staggered: both strips
# are subdivided at 0.95
LAYOUTS = [((4, 3), 150, 10, 240, 530), ((3, 3), 120, 8, 235, 512), ((2, 2, 2), 100, 4, 10, 212), ((4,), 160, 10, 255, 530),
           ((5, 2), 110, 6, 250, 596)]


def sheet_meets_condition(rects, cells, gap):
    """exactly one rectangle per planted cell, every edge within `gap` pixels of the cell's"""
    if len(rects) != len(cells):
        return False
    left = list(cells)
    for x, y, w, h in rects:
        hit = [c for c in left if abs(c[0] - x) <= gap and abs(c[1] - y) <= gap and abs(c[0] + c[2] - x - w) <= gap and
               abs(c[1] + c[3] - y - h) <= gap]
        if len(hit) != 1:
            return False
        left.remove(hit[0])
    return True


def textured_sheet(seed, ch=3):
    """a sheet tiled with difference_rules.textured: more than 100 lines a direction, a load for the line lists and
    step 6 (model equality only: the stripes split the tiles)"""
    img, _ = sheet((3, 2), 110, 6, 245, 400, seed, tile=lambda w, h, s: textured(w, h, s))
    return as_channels(img, ch, seed)


# ---- the hysteresis cases ------------------------------------------------------------------------------------------------
# On a horizontal ramp 0 .. 255 (so that clip_pct 0 stretches nothing; its own gradient is about 5) a one-pixel path 40
# above the ramp gives magnitudes around 160 beside it, a seed 200 above the ramp around 800
HYST_PARAMS = dict(clip_pct=0.0, pre_blur=0, post_blur=0, canny1=100, canny2=500)
RING_BOX = (slice(50, 112), slice(290, 352))


def spiral(seeds=(True, False), ring=True, w=400, h=200):
    """a rectangular spiral of weak candidates over 3 x 3 tiles of 64 pixels, run from the outside in: rightwards, down,
    LEFTWARDS, UPWARDS, ...; seeds = (strong at its outer end, strong at its inner end); ring: a closed weak square
    that touches no seed -> (image [h, w] one channel, the path's (x, y) points in order)"""
    bg = np.rint(np.arange(w) * 255.0 / (w - 1)).astype(np.int64)
    img = np.repeat(bg[None, :], h, 0)
    x0, y0, x1, y1, step, pts = 8, 8, 190, 190, 12, []
    while x1 - x0 > step and y1 - y0 > step:
        pts += [(x, y0) for x in range(x0, x1)] + [(x1, y) for y in range(y0, y1)]
        pts += [(x, y1) for x in range(x1, x0 + step, -1)] + [(x0 + step, y) for y in range(y1, y0 + step, -1)]
        x0, y0, x1, y1 = x0 + step, y0 + step, x1 - step, y1 - step
    for x, y in pts:
        img[y, x] = bg[x] + 40
    for x, y in (pts[:6] if seeds[0] else []) + (pts[-6:] if seeds[1] else []):
        img[y, x] = bg[x] + 200
    if ring:
        img[60, 300:341] -= 40
        img[100, 300:341] -= 40
        img[61:100, 300] -= 40
        img[61:100, 340] -= 40
    return np.clip(img, 0, 255).astype(np.uint8), pts


def follows(on, pts, miss=4):
    """does the on-set run along the whole path: all but `miss` points have an on-pixel among their 8 neighbours, and
    most of the last ten have"""
    hit = [bool(on[y - 1:y + 2, x - 1:x + 2].any()) for x, y in pts]
    return hit.count(False) <= miss and hit[-10:].count(True) >= 5


# ---- the vote cases (clip_pct 0 on images that hold 0 and 255, or nothing to stretch; no blurs) ------------------------------
VOTE_PARAMS = dict(clip_pct=0.0, pre_blur=0, post_blur=0, canny1=50, canny2=0)


def bar(length, w=100, h=60):
    """a bright bar of `length` columns from the left border, rows 10 .. 19: the edge rows 9 and 19 hold length - 1 and
    `length` pixels"""
    img = np.zeros((h, w), np.uint8)
    img[10:20, :length] = 255
    return img


def diagonal_case(anti):
    """50 x 70: a step along x + y = 44 (anti) or y - x = 7 and a bar whose edge row ties with the step's bin:
    -> (image, the row, its count).  anti: row 31 holds 41 pixels, as many as the 45 degree bin it lands on: rejected.
    Otherwise row 4 holds 47, as many as the 135 degree bin and more than the 45 degree one: kept"""
    c, r0, length, row, count = (44, 22, 45, 31, 41) if anti else (7, 5, 48, 4, 47)
    y, x = np.mgrid[0:70, 0:50]
    img = np.where(((x + y) if anti else (y - x)) >= c, 120, 0)
    img[r0:r0 + 10, :length] += 100
    return img.astype(np.uint8), row, count
