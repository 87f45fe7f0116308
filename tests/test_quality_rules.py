"""CPU suite for qualityScore (src/cimgops.cpp:313-596): two numpy restatements of what include/cbird_hip.h states --
quality_literal() with the reference's loops and its three transposes, for small shapes, and quality_stencil(), the
vectorised form without a transpose -- held against each other and against tests/golden/quality_cimg.npz, which the real
CImg.h produced (tests/golden/gen_golden_quality.py), bit for bit.  quality_stencil() and the cases built here are the
yardstick of the GPU tests (tests/test_quality.py, tests/test_quality_cpp.py)."""
import functools
import os

import numpy as np
import pytest

NO_SCORE = -(1 << 31)
FIELDS = ("h_sum", "v_sum", "h_mean", "v_mean", "h_long", "v_long", "num_edges", "qw", "qh", "score")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quality_cimg.npz")


# ---- the rules ----------------------------------------------------------------------------------------------------------
def crop_dims(w, h):
    """hCrop, vCrop, qw, qh of the inclusive crop (:333-335)"""
    hc, vc = int(w * 0.10), int(h * 0.10)
    return hc, vc, w - 2 * hc + 1, h - 2 * vc + 1


def working_plane(img):
    """the red channel (cv::Mat order: byte 2 of BGR / BGRA, the byte itself for one channel) under the inclusive crop;
    what lies outside the source is 0"""
    a = np.asarray(img, np.uint8)
    red = a if a.ndim == 2 else a[..., 0] if a.shape[2] == 1 else a[..., 2]
    h, w = red.shape
    hc, vc, qw, qh = crop_dims(w, h)
    p = np.zeros((qh, qw), np.uint8)
    src = red[vc: vc + qh, hc: hc + qw]
    p[: src.shape[0], : src.shape[1]] = src
    return p


def mean_and_byte(total, qw, qh, mean_mode="float"):
    """float(double(sum) / ((w-1) * (h-1))) and pixel_t(mean) (:252, :96).  mean_mode "int" is the WRONG integer division,
    kept to show that a case tells the two apart"""
    cnt = (qw - 1) * (qh - 1)
    mean = np.float32(np.float64(total) / np.float64(cnt))
    return mean, (int(total) // cnt if mean_mode == "int" else int(mean)) & 255


def score_of(h_long, v_long, num_edges, qw, qh):
    """:495, :500, :592 in float, every step rounded; no score without edges"""
    if num_edges == 0:
        return NO_SCORE
    elr = np.float32(v_long + h_long) / np.float32(num_edges)
    er = np.float32(num_edges) / np.float32((qw - 2) * (qh - 2))
    return int(np.float32(100) * er + np.float32(100) * elr)


def _no_plane():
    z = np.zeros((0, 0), np.uint8)
    return dict(h_sum=0, v_sum=0, h_mean=np.float32(0), v_mean=np.float32(0), h_long=0, v_long=0, num_edges=0, qw=0, qh=0,
                score=NO_SCORE, plane=z, edge=z, hd=z, vd=z, he=z, ve=z)


# ---- restatement 1: the reference's loops, transposes included -------------------------------------------------------------
def _filter_horizontal(img):
    """makeDiff, the mean, makeEdge and longEdgeCount on the transposed edge map (filterHorizontal, :197-209)"""
    h, w = img.shape
    diff = np.zeros((h, w), np.uint8)
    total = 0
    for y in range(h):
        for x in range(1, w - 1):
            d = abs(int(img[y, x - 1]) - int(img[y, x + 1]))
            total += d
            diff[y, x] = d
    mean, m = mean_and_byte(total, w, h)
    edge = np.zeros((h, w), np.uint8)
    for y in range(h):
        center = int(diff[y, 0]) if diff[y, 0] > m else 0
        right = int(diff[y, 1]) if diff[y, 1] > m else 0
        for x in range(1, w - 1):
            left, center = center, right
            right = int(diff[y, x + 1]) if diff[y, x + 1] > m else 0
            edge[y, x] = 255 if center > left and center > right else 0
    edge_t = np.ascontiguousarray(edge.T)
    count = 0
    for y in range(edge_t.shape[0]):
        run = 0
        for x in range(1, edge_t.shape[1] - 1):
            if edge_t[y, x] != 0:
                run += 1
            else:
                if run > 1:
                    count += 1
                run = 0
    return diff, edge, total, mean, count


def quality_literal(img):
    p = working_plane(img)
    qh, qw = p.shape
    if qw < 3 or qh < 3:
        return _no_plane()
    hd, he, h_sum, h_mean, h_long = _filter_horizontal(p)
    vd_t, ve_t, v_sum, v_mean, v_long = _filter_horizontal(np.ascontiguousarray(p.T))
    vd, ve = np.ascontiguousarray(vd_t.T), np.ascontiguousarray(ve_t.T)
    edge = he | ve
    num_edges = 0
    for y in range(1, qh - 1):
        for x in range(1, qw - 1):
            if edge[y, x]:
                num_edges += 1
    return dict(h_sum=h_sum, v_sum=v_sum, h_mean=h_mean, v_mean=v_mean, h_long=h_long, v_long=v_long, num_edges=num_edges,
                qw=qw, qh=qh, score=score_of(h_long, v_long, num_edges, qw, qh), plane=p, edge=edge, hd=hd, vd=vd,
                he=he, ve=ve)


# ---- restatement 2: stencils, no transpose (the yardstick of the GPU tests) ---------------------------------------------------
def _diff_x(p):
    d = np.zeros(p.shape, np.int32)
    q = p.astype(np.int32)
    d[:, 1:-1] = np.abs(q[:, :-2] - q[:, 2:])
    return d


def _edge_x(d, m):
    c = np.where(d > m, d, 0)
    e = np.zeros(d.shape, bool)
    e[:, 1:-1] = (c[:, 1:-1] > c[:, :-2]) & (c[:, 1:-1] > c[:, 2:])
    return e


def _long_along_y(e):
    """positions t in [3, L-2] of every column with e[t] = 0 and e[t-1], e[t-2] set"""
    n = e.shape[0]
    if n < 5:
        return 0
    return int((~e[3: n - 1] & e[2: n - 2] & e[1: n - 3]).sum())


def quality_stencil(img, mean_mode="float"):
    p = working_plane(img)
    qh, qw = p.shape
    if qw < 3 or qh < 3:
        return _no_plane()
    hd, vd = _diff_x(p), _diff_x(p.T).T
    h_sum, v_sum = int(hd.sum()), int(vd.sum())
    h_mean, mh = mean_and_byte(h_sum, qw, qh, mean_mode)
    v_mean, mv = mean_and_byte(v_sum, qw, qh, mean_mode)
    he, ve = _edge_x(hd, mh), _edge_x(vd.T, mv).T
    h_long, v_long = _long_along_y(he), _long_along_y(ve.T)
    edge = he | ve
    num_edges = int(edge[1:-1, 1:-1].sum())
    u8 = lambda a: np.ascontiguousarray(a).astype(np.uint8)  # noqa: E731
    return dict(h_sum=h_sum, v_sum=v_sum, h_mean=h_mean, v_mean=v_mean, h_long=h_long, v_long=v_long, num_edges=num_edges,
                qw=qw, qh=qh, score=score_of(h_long, v_long, num_edges, qw, qh), plane=p, edge=u8(edge) * np.uint8(255),
                hd=u8(hd), vd=u8(vd), he=u8(he) * np.uint8(255), ve=u8(ve) * np.uint8(255))


def same(a, b, planes=("plane", "edge", "hd", "vd")):
    """every detail field and plane of two results equal, floats by their bits"""
    for f in FIELDS:
        x, y = a[f], b[f]
        if f.endswith("_mean"):
            x, y = np.float32(x).view(np.uint32), np.float32(y).view(np.uint32)
        assert int(x) == int(y), (f, a[f], b[f])
    for k in planes:
        assert a[k].shape == b[k].shape and (a[k] == b[k]).all(), k
    return True


# ---- the cases (shared with the GPU tests) --------------------------------------------------------------------------------------
def source_side(q):
    """the smallest source side >= 10 whose working side is q (the crop is at least 1, so the plane lies inside)"""
    for s in range(10, 4 * q + 40):
        if s - 2 * int(s * 0.10) + 1 == q:
            return s
    raise ValueError(q)


def embed(plane, rng, channels=3):
    """a source image whose working plane is `plane`: random everywhere else, red = byte 2"""
    qh, qw = plane.shape
    w, h = source_side(qw), source_side(qh)
    hc, vc = int(w * 0.10), int(h * 0.10)
    if channels == 1:
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        img[vc: vc + qh, hc: hc + qw] = plane
    else:
        img = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
        img[vc: vc + qh, hc: hc + qw, 2] = plane
    assert (working_plane(img) == plane).all()
    return img


def noise(rng, w, h, channels):
    shape = (h, w) if channels == 1 else (h, w, channels)
    return rng.integers(0, 256, shape, dtype=np.uint8)


def blocky(rng, w, h, channels, cell):
    """cell x cell replicated cells over a little noise: edges that run for several pixels"""
    cells = rng.integers(0, 256, ((h + cell - 1) // cell, (w + cell - 1) // cell)).astype(np.int32)
    red = np.kron(cells, np.ones((cell, cell), np.int32))[:h, :w]
    red = (red + rng.integers(-2, 3, red.shape)).clip(0, 255).astype(np.uint8)
    if channels == 1:
        return red
    img = noise(rng, w, h, channels)
    img[..., 2] = red
    return img


EDGE_COL = 5


def run_plane(rows_with_edge, n=12):
    """an n x n working plane, flat 50 but for a ramp 50 50 120 200 200 in the given rows: hE is set at column EDGE_COL of
    exactly those rows (hd 70 150 80 around it, mean below 70)"""
    p = np.full((n, n), 50, np.uint8)
    for y in rows_with_edge:
        p[y, EDGE_COL] = 120
        p[y, EDGE_COL + 1:] = 200
    return p


def rounding_plane(rng, q=602):
    """a q x q working plane whose hd sum is exactly k * cnt - 1: columns v v 0 0 v v 0 0 ... (hd = v inside a row) with a
    band of noise rows, then single pixels moved until the sum fits.  Returns (plane, k)"""
    v = 140
    p = np.zeros((q, q), np.uint8)
    p[:, (np.arange(q) % 4) < 2] = v
    band = slice(200, 300)
    p[band] = rng.integers(0, 256, (100, q), dtype=np.uint8)
    cnt = (q - 1) * (q - 1)
    cur = int(_diff_x(p).sum())
    k = (cur + cnt // 2) // cnt
    diff = k * cnt - 1 - cur
    rows = [y for y in range(q) if not band.start <= y < band.stop]
    for y in rows:  # a v pixel between two zeros: moving it by d moves two differences by d each
        for x in range(4, q - 3, 4):
            d = int(np.clip(int(diff / 2), -100, 100))
            if d == 0:
                break
            p[y, x] = v + d
            diff -= 2 * d
    for y in rows:  # column 0 takes part in one difference only
        d = int(np.clip(diff, -100, 100))
        p[y, 0] = v + d
        diff -= d
    assert diff == 0 and int(_diff_x(p).sum()) == k * cnt - 1
    return p, k


def strip_plane(rng, qw, qh, strip):
    """blocky noise plus ramp edges along y that break at rows b, b + 1 and b + 2 of every multiple b of `strip`, and the
    same along x at every multiple of 16: runs end on, just behind and two behind every boundary"""
    cells = rng.integers(0, 256, ((qh + 2) // 3, (qw + 2) // 3)).astype(np.int32)
    p = np.kron(cells, np.ones((3, 3), np.int32))[:qh, :qw].astype(np.uint8)
    # (edge columns at 8 mod 16 and edge rows at strip / 2 mod strip: the ramps stay clear of the boundaries they test)
    for k, c in enumerate(range(8, qw - 8, 32)):  # vertical edges: hE runs along y
        rows = np.ones(qh, bool)
        rows[np.arange(k % 3, qh, strip)] = False
        p[rows, c - 3: c] = 40
        p[rows, c] = 120
        p[rows, c + 1: c + 4] = 210
    for k, r in enumerate(range(strip // 2, qh - 8, 2 * strip)):  # horizontal edges: vE runs along x
        cols = np.ones(qw, bool)
        cols[np.arange(k % 3, qw, 16)] = False
        for dy, val in ((-3, 40), (-2, 40), (-1, 40), (0, 120), (1, 210), (2, 210), (3, 210)):
            p[r + dy, cols] = val
    return p


STRIP_ROWS_ASSUMED = 16  # only for the CPU checks here; the GPU test asks the library ("quality_strip_rows")


@functools.lru_cache(maxsize=None)
def cases(strip=STRIP_ROWS_ASSUMED):
    """name -> image: every shape the GPU test lists.  Built once; nobody writes to the arrays."""
    rng = np.random.default_rng(20240607)
    out = {}
    sides = [2, 3, 9, 10, 11, 19, 20]
    for i, w in enumerate(sides):  # every listed side as a width and as a height, all three channel counts in turn
        for j, h in enumerate((sides[(i + 3) % 7], w)):
            ch = (1, 3, 4)[(i + j) % 3]
            out[f"side_{w}x{h}_c{ch}"] = blocky(rng, w, h, ch, 3) if (i + j) % 2 else noise(rng, w, h, ch)
    for i, q in enumerate((15, 16, 17, 63, 64, 65, 257)):  # working widths around the load width
        ch = (3, 4, 1)[i % 3]
        w, h = source_side(q), (23, 37, 12)[i % 3]
        out[f"qw_{q}_c{ch}"] = blocky(rng, w, h, ch, 4) if i % 2 else noise(rng, w, h, ch)
    out["vga_c3"] = blocky(rng, 640, 480, 3, 4)
    out["photo_1600x900_c3"] = blocky(rng, 1600, 900, 3, 4)  # (with the others: more than one piece at a 1 MB budget)
    out["wide_5200x12_c3"] = blocky(rng, 5200, 12, 3, 3)  # more than 256 chunks of 16 pixels in a row
    out["wide_5200x12_c1"] = noise(rng, 5200, 12, 1)
    out["tall_7x300_c3"] = blocky(rng, 7, 300, 3, 3)
    out["flat_300x7_c4"] = blocky(rng, 300, 7, 4, 3)
    out["tall_7x300_c1"] = noise(rng, 7, 300, 1)
    for ch in (1, 3, 4):
        out[f"side1_1x40_c{ch}"] = noise(rng, 1, 40, ch)
        out[f"side1_40x1_c{ch}"] = noise(rng, 40, 1, ch)
        out[f"constant_c{ch}"] = np.full((30, 45) if ch == 1 else (30, 45, ch), 77, np.uint8)
    for ch in (3, 4):  # red constant, green / blue (and alpha) busy
        img = noise(rng, 50, 40, ch)
        img[..., 2] = 131
        out[f"red_constant_c{ch}"] = img
    for cell in (3, 4):
        for ch in (1, 3, 4):
            out[f"blocky{cell}_c{ch}"] = blocky(rng, 90 + 7 * cell + ch, 70 + ch, ch, cell)
    n = 12
    runs = {"run_ends_at_L-2": [n - 4, n - 3, n - 2], "run_from_0": [0, 1], "run_of_2_ends_at_3": [1, 2],
            "run_0_1_2": [0, 1, 2]}
    for name, rows in runs.items():
        p = run_plane(rows, n)
        out[f"{name}_y_c3"] = embed(p, rng, 3)
        out[f"{name}_x_c1"] = embed(np.ascontiguousarray(p.T), rng, 1)
    p, _k = rounding_plane(rng)
    out["rounding_c3"] = embed(p, rng, 3)
    out["strips_c3"] = embed(strip_plane(rng, 481, 10 * strip + 5, strip), rng, 3)
    out["strips_c1"] = embed(strip_plane(rng, 100, 19 * strip + 3, strip), rng, 1)
    for a in out.values():
        a.setflags(write=False)
    return out


def pack_ragged(images, rng, fill=0xA5):
    """one buffer for images of one channel count, the way a caller's memory may look: every other image with an odd base
    offset and rows padded by an odd number of bytes, the others on 16-byte offsets with rows padded to 16 bytes; gaps
    between images; everything that is not a pixel is `fill`.  -> (buf, off u64, w u32, h u32, stride u32)"""
    off, w, h, stride, pos = [], [], [], [], 0
    for i, im in enumerate(images):
        ch = 1 if im.ndim == 2 else im.shape[2]
        row = im.shape[1] * ch
        if i % 2:
            pos += int(rng.integers(0, 40))
            pos |= 1
            st = row + 2 * int(rng.integers(0, 6)) + (row % 2 == 0)  # odd
        else:
            pos = (pos + int(rng.integers(0, 3)) * 16 + 15) // 16 * 16
            st = (row + 15) // 16 * 16 if i % 4 == 0 else row
        off.append(pos), w.append(im.shape[1]), h.append(im.shape[0]), stride.append(st)
        pos += (im.shape[0] - 1) * st + row
    buf = np.full(pos, fill, np.uint8)
    for im, o, st in zip(images, off, stride):
        rows = im.reshape(im.shape[0], -1)
        for y in range(im.shape[0]):
            buf[o + y * st: o + y * st + rows.shape[1]] = rows[y]
    return (buf, np.asarray(off, np.uint64), np.asarray(w, np.uint32), np.asarray(h, np.uint32),
            np.asarray(stride, np.uint32))


def plane_offsets(images):
    """packed offsets of the three diagnostic planes of every image, and the total"""
    sizes = []
    for im in images:
        _, _, qw, qh = crop_dims(im.shape[1], im.shape[0])
        sizes.append(3 * qw * qh if qw >= 3 and qh >= 3 else 0)
    off = np.zeros(len(images), np.uint64)
    off[1:] = np.cumsum(sizes[:-1])
    return off, int(sum(sizes))


def check_result(name, want, score, detail, planes=None):
    """one image's score, detail record (a numpy record or anything indexable by field) and, if given, its three planes
    [3, qh, qw] against a restatement's result: everything equal, floats by their bits"""
    got = {f: detail[f] for f in FIELDS}
    assert int(score) == int(want["score"]) == int(got["score"]), (name, score, want["score"], got["score"])
    assert same(got, want, planes=()), name
    if planes is not None:
        for k, p in zip(("edge", "hd", "vd"), planes):
            assert p.shape == want[k].shape and (p == want[k]).all(), (name, k)


RUN_EXPECT = {"run_ends_at_L-2": 0, "run_from_0": 0, "run_of_2_ends_at_3": 1, "run_0_1_2": 1}


@functools.lru_cache(maxsize=None)
def yardstick(strip=STRIP_ROWS_ASSUMED):
    return {name: quality_stencil(img) for name, img in cases(strip).items()}


def small(name, img):
    return img.shape[0] * img.shape[1] <= 12000


# ---- tests ------------------------------------------------------------------------------------------------------------------
def test_crop_is_inclusive_and_only_red_counts():
    assert crop_dims(640, 480) == (64, 48, 513, 385) and crop_dims(9, 2) == (0, 0, 10, 3) and crop_dims(1, 40)[2] == 2
    img = np.arange(9 * 11 * 3, dtype=np.uint8).reshape(9, 11, 3)
    p = working_plane(img)  # w 11: crop 1, h 9: crop 0 and a blank last row
    assert p.shape == (10, 10) and (p[:9] == img[:, 1:11, 2]).all() and (p[9] == 0).all()
    assert (working_plane(img[..., 2]) == p).all()
    bgra = np.concatenate([img, np.full((9, 11, 1), 200, np.uint8)], axis=2)
    assert (working_plane(bgra) == p).all()


def test_literal_and_stencil_restatements_agree():
    checked = 0
    for name, img in cases().items():
        if small(name, img):
            assert same(quality_literal(img), yardstick()[name]), name
            checked += 1
    assert checked >= 45


def test_cases_cover_what_they_are_for():
    y = yardstick()
    for name, img in cases().items():
        hc, vc, qw, qh = crop_dims(img.shape[1], img.shape[0])
        if name.startswith("side1_"):
            assert min(qw, qh) == 2 and y[name]["score"] == NO_SCORE and y[name]["qw"] == 0
        if name.startswith(("constant", "red_constant")):
            assert y[name]["num_edges"] == 0 and y[name]["score"] == NO_SCORE and y[name]["qw"] == qw
        if name.startswith("qw_"):
            assert qw == int(name.split("_")[1])
        if name.startswith("blocky"):
            assert y[name]["h_long"] > 20 and y[name]["v_long"] > 20 and y[name]["score"] > 0
    assert {a.shape[1] for a in cases().values()} >= {2, 3, 9, 10, 11, 19, 20}
    assert {a.shape[0] for a in cases().values()} >= {2, 3, 9, 10, 11, 19, 20}
    for name, want in RUN_EXPECT.items():
        r = y[name + "_y_c3"]
        rows = {"run_ends_at_L-2": [8, 9, 10], "run_from_0": [0, 1], "run_of_2_ends_at_3": [1, 2], "run_0_1_2": [0, 1, 2]}[name]
        col = np.zeros(12, bool)
        col[rows] = True
        assert ((r["he"][:, EDGE_COL] != 0) == col).all() and not r["he"][:, :EDGE_COL].any(), name
        assert not r["he"][:, EDGE_COL + 1:].any() and r["h_long"] == want, name
        t = y[name + "_x_c1"]
        assert ((t["ve"][EDGE_COL] != 0) == col).all() and t["v_long"] == want, name


def test_rounding_case_tells_float_from_integer_division():
    img = cases()["rounding_c3"]
    r = yardstick()["rounding_c3"]
    cnt = (r["qw"] - 1) * (r["qh"] - 1)
    k = (r["h_sum"] + 1) // cnt
    assert r["h_sum"] == k * cnt - 1 and 120 <= k <= 140
    assert np.float32(np.float64(r["h_sum"]) / np.float64(cnt)) == np.float32(k) and r["h_sum"] // cnt == k - 1
    wrong = quality_stencil(img, mean_mode="int")
    assert wrong["num_edges"] != r["num_edges"] and (wrong["edge"] != r["edge"]).any()  # (every field is compared)


def test_strip_case_puts_runs_across_every_boundary():
    for name, strip in (("strips_c3", STRIP_ROWS_ASSUMED), ("strips_c1", STRIP_ROWS_ASSUMED)):
        check_strip_case(yardstick()[name], strip)


def check_strip_case(r, strip):
    """a counted run ends on, one behind and two behind every strip boundary (rows) and every 16-column boundary"""
    he, ve = r["he"] != 0, r["ve"] != 0
    qh, qw = he.shape
    assert qh > 2 * strip
    ev = np.zeros(he.shape, bool)
    ev[3: qh - 1] = ~he[3: qh - 1] & he[2: qh - 2] & he[1: qh - 3]
    for b in range(strip, qh - 3, strip):
        assert ev[b].any() and ev[b + 1].any() and ev[b + 2].any(), b
    ex = np.zeros(ve.shape, bool)
    ex[:, 3: qw - 1] = ~ve[:, 3: qw - 1] & ve[:, 2: qw - 2] & ve[:, 1: qw - 3]
    for b in range(16, qw - 3, 16):
        assert ex[:, b].any() and ex[:, b + 1].any() and ex[:, b + 2].any(), b
    assert r["h_long"] == int(ev.sum()) and r["v_long"] == int(ex.sum())


def load_golden():
    z = np.load(GOLDEN)
    n = len(z["score"])
    out = []
    for i in range(n):
        g = {f: z[f][i] for f in FIELDS}
        qw, qh = int(g["qw"]), int(g["qh"])
        for k in ("plane", "edge", "hd", "vd"):
            o = int(z[k + "_off"][i])
            g[k] = z[k][o: o + qw * qh].reshape(qh, qw)
        o, (h, w, c) = int(z["image_off"][i]), z["image_shape"][i]
        g["image"] = z["image"][o: o + h * w * c].reshape(h, w, c)
        out.append(g)
    return out


def test_both_restatements_equal_the_real_cimg():
    gold = load_golden()
    assert 20 <= len(gold) <= 40
    scored = 0
    for i, g in enumerate(gold):
        assert same(quality_stencil(g["image"]), g), i
        if g["image"].shape[0] * g["image"].shape[1] <= 12000:
            assert same(quality_literal(g["image"]), g), i
        scored += g["score"] != NO_SCORE
    assert scored >= 20
    assert os.path.getsize(GOLDEN) < 600 * 1024


@pytest.mark.parametrize("wh", [(1, 1), (1, 50), (2, 2), (9, 9), (10, 10), (640, 480), (65535, 3)])
def test_dims_helper_of_the_library_follows_the_rule(wh):
    from cbird_amd.quality import quality_dims

    _, _, qw, qh = crop_dims(*wh)
    assert quality_dims(*wh) == ((qw, qh) if qw >= 3 and qh >= 3 else (0, 0))
