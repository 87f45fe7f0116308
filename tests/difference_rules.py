"""The numpy restatement of brightnessAndContrastAuto (src/cvutil.cpp:578-665) and differenceImage
(src/gui/mediagrouplistwidget.cpp:98-208) as include/cbird_hip.h states them, and the builders of the cases the tests run.
Plain loops or vector code, float32 where the rule says float32, no fused operations (numpy rounds every product and
every sum).  Every output is an integer, so the device is held to this with no tolerance.
tests/test_difference_rules.py holds this file to hand-computed values."""
import numpy as np

F = np.float32
IDENT = np.array([1.0, 0, 0, 0, 1.0, 0])


# ---- stage A: brightnessAndContrastAuto ----------------------------------------------------------------------------------
def gray_view(img):
    """cvtColor BGR2GRAY / BGRA2GRAY on 8-bit data (14-bit fixed point); a one-channel image is its own grey view"""
    img = np.asarray(img)
    if img.ndim == 2 or img.shape[2] == 1:
        return img.reshape(img.shape[:2])
    b, g, r = (img[:, :, k].astype(np.int64) for k in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def histogram(gray):
    return np.bincount(np.asarray(gray).reshape(-1), minlength=256).astype(np.uint32)


def gray_cuts(count, clip_pct):
    """grayLevel (:589-625) on 256 counts"""
    count = np.asarray(count)
    if clip_pct == 0:
        present = np.nonzero(count)[0]
        return (int(present[0]), int(present[-1])) if len(present) else (256, -1)
    acc = [F(count[0])]
    for i in range(1, 256):
        acc.append(F(acc[i - 1] + F(count[i])))
    mx = acc[255]
    clip = F(F(clip_pct) * F(mx / F(100.0)))
    clip = F(clip / F(2.0))
    lo = 0
    while lo < 256 and acc[lo] < clip:
        lo += 1
    hi = 255
    upper = F(mx - clip)
    while hi >= 0 and acc[hi] >= upper:
        hi -= 1
    return lo, hi


def stretch_table(lo, hi):
    """stretchContrast (:628-655) as a table of the 256 byte values"""
    s = np.arange(256)
    if lo >= hi:
        return s.astype(np.uint8)
    alpha = F(255.0) / F(hi - lo)
    beta = F(F(-lo) * alpha)
    prod = (s.astype(F) * alpha).astype(F)
    t = np.rint((prod + beta).astype(F))  # half to even
    return np.clip(t, 0, 255).astype(np.uint8)


def auto_contrast(img, clip_pct):
    """-> (stretched image: every byte of every channel, (min_gray, max_gray), histogram)"""
    img = np.asarray(img, np.uint8)
    hist = histogram(gray_view(img))
    lo, hi = gray_cuts(hist, clip_pct)
    return stretch_table(lo, hi)[img], (lo, hi), hist


# ---- stage B: differenceImage ------------------------------------------------------------------------------------------
def rgb32(img):
    """the B, G, R planes of convertToFormat(Format_RGB32): grey replicated, alpha dropped"""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2 or img.shape[2] == 1:
        return np.repeat(img.reshape(img.shape[0], img.shape[1], 1), 3, axis=2)
    return img[:, :, :3]


def warp_matrix(tx, has_tx=True):
    """None when the pair is not warped, else the matrix canvas -> right image (the identity for a singular tx)"""
    if tx is None or not has_tx:
        return None
    t = np.asarray(tx, np.float64).reshape(6)
    if np.array_equal(t, IDENT):
        return None
    det = t[0] * t[4] - t[1] * t[3]
    return IDENT.copy() if det == 0.0 else t


def sample_coords(m, lw, lh):
    x = (np.arange(lw, dtype=np.float64) + 0.5)[None, :]
    y = (np.arange(lh, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(all="ignore"):
        fx = (m[0] * x + m[1] * y) + m[2]
        fy = (m[3] * x + m[4] * y) + m[5]
    return fx, fy


def assert_floor_unambiguous(m, lw, lh):
    """no sample coordinate within 2^-30 of an integer: floor is the same however the f64 products are ordered"""
    for f in sample_coords(m, lw, lh):
        assert np.abs(f - np.rint(f)).min() > 2.0 ** -30


def warp_canvas(right_bgr, m, lw, lh):
    rh, rw = right_bgr.shape[:2]
    fx, fy = sample_coords(m, lw, lh)
    with np.errstate(all="ignore"):
        sx, sy = np.floor(fx), np.floor(fy)
        inside = (sx >= 0) & (sx < rw) & (sy >= 0) & (sy < rh)
    ix = np.where(inside, sx, 0).astype(np.int64)
    iy = np.where(inside, sy, 0).astype(np.int64)
    out = right_bgr[iy, ix]
    out[~inside] = 0
    return out


def scale_nearest(img, dw, dh):
    sh, sw = img.shape[:2]
    ys = ((2 * np.arange(dh) + 1) * sh) // (2 * dh)
    xs = ((2 * np.arange(dw) + 1) * sw) // (2 * dw)
    return img[ys][:, xs]


def colour(s):
    """(b, g, r) of one squared distance (:199-203)"""
    s = np.asarray(s, np.int64)
    return (s & 31) << 3, ((s >> 5) & 31) << 3, ((s >> 10) << 1) & 255


def difference_image(left, right, tx=None, has_tx=True, clip_pct=5):
    """-> (picture uint8 [h, w, 4] BGRA, the record as a dict)"""
    l, r = rgb32(left), rgb32(right)
    lh, lw = l.shape[:2]
    m = warp_matrix(tx, has_tx)
    if m is not None:
        r = warp_canvas(r, m, lw, lh)
    ln, lcut, _ = auto_contrast(l, clip_pct)  # (the grey view of the replicated grey is the grey itself)
    rn, rcut, _ = auto_contrast(r, clip_pct)
    if rn.shape[0] * rn.shape[1] < lh * lw:
        rn = scale_nearest(rn, lw, lh)
    else:
        ln = scale_nearest(ln, rn.shape[1], rn.shape[0])
    d = ln.astype(np.int64) - rn.astype(np.int64)
    s = (d * d).sum(axis=2)
    b, g, rr = colour(s)
    pic = np.stack([b, g, rr, np.full_like(b, 255)], axis=2).astype(np.uint8)
    rec = dict(sum_total=int(s.sum()), sum_max=int(s.max()), n_ge32=int((s >= 32).sum()), n_ge1024=int((s >= 1024).sum()),
               w=s.shape[1], h=s.shape[0], warped=int(m is not None), left_min=lcut[0], left_max=lcut[1],
               right_min=rcut[0], right_max=rcut[1])
    return pic, rec


# ---- case builders -----------------------------------------------------------------------------------------------------
def textured(w, h, seed, ch=3):
    """smooth structure plus noise, full range"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 90 * np.sin(x * 0.37 + seed) * np.cos(y * 0.23) + 30 * np.sin((x + 2 * y) * 0.11)
    img = base[:, :, None] + rng.integers(-25, 26, (h, w, 3)) + np.array([0, 12, -9])
    img = np.clip(img, 0, 255).astype(np.uint8)
    return as_channels(img, ch, seed)


def as_channels(bgr, ch, seed=0):
    """a BGR base image as 1 (its green plane), 3 or 4 channels (a random alpha that must take no part in a difference)"""
    bgr = np.asarray(bgr, np.uint8)
    if ch == 3:
        return bgr.copy()
    if ch == 1:
        return bgr[:, :, 1].copy()
    a = np.random.default_rng(seed + 77).integers(0, 256, bgr.shape[:2] + (1,), dtype=np.uint8)
    return np.concatenate([bgr, a], axis=2)


def contrast_cases(ch, block_pixels=4096):
    """name -> image for stage A: degenerate sides, widths around the 16-pixel and 64-lane boundaries, an image above one
    workgroup's portion, a constant image and one with two grey levels"""
    c = {}
    for k, (w, h) in enumerate([(1, 1), (37, 1), (1, 37), (15, 5), (16, 5), (17, 5), (63, 3), (64, 3), (65, 3)]):
        c[f"{w}x{h}"] = textured(w, h, 10 + k, ch)
    side = int(np.ceil(np.sqrt(block_pixels))) + 9
    c["two_blocks"] = textured(side, side + 3, 31, ch)
    c["constant"] = np.full((6, 9) if ch == 1 else (6, 9, ch), 77, np.uint8)
    two = np.where(np.arange(7 * 11).reshape(7, 11) % 3 == 0, 40, 200).astype(np.uint8)
    c["two_levels"] = two if ch == 1 else np.repeat(two[:, :, None], ch, axis=2)
    dim = (textured(21, 13, 5, ch) // 4 + 60).astype(np.uint8)  # a narrow range: the stretch does something
    c["narrow_range"] = dim
    return c


def rot(deg, scale, cx, cy, tx, ty):
    """rotation by deg and scale about (cx, cy), then a shift"""
    a = np.deg2rad(deg)
    c, s = scale * np.cos(a), scale * np.sin(a)
    return np.array([c, -s, cx - c * cx + s * cy + tx, s, c, cy - s * cx - c * cy + ty])


def pair_groups(block_pixels=4096):
    """Each group: one left image and its right images with their transforms (None = no transform given), as BGR base
    images -- the tests turn them into 1, 3 or 4 channels.  `general` lists the pairs whose coordinates are not dyadic."""
    g = []
    # -- the size rule and the colour extremes, no transforms
    L = textured(23, 17, 1)
    brighter = np.clip(L.astype(int) // 2 + 40, 0, 255).astype(np.uint8)  # the same picture up to brightness and contrast
    chk = np.where((np.add.outer(np.arange(17), np.arange(23)) % 2) == 0, 0, 255).astype(np.uint8)
    chk = np.repeat(chk[:, :, None], 3, axis=2)
    g.append(dict(name="sizes", left=L, rights=[L.copy(), brighter, textured(10, 7, 2), textured(31, 29, 3),
                                                textured(17, 23, 4), textured(1, 1, 5), textured(64, 2, 6)], tx=None))
    g.append(dict(name="extremes", left=chk, rights=[255 - chk, chk.copy()], tx=None))
    g.append(dict(name="10x2_vs_4x6", left=textured(10, 2, 7), rights=[textured(4, 6, 8)], tx=None))
    g.append(dict(name="1x1_vs_7x5", left=textured(1, 1, 9), rights=[textured(7, 5, 10)], tx=None))
    g.append(dict(name="equal_areas", left=textured(6, 4, 11), rights=[textured(4, 6, 12), textured(8, 3, 13)], tx=None))
    # -- transforms with dyadic entries on a 24 x 18 canvas and a 30 x 22 right image; -1 marks has_tx = 0
    L = textured(24, 18, 20)
    R = textured(30, 22, 21)
    txs = [IDENT,                                   # identity with has_tx set: no warp, so the sides are scaled
           [1, 0, 3, 0, 1, 2],                      # integer translation
           [1, 0, 2.5, 0, 1, -1.5],                 # half-pixel translation
           [0, -1, 20, 1, 0, 1],                    # 90 degrees
           [-1, 0, 27, 0, -1, 20],                  # 180 degrees
           [0.5, 0, 0, 0, 0.5, 0], [2, 0, 0, 0, 2, 0],
           [1, 0, 20, 0, 1, 10],                    # the canvas partly covered
           [1, 0, 1000, 0, 1, 1000],                # not covered at all
           [0, 0, 5, 0, 0, 5],                      # determinant 0: drawn unscaled at the origin
           [2, 4, 1, 1, 2, 3],                      # determinant 0 again, no zero entry
           [3, 1, 4, 1, 5, 9]]                      # has_tx = 0: ignored
    has = [1] * 11 + [0]
    g.append(dict(name="dyadic", left=L, rights=[R.copy() for _ in txs], tx=np.array(txs, np.float64), has=has))
    # -- two general rotations, on images above one workgroup's portion, in a batch with unwarped pairs
    side = int(np.ceil(np.sqrt(block_pixels))) + 7
    L = textured(side + 5, side, 30)
    R = textured(side + 11, side + 2, 31)
    txs = [rot(17, 1.0, side / 2, side / 2, 2.3, -1.7), IDENT, rot(-133, 1.3, side / 2, side / 2, 0.4, 3.1), IDENT]
    g.append(dict(name="general", left=L, rights=[R, R.copy(), R.copy(), textured(40, 30, 32)],
                  tx=np.array(txs, np.float64), has=[1, 0, 1, 1], general=[0, 2]))
    return g


def group_in_channels(grp, lch, rch):
    """(left, rights) of a group in the given channel counts"""
    return as_channels(grp["left"], lch, 1), [as_channels(r, rch, 2 + i) for i, r in enumerate(grp["rights"])]


def model_group(left, rights, grp, clip_pct=5):
    """[(picture, record)] of a group from the model; asserts the margin of the general pairs first"""
    out = []
    for i, r in enumerate(rights):
        tx = None if grp.get("tx") is None else grp["tx"][i]
        has = True if grp.get("has") is None else bool(grp["has"][i])
        if i in grp.get("general", ()):
            assert_floor_unambiguous(warp_matrix(tx, has), left.shape[1], left.shape[0])
        out.append(difference_image(left, r, tx, has, clip_pct))
    return out
