"""Seeded builders of hash inputs whose deciding coefficient sits ON the threshold (CPU only, through the oracle).

Stages 3-6 of dctHash64 set bit k = coef[k] > thr, with coef from cv::dct's float evaluation and thr from cv::sum's
grouping (oracle/cv_dct32.c).  A device tail that rounds one operation differently -- a contracted multiply-add, a
reordered butterfly, another summation order -- moves coef[k] - thr by a few ulps, which shows in a hash only when the
two are within those ulps of each other.  Random images practically never are (NOTES.md, "Hash: PARITY UNPINNED").
The tiles built here are: for every bit 1..63 a 32 x 32 tile whose float32 coef[k] and thr, in oracle variant 1, are
EQUAL or ADJACENT floats.

  near_threshold_tiles(seed)   the tiles, with bit and relation
  lift_to_256(case, seed)      a 256 x 256 image whose blurred, area-resized tile is exactly that tile
  kp_square_case(seed)         the same for a 256-pixel keypoint square inside a 300 x 300 image (in-place blur that
                               reads the parent around the square)

Construction of a tile.  coef[k] - thr is linear in the pixels; G[k] (impulse_responses) is its exact float64
response to +1 on each pixel.  From the family tile whose float64 margin for bit k is smallest, (1) coarse single-pixel
steps of at most +-3 grey levels on the pixels with the largest response bring the margin below 0.02, (2) all sums
+-G[p] +- G[q] over untouched pixel pairs are searched, sorted, for the ones that cancel what is left -- there are some
two million of them within +-0.12, far denser than float32's spacing at thr -- and (3) since the float32 evaluation's own
rounding error (~1e-4) is a hundred times that spacing, the candidates around the float64 solution are run through the
oracle until one lands where it is wanted: ordered-int distance 0, +1 or -1.

Construction of an image.  The 7 x 7 blur window of each of the four centre pixels of an 8 x 8 source cell lies inside
the cell, so +-49 on such a pixel changes all 49 blurred values it reaches by exactly +-1 and the cell's block sum by
exactly +-49 -- no other cell notices.  (In the cells along the image's edge the border reflection reaches rows and
columns 1..3 a second time, so those cells have two usable centre pixels, the corner cells one.)  The base image (the tile, enlarged, plus noise, pulled towards the tile by a few
rounds of "add what is missing to the whole cell") is finished off that way, cell by cell, and confirmed through
orc.tile32.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

# tile: u8 [32, 32]; bit: 1..63; rel: ordered-int distance of float32 coef[bit] from thr in oracle variant 1
# (0: equal, the bit must be 0; +1: the next float above, bit 1; -1: the next float below, bit 0); hash: the oracle's
TileCase = namedtuple("TileCase", "tile bit rel hash")
# image: u8 [300, 300]; kp: float32 [1, 3] (x, y, 256.0); tile / bit / rel / hash as above
KpCase = namedtuple("KpCase", "image kp tile bit rel hash")

PIX_LO, PIX_HI = 20, 235    # every tile pixel stays inside
FAM_LO, FAM_HI = 72, 184    # the family's own range (the +-3 of the coarse steps stay far inside PIX_LO..PIX_HI)
IMG_LO, IMG_HI = 55, 200    # base images: one +-49 step of a centre pixel is always possible
MAX_DEV = 3                 # coarse steps: grey levels per pixel
COARSE_DONE = 0.02
N_FAMILY = 256              # family tiles a seed draws to pick each bit's base from
N_EVAL = 1500               # candidates run through the float32 oracle per base tile before giving up on it
CENTRE = ((3, 3), (3, 4), (4, 3), (4, 4))


@functools.lru_cache(maxsize=1)
def _orc():
    from oracle import Oracle

    return Oracle()


def dct_matrix(n=32):
    k = np.arange(n)[:, None]
    j = np.arange(n)[None, :]
    return np.sqrt(np.where(k == 0, 1.0, 2.0) / n) * np.cos(np.pi * (2 * j + 1) * k / (2 * n))


@functools.lru_cache(maxsize=1)
def impulse_responses():
    """G float64 [64, 32, 32]: G[k, r, c] = what +1 on tile pixel (r, c) adds to coef[k] - thr in exact arithmetic
    (thr = the mean of the 64 selected coefficients)"""
    zz = _orc().zigzag81()
    C = dct_matrix()
    B = np.stack([np.outer(C[int(z) // 9], C[int(z) % 9]) for z in zz[6:70]])
    G = B - B.mean(axis=0, keepdims=True)
    G.setflags(write=False)
    return G


def family_tiles(rng, n):
    """n smooth-plus-noise 32 x 32 tiles, u8 in FAM_LO..FAM_HI: three low-frequency cosine products + white noise"""
    y = (2 * np.arange(32) + 1)[None, :, None]
    x = (2 * np.arange(32) + 1)[None, None, :]
    t = np.full((n, 32, 32), 128.0)
    for _ in range(3):
        u = rng.integers(0, 5, (n, 1, 1))
        v = rng.integers(0, 5, (n, 1, 1))
        a = rng.uniform(8, 22, (n, 1, 1))
        t += a * np.cos(np.pi * y * u / 64 + rng.uniform(0, 6.3, (n, 1, 1))) * np.cos(
            np.pi * x * v / 64 + rng.uniform(0, 6.3, (n, 1, 1)))
    t += rng.normal(0, 6, (n, 32, 32))
    return np.clip(np.rint(t), FAM_LO, FAM_HI).astype(np.uint8)


def ordered_int(x):
    """float32 -> the integer whose order and spacing are the floats' (adjacent floats differ by 1; +0 == -0)"""
    i = int(np.float32(x).view(np.int32))
    return i if i >= 0 else -(i & 0x7FFFFFFF)


def coef_thr_distance(orc, tile, bit, variant=1):
    """(ordered-int distance of coef[bit] from thr, hash, any bit set before the 0 -> 1 rule) in a float variant"""
    h, co, th = orc.hash_from_tile32_v(tile, variant, with_coefs=True)
    th = np.float32(th)  # (handed over as a Python float: exact)
    return ordered_int(co[bit]) - ordered_int(th), h, bool((co[1:] > th).any())


def _search_bit(orc, base, bit, want):
    """tiles near `base` (u8 [32, 32]) with coef[bit] at ordered-int distance d from thr for the d in `want` that can be
    found: {d: (tile, hash)}"""
    g = impulse_responses()[bit].reshape(-1)
    t = base.astype(np.int64).reshape(-1).copy()
    m = float(g @ t)
    touched = np.zeros(1024, bool)
    for p in np.argsort(-np.abs(g)):  # (1) coarse: the strongest pixels first
        if abs(m) < COARSE_DONE:
            break
        a = int(np.clip(np.rint(-m / g[p]), -MAX_DEV, MAX_DEV))
        a = int(np.clip(t[p] + a, PIX_LO, PIX_HI) - t[p])
        if a:
            t[p] += a
            m += a * g[p]
            touched[p] = True
    if abs(m) >= COARSE_DONE:
        return {}
    coarse = t.astype(np.uint8).reshape(32, 32)
    # from here on the margin as the float32 evaluation has it at this tile (its offset from the exact one, ~1e-4, moves
    # little under two +-1 steps): the candidates are centred on cancelling that
    _, co, th = orc.hash_from_tile32_v(coarse, 1, with_coefs=True)
    m = float(co[bit]) - th
    # (2) pairs of untouched pixels, +-1 each: vals[i] + vals[j] ~ -m
    free = np.nonzero(~touched & (t > PIX_LO) & (t < PIX_HI))[0]
    pix = np.concatenate([free, free])
    sgn = np.concatenate([np.ones(len(free), np.int64), -np.ones(len(free), np.int64)])
    vals = sgn * g[pix]
    order = np.argsort(vals, kind="stable")
    sv = vals[order]
    pos = np.searchsorted(sv, -m - vals)
    ii, jj = [], []
    for o in range(-4, 4):
        j = np.clip(pos + o, 0, len(sv) - 1)
        ii.append(np.arange(len(vals)))
        jj.append(order[j])
    ii, jj = np.concatenate(ii), np.concatenate(jj)
    keep = pix[ii] < pix[jj]  # a pair once, two different pixels
    ii, jj = ii[keep], jj[keep]
    res = np.abs(vals[ii] + vals[jj] + m)
    pick = np.argsort(res, kind="stable")[:N_EVAL]
    found = {}
    for c in pick:  # (3) through the float32 oracle
        cand = t.copy()
        cand[pix[ii[c]]] += sgn[ii[c]]
        cand[pix[jj[c]]] += sgn[jj[c]]
        tile = cand.astype(np.uint8).reshape(32, 32)
        d, h, any_bit = coef_thr_distance(orc, tile, bit)
        if d in want and d not in found and any_bit:
            tile.setflags(write=False)  # (the builders' results are cached and shared between tests)
            found[d] = (tile, h)
            if len(found) == len(want):
                break
    return found


def _cases_from_bases(orc, bases, bits):
    """one case per bit in `bits`, relations taken in turn (0, +1, -1) where the search offers the choice"""
    flat = bases.reshape(len(bases), -1).astype(np.float64)
    G = impulse_responses()
    out = []
    for n_done, bit in enumerate(bits):
        margins = np.abs(flat @ G[bit].reshape(-1))
        pref = (0, 1, -1)[n_done % 3]
        got = None
        for b in np.argsort(margins, kind="stable")[:8]:  # another base tile until the bit has its case
            found = _search_bit(orc, bases[b], bit, (0, 1, -1))
            if found:
                d = pref if pref in found else sorted(found, key=abs)[0]
                got = TileCase(found[d][0], int(bit), int(d), int(found[d][1]))
                if pref in found:
                    break
        if got is None:
            raise RuntimeError(f"no tile within one ulp of the threshold for bit {bit}: try another seed")
        out.append(got)
    return out


@functools.lru_cache(maxsize=4)
def near_threshold_tiles(seed):
    """list of TileCase, one per bit 1..63 in bit order, about a third each with coef == thr, coef the next float above
    thr and the next float below (at least 8 of each, or RuntimeError); pixel values in PIX_LO..PIX_HI; no tile is one
    whose bits are all zero.  The same seed gives the same bytes."""
    orc = _orc()
    rng = np.random.default_rng([int(seed), 0x7e57])
    bases = family_tiles(rng, N_FAMILY)
    cases = _cases_from_bases(orc, bases, range(1, 64))
    for d in (0, 1, -1):
        if sum(c.rel == d for c in cases) < 8:
            raise RuntimeError(f"fewer than 8 cases at distance {d}: try another seed")
    return cases


def _block_sums(a):
    return a.astype(np.int64).reshape(32, 8, 32, 8).sum(axis=(1, 3))


def _centre_steps(img, x0, y0, sums, target, rng):
    """finish a 256 x 256 square at (x0, y0) of `img` (modified in place) whose blurred 8 x 8 block sums are `sums`, so
    that rint(sum / 64) == target in every cell: +-49 steps on the cells' centre pixels.  False if a cell has no room."""
    have = np.rint(sums / 64.0).astype(np.int64)
    for r, c in zip(*np.nonzero(have != target)):
        ks = [k for k in sorted(range(-16, 17), key=abs) if np.rint((sums[r, c] + 49 * k) / 64.0) == target[r, c]]
        if not ks:
            return False
        k = ks[0]
        step = 49 if k > 0 else -49
        # (at the image's own edge REFLECT_101 counts rows / columns 1..3 and their mirror images twice in the outermost
        # windows: there only the centre pixels that no reflection reaches will do)
        H, W = img.shape
        cells = [CENTRE[i] for i in rng.permutation(4)]
        cells = [(dy, dx) for (dy, dx) in cells if 4 <= y0 + 8 * r + dy <= H - 5 and 4 <= x0 + 8 * c + dx <= W - 5]
        left = abs(k)
        while left:
            moved = False
            for (dy, dx) in cells:  # the next centre pixel, round and round
                y, x = y0 + 8 * r + dy, x0 + 8 * c + dx
                if left and 0 <= int(img[y, x]) + step <= 255:
                    img[y, x] += step
                    left -= 1
                    moved = True
            if not moved:
                return False
    return True


def lift_to_256(case, seed):
    """u8 [256, 256] with orc.tile32(image) == case.tile exactly, or None when the tile cannot be reached (a cell whose
    value the base image's range IMG_LO..IMG_HI does not allow).  `seed` draws the base image's noise and the order of
    the centre pixels; the same (case, seed) gives the same bytes."""
    orc = _orc()
    rng = np.random.default_rng([int(seed), int(case.bit), 0x11f7])
    target = case.tile.astype(np.int64)
    img = np.clip(np.kron(target, np.ones((8, 8), np.int64)) + np.rint(rng.normal(0, 5, (256, 256))).astype(np.int64),
                  IMG_LO, IMG_HI)
    for _ in range(12):  # the blur leaks a cell into its neighbours: add what is missing, cell-wide, until little is
        d = target - orc.tile32(img.astype(np.uint8)).astype(np.int64)
        if np.abs(d).max() <= 1:
            break
        img = np.clip(img + np.kron(d, np.ones((8, 8), np.int64)), IMG_LO, IMG_HI)
    img = img.astype(np.int64)
    sums = _block_sums(orc.box_blur(img.astype(np.uint8), 7))
    if not _centre_steps(img, 0, 0, sums, target, rng):
        return None
    out = img.astype(np.uint8)
    return out if (orc.tile32(out) == case.tile).all() else None


@functools.lru_cache(maxsize=4)
def lifted_cases(seed):
    """(cases that lift, their 256 x 256 images u8 [n, 256, 256], bits that did not lift) for near_threshold_tiles(seed)"""
    cases, imgs, failed = [], [], []
    for c in near_threshold_tiles(seed):
        im = lift_to_256(c, seed)
        if im is None:
            failed.append(c.bit)
        else:
            cases.append(c)
            imgs.append(im)
    imgs = np.stack(imgs)
    imgs.setflags(write=False)
    return cases, imgs, failed


KP_CASES = 12  # the keypoint square's cases: the bits its one base tile is nearest the threshold on


@functools.lru_cache(maxsize=4)
def kp_square_case(seed):
    """list of KpCase: 300 x 300 images with one keypoint of size 256.0 whose square, blurred in place 7 x 7 (the blur
    reads the parent around it) and reduced 8 x 8 -> 1, is a tile with coef[bit] within one ulp of thr.  The base
    tile is the round-half-even block mean of the oracle's in-place-blurred square, checked by hashing it; the
    near-threshold tiles are searched from that tile and reached with centre-pixel steps."""
    orc = _orc()
    rng = np.random.default_rng([int(seed), 0x6b70])
    yy, xx = np.mgrid[0:300, 0:300]
    base = 128 + 40 * np.sin(xx / 31.0 + 0.7) * np.cos(yy / 43.0) + 18 * np.cos((xx + 2 * yy) / 57.0)
    base = np.clip(np.rint(base + rng.normal(0, 5, base.shape)), IMG_LO, IMG_HI).astype(np.uint8)
    kp = np.array([[21.5, 17.25, 256.0]], np.float32)
    x0, y0 = 21, 17
    want, blurred = orc.keypoint_hashes(base, kp)
    assert len(want) == 1
    sums = _block_sums(blurred[y0:y0 + 256, x0:x0 + 256])
    base_tile = np.rint(sums / 64.0).astype(np.uint8)
    if orc.hash_from_tile32(base_tile) != int(want[0]):
        raise RuntimeError("the block mean of the blurred square is not the oracle's tile")
    margins = np.abs(impulse_responses().reshape(64, -1) @ base_tile.reshape(-1).astype(np.float64))
    bits = sorted(int(b) for b in np.argsort(margins[1:], kind="stable")[:KP_CASES] + 1)
    out = []
    for tc in _cases_from_bases(orc, base_tile[None], bits):
        img = base.astype(np.int64)
        if not _centre_steps(img, x0, y0, sums, tc.tile.astype(np.int64), rng):
            continue
        img = img.astype(np.uint8)
        got, _ = orc.keypoint_hashes(img, kp)
        if len(got) == 1 and int(got[0]) == tc.hash:
            img.setflags(write=False)
            out.append(KpCase(img, kp, tc.tile, tc.bit, tc.rel, tc.hash))
    return out
