"""Images for ColorDescriptor::create on the device (cbird_amd/csrc/colordesc_create.hip) whose SAMPLE COUNT is chosen, not
found: every sum in the kernels is an ordered floating-point chain over an image's N samples, so the places where they
can go wrong are the values of N at the edges of their loops, and the places an image takes inside a wave that carries G
of them (k_cdw_round<G>, G = 1, 2, 4, 8, 16, 21).  Fixtures only -- the tests are tests/test_color_create_shapes.py.

    lit(cols, rows, N, ...)   a black image with exactly N lit pixels inside the oracle's ellipse mask: N samples
    RAGGED                    47 images (odd; a partly filled last wave for every G > 1): every edge N, two palettes, four
                              geometries, placed so that invalid images and the one large image meet the lanes that matter
    ALL_INVALID               21 black images, then 5 valid ones: at G = 21 the first wave has nmax == 0
    rotations(cases, G)       the list at three offsets, so every image meets other lane groups and other neighbours
    want(case)                the oracle's (descriptor or None, stage), computed once per image

The loops of k_cdw_round<G> (kTRow tiles of 64 samples, quarter rows of 16):
    the sum   runs over N elements:      a tile with >= 64 left takes the unmasked branch, the last one the masked tail
    the walk  runs over N - 1 elements:  64-element tiles, 16-element quarters subtracted blind, one quarter re-walked
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np

K = 32            # clusters; an image with fewer samples has no descriptor ("not enough colors")
GROUPS = (1, 2, 4, 8, 16, 21)   # the instantiations of k_cdw_round<G>
DESC_BYTES = 258
CHUNK_MB_DEFAULT = 32768        # "color_create_chunk_mb" as shipped

# N -> why it is in the list
EDGE_N = {
    0: "all black: no sample at all",
    31: "one short of valid",
    32: "the minimum; the walk visits 31 elements (two quarters, the second one short by one)",
    33: "the walk visits exactly two quarters (32 elements); the sum two quarters + one element",
    48: "the sum ends on a quarter edge; the walk one short of it (47)",
    49: "the walk ends on a quarter edge (48); the sum one past it",
    63: "the sum one short of a tile (masked tail of 63, odd end of the float2 reads); the walk 62",
    64: "the sum exactly one tile (unmasked branch only); the walk 63, one short of a tile",
    65: "the walk exactly one tile; the sum one tile + a tail of ONE element",
    66: "the walk one tile + one element; the sum one tile + one whole float2",
    80: "the sum one tile + exactly one quarter; the walk one short of that",
    81: "the walk one tile + exactly one quarter; the sum one past",
    113: "off every edge: one tile + 49 (sum) / + 48 (walk: three whole quarters)",
    127: "the sum one short of two tiles; the walk 126",
    128: "the sum exactly two tiles; the walk 127",
    129: "the walk exactly two tiles; the sum two tiles + 1",
    130: "the walk two tiles + 1; the sum two tiles + one float2",
    192: "three tiles (sum) / one short (walk)",
    193: "three tiles (walk) / one past (sum)",
    256: "four tiles (sum) / one short (walk)",
    257: "four tiles (walk) / one past (sum)",
    1000: "15 tiles + 40 (sum) / + 39 (walk); 250 float4 blocks for k_cdw_update / k_cdw_freq",
    1025: "16 tiles + 1 (sum) / exactly 16 tiles (walk); 257 float4 blocks, the last holding one sample",
}


@dataclass(eq=False)   # identity, not value: want() caches by the object
class Case:
    name: str
    img: np.ndarray      # uint8 [rows, cols, 3], BGR, read-only
    cols: int
    rows: int
    N: int               # samples the oracle must report
    palette: str         # "spread" | "few" | "grey" | "random" | "photo" | "black"

    @property
    def valid(self) -> bool:
        return self.N >= K


@functools.cache
def oracle():
    from oracle import ColorCreateOracle

    return ColorCreateOracle()


_FEW = np.array([(40, 90, 200), (250, 60, 60), (50, 240, 45), (128, 128, 128), (255, 255, 255)], np.uint8)
_BASES = np.random.default_rng(1234).integers(48, 248, (40, 3))


def lit(cols: int, rows: int, N: int, palette: str = "spread", seed: int = 0) -> Case:
    """All black, no resize (both sides <= 256), exactly N pixels lit among those the oracle's ellipse mask keeps, chosen by
    a seeded generator and taken in raster order.  Every lit channel is >= 40, far above the L > 4 cut; black has L = 0
    and is dropped.  "spread": ~40 base colours +- 8 jitter (32 well separated seeds exist).  "few": 5 exact colours --
    fewer distinct colours than clusters: duplicate seeds, sum0 == 0, p == 0 walks that must stop at element 0, tied
    trial sums where the first must win, empty clusters for k_cdw_post."""
    assert 1 <= cols <= 256 and 1 <= rows <= 256
    rng = np.random.default_rng([cols, rows, N, seed, {"spread": 0, "few": 1}[palette]])
    inside = np.flatnonzero(oracle().ellipse_mask(cols, rows).reshape(-1) == 255)
    assert N <= len(inside), (cols, rows, N, len(inside))
    at = np.sort(rng.choice(inside, N, replace=False))
    if palette == "few":
        colours = _FEW[rng.integers(0, len(_FEW), N)]
        if N >= len(_FEW):
            colours[rng.permutation(N)[: len(_FEW)]] = _FEW   # every one of the five is there
    else:
        colours = (_BASES[rng.integers(0, len(_BASES), N)] + rng.integers(-8, 9, (N, 3))).clip(40, 255).astype(np.uint8)
    img = np.zeros((rows * cols, 3), np.uint8)
    img[at] = colours
    return _case(f"lit{cols}x{rows}-{N}-{palette}-{seed}", img.reshape(rows, cols, 3), N, palette if N else "black")


def _case(name, img, N, palette) -> Case:
    img = np.ascontiguousarray(img, np.uint8)
    img.setflags(write=False)
    return Case(name, img, img.shape[1], img.shape[0], N, palette)


def grey_15_16(cols: int = 64, rows: int = 48, pixels: int = 400) -> Case:
    """`pixels` lit pixels, alternately grey 15 and grey 16: 16 is the first grey level the L > 4 rule keeps, so half of
    them are samples -- all of one colour, and the cut itself is in the batch"""
    inside = np.flatnonzero(oracle().ellipse_mask(cols, rows).reshape(-1) == 255)
    at = np.sort(np.random.default_rng(15).choice(inside, pixels, replace=False))
    img = np.zeros((rows * cols, 3), np.uint8)
    img[at[0::2]] = 15
    img[at[1::2]] = 16
    return _case(f"grey15_16-{pixels}", img.reshape(rows, cols, 3), pixels // 2, "grey")


def whole(cols: int, rows: int, seed: int) -> Case:
    """every pixel random with channels >= 40: as many samples as the mask has pixels"""
    img = np.random.default_rng([cols, rows, seed]).integers(40, 256, (rows, cols, 3), dtype=np.uint8)
    return _case(f"whole{cols}x{rows}-{seed}", img, int((oracle().ellipse_mask(cols, rows) == 255).sum()), "random")


def photo(w: int, h: int, seed: int, blocks: int = 40) -> Case:
    """random BGR with flat rectangles, as tests/test_color_create.py's _photo makes them; N is whatever survives L > 4
    (asked of the oracle here: the one fixture whose count is found, not made)"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for _ in range(blocks):
        x, y = int(rng.integers(0, max(1, w - 4))), int(rng.integers(0, max(1, h - 4)))
        img[y: y + int(rng.integers(3, max(4, h // 3))), x: x + int(rng.integers(3, max(4, w // 3)))] = \
            rng.integers(0, 256, 3)
    return _case(f"photo{w}x{h}-{seed}", img, oracle().create(img)[1][2], "photo")


@functools.cache
def big() -> Case:
    return whole(256, 192, 0)   # every pixel of the mask: 31543 samples, 493 tiles -- the other images of its wave have n far below nmax


@functools.cache
def ragged() -> list:
    """RAGGED.  Places (asserted by test_ragged_order, from the list and G):
      invalid images at 0, 7, 20, 41 -- slot 0 of a wave for every G; the last slot for G = 4 and 8 (7) and for G = 21
      (20, 41); a middle slot for G = 4 (41), G = 8 (20, 41) and G = 21 (7)
      the 256 x 192 image at 1, N = 32 at 2: from G = 4 on one wave holds an invalid image, the longest and the shortest"""
    pal = ("spread", "few")
    edge = [lit(64, 48, N, pal[i % 2]) for i, N in enumerate(sorted(EDGE_N))]   # 23: N = 0, 31, 32, ... 1025
    by_n = {c.N: c for c in edge}
    # the fill: edge N again with the other palette (and another choice of pixels)
    fill_n = (0, 31, 33, 49, 63, 64, 65, 66, 81, 113, 127, 128, 129, 193, 257, 1000, 48, 80, 1025)
    fill = [lit(64, 48, N, pal[1 - sorted(EDGE_N).index(N) % 2], seed=1) for N in fill_n]
    extra = [grey_15_16(), whole(16, 12, 1), whole(16, 12, 2), photo(100, 100, 8)]
    order = [None] * 47
    order[0], order[7], order[20], order[41] = by_n[0], by_n[31], fill[0], fill[1]
    order[1], order[2] = big(), by_n[32]
    order[46] = fill[-1]   # the odd image out of k_cdw_update / k_cdw_freq's pairs: "few", 257 float4 blocks
    rest = [c for c in edge if c.N not in (0, 31, 32)] + extra + fill[2:-1]
    # interleave so that neighbours differ in N by much (a lane's n well below its wave's nmax) -- a fixed shuffle
    rest = [rest[i] for i in np.random.default_rng(47).permutation(len(rest))]
    free = [i for i, c in enumerate(order) if c is None]
    assert len(free) == len(rest), (len(free), len(rest))
    for i, c in zip(free, rest):
        order[i] = c
    return order


@functools.cache
def all_invalid() -> list:
    black = [lit(64, 48, 0, seed=s) for s in range(21)]
    return black + [lit(64, 48, N, p, seed=2) for N, p in ((32, "few"), (64, "spread"), (65, "few"), (129, "spread"),
                                                            (1000, "few"))]


def __getattr__(name):   # RAGGED / ALL_INVALID are built on first use (they need the oracle's mask)
    if name == "RAGGED":
        return ragged()
    if name == "ALL_INVALID":
        return all_invalid()
    raise AttributeError(name)


def rotations(cases, G: int) -> list:
    """the list rotated by 0, ceil(G / 3) and ceil(2 G / 3): three places in a wave of G for every image"""
    out = []
    for r in dict.fromkeys((0, -(-G // 3), -(-2 * G // 3))):
        r %= len(cases)
        out.append(list(cases[r:]) + list(cases[:r]))
    return out


def wave_slots(n: int, G: int):
    """(wave, slot, images in that wave) of image i in a batch of n at G images per wave, as k_cdw_round<G> places them"""
    return [(i // G, i % G, min(G, n - i // G * G)) for i in range(n)]


_WANT: dict = {}


def want(case: Case):
    """the oracle's (descriptor [258] uint8 or None, (cols, rows, samples, k-means iterations)) -- once per image: a
    descriptor does not depend on the batch the image is in"""
    hit = _WANT.get(id(case))
    if hit is None:
        hit = _WANT[id(case)] = (case, *oracle().create(case.img))
    return hit[1], hit[2]


def want_arrays(cases):
    """(descs uint8 [n, 258] -- zeros where there is none --, ok uint8 [n]) as the device must return them"""
    d = np.zeros((len(cases), DESC_BYTES), np.uint8)
    ok = np.zeros(len(cases), np.uint8)
    for i, c in enumerate(cases):
        w, _ = want(c)
        if w is not None:
            d[i], ok[i] = w, 1
    return d, ok


# ---- calling the library ---------------------------------------------------------------------------------------------
def pack(imgs, pad: int = 0, fill: int = 255):
    """images [h, w, ch] -> (buffer, offsets u64, w u32, h u32, row strides u32): rows `pad` bytes longer than w * ch, the
    padding (and the gaps between images) filled with `fill`"""
    ch = imgs[0].shape[2]
    w = np.array([im.shape[1] for im in imgs], np.uint32)
    h = np.array([im.shape[0] for im in imgs], np.uint32)
    stride = (w * np.uint32(ch) + np.uint32(pad)).astype(np.uint32)
    sizes = stride.astype(np.uint64) * h.astype(np.uint64)
    off = np.zeros(len(imgs), np.uint64)
    off[1:] = np.cumsum((sizes[:-1] + np.uint64(15)) // np.uint64(16) * np.uint64(16))
    buf = np.full(int(off[-1] + sizes[-1]), fill, np.uint8)
    for im, o, s in zip(imgs, off, stride):
        rows = buf[int(o): int(o) + im.shape[0] * int(s)].reshape(im.shape[0], int(s))
        rows[:, : im.shape[1] * ch] = im.reshape(im.shape[0], -1)
    return buf, off, w, h, stride


def run_host(L, packed, ch: int = 3):
    """cbh_color_descriptors on a packed batch -> (descs uint8 [n, 258], ok uint8 [n])"""
    buf, off, w, h, stride = packed
    n = len(off)
    descs, ok = np.full((n, DESC_BYTES), 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
    rc = L.cbh_color_descriptors(buf.ctypes.data, buf.size, n, off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                 stride.ctypes.data, ch, descs.ctypes.data, ok.ctypes.data, 0)
    assert rc == 0, rc
    return descs, ok


def run_dev(L, packed, ch: int = 3):
    """cbh_color_descriptors_dev: pixels, descriptors and flags in torch tensors on the device"""
    import torch

    buf, off, w, h, stride = packed
    n = len(off)
    d_img = torch.from_numpy(buf).cuda()
    d_descs = torch.full((n, DESC_BYTES), 0xEE, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.cbh_color_descriptors_dev(d_img.data_ptr(), n, off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                     stride.ctypes.data, ch, d_descs.data_ptr(), d_ok.data_ptr(), 0, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return d_descs.cpu().numpy(), d_ok.cpu().numpy()


def tuning(L, key: bytes) -> int:
    v = C.c_longlong(-1)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0, key
    return int(v.value)
