"""Reflection search on the device (SearchParams::mirrorMask; Engine::query / Engine::mirrored, src/engine.cpp:357-365,
423-436): cbh_gray_views_dev and cbh_index_images_views make the index data of an image's reflections from one upload.
Each view must be what cbh_index_images makes of the image flipped on the host, byte for byte; the grey planes and the
hash are also held against the C restatements in oracle/; and database.query / query_batch find flipped copies."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLAGS = (0, 1, 2, 4)  # identity, left-right, top-bottom, both


def flip(img, flag):
    """QImage::mirrored(h, v) of [h, w] or [h, w, c]"""
    if flag in (1, 4):
        img = img[:, ::-1]
    if flag in (2, 4):
        img = img[::-1]
    return np.ascontiguousarray(img)


def frames(n, h, w, ch, seed):
    """photo-like frames; the odd ones letterboxed / pillarboxed with bars of unequal size, so that autocrop keeps a
    different region in every view"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = []
    for i in range(n):
        pal = rng.integers(40, 256, (5, 3)).astype(np.float32)
        img = pal[0] * 0.7 + (35 * np.sin(xx / rng.uniform(5, 60) + i) * np.cos(yy / rng.uniform(5, 60)))[..., None]
        for _ in range(12):  # rectangles of any size down to a pixel, anywhere
            x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
            img[y0:y0 + int(rng.integers(1, w // 2 + 2)), x0:x0 + int(rng.integers(1, w // 2 + 2))] = pal[int(rng.integers(1, 5))]
        img = np.clip(img + rng.normal(0, 3, img.shape), 0, 255).astype(np.uint8)
        if i % 2:
            t, b = h // 7, h // 19
            l, r = w // 11, w // 29
            img[:t], img[h - b:], img[:, :l], img[:, w - r:] = 0, 0, 0, 0
        out.append(img)
    a = np.stack(out)
    if ch == 1:
        return np.ascontiguousarray(a.mean(axis=3).astype(np.uint8))
    if ch == 4:
        return np.ascontiguousarray(np.concatenate([a, rng.integers(0, 256, a.shape[:3] + (1,), dtype=np.uint8)], 3))
    return a


def padded(imgs, row_pad, img_pad):
    """the batch in a buffer with row_pad bytes after every row and img_pad after every image"""
    n, h, w = imgs.shape[:3]
    ch = 1 if imgs.ndim == 3 else imgs.shape[3]
    rs, ist = w * ch + row_pad, h * (w * ch + row_pad) + img_pad
    buf = np.full(n * ist, 0xA5, np.uint8)
    for i in range(n):
        v = buf[i * ist:i * ist + h * rs].reshape(h, rs)
        v[:, :w * ch] = imgs[i].reshape(h, w * ch)
    return buf, rs, ist


def run(buf, n, w, h, rs, ist, ch, mask, algos=15, autocrop=20, cap=464):
    """cbh_index_images (mask None) or cbh_index_images_views on a raw buffer: every output array"""
    from cbird_amd import _lib
    from cbird_amd.colordesc import COLOR_DTYPE
    from cbird_amd.orb import KP_DTYPE
    from cbird_amd.scanner import _Params

    L = _lib.lib()
    V = 1 if mask is None else 1 + bin(mask).count("1")
    nr = n * V
    out = [np.zeros(nr, np.uint64), np.zeros((nr, 4), np.int32), np.zeros((nr, 2), np.int32), np.zeros(nr, np.uint32),
           np.zeros((nr, cap), KP_DTYPE), np.zeros((nr, cap, 32), np.uint8), np.zeros(nr, np.uint32),
           np.zeros((nr, cap), np.uint64), np.zeros(nr, COLOR_DTYPE), np.zeros(nr, np.uint8)]
    p = _Params(autocrop, algos, 400, 400, cap)
    ptrs = [a.ctypes.data for a in out]
    if mask is None:
        rc = L.cbh_index_images(buf.ctypes.data, n, w, h, rs, ist, ch, C.byref(p), *ptrs, 0)
    else:
        rc = L.cbh_index_images_views(buf.ctypes.data, n, w, h, rs, ist, ch, mask, C.byref(p), *ptrs, 0)
    _lib.check(rc, "index")
    assert int(out[3].max()) <= cap
    for i, c in enumerate(out[3]):  # (descriptor rows past a list's end are left as the device buffer had them)
        out[5][i, c:] = 0
    return out


NAMES = ("hash", "rects", "resized dims", "kp counts", "keypoints", "descriptors", "kp hash counts", "kp hashes",
         "colour descriptor", "colour ok")


def same_rows(got, row, want, wrow, what):
    for name, g, w_ in zip(NAMES, got, want):
        assert g[row].tobytes() == w_[wrow].tobytes(), f"{what}: {name} differs"


# (h, w, channels): odd sizes and widths = 1, 2, 3 mod 4
SHAPES = [(29, 37, 3), (299, 401, 1), (480, 640, 4), (721, 1283, 3), (64, 66, 4), (120, 203, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}x{s[2]}")
def test_views_equal_the_pipeline_on_host_flipped_images(gpu, shape):
    from cbird_amd import orb

    orb.set_pattern(orb.synthetic_pattern())
    h, w, ch = shape
    n = 2 if w > 1000 else 3
    imgs = frames(n, h, w, ch, seed=w)
    # the views from a padded buffer (row_stride > w * ch, img_stride > h * row_stride)
    buf, rs, ist = padded(imgs, row_pad=5 + (w % 3), img_pad=13)
    want = {f: run(np.stack([flip(im, f) for im in imgs]).reshape(-1), n, w, h, w * ch, h * w * ch, ch, None) for f in FLAGS}
    for mask in range(8):
        got = run(buf, n, w, h, rs, ist, ch, mask)
        flags = [0] + [f for f in (1, 2, 4) if mask & f]
        for i in range(n):
            for v, f in enumerate(flags):
                same_rows(got, i * len(flags) + v, want[f], i, f"{w}x{h}x{ch} mask {mask} image {i} view {f}")
    # the letterboxed frame (bars of unequal size, so every view crops other pixels) was cropped in every view
    if h > 100:
        got = run(buf, n, w, h, rs, ist, ch, 7)
        assert all(tuple(got[1][1 * 4 + v]) != (0, 0, w, h) for v in range(4))
    # mask 0 is cbh_index_images on the same buffer, every array
    got0, plain = run(buf, n, w, h, rs, ist, ch, 0), run(buf, n, w, h, rs, ist, ch, None)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got0, plain))


def test_process_images_views_matches_process_images(gpu):
    from cbird_amd import orb
    from cbird_amd.scanner import IndexParams, process_images, process_images_views

    orb.set_pattern(orb.synthetic_pattern())
    imgs = frames(3, 97, 131, 3, seed=4)
    p = IndexParams(algos=15)
    views = process_images_views(imgs, 5, p)
    assert [sorted(v) for v in views] == [[0, 1, 4]] * 3
    for f in (0, 1, 4):
        want = process_images(np.stack([flip(im, f) for im in imgs]), p)
        for v, r in zip(views, want):
            g = v[f]
            assert g.dctHash == r.dctHash and g.cropRect == r.cropRect and g.resizedDims == r.resizedDims
            assert g.keyPoints.tobytes() == r.keyPoints.tobytes()
            assert g.keyPointHashes.tobytes() == r.keyPointHashes.tobytes()
            assert g.keyPointDescriptors.tobytes() == r.keyPointDescriptors.tobytes()
            assert (g.colorDescriptor is None) == (r.colorDescriptor is None)
            if r.colorDescriptor is not None:
                assert g.colorDescriptor.tobytes() == r.colorDescriptor.tobytes()
    with pytest.raises(ValueError):
        process_images_views(imgs, 8, p)


def test_view_hashes_equal_the_oracle_on_flipped_grey_images(gpu, orc):
    """grey input, autocrop off, algos = 1: every view's hash is dctHash64 (oracle/cbird_oracle.c) of the flipped image"""
    for h, w in ((33, 45), (240, 321), (128, 128)):
        imgs = frames(3, h, w, 1, seed=h)
        got = run(imgs.reshape(-1), 3, w, h, w, w * h, 1, 7, algos=1, autocrop=-1)[0]
        for i in range(3):
            for v, f in enumerate(FLAGS):
                assert int(got[i * 4 + v]) == orc.dcthash64(flip(imgs[i], f)), (h, w, i, f)


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_gray_views_dev_equal_the_oracle_through_torch_memory(gpu, ch):
    """cbh_gray_views_dev on torch device memory (padded strides): the grey planes equal PrestageOracle.bgr2gray (the
    restatement tests/test_prestage.py holds the device grey image against) of the flipped image, the colour views the
    flipped image itself"""
    import torch

    from cbird_amd import _lib
    from oracle import PrestageOracle

    po = PrestageOracle()
    L = _lib.lib()
    for (h, w), mask in (((37, 29), 7), ((299, 401), 6), ((64, 640), 1), ((17, 1283), 3)):
        n = 3
        imgs = frames(n, h, w, 3, seed=w + ch) if ch != 1 else frames(n, h, w, 1, seed=w)
        if ch == 4:
            imgs = np.concatenate([imgs, np.full(imgs.shape[:3] + (1,), 7, np.uint8)], 3)
        buf, rs, ist = padded(imgs, row_pad=3, img_pad=(ch * 5) % 16 + 1)
        flags = [0] + [f for f in (1, 2, 4) if mask & f]
        V = len(flags)
        d_src = torch.from_numpy(buf).cuda()
        d_gray = torch.full((n * V, h, w), 0x5A, dtype=torch.uint8, device="cuda")
        d_col = torch.full((n * (V - 1), h, w, ch), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = L.cbh_gray_views_dev(d_src.data_ptr(), n, w, h, rs, ist, ch, mask, d_gray.data_ptr(), d_col.data_ptr(), 0,
                                  None)
        assert rc == 0
        torch.cuda.synchronize()
        gray, col = d_gray.cpu().numpy(), d_col.cpu().numpy()
        for i in range(n):
            for v, f in enumerate(flags):
                fl = flip(imgs[i], f)
                want = fl if ch == 1 else po.bgr2gray(fl)
                assert (gray[i * V + v] == want).all(), (h, w, ch, mask, i, f)
                if v:
                    assert (col[i * (V - 1) + v - 1].reshape(fl.shape) == fl).all(), (h, w, ch, mask, i, f)


def test_gray_views_dev_rejects_bad_arguments(gpu):
    import torch

    from cbird_amd import _lib

    L = _lib.lib()
    src = torch.zeros(4 * 16 * 16 * 3, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(4 * 4 * 16 * 16, dtype=torch.uint8, device="cuda")
    a = (src.data_ptr(), 4, 16, 16, 48, 768)
    for mask in (-1, 8, 255):
        assert L.cbh_gray_views_dev(*a, 3, mask, dst.data_ptr(), None, 0, None) == _lib.CBH_E_INVAL
    assert L.cbh_gray_views_dev(*a, 3, 7, None, None, 0, None) == _lib.CBH_E_INVAL
    assert L.cbh_gray_views_dev(None, 4, 16, 16, 48, 768, 3, 7, dst.data_ptr(), None, 0, None) == _lib.CBH_E_INVAL
    for ch in (0, 2, 5):
        assert L.cbh_gray_views_dev(*a, ch, 7, dst.data_ptr(), None, 0, None) == _lib.CBH_E_INVAL
    assert L.cbh_gray_views_dev(src.data_ptr(), 4, 16, 16, 47, 768, 3, 7, dst.data_ptr(), None, 0, None) == _lib.CBH_E_INVAL
    assert L.cbh_gray_views_dev(*a, 3, 7, dst.data_ptr(), None, 0, None) == 0
    torch.cuda.synchronize()


def test_index_images_views_rejects_bad_arguments(gpu):
    from cbird_amd import _lib
    from cbird_amd.scanner import _Params

    L = _lib.lib()
    imgs = frames(2, 32, 40, 3, seed=1)
    hashes, rects = np.zeros(8, np.uint64), np.zeros((8, 4), np.int32)
    p = _Params(20, 1, 400, 400, 464)
    z = [None] * 8
    args = lambda mask, ch=3, hp=hashes.ctypes.data: (imgs.ctypes.data, 2, 40, 32, 40 * ch, 40 * 32 * ch, ch, mask, C.byref(p),
                                                     hp, rects.ctypes.data, *z, 0)
    for mask in (-1, 8):
        assert L.cbh_index_images_views(*args(mask)) == _lib.CBH_E_INVAL
    assert L.cbh_index_images_views(*args(7, hp=None)) == _lib.CBH_E_INVAL  # the dct hash output is NULL
    assert L.cbh_index_images_views(*args(7, ch=2)) == _lib.CBH_E_INVAL
    assert L.cbh_index_images_views(*args(7)) == 0


def test_every_allocation_of_the_views_call_may_fail_once(gpu):
    """the fault_alloc_after walk of tests/test_error_paths.py over cbh_index_images_views (all four stages and the
    colour views): every allocation fails once in turn, the call returns CBH_E_NOMEM, the next call is right, and no
    arena block or device memory is left behind"""
    import gc

    from cbird_amd import _lib, orb
    from test_error_paths import _free_bytes, _tuning, _walk

    orb.set_pattern(orb.synthetic_pattern())
    L = _lib.lib()
    imgs = frames(3, 120, 161, 3, seed=9)
    call = lambda: tuple(run(imgs.reshape(-1), 3, 161, 120, 161 * 3, 161 * 120 * 3, 3, 7))
    call()
    _walk(L, call)
    gc.collect()
    live0 = _tuning(L, b"arena_live_blocks")
    free0 = _free_bytes(L)
    failed, absorbed = _walk(L, call)
    assert failed >= 1
    gc.collect()
    assert _tuning(L, b"arena_live_blocks") == live0, "an error path kept an arena block"
    assert _free_bytes(L) >= free0 - (8 << 20)


# ---- search --------------------------------------------------------------------------------------------------------


class Med:
    """the slice of cbird's Media the indexes and database.query read"""

    def __init__(self, id_, path, r):
        self.id, self.path, self.score = id_, path, -1
        self.dctHash = int(r.dctHash)
        self.keyPointHashes = [int(x) for x in r.keyPointHashes]
        self.keyPointDescriptors = np.ascontiguousarray(r.keyPointDescriptors)
        self.colorDescriptor = r.colorDescriptor
        self.videoIndex = None

    def isValid(self):
        return self.id != 0


@pytest.fixture(scope="module")
def library(gpu):
    """12 scenes, a smaller copy of each, the H-, V- and HV-flipped copies of scenes 0..3 and a left-right symmetric
    image; and the views (mask 7) of every scene, as process_images_views gives them for a needle"""
    from cbird_amd import orb
    from cbird_amd.scanner import IndexParams, process_images, process_images_views
    from test_end_to_end import resized, scene

    orb.set_pattern(orb.synthetic_pattern())
    p = IndexParams(algos=15)
    scenes = np.stack([scene(500 + s) for s in range(12)])
    sym = scene(777)
    sym[:, 256:] = sym[:, :256][:, ::-1]
    items = [(f"/lib/s{s:02d}.png", scenes[s]) for s in range(12)]
    items += [(f"/lib/s{s:02d}_small.png", resized(scenes[s], 0.75)) for s in range(12)]
    items += [(f"/lib/s{s:02d}_flip{f}.png", flip(scenes[s], f)) for s in range(4) for f in (1, 2, 4)]
    items += [("/lib/symmetric.png", sym)]
    media = []
    from cbird_amd.scanner import process_image_list

    for k, ((path, _), r) in enumerate(zip(items, process_image_list([im for _, im in items], p))):
        media.append(Med(k + 1, path, r))
    needles = media[:12] + [media[-1]]
    views = process_images_views(np.stack(list(scenes) + [sym]), 7, p)
    return media, needles, views


def make_index(algo, media):
    from cbird_amd import DctFeaturesIndex, DctHashIndex
    from cbird_amd.colordesc import ColorDescIndex
    from cbird_amd.cvfeatures import CvFeaturesIndex

    idx = {0: DctHashIndex, 1: DctFeaturesIndex, 2: CvFeaturesIndex, 3: ColorDescIndex}[algo]()
    if algo == 0:
        idx.load([m.dctHash for m in media], [m.id for m in media])
    elif algo == 1:
        idx.load([(m.id, m.keyPointHashes) for m in media])
    else:
        idx.add(media)
    return idx


def test_flipped_copies_are_found_only_with_mirror_mask(library):
    from cbird_amd import SearchParams
    from cbird_amd.database import query

    media, needles, views = library
    idx = make_index(0, media)
    id_map = {m.id: m for m in media}
    by_path = {m.path: m for m in media}
    for s in range(4):
        needle = copy.copy(needles[s])
        flipped = {f: by_path[f"/lib/s{s:02d}_flip{f}.png"] for f in (1, 2, 4)}
        p0 = SearchParams(algo=0, mirrorMask=0)
        # the data: a flipped copy is farther from the needle than dctThresh, so a plain search cannot find it
        for f, m in flipped.items():
            assert bin(m.dctHash ^ needle.dctHash).count("1") >= p0.dctThresh, (s, f)
        got0 = query(idx, needle, p0, id_map, views[s])
        assert not {m.id for m in flipped.values()} & {m.id for m in got0}
        p7 = SearchParams(algo=0, mirrorMask=7)
        got7 = query(idx, needle, p7, id_map, views[s])
        for f, m in flipped.items():
            d = bin(int(views[s][f].dctHash) ^ m.dctHash).count("1")
            assert d < p7.dctThresh and [x for x in got7 if x.id == m.id and x.score == d], (s, f)
        assert [m.score for m in got7] == sorted(m.score for m in got7)


def test_symmetric_image_finds_itself_through_its_h_view(library):
    from cbird_amd import SearchParams
    from cbird_amd.database import query

    media, needles, views = library
    idx = make_index(0, media)
    id_map = {m.id: m for m in media}
    needle, v = needles[-1], views[-1]
    assert int(v[1].dctHash) == needle.dctHash  # left-right symmetric: the H view hashes like the image
    p = SearchParams(algo=0, filterSelf=True)
    assert needle.id not in [m.id for m in query(idx, needle, p, id_map, v)]
    p.mirrorMask = SearchParams.MirrorHorizontal
    got = query(idx, needle, p, id_map, v)
    assert [m for m in got if m.id == needle.id and m.score == 0]  # the mirrored needle has id 0: filterSelf keeps it


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_query_batch_equals_one_query_per_needle(library, algo):
    import warnings

    from cbird_amd import SearchParams
    from cbird_amd.database import query, query_batch

    media, needles, views = library
    idx = make_index(algo, media)
    id_map = {m.id: m for m in media}
    found = 0
    for kw in (dict(mirrorMask=7), dict(mirrorMask=5, filterSelf=False, maxMatches=3),
               dict(mirrorMask=6, minMatches=2, maxThresh=9), dict(mirrorMask=0, path="/lib/s0", inPath=True)):
        p = SearchParams(algo=algo, **kw)
        got = query_batch(idx, needles, views, p, id_map)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = [query(idx, n, p, id_map, v) for n, v in zip(needles, views)]
        assert [[(m.id, m.score) for m in g] for g in got] == [[(m.id, m.score) for m in g] for g in want], (algo, kw)
        found += sum(len(g) for g in got)
    assert found
