"""Scanner::processImage for a batch (cbh_index_images, /root/reference/src/scanner.cpp:828-895): the chained device
pipeline equals the stages of the oracle applied one after the other in the reference's order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _images(rng, n, w, h, border):
    imgs = np.zeros((n, h, w, 3), np.uint8)
    for i in range(n):
        img = np.full((h, w, 3), 120, np.int32)
        for _ in range(60):
            x, y = int(rng.integers(0, w - 8)), int(rng.integers(0, h - 8))
            img[y: y + int(rng.integers(6, h // 3)), x: x + int(rng.integers(6, w // 3))] = rng.integers(0, 256, 3)
        img = (img + rng.integers(-4, 5, img.shape)).clip(0, 255)
        if border and i % 2 == 0:   # letterbox: autocrop removes it, every later stage works on the kept region
            img[: 20 + i] = 0
            img[h - 25:] = 0
        imgs[i] = img
    return imgs


@pytest.mark.parametrize("w,h,border", [(480, 360, True), (300, 420, False)])
def test_pipeline_equals_the_stages_in_order(gpu, orc, w, h, border):
    from cbird_amd import orb as gorb
    from cbird_amd.scanner import IndexParams, process_images
    from oracle import ColorCreateOracle, OrbOracle, PrestageOracle

    rng = np.random.default_rng(w)
    imgs = _images(rng, 5, w, h, border)
    pat = gorb.synthetic_pattern(2)
    gorb.set_pattern(pat)
    oo, co, po = OrbOracle(), ColorCreateOracle(), PrestageOracle()
    oo.set_pattern(pat)
    res = process_images(imgs, IndexParams())
    ncrop = 0
    for img, r in zip(imgs, res):
        gray = po.bgr2gray(img)
        hsh, rect = po.process_image(img, 20)
        assert r.dctHash == hsh and r.cropRect == tuple(int(v) for v in rect)
        ncrop += r.cropRect != (0, 0, w, h)
        kept = np.ascontiguousarray(gray[rect[1]: rect[3], rect[0]: rect[2]])
        small = orc.size_longest_side(kept, 400)
        assert r.resizedDims == (small.shape[1], small.shape[0])
        kp = oo.detect(small, 400)
        kp2, desc = oo.compute(small, kp)
        assert len(kp2) > 100 and (r.keyPoints == kp2).all() and (r.keyPointDescriptors == desc).all()
        tri = np.stack([kp2["x"], kp2["y"], kp2["size"]], 1)
        want_h, _ = orc.keypoint_hashes(small, tri)
        assert len(want_h) > 10 and (r.keyPointHashes == want_h).all()
        want_c, _ = co.create(img)
        assert (np.frombuffer(r.colorDescriptor.tobytes(), np.uint8) == want_c).all()
    assert ncrop > 0 or not border
    # fdct alone: the hashes start from the keypoints as DETECTED (no descriptor pass rewrote them)
    only = process_images(imgs[:2], IndexParams(algos=1 << 1))
    for img, r in zip(imgs[:2], only):
        gray = po.bgr2gray(img)
        _, rect = po.process_image(img, 20)
        small = orc.size_longest_side(np.ascontiguousarray(gray[rect[1]: rect[3], rect[0]: rect[2]]), 400)
        kp = oo.detect(small, 400)
        assert (r.keyPoints == kp).all() and r.dctHash == 0 and r.colorDescriptor is None
        want_h, _ = orc.keypoint_hashes(small, np.stack([kp["x"], kp["y"], kp["size"]], 1))
        assert (r.keyPointHashes == want_h).all() and len(r.keyPointDescriptors) == 0


def test_pipeline_grey_input_and_arguments(gpu, orc):
    from cbird_amd import _lib
    from cbird_amd.scanner import IndexParams, process_images

    rng = np.random.default_rng(5)
    grey = rng.integers(0, 256, (3, 200, 260), dtype=np.uint8)
    res = process_images(grey, IndexParams(algos=(1 << 0) | (1 << 3), autocrop=False))
    for img, r in zip(grey, res):
        assert r.dctHash == orc.dcthash64(img) and r.colorDescriptor is None   # "passed a grayscale image"
        assert r.cropRect == (0, 0, 260, 200) and len(r.keyPoints) == 0
    assert process_images(np.zeros((0, 10, 10), np.uint8)) == []
    with pytest.raises(ValueError):
        process_images(np.zeros((2, 10), np.uint8))
    L = _lib.lib()
    assert L.cbh_index_images(None, 1, 4, 4, 4, 16, 1, None, None, None, None, None, None, None, None, None, None, None,
                              0) == _lib.CBH_E_INVAL


@pytest.mark.gpu
def test_large_batches_are_split_over_host_threads_with_the_same_results(gpu):
    """cbh_index_images cuts a batch of >= 1024 images without the colour leg into sub-batches on their own host threads
    and streams (upload of one overlapping the kernels of another): image by image the results of the unsplit calls"""
    from cbird_amd import orb
    from cbird_amd.scanner import IndexParams, process_images

    orb.set_pattern(orb.synthetic_pattern())
    rng = np.random.default_rng(12)
    base = []
    for _ in range(25):
        blocks = rng.integers(20, 256, (8, 10)).astype(np.uint8)
        base.append(np.kron(blocks, np.ones((12, 12), np.uint8)) + rng.integers(0, 5, (96, 120)).astype(np.uint8))
    imgs = np.stack([np.roll(base[i % 25], i // 25, axis=1) for i in range(1100)])
    p = IndexParams(algos=7, numFeatures=60)
    whole = process_images(imgs, p)                       # 1100 images: two sub-batches of 550
    parts = process_images(imgs[:600], p) + process_images(imgs[600:], p)  # both below the splitting size
    assert len(whole) == len(parts) == 1100
    for a, b in zip(whole, parts):
        assert a.dctHash == b.dctHash and a.cropRect == b.cropRect and a.resizedDims == b.resizedDims
        assert (a.keyPoints == b.keyPoints).all() and (a.keyPointDescriptors == b.keyPointDescriptors).all()
        assert (a.keyPointHashes == b.keyPointHashes).all()
    assert sum(len(r.keyPoints) for r in whole) > 1100 * 10


@pytest.mark.gpu
def test_mixed_geometries_are_grouped_and_returned_in_input_order(gpu):
    from cbird_amd import orb
    from cbird_amd.scanner import IndexParams, process_image_list, process_images

    orb.set_pattern(orb.synthetic_pattern())
    rng = np.random.default_rng(21)
    shapes = [(120, 160), (120, 160, 3), (200, 150, 3), (120, 160), (96, 96, 4), (200, 150, 3), (120, 160, 3)]
    imgs = []
    for sh in shapes:
        blocks = rng.integers(20, 256, (sh[0] // 8 + 1, sh[1] // 8 + 1) + sh[2:]).astype(np.uint8)
        rep = (8, 8) + ((1,) if len(sh) == 3 else ())
        imgs.append(np.ascontiguousarray(np.kron(blocks, np.ones(rep, np.uint8))[: sh[0], : sh[1]]))
    p = IndexParams(algos=15, numFeatures=80)
    got = process_image_list(imgs, p)
    assert len(got) == len(imgs)
    for im, r in zip(imgs, got):
        one = process_images(im[None], p)[0]
        assert r.dctHash == one.dctHash and r.cropRect == one.cropRect
        assert (r.keyPoints == one.keyPoints).all() and (r.keyPointDescriptors == one.keyPointDescriptors).all()
        assert (r.keyPointHashes == one.keyPointHashes).all()
        assert (r.colorDescriptor is None) == (one.colorDescriptor is None)
        if r.colorDescriptor is not None:
            assert r.colorDescriptor.tobytes() == one.colorDescriptor.tobytes()
    assert process_image_list([], p) == []


# ---- kept regions: the launch plan shared by the three callers that hash autocropped images (cbh_regions.h) ----------

_W, _H = 160, 120
_WHOLE, _A, _B, _C = (0, 0, _W, _H), (0, 16, _W, _H - 16), (24, 0, _W - 24, _H), (0, 10, _W, _H - 10)


def _framed(rng, rect, channels=None):
    """content inside `rect`, bars of a flat colour within the autocrop range around it"""
    shape = (_H, _W) if channels is None else (_H, _W, channels)
    img = (16 + rng.integers(0, 4, shape)).astype(np.uint8)
    l, t, r, b = rect
    img[t:b, l:r] = rng.integers(60, 256, (b - t, r - l) + shape[2:], dtype=np.uint8)
    img[0, 0] = 16
    return img


def _frames(rng, regions, channels=None):
    from oracle import PrestageOracle

    po = PrestageOracle()
    imgs = np.stack([_framed(rng, r, channels) for r in regions])
    for img, r in zip(imgs, regions):  # the oracle's autocrop keeps what the frame was built to keep
        assert tuple(po.autocrop(img if channels is None else po.bgr2gray(img), 20).tolist()) == r
    return imgs, po


def test_the_three_callers_of_the_kept_region_plan_agree(gpu):
    """process_images, the scanner pipeline and the video indexer (one chunk; chunks of 1) hash the same kept views:
    hashes and rectangles equal one another and the oracle's, on a chunk whose regions change and come back"""
    from cbird_amd import hashing
    from cbird_amd.scanner import IndexParams, process_images
    from cbird_amd.video import VideoIndexer

    regions = [_WHOLE, _A, _A, _B, _WHOLE, _B]
    gray, po = _frames(np.random.default_rng(160), regions)
    assert len(set(regions)) == 3
    want = [po.process_image(g, 20) for g in gray]
    want_h = [int(h) for h, _ in want]
    assert [tuple(int(v) for v in r) for _, r in want] == regions
    assert len(set(want_h)) == len(want_h)
    h1, r1 = hashing.process_images(gray, 20)
    assert [int(x) for x in h1] == want_h and [tuple(r) for r in r1.tolist()] == regions
    res = process_images(gray, IndexParams(algos=1))
    assert [r.dctHash for r in res] == want_h and [r.cropRect for r in res] == regions
    ix = VideoIndexer(threshold=0)
    ix.push(gray)
    assert ix.finish().hashes == want_h
    ix = VideoIndexer(threshold=0)
    for g in gray:
        ix.push(g[None])
    assert ix.finish().hashes == want_h


def _same_result(a, b):
    assert a.dctHash == b.dctHash and a.cropRect == b.cropRect and a.resizedDims == b.resizedDims
    assert (a.keyPoints == b.keyPoints).all() and (a.keyPointDescriptors == b.keyPointDescriptors).all()
    assert (a.keyPointHashes == b.keyPointHashes).all()


def test_pipeline_plans_with_cropping_equal_the_images_alone(gpu):
    """hash, resize, ORB and keypoint hashes of cropped images in one chunk, on both launch plans: runs ([A, A, B, B]:
    two runs, and 1 + 2 odd images is not less than 2) and mode first ([A, B, A, C, A]: A over the chunk, B and C redone).
    Every field equals the same image processed alone, bit for bit"""
    from cbird_amd import orb
    from cbird_amd.scanner import IndexParams, process_images

    orb.set_pattern(orb.synthetic_pattern())
    p = IndexParams(algos=7, numFeatures=40)
    for seed, regions in ((4, [_A, _A, _B, _B]), (5, [_A, _B, _A, _C, _A])):
        imgs, _ = _frames(np.random.default_rng(seed), regions, channels=3)
        got = process_images(imgs, p)
        assert [r.cropRect for r in got] == regions
        for img, r in zip(imgs, got):
            _same_result(r, process_images(img[None], p)[0])
        assert min(len(r.keyPoints) for r in got) > 10 and min(len(r.keyPointHashes) for r in got) > 0
        assert len({r.dctHash for r in got}) == len(got)
