"""The hash tail (stages 3-6: cv::dct, cv::sum, coef > mean) on inputs whose deciding coefficient is EQUAL or ADJACENT to
the threshold in float32 (tests/hash_threshold_cases.py), on every kernel that hosts a tail, exact against the oracle.
cv_dct32_dev.h "must stay operation-for-operation identical" to oracle/cv_dct32.c; one rounding of difference anywhere
in the device's transform or sum flips a bit of these inputs -- tests/test_hash_threshold_model.py measures that a
contracted multiply-add changes a third of them and none of 20 000 random tiles.

Where each kernel's tail is (cbird_amd/csrc): hash_from_tile (one tile per workgroup; sum64_lanes) in k_rect_hashes,
k_kp_hashes and k_tile_hash; hash_halfwave (one tile per half-wave; sum64_halfwave for both halves at once) in
k_dcthash_256_band (4 images per workgroup), k_dcthash_256 (8) and k_tiles_hash2 (2)."""
import numpy as np
import pytest

import hash_threshold_cases as H

pytestmark = pytest.mark.gpu

SEED = 1
N_FILL = 8


@pytest.fixture(scope="module")
def tile_cases(orc):
    """the 32 x 32 cases: every bit 1..63 once, then the keypoint square's tiles -- (tiles u8 [n, 32, 32], hashes u64 [n])"""
    cs = list(H.near_threshold_tiles(SEED)) + list(H.kp_square_case(SEED))
    return np.stack([c.tile for c in cs]), np.array([c.hash for c in cs], np.uint64)


@pytest.fixture(scope="module")
def lifted(orc):
    """the 256 x 256 cases and N_FILL random filler images, with what the oracle makes of them (computed once)"""
    cases, imgs, _ = H.lifted_cases(SEED)
    assert len(cases) >= 48
    fill = np.random.default_rng(SEED + 100).integers(0, 256, (N_FILL, 256, 256), dtype=np.uint8)
    d = dict(imgs=imgs, tiles=np.stack([c.tile for c in cases]), hashes=np.array([c.hash for c in cases], np.uint64),
             fill=fill, fill_tiles=np.stack([orc.tile32(f) for f in fill]), fill_hashes=orc.dcthash64_batch(fill))
    for v in d.values():
        v.setflags(write=False)
    return d


def _tiles_dev(buf, n, w, h, row_stride, img_stride):
    """cbh_dcthash_tiles_dev on n images inside the u8 array buf: (hashes u64 [n], tiles u8 [n, 32, 32])"""
    import torch

    from cbird_amd import _lib

    d = torch.from_numpy(np.ascontiguousarray(buf).reshape(-1)).cuda()
    out = torch.zeros(n, dtype=torch.int64, device="cuda")
    tiles = torch.zeros((n, 32, 32), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().cbh_dcthash_tiles_dev(d.data_ptr(), n, w, h, row_stride, img_stride, out.data_ptr(),
                                                tiles.data_ptr(), 0, None), "tiles")
    return out.cpu().numpy().view(np.uint64), tiles.cpu().numpy()


def _named(bad, hashes_got, hashes_want):
    return [(int(i), hex(int(hashes_got[i] ^ hashes_want[i]))) for i in np.nonzero(bad)[0][:8]]


def test_tiles_as_32x32_images(gpu, tile_cases):
    """launch_dcthash sends w == h == 32 to launch_rect_hashes: k_rect_hashes, one whole-image rectangle per image, copy
    mode (no blur, no resize), then hash_from_tile.  The plain entry and the one that hands the tiles back."""
    tiles, want = tile_cases
    got = gpu.dct_hash64_batch(tiles)
    assert (got == want).all(), _named(got != want, got, want)
    got, back = _tiles_dev(tiles, len(tiles), 32, 32, 32, 1024)
    assert (back == tiles).all()
    assert (got == want).all(), _named(got != want, got, want)


def _pasted(tiles, rng, w=180, h=140):
    """noise images of w x h with the tiles pasted at odd offsets, 15 per image: (images [m, h, w], per image a list of
    (x, y, index of the tile))"""
    spots = [(1 + 34 * i, 3 + 34 * j) for j in range(3) for i in range(5)]
    m = (len(tiles) + len(spots) - 1) // len(spots)
    imgs = rng.integers(0, 256, (m, h, w), dtype=np.uint8)
    where = [[] for _ in range(m)]
    for t, tile in enumerate(tiles):
        x, y = spots[t % len(spots)]
        imgs[t // len(spots), y:y + 32, x:x + 32] = tile
        where[t // len(spots)].append((x, y, t))
    return imgs, where


def test_tiles_as_rectangles_inside_noise(gpu, orc, tile_cases):
    """cbh_dcthash_rects: k_rect_hashes walks an image's rectangles one after the other on the same LDS; each tile is a
    32 x 32 rectangle at an odd offset (rows not 4-byte aligned) of a noise image"""
    from cbird_amd import _lib

    tiles, want = tile_cases
    imgs, where = _pasted(tiles, np.random.default_rng(SEED + 1))
    m, h, w = imgs.shape
    off = (np.arange(m) * (h * w)).astype(np.uint64)
    ww, hh = np.full(m, w, np.uint32), np.full(m, h, np.uint32)
    rects = np.array([[x, y, 32, 32] for per in where for (x, y, _) in per], np.int32)
    first = np.zeros(m + 1, np.uint32)
    first[1:] = np.cumsum([len(per) for per in where])
    out = np.zeros(len(rects), np.uint64)
    _lib.check(_lib.lib().cbh_dcthash_rects(imgs.ctypes.data, imgs.size, m, off.ctypes.data, ww.ctypes.data, hh.ctypes.data,
                                            ww.ctypes.data, rects.ctypes.data, first.ctypes.data, 0, out.ctypes.data, None,
                                            0), "rects")
    order = [t for per in where for (_, _, t) in per]
    assert order == list(range(len(tiles)))
    for i in (0, m - 1):  # the oracle's own walk over the same rectangles agrees with the tiles' hashes
        for (x, y, t) in where[i]:
            assert orc.dcthash64_rect_inplace(imgs[i].copy(), x, y, 32, 32) == int(want[t])
    assert (out == want).all(), _named(out != want, out, want)


def test_tiles_as_keypoint_squares_in_lds(gpu, orc, tile_cases):
    """keypoints of size 32.0 whose squares are the tiles, 15 per image: k_kp_hashes' LDS routine (sides up to
    "kp_lds_side"), copy mode, hash_from_tile once per keypoint on the LDS the per-image loop reuses"""
    from cbird_amd.hashing import make_keypoint_hashes

    tiles, want = tile_cases
    imgs, where = _pasted(tiles, np.random.default_rng(SEED + 2))
    kps = [np.array([[x + 0.25, y + 0.5, 32.0] for (x, y, _) in per], np.float32) for per in where]
    got = make_keypoint_hashes(list(imgs), kps)
    for i, per in enumerate(where):
        w_i = want[[t for (_, _, t) in per]]
        if i in (0, len(where) - 1):
            assert (orc.keypoint_hashes(imgs[i], kps[i])[0] == w_i).all()
        assert len(got[i]) == len(per) and (got[i] == w_i).all(), (i, _named(got[i] != w_i, got[i], w_i))


def _check_256(gpu, lifted, row_stride):
    """every lifted case at every batch index mod 8, between filler images, in batches whose sizes leave the last
    workgroup of 8, 4 and 2 images ragged (n mod 8 = 1, 3, 5, 7 in turn): plain hashes, then hashes and tiles"""
    nc = len(lifted["imgs"])
    sizes = set()
    for s in range(8):
        tail = ((1, 3, 5, 7)[s % 4] - s - nc) % 8
        n = s + nc + tail
        sizes.add(n % 8)
        buf = np.zeros((n, 256, row_stride), np.uint8)
        pick = np.array([(s + j) % N_FILL for j in range(tail)], np.intp)
        buf[:s, :, :256] = lifted["fill"][:s]
        buf[s:s + nc, :, :256] = lifted["imgs"]
        buf[s + nc:, :, :256] = lifted["fill"][pick]
        want = np.concatenate([lifted["fill_hashes"][:s], lifted["hashes"], lifted["fill_hashes"][pick]])
        want_tiles = np.concatenate([lifted["fill_tiles"][:s], lifted["tiles"], lifted["fill_tiles"][pick]])
        got = gpu.dct_hash64_batch(buf[:, :, :256])
        assert (got == want).all(), (s, n, _named(got != want, got, want))
        got, tiles = _tiles_dev(buf, n, 256, 256, row_stride, 256 * row_stride)
        assert (tiles == want_tiles).all(), (s, n)
        assert (got == want).all(), (s, n, _named(got != want, got, want))
    assert sizes == {1, 3, 5, 7}


def test_256_band_kernel(gpu, lifted):
    """default knobs, contiguous 16-byte aligned images: launch_dcthash's 256 x 256 branch with "hash_mfma" != 0 ->
    k_dcthash_256_band<false> / <true> (4 images per 64-lane workgroup, hash_halfwave twice per wave)"""
    _check_256(gpu, lifted, 256)


def test_256_valu_kernel(gpu, lifted):
    """"hash_mfma" 0: the 256 x 256 branch falls to k_dcthash_256<false> / <true> (8 images per 256-lane workgroup,
    hash_halfwave on each of its four waves)"""
    from cbird_amd import _lib

    L = _lib.lib()
    try:
        L.cbh_set_tuning(b"hash_mfma", 0)
        _check_256(gpu, lifted, 256)
    finally:
        L.cbh_set_tuning(b"hash_mfma", 2)


def test_256_rows_not_8_byte_aligned_band_area(gpu, lifted):
    """row stride 260: not the 256 x 256 branch (it wants 8-byte aligned rows) but "every other geometry" -- K = 7, integer
    ratio 8, "hash_band_area" on -> k_band_area<T, RS, true> writes the tiles, k_tiles_hash2 (two tiles per workgroup,
    hash_halfwave) hashes them"""
    _check_256(gpu, lifted, 260)


def test_256_fused_strip_kernel(gpu, lifted):
    """row stride 260 with "hash_band_area" 0, "hash_fuse" 2, "hash_stream" 4: steps = 4, one column strip ->
    k_blur_area_regs<7, GEN, FUSE> (whole image per workgroup, tile made inside) + k_tiles_hash2"""
    from cbird_amd import _lib

    L = _lib.lib()
    try:
        L.cbh_set_tuning(b"hash_band_area", 0)
        L.cbh_set_tuning(b"hash_fuse", 2)
        L.cbh_set_tuning(b"hash_stream", 4)
        _check_256(gpu, lifted, 260)
    finally:
        L.cbh_set_tuning(b"hash_band_area", 1)
        L.cbh_set_tuning(b"hash_fuse", 1)
        L.cbh_set_tuning(b"hash_stream", 1)


def test_256_band_staged_kernel(gpu, lifted):
    """row stride 260 with "hash_band_area" 0, "hash_stream" 0: never strips -> k_blur_area<7> (16-row bands staged in
    LDS, horizontal pass to float rows) + k_tile_hash (vertical pass, then hash_from_tile)"""
    from cbird_amd import _lib

    L = _lib.lib()
    try:
        L.cbh_set_tuning(b"hash_band_area", 0)
        L.cbh_set_tuning(b"hash_stream", 0)
        _check_256(gpu, lifted, 260)
    finally:
        L.cbh_set_tuning(b"hash_band_area", 1)
        L.cbh_set_tuning(b"hash_stream", 1)


def test_keypoint_square_of_256_global_routine(gpu, orc):
    """a keypoint of size 256.0 is larger than "kp_lds_side" (default 134): k_kp_hashes' global-memory routine -- the
    square blurred in place 7 x 7 from the parent's pixels, reduced 8 x 8 -> 1, then hash_from_tile.  All cases in one
    call (one workgroup per image), each followed by a 32-pixel square over the large one's corner, so the workgroup
    goes on to its LDS routine on the pixels the large square's blur left behind."""
    from cbird_amd.hashing import make_keypoint_hashes

    cases = H.kp_square_case(SEED)
    assert len(cases) >= 6
    small = np.array([[1.5, 1.5, 32.0]], np.float32)
    kps = [np.concatenate([c.kp, small]) for c in cases]
    got, after = make_keypoint_hashes([c.image for c in cases], kps, return_images=True)
    for i, c in enumerate(cases):
        want, want_img = orc.keypoint_hashes(c.image, kps[i])
        assert int(want[0]) == c.hash and len(want) == 2
        assert (got[i] == want).all(), (i, c.bit, c.rel, hex(int(got[i][0] ^ want[0])))
        assert (after[i] == want_img).all(), i
