"""The quarter turns and transposes of a needle on the device (SearchParams.turnMask): cbh_turn_views_dev and
cbh_index_images_views_ex make the index data of the four views that swap width and height from the one upload that also
feeds the reflections.  A turn moves bytes and nothing else, so each view must be what cbh_index_images makes of the image
turned on the host, byte for byte; the grey planes and the hash are also held against the C restatements in oracle/; and
database.query / query_batch find turned copies that no dctThresh brings near their original."""
import copy
import ctypes as C

import numpy as np
import pytest

from test_mirror_views import Med, flip, frames, padded, same_rows

pytestmark = pytest.mark.gpu

TURNS = (8, 16, 32, 64)
VIEW_FLAGS = (0, 1, 2, 4) + TURNS


def turn(img, flag):
    """view `flag` of [h, w] or [h, w, c]: the reflections as QImage::mirrored, 8 = QTransform().rotate(90) (clockwise),
    16 = the quarter turn counter-clockwise, 32 = the transpose, 64 = the anti-transpose"""
    if flag < 8:
        return flip(img, flag)
    out = {8: lambda a: np.rot90(a, -1), 16: lambda a: np.rot90(a, 1), 32: lambda a: a.swapaxes(0, 1),
           64: lambda a: np.rot90(a, 2).swapaxes(0, 1)}[flag](img)
    return np.ascontiguousarray(out)


def flags_of(mask):
    return [0] + [f for f in VIEW_FLAGS[1:] if mask & f]


def test_turn_is_the_index_map_of_its_definition():
    """(the helper itself, on the CPU side of this file: out[y', x'] of each flag)"""
    a = np.arange(3 * 5).reshape(3, 5)
    h, w = a.shape
    for f, src in ((8, lambda y, x: a[h - 1 - x, y]), (16, lambda y, x: a[x, w - 1 - y]), (32, lambda y, x: a[x, y]),
                   (64, lambda y, x: a[h - 1 - x, w - 1 - y])):
        t = turn(a, f)
        assert t.shape == (w, h) and all(t[y, x] == src(y, x) for y in range(w) for x in range(h)), f


# ---- the kernel --------------------------------------------------------------------------------------------------------

# (h, w): single rows and columns, one pixel either side of a 64-pixel tile edge, every residue of h and w mod 16 that
# switches between the 16-byte and the byte-wise loads and stores
KERNEL_SHAPES = [(1, 1), (1, 70), (70, 1), (3, 5), (63, 65), (64, 64), (65, 127), (129, 64), (37, 29), (17, 1283)]


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_turn_views_dev_equal_the_turned_image_through_torch_memory(gpu, ch):
    """cbh_turn_views_dev on torch device memory (padded strides): the grey planes equal PrestageOracle.bgr2gray of the
    numpy-turned image (one channel: the turned bytes), the colour views the turned image itself, and nothing is written
    behind the last plane"""
    import torch

    from cbird_amd import _lib
    from oracle import PrestageOracle

    po = PrestageOracle()
    L = _lib.lib()
    n = 2
    for h, w in KERNEL_SHAPES:
        imgs = frames(n, h, w, 3, seed=w + ch) if ch != 1 else frames(n, h, w, 1, seed=w)
        if ch == 4:
            imgs = np.concatenate([imgs, np.full(imgs.shape[:3] + (1,), 7, np.uint8)], 3)
        buf, rs, ist = padded(imgs, row_pad=3, img_pad=(ch * 5) % 16 | 1)
        d_src = torch.from_numpy(buf).cuda()
        want = {f: [turn(im, f) for im in imgs] for f in TURNS}
        want_gray = want if ch == 1 else {f: [po.bgr2gray(t) for t in want[f]] for f in TURNS}
        for mask in (range(8, 128, 8) if (h, w) == (63, 65) else (120, 8)):
            fl = [f for f in TURNS if mask & f]
            T = len(fl)
            d_gray = torch.full((n * T * h * w + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            d_col = torch.full((n * T * h * w * ch + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rc = L.cbh_turn_views_dev(d_src.data_ptr(), n, w, h, rs, ist, ch, mask, d_gray.data_ptr(), d_col.data_ptr(), 0,
                                      None)
            assert rc == 0
            torch.cuda.synchronize()
            gray, col = d_gray.cpu().numpy(), d_col.cpu().numpy()
            assert (gray[-64:] == 0x5A).all() and (col[-64:] == 0x5A).all(), (h, w, ch, mask)
            gray, col = gray[:-64].reshape(n * T, w, h), col[:-64].reshape((n * T, w, h) + imgs.shape[3:])
            for i in range(n):
                for t, f in enumerate(fl):
                    assert (gray[i * T + t] == want_gray[f][i]).all(), (h, w, ch, mask, i, f)
                    assert (col[i * T + t] == want[f][i]).all(), (h, w, ch, mask, i, f)
        # without the colour leg: the same grey planes
        d_gray = torch.full((n * 4 * h * w + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        assert L.cbh_turn_views_dev(d_src.data_ptr(), n, w, h, rs, ist, ch, 120, d_gray.data_ptr(), None, 0, None) == 0
        torch.cuda.synchronize()
        assert (d_gray.cpu().numpy() == gray_all(want_gray, n)).all(), (h, w, ch)


def gray_all(want_gray, n):
    """the planes of mask 120 in the order the call writes them, and the untouched tail"""
    planes = [want_gray[f][i].reshape(-1) for i in range(n) for f in TURNS]
    return np.concatenate(planes + [np.full(64, 0x5A, np.uint8)])


def test_turn_views_dev_rejects_bad_arguments(gpu):
    import torch

    from cbird_amd import _lib

    L = _lib.lib()
    src = torch.zeros(4 * 16 * 16 * 3, dtype=torch.uint8, device="cuda")
    dst = torch.full((4 * 4 * 16 * 16,), 0x5A, dtype=torch.uint8, device="cuda")
    a = (src.data_ptr(), 4, 16, 16, 48, 768)
    for mask in (0, 1, 7, 128, -1):
        assert L.cbh_turn_views_dev(*a, 3, mask, dst.data_ptr(), None, 0, None) == _lib.CBH_E_INVAL
    assert L.cbh_turn_views_dev(*a, 3, 120, None, None, 0, None) == _lib.CBH_E_INVAL
    assert L.cbh_turn_views_dev(None, 4, 16, 16, 48, 768, 3, 120, dst.data_ptr(), None, 0, None) == _lib.CBH_E_INVAL
    for ch in (0, 2, 5):
        assert L.cbh_turn_views_dev(*a, ch, 120, dst.data_ptr(), None, 0, None) == _lib.CBH_E_INVAL
    assert L.cbh_turn_views_dev(src.data_ptr(), 4, 16, 16, 47, 768, 3, 120, dst.data_ptr(), None, 0, None) == _lib.CBH_E_INVAL
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0x5A).all()  # no work was done
    assert L.cbh_turn_views_dev(*a, 3, 120, dst.data_ptr(), None, 0, None) == 0
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0).all()


def test_index_images_views_ex_rejects_bad_arguments(gpu):
    from cbird_amd import _lib
    from cbird_amd.scanner import _Params

    L = _lib.lib()
    imgs = frames(2, 32, 40, 3, seed=1)
    hashes, rects = np.zeros(16, np.uint64), np.zeros((16, 4), np.int32)
    p = _Params(20, 1, 400, 400, 464)
    z = [None] * 8
    args = lambda mask, ch=3, hp=hashes.ctypes.data: (imgs.ctypes.data, 2, 40, 32, 40 * ch, 40 * 32 * ch, ch, mask, C.byref(p),
                                                     hp, rects.ctypes.data, *z, 0)
    for mask in (-1, 128):
        assert L.cbh_index_images_views_ex(*args(mask)) == _lib.CBH_E_INVAL
    assert L.cbh_index_images_views_ex(*args(127, hp=None)) == _lib.CBH_E_INVAL  # the dct hash output is NULL
    assert L.cbh_index_images_views_ex(*args(127, ch=2)) == _lib.CBH_E_INVAL
    assert L.cbh_index_images_views_ex(*args(127)) == 0
    assert L.cbh_index_images_views(*args(8)) == _lib.CBH_E_INVAL  # the reflections' call keeps its range


# ---- the pipeline ------------------------------------------------------------------------------------------------------


def run_ex(buf, n, w, h, rs, ist, ch, mask, algos=15, autocrop=20, cap=464, entry="cbh_index_images_views_ex"):
    """test_mirror_views.run for cbh_index_images_views_ex (mask None: cbh_index_images): every output array"""
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
        rc = getattr(L, entry)(buf.ctypes.data, n, w, h, rs, ist, ch, mask, C.byref(p), *ptrs, 0)
    _lib.check(rc, "index")
    assert int(out[3].max()) <= cap
    for i, c in enumerate(out[3]):  # (descriptor rows past a list's end are left as the device buffer had them)
        out[5][i, c:] = 0
    return out


# (h, w, channels)
SHAPES = [(29, 37, 3), (299, 401, 1), (64, 66, 4), (120, 203, 1), (480, 640, 4)]
N = 3
_cases = {}


def case(shape):
    """the frames of a shape, their padded buffer, and cbh_index_images of each host-turned batch -- made once"""
    if shape not in _cases:
        from cbird_amd import orb

        orb.set_pattern(orb.synthetic_pattern())
        h, w, ch = shape
        imgs = frames(N, h, w, ch, seed=w)
        want = {}
        for f in VIEW_FLAGS:
            t = np.stack([turn(im, f) for im in imgs])
            th, tw = t.shape[1:3]
            want[f] = run_ex(t.reshape(-1), N, tw, th, tw * ch, th * tw * ch, ch, None)
        _cases[shape] = (imgs, padded(imgs, row_pad=5 + (w % 3), img_pad=13), want)
    return _cases[shape]


@pytest.mark.parametrize("mask", [8, 16, 32, 64, 120, 127, 9, 36])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}x{s[2]}")
def test_views_ex_equal_the_pipeline_on_host_turned_images(gpu, shape, mask):
    h, w, ch = shape
    imgs, (buf, rs, ist), want = case(shape)
    got = run_ex(buf, N, w, h, rs, ist, ch, mask)
    flags = flags_of(mask)
    for i in range(N):
        for v, f in enumerate(flags):
            same_rows(got, i * len(flags) + v, want[f], i, f"{w}x{h}x{ch} mask {mask} image {i} view {f}")
    # the barred frame (bars of unequal size, so every view crops other pixels) was cropped in every turned view, which
    # is h wide and w high
    if h > 100:
        for v, f in enumerate(flags):
            if f >= 8:
                assert tuple(got[1][1 * len(flags) + v]) != (0, 0, h, w), (shape, mask, f)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}x{s[2]}")
def test_views_ex_without_turns_is_the_reflections_call(gpu, shape):
    h, w, ch = shape
    imgs, (buf, rs, ist), want = case(shape)
    for mask in range(8):
        got = run_ex(buf, N, w, h, rs, ist, ch, mask)
        old = run_ex(buf, N, w, h, rs, ist, ch, mask, entry="cbh_index_images_views")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, old)), (shape, mask)
    got0, plain = run_ex(buf, N, w, h, rs, ist, ch, 0), run_ex(buf, N, w, h, rs, ist, ch, None)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got0, plain))


def test_view_hashes_equal_the_oracle_on_turned_grey_images(gpu, orc):
    """grey input, autocrop off, algos = 1: every view's hash is dctHash64 (oracle/cbird_oracle.c) of the turned image"""
    for h, w in ((33, 45), (240, 321), (128, 128)):
        imgs = frames(3, h, w, 1, seed=h)
        got = run_ex(imgs.reshape(-1), 3, w, h, w, w * h, 1, 127, algos=1, autocrop=-1)[0]
        for i in range(3):
            for v, f in enumerate(VIEW_FLAGS):
                assert int(got[i * 8 + v]) == orc.dcthash64(turn(imgs[i], f)), (h, w, i, f)


def test_process_images_views_with_turn_mask_matches_process_images(gpu):
    from cbird_amd import orb
    from cbird_amd.scanner import IndexParams, process_images, process_images_views

    orb.set_pattern(orb.synthetic_pattern())
    imgs = frames(3, 97, 131, 3, seed=4)
    p = IndexParams(algos=15)
    views = process_images_views(imgs, 5, p, turn_mask=72)
    assert [list(v) for v in views] == [[0, 1, 4, 8, 64]] * 3
    assert [list(v) for v in process_images_views(imgs, 0, p, turn_mask=16)] == [[0, 16]] * 3
    for f in (0, 1, 4, 8, 64):
        want = process_images(np.stack([turn(im, f) for im in imgs]), p)
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
    for bad in (1, 128, -8):
        with pytest.raises(ValueError):
            process_images_views(imgs, 0, p, turn_mask=bad)


def test_every_allocation_of_the_views_ex_call_may_fail_once(gpu):
    """the fault_alloc_after walk of tests/test_error_paths.py over cbh_index_images_views_ex with all eight views (both
    geometries, all four stages, the reflected and the turned colour views): every allocation fails once in turn, the
    call returns CBH_E_NOMEM, the next call is right, and no arena block or device memory is left behind"""
    import gc

    from cbird_amd import _lib, orb
    from test_error_paths import _free_bytes, _tuning, _walk

    orb.set_pattern(orb.synthetic_pattern())
    L = _lib.lib()
    imgs = frames(3, 120, 161, 3, seed=9)
    call = lambda: tuple(run_ex(imgs.reshape(-1), 3, 161, 120, 161 * 3, 161 * 120 * 3, 3, 127))
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


# ---- search ------------------------------------------------------------------------------------------------------------

LIB_SEED = 11  # a seed for which the precondition of test_turned_copies_are_found_only_with_turn_mask holds


def hamming(a, b):
    return bin(int(a) ^ int(b)).count("1")


def test_turned_copies_are_found_only_with_turn_mask(gpu, orc):
    """24 photo-like frames and, of four of them, one copy per turn flag hashed from the host-turned pixels.  A turned copy
    is far beyond dctThresh from its original, so a plain search cannot find it; with turnMask the view that matches
    finds it at distance 0, and the lists compose as _compose orders them."""
    from cbird_amd import DctHashIndex, SearchParams
    from cbird_amd.database import _compose, mirrored, query, query_batch, similar_to
    from cbird_amd.scanner import IndexParams, process_images, process_images_views
    from oracle import PrestageOracle

    po = PrestageOracle()
    scenes = frames(24, 97, 131, 3, seed=LIB_SEED)
    p = SearchParams(algo=0, dctThresh=5, turnMask=120)
    # the precondition, on the inputs alone: every turn takes an original farther than dctThresh + 3 from itself, and no
    # two originals are that near each other
    far = p.dctThresh + 3
    own = [orc.dcthash64(po.bgr2gray(s)) for s in scenes]
    for s in range(4):
        for f in TURNS:
            assert hamming(own[s], orc.dcthash64(po.bgr2gray(turn(scenes[s], f)))) > far, (s, f)
    assert all(hamming(own[a], own[b]) > far for a in range(24) for b in range(a))

    ip = IndexParams(algos=1, autocrop=False)
    items = [(f"/lib/s{s:02d}.png", r) for s, r in enumerate(process_images(scenes, ip))]
    for f in TURNS:
        res = process_images(np.stack([turn(scenes[s], f) for s in range(4)]), ip)
        items += [(f"/lib/s{s:02d}_turn{f}.png", r) for s, r in enumerate(res)]
    media = [Med(k + 1, path, r) for k, (path, r) in enumerate(items)]
    assert [m.dctHash for m in media[:24]] == own
    by_path = {m.path: m for m in media}
    id_map = {m.id: m for m in media}
    idx = DctHashIndex()
    idx.load([m.dctHash for m in media], [m.id for m in media])
    needles = [copy.copy(m) for m in media[:4]]
    views = process_images_views(scenes[:4], 0, ip, turn_mask=120)

    got = query_batch(idx, needles, views, p, id_map)
    for s in range(4):
        lists = [similar_to(idx, needles[s], p, id_map)]
        for f in TURNS:
            cp = by_path[f"/lib/s{s:02d}_turn{f}.png"]
            assert int(views[s][f].dctHash) == cp.dctHash
            lists.append(similar_to(idx, mirrored(needles[s], views[s][f]), p, id_map))
            assert [m for m in lists[-1] if m.id == cp.id and m.score == 0], (s, f)  # in the list of its own view
            assert [m for m in got[s] if m.id == cp.id and m.score == 0], (s, f)
        assert [(m.id, m.score) for m in got[s]] == [(m.id, m.score) for m in _compose(lists)]
        assert [m.score for m in got[s]] == sorted(m.score for m in got[s])
    one = query(idx, needles[2], p, id_map, views[2])
    assert [(m.id, m.score) for m in one] == [(m.id, m.score) for m in got[2]]

    p0 = SearchParams(algo=0, dctThresh=5, turnMask=0)
    got0 = query_batch(idx, needles, views, p0, id_map)
    for s in range(4):
        copies = {by_path[f"/lib/s{s:02d}_turn{f}.png"].id for f in TURNS}
        assert not copies & {m.id for m in got0[s]}, s
