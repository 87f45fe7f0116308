"""GPU: cbh_demosaic / cbh_edge_maps_dev / cbh_grid_lines_dev against tests/demosaic_rules.py, stage by stage and with no
tolerance: class maps, edge maps, line lists, rectangles.  Host and device entries, a side stream, padded rows, odd
offsets and guard bytes around every output."""
import ctypes as C

import numpy as np
import pytest

import demosaic_rules as M
import difference_rules as R

pytestmark = pytest.mark.gpu
PAD, GUARD = 0x5A, 0xA5
TILE = 64  # the hysteresis tile side and the row-staging width of cbird_amd/csrc/demosaic.hip


def _tuning(L, key):
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0
    return v.value


@pytest.fixture(scope="module")
def lib(gpu):
    from cbird_amd import _lib

    return _lib.lib()


def _ch(im):
    return 1 if im.ndim == 2 else im.shape[2]


def pack_ragged(imgs, seed, gap=40):
    """images with padded rows, gaps and odd offsets; everything that is not a pixel is PAD (tests/test_alignment.py)"""
    rng = np.random.default_rng(seed)
    off, stride, pos = [], [], 1 + 2 * int(rng.integers(0, 4))
    for im in imgs:
        h, w = im.shape[:2]
        st = w * _ch(im) + int(rng.integers(0, 7))
        off.append(pos), stride.append(st)
        pos += st * h + int(rng.integers(0, gap))
    buf = np.full(pos + 32, PAD, np.uint8)
    for im, o, st in zip(imgs, off, stride):
        h, w = im.shape[:2]
        np.lib.stride_tricks.as_strided(buf[o:], (h, w * _ch(im)), (st, 1))[:] = im.reshape(h, w * _ch(im))
    return (buf, np.array(off, np.uint64), np.array([im.shape[1] for im in imgs], np.uint32),
            np.array([im.shape[0] for im in imgs], np.uint32), np.array(stride, np.uint32))


def pack(imgs, ragged_seed):
    from cbird_amd.quality import pack_images

    return pack_images([np.ascontiguousarray(im) for im in imgs]) if ragged_seed is None else pack_ragged(imgs, ragged_seed)


def c_params(p):
    from cbird_amd.demosaic import default_params

    return default_params(**p)


def split_planes(flat, imgs):
    out, at = [], 0
    for im in imgs:
        h, w = im.shape[:2]
        out.append(flat[at:at + w * h].reshape(h, w))
        at += w * h
    return out


def run_dev(L, imgs, p, stream=None, ragged_seed=None, cap=None):
    """the three device entries on one upload -> dict(rc, cls, edges, passes, hor, ver, rects); checks the guards"""
    import torch

    n = len(imgs)
    buf, off, w, h, st = pack(imgs, ragged_seed)
    ch = _ch(imgs[0])
    cp = c_params(p)
    d = torch.from_numpy(buf).cuda()
    total = int((w.astype(np.int64) * h).sum())
    d_e = torch.full((total + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_c = torch.full((total + 64,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = stream.cuda_stream if stream else None
    tabs = (off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, ch, C.addressof(cp))
    passes = C.c_uint32(0)
    rc = L.cbh_edge_maps_dev(d.data_ptr(), n, *tabs, d_e.data_ptr(), d_c.data_ptr(), C.addressof(passes), 0, s)
    torch.cuda.synchronize()
    e, c = d_e.cpu().numpy(), d_c.cpu().numpy()
    assert rc == 0 and (e[total:] == GUARD).all() and (c[total:] == GUARD).all()
    assert (d.cpu().numpy() == buf).all()  # the source is read, never written
    hor, ver = np.full(int(h.sum()) + 8, -7, np.int32), np.full(int(w.sum()) + 8, -7, np.int32)
    hf, vf = np.full(n + 3, 0xDEAD, np.uint32), np.full(n + 3, 0xDEAD, np.uint32)
    rc = L.cbh_grid_lines_dev(d.data_ptr(), n, *tabs, hor.ctypes.data, hf.ctypes.data, ver.ctypes.data, vf.ctypes.data, 0, s)
    assert rc == 0 and (hf[n + 1:] == 0xDEAD).all() and (vf[n + 1:] == 0xDEAD).all()
    assert (hor[hf[n]:] == -7).all() and (ver[vf[n]:] == -7).all()
    cap = 64 * n if cap is None else cap
    rects = np.full(4 * cap + 8, -7, np.int32)
    first = np.full(n + 3, 0xDEAD, np.uint32)
    rc = L.cbh_demosaic_dev(d.data_ptr(), n, *tabs, rects.ctypes.data, cap, first.ctypes.data, 0, s)
    assert (first[n + 1:] == 0xDEAD).all() and (rects[4 * cap:] == -7).all()
    if rc != 0:
        assert (rects == -7).all()
    else:
        assert (rects[4 * first[n]:] == -7).all()
    return dict(rc=rc, cls=split_planes(c, imgs), edges=split_planes(e, imgs), passes=passes.value,
                hor=[hor[hf[i]:hf[i + 1]].tolist() for i in range(n)], ver=[ver[vf[i]:vf[i + 1]].tolist() for i in range(n)],
                rects=[[tuple(r) for r in rects[4 * first[i]:4 * first[i + 1]].reshape(-1, 4).tolist()] for i in range(n)],
                first=first[:n + 1].copy())


def run_host(L, imgs, p, cap=None, ragged_seed=None):
    n = len(imgs)
    buf, off, w, h, st = pack(imgs, ragged_seed)
    cp = c_params(p)
    cap = 64 * n if cap is None else cap
    rects = np.full(4 * cap + 8, -7, np.int32)
    first = np.full(n + 3, 0xDEAD, np.uint32)
    rc = L.cbh_demosaic(buf.ctypes.data, buf.size, n, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data,
                        _ch(imgs[0]), C.addressof(cp), rects.ctypes.data, cap, first.ctypes.data, 0)
    assert (first[n + 1:] == 0xDEAD).all() and (rects[4 * cap:] == -7).all()
    return rc, [[tuple(r) for r in rects[4 * first[i]:4 * first[i + 1]].reshape(-1, 4).tolist()] for i in range(n)], first


_model: dict = {}


def want(img, p):
    """the model's stages and rectangles of an image: worked out once per distinct image and parameter set"""
    key = (img.shape, hash(img.tobytes()), tuple(sorted(p.items())))
    if key not in _model:
        st = M.stages(img, p)
        st["final"] = M.demosaic(img, p)
        _model[key] = st
    return _model[key]


def check_all(what, imgs, p, got):
    for i, im in enumerate(imgs):
        w = want(im, p)
        assert (got["cls"][i] == w["cls"]).all(), (what, i, "classes", np.argwhere(got["cls"][i] != w["cls"])[:4])
        assert (got["edges"][i] == w["edges"]).all(), (what, i, "edges", np.argwhere(got["edges"][i] != w["edges"])[:4])
        assert got["hor"][i] == w["hor"] and got["ver"][i] == w["ver"], (what, i, "lines")
        assert got["rects"][i] == [tuple(r) for r in w["final"]], (what, i, got["rects"][i], w["final"])


def sheets(ch):
    out = [R.as_channels(M.sheet(*layout, seed=1)[0], ch, k) for k, layout in enumerate(M.LAYOUTS)]
    return out + [M.textured_sheet(1, ch), M.textured_sheet(2, ch)]


# ---- stage by stage ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_sheets_equal_the_model_stage_by_stage(lib, ch):
    """the five layouts the model finds every cell of (two staggered: subdivided at 0.95) and two textured sheets with
    long line lists, in one ragged batch on a side stream: sheets that subdivide next to sheets that do not"""
    import torch

    imgs = sheets(ch)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    got = run_dev(lib, imgs, M.DEFAULTS, stream=side, ragged_seed=20 + ch)
    assert got["rc"] == 0
    check_all("dev", imgs, M.DEFAULTS, got)
    if ch == 3:
        for layout, r in zip(M.LAYOUTS, got["rects"]):
            assert M.sheet_meets_condition(r, M.sheet(*layout, seed=1)[1], layout[2])
    rc, rects, first = run_host(lib, imgs, M.DEFAULTS)
    assert rc == 0 and rects == got["rects"] and (first[:len(imgs) + 1] == got["first"]).all()
    rc, rects, first = run_host(lib, imgs, M.DEFAULTS, ragged_seed=40 + ch)  # padded rows, odd offsets, gaps
    assert rc == 0 and rects == got["rects"] and (first[:len(imgs) + 1] == got["first"]).all()


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_small_and_boundary_sizes(lib, ch):
    """a smooth photograph-like image (one rectangle), a flat one, 1 x 1, 1 x 40, 40 x 1, 5 x 7, and sides one below, at and
    one above the 64-pixel tile and staging width and the 16-row tile height; with and without the blurs; then the small
    ones with a spacing of 6 and no crop margin, so that they subdivide over several levels and cells without pixels come up"""
    sizes = [(1, 1), (1, 40), (40, 1), (5, 7), (63, 63), (64, 64), (65, 65), (64, 17), (17, 64), (15, 16), (129, 33), (130, 127)]
    imgs = [R.textured(w, h, 70 + k, ch) for k, (w, h) in enumerate(sizes)]
    imgs.append(R.as_channels(M.smooth_tile(300, 200, 5), ch, 5))
    imgs.append(np.full((50, 70) if ch == 1 else (50, 70, ch), 90, np.uint8))
    for p in (M.DEFAULTS, M.params(pre_blur=0, post_blur=0, clip_pct=0.0, canny1=10, canny2=120)):
        got = run_dev(lib, imgs, p, ragged_seed=30 + ch)
        assert got["rc"] == 0
        check_all("small", imgs, p, got)
        assert got["rects"][-2] == [(0, 0, 300, 200)] and got["rects"][-1] == [(0, 0, 70, 50)]
        assert (got["edges"][-1] == 0).all()
    p = M.params(min_grid_spacing=6, crop_margin=0, hough_thresh_factor=0.5)
    got = run_dev(lib, imgs[:10], p, ragged_seed=50 + ch, cap=4096)
    assert got["rc"] == 0 and int(got["first"][10]) > 1000  # (hundreds of cells an image, over several levels)
    check_all("levels", imgs[:10], p, got)


# ---- the hysteresis --------------------------------------------------------------------------------------------------------
def test_hysteresis_follows_a_spiral_across_tiles(lib):
    """weak candidates along a spiral over 3 x 3 tiles that runs rightwards, down, leftwards and upwards: on from one
    strong end to the other end, off without the seed; two seeds whose paths meet; a ring that touches no seed stays
    off.  The model confirms each on the CPU first."""
    p = M.params(**M.HYST_PARAMS)
    cases = {s: M.spiral(s) for s in ((True, False), (False, False), (True, True))}
    for s, (img, pts) in cases.items():
        e, cls = M.edge_map(img, p)
        on = e == 255
        tiles = {(y // TILE, x // TILE) for y, x in zip(*np.nonzero(on))}
        assert (cls[M.RING_BOX] == 1).sum() > 300 and not on[M.RING_BOX].any()
        if any(s):
            assert M.follows(on, pts) and len(tiles) >= 6 and (cls == 2).sum() <= 20
        else:
            assert not on.any() and (cls == 1).sum() > 6000 and not (cls == 2).any()
    imgs = [c[0] for c in cases.values()]
    got = run_dev(lib, imgs, p, ragged_seed=3)
    assert got["rc"] == 0
    check_all("spiral", imgs, p, got)
    assert got["passes"] > 6  # the path crosses many tile borders: a launch per crossing, then one that changes nothing
    alone = run_dev(lib, imgs[1:2], p)
    assert alone["passes"] == 1 and not alone["edges"][0].any()


# ---- the votes --------------------------------------------------------------------------------------------------------------
def test_vote_thresholds_and_diagonal_ties(lib):
    p = M.params(**M.VOTE_PARAMS)
    b = M.bar(81)  # threshold int(100 * 0.8) = 80: row 9 holds exactly 80 pixels, row 19 holds 81
    e, _ = M.edge_map(b, p)
    assert (e[9] != 0).sum() == 80 and (e[19] != 0).sum() == 81 and M.grid_lines(e, 0.8)[0] == [18]
    bt = M.bar(49, 60, 100).T.copy()  # columns of a 60-row image: int(60 * 0.8) = 48
    et, _ = M.edge_map(bt, p)
    assert (et[:, 9] != 0).sum() == 48 and (et[:, 19] != 0).sum() == 49 and M.grid_lines(et, 0.8)[1] == [18]
    imgs = [b, bt]
    for anti in (True, False):
        img, row, count = M.diagonal_case(anti)
        acc = M.accumulator(M.edge_map(img, p)[0])
        at = 2 * row + 2 * (50 + 70)
        assert acc[2][at] == count > 40
        if anti:  # equal to the 45 degree bin: rejected
            assert acc[1][at] == count and row - 1 not in want(img, p)["hor"]
        else:     # equal to the 135 degree bin, above the 45 degree one: kept
            assert acc[3][at] == count > acc[1][at] and row - 1 in want(img, p)["hor"]
        imgs.append(img)
    got = run_dev(lib, imgs, p, ragged_seed=4)
    assert got["rc"] == 0
    check_all("votes", imgs, p, got)
    assert got["hor"][0] == [18] and got["ver"][1] == [18]
    pm = M.params(h_margin=19, v_margin=19, **M.VOTE_PARAMS)  # 18 < margin: dropped
    gm = run_dev(lib, imgs[:2], pm)
    check_all("margins", imgs[:2], pm, gm)
    assert gm["hor"][0] == [] and gm["ver"][1] == []


# ---- plumbing ----------------------------------------------------------------------------------------------------------------
def test_short_capacity_and_empty_batch(lib):
    imgs = sheets(3)[:2]
    full = run_dev(lib, imgs, M.DEFAULTS)
    need = int(full["first"][2])
    assert need == 13
    short = run_dev(lib, imgs, M.DEFAULTS, cap=need - 1)  # (run_dev asserts that nothing was written)
    from cbird_amd import _lib

    assert short["rc"] == _lib.CBH_E_OVERFLOW and (short["first"] == full["first"]).all()
    exact = run_dev(lib, imgs, M.DEFAULTS, cap=need)
    assert exact["rc"] == 0 and exact["rects"] == full["rects"]
    rc, _, first = run_host(lib, imgs, M.DEFAULTS, cap=0)
    assert rc == _lib.CBH_E_OVERFLOW and int(first[2]) == need
    first = np.full(2, 9, np.uint32)
    cp = c_params(M.DEFAULTS)
    assert lib.cbh_demosaic_dev(None, 0, None, None, None, None, 3, C.addressof(cp), None, 0, first.ctypes.data, 0, None) == 0
    assert lib.cbh_demosaic(None, 0, 0, None, None, None, None, 3, C.addressof(cp), None, 0, first.ctypes.data, 0) == 0
    assert first[0] == 0


def test_arguments(lib):
    import torch

    from cbird_amd import _lib

    L, INVAL, UNSUP = lib, _lib.CBH_E_INVAL, _lib.CBH_E_UNSUPPORTED
    img = R.textured(40, 30, 3)
    buf, off, w, h, st = pack([img], None)
    d = torch.from_numpy(buf).cuda()
    rects, first = np.zeros(64, np.int32), np.zeros(2, np.uint32)

    def call(ch=3, n=1, w=w, st=st, rects=rects, first=first, src=None, **p):
        cp = c_params(M.params(**p))
        return L.cbh_demosaic_dev(d.data_ptr() if src is None else src, n, off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                  st.ctypes.data, ch, C.addressof(cp), None if rects is None else rects.ctypes.data, 16,
                                  None if first is None else first.ctypes.data, 0, None)

    assert call() == 0
    for p in (dict(pre_blur=5), dict(post_blur=1), dict(hough_rho=1.0), dict(hough_theta=90.0)):
        assert call(**p) == UNSUP, p
    assert call(pre_blur=0, post_blur=0) == 0
    assert call(clip_pct=-1.0) == INVAL and call(clip_pct=float("nan")) == INVAL
    # cells outside their image, a line paired with itself: refused, not run
    assert call(crop_margin=-1) == INVAL and call(min_grid_spacing=0) == INVAL and call(min_grid_spacing=-5) == INVAL
    assert call(crop_margin=0) == 0 and call(min_grid_spacing=1) in (0, _lib.CBH_E_OVERFLOW)  # (accepted: more than 16 cells)
    assert call(ch=2) == INVAL and call(n=(1 << 20) + 1) == INVAL and call(first=None) == INVAL and call(rects=None) == INVAL
    assert call(w=np.array([0], np.uint32)) == INVAL and call(w=np.array([32768], np.uint32)) == INVAL
    assert call(st=np.array([119], np.uint32)) == INVAL
    cp = c_params(M.DEFAULTS)
    assert L.cbh_demosaic_dev(d.data_ptr(), 1, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, 3, None,
                              rects.ctypes.data, 16, first.ctypes.data, 0, None) == INVAL
    short = L.cbh_demosaic(buf.ctypes.data, 100, 1, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, 3,
                           C.addressof(cp), rects.ctypes.data, 16, first.ctypes.data, 0)
    assert short == INVAL  # the image ends outside its buffer
    assert L.cbh_edge_maps_dev(d.data_ptr(), 1, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, 3,
                               C.addressof(cp), None, None, None, 0, None) == INVAL
    assert call() == 0


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_every_allocation_may_be_refused(lib, entry):
    """the walk of tests/test_error_paths.py: "fault_alloc_after" 0, 1, 2, ... until the call makes fewer allocations.
    Every refused call returns CBH_E_NOMEM, leaves no scratch handed out, and the next call gives the same results.  The
    sheet subdivides, so the walk passes through both levels."""
    from cbird_amd import _lib

    L = lib
    imgs = [M.sheet(*M.LAYOUTS[0], seed=1)[0], R.textured(40, 30, 3)]

    def call():
        if entry == "host":
            rc, rects, _ = run_host(L, imgs, M.DEFAULTS)
            return rc, rects
        got = run_dev(L, imgs, M.DEFAULTS)
        return got["rc"], got["rects"]

    def call_rc():
        if entry == "host":
            return run_host(L, imgs, M.DEFAULTS)[0]
        import torch

        buf, off, w, h, st = pack(imgs, None)
        d = torch.from_numpy(buf).cuda()
        cp = c_params(M.DEFAULTS)
        rects, first = np.zeros(4 * 64, np.int32), np.zeros(3, np.uint32)
        torch.cuda.synchronize()
        return L.cbh_demosaic_dev(d.data_ptr(), 2, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, 3,
                                  C.addressof(cp), rects.ctypes.data, 64, first.ctypes.data, 0, None)

    rc, first = call()  # (one-time costs are not part of the walk)
    assert rc == 0 and len(first[0]) == 7
    refused = 0
    for k in range(100):
        live0, fired0 = _tuning(L, b"arena_live_bytes"), _tuning(L, b"fault_fired")
        L.cbh_set_tuning(b"fault_alloc_after", k)
        try:
            rc = call_rc()
        finally:
            L.cbh_set_tuning(b"fault_alloc_after", -1)
        if _tuning(L, b"fault_fired") == fired0:
            assert rc == 0
            break
        refused += 1
        assert rc == _lib.CBH_E_NOMEM, (k, rc)
        assert _tuning(L, b"arena_live_bytes") == live0, k
        rc, again = call()
        assert rc == 0 and again == first, k
    else:
        pytest.fail("the call never ran out of allocations to refuse")
    # a pass takes at least its two planes, its counters and its tables from the arena, and there are two levels; the
    # host entry stages the images in front of them
    assert refused >= 2 * 4 + (entry == "host")


# ---- the Python entries ----------------------------------------------------------------------------------------------------
def test_python_entries(lib):
    import torch

    from cbird_amd import demosaic, edge_maps, grid_lines, grid_tiles

    imgs = [M.sheet(*M.LAYOUTS[0], seed=1)[0], R.textured(40, 30, 3, 1), R.as_channels(M.sheet(*M.LAYOUTS[3], seed=1)[0], 4, 2)]
    wants = [want(im, M.DEFAULTS) for im in imgs]
    for src in (imgs, [torch.from_numpy(im).cuda() for im in imgs]):
        rects = demosaic(src)
        assert [[tuple(r) for r in a.tolist()] for a in rects] == [[tuple(r) for r in w["final"]] for w in wants]
    edges, cls, passes = edge_maps(imgs, classes=True)
    lines = grid_lines(imgs)
    for i, w in enumerate(wants):
        assert (edges[i] == w["edges"]).all() and (cls[i] == w["cls"]).all() and passes >= 1
        assert lines[i][0].tolist() == w["hor"] and lines[i][1].tolist() == w["ver"]
    assert demosaic(imgs[:1], dict(hough_thresh_factor=0.99))[0].tolist() == [list(r) for r in
                                                                               M.demosaic(imgs[0], M.params(hough_thresh_factor=0.99))]
    tiles = grid_tiles(imgs[0], rects[0])
    for (x, y, w, h), t in zip(rects[0].tolist(), tiles):
        assert t.shape == (h, w, 3) and (t == imgs[0][y:y + h, x:x + w]).all()
    out = grid_tiles(imgs[1], [(-2, -1, 5, 4)])[0]  # QImage::copy fills what lies outside with 0
    assert (out[1:, 2:] == imgs[1][:3, :3]).all() and not out[0].any() and not out[:, :2].any()
    # the crops are what the hash entries take
    from cbird_amd import dct_hash64_batch

    gray = [np.ascontiguousarray(R.gray_view(t)) for t in tiles if t.shape[0] >= 32 and t.shape[1] >= 32]
    same = [g for g in gray if g.shape == gray[0].shape]
    assert len(dct_hash64_batch(np.stack(same))) == len(same)
