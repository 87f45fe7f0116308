"""GPU: brightnessAndContrastAuto and differenceImage on the device (cbird_amd/csrc/diffimage.hip) against the numpy model
(tests/difference_rules.py) with no tolerance: pictures, stretched images, cuts, histograms and every field of the
record; host and device entries, a side stream, padded rows, odd offsets and guard bytes around every output."""
import ctypes as C

import numpy as np
import pytest

import difference_rules as R

pytestmark = pytest.mark.gpu
GUARD, PAD = 0x5A, 0xA5
FIELDS = ["sum_total", "sum_max", "n_ge32", "n_ge1024", "w", "h", "warped", "left_min", "left_max", "right_min", "right_max"]


def _tuning(L, key):
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0
    return v.value


@pytest.fixture(scope="module")
def lib(gpu):
    from cbird_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def block_pixels(lib):
    return int(_tuning(lib, b"diff_block_pixels"))


_models: dict = {}


def model(block_pixels, name, lch, rch, clip=5):
    """(left, rights, [(picture, record)]) of one group in one channel pairing: computed once, never written to"""
    key = (name, lch, rch, clip)
    if key not in _models:
        grp = next(g for g in R.pair_groups(block_pixels) if g["name"] == name)
        left, rights = R.group_in_channels(grp, lch, rch)
        _models[key] = (grp, left, rights, R.model_group(left, rights, grp, clip))
    return _models[key]


def pack_ragged(imgs, rng, gap=40):
    """images with padded rows, gaps and odd offsets; everything that is not a pixel is PAD"""
    off, stride, pos = [], [], 1 + 2 * int(rng.integers(0, 4))
    for im in imgs:
        h, w = im.shape[:2]
        ch = 1 if im.ndim == 2 else im.shape[2]
        st = w * ch + int(rng.integers(0, 7))
        off.append(pos), stride.append(st)
        pos += st * h + int(rng.integers(0, gap))
    buf = np.full(pos + 32, PAD, np.uint8)
    for im, o, st in zip(imgs, off, stride):
        h, w = im.shape[:2]
        ch = 1 if im.ndim == 2 else im.shape[2]
        np.lib.stride_tricks.as_strided(buf[o:], (h, w * ch), (st, 1))[:] = im.reshape(h, w * ch)
    return (buf, np.array(off, np.uint64), np.array([im.shape[1] for im in imgs], np.uint32),
            np.array([im.shape[0] for im in imgs], np.uint32), np.array(stride, np.uint32))


def pack_plain(imgs):
    from cbird_amd.quality import pack_images

    return pack_images(imgs)


def _ch(im):
    return 1 if im.ndim == 2 else im.shape[2]


def _ptr(a):
    return None if a is None else a.ctypes.data


# ---- stage A ---------------------------------------------------------------------------------------------------------------
def contrast_dev(L, packed, ch, clip, want_out=True, want_hist=True, stream=None):
    import torch

    buf, off, w, h, st = packed
    n = len(off)
    d_img = torch.from_numpy(buf).cuda()
    d_out = torch.full((buf.size + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_cuts = torch.full((2 * n + 16,), -77, dtype=torch.int32, device="cuda")
    d_hist = torch.full((256 * n + 16,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = L.cbh_auto_contrast_dev(d_img.data_ptr(), n, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, ch,
                                 float(clip), d_out.data_ptr() if want_out else None, d_cuts.data_ptr(),
                                 d_hist.data_ptr() if want_hist else None, 0, stream.cuda_stream if stream else None)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy(), d_cuts.cpu().numpy(), d_hist.cpu().numpy(), d_img.cpu().numpy()


def contrast_host(L, packed, ch, clip, want_out=True, want_hist=True):
    buf, off, w, h, st = packed
    n = len(off)
    out = np.full(buf.size + 64, GUARD, np.uint8)
    cuts = np.full(2 * n + 16, -77, np.int32)
    hist = np.full(256 * n + 16, 0xfffffff0, np.uint32)
    rc = L.cbh_auto_contrast(buf.ctypes.data, buf.size, n, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data,
                             ch, float(clip), _ptr(out) if want_out else None, cuts.ctypes.data,
                             _ptr(hist) if want_hist else None, 0)
    return rc, out, cuts, hist


def rows_view(buf, o, st, h, rowbytes):
    return np.lib.stride_tricks.as_strided(buf[int(o):], (int(h), int(rowbytes)), (int(st), 1))


@pytest.mark.parametrize("clip", [0, 5])
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_auto_contrast_equals_the_model(lib, block_pixels, ch, clip):
    import torch

    cases = R.contrast_cases(ch, block_pixels)
    names, imgs = list(cases), list(cases.values())
    assert max(im.shape[0] * im.shape[1] for im in imgs) > block_pixels  # more than one workgroup on one image
    want = [R.auto_contrast(im, clip) for im in imgs]
    assert any(lo >= hi for _, (lo, hi), _ in want) and sum(lo < hi for _, (lo, hi), _ in want) >= 8
    n = len(imgs)
    packed = pack_ragged(imgs, np.random.default_rng(ch))
    buf, off, w, h, st = packed
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    rc, out, cuts, hist, src_after = contrast_dev(lib, packed, ch, clip, stream=side)
    assert rc == 0 and (src_after == buf).all()
    expect = np.full(buf.size + 64, GUARD, np.uint8)  # nothing but the pixels' bytes is written
    for i, (img, (lo, hi), hh) in enumerate(want):
        rows_view(expect, off[i], st[i], h[i], w[i] * ch)[:] = img.reshape(int(h[i]), -1)
        assert (int(cuts[2 * i]), int(cuts[2 * i + 1])) == (lo, hi), names[i]
        assert (hist[256 * i: 256 * i + 256].view(np.uint32) == hh).all(), names[i]
    assert (out == expect).all()
    assert (cuts[2 * n:] == -77).all() and (hist[256 * n:] == -77).all()
    # without the optional outputs; and in place
    rc, out2, cuts2, hist2, _ = contrast_dev(lib, packed, ch, clip, want_out=False, want_hist=False)
    assert rc == 0 and (out2 == GUARD).all() and (hist2 == -77).all() and (cuts2 == cuts).all()
    d = torch.from_numpy(buf).cuda()
    d_cuts = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.cbh_auto_contrast_dev(d.data_ptr(), n, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, ch,
                                     float(clip), d.data_ptr(), d_cuts.data_ptr(), None, 0, None) == 0
    inplace = np.where(expect[:buf.size] == GUARD, buf, expect[:buf.size])
    for i in range(n):  # (a pixel byte may equal GUARD: take the rows from the expectation)
        rows_view(inplace, off[i], st[i], h[i], w[i] * ch)[:] = rows_view(expect, off[i], st[i], h[i], w[i] * ch)
    assert (d.cpu().numpy() == inplace).all()
    # the host entry: the whole buffer comes back, the bytes between the images as they were
    rc, out3, cuts3, hist3 = contrast_host(lib, packed, ch, clip)
    assert rc == 0 and (out3[:buf.size] == inplace).all() and (out3[buf.size:] == GUARD).all()
    assert (cuts3 == cuts).all() and (hist3[:256 * n] == hist[:256 * n].view(np.uint32)).all()
    assert (hist3[256 * n:] == 0xfffffff0).all()


def test_auto_contrast_python_entry(lib, block_pixels):
    import torch

    from cbird_amd import auto_contrast

    imgs = []
    for ch in (3, 1, 4):
        imgs += list(R.contrast_cases(ch, block_pixels).values())[3:8]
    want = [R.auto_contrast(im, 5) for im in imgs]
    outs, cuts, hist = auto_contrast(imgs, 5, histograms=True)
    t_outs, t_cuts = auto_contrast([torch.from_numpy(im).cuda() for im in imgs], 5)
    for i, (img, cut, hh) in enumerate(want):
        assert outs[i].shape == imgs[i].shape and (outs[i] == img).all() and tuple(cuts[i]) == cut and (hist[i] == hh).all()
        assert t_outs[i].is_cuda and (t_outs[i].cpu().numpy() == img).all() and tuple(t_cuts[i]) == cut
    outs0, cuts0 = auto_contrast(imgs[:2])  # the default keeps the full range
    assert all(tuple(cuts0[i]) == R.auto_contrast(imgs[i], 0)[1] for i in range(2))
    outs, cuts = auto_contrast([])
    assert outs == [] and cuts.shape == (0, 2)


# ---- stage B ---------------------------------------------------------------------------------------------------------------
def guarded_layout(sizes):
    """16-byte aligned offsets with a guard band in front of, between and behind the pictures -> (offsets, total)"""
    off, pos = [], 16
    for s in sizes:
        off.append(pos)
        pos += (int(s) + 15) // 16 * 16 + 16
    return np.array(off, np.uint64), pos


def dims(L, left, rights, tx, has):
    n = len(rights)
    w = np.array([r.shape[1] for r in rights], np.uint32)
    h = np.array([r.shape[0] for r in rights], np.uint32)
    ow, oh, wp = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    assert L.cbh_difference_dims(left.shape[1], left.shape[0], n, _ptr(w), _ptr(h), _ptr(tx), _ptr(has), _ptr(ow), _ptr(oh),
                                 _ptr(wp)) == 0
    return ow, oh, wp


def tx_of(grp):
    tx = None if grp.get("tx") is None else np.ascontiguousarray(grp["tx"], np.float64).reshape(-1, 6)
    has = None if grp.get("has") is None else np.array(grp["has"], np.uint8)
    return tx, has


def diff_dev(L, left, rights, tx, has, clip=5, pictures=True, detail=True, stream=None, ragged_seed=None):
    """-> (rc, pictures or None, records or None); checks the guards itself"""
    import torch

    from cbird_amd.difference import DIFF_DETAIL_DTYPE

    n = len(rights)
    lp = pack_ragged([left], np.random.default_rng(99)) if ragged_seed is not None else pack_plain([left])
    rp = pack_ragged(rights, np.random.default_rng(ragged_seed)) if ragged_seed is not None else pack_plain(rights)
    ow, oh, _ = dims(L, left, rights, tx, has)
    sizes = ow.astype(np.int64) * oh * 4
    ooff, total = guarded_layout(sizes)
    d_left = torch.from_numpy(lp[0]).cuda()
    d_rights = torch.from_numpy(rp[0]).cuda()
    d_pics = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    d_det = torch.full((n * 48 + 64,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.cbh_difference_images_dev(d_left.data_ptr() + int(lp[1][0]), left.shape[1], left.shape[0], int(lp[4][0]),
                                     _ch(left), d_rights.data_ptr(), n, _ptr(rp[1]), _ptr(rp[2]), _ptr(rp[3]), _ptr(rp[4]),
                                     _ch(rights[0]), _ptr(tx), _ptr(has), float(clip),
                                     d_pics.data_ptr() if pictures else None, _ptr(ooff),
                                     d_det.data_ptr() if detail else None, 0, stream.cuda_stream if stream else None)
    torch.cuda.synchronize()
    flat, det = d_pics.cpu().numpy(), d_det.cpu().numpy()
    assert (det[n * 48:] == GUARD).all()
    keep = np.ones(total, bool)
    pics = []
    for i in range(n):
        o = int(ooff[i])
        keep[o: o + int(sizes[i])] = False
        pics.append(flat[o: o + int(sizes[i])].reshape(int(oh[i]), int(ow[i]), 4))
    if rc == 0 and pictures:
        assert (flat[keep] == GUARD).all()
    else:
        assert (flat == GUARD).all()
    if not detail:
        assert (det == GUARD).all()
    return rc, pics if pictures else None, det[:n * 48].view(DIFF_DETAIL_DTYPE) if detail else None


def diff_host(L, left, rights, tx, has, clip=5, pictures=True):
    from cbird_amd.difference import DIFF_DETAIL_DTYPE

    n = len(rights)
    left = np.ascontiguousarray(left)
    buf, off, w, h, st = pack_plain(rights)
    ow, oh, _ = dims(L, left, rights, tx, has)
    sizes = ow.astype(np.int64) * oh * 4
    ooff, total = guarded_layout(sizes)
    flat = np.full(total, GUARD, np.uint8)
    det = np.zeros(n, DIFF_DETAIL_DTYPE)
    rc = L.cbh_difference_images(left.ctypes.data, left.shape[1], left.shape[0], left.shape[1] * _ch(left), _ch(left),
                                 buf.ctypes.data, buf.size, n, _ptr(off), _ptr(w), _ptr(h), _ptr(st), _ch(rights[0]),
                                 _ptr(tx), _ptr(has), float(clip), _ptr(flat) if pictures else None, flat.size, _ptr(ooff),
                                 det.ctypes.data, 0)
    keep = np.ones(total, bool)
    pics = []
    for i in range(n):
        o = int(ooff[i])
        keep[o: o + int(sizes[i])] = False
        pics.append(flat[o: o + int(sizes[i])].reshape(int(oh[i]), int(ow[i]), 4))
    assert (flat[keep] == GUARD).all()
    return rc, pics, det


def check_pair(what, want, pic, rec):
    wpic, wrec = want
    for f in FIELDS:
        assert int(rec[f]) == wrec[f], (what, f, int(rec[f]), wrec[f])
    if pic is not None:
        assert pic.shape == wpic.shape and (pic == wpic).all(), what


GROUPS = [g["name"] for g in R.pair_groups()]


@pytest.mark.parametrize("rch", [1, 3, 4])
@pytest.mark.parametrize("lch", [1, 3, 4])
def test_difference_images_equal_the_model(lib, block_pixels, lch, rch):
    """every group on the device entry -- a side stream, padded rows, odd offsets, guards -- and, record for record,
    without the pictures"""
    import torch

    side = torch.cuda.Stream()
    for name in GROUPS:
        grp, left, rights, want = model(block_pixels, name, lch, rch)
        tx, has = tx_of(grp)
        rc, pics, det = diff_dev(lib, left, rights, tx, has, stream=side, ragged_seed=lch * 10 + rch)
        assert rc == 0, name
        for i, wnt in enumerate(want):
            check_pair((name, i), wnt, pics[i], det[i])
        rc, none, det2 = diff_dev(lib, left, rights, tx, has, pictures=False)
        assert rc == 0 and none is None and det2.tobytes() == det.tobytes(), name


def test_difference_host_and_python_entries(lib, block_pixels):
    import torch

    from cbird_amd import difference_images

    for name in ("sizes", "dyadic"):
        grp, left, rights, want = model(block_pixels, name, 3, 3)
        tx, has = tx_of(grp)
        rc, pics, det = diff_host(lib, left, rights, tx, has)
        assert rc == 0
        for i, wnt in enumerate(want):
            check_pair((name, i), wnt, pics[i], det[i])
        rc, _, det2 = diff_host(lib, left, rights, tx, has, pictures=False)
        assert rc == 0 and det2.tobytes() == det.tobytes()
    # the Python entry: rights of mixed channel counts, numpy and device tensors, matrices with flags
    grp, left, rights, _ = model(block_pixels, "dyadic", 4, 3)
    mixed = [R.as_channels(r, (1, 3, 4)[i % 3], i) for i, r in enumerate(grp["rights"])]
    want = R.model_group(left, mixed, grp)
    tr = (grp["tx"].reshape(-1, 2, 3), grp["has"])
    pics, det = difference_images(left, mixed, tr)
    t_pics, t_det = difference_images(torch.from_numpy(left).cuda(), [torch.from_numpy(m).cuda() for m in mixed], tr)
    for i, wnt in enumerate(want):
        check_pair(("python", i), wnt, pics[i], det[i])
        assert t_pics[i].is_cuda
        check_pair(("python tensors", i), wnt, t_pics[i].cpu().numpy(), t_det[i])
    none, det3 = difference_images(left, mixed, tr, pictures=False)
    assert none == [None] * len(mixed) and det3.tobytes() == det.tobytes()
    assert difference_images(left, [])[0] == []


def test_one_pair_and_none(lib, block_pixels):
    grp, left, rights, want = model(block_pixels, "dyadic", 3, 3)
    tx, has = tx_of(grp)
    rc, pics, det = diff_dev(lib, left, rights[3:4], tx[3:4].copy(), has[3:4].copy())
    assert rc == 0
    check_pair("n = 1", want[3], pics[0], det[0])
    rc, pics, det = diff_dev(lib, left, rights[3:4], tx[3:4].copy(), None)  # no flags: every matrix counts
    assert rc == 0
    check_pair("n = 1, no flags", want[3], pics[0], det[0])
    L = lib
    assert L.cbh_difference_images_dev(None, 5, 5, 15, 3, None, 0, None, None, None, None, 3, None, None, 5.0, None, None,
                                       None, 0, None) == 0
    assert L.cbh_difference_images(None, 5, 5, 15, 3, None, 0, 0, None, None, None, None, 3, None, None, 5.0, None, 0, None,
                                   None, 0) == 0
    assert L.cbh_auto_contrast_dev(None, 0, None, None, None, None, 3, 0.0, None, None, None, 0, None) == 0
    assert L.cbh_auto_contrast(None, 0, 0, None, None, None, None, 3, 0.0, None, None, None, 0) == 0


def test_arguments(lib, block_pixels):
    import torch

    from cbird_amd import _lib

    L, INVAL = lib, _lib.CBH_E_INVAL
    grp, left, rights, _ = model(block_pixels, "sizes", 3, 3)
    packed = pack_plain(rights)
    buf, off, w, h, st = packed
    n = len(rights)
    for ch in (0, 2, 5):
        assert contrast_host(L, packed, ch, 5)[0] == INVAL
    assert contrast_host(L, packed, 3, -1)[0] == INVAL
    assert contrast_host(L, packed, 3, float("nan"))[0] == INVAL
    assert contrast_host(L, (buf[:-1], off, w, h, st), 3, 5)[0] == INVAL  # the last pixel lies outside
    assert contrast_host(L, (buf, off, w, h, (w * 3 - 1).astype(np.uint32)), 3, 5)[0] == INVAL
    big = w.copy()
    big[0] = 32768
    assert contrast_host(L, (buf, off, big, h, (big * 3).astype(np.uint32)), 3, 5)[0] == INVAL
    ow, oh, _ = dims(L, left, rights, None, None)
    ooff, total = guarded_layout(ow.astype(np.int64) * oh * 4)
    flat = np.zeros(total, np.uint8)

    def host(lw=23, lch=3, ch=3, clip=5.0, out_off=ooff, total=total, w=w, stride=st):
        return L.cbh_difference_images(left.ctypes.data, lw, 17, 23 * 3, lch, buf.ctypes.data, buf.size, n, _ptr(off),
                                       _ptr(w), _ptr(h), _ptr(stride), ch, None, None, clip, flat.ctypes.data, total,
                                       _ptr(out_off), None, 0)

    assert host() == 0
    assert host(lch=2) == INVAL and host(ch=5) == INVAL and host(clip=-0.5) == INVAL and host(lw=0) == INVAL
    assert host(lw=32768) == INVAL and host(lw=24) == INVAL  # (24 * 3 bytes do not fit the left image's rows)
    assert host(out_off=ooff + np.uint64(4)) == INVAL  # misaligned
    assert host(total=int(ooff[-1])) == INVAL  # the last picture does not fit
    assert host(w=big, stride=(big * 3).astype(np.uint32)) == INVAL
    d = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    d_l, d_r = torch.from_numpy(left).cuda(), torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()

    def dev(pics, out_off):
        return L.cbh_difference_images_dev(d_l.data_ptr(), 23, 17, 69, 3, d_r.data_ptr(), n, _ptr(off), _ptr(w), _ptr(h),
                                           _ptr(st), 3, None, None, 5.0, pics, _ptr(out_off), None, 0, None)

    assert dev(d.data_ptr(), ooff) == 0
    assert dev(d.data_ptr() + 4, ooff) == INVAL and dev(d.data_ptr(), ooff + np.uint64(8)) == INVAL
    assert dev(d.data_ptr(), None) == INVAL


@pytest.mark.parametrize("entry", ["host", "dev", "contrast_host", "contrast_dev"])
def test_every_allocation_may_be_refused(lib, block_pixels, entry):
    """the walk of tests/test_error_paths.py: "fault_alloc_after" 0, 1, 2, ... until the call makes fewer allocations.
    Every refused call returns CBH_E_NOMEM, leaves no scratch handed out, and the next call gives the same results"""
    from cbird_amd import _lib

    L = lib
    grp, left, rights, want = model(block_pixels, "dyadic", 3, 3)
    tx, has = tx_of(grp)
    packed = pack_plain(rights)

    def call():
        if entry == "host":
            rc, pics, det = diff_host(L, left, rights, tx, has)
            return rc, b"".join(p.tobytes() for p in pics) + det.tobytes()
        if entry == "dev":
            rc, pics, det = diff_dev(L, left, rights, tx, has)
            return rc, b"".join(p.tobytes() for p in pics) + det.tobytes()
        if entry == "contrast_host":
            rc, out, cuts, hist = contrast_host(L, packed, 3, 5)
            return rc, out.tobytes() + cuts.tobytes() + hist.tobytes()
        rc, out, cuts, hist, _ = contrast_dev(L, packed, 3, 5)
        return rc, out.tobytes() + cuts.tobytes() + hist.tobytes()

    rc, first = call()  # (one-time costs are not part of the walk)
    assert rc == 0
    refused = 0
    for k in range(100):
        live0, fired0 = _tuning(L, b"arena_live_bytes"), _tuning(L, b"fault_fired")
        L.cbh_set_tuning(b"fault_alloc_after", k)
        try:
            rc, _ = call()
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
    assert refused >= {"host": 10, "dev": 6, "contrast_host": 6, "contrast_dev": 3}[entry]


def test_template_match_records_chain_into_difference_images(lib, block_pixels):
    """the records of template_match_images for a shifted and a rotated copy of a textured 96 x 96 template go straight
    into difference_images; the pictures equal the model fed the same tx"""
    import template_match_rules as T

    from cbird_amd import difference_images, orb
    from cbird_amd.hashing import TM_SCORED, template_match_images

    orb.set_pattern(orb.synthetic_pattern())
    rng = np.random.default_rng(4)  # (a scene on which the matcher's numpy model finds both transforms)
    tmpl = T.scene(rng, 96, 96, 3)
    shifted = np.full((130, 140, 3), 90, np.uint8)
    shifted[21:117, 17:113] = tmpl
    rotated = T.warp_affine(tmpl, T.invert(T.similarity(10, 1.0, 30.0, 8.0)), 150, 140)[0].reshape(140, 150, 3)
    cands = [shifted, np.ascontiguousarray(rotated)]
    res = template_match_images(tmpl, cands)
    assert [int(s) for s in res["status"]] == [TM_SCORED, TM_SCORED] and res["r"]["tx_found"].all()
    pics, det = difference_images(tmpl, cands, res)
    for i, c in enumerate(cands):
        R.assert_floor_unambiguous(res["r"]["tx"][i], 96, 96)
        want = R.difference_image(tmpl, c, res["r"]["tx"][i], True, 5)
        check_pair(("chain", i), want, pics[i], det[i])
        assert det[i]["warped"] == 1 and (det[i]["w"], det[i]["h"]) == (96, 96)
    # aligned, the copies differ from the template less per pixel than when compared as they lie
    _, apart = difference_images(tmpl, cands, pictures=False)
    assert (det["sum_total"] / (det["w"] * det["h"]) < apart["sum_total"] / (apart["w"] * apart["h"])).all()
