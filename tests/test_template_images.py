"""GPU suite for cbird_amd/csrc/tmimages.hip: the ragged Lanczos-4 resize, the ragged grey conversion, the descriptor
match + point gather, and the chain cbh_template_match_images(_dev), held to the model of tests/template_images_rules.py.
Everything is compared bit for bit but the matrices m / tx, which keep template_match_rules.m_tolerance()."""
import ctypes as C

import numpy as np
import pytest

import template_images_rules as M
import template_match_rules as R

pytestmark = pytest.mark.gpu

GUARD, PAD = 0x5A, 0xA5


def _tuning(L, key):
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0
    return v.value


@pytest.fixture(scope="module")
def lib(gpu):
    from cbird_amd import _lib, orb

    L = _lib.lib()
    orb.set_pattern(orb.synthetic_pattern())  # the model's (template_images_rules.oracles)
    L.cbh_set_tuning(b"orb_retain_order", 1)
    return L


def pack_ragged(imgs, rng, gap=40):
    """images with padded rows, gaps and odd offsets; everything that is not a pixel is PAD"""
    off, stride, pos = [], [], int(rng.integers(1, 9))
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


def guarded_layout(sizes):
    """16-byte aligned offsets with a 16-byte guard band in front of, between and behind the images -> (offsets, total)"""
    off, pos = [], 16
    for s in sizes:
        off.append(pos)
        pos += (s + 15) // 16 * 16 + 16
    return np.array(off, np.uint64), pos


def check_guards(out, off, sizes):
    keep = np.ones(len(out), bool)
    for o, s in zip(off, sizes):
        keep[int(o): int(o) + s] = False
    assert (out[keep] == GUARD).all()


def image(rng, w, h, ch):
    im = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
    return im[..., 0] if ch == 1 else im


# ---- 1. the resize stage -------------------------------------------------------------------------------------------------
RESIZE_CASES = [((9, 7), (4, 3)), ((64, 48), (63, 47)), ((257, 131), (100, 51)), ((300, 200), (300, 200)), ((20, 20), (33, 31))]


def _resize_dev(L, imgs, ch, targets, rng, stream=None):
    import torch

    buf, off, w, h, st = pack_ragged(imgs, rng)
    sizes = [dw * dh * ch for dw, dh in targets]
    doff, total = guarded_layout(sizes)
    dw = np.array([t[0] for t in targets], np.uint32)
    dh = np.array([t[1] for t in targets], np.uint32)
    d_src = torch.from_numpy(buf).cuda()
    d_dst = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.cbh_resize_lanczos4_ragged_dev(d_src.data_ptr(), len(imgs), off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                          st.ctypes.data, ch, doff.ctypes.data, dw.ctypes.data, dh.ctypes.data,
                                          d_dst.data_ptr(), 0, stream.cuda_stream if stream else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy()
    check_guards(out, doff, sizes)
    assert (d_src.cpu().numpy() == buf).all()
    return rc, [out[int(o): int(o) + s].reshape((t[1], t[0]) + ((ch,) if ch > 1 else ())) for o, s, t in zip(doff, sizes, targets)]


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_resize_stage_equals_the_oracle(lib, ch):
    import torch

    rng = np.random.default_rng(40 + ch)
    imgs = [image(rng, w, h, ch) for (w, h), _ in RESIZE_CASES]
    targets = [t for _, t in RESIZE_CASES]
    want = [M.resize(im, dw, dh) for im, (dw, dh) in zip(imgs, targets)]
    assert (want[3] == imgs[3]).all()  # same size: every weight but the centre one is 0
    rc, got = _resize_dev(lib, imgs, ch, targets, rng)
    assert rc == 0
    for k, (g, w_) in enumerate(zip(got, want)):
        assert (g == w_).all(), RESIZE_CASES[k]
    rc, one = _resize_dev(lib, imgs[2:3], ch, targets[2:3], rng)  # n = 1
    assert rc == 0 and (one[0] == want[2]).all()
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    rc, got = _resize_dev(lib, imgs, ch, targets, rng, side)
    assert rc == 0 and all((g == w_).all() for g, w_ in zip(got, want))


# ---- 2. the grey stage ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [3, 4])
def test_gray_stage_equals_the_oracle(lib, ch):
    import torch

    rng = np.random.default_rng(50 + ch)
    imgs = [image(rng, w, h, ch) for w, h in ((1, 5), (63, 3), (64, 2), (65, 7), (1, 1))]
    buf, off, w, h, st = pack_ragged(imgs, rng)
    sizes = [im.shape[0] * im.shape[1] for im in imgs]
    doff, total = guarded_layout(sizes)
    d_src = torch.from_numpy(buf).cuda()
    d_dst = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.cbh_bgr2gray_ragged_dev(d_src.data_ptr(), len(imgs), off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                       st.ctypes.data, ch, doff.ctypes.data, d_dst.data_ptr(), 0, None) == 0
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy()
    check_guards(out, doff, sizes)
    for im, o, s in zip(imgs, doff, sizes):
        assert (out[int(o): int(o) + s].reshape(im.shape[:2]) == M.gray(im)).all(), im.shape


# ---- 3. match and gather -------------------------------------------------------------------------------------------------
def _match_dev(L, case, max_dist, cap=None, records=True, stream=None):
    import torch

    train, txy, desc, xy, counts = case
    n = len(counts)
    first = np.full(n + 1, 0xDEAD, np.uint64)
    total = cap if cap is not None else int(M.KP_CAP * len(train) * n)  # (never reached: only the model knows the count)
    d_train, d_txy, d_desc, d_xy, d_counts = (torch.from_numpy(np.ascontiguousarray(v)).cuda()
                                              for v in (train, txy, desc, xy, counts.view(np.int32)))
    mk = lambda elems, dt: torch.full((max(total, 1) * elems + 16,), 7, dtype=dt, device="cuda")  # noqa: E731
    d_a, d_b, d_rec = mk(2, torch.float32), mk(2, torch.float32), mk(3, torch.int32)
    torch.cuda.synchronize()
    rc = L.cbh_tm_match_points_dev(d_train.data_ptr(), d_txy.data_ptr(), len(train), d_desc.data_ptr(), d_xy.data_ptr(),
                                   d_counts.data_ptr(), n, M.KP_CAP, max_dist, d_rec.data_ptr() if records else None,
                                   d_a.data_ptr(), d_b.data_ptr(), total, first.ctypes.data, 0,
                                   stream.cuda_stream if stream else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return rc, first, d_a.cpu().numpy(), d_b.cpu().numpy(), d_rec.cpu().numpy()


@pytest.mark.parametrize("max_dist", [0, 25, 256])
@pytest.mark.parametrize("n_train", [1, 63, 100, 257, 2048])
def test_match_and_gather_equal_the_model(lib, n_train, max_dist):
    from cbird_amd import _lib

    case = M.match_case(n_train, max_dist)
    first, rec, a, b = M.match_model(*case, max_dist)
    total = int(first[-1])
    per = np.diff(first.astype(np.int64))
    if max_dist == 256:
        assert (per == case[4].astype(np.int64) * n_train).all()  # every pair
    else:
        assert total >= 70 and per[0] == 0
        assert n_train < 6 or per[5:].tolist() == [0, 1, 2, 3]
    rc, f, ga, gb, grec = _match_dev(lib, case, max_dist, cap=total)
    assert rc == 0 and (f == first).all()
    assert (grec[:total * 3].reshape(-1, 3) == rec).all()
    assert ga[:total * 2].tobytes() == a.tobytes() and gb[:total * 2].tobytes() == b.tobytes()
    assert (ga[total * 2:] == 7).all() and (gb[total * 2:] == 7).all() and (grec[total * 3:] == 7).all()
    # one short: the count comes back complete and nothing is written
    rc, f, ga, gb, grec = _match_dev(lib, case, max_dist, cap=total - 1, records=False)
    assert rc == _lib.CBH_E_OVERFLOW and (f == first).all()
    assert (ga == 7).all() and (gb == 7).all() and (grec == 7).all()


# ---- 4. the chain --------------------------------------------------------------------------------------------------------
def check_chain(name, want, tol, got, patch, th, tw):
    from cbird_amd.hashing import NO_TRANSFORM_SCORE

    assert int(got["status"]) == want["status"], name
    assert got["cand_scale"] == want["scale"] and (int(got["w"]), int(got["h"])) == (want["w"], want["h"]), name
    assert (int(got["n_keypoints"]), int(got["n_matches"])) == (want["n_keypoints"], want["n_matches"]), name
    g, r = got["r"], want["r"]
    if r is None:
        assert int(g["score"]) == NO_TRANSFORM_SCORE and not g["found"] and not g["m"].any(), name
        assert patch is None or not patch.any(), name
        return
    assert bool(g["found"]) == r["found"] and bool(g["tx_found"]) == r["tx_found"], name
    assert int(g["score"]) == r["score"] and int(g["cand_hash"]) == r["cand_hash"], name
    assert int(g["tmpl_hash"]) == r["tmpl_hash"] and (g["roi"] == r["roi"]).all(), name
    assert (int(g["iterations"]), int(g["good_count"])) == (r["iterations"], r["good_count"]), name
    print(name, "largest |m - model|", float(np.abs(g["m"] - r["m"]).max()), float(np.abs(g["tx"] - r["tx"]).max()))
    assert np.abs(g["m"] - r["m"]).max() <= tol and np.abs(g["tx"] - r["tx"]).max() <= tol, name
    assert (int(got["status"]) == M.SCORED) == r["found"] or want["n_matches"] < 3, name
    if patch is not None:
        assert (patch.reshape(r["patch"].shape) == r["patch"]).all(), name


def _params(**kw):
    from cbird_amd.hashing import TM_PARAMS_DTYPE

    p = np.zeros(1, TM_PARAMS_DTYPE)
    p[0] = (kw.get("needle", 100), kw.get("haystack", 1000), kw.get("cv_thresh", 25), kw.get("scale_pct", 200))
    return p


def _shape(tmpl):
    th, tw = tmpl.shape[:2]
    return th, tw, 1 if tmpl.ndim == 2 else tmpl.shape[2]


def _chain_host(L, tmpl, packed, patches=True, params=None):
    from cbird_amd.hashing import TEMPLATE_IMAGE_RESULT_DTYPE

    buf, off, w, h, st = packed
    th, tw, ch = _shape(tmpl)
    n = len(off)
    p = _params() if params is None else params
    res = np.zeros(n, TEMPLATE_IMAGE_RESULT_DTYPE)
    out = np.full((n, th, tw, ch), GUARD, np.uint8)
    rc = L.cbh_template_match_images(tmpl.ctypes.data, tw, th, tw * ch, buf.ctypes.data, buf.size, n, off.ctypes.data,
                                     w.ctypes.data, h.ctypes.data, st.ctypes.data, ch, p.ctypes.data, res.ctypes.data,
                                     out.ctypes.data if patches else None, 0)
    return rc, res, out


def _chain_dev(L, tmpl, packed, stream=None, patches=True):
    import torch

    from cbird_amd.hashing import TEMPLATE_IMAGE_RESULT_DTYPE

    buf, off, w, h, st = packed
    th, tw, ch = _shape(tmpl)
    n = len(off)
    size = n * th * tw * ch
    p = _params()
    res = np.zeros(n, TEMPLATE_IMAGE_RESULT_DTYPE)
    d_t, d_img = torch.from_numpy(tmpl).cuda(), torch.from_numpy(buf).cuda()
    d_out = torch.full((size + 64,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.cbh_template_match_images_dev(d_t.data_ptr(), tw, th, tw * ch, d_img.data_ptr(), n, off.ctypes.data, w.ctypes.data,
                                         h.ctypes.data, st.ctypes.data, ch, p.ctypes.data, res.ctypes.data,
                                         d_out.data_ptr() if patches else None, 0, stream.cuda_stream if stream else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[size:] == GUARD).all() and (d_img.cpu().numpy() == buf).all()
    return rc, res, out[:size].reshape(n, th, tw, ch)


def spread(imgs, step=1 << 20):
    """every image at its own multiple of `step` bytes: a run of two spans more than `step`"""
    assert all(im.size <= step for im in imgs)
    buf = np.full(step * len(imgs) + 1, PAD, np.uint8)
    off = np.arange(len(imgs), dtype=np.uint64) * np.uint64(step) + np.uint64(1)  # (and none of them aligned)
    for im, o in zip(imgs, off):
        buf[int(o): int(o) + im.size] = im.reshape(-1)
    ch = 1 if imgs[0].ndim == 2 else imgs[0].shape[2]
    w = np.array([im.shape[1] for im in imgs], np.uint32)
    return buf, off, w, np.array([im.shape[0] for im in imgs], np.uint32), (w * np.uint32(ch)).astype(np.uint32)


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_chain_equals_the_composed_model(lib, ch):
    import torch

    from cbird_amd.hashing import template_match_images
    from cbird_amd.quality import pack_images

    tmpl, cands, model = M.chain_fixture(ch)
    assert M.chain_conditions(model) == []
    tol, _ = R.m_tolerance()
    th, tw, _ = _shape(tmpl)
    packed = pack_images(cands)
    rc, res, patches = _chain_host(lib, tmpl, packed)
    assert rc == 0
    for i, want in enumerate(model):
        check_chain(M.NAMES[i], want, tol, res[i], patches[i], th, tw)
    rc, res2, _ = _chain_host(lib, tmpl, packed, patches=False)
    assert rc == 0 and res2.tobytes() == res.tobytes()
    # the device entry on a side stream, ragged rows and odd offsets
    side = torch.cuda.Stream()
    rc, res3, patches3 = _chain_dev(lib, tmpl, pack_ragged(cands, np.random.default_rng(ch)), side)
    assert rc == 0 and res3.tobytes() == res.tobytes() and (patches3 == patches).all()
    # the Python entry
    res4, patches4 = template_match_images(tmpl, cands, patches=True)
    assert res4.tobytes() == res.tobytes() and (patches4.reshape(patches.shape) == patches).all()
    # every candidate its own chunk: 1 MB pieces of a buffer that holds one candidate per MB
    default = _tuning(lib, b"tmatch_chunk_mb")
    wide = spread(cands)
    assert lib.cbh_set_tuning(b"tmatch_chunk_mb", 1) == 0
    try:
        rc, res5, patches5 = _chain_host(lib, tmpl, wide)
        rc2, res6, patches6 = _chain_dev(lib, tmpl, wide)
    finally:
        lib.cbh_set_tuning(b"tmatch_chunk_mb", int(default))
    assert rc == 0 and res5.tobytes() == res.tobytes() and (patches5 == patches).all()
    assert rc2 == 0 and res6.tobytes() == res.tobytes() and (patches6 == patches).all()


def test_chain_flat_template_and_nothing_to_do(lib):
    from cbird_amd.hashing import NO_TRANSFORM_SCORE, TM_NO_TEMPLATE_KEYPOINTS, template_match_images
    from cbird_amd.quality import pack_images

    tmpl, cands, _ = M.chain_fixture(3)
    flat = np.full_like(tmpl, 100)
    rc, res, patches = _chain_host(lib, flat, pack_images(cands))
    assert rc == 0 and (res["status"] == TM_NO_TEMPLATE_KEYPOINTS).all() and (res["r"]["score"] == NO_TRANSFORM_SCORE).all()
    assert not patches.any() and (res["cand_scale"] == 1).all()
    assert [(int(r["w"]), int(r["h"])) for r in res] == [c.shape[1::-1] for c in cands]
    assert lib.cbh_template_match_images(None, 8, 8, 8, None, 0, 0, None, None, None, None, 1, None, None, None, 0) == 0
    assert lib.cbh_template_match_images_dev(None, 8, 8, 8, None, 0, None, None, None, None, 1, None, None, None, 0, None) == 0
    assert len(template_match_images(tmpl, [])) == 0
    # a candidate whose resize target has a side of 0
    thin = np.full((8, 3000, 3), 77, np.uint8)
    res, patches = template_match_images(tmpl, [thin, cands[0]], patches=True)
    want = M.template_match_images(tmpl, [thin, cands[0]])
    assert [int(s) for s in res["status"]] == [w["status"] for w in want] == [M.EMPTY_RESIZE, M.SCORED]
    assert (int(res[0]["w"]), int(res[0]["h"]), res[0]["cand_scale"]) == (want[0]["w"], want[0]["h"], want[0]["scale"])
    assert want[0]["h"] == 0 and not patches[0].any() and (patches[1] == want[1]["r"]["patch"]).all()
    assert int(res[1]["r"]["score"]) == 0


# ---- 5. the staged path a caller had before gives the same results -------------------------------------------------------
def test_staged_path_equals_the_fused_entry(lib):
    import torch

    from cbird_amd import orb
    from cbird_amd.cvfeatures import CvFeaturesIndex
    from cbird_amd.hashing import template_match, template_match_images

    tmpl, cands, model = M.chain_fixture(1)
    fused = template_match_images(tmpl, cands)
    th, tw = tmpl.shape
    work, scales = [], []
    for img in cands:  # the grey resize that exists: one geometry per call
        s, dw, dh, resized = M.cand_target(tw, th, img.shape[1], img.shape[0], 200)
        if resized:
            d_src = torch.from_numpy(img).cuda()
            d_dst = torch.zeros(dw * dh, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert lib.cbh_resize_lanczos4_dev(d_src.data_ptr(), 1, img.shape[1], img.shape[0], img.shape[1], img.size, dw,
                                               dh, d_dst.data_ptr(), 0, None) == 0
            img = d_dst.cpu().numpy().reshape(dh, dw)
        work.append(img), scales.append(s)
    (_, t_xy, t_desc), = orb.orb([tmpl], 100)

    class Rows:
        id, path, keyPointDescriptors = 1, "template", t_desc

    idx = CvFeaturesIndex()
    idx.add([Rows])
    al, bl = [], []
    for _, c_xy, c_desc in orb.orb(work, 1000):
        rec = idx.radius_match(c_desc, 25)[0] if len(c_desc) else np.zeros((0, 3), np.int32)
        al.append(t_xy[rec[:, 1]].reshape(-1, 2)), bl.append(c_xy[rec[:, 0]].reshape(-1, 2))
    staged = template_match(tmpl, work, al, bl, np.array(scales, np.float32))
    assert staged.tobytes() == fused["r"].tobytes()
    assert [len(a) for a in al] == [int(v) for v in fused["n_matches"]]


# ---- 6. arguments and refusals -------------------------------------------------------------------------------------------
def test_arguments(lib):
    from cbird_amd import _lib
    from cbird_amd.quality import pack_images

    INVAL = _lib.CBH_E_INVAL
    tmpl, cands, _ = M.chain_fixture(3)
    buf, off, w, h, st = packed = pack_images(cands)
    assert _chain_host(lib, tmpl, (buf[:-1], off, w, h, st))[0] == INVAL                       # ends outside the buffer
    assert _chain_host(lib, tmpl, (buf, off, w, h, (w * 3 - 1).astype(np.uint32)))[0] == INVAL  # stride below the row
    zero = w.copy()
    zero[2] = 0
    assert _chain_host(lib, tmpl, (buf, off, zero, h, st))[0] == INVAL
    assert _chain_host(lib, tmpl, packed, params=_params(cv_thresh=257))[0] == INVAL
    assert _chain_host(lib, tmpl, packed, params=_params(needle=-1))[0] == INVAL
    th, tw, ch = _shape(tmpl)
    res = np.zeros(len(off) * 192, np.uint8)
    p = _params()
    tabs = (off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data)
    host = lambda c, tables=tabs, pp=p.ctypes.data, r=res.ctypes.data: lib.cbh_template_match_images(  # noqa: E731
        tmpl.ctypes.data, tw, th, tw * ch, buf.ctypes.data, buf.size, len(off), *tables, c, pp, r, None, 0)
    assert host(3) == 0
    assert host(2) == INVAL and host(0) == INVAL and host(3, pp=None) == INVAL and host(3, r=None) == INVAL
    for k in range(4):
        assert host(3, tables=tabs[:k] + (None,) + tabs[k + 1:]) == INVAL
    dev = lambda c=3, patches=None, tables=tabs: lib.cbh_template_match_images_dev(  # noqa: E731
        16, tw, th, tw * ch, 16, len(off), *tables, c, p.ctypes.data, res.ctypes.data, patches, 0, None)
    assert dev(2) == INVAL and dev(3, 17) == INVAL and dev(3, None, (None,) + tabs[1:]) == INVAL
    one = np.array([16], np.uint64)
    dims = np.array([8], np.uint32)
    st8 = np.array([24], np.uint32)
    rs = lambda c=3, dst=16, doff=one, dw=dims, tables=(one, dims, dims, st8): lib.cbh_resize_lanczos4_ragged_dev(  # noqa: E731
        16, 1, *(None if t is None else t.ctypes.data for t in tables), c, None if doff is None else doff.ctypes.data,
        dw.ctypes.data, dims.ctypes.data, dst, 0, None)
    assert rs(2) == INVAL and rs(3, 17) == INVAL and rs(3, 16, np.array([8], np.uint64)) == INVAL and rs(3, 16, None) == INVAL
    assert rs(3, 16, one, np.array([0], np.uint32)) == INVAL and rs(3, 16, one, dims, (None, dims, dims, st8)) == INVAL
    assert rs(3, 16, one, dims, (one, dims, dims, np.array([23], np.uint32))) == INVAL
    assert lib.cbh_resize_lanczos4_ragged_dev(None, 0, None, None, None, None, 3, None, None, None, None, 0, None) == 0
    gr = lambda c=3, dst=16, tables=(one, dims, dims, st8, one): lib.cbh_bgr2gray_ragged_dev(  # noqa: E731
        16, 1, *(None if t is None else t.ctypes.data for t in tables[:4]), c, None if tables[4] is None else tables[4].ctypes.data,
        dst, 0, None)
    assert gr(1) == INVAL and gr(2) == INVAL and gr(3, 24) == INVAL and gr(3, 16, (one, dims, dims, st8, None)) == INVAL
    assert gr(3, 16, (one, np.array([0], np.uint32), dims, st8, one)) == INVAL
    assert lib.cbh_bgr2gray_ragged_dev(None, 0, None, None, None, None, 3, None, None, 0, None) == 0
    first = np.zeros(2, np.uint64)
    mp = lambda kp_cap=8, md=25, fi=first, nt=4, tr=16: lib.cbh_tm_match_points_dev(  # noqa: E731
        tr, 16, nt, 16, 16, 16, 1, kp_cap, md, None, 16, 16, 8, None if fi is None else fi.ctypes.data, 0, None)
    assert mp(0) == INVAL and mp(8, 257) == INVAL and mp(8, -1) == INVAL and mp(8, 25, None) == INVAL
    assert mp(8, 25, first, 4, None) == INVAL and mp(1 << 24) == INVAL and mp(1 << 13, 25, first, 1 << 20) == INVAL
    assert lib.cbh_tm_match_points_dev(None, None, 0, None, None, None, 0, 8, 25, None, None, None, 0, first.ctypes.data, 0,
                                       None) == 0


@pytest.mark.parametrize("entry", ["images", "images_dev", "resize", "gray", "match_points"])
def test_every_allocation_may_be_refused(lib, entry):
    """the walk of tests/test_template_match.py over each new entry: "fault_alloc_after" 0, 1, 2, ... until the call makes
    fewer allocations.  Every refused call returns CBH_E_NOMEM, leaves no scratch handed out, and the next call gives the
    same bytes"""
    from cbird_amd import _lib
    from cbird_amd.quality import pack_images

    L = lib
    tmpl, cands, _ = M.chain_fixture(3)
    packed = pack_images(cands[:5])
    rng_seed = 3
    imgs = [image(np.random.default_rng(9), w, h, 3) for (w, h), _ in RESIZE_CASES[:3]]
    case = M.match_case(63, 25)
    total = int(M.match_model(*case, 25)[0][-1])

    def call():
        if entry == "images":
            rc, res, out = _chain_host(L, tmpl, packed)
            return rc, res.tobytes() + out.tobytes()
        if entry == "images_dev":
            rc, res, out = _chain_dev(L, tmpl, packed)
            return rc, res.tobytes() + out.tobytes()
        if entry == "resize":
            rc, got = _resize_dev(L, imgs, 3, [t for _, t in RESIZE_CASES[:3]], np.random.default_rng(rng_seed))
            return rc, b"".join(g.tobytes() for g in got)
        if entry == "gray":
            import torch

            buf, off, w, h, st = pack_ragged(imgs, np.random.default_rng(rng_seed))
            sizes = [im.shape[0] * im.shape[1] for im in imgs]
            doff, tot = guarded_layout(sizes)
            d_src = torch.from_numpy(buf).cuda()
            d_dst = torch.full((tot,), GUARD, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rc = L.cbh_bgr2gray_ragged_dev(d_src.data_ptr(), len(imgs), off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                           st.ctypes.data, 3, doff.ctypes.data, d_dst.data_ptr(), 0, None)
            torch.cuda.synchronize()
            return rc, d_dst.cpu().numpy().tobytes()
        rc, f, a, b, rec = _match_dev(L, case, 25, cap=total)
        return rc, f.tobytes() + a.tobytes() + b.tobytes() + rec.tobytes()

    rc, first_result = call()  # (one-time costs are not part of the walk)
    assert rc == 0
    refused = 0
    for k in range(200):
        live0, fired0 = _tuning(L, b"arena_live_bytes"), _tuning(L, b"fault_fired")
        L.cbh_set_tuning(b"fault_alloc_after", k)
        try:
            rc, got = call()
        finally:
            L.cbh_set_tuning(b"fault_alloc_after", -1)
        if _tuning(L, b"fault_fired") == fired0:
            assert rc == 0
            break
        refused += 1
        assert rc == _lib.CBH_E_NOMEM, (k, rc)
        assert _tuning(L, b"arena_live_bytes") == live0, k
        rc, again = call()
        assert rc == 0 and again == first_result, k
    else:
        pytest.fail("the call never ran out of allocations to refuse")
    # (at least: the buffers the entry itself takes, before those of the stages it calls)
    assert refused >= {"images": 12, "images_dev": 9, "resize": 3, "gray": 1, "match_points": 5}[entry]
