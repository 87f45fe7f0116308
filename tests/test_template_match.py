"""GPU suite for cbird_amd/csrc/tmatch.hip: estimateRigidTransform, invertAffineTransform + warpAffine and the chain
transform -> warp -> score of TemplateMatcher::match (src/templatematcher.cpp:264-374), held to the numpy model of
tests/template_match_rules.py (as recalled from OpenCV 2.4.13: unpinned until tests/golden/opencv_tmatch.npz exists).

Estimate: found, the iterations run, the inlier count and the number of RNG draws equal the model's; M within the MEASURED
tolerance R.m_tolerance(): 16 x the largest difference between the model's Jacobi and numpy.linalg.solve over the final
solves of the whole fixture = 16 x 3.1e-15 = 4.97e-14 (solver-order noise of the device's division and square root
against libm's, nothing else).  That no inlier decision can flip inside that tolerance is asserted, not assumed: every
case's residual margin is at least 1e6 x the tolerance (tests/test_template_match_rules.py prints the figures: 1.0e-3 px at
the least against 5.0e-8).
Warp: M is given, so the patches equal the model's bit for bit.
Chain: found, roi, both hashes, score, iterations, inliers and patches equal the composed model (its score is
oracle.PrestageOracle.template_score); tx within the tolerance; the model's rounding margins are at least
1e6 x tolerance x 1024 x 40 = 2.04e-3 (measured 2.4e-3 .. 7.1e-3)."""
import ctypes as C

import numpy as np
import pytest

import template_match_rules as R
import test_template_match_rules as T

pytestmark = pytest.mark.gpu


def _tuning(L, key):
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0
    return v.value


# ---- estimate ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def est():
    """(names, a lists, b lists, yardstick, tolerance) with the asserted condition on the margins"""
    fx, yard = R.estimate_fixture(), R.estimate_yardstick()
    tol, _ = R.m_tolerance()
    names = [c[0] for c in R.ESTIMATE_CASES]
    assert len(names) == 14 and [len(fx[n][0]) for n in names[:10]] == [0, 2, 3, 5, 63, 64, 65, 200, 1000, 4097]
    for n in names:
        assert yard[n]["residual_margin"] >= 1e6 * tol, n
    return names, [fx[n][0] for n in names], [fx[n][1] for n in names], yard, tol


def check_estimate(name, want, tol, m, found, det):
    assert bool(found) == want["found"], name
    assert (int(det["iterations"]), int(det["good_count"]), int(det["draws"])) == \
        (want["iterations"], want["good_count"], want["draws"]), name
    print(name, "largest |M - model|", float(np.abs(m.reshape(6) - want["m"]).max()))
    assert np.abs(m.reshape(6) - want["m"]).max() <= tol, name
    if not want["found"]:
        assert not m.any(), name


def test_estimate_one_ragged_call(gpu, est):
    from cbird_amd.hashing import estimate_rigid

    names, al, bl, yard, tol = est
    m, found, det = estimate_rigid(al, bl, detail=True)
    for i, n in enumerate(names):
        check_estimate(n, yard[n], tol, m[i], found[i], det[i])
    m2, found2 = estimate_rigid(al, bl)  # without the detail record
    assert m2.tobytes() == m.tobytes() and (found2 == found).all()


def test_estimate_one_list_per_call(gpu, est):
    from cbird_amd.hashing import estimate_rigid

    names, al, bl, yard, tol = est
    for n, a, b in zip(names, al, bl):
        m, found, det = estimate_rigid([a], [b], detail=True)
        check_estimate(n, yard[n], tol, m[0], found[0], det[0])


def _estimate_dev(L, al, bl, stream=None, detail=True):
    import torch

    from cbird_amd.hashing import RIGID_DETAIL_DTYPE, pack_point_lists

    a, b, first = pack_point_lists(al, bl)
    n = len(first) - 1
    d_a, d_b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    d_m = torch.full((n * 6 + 8,), 7.0, dtype=torch.float64, device="cuda")
    d_f = torch.full((n + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    d_d = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.cbh_estimate_rigid_dev(d_a.data_ptr(), d_b.data_ptr(), n, first.ctypes.data, d_m.data_ptr(), d_f.data_ptr(),
                                  d_d.data_ptr() if detail else None, 0, stream.cuda_stream if stream else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    m, f = d_m.cpu().numpy(), d_f.cpu().numpy()
    assert (m[n * 6:] == 7.0).all() and (f[n:] == 0x5A).all()  # the guard bands
    return rc, m[:n * 6].reshape(n, 6), f[:n], d_d.cpu().numpy().view(RIGID_DETAIL_DTYPE)


def test_estimate_dev_entry_on_a_side_stream(gpu, est):
    import torch

    from cbird_amd import _lib

    names, al, bl, yard, tol = est
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    rc, m, found, det = _estimate_dev(_lib.lib(), al, bl, side)
    assert rc == 0
    for i, n in enumerate(names):
        check_estimate(n, yard[n], tol, m[i], found[i], det[i])
    rc, m2, found2, _ = _estimate_dev(_lib.lib(), al, bl, None, detail=False)  # NULL stream: synchronous
    assert rc == 0 and m2.tobytes() == m.tobytes() and (found2 == found).all()


# ---- warp ----------------------------------------------------------------------------------------------------------------
IMAGE_SIZES, BEYOND, transforms = R.WARP_IMAGE_SIZES, R.BEYOND, R.warp_transforms


def pack_ragged(imgs, rng):
    """images with padded rows, gaps and odd offsets; everything that is not a pixel is 0xA5"""
    off, stride, pos = [], [], int(rng.integers(1, 9))
    for im in imgs:
        h, w = im.shape[:2]
        ch = 1 if im.ndim == 2 else im.shape[2]
        st = w * ch + int(rng.integers(0, 7))
        off.append(pos), stride.append(st)
        pos += st * h + int(rng.integers(0, 40))
    buf = np.full(pos + 32, 0xA5, np.uint8)
    for im, o, st in zip(imgs, off, stride):
        h, w = im.shape[:2]
        ch = 1 if im.ndim == 2 else im.shape[2]
        rows = np.lib.stride_tricks.as_strided(buf[o:], (h, w * ch), (st, 1))
        rows[:] = im.reshape(h, w * ch)
    return (buf, np.array(off, np.uint64), np.array([im.shape[1] for im in imgs], np.uint32),
            np.array([im.shape[0] for im in imgs], np.uint32), np.array(stride, np.uint32))


def _warp_dev(L, packed, ch, m, found, tw, th, stream=None):
    import torch

    buf, off, w, h, st = packed
    n = len(off)
    size = n * th * tw * ch
    d_img = torch.from_numpy(buf).cuda()
    d_m = torch.from_numpy(np.ascontiguousarray(m, np.float64).reshape(-1)).cuda()
    d_f = torch.from_numpy(np.ascontiguousarray(found, np.uint8)).cuda()
    d_out = torch.full((size + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((n + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.cbh_warp_affine_dev(d_img.data_ptr(), n, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, ch,
                               d_m.data_ptr(), d_f.data_ptr(), tw, th, d_out.data_ptr(), d_ok.data_ptr(), 0,
                               stream.cuda_stream if stream else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    out, ok = d_out.cpu().numpy(), d_ok.cpu().numpy()
    assert (out[size:] == 0x5A).all() and (ok[n:] == 0x5A).all()  # the guard bands
    assert (d_img.cpu().numpy() == buf).all()
    return rc, out[:size].reshape(n, th, tw, ch), ok[:n]


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("tw,th", [(33, 47), (90, 120), (256, 256)])
def test_warp_equals_the_model_bit_for_bit(gpu, tw, th, ch):
    import torch

    from cbird_amd import _lib

    rng = np.random.default_rng(1000 * ch + tw)
    imgs, ms, names = [], [], []
    for w, h in IMAGE_SIZES:
        img = rng.integers(1, 256, (h, w, ch), dtype=np.uint8)
        for name, m in transforms(w, h).items():
            imgs.append(img[..., 0] if ch == 1 else img), ms.append(m), names.append(f"{w}x{h} {name}")
    found = np.ones(len(imgs), np.uint8)
    found[3] = 0  # one candidate that came without a transform
    packed = pack_ragged(imgs, rng)
    assert (packed[4] > packed[2] * ch).any() and (packed[1] % 2 == 1).any()
    side = torch.cuda.Stream() if (tw, ch) == (33, 3) else None  # once on a side stream
    rc, out, ok = _warp_dev(_lib.lib(), packed, ch, np.stack(ms), found, tw, th, side)
    assert rc == 0
    for i, (img, m, name) in enumerate(zip(imgs, ms, names)):
        want, _ = R.warp_affine(img, m, tw, th)
        if not found[i] or want is None:
            assert name.endswith(BEYOND) or not found[i]
            assert ok[i] == 0 and not out[i].any(), name
            continue
        assert ok[i] == 1 and (out[i] == want.reshape(th, tw, ch)).all(), name
        if name.endswith("outside"):
            assert (out[i] == np.array(R.BORDER[ch], np.uint8)).all(), name
    assert sum(n.endswith(BEYOND) for n in names) == len(IMAGE_SIZES)


def test_warp_python_entry(gpu):
    from cbird_amd.hashing import warp_affine

    rng = np.random.default_rng(8)
    imgs = [rng.integers(1, 256, (h, w, 3), dtype=np.uint8) for w, h in ((37, 23), (50, 61), (9, 5))]
    ms = [R.similarity(30, 0.9, 10.5, -3.25), R.similarity(90, 1.4, 45.5, 2.0), R.similarity(0, 1, 2.0e6, 0)]
    out, ok = warp_affine(imgs, np.stack(ms), 33, 47)
    assert list(ok) == [True, True, False] and not out[2].any()
    for i in range(2):
        assert (out[i] == R.warp_affine(imgs[i], ms[i], 33, 47)[0]).all()


# ---- chain ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    """(fixture, yardstick, tolerance) with the asserted conditions on the model's margins"""
    fx, yard = R.chain_fixture(), T.chain_yardstick()
    tol, _ = R.m_tolerance()
    bound = 1e6 * tol * 1024 * max(R.CHAIN_TW, R.CHAIN_TH)
    assert [r["found"] for r in yard] == [True, True, False, True, False, True]
    for r in yard:
        assert r["residual_margin"] >= 1e6 * tol and (not r["found"] or r["rounding_margin"] >= bound)
    return fx, yard, tol


def check_chain(i, want, tol, got, patch):
    assert bool(got["found"]) == want["found"], i
    assert int(got["score"]) == want["score"] and int(got["cand_hash"]) == want["cand_hash"], i
    assert int(got["tmpl_hash"]) == want["tmpl_hash"] and (got["roi"] == want["roi"]).all(), i
    assert (int(got["iterations"]), int(got["good_count"])) == (want["iterations"], want["good_count"]), i
    assert bool(got["tx_found"]) == want["tx_found"], i
    assert np.abs(got["m"] - want["m"]).max() <= tol and np.abs(got["tx"] - want["tx"]).max() <= tol, i
    if patch is not None:
        assert (patch == want["patch"]).all(), i


def test_chain_equals_the_composed_model(gpu, chain):
    from cbird_amd.hashing import NO_TRANSFORM_SCORE, template_match

    (tmpl, cands, al, bl, scales), yard, tol = chain
    res, patches = template_match(tmpl, cands, al, bl, scales, patches=True)
    for i, want in enumerate(yard):
        check_chain(i, want, tol, res[i], patches[i])
    assert (res["score"][[2, 4]] == NO_TRANSFORM_SCORE).all() and NO_TRANSFORM_SCORE == R.INT32_MAX
    res2 = template_match(tmpl, cands, al, bl, scales)  # without the patches
    assert res2.tobytes() == res.tobytes()


def _chain_args(fx, reps=1):
    from cbird_amd.hashing import pack_point_lists
    from cbird_amd.quality import pack_images

    tmpl, cands, al, bl, scales = fx
    cands, al, bl, scales = list(cands) * reps, list(al) * reps, list(bl) * reps, np.tile(scales, reps)
    return tmpl, pack_images(cands), pack_point_lists(al, bl), scales, len(cands)


def _chain_host(L, args, patches=True):
    from cbird_amd.hashing import TEMPLATE_RESULT_DTYPE

    tmpl, (buf, off, w, h, st), (a, b, first), scales, n = args
    th, tw, ch = tmpl.shape
    res = np.zeros(n, TEMPLATE_RESULT_DTYPE)
    out = np.full((n, th, tw, ch), 0x5A, np.uint8)
    rc = L.cbh_template_match(tmpl.ctypes.data, tw, th, tw * ch, ch, buf.ctypes.data, buf.size, n, off.ctypes.data,
                              w.ctypes.data, h.ctypes.data, st.ctypes.data, ch, a.ctypes.data, b.ctypes.data,
                              first.ctypes.data, scales.ctypes.data, res.ctypes.data,
                              out.ctypes.data if patches else None, 0)
    return rc, res, out


def _chain_dev(L, args, stream=None, patches=True):
    import torch

    from cbird_amd.hashing import TEMPLATE_RESULT_DTYPE

    tmpl, (buf, off, w, h, st), (a, b, first), scales, n = args
    th, tw, ch = tmpl.shape
    size = n * th * tw * ch
    d_t, d_img, d_a, d_b = (torch.from_numpy(v).cuda() for v in (tmpl, buf, a, b))
    d_res = torch.zeros(n * TEMPLATE_RESULT_DTYPE.itemsize + 64, dtype=torch.uint8, device="cuda")
    d_res[n * TEMPLATE_RESULT_DTYPE.itemsize:] = 0x5A
    d_out = torch.full((size + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.cbh_template_match_dev(d_t.data_ptr(), tw, th, tw * ch, ch, d_img.data_ptr(), n, off.ctypes.data, w.ctypes.data,
                                  h.ctypes.data, st.ctypes.data, ch, d_a.data_ptr(), d_b.data_ptr(), first.ctypes.data,
                                  scales.ctypes.data, d_res.data_ptr(), d_out.data_ptr() if patches else None, 0,
                                  stream.cuda_stream if stream else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    res, out = d_res.cpu().numpy(), d_out.cpu().numpy()
    assert (res[n * TEMPLATE_RESULT_DTYPE.itemsize:] == 0x5A).all() and (out[size:] == 0x5A).all()
    assert patches or (out == 0x5A).all()
    return rc, res[:n * TEMPLATE_RESULT_DTYPE.itemsize].view(TEMPLATE_RESULT_DTYPE), out[:size].reshape(n, th, tw, ch)


def test_chain_dev_entry_on_a_side_stream(gpu, chain):
    import torch

    from cbird_amd import _lib

    fx, yard, tol = chain
    args = _chain_args(fx)
    side = torch.cuda.Stream()
    rc, res, patches = _chain_dev(_lib.lib(), args, side)
    assert rc == 0
    for i, want in enumerate(yard):
        check_chain(i, want, tol, res[i], patches[i])
    rc, res2, _ = _chain_dev(_lib.lib(), args, None, patches=False)  # NULL stream, the patches stay in scratch
    assert rc == 0 and res2.tobytes() == res.tobytes()


def test_chunked_uploads_give_the_same_results(gpu, chain):
    """"tmatch_chunk_mb" 1: fifty copies of the group (8 MB of images, 300 patches of 4320 bytes) go up in several pieces; the device entry splits
    its patches likewise"""
    from cbird_amd import _lib

    L = _lib.lib()
    fx, yard, tol = chain
    args = _chain_args(fx, reps=50)
    assert args[1][0].size > 3 << 20
    default = _tuning(L, b"tmatch_chunk_mb")
    assert default >= 64
    rc, r_one, p_one = _chain_host(L, args)
    assert rc == 0
    assert L.cbh_set_tuning(b"tmatch_chunk_mb", 1) == 0
    try:
        rc, r_many, p_many = _chain_host(L, args)
        rc2, r_dev, _ = _chain_dev(L, args, patches=False)
    finally:
        L.cbh_set_tuning(b"tmatch_chunk_mb", int(default))
    assert rc == 0 and rc2 == 0
    assert r_many.tobytes() == r_one.tobytes() and (p_many == p_one).all() and r_dev.tobytes() == r_one.tobytes()
    for i in range(len(r_one)):
        check_chain(i, yard[i % 6], tol, r_many[i], p_many[i])


# ---- arguments and refusals ----------------------------------------------------------------------------------------------
def test_arguments(gpu, chain, est):
    from cbird_amd import _lib
    from cbird_amd.hashing import estimate_rigid, pack_point_lists, template_match, warp_affine

    L = _lib.lib()
    INVAL = _lib.CBH_E_INVAL
    # nothing to do
    assert L.cbh_estimate_rigid(None, None, 0, None, None, None, None, 0) == 0
    assert L.cbh_estimate_rigid_dev(None, None, 0, None, None, None, None, 0, None) == 0
    assert L.cbh_warp_affine_dev(None, 0, None, None, None, None, 3, None, None, 8, 8, None, None, 0, None) == 0
    assert L.cbh_template_match(None, 8, 8, 8, 1, None, 0, 0, None, None, None, None, 1, None, None, None, None, None, None,
                                0) == 0
    m, found = estimate_rigid([], [])
    assert m.shape == (0, 2, 3) and len(found) == 0
    assert len(template_match(chain[0][0], [], [], [])) == 0
    res, patches = template_match(chain[0][0], [], [], [], patches=True)  # the empty cases agree with each other
    assert len(res) == 0 and patches.shape == (0,) + chain[0][0].shape
    out, ok = warp_affine([], np.zeros((0, 2, 3)), 33, 47)
    assert out.shape == (0, 47, 33) and ok.shape == (0,)
    with pytest.raises(ValueError):
        estimate_rigid([np.zeros((3, 2))], [np.zeros((4, 2))])
    # estimate: lists that do not start at 0, run backwards, or have no outputs
    a, b, first = pack_point_lists(est[1][2:5], est[2][2:5])
    mm, ff = np.zeros(18), np.zeros(3, np.uint8)
    call = lambda fi, m_=mm, f_=ff: L.cbh_estimate_rigid(a.ctypes.data, b.ctypes.data, 3, fi.ctypes.data,  # noqa: E731
                                                         m_.ctypes.data if m_ is not None else None,
                                                         f_.ctypes.data if f_ is not None else None, None, 0)
    assert call(first) == 0
    assert call(first + np.uint64(1)) == INVAL and call(first[::-1].copy()) == INVAL
    assert call(first, None) == INVAL and call(first, mm, None) == INVAL
    # chain: channel counts, a row stride below the row, an image that ends outside the buffer, a scale of 0, sizes
    args = _chain_args(chain[0])
    tmpl, (buf, off, w, h, st), pts, scales, n = args
    assert _chain_host(L, args)[0] == 0
    assert _chain_host(L, (tmpl, (buf[:-1], off, w, h, st), pts, scales, n))[0] == INVAL
    assert _chain_host(L, (tmpl, (buf, off, w, h, (w * 3 - 1).astype(np.uint32)), pts, scales, n))[0] == INVAL
    bad = scales.copy()
    bad[1] = 0
    assert _chain_host(L, (tmpl, (buf, off, w, h, st), pts, bad, n))[0] == INVAL
    assert _chain_host(L, (tmpl, (buf, off, w, h, st), (pts[0], pts[1], pts[2][:-1]), scales, n - 1))[0] == 0  # fewer lists
    big = w.copy()
    big[0] = 40000
    assert _chain_host(L, (tmpl, (buf, off, big, h, (big * 3).astype(np.uint32)), pts, scales, n))[0] == INVAL
    for ch in (0, 2, 5):
        assert L.cbh_warp_affine_dev(1, 1, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, ch, 1, 1, 8, 8, 16,
                                     None, 0, None) == INVAL
    assert L.cbh_warp_affine_dev(1, 1, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, 3, 1, 1, 8, 8, 17,
                                 None, 0, None) == INVAL  # patches not 16-byte aligned
    assert L.cbh_warp_affine_dev(1, 1, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, 3, 1, 1, 0, 8, 16,
                                 None, 0, None) == INVAL


@pytest.mark.parametrize("entry", ["estimate", "estimate_dev", "warp_dev", "match", "match_dev"])
def test_every_allocation_may_be_refused(gpu, chain, est, entry):
    """the walk of tests/test_quality.py for each new entry point: "fault_alloc_after" 0, 1, 2, ... until the call makes
    fewer allocations.  Every refused call returns CBH_E_NOMEM, leaves no scratch handed out, and the next call gives
    the same results"""
    from cbird_amd import _lib
    from cbird_amd.hashing import RIGID_DETAIL_DTYPE, pack_point_lists

    L = _lib.lib()
    fx, yard, tol = chain
    names, al, bl, _, _ = est
    keep = [i for i, n in enumerate(names) if n not in ("same_a", "collinear", "n4097_60")]  # (the quick ones)
    al, bl = [al[i] for i in keep], [bl[i] for i in keep]
    args = _chain_args(fx)

    def call():
        if entry == "estimate":
            a, b, first = pack_point_lists(al, bl)
            n = len(first) - 1
            m, f, d = np.zeros(n * 6), np.zeros(n, np.uint8), np.zeros(n, RIGID_DETAIL_DTYPE)
            rc = L.cbh_estimate_rigid(a.ctypes.data, b.ctypes.data, n, first.ctypes.data, m.ctypes.data, f.ctypes.data,
                                      d.ctypes.data, 0)
            return rc, m.tobytes() + f.tobytes() + d.tobytes()
        if entry == "estimate_dev":
            rc, m, f, d = _estimate_dev(L, al, bl)
            return rc, m.tobytes() + f.tobytes() + d.tobytes()
        if entry == "warp_dev":
            ms = np.stack([r["m"] for r in yard])
            rc, out, ok = _warp_dev(L, args[1], 3, ms, np.array([r["found"] for r in yard], np.uint8), R.CHAIN_TW,
                                    R.CHAIN_TH)
            return rc, out.tobytes() + ok.tobytes()
        rc, res, out = _chain_host(L, args) if entry == "match" else _chain_dev(L, args)
        return rc, res.tobytes() + out.tobytes()

    rc, first_result = call()  # (one-time costs are not part of the walk)
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
        assert rc == 0 and again == first_result, k
    else:
        pytest.fail("the call never ran out of allocations to refuse")
    assert refused >= {"estimate": 6, "estimate_dev": 1, "warp_dev": 3, "match": 7, "match_dev": 11}[entry]
