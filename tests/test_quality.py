"""GPU suite for the batched qualityScore (cbird_amd/csrc/quality.hip; src/cimgops.cpp:313-596): scores, every field of
the detail record and the three diagnostic planes must EQUAL the numpy restatement of tests/test_quality_rules.py and the
golden file the real CImg.h produced -- no tolerance: everything is integer but two float means and one float formula of
fixed evaluation order.  The cases are the smallest shapes at which the kernels can still go wrong (R.cases): sides 2 ..
20 (crop 0 with the blank column / row, crop 1 and 2), working widths around the 16-pixel load width, 640 x 480, tall-thin
and wide-flat, 1 / 3 / 4 channels, no score for a side of 1, a constant image and a constant red channel, blocky images
with long edges and the three run edge cases, the mean that rounds up in float, runs across every strip boundary."""
import ctypes as C

import numpy as np
import pytest

import test_quality_rules as R

pytestmark = pytest.mark.gpu


def _tuning(L, key):
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0
    return v.value


@pytest.fixture(scope="module")
def strip(gpu):
    from cbird_amd import _lib

    return int(_tuning(_lib.lib(), b"quality_strip_rows"))


@pytest.fixture(scope="module")
def data(strip):
    """(cases by channel count, yardstick): built and computed once for the module, never written to"""
    cases, yard = R.cases(strip), R.yardstick(strip)
    by_ch = {ch: [n for n, a in cases.items() if (1 if a.ndim == 2 else a.shape[2]) == ch] for ch in (1, 3, 4)}
    assert all(len(v) >= 12 for v in by_ch.values())
    return cases, yard, by_ch


def _host(L, packed, ch, detail=True, device=0):
    from cbird_amd.quality import DETAIL_DTYPE

    buf, off, w, h, st = packed
    scores = np.full(len(off), 12345, np.int32)
    det = np.zeros(len(off), DETAIL_DTYPE)
    rc = L.cbh_quality_scores(buf.ctypes.data, buf.size, len(off), off.ctypes.data, w.ctypes.data, h.ctypes.data,
                              st.ctypes.data, ch, scores.ctypes.data, det.ctypes.data if detail else None, device)
    return rc, scores, det


def _dev(L, packed, ch, imgs, planes=True, stream=None):
    """cbh_quality_scores_dev on torch tensors -> (rc, scores, detail, per-image planes or None); a guard band behind the
    planes must stay as it was"""
    import torch

    from cbird_amd.quality import DETAIL_DTYPE

    buf, off, w, h, st = packed
    n = len(off)
    poff, pbytes = R.plane_offsets(imgs)
    d_img = torch.from_numpy(buf).cuda()
    d_scores = torch.full((n,), 12345, dtype=torch.int32, device="cuda")
    d_det = torch.zeros(n * DETAIL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_planes = torch.full((pbytes + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.cbh_quality_scores_dev(d_img.data_ptr(), n, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, ch,
                                  d_scores.data_ptr(), d_det.data_ptr(), d_planes.data_ptr() if planes else None,
                                  poff.ctypes.data if planes else None, 0, stream.cuda_stream if stream else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    flat = d_planes.cpu().numpy()
    assert (flat[pbytes:] == 0x5A).all() and (planes or (flat == 0x5A).all())
    out = None
    if planes and rc == 0:
        out = []
        for im, o in zip(imgs, poff):
            _, _, qw, qh = R.crop_dims(im.shape[1], im.shape[0])
            if qw < 3 or qh < 3:
                qw = qh = 0
            out.append(flat[int(o): int(o) + 3 * qw * qh].reshape(3, qh, qw))
    return rc, d_scores.cpu().numpy(), d_det.cpu().numpy().view(DETAIL_DTYPE), out


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_host_entry_on_ragged_batches(gpu, data, ch):
    """padded rows, gaps and odd base offsets, everything that is not a pixel 0xA5; alpha is random"""
    from cbird_amd import _lib

    cases, yard, by_ch = data
    names = by_ch[ch]
    packed = R.pack_ragged([cases[n] for n in names], np.random.default_rng(ch))
    assert (packed[1] % 2 == 1).any() and (packed[4] % 2 == 1).any() and (packed[1] % 16 == 0).any()
    rc, scores, det = _host(_lib.lib(), packed, ch)
    assert rc == 0
    for i, n in enumerate(names):
        R.check_result(n, yard[n], scores[i], det[i])
    rc, scores2, _ = _host(_lib.lib(), packed, ch, detail=False)
    assert rc == 0 and (scores2 == scores).all()


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_dev_entry_on_a_side_stream_with_planes(gpu, data, ch):
    import torch

    from cbird_amd import _lib

    cases, yard, by_ch = data
    names = by_ch[ch]
    imgs = [cases[n] for n in names]
    packed = R.pack_ragged(imgs, np.random.default_rng(10 + ch))
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    rc, scores, det, planes = _dev(_lib.lib(), packed, ch, imgs, planes=True, stream=side)
    assert rc == 0
    for i, n in enumerate(names):
        R.check_result(n, yard[n], scores[i], det[i], planes[i])
    rc, scores2, det2, _ = _dev(_lib.lib(), packed, ch, imgs, planes=False, stream=side)  # the kernel without the stores
    assert rc == 0 and (scores2 == scores).all() and det2.tobytes() == det.tobytes()
    rc, scores3, det3, _ = _dev(_lib.lib(), packed, ch, imgs, planes=False, stream=None)  # NULL stream: synchronous
    assert rc == 0 and (scores3 == scores).all() and det3.tobytes() == det.tobytes()


def test_no_score_cases_and_the_rounding_case(gpu, data):
    """what the cases are for, asserted here so that none can silently stop testing it, then the device's answers"""
    from cbird_amd.quality import NO_SCORE, quality_scores

    cases, yard, _ = data
    none = [n for n in cases if n.startswith(("side1_", "constant", "red_constant"))]
    assert len(none) >= 11 and all(yard[n]["score"] == R.NO_SCORE for n in none) and NO_SCORE == R.NO_SCORE
    r = yard["rounding_c3"]
    cnt = (r["qw"] - 1) * (r["qh"] - 1)
    k = (r["h_sum"] + 1) // cnt
    assert r["h_sum"] == k * cnt - 1 and 120 <= k <= 140 and r["qw"] >= 600 and r["qh"] >= 600
    assert np.float32(np.float64(r["h_sum"]) / np.float64(cnt)) == np.float32(k) and r["h_sum"] // cnt == k - 1
    assert R.quality_stencil(cases["rounding_c3"], mean_mode="int")["num_edges"] != r["num_edges"]
    names = none + ["rounding_c3"]
    scores, det = quality_scores([cases[n] for n in names], detail=True)  # (a mix of channel counts)
    for i, n in enumerate(names):
        R.check_result(n, yard[n], scores[i], det[i])
    assert (scores[:-1] == NO_SCORE).all() and det["h_mean"][-1] == np.float32(k)


def test_runs_cross_every_strip_boundary(gpu, data, strip):
    """the strip height is the library's; the case is checked against it, then the planes of the device"""
    from cbird_amd.quality import quality_planes

    cases, yard, _ = data
    assert strip >= 4
    for n in ("strips_c3", "strips_c1"):
        R.check_strip_case(yard[n], strip)
    names = ["strips_c3", "strips_c1", "vga_c3"]
    assert yard["vga_c3"]["qh"] > 8 * strip
    scores, det, planes = quality_planes([cases[n] for n in names])
    for i, n in enumerate(names):
        R.check_result(n, yard[n], scores[i], det[i], planes[i])


def test_long_edge_rule_cases(gpu, data):
    from cbird_amd.quality import quality_scores

    cases, yard, _ = data
    for suffix, field in (("_y_c3", "h_long"), ("_x_c1", "v_long")):
        names = [k + suffix for k in R.RUN_EXPECT]
        scores, det = quality_scores([cases[n] for n in names], detail=True)
        for i, n in enumerate(names):
            R.check_result(n, yard[n], scores[i], det[i])
        assert [int(d[field]) for d in det] == list(R.RUN_EXPECT.values())


def test_chunked_uploads_give_the_same_results(gpu, data):
    """"quality_chunk_mb" 1: the three-channel cases (several MB) go up in several pieces, and the working planes of the
    device entry are split likewise"""
    from cbird_amd import _lib

    L = _lib.lib()
    cases, yard, by_ch = data
    names = by_ch[3]
    imgs = [cases[n] for n in names]
    packed = R.pack_ragged(imgs, np.random.default_rng(3))
    assert packed[0].size > 3 << 20 and sum(yard[n]["qw"] * yard[n]["qh"] for n in names) > 1 << 20
    default = _tuning(L, b"quality_chunk_mb")
    assert default >= 64
    rc, s_one, d_one = _host(L, packed, 3)
    assert rc == 0
    assert L.cbh_set_tuning(b"quality_chunk_mb", 1) == 0
    try:
        rc, s_many, d_many = _host(L, packed, 3)
        rc2, s_dev, d_dev, planes = _dev(L, packed, 3, imgs)
    finally:
        L.cbh_set_tuning(b"quality_chunk_mb", int(default))
    assert rc == 0 and rc2 == 0
    assert (s_many == s_one).all() and d_many.tobytes() == d_one.tobytes()
    assert (s_dev == s_one).all() and d_dev.tobytes() == d_one.tobytes()
    for i, n in enumerate(names):
        R.check_result(n, yard[n], s_many[i], d_many[i], planes[i])


def test_golden_images_from_the_real_cimg(gpu):
    from cbird_amd.quality import quality_planes, quality_scores

    gold = R.load_golden()
    imgs = [g["image"] for g in gold]
    scores, det, planes = quality_planes(imgs)
    for i, g in enumerate(gold):
        R.check_result(f"golden {i}", g, scores[i], det[i], planes[i])
    s2, d2 = quality_scores(imgs, detail=True)
    assert (s2 == scores).all() and d2.tobytes() == det.tobytes()
    assert (quality_scores(imgs) == scores).all()


def test_arguments(gpu, data):
    from cbird_amd import _lib

    L = _lib.lib()
    cases, _, by_ch = data
    packed = R.pack_ragged([cases[by_ch[3][0]]], np.random.default_rng(0))
    for ch in (0, 2, 5):
        assert _host(L, packed, ch)[0] == _lib.CBH_E_INVAL
    buf, off, w, h, st = packed
    assert _host(L, (buf[:-1], off, w, h, st), 3)[0] == _lib.CBH_E_INVAL  # the last pixel lies outside
    assert _host(L, (buf, off, w, h, (w * 3 - 1).astype(np.uint32)), 3)[0] == _lib.CBH_E_INVAL
    assert L.cbh_quality_scores(None, 0, 0, None, None, None, None, 3, None, None, 0) == 0  # nothing to do


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_every_allocation_may_be_refused(gpu, data, entry):
    """the walk of tests/test_error_paths.py: "fault_alloc_after" 0, 1, 2, ... until the call makes fewer allocations.
    Every refused call returns CBH_E_NOMEM, leaves no scratch handed out, and the next call gives the same results"""
    from cbird_amd import _lib

    L = _lib.lib()
    cases, yard, by_ch = data
    names = by_ch[4][:10]
    imgs = [cases[n] for n in names]
    packed = R.pack_ragged(imgs, np.random.default_rng(4))

    def call():
        if entry == "host":
            return _host(L, packed, 4)
        return _dev(L, packed, 4, imgs)[:3]

    rc, s0, d0 = call()  # (one-time costs are not part of the walk)
    assert rc == 0
    for i, n in enumerate(names):
        R.check_result(n, yard[n], s0[i], d0[i])
    refused = 0
    for k in range(100):
        live0, fired0 = _tuning(L, b"arena_live_bytes"), _tuning(L, b"fault_fired")
        L.cbh_set_tuning(b"fault_alloc_after", k)
        try:
            rc, _, _ = call()
        finally:
            L.cbh_set_tuning(b"fault_alloc_after", -1)
        if _tuning(L, b"fault_fired") == fired0:
            assert rc == 0
            break
        refused += 1
        assert rc == _lib.CBH_E_NOMEM, (k, rc)
        assert _tuning(L, b"arena_live_bytes") == live0, k
        rc, s1, d1 = call()
        assert rc == 0 and (s1 == s0).all() and d1.tobytes() == d0.tobytes(), k
    else:
        pytest.fail("the call never ran out of allocations to refuse")
    assert refused >= (7 if entry == "host" else 4)
