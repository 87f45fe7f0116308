"""dctHash64 over batches of decoded 8-bit grayscale tiles (src/cvutil.cpp:435-545).

``dct_hash64`` mirrors the reference call (one image -> one u64); ``dct_hash64_batch`` is the
MI355X-native shape: many pre-decoded images per launch.  Both go through
``cbh_dcthash_batch`` in libcbird_hip.so; there is no CPU implementation here.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check


def dct_hash64_batch(imgs: np.ndarray, device: int = 0) -> np.ndarray:
    """imgs: u8 array [n, h, w] (C-contiguous rows; row/image strides are taken from the array).
    Returns u64[n]."""
    imgs = np.asarray(imgs)
    if imgs.dtype != np.uint8 or imgs.ndim != 3:
        raise ValueError("expected uint8 array [n, h, w]")
    if imgs.strides[2] != 1:
        imgs = np.ascontiguousarray(imgs)
    n, h, w = imgs.shape
    out = np.zeros(n, np.uint64)
    if n == 0:
        return out
    check(_lib.lib().cbh_dcthash_batch(imgs.ctypes.data, n, w, h, imgs.strides[1], imgs.strides[0],
                                       out.ctypes.data, device), "dcthash_batch")
    return out


def dct_hash64(img: np.ndarray, device: int = 0) -> int:
    """uint64_t dctHash64(const cv::Mat& cvImg) for an 8UC1 image."""
    img = np.asarray(img)
    if img.ndim != 2:
        raise ValueError("expected a single-channel 2-D uint8 image")
    return int(dct_hash64_batch(img[None, ...], device)[0])


def process_images(imgs: np.ndarray, autocrop: int | None = 20, device: int = 0):
    """The hash Scanner::processImage stores for decoded images (src/scanner.cpp:852-862): grayscale ->
    autocrop(gray, 20) when enabled -> dctHash64.  imgs: uint8 [n,h,w] (gray) or [n,h,w,3|4] (BGR/BGRA).
    Returns (hashes u64[n], rects int32[n,4] = left, top, right, bottom of the kept region)."""
    imgs = np.ascontiguousarray(imgs)
    if imgs.dtype != np.uint8 or imgs.ndim not in (3, 4):
        raise ValueError("expected uint8 [n,h,w] or [n,h,w,c]")
    n, h, w = imgs.shape[:3]
    ch = 1 if imgs.ndim == 3 else imgs.shape[3]
    out = np.zeros(n, np.uint64)
    rects = np.zeros((n, 4), np.int32)
    if n:
        check(_lib.lib().cbh_process_images(imgs.ctypes.data, n, w, h, w * ch, w * h * ch, ch,
                                            -1 if autocrop is None else int(autocrop), out.ctypes.data,
                                            rects.ctypes.data, device), "process_images")
    return out, rects


def template_scores(cands: np.ndarray, tmpl: np.ndarray, device: int = 0):
    """TemplateMatcher::match's score (src/templatematcher.cpp:331-374) for n candidate patches against one template:
    cands uint8 [n,h,w] or [n,h,w,3|4] as warpAffine left them (0 outside the patch), tmpl uint8 [h,w] or [h,w,3|4].
    Returns (scores int32[n] = hamm64(candHash, tmplHash), candHashes u64[n], tmplHashes u64[n])."""
    cands = np.ascontiguousarray(cands)
    tmpl = np.ascontiguousarray(tmpl)
    if cands.dtype != np.uint8 or cands.ndim not in (3, 4) or tmpl.dtype != np.uint8 or tmpl.ndim not in (2, 3):
        raise ValueError("expected uint8 cands [n,h,w(,c)] and tmpl [h,w(,c)]")
    n, h, w = cands.shape[:3]
    if tmpl.shape[:2] != (h, w):
        raise ValueError("the candidate patches are template-sized (warpAffine's dsize = tmplImg.size())")
    cc = 1 if cands.ndim == 3 else cands.shape[3]
    tc = 1 if tmpl.ndim == 2 else tmpl.shape[2]
    scores = np.zeros(n, np.int32)
    ch = np.zeros(n, np.uint64)
    th = np.zeros(n, np.uint64)
    if n:
        check(_lib.lib().cbh_template_scores(cands.ctypes.data, n, w, h, w * cc, w * h * cc, cc, tmpl.ctypes.data, w * tc,
                                             tc, ch.ctypes.data, th.ctypes.data, scores.ctypes.data, device),
              "template_scores")
    return scores, ch, th


def process_images_ex(imgs: np.ndarray, autocrop: int | None = 20, resize: int = 400, device: int = 0):
    """process_images plus, from the same upload, sizeLongestSide(cvGray, resize) of every (autocropped) grey image --
    what Scanner::processImage hands to ORB (src/scanner.cpp:876).  Returns (hashes, rects, list of uint8 images)."""
    imgs = np.ascontiguousarray(imgs)
    if imgs.dtype != np.uint8 or imgs.ndim not in (3, 4):
        raise ValueError("expected uint8 [n,h,w] or [n,h,w,c]")
    n, h, w = imgs.shape[:3]
    ch = 1 if imgs.ndim == 3 else imgs.shape[3]
    out = np.zeros(n, np.uint64)
    rects = np.zeros((n, 4), np.int32)
    slots = np.zeros((n, resize * resize), np.uint8)
    dims = np.zeros((n, 2), np.int32)
    if n:
        check(_lib.lib().cbh_process_images_ex(imgs.ctypes.data, n, w, h, w * ch, w * h * ch, ch,
                                               -1 if autocrop is None else int(autocrop), out.ctypes.data,
                                               rects.ctypes.data, int(resize), slots.ctypes.data, dims.ctypes.data,
                                               device), "process_images_ex")
    small = [slots[i, : dims[i, 0] * dims[i, 1]].reshape(dims[i, 1], dims[i, 0]).copy() for i in range(n)]
    return out, rects, small


def keypoint_rects(cols: int, rows: int, keypoints) -> np.ndarray:
    """The rectangles Media::makeKeyPointHashes derives from keypoints (src/media.cpp:880-901): keypoints is
    [k, 3] float32 (pt.x, pt.y, size); returns int32 [m, 3] (x, y, side)."""
    kp = np.ascontiguousarray(keypoints, np.float32).reshape(-1, 3)
    r = np.zeros((max(1, len(kp)), 3), np.int32)
    n = _lib.lib().cbh_keypoint_rects(int(cols), int(rows), kp.ctypes.data, len(kp), r.ctypes.data)
    if n < 0:
        check(int(n), "keypoint_rects")
    return r[:n].copy()


def make_keypoint_hashes(images, keypoints, device: int = 0, return_images: bool = False):
    """Media::makeKeyPointHashes (src/media.cpp:874-923) for a batch: images is a list of 2-D uint8 grey images (any
    sizes), keypoints a list of [k_i, 3] float32 arrays (pt.x, pt.y, size) in detector order.  Returns a list of
    uint64 arrays (one hash per accepted keypoint, in order); with return_images also the images as the in-place
    blurs of dctHash64(sub, inPlace=true) left them."""
    if len(images) != len(keypoints):
        raise ValueError("one keypoint array per image")
    n = len(images)
    if n == 0:
        return ([], []) if return_images else []
    imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
    if any(im.ndim != 2 or im.size == 0 for im in imgs):
        raise ValueError("expected non-empty single-channel 2-D uint8 images")
    kps = [np.ascontiguousarray(k, np.float32).reshape(-1, 3) for k in keypoints]
    sizes = np.array([im.size for im in imgs], np.uint64)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum((sizes[:-1] + np.uint64(15)) // np.uint64(16) * np.uint64(16))  # 16-byte aligned starts
    total = int(off[-1] + sizes[-1])
    buf = np.zeros(total, np.uint8)
    for im, o in zip(imgs, off):
        buf[int(o): int(o) + im.size] = im.reshape(-1)
    w = np.array([im.shape[1] for im in imgs], np.uint32)
    h = np.array([im.shape[0] for im in imgs], np.uint32)
    kp_first = np.zeros(n + 1, np.uint32)
    kp_first[1:] = np.cumsum([len(k) for k in kps])
    kp = np.concatenate(kps) if kp_first[-1] else np.zeros((1, 3), np.float32)
    out = np.zeros(max(1, int(kp_first[-1])), np.uint64)
    out_first = np.zeros(n + 1, np.uint32)
    after = np.zeros(total, np.uint8) if return_images else None
    check(_lib.lib().cbh_keypoint_hashes(buf.ctypes.data, total, n, off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                         w.ctypes.data, kp.ctypes.data, kp_first.ctypes.data, out.ctypes.data,
                                         out_first.ctypes.data, after.ctypes.data if return_images else None,
                                         device), "keypoint_hashes")
    hashes = [out[int(out_first[i]): int(out_first[i + 1])].copy() for i in range(n)]
    if not return_images:
        return hashes
    return hashes, [after[int(o): int(o) + im.size].reshape(im.shape).copy() for im, o in zip(imgs, off)]


def size_longest_side(imgs: np.ndarray, size: int = 400, device: int = 0) -> np.ndarray:
    """sizeLongestSide(img, size) (src/cvutil.cpp:1932-1950, INTER_LANCZOS4) for uint8 grey images [n, h, w] of one
    geometry; returns uint8 [n, h', w'].  size defaults to IndexParams::resizeLongestSide (src/scanner.h:71)."""
    import ctypes as C

    imgs = np.asarray(imgs)
    if imgs.dtype != np.uint8 or imgs.ndim != 3:
        raise ValueError("expected uint8 array [n, h, w]")
    if imgs.strides[2] != 1:
        imgs = np.ascontiguousarray(imgs)
    n, h, w = imgs.shape
    ow, oh = C.c_int(0), C.c_int(0)
    L = _lib.lib()
    L.cbh_longest_side_dims(w, h, int(size), C.byref(ow), C.byref(oh))
    out = np.zeros((n, max(oh.value, 0), max(ow.value, 0)), np.uint8)
    check(L.cbh_size_longest_side(imgs.ctypes.data, n, w, h, imgs.strides[1], imgs.strides[0] if n else 0, int(size),
                                  out.ctypes.data, C.byref(ow), C.byref(oh), device), "size_longest_side")
    return out


# ---- TemplateMatcher::match between the descriptor match and the score (src/templatematcher.cpp:264-333) -------------
RIGID_DETAIL_DTYPE = np.dtype([("iterations", np.int32), ("good_count", np.int32), ("draws", np.uint32),
                               ("reserved", np.uint32)])
TEMPLATE_RESULT_DTYPE = np.dtype([("m", np.float64, 6), ("tx", np.float64, 6), ("cand_hash", np.uint64),
                                  ("tmpl_hash", np.uint64), ("roi", np.int32, 8), ("found", np.int32),
                                  ("tx_found", np.int32), ("score", np.int32), ("iterations", np.int32),
                                  ("good_count", np.int32), ("reserved", np.int32)])
assert RIGID_DETAIL_DTYPE.itemsize == 16 and TEMPLATE_RESULT_DTYPE.itemsize == 168
NO_TRANSFORM_SCORE = (1 << 31) - 1  # INT_MAX, what the reference caches for a candidate without a transform


def pack_point_lists(a_lists, b_lists):
    """lists of [k_i, 2] float32 point arrays -> (a_xy, b_xy float32 [total, 2], first uint64 [n + 1])"""
    if len(a_lists) != len(b_lists):
        raise ValueError("one list of B points per list of A points")
    a = [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in a_lists]
    b = [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in b_lists]
    if any(len(p) != len(q) for p, q in zip(a, b)):
        raise ValueError("A and B of a list hold the same number of points")
    first = np.zeros(len(a) + 1, np.uint64)
    first[1:] = np.cumsum([len(p) for p in a], dtype=np.uint64)
    cat = lambda ps: np.concatenate(ps) if ps and first[-1] else np.zeros((1, 2), np.float32)  # noqa: E731
    return cat(a), cat(b), first


def estimate_rigid(a_lists, b_lists, detail: bool = False, device: int = 0):
    """cv::estimateRigidTransform(A, B, fullAffine=false) (src/templatematcher.cpp:264, 309) for n point-pair lists in one
    call.  Returns (m float64 [n, 2, 3], found bool [n]) and, with detail=True, RIGID_DETAIL_DTYPE [n] (outer iterations
    run, inliers of the stopping iteration, RNG values drawn)."""
    a, b, first = pack_point_lists(a_lists, b_lists)
    n = len(first) - 1
    m = np.zeros((n, 2, 3), np.float64)
    found = np.zeros(n, np.uint8)
    det = np.zeros(n, RIGID_DETAIL_DTYPE)
    if n:
        check(_lib.lib().cbh_estimate_rigid(a.ctypes.data, b.ctypes.data, n, first.ctypes.data, m.ctypes.data,
                                            found.ctypes.data, det.ctypes.data if detail else None, device),
              "estimate_rigid")
    return (m, found.astype(bool), det) if detail else (m, found.astype(bool))


def warp_affine(images, m, tw: int, th: int, found=None, device: int = 0):
    """invertAffineTransform(m) + warpAffine(img, m, (tw, th), INTER_AREA, BORDER_CONSTANT, (0,0,0,255))
    (src/templatematcher.cpp:331-333) for a list of uint8 images of one channel count (1, 3 or 4) and any sizes: m
    [n, 2, 3] maps the template to each candidate.  Returns (patches uint8 [n, th, tw(, ch)], warped bool [n]) -- for an empty list ([0, th, tw], []); the patch
    of a candidate that is not found, or whose coordinates leave the reference's integer range, is zero."""
    import torch

    from .quality import pack_images

    imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
    n = len(imgs)
    chs = {1 if im.ndim == 2 else im.shape[2] for im in imgs}
    if n == 0:  # nothing to do, as in the C entry (no image says how many channels: the patches have no channel axis)
        return np.zeros((0, th, tw), np.uint8), np.zeros(0, bool)
    if len(chs) != 1 or not chs <= {1, 3, 4} or any(im.size == 0 for im in imgs):
        raise ValueError("expected non-empty uint8 images of one channel count: [h, w], [h, w, 3] or [h, w, 4]")
    ch = chs.pop()
    m = np.ascontiguousarray(m, np.float64).reshape(n, 6)
    found = np.ones(n, np.uint8) if found is None else np.ascontiguousarray(found).astype(np.uint8).reshape(n)
    buf, off, w, h, stride = pack_images(imgs)
    dev = torch.device("cuda", device)
    d_img, d_m, d_found = (torch.from_numpy(v).to(dev) for v in (buf, m, found))
    d_out = torch.zeros(n * th * tw * ch, dtype=torch.uint8, device=dev)
    d_ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    check(_lib.lib().cbh_warp_affine_dev(d_img.data_ptr(), n, off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                         stride.ctypes.data, ch, d_m.data_ptr(), d_found.data_ptr(), int(tw), int(th),
                                         d_out.data_ptr(), d_ok.data_ptr(), device, None), "warp_affine")
    torch.cuda.synchronize(dev)
    shape = (n, th, tw) if imgs[0].ndim == 2 else (n, th, tw, ch)
    return d_out.cpu().numpy().reshape(shape), d_ok.cpu().numpy().astype(bool)


def template_match(tmpl, cands, tmpl_points, match_points, cand_scales=None, patches: bool = False, device: int = 0):
    """TemplateMatcher::match from the point lists to the score (src/templatematcher.cpp:264-374) for ONE template and n
    candidate images (a list of uint8 images of one channel count, any sizes): both rigid estimates, the roi, the warp,
    the masked hashes and their distance, in one call that does not leave the device.  tmpl_points[i] / match_points[i]:
    [k_i, 2] float32, the matched keypoints of candidate i in the caller's order (:243-250); cand_scales[i]: candScale.
    Returns TEMPLATE_RESULT_DTYPE [n] (score = NO_TRANSFORM_SCORE where found is 0) and, with patches=True, the warped
    patches uint8 [n, th, tw(, ch)]."""
    from .quality import pack_images

    tmpl = np.ascontiguousarray(tmpl, np.uint8)
    imgs = [np.ascontiguousarray(im, np.uint8) for im in cands]
    n = len(imgs)
    res = np.zeros(n, TEMPLATE_RESULT_DTYPE)
    if tmpl.ndim not in (2, 3) or tmpl.size == 0:
        raise ValueError("expected a uint8 template [h, w] or [h, w, c]")
    th, tw = tmpl.shape[:2]
    tc = 1 if tmpl.ndim == 2 else tmpl.shape[2]
    if n == 0:  # (no candidate says how many channels: the empty patches take the template's layout)
        return (res, np.zeros((0,) + tmpl.shape, np.uint8)) if patches else res
    chs = {1 if im.ndim == 2 else im.shape[2] for im in imgs}
    if len(chs) != 1 or not chs <= {1, 3, 4} or tc not in (1, 3, 4) or any(im.size == 0 for im in imgs):
        raise ValueError("expected non-empty uint8 images of one channel count: [h, w], [h, w, 3] or [h, w, 4]")
    ch = chs.pop()
    a, b, first = pack_point_lists(tmpl_points, match_points)
    if len(first) - 1 != n:
        raise ValueError("one point list per candidate")
    scales = np.ones(n, np.float32) if cand_scales is None else np.ascontiguousarray(cand_scales, np.float32).reshape(n)
    buf, off, w, h, stride = pack_images(imgs)
    out = np.zeros((n, th, tw) if imgs[0].ndim == 2 else (n, th, tw, ch), np.uint8)
    check(_lib.lib().cbh_template_match(tmpl.ctypes.data, tw, th, tw * tc, tc, buf.ctypes.data, buf.size, n,
                                        off.ctypes.data, w.ctypes.data, h.ctypes.data, stride.ctypes.data, ch,
                                        a.ctypes.data, b.ctypes.data, first.ctypes.data, scales.ctypes.data,
                                        res.ctypes.data, out.ctypes.data if patches else None, device), "template_match")
    return (res, out) if patches else res


# ---- TemplateMatcher::match from the decoded images to the score (src/templatematcher.cpp:105-374) --------------------
TEMPLATE_IMAGE_RESULT_DTYPE = np.dtype([("r", TEMPLATE_RESULT_DTYPE), ("cand_scale", np.float32), ("status", np.int32),
                                        ("w", np.int32), ("h", np.int32), ("n_keypoints", np.uint32),
                                        ("n_matches", np.uint32)])  # struct cbh_tm_image_result
TM_PARAMS_DTYPE = np.dtype([("needle_features", np.int32), ("haystack_features", np.int32), ("cv_thresh", np.int32),
                            ("tm_scale_pct", np.int32)])  # struct cbh_tm_params
assert TEMPLATE_IMAGE_RESULT_DTYPE.itemsize == 192 and TM_PARAMS_DTYPE.itemsize == 16
(TM_SCORED, TM_NO_TEMPLATE_KEYPOINTS, TM_NO_KEYPOINTS, TM_NO_MATCHES, TM_FEW_POINTS, TM_NO_TRANSFORM,
 TM_EMPTY_RESIZE) = range(7)  # CBH_TM_*


def tm_params(params=None) -> np.ndarray:
    """struct cbh_tm_params from a SearchParams (or anything with its template matcher fields); None = the defaults"""
    from .index import SearchParams

    p = SearchParams() if params is None else params
    out = np.zeros(1, TM_PARAMS_DTYPE)
    out[0] = (p.needleFeatures, p.haystackFeatures, p.cvThresh, p.tmScalePct)
    return out


def template_match_images(tmpl, cands, params=None, patches: bool = False, device: int = 0):
    """TemplateMatcher::match from the decoded images to the score (src/templatematcher.cpp:105-374) for ONE template and
    n candidate images (uint8, one channel count, the template's included; any sizes) in one call that does not come back
    to the host between the upload and the results: the candidate's resize, ORB on both sides, the descriptor match, the
    point lists, both rigid estimates, the warp, the masked hashes and their distance.  params: a SearchParams
    (needleFeatures, haystackFeatures, cvThresh, tmScalePct).  Needs orb.set_pattern.  Returns
    TEMPLATE_IMAGE_RESULT_DTYPE [n] (status TM_*; r.score = NO_TRANSFORM_SCORE unless TM_SCORED) and, with patches=True, the
    warped patches uint8 [n, th, tw(, ch)]."""
    from .quality import pack_images

    tmpl = np.ascontiguousarray(tmpl, np.uint8)
    imgs = [np.ascontiguousarray(im, np.uint8) for im in cands]
    n = len(imgs)
    res = np.zeros(n, TEMPLATE_IMAGE_RESULT_DTYPE)
    if tmpl.ndim not in (2, 3) or tmpl.size == 0:
        raise ValueError("expected a uint8 template [h, w] or [h, w, c]")
    th, tw = tmpl.shape[:2]
    tc = 1 if tmpl.ndim == 2 else tmpl.shape[2]
    if n == 0:
        return (res, np.zeros((0,) + tmpl.shape, np.uint8)) if patches else res
    chs = {1 if im.ndim == 2 else im.shape[2] for im in imgs}
    if chs != {tc} or tc not in (1, 3, 4) or any(im.size == 0 for im in imgs):
        raise ValueError("expected non-empty uint8 images of the template's channel count: 1, 3 (BGR) or 4 (BGRA)")
    p = tm_params(params)
    buf, off, w, h, stride = pack_images(imgs)
    out = np.zeros((n,) + tmpl.shape, np.uint8)
    check(_lib.lib().cbh_template_match_images(tmpl.ctypes.data, tw, th, tw * tc, buf.ctypes.data, buf.size, n,
                                               off.ctypes.data, w.ctypes.data, h.ctypes.data, stride.ctypes.data, tc,
                                               p.ctypes.data, res.ctypes.data, out.ctypes.data if patches else None,
                                               device), "template_match_images")
    return (res, out) if patches else res


def template_match_pairs(images, pair_tmpl, pair_cand, params=None, device: int = 0):
    """template_match_images for a batch of result groups in ONE call (Database::similar with params.templateMatch): `images`
    is one table of uint8 images of one channel count, pair p matches template images[pair_tmpl[p]] against candidate
    images[pair_cand[p]].  An image may be a template in some pairs and a candidate in others, the pairs of one template
    need not be adjacent.  Returns TEMPLATE_IMAGE_RESULT_DTYPE [n_pairs] in the caller's order, entry p equal to
    template_match_images(images[pair_tmpl[p]], [images[pair_cand[p]]], params)[0].  Needs orb.set_pattern."""
    from .quality import pack_images

    pt = np.ascontiguousarray(pair_tmpl, np.uint32).reshape(-1)
    pc = np.ascontiguousarray(pair_cand, np.uint32).reshape(-1)
    if len(pt) != len(pc):
        raise ValueError("one template and one candidate index per pair")
    res = np.zeros(len(pt), TEMPLATE_IMAGE_RESULT_DTYPE)
    if len(pt) == 0:
        return res
    imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
    chs = {1 if im.ndim == 2 else im.shape[2] for im in imgs}
    if len(chs) != 1 or not chs <= {1, 3, 4} or any(im.size == 0 or im.ndim not in (2, 3) for im in imgs):
        raise ValueError("expected non-empty uint8 images of one channel count: [h, w], [h, w, 3] or [h, w, 4]")
    if max(int(pt.max()), int(pc.max())) >= len(imgs):
        raise ValueError("a pair names an image that is not in the table")
    p = tm_params(params)
    buf, off, w, h, stride = pack_images(imgs)
    check(_lib.lib().cbh_template_match_pairs(buf.ctypes.data, buf.size, len(imgs), off.ctypes.data, w.ctypes.data,
                                              h.ctypes.data, stride.ctypes.data, chs.pop(), pt.ctypes.data, pc.ctypes.data,
                                              len(pt), p.ctypes.data, res.ctypes.data, device), "template_match_pairs")
    return res
