"""qualityScore(const Media&) (src/cimgops.cpp:313-596) for batches of images of any mix of sizes: the no-reference
score cbird shows for every member of a duplicate group (src/gui/mediagrouplistwidget.cpp:1433-1441).  What is computed,
and where it cannot follow the reference (no score for an image without edges), is stated in include/cbird_hip.h."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check

NO_SCORE = -(1 << 31)  # INT32_MIN: no edges at all, or a working plane below 3 x 3
DETAIL_DTYPE = np.dtype([("h_sum", np.uint64), ("v_sum", np.uint64), ("h_mean", np.float32), ("v_mean", np.float32),
                         ("h_long", np.int32), ("v_long", np.int32), ("num_edges", np.int32), ("qw", np.int32),
                         ("qh", np.int32), ("score", np.int32)])
assert DETAIL_DTYPE.itemsize == 48


def quality_dims(w: int, h: int) -> tuple[int, int]:
    """the working size (qw, qh) after the inclusive 10 % crop (:333-335); (0, 0) when it is below 3 x 3"""
    qw, qh = np.zeros(1, np.int32), np.zeros(1, np.int32)
    _lib.lib().cbh_quality_dims(int(w), int(h), qw.ctypes.data, qh.ctypes.data)
    return int(qw[0]), int(qh[0])


def pack_images(images, align: int = 16):
    """one buffer for a list of contiguous uint8 images of one channel count -> (buf, off, w, h, stride)"""
    n = len(images)
    sizes = np.array([im.size for im in images], np.uint64)
    off = np.zeros(n, np.uint64)
    a = np.uint64(align)
    off[1:] = np.cumsum((sizes[:-1] + a - np.uint64(1)) // a * a)
    buf = np.zeros(int(off[-1] + sizes[-1]), np.uint8)
    for im, o in zip(images, off):
        buf[int(o): int(o) + im.size] = im.reshape(-1)
    w = np.array([im.shape[1] for im in images], np.uint32)
    h = np.array([im.shape[0] for im in images], np.uint32)
    ch = images[0].shape[2] if images[0].ndim == 3 else 1
    return buf, off, w, h, (w * np.uint32(ch)).astype(np.uint32)


def _by_channels(images):
    """the images as contiguous uint8 arrays, and their indices grouped by channel count (one call per count)"""
    imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
    groups: dict[int, list[int]] = {}
    for i, im in enumerate(imgs):
        ch = 1 if im.ndim == 2 else im.shape[2] if im.ndim == 3 else 0
        if ch not in (1, 3, 4) or im.size == 0:
            raise ValueError("expected non-empty uint8 images [h, w], [h, w, 1], [h, w, 3] (BGR) or [h, w, 4] (BGRA)")
        groups.setdefault(ch, []).append(i)
    return imgs, groups


def quality_scores(images, detail: bool = False, device: int = 0):
    """qualityScore of every image: int32 [n], NO_SCORE where the reference has none.  With detail=True also the
    intermediate figures as DETAIL_DTYPE [n] (sums and means of the two difference maps, long-edge counts, edge count,
    working size)."""
    imgs, groups = _by_channels(images)
    scores = np.zeros(len(imgs), np.int32)
    det = np.zeros(len(imgs), DETAIL_DTYPE)
    for ch, idx in groups.items():
        buf, off, w, h, stride = pack_images([imgs[i] for i in idx])
        s = np.zeros(len(idx), np.int32)
        d = np.zeros(len(idx), DETAIL_DTYPE)
        check(_lib.lib().cbh_quality_scores(buf.ctypes.data, buf.size, len(idx), off.ctypes.data, w.ctypes.data,
                                            h.ctypes.data, stride.ctypes.data, ch, s.ctypes.data,
                                            d.ctypes.data if detail else None, device), "quality_scores")
        scores[idx], det[idx] = s, d
    return (scores, det) if detail else scores


def quality_planes(images, device: int = 0):
    """The diagnostic form: (scores int32 [n], detail DETAIL_DTYPE [n], planes) with planes[i] = uint8 [3, qh, qw] -- the
    edge map hE | vE (0 / 255), the horizontal and the vertical difference map, the three images qualityScore hands to
    addVisual (:430-432) before its normalisation; [3, 0, 0] for an image without a working plane."""
    import torch

    imgs, groups = _by_channels(images)
    scores = np.zeros(len(imgs), np.int32)
    det = np.zeros(len(imgs), DETAIL_DTYPE)
    planes: list = [None] * len(imgs)
    dev = torch.device("cuda", device)
    for ch, idx in groups.items():
        buf, off, w, h, stride = pack_images([imgs[i] for i in idx])
        dims = [quality_dims(int(a), int(b)) for a, b in zip(w, h)]
        sizes = np.array([3 * qw * qh for qw, qh in dims], np.uint64)
        poff = np.zeros(len(idx), np.uint64)
        poff[1:] = np.cumsum(sizes[:-1])
        d_img = torch.from_numpy(buf).to(dev)
        d_scores = torch.zeros(len(idx), dtype=torch.int32, device=dev)
        d_detail = torch.zeros(len(idx) * DETAIL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_planes = torch.zeros(max(int(sizes.sum()), 1), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        check(_lib.lib().cbh_quality_scores_dev(d_img.data_ptr(), len(idx), off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                                stride.ctypes.data, ch, d_scores.data_ptr(), d_detail.data_ptr(),
                                                d_planes.data_ptr(), poff.ctypes.data, device, None), "quality_planes")
        torch.cuda.synchronize(dev)
        scores[idx] = d_scores.cpu().numpy()
        det[idx] = d_detail.cpu().numpy().view(DETAIL_DTYPE)
        flat = d_planes.cpu().numpy()
        for k, i in enumerate(idx):
            qw, qh = dims[k]
            planes[i] = flat[int(poff[k]): int(poff[k]) + 3 * qw * qh].reshape(3, qh, qw).copy()
    return scores, det, planes
