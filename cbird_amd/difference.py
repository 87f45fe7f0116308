"""brightnessAndContrastAuto (src/cvutil.cpp:578-665) for batches of images, and differenceImage
(src/gui/mediagrouplistwidget.cpp:98-208) for one left image against n right images: the false-colour picture of where
two matched images differ, aligned with the transform the template matcher found.  What is computed, what is an exact
restatement of the reference and what is unpinned against OpenCV / Qt is stated in include/cbird_hip.h.

Both functions take numpy arrays (host entry points) or torch tensors on the device (device entry points: nothing comes
back to the host but the small records) and answer in kind."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check
from .quality import pack_images

DIFF_DETAIL_DTYPE = np.dtype([("sum_total", np.uint64), ("sum_max", np.uint32), ("n_ge32", np.uint32),
                              ("n_ge1024", np.uint32), ("w", np.int32), ("h", np.int32), ("warped", np.int32),
                              ("left_min", np.int32), ("left_max", np.int32), ("right_min", np.int32),
                              ("right_max", np.int32)])  # struct cbh_diff_detail
assert DIFF_DETAIL_DTYPE.itemsize == 48


def gray_cuts(hist, clip_pct: float):
    """grayLevel's cut rule (:595-625) on given counts: hist uint32 [n, 256] -> (min_gray, max_gray) int32 [n] each.
    Runs on the host, in the function the device runs."""
    h = np.ascontiguousarray(hist, np.uint32).reshape(-1, 256)
    lo, hi = np.zeros(len(h), np.int32), np.zeros(len(h), np.int32)
    check(_lib.lib().cbh_gray_cuts(h.ctypes.data, len(h), float(clip_pct), lo.ctypes.data, hi.ctypes.data), "gray_cuts")
    return lo, hi


def _is_tensor(x) -> bool:
    return type(x).__module__.startswith("torch")


def _channels(shape) -> int:
    ch = 1 if len(shape) == 2 else shape[2] if len(shape) == 3 else 0
    if ch not in (1, 3, 4) or 0 in tuple(shape):
        raise ValueError("expected non-empty uint8 images [h, w], [h, w, 1], [h, w, 3] (BGR) or [h, w, 4] (BGRA)")
    return ch


def _groups(images):
    groups: dict[int, list[int]] = {}
    for i, im in enumerate(images):
        groups.setdefault(_channels(im.shape), []).append(i)
    return groups


def _pack_tensors(images, dev):
    """device images of one channel count in one device buffer, rows packed, 16-byte aligned starts"""
    import torch

    sizes = np.array([im.numel() for im in images], np.uint64)
    a = np.uint64(16)
    off = np.zeros(len(images), np.uint64)
    off[1:] = np.cumsum((sizes[:-1] + a - np.uint64(1)) // a * a)
    buf = torch.zeros(int(off[-1] + sizes[-1]), dtype=torch.uint8, device=dev)
    for im, o in zip(images, off):
        buf[int(o): int(o) + im.numel()] = im.contiguous().reshape(-1)
    w = np.array([im.shape[1] for im in images], np.uint32)
    h = np.array([im.shape[0] for im in images], np.uint32)
    ch = _channels(images[0].shape)
    return buf, off, w, h, (w * np.uint32(ch)).astype(np.uint32)


def auto_contrast(images, clip_pct: float = 0, histograms: bool = False, device: int = 0):
    """brightnessAndContrastAuto(src, dst, clip_pct) of every image.  Returns (stretched, cuts) -- stretched[i] shaped as
    images[i], cuts int32 [n, 2] = {min_gray, max_gray} -- and with histograms=True also the grey histograms uint32
    [n, 256].  An image whose min_gray >= max_gray comes back unchanged.  Device tensors in, device tensors out."""
    on_device = len(images) > 0 and all(_is_tensor(im) for im in images)
    n = len(images)
    outs: list = [None] * n
    cuts = np.zeros((n, 2), np.int32)
    hist = np.zeros((n, 256), np.uint32)
    L = _lib.lib()
    if on_device:
        import torch

        dev = torch.device("cuda", device)
        for ch, idx in _groups(images).items():
            buf, off, w, h, stride = _pack_tensors([images[i] for i in idx], dev)
            d_out = torch.zeros_like(buf)
            d_cuts = torch.zeros(2 * len(idx), dtype=torch.int32, device=dev)
            d_hist = torch.zeros(256 * len(idx), dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            check(L.cbh_auto_contrast_dev(buf.data_ptr(), len(idx), off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                          stride.ctypes.data, ch, float(clip_pct), d_out.data_ptr(), d_cuts.data_ptr(),
                                          d_hist.data_ptr() if histograms else None, device, None), "auto_contrast")
            cuts[idx] = d_cuts.cpu().numpy().reshape(-1, 2)
            if histograms:
                hist[idx] = d_hist.cpu().numpy().view(np.uint32).reshape(-1, 256)
            for k, i in enumerate(idx):
                outs[i] = d_out[int(off[k]): int(off[k]) + images[i].numel()].reshape(images[i].shape)
    else:
        imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
        for ch, idx in _groups(imgs).items():
            buf, off, w, h, stride = pack_images([imgs[i] for i in idx])
            out = np.zeros_like(buf)
            c = np.zeros((len(idx), 2), np.int32)
            hh = np.zeros((len(idx), 256), np.uint32)
            check(L.cbh_auto_contrast(buf.ctypes.data, buf.size, len(idx), off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                      stride.ctypes.data, ch, float(clip_pct), out.ctypes.data, c.ctypes.data,
                                      hh.ctypes.data if histograms else None, device), "auto_contrast")
            cuts[idx], hist[idx] = c, hh
            for k, i in enumerate(idx):
                outs[i] = out[int(off[k]): int(off[k]) + imgs[i].size].reshape(imgs[i].shape).copy()
    return (outs, cuts, hist) if histograms else (outs, cuts)


def _transforms(transforms, n):
    """(tx float64 [n, 6], has_tx uint8 [n]) or (None, None) from: None; the records of template_match_images /
    template_match (fields r.tx / r.tx_found or tx / tx_found); matrices [n, 2, 3] or [n, 6]; a (matrices, flags) pair"""
    if transforms is None:
        return None, None
    flags = None
    if isinstance(transforms, tuple):
        transforms, flags = transforms
    t = np.asarray(transforms)
    if t.dtype.names:
        if "r" in t.dtype.names:
            t = t["r"]
        tx, flags = t["tx"], t["tx_found"]
    else:
        tx = t
    tx = np.ascontiguousarray(tx, np.float64).reshape(-1, 6)
    has = np.ones(n, np.uint8) if flags is None else (np.asarray(flags).reshape(-1) != 0).astype(np.uint8)
    if len(tx) != n or len(has) != n:
        raise ValueError("one transform per right image")
    return tx, has


def difference_dims(left_shape, right_shapes, transforms=None):
    """(w uint32 [n], h uint32 [n], warped bool [n]): each pair's picture size"""
    n = len(right_shapes)
    tx, has = _transforms(transforms, n)
    w = np.array([s[1] for s in right_shapes], np.uint32)
    h = np.array([s[0] for s in right_shapes], np.uint32)
    ow, oh, wp = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    check(_lib.lib().cbh_difference_dims(int(left_shape[1]), int(left_shape[0]), n, w.ctypes.data, h.ctypes.data,
                                         tx.ctypes.data if tx is not None else None,
                                         has.ctypes.data if has is not None else None, ow.ctypes.data, oh.ctypes.data,
                                         wp.ctypes.data), "difference_dims")
    return ow, oh, wp.astype(bool)


def difference_images(left, rights, transforms=None, clip_pct: float = 5, pictures: bool = True, device: int = 0):
    """differenceImage(left, right) for one left image and every right image (any sizes and channel counts of 1, 3 =
    BGR, 4 = BGRA).  transforms: None, or per right image the template -> right matrix: the result records of
    template_match_images / TemplateMatcher (their tx / tx_found), matrices [n, 2, 3], or (matrices, flags).
    Returns (pics, detail): pics[i] uint8 [h, w, 4] BGRA (None with pictures=False), detail DIFF_DETAIL_DTYPE [n].
    Device tensors in, device pictures out; the records are host memory either way."""
    n = len(rights)
    on_device = _is_tensor(left)
    if n and any(_is_tensor(r) != on_device for r in rights):
        raise ValueError("left and rights are either all numpy arrays or all device tensors")
    lch = _channels(left.shape)
    tx, has = _transforms(transforms, n)
    pics: list = [None] * n
    detail = np.zeros(n, DIFF_DETAIL_DTYPE)
    if n == 0:
        return pics, detail
    L = _lib.lib()
    if on_device:
        import torch

        dev = torch.device("cuda", device)
        left = left.contiguous()
    else:
        left = np.ascontiguousarray(left, np.uint8)
        rights = [np.ascontiguousarray(r, np.uint8) for r in rights]
    lh, lw = left.shape[:2]
    for ch, idx in _groups(rights).items():
        sel = [rights[i] for i in idx]
        sub = None if tx is None else (tx[idx], has[idx])
        ow, oh, _ = difference_dims(left.shape, [r.shape for r in sel], sub)
        sizes = ow.astype(np.uint64) * oh.astype(np.uint64) * np.uint64(4)
        ooff = np.zeros(len(idx), np.uint64)
        ooff[1:] = np.cumsum((sizes[:-1] + np.uint64(15)) // np.uint64(16) * np.uint64(16))
        total = int(ooff[-1] + sizes[-1])
        txp = sub[0].ctypes.data if sub else None
        hasp = sub[1].ctypes.data if sub else None
        det = np.zeros(len(idx), DIFF_DETAIL_DTYPE)
        if on_device:
            buf, off, w, h, stride = _pack_tensors(sel, dev)
            d_pics = torch.zeros(total if pictures else 16, dtype=torch.uint8, device=dev)
            d_det = torch.zeros(len(idx) * DIFF_DETAIL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            check(L.cbh_difference_images_dev(left.data_ptr(), lw, lh, lw * lch, lch, buf.data_ptr(), len(idx),
                                              off.ctypes.data, w.ctypes.data, h.ctypes.data, stride.ctypes.data, ch, txp,
                                              hasp, float(clip_pct), d_pics.data_ptr() if pictures else None,
                                              ooff.ctypes.data, d_det.data_ptr(), device, None), "difference_images")
            det = d_det.cpu().numpy().view(DIFF_DETAIL_DTYPE)
            flat = d_pics
        else:
            buf, off, w, h, stride = pack_images(sel)
            flat = np.zeros(total if pictures else 16, np.uint8)
            check(L.cbh_difference_images(left.ctypes.data, lw, lh, lw * lch, lch, buf.ctypes.data, buf.size, len(idx),
                                          off.ctypes.data, w.ctypes.data, h.ctypes.data, stride.ctypes.data, ch, txp, hasp,
                                          float(clip_pct), flat.ctypes.data if pictures else None, flat.size,
                                          ooff.ctypes.data, det.ctypes.data, device), "difference_images")
        detail[idx] = det
        if pictures:
            for k, i in enumerate(idx):
                pics[i] = flat[int(ooff[k]): int(ooff[k]) + int(sizes[k])].reshape(int(oh[k]), int(ow[k]), 4)
    return pics, detail
