"""demosaicHough (src/cvutil.cpp:1445-1688) for batches of contact sheets or thumbnail grids: every tile of a sheet as a
rectangle, in the reference's order, and the crops that -select-grid (src/main.cpp:1310-1332) turns into needles.  What
is computed, what is an exact restatement of the reference and what is unpinned against OpenCV is stated in
include/cbird_hip.h.

The functions take numpy arrays (host entry point) or torch tensors on the device (device entry points); rectangles and
line positions are small and always come back as numpy arrays."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import cbh_demosaic_params, check
from .difference import _groups, _is_tensor, _pack_tensors
from .quality import pack_images


def default_params(**changes) -> cbh_demosaic_params:
    """DemosaicParams' defaults (src/cvutil.h:183-201), with the given fields changed"""
    p = cbh_demosaic_params()
    _lib.lib().cbh_demosaic_default_params(C.byref(p))
    for k, v in changes.items():
        if not hasattr(p, k):
            raise TypeError(f"cbh_demosaic_params has no field {k!r}")
        setattr(p, k, v)
    return p


def _params(params) -> cbh_demosaic_params:
    if params is None:
        return default_params()
    return default_params(**params) if isinstance(params, dict) else params


def grid_select(lines, side: int, cols: int, min_grid_spacing: int = 96, grid_tolerance: int = 4):
    """selectLines (:1552-1617) on the positions of one direction, 0 and `side` appended: the grid, int32.  Host code."""
    a = np.ascontiguousarray(lines, np.int32).reshape(-1)
    out = np.zeros(len(a) + 2, np.int32)
    n = C.c_size_t(0)
    check(_lib.lib().cbh_grid_select(a.ctypes.data, len(a), int(side), int(cols), int(min_grid_spacing), int(grid_tolerance),
                                     out.ctypes.data, C.byref(n)), "grid_select")
    return out[:n.value].copy()


def grid_rects(hgrid, vgrid, w: int, h: int, crop_margin: int = 2):
    """the rectangles of a grid (:1629-1664), int32 [k, 4] = (x, y, w, h), row by row.  Host code."""
    hg, vg = np.ascontiguousarray(hgrid, np.int32).reshape(-1), np.ascontiguousarray(vgrid, np.int32).reshape(-1)
    cap = max(1, (max(len(hg), 2) - 1) * (max(len(vg), 2) - 1))
    out = np.zeros((cap, 4), np.int32)
    n = C.c_size_t(0)
    check(_lib.lib().cbh_grid_rects(hg.ctypes.data, len(hg), vg.ctypes.data, len(vg), int(w), int(h), int(crop_margin),
                                    out.ctypes.data, cap, C.byref(n)), "grid_rects")
    return out[:n.value].copy()


def _device_groups(images, device):
    """(channel count, indices, buffer, off, w, h, stride) per channel count, on the device"""
    import torch

    dev = torch.device("cuda", device)
    on_device = len(images) > 0 and all(_is_tensor(im) for im in images)
    if not on_device:
        if any(_is_tensor(im) for im in images):
            raise ValueError("the images are either all numpy arrays or all device tensors")
        images = [torch.from_numpy(np.ascontiguousarray(im, np.uint8)).to(dev) for im in images]
    for ch, idx in _groups(images).items():
        packed = _pack_tensors([images[i] for i in idx], dev)
        torch.cuda.synchronize(dev)  # the library's call may run on another stream than the packing
        yield (ch, idx) + tuple(packed)


def edge_maps(images, params=None, classes: bool = False, device: int = 0):
    """Steps 1-4 of demosaicHough per image: the edge maps uint8 [h, w] (numpy), with classes=True also the class maps
    before the hysteresis (0 none, 1 candidate, 2 strong) and the number of hysteresis launches of the last call."""
    import torch

    p = _params(params)
    n = len(images)
    edges, cls, passes = [None] * n, [None] * n, C.c_uint32(0)
    L = _lib.lib()
    for ch, idx, buf, off, w, h, stride in _device_groups(images, device):
        total = int((w.astype(np.int64) * h).sum())
        d_e = torch.zeros(total, dtype=torch.uint8, device=buf.device)
        d_c = torch.zeros(total if classes else 1, dtype=torch.uint8, device=buf.device)
        torch.cuda.synchronize(buf.device)
        check(L.cbh_edge_maps_dev(buf.data_ptr(), len(idx), off.ctypes.data, w.ctypes.data, h.ctypes.data, stride.ctypes.data,
                                  ch, C.addressof(p), d_e.data_ptr(), d_c.data_ptr() if classes else None, C.addressof(passes),
                                  device, None), "edge_maps")
        he, hc, at = d_e.cpu().numpy(), d_c.cpu().numpy(), 0
        for k, i in enumerate(idx):
            size = int(w[k]) * int(h[k])
            edges[i] = he[at:at + size].reshape(int(h[k]), int(w[k])).copy()
            if classes:
                cls[i] = hc[at:at + size].reshape(int(h[k]), int(w[k])).copy()
            at += size
    return (edges, cls, passes.value) if classes else edges


def grid_lines(images, params=None, device: int = 0):
    """Steps 1-5 per image: [(horizontal positions, vertical positions)], int32, ascending, duplicates kept"""
    p = _params(params)
    out = [None] * len(images)
    L = _lib.lib()
    for ch, idx, buf, off, w, h, stride in _device_groups(images, device):
        m = len(idx)
        hor, ver = np.zeros(int(h.sum()), np.int32), np.zeros(int(w.sum()), np.int32)
        hf, vf = np.zeros(m + 1, np.uint32), np.zeros(m + 1, np.uint32)
        check(L.cbh_grid_lines_dev(buf.data_ptr(), m, off.ctypes.data, w.ctypes.data, h.ctypes.data, stride.ctypes.data, ch,
                                   C.addressof(p), hor.ctypes.data, hf.ctypes.data, ver.ctypes.data, vf.ctypes.data, device,
                                   None), "grid_lines")
        for k, i in enumerate(idx):
            out[i] = (hor[hf[k]:hf[k + 1]].copy(), ver[vf[k]:vf[k + 1]].copy())
    return out


def demosaic(images, params=None, device: int = 0):
    """demosaicHough of every image (sheets of mixed channel counts are answered in one call per count): a list of
    int32 [k, 4] arrays of (x, y, w, h), one per image, in the reference's order.  params: None, a cbh_demosaic_params or
    a dict of the fields to change."""
    p = _params(params)
    n = len(images)
    out = [None] * n
    if n == 0:
        return out
    L = _lib.lib()
    on_device = all(_is_tensor(im) for im in images)
    if not on_device and any(_is_tensor(im) for im in images):
        raise ValueError("the images are either all numpy arrays or all device tensors")
    if on_device:
        groups = _device_groups(images, device)
    else:
        imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
        groups = ((ch, idx) + tuple(pack_images([imgs[i] for i in idx])) for ch, idx in _groups(imgs).items())
    for ch, idx, buf, off, w, h, stride in groups:
        m = len(idx)
        first = np.zeros(m + 1, np.uint32)
        cap = 64 * m
        while True:
            rects = np.zeros((cap, 4), np.int32)
            if on_device:
                rc = L.cbh_demosaic_dev(buf.data_ptr(), m, off.ctypes.data, w.ctypes.data, h.ctypes.data, stride.ctypes.data,
                                        ch, C.addressof(p), rects.ctypes.data, cap, first.ctypes.data, device, None)
            else:
                rc = L.cbh_demosaic(buf.ctypes.data, buf.size, m, off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                    stride.ctypes.data, ch, C.addressof(p), rects.ctypes.data, cap, first.ctypes.data, device)
            if rc != _lib.CBH_E_OVERFLOW:
                break
            cap = int(first[m])  # the needed count
        check(rc, "demosaic")
        for k, i in enumerate(idx):
            out[i] = rects[first[k]:first[k + 1]].copy()
    return out


def grid_tiles(image, rects):
    """the needles of -select-grid: qImg.copy(r) for every rectangle -- the part of r inside the image keeps its pixels,
    the rest is 0, as QImage::copy fills it.  The hash and search entry points take the crops as they are."""
    tiles = []
    ih, iw = image.shape[:2]
    for x, y, w, h in np.asarray(rects).reshape(-1, 4).tolist():
        if w < 1 or h < 1:
            raise ValueError("a rectangle with a side below 1 has no pixels")
        if _is_tensor(image):
            tile = image.new_zeros((h, w) + tuple(image.shape[2:]))
        else:
            tile = np.zeros((h, w) + image.shape[2:], image.dtype)
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, iw), min(y + h, ih)
        if x0 < x1 and y0 < y1:
            tile[y0 - y:y1 - y, x0 - x:x1 - x] = image[y0:y1, x0:x1]
        tiles.append(tile)
    return tiles
