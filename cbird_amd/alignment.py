"""alignSpatially (src/gui/videocomparewidget.cpp:590-627) for one left image against n right images, and alignTemporally
with sad128 (:629-680) for a window of right frames slid over a left clip: searches for the smallest sum of absolute byte
differences of images brought to 256 x 256 (17 x 17 shifts of +-8 pixels) or 128 x 128 (every placement of the window).
What is computed, what is an exact restatement of the reference and what is unpinned against Qt is stated in
include/cbird_hip.h.

Both functions take numpy arrays (host entry points) or torch tensors on the device (device entry points: only the
records and the tables asked for come back to the host)."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check
from .difference import _channels, _groups, _is_tensor, _pack_tensors
from .quality import pack_images

ALIGN_SPATIAL_DTYPE = np.dtype([("min_x", np.int32), ("min_y", np.int32), ("min_sad", np.uint32),
                                ("sad_at_zero", np.uint32)])  # struct cbh_align_spatial_result
ALIGN_TEMPORAL_DTYPE = np.dtype([("placement", np.int32), ("offset", np.int32), ("min_mean", np.uint32),
                                 ("start_mean", np.uint32)])  # struct cbh_align_temporal_result
assert ALIGN_SPATIAL_DTYPE.itemsize == 16 and ALIGN_TEMPORAL_DTYPE.itemsize == 16
SHIFTS = 17  # -8 .. 8


def align_spatial(left, rights, table: bool = False, device: int = 0):
    """alignSpatially(left, right) for one left image and every right image (any sizes, channel counts of 1, 3 or 4).
    Returns ALIGN_SPATIAL_DTYPE [n]: left pixel (x + min_x, y + min_y) lies on right pixel (x, y) at 256 x 256 (the
    reference's _alignX, _alignY are min_x / 256, min_y / 256); with table=True also the sads uint32 [n, 17, 17] indexed
    [xo + 8, yo + 8].  Rights of mixed channel counts are answered in one call per count."""
    n = len(rights)
    on_device = _is_tensor(left)
    if n and any(_is_tensor(r) != on_device for r in rights):
        raise ValueError("left and rights are either all numpy arrays or all device tensors")
    lch = _channels(left.shape)
    res = np.zeros(n, ALIGN_SPATIAL_DTYPE)
    tab = np.zeros((n, SHIFTS, SHIFTS), np.uint32)
    if n == 0:
        return (res, tab) if table else res
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
        m = len(idx)
        if on_device:
            buf, off, w, h, stride = _pack_tensors(sel, dev)
            d_res = torch.zeros(m * 16, dtype=torch.uint8, device=dev)
            d_tab = torch.zeros(m * SHIFTS * SHIFTS if table else 1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            check(L.cbh_align_spatial_dev(left.data_ptr(), lw, lh, lw * lch, lch, buf.data_ptr(), m, off.ctypes.data,
                                          w.ctypes.data, h.ctypes.data, stride.ctypes.data, ch, d_res.data_ptr(),
                                          d_tab.data_ptr() if table else None, device, None), "align_spatial")
            res[idx] = d_res.cpu().numpy().view(ALIGN_SPATIAL_DTYPE)
            if table:
                tab[idx] = d_tab.cpu().numpy().view(np.uint32).reshape(m, SHIFTS, SHIFTS)
        else:
            buf, off, w, h, stride = pack_images(sel)
            r = np.zeros(m, ALIGN_SPATIAL_DTYPE)
            t = np.zeros((m, SHIFTS, SHIFTS), np.uint32)
            check(L.cbh_align_spatial(left.ctypes.data, lw, lh, lw * lch, lch, buf.ctypes.data, buf.size, m, off.ctypes.data,
                                      w.ctypes.data, h.ctypes.data, stride.ctypes.data, ch, r.ctypes.data,
                                      t.ctypes.data if table else None, device), "align_spatial")
            res[idx], tab[idx] = r, t
    return (res, tab) if table else res


def default_start(placements: int) -> int:
    """the placement the search starts from when none is given: (P - 1) // 2 + (P - 1) % 2 clamped into [0, P) -- for the
    reference's 60 placements 30, its offsets -30 .. +29 around the current frame"""
    p = int(placements)
    return min(max((p - 1) // 2 + (p - 1) % 2, 0), p - 1)


def _one_count(frames, what):
    counts = {_channels(f.shape) for f in frames}
    if len(counts) != 1:
        raise ValueError(f"{what}: expected at least one frame, all of one channel count")
    return counts.pop()


def align_temporal(left_frames, right_frames, start=None, cells: bool = False, device: int = 0):
    """alignTemporally: the W right frames against the left frames at every placement d = 0 .. P - 1, P = nL - W + 1
    (right frame i on left frame d + i).  start: the placement the search starts from and keeps unless another has a
    strictly smaller mean; None = default_start(P).  Frames of a side share a channel count; sizes are free.
    Returns (record ALIGN_TEMPORAL_DTYPE scalar, means uint32 [P]) and with cells=True also the sads uint32 [P, W]."""
    nl, nw = len(left_frames), len(right_frames)
    if nw < 1 or nl < nw:
        raise ValueError("expected 1 <= len(right_frames) <= len(left_frames)")
    p = nl - nw + 1
    start = default_start(p) if start is None else int(start)
    on_device = _is_tensor(left_frames[0])
    if any(_is_tensor(f) != on_device for f in list(left_frames) + list(right_frames)):
        raise ValueError("the frames are either all numpy arrays or all device tensors")
    rec = np.zeros(1, ALIGN_TEMPORAL_DTYPE)
    means = np.zeros(p, np.uint32)
    cel = np.zeros((p, nw), np.uint32)
    L = _lib.lib()
    if on_device:
        import torch

        dev = torch.device("cuda", device)
        lch, rch = _one_count(left_frames, "left_frames"), _one_count(right_frames, "right_frames")
        lb, lo, lw, lh, ls = _pack_tensors(list(left_frames), dev)
        rb, ro, rw, rh, rs = _pack_tensors(list(right_frames), dev)
        d_rec = torch.zeros(16, dtype=torch.uint8, device=dev)
        d_means = torch.zeros(p, dtype=torch.int32, device=dev)
        d_cells = torch.zeros(p * nw if cells else 1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        check(L.cbh_align_temporal_dev(lb.data_ptr(), nl, lo.ctypes.data, lw.ctypes.data, lh.ctypes.data, ls.ctypes.data, lch,
                                       rb.data_ptr(), nw, ro.ctypes.data, rw.ctypes.data, rh.ctypes.data, rs.ctypes.data, rch,
                                       start, d_rec.data_ptr(), d_means.data_ptr(), d_cells.data_ptr() if cells else None,
                                       device, None), "align_temporal")
        rec = d_rec.cpu().numpy().view(ALIGN_TEMPORAL_DTYPE)
        means = d_means.cpu().numpy().view(np.uint32)
        if cells:
            cel = d_cells.cpu().numpy().view(np.uint32).reshape(p, nw)
    else:
        lf = [np.ascontiguousarray(f, np.uint8) for f in left_frames]
        rf = [np.ascontiguousarray(f, np.uint8) for f in right_frames]
        lch, rch = _one_count(lf, "left_frames"), _one_count(rf, "right_frames")
        lb, lo, lw, lh, ls = pack_images(lf)
        rb, ro, rw, rh, rs = pack_images(rf)
        check(L.cbh_align_temporal(lb.ctypes.data, lb.size, nl, lo.ctypes.data, lw.ctypes.data, lh.ctypes.data, ls.ctypes.data,
                                   lch, rb.ctypes.data, rb.size, nw, ro.ctypes.data, rw.ctypes.data, rh.ctypes.data,
                                   rs.ctypes.data, rch, start, rec.ctypes.data, means.ctypes.data,
                                   cel.ctypes.data if cells else None, device), "align_temporal")
    return (rec[0], means, cel) if cells else (rec[0], means)


def alignment_transform(min_x, min_y, left_shape, right_shape):
    """The 2 x 3 matrix template -> right image that difference_images accepts, for a shift align_spatial found.  The
    SAD compares left (x + xo, y + yo) with right (x, y) in the 256 x 256 space, so left pixel (lx, ly) lies on
    rx = lx * rw / lw - xo * rw / 256, ry = ly * rh / lh - yo * rh / 256 (float64).  This is the library's definition;
    the widget's own draw offset is not restated."""
    lh, lw = (float(v) for v in left_shape[:2])
    rh, rw = (float(v) for v in right_shape[:2])
    return np.array([[rw / lw, 0.0, -float(min_x) * rw / 256.0], [0.0, rh / lh, -float(min_y) * rh / 256.0]], np.float64)
