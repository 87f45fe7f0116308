"""Reflection search on the device: what one upload for every view is worth.

    python tools/mirror_bench.py e2e [--n 1024] [--w 640] [--h 480] [--reps 7] [--out FILE]
        cbh_index_images_views (algos = 1: grey -> autocrop -> dct hash, mask 7) against four cbh_index_images calls on
        copies flipped on the host beforehand; host in / host out, wall time of each call (the C call ends in a device
        synchronisation).  Warm-up first, then the two alternate; medians and the ratio.  The hashes must agree.
    python tools/mirror_bench.py kernel [--n 256] [--w 1920] [--h 1080] [--iters 20] [--out FILE]
        cbh_gray_views_dev alone on device-resident BGR images (mask 7, no colour views), for
        `rocprofv3 --kernel-trace --stats -- python tools/mirror_bench.py kernel`: the bytes the kernel has to move
        (read w*h*3, write 4*w*h per image) and the event-timed rate.
One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def images(n, h, w, seed=1):
    """smooth photo-like BGR frames with noise (hashes differ between the views)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([np.sin(xx / 37 + c) * 60 + np.cos(yy / 53 + 2 * c) * 50 + xx * 0.05 for c in range(3)], 2) + 120
    noisy = [np.clip(base + rng.normal(0, 8, (h, w, 3)), 0, 255).astype(np.uint8) for _ in range(min(n, 8))]
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        out[i] = np.roll(noisy[i % len(noisy)], int(rng.integers(0, w)), axis=1)
    return out


def e2e(a):
    from cbird_amd import _lib
    from cbird_amd.scanner import _Params

    L = _lib.lib()
    n, h, w = a.n, a.h, a.w
    imgs = images(n, h, w)
    flips = [imgs, np.ascontiguousarray(imgs[:, :, ::-1]), np.ascontiguousarray(imgs[:, ::-1]),
             np.ascontiguousarray(imgs[:, ::-1, ::-1])]
    p = _Params(20, 1, 400, 400, 464)
    hv, h4 = np.zeros(4 * n, np.uint64), np.zeros((4, n), np.uint64)
    rs, ist = w * 3, w * h * 3
    z = [None] * 9

    def views():
        _lib.check(L.cbh_index_images_views(imgs.ctypes.data, n, w, h, rs, ist, 3, 7, C.byref(p), hv.ctypes.data, *z, 0),
                   "views")

    def four():
        for k in range(4):
            _lib.check(L.cbh_index_images(flips[k].ctypes.data, n, w, h, rs, ist, 3, C.byref(p), h4[k].ctypes.data, *z, 0),
                       "index")

    for _ in range(2):
        views(), four()
    assert (hv.reshape(n, 4).T == h4).all(), "views and flipped copies disagree"
    tv, tf = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter(); views(); tv.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); four(); tf.append(time.perf_counter() - t0)
    mv, mf = statistics.median(tv), statistics.median(tf)
    return {"mode": "e2e", "n": n, "w": w, "h": h, "algos": 1, "mask": 7, "views_ms": round(mv * 1e3, 2),
            "four_calls_ms": round(mf * 1e3, 2), "ratio": round(mv / mf, 3),
            "views_ms_all": [round(t * 1e3, 2) for t in tv], "four_calls_ms_all": [round(t * 1e3, 2) for t in tf]}


def kernel(a):
    import torch

    from cbird_amd import _lib

    L = _lib.lib()
    n, h, w = a.n, a.h, a.w
    src = torch.from_numpy(images(min(n, 16), h, w)).cuda()
    src = src.repeat((n + src.shape[0] - 1) // src.shape[0], 1, 1, 1)[:n].contiguous()
    gray = torch.empty((4 * n, h, w), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()
    args = (src.data_ptr(), n, w, h, w * 3, w * h * 3, 3, 7, gray.data_ptr(), None, 0, s.cuda_stream)
    for _ in range(3):
        _lib.check(L.cbh_gray_views_dev(*args), "gray_views")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(a.iters):
        _lib.check(L.cbh_gray_views_dev(*args), "gray_views")
    e1.record(s)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    bytes_ = n * w * h * (3 + 4)
    return {"mode": "kernel", "n": n, "w": w, "h": h, "mask": 7, "ms_per_call": round(ms, 3), "bytes": bytes_,
            "tb_per_s": round(bytes_ / ms / 1e9, 3), "of_8tbs": round(bytes_ / ms / 1e9 / 8.0, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["e2e", "kernel"])
    ap.add_argument("--n", type=int)
    ap.add_argument("--w", type=int)
    ap.add_argument("--h", type=int)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    dflt = {"e2e": (1024, 640, 480), "kernel": (256, 1920, 1080)}[a.mode]
    a.n, a.w, a.h = a.n or dflt[0], a.w or dflt[1], a.h or dflt[2]
    r = e2e(a) if a.mode == "e2e" else kernel(a)
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
