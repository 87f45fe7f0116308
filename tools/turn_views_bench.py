"""Quarter turns and transposes on the device: the byte rate of k_turn_views beside k_gray_views, and what one upload
for the turned views is worth.

    python tools/turn_views_bench.py [--n 256] [--iters 200] [--reps 5] [--out profiles/turn_views.jsonl]

For each shape (640 x 480 x 3, 400 x 300 x 3, 1920 x 1080 x 1; n device-resident images) one JSON line:
  kernel    cbh_turn_views_dev with turn_mask 8 | 16 (T = 2) and, in the same process at the same shape, cbh_gray_views_dev
            with mirror_mask 3 -- the same bytes read (w*h*ch) and written (the turn kernel 2*w*h, the mirror kernel
            3*w*h: it also writes the identity plane), neither with colour views.  Device events around `iters` calls,
            the two alternating `reps` times after a warm-up; medians, bytes moved per second, and the ratio of the rates.
  pipeline  cbh_index_images_views_ex with view_mask 8 | 16 (algos = 1: grey -> autocrop -> dct hash) against the route it
            replaces: np.rot90 twice on the host, then cbh_index_images on the batch and on each turned batch (three
            uploads); host in / host out, wall time of each route (every C call ends in a device synchronisation), the
            two alternating `reps` times after a warm-up; medians, the ratio, and how much of the host route is the two
            np.rot90 passes.  The hashes and rectangles must agree.
Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from mirror_bench import images  # noqa: E402

SHAPES = [(640, 480, 3), (400, 300, 3), (1920, 1080, 1)]  # w, h, channels


def batch(n, h, w, ch):
    if ch == 3:
        return images(n, h, w)
    few = images(8, h, w).mean(axis=3).astype(np.uint8)  # grey: eight frames, rolled
    rng = np.random.default_rng(2)
    return np.stack([np.roll(few[i % 8], int(rng.integers(0, w)), axis=1) for i in range(n)])


def kernel(L, imgs, ch, iters, reps):
    import torch

    from cbird_amd import _lib

    n, h, w = imgs.shape[:3]
    src = torch.from_numpy(imgs).cuda()
    out = torch.empty(3 * n * h * w, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()
    head = (src.data_ptr(), n, w, h, w * ch, w * h * ch, ch)
    tail = (out.data_ptr(), None, 0, s.cuda_stream)
    calls = {"turn": lambda: _lib.check(L.cbh_turn_views_dev(*head, 24, *tail), "turn_views"),
             "mirror": lambda: _lib.check(L.cbh_gray_views_dev(*head, 3, *tail), "gray_views")}
    bytes_ = {"turn": n * w * h * (ch + 2), "mirror": n * w * h * (ch + 3)}
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(iters):
                f()
            e1.record(s)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / iters)
    r = {}
    for k in calls:
        m = statistics.median(ms[k])
        r[k + "_ms"] = round(m, 4)
        r[k + "_bytes"] = bytes_[k]
        r[k + "_tb_per_s"] = round(bytes_[k] / m / 1e9, 3)
        r[k + "_ms_all"] = [round(x, 4) for x in ms[k]]
    r["turn_over_mirror_rate"] = round(r["turn_tb_per_s"] / r["mirror_tb_per_s"], 3)
    return r


def pipeline(L, imgs, ch, reps):
    from cbird_amd import _lib
    from cbird_amd.scanner import _Params

    n, h, w = imgs.shape[:3]
    p = _Params(20, 1, 400, 400, 464)
    hv, rv = np.zeros(3 * n, np.uint64), np.zeros((3 * n, 4), np.int32)
    hh, rh = np.zeros((3, n), np.uint64), np.zeros((3, n, 4), np.int32)
    z = [None] * 8

    def device():
        _lib.check(L.cbh_index_images_views_ex(imgs.ctypes.data, n, w, h, w * ch, w * h * ch, ch, 24, C.byref(p),
                                               hv.ctypes.data, rv.ctypes.data, *z, 0), "views_ex")

    turn_s = []  # the share of the host route that is numpy turning the batch

    def host():
        t0 = time.perf_counter()
        turned = [imgs, np.ascontiguousarray(np.rot90(imgs, -1, axes=(1, 2))), np.ascontiguousarray(np.rot90(imgs, 1, axes=(1, 2)))]
        turn_s.append(time.perf_counter() - t0)
        for k, t in enumerate(turned):
            th, tw = t.shape[1:3]
            _lib.check(L.cbh_index_images(t.ctypes.data, n, tw, th, tw * ch, tw * th * ch, ch, C.byref(p), hh[k].ctypes.data,
                                          rh[k].ctypes.data, *z, 0), "index")

    for _ in range(2):
        device(), host()
    assert (hv.reshape(n, 3).T == hh).all() and (rv.reshape(n, 3, 4).transpose(1, 0, 2) == rh).all(), \
        "the device's turned views and the host-turned copies disagree"
    td, th_ = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); device(); td.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); host(); th_.append(time.perf_counter() - t0)
    md, mh = statistics.median(td), statistics.median(th_)
    return {"views_ex_ms": round(md * 1e3, 2), "host_route_ms": round(mh * 1e3, 2), "ratio": round(md / mh, 3),
            "host_route_rot90_ms": round(statistics.median(turn_s[-reps:]) * 1e3, 2),
            "views_ex_ms_all": [round(t * 1e3, 2) for t in td], "host_route_ms_all": [round(t * 1e3, 2) for t in th_]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "turn_views.jsonl"))
    a = ap.parse_args()
    import cbird_amd
    from cbird_amd import _lib

    cbird_amd.require_device()
    L = _lib.lib()
    for w, h, ch in SHAPES:
        imgs = batch(a.n, h, w, ch)
        r = {"n": a.n, "w": w, "h": h, "channels": ch, "turn_mask": 24, "mirror_mask": 3,
             "kernel": kernel(L, imgs, ch, a.iters, a.reps), "pipeline": pipeline(L, imgs, ch, a.reps)}
        line = json.dumps(r)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
