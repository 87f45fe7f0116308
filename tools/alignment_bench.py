"""alignSpatially / alignTemporally throughput (cbird_amd/csrc/align.hip): one 640 x 480 BGR left image against --pairs
640 x 480 BGR right images resident on the device, and one reference-shaped temporal call (64 left and 5 right frames of
640 x 360, start 30), each timed by device events on a side stream after warm-up calls; then both through the host
entries (wall time: uploads, the call, the records back).  The time is that of the whole call -- the host builds and
uploads the image table, the scale, SAD and pick kernels run, the stream is synchronised -- not of a kernel.
Byte differences per second: 289 shifts x 240 x 240 x 3 bytes per pair, 128 x 128 x 3 x P x W per clip.  The first pair
and the clip are checked against the numpy model (tests/alignment_rules.py).  Prints and gates nothing else.

    python tools/alignment_bench.py [--pairs 256] [--iters 7] [--out profiles/alignment.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PAIR_DIFFS = 289 * 240 * 240 * 3
CELL_DIFFS = 128 * 128 * 3


def timed(run, stream, iters):
    import torch

    ms, wall = [], []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        run()
        e1.record(stream)
        e1.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(e0.elapsed_time(e1))
    return ms, wall


def stats(ms, wall):
    return {"event_ms_median": float(np.median(ms)), "event_ms_min": float(min(ms)), "event_ms_max": float(max(ms)),
            "wall_ms_median": float(np.median(wall))}


def spatial(n, iters):
    import torch

    import alignment_rules as A
    import difference_rules as R
    from cbird_amd import _lib
    from cbird_amd.alignment import ALIGN_SPATIAL_DTYPE, align_spatial

    W, H = 640, 480
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    left = R.textured(W, H, 1)
    pool = [R.textured(W, H, 2 + k) for k in range(8)]
    size = W * H * 3
    d_left = torch.from_numpy(left.reshape(-1)).to(dev)
    d_pool = [torch.from_numpy(p.reshape(-1)).to(dev) for p in pool]
    d_rights = torch.empty(n * size, dtype=torch.uint8, device=dev)
    for i in range(n):
        d_rights[i * size: (i + 1) * size] = d_pool[i % 8]
    off = np.arange(n, dtype=np.uint64) * np.uint64(size)
    ww, hh, ss = np.full(n, W, np.uint32), np.full(n, H, np.uint32), np.full(n, W * 3, np.uint32)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_tab = torch.zeros(n * 289, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()

    def run():
        _lib.check(L.cbh_align_spatial_dev(d_left.data_ptr(), W, H, W * 3, 3, d_rights.data_ptr(), n, off.ctypes.data,
                                           ww.ctypes.data, hh.ctypes.data, ss.ctypes.data, 3, d_res.data_ptr(),
                                           d_tab.data_ptr(), 0, C.c_void_p(stream.cuda_stream)), "align_spatial")

    torch.cuda.synchronize()
    run()  # warm-up: code objects, the scratch arena's blocks
    run()
    ms, wall = timed(run, stream, iters)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(ALIGN_SPATIAL_DTYPE)
    tab0 = d_tab[:289].cpu().numpy().view(np.uint32).reshape(17, 17)
    wtab, wrec = A.align_spatial(left, pool[0])
    ok = bool((tab0 == wtab).all() and all(int(res[0][k]) == v for k, v in wrec.items()))
    med = float(np.median(ms))
    out = {"workload": f"{n} right images 640x480 BGR against a 640x480 BGR left image, device resident", "pairs": n,
           "iters": iters, **stats(ms, wall), "us_per_pair": med * 1e3 / n, "byte_differences": PAIR_DIFFS * n,
           "byte_differences_per_s": PAIR_DIFFS * n / (med * 1e-3), "first_pair_equals_numpy": ok}
    rights = [pool[i % 8] for i in range(n)]
    align_spatial(left, rights)
    hw = []
    for _ in range(iters):
        t0 = time.perf_counter()
        align_spatial(left, rights)
        hw.append((time.perf_counter() - t0) * 1e3)
    hmed = float(np.median(hw))
    host = {"workload": f"{n} right images 640x480 BGR against a 640x480 BGR left image, host entry (align_spatial)",
            "pairs": n, "iters": iters, "wall_ms_median": hmed, "wall_ms_min": float(min(hw)), "us_per_pair": hmed * 1e3 / n,
            "byte_differences_per_s": PAIR_DIFFS * n / (hmed * 1e-3)}
    return [out, host]


def temporal(iters):
    import torch

    import alignment_rules as A
    import difference_rules as R
    from cbird_amd import _lib
    from cbird_amd.alignment import ALIGN_TEMPORAL_DTYPE, align_temporal

    W, H, NL, NW, START = 640, 360, 64, 5, 30
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    pool = [R.textured(W, H, 50 + k) for k in range(16)]
    lf = [pool[(k * 7) % 16] if k not in range(41, 46) else pool[k - 41] for k in range(NL)]
    rf = [pool[k] for k in range(NW)]  # the window lies at placement 41
    size = W * H * 3
    d_l = torch.cat([torch.from_numpy(f.reshape(-1)) for f in lf]).to(dev)
    d_r = torch.cat([torch.from_numpy(f.reshape(-1)) for f in rf]).to(dev)

    def tables(n):
        return (np.arange(n, dtype=np.uint64) * np.uint64(size), np.full(n, W, np.uint32), np.full(n, H, np.uint32),
                np.full(n, W * 3, np.uint32))

    lo, lw, lh, ls = tables(NL)
    ro, rw, rh, rs = tables(NW)
    p = NL - NW + 1
    d_rec = torch.zeros(16, dtype=torch.uint8, device=dev)
    d_means = torch.zeros(p, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()

    def run():
        _lib.check(L.cbh_align_temporal_dev(d_l.data_ptr(), NL, lo.ctypes.data, lw.ctypes.data, lh.ctypes.data, ls.ctypes.data,
                                            3, d_r.data_ptr(), NW, ro.ctypes.data, rw.ctypes.data, rh.ctypes.data,
                                            rs.ctypes.data, 3, START, d_rec.data_ptr(), d_means.data_ptr(), None, 0,
                                            C.c_void_p(stream.cuda_stream)), "align_temporal")

    torch.cuda.synchronize()
    run()
    run()
    ms, wall = timed(run, stream, iters)
    torch.cuda.synchronize()
    rec = d_rec.cpu().numpy().view(ALIGN_TEMPORAL_DTYPE)[0]
    _, wmeans, wrec = A.align_temporal(lf, rf, START)
    ok = bool((d_means.cpu().numpy().view(np.uint32) == wmeans).all() and all(int(rec[k]) == v for k, v in wrec.items()))
    med = float(np.median(ms))
    out = {"workload": "64 left and 5 right frames 640x360 BGR, start 30, device resident", "placements": p, "window": NW,
           "iters": iters, **stats(ms, wall), "byte_differences": CELL_DIFFS * p * NW,
           "byte_differences_per_s": CELL_DIFFS * p * NW / (med * 1e-3), "placement": int(rec["placement"]),
           "equals_numpy": ok}
    align_temporal(lf, rf, START)
    hw = []
    for _ in range(iters):
        t0 = time.perf_counter()
        align_temporal(lf, rf, START)
        hw.append((time.perf_counter() - t0) * 1e3)
    hmed = float(np.median(hw))
    host = {"workload": "64 left and 5 right frames 640x360 BGR, start 30, host entry (align_temporal)", "placements": p,
            "window": NW, "iters": iters, "wall_ms_median": hmed, "wall_ms_min": float(min(hw)),
            "byte_differences_per_s": CELL_DIFFS * p * NW / (hmed * 1e-3)}
    return [out, host]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alignment.jsonl"))
    args = ap.parse_args()
    from cbird_amd import require_device

    require_device()  # no device: no number
    results = spatial(args.pairs, args.iters) + temporal(args.iters)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in results:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
