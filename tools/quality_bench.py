"""qualityScore throughput (cbird_amd/csrc/quality.hip): images resident on the device, cbh_quality_scores_dev timed by
device events on a side stream after a warm-up call.  Two workloads: --images BGR images of 640 x 480, and a ragged batch
of group-like sizes.  The time is that of the whole call -- the host builds and uploads the strip table, three kernels
run, the stream is synchronised -- not of a kernel.  Bytes are what the algorithm needs by shape: the cropped source
pixels once, the working plane written once and read once; their rate is set against the 8 TB/s of HBM.  Beside it the
rate of the vectorised numpy restatement (tests/test_quality_rules.py) on one host core, for scale.

    python tools/quality_bench.py [--images 4096] [--ragged 1024] [--iters 5] [--out profiles/quality_scores.jsonl]
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
HBM_BYTES_PER_S = 8e12


def blocky(rng, w, h, cell=4):
    cells = rng.integers(0, 256, ((h + cell - 1) // cell, (w + cell - 1) // cell, 3)).astype(np.int32)
    img = np.kron(cells, np.ones((cell, cell, 1), np.int32))[:h, :w]
    return (img + rng.integers(-3, 4, img.shape)).clip(0, 255).astype(np.uint8)


def measure(name, imgs_of, n, iters):
    """imgs_of(i) -> the i-th image of the batch (a few distinct arrays, repeated)"""
    import torch

    import test_quality_rules as R
    from cbird_amd import _lib
    from cbird_amd.quality import DETAIL_DTYPE

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    imgs = [imgs_of(i) for i in range(n)]
    sizes = np.array([im.size for im in imgs], np.uint64)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum((sizes[:-1] + np.uint64(15)) // np.uint64(16) * np.uint64(16))
    total = int(off[-1] + sizes[-1])
    d = torch.empty(total, dtype=torch.uint8, device=dev)
    cache = {}
    for im, o in zip(imgs, off):  # (distinct arrays go up once)
        if id(im) not in cache:
            cache[id(im)] = torch.from_numpy(im.reshape(-1)).to(dev)
        d[int(o): int(o) + im.size] = cache[id(im)]
    ww = np.array([im.shape[1] for im in imgs], np.uint32)
    hh = np.array([im.shape[0] for im in imgs], np.uint32)
    ss = (ww * np.uint32(3)).astype(np.uint32)
    d_scores = torch.zeros(n, dtype=torch.int32, device=dev)
    d_detail = torch.zeros(n * DETAIL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()

    def run():
        _lib.check(L.cbh_quality_scores_dev(d.data_ptr(), n, off.ctypes.data, ww.ctypes.data, hh.ctypes.data,
                                            ss.ctypes.data, 3, d_scores.data_ptr(), d_detail.data_ptr(), None, None, 0,
                                            C.c_void_p(stream.cuda_stream)), "quality_scores")

    torch.cuda.synchronize()
    run()  # warm-up: code objects, the scratch arena's blocks
    run()
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
    nbytes = 0
    for w, h in zip(ww.tolist(), hh.tolist()):
        _, _, qw, qh = R.crop_dims(w, h)
        nbytes += qw * qh * 3 + 2 * ((qw + 15) // 16 * 16) * qh
    scores = d_scores.cpu().numpy()
    distinct = {}
    for i, im in enumerate(imgs):
        distinct.setdefault(id(im), (i, im))
    t0 = time.perf_counter()
    px, ok = 0, True
    for i, im in list(distinct.values())[:4]:
        ok &= int(R.quality_stencil(im)["score"]) == int(scores[i])
        px += im.shape[0] * im.shape[1]
    host_s = time.perf_counter() - t0
    med = float(np.median(ms))
    return {"workload": name, "images": n, "source_bytes": total, "algorithm_bytes": int(nbytes), "iters": iters,
            "event_ms_median": med, "event_ms_min": float(min(ms)), "event_ms_max": float(max(ms)),
            "wall_ms_median": float(np.median(wall)), "images_per_s": n / (med * 1e-3),
            "algorithm_bytes_per_s": nbytes / (med * 1e-3), "fraction_of_hbm_8TBps": nbytes / (med * 1e-3) / HBM_BYTES_PER_S,
            "numpy_restatement_megapixels_per_s_1core": px / host_s / 1e6,
            "device_megapixels_per_s": float(ww.astype(np.float64) @ hh.astype(np.float64)) / (med * 1e-3) / 1e6,
            "sample_scores_equal_numpy": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--ragged", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_scores.jsonl"))
    args = ap.parse_args()
    from cbird_amd import require_device

    require_device()  # no device: no number
    rng = np.random.default_rng(1)
    vga = [blocky(rng, 640, 480) for _ in range(8)]
    # members of duplicate groups: the same picture at the sizes people keep
    shapes = [(1920, 1080), (1600, 1200), (1280, 720), (1024, 768), (800, 600), (640, 480), (500, 375), (320, 240),
              (1080, 1350), (150, 150)]
    group = [blocky(rng, w, h) for w, h in shapes]
    order = rng.integers(0, len(group), args.ragged)
    results = [measure(f"{args.images} BGR images 640x480", lambda i: vga[i % 8], args.images, args.iters),
               measure(f"{args.ragged} BGR images of {len(shapes)} sizes from 150x150 to 1920x1080",
                       lambda i: group[int(order[i])], args.ragged, args.iters)]
    with open(args.out, "a") as f:
        for r in results:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
