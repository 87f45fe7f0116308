"""demosaicHough throughput (cbird_amd/csrc/demosaic.hip): --sheets contact sheets resident on the device, at 1024 x 768
(a 4 x 3 grid of smooth tiles, then a staggered 4 + 3 sheet every fourth) and at the test suite's sizes, through the stage
entries -- cbh_auto_contrast_dev (the cuts alone), cbh_edge_maps_dev (steps 1-4), cbh_grid_lines_dev (steps 1-5) and
cbh_demosaic_dev (everything, subdivision passes included) -- each timed by device events on a side stream after warm-up
calls.  The time is that of the whole call: the host builds and uploads its tables, the kernels run, the hysteresis flag
comes back after every launch, the host runs steps 6-8.  A stage's own time is the difference of two entries.
Bytes: what the passes of one level must move through HBM if every plane is read and written once per kernel -- the source
twice (histogram, classes), the class plane written, read and written once per hysteresis launch, read for the edges, the
edge plane written and read -- against the 8 TB/s of the MI355X.  The first sheets are checked against the numpy model
(tests/demosaic_rules.py).  Prints and gates nothing else.

    python tools/demosaic_bench.py [--sheets 256] [--iters 5] [--out profiles/demosaic.jsonl]
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
HBM_PEAK = 8.0e12


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
    return float(np.median(ms)), float(min(ms)), float(max(ms)), float(np.median(wall))


def bench(name, pool, n, iters, check):
    """pool: distinct BGR sheets, repeated to n"""
    import torch

    import demosaic_rules as M
    from cbird_amd import _lib
    from cbird_amd.demosaic import default_params
    from cbird_amd.difference import _pack_tensors

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    imgs = [pool[i % len(pool)] for i in range(n)]
    buf, off, w, h, st = _pack_tensors([torch.from_numpy(im).to(dev) for im in imgs], dev)
    pixels = int((w.astype(np.int64) * h).sum())
    p = default_params()
    d_cuts = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    d_edges = torch.zeros(pixels, dtype=torch.uint8, device=dev)
    hor, ver = np.zeros(int(h.sum()), np.int32), np.zeros(int(w.sum()), np.int32)
    hf, vf, first = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
    rects = np.zeros((64 * n, 4), np.int32)
    passes = C.c_uint32(0)
    stream = torch.cuda.Stream()
    s = C.c_void_p(stream.cuda_stream)
    tabs = (off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, 3)
    runs = {
        "contrast": lambda: _lib.check(L.cbh_auto_contrast_dev(buf.data_ptr(), n, *tabs, p.clip_pct, None, d_cuts.data_ptr(), None,
                                                               0, s), "auto_contrast"),
        "edge_maps": lambda: _lib.check(L.cbh_edge_maps_dev(buf.data_ptr(), n, *tabs, C.addressof(p), d_edges.data_ptr(), None,
                                                            C.addressof(passes), 0, s), "edge_maps"),
        "grid_lines": lambda: _lib.check(L.cbh_grid_lines_dev(buf.data_ptr(), n, *tabs, C.addressof(p), hor.ctypes.data,
                                                              hf.ctypes.data, ver.ctypes.data, vf.ctypes.data, 0, s), "grid_lines"),
        "demosaic": lambda: _lib.check(L.cbh_demosaic_dev(buf.data_ptr(), n, *tabs, C.addressof(p), rects.ctypes.data, len(rects),
                                                          first.ctypes.data, 0, s), "demosaic"),
    }
    torch.cuda.synchronize()
    out = {"workload": f"{n} BGR sheets {name}, device resident", "sheets": n, "pixels": pixels, "iters": iters}
    for key, run in runs.items():
        run()  # warm-up: code objects, the scratch arena's blocks
        run()
        med, lo, hi, wall = timed(run, stream, iters)
        out[key] = {"event_ms_median": med, "event_ms_min": lo, "event_ms_max": hi, "wall_ms_median": wall,
                    "us_per_sheet": med * 1e3 / n}
    torch.cuda.synchronize()
    stages = {"contrast_cuts": out["contrast"]["event_ms_median"],
              "blur_canny_hysteresis_edges": out["edge_maps"]["event_ms_median"] - out["contrast"]["event_ms_median"],
              "votes_and_lines": out["grid_lines"]["event_ms_median"] - out["edge_maps"]["event_ms_median"],
              "grids_rects_subdivision": out["demosaic"]["event_ms_median"] - out["grid_lines"]["event_ms_median"]}
    out["stage_ms"] = stages
    out["hysteresis_launches"] = int(passes.value)
    # one level: source 2 x 3 bytes a pixel; classes 1 written + 2 per hysteresis launch + 1 read; edges 1 written, 1 read
    moved = pixels * (6 + 1 + 2 * int(passes.value) + 1 + 2)
    out["level_bytes"] = moved
    out["level_bytes_per_s"] = moved / (out["grid_lines"]["event_ms_median"] * 1e-3)
    out["share_of_hbm_peak"] = out["level_bytes_per_s"] / HBM_PEAK
    out["rectangles"] = int(first[n])
    ok = True
    for i in range(check):
        want = [tuple(r) for r in M.demosaic(imgs[i])]
        ok = ok and [tuple(r) for r in rects[first[i]:first[i + 1]].tolist()] == want
    out["first_sheets_equal_numpy"] = bool(ok)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sheets", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demosaic.jsonl"))
    args = ap.parse_args()
    from cbird_amd import require_device

    require_device()  # no device: no number
    import demosaic_rules as M

    big = [M.sheet((4, 4, 4), 240, 12, 240, 1024, seed=k)[0] for k in range(3)] + [M.sheet((4, 3, 4), 240, 12, 240, 1024, seed=9)[0]]
    assert all(b.shape == (768, 1024, 3) for b in big)
    small = [M.sheet(*layout, seed=1)[0] for layout in M.LAYOUTS]
    results = [bench("1024x768", big, args.sheets, args.iters, 2), bench("of the test layouts (212..596 px)", small, args.sheets,
                                                                         args.iters, len(small))]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in results:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
