"""Per-stage times of the template-match chain (cbird_amd/csrc/tmatch.hip) at the reference's own sizes: 100 template
features, 1000 candidate features (-p.nf / -p.hf: here 1000 matched pairs per candidate, 70 % inliers), BGR candidate
images of 400 .. 600 px, a 400 x 300 template, 32 to 1024 candidates.  Everything is resident on the device; each stage is
timed by device events on a side stream around its whole call (table uploads, launches and the call's synchronisation
included), median of --iters after a warm-up:
    estimate  cbh_estimate_rigid_dev on the 2 n lists the chain solves (the points as they are and divided by candScale)
    warp      cbh_warp_affine_dev with the matrices of the first estimate
    hashes    cbh_template_hashes_dev on the warped patches
    chain     cbh_template_match_dev: all of the above plus the roi and the result records
The warp's bytes are what it must move by shape -- the patches written once, plus four taps of `channels` bytes per pixel
read -- set against the 8 TB/s of HBM.

    python tools/template_match_bench.py [--counts 32,128,1024] [--iters 5] [--out profiles/template_match.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_BYTES_PER_S = 8e12
TW, TH, CH = 400, 300, 3


def timed(stream, fn, iters):
    import torch

    fn()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def measure(n, iters, pairs):
    import torch

    import template_match_rules as R
    from cbird_amd import _lib
    from cbird_amd.hashing import TEMPLATE_RESULT_DTYPE, pack_point_lists
    from cbird_amd.quality import pack_images

    L = _lib.lib()
    rng = np.random.default_rng(n)
    tmpl = R.scene(rng, TH, TW, CH)
    sizes = [(600, 450), (400, 600), (512, 512), (600, 400)]
    base, al, bl = [], [], []
    for k, (w, h) in enumerate(sizes):  # four distinct candidates, repeated
        m = R.similarity(10.0 * k, 0.8 + 0.1 * k, 30.0 + 5 * k, 20.0 + 3 * k)
        base.append(R.scene(rng, h, w, CH))
        a, b = R.planted(rng, pairs, int(pairs * 0.7), m, (TW, TH), (TW / 2, TH / 2))
        al.append(a), bl.append(b)
    pick = [i % len(sizes) for i in range(n)]
    buf, off, ww, hh, ss = pack_images([base[i] for i in pick])
    a, b, first = pack_point_lists([al[i] for i in pick], [bl[i] for i in pick])
    scales = np.where(np.arange(n) % 2 == 0, 1.0, 0.37).astype(np.float32)
    # the 2 n lists of the chain: every list twice, the second divided by its scale
    a2, b2, first2 = pack_point_lists([al[i] for i in pick for _ in (0, 1)],
                                      [bl[i] / np.float32(1.0 if r == 0 else scales[j]) for j, i in enumerate(pick)
                                       for r in (0, 1)])
    d_t, d_img, d_a, d_b, d_a2, d_b2 = (torch.from_numpy(v).cuda() for v in (tmpl, buf, a, b, a2, b2))
    d_m2 = torch.zeros(2 * n * 6, dtype=torch.float64, device="cuda")
    d_f2 = torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
    d_m, d_f = d_m2.view(n, 12)[:, :6].contiguous(), d_f2.view(n, 2)[:, 0].contiguous()
    d_p = torch.zeros(n * TH * TW * CH, dtype=torch.uint8, device="cuda")
    d_h = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(n * TEMPLATE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    s = C.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize()

    def estimate():
        _lib.check(L.cbh_estimate_rigid_dev(d_a2.data_ptr(), d_b2.data_ptr(), 2 * n, first2.ctypes.data, d_m2.data_ptr(),
                                            d_f2.data_ptr(), None, 0, s), "estimate")

    estimate()
    stream.synchronize()
    d_m.copy_(d_m2.view(n, 12)[:, :6])
    d_f.copy_(d_f2.view(n, 2)[:, 0])
    torch.cuda.synchronize()

    def warp():
        _lib.check(L.cbh_warp_affine_dev(d_img.data_ptr(), n, off.ctypes.data, ww.ctypes.data, hh.ctypes.data,
                                         ss.ctypes.data, CH, d_m.data_ptr(), d_f.data_ptr(), TW, TH, d_p.data_ptr(), None, 0,
                                         s), "warp")

    def hashes():
        _lib.check(L.cbh_template_hashes_dev(d_p.data_ptr(), n, TW, TH, TW * CH, TW * TH * CH, CH, d_t.data_ptr(), TW * CH,
                                             CH, d_h.data_ptr(), d_h.data_ptr() + 8 * n, 0, s), "hashes")
        stream.synchronize()

    def chain():
        _lib.check(L.cbh_template_match_dev(d_t.data_ptr(), TW, TH, TW * CH, CH, d_img.data_ptr(), n, off.ctypes.data,
                                            ww.ctypes.data, hh.ctypes.data, ss.ctypes.data, CH, d_a.data_ptr(),
                                            d_b.data_ptr(), first.ctypes.data, scales.ctypes.data, d_res.data_ptr(),
                                            d_p.data_ptr(), 0, s), "chain")

    t = {k: timed(stream, f, iters) for k, f in (("estimate", estimate), ("warp", warp), ("hashes", hashes),
                                                 ("chain", chain))}
    res = d_res.cpu().numpy().view(TEMPLATE_RESULT_DTYPE)
    warp_bytes = n * TW * TH * CH * (1 + 4)
    return {"candidates": n, "pairs_per_candidate": pairs, "template": [TW, TH, CH], "candidate_sizes": sizes,
            "iters": iters, "estimate_ms": t["estimate"], "warp_ms": t["warp"], "hashes_ms": t["hashes"],
            "chain_ms": t["chain"], "candidates_per_s": n / (t["chain"] * 1e-3), "found": int(res["found"].sum()),
            "median_score": float(np.median(res["score"][res["found"] != 0])) if res["found"].any() else None,
            "warp_algorithm_bytes": warp_bytes, "warp_bytes_per_s": warp_bytes / (t["warp"] * 1e-3),
            "warp_fraction_of_hbm_8TBps": warp_bytes / (t["warp"] * 1e-3) / HBM_BYTES_PER_S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="32,128,1024")
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_match.jsonl"))
    args = ap.parse_args()
    from cbird_amd import require_device

    require_device()  # no device: no number
    with open(args.out, "a") as f:
        for n in (int(v) for v in args.counts.split(",")):
            r = measure(n, args.iters, args.pairs)
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
