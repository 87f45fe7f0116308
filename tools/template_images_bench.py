"""The fused template-match entry (cbird_amd/csrc/tmimages.hip) against the staged path a caller had before it, on one
MI355X: one 400 x 300 BGR template, 256 BGR candidates of mixed sizes up to twice its side (five distinct images, the
template under a similarity on a canvas, repeated), the reference's parameters (100 / 1000 features, cvThresh 25).

  fused_ms    cbh_template_match_images, host images in, results out: wall clock around the synchronous call
  staged_ms   the same answer from the entry points that existed before: cbh_bgr2gray_dev per geometry, orb.orb (upload,
              ORB, download of keypoints and descriptors), CvFeaturesIndex.radius_match per candidate (descriptors up
              again, records down), the gather in numpy, hashing.template_match (images up a second time) -- wall clock
  stages      the fused entry's stages on device-resident data, device events on a side stream around each stage call
              (its table uploads and its synchronisation included): grey, ORB, match + gather, estimate .. score
  resize      the ragged colour resize on 64 BGR images 1200 x 900 -> 800 x 600 beside k_resize_lanczos4
              (cbh_resize_lanczos4_dev) on the same pixels as grey planes: bytes = source + destination, per second
All after a warm-up call, median of --iters.  The two paths are checked to give the same results before they are timed.

    python tools/template_images_bench.py [--n 256] [--iters 5] [--out profiles/template_images.jsonl]
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
TW, TH, CH = 400, 300, 3
SIZES = [(400, 300), (600, 450), (800, 600), (640, 360), (500, 700)]


def wall(fn, iters):
    fn()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


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


def inputs(n):
    import template_match_rules as R

    rng = np.random.default_rng(400)
    tmpl = R.scene(rng, TH, TW, CH)
    base = []
    for k, (w, h) in enumerate(SIZES):
        sc = min(w / TW, h / TH) * 0.9
        m = R.similarity(4.0 * k, sc, 0.04 * w, 0.03 * h)
        base.append(np.maximum(R.warp_affine(tmpl, R.invert(m), w, h)[0], 1))
    return tmpl, [base[i % len(SIZES)] for i in range(n)]


def staged(L, tmpl, cands, params):
    """the path of tests/test_template_images.py::test_staged_path_equals_the_fused_entry for colour candidates"""
    import torch

    from cbird_amd import orb
    from cbird_amd.cvfeatures import CvFeaturesIndex
    from cbird_amd.hashing import template_match

    def gray(imgs):  # one call per geometry
        out = [None] * len(imgs)
        groups = {}
        for i, im in enumerate(imgs):
            groups.setdefault(im.shape, []).append(i)
        for (h, w, ch), ids in groups.items():
            d_src = torch.from_numpy(np.stack([imgs[i] for i in ids])).cuda()
            d_g = torch.empty((len(ids), h, w), dtype=torch.uint8, device="cuda")
            assert L.cbh_bgr2gray_dev(d_src.data_ptr(), len(ids), w, h, w * ch, w * h * ch, ch, d_g.data_ptr(), 0, None) == 0
            for i, g in zip(ids, d_g.cpu().numpy()):
                out[i] = g
        return out

    (_, t_xy, t_desc), = orb.orb(gray([tmpl]), params.needleFeatures)

    class Rows:
        id, path, keyPointDescriptors = 1, "template", t_desc

    idx = CvFeaturesIndex()
    idx.add([Rows])
    al, bl = [], []
    for _, c_xy, c_desc in orb.orb(gray(cands), params.haystackFeatures):
        rec = idx.radius_match(c_desc, params.cvThresh)[0] if len(c_desc) else np.zeros((0, 3), np.int32)
        al.append(t_xy[rec[:, 1]].reshape(-1, 2)), bl.append(c_xy[rec[:, 0]].reshape(-1, 2))
    return template_match(tmpl, cands, al, bl)


def stage_times(L, tmpl, cands, params, iters):
    import torch

    from cbird_amd.hashing import TEMPLATE_RESULT_DTYPE, TEMPLATE_IMAGE_RESULT_DTYPE, tm_params
    from cbird_amd.orb import KP_DTYPE
    from cbird_amd.quality import pack_images

    n = len(cands)
    buf, off, w, h, st = pack_images(cands)
    goff = np.zeros(n, np.uint64)
    goff[1:] = np.cumsum([(c.shape[0] * c.shape[1] + 15) // 16 * 16 for c in cands[:-1]])
    gtotal = int(goff[-1]) + cands[-1].shape[0] * cands[-1].shape[1]
    cap = params.haystackFeatures + 64
    stream = torch.cuda.Stream()
    s = C.c_void_p(stream.cuda_stream)
    dev = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
    d_t, d_img = torch.from_numpy(tmpl).cuda(), torch.from_numpy(buf).cuda()
    d_tg, d_g = dev(TW * TH), dev(gtotal)
    d_kp, d_after, d_desc, d_counts = dev(n * cap * KP_DTYPE.itemsize), dev(n * cap * 2, dt=torch.float32), dev(n * cap * 32), dev(n, dt=torch.int32)
    tcap = params.needleFeatures + 64
    t_kp, t_after, t_desc, t_count = dev(tcap * KP_DTYPE.itemsize), dev(tcap * 2, dt=torch.float32), dev(tcap * 32), dev(1, dt=torch.int32)
    zero, tw_, th_ = np.zeros(1, np.uint64), np.array([TW], np.uint32), np.array([TH], np.uint32)
    tst = np.array([TW * CH], np.uint32)
    torch.cuda.synchronize()
    ok = lambda rc, what: _check(rc, what)  # noqa: E731

    def gray():
        ok(L.cbh_bgr2gray_ragged_dev(d_t.data_ptr(), 1, zero.ctypes.data, tw_.ctypes.data, th_.ctypes.data, tst.ctypes.data, CH,
                                     zero.ctypes.data, d_tg.data_ptr(), 0, s), "grey")
        ok(L.cbh_bgr2gray_ragged_dev(d_img.data_ptr(), n, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, CH,
                                     goff.ctypes.data, d_g.data_ptr(), 0, s), "grey")

    def orb():
        ok(L.cbh_orb_dev(d_tg.data_ptr(), 1, zero.ctypes.data, tw_.ctypes.data, th_.ctypes.data, tw_.ctypes.data,
                         params.needleFeatures, tcap, t_kp.data_ptr(), t_after.data_ptr(), t_desc.data_ptr(), t_count.data_ptr(),
                         0, s), "orb")
        ok(L.cbh_orb_dev(d_g.data_ptr(), n, goff.ctypes.data, w.ctypes.data, h.ctypes.data, w.ctypes.data,
                         params.haystackFeatures, cap, d_kp.data_ptr(), d_after.data_ptr(), d_desc.data_ptr(),
                         d_counts.data_ptr(), 0, s), "orb")
        stream.synchronize()

    t = {"gray_ms": timed(stream, gray, iters), "orb_ms": timed(stream, orb, iters)}
    n_train = min(int(t_count.item()), tcap)
    assert int(d_counts.max().item()) <= cap
    first = np.zeros(n + 1, np.uint64)
    probe = lambda pts, a, b: L.cbh_tm_match_points_dev(  # noqa: E731
        t_desc.data_ptr(), t_after.data_ptr(), n_train, d_desc.data_ptr(), d_after.data_ptr(), d_counts.data_ptr(), n, cap,
        params.cvThresh, None, a, b, pts, first.ctypes.data, 0, s)
    probe(0, None, None)  # the count alone: CBH_E_OVERFLOW with `first` complete, or nothing matched
    total = int(first[-1])
    d_a, d_b = dev(max(total, 1) * 2, dt=torch.float32), dev(max(total, 1) * 2, dt=torch.float32)
    t["match_gather_ms"] = timed(stream, lambda: ok(probe(total, d_a.data_ptr(), d_b.data_ptr()), "match"), iters)
    scales = np.ones(n, np.float32)
    d_res = dev(n * TEMPLATE_RESULT_DTYPE.itemsize)

    def score():
        ok(L.cbh_template_match_dev(d_t.data_ptr(), TW, TH, TW * CH, CH, d_img.data_ptr(), n, off.ctypes.data, w.ctypes.data,
                                    h.ctypes.data, st.ctypes.data, CH, d_a.data_ptr(), d_b.data_ptr(), first.ctypes.data,
                                    scales.ctypes.data, d_res.data_ptr(), None, 0, s), "score")

    t["estimate_to_score_ms"] = timed(stream, score, iters)
    res = np.zeros(n, TEMPLATE_IMAGE_RESULT_DTYPE)
    p = tm_params(params)
    t["fused_dev_ms"] = timed(stream, lambda: ok(L.cbh_template_match_images_dev(
        d_t.data_ptr(), TW, TH, TW * CH, d_img.data_ptr(), n, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data,
        CH, p.ctypes.data, res.ctypes.data, None, 0, s), "fused"), iters)
    t["matched_pairs"] = total
    return t


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: rc={rc}")


def resize_rates(L, iters):
    import torch

    n, (sw, sh), (dw, dh) = 64, (1200, 900), (800, 600)
    rng = np.random.default_rng(1)
    src = torch.from_numpy(rng.integers(0, 256, (n, sh, sw, CH), dtype=np.uint8)).cuda()
    grey = torch.from_numpy(rng.integers(0, 256, (n * CH, sh, sw), dtype=np.uint8)).cuda()  # the same pixel count
    dst = torch.zeros(n * dw * dh * CH, dtype=torch.uint8, device="cuda")
    off = np.arange(n, dtype=np.uint64) * np.uint64(sw * sh * CH)
    doff = np.arange(n, dtype=np.uint64) * np.uint64(dw * dh * CH)
    full = lambda v: np.full(n, v, np.uint32)  # noqa: E731
    w, h, st, tw_, th_ = full(sw), full(sh), full(sw * CH), full(dw), full(dh)
    stream = torch.cuda.Stream()
    s = C.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize()
    ragged = timed(stream, lambda: _check(L.cbh_resize_lanczos4_ragged_dev(
        src.data_ptr(), n, off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data, CH, doff.ctypes.data, tw_.ctypes.data,
        th_.ctypes.data, dst.data_ptr(), 0, s), "ragged resize"), iters)
    plain = timed(stream, lambda: _check(L.cbh_resize_lanczos4_dev(grey.data_ptr(), n * CH, sw, sh, sw, sw * sh, dw, dh,
                                                                   dst.data_ptr(), 0, s), "resize"), iters)
    nbytes = n * CH * (sw * sh + dw * dh)
    return {"resize_images": n, "resize_from": [sw, sh], "resize_to": [dw, dh], "resize_bytes": nbytes,
            "resize_ragged_ms": ragged, "resize_ragged_bytes_per_s": nbytes / (ragged * 1e-3),
            "resize_lanczos4_ms": plain, "resize_lanczos4_bytes_per_s": nbytes / (plain * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_images.jsonl"))
    args = ap.parse_args()
    from cbird_amd import _lib, orb, require_device
    from cbird_amd.hashing import template_match_images
    from cbird_amd.index import SearchParams

    require_device()  # no device: no number
    L = _lib.lib()
    orb.set_pattern(orb.synthetic_pattern())
    params = SearchParams()
    tmpl, cands = inputs(args.n)
    fused = template_match_images(tmpl, cands, params)
    assert staged(L, tmpl, cands, params).tobytes() == fused["r"].tobytes(), "the two paths disagree"
    r = {"candidates": args.n, "template": [TW, TH, CH], "candidate_sizes": SIZES, "iters": args.iters,
         "scored": int((fused["status"] == 0).sum()), "median_score": float(np.median(fused["r"]["score"][fused["status"] == 0])),
         "fused_ms": wall(lambda: template_match_images(tmpl, cands, params), args.iters),
         "staged_ms": wall(lambda: staged(L, tmpl, cands, params), args.iters)}
    r["fused_not_slower"] = r["fused_ms"] <= r["staged_ms"]
    r.update(stage_times(L, tmpl, cands, params, args.iters))
    r.update(resize_rates(L, args.iters))
    print(json.dumps(r), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
