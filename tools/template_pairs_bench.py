"""The grouped template match (cbh_template_match_pairs_dev, cbird_amd/csrc/tmimages.hip) against what a caller had
before it -- a loop of cbh_template_match_images_dev, one call per result group -- on the same device-resident images in
the same run, on one MI355X.  BGR templates of five sizes (131 x 97 .. 240 x 180), every candidate its template under a
similarity on a canvas 1.25 times its size, the reference's parameters (100 / 1000 features, cvThresh 25).

  shapes      groups x candidates per group: 1024 x 4 (what -similar -p.tm 1 produces), 16 x 256, 4096 x 1; every group
              has a table row of its own for its template, so nothing is shared between groups on either side
  grouped_ms  one cbh_template_match_pairs_dev call for all pairs: wall clock around the synchronous call
  loop_ms     cbh_template_match_images_dev once per group, same images, same stream: wall clock around the loop
  stages      the grouped entry's own device-event times (cbh_tm_pairs_stage_ms; a separate call, every stage then ends in
              a wait): grey + resize, ORB of the templates, ORB of the candidates, match + gather, estimate .. score; and
              how many runs of one template size and how many launch_dcthash calls the shape had
Both sides are asserted to give equal bytes before anything is timed.  Medians of --iters after a warm-up call.

    python tools/template_pairs_bench.py [--iters 3] [--scale 1] [--out profiles/template_pairs.jsonl]
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
CH = 3
TMPL_SIZES = [(160, 128), (200, 150), (131, 97), (240, 180), (180, 200)]
SHAPES = [(1024, 4), (16, 256), (4096, 1)]
VARIANTS = 4  # distinct candidates per template size


def wall(fn, iters):
    fn()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def pool():
    """per template size: (template, VARIANTS candidates)"""
    import template_match_rules as R

    rng = np.random.default_rng(500)
    out = []
    for tw, th in TMPL_SIZES:
        tmpl = R.scene(rng, th, tw, CH)
        w, h = tw * 5 // 4, th * 5 // 4
        cands = [np.maximum(R.warp_affine(tmpl, R.invert(R.similarity(3.0 * k, 1.0 + 0.05 * k, 0.05 * w, 0.04 * h)), w, h)[0], 1)
                 for k in range(VARIANTS)]
        out.append((tmpl, cands))
    return out


def table(groups, per):
    """the image table of `groups` groups of `per` candidates: group g's template (size g mod 5), then its candidates"""
    from cbird_amd.quality import pack_images

    p = pool()
    images, pt, pc = [], [], []
    for g in range(groups):
        tmpl, cands = p[g % len(p)]
        t = len(images)
        images.append(tmpl)
        for k in range(per):
            pt.append(t), pc.append(len(images))
            images.append(cands[k % VARIANTS])
    return pack_images(images), np.array(pt, np.uint32), np.array(pc, np.uint32)


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: rc={rc}")


def measure(L, groups, per, params, iters):
    import torch

    from cbird_amd.hashing import TEMPLATE_IMAGE_RESULT_DTYPE, tm_params

    (buf, off, w, h, st), pt, pc = table(groups, per)
    n_imgs, n = len(off), len(pt)
    d_img = torch.from_numpy(buf).cuda()
    stream = torch.cuda.Stream()
    s = C.c_void_p(stream.cuda_stream)
    p = tm_params(params)
    res_g, res_l = np.zeros(n, TEMPLATE_IMAGE_RESULT_DTYPE), np.zeros(n, TEMPLATE_IMAGE_RESULT_DTYPE)
    torch.cuda.synchronize()

    def grouped():
        _check(L.cbh_template_match_pairs_dev(d_img.data_ptr(), n_imgs, off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                              st.ctypes.data, CH, pt.ctypes.data, pc.ctypes.data, n, p.ctypes.data,
                                              res_g.ctypes.data, 0, s), "grouped")

    # the loop's tables, built once: group g's candidates are rows pc[g * per .. (g + 1) * per) of the same buffer
    coff, cw, chh, cst = (np.ascontiguousarray(v[pc]) for v in (off, w, h, st))
    base = d_img.data_ptr()
    row = TEMPLATE_IMAGE_RESULT_DTYPE.itemsize

    def loop():
        for g in range(groups):
            t, k = int(pt[g * per]), g * per
            _check(L.cbh_template_match_images_dev(base + int(off[t]), int(w[t]), int(h[t]), int(st[t]), base, per,
                                                   coff[k:].ctypes.data, cw[k:].ctypes.data, chh[k:].ctypes.data,
                                                   cst[k:].ctypes.data, CH, p.ctypes.data, res_l.ctypes.data + k * row, None, 0,
                                                   s), "loop")

    grouped(), loop()
    assert res_g.tobytes() == res_l.tobytes(), "the grouped entry and the loop disagree"
    r = {"groups": groups, "per_group": per, "pairs": n, "image_bytes": int(buf.size), "iters": iters,
         "scored": int((res_g["status"] == 0).sum()), "equal_bytes": True,
         "grouped_ms": wall(grouped, iters), "loop_ms": wall(loop, max(1, min(iters, 3)))}
    r["loop_over_grouped"] = r["loop_ms"] / r["grouped_ms"]
    r["grouped_us_per_pair"], r["loop_us_per_group"] = 1e3 * r["grouped_ms"] / n, 1e3 * r["loop_ms"] / groups
    ms, sizes, launches = (C.c_double * 5)(), C.c_uint32(0), C.c_uint32(0)
    L.cbh_tm_pairs_stage_ms(1, None, None, None)
    try:
        grouped()
    finally:
        L.cbh_tm_pairs_stage_ms(0, ms, C.byref(sizes), C.byref(launches))
    for name, v in zip(("gray_resize_ms", "orb_templates_ms", "orb_candidates_ms", "match_gather_ms", "estimate_to_score_ms"), ms):
        r[name] = float(v)
    r["template_size_runs"], r["hash_launches"] = int(sizes.value), int(launches.value)
    r["distinct_template_sizes"] = len({(int(w[t]), int(h[t])) for t in set(pt.tolist())})
    r["hash_launch_note"] = "launch_dcthash takes arena scratch per call (no driver call once warm) and does not synchronise"
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1, help="divide every shape's group count by this (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_pairs.jsonl"))
    args = ap.parse_args()
    from cbird_amd import _lib, orb, require_device
    from cbird_amd.index import SearchParams

    require_device()  # no device: no number
    L = _lib.lib()
    orb.set_pattern(orb.synthetic_pattern())
    params = SearchParams()
    for groups, per in SHAPES:
        r = measure(L, max(1, groups // args.scale), per, params, args.iters)
        print(json.dumps(r), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
