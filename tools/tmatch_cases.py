#!/usr/bin/env python3
"""Write the cases file tools/gen_golden_opencv.cpp reads for its template-match records (step 2b of
tools/pin_with_opencv.sh): the numpy model's own cases of tests/template_match_rules.py --
    E  every point-pair list of R.estimate_fixture() and of the chain's group (as they are and divided by candScale)
    W  every transform of R.warp_transforms() that lies inside the reference's integer domain, on candidates of
       R.WARP_IMAGE_SIZES, a 33 x 47 template, the channel count going round 1 / 3 / 4
The images are not in the file: channel c of a w x h image is gen_image(w, h, seed + c), which both sides generate.

    python tools/tmatch_cases.py > tmatch_cases.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import template_match_rules as R  # noqa: E402

TW, TH = 33, 47


def estimate_cases():
    """[(name, a float32 [k, 2], b float32 [k, 2])]"""
    out = [(n, a, b) for n, (a, b) in R.estimate_fixture().items()]
    _, _, al, bl, scales = R.chain_fixture()
    for i, (a, b, s) in enumerate(zip(al, bl, scales)):
        out.append((f"chain{i}", a, b))
        out.append((f"chain{i}_unscaled", a, (np.asarray(b, np.float32) / np.float32(s)).astype(np.float32)))
    return out


def warp_cases():
    """[(name, w, h, channels, seed, tw, th, m float64 [6])]"""
    out, k = [], 0
    for w, h in R.WARP_IMAGE_SIZES:
        for name, m in R.warp_transforms(w, h).items():
            if name == R.BEYOND:
                continue  # undefined in the reference
            out.append((f"{w}x{h}_{name}", w, h, (1, 3, 4)[k % 3], 2000 + 7 * k, TW, TH, np.asarray(m, np.float64)))
            k += 1
    return out


def lines():
    for name, a, b in estimate_cases():
        pts = np.concatenate([np.asarray(a, np.float32).reshape(-1, 2), np.asarray(b, np.float32).reshape(-1, 2)], 1)
        yield " ".join(["E", name, str(len(pts))] + ["%08x" % v for v in pts.reshape(-1).view(np.uint32)])
    for name, w, h, ch, seed, tw, th, m in warp_cases():
        yield " ".join(["W", name, str(w), str(h), str(ch), str(seed), str(tw), str(th)] +
                       ["%016x" % v for v in m.view(np.uint64)])


if __name__ == "__main__":
    for ln in lines():
        print(ln)
