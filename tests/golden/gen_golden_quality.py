#!/usr/bin/env python3
"""Golden vectors for qualityScore (src/cimgops.cpp:313-596) from the REAL CImg: a small wrapper, compiled into a
temporary directory against the reference's vendored src/lib/CImg.h where it lies (cimg_display 0, no jpeg / png), runs
CImg's own crop (the reference's call), get_norm(1), the conversion to CImg<uint8_t>, transpose and operator| on
three-channel images filled the way qImageToCImg fills them; the three short loops of the reference (makeDiff, makeEdge,
longEdgeCount) and its score formula are restated in the wrapper.  Nothing compiled is kept and no reference text is
copied.  Where the reference has no defined answer the wrapper does not run it: a cropped image below 3 x 3 (buffer
overrun, :337) and an image without edges (NaN to int, :495 / :592) are recorded as "no score", INT32_MIN.

    CBIRD_REF=/path/to/reference python tests/golden/gen_golden_quality.py   -> tests/golden/quality_cimg.npz

The tests read only the .npz."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_quality_rules as R  # noqa: E402  (case builders only; the expected values come from the wrapper)

REF = os.environ.get("CBIRD_REF", "/root/reference")

WRAPPER = r"""
#define cimg_display 0
#include "lib/CImg.h"
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace cimg_library;
typedef CImg<uint8_t> img8;

// |left - right| of the two neighbours inside every row, first and last column 0; returns the sum
static double diff_rows(const img8& img, img8& diff) {
  const unsigned w = img.width(), h = img.height();
  double sum = 0;
  for (unsigned y = 0; y < h; ++y) {
    const uint8_t* s = img.data() + y * w;
    uint8_t* d = diff.data() + y * w;
    d[0] = 0;
    for (unsigned x = 1; x < w - 1; ++x) {
      const double v = abs(int(s[x - 1]) - int(s[x + 1]));
      sum += v;
      d[x] = v;
    }
    d[w - 1] = 0;
  }
  return sum;
}

// a difference above the mean that is greater than both neighbouring candidates
static void edge_rows(const img8& diff, float mean, img8& edge) {
  const unsigned w = diff.width(), h = diff.height();
  const uint8_t m = uint8_t(mean);
  for (unsigned y = 0; y < h; ++y) {
    const uint8_t* d = diff.data() + y * w;
    uint8_t* e = edge.data() + y * w;
    e[0] = 0;
    uint8_t center = d[0] > m ? d[0] : 0, right = d[1] > m ? d[1] : 0;
    for (unsigned x = 1; x < w - 1; ++x) {
      const uint8_t left = center;
      center = right;
      right = d[x + 1] > m ? d[x + 1] : 0;
      e[x] = center > left && center > right ? 255 : 0;
    }
    e[w - 1] = 0;
  }
}

// runs longer than 1 that a zero ends, scanning positions 1 .. w-2 of every row of the TRANSPOSED edge map
static int long_runs(const img8& edgeT) {
  const unsigned w = edgeT.width(), h = edgeT.height();
  int count = 0;
  for (unsigned y = 0; y < h; ++y) {
    const uint8_t* s = edgeT.data() + y * w;
    int len = 0;
    for (unsigned x = 1; x < w - 1; ++x) {
      if (s[x] != 0) ++len;
      else {
        if (len > 1) ++count;
        len = 0;
      }
    }
  }
  return count;
}

static void one_direction(const img8& img, img8& diff, img8& edge, double& sum, float& mean, int& runs) {
  sum = diff_rows(img, diff);
  mean = sum / ((img.width() - 1) * (img.height() - 1));
  edge_rows(diff, mean, edge);
  img8 edgeT = edge;
  edgeT.transpose();
  runs = long_runs(edgeT);
}

template <class T> static void put(FILE* f, const T& v) { fwrite(&v, sizeof v, 1, f); }

int main(int argc, char** argv) {
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  int32_t n = 0;
  if (!in || !out || fread(&n, 4, 1, in) != 1) return 1;
  for (int i = 0; i < n; ++i) {
    int32_t W, H;
    if (fread(&W, 4, 1, in) != 1 || fread(&H, 4, 1, in) != 1) return 1;
    std::vector<uint8_t> bgr(size_t(W) * H * 3);
    if (fread(bgr.data(), 1, bgr.size(), in) != bgr.size()) return 1;
    img8 src(W, H, 1, 3);  // planes r, g, b
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const uint8_t* p = &bgr[(size_t(y) * W + x) * 3];
        src(x, y, 0, 0) = p[2];
        src(x, y, 0, 1) = p[1];
        src(x, y, 0, 2) = p[0];
      }
    const int hCrop = int(src.width() * 0.10), vCrop = int(src.height() * 0.10);
    src.crop(hCrop, vCrop, 0, 0, src.width() - hCrop, src.height() - vCrop, 0, 0);
    img8 img = src.get_norm(1);
    const int32_t w = img.width(), h = img.height();
    if (w < 3 || h < 3) {
      put(out, int32_t(0)), put(out, int32_t(0));
      continue;
    }
    img8 imgT = img;
    imgT.transpose();
    img8 hDiff(w, h), hEdge(w, h), vDiff(h, w), vEdge(h, w);
    double hSum, vSum;
    float hMean, vMean;
    int hRuns, vRuns;
    one_direction(img, hDiff, hEdge, hSum, hMean, hRuns);
    one_direction(imgT, vDiff, vEdge, vSum, vMean, vRuns);
    vEdge.transpose();
    vDiff.transpose();
    const img8 edge = vEdge | hEdge;
    int numEdges = 0;
    for (int y = 1; y < h - 1; ++y)
      for (int x = 1; x < w - 1; ++x)
        if (edge(x, y)) ++numEdges;
    int32_t score = INT_MIN;
    if (numEdges) {
      volatile float elr = float(vRuns + hRuns) / numEdges;
      volatile float er = float(numEdges) / ((unsigned(w) - 2) * (unsigned(h) - 2));
      volatile float a = 100 * er, b = 100 * elr;  // (volatile: two rounded products, then the sum, on any compiler)
      volatile float s = a + b;
      score = int(s);
    }
    put(out, w), put(out, h);
    fwrite(img.data(), 1, size_t(w) * h, out);
    fwrite(edge.data(), 1, size_t(w) * h, out);
    fwrite(hDiff.data(), 1, size_t(w) * h, out);
    fwrite(vDiff.data(), 1, size_t(w) * h, out);
    put(out, uint64_t(hSum)), put(out, uint64_t(vSum)), put(out, hMean), put(out, vMean);
    put(out, int32_t(hRuns)), put(out, int32_t(vRuns)), put(out, int32_t(numEdges)), put(out, score);
  }
  fclose(out);
  return 0;
}
"""


def golden_images():
    """about 25 three-channel images: most below 64 px on a side, three around 200 px"""
    rng = np.random.default_rng(777)
    imgs = []
    for w, h in [(2, 2), (3, 9), (9, 3), (10, 10), (11, 19), (19, 11), (20, 20), (1, 17), (33, 2)]:
        imgs.append(R.noise(rng, w, h, 3))
    for w, h, cell in [(17, 23, 3), (31, 40, 3), (48, 33, 4), (63, 63, 4), (64, 21, 3), (21, 64, 4), (57, 60, 3)]:
        imgs.append(R.blocky(rng, w, h, 3, cell))
    imgs.append(np.full((25, 31, 3), 90, np.uint8))  # no edges
    busy = R.noise(rng, 40, 30, 3)
    busy[..., 2] = 17  # red constant
    imgs.append(busy)
    for name in ("run_ends_at_L-2", "run_from_0", "run_of_2_ends_at_3"):
        p = R.run_plane({"run_ends_at_L-2": [8, 9, 10], "run_from_0": [0, 1], "run_of_2_ends_at_3": [1, 2]}[name])
        imgs.append(R.embed(p, rng, 3))
        imgs.append(R.embed(np.ascontiguousarray(p.T), rng, 3))
    imgs.append(R.blocky(rng, 200, 160, 3, 4))
    imgs.append(R.blocky(rng, 181, 212, 3, 3))
    imgs.append(R.embed(R.strip_plane(rng, 170, 150, 16), rng, 3))
    return imgs


def main():
    imgs = golden_images()
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "quality_cimg.cpp"), os.path.join(tmp, "quality_cimg")
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        open(src, "w").write(WRAPPER)
        # -O2 for baseline x86-64 (no FMA): float steps are rounded one by one, as in the reference's release build
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-w", "-I" + os.path.join(REF, "src"),
                               "-Dcimg_display=0", "-o", exe, src, "-lpthread"])
        with open(fin, "wb") as f:
            f.write(np.int32(len(imgs)).tobytes())
            for im in imgs:
                f.write(np.array([im.shape[1], im.shape[0]], np.int32).tobytes())
                f.write(np.ascontiguousarray(im).tobytes())
        subprocess.check_call([exe, fin, fout])
        raw = open(fout, "rb").read()
    pos = 0

    def take(dtype, count=1):
        nonlocal pos
        a = np.frombuffer(raw, dtype, count, pos)
        pos += a.nbytes
        return a

    cols = {f: [] for f in R.FIELDS}
    planes = {k: [] for k in ("plane", "edge", "hd", "vd")}
    offs = {k: [] for k in planes}
    total = 0
    for im in imgs:
        qw, qh = (int(v) for v in take(np.int32, 2))
        rec = dict.fromkeys(R.FIELDS, 0)
        rec["score"] = R.NO_SCORE
        for k in planes:
            offs[k].append(total)
            planes[k].append(take(np.uint8, qw * qh))
        total += qw * qh
        if qw:
            rec["h_sum"], rec["v_sum"] = (int(v) for v in take(np.uint64, 2))
            rec["h_mean"], rec["v_mean"] = take(np.float32, 2)
            rec["h_long"], rec["v_long"], rec["num_edges"], rec["score"] = (int(v) for v in take(np.int32, 4))
            rec["qw"], rec["qh"] = qw, qh
        for f in R.FIELDS:
            cols[f].append(rec[f])
    assert pos == len(raw)
    dt = {"h_sum": np.uint64, "v_sum": np.uint64, "h_mean": np.float32, "v_mean": np.float32}
    data = {f: np.asarray(cols[f], dt.get(f, np.int32)) for f in R.FIELDS}
    for k in planes:
        data[k] = np.concatenate(planes[k])
        data[k + "_off"] = np.asarray(offs[k], np.int64)
    data["image"] = np.concatenate([im.reshape(-1) for im in imgs])
    sizes = [im.size for im in imgs]
    data["image_off"] = np.asarray(np.concatenate([[0], np.cumsum(sizes[:-1])]), np.int64)
    data["image_shape"] = np.asarray([im.shape for im in imgs], np.int32)
    path = os.path.join(HERE, "quality_cimg.npz")
    np.savez_compressed(path, **data)
    print("cases", len(imgs), "scored", int((data["score"] != R.NO_SCORE).sum()), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
