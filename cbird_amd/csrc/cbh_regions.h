// cbh_regions.h -- internal: which images of a chunk share a launch once autocrop has given each its kept region, and
// where each resized kept region lands in the chunk's packed buffer.  The callers that hash autocropped images
// (cbh_process_images_ex, cbh_index_images, the video indexer) take their launch plan from here.
// Plain C++ with no HIP in it: a host compiler builds it alone (tests/cpp/regions.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <array>
#include <map>
#include <vector>

namespace cbh {

// rects: m x {left, top, right, bottom}, as cbh_autocrop_dev writes them
inline bool same_rect(const int* a, const int* b) { return !memcmp(a, b, 4 * sizeof(int)); }

// without autocrop every image keeps its whole frame
inline void fill_whole(int* rects, size_t m, int w, int h) {
  for (size_t i = 0; i < m; ++i) rects[i * 4] = rects[i * 4 + 1] = 0, rects[i * 4 + 2] = w, rects[i * 4 + 3] = h;
}

// images first .. first + count of the chunk, launched together on the kept region `rect`
struct RegionRun {
  size_t first, count;
  int rect[4];
};

// the maximal runs of equal rectangles, in order (the frames of one letterboxed video all share theirs)
inline void region_runs(const int* rects, size_t m, std::vector<RegionRun>* out) {
  out->clear();
  for (size_t i = 0, run = 1; i < m; i += run) {
    const int* r = rects + i * 4;
    run = 1;
    while (i + run < m && same_rect(r, rects + (i + run) * 4)) ++run;
    out->push_back(RegionRun{i, run, {r[0], r[1], r[2], r[3]}});
  }
}

// Launch plan for the per-geometry stages (hash, resize).  Runs of equal kept regions take one launch each; with
// mode_first, when a few odd regions are scattered among images that share one region (photos: almost all keep the
// whole frame), it is cheaper to run that region over the WHOLE chunk once and redo the odd images one by one: the plan
// is then {0, m, mode} followed by every other image as a run of one, whose results replace the chunk-wide pass's.
// The mode is the most frequent rectangle, of several the lexicographically smallest.
inline void plan_regions(const int* rects, size_t m, bool mode_first, std::vector<RegionRun>* out) {
  region_runs(rects, m, out);
  if (!mode_first || m == 0) return;
  std::map<std::array<int, 4>, size_t> freq;
  for (size_t i = 0; i < m; ++i) ++freq[{rects[i * 4], rects[i * 4 + 1], rects[i * 4 + 2], rects[i * 4 + 3]}];
  int mode[4] = {0, 0, 0, 0};
  size_t best = 0;
  for (const auto& kv : freq)
    if (kv.second > best) best = kv.second, memcpy(mode, kv.first.data(), sizeof mode);
  const size_t n_odd = m - best;
  if (!(1 + n_odd < out->size())) return;
  out->assign(1, RegionRun{0, m, {mode[0], mode[1], mode[2], mode[3]}});
  for (size_t i = 0; i < m; ++i) {
    const int* r = rects + i * 4;
    if (!same_rect(r, mode)) out->push_back(RegionRun{i, 1, {r[0], r[1], r[2], r[3]}});
  }
}

// sizeLongestSide's destination size (src/cvutil.cpp:1934-1942): float aspect, truncation
inline void longest_side_dims(int w, int h, int size, int* out_w, int* out_h) {
  const float aspect = (float)w / (float)h;
  if (w > h) {
    *out_w = size;
    *out_h = (int)((float)size / aspect);
  } else {
    *out_h = size;
    *out_w = (int)(aspect * (float)size);
  }
}

// ... of a kept region; false and 0 x 0 where the reference throws ("computed width or height is 0"): no image
inline bool kept_region_dims(const int* rect, int size, int* dw, int* dh) {
  longest_side_dims(rect[2] - rect[0], rect[3] - rect[1], size, dw, dh);
  if (*dw <= 0 || *dh <= 0 || *dw > size || *dh > size) *dw = *dh = 0;
  return *dw != 0;
}

// The resized images of a chunk packed back to back in plan order (ORB and the keypoint hashes take per-image offsets):
// every run starts on a multiple of 16 bytes, image t of a run sits at its base + t * dw * dh, a rejected run takes no
// room, and a later entry of the plan for an image (mode-first's odd images) overrides its slot from the chunk-wide
// pass.  ws / hs / off: per image; base: per plan entry.  Returns the bytes used, at most 2 * m * (size * size + 16).
inline size_t pack_resized(const std::vector<RegionRun>& plan, int size, uint32_t* ws, uint32_t* hs, uint64_t* off,
                           std::vector<size_t>* base) {
  size_t cur = 0;
  base->clear();
  for (const RegionRun& r : plan) {
    int dw, dh;
    kept_region_dims(r.rect, size, &dw, &dh);
    cur = (cur + 15) & ~(size_t)15;
    base->push_back(cur);
    for (size_t t = 0; t < r.count; ++t) {
      ws[r.first + t] = (uint32_t)dw, hs[r.first + t] = (uint32_t)dh;
      off[r.first + t] = cur + t * (size_t)dw * dh;
    }
    cur += r.count * (size_t)dw * dh;
  }
  return cur;
}

}  // namespace cbh
