// cbh_runs.h -- internal: the shape rules the host-memory entry points share, and the bounded-span upload rule.
// Plain C++ with no HIP in it: a host compiler builds it alone (tests/cpp/staging_runs.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace cbh {

inline bool channels_ok(int c) { return c == 1 || c == 3 || c == 4; }

// one past the last byte of an image that starts at `off`
inline uint64_t image_end(uint64_t off, uint32_t w, uint32_t h, uint32_t stride, int channels) {
  return off + (uint64_t)(h - 1) * stride + (uint64_t)w * channels;
}

// the template-match chain's images: remap addresses its source with shorts
inline bool image_ok(uint32_t w, uint32_t h, uint32_t stride, int channels) {
  return w >= 1 && h >= 1 && w <= 32767 && h <= 32767 && stride >= w * (uint32_t)channels;
}

// Images i0 .. i0 + m of a batch, whose bytes lie in [lo, hi): what one upload takes.
struct Run {
  size_t i0, m;
  uint64_t lo, hi;
};

// The batch cut into runs, in order: a run starts with one image and takes the next one while it has fewer than max_m
// and the bytes from its lowest offset to its highest end still span at most `budget` (the offsets need not ascend).
// An image larger than the budget is a run of its own.
inline std::vector<Run> make_runs(size_t n, const uint64_t* off, const uint64_t* end, uint64_t budget, size_t max_m) {
  std::vector<Run> runs;
  for (size_t i0 = 0; i0 < n;) {
    Run r{i0, 1, off[i0], end[i0]};
    while (r.i0 + r.m < n && r.m < max_m) {
      const size_t j = r.i0 + r.m;
      const uint64_t lo = std::min(r.lo, off[j]), hi = std::max(r.hi, end[j]);
      if (hi - lo > budget) break;
      r.lo = lo, r.hi = hi, ++r.m;
    }
    runs.push_back(r);
    i0 += r.m;
  }
  return runs;
}

// the run's offsets counted from its first uploaded byte
inline void rebase(const Run& r, const uint64_t* off, std::vector<uint64_t>* rel) {
  rel->resize(r.m);
  for (size_t i = 0; i < r.m; ++i) (*rel)[i] = off[r.i0 + i] - r.lo;
}

}  // namespace cbh
