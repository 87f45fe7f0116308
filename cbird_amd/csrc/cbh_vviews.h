// cbh_vviews.h -- internal, host only and free of HIP: what cbh_video_coverage (vcoverage.hip) and cbh_video_segments
// (vsegments.hip) share before anything is launched -- the two views of every video a call names -- and the range and
// budget arithmetic of the segments' difference arrays.  Plain C++ over the caller's arrays, so that a small program with
// its own main can run it under a host sanitizer.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "cbird_hip.h"

namespace cbh {

// the views of one video for this call's skip: which of its stored frames are searched, which are entries
struct VideoView {
  uint32_t s_begin = 0, s_n = 0, d_begin = 0, d_n = 0;
};
struct VideoViews {
  std::vector<VideoView> views;  // one per video of the table; empty ranges for a video no pair names
  std::vector<uint64_t> sh, dh;  // source views: hash, frame, span; destination views: hash, frame
  std::vector<int32_t> sf, ss, df;
};

constexpr uint32_t kMostVideoEntries = 1u << 24;  // MAX_FRAMES_PER_VIDEO of the reference

// The source view of every video with as_src set and the destination view of every one with as_dst set (the rules are in
// include/cbird_hip.h at cbh_video_coverage).  rising: refuse a used video whose frame numbers fall.  CBH_OK, or a code
// with *why = "<what>: <reason>".
inline int build_video_views(const char* what, const int32_t* frames, const uint64_t* hashes, const uint64_t* voff,
                             size_t n_videos, const std::vector<uint8_t>& as_src, const std::vector<uint8_t>& as_dst,
                             int skip, bool rising, VideoViews* out, std::string* why) {
  auto fail = [&](int rc, const char* reason) {
    *why = std::string(what) + ": " + reason;
    return rc;
  };
  VideoViews& w = *out;
  w.views.assign(n_videos, VideoView());
  {
    size_t most_s = 0, most_d = 0;  // room for every frame, so that the views below never move
    for (size_t v = 0; v < n_videos; ++v) {
      if (voff[v + 1] < voff[v]) return fail(CBH_E_INVAL, "video_offsets fall");
      if (as_src[v]) most_s += (size_t)(voff[v + 1] - voff[v]);
      if (as_dst[v]) most_d += (size_t)(voff[v + 1] - voff[v]);
    }
    w.sh.reserve(most_s), w.sf.reserve(most_s), w.ss.reserve(most_s), w.dh.reserve(most_d), w.df.reserve(most_d);
  }
  for (size_t v = 0; v < n_videos; ++v) {
    const size_t b = (size_t)voff[v], n = (size_t)(voff[v + 1] - voff[v]);
    if (n == 0 || !(as_src[v] | as_dst[v])) continue;
    if (n > kMostVideoEntries) return fail(CBH_E_UNSUPPORTED, "a video with more than 2^24 stored frames");
    if (rising)
      for (size_t i = 1; i < n; ++i)
        if (frames[b + i] < frames[b + i - 1]) return fail(CBH_E_INVAL, "the frame numbers of a video fall");
    const long long last = frames[b + n - 1];
    VideoView& x = w.views[v];
    if (as_src[v]) {  // findVideo's needle frames (:431): the trim is unconditional
      x.s_begin = (uint32_t)w.sh.size();
      for (size_t i = 0; i < n; ++i) {
        const long long f = frames[b + i];
        if (f < skip || f > last - skip) continue;
        w.sh.push_back(hashes[b + i]);
        w.sf.push_back((int32_t)f);
        w.ss.push_back(i + 1 < n ? (int32_t)((long long)frames[b + i + 1] - f) : 1);
      }
      x.s_n = (uint32_t)(w.sh.size() - x.s_begin);
    }
    if (as_dst[v]) {  // insertHashes (:61-111): the detail rule, and the trim only on a video long enough for it
      x.d_begin = (uint32_t)w.dh.size();
      const bool trim = skip && last / 2 > skip;
      for (size_t i = 0; i < n; ++i) {
        const int pc = __builtin_popcountll(hashes[b + i]);
        if (pc < 5 || 64 - pc < 5) continue;
        const long long f = frames[b + i];
        if (trim && (f < skip || f > last - skip)) continue;
        w.dh.push_back(hashes[b + i]);
        w.df.push_back((int32_t)f);
      }
      x.d_n = (uint32_t)(w.dh.size() - x.d_begin);
    }
    if (w.sh.size() >= 0xffffffffull || w.dh.size() >= 0xffffffffull)
      return fail(CBH_E_UNSUPPORTED, "the videos of one call hold 2^32 frames or more");
  }
  return CBH_OK;
}

// ---- the segments' difference arrays ------------------------------------------------------------------------------------
// The offsets of one pair are [omin, omin + n_off): from the lowest destination frame minus the highest source frame minus
// tol to the highest destination frame minus the lowest source frame plus tol.  The difference array has one word more
// (the -1 one past the last offset), rounded up to 4 words.
struct VsegRange {
  int32_t omin = 0;
  uint32_t n_off = 0;  // 0: a pair without considered frames or without entries; it has no array
  uint64_t words = 0;
};
constexpr uint64_t kMostVsegWords = 1ull << 30;

// CBH_OK; CBH_E_UNSUPPORTED when an offset does not fit 32 bits; CBH_E_NOMEM when the array alone is above the budget
inline int vseg_range(long long fs_min, long long fs_max, long long fd_min, long long fd_max, long long tol,
                      uint64_t budget_bytes, VsegRange* r) {
  const long long omin = fd_min - fs_max - tol, omax = fd_max - fs_min + tol;  // |each term| <= 2^31: no overflow
  if (omin < INT32_MIN || omax > INT32_MAX) return CBH_E_UNSUPPORTED;
  const uint64_t n_off = (uint64_t)(omax - omin) + 1, words = (n_off + 1 + 3) & ~3ull;
  if (words > kMostVsegWords || words * 4 > budget_bytes) return CBH_E_NOMEM;
  r->omin = (int32_t)omin, r->n_off = (uint32_t)n_off, r->words = words;
  return CBH_OK;
}

// Pairs in order, cut into groups whose arrays fit the budget together: the first pair of every group and, last, the
// number of pairs.  Every single array fits (vseg_range).
inline std::vector<size_t> vseg_groups(const std::vector<VsegRange>& ranges, uint64_t budget_bytes) {
  std::vector<size_t> first(1, 0);
  uint64_t used = 0;
  for (size_t k = 0; k < ranges.size(); ++k) {
    const uint64_t b = ranges[k].words * 4;
    if (used + b > budget_bytes && used) first.push_back(k), used = 0;
    used += b;
  }
  first.push_back(ranges.size());
  return first;
}

}  // namespace cbh
