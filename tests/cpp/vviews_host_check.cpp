// vviews_host_check.cpp -- a stand-alone host program over cbird_amd/csrc/cbh_vviews.h: the two views of a video and the
// range, budget and grouping arithmetic of the segments' difference arrays, on hand-made inputs and at the edges of 32
// bits.  tests/test_video_segments_host.py builds it with -fsanitize=address,undefined and runs it (no GPU, no HIP).
#include <cstdio>
#include <cstdlib>

#include "cbh_vviews.h"

#define CHECK(x)                                             \
  do {                                                       \
    if (!(x)) {                                              \
      printf("%s:%d: %s\n", __FILE__, __LINE__, #x);         \
      return 1;                                              \
    }                                                        \
  } while (0)

int main() {
  using namespace cbh;
  const uint64_t B = 0x0123456789ABCDEFull, MB = 1ull << 20;
  // video 0: five frames 0..40; video 1: empty; video 2: low-detail hashes; video 3: frames that fall; video 4: unused
  const int32_t frames[] = {0, 10, 20, 30, 40, 0, 1, 5, 4, 6, 7};
  const uint64_t hashes[] = {B, B, B, B, B, 0xF, ~0xFull, B, B, B, B};
  const uint64_t voff[] = {0, 5, 5, 7, 10, 11};
  std::vector<uint8_t> as_src = {1, 1, 1, 0, 0}, as_dst = {1, 1, 1, 0, 0};
  VideoViews v;
  std::string why;
  CHECK(build_video_views("check", frames, hashes, voff, 5, as_src, as_dst, 20, true, &v, &why) == CBH_OK);
  CHECK(v.views[0].s_n == 1 && v.sf[v.views[0].s_begin] == 20 && v.ss[v.views[0].s_begin] == 10);  // the source trim
  CHECK(v.views[0].d_n == 5);  // 40 / 2 is not above 20
  CHECK(v.views[1].s_n == 0 && v.views[1].d_n == 0);
  CHECK(v.views[2].s_n == 0 && v.views[2].d_n == 0);  // trimmed to nothing; no entry passes the detail rule
  CHECK(v.views[3].s_n == 0 && v.views[4].d_n == 0);
  CHECK(build_video_views("check", frames, hashes, voff, 5, as_src, as_dst, 0, true, &v, &why) == CBH_OK);
  CHECK(v.views[0].s_n == 5 && v.views[2].s_n == 2 && v.views[2].d_n == 0 && v.ss[v.views[0].s_begin + 4] == 1);
  as_src[3] = 1;  // the falling video is named now
  CHECK(build_video_views("check", frames, hashes, voff, 5, as_src, as_dst, 0, true, &v, &why) == CBH_E_INVAL);
  CHECK(why == "check: the frame numbers of a video fall");
  CHECK(build_video_views("check", frames, hashes, voff, 5, as_src, as_dst, 0, false, &v, &why) == CBH_OK);  // coverage takes it
  const uint64_t falling[] = {0, 5, 4, 7, 10, 11};
  CHECK(build_video_views("check", frames, hashes, falling, 5, as_src, as_dst, 0, true, &v, &why) == CBH_E_INVAL);

  VsegRange r;
  CHECK(vseg_range(0, 90, 0, 90, 2, 256 * MB, &r) == CBH_OK && r.omin == -92 && r.n_off == 185 && r.words == 188);
  CHECK(vseg_range(7, 7, 7, 7, 0, 256 * MB, &r) == CBH_OK && r.omin == 0 && r.n_off == 1 && r.words == 4);
  CHECK(vseg_range(0, 0, 0, 0, 1, 16, &r) == CBH_OK && r.n_off == 3 && r.words == 4);  // 16 bytes hold it exactly
  CHECK(vseg_range(0, 0, 0, 0, 2, 16, &r) == CBH_E_NOMEM);  // 5 offsets + 1 round up to 8 words
  CHECK(vseg_range(0, 100000, 0, 100000, 15, 1 * MB, &r) == CBH_OK);  // 200 031 offsets: 800 128 bytes
  CHECK(vseg_range(0, 200000, 0, 200000, 15, 1 * MB, &r) == CBH_E_NOMEM);
  CHECK(vseg_range(0, 0, 0, 0, INT32_MAX, 4096 * MB, &r) == CBH_E_NOMEM);  // 2^32 - 1 offsets
  CHECK(vseg_range(0, 0, 0, 0, (1ll << 29) - 2, 4096 * MB, &r) == CBH_OK && r.words == kMostVsegWords);
  CHECK(vseg_range(0, 0, 0, 0, (1ll << 29), 4096 * MB, &r) == CBH_E_NOMEM);
  // the extremes of int32 frame numbers: the offsets leave 32 bits before they leave the budget
  CHECK(vseg_range(INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, 0, 4096 * MB, &r) == CBH_E_UNSUPPORTED);
  CHECK(vseg_range(INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX, INT32_MAX, 4096 * MB, &r) == CBH_E_UNSUPPORTED);
  CHECK(vseg_range(INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, 0, 4096 * MB, &r) == CBH_E_UNSUPPORTED);
  CHECK(vseg_range(INT32_MAX - 5, INT32_MAX, INT32_MAX - 5, INT32_MAX, 3, 4096 * MB, &r) == CBH_OK && r.omin == -8 &&
        r.n_off == 17);
  CHECK(vseg_range(0, 1, INT32_MAX - 1, INT32_MAX, 0, 4096 * MB, &r) == CBH_OK && r.omin == INT32_MAX - 2 && r.n_off == 3);

  std::vector<VsegRange> ranges(6);
  const uint64_t words[] = {100, 0, 100, 56, 200, 4};  // in bytes 400, 0, 400, 224, 800, 16 against a budget of 800
  for (int k = 0; k < 6; ++k) ranges[k].words = words[k];
  const std::vector<size_t> g = vseg_groups(ranges, 800);
  CHECK((g == std::vector<size_t>{0, 3, 4, 5, 6}));  // {400, 0, 400}, {224}, {800}, {16}
  CHECK((vseg_groups({}, 800) == std::vector<size_t>{0, 0}));
  CHECK((vseg_groups(ranges, 4096) == std::vector<size_t>{0, 6}));
  for (size_t k = 0; k + 1 < g.size(); ++k) {  // no group is above the budget
    uint64_t bytes = 0;
    for (size_t i = g[k]; i < g[k + 1]; ++i) bytes += ranges[i].words * 4;
    CHECK(bytes <= 800 && g[k] < g[k + 1]);
  }
  printf("ok\n");
  return 0;
}
