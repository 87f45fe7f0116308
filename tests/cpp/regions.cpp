// The host-only launch plan and resize packing of cbird_amd/csrc/cbh_regions.h, printed for tests/test_regions.py.  Host
// code only: includes nothing else of the library and links nothing.
// In (stdin), one command per line; rectangles are given as M followed by M x "l t r b".  Out, one line per command:
//   whole M W H              -> l t r b ...                                     fill_whole
//   runs M rects             -> n | first count l t r b | ...                   region_runs
//   plan MODE_FIRST M rects  -> n | first count l t r b | ...                   plan_regions
//   dims W H SIZE            -> dw dh                                           longest_side_dims
//   kept l t r b SIZE        -> ok dw dh                                        kept_region_dims (the reject rule)
//   pack MODE_FIRST SIZE M rects -> bytes | base ... | ws hs off ...            plan_regions, then pack_resized
#include <cstdio>
#include <cstring>

#include "cbh_regions.h"

using namespace cbh;

static bool read_rects(std::vector<int>* rects, size_t* m) {
  if (scanf("%zu", m) != 1) return false;
  rects->resize(*m * 4 + 1);  // (+ 1: data() of an empty batch is still a pointer)
  for (size_t i = 0; i < *m * 4; ++i)
    if (scanf("%d", &(*rects)[i]) != 1) return false;
  return true;
}

static void print_runs(const std::vector<RegionRun>& runs) {
  printf("%zu", runs.size());
  for (const RegionRun& r : runs) printf(" | %zu %zu %d %d %d %d", r.first, r.count, r.rect[0], r.rect[1], r.rect[2], r.rect[3]);
  printf("\n");
}

int main() {
  char cmd[16];
  std::vector<int> rects;
  std::vector<RegionRun> runs;
  size_t m;
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "whole")) {
      int w, h;
      if (scanf("%zu %d %d", &m, &w, &h) != 3) return 2;
      rects.assign(m * 4 + 1, -1);
      fill_whole(rects.data(), m, w, h);
      for (size_t i = 0; i < m * 4; ++i) printf("%s%d", i ? " " : "", rects[i]);
      printf("\n");
    } else if (!strcmp(cmd, "runs")) {
      if (!read_rects(&rects, &m)) return 2;
      region_runs(rects.data(), m, &runs);
      print_runs(runs);
    } else if (!strcmp(cmd, "plan")) {
      int mode_first;
      if (scanf("%d", &mode_first) != 1 || !read_rects(&rects, &m)) return 2;
      plan_regions(rects.data(), m, mode_first != 0, &runs);
      print_runs(runs);
    } else if (!strcmp(cmd, "dims")) {
      int w, h, size, dw = -1, dh = -1;
      if (scanf("%d %d %d", &w, &h, &size) != 3) return 2;
      longest_side_dims(w, h, size, &dw, &dh);
      printf("%d %d\n", dw, dh);
    } else if (!strcmp(cmd, "kept")) {
      int r[4], size, dw = -1, dh = -1;
      if (scanf("%d %d %d %d %d", &r[0], &r[1], &r[2], &r[3], &size) != 5) return 2;
      const bool ok = kept_region_dims(r, size, &dw, &dh);
      printf("%d %d %d\n", ok ? 1 : 0, dw, dh);
    } else if (!strcmp(cmd, "pack")) {
      int mode_first, size;
      if (scanf("%d %d", &mode_first, &size) != 2 || !read_rects(&rects, &m)) return 2;
      plan_regions(rects.data(), m, mode_first != 0, &runs);
      // exactly m entries on the heap: the sanitizer build sees a write past an image's slot
      std::vector<uint32_t> ws(m), hs(m);
      std::vector<uint64_t> off(m);
      std::vector<size_t> base;
      const size_t bytes = pack_resized(runs, size, ws.data(), hs.data(), off.data(), &base);
      if (base.size() != runs.size()) return 3;
      printf("%zu |", bytes);
      for (size_t b : base) printf(" %zu", b);
      printf(" |");
      for (size_t i = 0; i < m; ++i) printf(" %u %u %llu", ws[i], hs[i], (unsigned long long)off[i]);
      printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
