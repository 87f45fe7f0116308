// test_video_segments.cpp -- the segments drop-in (GpuDctVideoIndex::gpuSegments, cbird_amd/cpp/gpu_indexes.h) compiled
// against the mock cbird headers, run on the MI355X and compared with the model by the Python test
// (tests/test_video_segments_cpp.py).
//
//   test_video_segments <file> <dir> : int32 videos, thresh, skip, pairs, tol, min frames, max segments; per video int32
//   n, then n x int32 frame and n x uint64 hash; per pair int32 source, destination (1-based = media ids).  Every video is
//   written as <dir>/<id>.vdx and loaded the way cbird does.  Prints per pair "pair k" with the summary and the match
//   range, its segments, then "frame:dst:distance:segment ..." (with maps), then the summaries of a call without maps.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gpu_indexes.h"

static void print(const cbh_vsegments& s) {
  printf("%lld %lld %d %d %d %d %d %d %d %d", (long long)s.src_frames_total, (long long)s.src_frames_aligned, s.n_src, s.n_dst,
         s.n_segments, s.n_aligned, s.monotone, s.src_in, s.dst_in, s.len);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  int32_t head[7];
  if (!f || fread(head, 4, 7, f) != 7) return 2;
  QSqlDatabase db;
  for (int32_t v = 0; v < head[0]; ++v) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    VideoIndex vi;
    vi.frames.resize(n), vi.hashes.resize(n);
    if (n && (fread(vi.frames.data(), 4, n, f) != size_t(n) || fread(vi.hashes.data(), 8, n, f) != size_t(n))) return 2;
    vi.save(QString(std::string(argv[2]) + "/%1.vdx").arg(unsigned(v + 1)));
    db.media.push_back({uint32_t(v + 1), Media::TypeVideo, 0});
  }
  std::vector<std::pair<uint32_t, uint32_t>> pairs;
  for (int32_t k = 0; k < head[3]; ++k) {
    int32_t p[2];
    if (fread(p, 4, 2, f) != 2) return 2;
    pairs.push_back({uint32_t(p[0]), uint32_t(p[1])});
  }
  fclose(f);
  GpuDctVideoIndex index;
  index.load(db, "", argv[2]);
  SearchParams params;
  params.dctThresh = head[1];
  params.skipFrames = head[2];
  params.minFramesMatched = head[5];
  std::vector<GpuDctVideoIndex::Segments> with, without;
  // min frames once by the argument and once (0) by p.minFramesMatched
  if (!index.gpuSegments(pairs, params, &with, head[4], head[5], head[6]) ||
      !index.gpuSegments(pairs, params, &without, head[4], 0, head[6], false))
    return 1;
  if (with.size() != pairs.size() || without.size() != pairs.size()) return 1;
  for (size_t k = 0; k < with.size(); ++k) {
    const MatchRange r = with[k].matchRange();
    printf("pair %zu %d %d %d ", k, r.srcIn, r.dstIn, r.len);
    print(with[k].summary);
    printf("\n");
    for (const cbh_vsegment& g : with[k].segments)
      printf("%lld:%d:%d:%d:%d:%d:%d ", (long long)g.span_sum, g.offset, g.n_frames, g.src_first, g.src_last, g.dst_first,
             g.dst_last);
    printf("\n");
    for (const cbh_vsegment_frame& m : with[k].frames) printf("%d:%d:%d:%d ", m.src_frame, m.dst_frame, m.distance, m.segment);
    printf("\n");
  }
  for (size_t k = 0; k < without.size(); ++k) {
    if (!without[k].frames.empty() || without[k].segments.size() != with[k].segments.size()) return 1;
    printf("bare %zu ", k);
    print(without[k].summary);
    printf("\n");
  }
  // an id the index does not hold, and more segments than a call may ask for: false, nothing returned
  std::vector<GpuDctVideoIndex::Segments> none(1);
  if (index.gpuSegments({{1u, 9999u}}, params, &none) || !none.empty()) return 1;
  none.resize(1);
  if (index.gpuSegments(pairs, params, &none, 15, 1, 17) || !none.empty()) return 1;
  printf("done\n");
  return 0;
}
