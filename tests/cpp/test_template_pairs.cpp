// test_template_pairs.cpp -- the drop-in gpuTemplateMatchPairs (cbird_amd/cpp/gpu_cvutil.h) compiled against the mock
// cv::Mat, run on the MI355X and compared with numbers the Python test passes in (tests/test_template_pairs_cpp.py: the
// model of tests/template_pairs_rules.py).
//
//   test_template_pairs <file> : the file holds ORB's 1024 pattern bytes, int32 channels, int32 n_imgs, per image int32
//   w, h and w*h*channels bytes, int32 n_pairs, then per pair int32 template, candidate.
//   Prints one line per pair: status w h n_keypoints n_matches found score cand_hash tmpl_hash roi[0..8].
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "index.h"
#include "gpu_cvutil.h"

struct TmParams {  // the fields of SearchParams the template matcher reads, at the reference's defaults
  int needleFeatures = 100, haystackFeatures = 1000, cvThresh = 25, tmScalePct = 200;
};

static cv::Mat read_image(FILE* f, int w, int h, int cn) {
  cv::Mat m(h, w, cn == 1 ? CV_8UC1 : cn == 3 ? CV_8UC3 : CV_8UC4);
  for (int y = 0; y < h; ++y)
    if (fread(m.ptr<uint8_t>(y), 1, size_t(w) * cn, f) != size_t(w) * cn) exit(2);
  return m;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  int8_t pattern[1024];
  int32_t cn = 0, n_imgs = 0, n_pairs = 0;
  if (!f || fread(pattern, 1, 1024, f) != 1024 || fread(&cn, 4, 1, f) != 1 || fread(&n_imgs, 4, 1, f) != 1) return 2;
  if (cbh_orb_set_pattern(pattern) != CBH_OK) return 2;
  std::vector<cv::Mat> images;
  for (int i = 0; i < n_imgs; ++i) {
    int32_t d[2];
    if (fread(d, 4, 2, f) != 2) return 2;
    images.push_back(read_image(f, d[0], d[1], cn));
  }
  if (fread(&n_pairs, 4, 1, f) != 1) return 2;
  std::vector<std::pair<int, int>> pairs;
  for (int p = 0; p < n_pairs; ++p) {
    int32_t d[2];
    if (fread(d, 4, 2, f) != 2) return 2;
    pairs.push_back({d[0], d[1]});
  }
  fclose(f);
  std::vector<cbh_tm_image_result> res(2);  // replaced, not appended to
  cbird_gpu::gpuTemplateMatchPairs(images, pairs, TmParams(), res);
  if (res.size() != size_t(n_pairs)) return 3;
  for (const cbh_tm_image_result& r : res) {
    printf("%d %d %d %u %u %d %d %" PRIu64 " %" PRIu64, r.status, r.w, r.h, r.n_keypoints, r.n_matches, r.r.found, r.r.score,
           r.r.cand_hash, r.r.tmpl_hash);
    for (int k = 0; k < 8; ++k) printf(" %d", r.r.roi[k]);
    printf("\n");
  }
  cbird_gpu::gpuTemplateMatchPairs(images, std::vector<std::pair<int, int>>(), TmParams(), res);
  return res.empty() ? 0 : 3;
}
