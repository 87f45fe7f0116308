// test_template_match.cpp -- the drop-in gpuTemplateMatch (cbird_amd/cpp/gpu_cvutil.h) compiled against the mock cv::Mat,
// run on the MI355X and compared with numbers the Python test passes in (tests/test_template_match_cpp.py: the numpy model).
//
//   test_template_match <file> : the file holds int32 tw, th, tc and the template's bytes, int32 n, then per candidate
//   int32 w, h, channels, k, float candScale, w*h*channels bytes, k template points and k match points (x, y floats).
//   Prints one line per candidate: found score tx_found iterations good_count cand_hash tmpl_hash roi[0..8].
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "index.h"
#include "gpu_cvutil.h"

static cv::Mat read_image(FILE* f, int w, int h, int cn) {
  cv::Mat m(h, w, cn == 1 ? CV_8UC1 : cn == 3 ? CV_8UC3 : CV_8UC4);
  for (int y = 0; y < h; ++y)
    if (fread(m.ptr<uint8_t>(y), 1, size_t(w) * cn, f) != size_t(w) * cn) exit(2);
  return m;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  int32_t t[3], n = 0;
  if (!f || fread(t, 4, 3, f) != 3) return 2;
  const cv::Mat tmpl = read_image(f, t[0], t[1], t[2]);
  if (fread(&n, 4, 1, f) != 1) return 2;
  std::vector<cv::Mat> cands;
  std::vector<std::vector<cv::Point2f>> tp(n), mp(n);
  std::vector<float> scales(n);
  for (int i = 0; i < n; ++i) {
    int32_t d[4];
    if (fread(d, 4, 4, f) != 4 || fread(&scales[i], 4, 1, f) != 1) return 2;
    cands.push_back(read_image(f, d[0], d[1], d[2]));
    tp[i].resize(d[3]), mp[i].resize(d[3]);
    if (d[3] && (fread(tp[i].data(), 8, d[3], f) != size_t(d[3]) || fread(mp[i].data(), 8, d[3], f) != size_t(d[3]))) return 2;
  }
  fclose(f);
  std::vector<cbh_template_result> res(2);  // replaced, not appended to
  cbird_gpu::gpuTemplateMatch(tmpl, cands, tp, mp, scales, res);
  if (res.size() != size_t(n)) return 3;
  for (const cbh_template_result& r : res) {
    printf("%d %d %d %d %d %" PRIu64 " %" PRIu64, r.found, r.score, r.tx_found, r.iterations, r.good_count, r.cand_hash,
           r.tmpl_hash);
    for (int k = 0; k < 8; ++k) printf(" %d", r.roi[k]);
    printf("\n");
  }
  cbird_gpu::gpuTemplateMatch(tmpl, std::vector<cv::Mat>(), {}, {}, {}, res);
  return res.empty() ? 0 : 3;
}
