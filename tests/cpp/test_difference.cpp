// test_difference.cpp -- the brightnessAndContrastAuto / differenceImage drop-ins (cbird_amd/cpp/gpu_cvutil.h) compiled
// against the mock cv::Mat, run on the MI355X and compared with numbers the Python test works out with the numpy model
// (tests/test_difference_cpp.py).
//
//   test_difference <file> : int32 n, the left image, then n right images; an image is int32 w, h, channels, has_tx, six
//   doubles tx and w*h*channels bytes (cv::Mat order; the left image's has_tx / tx are ignored).  Prints per pair
//   "group i" and "single i" -- gpuDifferenceImages of all pairs at once, gpuDifferenceImage of that pair with the left
//   image as a view into a larger one -- each with w h warped sum_total sum_max n_ge32 n_ge1024 left_min left_max right_min
//   right_max and the FNV-1a hash of the picture's bytes; then "contrast" with min max and the hash of
//   gpuBrightnessAndContrastAuto(left, clip 5).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "index.h"
#include "gpu_cvutil.h"

struct Image {
  cv::Mat m;
  int32_t has_tx;
  double tx[6];
};

static bool read_image(FILE* f, Image* im) {
  int32_t d[4];
  if (fread(d, 4, 4, f) != 4 || fread(im->tx, 8, 6, f) != 6) return false;
  im->has_tx = d[3];
  im->m = cv::Mat(d[1], d[0], d[2] == 1 ? CV_8UC1 : d[2] == 3 ? CV_8UC3 : CV_8UC4);
  for (int y = 0; y < d[1]; ++y)
    if (fread(im->m.ptr<uint8_t>(y), 1, size_t(d[0]) * d[2], f) != size_t(d[0]) * d[2]) return false;
  return true;
}

static uint64_t fnv(const cv::Mat& m) {
  uint64_t h = 1469598103934665603ull;
  const size_t row = size_t(m.cols) * size_t(m.channels());
  for (int y = 0; y < m.rows; ++y)
    for (size_t x = 0; x < row; ++x) h = (h ^ m.ptr<uint8_t>(y)[x]) * 1099511628211ull;
  return h;
}

static void print(const char* what, size_t i, const cv::Mat& pic, const cbh_diff_detail& d) {
  printf("%s %zu %d %d %d %" PRIu64 " %u %u %u %d %d %d %d %" PRIu64 "\n", what, i, d.w, d.h, d.warped, d.sum_total, d.sum_max,
         d.n_ge32, d.n_ge1024, d.left_min, d.left_max, d.right_min, d.right_max, fnv(pic));
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  int32_t n = 0;
  Image left;
  if (!f || fread(&n, 4, 1, f) != 1 || !read_image(f, &left)) return 2;
  std::vector<Image> rights;
  rights.resize(size_t(n));
  for (Image& r : rights)
    if (!read_image(f, &r)) return 2;
  fclose(f);
  std::vector<cv::Mat> mats, pics(2);  // (pics: replaced, not appended to)
  std::vector<cbh_template_result> res(rights.size(), cbh_template_result());
  for (size_t i = 0; i < rights.size(); ++i) {
    mats.push_back(rights[i].m);
    res[i].tx_found = rights[i].has_tx;
    memcpy(res[i].tx, rights[i].tx, sizeof res[i].tx);
  }
  std::vector<cbh_diff_detail> det;
  cbird_gpu::gpuDifferenceImages(left.m, mats, res.data(), pics, det);
  if (pics.size() != rights.size() || det.size() != rights.size()) return 3;
  for (size_t i = 0; i < rights.size(); ++i) {
    if (pics[i].type() != CV_8UC4 || pics[i].cols != det[i].w || pics[i].rows != det[i].h) return 3;
    print("group", i, pics[i], det[i]);
  }
  // the left image as a view: its rows are read where they lie
  cv::Mat big(left.m.rows + 5, left.m.cols + 9, left.m.type());
  memset(big.data, 0x3c, size_t(big.rows) * big.step);
  cv::Mat view = big.colRange(4, 4 + left.m.cols).rowRange(2, 2 + left.m.rows);
  const size_t row = size_t(left.m.cols) * size_t(left.m.channels());
  for (int y = 0; y < left.m.rows; ++y) memcpy(view.ptr<uint8_t>(y), left.m.ptr<uint8_t>(y), row);
  for (size_t i = 0; i < rights.size(); ++i) {
    cbh_diff_detail d;
    const cv::Mat pic = cbird_gpu::gpuDifferenceImage(view, rights[i].m, rights[i].has_tx ? rights[i].tx : nullptr, &d);
    print("single", i, pic, d);
  }
  cv::Mat stretched;
  int lo = -5, hi = -5;
  cbird_gpu::gpuBrightnessAndContrastAuto(view, stretched, 5, &lo, &hi);
  if (stretched.rows != left.m.rows || stretched.cols != left.m.cols || stretched.type() != left.m.type()) return 3;
  printf("contrast %d %d %" PRIu64 "\n", lo, hi, fnv(stretched));
  cbird_gpu::gpuDifferenceImages(left.m, std::vector<cv::Mat>(), nullptr, pics, det);
  return pics.empty() && det.empty() ? 0 : 3;
}
