// test_alignment.cpp -- the alignSpatially / alignTemporally drop-ins (cbird_amd/cpp/gpu_cvutil.h) compiled against the
// mock cv::Mat, run on the MI355X and compared with numbers the Python test works out with the numpy model
// (tests/test_alignment_cpp.py).
//
//   test_alignment <file> : int32 n, the left image, n right images, then int32 nl, nw, start, nl left frames and nw
//   right frames; an image is int32 w, h, channels and w*h*channels bytes (cv::Mat order).  Prints per pair "group i" --
//   gpuAlignSpatial of all pairs at once -- and "single i" -- the one-pair overload with the left image as a view into a
//   larger one -- each with min_x min_y min_sad sad_at_zero, the single ones also alignX * 256 and alignY * 256; then
//   "clip" with placement offset min_mean start_mean of gpuAlignTemporal, and "clip_default" for start = -1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "index.h"
#include "gpu_cvutil.h"

static bool read_image(FILE* f, cv::Mat* m) {
  int32_t d[3];
  if (fread(d, 4, 3, f) != 3) return false;
  *m = cv::Mat(d[1], d[0], d[2] == 1 ? CV_8UC1 : d[2] == 3 ? CV_8UC3 : CV_8UC4);
  for (int y = 0; y < d[1]; ++y)
    if (fread(m->ptr<uint8_t>(y), 1, size_t(d[0]) * d[2], f) != size_t(d[0]) * d[2]) return false;
  return true;
}

static void print(const char* what, size_t i, const cbh_align_spatial_result& r) {
  printf("%s %zu %d %d %u %u", what, i, r.min_x, r.min_y, r.min_sad, r.sad_at_zero);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  int32_t n = 0, clip[3] = {0, 0, 0};
  cv::Mat left;
  if (!f || fread(&n, 4, 1, f) != 1 || !read_image(f, &left)) return 2;
  std::vector<cv::Mat> rights, lf, rf;
  rights.resize(size_t(n));
  for (cv::Mat& r : rights)
    if (!read_image(f, &r)) return 2;
  if (fread(clip, 4, 3, f) != 3) return 2;
  lf.resize(size_t(clip[0])), rf.resize(size_t(clip[1]));
  for (cv::Mat& m : lf)
    if (!read_image(f, &m)) return 2;
  for (cv::Mat& m : rf)
    if (!read_image(f, &m)) return 2;
  fclose(f);
  std::vector<cbh_align_spatial_result> out(1);  // (replaced, not appended to)
  cbird_gpu::gpuAlignSpatial(left, rights, out);
  if (out.size() != rights.size()) return 3;
  for (size_t i = 0; i < out.size(); ++i) {
    print("group", i, out[i]);
    printf("\n");
  }
  // the left image as a view: its rows are read where they lie
  cv::Mat big(left.rows + 5, left.cols + 9, left.type());
  memset(big.data, 0x3c, size_t(big.rows) * big.step);
  cv::Mat view = big.colRange(4, 4 + left.cols).rowRange(2, 2 + left.rows);
  const size_t row = size_t(left.cols) * size_t(left.channels());
  for (int y = 0; y < left.rows; ++y) memcpy(view.ptr<uint8_t>(y), left.ptr<uint8_t>(y), row);
  for (size_t i = 0; i < rights.size(); ++i) {
    float ax = -1, ay = -1;
    const cbh_align_spatial_result r = cbird_gpu::gpuAlignSpatial(view, rights[i], &ax, &ay);
    print("single", i, r);
    printf(" %.9g %.9g\n", double(ax) * 256.0, double(ay) * 256.0);
  }
  cbh_align_temporal_result t = cbird_gpu::gpuAlignTemporal(lf, rf, clip[2]);
  printf("clip %d %d %u %u\n", t.placement, t.offset, t.min_mean, t.start_mean);
  t = cbird_gpu::gpuAlignTemporal(lf, rf);
  printf("clip_default %d %d %u %u\n", t.placement, t.offset, t.min_mean, t.start_mean);
  cbird_gpu::gpuAlignSpatial(left, std::vector<cv::Mat>(), out);
  return out.empty() ? 0 : 3;
}
