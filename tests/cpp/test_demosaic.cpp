// test_demosaic.cpp -- the demosaicHough drop-ins (cbird_amd/cpp/gpu_cvutil.h) compiled against the mock cv::Mat, run on
// the MI355X and compared with rectangles the Python test works out with the numpy model (tests/test_demosaic_cpp.py).
//
//   test_demosaic <file> : int32 n, then n images; an image is int32 w, h, channels and w*h*channels bytes (cv::Mat
//   order).  Prints "batch i x y w h" per rectangle of gpuDemosaicHough on all sheets at once, then "single i x y w h"
//   from the one-sheet overload with the sheet as a view into a larger image, then "tight 0 x y w h" for the first sheet
//   with houghThreshFactor 0.99.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "index.h"

// what cbird's qrect.h and cvutil.h (:183-201) give the drop-in
struct QRect {
  int x_, y_, w_, h_;
  QRect(int x, int y, int w, int h) : x_(x), y_(y), w_(w), h_(h) {}
  int x() const { return x_; }
  int y() const { return y_; }
  int width() const { return w_; }
  int height() const { return h_; }
};
struct DemosaicParams {
  int clipHistogramPercent = 10;
  float borderThresh = 19.0;
  int preBlurKernel = 3;
  int cannyThresh1 = 50;
  int cannyThresh2 = 0;
  int postBlurKernel = 3;
  int hMargin = 0;
  int vMargin = 0;
  float houghRho = 0.5;
  float houghTheta = 45;
  float houghThreshFactor = 0.8;
  int minGridSpacing = 96;
  int gridTolerance = 4;
  int cropMargin = 2;
  float maxAspectRatio = 2.5;
  float minAspectRatio = 0.5;
};

#include "gpu_cvutil.h"

static bool read_image(FILE* f, cv::Mat* m) {
  int32_t d[3];
  if (fread(d, 4, 3, f) != 3) return false;
  *m = cv::Mat(d[1], d[0], d[2] == 1 ? CV_8UC1 : d[2] == 3 ? CV_8UC3 : CV_8UC4);
  for (int y = 0; y < d[1]; ++y)
    if (fread(m->ptr<uint8_t>(y), 1, size_t(d[0]) * d[2], f) != size_t(d[0]) * d[2]) return false;
  return true;
}

static void print(const char* what, size_t i, const QVector<QRect>& rects) {
  for (const QRect& r : rects) printf("%s %zu %d %d %d %d\n", what, i, r.x(), r.y(), r.width(), r.height());
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  int32_t n = 0;
  if (!f || fread(&n, 4, 1, f) != 1) return 2;
  std::vector<cv::Mat> sheets;
  sheets.resize(size_t(n));
  for (cv::Mat& m : sheets)
    if (!read_image(f, &m)) return 2;
  fclose(f);
  std::vector<QVector<QRect>> all;
  cbird_gpu::gpuDemosaicHough(sheets, all, DemosaicParams());
  if (all.size() != sheets.size()) return 3;
  for (size_t i = 0; i < all.size(); ++i) print("batch", i, all[i]);
  for (size_t i = 0; i < sheets.size(); ++i) {
    // the sheet as a view: its rows are read where they lie
    const cv::Mat& m = sheets[i];
    cv::Mat big(m.rows + 5, m.cols + 9, m.type());
    memset(big.data, 0x3c, size_t(big.rows) * big.step);
    cv::Mat view = big.colRange(4, 4 + m.cols).rowRange(2, 2 + m.rows);
    for (int y = 0; y < m.rows; ++y) memcpy(view.ptr<uint8_t>(y), m.ptr<uint8_t>(y), size_t(m.cols) * size_t(m.channels()));
    QVector<QRect> rects;
    cbird_gpu::gpuDemosaicHough(view, rects, DemosaicParams());
    print("single", i, rects);
  }
  DemosaicParams tight;
  tight.houghThreshFactor = 0.99f;
  QVector<QRect> rects;
  cbird_gpu::gpuDemosaicHough(sheets[0], rects, tight);
  print("tight", 0, rects);
  return 0;
}
