// test_quality.cpp -- the qualityScore drop-ins (cbird_amd/cpp/gpu_cvutil.h) compiled against the mock cv::Mat, run on
// the MI355X and compared with numbers the Python test passes in (tests/test_quality_cpp.py: the numpy restatement).
//
//   test_quality <file> : the file holds int32 n, then per image int32 w, h, channels, vx, vy, vw, vh and w*h*channels
//   bytes (cv::Mat order).  Prints "one" with gpuQualityScore of every image, "view" with gpuQualityScore of the view
//   (vx, vy, vw, vh) of every image, "group" with gpuQualityScores of all the images in one call, "views" with
//   gpuQualityScores of all the views in one call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "index.h"
#include "gpu_cvutil.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  int32_t n = 0;
  if (!f || fread(&n, 4, 1, f) != 1) return 2;
  std::vector<cv::Mat> images, views;
  for (int i = 0; i < n; ++i) {
    int32_t d[7];
    if (fread(d, 4, 7, f) != 7) return 2;
    cv::Mat m(d[1], d[0], d[2] == 1 ? CV_8UC1 : d[2] == 3 ? CV_8UC3 : CV_8UC4);
    for (int y = 0; y < d[1]; ++y)
      if (fread(m.ptr<uint8_t>(y), 1, size_t(d[0]) * d[2], f) != size_t(d[0]) * d[2]) return 2;
    images.push_back(m);
    views.push_back(m.colRange(d[3], d[3] + d[5]).rowRange(d[4], d[4] + d[6]));
  }
  fclose(f);
  printf("one");
  for (const cv::Mat& m : images) printf(" %d", cbird_gpu::gpuQualityScore(m));
  printf("\nview");
  for (const cv::Mat& m : views) printf(" %d", cbird_gpu::gpuQualityScore(m));
  std::vector<int> scores(3, 7);  // replaced, not appended to
  cbird_gpu::gpuQualityScores(images, scores);
  printf("\ngroup");
  for (int s : scores) printf(" %d", s);
  cbird_gpu::gpuQualityScores(views, scores);
  printf("\nviews");
  for (int s : scores) printf(" %d", s);
  printf("\n");
  cbird_gpu::gpuQualityScores(std::vector<cv::Mat>(), scores);
  return scores.empty() ? 0 : 3;
}
