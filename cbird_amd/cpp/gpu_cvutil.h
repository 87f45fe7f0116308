// gpu_cvutil.h -- drop-ins for the two hash producers of cbird's indexer, on libcbird_hip:
//
//   uint64_t dctHash64(const cv::Mat& cvImg, bool inPlace = false)                  src/cvutil.h, src/cvutil.cpp:435-545
//   void Media::makeKeyPointHashes(const cv::Mat&, const KeyPointList&, KeyPointHashList&) const   src/media.cpp:874-923
//   void sizeLongestSide(cv::Mat& img, int size, int filter = INTER_LANCZOS4)        src/cvutil.h:251, cvutil.cpp:1932-1950
//   void Media::makeKeyPoints(const cv::Mat&, int numKeyPoints, KeyPointList&) const                 src/media.cpp:859-866
//   void Media::makeKeyPointDescriptors(const cv::Mat&, KeyPointList&, KeyPointDescriptors&) const   src/media.cpp:868-872
//   static void ColorDescriptor::create(const cv::Mat& cvImg, ColorDescriptor& desc)                 src/cvutil.cpp:790-1099
//   void Media::makeVideoIndex(VideoContext&, int threshold, VideoIndex&, const std::function<void(int)>&) const
//                                                                                                  src/media.cpp:925-1037
//   the scoring block of TemplateMatcher::match (mask, two dctHash64, hamm64)                     src/templatematcher.cpp:331-371
//   int qualityScore(const Media&, QVector<QImage>* visuals = nullptr)   (decoded images, one or a group)   src/cimgops.cpp:313-596
//   void brightnessAndContrastAuto(const cv::Mat& src, cv::Mat& dst, float clipHistPercent = 0)       src/cvutil.cpp:657-665
//   static QImage differenceImage(const Media& ml, const Media& mr, ...)   (decoded images, one pair or a group)
//                                                                                 src/gui/mediagrouplistwidget.cpp:106-208
//   void VideoCompareWidget::alignSpatially() / alignTemporally()   (decoded frames, one pair, a group or a clip)
//                                                                                 src/gui/videocomparewidget.cpp:590-680
//   void demosaicHough(const cv::Mat& cvImg, QVector<QRect>& rects, const DemosaicParams& params = {})   (one sheet or a batch)
//                                                                                 src/cvutil.cpp:1445-1688
//
// Same arguments and effects as the originals for 8-bit single-channel images (what Scanner::processImage passes
// after grayscale(), src/scanner.cpp:859,876-889): the hash is returned, and with inPlace = true the blurred pixels
// are written back into the caller's image.  A cv::Mat that is a VIEW into a larger image (colRange/rowRange) is
// blurred with the parent's pixels around it, as cv::blur does (Mat::locateROI); the view's parent is what gets
// staged on the device.
//
// These are per-call conveniences (one image, one H2D copy per call).  The batched entry points
// cbh_dcthash_batch / cbh_process_images / cbh_keypoint_hashes are what an indexer that wants the GPU's throughput
// calls with many images at once.
//
// Build note: needs cbird's cvutil.h / media.h (OpenCV 2.4 cv::Mat, cv::KeyPoint) on the include path; in this
// repository it is compiled against tests/cpp/mock/index.h instead (tests/cpp/test_cvutil.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <vector>

#include "cbird_hip.h"

namespace cbird_gpu {

inline int& hashDevice() {  // the device the per-call helpers use
  static int dev = 0;
  return dev;
}

namespace detail {
struct ParentView {
  const uint8_t* base;  // first pixel of the parent image
  uint32_t w, h, step;
  int32_t x, y;         // the view's offset inside it
};
inline ParentView parentOf(const cv::Mat& m) {
  cv::Size whole;
  cv::Point ofs;
  m.locateROI(whole, ofs);
  ParentView p;
  p.step = uint32_t(m.step);
  p.base = m.data - size_t(ofs.y) * m.step - size_t(ofs.x);
  p.w = uint32_t(whole.width), p.h = uint32_t(whole.height);
  p.x = ofs.x, p.y = ofs.y;
  return p;
}
}  // namespace detail

// dctHash64(cvImg, inPlace) for CV_8UC1.  Colour input is converted by the caller exactly as before
// (grayscale(), cvutil.cpp:1265-1283; on the GPU: cbh_process_images).
inline uint64_t gpuDctHash64(const cv::Mat& cvImg, bool inPlace = false) {
  if (cvImg.type() != CV_8UC1 || cvImg.rows <= 0 || cvImg.cols <= 0)
    qFatal("gpuDctHash64: expected a non-empty CV_8UC1 image");
  const detail::ParentView p = detail::parentOf(cvImg);
  const size_t bytes = size_t(p.h - 1) * p.step + p.w;
  const uint64_t off = 0;
  const int32_t rect[4] = {p.x, p.y, cvImg.cols, cvImg.rows};
  const uint32_t first[2] = {0, 1};
  uint64_t hash = 0;
  // in place: the device copy of the parent comes back over the caller's pixels (only the view's rectangle differs)
  const int rc = cbh_dcthash_rects(p.base, bytes, 1, &off, &p.w, &p.h, &p.step, rect, first, inPlace ? 1 : 0, &hash,
                                   inPlace ? const_cast<uint8_t*>(p.base) : nullptr, hashDevice());
  if (rc) qFatal("gpuDctHash64: %s (%s)", cbh_strerror(rc), cbh_last_error());
  return hash;
}

// Media::makeKeyPointHashes: the hashes are appended to outHashes like the original does (push_back per rectangle);
// cvImg is modified by the in-place blurs.
inline void gpuMakeKeyPointHashes(const cv::Mat& cvImg, const KeyPointList& keyPoints, KeyPointHashList& outHashes) {
  Q_ASSERT(cvImg.type() == CV_8UC1);  // grayscale, media.cpp:877
  if (keyPoints.empty() || cvImg.rows <= 0 || cvImg.cols <= 0) return;
  const detail::ParentView p = detail::parentOf(cvImg);
  if (p.x != 0 || p.y != 0 || int(p.w) != cvImg.cols || int(p.h) != cvImg.rows)
    qFatal("gpuMakeKeyPointHashes: expected a whole image, not a view");
  std::vector<float> kp;
  kp.reserve(keyPoints.size() * 3);
  for (const cv::KeyPoint& k : keyPoints) {
    kp.push_back(k.pt.x);
    kp.push_back(k.pt.y);
    kp.push_back(k.size);
  }
  const size_t bytes = size_t(p.h - 1) * p.step + p.w;
  const uint64_t off = 0;
  const uint32_t kpFirst[2] = {0, uint32_t(keyPoints.size())};
  uint32_t outFirst[2] = {0, 0};
  std::vector<uint64_t> hashes(keyPoints.size());
  const int rc = cbh_keypoint_hashes(p.base, bytes, 1, &off, &p.w, &p.h, &p.step, kp.data(), kpFirst, hashes.data(),
                                     outFirst, const_cast<uint8_t*>(p.base), hashDevice());
  if (rc) qFatal("gpuMakeKeyPointHashes: %s (%s)", cbh_strerror(rc), cbh_last_error());
  for (uint32_t i = 0; i < outFirst[1]; ++i) outHashes.push_back(hashes[i]);
}

// sizeLongestSide(img, size) with the default INTER_LANCZOS4 filter: img is replaced by the resized image.
inline void gpuSizeLongestSide(cv::Mat& img, int size) {
  if (img.type() != CV_8UC1 || img.rows <= 0 || img.cols <= 0) qFatal("gpuSizeLongestSide: expected a CV_8UC1 image");
  int w = 0, h = 0;
  cbh_longest_side_dims(img.cols, img.rows, size, &w, &h);
  if (w == 0 || h == 0)  // the reference's own check (cvutil.cpp:1944-1946)
    throw std::invalid_argument("sizeLongestSide: computed width or height is 0, probably bad input");
  cv::Mat out(h, w, CV_8UC1);
  const int rc = cbh_size_longest_side(img.data, 1, img.cols, img.rows, size_t(img.step), 0, size, out.data, &w, &h,
                                       hashDevice());
  if (rc) qFatal("gpuSizeLongestSide: %s (%s)", cbh_strerror(rc), cbh_last_error());
  img = out;
}

// ---- ORB (cbh_orb*, cbird_amd/csrc/orb.hip) ---------------------------------------------------------------------
// rBRIEF's test pairs are OpenCV's learned table bit_pattern_31_ (modules/features2d/src/orb.cpp), an input of the
// library: hand it over once, e.g. gpuOrbSetPattern(bit_pattern_31_) from a translation unit that has the table.
inline void gpuOrbSetPattern(const int* bitPattern31 /* 256 * 4 */) {
  int8_t xy[1024];
  for (int i = 0; i < 1024; ++i) xy[i] = int8_t(bitPattern31[i]);
  const int rc = cbh_orb_set_pattern(xy);
  if (rc) qFatal("gpuOrbSetPattern: %s", cbh_strerror(rc));
}

namespace detail {
inline void wholeImage(const cv::Mat& cvImg, const char* who, ParentView* p) {
  if (cvImg.type() != CV_8UC1 || cvImg.rows <= 0 || cvImg.cols <= 0) qFatal("%s: expected a non-empty CV_8UC1 image", who);
  *p = parentOf(cvImg);
  if (p->x != 0 || p->y != 0 || int(p->w) != cvImg.cols || int(p->h) != cvImg.rows)
    qFatal("%s: expected a whole image, not a view", who);
}
}  // namespace detail

// Media::makeKeyPoints: outKeypoints is replaced, like cv::FeatureDetector::detect does
inline void gpuMakeKeyPoints(const cv::Mat& cvImg, int numKeyPoints, KeyPointList& outKeypoints) {
  detail::ParentView p;
  detail::wholeImage(cvImg, "gpuMakeKeyPoints", &p);
  const size_t bytes = size_t(p.h - 1) * p.step + p.w;
  const uint64_t off = 0;
  int cap = numKeyPoints + 64;
  std::vector<cbh_keypoint> kp;
  uint32_t count = 0;
  for (;;) {  // retainBest can keep ties beyond n: a count above the capacity asks for a second call
    kp.resize(size_t(cap));
    const int rc = cbh_orb(p.base, bytes, 1, &off, &p.w, &p.h, &p.step, numKeyPoints, cap, kp.data(), nullptr, nullptr,
                           &count, hashDevice());
    if (rc) qFatal("gpuMakeKeyPoints: %s (%s)", cbh_strerror(rc), cbh_last_error());
    if (int(count) <= cap) break;
    cap = int(count);
  }
  outKeypoints.clear();
  for (uint32_t i = 0; i < count; ++i)
    outKeypoints.push_back(cv::KeyPoint(kp[i].x, kp[i].y, kp[i].size, kp[i].angle, kp[i].response, kp[i].octave, -1));
}

// Media::makeKeyPointDescriptors: keyPoints is in/out as in the original (border filter, grouping by octave, the
// coordinate round trip); outDescriptors becomes a keyPoints.size() x 32 CV_8UC1 matrix
inline void gpuMakeKeyPointDescriptors(const cv::Mat& cvImg, KeyPointList& keyPoints, KeyPointDescriptors& outDescriptors) {
  detail::ParentView p;
  detail::wholeImage(cvImg, "gpuMakeKeyPointDescriptors", &p);
  const size_t bytes = size_t(p.h - 1) * p.step + p.w;
  const uint64_t off = 0;
  std::vector<cbh_keypoint> in(keyPoints.size()), out(keyPoints.size() + 1);
  for (size_t i = 0; i < keyPoints.size(); ++i) {
    const cv::KeyPoint& k = keyPoints[i];
    in[i] = cbh_keypoint{k.pt.x, k.pt.y, k.size, k.angle, k.response, k.octave};
  }
  std::vector<uint8_t> desc((keyPoints.size() + 1) * 32);
  const uint32_t first[2] = {0, uint32_t(keyPoints.size())};
  uint32_t outFirst[2] = {0, 0};
  const int rc = cbh_orb_describe(p.base, bytes, 1, &off, &p.w, &p.h, &p.step, in.data(), first, out.data(), desc.data(),
                                  outFirst, hashDevice());
  if (rc) qFatal("gpuMakeKeyPointDescriptors: %s (%s)", cbh_strerror(rc), cbh_last_error());
  keyPoints.clear();
  outDescriptors = cv::Mat(int(outFirst[1]), 32, CV_8UC1);
  for (uint32_t i = 0; i < outFirst[1]; ++i) {
    keyPoints.push_back(cv::KeyPoint(out[i].x, out[i].y, out[i].size, out[i].angle, out[i].response, out[i].octave, -1));
    memcpy(outDescriptors.ptr<uint8_t>(int(i)), desc.data() + size_t(i) * 32, 32);
  }
}

// ColorDescriptor::create: desc is written only when the reference would write it (a BGR / BGRA image with at least 32
// samples brighter than L = 4); one image per call -- an indexer that wants the GPU's throughput batches them through
// cbh_color_descriptors / cbh_index_images (the clustering kernel runs one lane per image)
inline void gpuColorDescriptorCreate(const cv::Mat& cvImg, ColorDescriptor& desc) {
  if (cvImg.type() != CV_8UC3 && cvImg.type() != CV_8UC4) {
    qDebug("passed a grayscale image");
    return;
  }
  static_assert(sizeof(ColorDescriptor) == 258, "the record ColorDescIndex stores");
  const uint64_t off = 0;
  const uint32_t w = uint32_t(cvImg.cols), h = uint32_t(cvImg.rows), step = uint32_t(cvImg.step);
  uint8_t rec[258], ok = 0;
  const int rc = cbh_color_descriptors(cvImg.data, size_t(h - 1) * step + size_t(w) * size_t(cvImg.channels()), 1, &off, &w,
                                       &h, &step, cvImg.channels(), rec, &ok, hashDevice());
  if (rc) qFatal("gpuColorDescriptorCreate: %s (%s)", cbh_strerror(rc), cbh_last_error());
  if (ok) memcpy(&desc, rec, sizeof desc);
  else qWarning("not enough colors");
}

// Media::makeVideoIndex(video, threshold, outIndex, progressCb) -- src/media.cpp:925-1037.  Same resume rule
// (:929-936), same result; the frames are collected chunkFrames at a time and hashed on the device
// (autocrop(img, 20) + dctHash64), the near-frame filter runs in the library between chunks.  VideoContextT is
// cbird's VideoContext: seek(int), nextFrame(cv::Mat&), metadata().frameRate / .duration.
template <class VideoContextT>
inline void gpuMakeVideoIndex(VideoContextT& video, int threshold, VideoIndex& outIndex,
                              const std::function<void(int)>& progressCb = std::function<void(int)>(),
                              int chunkFrames = 64) {
  VideoIndex& index = outIndex;
  cbh_vindexer* ix = cbh_vindexer_create(hashDevice(), threshold, 20 /* FIXME upstream: index settings, :961 */);
  if (!ix) qFatal("gpuMakeVideoIndex: no usable device");
  if (index.frames.size() > 0 && index.frames.size() == index.hashes.size() && video.seek(index.frames.back() + 1)) {
    static_assert(sizeof(index.frames[0]) == sizeof(int32_t) && sizeof(index.hashes[0]) == sizeof(uint64_t), "");
    const int rc = cbh_vindexer_resume(ix, reinterpret_cast<const int32_t*>(index.frames.data()),
                                       reinterpret_cast<const uint64_t*>(index.hashes.data()), index.frames.size());
    if (rc != CBH_OK) {
      cbh_vindexer_destroy(ix);
      qFatal("gpuMakeVideoIndex: cannot resume from the given index");
    }
    qDebug("resuming index from frame: %d", index.frames.back() + 1);
  }
  index.hashes.clear();
  index.frames.clear();
  const int totalFrames = int(video.metadata().frameRate * video.metadata().duration);
  if (chunkFrames < 1) chunkFrames = 1;
  std::vector<uint8_t> stage;
  int cw = 0, ch = 0, held = 0;
  auto flush = [&]() {
    if (held == 0) return;
    const int rc = cbh_vindexer_push(ix, stage.data(), size_t(held), cw, ch, size_t(cw), size_t(cw) * size_t(ch));
    if (rc != CBH_OK) {
      cbh_vindexer_destroy(ix);
      qFatal("gpuMakeVideoIndex: cbh_vindexer_push failed");
    }
    held = 0;
    if (progressCb) progressCb(int(cbh_vindexer_frames_seen(ix) * 100 / std::max(totalFrames, 1)));
  };
  cv::Mat cvFrame;
  while (video.nextFrame(cvFrame)) {
    if (cvFrame.type() != CV_8UC1 || cvFrame.rows <= 0 || cvFrame.cols <= 0)
      qFatal("gpuMakeVideoIndex: the decoder is expected to output grey frames (media.cpp:959)");
    if (cvFrame.cols != cw || cvFrame.rows != ch) {  // first frame (or a mid-stream size change)
      flush();
      cw = cvFrame.cols, ch = cvFrame.rows;
      stage.resize(size_t(chunkFrames) * size_t(cw) * size_t(ch));
    }
    uint8_t* dst = stage.data() + size_t(held) * size_t(cw) * size_t(ch);
    for (int y = 0; y < ch; ++y) memcpy(dst + size_t(y) * size_t(cw), cvFrame.template ptr<uint8_t>(y), size_t(cw));
    if (++held == chunkFrames) flush();
    if (cbh_vindexer_frames_seen(ix) + held >= (1 << 24)) break;  // MAX_FRAMES_PER_VIDEO, :1013-1016
  }
  flush();
  const long long n = cbh_vindexer_finish(ix, nullptr, nullptr, 0);
  if (n > 0) {
    index.frames.resize(size_t(n));
    index.hashes.resize(size_t(n));
    cbh_vindexer_finish(ix, reinterpret_cast<int32_t*>(index.frames.data()),
                        reinterpret_cast<uint64_t*>(index.hashes.data()), size_t(n));
  }
  cbh_vindexer_destroy(ix);
  if (progressCb) progressCb(100);
}

// The scoring block of TemplateMatcher::match, src/templatematcher.cpp:331-371: `img` is the candidate patch as
// cv::warpAffine(..., tmplImg.size(), ...) left it, tmplImg the template (8-bit, 1 / 3 / 4 channels each).  Replaces
//     cv::Mat tmplMasked = tmplImg.clone(); grayscale(img, img); { the masking loop }
//     uint64_t candHash = dctHash64(img); uint64_t tmplHash = dctHash64(tmplMasked); int dist = hamm64(candHash, tmplHash);
// by   int dist = cbird_gpu::gpuTemplateScore(img, tmplImg);
// (the caller's img / tmplImg are left as they are: nothing after :371 reads them).
inline int gpuTemplateScore(const cv::Mat& img, const cv::Mat& tmplImg, uint64_t* candHash = nullptr,
                            uint64_t* tmplHash = nullptr) {
  if (img.depth() != CV_8U || tmplImg.depth() != CV_8U || img.rows != tmplImg.rows || img.cols != tmplImg.cols ||
      img.rows <= 0 || img.cols <= 0)
    qFatal("gpuTemplateScore: expected two 8-bit images of the template's size");
  uint64_t ch = 0, th = 0;
  int32_t score = 0;
  const int rc = cbh_template_scores(img.data, 1, img.cols, img.rows, size_t(img.step), 0, img.channels(), tmplImg.data,
                                     size_t(tmplImg.step), tmplImg.channels(), &ch, &th, &score, hashDevice());
  if (rc != CBH_OK) qFatal("gpuTemplateScore: cbh_template_scores failed");
  if (candHash) *candHash = ch;
  if (tmplHash) *tmplHash = th;
  return score;
}

// TemplateMatcher::match from the point lists to the score, src/templatematcher.cpp:264-374, for ALL candidates of one
// template in one call that does not leave the device.  Per candidate i: tmplPoints[i] / matchPoints[i] as the loop at
// :243-250 fills them, candImgs[i] the candidate image the keypoints were taken from (8-bit, one channel count for the
// group), candScales[i] its candScale.  Replaces, inside the loop over the candidates,
//     cv::Mat transform = cv::estimateRigidTransform(tmplPoints, matchPoints, false);            (:264)
//     cv::transform(tmplRect, candRect, transform); roi.append(QPoint(int(candRect[i].x / candScale), ...)); (:284-300)
//     for (cv::Point2f& p : matchPoints) { p.x /= candScale; p.y /= candScale; }
//     const cv::Mat tx = cv::estimateRigidTransform(tmplPoints, matchPoints, false);             (:304-309)
//     cv::invertAffineTransform(transform, transform);
//     cv::warpAffine(img, img, transform, tmplImg.size(), cv::INTER_AREA, cv::BORDER_CONSTANT, cv::Scalar(0,0,0,255)); (:331-333)
//     ... the masking loop, the two dctHash64 and hamm64                                          (:337-374)
// by one call after the loop has gathered the lists:
//     std::vector<cbh_template_result> results;
//     cbird_gpu::gpuTemplateMatch(tmplImg, candImgs, tmplPoints, matchPoints, candScales, results);
// results[i].found == 0 is the reference's "no transform found" (score INT_MAX, :271); otherwise .roi holds the four
// QPoints of :299, .tx the matrix for QTransform (:315-316, valid when .tx_found), .score what m.setScore takes (:378).
// (OpenCV parity of the estimate and the warp is unpinned: see include/cbird_hip.h.)
inline void gpuTemplateMatch(const cv::Mat& tmplImg, const std::vector<cv::Mat>& candImgs,
                             const std::vector<std::vector<cv::Point2f>>& tmplPoints,
                             const std::vector<std::vector<cv::Point2f>>& matchPoints, const std::vector<float>& candScales,
                             std::vector<cbh_template_result>& results) {
  const size_t n = candImgs.size();
  if (tmplPoints.size() != n || matchPoints.size() != n || candScales.size() != n)
    qFatal("gpuTemplateMatch: one point list pair and one scale per candidate");
  results.assign(n, cbh_template_result());
  if (n == 0) return;
  if (tmplImg.depth() != CV_8U || tmplImg.rows <= 0 || tmplImg.cols <= 0)
    qFatal("gpuTemplateMatch: expected a non-empty 8-bit template");
  const int cn = candImgs[0].channels();
  std::vector<uint64_t> off, first(1, 0);
  std::vector<uint32_t> w, h, step;
  std::vector<uint8_t> buf;
  std::vector<float> a, b;
  for (size_t i = 0; i < n; ++i) {
    const cv::Mat& m = candImgs[i];
    if (m.rows <= 0 || m.cols <= 0 || m.depth() != CV_8U || m.channels() != cn)
      qFatal("gpuTemplateMatch: expected non-empty 8-bit candidates of one channel count");
    if (tmplPoints[i].size() != matchPoints[i].size()) qFatal("gpuTemplateMatch: the point lists of a candidate differ in length");
    const size_t row = size_t(m.cols) * size_t(cn);
    off.push_back((buf.size() + 15) / 16 * 16);
    buf.resize(size_t(off.back()) + row * size_t(m.rows));
    for (int y = 0; y < m.rows; ++y) memcpy(buf.data() + off.back() + size_t(y) * row, m.ptr<uint8_t>(y), row);
    w.push_back(uint32_t(m.cols)), h.push_back(uint32_t(m.rows)), step.push_back(uint32_t(row));
    for (size_t k = 0; k < tmplPoints[i].size(); ++k) {
      a.push_back(tmplPoints[i][k].x), a.push_back(tmplPoints[i][k].y);
      b.push_back(matchPoints[i][k].x), b.push_back(matchPoints[i][k].y);
    }
    first.push_back(first.back() + tmplPoints[i].size());
  }
  const int rc = cbh_template_match(tmplImg.data, tmplImg.cols, tmplImg.rows, size_t(tmplImg.step), tmplImg.channels(),
                                    buf.data(), buf.size(), n, off.data(), w.data(), h.data(), step.data(), cn, a.data(),
                                    b.data(), first.data(), candScales.data(), results.data(), nullptr, hashDevice());
  if (rc) qFatal("gpuTemplateMatch: %s (%s)", cbh_strerror(rc), cbh_last_error());
}

// TemplateMatcher::match from the decoded images to the score, src/templatematcher.cpp:113-374, for ALL candidates of one
// template in one call that does not come back to the host between the upload and the results.  tmplImg / candImgs[i]:
// what qImageToCvImg gave (:114, :173), 8-bit, one channel count for the template and the group; params: SearchParams
// (any type with needleFeatures, haystackFeatures, cvThresh, tmScalePct).  Replaces
//     tmplMedia.makeKeyPoints(tmplImg, params.needleFeatures, ...); makeKeyPointDescriptors(...)         (:118-121)
//     cv::BFMatcher matcher(cv::NORM_HAMMING, true); matcher.add(haystack);                              (:134-138)
// and, inside the loop over the candidates, everything from
//     float candScale = 1.0; ... sizeScaleFactor(img, candScale);                                        (:182-192)
//     m.makeKeyPoints(img, params.haystackFeatures, ...); m.makeKeyPointDescriptors(...)                  (:196-202)
//     matcher.radiusMatch(queryDescriptors, dmatch, params.cvThresh);                                     (:217)
//     ... the loops that fill matches, tmplPoints and matchPoints                                         (:221-250)
// to hamm64(candHash, tmplHash) (:374; gpuTemplateMatch above lists :264-374) by one call in front of the loop:
//     std::vector<cbh_tm_image_result> results;
//     cbird_gpu::gpuTemplateMatchImages(tmplImg, candImgs, params, results);
// The loop keeps what is the caller's: loading (:166-170), and per results[i].status the exits -- CBH_TM_NO_KEYPOINTS
// continues without caching (:210-213); NO_MATCHES / FEW_POINTS / NO_TRANSFORM cache INT_MAX (:230-235, :255-260,
// :268-273); SCORED takes .r.roi, .r.tx and .r.score (:294-320, :378-413); CBH_TM_NO_TEMPLATE_KEYPOINTS on every
// candidate is the return of :127-130.  cbh_orb_set_pattern must have been called (ORB's test pairs are OpenCV's table).
// (OpenCV parity of ORB, the estimate and the warp is unpinned: see include/cbird_hip.h.)
template <class Params>
inline void gpuTemplateMatchImages(const cv::Mat& tmplImg, const std::vector<cv::Mat>& candImgs, const Params& params,
                                   std::vector<cbh_tm_image_result>& results) {
  const size_t n = candImgs.size();
  results.assign(n, cbh_tm_image_result());
  if (n == 0) return;
  if (tmplImg.depth() != CV_8U || tmplImg.rows <= 0 || tmplImg.cols <= 0)
    qFatal("gpuTemplateMatchImages: expected a non-empty 8-bit template");
  const int cn = tmplImg.channels();
  std::vector<uint64_t> off;
  std::vector<uint32_t> w, h, step;
  std::vector<uint8_t> buf;
  for (size_t i = 0; i < n; ++i) {
    const cv::Mat& m = candImgs[i];
    if (m.rows <= 0 || m.cols <= 0 || m.depth() != CV_8U || m.channels() != cn)
      qFatal("gpuTemplateMatchImages: expected non-empty 8-bit candidates of the template's channel count");
    const size_t row = size_t(m.cols) * size_t(cn);
    off.push_back((buf.size() + 15) / 16 * 16);
    buf.resize(size_t(off.back()) + row * size_t(m.rows));
    for (int y = 0; y < m.rows; ++y) memcpy(buf.data() + off.back() + size_t(y) * row, m.ptr<uint8_t>(y), row);
    w.push_back(uint32_t(m.cols)), h.push_back(uint32_t(m.rows)), step.push_back(uint32_t(row));
  }
  const cbh_tm_params p = {int32_t(params.needleFeatures), int32_t(params.haystackFeatures), int32_t(params.cvThresh),
                           int32_t(params.tmScalePct)};
  const int rc = cbh_template_match_images(tmplImg.data, tmplImg.cols, tmplImg.rows, size_t(tmplImg.step), buf.data(),
                                           buf.size(), n, off.data(), w.data(), h.data(), step.data(), cn, &p,
                                           results.data(), nullptr, hashDevice());
  if (rc) qFatal("gpuTemplateMatchImages: %s (%s)", cbh_strerror(rc), cbh_last_error());
}

// gpuTemplateMatchImages for a batch of result groups in ONE call: what Database::similar does once per needle when
// params.templateMatch is set (src/database.cpp:1418: TemplateMatcher().match(needle, match, params) right after
// searchIndex).  images: every decoded image once (the needles and their candidates; an image may be a template in some
// pairs and a candidate in others), 8-bit, one channel count; pairs[p] = (template, candidate) as indexes of `images`, in
// any order.  results[p] is what gpuTemplateMatchImages(images[pairs[p].first], {images[pairs[p].second]}, ...) gives as
// results[0].  The caller keeps what is its own, per group: loading, the md5-pair cache, the threshold and the sort.
template <class Params>
inline void gpuTemplateMatchPairs(const std::vector<cv::Mat>& images, const std::vector<std::pair<int, int>>& pairs,
                                  const Params& params, std::vector<cbh_tm_image_result>& results) {
  const size_t n = pairs.size();
  results.assign(n, cbh_tm_image_result());
  if (n == 0) return;
  if (images.empty()) qFatal("gpuTemplateMatchPairs: pairs without images");
  const int cn = images[0].channels();
  std::vector<uint64_t> off;
  std::vector<uint32_t> w, h, step, pt, pc;
  std::vector<uint8_t> buf;
  for (size_t i = 0; i < images.size(); ++i) {
    const cv::Mat& m = images[i];
    if (m.rows <= 0 || m.cols <= 0 || m.depth() != CV_8U || m.channels() != cn)
      qFatal("gpuTemplateMatchPairs: expected non-empty 8-bit images of one channel count");
    const size_t row = size_t(m.cols) * size_t(cn);
    off.push_back((buf.size() + 15) / 16 * 16);
    buf.resize(size_t(off.back()) + row * size_t(m.rows));
    for (int y = 0; y < m.rows; ++y) memcpy(buf.data() + off.back() + size_t(y) * row, m.ptr<uint8_t>(y), row);
    w.push_back(uint32_t(m.cols)), h.push_back(uint32_t(m.rows)), step.push_back(uint32_t(row));
  }
  for (size_t p = 0; p < n; ++p) {
    if (pairs[p].first < 0 || pairs[p].second < 0 || size_t(pairs[p].first) >= images.size() ||
        size_t(pairs[p].second) >= images.size())
      qFatal("gpuTemplateMatchPairs: a pair names an image that is not in the table");
    pt.push_back(uint32_t(pairs[p].first)), pc.push_back(uint32_t(pairs[p].second));
  }
  const cbh_tm_params p = {int32_t(params.needleFeatures), int32_t(params.haystackFeatures), int32_t(params.cvThresh),
                           int32_t(params.tmScalePct)};
  const int rc = cbh_template_match_pairs(buf.data(), buf.size(), images.size(), off.data(), w.data(), h.data(), step.data(),
                                          cn, pt.data(), pc.data(), n, &p, results.data(), hashDevice());
  if (rc) qFatal("gpuTemplateMatchPairs: %s (%s)", cbh_strerror(rc), cbh_last_error());
}

// qualityScore(const Media&) (src/cimgops.cpp:313-596) for images that are already decoded: 8-bit cv::Mat of 1, 3 (BGR)
// or 4 (BGRA) channels, the layout loadImage / qImageToCvImg give.  Only the red channel takes part, as in the
// reference (its crop keeps channel 0 of qImageToCImg's planes).  INT32_MIN = no score (no edges at all, or a side of 1,
// where the reference's behaviour is undefined).  The visuals of the original are cbh_quality_scores_dev's planes.
// One group per call: what qualityScoreAction (src/gui/mediagrouplistwidget.cpp:1433-1441) would call once per group
// instead of once per member; images of different channel counts go in separate calls to the library.
inline void gpuQualityScores(const std::vector<cv::Mat>& images, std::vector<int>& scores) {
  scores.assign(images.size(), 0);
  for (int cn : {1, 3, 4}) {
    std::vector<size_t> which;
    std::vector<uint64_t> off;
    std::vector<uint32_t> w, h, step;
    std::vector<uint8_t> buf;
    for (size_t i = 0; i < images.size(); ++i) {
      const cv::Mat& m = images[i];
      if (m.rows <= 0 || m.cols <= 0 || (m.type() != CV_8UC1 && m.type() != CV_8UC3 && m.type() != CV_8UC4))
        qFatal("gpuQualityScores: expected non-empty 8-bit images of 1, 3 or 4 channels");
      if (m.channels() != cn) continue;
      const size_t row = size_t(m.cols) * size_t(cn);
      off.push_back((buf.size() + 15) / 16 * 16);
      buf.resize(size_t(off.back()) + row * size_t(m.rows));
      for (int y = 0; y < m.rows; ++y) memcpy(buf.data() + off.back() + size_t(y) * row, m.ptr<uint8_t>(y), row);
      which.push_back(i), w.push_back(uint32_t(m.cols)), h.push_back(uint32_t(m.rows)), step.push_back(uint32_t(row));
    }
    if (which.empty()) continue;
    std::vector<int32_t> out(which.size());
    const int rc = cbh_quality_scores(buf.data(), buf.size(), which.size(), off.data(), w.data(), h.data(), step.data(), cn,
                                      out.data(), nullptr, hashDevice());
    if (rc) qFatal("gpuQualityScores: %s (%s)", cbh_strerror(rc), cbh_last_error());
    for (size_t k = 0; k < which.size(); ++k) scores[which[k]] = out[k];
  }
}

// one image, read where it lies (rows may be padded; a view's rows are read from its parent)
inline int gpuQualityScore(const cv::Mat& img) {
  if (img.rows <= 0 || img.cols <= 0 || (img.type() != CV_8UC1 && img.type() != CV_8UC3 && img.type() != CV_8UC4))
    qFatal("gpuQualityScore: expected a non-empty 8-bit image of 1, 3 or 4 channels");
  const uint64_t off = 0;
  const uint32_t w = uint32_t(img.cols), h = uint32_t(img.rows), step = uint32_t(img.step);
  int32_t score = 0;
  const int rc = cbh_quality_scores(img.data, size_t(h - 1) * step + size_t(w) * size_t(img.channels()), 1, &off, &w, &h,
                                    &step, img.channels(), &score, nullptr, hashDevice());
  if (rc) qFatal("gpuQualityScore: %s (%s)", cbh_strerror(rc), cbh_last_error());
  return score;
}

// void brightnessAndContrastAuto(const cv::Mat& src, cv::Mat& dst, float clipHistPercent = 0)   src/cvutil.cpp:657-665
// for CV_8UC1 / CV_8UC3 / CV_8UC4, read where it lies (a view's rows are read from its parent).  dst is replaced by a new
// image of src's size and type; when no adjustment is possible (minGray >= maxGray) it is a copy where the reference
// shares src's storage.  minGray / maxGray: what grayLevel found.  (convertTo's rounding is unpinned against OpenCV: see
// include/cbird_hip.h.)
inline void gpuBrightnessAndContrastAuto(const cv::Mat& src, cv::Mat& dst, float clipHistPercent = 0, int* minGray = nullptr,
                                         int* maxGray = nullptr) {
  if (src.rows <= 0 || src.cols <= 0 || (src.type() != CV_8UC1 && src.type() != CV_8UC3 && src.type() != CV_8UC4))
    qFatal("gpuBrightnessAndContrastAuto: expected a non-empty 8-bit image of 1, 3 or 4 channels");
  const uint64_t off = 0;
  const uint32_t w = uint32_t(src.cols), h = uint32_t(src.rows), step = uint32_t(src.step);
  const size_t row = size_t(w) * size_t(src.channels()), bytes = size_t(h - 1) * step + row;
  std::vector<uint8_t> out(bytes);
  int32_t cuts[2] = {0, 0};
  const int rc = cbh_auto_contrast(src.data, bytes, 1, &off, &w, &h, &step, src.channels(), clipHistPercent, out.data(), cuts,
                                   nullptr, hashDevice());
  if (rc) qFatal("gpuBrightnessAndContrastAuto: %s (%s)", cbh_strerror(rc), cbh_last_error());
  cv::Mat res(src.rows, src.cols, src.type());
  for (int y = 0; y < src.rows; ++y) memcpy(res.ptr<uint8_t>(y), out.data() + size_t(y) * step, row);
  dst = res;
  if (minGray) *minGray = cuts[0];
  if (maxGray) *maxGray = cuts[1];
}

// static QImage differenceImage(const Media& ml, const Media& mr, ...)   src/gui/mediagrouplistwidget.cpp:106-208
// for images that are already decoded (8-bit cv::Mat of 1, 3 = BGR or 4 = BGRA channels, what qImageToCvImg gives), ONE
// left image against all the right images of a group in one call.  results: NULL, or per right image the record the
// template matcher returned (gpuTemplateMatch / gpuTemplateMatchImages' .r): .tx is the matrix Media::transform() holds
// (:315-316; for a QTransform t: {t.m11(), t.m21(), t.dx(), t.m12(), t.m22(), t.dy()}) and is used where .tx_found is set
// and it is not the identity (:114).  images[i] becomes a CV_8UC4 BGRA image, the bytes of the reference's Format_RGB32
// picture; details[i] the record to rank the group by (include/cbird_hip.h).  The clip of 5 % is the reference's (:135).
// (The aligned right image and QImage::scaled are unpinned against Qt, convertTo against OpenCV: see include/cbird_hip.h.)
inline void gpuDifferenceImages(const cv::Mat& left, const std::vector<cv::Mat>& rights, const cbh_template_result* results,
                                std::vector<cv::Mat>& images, std::vector<cbh_diff_detail>& details,
                                float clipHistPercent = 5) {
  images.assign(rights.size(), cv::Mat());
  details.assign(rights.size(), cbh_diff_detail());
  if (left.rows <= 0 || left.cols <= 0 || (left.type() != CV_8UC1 && left.type() != CV_8UC3 && left.type() != CV_8UC4))
    qFatal("gpuDifferenceImages: expected a non-empty 8-bit left image of 1, 3 or 4 channels");
  for (int cn : {1, 3, 4}) {
    std::vector<size_t> which;
    std::vector<uint64_t> off, outOff;
    std::vector<uint32_t> w, h, step;
    std::vector<uint8_t> buf, has;
    std::vector<double> tx;
    for (size_t i = 0; i < rights.size(); ++i) {
      const cv::Mat& m = rights[i];
      if (m.rows <= 0 || m.cols <= 0 || (m.type() != CV_8UC1 && m.type() != CV_8UC3 && m.type() != CV_8UC4))
        qFatal("gpuDifferenceImages: expected non-empty 8-bit images of 1, 3 or 4 channels");
      if (m.channels() != cn) continue;
      const size_t row = size_t(m.cols) * size_t(cn);
      off.push_back((buf.size() + 15) / 16 * 16);
      buf.resize(size_t(off.back()) + row * size_t(m.rows));
      for (int y = 0; y < m.rows; ++y) memcpy(buf.data() + off.back() + size_t(y) * row, m.ptr<uint8_t>(y), row);
      which.push_back(i), w.push_back(uint32_t(m.cols)), h.push_back(uint32_t(m.rows)), step.push_back(uint32_t(row));
      has.push_back(results && results[i].tx_found ? 1 : 0);
      for (int k = 0; k < 6; ++k) tx.push_back(results ? results[i].tx[k] : 0.0);
    }
    if (which.empty()) continue;
    const size_t n = which.size();
    std::vector<uint32_t> ow(n), oh(n);
    int rc = cbh_difference_dims(left.cols, left.rows, n, w.data(), h.data(), tx.data(), has.data(), ow.data(), oh.data(),
                                 nullptr);
    if (rc) qFatal("gpuDifferenceImages: %s", cbh_strerror(rc));
    size_t total = 0;
    for (size_t k = 0; k < n; ++k) {
      outOff.push_back(total);
      total += (size_t(ow[k]) * oh[k] * 4 + 15) / 16 * 16;
    }
    std::vector<uint8_t> out(total);
    std::vector<cbh_diff_detail> det(n);
    rc = cbh_difference_images(left.data, left.cols, left.rows, size_t(left.step), left.channels(), buf.data(), buf.size(), n,
                               off.data(), w.data(), h.data(), step.data(), cn, tx.data(), has.data(), clipHistPercent,
                               out.data(), out.size(), outOff.data(), det.data(), hashDevice());
    if (rc) qFatal("gpuDifferenceImages: %s (%s)", cbh_strerror(rc), cbh_last_error());
    for (size_t k = 0; k < n; ++k) {
      cv::Mat img(int(oh[k]), int(ow[k]), CV_8UC4);
      memcpy(img.data, out.data() + outOff[k], size_t(ow[k]) * oh[k] * 4);
      images[which[k]] = img;
      details[which[k]] = det[k];
    }
  }
}

// one pair; tx: NULL, or the six numbers of the right image's transform as above
inline cv::Mat gpuDifferenceImage(const cv::Mat& left, const cv::Mat& right, const double* tx = nullptr,
                                  cbh_diff_detail* detail = nullptr, float clipHistPercent = 5) {
  cbh_template_result r = cbh_template_result();
  if (tx) {
    r.tx_found = 1;
    for (int k = 0; k < 6; ++k) r.tx[k] = tx[k];
  }
  std::vector<cv::Mat> images;
  std::vector<cbh_diff_detail> details;
  gpuDifferenceImages(left, std::vector<cv::Mat>(1, right), tx ? &r : nullptr, images, details, clipHistPercent);
  if (detail) *detail = details[0];
  return images[0];
}

namespace detail {
// 8-bit images of ONE channel count behind each other in `buf`, rows packed, 16-byte aligned starts
inline void packMats(const std::vector<cv::Mat>& mats, const std::vector<size_t>& which, int cn, std::vector<uint8_t>& buf,
                     std::vector<uint64_t>& off, std::vector<uint32_t>& w, std::vector<uint32_t>& h,
                     std::vector<uint32_t>& step) {
  for (size_t i : which) {
    const cv::Mat& m = mats[i];
    const size_t row = size_t(m.cols) * size_t(cn);
    off.push_back((buf.size() + 15) / 16 * 16);
    buf.resize(size_t(off.back()) + row * size_t(m.rows));
    for (int y = 0; y < m.rows; ++y) memcpy(buf.data() + off.back() + size_t(y) * row, m.ptr<uint8_t>(y), row);
    w.push_back(uint32_t(m.cols)), h.push_back(uint32_t(m.rows)), step.push_back(uint32_t(row));
  }
}
inline bool is8bit(const cv::Mat& m) {
  return m.rows > 0 && m.cols > 0 && (m.type() == CV_8UC1 || m.type() == CV_8UC3 || m.type() == CV_8UC4);
}
}  // namespace detail

// void VideoCompareWidget::alignSpatially()   src/gui/videocomparewidget.cpp:590-627
// for frames that are already decoded (8-bit cv::Mat of 1, 3 or 4 channels), ONE left image against all the right images
// of a group in one call: out[i] is the shift of +-8 pixels at 256 x 256 with the smallest sum of absolute differences,
// ties as the reference's loops break them (include/cbird_hip.h).  (QImage::scaled is unpinned against Qt.)
inline void gpuAlignSpatial(const cv::Mat& left, const std::vector<cv::Mat>& rights, std::vector<cbh_align_spatial_result>& out) {
  out.assign(rights.size(), cbh_align_spatial_result());
  if (!detail::is8bit(left)) qFatal("gpuAlignSpatial: expected a non-empty 8-bit left image of 1, 3 or 4 channels");
  for (const cv::Mat& m : rights)
    if (!detail::is8bit(m)) qFatal("gpuAlignSpatial: expected non-empty 8-bit images of 1, 3 or 4 channels");
  for (int cn : {1, 3, 4}) {
    std::vector<size_t> which;
    for (size_t i = 0; i < rights.size(); ++i)
      if (rights[i].channels() == cn) which.push_back(i);
    if (which.empty()) continue;
    std::vector<uint64_t> off;
    std::vector<uint32_t> w, h, step;
    std::vector<uint8_t> buf;
    detail::packMats(rights, which, cn, buf, off, w, h, step);
    std::vector<cbh_align_spatial_result> res(which.size());
    const int rc = cbh_align_spatial(left.data, left.cols, left.rows, size_t(left.step), left.channels(), buf.data(), buf.size(),
                                     which.size(), off.data(), w.data(), h.data(), step.data(), cn, res.data(), nullptr,
                                     hashDevice());
    if (rc) qFatal("gpuAlignSpatial: %s (%s)", cbh_strerror(rc), cbh_last_error());
    for (size_t k = 0; k < which.size(); ++k) out[which[k]] = res[k];
  }
}

// one pair: the reference's _alignX, _alignY (:624-625), fractions of the frame's sides; returns the record
inline cbh_align_spatial_result gpuAlignSpatial(const cv::Mat& left, const cv::Mat& right, float* alignX, float* alignY) {
  std::vector<cbh_align_spatial_result> out;
  gpuAlignSpatial(left, std::vector<cv::Mat>(1, right), out);
  if (alignX) *alignX = float(out[0].min_x) / 256.0f;
  if (alignY) *alignY = float(out[0].min_y) / 256.0f;
  return out[0];
}

// void VideoCompareWidget::alignTemporally()   src/gui/videocomparewidget.cpp:629-680
// the window `right` (the reference: 5 frames) against `left` (64) at every placement d = 0 .. left.size() - right.size():
// right[i] on left[d + i].  start: the placement that is kept unless another has a strictly smaller mean SAD (the
// reference's current offset, 30 of 60); -1 = the middle, (P - 1) / 2 + (P - 1) % 2.  The frames of a side share a channel
// count.  Which frame stands in for an index outside the video is the caller's business, as it is FrameCache's.
inline cbh_align_temporal_result gpuAlignTemporal(const std::vector<cv::Mat>& left, const std::vector<cv::Mat>& right,
                                                  int start = -1) {
  if (right.empty() || right.size() > 64 || left.size() < right.size() || left.size() > 65535)
    qFatal("gpuAlignTemporal: expected 1 .. 64 right frames and at least as many, at most 65535, left frames");
  const int placements = int(left.size() - right.size()) + 1;
  if (start < 0) start = (placements - 1) / 2 + (placements - 1) % 2;
  if (start >= placements) qFatal("gpuAlignTemporal: start is no placement");
  std::vector<uint8_t> buf[2];
  std::vector<uint64_t> off[2];
  std::vector<uint32_t> w[2], h[2], step[2];
  int cn[2];
  for (int side = 0; side < 2; ++side) {
    const std::vector<cv::Mat>& frames = side ? right : left;
    cn[side] = frames[0].channels();
    std::vector<size_t> which;
    for (size_t i = 0; i < frames.size(); ++i) {
      if (!detail::is8bit(frames[i]) || frames[i].channels() != cn[side])
        qFatal("gpuAlignTemporal: expected non-empty 8-bit frames of 1, 3 or 4 channels, one channel count per side");
      which.push_back(i);
    }
    detail::packMats(frames, which, cn[side], buf[side], off[side], w[side], h[side], step[side]);
  }
  cbh_align_temporal_result res = cbh_align_temporal_result();
  const int rc = cbh_align_temporal(buf[0].data(), buf[0].size(), left.size(), off[0].data(), w[0].data(), h[0].data(),
                                    step[0].data(), cn[0], buf[1].data(), buf[1].size(), right.size(), off[1].data(),
                                    w[1].data(), h[1].data(), step[1].data(), cn[1], start, &res, nullptr, nullptr, hashDevice());
  if (rc) qFatal("gpuAlignTemporal: %s (%s)", cbh_strerror(rc), cbh_last_error());
  return res;
}

// void demosaicHough(const cv::Mat& cvImg, QVector<QRect>& rects, const DemosaicParams& params, QList<QImage>*)
//                                                                                 src/cvutil.cpp:1445-1688
// for a batch of decoded contact sheets (8-bit cv::Mat of 1, 3 or 4 channels): rects[i] receives the tiles of sheets[i]
// in the reference's order and replaces what it held.  (The reference appends to the caller's vector, counts what was
// already there in its `rects.count() < 2` test and then assigns the subdivided list; for the empty vector that
// -select-grid passes the two are the same.)  Templates, so that this header needs neither QRect
// nor DemosaicParams until a caller names them: Params is cbird's DemosaicParams (borderThresh acts nowhere in the
// reference and is not passed on), Rects a QVector<QRect>.  Blur kernels other than 0 and 3, houghRho other than 0.5
// and houghTheta other than 45 are not implemented (include/cbird_hip.h); the outImages drawings are not produced.
template <class Params, class Rects>
inline void gpuDemosaicHough(const std::vector<cv::Mat>& sheets, std::vector<Rects>& rects, const Params& params) {
  rects.assign(sheets.size(), Rects());
  for (const cv::Mat& m : sheets)
    if (!detail::is8bit(m)) qFatal("gpuDemosaicHough: expected non-empty 8-bit images of 1, 3 or 4 channels");
  cbh_demosaic_params p;
  cbh_demosaic_default_params(&p);
  p.clip_pct = float(params.clipHistogramPercent), p.pre_blur = params.preBlurKernel, p.canny1 = params.cannyThresh1;
  p.canny2 = params.cannyThresh2, p.post_blur = params.postBlurKernel, p.h_margin = params.hMargin, p.v_margin = params.vMargin;
  p.hough_rho = params.houghRho, p.hough_theta = params.houghTheta, p.hough_thresh_factor = params.houghThreshFactor;
  p.min_grid_spacing = params.minGridSpacing, p.grid_tolerance = params.gridTolerance, p.crop_margin = params.cropMargin;
  p.max_aspect = params.maxAspectRatio, p.min_aspect = params.minAspectRatio;
  for (int cn : {1, 3, 4}) {
    std::vector<size_t> which;
    for (size_t i = 0; i < sheets.size(); ++i)
      if (sheets[i].channels() == cn) which.push_back(i);
    if (which.empty()) continue;
    std::vector<uint64_t> off;
    std::vector<uint32_t> w, h, step, first(which.size() + 1);
    std::vector<uint8_t> buf;
    detail::packMats(sheets, which, cn, buf, off, w, h, step);
    std::vector<int32_t> quads(4 * 64 * which.size());
    int rc = cbh_demosaic(buf.data(), buf.size(), which.size(), off.data(), w.data(), h.data(), step.data(), cn, &p,
                          quads.data(), quads.size() / 4, first.data(), hashDevice());
    if (rc == CBH_E_OVERFLOW) {  // first[n] is the count it takes
      quads.resize(4 * size_t(first.back()));
      rc = cbh_demosaic(buf.data(), buf.size(), which.size(), off.data(), w.data(), h.data(), step.data(), cn, &p,
                        quads.data(), quads.size() / 4, first.data(), hashDevice());
    }
    if (rc) qFatal("gpuDemosaicHough: %s (%s)", cbh_strerror(rc), cbh_last_error());
    for (size_t k = 0; k < which.size(); ++k)
      for (uint32_t r = first[k]; r < first[k + 1]; ++r)
        rects[which[k]].append({quads[4 * r], quads[4 * r + 1], quads[4 * r + 2], quads[4 * r + 3]});
  }
}

// one sheet, as -select-grid calls it (src/main.cpp:1320)
template <class Params, class Rects>
inline void gpuDemosaicHough(const cv::Mat& cvImg, Rects& rects, const Params& params) {
  std::vector<Rects> all(1);
  gpuDemosaicHough(std::vector<cv::Mat>(1, cvImg), all, params);
  rects = all[0];
}

}  // namespace cbird_gpu
