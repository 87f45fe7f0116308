/* cbird_hip.h -- C-ABI of libcbird_hip.so: cbird's perceptual-hash build + Hamming find hot
 * path on AMD MI355X (gfx950 / CDNA4).
 *
 * This is the drop-in boundary: plain pointers and sizes only, no C++/torch/Qt types.  Each
 * entry point names the reference interface it replaces (paths relative to the cbird source
 * tree, v0.8.1).  A cbird maintainer binds these from a thin `Index` subclass -- see
 * INTEGRATION.md and cbird_amd/cpp/gpu_dcthashindex.h.
 *
 * Conventions
 *  - return 0 (CBH_OK) or a negative CBH_E_* code; nothing aborts, nothing throws.
 *  - the caller owns every buffer it passes; the library copies what it keeps.
 *  - "host" entry points take host pointers and perform the transfers themselves;
 *    "*_dev" entry points take device pointers (hipMalloc'ed memory of the index's device)
 *    and enqueue on `stream` (a hipStream_t passed as void*; NULL = the library's stream for
 *    that call, synchronised before return).
 *  - find/find_batch/scan may be called concurrently from many host threads on one index
 *    (cbird calls Index::find from QThreadPool workers under a read lock,
 *    src/database.cpp:1400-1432,1698); load/add/remove/destroy need exclusive access
 *    (cbird holds the write lock there, src/database.cpp:371,544,1673).
 *  - there is NO CPU fallback: without a usable gfx950 device every compute entry point
 *    returns CBH_E_NODEVICE.
 */
#ifndef CBIRD_HIP_H
#define CBIRD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CBH_VERSION 100 /* 0.1.0 */

enum {
  CBH_OK = 0,
  CBH_E_INVAL = -1,       /* bad argument */
  CBH_E_UNSUPPORTED = -2, /* valid in cbird, not implemented by this build (e.g. image size) */
  CBH_E_NODEVICE = -3,    /* no HIP device / kernel image not loadable */
  CBH_E_NOMEM = -4,       /* host or device allocation failed */
  CBH_E_HIP = -5,         /* HIP runtime error, see cbh_last_error() */
  CBH_E_OVERFLOW = -6,    /* result does not fit the record buffer; see cbh_idx64_set_record_capacity */
  CBH_E_NOTLOADED = -7    /* index used before load (src/index.h:233-237) */
};

/* Index::Match without the MatchRange (src/index.h:157-166); score = Hamming distance. */
typedef struct cbh_match {
  uint32_t id;   /* mediaId */
  int32_t score; /* lower is better */
} cbh_match;

/* Raw scan record, one per (query, haystack entry) pair under threshold:
 *   bits 63..39  query index within the call (< 2^25)
 *   bits 38..32  Hamming distance (0..64)
 *   bits 31..0   mediaId
 * so that an ascending u64 sort yields cbird's order: query, then score, then mediaId. */
typedef uint64_t cbh_record;
#define CBH_REC_QUERY(r) ((uint32_t)((r) >> 39))
#define CBH_REC_DIST(r) ((int)(((r) >> 32) & 0x7f))
#define CBH_REC_ID(r) ((uint32_t)((r)&0xffffffffu))
#define CBH_MAX_QUERIES_PER_CALL (1u << 25)

typedef struct cbh_idx64 cbh_idx64; /* opaque: DctHashIndex state on one device */
typedef struct cbh_idx256 cbh_idx256; /* opaque: CvFeaturesIndex state */

/* ---- library ------------------------------------------------------------------------- */
int cbh_version(void);
int cbh_device_count(void);             /* number of usable gfx950 devices, 0 if none */
/* bit d set for every HIP ordinal d < 32 that is a usable gfx950 device (the ordinals need not be contiguous: a node
 * may list another device first) -- what GpuDeviceSet::all() / cbh_idx64_create_sharded take */
uint32_t cbh_usable_device_mask(void);
const char* cbh_strerror(int code);     /* static string */
const char* cbh_last_error(void);       /* thread-local detail of the last failure (HIP call and reason) */
/* the CBH_E_* that goes with cbh_last_error() -- for the entry points that return a handle (create / slice): NULL
 * says "failed", this says whether it was CBH_E_NOMEM (transient: cbh_trim and try again) or something else */
int cbh_last_error_code(void);
/* Forget the thread's last error (text and code).  The entry points that return a handle do this themselves on entry;
 * a caller that decides on cbh_last_error_code() after an int-returning call (the adapters' retry-after-trim rule,
 * cbird_amd/cpp/gpu_errors.h) clears first so that the code it reads belongs to that call. */
void cbh_clear_error(void);
/* Scratch memory.  Kernel scratch comes from the library's own stream-ordered arena: hipMalloc'ed blocks cached per
 * (device, stream) -- a freed block is reused only by the stream that freed it, so the next call on that stream finds
 * its buffers mapped.  A stream's cache lives as long as the stream: when the library destroys one of its own streams,
 * or finds a caller's stream gone or idle while more than 32 streams have caches, the blocks move to a per-device
 * list any stream may take from, of which at most "pool_keep_mb" (default 16384) stay cached; a live stream's own
 * cache holds at most "pool_live_keep_mb" (default: a quarter of the device's memory).  cbh_trim synchronises
 * `device` and returns EVERY cached block to the driver; *released_bytes (optional) = what that gave back.  Safe to
 * call at any time between calls. */
int cbh_trim(int device, unsigned long long* released_bytes);

/* ---- hash build: replaces dctHash64(const cv::Mat&, bool) -- src/cvutil.cpp:435-545,
 * called once per image from Scanner::processImage (src/scanner.cpp:862).
 * imgs: n 8-bit single-channel images (cv::Mat CV_8UC1 after grayscale()), image i at
 * imgs + i*img_stride, row y at + y*row_stride.  Supported geometry: 1 <= w,h <= 8192 (cv::resize INTER_AREA's
 * integer-ratio and weighted paths; with a side < 32 its bilinear emulation for enlarging axes); larger:
 * CBH_E_UNSUPPORTED.  out[i] = 64-bit hash (bit 0 clear unless the hash would be 0 -> 1). */
int cbh_dcthash_batch(const uint8_t* imgs, size_t n, int w, int h, size_t row_stride,
                      size_t img_stride, uint64_t* out, int device);
int cbh_dcthash_batch_dev(const void* d_imgs, size_t n, int w, int h, size_t row_stride,
                          size_t img_stride, void* d_out, int device, void* stream);

/* ---- keypoint hashes: replaces Media::makeKeyPointHashes(cvImg, keyPoints, outHashes) -- src/media.cpp:874-923,
 * called per image from Scanner::processImage (src/scanner.cpp:888) to produce the DctFeaturesIndex rows.
 * kp: (x, y, size) float triples = cv::KeyPoint::pt.x, pt.y, size; image i owns kp[3*kp_first[i] .. 3*kp_first[i+1]).
 * A keypoint becomes the square Rect(floor x, floor y, ceil size) when size >= 31 and it lies inside the image as
 * :887-894 tests; cbh_keypoint_rects is that rule alone (rects = x, y, s triples; returns their number).
 * Each square is hashed with dctHash64(sub, inPlace = true), in keypoint order: a blurred square is written back into
 * the image before the next (possibly overlapping) one is read, exactly like the reference's shared cv::Mat.
 * Images: 8-bit grey, image i at imgs + img_off[i], img_w[i] x img_h[i], rows img_row_stride[i] bytes apart (sizes may
 * differ per image; cbird scales to <= 400 px first, scanner.cpp:876).  out_first[i] = index of image i's first hash
 * (n + 1 entries; out_first[n] = total <= kp_first[n], the capacity out_hashes needs).  imgs_after (NULL or imgs_bytes
 * bytes) receives the images as the in-place blurs left them.  _dev: d_imgs is modified in place, d_out on the
 * device, the descriptor arrays on the host; the call returns when the hashes are complete. */
long long cbh_keypoint_rects(int cols, int rows, const float* kp, size_t nkp, int32_t* rects);
/* The building block of the above, also the drop-in for dctHash64(view, inPlace) on arbitrary sub-rectangle views
 * (cvImg.colRange(..).rowRange(..), src/media.cpp:908-910): rects = (x, y, w, h) int32 quadruples, image i owns
 * rects[4*rect_first[i] .. 4*rect_first[i+1]) (rect_first[0] = 0), hashed in that order; out_hashes[j] belongs to
 * rectangle j.  The blur takes the pixels around a rectangle from the parent image, as cv::blur does on a view.
 * in_place != 0: each blurred rectangle is written back before the next is read (inPlace = true); 0: the image is
 * left alone (inPlace = false on an 8UC1 view copies). */
int cbh_dcthash_rects(const uint8_t* imgs, size_t imgs_bytes, size_t n, const uint64_t* img_off,
                      const uint32_t* img_w, const uint32_t* img_h, const uint32_t* img_row_stride,
                      const int32_t* rects, const uint32_t* rect_first, int in_place, uint64_t* out_hashes,
                      uint8_t* imgs_after, int device);
int cbh_keypoint_hashes(const uint8_t* imgs, size_t imgs_bytes, size_t n, const uint64_t* img_off,
                        const uint32_t* img_w, const uint32_t* img_h, const uint32_t* img_row_stride,
                        const float* kp, const uint32_t* kp_first, uint64_t* out_hashes, uint32_t* out_first,
                        uint8_t* imgs_after, int device);
int cbh_keypoint_hashes_dev(void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                            const uint32_t* img_h, const uint32_t* img_row_stride, const float* kp,
                            const uint32_t* kp_first, void* d_out, uint32_t* out_first, int device, void* stream);

/* ---- ORB keypoints and descriptors -- Media::makeKeyPoints / makeKeyPointDescriptors (src/media.cpp:859-872) ----
 * cbird configures OpenCV 2.4's ORB as OrbFeatureDetector(numKeyPoints, 1.2f, 12, 31, 0, 2, HARRIS_SCORE, 31) and a
 * default OrbDescriptorExtractor (256-bit rBRIEF): 12-level pyramid at 1.2 (cv::resize INTER_LINEAR), FAST-9/16
 * (threshold 20, 3x3 non-maximum suppression), the 31-pixel border, retainBest(2N) on the FAST score, Harris response
 * (7x7, k 0.04), retainBest(N), intensity-centroid orientation (cv::fastAtan2), 7x7 sigma-2 Gaussian, rotated test
 * pairs.  n grey images of any sizes in one buffer (image i: img_w[i] x img_h[i] at byte img_off[i], pitch
 * img_row_stride[i]; cbird feeds <= 400 px on the longest side, src/scanner.cpp:876).
 *   kp[i*kp_cap + j]       j-th keypoint of image i as detect() returns it: pyramid level by level, inside a level in
 *                          the retainBest order selected below; x, y in image coordinates, size = 31 * 1.2^octave,
 *                          angle in degrees
 *   kp_after[2*(i*kp_cap+j)]  (optional) the keypoint's x, y as compute() leaves them in cbird's non-const list
 *                          (pt * (1/scale) * scale): what Media::makeKeyPointHashes sees when both algorithms run
 *   desc[(i*kp_cap+j)*32]  (optional) its descriptor row, the layout CvFeaturesIndex stores
 *   counts[i]              keypoints found for image i; only the first kp_cap are written -- a count above kp_cap
 *                          means the call must be repeated with more room (ties at a cut can be kept: see below)
 * Two things depend on what the cbird binary was built with and are stated in oracle/orb_oracle.c.
 * (1) KeyPointsFilter::retainBest is std::nth_element + std::partition: which of several keypoints with EQUAL response
 * survive a cut, and the ORDER of the survivors, follow from the C++ library.  cbh_set_tuning("orb_retain_order", v):
 *   1 (default)  what libstdc++ (the Linux builds' library) leaves: its introselect and partition restated on the
 *                device and checked against the real std::nth_element (oracle/retain_stl.cpp);
 *   0            canonical: every keypoint whose response is >= the n-th best is kept, raster order inside a level
 *                (a superset of what any library leaves).
 * cbh_orb_retain_best_dev is that one step on its own: count float responses in device memory -> d_order (uint32, room
 * for count) = the original positions of the survivors of retainBest(n_points) in the order they are left, *d_count =
 * how many.  depth_limit < 0 is nth_element's own 2 * lg(count); >= 0 enters the selection with that limit (its
 * heap-select branch, which only adversarial orders reach).
 * (2) The 256 test pairs are a learned table inside OpenCV (bit_pattern_31_), an input here: cbh_orb_set_pattern(xy)
 * takes its 1024 integers (x0, y0, x1, y1 per bit, each within [-15, 15]).  Without a pattern a call that asks for
 * descriptors fails with CBH_E_INVAL; detection alone (desc == NULL) needs none. */
typedef struct cbh_keypoint {
  float x, y, size, angle, response;
  int32_t octave;
} cbh_keypoint;
int cbh_orb_set_pattern(const int8_t* xy);
int cbh_orb_retain_best_dev(const void* d_responses, uint32_t count, int n_points, int depth_limit, void* d_order,
                            void* d_count, int device, void* stream);
int cbh_orb(const uint8_t* imgs, size_t imgs_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w,
            const uint32_t* img_h, const uint32_t* img_row_stride, int nfeatures, int kp_cap, cbh_keypoint* kp,
            float* kp_after, uint8_t* desc, uint32_t* counts, int device);
/* Media::makeKeyPointDescriptors alone (src/media.cpp:868-872), on keypoints the caller provides -- ORB::operator()
 * with useProvidedKeypoints: keypoints whose rounded position lies within 31 pixels of the image border are dropped,
 * the rest grouped by octave (order kept inside an octave), pt scaled to the level, described, scaled back.  Image i
 * provides kp[kp_first[i] .. kp_first[i+1]); out_kp / out_desc (room for kp_first[n] entries) receive what compute()
 * leaves in cbird's non-const keypoint list and the descriptor rows, image i owning [out_first[i], out_first[i+1]).
 * A keypoint whose octave has no pyramid level in its image, or whose patch leaves that level, is CBH_E_INVAL
 * (OpenCV would read outside the image). */
int cbh_orb_describe(const uint8_t* imgs, size_t imgs_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                     const uint32_t* img_h, const uint32_t* img_row_stride, const cbh_keypoint* kp,
                     const uint32_t* kp_first, cbh_keypoint* out_kp, uint8_t* out_desc, uint32_t* out_first, int device);
/* images and outputs in device memory (the size arrays stay on the host); stream NULL = synchronous */
int cbh_orb_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                const uint32_t* img_row_stride, int nfeatures, int kp_cap, void* d_kp, void* d_kp_after, void* d_desc,
                void* d_counts, int device, void* stream);

/* ---- ColorDescriptor::create (src/cvutil.cpp:790-1099) for a batch of 8-bit BGR (channels 3) or BGRA (4) images --
 * sizeLongestSide(rgb, 256, INTER_NEAREST) when a side exceeds 256; the elliptic centre mask (cv::ellipse of 0.9 x the
 * image, pix * alpha >> 8); float BGR -> Luv (cv::cvtColor's spline tables); samples with l > 4; cv::kmeans(K = 32,
 * TermCriteria(ITER|EPS, 100, 10), 1 attempt, KMEANS_PP_CENTERS); per quantised centre colour the sum of
 * (maxDist - dist) / maxDist over its pixels; colours by descending frequency; w = int(freq * 65535 / maxFreq);
 * numColors = index of the last colour (as the reference writes it).  descs: n x 258 bytes (32 x {l, u, v, w : u16},
 * numColors : u8, pad) -- the record ColorDescIndex stores; ok[i] = 0 where the reference returns without touching the
 * descriptor ("not enough colors": fewer than 32 samples), the record is then all zero.
 * Three things cannot match the cbird binary by its own construction (oracle/colordesc_oracle.c): kmeans draws from the
 * worker thread's never-reseeded cv::theRNG() -- here every image starts from a fresh thread's state; equal frequencies
 * are ordered by key; the rim of the ellipse is OpenCV's polygon fill as recalled.
 * The _dev call returns when the descriptors are complete (it synchronises the stream). */
void cbh_color_descriptor_dims(int w, int h, int* cols, int* rows);      /* the working size after the resize */
int cbh_color_ellipse_mask(int cols, int rows, uint8_t* mask);           /* the mask itself (cols x rows bytes) */
int cbh_color_descriptors(const uint8_t* imgs, size_t imgs_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                          const uint32_t* img_h, const uint32_t* img_row_stride, int channels, uint8_t* descs, uint8_t* ok,
                          int device);
int cbh_color_descriptors_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                              const uint32_t* img_h, const uint32_t* img_row_stride, int channels, void* d_descs,
                              void* d_ok, int device, void* stream);

/* ---- qualityScore(const Media&) (src/cimgops.cpp:313-596) for a ragged batch of 8-bit images -------------------
 * The no-reference score the result browser shows per group member (src/gui/mediagrouplistwidget.cpp:1433-1441).
 * Images in cv::Mat order, channels 1 (the byte itself), 3 (BGR) or 4 (BGRA, alpha ignored): only the RED channel
 * takes part -- src.crop(.., 0, 0, .., 0, 0) keeps channel 0 of qImageToCImg's r, g, b planes (:335, :154-167) and
 * get_norm(1) of one channel is its absolute value (:344).  The crop hCrop = int(w * 0.10), vCrop = int(h * 0.10) is
 * inclusive: the working plane is (w - 2 hCrop + 1) x (h - 2 vCrop + 1), and with a crop of 0 its last column / row
 * lies outside the image and is 0 (:332-335).  hd = |p(x-1) - p(x+1)| inside each row (makeDiff, :37-60),
 * hMean = float(double(sum hd) / ((qw-1) * (qh-1))) (filterHorizontalMT, :252), hE = the local maxima along x of
 * hd > uint8(hMean) ? hd : 0 (makeEdge, :88-121); vd, vMean, vE the same along y.  h_long = runs of hE along y,
 * v_long = runs of vE along x, counted where a zero ends a run longer than 1 at positions 3 .. L-2 of the line
 * (longEdgeCount on the transposed maps, :131-152, :264-270); num_edges = set pixels of hE | vE inside
 * [1, qw-2] x [1, qh-2] (:456-464).  score = int(100 * er + 100 * elr) in float, er = float(num_edges) /
 * ((qw-2) * (qh-2)), elr = float(v_long + h_long) / num_edges (:495, :500, :592).
 * INT32_MIN = no score: num_edges == 0 (the reference converts NaN), or a working plane below 3 x 3 (a source side of
 * 1: the reference overruns its buffers, :337); the detail record of the latter is all zero.  A mean above 255 (only
 * working planes three rows or columns high can reach one) keeps the low byte of its integer part. */
void cbh_quality_dims(int w, int h, int* qw, int* qh);   /* working size after the crop; 0 x 0 when below 3 x 3 */
typedef struct cbh_quality_detail {
  uint64_t h_sum, v_sum; float h_mean, v_mean;
  int32_t h_long, v_long, num_edges, qw, qh, score;
} cbh_quality_detail;
/* images in host memory, uploaded in pieces of at most "quality_chunk_mb" (cbh_set_tuning) */
int cbh_quality_scores(const uint8_t* imgs, size_t imgs_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                       const uint32_t* img_h, const uint32_t* img_row_stride, int channels, int32_t* scores,
                       cbh_quality_detail* detail /* NULL or n */, int device);
/* images and outputs in device memory (the size arrays stay on the host).  d_planes: NULL, or per image at plane_off[i]
 * three packed qw x qh byte planes -- hE | vE (0 / 255), hd, vd: the images qualityScore hands to addVisual (:430-432),
 * before its normalisation.  Returns when the scores are complete (it synchronises the stream). */
int cbh_quality_scores_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                           const uint32_t* img_h, const uint32_t* img_row_stride, int channels, void* d_scores,
                           void* d_detail /* NULL or n */, void* d_planes /* NULL or see above */,
                           const uint64_t* plane_off /* n, with d_planes */, int device, void* stream);

/* ---- brightnessAndContrastAuto (src/cvutil.cpp:578-665) and differenceImage (src/gui/mediagrouplistwidget.cpp:98-208) --
 * cbird_amd/csrc/diffimage.hip; tests/difference_rules.py is the numpy model the device is held to, bit for bit.  Images
 * as everywhere above: the img_off / img_w / img_h / img_row_stride host tables of cbh_warp_affine_dev, channels 1 / 3 =
 * BGR / 4 = BGRA, one channel count per call, sides 1 .. 32767, at most 2^20 images per call.  clip_pct >= 0, finite.
 *
 * EXACT restatements of the reference's own arithmetic: the cut rule (grayLevel, :578-626), the colour map (:173-206)
 * and the size rule (:153-161: which side is scaled).  UNPINNED, restated without the library they come from:
 *   - the stretch, Mat::convertTo(dst, -1, alpha, beta), as recalled from OpenCV 2.4.13: saturate_cast<uchar>(cvRound(
 *     float(s) * alpha + beta)) with a float32 multiply, a float32 add and round-half-to-even;
 *   - the aligned right image (QPainter::drawImage under QTransform::inverted): nearest neighbour at pixel centres in
 *     f64 where Qt's raster engine samples in 16.16 fixed point, and B = G = R = 0 where the right image does not cover
 *     the canvas, which the reference leaves uninitialised -- both are this library's definitions;
 *   - QImage::scaled(size): nearest neighbour, aspect ignored, src = ((2 * dst + 1) * ssize) / (2 * dsize) in integers.
 *
 * The cut rule on given counts, in host memory and without a device: hist = n x 256 counts, count[j] = pixels of grey
 * value j.  clip_pct == 0: the lowest and highest value present (256 / -1 when all counts are 0).  Otherwise acc[0] =
 * float(count[0]), acc[i] = acc[i-1] + float(count[i]) in float32, max = acc[255], clip = (clip_pct * (max / 100.0f)) /
 * 2.0f; min_gray = the first i with !(acc[i] < clip), 256 if none; max_gray = the last i with !(acc[i] >= max - clip),
 * -1 if none.  The device runs the same function. */
int cbh_gray_cuts(const uint32_t* hist, size_t n, float clip_pct, int32_t* min_gray, int32_t* max_gray);
/* brightnessAndContrastAuto(src, dst, clip_pct) per image.  The histogram is that of the grey view (a one-channel image
 * itself, cvtColor's fixed-point weights otherwise, alpha ignored); min_gray >= max_gray copies the image, otherwise
 * alpha = 255 / float(max_gray - min_gray), beta = -min_gray * alpha and EVERY byte of every channel, alpha included
 * (the reference's alpha restore is commented out, :647-653), goes through the stretch above.  UNPINNED: convertTo.
 * d_out: NULL, or a buffer of d_imgs' layout that receives the pixels' bytes (nothing between them is written; it may be
 * d_imgs); d_cuts: int32 2n, {min_gray, max_gray} per image; d_hist: NULL or u32 256 n.  Synchronises the stream. */
int cbh_auto_contrast_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                          const uint32_t* img_h, const uint32_t* img_row_stride, int channels, float clip_pct, void* d_out,
                          void* d_cuts, void* d_hist /* NULL or 256 n */, int device, void* stream);
/* the same from and to host memory; out: NULL or imgs_bytes bytes, the bytes between the images copied from imgs */
int cbh_auto_contrast(const uint8_t* imgs, size_t imgs_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                      const uint32_t* img_h, const uint32_t* img_row_stride, int channels, float clip_pct, uint8_t* out,
                      int32_t* cuts /* 2n */, uint32_t* hist /* NULL or 256 n */, int device);
/* differenceImage(left, right_i) for ONE left image (the needle or template) and n right images (the candidates).
 *  1. Both sides as RGB32: grey replicated into B, G, R; the alpha of BGRA dropped (not premultiplied), alpha = 255.
 *  2. Pair i is WARPED when tx != NULL, has_tx (NULL = all set) [i] != 0 and tx[6 * i ..], the 2 x 3 matrix template ->
 *     right image that cbh_template_result.tx holds, is not exactly the identity: the right image is redrawn on a canvas
 *     of the left image's size, canvas pixel (x, y) = the right image's pixel (sx, sy), sx = floor((a * (x + 0.5) + b *
 *     (y + 0.5)) + c) in f64 without fusing, sy from the second row; 0 outside.  A matrix whose determinant a * e - b * d
 *     is exactly 0 samples through the identity (QTransform::inverted returns it).  UNPINNED against Qt, see above.
 *  3. cbh_auto_contrast's rule with clip_pct (the reference passes 5) on the left image and on the aligned right image
 *     -- the zero fill of a canvas counts in its histogram, as in the reference.
 *  4. area(aligned right) < area(left): the right side is scaled to the left's size, else the left side to the right's
 *     (nearest neighbour as above; UNPINNED against QImage::scaled).
 *  5. Per pixel sum = dr^2 + dg^2 + db^2; r = ((sum >> 10) << 1) & 255 (it wraps above 131071, as qRgb masks it),
 *     g = ((sum >> 5) & 31) << 3, b = (sum & 31) << 3; the picture is BGRA, alpha 255.
 * cbh_difference_dims gives each pair's output size (and whether it is warped) for the caller to lay out out_off.  The
 * record has no counterpart in the reference: it ranks the pairs of a group without fetching n pictures. */
typedef struct cbh_diff_detail {
  uint64_t sum_total;                 /* sum over all output pixels */
  uint32_t sum_max, n_ge32, n_ge1024; /* the largest sum; pixels with green set ("noticeable") / red set ("obvious") */
  int32_t w, h, warped;               /* the output's size; 1 = the right image was redrawn through tx */
  int32_t left_min, left_max, right_min, right_max; /* the cuts of both sides */
} cbh_diff_detail;
int cbh_difference_dims(int left_w, int left_h, size_t n, const uint32_t* img_w, const uint32_t* img_h,
                        const double* tx /* NULL or 6n */, const uint8_t* has_tx /* NULL or n */, uint32_t* out_w,
                        uint32_t* out_h, uint8_t* warped /* NULL or n */);
/* images in device memory; the tables, tx and has_tx are host memory.  d_images: NULL (the record alone), or 16-byte
 * aligned, picture i packed (pitch 4 * w) at out_off[i], a multiple of 16; d_detail: NULL or n records.  Synchronises
 * the stream. */
int cbh_difference_images_dev(const void* d_left, int left_w, int left_h, size_t left_row_stride, int left_channels,
                              const void* d_rights, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                              const uint32_t* img_h, const uint32_t* img_row_stride, int channels, const double* tx,
                              const uint8_t* has_tx, float clip_pct, void* d_images, const uint64_t* out_off,
                              void* d_detail, int device, void* stream);
/* the same from and to host memory; images: NULL or images_bytes bytes of which only the pictures are written */
int cbh_difference_images(const uint8_t* left, int left_w, int left_h, size_t left_row_stride, int left_channels,
                          const uint8_t* rights, size_t rights_bytes, size_t n, const uint64_t* img_off,
                          const uint32_t* img_w, const uint32_t* img_h, const uint32_t* img_row_stride, int channels,
                          const double* tx, const uint8_t* has_tx, float clip_pct, uint8_t* images, size_t images_bytes,
                          const uint64_t* out_off, cbh_diff_detail* detail /* NULL or n */, int device);

/* ---- alignSpatially (src/gui/videocomparewidget.cpp:590-627) and alignTemporally with sad128 (:629-680) -------------------
 * cbird_amd/csrc/align.hip; tests/alignment_rules.py is the numpy model the device is held to, bit for bit (everything is
 * integer arithmetic).  Images as above: the img_off / img_w / img_h / img_row_stride host tables, channels 1 / 3 / 4, one
 * channel count per table, sides 1 .. 32767, at most 2^20 images per call.  The three bytes of a pixel are the grey byte
 * three times, the three bytes, or the first three of four (alpha ignored); their order does not matter to a sum.
 *
 * EXACT restatements of the reference's own arithmetic: the SAD windows, the scan order and the tie rules, the integer
 * mean and the start rule.  UNPINNED, as for the difference image: QImage::scaled(S, S) -- nearest neighbour, aspect
 * ignored, src = ((2 * dst + 1) * ssize) / (2 * dsize) in integers -- restated without Qt.
 *
 * Spatial, S = 256, ONE left image A against n right images B_i.  For xo = -8 .. 8 (outer loop) and yo = -8 .. 8 (inner):
 *   sad(xo, yo) = sum over y = 8 .. 247, x = 8 .. 247, c of |A[y + yo][x + xo][c] - B[y][x][c]|   (<= 44 064 000)
 * and the answer is the first shift in that order whose sad is strictly below every earlier one: on a tie the smaller
 * xo, then the smaller yo; (-8, -8) when all are equal.  The table is uint32 [n][289], entry (xo + 8) * 17 + (yo + 8).
 * The reference's _alignX, _alignY are min_x / 256.0f, min_y / 256.0f. */
typedef struct cbh_align_spatial_result {
  int32_t min_x, min_y;          /* the shift: left pixel (x + min_x, y + min_y) lies on right pixel (x, y) at 256 x 256 */
  uint32_t min_sad, sad_at_zero; /* its sad; the sad of (0, 0) */
} cbh_align_spatial_result;
/* images in device memory, the tables in host memory; d_results: n records; d_table: NULL or 289 n words.  n == 0
 * returns CBH_OK and touches nothing.  CBH_E_INVAL (with a cbh_last_error text): a side of 0 or above 32767, rows shorter
 * than their pixels, a channel count other than 1 / 3 / 4, n above 2^20.  Synchronises the stream. */
int cbh_align_spatial_dev(const void* d_left, int left_w, int left_h, size_t left_row_stride, int left_channels,
                          const void* d_rights, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                          const uint32_t* img_h, const uint32_t* img_row_stride, int channels, void* d_results,
                          void* d_table /* NULL or 289 n */, int device, void* stream);
/* the same from and to host memory */
int cbh_align_spatial(const uint8_t* left, int left_w, int left_h, size_t left_row_stride, int left_channels,
                      const uint8_t* rights, size_t rights_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                      const uint32_t* img_h, const uint32_t* img_row_stride, int channels, cbh_align_spatial_result* results,
                      uint32_t* table /* NULL or 289 n */, int device);
/* Temporal, S = 128: left frames F_0 .. F_{nL-1} against the window of right frames G_0 .. G_{W-1}, 1 <= W <= 64,
 * W <= nL <= 65535, P = nL - W + 1 placements.  cell(d, i) = the SAD of all 128 * 128 * 3 bytes of F_{d+i} and G_i
 * (<= 12 533 760); mean(d) = (sum over i of cell(d, i)) / W in integer division.  With start in [0, P): best = start,
 * min = mean(start); then for d = 0 .. P - 1 ascending, mean(d) < min replaces both -- a placement that only equals the
 * start's mean never wins, among equal better ones the earliest does.  The reference's call is nL = 64, W = 5, start = 30:
 * offsets -30 .. +29 around the current frame.  Which frame stands in for an index outside the video is the caller's
 * business (FrameCache's in the reference). */
typedef struct cbh_align_temporal_result {
  int32_t placement, offset;     /* the placement kept; placement - start */
  uint32_t min_mean, start_mean; /* its mean; the mean at start */
} cbh_align_temporal_result;
/* frames in device memory, the tables in host memory, one channel count per side; d_result: one record; d_means: NULL or
 * P words; d_cells: NULL or P * W words, cell(d, i) at d * W + i.  CBH_E_INVAL (with a cbh_last_error text): as above, W
 * outside 1 .. 64, W > nL, nL above 65535, start outside [0, P).  Synchronises the stream. */
int cbh_align_temporal_dev(const void* d_left, size_t n_left, const uint64_t* left_off, const uint32_t* left_w,
                           const uint32_t* left_h, const uint32_t* left_row_stride, int left_channels, const void* d_right,
                           size_t n_right, const uint64_t* right_off, const uint32_t* right_w, const uint32_t* right_h,
                           const uint32_t* right_row_stride, int right_channels, int start, void* d_result,
                           void* d_means /* NULL or P */, void* d_cells /* NULL or P * W */, int device, void* stream);
/* the same from and to host memory */
int cbh_align_temporal(const uint8_t* left, size_t left_bytes, size_t n_left, const uint64_t* left_off, const uint32_t* left_w,
                       const uint32_t* left_h, const uint32_t* left_row_stride, int left_channels, const uint8_t* right,
                       size_t right_bytes, size_t n_right, const uint64_t* right_off, const uint32_t* right_w,
                       const uint32_t* right_h, const uint32_t* right_row_stride, int right_channels, int start,
                       cbh_align_temporal_result* result, uint32_t* means /* NULL or P */,
                       uint32_t* cells /* NULL or P * W */, int device);

/* ---- demosaicHough (src/cvutil.cpp:1445-1688; -select-grid, src/main.cpp:1310-1332): contact sheets into tiles ------------
 * cbird_amd/csrc/demosaic.hip; tests/demosaic_rules.py is the numpy model the device is held to, bit for bit.  Images as
 * above: the img_off / img_w / img_h / img_row_stride host tables, channels 1 / 3 = BGR / 4 = BGRA, one channel count per
 * call, sides 1 .. 32767, at most 2^20 images per call.  The working planes take two bytes per pixel of the batch.
 *
 * EXACT restatements of the reference's own arithmetic: the thresholds, the angle test, selectLines, the rectangles and the
 * subdivision.  UNPINNED, restated as recalled from OpenCV 2.4.13 without the library: GaussianBlur, Canny, HoughLines
 * (and convertTo inside step 1, as for cbh_auto_contrast).  Per image:
 *  1. adjusted = brightnessAndContrastAuto(img, clip_pct) (cbh_auto_contrast's rule), g = the grey view of adjusted (a
 *     one-channel image itself, cvtColor's fixed-point weights otherwise, alpha ignored).
 *  2. pre_blur == 3: g through the 3 x 3 Gaussian on bytes, weights (1,2,1) x (1,2,1), border REFLECT_101 (a 1-pixel side
 *     reflects onto itself): out = (S + 8) >> 4, S the weighted sum of the nine bytes.  0 skips it; other values are
 *     CBH_E_UNSUPPORTED.  UNPINNED.
 *  3. Canny(g, canny1, canny2), aperture 3, L1 norm: low = min, high = max of the two.  dx, dy = the 3 x 3 Sobel as
 *     integers, border REPLICATE; m = |dx| + |dy|, 0 outside the image.  A pixel is a CANDIDATE when m > low and it passes
 *     the suppression: with x = |dx|, y = |dy| << 15, t22 = x * 13573, t67 = t22 + (x << 16): y < t22 needs m > m(left)
 *     && m >= m(right); otherwise y > t67 needs m > m(up) && m >= m(down); otherwise, with s = ((dx ^ dy) < 0) ? -1 : 1,
 *     m > m(up, x - s) && m > m(down, x + s).  A candidate with m > high is STRONG.  edges = 255 on every candidate that is
 *     8-connected, through candidates, to a strong pixel, 0 elsewhere.  UNPINNED.
 *  4. post_blur == 3: the same Gaussian on edges.
 *  5. HoughLines(edges, rho 0.5, theta 45 degrees, threshold), the standard transform; other rho / theta are
 *     CBH_E_UNSUPPORTED.  numrho = 4 (w + h) + 2; theta = float(45 pi / 180), the four angles accumulated in float32,
 *     tabCos[n] = float(cos(double(ang_n)) * 2), tabSin likewise; a non-zero pixel (row i, column j) votes at r =
 *     rint_half_even(float(j * tabCos[n]) + float(i * tabSin[n])) + (numrho - 1) / 2, float32 and unfused.  Bin (n, r) is a
 *     line when acc > threshold, acc > acc(n, r-1), acc >= acc(n, r+1), acc > acc(n-1, r), acc >= acc(n+1, r), missing
 *     neighbours counting 0; its position is int(rho), rho = (float(r) - (numrho - 1) * 0.5f) * 0.5f.  The reference's angle
 *     test keeps n = 2 as horizontal (threshold int(float(w) * factor)) and n = 0 as vertical (int(float(h) * factor)):
 *     a row i with enough non-zero pixels gives y = i - 1 (0 for row 0), likewise columns; the diagonals only take part
 *     as neighbours.  y is kept when h_margin <= y < h - h_margin, x when v_margin <= x < w - v_margin.  factor =
 *     hough_thresh_factor for an image, 0.95f for every subdivision.  UNPINNED.
 *  6. selectLines (:1552-1617) on the positions with 0 and the side appended, sorted, duplicates kept; the loops as they
 *     stand, `s > img.cols` bounding both directions included.  Host code.
 *  7. An empty grid becomes {0, side}.  Fewer than 3 lines both ways: one rectangle, the whole image.  Otherwise the
 *     cells row by row, each shrunk by crop_margin on every side (a side may come out below 1, as in the reference).
 *  8. With at least 2 rectangles, each whose float(w) / float(h) is above max_aspect or below min_aspect goes through
 *     steps 1-8 again as an image of its own (a view of the ORIGINAL pixels, its own histogram and borders) and is
 *     replaced by the answer, offset by its origin.  The reference would assert or throw on a rectangle with a side below
 *     1 or one that leaves its image, and would recurse without end on one that is its whole image; this library does
 *     not subdivide any of them.  One batched pass per level of subdivision.
 * crop_margin < 0 and min_grid_spacing < 1 are CBH_E_INVAL: with them the cells of step 7 leave their image, or
 * selectLines pairs a line with itself.  The other integer fields take any value. */
typedef struct cbh_demosaic_params {
  float clip_pct;                                        /* clipHistogramPercent 10 */
  int32_t pre_blur, canny1, canny2, post_blur;           /* 3, 50, 0, 3 */
  int32_t h_margin, v_margin;                            /* 0, 0 */
  float hough_rho, hough_theta, hough_thresh_factor;     /* 0.5, 45, 0.8 */
  int32_t min_grid_spacing, grid_tolerance, crop_margin; /* 96, 4, 2 */
  float max_aspect, min_aspect;                          /* 2.5, 0.5 */
} cbh_demosaic_params;
void cbh_demosaic_default_params(cbh_demosaic_params* p);
/* Step 6 on one list, host code, no device: lines = n_lines positions in 0 .. side, in any order; 0 and side are appended.
 * cols = the image's width for both directions.  grid: room for n_lines + 2 entries; *n_grid = how many were written. */
int cbh_grid_select(const int32_t* lines, size_t n_lines, int side, int cols, int min_grid_spacing, int grid_tolerance,
                    int32_t* grid, size_t* n_grid);
/* Step 7, host code, no device: rects = (x, y, w, h) quadruples, row by row.  *n_rects = how many there are;
 * CBH_E_OVERFLOW with nothing written when that is above rects_cap. */
int cbh_grid_rects(const int32_t* hgrid, size_t n_h, const int32_t* vgrid, size_t n_v, int w, int h, int crop_margin,
                   int32_t* rects, size_t rects_cap, size_t* n_rects);
/* Steps 1-4 of every image, no subdivision.  d_edges: the edge maps, image i packed (rows of img_w[i] bytes) behind
 * image i - 1; d_classes: NULL, or in the same layout the classes before the hysteresis (0 none, 1 candidate, 2 strong);
 * passes: NULL, or a host word that receives the number of hysteresis launches.  Synchronises the stream. */
int cbh_edge_maps_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                      const uint32_t* img_row_stride, int channels, const cbh_demosaic_params* params, void* d_edges,
                      void* d_classes, uint32_t* passes, int device, void* stream);
/* Steps 1-5 of every image with factor = hough_thresh_factor: the positions in host memory, ascending, duplicates kept;
 * image i owns hor[hor_first[i] .. hor_first[i+1]) and ver likewise (n + 1 entries each).  hor needs room for the sum of
 * img_h entries, ver for the sum of img_w. */
int cbh_grid_lines_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                       const uint32_t* img_row_stride, int channels, const cbh_demosaic_params* params, int32_t* hor,
                       uint32_t* hor_first, int32_t* ver, uint32_t* ver_first, int device, void* stream);
/* demosaicHough of every image.  rects (host memory) = (x, y, w, h) int32 quadruples in the reference's order, image i
 * owns rects[4 * rect_first[i] .. 4 * rect_first[i+1]) as cbh_dcthash_rects takes them; rect_first has n + 1 entries.
 * CBH_E_OVERFLOW with rect_first complete and nothing written to rects when rect_first[n] > rects_cap.  n == 0 returns
 * CBH_OK.  CBH_E_INVAL (with a cbh_last_error text): a side of 0 or above 32767, rows shorter than their pixels, a channel
 * count other than 1 / 3 / 4, n above 2^20, clip_pct negative or not finite, crop_margin negative, min_grid_spacing below 1.
 * Synchronises the stream after every hysteresis launch and at the end. */
int cbh_demosaic_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                     const uint32_t* img_row_stride, int channels, const cbh_demosaic_params* params, int32_t* rects,
                     size_t rects_cap, uint32_t* rect_first, int device, void* stream);
/* the same from host memory */
int cbh_demosaic(const uint8_t* imgs, size_t imgs_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                 const uint32_t* img_h, const uint32_t* img_row_stride, int channels, const cbh_demosaic_params* params,
                 int32_t* rects, size_t rects_cap, uint32_t* rect_first, int device);

/* ---- the steps in front of dctHash64 in Scanner::processImage (src/scanner.cpp:852-862) -------------------
 * grayscale(): cv::cvtColor(BGR2GRAY/BGRA2GRAY) on 8-bit data (src/cvutil.cpp:1265-1283); d_gray is packed
 * n*w*h bytes. */
int cbh_bgr2gray_dev(const void* d_src, size_t n, int w, int h, size_t row_stride, size_t img_stride,
                     int channels, void* d_gray, int device, void* stream);
/* The grey planes of the reflected images a reflection search processes (SearchParams::mirrorMask, src/index.h:51-59;
 * Engine::mirrored, src/engine.cpp:357-365: QImage::mirrored(h, v)), all from one read of each image.  mirror_mask: bit
 * 1 left-right, 2 top-bottom, 4 both (0..7, else CBH_E_INVAL); V = 1 + popcount(mirror_mask).  d_gray: n*V packed
 * planes of w*h, plane i*V + v, the views of image i in the order identity, 1, 2, 4 (the set bits); each plane equals
 * cbh_bgr2gray_dev of the reflected image (channels 1: the reflected bytes).  d_color: NULL, or n*(V-1) packed images of
 * w*h*channels bytes (row stride w*channels), image i*(V-1) + v-1 = the reflected colour image of view v >= 1 -- what
 * ColorDescriptor::create reads for that view; the identity view is the input itself.  Channels 1 / 3 / 4. */
int cbh_gray_views_dev(const void* d_src, size_t n, int w, int h, size_t row_stride, size_t img_stride, int channels,
                       int mirror_mask, void* d_gray, void* d_color, int device, void* stream);
/* The views that swap width and height, the other four symmetries of a rectangle, from one read of each image.
 * turn_mask: bit 8 quarter turn clockwise (QTransform().rotate(90): out[y][x] = in[h-1-x][y]), 16 quarter turn
 * counter-clockwise (in[x][w-1-y]), 32 transpose (in[x][y]), 64 anti-transpose (in[h-1-x][w-1-y]); bits 8 / 16 / 32 / 64
 * only, at least one (else CBH_E_INVAL); T = popcount.  d_gray: n*T packed planes of w rows x h columns, plane i*T + t,
 * set bits in rising order; each equals cbh_bgr2gray_dev of the turned image (channels 1: the turned bytes).
 * d_color: NULL, or n*T packed images of w x h x channels, the turned colour images.  Channels 1 / 3 / 4. */
int cbh_turn_views_dev(const void* d_src, size_t n, int w, int h, size_t row_stride, size_t img_stride, int channels,
                       int turn_mask, void* d_gray, void* d_color, int device, void* stream);
/* autocrop(gray, range) (src/cvutil.cpp:1285-1402): d_rects[i] = {left, top, right, bottom} (int32 x4) of the
 * region kept (the whole image when nothing is cropped). */
int cbh_autocrop_dev(const void* d_gray, size_t n, int w, int h, size_t row_stride, size_t img_stride, int range,
                     void* d_rects, int device, void* stream);
/* processImage's hash for n decoded images of one size in host memory: grayscale (channels 1/3/4) ->
 * autocrop when autocrop_range >= 0 (cbird uses 20) -> dctHash64 of the kept region.  autocrop() leaves cvGray as a
 * colRange/rowRange VIEW of the full image (src/cvutil.cpp:1397-1401), so -- as with any cv::Mat view -- the blur inside
 * dctHash64 still reads the cropped-away margins at the view's edges; the same is done here.  rects may be NULL. */
int cbh_process_images(const uint8_t* imgs, size_t n, int w, int h, size_t row_stride, size_t img_stride,
                       int channels, int autocrop_range, uint64_t* out, int32_t* rects, int device);
/* The same, and from the same upload the image processImage hands to ORB next: sizeLongestSide(cvGray, resize_size) of
 * the (autocropped) grey image (src/scanner.cpp:876; cbird: 400).  resized = n slots of resize_size^2 bytes, image i
 * packed (pitch = its width) at the start of slot i with the size resized_dims[2i] x resized_dims[2i+1] (0 x 0 where
 * the reference's sizeLongestSide throws).  resize_size 0: exactly cbh_process_images. */
int cbh_process_images_ex(const uint8_t* imgs, size_t n, int w, int h, size_t row_stride, size_t img_stride,
                          int channels, int autocrop_range, uint64_t* out, int32_t* rects, int resize_size,
                          uint8_t* resized, int32_t* resized_dims, int device);

/* ---- Scanner::processImage for a batch (src/scanner.cpp:828-895): every feature stage of one image, chained on the
 * device from ONE upload: grayscale -> autocrop -> dctHash64 of the kept region; ColorDescriptor::create of the colour
 * image; sizeLongestSide(kept region, resize_longest_side); makeKeyPoints; makeKeyPointDescriptors; makeKeyPointHashes
 * on the keypoints as compute() left them.  n decoded images of one geometry in host memory (channels 1 / 3 / 4).
 * algos = IndexParams::algos, bit (1 << SearchParams::Algo*): 1 dct, 2 dct features (keypoint hashes), 4 cv features
 * (ORB descriptors; needs cbh_orb_set_pattern), 8 colour.  Outputs of stages that are switched off may be NULL.
 *   dct_hashes[n], rects[4n] (kept region: left, top, right, bottom), resized_dims[2n] (0 x 0: the reference throws,
 *   no features); kp_counts[n] (found; at most kp_cap are written), kp[n * kp_cap] (the keypoint list as processImage
 *   holds it at the end), desc[n * kp_cap * 32]; kph_counts[n], kp_hashes[n * kp_cap]; color_descs[n * 258],
 *   color_ok[n]. */
typedef struct cbh_index_params {
  int autocrop_range;       /* cbird: 20; < 0: no autocrop (IndexParams::autocrop = false) */
  int algos;                /* IndexParams::algos */
  int resize_longest_side;  /* IndexParams::resizeLongestSide = 400 */
  int num_features;         /* IndexParams::numFeatures = 400 */
  int kp_cap;               /* room per image in kp / desc / kp_hashes */
} cbh_index_params;
int cbh_index_images(const uint8_t* imgs, size_t n, int w, int h, size_t row_stride, size_t img_stride, int channels,
                     const cbh_index_params* p, uint64_t* dct_hashes, int32_t* rects, int32_t* resized_dims,
                     uint32_t* kp_counts, cbh_keypoint* kp, uint8_t* desc, uint32_t* kph_counts, uint64_t* kp_hashes,
                     uint8_t* color_descs, uint8_t* color_ok, int device);
/* cbh_index_images for a reflection search: Engine::query (src/engine.cpp:423-436) runs processImage again on the needle
 * mirrored left-right, top-bottom and both ways (Engine::mirrored, :357-365) for the bits of SearchParams::mirrorMask.
 * Each chunk of images is uploaded once; cbh_gray_views_dev makes the grey (and, with the colour leg, colour) images of
 * the V = 1 + popcount(mirror_mask) views and the stages run on all of them.  Every output array is sized for n*V results,
 * result i*V + v = view v of image i (views in the order identity, 1, 2, 4), each exactly what cbh_index_images gives for
 * the reflected image (rects and keypoints in the coordinates of that view).  mirror_mask 0..7, else CBH_E_INVAL. */
int cbh_index_images_views(const uint8_t* imgs, size_t n, int w, int h, size_t row_stride, size_t img_stride,
                           int channels, int mirror_mask, const cbh_index_params* p, uint64_t* dct_hashes, int32_t* rects,
                           int32_t* resized_dims, uint32_t* kp_counts, cbh_keypoint* kp, uint8_t* desc,
                           uint32_t* kph_counts, uint64_t* kp_hashes, uint8_t* color_descs, uint8_t* color_ok, int device);
/* cbh_index_images_views for all eight views of an image: view_mask = the reflection bits 1 / 2 / 4 and the bits of
 * cbh_turn_views_dev, 8 / 16 / 32 / 64 (0..127, else CBH_E_INVAL); V = 1 + popcount(view_mask), views in the order
 * identity, then the set bits rising.  Every output array is sized n*V, row i*V + v = exactly what cbh_index_images
 * gives for view v of image i, rects / keypoints / resized dims in that view's own coordinates (turned views are h wide
 * and w high).  One upload per chunk; the stages after the grey step run once per geometry present. */
int cbh_index_images_views_ex(const uint8_t* imgs, size_t n, int w, int h, size_t row_stride, size_t img_stride,
                              int channels, int view_mask, const cbh_index_params* p, uint64_t* dct_hashes,
                              int32_t* rects, int32_t* resized_dims, uint32_t* kp_counts, cbh_keypoint* kp, uint8_t* desc,
                              uint32_t* kph_counts, uint64_t* kp_hashes, uint8_t* color_descs, uint8_t* color_ok,
                              int device);

/* sizeLongestSide(cv::Mat& img, int size, int filter = INTER_LANCZOS4) -- src/cvutil.cpp:1932-1950, the resize in
 * front of ORB detection (src/scanner.cpp:876, size = IndexParams::resizeLongestSide = 400): target size from the
 * float aspect ratio (cbh_longest_side_dims; a zero side is the reference's std::invalid_argument -> CBH_E_INVAL),
 * then cv::resize's 8-bit Lanczos-4 path.  n grey images of one geometry; out / d_dst: n packed out_w x out_h
 * images.  cbh_resize_lanczos4_dev resizes to any dw x dh. */
void cbh_longest_side_dims(int w, int h, int size, int* out_w, int* out_h);
int cbh_size_longest_side(const uint8_t* imgs, size_t n, int w, int h, size_t row_stride, size_t img_stride, int size,
                          uint8_t* out, int* out_w, int* out_h, int device);
int cbh_resize_lanczos4_dev(const void* d_src, size_t n, int w, int h, size_t row_stride, size_t img_stride, int dw,
                            int dh, void* d_dst, int device, void* stream);

/* Stage-level diagnostics: as cbh_dcthash_batch_dev, and additionally writes the 32x32 u8 tile
 * each image is reduced to after stages 1-2 (blur + INTER_AREA) to d_tiles[i*1024 ..]. */
int cbh_dcthash_tiles_dev(const void* d_imgs, size_t n, int w, int h, size_t row_stride,
                          size_t img_stride, void* d_out, void* d_tiles, int device, void* stream);

/* ---- DctHashIndex: src/dcthashindex.{h,cpp} -------------------------------------------- */
cbh_idx64* cbh_idx64_create(int device);                         /* DctHashIndex() :30-41 */
void cbh_idx64_destroy(cbh_idx64*);                              /* ~DctHashIndex/unload :43-54 */
/* ONE process, several GPUs.  cbird registers each Index once (src/engine.cpp:38-45) and fans find() out from its own
 * thread pool (src/database.cpp:1400-1432), so a drop-in that is to use every GPU of the node shards INSIDE the handle:
 * device_mask = bit d set for every HIP device d that takes a share (all must be usable gfx950 devices, else NULL);
 * shards_per_device >= 2 additionally cuts each device's share into that many logical shards with their own streams
 * (0 and 1 mean one).  The handle is a cbh_idx64 like any other: load/add/remove/find/find_batch/find_coalesced/slice/
 * search_index_batch, the fdct_* calls and cbh_vidx / cbh_color built on it all accept it and return what the
 * one-device index returns, bit for bit.  Rows are sharded in load order, shard s of R owning [s*n/R, (s+1)*n/R); add()
 * appends to the emptiest shard; needles are replicated; per search every shard scans its rows on its own device into
 * a { count, records } block, and the records meet on the first device of the mask, which alone consumes them: copies
 * of exactly count_s records per shard (device-to-device inside a device, hipMemcpyPeerAsync over xGMI between
 * devices), or -- cbh_set_tuning("shard_exchange", 0) -- ONE grouped ncclAllGather of the per-device blocks (librccl,
 * dlopen'ed on first use; an index that cannot get a communicator keeps using the copies and says so once in
 * cbh_last_error / stderr and in cbh_shard_stats.collective_fallbacks) (cbird_amd/csrc/sharded.hip).
 * The first device of the mask is the handle's device: *_dev calls take pointers on it. */
cbh_idx64* cbh_idx64_create_sharded(uint32_t device_mask, int shards_per_device);
uint32_t cbh_idx64_device_mask(const cbh_idx64*);   /* a plain index: 1 << device */
int cbh_idx64_shards_per_device(const cbh_idx64*);  /* a plain index: 1 */
int cbh_idx64_shard_count(const cbh_idx64*);        /* a plain index: 1 */
/* shard i as a plain one-device index, BORROWED (never destroy it): its count / download / scan_dev / time_scan_dev
 * show what one shard holds and does; a plain index is its own shard 0 */
cbh_idx64* cbh_idx64_shard(cbh_idx64*, int i);
typedef struct cbh_shard_stats {
  uint32_t shards, devices, device_mask;
  uint64_t segments;     /* runs of the global slot order (1 per shard after load; add() appends runs) */
  uint64_t scans;        /* shard-local scan launches */
  uint64_t rescans;      /* ... of which repeated because a shard's block overflowed */
  uint64_t collectives;  /* grouped ncclAllGather calls */
  uint64_t peer_copies;  /* hipMemcpyPeerAsync calls (needles out; records back unless "shard_exchange" is 0) */
  uint64_t local_copies; /* device-to-device copies of shard blocks inside one device */
  uint64_t collective_fallbacks; /* exchanges that asked for ncclAllGather and went by copies (no communicator) */
} cbh_shard_stats;
int cbh_idx64_shard_stats(const cbh_idx64*, cbh_shard_stats* out);
/* load(): replaces the SoA fill of DctHashIndex::load (:70-114); the caller runs the SQL
 * (`select id,phash_dct from media where type=1`, :89) and hands over the two columns.
 * n == 0 is valid (loaded, empty). */
int cbh_idx64_load(cbh_idx64*, const uint64_t* hashes, const uint32_t* ids, size_t n);
int cbh_idx64_load_dev(cbh_idx64*, const void* d_hashes, const void* d_ids, size_t n, void* stream);
int cbh_idx64_is_loaded(const cbh_idx64*);                       /* isLoaded() */
int cbh_idx64_add(cbh_idx64*, const uint64_t* hashes, const uint32_t* ids, size_t n); /* add() :158-173 */
/* remove(): zero id AND hash of every slot whose id is listed, in place (:175-191);
 * count() does not shrink. */
int cbh_idx64_remove(cbh_idx64*, const uint32_t* ids, size_t n);
size_t cbh_idx64_count(const cbh_idx64*);                        /* count() = _numHashes */
size_t cbh_idx64_memory_usage(const cbh_idx64*);                 /* memoryUsage() = 12 B * count (:56-59) */
/* mediaIds(), loaded branch (:129-133): ids of slots with hash != 0.  Writes up to cap,
 * *n_out = full number. */
int cbh_idx64_media_ids(const cbh_idx64*, uint32_t* out, size_t cap, size_t* n_out);
/* slice(): new index holding the slots whose id is in ids[], original order (:222-250);
 * caller destroys it (src/database.cpp:1435,1491).  A wanted 0 keeps removed slots; ids == NULL or n == 0 gives a
 * loaded, empty index.  This one still goes through the host (download, filter, load); a slice of a sharded index is
 * sharded the same way.  NULL + cbh_last_error_code() on failure; the parent stays usable. */
cbh_idx64* cbh_idx64_slice(const cbh_idx64*, const uint32_t* ids, size_t n);
/* copy the resident SoA back (tests, save()) */
int cbh_idx64_download(const cbh_idx64*, uint64_t* hashes, uint32_t* ids, size_t cap);

/* find(): every slot with hamm64(q, hash) < thresh and id != 0 (:193-220 with the brute-force
 * predicate of :210-217), as Match(id, distance), ascending (score, id).  q == 0 -> CBH_OK with
 * *n_out = 0 (:196-200).  Writes the first min(*n_out, cap) matches; *n_out is the full count. */
int cbh_idx64_find(cbh_idx64*, uint64_t q, int thresh, cbh_match* out, size_t cap, size_t* n_out);
/* Batched find + the sort/truncate of Database::searchIndex (src/database.cpp:1729-1735):
 * for query j, out[j*max_per_query ..] receives its first min(counts[j], max_per_query)
 * matches in (score, id) order (unused slots zeroed), counts[j] the full match count.
 * nq <= CBH_MAX_QUERIES_PER_CALL. */
int cbh_idx64_find_batch(cbh_idx64*, const uint64_t* q, size_t nq, int thresh, int max_per_query,
                         cbh_match* out, uint32_t* counts);
/* Same with device-resident queries and outputs (d_out: nq*max_per_query cbh_match,
 * d_counts: nq u32); *total_out (host) = total number of matching pairs. */
/* find_batch with one equal-bits mask per needle: additionally requires ((q ^ hash) & qmask) == 0.  This is
 * how the reference's APPROXIMATE structures restrict a search -- a HammingTree needle only sees the leaf
 * that shares its low bits (src/tree/hammingtree.h:244-252), a RadixMap needle only its bucket
 * (src/tree/radix.h:135-141) -- so with the right masks the results equal the reference's instead of being
 * a superset.  qmask == NULL is cbh_idx64_find_batch. */
int cbh_idx64_find_batch_masked(cbh_idx64*, const uint64_t* q, const uint64_t* qmask, size_t nq, int thresh,
                                int max_per_query, cbh_match* out, uint32_t* counts);
/* masks that make a search see exactly what HammingTree::search (hammingtree.h:103-108,244-293) would see
 * for the index's current contents: out_masks[i] = (1 << depth of q[i]'s leaf) - 1.  The tree shape (a node
 * splits on bit = depth once more than 8192 values were routed to it, :384-414) is rebuilt lazily after
 * load/add. */
int cbh_idx64_tree_masks(cbh_idx64*, const uint64_t* q, size_t nq, uint64_t* out_masks);
/* find() for an UNMODIFIED caller that issues one synchronous call per needle from many threads
 * (Database::similar: QtConcurrent::map -> searchIndex -> index->find, src/database.cpp:1400-1432,1698-1700).
 * Same results as cbh_idx64_find, bit for bit.  Concurrent callers are combined into one scan per round trip, and
 * once the time spent that way for a threshold exceeds what scanning the whole index against itself would cost
 * (the needles of an all-pairs search ARE the index entries), that self-join is run once, kept on the host, and
 * later calls whose needle hash is an index entry become table lookups (cbird_amd/csrc/coalesce.hip).  load / add /
 * remove drop the cache.  Thread-safe for concurrent readers; writers exclusive, as the reference's lock provides. */
int cbh_idx64_find_coalesced(cbh_idx64*, uint64_t q, int thresh, cbh_match* out, size_t cap, size_t* n_out);
typedef struct cbh_coalesce_stats {
  uint64_t finds;           /* calls */
  uint64_t cache_hits;      /* answered from a cached self-join */
  uint64_t rounds;          /* combined scans */
  uint64_t scanned_needles; /* needles served by those scans (finds - cache_hits, once everything has returned) */
  uint64_t self_joins;      /* whole-index self-joins built */
} cbh_coalesce_stats;
int cbh_idx64_coalesce_stats(cbh_idx64*, cbh_coalesce_stats* out);
int cbh_idx64_coalesce_set_self_join(cbh_idx64*, int enabled); /* default 1; 0 = combining only */
int cbh_idx64_find_batch_dev(cbh_idx64*, const void* d_q, size_t nq, int thresh,
                             int max_per_query, void* d_out, void* d_counts,
                             uint64_t* total_out, void* stream);
/* Raw scan stage only (the Hamming kernel): appends one cbh_record per matching pair to
 * d_records (capacity cap records, unordered) and adds the number of matching pairs to
 * *d_total (u64 on device, NOT reset by the call).  Records beyond cap are dropped but still
 * counted.  Asynchronous on `stream`.  This is the shard-local step of the multi-GPU path. */
int cbh_idx64_scan_dev(cbh_idx64*, const void* d_q, size_t nq, int thresh, void* d_records,
                       size_t cap, void* d_total, void* stream);
/* K4, the per-needle cut of Database::searchIndex (std::sort by score + stop at maxMatches,
 * src/database.cpp:1729-1737) as a counting select over UNORDERED scan records -- no global sort, no record count on
 * the host, nothing synchronises (cbird_amd/csrc/topk.hip).  Input: n_blocks blocks of u64 words, block b at
 * d_blocks + b*block_stride words = { count, records[cap] } -- what cbh_idx64_scan_dev produces when d_total points
 * at word 0 and d_records at word 1, and what ONE all_gather_into_tensor of such blocks delivers in the multi-GPU
 * path.  Output as cbh_idx64_find_batch_dev: the first max_per_query matches of every needle in ascending
 * (score, mediaId) order + the full match count per needle.  *d_status (u32 on device, NOT reset by the call) gets
 * bit 0 set when some block's count exceeds cap (records were dropped: rescan with a larger cap).  Asynchronous
 * on `stream` (NULL: synchronous).  nq <= 2^25, n_blocks*cap < 2^32. */
int cbh_records_topk_dev(const void* d_blocks, size_t n_blocks, size_t block_stride, size_t cap, size_t nq,
                         int max_per_query, void* d_out, void* d_counts, void* d_status, int device, void* stream);
/* Sort records ascending in place (device), n records, only bits [0, 39+ceil(log2(nq))). */
int cbh_sort_records_dev(void* d_records, size_t n, size_t nq, int device, void* stream);
/* Records (sorted) -> per-query top max_per_query + counts, as find_batch_dev does. */
int cbh_select_records_dev(const void* d_sorted_records, size_t n, size_t nq, int max_per_query,
                           void* d_out, void* d_counts, int device, void* stream);
/* capacity (records) of the internal match buffer used by find/find_batch; default 1<<24 */
int cbh_idx64_set_record_capacity(cbh_idx64*, size_t records);

/* Per-index counters of the Hamming scan kernel as launched by find/find_batch(_dev): number of
 * launches, GPU time between HIP events recorded around each launch on its own stream, and the
 * (needle x slot) pairs those launches evaluated. */
typedef struct cbh_stats {
  uint64_t scan_launches;
  uint64_t scan_pairs;
  double scan_ms;
} cbh_stats;
int cbh_idx64_get_stats(const cbh_idx64*, cbh_stats* out);
int cbh_idx64_reset_stats(cbh_idx64*);
int cbh_idx256_get_stats(const cbh_idx256*, cbh_stats* out);

/* ---- the bucketed join's resident slot tables (cbird_amd/csrc/hamm64_join.hip) -----------------------------------
 * The reference builds its tree once -- buildTree (src/dcthashindex.cpp:61-68), called when load() has read the rows
 * (:110) -- and every find() searches that tree (:208).  A handle that opts in keeps the join's view of its slots the same
 * way: per join plan m = max(4, thresh) the chunk values' histogram, its scans and the m chunk-ordered copies of the slots
 * (12 m n bytes plus the per-value arrays), built by the first joined call at that plan or by join_prepare, reused by
 * every later joined call, dropped by load / load_dev / add / remove / remove_ids_only / destroy.  A slice starts without
 * tables and is not opted in.  Which calls take the join is "scan_mfma"'s business as before; results never change.
 * cbh_idx64_memory_usage keeps the reference's formula (:56-59): the tables are reported here, in `bytes`. */
typedef struct {
  uint64_t builds;         /* table sets built (per plan, summed over shards) */
  uint64_t hits;           /* joined launches that reused resident tables */
  uint64_t drops;          /* table sets dropped by a mutation or release */
  uint64_t failed_builds;  /* builds given up for lack of memory or budget */
  uint64_t bytes;          /* resident now, all plans, all shards */
  uint32_t plans;          /* bit m: plan m resident and current on every non-empty shard */
} cbh_join_stats;
/* thresh 1..8, else CBH_E_INVAL; opts the handle in and builds plan max(4, thresh) now (the tree built at load, :110);
 * CBH_E_NOMEM if it cannot (no memory, or over "join_resident_mb"): the handle stays opted in and searches as before */
int cbh_idx64_join_prepare(cbh_idx64*, int thresh);
/* frees the tables and opts the handle out (unload()'s `delete _tree`, src/dcthashindex.cpp:52) */
int cbh_idx64_join_release(cbh_idx64*);
/* (the reference has no counters: what `_tree != nullptr` says, :202, and what the tables cost) */
int cbh_idx64_join_stats(const cbh_idx64*, cbh_join_stats*);

/* ---- Database::searchIndex / Database::similar for a whole needle batch (cbird_amd/csrc/search.hip) ------------
 * searchIndex (src/database.cpp:1691-1757) over DctHashIndex for nq needles: find at `thresh`; when max_thresh > 0 the
 * needles whose match count is <= min_matches are searched again at thresh + 1, + 2, ... <= max_thresh (:1703-1725);
 * matches in ascending (score, mediaId) order (:1729, ties fixed); the needle's own id dropped when filter_self
 * (:1735); at most max_matches kept (:1736); ids not in valid_ids_sorted (the caller's idMap; NULL = every id is
 * known) skipped without consuming a place (:1755).  out[j*max_matches ..], out_counts[j] = kept matches of needle j.
 * max_matches <= 55. */
int cbh_search_index_batch(cbh_idx64*, const uint64_t* q, const uint32_t* needle_ids, size_t nq, int thresh,
                           int max_thresh, int min_matches, int max_matches, int filter_self,
                           const uint32_t* valid_ids_sorted, size_t n_valid, cbh_match* out, uint32_t* out_counts);
/* The group filtering of Database::similar on those results (host code): a needle with no match is no group (:1409);
 * a group needs more than min_matches members, needle included (filterMatch, :1245); with filter_groups a group whose
 * set of paths equals an earlier group's is dropped (filterMatches, :1252-1272), "earlier" in needle-path order; the
 * result is in needle-path order (:1463).  Paths enter as ranks: path_rank[i] = position of the path of media
 * ids_sorted[i] in the sorted order of all paths.  out_group[0..*n_out) = needle indices of the surviving groups. */
int cbh_filter_groups(const uint32_t* needle_ids, const cbh_match* matches, const uint32_t* counts, size_t nq,
                      int max_matches, int min_matches, int filter_groups, const uint32_t* ids_sorted,
                      const uint32_t* path_rank, size_t n_ids, uint32_t* out_group, size_t* n_out);

/* searchIndex for a needle batch over the other four indexes (cbird_amd/csrc/searchbatch.hip): per threshold level ONE
 * batched find of every needle still pending (the *_find_batch entry points below), needles with <= min_matches results
 * go on to the next level -- dctThresh + 1 for dct features and video, cvThresh + 5 for ORB, no levels for colour
 * (:1707-1718) -- while it does not pass max_thresh (max_thresh 0: no escalation); then (score, mediaId) order,
 * filter_self, the max_matches cut and the idMap rule as above.  out[j*max_matches ..], out_counts[j].  Needle data as
 * in the corresponding *_find_batch call. */
int cbh_fdct_search_index_batch(cbh_idx64*, const uint64_t* hashes, const uint64_t* offsets, const uint32_t* needle_ids,
                                size_t n_needles, int thresh, int max_thresh, int tree_compat, int min_matches,
                                int max_matches, int filter_self, const uint32_t* valid_ids_sorted, size_t n_valid,
                                cbh_match* out, uint32_t* out_counts);
struct cbh_vidx;
struct cbh_vmatch;
int cbh_vidx_search_index_batch(struct cbh_vidx*, const int32_t* frames, const uint64_t* hashes, const uint64_t* offsets,
                                const uint32_t* needle_ids, size_t n_needles, int thresh, int max_thresh, int skip_frames,
                                int min_frames_matched, int min_frames_near, int min_matches, int max_matches,
                                int filter_self, const uint32_t* valid_ids_sorted, size_t n_valid, struct cbh_vmatch* out,
                                uint32_t* out_counts);
/* the same for IMAGE needles of the video index (DctVideoIndex::find -> findFrame, src/dctvideoindex.cpp:282-289): needle j
 * is hashes[j] with src_in[j] (src_in NULL: all -1); per dctThresh level one cbh_vidx_find_frames_batch of the pending
 * needles; a needle goes on while the rows findFrame returned for it -- counted before filter_self and the idMap rule,
 * findFrame knows neither -- are <= min_matches; order (score, mediaId, video index) */
int cbh_vidx_search_index_frames_batch(struct cbh_vidx*, const uint64_t* hashes, const int32_t* src_in,
                                       const uint32_t* needle_ids, size_t n_needles, int thresh, int max_thresh,
                                       int skip_frames, int min_matches, int max_matches, int filter_self,
                                       const uint32_t* valid_ids_sorted, size_t n_valid, struct cbh_vmatch* out,
                                       uint32_t* out_counts);
int cbh_idx256_search_index_batch(cbh_idx256*, const uint8_t* rows, const uint64_t* offsets, const uint32_t* needle_ids,
                                  size_t n_needles, int thresh, int max_thresh, int k, int min_matches, int max_matches,
                                  int filter_self, const uint32_t* valid_ids_sorted, size_t n_valid, cbh_match* out,
                                  uint32_t* out_counts);
struct cbh_color;
int cbh_color_search_index_batch(struct cbh_color*, const void* needle_descs, const uint32_t* needle_ids, size_t n_needles,
                                 int max_matches, int filter_self, const uint32_t* valid_ids_sorted, size_t n_valid,
                                 cbh_match* out, uint32_t* out_counts);

/* find() for an UNMODIFIED caller on the other four indexes (cbird_amd/csrc/combine.hip): same arguments and results as
 * cbh_fdct_find_ex / cbh_vidx_find_video / cbh_idx256_find / cbh_color_find; callers that arrive from other threads
 * while a search is in flight are served together by ONE call of the index's batch entry point (leader / follower, up
 * to 256 needles per round trip, requests grouped by equal search parameters).  This is what the Gpu*Index::find
 * adapters call.  cbh_combine_stats(handle): calls and combined searches so far. */
int cbh_fdct_find_coalesced(cbh_idx64*, const uint64_t* hashes, size_t n, uint32_t needle_id, int thresh, int tree_compat,
                            cbh_match* out, size_t cap, size_t* n_out);
int cbh_vidx_find_video_coalesced(struct cbh_vidx*, const int32_t* frames, const uint64_t* hashes, size_t n,
                                  uint32_t needle_id, int thresh, int skip_frames, int min_frames_matched,
                                  int min_frames_near, int filter_self, struct cbh_vmatch* out, size_t cap, size_t* n_out);
/* ... and cbh_vidx_find_frame for the image needles of a DctVideoIndex (a queue of its own beside the video needles';
 * cbh_combine_stats of the handle counts both): one cbh_vidx_find_frames_batch per round */
int cbh_vidx_find_frame_coalesced(struct cbh_vidx*, uint64_t hash, int thresh, int skip_frames, int src_in,
                                  struct cbh_vmatch* out, size_t cap, size_t* n_out);
int cbh_idx256_find_coalesced(cbh_idx256*, const uint8_t* needle_rows, size_t n_desc, int thresh, int k, cbh_match* out,
                              size_t cap, size_t* n_out);
int cbh_color_find_coalesced(struct cbh_color*, const void* needle_desc, cbh_match* out, size_t cap, size_t* n_out);
int cbh_combine_stats(const void* handle, uint64_t* finds, uint64_t* rounds);

/* All of filterMatch (src/database.cpp:1209-1248) and filterMatches (:1250-1278) on those results, host code:
 *   path_mode      params.path / inPath (:1217-1229): 0 = no path filter, 1 = keep only matches under the prefix
 *                  (inPath), 2 = keep only matches NOT under it; the needle always stays
 *   filter_parent  a match in the needle's directory -- or zip archive, Media::dirPath (src/media.cpp:198-208) -- is
 *                  removed (:1231-1242)
 *   min_matches    a group needs more than min_matches members, needle included, AFTER those removals (:1245)
 *   filter_groups  groups in needle-path order, a group whose set of paths was seen before is dropped (:1253-1272)
 *   merge_groups   Media::mergeGroupList (src/media.cpp:300-324): if group a contains the first member of group b, b's
 *                  other members join a, a is re-ordered by score (ties: by path) and b disappears
 *   expand_groups  (when not merging) Media::expandGroupList (:326-331): a,b,c,d becomes (a,b), (a,c), (a,d)
 * and the final stable order by the first member's path (:1463).  negativeMatch and the weed marks need other tables of
 * the database and stay with the caller.  Media enter as ids with three attributes the caller derives from their paths,
 * parallel to ids_sorted: path_rank (position of the path among all sorted paths), dir_id (equal numbers <=> equal
 * dirPath(); may be NULL without filter_parent), under_prefix (path.startsWith(prefix) as :1223-1227 builds the prefix;
 * may be NULL with path_mode 0).
 * Output: group g = out_members[out_first[g] .. out_first[g+1]) as (mediaId, score), the needle first with score -1 (a
 * haystack Media's default, src/media.cpp:112) unless a merge re-ordered the group.  CBH_E_OVERFLOW with *n_groups /
 * *n_members = the room needed when cap_groups (+1 entries in out_first) or cap_members is too small. */
typedef struct cbh_filter_params {
  int min_matches, filter_groups, filter_parent, path_mode, merge_groups, expand_groups;
} cbh_filter_params;
int cbh_filter_groups_ex(const uint32_t* needle_ids, const cbh_match* matches, const uint32_t* counts, size_t nq,
                         int max_matches, const cbh_filter_params* p, const uint32_t* ids_sorted,
                         const uint32_t* path_rank, const uint32_t* dir_id, const uint8_t* under_prefix, size_t n_ids,
                         uint64_t* out_first, size_t cap_groups, cbh_match* out_members, size_t cap_members,
                         size_t* n_groups, size_t* n_members);

/* ---- clusters: the connected components of a DctHashIndex's match graph (cbird_amd/csrc/clusters.hip) ------------------
 * "Which of my files are the same picture?" as a partition of the library.  The reference has no counterpart: -similar
 * gives one group per needle, and Media::mergeGroupList (src/media.cpp:300-324), its only tool for making sets of them,
 * is not transitive (a ~ c, c ~ b, a !~ b leaves b and c in two groups, and which two depends on the path order) and
 * quadratic in the number of groups.  Here: single-linkage clusters at dctThresh, exact.
 *   nodes     the live entries: slots with id != 0 and hash != 0 -- what mediaIds() counts; a null hash finds nothing
 *             (src/dcthashindex.cpp:196-200).  Live ids must be unique, else CBH_E_UNSUPPORTED (a keypoint-hash handle is
 *             not a DctHashIndex).
 *   edges     nodes i != j with popcount(h_i ^ h_j) < thresh, find()'s predicate (:210-217).  thresh 0..65, else
 *             CBH_E_INVAL; at 0 there are no edges, at 1 edges join equal hashes only.
 *   clusters  connected components with at least min_members nodes; min_members >= 2, else CBH_E_INVAL (callers pass
 *             minMatches + 1, the rule of filterMatch, src/database.cpp:1244).
 *   order     members in ascending id, clusters in ascending first id.  Nothing depends on the slot order, the shard layout
 *             or the chunking below.
 *   score     of a member = its distance to its nearest other member, 0..thresh-1.
 * The live (id, hash) pairs are put in id order once per call; ranges of "cluster_chunk" of them (cbh_set_tuning) are
 * the needles of one scan each, whose records are consumed and dropped before the next.  A scan with more than
 * "cluster_max_records" records is not materialised: its range is halved and scanned again (stats.rescans); a single
 * entry with more matches than that is CBH_E_OVERFLOW.  The call takes the handle as a reader, like
 * cbh_search_index_batch.  CBH_E_NOMEM when an allocation is refused: nothing is kept, the handle stays usable.
 * stats (may be NULL): nodes, records consumed, clusters / members found (cbh_idx64_clusters), scans that delivered
 * (chunks) and scans given up for their size (rescans). */
typedef struct cbh_cluster_stats {
  uint64_t nodes, records, clusters, members;
  uint32_t chunks, rescans;
} cbh_cluster_stats;
/* Per node, in ascending id order: ids[], label[] (the smallest id of its component), nearest[] (the distance to its
 * nearest neighbour under thresh, 0xFF for a node without one).  Writes min(n, cap) entries; *n_out = the node count. */
int cbh_idx64_cluster_labels(cbh_idx64*, int thresh, uint32_t* ids, uint32_t* label, uint8_t* nearest, size_t cap,
                             size_t* n_out, cbh_cluster_stats* stats);
/* The same into arrays on the handle's device; the work is queued on `stream` (NULL: a stream of the handle's), which
 * the call has synchronised when it returns. */
int cbh_idx64_cluster_labels_dev(cbh_idx64*, int thresh, void* d_ids, void* d_label, void* d_nearest, size_t cap,
                                 size_t* n_out, cbh_cluster_stats* stats, void* stream);
/* The clusters: cluster g = out_members[out_first[g] .. out_first[g+1]) as cbh_match{id, score}.  CBH_E_OVERFLOW with
 * *n_clusters / *n_members = the room needed when cap_clusters (+1 entries in out_first) or cap_members is too small,
 * exactly as cbh_filter_groups_ex. */
int cbh_idx64_clusters(cbh_idx64*, int thresh, int min_members, uint64_t* out_first, size_t cap_clusters,
                       cbh_match* out_members, size_t cap_members, size_t* n_clusters, size_t* n_members,
                       cbh_cluster_stats* stats);

/* ---- -sort-similar: src/main.cpp:1523-1580 ----------------------------------------------------------------------------
 * Orders selections so that every item is followed by its nearest remaining neighbour, the reference's loop and its
 * side effects restated exactly (AlgoDCT; items = 64-bit hash + unique non-zero id):
 *   sorted = [first item], unsorted = the rest; for i in 0 .. n-2, for j in 0 .. min(look_behind, len(sorted)) - 1 --
 *   len(sorted) read again on every pass -- the needle sorted[len-1-j] is queried inside unsorted + needle (:1552-1561);
 *   a hit is inserted at len-j and leaves unsorted (:1563-1567), a miss counts in not_found; every pass counts in
 *   queries; there is no break after a hit.  So after a hit at j the same needle is asked again and its next neighbour
 *   lands in front of the previous one, passes go on failing once unsorted is empty, and items never reached are
 *   dropped (selection = sorted, :1579).
 * One query is Database::similarTo + searchIndex + filterMatch (src/database.cpp:1468-1503, 1691-1757, 1209-1247) and
 * matches[0] after the sort of src/engine.cpp:441, with filterSelf on:
 *   a needle with hash 0 finds nothing (src/dcthashindex.cpp:196-200); a haystack hash 0 is a value like any other;
 *   candidates = unsorted items flagged in_index with popcount(needle ^ hash) < t, t from thresh; with max_thresh > 0,
 *   while candidates + self <= min_matches, t + 1 unless that passes max_thresh (:1703-1725) -- self = 1 when t > 0 and
 *   the needle is in_index (its slice holds it at distance 0); order by (distance, id); the first max_matches; of those,
 *   path_mode and filter_parent as in cbh_filter_params; accepted iff 1 + kept > min_matches; the answer is the first kept.
 * mirrorMask and templateMatch need images and have no counterpart here.
 * The batch is ragged: set s = items set_first[s] .. set_first[s+1] of hashes / ids / in_index (NULL: all in the index) /
 * dir_id (may be NULL without filter_parent) / under_prefix (may be NULL with path_mode 0); its first item is the start.
 * out_ids is parallel to ids: out_ids[set_first[s] .. + out[s].sorted) is the order, the rest of the set's range is 0.
 * out[s]: sorted = items placed, queries, not_found as the loop counts them, behind = hits at j > 0.  Sets of 0 or 1
 * items: sorted = n, no queries.  One launch for the whole batch, one workgroup per set (sortsimilar.hip).
 * CBH_E_INVAL: an id 0, an id twice in a set, look_behind outside 1..8, max_matches outside 1..55, thresholds outside
 * 0..65, an attribute array the params need missing; CBH_E_UNSUPPORTED: a set above CBH_SORT_SIMILAR_MAX items.
 * _dev: every array in device memory, work queued on `stream`; it waits for the stream twice (the set sizes, the id
 * check) before the ordering kernel is queued, and not after it. */
#define CBH_SORT_SIMILAR_MAX 65536
typedef struct cbh_sort_similar_params {
  int thresh, max_thresh, min_matches, max_matches; /* max_matches 1..55 */
  int filter_parent, path_mode;                     /* as cbh_filter_params */
  int look_behind;                                  /* the reference's 5 (:1530); 1..8 */
} cbh_sort_similar_params;
typedef struct cbh_sort_similar_result {
  uint32_t sorted, queries, not_found, behind;
} cbh_sort_similar_result;
int cbh_sort_similar(const uint64_t* hashes, const uint32_t* ids, const uint8_t* in_index, const uint32_t* dir_id,
                     const uint8_t* under_prefix, const uint64_t* set_first, size_t n_sets,
                     const cbh_sort_similar_params* params, uint32_t* out_ids, cbh_sort_similar_result* out, int device);
int cbh_sort_similar_dev(const void* d_hashes, const void* d_ids, const void* d_in_index, const void* d_dir_id,
                         const void* d_under_prefix, const void* d_set_first, size_t n_sets,
                         const cbh_sort_similar_params* params, void* d_out_ids, void* d_out, int device, void* stream);

/* The same loop over a TABLE of pair scores, for an index whose score of a pair does not depend on what else is in the
 * slice (sortsimilar_table.hip).  Everything said above holds -- sorted / unsorted, look_behind passes whose bound is read
 * again on every pass, no break after a hit, failing passes counted, items never reached dropped -- except the rule for
 * candidates: the score of (needle r, candidate c) is the set's table[r * n + c], a uint16_t, 0xFFFF = no match.  A
 * candidate is an item that is unsorted, flagged in_index (NULL: all) and has a score other than 0xFFFF; there are no
 * thresholds and no escalation.  Candidates order by (score, id); the first max_matches; of those, path_mode and
 * filter_parent as in cbh_filter_params; accepted iff 1 + kept > min_matches; the answer is the first kept.  The needle
 * is not unsorted, so it never takes one of the max_matches places.
 * set s = items set_first[s] .. set_first[s+1]; its table = scores + table_first[s], n_s * n_s entries in the CALLER's
 * item order, row = needle, column = candidate (the table need not be symmetric).
 * Outputs and error codes are cbh_sort_similar's: out_ids parallel to ids with the rest of a set's range 0; out[s] =
 * {sorted, queries, not_found, behind}; sets of 0 or 1 items make no queries.  CBH_E_INVAL: an id 0, an id twice in a
 * set, look_behind outside 1..8, max_matches outside 1..55, path_mode outside 0..2, an attribute array the params need
 * missing; CBH_E_UNSUPPORTED: a set above CBH_SORT_SIMILAR_MAX items.  The device holds a second copy of the tables
 * (rows and columns in id order, rows padded to 16 bytes).  _dev: every array in device memory, work queued on `stream`;
 * it waits for the stream twice before the ordering kernel is queued, and not after it. */
typedef struct cbh_sort_table_params {
  int min_matches, max_matches; /* max_matches 1..55 */
  int filter_parent, path_mode; /* as cbh_filter_params */
  int look_behind;              /* 1..8; the reference's 5 */
} cbh_sort_table_params;
int cbh_sort_similar_table(const uint16_t* scores, const uint64_t* table_first, const uint32_t* ids,
                           const uint8_t* in_index, const uint32_t* dir_id, const uint8_t* under_prefix,
                           const uint64_t* set_first, size_t n_sets, const cbh_sort_table_params* params,
                           uint32_t* out_ids, cbh_sort_similar_result* out, int device);
int cbh_sort_similar_table_dev(const void* d_scores, const void* d_table_first, const void* d_ids, const void* d_in_index,
                               const void* d_dir_id, const void* d_under_prefix, const void* d_set_first, size_t n_sets,
                               const cbh_sort_table_params* params, void* d_out_ids, void* d_out, int device, void* stream);

/* ---- -merge A B: src/main.cpp:1582-1652 --------------------------------------------------------------------------------
 * Puts every item of selection B into selection A next to its closest match.  The reference, restated:
 *   sets: for needle b_k, in B's order, params.set = the original A followed by b_0 .. b_k, with inSet (:1619-1625); the
 *   set grows by appended needles only and never holds the mutated A, so the searches do not depend on one another.
 *   one search, the lambda multiSearch (:1587-1615): maxMatches = 2; from params.algo on, Engine::query, accepted when
 *   there is a match and matches[0].score < thresholds[algo], thresholds = {12, 1000, 1000, INT_MAX} for algos 0..3;
 *   otherwise algo + 1, until algo > 3, then no matches.  (A start at AlgoVideo reads past the table: refused here.)
 *   placement (:1628-1650), sequential in B's order on the list L = A with every needle placed so far: no match --
 *   qCritical("no match"), the needle is dropped; else pos = the place of matches[0] in L; if 0 < pos < len - 1 and
 *   hamm64(needle, L[pos+1]) < hamm64(needle, L[pos-1]) then pos + 1; L.insert(pos, needle).  A needle lands in front of
 *   its match, and behind it only when the match has neighbours on both sides and the needle is strictly nearer to the
 *   one behind.  The two distances are of the dctHash, whichever algorithm answered.
 *   A match may be an earlier needle that was itself dropped: the reference's Q_ASSERT (:1640) aborts the process.  Here
 *   that needle is dropped with CBH_MERGE_MATCH_UNPLACED and the merge goes on -- a chosen deviation; any match on an
 *   empty A is such a case.
 * cbh_merge_find is the AlgoDCT stage for all needles in one launch (merge.hip): the arrays hold A (n_a items) then B
 * (n_b items); items = 64-bit hash + unique non-zero id.  One query is exactly the one cbh_sort_similar defines above --
 * a needle hash of 0, escalation with self, the order by (distance, id), the first max_matches, path_mode and
 * filter_parent, accepted iff 1 + kept > min_matches, filterSelf on -- with one difference: the candidates of needle b_k
 * are not "unsorted items" but the items of A and b_0 .. b_{k-1} flagged in_index (the slice of its set, Database::similarTo
 * with inSet, src/database.cpp:1475-1486, without the needle).  in_index (NULL: all in the index), dir_id (may be NULL
 * without filter_parent), under_prefix (may be NULL with path_mode 0) are parallel to hashes.  multiSearch's own
 * parameters are max_matches = 2 and the caller's thresholds; the score limit 12 is the caller's to apply.
 * out_match[k] = the place of needle k's answer in the caller's arrays (0 .. n_a + n_b - 1), 0xFFFFFFFF without one;
 * out_score[k] = its distance, -1 without one.
 * CBH_E_INVAL: an id 0, an id twice in A and B, max_matches outside 1..55, thresholds outside 0..65, path_mode outside
 * 0..2, an attribute array the params need missing; CBH_E_UNSUPPORTED: n_a + n_b >= 2^24 (a query's key holds the
 * position in 24 bits); CBH_E_NOMEM when an allocation is refused: nothing is kept.
 * cbh_merge_place is the placement above, on the host with no device use: match[k] as cbh_merge_find writes it, from
 * whichever stage of the cascade answered (0xFFFFFFFF: none).  out_order (room for n_a + n_b) = the places in the
 * caller's arrays in merged order, *n_out of them; out_status[k] = CBH_MERGE_* of needle k.  CBH_E_INVAL: a match
 * outside the arrays. */
#define CBH_MERGE_PLACED 0
#define CBH_MERGE_NO_MATCH 1
#define CBH_MERGE_MATCH_UNPLACED 2
typedef struct cbh_merge_params {
  int thresh, max_thresh, min_matches, max_matches; /* max_matches 1..55; multiSearch's is 2 */
  int filter_parent, path_mode;                     /* as cbh_filter_params */
} cbh_merge_params;
int cbh_merge_find(const uint64_t* hashes, const uint32_t* ids, const uint8_t* in_index, const uint32_t* dir_id,
                   const uint8_t* under_prefix, size_t n_a, size_t n_b, const cbh_merge_params* params, uint32_t* out_match,
                   int32_t* out_score, int device);
int cbh_merge_place(const uint64_t* hashes, size_t n_a, size_t n_b, const uint32_t* match, uint32_t* out_order,
                    uint8_t* out_status, size_t* n_out);

/* ---- DctFeaturesIndex: src/dctfeaturesindex.{h,cpp} over src/tree/hammingtree.h -----------------
 * The index is a cbh_idx64 whose entries are (mediaId, keypoint hash) pairs, several per media:
 *   load/add      -> cbh_idx64_load / cbh_idx64_add with one entry per hash (:229-238, :143-156)
 *   remove        -> cbh_idx64_remove_ids_only: HammingTree::remove zeroes the index and KEEPS the
 *                    hash (hammingtree.h:349-361, dctfeaturesindex.cpp:240-249)
 *   count()       -> cbh_idx64_count (= _tree->size(), removed entries included) */
int cbh_idx64_remove_ids_only(cbh_idx64*, const uint32_t* ids, size_t n);
/* HammingTree::findIndex (hammingtree.h:110-112): hashes stored for one mediaId */
int cbh_idx64_hashes_for_id(const cbh_idx64*, uint32_t id, uint64_t* out, size_t cap, size_t* n_out);
/* DctFeaturesIndex::find (:260-358) for one needle with keypoint hashes[n] and id needle_id:
 * per needle hash the 10 nearest entries under thresh (removed entries take part in the cut and are
 * skipped afterwards, :301-308), votes per mediaId, score -1 for the needle itself, 10*avg distance
 * when no other media got more than one vote, else maxMatches - votes.  Results ascending mediaId
 * (QMap order).  Exact candidates (the reference tree is approximate). */
int cbh_fdct_find(cbh_idx64*, const uint64_t* hashes, size_t n, uint32_t needle_id, int thresh,
                  cbh_match* out, size_t cap, size_t* n_out);
/* Many needles in one scan: needle i owns hashes[offsets[i] .. offsets[i+1]); results of needle i
 * go to out[out_offsets[i] .. out_offsets[i+1]).  CBH_E_OVERFLOW when the total exceeds cap
 * (out_offsets[n_needles] then holds the required capacity). */
/* as cbh_fdct_find / _batch; tree_compat != 0 restricts every needle hash to its HammingTree leaf
 * (cbh_idx64_tree_masks), reproducing the reference's approximate candidate sets on multi-leaf trees */
int cbh_fdct_find_ex(cbh_idx64*, const uint64_t* hashes, size_t n, uint32_t needle_id, int thresh,
                     int tree_compat, cbh_match* out, size_t cap, size_t* n_out);
int cbh_fdct_find_batch_ex(cbh_idx64*, const uint64_t* hashes, const uint64_t* offsets,
                           const uint32_t* needle_ids, size_t n_needles, int thresh, int tree_compat,
                           cbh_match* out, size_t cap, uint64_t* out_offsets);
int cbh_fdct_find_batch(cbh_idx64*, const uint64_t* hashes, const uint64_t* offsets,
                        const uint32_t* needle_ids, size_t n_needles, int thresh, cbh_match* out,
                        size_t cap, uint64_t* out_offsets);

/* ---- DctVideoIndex: src/dctvideoindex.{h,cpp}, VideoIndex: src/videoindex.{h,cpp} -----------------
 * Index::Match with its MatchRange (src/index.h:157-166, src/media.h:62-78). */
typedef struct cbh_vmatch {
  uint32_t id;   /* mediaId of the matched video */
  int32_t score; /* findVideo: 100 - percentNear; findFrame: Hamming distance */
  int32_t src_in, dst_in, len; /* MatchRange: needle frame, matched frame, length */
} cbh_vmatch;
typedef struct cbh_vidx cbh_vidx; /* opaque: DctVideoIndex state */

cbh_vidx* cbh_vidx_create(int device);
/* the search structure built over all videos' frames becomes a sharded cbh_idx64 (above); entries are in video order,
 * so the contiguous row shares are shares BY VIDEO up to one video at each boundary */
cbh_vidx* cbh_vidx_create_sharded(uint32_t device_mask, int shards_per_device);
void cbh_vidx_destroy(cbh_vidx*);
/* 0 (default) = exact search; N > 0 = the reference's RadixMap(videoRadix = N) behaviour: a needle frame only
 * sees index entries of its bucket (hash >> 1) & (2^N - 1) (src/tree/radix.h:135-141, `-p.vradix`, default 10
 * in cbird); N is limited to 24 like the reference's constructor does (:105-112) */
int cbh_vidx_set_radix(cbh_vidx*, int radix);
/* load()/add() (:172-211, :250-254) only register media ids; the per-video (frame, hash) lists come
 * from <dataPath>/<id>.vdx when the tree is built (insertHashes :61-111).  Here the caller hands the
 * decoded lists over (cbh_vdx_decode below reads the files).  Order of calls = _mediaId order. */
int cbh_vidx_add_video(cbh_vidx*, uint32_t media_id, const int32_t* frames, const uint64_t* hashes, size_t n);
int cbh_vidx_remove(cbh_vidx*, const uint32_t* media_ids, size_t n);           /* remove() :256-275 */
/* slice() (:389-397): a new index of the same device or sharded shape and radix with the videos whose media id is
 * listed, in the order of ids[] (first occurrence of an id only; ids the handle lacks are skipped) -- copied from the
 * frames and hashes the handle holds, no .vdx file is read.  Host code; the result builds its search structure on the
 * first search.  Caller destroys it; NULL + cbh_last_error_code() on failure. */
cbh_vidx* cbh_vidx_slice(const cbh_vidx*, const uint32_t* ids, size_t n);
size_t cbh_vidx_count(const cbh_vidx*);                                         /* count() = #videos */
/* memoryUsage() (src/dctvideoindex.cpp:57-59: `_tree ? _tree->stats().memory : 0`): 0 until the search structure is
 * built; then the payload bytes the reference's RadixMap holds for the same entries -- 8 (hash_t) + 6 (the packed 24+24-bit
 * VideoTreeIndex, src/dctvideoindex.h:37-43) per entry -- without std::vector's capacity slack and the bucket table
 * (src/tree/radix.h:80-83,167), which depend on insertion history */
size_t cbh_vidx_memory_usage(const cbh_vidx*);
/* number of entries in the search structure after the insertHashes filters; builds it (buildTree
 * :113-170) with vtrim = skip_frames if it is not built yet (a built tree is NOT rebuilt for another
 * skip_frames, like `if (_tree) return;`). */
size_t cbh_vidx_entries(cbh_vidx*, int skip_frames);
/* findFrame (:291-387), image needle: nearest frame per video under thresh; results ascending video
 * index; range = (src_in<0 ? 0 : src_in, matched frame, 1). */
int cbh_vidx_find_frame(cbh_vidx*, uint64_t hash, int thresh, int skip_frames, int src_in,
                        cbh_vmatch* out, size_t cap, size_t* n_out);
/* findFrame for n image needles with one scan and one reduction on the device (cbird_amd/csrc/frames.hip) per
 * CBH_MAX_QUERIES_PER_CALL needles: the results of needle i, those of cbh_vidx_find_frame(hashes[i], .., src_in[i]), go to
 * out[out_offsets[i] .. out_offsets[i+1]).  src_in NULL: every needle -1.  A needle whose hash is 0 gets none (:333-337).
 * CBH_E_OVERFLOW when the total exceeds cap (out_offsets is complete, out_offsets[n] holds the required capacity, out is
 * not written), or when one chunk's scan finds 2^32 records or more (out_offsets is not written).  Honours
 * cbh_vidx_set_radix; plain and sharded handles. */
int cbh_vidx_find_frames_batch(cbh_vidx*, const uint64_t* hashes, const int32_t* src_in, size_t n, int thresh,
                               int skip_frames, cbh_vmatch* out, size_t cap, uint64_t* out_offsets);
/* findVideo (:399-657), video needle given as its (frames, hashes) list (needle_id 0 = not in the db).
 * thresh = dctThresh, skip_frames = vtrim (skipFrames), min_frames_matched = vfm, min_frames_near = vfn. */
int cbh_vidx_find_video(cbh_vidx*, const int32_t* frames, const uint64_t* hashes, size_t n,
                        uint32_t needle_id, int thresh, int skip_frames, int min_frames_matched,
                        int min_frames_near, int filter_self, cbh_vmatch* out, size_t cap, size_t* n_out);
/* many video needles in one scan (needle i = [offsets[i], offsets[i+1]) of frames/hashes) */
int cbh_vidx_find_videos_batch(cbh_vidx*, const int32_t* frames, const uint64_t* hashes,
                               const uint64_t* offsets, const uint32_t* needle_ids, size_t n_needles,
                               int thresh, int skip_frames, int min_frames_matched, int min_frames_near,
                               int filter_self, cbh_vmatch* out, size_t cap, uint64_t* out_offsets);
/* ---- the coverage map of video pairs (cbird_amd/csrc/vcoverage.hip) -------------------------------------------------------
 * Which frames of one video another contains: the list "needle frame -> closest frame" that findVideo (:399-657) builds
 * per matched video and drops, kept, for a batch of ordered pairs (source video, destination video), with a summary per
 * pair.  The reference's wish list names it (doc/cbird-devel.md, Search: "video coverage map to tell if one clip includes
 * all frames of another clip").  A video is the (frames, hashes) list of its .vdx, frame numbers rising.
 *   source frames considered  the stored frames findVideo searches (:431): frame f is dropped when f < skip_frames or
 *                 f > last - skip_frames, unconditionally; last = the last stored frame number
 *   destination entries       the frames insertHashes stores (:61-111): not a hash with fewer than 5 set or fewer than 5
 *                 clear bits; the same trim, but only when skip_frames && last / 2 > skip_frames -- with the skip_frames
 *                 of THIS call, whatever a handle's search structure was built with
 *   nearest       for considered frame i the entry j with the smallest hamm64, the lowest j among equals: the unsigned
 *                 minimum of distance << 24 | j.  Reported whether or not it is under thresh; a destination without
 *                 entries gives frame -1 and distance 65
 *   covered       distance < thresh, the comparison of every find of this library
 *   span          of a stored source frame: the next stored frame number of the untrimmed list minus its own, 1 for the
 *                 last one -- the indexer only drops a frame that is near every frame since the last stored one
 *                 (src/media.cpp:998-1012), so a stored frame stands for that stretch */
typedef struct cbh_vcover {
  int64_t src_frames_total;   /* sum of the spans of the considered frames */
  int64_t src_frames_covered; /* ... of the covered ones */
  int64_t gap_len;            /* the longest run of consecutive uncovered considered frames, as the sum of its spans: the */
  int32_t gap_begin;          /* run with the largest sum, the earliest among equals, and its first frame number; 0, 0   */
                              /* without an uncovered frame                                                              */
  int32_t n_src, n_dst;       /* considered frames, destination entries */
  int32_t n_covered;
  int32_t n_low_detail;       /* considered frames whose own hash fails the 5-bit rule (searched all the same, as findVideo does) */
  int32_t near_percent;       /* findVideo's percentNear over the covered frames in frame order (frameMargin 15, lastFrame */
                              /* starting at 0, integer division); 0 when nothing is covered                               */
  int32_t src_in, dst_in, len; /* the MatchRange findVideo reports for the pair; -1, -1, 0 when nothing is covered */
  int32_t dst_min, dst_max;   /* lowest and highest destination frame a covered frame matched; -1, -1 when none */
  int32_t reserved;           /* 0 */
} cbh_vcover;
typedef struct cbh_vcover_frame {
  int32_t src_frame, dst_frame, distance;
} cbh_vcover_frame;
/* Video v of the table is frames / hashes [video_offsets[v], video_offsets[v + 1]); pair k is source video pairs[2 k]
 * against destination video pairs[2 k + 1], both indexes into the table (equal ones allowed).  Every video is uploaded
 * once, however many pairs name it; no handle is involved, so a needle outside the database is served as well.
 * summaries[n_pairs] is always written.  map == NULL: nothing else comes back from the device (map_offsets, if given,
 * is still filled).  Otherwise the map of pair k, one entry per considered source frame in frame order, goes to
 * map[map_offsets[k] .. map_offsets[k + 1]); the sizes are known before anything is launched, and when they exceed
 * map_cap (in entries) the call returns CBH_E_OVERFLOW with map_offsets complete, map_offsets[n_pairs] the capacity
 * needed, and nothing else written -- the protocol of cbh_vidx_find_frames_batch.
 * n_pairs == 0 returns CBH_OK.  CBH_E_INVAL: a NULL required pointer, a map without map_offsets, a pair outside the table,
 * falling offsets, skip_frames < 0.  CBH_E_UNSUPPORTED: a video of more than 2^24 stored frames.  CBH_E_NOMEM when an
 * allocation is refused: nothing is kept.  The result does not depend on "vcover_chunk" / "vcover_tile" (cbh_set_tuning). */
int cbh_video_coverage(int device, const int32_t* frames, const uint64_t* hashes, const uint64_t* video_offsets,
                       size_t n_videos, const uint32_t* pairs, size_t n_pairs, int thresh, int skip_frames,
                       cbh_vcover* summaries, cbh_vcover_frame* map, size_t map_cap, uint64_t* map_offsets);
/* The same for videos the handle holds: pair k is the video of media id src_ids[k] against that of dst_ids[k].  The lists
 * are gathered from the handle (they live on the host, on a plain and on a sharded handle alike), each distinct video
 * once, and go through cbh_video_coverage on the handle's device; the search structure is neither needed nor built, and
 * cbh_vidx_set_radix does not apply (the map is exact).  Of two videos that carry one media id the FIRST is used.  An id
 * the handle does not hold: CBH_E_INVAL, nothing written. */
int cbh_vidx_coverage(cbh_vidx*, const uint32_t* src_ids, const uint32_t* dst_ids, size_t n_pairs, int thresh,
                      int skip_frames, cbh_vcover* summaries, cbh_vcover_frame* map, size_t map_cap,
                      uint64_t* map_offsets);
/* ---- where one video lies inside another: offsets and segments (cbird_amd/csrc/vsegments.hip) ------------------------------
 * The coverage map gives a frame its nearest frame ANYWHERE in the destination; a black frame or a static scene matches
 * wherever there is one.  This finds, for an ordered pair (source, destination), the frame-number offsets at which the
 * source lies in the destination and returns one segment per offset (doc/cbird-devel.md, Search: "refine video search
 * matches using neighboring hashes").  Considered source frames fs_i / hs_i, destination entries fd_j / hd_j, span and the
 * predicate hamm64 < thresh are cbh_video_coverage's, unchanged.  A match is (i, j) with hamm64(hs_i, hd_j) < thresh; its
 * offset is fd_j - fs_i.  Integers only:
 *   1 support     for a set L of live source frames, support(o) = the number of i in L with a match whose offset lies
 *                 within tol of o; a frame counts once per offset however many entries it matches.  o ranges over
 *                 [min fd - max fs - tol, max fd - min fs + tol]
 *   2 offset      m = the maximum support; of the maximal runs [lo, hi] of consecutive offsets with support m the one
 *                 whose centre c = floor((lo + hi) / 2) (toward minus infinity) has the smallest |c|, the negative c of
 *                 two; the round's offset is that c -- the centre of the plateau, not its edge
 *   3 members     every live i with a match within tol of c joins the segment and leaves L; its destination frame is the
 *                 match with the smallest |fd_j - fs_i - c|, then the smallest distance, then the lowest j
 *   4 rounds      L starts as every considered frame; 1 - 3 repeat until m < min_frames, max_segments segments exist or L
 *                 has no match left.  Segments come in the order found; their n_frames (= m) never rise
 *   5 empty       no considered frame, no entry or no match: no segment
 * The result does not depend on launch shapes, on "vseg_budget_mb" or on any order of accumulation. */
#define CBH_VSEGMENTS_MAX 16
typedef struct cbh_vsegment {
  int64_t span_sum;            /* sum of the members' spans */
  int32_t offset, n_frames;    /* rule 2, rule 3 */
  int32_t src_first, src_last; /* frame numbers of the first and last member */
  int32_t dst_first, dst_last; /* the destination frames those two members chose */
} cbh_vsegment;
typedef struct cbh_vsegments {
  int64_t src_frames_total, src_frames_aligned; /* span sums: considered / members of any segment */
  int32_t n_src, n_dst, n_segments, n_aligned;
  int32_t monotone;       /* 1: sorted by src_first (the earlier found of two equals first), src_first + offset never */
                          /* falls -- no scenes swapped; 0 or 1 segments: 1                                           */
  int32_t src_in, dst_in, len;  /* of segment 0: src_first, dst_first, dst_last - dst_first + 1; -1, -1, 0 without */
} cbh_vsegments;
typedef struct cbh_vsegment_frame {
  int32_t src_frame, dst_frame, distance, segment;
} cbh_vsegment_frame;
/* The video table, the pairs, the map, map_cap / map_offsets and the CBH_E_OVERFLOW protocol are cbh_video_coverage's.
 * summaries[n_pairs] and segments[n_pairs * max_segments] are always written: the segments of pair k from
 * segments[k * max_segments] on, unused records zero.  The map has one entry per considered source frame in frame order;
 * a frame in no segment holds dst_frame -1, distance 65, segment -1.  tol >= 0 frames of slack (stored frames are sparse:
 * two encodes of one clip rarely store the same frame numbers; findVideo's frameMargin is 15), min_frames >= 1,
 * max_segments 1 .. CBH_VSEGMENTS_MAX.
 * Errors: those of cbh_video_coverage; CBH_E_INVAL also for tol < 0, min_frames < 1, max_segments outside 1..16, and for a
 * named video whose frame numbers fall -- this is how no input reaches an index outside an array: the first and last
 * frame of a view are its extremes.  CBH_E_UNSUPPORTED also for an offset outside 32 bits.  Every pair has an array of one
 * word per offset of its domain; pairs are processed in groups whose arrays fit "vseg_budget_mb" together, and a pair
 * whose array alone exceeds it (a huge tol) returns CBH_E_NOMEM with nothing kept. */
int cbh_video_segments(int device, const int32_t* frames, const uint64_t* hashes, const uint64_t* video_offsets,
                       size_t n_videos, const uint32_t* pairs, size_t n_pairs, int thresh, int skip_frames, int tol,
                       int min_frames, int max_segments, cbh_vsegments* summaries, cbh_vsegment* segments,
                       cbh_vsegment_frame* map, size_t map_cap, uint64_t* map_offsets);
/* The same for videos the handle holds, plain or sharded, gathered as cbh_vidx_coverage gathers them. */
int cbh_vidx_segments(cbh_vidx*, const uint32_t* src_ids, const uint32_t* dst_ids, size_t n_pairs, int thresh,
                      int skip_frames, int tol, int min_frames, int max_segments, cbh_vsegments* summaries,
                      cbh_vsegment* segments, cbh_vsegment_frame* map, size_t map_cap, uint64_t* map_offsets);
/* .vdx v2 (VideoIndex::save_v2/load_v2/verify_v2, src/videoindex.cpp:248-429).  encode returns the file
 * size (0 = invalid input: first frame must be 0, frames strictly increasing) and writes it when it fits;
 * decode = load_v2: the frame count or a negative CBH_E_* (bad header, short data); like the reference's loader it
 * does not look at the trailer and loads a file with more than 2^24 frames up to that limit; verify = verify_v2
 * (what VideoIndex::isValid runs): header + "cbir" trailer, 1 = valid. */
size_t cbh_vdx_encode(const int32_t* frames, const uint64_t* hashes, size_t n, const char* cbird_version,
                      uint8_t* out, size_t cap);
long long cbh_vdx_decode(const uint8_t* buf, size_t len, int32_t* frames, uint64_t* hashes, size_t cap);
int cbh_vdx_verify(const uint8_t* buf, size_t len);
/* the old version-1 files (src/videoindex.cpp:41-68, 431-541: u16 frame count, u16 frame numbers, u64 hashes): decode and
 * verify above pick the version by the magic like VideoIndex::load / isValid and apply load_v1's two repairs (frame
 * numbers that wrapped past 65535; a missing frame 0); cbh_vdx_version tells which it is, cbh_vdx_encode_v1 = save_v1. */
int cbh_vdx_version(const uint8_t* buf, size_t len);
size_t cbh_vdx_encode_v1(const int32_t* frames, const uint64_t* hashes, size_t n, uint8_t* out, size_t cap);
/* frame de-dup of Media::makeVideoIndex (src/media.cpp:958-1024); keep[i]=1 for stored frames */
size_t cbh_video_dedup(const uint64_t* hashes, size_t n, int threshold, uint8_t* keep);

/* Media::makeVideoIndex (src/media.cpp:925-1037) for a decoder that delivers its frames in chunks: per frame
 * grayscale (the decoder outputs grey: a no-op, :958) -> autocrop(img, 20) -> dctHash64 (:961-962, :987-992) on the
 * device, then the near-frame filter (:994-1011), whose state -- frameNumber, window, the stored (frame, hash) lists --
 * lives in the handle between pushes.  threshold = IndexParams::videoThreshold (src/scanner.h; <= 0 stores every
 * frame), autocrop_range = 20 in cbird (< 0: no autocrop).
 *   resume(): start from an index written earlier (:929-936: the next frame is frames[n-1] + 1 and, like the first
 *             frame of a fresh run, is stored unconditionally); only before the first push.
 *   push():   n grey frames of one geometry in host memory, in decode order; push_dev(): the same in device memory
 *             (a hardware decoder's output).  Frames after MAX_FRAMES_PER_VIDEO (1 << 24, src/dctvideoindex.h:32,50)
 *             are dropped as at :1013-1016.
 *   finish(): the index as makeVideoIndex leaves it, with the last frame appended if it was not stored (:1018-1024);
 *             returns the number of entries and writes them when cap suffices.  Does not change the handle: more
 *             frames may be pushed afterwards.
 * One handle = one video, used by one thread at a time (Scanner::processVideo runs one per worker thread); handles of
 * different threads are independent (each owns its stream and buffers). */
typedef struct cbh_vindexer cbh_vindexer;
cbh_vindexer* cbh_vindexer_create(int device, int threshold, int autocrop_range);
void cbh_vindexer_destroy(cbh_vindexer*);
int cbh_vindexer_resume(cbh_vindexer*, const int32_t* frames, const uint64_t* hashes, size_t n);
int cbh_vindexer_push(cbh_vindexer*, const uint8_t* frames, size_t n, int w, int h, size_t row_stride,
                      size_t img_stride);
int cbh_vindexer_push_dev(cbh_vindexer*, const void* d_frames, size_t n, int w, int h, size_t row_stride,
                          size_t img_stride);
long long cbh_vindexer_frames_seen(const cbh_vindexer*);   /* makeVideoIndex's frameNumber */
long long cbh_vindexer_finish(const cbh_vindexer*, int32_t* frames, uint64_t* hashes, size_t cap);

/* ---- TemplateMatcher::match's score (src/templatematcher.cpp:331-374) ------------------------------------------------
 * For n candidate patches as warpAffine left them (template-sized; channels 1, 3 = BGR or 4 = BGRA; pixels outside the
 * warped patch are 0) and ONE template image: grayscale(cand); per pixel the candidate's grey value is the mask -- where
 * it is 0 the template's pixel is zeroed too, a BGRA template is premultiplied by its alpha (and scales the candidate's
 * grey value by it) (:343-364); candHash = dctHash64(cand), tmplHash = dctHash64(tmplMasked); score = hamm64 of the two
 * (:366-371; the caller compares with tmThresh, :373).  The descriptor match in front of it is cbh_idx256_radius_match;
 * estimateRigidTransform / warpAffine between the two are cbh_estimate_rigid / cbh_warp_affine_dev below, and
 * cbh_template_match runs transform -> warp -> these hashes -> score for a batch without leaving the device. */
int cbh_template_scores(const uint8_t* cands, size_t n, int w, int h, size_t cand_row_stride, size_t cand_img_stride,
                        int cand_channels, const uint8_t* tmpl, size_t tmpl_row_stride, int tmpl_channels,
                        uint64_t* cand_hashes, uint64_t* tmpl_hashes, int32_t* scores, int device);
int cbh_template_hashes_dev(const void* d_cands, size_t n, int w, int h, size_t cand_row_stride, size_t cand_img_stride,
                            int cand_channels, const void* d_tmpl, size_t tmpl_row_stride, int tmpl_channels,
                            void* d_cand_hashes, void* d_tmpl_hashes, int device, void* stream);

/* ---- TemplateMatcher::match between the descriptor match and the score (src/templatematcher.cpp:264-333) ----------
 * UNPINNED: OpenCV is not available to this repository; estimateRigidTransform, cv::transform, invertAffineTransform and
 * warpAffine are restated as recalled from OpenCV 2.4.13 (cbird_amd/csrc/tmatch.hip; tests/template_match_rules.py is the
 * numpy model the device is held to) until tools/pin_with_opencv.sh has written tests/golden/opencv_tmatch.npz.
 *
 * estimateRigidTransform(A, B, fullAffine = false) on point sets (:264, :309) for n ragged lists: list i = pairs
 * first[i] .. first[i + 1] of a_xy / b_xy (x, y floats; first[0] = 0; `first` is host memory in both entries).  RANSAC
 * with cv::RNG((uint64)-1), at most 500 outer iterations of three draws, inlier threshold 0.05 * the larger side of
 * boundingRect(B), stop at half the pairs, final getRTMatrix over the inliers in order.  m[6 * i ..] = the 2 x 3 matrix in
 * row order (zeros when found[i] == 0: fewer than three pairs, or no iteration stopped); detail (NULL or n): outer
 * iterations run (0 below three pairs, 500 when none stopped), inliers of the stopping iteration (0 when not found), RNG
 * values drawn.  Any count up to 2^31 - 1 pairs per list. */
typedef struct cbh_rigid_detail {
  int32_t iterations, good_count;
  uint32_t draws, reserved;
} cbh_rigid_detail;
int cbh_estimate_rigid(const float* a_xy, const float* b_xy, size_t n, const uint64_t* first, double* m, uint8_t* found,
                       cbh_rigid_detail* detail, int device);
int cbh_estimate_rigid_dev(const void* d_a_xy, const void* d_b_xy, size_t n, const uint64_t* first, void* d_m /* f64 6n */,
                           void* d_found /* u8 n */, void* d_detail /* NULL or n */, int device, void* stream);
/* invertAffineTransform(m) + warpAffine(img, m, Size(tw, th), INTER_AREA -> INTER_LINEAR, BORDER_CONSTANT, (0,0,0,255))
 * (:331-333) for n ragged candidate images (the img_off / img_w / img_h / img_row_stride host tables and the channel
 * counts 1 / 3 / 4 of cbh_quality_scores_dev; sides up to 32767) into packed n x th x tw x channels patches: d_m[6 * i ..]
 * maps the template to the candidate, as estimateRigidTransform returned it.  The patch of a candidate with
 * d_found[i] == 0 is zero; so is one whose coordinate integers would reach 2^30 (|M (x, y)| * 1024, where the reference's
 * arithmetic is undefined) -- d_warped (NULL or u8 n) tells: 1 = warped.  d_patches is 16-byte aligned. */
int cbh_warp_affine_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                        const uint32_t* img_row_stride, int channels, const void* d_m, const void* d_found, int tw, int th,
                        void* d_patches, void* d_warped, int device, void* stream);
/* The chain for ONE template and n candidates: both estimates (the second on matchPoints / cand_scale[i], :304-309), the
 * corners and the roi (:284-300), the warp, cbh_template_hashes_dev, hamm64.  tmpl_xy / match_xy / first: the point lists
 * of the candidates in the caller's order (:243-250).  A candidate without a transform, or outside the warp's domain, has
 * found = 0, score = INT32_MAX (the reference's INT_MAX, :233, :258, :271) and zeros elsewhere but iterations /
 * good_count.  patches (NULL or n x th x tw x channels; the device entry's 16-byte aligned) receives the warped patches.
 * Host images go up in pieces of at most "tmatch_chunk_mb" (cbh_set_tuning). */
typedef struct cbh_template_result {
  double m[6];   /* template -> candidate (:264) */
  double tx[6];  /* template -> unscaled candidate (:309); zeros unless tx_found */
  uint64_t cand_hash, tmpl_hash;
  int32_t roi[8]; /* x, y of the four corners / candScale (:299) */
  int32_t found, tx_found, score, iterations, good_count, reserved;
} cbh_template_result;
int cbh_template_match(const uint8_t* tmpl, int tw, int th, size_t tmpl_row_stride, int tmpl_channels, const uint8_t* imgs,
                       size_t imgs_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                       const uint32_t* img_row_stride, int channels, const float* tmpl_xy, const float* match_xy,
                       const uint64_t* first, const float* cand_scale, cbh_template_result* results, uint8_t* patches,
                       int device);
int cbh_template_match_dev(const void* d_tmpl, int tw, int th, size_t tmpl_row_stride, int tmpl_channels, const void* d_imgs,
                           size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                           const uint32_t* img_row_stride, int channels, const void* d_tmpl_xy, const void* d_match_xy,
                           const uint64_t* first, const float* cand_scale, void* d_results, void* d_patches, int device,
                           void* stream);

/* ---- TemplateMatcher::match from the decoded images to the score (src/templatematcher.cpp:105-374) -------------------
 * One template and n candidate images (8-bit, channels 1 / 3 = BGR / 4 = BGRA, one channel count per call, the template's
 * included; ragged: the img_off / img_w / img_h / img_row_stride host tables of cbh_warp_affine_dev, sides up to 32767) ->
 * one cbh_tm_image_result each, with no host round trip between the upload and the results but the keypoint counts and
 * the match counts (cbh_orb_dev's and cbh_template_match_dev's host tables).  cbird_amd/csrc/tmimages.hip.
 * UNPINNED where its parts are: the estimate, the warp (cbh_template_match above) and ORB (cbh_orb) are restated as
 * recalled from OpenCV 2.4.13; the resize, the grey conversion, the descriptor match and the gather are integer / copy
 * steps held to the oracle bit for bit.
 * Per candidate (:161-414): candScale and the target size (:182-192; sizeScaleFactor, src/cvutil.cpp:1951-1956: areas
 * compared as integers, maxSize = int(tSize * tm_scale_pct / 100.0), candScale = float(maxSize) / cSize, sides
 * int(cols * candScale)); cv::resize(INTER_LANCZOS4) of every channel -- the resized image replaces the candidate for
 * everything after it, the warp included (:190, :332); ORB of the grey view with haystack_features (:197-202; the template:
 * needle_features, :120-121; ORB's own limit of 8192 pixels per side applies to the template and to the candidates as they
 * reach it, CBH_E_INVAL beyond; needs cbh_orb_set_pattern); radiusMatch against the template's rows within cv_thresh
 * (:217); the point lists (:221-250, from the keypoints as compute() left them); then cbh_template_match_dev.
 * Host images go up, and device images are worked on, in runs of candidates that span at most "tmatch_chunk_mb". */
typedef struct cbh_tm_params {
  int32_t needle_features, haystack_features, cv_thresh, tm_scale_pct; /* src/index.h:76-84: 100, 1000, 25, 200 */
} cbh_tm_params;
enum {                              /* the exits of the reference's loop */
  CBH_TM_SCORED = 0,
  CBH_TM_NO_TEMPLATE_KEYPOINTS = 1, /* :127-130, every candidate of the call; cand_scale 1 and the candidate's own size */
  CBH_TM_NO_KEYPOINTS = 2,          /* :210-213 (the reference continues without caching) */
  CBH_TM_NO_MATCHES = 3,            /* :230-235 */
  CBH_TM_FEW_POINTS = 4,            /* :255-260 */
  CBH_TM_NO_TRANSFORM = 5,          /* :268-273; also a candidate outside the warp's domain (cbh_template_match) */
  CBH_TM_EMPTY_RESIZE = 6           /* a resize target side of 0: the reference's cv::resize throws */
};
typedef struct cbh_tm_image_result {
  cbh_template_result r;        /* as cbh_template_match gives it; score INT32_MAX unless status == CBH_TM_SCORED */
  float cand_scale;             /* 1 when not resized */
  int32_t status;
  int32_t w, h;                 /* the candidate's size after the resize */
  uint32_t n_keypoints, n_matches;
} cbh_tm_image_result;
/* images in host memory; patches: NULL or n x th x tw x channels */
int cbh_template_match_images(const uint8_t* tmpl, int tw, int th, size_t tmpl_row_stride, const uint8_t* imgs,
                              size_t imgs_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                              const uint32_t* img_h, const uint32_t* img_row_stride, int channels,
                              const cbh_tm_params* params, cbh_tm_image_result* results, uint8_t* patches, int device);
/* images (and d_patches: NULL or 16-byte aligned) in device memory; the size tables and the results are host memory.
 * Returns with the stream synchronised. */
int cbh_template_match_images_dev(const void* d_tmpl, int tw, int th, size_t tmpl_row_stride, const void* d_imgs, size_t n,
                                  const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                                  const uint32_t* img_row_stride, int channels, const cbh_tm_params* params,
                                  cbh_tm_image_result* results, void* d_patches, int device, void* stream);
/* Its stages.  All return with the stream synchronised (their tables are host memory).
 * sizeScaleFactor's cv::resize(INTER_LANCZOS4) (src/cvutil.cpp:1955) for n ragged images, image i from img_w[i] x
 * img_h[i] to dst_w[i] x dst_h[i], every channel with cbh_resize_lanczos4_dev's arithmetic; the results are packed
 * (pitch dst_w * channels) at d_dst + dst_off[i], 16-byte aligned offsets the caller lays out. */
int cbh_resize_lanczos4_ragged_dev(const void* d_src, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                                   const uint32_t* img_h, const uint32_t* img_row_stride, int channels,
                                   const uint64_t* dst_off, const uint32_t* dst_w, const uint32_t* dst_h, void* d_dst,
                                   int device, void* stream);
/* cvtColor(BGR2GRAY / BGRA2GRAY) as ORB applies it to a colour input (channels 3 / 4; a grey image needs no copy): grey
 * planes with pitch img_w[i] at d_dst + dst_off[i] (16-byte aligned) */
int cbh_bgr2gray_ragged_dev(const void* d_src, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                            const uint32_t* img_row_stride, int channels, const uint64_t* dst_off, void* d_dst, int device,
                            void* stream);
/* radiusMatch (:134, :217) and the point lists (:221-250) for n candidates as cbh_orb_dev left them: candidate i has
 * min(d_counts[i], kp_cap) descriptor rows d_desc[(i * kp_cap + j) * 32] and points d_xy[2 * (i * kp_cap + j)] (kp_after);
 * the train set is n_train template rows d_tmpl_desc / points d_tmpl_xy.  Every (query, train) pair with distance <=
 * max_dist (0..256), grouped by candidate, inside a candidate by query row, inside a query ascending (distance, train
 * row) -- cbh_idx256_radius_match's order.  first (host, n + 1): candidate i owns entries first[i] .. first[i + 1] of
 * d_tmpl_pts / d_match_pts (x, y floats) and of d_records (NULL, or cbh_dmatch with query_idx = the row inside its
 * candidate).  CBH_E_OVERFLOW with first complete and nothing written when first[n] > points_cap.  kp_cap <= 2^23,
 * n_train <= 2^20, kp_cap * n_train < 2^32. */
int cbh_tm_match_points_dev(const void* d_tmpl_desc, const void* d_tmpl_xy, size_t n_train, const void* d_desc,
                            const void* d_xy, const void* d_counts, size_t n, int kp_cap, int max_dist, void* d_records,
                            void* d_tmpl_pts, void* d_match_pts, size_t points_cap, uint64_t* first, int device,
                            void* stream);

/* ---- TemplateMatcher::match for a batch of result groups (Database::similar with params.templateMatch,
 * src/database.cpp:1418: once per needle there) ------------------------------------------------------------------------
 * One ragged image table (img_off / img_w / img_h / img_row_stride, one channel count per call) and n_pairs (template
 * image, candidate image) pairs that index it; an image may be a template in some pairs and a candidate in others,
 * pair_tmpl[p] == pair_cand[p] is legal, and the pairs of one template need not be adjacent (the entry groups them itself).
 * results[p], in the caller's pair order, is byte for byte what cbh_template_match_images returns for template = image
 * pair_tmpl[p], candidates = [image pair_cand[p]] and the same params -- every status, CBH_TM_NO_TEMPLATE_KEYPOINTS for
 * every pair of a template without keypoints, cand_scale, w, h, n_keypoints, n_matches.  There are no patches.
 * The distinct templates of a chunk go through grey and ORB once, the candidates once per pair (the resize target depends
 * on the pair's template; ORB is not shared between unresized occurrences of one image); the host waits for the two sets
 * of ORB counts, the match counts and the results per chunk, however many templates it holds.  Chunks: pairs whose
 * working set (templates once, candidate images, patches) stays within "tmatch_chunk_mb".
 * n_imgs, n_pairs <= 2^24; an index >= n_imgs, a template side above 8192 or a candidate that reaches ORB above 8192:
 * CBH_E_INVAL; zero pairs: CBH_OK with nothing read.  cbird_amd/csrc/tmimages.hip. */
int cbh_template_match_pairs(const uint8_t* imgs, size_t imgs_bytes, size_t n_imgs, const uint64_t* img_off,
                             const uint32_t* img_w, const uint32_t* img_h, const uint32_t* img_row_stride, int channels,
                             const uint32_t* pair_tmpl, const uint32_t* pair_cand, size_t n_pairs,
                             const cbh_tm_params* params, cbh_tm_image_result* results, int device);
/* images in device memory; every table and the results are host memory.  Returns with the stream synchronised. */
int cbh_template_match_pairs_dev(const void* d_imgs, size_t n_imgs, const uint64_t* img_off, const uint32_t* img_w,
                                 const uint32_t* img_h, const uint32_t* img_row_stride, int channels,
                                 const uint32_t* pair_tmpl, const uint32_t* pair_cand, size_t n_pairs,
                                 const cbh_tm_params* params, cbh_tm_image_result* results, int device, void* stream);
/* Its two own stages.  cbh_tm_match_points_dev with a train set per candidate: template g owns rows tmpl_first[g] ..
 * tmpl_first[g + 1] (host, n_tmpl + 1, ascending from 0, below 2^32) of d_tmpl_desc / d_tmpl_xy, candidate i is matched
 * against template tmpl_of[i] (host, n); train_idx counts inside the candidate's own set.  Otherwise that entry's
 * contract, CBH_E_OVERFLOW included; the n_train limits apply to the largest set. */
int cbh_tm_match_points_pairs_dev(const void* d_tmpl_desc, const void* d_tmpl_xy, const uint64_t* tmpl_first, size_t n_tmpl,
                                  const uint32_t* tmpl_of, const void* d_desc, const void* d_xy, const void* d_counts,
                                  size_t n, int kp_cap, int max_dist, void* d_records, void* d_tmpl_pts, void* d_match_pts,
                                  size_t points_cap, uint64_t* first, int device, void* stream);
/* cbh_warp_affine_dev with a patch size per candidate: candidate i warps into tw[i] x th[i] pixels (pitch tw[i] *
 * channels) at d_patches + patch_off[i] (host tables; offsets 16-byte aligned, patches must not overlap).  No byte outside
 * a patch is written. */
int cbh_warp_affine_ragged_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                               const uint32_t* img_h, const uint32_t* img_row_stride, int channels, const void* d_m,
                               const void* d_found, const uint32_t* tw, const uint32_t* th, const uint64_t* patch_off,
                               void* d_patches, void* d_warped, int device, void* stream);
/* Measurement (tools/template_pairs_bench.py): reads the device-event times the grouped entry has summed since the last
 * call -- ms5: grey and resize, ORB of the templates, ORB of the candidates, match + gather, estimate to score; sizes:
 * runs of one template size; hash_launches: launch_dcthash calls -- then clears them and switches the clock on or off.
 * While it is on every stage ends in a host wait of its own: never leave it on outside a measurement. */
int cbh_tm_pairs_stage_ms(int on, double* ms5, uint32_t* sizes, uint32_t* hash_launches);

/* ---- CvFeaturesIndex: src/cvfeaturesindex.{h,cpp} ---------------------------------------------------
 * N x 32-byte ORB/BRIEF descriptor rows (cv::Mat CV_8U, cvfeaturesindex.h:73) + the first-row -> mediaId
 * map (_indexMap/_idMap, :77-81).  Searches are exact brute force (the reference asks a FLANN LSH index,
 * :497, which returns a subset). */
cbh_idx256* cbh_idx256_create(int device);
/* ONE CvFeaturesIndex over several GPUs / logical shards in one process (as cbh_idx64_create_sharded): sharded BY IMAGE
 * -- a media's descriptor rows stay together (runs of 16384 rows per shard in add order), the first-row -> mediaId maps
 * stay with the handle in global row numbers, every search scans all shards on their own devices and streams, rewrites
 * the shard-local rows of the records to global ones and merges them on the first device of the mask (device-to-device
 * copies inside a device, one grouped ncclAllGather between devices).  Every other cbh_idx256_* call accepts the handle
 * and returns what the one-device index returns, bit for bit (the knn tie-break is (distance, global row)). */
cbh_idx256* cbh_idx256_create_sharded(uint32_t device_mask, int shards_per_device);
int cbh_idx256_shard_count(const cbh_idx256*);
size_t cbh_idx256_shard_rows(const cbh_idx256*, int i); /* rows held by shard i */
int cbh_idx256_shard_stats(const cbh_idx256*, cbh_shard_stats* out);
void cbh_idx256_destroy(cbh_idx256*);
/* add() (:122-150): append one media's rows; n_rows == 0 is skipped ("no descriptors for ...").
 * load() is add() per row of `select media_id,... from matrix`. */
int cbh_idx256_add(cbh_idx256*, uint32_t media_id, const uint8_t* rows, size_t n_rows);
/* remove() (:152-165): the map entry's id becomes 0, descriptors stay and keep taking knn places */
int cbh_idx256_remove(cbh_idx256*, const uint32_t* ids, size_t n);
int cbh_idx256_is_loaded(const cbh_idx256*);
size_t cbh_idx256_count(const cbh_idx256*);        /* count() = _descriptors.rows (:103) */
size_t cbh_idx256_memory_usage(const cbh_idx256*); /* memoryUsage() = 2 * rows * 32 (:105-120) */
/* descriptorsForMediaId (:421-436): row range of a media; download of a row range */
int cbh_idx256_rows_of(const cbh_idx256*, uint32_t media_id, size_t* first, size_t* count);
int cbh_idx256_download_rows(const cbh_idx256*, size_t first, size_t count, uint8_t* out);
/* slice() (:285-309): a new index of the same device or sharded shape with the rows of the listed media, built as add()
 * in ascending id order builds it -- ids may come in any order and repeat; an id without rows is skipped; a media that
 * was remove()d keeps its rows and comes back under its id, as cbh_idx256_rows_of still reports it (_idMap, :152-165).
 * The rows move on the device.  Takes the index's search lock.  Caller destroys the result; NULL +
 * cbh_last_error_code() on failure, the parent stays usable. */
cbh_idx256* cbh_idx256_slice(const cbh_idx256*, const uint32_t* ids, size_t n);
/* exact `knnSearch(needles, k)` below thresh: out_row/out_dist[nq*k] ordered (distance, row), counts[nq] =
 * rows under thresh.  nq < 2^23. */
int cbh_idx256_knn(cbh_idx256*, const uint8_t* needles, size_t nq, int k, int thresh, uint32_t* out_row,
                   uint16_t* out_dist, uint32_t* counts);
/* Multi-GPU halves of find() (shard by image): the knn table with the mediaId of every candidate row
 * (0 = removed; the first-row -> mediaId map is shard-local), and the scoring of a (merged) table -- votes per media,
 * median distance * 1000 / votes (:499-596; host code), needle i owning table rows [offsets[i], offsets[i+1]). */
int cbh_idx256_knn_media(cbh_idx256*, const uint8_t* needles, size_t nq, int k, int thresh, uint32_t* out_row,
                         uint16_t* out_dist, uint32_t* out_media, uint32_t* counts);
int cbh_cvfeatures_score(const uint32_t* media, const uint16_t* dist, const uint32_t* counts, const uint64_t* offsets,
                         size_t n_needles, int k, cbh_match* out, size_t cap, uint64_t* out_offsets);
/* find() (:438-604): knn k (reference: 10) per needle descriptor, distance < thresh (cvThresh), votes per
 * media, score = median distance * 1000 / votes; results ascending mediaId. */
int cbh_idx256_find(cbh_idx256*, const uint8_t* needle_rows, size_t n_desc, int thresh, int k, cbh_match* out,
                    size_t cap, size_t* n_out);
int cbh_idx256_find_batch(cbh_idx256*, const uint8_t* needle_rows, const uint64_t* offsets, size_t n_needles,
                          int thresh, int k, cbh_match* out, size_t cap, uint64_t* out_offsets);
/* TemplateMatcher's descriptor match (src/templatematcher.cpp:134,217): cv::BFMatcher(NORM_HAMMING).radiusMatch with
 * the index rows as the train set (load the template's descriptors with cbh_idx256_add): every (query, train) pair
 * with distance <= max_dist, grouped by query, each group in ascending (distance, train row) order (OpenCV: by
 * distance, ties unspecified).  out_first has nq + 1 entries; returns CBH_E_OVERFLOW (with out_first complete) when
 * cap is too small.  The steps after it (estimateRigidTransform's RANSAC, warpAffine, the score) are
 * cbh_template_match; gathering its point lists from these records and the keypoints is the caller's (:241-250) --
 * or cbh_tm_match_points_dev's, which matches and gathers for a batch of candidates on the device. */
typedef struct {
  int32_t query_idx, train_idx, distance; /* cv::DMatch::queryIdx, trainIdx, distance */
} cbh_dmatch;
int cbh_idx256_radius_match(cbh_idx256*, const uint8_t* queries, size_t nq, int max_dist, cbh_dmatch* out,
                            size_t cap, uint64_t* out_first);

/* ---- ColorDescIndex: src/colordescindex.{h,cpp}; ColorDescriptor: src/cvutil.h:57-113 -----------------
 * A descriptor is the reference's 258-byte struct: 32 x {l,u,v,w : uint16} + numColors : uint8 (+1 pad). */
#define CBH_COLOR_DESC_BYTES 258
typedef struct cbh_color cbh_color;
cbh_color* cbh_color_create(int device);
void cbh_color_destroy(cbh_color*);
int cbh_color_add(cbh_color*, const uint32_t* ids, const void* descs, size_t n); /* load/add :123-168,201-213 */
int cbh_color_remove(cbh_color*, const uint32_t* ids, size_t n);                  /* remove :215-229 */
size_t cbh_color_count(const cbh_color*);
int cbh_color_is_loaded(const cbh_color*);                                       /* _count > 0 (:114) */
size_t cbh_color_memory_usage(const cbh_color*);                                 /* (258 + 4) * count (:118-121) */
int cbh_color_find_index_data(const cbh_color*, uint32_t id, void* out_desc);    /* :231-239; returns 1/0 */
int cbh_color_download(const cbh_color*, uint32_t* ids, void* descs, size_t cap);
/* slice() (:231-248): a new index on the same device with the entries whose id is listed, in index order (a listed 0
 * keeps removed entries).  The device planes are gathered from the parent's on the device.  Takes the index's search
 * lock, and under it creates the parent's stream if no search has yet: const here means that the parent's entries do
 * not change, not that the handle is untouched.  Caller destroys the result; NULL + cbh_last_error_code() on failure,
 * the parent stays usable. */
cbh_color* cbh_color_slice(const cbh_color*, const uint32_t* ids, size_t n);
/* find() (:250-278) with ColorDescriptor::distance (src/cvutil.cpp:682-749): every entry whose distance is
 * finite (both sides have colours, counts differ by <= 2) and whose id != 0, in index order,
 * score = int(1 + sum of nearest-colour distances).  Bit-exact to the reference's float arithmetic. */
int cbh_color_find(cbh_color*, const void* needle_desc, cbh_match* out, size_t cap, size_t* n_out);
/* cbh_color_find for nq needles in one pass (needle q: out[out_offsets[q] .. out_offsets[q+1]), index order) */
int cbh_color_find_all_batch(cbh_color*, const void* needle_descs, size_t nq, cbh_match* out, size_t cap,
                             uint64_t* out_offsets);
/* ColorDescriptor::distance (src/cvutil.cpp:682-749) as FLOATS, nq needles x every index entry: out[q*count + i]
 * for entry i in add order (whatever its id); FLT_MAX where the reference returns FLT_MAX (:683-684).  The int
 * scores of cbh_color_find are (int) of exactly these values. */
int cbh_color_distances(cbh_color*, const void* needle_descs, size_t nq, float* out);
/* many needles + the sort/cut of Database::searchIndex: first min(counts[q], k) matches by (score, id) */
int cbh_color_find_batch(cbh_color*, const void* needle_descs, size_t nq, int k, cbh_match* out,
                         uint32_t* counts);
/* -sort-similar with -p.alg color for a ragged batch of selections (cbh_sort_similar_table has the loop's rules and the
 * outputs): per selection the table the loop's queries would see is filled on the device and walked by one workgroup.
 *   in_index[c]  this index holds id c as a live entry (removed entries have id 0 and are no candidates, :272-273)
 *   candidate c  the index's own descriptor, gathered on the device as cbh_color_slice does
 *   needle r     the caller's descriptor (needle_descs, n x 258 bytes parallel to ids) when its numColors > 0, else the
 *                index's entry for that id when held (findIndexData, :257-266), else none: the row is all 0xFFFF;
 *                needle_descs NULL: the index's for every item
 *   table[r][c]  (int) ColorDescriptor::distance(needle_r, entry_c), the needle as the first argument -- the distance is
 *                not symmetric when both sides have equal numColors (src/cvutil.cpp:702-708); FLT_MAX (a side without
 *                colours, counts that differ by more than 2) is 0xFFFF.  The arithmetic is cbh_color_find's, "color_fma"
 *                included: the scores are its scores bit for bit.  A score is at most 1 + 32 * sqrt(100^2 + 354^2 +
 *                262^2) < 14 454 (src/cvutil.h:83-87), so a uint16_t holds it.
 * The tables are filled in row chunks ("color_chunk_scores") and a batch goes in groups of consecutive sets whose tables
 * (n rows of n rounded up to 8 scores, 2 bytes each) fit "color_sort_table_kb" (default 2 GiB).  CBH_E_UNSUPPORTED: a set
 * above CBH_COLOR_SORT_SIMILAR_MAX items or whose own table does not fit that budget, or the index holds a listed id
 * more than once; CBH_E_INVAL as cbh_sort_similar_table; CBH_E_NOMEM when an allocation is refused (nothing is kept,
 * the handle stays usable).  Takes the index's search lock, like cbh_color_slice. */
#define CBH_COLOR_SORT_SIMILAR_MAX 32768
int cbh_color_sort_similar(cbh_color*, const uint32_t* ids, const void* needle_descs, const uint32_t* dir_id,
                           const uint8_t* under_prefix, const uint64_t* set_first, size_t n_sets,
                           const cbh_sort_table_params* params, uint32_t* out_ids, cbh_sort_similar_result* out);

/* Knobs (34). Results never change with any of them except "color_fma".  Unknown keys return CBH_E_INVAL.
 * Which kernel serves a call:
 *   "scan_mfma"     64-bit scan on the matrix cores (k_hamm64_mfma*): 0 = never (the popcount kernel k_hamm64_scan), 1 = calls
 *                   with >= 256 needles and >= 4096 slots (default), 2 = always; 3 = as 1, and calls with thresholds <= 8 and
 *                   no needle masks whose scan would take >= 1 ms go to the bucketed join (hamm64_join.hip: multi-index
 *                   hashing -- only pairs that share one of max(4, thresh) chunk values are compared; the same records) when
 *                   its exact candidate count says it is cheaper; 4 = the join for every call it can represent (tests).
 *                   The join avoids comparisons rather than making them faster: it is opt-in, the default compares every pair.
 *                   Other values return CBH_E_INVAL and leave the knob as it was
 *   "join_resident" which handles keep the join's slot tables between calls (cbh_idx64_join_prepare above): 0 (default) =
 *                   those opted in by cbh_idx64_join_prepare, 1 = every handle, built by its first joined call at a plan.
 *                   Other values return CBH_E_INVAL and leave the knob as it was
 *   "join_resident_mb" what those tables may hold per index (per shard of a sharded handle), all plans together, in MB
 *                   (default 2048: every plan of 5 * 10^6 slots; a plan costs 12 m n bytes).  A plan that would not fit is
 *                   not kept: the call prepares the slots itself, as without tables.  Negative values: CBH_E_INVAL
 *   "scan_mfma_pre_max" prefilter kernel or three-field 64-bit kernel: -1 (default) = per launch, by the candidate rate of the
 *                   launch's own data -- r_cand = P[popc(fold(a) ^ fold(b)) < thresh] and r_true = P[hamm64(a, b) < thresh], counted
 *                   on 2048 x 2048 sampled (slot, needle) pairs by k_fold_probe; the prefilter while r_cand - 8 r_true <=
 *                   "scan_pre_rate_e9" (a candidate costs the prefilter a re-check, a true match costs the three-field kernel
 *                   eight times that more than it costs the prefilter); launches of < 2^31 pairs: thresholds <= 6 -- 0 = never the prefilter, t > 0 =
 *                   thresholds <= t (<= 32) take it whatever the data
 *   "scan_pre_rate_e9" that bound x 1e9 (default 300000 = 3.0e-4: where the two kernels tie, profiles/r07_adaptive_ab_*.jsonl)
 *   "scan_pre48"    the 48-bit prefilter kernel (16 folds + 32 plain bits; three MFMAs per four needle tiles): -1 (default) =
 *                   per launch, where the probe's rates model it faster than the three-field kernel, or than 0.9 x the
 *                   prefilter's time, whichever of the two the launch would otherwise take; 0 = never; 1 = always for
 *                   thresholds <= 16.  Launches too small to probe never take it
 *   "scan_pre16"    the 16-bit prefilter kernel (the fold lo ^ hi folded once more; ONE MFMA per four needle tiles, half the
 *                   32-bit prefilter's matrix work, for candidates at the rate of 16-bit words): -1 (default) = per launch,
 *                   where the probe's rates model it below 0.9 x the 32-bit prefilter's time -- threshold 1 of unrelated
 *                   hashes; 0 = never; 1 = always for thresholds <= 8 (larger thresholds are routed as with -1).  Other
 *                   values return CBH_E_INVAL and leave the knob as it was.  Launches too small to probe never take it
 *   "scan256_mfma"  256-bit scan on the matrix cores (k_hamm256_*): 0 = never (k_hamm256_scan), 1 = calls with >= 64 needle
 *                   descriptors and >= 4096 rows (default), 2 = always.  Other values return CBH_E_INVAL and leave the knob
 *                   as it was
 *   "scan256_small" 1 = searches with <= 512 needle descriptors (one ORB needle image) and thresholds <= 40 use the
 *                   stationary-needle kernel k_hamm256_small (default), 0 = the row-stationary kernels.  Other values return
 *                   CBH_E_INVAL and leave the knob as it was
 *   "hash_mfma"     256 x 256 tiles: non-zero (default 2) = k_dcthash_256_band (the 7 x 7 box filter as i8 MFMAs, its vertical
 *                   sum kept in their accumulators; rows must be 16-byte aligned, otherwise 0 is taken), 0 = k_dcthash_256
 *                   (all VALU; also what runs if the band table cannot be made)
 *   "hash_band_area" fractional resize ratios, 7 x 7 blur, <= 1920 columns: 1 (default) = k_band_area (the matrix-core blur
 *                   for any width and height; whole images and views whose vertical edges are the parent's or lie >= 8 / >= 3
 *                   columns inside it), 0 = the VALU kernels that serve every other geometry
 *   "hash_stream"   the VALU kernels: 1 (default) = k_blur_area_regs walks strips of 3..8 steps when the batch has enough
 *                   workgroups for that, k_blur_area (a workgroup per 16-row band) otherwise; 0 = always the band kernel;
 *                   v >= 2 = always strips, of v steps
 *   "hash_fuse"     k_blur_area_regs: 1 (default) = vertical INTER_AREA pass and tile inside the kernel when a workgroup per
 *                   image still fills the machine, 2 = always, 0 = never (k_tile_hash reads the rows back)
 *   "kp_lds_side"   largest keypoint square k_kp_hashes stages in LDS (default 134; larger: global-memory routine)
 *   "kp_blur_side"  largest keypoint square whose blurred copy also stays in LDS (default 112)
 *   "fdct_host_vote", "video_host_reduce"  the per-needle reductions of DctFeaturesIndex / DctVideoIndex finds: 0 (default) =
 *                   on the device for batches, on the host for a single needle; 1 = host, 2 = device
 *   "color_create_group" images per wave of ColorDescriptor::create's seeding kernel k_cdw_round<G>: 0 (default) = by the
 *                   chunk's size (G = 1 up to 2048 images, 2 up to 4096, 4 up to 8192, 8 up to 16384, 16 up to 32768, 21 above),
 *                   1 / 2 / 4 / 8 / 16 / 21 = that G for every chunk (tests: every instantiation on a few dozen images).  Other
 *                   values return CBH_E_INVAL and leave the knob as it was
 *   "orb_retain_order" KeyPointsFilter::retainBest: 1 (default) = the survivors in the order libstdc++'s nth_element +
 *                   partition leave them (cbird's Linux builds), 0 = canonical (every tie kept, raster order)
 * The one knob that CHANGES results (within north_star's float tolerance; not the default: the shipped kernel is
 * deliberately stricter -- raw floats bitwise equal to ColorDescriptor::distance -- at a cost of 9 % of its time):
 *   "color_fma"     1 = dl^2 + du^2 + dv^2 with fused multiply-adds: distances within 1e-5 (relative) of the reference's,
 *                   int(score) can move by one at an integer boundary (2 of 188 902 on profiles/r04_knobs_area_color.json)
 * Memory:
 *   "color_create_chunk_mb" scratch one launch of ColorDescriptor::create may take, in MB (default 32768): larger batches
 *                   are worked off in chunks of that many images (1.6 MB per 256 x 192 image)
 *   "color_chunk_scores" the most score elements (needles x entries) one chunk of the needle loops of
 *                   cbh_color_find_batch, cbh_color_find_all_batch and cbh_color_distances may hold: 0 (default) = 2^28 /
 *                   2^27 / 2^27; at least one needle per chunk (tests: the later chunks on a small index).  Negative
 *                   values return CBH_E_INVAL and leave the knob as it was
 *   "color_sort_table_kb" KiB of score tables one group of sets of cbh_color_sort_similar may hold: 0 (default) = 2 GiB; a
 *                   set whose own table does not fit is CBH_E_UNSUPPORTED (tests: several groups on small sets).
 *                   Negative values return CBH_E_INVAL and leave the knob as it was
 *   "color_sort_timing" 1 = cbh_color_sort_similar times its table fill and its chain apart with events and waits for
 *                   each group (tools/sort_similar_color_bench.py); read "color_sort_fill_us" / "color_sort_chain_us"
 *   "cluster_chunk" needle entries per scan of cbh_idx64_clusters / cbh_idx64_cluster_labels: 1 .. 2^25 (default 2^20; tests:
 *                   several chunks on a small index).  Other values return CBH_E_INVAL and leave the knob as it was
 *   "cluster_max_records" records one of those scans may materialise (default 2^26 = 512 MB): a range with more is halved
 *                   and scanned again.  Values below 1 return CBH_E_INVAL and leave the knob as it was
 *   "cluster_timing" 1 = the cluster calls time their stages apart with events and wait for each
 *                   (tools/clusters_bench.py); read "cluster_table_us" / "cluster_hook_us" / "cluster_emit_us"
 *   "vcover_chunk"  destination entries one workgroup of cbh_video_coverage takes: 0 (default) = 4096, halved down to 256
 *                   while the batch has fewer than 2048 workgroups; 1 .. 2^24 = that many (tests: several chunks on short
 *                   videos).  Other values return CBH_E_INVAL and leave the knob as it was
 *   "vcover_tile"   source frames one workgroup of it takes: 256, 512, 1024 (default) or 2048, that is 1, 2, 4 or 8 per
 *                   lane.  Other values return CBH_E_INVAL and leave the knob as it was
 *   "vseg_budget_mb" what the difference arrays of one group of pairs of cbh_video_segments may take together, in MB:
 *                   1 .. 4096 (default 256).  Other values return CBH_E_INVAL and leave the knob as it was
 *   "quality_chunk_mb" what one upload of cbh_quality_scores, and the working planes of one group of launches of
 *                   cbh_quality_scores_dev, may take, in MB (default 1024; at least one image each)
 *   "tmatch_chunk_mb" what one upload of cbh_template_match, and the patches of one group of candidates of
 *                   cbh_template_match_dev when the caller does not take them, may take, in MB (default 1024)
 *   "pool_keep_mb"  cached scratch that may outlive its stream, per device, in MB (default 16384; < 0: everything)
 *   "pool_live_keep_mb" what the cache of a LIVE stream may hold, in MB (0 = default: a quarter of the device's memory, at
 *                   least 16384; < 0: everything).  Beyond it the blocks freed longest ago go back to the driver once the
 *                   work queued behind them has run.  Whatever is cached stays reclaimable: an allocation the driver
 *                   refuses -- scratch or index storage alike -- gives the device's cached blocks back and is tried again
 * Multi-device handles:
 *   "shard_force_rccl" 1 = a sharded index on ONE device still sends its blocks through ncclAllGather (one rank): the
 *                   transport test of a one-GPU box (default 0)
 *   "shard_exchange" how the records of a multi-device index reach the root device: 1 = hipMemcpyPeerAsync of exactly
 *                   count_s records per shard into the root block (default: only the root consumes them), 0 = one
 *                   grouped ncclAllGather of the per-device blocks (falls back to 1, with a note in cbh_last_error, when
 *                   librccl cannot be loaded, its version does not match the headers, or ncclCommInitAll fails)
 * Fault injection (tests/test_error_paths.py; never armed by the library itself):
 *   "fault_alloc_after" n >= 0: the n-th allocation from now (0 = the next; device, pinned and scratch allocations all
 *                   count) fails once with out-of-memory and the knob disarms itself; -1 disarms
 *   "fault_alloc_sticky" 1 = once that countdown has run out, every later allocation fails too, until disarmed
 *   "fault_driver_oom" n >= 0: the n-th driver allocation of the scratch arena is refused once (its trim-and-retry path)
 *   "fault_persist_oom" n >= 0: the n-th allocation of index / workspace / table memory is refused by the driver once (the
 *                   arena gives its cached blocks of the device back, the allocation is tried again)
 *   "fault_rccl"    1 = librccl is treated as absent
 * (Rounds 1-5 carried 57 knobs, most of them A/B switches between kernel generations; the losers and their switches
 * went with round 6 -- git history and NOTES.md keep what each measured.) */
int cbh_set_tuning(const char* key, int value);
/* Read-back for tests and soak tools: "fault_alloc_after" (what is left of the countdown, -1 = disarmed or fired),
 * "fault_fired", "alloc_calls" (allocations seen since the library loaded), and the scratch arena's
 * "arena_cached_bytes", "arena_pending_bytes", "arena_live_bytes", "arena_live_blocks", "arena_trimmed_live",
 * "arena_oom_retry_stream", "arena_oom_retry_device", "arena_oom_retry_persistent", "arena_released"; "scan_mfma" (the
 * knob's value); "scan_pre_mask"
 * (bit t = the most recent matrix-core launch at threshold t took the prefilter kernel), "scan_pre48_mask" (... took the
 * 48-bit prefilter kernel; a launch sets its bit in at most one of the two), "scan_pre16_mask" (... took the 16-bit prefilter
 * kernel; such a launch sets its bit in "scan_pre_mask" as well: it is a fold prefilter), "scan_joins" (calls the bucketed join has answered), "join_needle_preps" (needle sides -- histogram, starts,
 * chunk-ordered copies -- the join has prepared at thresholds 5..8: one per launch, one per device and call on a sharded handle that keeps
 * tables), "join_resident" / "join_resident_mb" (the knobs' values), "scan_probes" (candidate-rate
 * probes run so far), "scan_probe_rate_e9" / "scan_probe_true_e9" / "scan_probe_rate48_e9" / "scan_probe_rate16_e9" (the candidate and true-match rates the last one
 * found for its threshold and the 48-bit and 16-bit prefilters' candidate rates, x 1e9; -1 = none yet); "scan256_mfma", "scan256_small", "color_create_group" (the knobs' values);
 * "color_create_group_last" (the G of the most recent k_cdw_round<G> chunk launch, 0 before any; read-only); "scan256_kernels" (a bit mask of the kernels
 * that 256-bit scan launches have used since it was last cleared -- cbh_set_tuning("scan256_kernels", 0) clears it, any
 * other value written is CBH_E_INVAL; bit 0 k_hamm256_scan, 1 k_hamm256_mfma<6,3,2> (first-128-bit prefilter, one needle
 * tile per accumulator), 2 k_hamm256_mfma<6,3,4> (all 256 bits), 3 k_hamm256_mfma3, 4 / 5 / 6 k_hamm256_small<4 / 8 / 16>;
 * a sharded handle notes one launch per shard, a buffer that had to grow one per attempt); "slices_on_device" (the
 * cbh_idx256_slice and cbh_color_slice calls so far that succeeded on the device route, the one that
 * runs the kernels of slice.hip; a call that had nothing to move -- an empty list, an empty index, nothing kept --
 * counts too, although it launches none of them); "color_chunk_scores" (the knob's value); "color_sort_table_kb" (the
 * knob's value); "color_sort_groups" / "color_sort_fill_us" / "color_sort_chain_us" (of the last cbh_color_sort_similar
 * call that succeeded: the groups its sets went in and, with "color_sort_timing" 1, the microseconds its table fills and
 * its chains took on the device, else 0; read-only); "color_full_sorts" / "color_window_cuts" (needles of
 * cbh_color_find_batch sent through the full sort -- k above 4096, or more than 4096 candidates at or under the k-th score
 * -- / answered from the candidate list, since the library loaded; needles without a match, and k = 0, count as neither;
 * read-only); "quality_chunk_mb" (the knob's value); "quality_strip_rows" (rows of
 * the working plane one thread of the quality kernels walks: their strips start at every multiple of it; read-only);
 * "cluster_chunk" / "cluster_max_records" (the knobs' values); "cluster_table_us" / "cluster_hook_us" / "cluster_emit_us"
 * (of the last cluster call that succeeded, with "cluster_timing" 1: the microseconds its node table, its k_cl_hook +
 * k_cl_flatten launches and its output stage took on the device, else 0; read-only);
 * "tmatch_chunk_mb" (the knob's value); "diff_block_pixels" (consecutive pixels of one image a workgroup of the
 * difference-image passes takes: an image above it spans several workgroups; read-only). */
int cbh_get_tuning(const char* key, long long* value);

/* ---- measurement support ---------------------------------------------------------------- */
/* Run the scan kernel `iters` times on the index's own stream bracketed by hipEvents and
 * return the average kernel time in milliseconds (bench.py roofline leg).  */
int cbh_idx64_time_scan_dev(cbh_idx64*, const void* d_q, size_t nq, int thresh, void* d_records,
                            size_t cap, void* d_total, int iters, float* ms_avg);
int cbh_time_dcthash_dev(const void* d_imgs, size_t n, int w, int h, size_t row_stride,
                         size_t img_stride, void* d_out, int device, int iters, float* ms_avg);
/* The hardware behaviour three kernels rely on (k_hamm256_small's row tiles past the end, k_band_area's rows at the end of
 * the buffer, the prestage first look): a raw buffer load whose SCALAR offset alone carries it past the descriptor's
 * num_records -- the per-lane offset inside the range -- returns zeros and touches nothing.  Loads a 4 KB window of an
 * 8 KB allocation whose second half is poisoned, with scalar offsets inside, at and beyond the window's end; *ok = 1 iff
 * every load that starts at or past num_records returned 0 and every load inside it returned the data
 * (tests/test_boundary.py; no product call depends on this entry point). */
int cbh_selftest_buffer_range(int device, int* ok);
/* The FP4 arithmetic the 48-bit prefilter of the 64-bit scan rests on (hamm64_mfma.hip): the values 0.5 (E2M1's one
 * subnormal), 1 and 4 under the block scales 2, 2^7, 2^10, 2^13, 2^19.  One 32x32x64 MFMA per combination, everything
 * else zero: out[(((ia * 6 + ib) * 5 + k) * 2 + c) * 2 + kb] = cnt * a * b * scale as the hardware returns it, a, b of
 * {0.5, -0.5, 1, -1, 4, -4} by ia, ib, scale k of the five above, cnt = 1 | 16 elements by c, in K block kb.  720 floats
 * of host memory (tests/test_scan_prefilter48.py; no product call depends on this entry point). */
int cbh_selftest_fp4_products(int device, float* out);

#ifdef __cplusplus
}
#endif
#endif /* CBIRD_HIP_H */
