// quality.hip -- qualityScore(const Media&) (src/cimgops.cpp:313-596; makeDiff :37-60, makeEdge :88-121, longEdgeCount
// :131-152) for a ragged batch of images: the edge ratio plus long-edge ratio of the red channel of the cropped image.
//
// The reference transposes the image three times so that one horizontal routine serves both directions; here both
// directions are stencils on one packed plane and the long-edge count is its local form -- a run is counted where a zero
// follows two set positions, at positions 3 .. L-2 of a line -- so no transpose exists.
//
// A thread owns kChunk consecutive working pixels of kStripRows consecutive rows and walks down them with the rows it
// needs in registers; a work item (one workgroup) is as many such strips of one image as fit 256 threads.  Three launches:
//   k_quality_pack   reads the cropped source rows once (16 * CH bytes per thread and row in CH 16-byte loads where the
//                    address allows, the red bytes one by one elsewhere), writes the working plane (rows padded to 16
//                    bytes, padding zero) and adds up |p(x-1) - p(x+1)| and |p(y-1) - p(y+1)|: v_sad_u8 on packed bytes,
//                    one 64-bit atomic per sum and workgroup
//   k_quality_edges  the same strips with two rows of halo above and below: thresholds from the sums, the difference and
//                    edge maps row by row, the union count and the two long-edge counts (one 32-bit atomic each per
//                    workgroup), and optionally the three diagnostic planes of addVisual (:430-432)
//   k_quality_score  one lane per image: the means, the score's float formula (:495-500, :592) and the detail record
// Everything but the two means and the formula is integer arithmetic, so the result does not depend on the schedule.
// Bound by HBM: w*h*CH source bytes in, one byte per working pixel out and back (three more with planes).
#include <climits>
#include <cstdint>

#include <algorithm>
#include <vector>

#include "cbh_index.h"
#include "cbh_runs.h"
#include "cbh_staging.h"

namespace cbh {
namespace {

constexpr int kStripRows = 16;  // rows a thread walks ("quality_strip_rows")
constexpr int kChunk = 16;      // working pixels per thread and row
constexpr int kBlock = 256;

int g_quality_chunk_mb = 1024;  // "quality_chunk_mb"

struct QImage {
  unsigned long long src_off, work_off, out_off;  // first source byte; working plane in the scratch; diagnostic planes
  unsigned w, h, stride;                          // source
  int qw, qh, pitch, hcrop, vcrop;                // working size (0 x 0: no score), bytes per working row, the crop
};
struct QItem {
  unsigned img, y0, cx0, ncx;  // rows from y0, chunks cx0 .. cx0 + ncx of every row; kBlock / ncx strips below each other
};
struct QCount {
  unsigned long long h_sum, v_sum;
  unsigned num_edges, h_long, v_long, pad;
};

__device__ __forceinline__ unsigned byte_of(const unsigned* v, int i) { return (v[i >> 2] >> (8 * (i & 3))) & 0xffu; }
__device__ __forceinline__ unsigned abs_diff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }
// bits j of 0..15 with lo <= j <= hi
__device__ __forceinline__ unsigned bit_range(int lo, int hi) {
  lo = max(lo, 0), hi = min(hi, 15);
  return hi < lo ? 0u : ((2u << hi) - 1u) & ~((1u << lo) - 1u);
}

// 0xff in the lowest n bytes of a dword (n <= 0: none, n >= 4: all)
__device__ __forceinline__ unsigned low_bytes(int n) { return n <= 0 ? 0u : n >= 4 ? 0xffffffffu : (1u << (8 * n)) - 1u; }

struct QTask {
  bool on;
  int x0, ys, ye;  // first column, rows ys .. ye
};
__device__ __forceinline__ QTask task_of(const QItem& it, const QImage& im) {
  const int t = (int)threadIdx.x, sub = t / (int)it.ncx;
  QTask k;
  k.x0 = ((int)it.cx0 + t - sub * (int)it.ncx) * kChunk;
  k.ys = (int)it.y0 + sub * kStripRows;
  k.ye = min(k.ys + kStripRows, im.qh);
  k.on = sub < kBlock / (int)it.ncx && k.ys < im.qh && k.x0 < im.qw;
  return k;
}

// the sums of every thread of the workgroup in thread 0 (all threads call)
template <int N>
__device__ __forceinline__ void block_sum(unsigned (&v)[N], unsigned* sh /* [4 * N] */) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v[i] += __shfl_down(v[i], d, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) sh[wave * N + i] = v[i];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = sh[i] + sh[N + i] + sh[2 * N + i] + sh[3 * N + i];
}

// the red bytes of working pixels x0 .. x0 + 15 of working row y, pixel j in byte j; 0 outside the working plane and
// outside the source (the inclusive crop's last column / row when the crop is 0, src.crop at :335)
template <int CH>
__device__ __forceinline__ void load_red16(const unsigned char* __restrict__ s, const QImage& im, int x0, int y,
                                           unsigned (&r)[4]) {
  constexpr int RO = CH == 1 ? 0 : 2;  // cv::Mat order: B G R (A)
  r[0] = r[1] = r[2] = r[3] = 0;
  if (y < 0 || y >= im.qh || (unsigned)(y + im.vcrop) >= im.h) return;
  const int nps = min(kChunk, min(im.qw - x0, (int)im.w - im.hcrop - x0));
  if (nps <= 0) return;
  const unsigned char* p = s + (size_t)(y + im.vcrop) * im.stride + (size_t)(x0 + im.hcrop) * CH;
  if (nps == kChunk && ((uintptr_t)p & 15) == 0) {
    unsigned px[4 * CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const uint4 q = reinterpret_cast<const uint4*>(p)[k];
      px[4 * k] = q.x, px[4 * k + 1] = q.y, px[4 * k + 2] = q.z, px[4 * k + 3] = q.w;
    }
#pragma unroll
    for (int j = 0; j < kChunk; ++j) r[j >> 2] |= byte_of(px, j * CH + RO) << (8 * (j & 3));
  } else {  // (a loop of nps steps into two 64-bit words: sixteen predicated loads would hold sixteen lane masks)
    unsigned long long lo = 0, hi = 0;
    for (int j = 0; j < nps; ++j) {
      const unsigned long long b = p[j * CH + RO];
      if (j < 8) lo |= b << (8 * j);
      else hi |= b << (8 * (j - 8));
    }
    r[0] = (unsigned)lo, r[1] = (unsigned)(lo >> 32), r[2] = (unsigned)hi, r[3] = (unsigned)(hi >> 32);
  }
}

template <int CH>
__global__ __launch_bounds__(kBlock) void k_quality_pack(const unsigned char* __restrict__ src,
                                                         const QImage* __restrict__ images,
                                                         const QItem* __restrict__ items,
                                                         unsigned char* __restrict__ work, QCount* __restrict__ counts) {
  constexpr int RO = CH == 1 ? 0 : 2;
  __shared__ unsigned sh[8];
  const QItem it = items[blockIdx.x];
  const QImage im = images[it.img];
  const QTask k = task_of(it, im);
  unsigned sums[2] = {0u, 0u};  // hd, vd
  if (k.on) {
    const unsigned char* s = src + im.src_off;
    unsigned char* wp = work + im.work_off;
    const int x0 = k.x0;
    unsigned a2[4] = {0u, 0u, 0u, 0u}, a1[4] = {0u, 0u, 0u, 0u}, a0[4];
    unsigned hm[4];  // 0xff in byte j of the chunk where the centre x0 + j + 1 lies in 1 .. qw - 2
#pragma unroll
    for (int q = 0; q < 4; ++q) hm[q] = low_bytes(im.qw - 2 - x0 - 4 * q);
    for (int y = k.ys - 2; y < k.ye; ++y) {
      load_red16<CH>(s, im, x0, y, a0);
      if (y >= k.ys) {
        *reinterpret_cast<uint4*>(wp + (size_t)y * im.pitch + x0) = make_uint4(a0[0], a0[1], a0[2], a0[3]);
        // hd(c, y) = |p(c-1) - p(c+1)| for the centres c = x0 + 1 .. x0 + 16 that lie in 1 .. qw - 2 (makeDiff :50-54)
        unsigned nx = 0;  // working pixels x0 + 16, x0 + 17
        if ((unsigned)(y + im.vcrop) < im.h) {
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int c = x0 + kChunk + j;
            if (c < im.qw && c + im.hcrop < (int)im.w)
              nx |= (unsigned)s[(size_t)(y + im.vcrop) * im.stride + (size_t)(c + im.hcrop) * CH + RO] << (8 * j);
          }
        }
        const unsigned e[5] = {a0[0], a0[1], a0[2], a0[3], nx};
#pragma unroll
        for (int q = 0; q < 4; ++q)  // (both operands masked: a centre outside 1 .. qw - 2 adds |0 - 0|)
          sums[0] = __builtin_amdgcn_sad_u8(e[q] & hm[q], __builtin_amdgcn_alignbyte(e[q + 1], e[q], 2) & hm[q], sums[0]);
        // vd(x, y - 1) = |p(y-2) - p(y)| for the centre rows 1 .. qh - 2, every column
        if (y >= 2)
#pragma unroll
          for (int q = 0; q < 4; ++q) sums[1] = __builtin_amdgcn_sad_u8(a2[q], a0[q], sums[1]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) a2[q] = a1[q], a1[q] = a0[q];
    }
  }
  block_sum(sums, sh);
  if (threadIdx.x == 0) {
    if (sums[0]) atomicAdd(&counts[it.img].h_sum, (unsigned long long)sums[0]);
    if (sums[1]) atomicAdd(&counts[it.img].v_sum, (unsigned long long)sums[1]);
  }
}

// mean = float(double(sum) / ((w-1) * (h-1))) (filterHorizontalMT :252), m = pixel_t(mean) (makeEdge :96).  A mean above
// 255 (working planes three rows high) keeps the low byte of the integer, as the reference's x86 build does
__device__ __forceinline__ float mean_of(unsigned long long sum, int qw, int qh) {
  return (float)((double)sum / (double)((qw - 1) * (qh - 1)));
}
__device__ __forceinline__ unsigned mean_byte(float mean) { return (unsigned)(int)mean & 0xffu; }

// working pixels x0 - 4 .. x0 + 19 of row y in six dwords, 0 outside the plane (the rows' padding is zero)
__device__ __forceinline__ void load_row(const unsigned char* __restrict__ wp, const QImage& im, int x0, int y,
                                         unsigned (&p)[6]) {
  if (y < 0 || y >= im.qh) {
#pragma unroll
    for (int q = 0; q < 6; ++q) p[q] = 0;
    return;
  }
  const unsigned char* row = wp + (size_t)y * im.pitch + x0;
  p[0] = x0 ? *reinterpret_cast<const unsigned*>(row - 4) : 0u;
  const uint4 q = *reinterpret_cast<const uint4*>(row);
  p[1] = q.x, p[2] = q.y, p[3] = q.z, p[4] = q.w;
  p[5] = x0 + kChunk < im.pitch ? *reinterpret_cast<const unsigned*>(row + kChunk) : 0u;
}

__device__ __forceinline__ void store16(unsigned char* __restrict__ d, const unsigned (&v)[4], int np) {
  if (np == kChunk && ((uintptr_t)d & 15) == 0) {
    *reinterpret_cast<uint4*>(d) = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
    const unsigned long long lo = v[0] | (unsigned long long)v[1] << 32, hi = v[2] | (unsigned long long)v[3] << 32;
    for (int j = 0; j < np; ++j) d[j] = (unsigned char)((j < 8 ? lo : hi) >> (8 * (j & 7)));
  }
}

template <bool PLANES>
__global__ __launch_bounds__(kBlock) void k_quality_edges(const QImage* __restrict__ images,
                                                          const QItem* __restrict__ items,
                                                          const unsigned char* __restrict__ work,
                                                          QCount* __restrict__ counts, unsigned char* __restrict__ planes) {
  __shared__ unsigned sh[12 + 2];
  const QItem it = items[blockIdx.x];
  const QImage im = images[it.img];
  const QTask k = task_of(it, im);
  if (threadIdx.x == 0) {
    sh[12] = mean_byte(mean_of(counts[it.img].h_sum, im.qw, im.qh));
    sh[13] = mean_byte(mean_of(counts[it.img].v_sum, im.qw, im.qh));  // the same divisor (h-1) * (w-1)
  }
  __syncthreads();
  const unsigned mh = sh[12], mv = sh[13];
  unsigned cnt[3] = {0u, 0u, 0u};  // numEdges, hLong, vLong
  if (k.on) {
    const unsigned char* wp = work + im.work_off;
    const int x0 = k.x0, qw = im.qw, qh = im.qh;
    const unsigned inner = bit_range(1 - x0, qw - 2 - x0);   // own columns inside 1 .. qw - 2
    const unsigned longs = bit_range(3 - x0, qw - 2 - x0);   // own columns that may end a run along x
    // 0xff in byte i where column x0 - 1 + i lies in 1 .. qw - 2, the centres of hd (held as data, not as lane masks)
    unsigned hv[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) hv[q] = low_bytes(qw - x0 - 4 * q) & ~low_bytes(2 - x0 - 4 * q);
    // rows r - 2 and r - 1 of the row r that arrives; byte j of a row is column x0 - 4 + j
    unsigned pm2[6], pm1[6];
    load_row(wp, im, x0, k.ys - 2, pm2);
    load_row(wp, im, x0, k.ys - 1, pm1);
    // vd > mv ? vd : 0 of rows r - 3 and r - 2 and vd of row r - 2, byte i = column x0 - 2 + i; hE of rows r - 3, r - 4
    unsigned cva[5] = {0u, 0u, 0u, 0u, 0u}, cvb[5] = {0u, 0u, 0u, 0u, 0u}, vdb[5] = {0u, 0u, 0u, 0u, 0u};
    unsigned he1 = 0, he2 = 0;
    for (int r = k.ys; r <= k.ye + 1; ++r) {
      unsigned pr[6];
      load_row(wp, im, x0, r, pr);
      unsigned vdc[5] = {0u, 0u, 0u, 0u, 0u}, cvc[5] = {0u, 0u, 0u, 0u, 0u};
      if (r - 1 >= 1 && r - 1 <= qh - 2) {
#pragma unroll
        for (int i = 0; i < 18; ++i) {
          const unsigned d = abs_diff(byte_of(pm2, i + 2), byte_of(pr, i + 2));
          vdc[i >> 2] |= d << (8 * (i & 3));
          cvc[i >> 2] |= (d > mv ? d : 0u) << (8 * (i & 3));
        }
      }
      const int y = r - 2;
      // hd and its candidates of row y at columns x0 - 1 .. x0 + 16, hE at the own columns (makeEdge :100-115)
      unsigned ch[18], hd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < 18; ++i) {
        const unsigned d = abs_diff(byte_of(pm2, i + 2), byte_of(pm2, i + 4)) & byte_of(hv, i);
        ch[i] = d > mh ? d : 0u;
        if (i >= 1 && i <= 16) hd[(i - 1) >> 2] |= d << (8 * ((i - 1) & 3));
      }
      unsigned he = 0;
#pragma unroll
      for (int j = 0; j < kChunk; ++j) he |= (ch[j + 1] > ch[j] && ch[j + 1] > ch[j + 2] ? 1u : 0u) << j;
      if (y >= k.ys) {
        unsigned ve = 0;  // bit i = column x0 - 2 + i
#pragma unroll
        for (int i = 0; i < 18; ++i) {
          const unsigned b = byte_of(cvb, i);
          ve |= (b > byte_of(cva, i) && b > byte_of(cvc, i) ? 1u : 0u) << i;
        }
        const unsigned any = ((ve >> 2) | he) & 0xffffu;
        if (y >= 1 && y <= qh - 2) cnt[0] += __popc(any & inner);
        // longEdgeCount (:139-148) on the transposed maps: hE in runs along y, vE in runs along x
        if (y >= 3 && y <= qh - 2) cnt[1] += __popc(~he & he1 & he2 & 0xffffu);
        cnt[2] += __popc(~(ve >> 2) & (ve >> 1) & ve & longs);
        if (PLANES) {
          const int np = min(kChunk, qw - x0);
          const size_t plane = (size_t)qw * qh;
          unsigned char* d = planes + im.out_off + (size_t)y * qw + x0;
          unsigned ev[4], vo[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            ev[q] = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) ev[q] |= ((any >> (4 * q + j)) & 1u ? 0xffu : 0u) << (8 * j);
            vo[q] = __builtin_amdgcn_alignbyte(vdb[q + 1], vdb[q], 2);
          }
          store16(d, ev, np);
          store16(d + plane, hd, np);
          store16(d + 2 * plane, vo, np);
        }
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) pm2[q] = pm1[q], pm1[q] = pr[q];
#pragma unroll
      for (int q = 0; q < 5; ++q) cva[q] = cvb[q], cvb[q] = cvc[q], vdb[q] = vdc[q];
      he2 = he1, he1 = he;
    }
  }
  block_sum(cnt, sh);
  if (threadIdx.x == 0) {
    if (cnt[0]) atomicAdd(&counts[it.img].num_edges, cnt[0]);
    if (cnt[1]) atomicAdd(&counts[it.img].h_long, cnt[1]);
    if (cnt[2]) atomicAdd(&counts[it.img].v_long, cnt[2]);
  }
}

__global__ __launch_bounds__(64) void k_quality_score(const QImage* __restrict__ images, const QCount* __restrict__ counts,
                                                      unsigned n, int* __restrict__ scores,
                                                      cbh_quality_detail* __restrict__ detail) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const QImage im = images[i];
  cbh_quality_detail d = {};
  d.score = INT_MIN;
  if (im.qw >= 3 && im.qh >= 3) {
    const QCount c = counts[i];
    d.h_sum = c.h_sum, d.v_sum = c.v_sum;
    d.h_mean = mean_of(c.h_sum, im.qw, im.qh), d.v_mean = mean_of(c.v_sum, im.qw, im.qh);
    d.h_long = (int)c.h_long, d.v_long = (int)c.v_long, d.num_edges = (int)c.num_edges;
    d.qw = im.qw, d.qh = im.qh;
    if (c.num_edges) {
      // :495, :500, :592 -- float, every step rounded (the file is built with -ffp-contract=off)
      const float elr = (float)(d.v_long + d.h_long) / (float)d.num_edges;
      const float er = (float)d.num_edges / (float)((unsigned)(im.qw - 2) * (unsigned)(im.qh - 2));
      const float a = 100.f * er, b = 100.f * elr;
      d.score = (int)(a + b);
    }
  }
  scores[i] = d.score;
  if (detail) detail[i] = d;
}

void quality_dims(int w, int h, int* qw, int* qh, int* hcrop, int* vcrop) {
  const int hc = (int)(w * 0.10), vc = (int)(h * 0.10);  // :333-334
  int a = w - 2 * hc + 1, b = h - 2 * vc + 1;            // crop(hCrop, vCrop, .., w - hCrop, h - vCrop, ..) is inclusive
  if (w < 1 || h < 1 || a < 3 || b < 3) a = b = 0;       // (below 3 x 3 the reference overruns its buffers, :337)
  *qw = a, *qh = b;
  if (hcrop) *hcrop = hc;
  if (vcrop) *vcrop = vc;
}

// images i0 .. i0 + m: one upload of the tables, three launches, one synchronisation (the tables are host memory)
int launch_quality_group(const uint8_t* d_imgs, size_t m, const uint64_t* img_off, const uint32_t* img_w,
                         const uint32_t* img_h, const uint32_t* img_row_stride, int channels, int* d_scores,
                         cbh_quality_detail* d_detail, uint8_t* d_planes, const uint64_t* plane_off, hipStream_t s) {
  std::vector<QImage> images(m);
  std::vector<QItem> items;
  size_t work_bytes = 0;
  for (size_t i = 0; i < m; ++i) {
    QImage& im = images[i];
    im.src_off = img_off[i], im.out_off = plane_off ? plane_off[i] : 0;
    im.w = img_w[i], im.h = img_h[i], im.stride = img_row_stride[i];
    quality_dims((int)im.w, (int)im.h, &im.qw, &im.qh, &im.hcrop, &im.vcrop);
    im.pitch = (im.qw + kChunk - 1) & ~(kChunk - 1);
    im.work_off = work_bytes;
    work_bytes += (size_t)im.pitch * im.qh;
    const int cpr = im.pitch / kChunk;
    for (int cx0 = 0; cx0 < cpr; cx0 += kBlock) {
      const int ncx = std::min(cpr - cx0, kBlock), rows = (kBlock / ncx) * kStripRows;
      for (int y0 = 0; y0 < im.qh; y0 += rows) items.push_back({(unsigned)i, (unsigned)y0, (unsigned)cx0, (unsigned)ncx});
    }
  }
  Scratch scratch(s);
  QImage* d_images = nullptr;
  QItem* d_items = nullptr;
  QCount* d_counts = nullptr;
  unsigned char* d_work = nullptr;
  hipError_t e = scratch.get(&d_images, m * sizeof(QImage));
  if (e == hipSuccess) e = scratch.get(&d_items, std::max<size_t>(items.size(), 1) * sizeof(QItem));
  if (e == hipSuccess) e = scratch.get(&d_counts, m * sizeof(QCount));
  if (e == hipSuccess) e = scratch.get(&d_work, std::max<size_t>(work_bytes, 256));
  if (e == hipSuccess) e = hipMemsetAsync(d_counts, 0, m * sizeof(QCount), s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_images, images.data(), m * sizeof(QImage), hipMemcpyHostToDevice, s);
  if (e == hipSuccess && !items.empty())
    e = hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(QItem), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    const unsigned ni = (unsigned)items.size();
    if (ni) {
      if (channels == 1)
        hipLaunchKernelGGL(k_quality_pack<1>, dim3(ni), dim3(kBlock), 0, s, d_imgs, d_images, d_items, d_work, d_counts);
      else if (channels == 3)
        hipLaunchKernelGGL(k_quality_pack<3>, dim3(ni), dim3(kBlock), 0, s, d_imgs, d_images, d_items, d_work, d_counts);
      else
        hipLaunchKernelGGL(k_quality_pack<4>, dim3(ni), dim3(kBlock), 0, s, d_imgs, d_images, d_items, d_work, d_counts);
      if (d_planes)
        hipLaunchKernelGGL(k_quality_edges<true>, dim3(ni), dim3(kBlock), 0, s, d_images, d_items, d_work, d_counts,
                           d_planes);
      else
        hipLaunchKernelGGL(k_quality_edges<false>, dim3(ni), dim3(kBlock), 0, s, d_images, d_items, d_work, d_counts,
                           d_planes);
    }
    hipLaunchKernelGGL(k_quality_score, dim3(((unsigned)m + 63) / 64), dim3(64), 0, s, d_images, d_counts, (unsigned)m,
                       d_scores, d_detail);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the host tables above must outlive the copies
  return e == hipSuccess ? CBH_OK : fail("quality scores", e);
}

bool quality_shape_ok(uint32_t w, uint32_t h, uint32_t stride, int channels) {
  // (w-1) * (h-1) and the plane offsets stay below 2^31, as the reference's int arithmetic needs
  return w >= 1 && h >= 1 && w <= 65535 && h <= 65535 && (uint64_t)(w + 1) * (h + 1) < (1ull << 31) &&
         stride >= w * (uint32_t)channels;
}

size_t quality_budget() { return (size_t)std::max(g_quality_chunk_mb, 1) << 20; }

}  // namespace

void set_quality_chunk_mb(int v) {
  if (v > 0) g_quality_chunk_mb = v;
}
int get_quality_chunk_mb() { return g_quality_chunk_mb; }
int get_quality_strip_rows() { return kStripRows; }

}  // namespace cbh

extern "C" {

void cbh_quality_dims(int w, int h, int* qw, int* qh) {
  int a = 0, b = 0;
  cbh::quality_dims(w, h, &a, &b, nullptr, nullptr);
  if (qw) *qw = a;
  if (qh) *qh = b;
}

int cbh_quality_scores_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                           const uint32_t* img_h, const uint32_t* img_row_stride, int channels, void* d_scores,
                           void* d_detail, void* d_planes, const uint64_t* plane_off, int device, void* stream) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) return CBH_OK;
  if (!d_imgs || !img_off || !img_w || !img_h || !img_row_stride || !d_scores || (d_planes && !plane_off) ||
      !cbh::channels_ok(channels) || n > (1u << 24))
    return CBH_E_INVAL;
  for (size_t i = 0; i < n; ++i)
    if (!cbh::quality_shape_ok(img_w[i], img_h[i], img_row_stride[i], channels)) return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  // groups whose working planes fit "quality_chunk_mb" of scratch (at least one image each)
  const size_t budget = cbh::quality_budget();
  for (size_t i0 = 0; i0 < n;) {
    size_t m = 0, bytes = 0;
    while (i0 + m < n && m < (1u << 20)) {
      int qw = 0, qh = 0;
      cbh::quality_dims((int)img_w[i0 + m], (int)img_h[i0 + m], &qw, &qh, nullptr, nullptr);
      const size_t b = (size_t)((qw + 15) & ~15) * qh;
      if (m && bytes + b > budget) break;
      bytes += b, ++m;
    }
    const int rc = cbh::launch_quality_group(
        (const uint8_t*)d_imgs, m, img_off + i0, img_w + i0, img_h + i0, img_row_stride + i0, channels, (int*)d_scores + i0,
        d_detail ? (cbh_quality_detail*)d_detail + i0 : nullptr, (uint8_t*)d_planes, d_planes ? plane_off + i0 : nullptr,
        (hipStream_t)stream);
    if (rc != CBH_OK) return rc;
    i0 += m;
  }
  return CBH_OK;
}

int cbh_quality_scores(const uint8_t* imgs, size_t imgs_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                       const uint32_t* img_h, const uint32_t* img_row_stride, int channels, int32_t* scores,
                       cbh_quality_detail* detail, int device) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) return CBH_OK;
  if (!imgs || !scores || !img_off || !img_w || !img_h || !img_row_stride ||
      !cbh::channels_ok(channels))
    return CBH_E_INVAL;
  std::vector<uint64_t> end(n);
  for (size_t i = 0; i < n; ++i) {
    if (!cbh::quality_shape_ok(img_w[i], img_h[i], img_row_stride[i], channels)) return CBH_E_INVAL;
    end[i] = cbh::image_end(img_off[i], img_w[i], img_h[i], img_row_stride[i], channels);
    if (end[i] > imgs_bytes) return CBH_E_INVAL;
  }
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  // uploads of at most "quality_chunk_mb" each: runs of images whose bytes span no more than that (at least one image)
  const std::vector<cbh::Run> runs = cbh::make_runs(n, img_off, end.data(), cbh::quality_budget(), SIZE_MAX);
  size_t span = 0;
  for (const cbh::Run& r : runs) span = std::max<size_t>(span, r.hi - r.lo);
  cbh::Staging st("quality scores");
  uint8_t* d_imgs;
  int32_t* d_scores;
  cbh_quality_detail* d_detail = nullptr;
  st.alloc(&d_imgs, span);
  st.alloc(&d_scores, n * sizeof(int32_t));
  if (detail) st.alloc(&d_detail, n * sizeof(cbh_quality_detail));
  int rc = st.status();
  std::vector<uint64_t> off;
  for (size_t k = 0; k < runs.size() && rc == CBH_OK; ++k) {
    const cbh::Run& r = runs[k];
    cbh::rebase(r, img_off, &off);
    // (the group's kernels have finished: cbh_quality_scores_dev synchronises the stream before it returns)
    st.up(d_imgs, imgs + r.lo, r.hi - r.lo);
    if ((rc = st.status()) == CBH_OK)
      rc = cbh_quality_scores_dev(d_imgs, r.m, off.data(), img_w + r.i0, img_h + r.i0, img_row_stride + r.i0, channels,
                                  d_scores + r.i0, d_detail ? d_detail + r.i0 : nullptr, nullptr, nullptr, device, st.s);
  }
  if (rc != CBH_OK) return rc;
  st.down(scores, d_scores, n * sizeof(int32_t));
  if (detail) st.down(detail, d_detail, n * sizeof(cbh_quality_detail));
  st.sync();
  return st.status();
}

}  // extern "C"
