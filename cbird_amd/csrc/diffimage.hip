// diffimage.hip -- brightnessAndContrastAuto (src/cvutil.cpp:578-665: grayLevel, stretchContrast) for a ragged batch of
// images, and differenceImage (src/gui/mediagrouplistwidget.cpp:98-208) for one left image against n right images: the
// false-colour picture of where two matched images differ, and a record per pair to rank a group by.
//
// A pass walks a grid of pixels four at a time (a "quad": x0 = 4k .. 4k + 3 of one row); a workgroup takes kBlockPixels
// consecutive pixels of one grid, kSteps quads per thread.  How a grid pixel finds its source pixel is the view's mode:
// itself, the nearest pixel of a source of another size (the size rule, :153-161), or the source pixel under the pair's
// transform (:113-121).  Nothing between the sources and the output exists in memory: neither the RGB32 views nor the
// warped canvas nor the stretched images.
//   k_diff_hist     the grey view's 256 bins per view, one LDS copy per wave, one global atomic per bin and workgroup
//   k_diff_tables   one workgroup per view: gray_cuts (thread 0), then the 256 bytes of the stretch, one per thread
//   k_diff_stretch  stage A's output: every byte of every image through its table, 16 bytes per thread and step
//   k_diff_detail   one lane per pair: the record's sizes and cuts, its sums zeroed
//   k_diff_color    both fetches, both tables, the squared distance, the colour, one 16-byte store per quad, and the
//                   record's sums: reduced per wave, one atomic per field and wave
// Everything is integer arithmetic but the cut rule's float32 running sum and the table's multiply-add (the file is built
// with -ffp-contract=off), and the f64 sample coordinates of a warped pair.
// Bound by HBM: the sources are read twice (histograms, then the colour pass), the output is written once.
#include <cmath>
#include <cstdint>

#include <algorithm>
#include <vector>

#include "cbh_index.h"
#include "cbh_runs.h"
#include "cbh_staging.h"
#include "gray_px.h"
#include "stretch_px.h"

namespace cbh {
namespace {

constexpr int kBlock = 256;
constexpr int kSteps = 4;                         // quads (chunks) per thread
constexpr int kBlockPixels = kBlock * kSteps * 4; // pixels of one grid a workgroup takes ("diff_block_pixels")
constexpr unsigned kMaxSide = 32767;
constexpr size_t kMaxBatch = (size_t)1 << 20;

enum : unsigned { kDirect = 0, kScale = 1, kWarp = 2 };

// One side of a pass: a source image and the w x h grid it is walked on
struct DView {
  unsigned long long off;   // first source byte
  unsigned sw, sh, stride;  // the source
  unsigned w, h;            // the grid
  unsigned mode;            // kDirect: grid = source; kScale: the nearest source pixel; kWarp: through m, 0 outside
  double m[6];              // grid -> source
};
struct DItem {
  unsigned view, first;  // quads (k_diff_stretch: 16-byte chunks) first .. first + kBlock * kSteps of the view's grid
};
struct DPair {
  DView l, r;  // both on the output's grid
  unsigned long long out_off;
};

// ---- the cut rule of grayLevel (:578-626), the same function on both sides -------------------------------------------
// count[j] = pixels of grey value j.  clip_pct == 0: the lowest and the highest value present (256 / -1 without a pixel).
// Otherwise the reference's float32 running sum acc[i], its total, clip = (clip_pct * (total / 100)) / 2, min_gray =
// the first i with !(acc[i] < clip) (256: none), max_gray = the last i with !(acc[i] >= total - clip) (-1: none).  The
// sum is run twice instead of kept: the total first, then the two cuts.
__host__ __device__ inline void gray_cuts(const uint32_t* count, float clip_pct, int* min_gray, int* max_gray) {
  int lo = 256, hi = -1;
  if (clip_pct == 0.0f) {
    for (int i = 0; i < 256; ++i)
      if (count[i]) {
        if (lo == 256) lo = i;
        hi = i;
      }
  } else {
    float total = (float)count[0];
    for (int i = 1; i < 256; ++i) total = total + (float)count[i];
    float clip = clip_pct * (total / 100.0f);
    clip = clip / 2.0f;
    const float upper = total - clip;
    float acc = 0.0f;
    for (int i = 0; i < 256; ++i) {
      acc = i ? acc + (float)count[i] : (float)count[0];
      if (lo == 256 && !(acc < clip)) lo = i;
      if (!(acc >= upper)) hi = i;
    }
  }
  *min_gray = lo, *max_gray = hi;
}

// ---- fetching ---------------------------------------------------------------------------------------------------------
// a pixel as b | g << 8 | r << 16 (the RGB32 view: grey replicated, alpha dropped)
template <int CH>
__device__ __forceinline__ unsigned px_at(const unsigned char* __restrict__ p) {
  if (CH == 1) return (unsigned)p[0] * 0x010101u;
  return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
}
template <int CH>
__device__ __forceinline__ unsigned gray_of(unsigned px) {
  if (CH == 1) return px & 0xffu;
  return cbh_gray_px((int)(px & 0xffu), (int)((px >> 8) & 0xffu), (int)(px >> 16));
}

// grid pixels x0 .. x0 + np - 1 (np <= 4) of grid row y; the others stay 0
template <int CH>
__device__ __forceinline__ void fetch4(const unsigned char* __restrict__ s, const DView& v, unsigned x0, unsigned y, int np,
                                       unsigned (&px)[4]) {
  px[0] = px[1] = px[2] = px[3] = 0;
  if (v.mode == kDirect) {
    const unsigned char* p = s + (size_t)y * v.stride + (size_t)x0 * CH;
    if (np == 4 && ((uintptr_t)p & (CH == 4 ? 15 : 3)) == 0) {
      if (CH == 1) {
        const unsigned d = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) px[j] = ((d >> (8 * j)) & 0xffu) * 0x010101u;
      } else if (CH == 3) {
        const unsigned d0 = reinterpret_cast<const unsigned*>(p)[0], d1 = reinterpret_cast<const unsigned*>(p)[1],
                       d2 = reinterpret_cast<const unsigned*>(p)[2];
        px[0] = d0 & 0xffffffu;
        px[1] = (d0 >> 24) | (d1 & 0xffffu) << 8;
        px[2] = (d1 >> 16) | (d2 & 0xffu) << 16;
        px[3] = d2 >> 8;
      } else {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        px[0] = q.x & 0xffffffu, px[1] = q.y & 0xffffffu, px[2] = q.z & 0xffffffu, px[3] = q.w & 0xffffffu;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < np) px[j] = px_at<CH>(p + j * CH);
    }
  } else if (v.mode == kScale) {
    // src = ((2 * dst + 1) * ssize) / (2 * dsize): the source pixel under the centre of the destination pixel
    const unsigned sy = ((2u * y + 1u) * v.sh) / (2u * v.h);
    const unsigned char* row = s + (size_t)sy * v.stride;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < np) px[j] = px_at<CH>(row + (size_t)(((2u * (x0 + j) + 1u) * v.sw) / (2u * v.w)) * CH);
  } else {
    // per pixel, in f64, left to right, nothing fused and nothing stepped: the numpy model does the same operations
    const double fy = (double)y + 0.5;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < np) {
        const double fx = (double)(x0 + j) + 0.5;
        const double sx = floor((v.m[0] * fx + v.m[1] * fy) + v.m[2]);
        const double sy = floor((v.m[3] * fx + v.m[4] * fy) + v.m[5]);
        if (sx >= 0.0 && sx < (double)v.sw && sy >= 0.0 && sy < (double)v.sh)  // (a NaN is outside)
          px[j] = px_at<CH>(s + (size_t)(unsigned)sy * v.stride + (size_t)(unsigned)sx * CH);
      }
  }
}

// quad q of a w-wide grid
__device__ __forceinline__ void quad_at(unsigned q, unsigned w, unsigned* x0, unsigned* y, int* np) {
  const unsigned qpr = (w + 3u) >> 2;
  *y = q / qpr;
  *x0 = (q - *y * qpr) << 2;
  *np = (int)min(4u, w - *x0);
}

template <int CH>
__global__ __launch_bounds__(kBlock) void k_diff_hist(const unsigned char* __restrict__ src,
                                                      const DView* __restrict__ views, const DItem* __restrict__ items,
                                                      unsigned* __restrict__ hist) {
  __shared__ unsigned sh[kBlock / 64][256];
  const unsigned tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < kBlock / 64; ++k) sh[k][tid] = 0;
  __syncthreads();
  const DItem it = items[blockIdx.x];
  const DView v = views[it.view];
  const unsigned total = ((v.w + 3u) >> 2) * v.h;
  unsigned* mine = sh[tid >> 6];
  for (int step = 0; step < kSteps; ++step) {
    const unsigned q = it.first + step * kBlock + tid;
    if (q >= total) break;
    unsigned x0, y, px[4];
    int np;
    quad_at(q, v.w, &x0, &y, &np);
    fetch4<CH>(src + v.off, v, x0, y, np, px);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < np) atomicAdd(&mine[gray_of<CH>(px[j])], 1u);
  }
  __syncthreads();
  unsigned c = 0;
#pragma unroll
  for (int k = 0; k < kBlock / 64; ++k) c += sh[k][tid];
  if (c) atomicAdd(&hist[(size_t)it.view * 256 + tid], c);
}

// stretchContrast (:628-655): min >= max copies; else alpha = 255 / float(max - min), beta = -min * alpha and
// convertTo's saturate_cast<uchar>(cvRound(s * alpha + beta)) -- a float multiply, a float add, round half to even
__global__ __launch_bounds__(256) void k_diff_tables(const unsigned* __restrict__ hist, float clip_pct,
                                                     int* __restrict__ cuts, unsigned char* __restrict__ tables) {
  __shared__ int sh[2];
  const unsigned v = blockIdx.x, s = threadIdx.x;
  if (s == 0) {
    int lo, hi;
    gray_cuts(hist + (size_t)v * 256, clip_pct, &lo, &hi);
    sh[0] = lo, sh[1] = hi;
    cuts[2 * v] = lo, cuts[2 * v + 1] = hi;
  }
  __syncthreads();
  const int lo = sh[0], hi = sh[1];
  tables[(size_t)v * 256 + s] = (unsigned char)cbh_stretch_px(lo, hi, s);
}

// every byte of the images' rows through the view's table (alpha included: the reference's restore is commented out);
// dst has the layout of src and may be src
__global__ __launch_bounds__(kBlock) void k_diff_stretch(const unsigned char* src, unsigned char* dst,
                                                         const DView* __restrict__ views, const DItem* __restrict__ items,
                                                         const unsigned char* __restrict__ tables, int channels) {
  __shared__ unsigned char tab[256];
  const DItem it = items[blockIdx.x];
  const DView v = views[it.view];
  tab[threadIdx.x] = tables[(size_t)it.view * 256 + threadIdx.x];
  __syncthreads();
  const unsigned rb = v.w * (unsigned)channels, cpr = (rb + 15u) >> 4, total = cpr * v.h;
  for (int step = 0; step < kSteps; ++step) {
    const unsigned c = it.first + step * kBlock + threadIdx.x;
    if (c >= total) break;
    const unsigned y = c / cpr, b0 = (c - y * cpr) << 4, nb = min(16u, rb - b0);
    const size_t at = v.off + (size_t)y * v.stride + b0;
    const unsigned char* p = src + at;
    unsigned char* d = dst + at;
    if (nb == 16 && (((uintptr_t)p | (uintptr_t)d) & 15) == 0) {
      const uint4 q = *reinterpret_cast<const uint4*>(p);
      const unsigned in[4] = {q.x, q.y, q.z, q.w};
      unsigned out[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        out[k] = (unsigned)tab[in[k] & 0xffu] | (unsigned)tab[(in[k] >> 8) & 0xffu] << 8 |
                 (unsigned)tab[(in[k] >> 16) & 0xffu] << 16 | (unsigned)tab[in[k] >> 24] << 24;
      *reinterpret_cast<uint4*>(d) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
      for (unsigned k = 0; k < nb; ++k) d[k] = tab[p[k]];
    }
  }
}

__global__ __launch_bounds__(64) void k_diff_detail(const DPair* __restrict__ pairs, const int* __restrict__ cuts, unsigned n,
                                                    cbh_diff_detail* __restrict__ detail) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cbh_diff_detail d = {};
  d.w = (int)pairs[i].r.w, d.h = (int)pairs[i].r.h, d.warped = pairs[i].r.mode == kWarp;
  d.left_min = cuts[0], d.left_max = cuts[1], d.right_min = cuts[2 * (i + 1)], d.right_max = cuts[2 * (i + 1) + 1];
  detail[i] = d;
}

// the colour of :173-206 as BGRA; qRgb masks r, so it wraps above 131071
__device__ __forceinline__ unsigned diff_colour(unsigned sum) {
  const unsigned r = ((sum >> 10) << 1) & 255u, g = ((sum >> 5) & 31u) << 3, b = (sum & 31u) << 3;
  return b | g << 8 | r << 16 | 0xff000000u;
}

template <int CHL, int CHR>
__global__ __launch_bounds__(kBlock) void k_diff_color(const unsigned char* __restrict__ left,
                                                       const unsigned char* __restrict__ rights,
                                                       const DPair* __restrict__ pairs, const DItem* __restrict__ items,
                                                       const unsigned char* __restrict__ tables,
                                                       unsigned char* __restrict__ images,
                                                       cbh_diff_detail* __restrict__ detail) {
  __shared__ unsigned char tl[256], tr[256];
  const unsigned tid = threadIdx.x;
  const DItem it = items[blockIdx.x];
  tl[tid] = tables[tid];  // view 0 is the left image, view 1 + i the aligned right image of pair i
  tr[tid] = tables[(size_t)(it.view + 1) * 256 + tid];
  __syncthreads();
  const DPair& p = pairs[it.view];
  const DView vl = p.l, vr = p.r;
  const unsigned ow = vr.w, total = ((ow + 3u) >> 2) * vr.h;
  unsigned char* out = images ? images + p.out_off : nullptr;
  unsigned tot = 0, top = 0, n32 = 0, n1024 = 0;
  for (int step = 0; step < kSteps; ++step) {
    const unsigned q = it.first + step * kBlock + tid;
    if (q >= total) break;
    unsigned x0, y, a[4], b[4], c[4];
    int np;
    quad_at(q, ow, &x0, &y, &np);
    fetch4<CHL>(left + vl.off, vl, x0, y, np, a);
    fetch4<CHR>(rights + vr.off, vr, x0, y, np, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int db = (int)tl[a[j] & 0xffu] - (int)tr[b[j] & 0xffu];
      const int dg = (int)tl[(a[j] >> 8) & 0xffu] - (int)tr[(b[j] >> 8) & 0xffu];
      const int dr = (int)tl[a[j] >> 16] - (int)tr[b[j] >> 16];
      const unsigned sum = j < np ? (unsigned)(dr * dr + dg * dg + db * db) : 0u;
      c[j] = diff_colour(sum);
      tot += sum, top = max(top, sum), n32 += sum >= 32u, n1024 += sum >= 1024u;
    }
    if (out) {
      unsigned* d = reinterpret_cast<unsigned*>(out + ((size_t)y * ow + x0) * 4);  // (out_off is a multiple of 16)
      if (np == 4 && ((uintptr_t)d & 15) == 0) {
        *reinterpret_cast<uint4*>(d) = make_uint4(c[0], c[1], c[2], c[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < np) d[j] = c[j];
      }
    }
  }
  // a thread holds at most 16 sums of at most 195075, a wave 64 times that: 32 bits
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    tot += __shfl_down(tot, d, 64);
    top = max(top, __shfl_down(top, d, 64));
    n32 += __shfl_down(n32, d, 64);
    n1024 += __shfl_down(n1024, d, 64);
  }
  if ((tid & 63) == 0 && tot) {
    cbh_diff_detail* r = detail + it.view;
    atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_total), (unsigned long long)tot);
    atomicMax(&r->sum_max, top);
    if (n32) atomicAdd(&r->n_ge32, n32);
    if (n1024) atomicAdd(&r->n_ge1024, n1024);
  }
}

// ---- the host side ------------------------------------------------------------------------------------------------------
bool side_ok(uint32_t w, uint32_t h, uint32_t stride, int channels) {
  return w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide && stride >= w * (uint32_t)channels;
}
bool clip_ok(float c) { return c >= 0.0f && std::isfinite(c); }

DView direct_view(uint64_t off, uint32_t w, uint32_t h, uint32_t stride) {
  DView v = {};
  v.off = off, v.sw = v.w = w, v.sh = v.h = h, v.stride = stride, v.mode = kDirect;
  return v;
}
// `units` quads or chunks of view `view` in workgroup portions
void add_items(std::vector<DItem>* items, unsigned view, uint64_t units) {
  for (uint64_t f = 0; f < units; f += kBlock * kSteps) items->push_back({view, (unsigned)f});
}
uint64_t quads_of(const DView& v) { return (uint64_t)((v.w + 3) / 4) * v.h; }

// does pair i redraw its right image (:114), and through which matrix: tx itself maps the canvas to the right image;
// a singular one counts as the identity, as QTransform::inverted returns it
bool pair_warps(const double* tx, const uint8_t* has_tx, size_t i, double (&m)[6]) {
  static const double ident[6] = {1, 0, 0, 0, 1, 0};
  if (!tx || (has_tx && !has_tx[i])) return false;
  const double* t = tx + 6 * i;
  if (std::equal(t, t + 6, ident)) return false;  // (compared as numbers: -0.0 is 0)
  const double det = t[0] * t[4] - t[1] * t[3];
  for (int k = 0; k < 6; ++k) m[k] = det == 0.0 ? ident[k] : t[k];
  return true;
}
// the size rule (:153-161) on the left image and the aligned right image
void out_dims(uint32_t lw, uint32_t lh, uint32_t aw, uint32_t ah, uint32_t* ow, uint32_t* oh) {
  const int right_area = (int)aw * (int)ah, left_area = (int)lw * (int)lh;
  if (right_area < left_area) *ow = lw, *oh = lh;
  else *ow = aw, *oh = ah;
}
DView on_grid(DView v, uint32_t ow, uint32_t oh) {
  if (v.mode == kWarp) return v;  // (the canvas has the left image's size, which then is the output's)
  v.w = ow, v.h = oh, v.mode = (ow == v.sw && oh == v.sh) ? kDirect : kScale;
  return v;
}

template <int CH>
void launch_hist(const uint8_t* src, const DView* views, const DItem* items, size_t n_items, unsigned* hist, hipStream_t s) {
  if (n_items) hipLaunchKernelGGL(k_diff_hist<CH>, dim3((unsigned)n_items), dim3(kBlock), 0, s, src, views, items, hist);
}
void launch_hist(int ch, const uint8_t* src, const DView* views, const DItem* items, size_t n_items, unsigned* hist,
                 hipStream_t s) {
  if (ch == 1) launch_hist<1>(src, views, items, n_items, hist, s);
  else if (ch == 3) launch_hist<3>(src, views, items, n_items, hist, s);
  else launch_hist<4>(src, views, items, n_items, hist, s);
}
template <int CHL>
void launch_color(int chr, unsigned ni, hipStream_t s, const uint8_t* l, const uint8_t* r, const DPair* pairs,
                  const DItem* items, const uint8_t* tables, uint8_t* images, cbh_diff_detail* detail) {
  if (chr == 1) hipLaunchKernelGGL((k_diff_color<CHL, 1>), dim3(ni), dim3(kBlock), 0, s, l, r, pairs, items, tables, images, detail);
  else if (chr == 3) hipLaunchKernelGGL((k_diff_color<CHL, 3>), dim3(ni), dim3(kBlock), 0, s, l, r, pairs, items, tables, images, detail);
  else hipLaunchKernelGGL((k_diff_color<CHL, 4>), dim3(ni), dim3(kBlock), 0, s, l, r, pairs, items, tables, images, detail);
}

}  // namespace

int get_diff_block_pixels() { return kBlockPixels; }

}  // namespace cbh

extern "C" {

int cbh_gray_cuts(const uint32_t* hist, size_t n, float clip_pct, int32_t* min_gray, int32_t* max_gray) {
  if ((n && (!hist || !min_gray || !max_gray)) || !cbh::clip_ok(clip_pct)) return CBH_E_INVAL;
  for (size_t i = 0; i < n; ++i) {
    int lo, hi;
    cbh::gray_cuts(hist + 256 * i, clip_pct, &lo, &hi);
    min_gray[i] = lo, max_gray[i] = hi;
  }
  return CBH_OK;
}

int cbh_auto_contrast_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                          const uint32_t* img_h, const uint32_t* img_row_stride, int channels, float clip_pct, void* d_out,
                          void* d_cuts, void* d_hist, int device, void* stream) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  if (!channels_ok(channels) || !clip_ok(clip_pct) || n > kMaxBatch) return CBH_E_INVAL;
  if (n == 0) return CBH_OK;
  if (!d_imgs || !img_off || !img_w || !img_h || !img_row_stride || !d_cuts) return CBH_E_INVAL;
  std::vector<DView> views(n);
  std::vector<DItem> items;
  for (size_t i = 0; i < n; ++i) {
    if (!side_ok(img_w[i], img_h[i], img_row_stride[i], channels)) return CBH_E_INVAL;
    views[i] = direct_view(img_off[i], img_w[i], img_h[i], img_row_stride[i]);
    add_items(&items, (unsigned)i, quads_of(views[i]));
  }
  const size_t n_hist = items.size();
  if (d_out)
    for (size_t i = 0; i < n; ++i) add_items(&items, (unsigned)i, (uint64_t)((img_w[i] * channels + 15) / 16) * img_h[i]);
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  Scratch scratch(s);
  DView* dv = nullptr;
  DItem* di = nullptr;
  unsigned* hist = (unsigned*)d_hist;
  unsigned char* tables = nullptr;
  hipError_t e = upload(scratch, &dv, views, s);
  if (e == hipSuccess) e = upload(scratch, &di, items, s);
  if (e == hipSuccess && !hist) e = scratch.get(&hist, n * 256 * sizeof(unsigned));
  if (e == hipSuccess) e = scratch.get(&tables, n * 256);
  if (e == hipSuccess) e = hipMemsetAsync(hist, 0, n * 256 * sizeof(unsigned), s);
  if (e == hipSuccess) {
    launch_hist(channels, (const uint8_t*)d_imgs, dv, di, n_hist, hist, s);
    hipLaunchKernelGGL(k_diff_tables, dim3((unsigned)n), dim3(256), 0, s, hist, clip_pct, (int*)d_cuts, tables);
    if (d_out && items.size() > n_hist)
      hipLaunchKernelGGL(k_diff_stretch, dim3((unsigned)(items.size() - n_hist)), dim3(kBlock), 0, s,
                         (const unsigned char*)d_imgs, (unsigned char*)d_out, dv, di + n_hist, tables, channels);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the host tables above must outlive the copies
  return e == hipSuccess ? CBH_OK : fail("auto contrast", e);
}

int cbh_auto_contrast(const uint8_t* imgs, size_t imgs_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                      const uint32_t* img_h, const uint32_t* img_row_stride, int channels, float clip_pct, uint8_t* out,
                      int32_t* cuts, uint32_t* hist, int device) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  if (!channels_ok(channels) || !clip_ok(clip_pct) || n > kMaxBatch) return CBH_E_INVAL;
  if (n == 0) return CBH_OK;
  if (!imgs || !img_off || !img_w || !img_h || !img_row_stride || !cuts) return CBH_E_INVAL;
  for (size_t i = 0; i < n; ++i)
    if (!side_ok(img_w[i], img_h[i], img_row_stride[i], channels) ||
        image_end(img_off[i], img_w[i], img_h[i], img_row_stride[i], channels) > imgs_bytes)
      return CBH_E_INVAL;
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  Staging st("auto contrast");
  uint8_t* d_imgs;
  int32_t* d_cuts;
  uint32_t* d_hist = nullptr;
  st.alloc(&d_imgs, imgs_bytes);
  st.alloc(&d_cuts, n * 2 * sizeof(int32_t));
  if (hist) st.alloc(&d_hist, n * 256 * sizeof(uint32_t));
  st.up(d_imgs, imgs, imgs_bytes);
  int rc = st.status();
  // (in place on the device copy: the bytes between the images come back as they went up)
  if (rc == CBH_OK)
    rc = cbh_auto_contrast_dev(d_imgs, n, img_off, img_w, img_h, img_row_stride, channels, clip_pct, out ? d_imgs : nullptr,
                               d_cuts, d_hist, device, st.s);
  if (rc != CBH_OK) return rc;
  if (out) st.down(out, d_imgs, imgs_bytes);
  st.down(cuts, d_cuts, n * 2 * sizeof(int32_t));
  if (hist) st.down(hist, d_hist, n * 256 * sizeof(uint32_t));
  st.sync();
  return st.status();
}

int cbh_difference_dims(int left_w, int left_h, size_t n, const uint32_t* img_w, const uint32_t* img_h, const double* tx,
                        const uint8_t* has_tx, uint32_t* out_w, uint32_t* out_h, uint8_t* warped) {
  using namespace cbh;
  if (left_w < 1 || left_h < 1 || left_w > (int)kMaxSide || left_h > (int)kMaxSide) return CBH_E_INVAL;
  if (n && (!img_w || !img_h || !out_w || !out_h)) return CBH_E_INVAL;
  for (size_t i = 0; i < n; ++i) {
    if (img_w[i] < 1 || img_h[i] < 1 || img_w[i] > kMaxSide || img_h[i] > kMaxSide) return CBH_E_INVAL;
    double m[6];
    const bool warps = pair_warps(tx, has_tx, i, m);
    out_dims((uint32_t)left_w, (uint32_t)left_h, warps ? (uint32_t)left_w : img_w[i], warps ? (uint32_t)left_h : img_h[i],
             &out_w[i], &out_h[i]);
    if (warped) warped[i] = warps;
  }
  return CBH_OK;
}

int cbh_difference_images_dev(const void* d_left, int left_w, int left_h, size_t left_row_stride, int left_channels,
                              const void* d_rights, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                              const uint32_t* img_h, const uint32_t* img_row_stride, int channels, const double* tx,
                              const uint8_t* has_tx, float clip_pct, void* d_images, const uint64_t* out_off,
                              void* d_detail, int device, void* stream) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  if (!channels_ok(channels) || !channels_ok(left_channels) || !clip_ok(clip_pct) || n > kMaxBatch || left_w < 1 ||
      left_h < 1 || left_row_stride > 0xffffffffu ||
      !side_ok((uint32_t)left_w, (uint32_t)left_h, (uint32_t)left_row_stride, left_channels))
    return CBH_E_INVAL;
  if (n == 0) return CBH_OK;
  if (!d_left || !d_rights || !img_off || !img_w || !img_h || !img_row_stride || (d_images && !out_off) ||
      ((uintptr_t)d_images & 15))
    return CBH_E_INVAL;
  const uint32_t lw = (uint32_t)left_w, lh = (uint32_t)left_h;
  std::vector<DView> views(n + 1);
  std::vector<DPair> pairs(n);
  std::vector<DItem> items;
  views[0] = direct_view(0, lw, lh, (uint32_t)left_row_stride);
  add_items(&items, 0, quads_of(views[0]));
  const size_t n_left = items.size();
  for (size_t i = 0; i < n; ++i) {
    if (!side_ok(img_w[i], img_h[i], img_row_stride[i], channels) || (d_images && (out_off[i] & 15))) return CBH_E_INVAL;
    DView& v = views[i + 1];
    v = direct_view(img_off[i], img_w[i], img_h[i], img_row_stride[i]);
    if (pair_warps(tx, has_tx, i, v.m)) v.w = lw, v.h = lh, v.mode = kWarp;
    add_items(&items, (unsigned)(i + 1), quads_of(v));
  }
  const size_t n_hist = items.size();
  for (size_t i = 0; i < n; ++i) {
    uint32_t ow, oh;
    out_dims(lw, lh, views[i + 1].w, views[i + 1].h, &ow, &oh);
    pairs[i].l = on_grid(views[0], ow, oh), pairs[i].r = on_grid(views[i + 1], ow, oh);
    pairs[i].out_off = d_images ? out_off[i] : 0;
    add_items(&items, (unsigned)i, quads_of(pairs[i].r));
  }
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  Scratch scratch(s);
  DView* dv = nullptr;
  DPair* dp = nullptr;
  DItem* di = nullptr;
  unsigned* hist = nullptr;
  int* cuts = nullptr;
  unsigned char* tables = nullptr;
  cbh_diff_detail* detail = (cbh_diff_detail*)d_detail;
  hipError_t e = upload(scratch, &dv, views, s);
  if (e == hipSuccess) e = upload(scratch, &dp, pairs, s);
  if (e == hipSuccess) e = upload(scratch, &di, items, s);
  if (e == hipSuccess) e = scratch.get(&hist, (n + 1) * 256 * sizeof(unsigned));
  if (e == hipSuccess) e = scratch.get(&cuts, (n + 1) * 2 * sizeof(int));
  if (e == hipSuccess) e = scratch.get(&tables, (n + 1) * 256);
  if (e == hipSuccess && !detail) e = scratch.get(&detail, n * sizeof(cbh_diff_detail));
  if (e == hipSuccess) e = hipMemsetAsync(hist, 0, (n + 1) * 256 * sizeof(unsigned), s);
  if (e == hipSuccess) {
    const uint8_t *l = (const uint8_t*)d_left, *r = (const uint8_t*)d_rights;
    launch_hist(left_channels, l, dv, di, n_left, hist, s);
    launch_hist(channels, r, dv, di + n_left, n_hist - n_left, hist, s);
    hipLaunchKernelGGL(k_diff_tables, dim3((unsigned)n + 1), dim3(256), 0, s, hist, clip_pct, cuts, tables);
    hipLaunchKernelGGL(k_diff_detail, dim3(((unsigned)n + 63) / 64), dim3(64), 0, s, dp, cuts, (unsigned)n, detail);
    const unsigned ni = (unsigned)(items.size() - n_hist);
    if (left_channels == 1) launch_color<1>(channels, ni, s, l, r, dp, di + n_hist, tables, (uint8_t*)d_images, detail);
    else if (left_channels == 3) launch_color<3>(channels, ni, s, l, r, dp, di + n_hist, tables, (uint8_t*)d_images, detail);
    else launch_color<4>(channels, ni, s, l, r, dp, di + n_hist, tables, (uint8_t*)d_images, detail);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the host tables above must outlive the copies
  return e == hipSuccess ? CBH_OK : fail("difference images", e);
}

int cbh_difference_images(const uint8_t* left, int left_w, int left_h, size_t left_row_stride, int left_channels,
                          const uint8_t* rights, size_t rights_bytes, size_t n, const uint64_t* img_off,
                          const uint32_t* img_w, const uint32_t* img_h, const uint32_t* img_row_stride, int channels,
                          const double* tx, const uint8_t* has_tx, float clip_pct, uint8_t* images, size_t images_bytes,
                          const uint64_t* out_off, cbh_diff_detail* detail, int device) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  if (!channels_ok(channels) || !channels_ok(left_channels) || !clip_ok(clip_pct) || n > kMaxBatch || left_w < 1 ||
      left_h < 1 || left_row_stride > 0xffffffffu ||
      !side_ok((uint32_t)left_w, (uint32_t)left_h, (uint32_t)left_row_stride, left_channels))
    return CBH_E_INVAL;
  if (n == 0) return CBH_OK;
  if (!left || !rights || !img_off || !img_w || !img_h || !img_row_stride || (images && !out_off)) return CBH_E_INVAL;
  std::vector<uint32_t> ow(n), oh(n);
  for (size_t i = 0; i < n; ++i)
    if (!side_ok(img_w[i], img_h[i], img_row_stride[i], channels) ||
        image_end(img_off[i], img_w[i], img_h[i], img_row_stride[i], channels) > rights_bytes)
      return CBH_E_INVAL;
  if (cbh_difference_dims(left_w, left_h, n, img_w, img_h, tx, has_tx, ow.data(), oh.data(), nullptr) != CBH_OK)
    return CBH_E_INVAL;
  if (images)
    for (size_t i = 0; i < n; ++i)
      if ((out_off[i] & 15) || out_off[i] + (uint64_t)ow[i] * oh[i] * 4 > images_bytes) return CBH_E_INVAL;
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  const size_t left_bytes = (size_t)(left_h - 1) * left_row_stride + (size_t)left_w * left_channels;
  Staging st("difference images");
  uint8_t *d_left, *d_rights, *d_images = nullptr;
  cbh_diff_detail* d_detail = nullptr;
  st.alloc(&d_left, left_bytes);
  st.alloc(&d_rights, rights_bytes);
  if (images) st.alloc(&d_images, std::max<size_t>(images_bytes, 16));
  if (detail) st.alloc(&d_detail, n * sizeof(cbh_diff_detail));
  st.up(d_left, left, left_bytes);
  st.up(d_rights, rights, rights_bytes);
  int rc = st.status();
  if (rc == CBH_OK)
    rc = cbh_difference_images_dev(d_left, left_w, left_h, left_row_stride, left_channels, d_rights, n, img_off, img_w,
                                   img_h, img_row_stride, channels, tx, has_tx, clip_pct, d_images, out_off, d_detail,
                                   device, st.s);
  if (rc != CBH_OK) return rc;
  // each picture where the caller laid it out: the bytes between them are the caller's
  for (size_t i = 0; i < n && images; ++i) st.down(images + out_off[i], d_images + out_off[i], (size_t)ow[i] * oh[i] * 4);
  if (detail) st.down(detail, d_detail, n * sizeof(cbh_diff_detail));
  st.sync();
  return st.status();
}

}  // extern "C"
