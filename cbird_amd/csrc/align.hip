// align.hip -- the alignment VideoCompareWidget runs before two matched frames or clips can be compared
// (src/gui/videocomparewidget.cpp): alignSpatially (:590-627), one left image against n right images, and
// alignTemporally with sad128 (:629-680), a window of right frames slid over a left clip.  Both are sums of absolute byte
// differences (SAD) of images brought to a fixed square size; everything is integer arithmetic, so any order of the
// partial sums gives the same tables.  include/cbird_hip.h states the rules, tests/alignment_rules.py is the numpy model.
//   k_align_scale   every image into a packed S x S x 3 plane (S = 256 spatial, 128 temporal): QImage::scaled's nearest
//                   neighbour, grey replicated, alpha dropped; rows of 768 / 384 bytes, so every row starts on a dword
//   k_align_sad     a workgroup takes kBand rows of one right plane and stages the kBand + 16 rows of the left plane they
//                   meet in LDS.  Per vertical shift a lane takes four consecutive dwords of a right row (one 16-byte load
//                   for 17 shifts; 17 loads of a dword for its 289 uses, from L2) and the 16 left dwords that cover all
//                   17 horizontal shifts of them (four ds_read_b128): the left operand
//                   of shift xo starts at byte 24 + 3 xo of the row, so its dwords are v_alignbyte_b32 of two neighbours,
//                   and v_sad_u8 adds four byte differences to the shift's accumulator.  17 accumulators per lane, reduced
//                   over the wave when the wave's vertical shift changes, one atomicAdd per shift and wave
//   k_align_pick    one wave per pair: the minimum of sad << 9 | scan index, which is the reference's tie rule
//   k_align_cell    one workgroup per (placement, window frame): the SAD of two 128 x 128 x 3 planes
//   k_align_means   one thread per placement: the integer mean of its cells
//   k_align_tpick   one workgroup: the start rule
// Bound by the vector ALU: 289 x 43 200 v_sad_u8 per pair, 12 of every 17 behind a v_alignbyte_b32; LDS serves four
// 16-byte reads per 116 of those operations.
#include <cstdint>

#include <algorithm>
#include <vector>

#include "cbh_index.h"
#include "cbh_runs.h"
#include "cbh_staging.h"

namespace cbh {
namespace {

constexpr int kBlock = 256;
constexpr unsigned kMaxSide = 32767;
constexpr size_t kMaxBatch = (size_t)1 << 20;
constexpr int kSpatial = 256, kTemporal = 128;        // the sides both searches scale to
constexpr int kRow = kSpatial * 3;                    // bytes of a spatial plane's row
constexpr size_t kPlaneS = (size_t)kSpatial * kRow;   // 196 608
constexpr size_t kPlaneT = (size_t)kTemporal * kTemporal * 3;  // 49 152
constexpr int kShifts = 17, kTable = kShifts * kShifts;
constexpr int kInterior = kSpatial - 2 * 8;           // 240 rows and columns take part
constexpr int kBand = 24;                             // right rows of one workgroup
constexpr int kBands = kInterior / kBand;
constexpr int kLdsRows = kBand + 2 * 8;               // left rows a band meets
constexpr int kQuads = kInterior * 3 / 16;            // 45 groups of four dwords in a row's window
constexpr int kItems = kBand * kQuads;                // lane items of a band: 1080, 16.9 rounds of a wave
constexpr int kRounds = (kItems + 63) / 64;
constexpr int kUnits = kShifts * kRounds;             // (vertical shift, round) in that order, dealt to the waves in runs
constexpr int kUnitsPerWave = (kUnits + kBlock / 64 - 1) / (kBlock / 64);
static_assert(kBands * kBand == kInterior && kQuads * 16 == kInterior * 3, "the window is whole bands and whole quads");

struct AImg {
  unsigned long long off;  // first source byte
  unsigned w, h, stride;
};

// ---- scaling ------------------------------------------------------------------------------------------------------------
// plane first + i = image i at S x S: src = ((2 * dst + 1) * ssize) / (2 * dsize), four pixels = three dwords per thread
template <int CH, int S>
__global__ __launch_bounds__(kBlock) void k_align_scale(const unsigned char* __restrict__ src, const AImg* __restrict__ imgs,
                                                        unsigned first, unsigned char* __restrict__ planes) {
  constexpr unsigned kWgs = S * S / 4 / kBlock;  // workgroups of one image
  const unsigned i = blockIdx.x / kWgs, q = (blockIdx.x % kWgs) * kBlock + threadIdx.x;
  const unsigned y = q / (S / 4), x0 = (q % (S / 4)) * 4;
  const AImg im = imgs[i];
  const unsigned sy = ((2u * y + 1u) * im.h) / (2u * S);
  const unsigned char* row = src + im.off + (size_t)sy * im.stride;
  unsigned b[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned sx = ((2u * (x0 + j) + 1u) * im.w) / (2u * S);
    const unsigned char* p = row + (size_t)sx * CH;
    b[3 * j] = p[0];
    b[3 * j + 1] = CH == 1 ? b[3 * j] : p[1];
    b[3 * j + 2] = CH == 1 ? b[3 * j] : p[2];
  }
  unsigned* d = reinterpret_cast<unsigned*>(planes + (size_t)(first + i) * ((size_t)S * S * 3) + (size_t)y * (S * 3) + x0 * 3);
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = b[4 * k] | b[4 * k + 1] << 8 | b[4 * k + 2] << 16 | b[4 * k + 3] << 24;
}

// ---- spatial ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void flush_shifts(unsigned (&acc)[kShifts], unsigned* __restrict__ out, unsigned yi, unsigned lane) {
#pragma unroll
  for (int xi = 0; xi < kShifts; ++xi) {
    unsigned v = acc[xi];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if (lane == 0 && v) atomicAdd(&out[xi * kShifts + yi], v);
    acc[xi] = 0;
  }
}

// planes: plane 0 the left image, plane 1 + i right image i; table: n x 289, zeroed.  Workgroup = (pair, band).
// Every read stays inside the two planes: the staged rows are rows y0 - 8 .. y0 + kBand + 7 <= 255 of plane 0, whole; a
// lane reads dwords 4c .. 4c + 15 <= 191 of a staged row, because the shifts whose operand starts on a dword (xo = -8, -4,
// 0, 4, 8) take the low dword alone and the others need no dword above 4c + 15; the right window is bytes 24 .. 743.
__global__ __launch_bounds__(kBlock) void k_align_sad(const unsigned char* __restrict__ planes, unsigned* __restrict__ table) {
  __shared__ uint4 sl[kLdsRows * kRow / 16];
  const unsigned tid = threadIdx.x, pair = blockIdx.x / kBands, band = blockIdx.x % kBands;
  const unsigned y0 = 8 + band * kBand;  // the band's first right row
  const uint4* lsrc = reinterpret_cast<const uint4*>(planes + (size_t)(y0 - 8) * kRow);
  for (unsigned k = tid; k < kLdsRows * kRow / 16; k += kBlock) sl[k] = lsrc[k];
  __syncthreads();
  const unsigned char* rp = planes + (size_t)(pair + 1) * kPlaneS + (size_t)y0 * kRow + 24;
  unsigned* out = table + (size_t)pair * kTable;
  const unsigned wave = tid >> 6, lane = tid & 63;
  const unsigned u0 = wave * kUnitsPerWave, u1 = min((unsigned)kUnits, u0 + kUnitsPerWave);
  unsigned acc[kShifts];
#pragma unroll
  for (int xi = 0; xi < kShifts; ++xi) acc[xi] = 0;
  unsigned cur = u0 / kRounds;
  for (unsigned u = u0; u < u1; ++u) {
    const unsigned yi = u / kRounds, round = u - yi * kRounds;  // yi = yo + 8
    if (yi != cur) {
      flush_shifts(acc, out, cur, lane);
      cur = yi;
    }
    const unsigned item = round * 64 + lane;
    if (item < kItems) {
      const unsigned r = item / kQuads, c = item - r * kQuads;
      const uint2* rq = reinterpret_cast<const uint2*>(rp + (size_t)r * kRow + c * 16);  // (8-byte aligned: 24 + 16 c)
      const uint2 r01 = rq[0], r23 = rq[1];
      const unsigned rr[4] = {r01.x, r01.y, r23.x, r23.y};
      const uint4* lq = sl + (r + yi) * (kRow / 16) + c;  // left row y + yo = staged row r + yo + 8
      unsigned l[16];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint4 v = lq[t];
        l[4 * t] = v.x, l[4 * t + 1] = v.y, l[4 * t + 2] = v.z, l[4 * t + 3] = v.w;
      }
#pragma unroll
      for (int xi = 0; xi < kShifts; ++xi) {
        const int byte = 3 * xi, d = byte >> 2, s = byte & 3;  // byte 24 + 3 xo of the row is byte 3 xi of l[]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned a = s ? __builtin_amdgcn_alignbyte(l[d + j + (s ? 1 : 0)], l[d + j], (unsigned)s) : l[d + j];
          acc[xi] = __builtin_amdgcn_sad_u8(a, rr[j], acc[xi]);
        }
      }
    }
  }
  if (u0 < u1) flush_shifts(acc, out, cur, lane);
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long k) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)k, d, 64), hi = __shfl_xor((unsigned)(k >> 32), d, 64);
    const unsigned long long o = (unsigned long long)hi << 32 | lo;
    k = o < k ? o : k;
  }
  return k;
}

// the first shift in scan order (xo outer, yo inner: the table's order) whose sad is below every earlier one
__global__ __launch_bounds__(64) void k_align_pick(const unsigned* __restrict__ table, cbh_align_spatial_result* __restrict__ res) {
  const unsigned* t = table + (size_t)blockIdx.x * kTable;
  unsigned long long k = ~0ull;
  for (unsigned i = threadIdx.x; i < (unsigned)kTable; i += 64) {
    const unsigned long long mine = (unsigned long long)t[i] << 9 | i;
    k = mine < k ? mine : k;
  }
  k = wave_min(k);
  if (threadIdx.x == 0) {
    const unsigned idx = (unsigned)(k & 511u);
    cbh_align_spatial_result r;
    r.min_x = (int)(idx / kShifts) - 8, r.min_y = (int)(idx % kShifts) - 8;
    r.min_sad = (unsigned)(k >> 9), r.sad_at_zero = t[8 * kShifts + 8];
    res[blockIdx.x] = r;
  }
}

// ---- temporal -----------------------------------------------------------------------------------------------------------
// planes: nL left planes, then W right planes.  cells[d * W + i] = sad(F[d + i], G[i]): 3072 uint4 per plane, 12 a thread
__global__ __launch_bounds__(kBlock) void k_align_cell(const unsigned char* __restrict__ planes, unsigned n_left, unsigned window,
                                                       unsigned* __restrict__ cells) {
  __shared__ unsigned part[kBlock / 64];
  const unsigned d = blockIdx.x / window, i = blockIdx.x - d * window, tid = threadIdx.x;
  const uint4* f = reinterpret_cast<const uint4*>(planes + (size_t)(d + i) * kPlaneT);
  const uint4* g = reinterpret_cast<const uint4*>(planes + (size_t)(n_left + i) * kPlaneT);
  unsigned acc = 0;
#pragma unroll 4
  for (unsigned k = tid; k < kPlaneT / 16; k += kBlock) {
    const uint4 a = f[k], b = g[k];
    acc = __builtin_amdgcn_sad_u8(a.x, b.x, acc);
    acc = __builtin_amdgcn_sad_u8(a.y, b.y, acc);
    acc = __builtin_amdgcn_sad_u8(a.z, b.z, acc);
    acc = __builtin_amdgcn_sad_u8(a.w, b.w, acc);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) acc += __shfl_down(acc, s, 64);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) cells[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// (a sum of at most 64 cells of at most 12 533 760 fits 32 bits)
__global__ __launch_bounds__(kBlock) void k_align_means(const unsigned* __restrict__ cells, unsigned placements, unsigned window,
                                                        unsigned* __restrict__ means) {
  const unsigned d = blockIdx.x * kBlock + threadIdx.x;
  if (d >= placements) return;
  unsigned sum = 0;
  for (unsigned i = 0; i < window; ++i) sum += cells[(size_t)d * window + i];
  means[d] = sum / window;
}

// best = start, min = mean(start); for d ascending, mean(d) < min replaces both: the earliest placement of the smallest
// mean if that mean is below the start's, else the start
__global__ __launch_bounds__(kBlock) void k_align_tpick(const unsigned* __restrict__ means, unsigned placements, unsigned start,
                                                        cbh_align_temporal_result* __restrict__ res) {
  __shared__ unsigned long long part[kBlock / 64];
  const unsigned tid = threadIdx.x;
  unsigned long long k = ~0ull;
  for (unsigned d = tid; d < placements; d += kBlock) {
    const unsigned long long mine = (unsigned long long)means[d] << 16 | d;
    k = mine < k ? mine : k;
  }
  k = wave_min(k);
  if ((tid & 63) == 0) part[tid >> 6] = k;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kBlock / 64; ++w) k = part[w] < k ? part[w] : k;
    const unsigned at_start = means[start], lowest = (unsigned)(k >> 16);
    cbh_align_temporal_result r;
    r.placement = lowest < at_start ? (int)(k & 0xffffu) : (int)start;
    r.offset = r.placement - (int)start;
    r.min_mean = lowest < at_start ? lowest : at_start;
    r.start_mean = at_start;
    *res = r;
  }
}

// ---- the host side ------------------------------------------------------------------------------------------------------
int inval(const char* why) {
  set_last_error_text(why);
  return CBH_E_INVAL;
}
bool side_ok(uint32_t w, uint32_t h, uint32_t stride, int channels) {
  return w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide && stride >= w * (uint32_t)channels;
}
// the tables of n images: 0, or the error's code
int tables_ok(const char* who, size_t n, const uint64_t* off, const uint32_t* w, const uint32_t* h, const uint32_t* stride,
              int channels, bool host, size_t bytes) {
  for (size_t i = 0; i < n; ++i) {
    if (!side_ok(w[i], h[i], stride[i], channels))
      return inval((std::string(who) + ": an image has a side of 0 or above 32767, or rows shorter than its pixels").c_str());
    if (host && image_end(off[i], w[i], h[i], stride[i], channels) > bytes)
      return inval((std::string(who) + ": an image ends outside its buffer").c_str());
  }
  return CBH_OK;
}

template <int S>
void launch_scale(int ch, const uint8_t* src, const AImg* imgs, size_t n, unsigned first, uint8_t* planes, hipStream_t s) {
  const dim3 grid((unsigned)(n * (S * S / 4 / kBlock))), block(kBlock);
  if (ch == 1) hipLaunchKernelGGL((k_align_scale<1, S>), grid, block, 0, s, src, imgs, first, planes);
  else if (ch == 3) hipLaunchKernelGGL((k_align_scale<3, S>), grid, block, 0, s, src, imgs, first, planes);
  else hipLaunchKernelGGL((k_align_scale<4, S>), grid, block, 0, s, src, imgs, first, planes);
}

int spatial_args(int left_w, int left_h, size_t left_row_stride, int left_channels, size_t n, int channels) {
  if (!channels_ok(channels) || !channels_ok(left_channels)) return inval("align spatial: a channel count is not 1, 3 or 4");
  if (n > kMaxBatch) return inval("align spatial: more than 2^20 right images");
  if (left_w < 1 || left_h < 1 || left_row_stride > 0xffffffffu ||
      !side_ok((uint32_t)left_w, (uint32_t)left_h, (uint32_t)left_row_stride, left_channels))
    return inval("align spatial: the left image has a side of 0 or above 32767, or rows shorter than its pixels");
  return CBH_OK;
}

int temporal_args(size_t n_left, int left_channels, size_t n_right, int right_channels, int start) {
  if (!channels_ok(left_channels) || !channels_ok(right_channels)) return inval("align temporal: a channel count is not 1, 3 or 4");
  if (n_right < 1 || n_right > 64) return inval("align temporal: the window is 1 .. 64 right frames");
  if (n_left < n_right) return inval("align temporal: fewer left frames than the window has");
  if (n_left > 65535) return inval("align temporal: more than 65535 left frames");
  if (start < 0 || (size_t)start >= n_left - n_right + 1) return inval("align temporal: start is no placement");
  return CBH_OK;
}

}  // namespace
}  // namespace cbh

extern "C" {

int cbh_align_spatial_dev(const void* d_left, int left_w, int left_h, size_t left_row_stride, int left_channels,
                          const void* d_rights, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                          const uint32_t* img_h, const uint32_t* img_row_stride, int channels, void* d_results, void* d_table,
                          int device, void* stream) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  int rc = spatial_args(left_w, left_h, left_row_stride, left_channels, n, channels);
  if (rc != CBH_OK) return rc;
  if (n == 0) return CBH_OK;
  if (!d_left || !d_rights || !img_off || !img_w || !img_h || !img_row_stride || !d_results)
    return inval("align spatial: a required pointer is NULL");
  if ((rc = tables_ok("align spatial", n, img_off, img_w, img_h, img_row_stride, channels, false, 0)) != CBH_OK) return rc;
  std::vector<AImg> imgs(n + 1);
  imgs[0] = {0, (unsigned)left_w, (unsigned)left_h, (unsigned)left_row_stride};
  for (size_t i = 0; i < n; ++i) imgs[i + 1] = {img_off[i], img_w[i], img_h[i], img_row_stride[i]};
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  Scratch scratch(s);
  AImg* di = nullptr;
  uint8_t* planes = nullptr;
  unsigned* table = (unsigned*)d_table;
  hipError_t e = upload(scratch, &di, imgs, s);
  // n + 1 whole planes and not a byte more: no kernel reads past a plane's last row (k_align_sad says why)
  if (e == hipSuccess) e = scratch.get(&planes, (n + 1) * kPlaneS);
  if (e == hipSuccess && !table) e = scratch.get(&table, n * kTable * sizeof(unsigned));
  if (e == hipSuccess) e = hipMemsetAsync(table, 0, n * kTable * sizeof(unsigned), s);
  if (e == hipSuccess) {
    launch_scale<kSpatial>(left_channels, (const uint8_t*)d_left, di, 1, 0, planes, s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    launch_scale<kSpatial>(channels, (const uint8_t*)d_rights, di + 1, n, 1, planes, s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_align_sad, dim3((unsigned)(n * kBands)), dim3(kBlock), 0, s, planes, table);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_align_pick, dim3((unsigned)n), dim3(64), 0, s, table, (cbh_align_spatial_result*)d_results);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the host table above must outlive its copy
  return e == hipSuccess ? CBH_OK : fail("align spatial", e);
}

int cbh_align_spatial(const uint8_t* left, int left_w, int left_h, size_t left_row_stride, int left_channels,
                      const uint8_t* rights, size_t rights_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                      const uint32_t* img_h, const uint32_t* img_row_stride, int channels, cbh_align_spatial_result* results,
                      uint32_t* table, int device) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  int rc = spatial_args(left_w, left_h, left_row_stride, left_channels, n, channels);
  if (rc != CBH_OK) return rc;
  if (n == 0) return CBH_OK;
  if (!left || !rights || !img_off || !img_w || !img_h || !img_row_stride || !results)
    return inval("align spatial: a required pointer is NULL");
  if ((rc = tables_ok("align spatial", n, img_off, img_w, img_h, img_row_stride, channels, true, rights_bytes)) != CBH_OK)
    return rc;
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  const size_t left_bytes = (size_t)(left_h - 1) * left_row_stride + (size_t)left_w * left_channels;
  Staging st("align spatial");
  uint8_t *d_left, *d_rights;
  cbh_align_spatial_result* d_results;
  uint32_t* d_table = nullptr;
  st.alloc(&d_left, left_bytes);
  st.alloc(&d_rights, rights_bytes);
  st.alloc(&d_results, n * sizeof(cbh_align_spatial_result));
  if (table) st.alloc(&d_table, n * kTable * sizeof(uint32_t));
  st.up(d_left, left, left_bytes);
  st.up(d_rights, rights, rights_bytes);
  rc = st.status();
  if (rc == CBH_OK)
    rc = cbh_align_spatial_dev(d_left, left_w, left_h, left_row_stride, left_channels, d_rights, n, img_off, img_w, img_h,
                               img_row_stride, channels, d_results, d_table, device, st.s);
  if (rc != CBH_OK) return rc;
  st.down(results, d_results, n * sizeof(cbh_align_spatial_result));
  if (table) st.down(table, d_table, n * kTable * sizeof(uint32_t));
  st.sync();
  return st.status();
}

int cbh_align_temporal_dev(const void* d_left, size_t n_left, const uint64_t* left_off, const uint32_t* left_w,
                           const uint32_t* left_h, const uint32_t* left_row_stride, int left_channels, const void* d_right,
                           size_t n_right, const uint64_t* right_off, const uint32_t* right_w, const uint32_t* right_h,
                           const uint32_t* right_row_stride, int right_channels, int start, void* d_result, void* d_means,
                           void* d_cells, int device, void* stream) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  int rc = temporal_args(n_left, left_channels, n_right, right_channels, start);
  if (rc != CBH_OK) return rc;
  if (!d_left || !d_right || !left_off || !left_w || !left_h || !left_row_stride || !right_off || !right_w || !right_h ||
      !right_row_stride || !d_result)
    return inval("align temporal: a required pointer is NULL");
  if ((rc = tables_ok("align temporal", n_left, left_off, left_w, left_h, left_row_stride, left_channels, false, 0)) != CBH_OK ||
      (rc = tables_ok("align temporal", n_right, right_off, right_w, right_h, right_row_stride, right_channels, false, 0)) != CBH_OK)
    return rc;
  const unsigned nl = (unsigned)n_left, window = (unsigned)n_right, placements = nl - window + 1;
  std::vector<AImg> imgs(n_left + n_right);
  for (size_t i = 0; i < n_left; ++i) imgs[i] = {left_off[i], left_w[i], left_h[i], left_row_stride[i]};
  for (size_t i = 0; i < n_right; ++i) imgs[n_left + i] = {right_off[i], right_w[i], right_h[i], right_row_stride[i]};
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  Scratch scratch(s);
  AImg* di = nullptr;
  uint8_t* planes = nullptr;
  unsigned *cells = (unsigned*)d_cells, *means = (unsigned*)d_means;
  hipError_t e = upload(scratch, &di, imgs, s);
  if (e == hipSuccess) e = scratch.get(&planes, (n_left + n_right) * kPlaneT);
  if (e == hipSuccess && !cells) e = scratch.get(&cells, (size_t)placements * window * sizeof(unsigned));
  if (e == hipSuccess && !means) e = scratch.get(&means, (size_t)placements * sizeof(unsigned));
  if (e == hipSuccess) {
    launch_scale<kTemporal>(left_channels, (const uint8_t*)d_left, di, n_left, 0, planes, s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    launch_scale<kTemporal>(right_channels, (const uint8_t*)d_right, di + n_left, n_right, nl, planes, s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_align_cell, dim3(placements * window), dim3(kBlock), 0, s, planes, nl, window, cells);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_align_means, dim3((placements + kBlock - 1) / kBlock), dim3(kBlock), 0, s, cells, placements, window,
                       means);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_align_tpick, dim3(1), dim3(kBlock), 0, s, means, placements, (unsigned)start,
                       (cbh_align_temporal_result*)d_result);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the host table above must outlive its copy
  return e == hipSuccess ? CBH_OK : fail("align temporal", e);
}

int cbh_align_temporal(const uint8_t* left, size_t left_bytes, size_t n_left, const uint64_t* left_off, const uint32_t* left_w,
                       const uint32_t* left_h, const uint32_t* left_row_stride, int left_channels, const uint8_t* right,
                       size_t right_bytes, size_t n_right, const uint64_t* right_off, const uint32_t* right_w,
                       const uint32_t* right_h, const uint32_t* right_row_stride, int right_channels, int start,
                       cbh_align_temporal_result* result, uint32_t* means, uint32_t* cells, int device) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  int rc = temporal_args(n_left, left_channels, n_right, right_channels, start);
  if (rc != CBH_OK) return rc;
  if (!left || !right || !left_off || !left_w || !left_h || !left_row_stride || !right_off || !right_w || !right_h ||
      !right_row_stride || !result)
    return inval("align temporal: a required pointer is NULL");
  if ((rc = tables_ok("align temporal", n_left, left_off, left_w, left_h, left_row_stride, left_channels, true, left_bytes)) != CBH_OK ||
      (rc = tables_ok("align temporal", n_right, right_off, right_w, right_h, right_row_stride, right_channels, true, right_bytes)) != CBH_OK)
    return rc;
  const size_t placements = n_left - n_right + 1;
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  Staging st("align temporal");
  uint8_t *d_left, *d_right;
  cbh_align_temporal_result* d_result;
  uint32_t *d_means = nullptr, *d_cells = nullptr;
  st.alloc(&d_left, left_bytes);
  st.alloc(&d_right, right_bytes);
  st.alloc(&d_result, sizeof(cbh_align_temporal_result));
  if (means) st.alloc(&d_means, placements * sizeof(uint32_t));
  if (cells) st.alloc(&d_cells, placements * n_right * sizeof(uint32_t));
  st.up(d_left, left, left_bytes);
  st.up(d_right, right, right_bytes);
  rc = st.status();
  if (rc == CBH_OK)
    rc = cbh_align_temporal_dev(d_left, n_left, left_off, left_w, left_h, left_row_stride, left_channels, d_right, n_right,
                                right_off, right_w, right_h, right_row_stride, right_channels, start, d_result, d_means,
                                d_cells, device, st.s);
  if (rc != CBH_OK) return rc;
  st.down(result, d_result, sizeof(cbh_align_temporal_result));
  if (means) st.down(means, d_means, placements * sizeof(uint32_t));
  if (cells) st.down(cells, d_cells, placements * n_right * sizeof(uint32_t));
  st.sync();
  return st.status();
}

}  // extern "C"
