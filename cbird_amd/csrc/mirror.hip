// mirror.hip -- the images Engine::mirrored hands to processImage (src/engine.cpp:357-365: QImage::mirrored(h, v)) for
// a reflection search (Engine::query, :423-436), made on the device from ONE upload.  k_gray_views reads each image once
// and writes the grey planes of the identity view and of the requested reflections (H, V, both), and with the colour
// leg the reflected colour images as well; every stage after the grey image takes them as a batch of planes.
//
// A thread owns 16 consecutive pixels of one source row: 16 * CH bytes in CH 16-byte loads (rows that are 16-byte aligned;
// others, and the last chunk of a row, byte by byte), 16 grey bytes in four dwords, and for each view one 16-byte store
// of those dwords -- reversed in registers (v_perm_b32) for the views that flip left and right -- where the destination
// is aligned, byte stores elsewhere.  Bound by HBM: w*h*CH bytes read, V*w*h written (+ (V-1)*w*h*CH with colour).
#include <cstdint>

#include "cbh_index.h"
#include "gray_px.h"

namespace {

__device__ __forceinline__ unsigned byte_of(const unsigned* v, int i) { return (v[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// QImage::mirrored(horizontal, vertical) for the flags of SearchParams::mirrorMask (src/index.h:51-59), in the order
// Engine::query takes them: 1 = left-right, 2 = top-bottom, 4 = both
__device__ __forceinline__ bool flips_x(int flag) { return flag == 1 || flag == 4; }
__device__ __forceinline__ bool flips_y(int flag) { return flag == 2 || flag == 4; }

template <int CH, bool COLOR>
__global__ __launch_bounds__(256) void k_gray_views(const unsigned char* __restrict__ src, int w, int h, size_t row_stride,
                                                    size_t img_stride, int mask, int nv,
                                                    unsigned char* __restrict__ gray /* n*nv planes of w*h */,
                                                    unsigned char* __restrict__ color /* n*(nv-1) images w*h*CH */) {
  const size_t img = blockIdx.y, plane = (size_t)w * h;
  const unsigned char* s = src + img * img_stride;
  unsigned char* g0 = gray + img * (size_t)nv * plane;
  unsigned char* c0 = COLOR ? color + img * (size_t)(nv - 1) * plane * CH : nullptr;
  const int cpr = (w + 15) >> 4;  // 16-pixel chunks per row
  const size_t total = (size_t)cpr * h;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const int y = (int)(t / cpr), x0 = (int)(t - (size_t)y * cpr) * 16;
    const int np = min(16, w - x0);  // pixels of this chunk inside the row
    const unsigned char* p = s + (size_t)y * row_stride + (size_t)x0 * CH;
    unsigned px[4 * CH];  // the chunk's 16 * CH source bytes
    if (np == 16 && ((uintptr_t)p & 15) == 0) {
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        const uint4 q = reinterpret_cast<const uint4*>(p)[k];
        px[4 * k] = q.x, px[4 * k + 1] = q.y, px[4 * k + 2] = q.z, px[4 * k + 3] = q.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4 * CH; ++k) px[k] = 0;
#pragma unroll
      for (int b = 0; b < 16 * CH; ++b)
        if (b < np * CH) px[b >> 2] |= (unsigned)p[b] << (8 * (b & 3));
    }
    unsigned gw[4];  // grey bytes of the 16 pixels, pixel j in byte j
    if (CH == 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) gw[k] = px[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        unsigned v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int b = (4 * k + j) * CH;
          v |= (unsigned)cbh_gray_px((int)byte_of(px, b), (int)byte_of(px, b + 1), (int)byte_of(px, b + 2)) << (8 * j);
        }
        gw[k] = v;
      }
    }
    unsigned gr[4];  // the same 16 bytes in reverse order: pixel j in byte 15 - j
#pragma unroll
    for (int k = 0; k < 4; ++k) gr[k] = __builtin_amdgcn_perm(0u, gw[3 - k], 0x00010203u);
    int slot = 0;
#pragma unroll
    for (int f = 0; f < 3 + 1; ++f) {
      const int flag = f == 0 ? 0 : 1 << (f - 1);
      if (flag && !(mask & flag)) continue;
      const bool fx = flips_x(flag);
      const size_t yy = (size_t)(flips_y(flag) ? h - 1 - y : y);
      // destination of pixel 0 of a whole chunk (a flipped chunk's 16 pixels end at w - x0)
      const int dx = fx ? w - x0 - 16 : x0;
      unsigned char* gd = g0 + (size_t)slot * plane + yy * (size_t)w;
      unsigned char* gq = gd + dx;
      if (np == 16 && ((uintptr_t)gq & 15) == 0) {
        *reinterpret_cast<uint4*>(gq) = fx ? make_uint4(gr[0], gr[1], gr[2], gr[3]) : make_uint4(gw[0], gw[1], gw[2], gw[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (j < np) gd[fx ? w - 1 - x0 - j : x0 + j] = (unsigned char)byte_of(gw, j);
      }
      if (COLOR && flag) {
        unsigned char* cd = c0 + (size_t)(slot - 1) * plane * CH + yy * (size_t)w * CH;
        unsigned char* cq = cd + (ptrdiff_t)dx * CH;
        if (np == 16 && ((uintptr_t)cq & 15) == 0) {
          unsigned o[4 * CH];
          if (!fx) {
#pragma unroll
            for (int k = 0; k < 4 * CH; ++k) o[k] = px[k];
          } else if (CH == 4) {
#pragma unroll
            for (int k = 0; k < 16; ++k) o[k] = px[15 - k];
          } else {  // 3-byte pixels: pixel j of the output is pixel 15 - j of the source (constant byte moves)
#pragma unroll
            for (int k = 0; k < 4 * CH; ++k) {
              unsigned v = 0;
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int b = 4 * k + j, q = b / CH, c = b - q * CH;
                v |= byte_of(px, (15 - q) * CH + c) << (8 * j);
              }
              o[k] = v;
            }
          }
#pragma unroll
          for (int k = 0; k < CH; ++k)
            reinterpret_cast<uint4*>(cq)[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        } else {
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (j < np) {
              unsigned char* d = cd + (size_t)(fx ? w - 1 - x0 - j : x0 + j) * CH;
#pragma unroll
              for (int c = 0; c < CH; ++c) d[c] = (unsigned char)byte_of(px, j * CH + c);
            }
        }
      }
      ++slot;
    }
  }
}

template <int CH>
void launch_views(const unsigned char* src, size_t m, int w, int h, size_t row_stride, size_t img_stride, int mask, int nv,
                  unsigned char* gray, unsigned char* color, hipStream_t s) {
  const size_t chunks = (size_t)((w + 15) >> 4) * h;
  const unsigned bx = (unsigned)std::min<size_t>(1024, (chunks + 255) / 256);
  if (color)
    hipLaunchKernelGGL((k_gray_views<CH, true>), dim3(bx, (unsigned)m), dim3(256), 0, s, src, w, h, row_stride, img_stride,
                       mask, nv, gray, color);
  else
    hipLaunchKernelGGL((k_gray_views<CH, false>), dim3(bx, (unsigned)m), dim3(256), 0, s, src, w, h, row_stride,
                       img_stride, mask, nv, gray, color);
}

}  // namespace

int cbh_gray_views_dev(const void* d_src, size_t n, int w, int h, size_t row_stride, size_t img_stride, int channels,
                       int mirror_mask, void* d_gray, void* d_color, int device, void* stream) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (mirror_mask < 0 || mirror_mask > 7) return CBH_E_INVAL;
  if (n == 0) return CBH_OK;
  if (!d_src || !d_gray || w <= 0 || h <= 0 || (channels != 1 && channels != 3 && channels != 4) ||
      row_stride < (size_t)w * channels)
    return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  const int nv = 1 + __builtin_popcount((unsigned)mirror_mask);
  unsigned char* color = nv > 1 ? (unsigned char*)d_color : nullptr;  // (no reflections: nothing to copy)
  const size_t plane = (size_t)w * h;
  for (size_t i0 = 0; i0 < n; i0 += 65535) {
    const size_t m = std::min<size_t>(65535, n - i0);
    const unsigned char* src = (const unsigned char*)d_src + i0 * img_stride;
    unsigned char* gr = (unsigned char*)d_gray + i0 * nv * plane;
    unsigned char* co = color ? color + i0 * (nv - 1) * plane * channels : nullptr;
    if (channels == 1) launch_views<1>(src, m, w, h, row_stride, img_stride, mirror_mask, nv, gr, co, s);
    else if (channels == 3) launch_views<3>(src, m, w, h, row_stride, img_stride, mirror_mask, nv, gr, co, s);
    else launch_views<4>(src, m, w, h, row_stride, img_stride, mirror_mask, nv, gr, co, s);
  }
  CBH_HIP(hipGetLastError());
  if (!stream) CBH_HIP(hipStreamSynchronize(s));
  return CBH_OK;
}
