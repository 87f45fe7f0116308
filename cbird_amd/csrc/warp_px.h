// warp_px.h -- internal: warpAffine's pixel (remap's bilinear fixed-point path as tmatch.hip restates it) and the tables
// of the kernels that call it: k_warp (tmatch.hip, one patch size per launch) and k_warp_ragged (tmpairs.hip, a size per
// candidate).  ONE place for the arithmetic: both kernels give the same bytes for the same pixel.
#pragma once
#include <hip/hip_runtime.h>

namespace cbh {

struct WImage {
  unsigned long long off;
  unsigned w, h, stride, pad;
};
// a candidate of the grouped chain: its own template (size, bytes at tmpl_off, rows tstride apart), its patch at patch_off
// (16-byte aligned, pitch tw * channels) and its two grey planes at gray_off
struct PPatch {
  unsigned long long patch_off, tmpl_off, gray_off;
  unsigned tw, th, tstride, pad;
};

template <int CH>
__device__ __forceinline__ void warp_pixel(const unsigned char* __restrict__ imgs, const WImage& im,
                                           const double* __restrict__ M, int x, int X0, int Y0, unsigned (&px)[CH]) {
  // adelta[x], bdelta[x] (AB_BITS 10, INTER_BITS 5); cvRound = round half to even; X0 / Y0 are the row's (row_start)
  const int adx = (int)rint(M[0] * (double)x * 1024.0), bdx = (int)rint(M[3] * (double)x * 1024.0);
  const int X = (X0 + adx) >> 5, Y = (Y0 + bdx) >> 5;
  const int sx = min(max(X >> 5, -32768), 32767), sy = min(max(Y >> 5, -32768), 32767);  // saturate_cast<short>
  const int fx = X & 31, fy = Y & 31;
  const int wgt[4] = {(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32};
  int acc[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) acc[c] = 16384;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int xx = sx + (t & 1), yy = sy + (t >> 1);
    const bool inside = xx >= 0 && xx < (int)im.w && yy >= 0 && yy < (int)im.h;
    const unsigned char* p = imgs + im.off + (unsigned long long)(inside ? yy : 0) * im.stride + (size_t)(inside ? xx : 0) * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int border = (CH == 4 && c == 3) ? 255 : 0;  // Scalar(0, 0, 0, 255)
      acc[c] += wgt[t] * (inside ? (int)p[c] : border);
    }
  }
#pragma unroll
  for (int c = 0; c < CH; ++c) px[c] = (unsigned)(acc[c] >> 15);
}

// X0 / Y0 of a patch row
__device__ __forceinline__ void row_start(const double* __restrict__ M, int y, int& X0, int& Y0) {
  X0 = (int)rint((M[1] * (double)y + M[2]) * 1024.0) + 16, Y0 = (int)rint((M[4] * (double)y + M[5]) * 1024.0) + 16;
}

}  // namespace cbh
