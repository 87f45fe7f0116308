// stretch_px.h -- stretchContrast of one byte (src/cvutil.cpp:628-655): min >= max copies; else alpha = 255 /
// float(max - min), beta = -min * alpha and convertTo's saturate_cast<uchar>(cvRound(s * alpha + beta)) -- a float
// multiply, a float add, round half to even (the library is built with -ffp-contract=off, so nothing is fused).
// k_diff_tables (diffimage.hip) and k_dm_class (demosaic.hip) both call it, so their stretched bytes are the same.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned cbh_stretch_px(int lo, int hi, unsigned s) {
  if (lo >= hi) return s;
  const float alpha = 255.0f / (float)(hi - lo);
  const float beta = (float)(-lo) * alpha;
  const float prod = (float)s * alpha;
  const float r = rintf(prod + beta);
  return r <= 0.0f ? 0u : r >= 255.0f ? 255u : (unsigned)r;
}
