// gray_px.h -- grayscale() of one pixel: cv::cvtColor BGR/BGRA -> gray on 8-bit data, 14-bit fixed point
// (src/cvutil.cpp:1265-1283).  k_bgr2gray (prestage.hip) and k_gray_views (mirror.hip) both call it, so their grey
// planes are the same bytes.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned char cbh_gray_px(int b, int g, int r) {
  return (unsigned char)((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14);
}
