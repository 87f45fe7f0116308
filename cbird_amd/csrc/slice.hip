// slice.hip -- Index::slice() on the device: the kernels behind cbh_idx256_slice and cbh_color_slice.
//
// cbird searches inside a subset by slicing every index once per command (Database::similar / similarTo with
// params.inSet, src/database.cpp:1325-1334, :1475-1483) and searching the slice like the whole index.  A slice keeps
// the entries whose mediaId is in a set, in index order; nothing is computed, bytes move:
//
//   256-bit rows   k_slice_rows: the host plans, from the maps, one (packed first, dst first, src first) range per kept
//                  media; a thread moves half a row and finds its range by binary search over the packed firsts
//   colour         k_slice_color: the planes l/u/v[32][cap], num and id of the kept entries from a list of source
//                  positions; the destination's padding (capacity a multiple of 4) is written as the distance kernels
//                  expect it (color.hip): 1e18 in L, no colours, id 0
//
// (The 64-bit index still slices through the host, cbh_idx64_slice in cbird_hip.hip: its route changes only with a
// measurement that shows no size of index made slower.)
//
// Stores are 16 bytes per lane, and so are the loads of the rows.  Every index x stride product is 64-bit.  HBM-bound,
// no scratch memory.
#include <algorithm>
#include <atomic>

#include "cbh_internal.h"

namespace cbh {
namespace {

std::atomic<long long> g_slices_on_device{0};

// Row ranges: range r covers packed rows [pk[r], pk[r + 1]) = dst rows from dstf[r] = src rows from srcf[r].
// A thread moves 16 bytes, half a row.
__global__ __launch_bounds__(256) void k_slice_rows(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                    const uint32_t* __restrict__ pk, const uint32_t* __restrict__ dstf,
                                                    const uint32_t* __restrict__ srcf, uint32_t n_ranges,
                                                    unsigned long long halves) {
  for (unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x; g < halves;
       g += (unsigned long long)gridDim.x * 256) {
    const uint32_t row = (uint32_t)(g >> 1);
    uint32_t lo = 0, hi = n_ranges;  // last range whose packed first is <= row
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (pk[mid] <= row)
        lo = mid;
      else
        hi = mid;
    }
    const uint32_t k = row - pk[lo];
    const unsigned long long half = g & 1ull;
    dst[((unsigned long long)dstf[lo] + k) * 2 + half] = src[((unsigned long long)srcf[lo] + k) * 2 + half];
  }
}

// blockIdx.y: 0..95 = the planes L, U, V x 32 colours; 96 = ids; 97 = num.  A lane takes 4 consecutive destination
// entries (dst_cap is a multiple of 4, so is every plane's start: 16-byte stores) up to dst_cap: entries past m are the
// padding.
__global__ __launch_bounds__(256) void k_slice_color(const float* __restrict__ sL, const float* __restrict__ sU,
                                                     const float* __restrict__ sV,
                                                     const unsigned char* __restrict__ s_num,
                                                     const uint32_t* __restrict__ s_ids, size_t src_cap,
                                                     const uint32_t* __restrict__ pos, uint32_t m, float* __restrict__ dL,
                                                     float* __restrict__ dU, float* __restrict__ dV,
                                                     unsigned char* __restrict__ d_num, uint32_t* __restrict__ d_ids,
                                                     size_t dst_cap) {
  const size_t j = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (j >= dst_cap) return;
  uint32_t p[4] = {0, 0, 0, 0};
  if (j + 4 <= m) {
    const uint4 q = *reinterpret_cast<const uint4*>(pos + j);
    p[0] = q.x, p[1] = q.y, p[2] = q.z, p[3] = q.w;
  } else {
    for (unsigned k = 0; k < 4; ++k)
      if (j + k < m) p[k] = pos[j + k];
  }
  const unsigned y = blockIdx.y;
  if (y < 96) {
    const unsigned which = y >> 5, colour = y & 31;
    const float* s = (which == 0 ? sL : which == 1 ? sU : sV) + (size_t)colour * src_cap;
    float* d = (which == 0 ? dL : which == 1 ? dU : dV) + (size_t)colour * dst_cap;
    const float pad = which == 0 ? 1e18f : 0.f;
    float4 v;
    v.x = j + 0 < m ? s[p[0]] : pad;
    v.y = j + 1 < m ? s[p[1]] : pad;
    v.z = j + 2 < m ? s[p[2]] : pad;
    v.w = j + 3 < m ? s[p[3]] : pad;
    *reinterpret_cast<float4*>(d + j) = v;
  } else if (y == 96) {
    uint4 v;
    v.x = j + 0 < m ? s_ids[p[0]] : 0u;
    v.y = j + 1 < m ? s_ids[p[1]] : 0u;
    v.z = j + 2 < m ? s_ids[p[2]] : 0u;
    v.w = j + 3 < m ? s_ids[p[3]] : 0u;
    *reinterpret_cast<uint4*>(d_ids + j) = v;
  } else {
    uint32_t v = 0;
#pragma unroll
    for (unsigned k = 0; k < 4; ++k)
      if (j + k < m) v |= (uint32_t)s_num[p[k]] << (8 * k);
    *reinterpret_cast<uint32_t*>(d_num + j) = v;
  }
}

}  // namespace

void note_slice_on_device() { g_slices_on_device++; }
long long get_slices_on_device() { return g_slices_on_device.load(); }

// d_table: 3 x (n_ranges + 1) words -- packed firsts (ascending from 0, the last one = total_rows), dst firsts, src firsts
int launch_slice_rows256(const uint8_t* d_src, uint8_t* d_dst, const uint32_t* d_table, size_t n_ranges,
                         size_t total_rows, hipStream_t stream) {
  if (total_rows == 0 || n_ranges == 0) return CBH_OK;
  if (n_ranges > 0xfffffff0ull || total_rows > 0xfffffff0ull) return CBH_E_INVAL;
  const unsigned long long halves = (unsigned long long)total_rows * 2;
  const unsigned grid = (unsigned)std::min<unsigned long long>((halves + 255) / 256, 1u << 16);
  hipLaunchKernelGGL(k_slice_rows, dim3(grid), dim3(256), 0, stream, (const uint4*)d_src, (uint4*)d_dst, d_table,
                     d_table + (n_ranges + 1), d_table + 2 * (n_ranges + 1), (uint32_t)n_ranges, halves);
  CBH_HIP(hipGetLastError());
  return CBH_OK;
}

// entries d_pos[0..m) of the source planes to entries 0..m of the destination planes, padding up to dst_cap
// (a multiple of 4, >= m)
int launch_slice_color(const float* sL, const float* sU, const float* sV, const unsigned char* s_num,
                       const uint32_t* s_ids, size_t src_cap, const uint32_t* d_pos, size_t m, float* dL, float* dU,
                       float* dV, unsigned char* d_num, uint32_t* d_ids, size_t dst_cap, hipStream_t stream) {
  if (dst_cap == 0) return CBH_OK;
  if ((dst_cap & 3) || m > dst_cap || dst_cap > 0xfffffff0ull) return CBH_E_INVAL;
  const unsigned gx = (unsigned)((dst_cap / 4 + 255) / 256);
  hipLaunchKernelGGL(k_slice_color, dim3(gx, 98), dim3(256), 0, stream, sL, sU, sV, s_num, s_ids, src_cap, d_pos,
                     (uint32_t)m, dL, dU, dV, d_num, d_ids, dst_cap);
  CBH_HIP(hipGetLastError());
  return CBH_OK;
}

}  // namespace cbh
