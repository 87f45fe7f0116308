// demosaic.hip -- demosaicHough (src/cvutil.cpp:1445-1688) for a ragged batch of contact sheets: every tile of a sheet as
// a rectangle, in the reference's order.  include/cbird_hip.h states the rules, tests/demosaic_rules.py is the numpy model.
// Everything the device computes is an integer; the only floats are the two products and the sum of a diagonal vote.
// A pass takes a list of views (an image, or a rectangle of one that is subdivided) and runs
//   cbh_auto_contrast_dev   the cuts of every view (diffimage.hip's histogram and cut kernels, nothing restated)
//   k_dm_class      a workgroup takes a 64 x 16 tile: the stretched grey of the 70 x 22 pixels around it into LDS (the
//                   table of cbh_stretch_px, cbh_gray_px), their 3 x 3 Gaussian (68 x 20), the Sobel magnitudes (66 x 18)
//                   and the class of its own pixels after non-maximum suppression: 0 none, 1 candidate, 2 strong
//   k_dm_hyst       a workgroup takes a 64 x 64 tile and its one-pixel halo into LDS and promotes candidates next to a
//                   strong pixel until the tile is at its fixed point (at most 4096 rounds, one per pixel); a tile that
//                   promoted something sets a flag, and the host launches the pass again while it is set: at most one
//                   launch per pixel of the largest view plus one, because a launch that sets the flag promotes a pixel.
//                   Classes only ever go from 1 to 2, so a halo read that misses a neighbour's promotion is caught by the
//                   next launch, and the fixed point is the flood fill
//   k_dm_edges      255 where the class is 2, through the 3 x 3 Gaussian when post_blur is set
//   k_dm_votes      the non-zero pixels of every row (a ballot per wave) and column (a register, then LDS), and of the
//                   45 and 135 degree bins that rows and columns land on: integer counts, so any order gives the same
// and the host applies the local-maximum rule to the counts, selectLines, the rectangles and the subdivision.
// Measured: no kernel is near the memory system's limit; they are bound by the byte loads and LDS passes they
// issue, and a pass by its hysteresis launches, each followed by a 4-byte copy of the flag and a stream synchronisation.
#include <cmath>
#include <cstdint>

#include <algorithm>
#include <string>
#include <vector>

#include "cbh_index.h"
#include "cbh_runs.h"
#include "cbh_staging.h"
#include "gray_px.h"
#include "stretch_px.h"

namespace cbh {
namespace {

constexpr int kBlock = 256;
constexpr int kTW = 64, kTH = 16;  // the tile of k_dm_class, k_dm_edges, k_dm_votes: a wave per row, four rows a step
constexpr int kHT = 64;            // the side of k_dm_hyst's tile
constexpr unsigned kMaxSide = 32767;
constexpr size_t kMaxBatch = (size_t)1 << 20;

struct MImg {
  unsigned long long off;    // first source byte
  unsigned long long plane;  // first byte of its class and edge planes: w * h bytes, rows of w
  unsigned long long acc;    // first word of its counters: rows [h], columns [w], 45 degrees [max(w, h)], 135 degrees [h]
  unsigned w, h, stride, pad;
};
struct MTile {
  unsigned img;
  unsigned short tx, ty;
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
// BORDER_REFLECT_101 for an index within one of the range; a 1-pixel side reflects onto itself
__device__ __forceinline__ int reflect101(int v, int n) { return n == 1 ? 0 : v < 0 ? -v : v >= n ? 2 * n - 2 - v : v; }

// ---- steps 1-3 without the hysteresis --------------------------------------------------------------------------------
// LDS rows are indexed by image coordinate minus the array's origin; every read below stays inside the arrays: the blur of
// position (X, Y) is taken at the clamped position, whose neighbours reflect into [clamp - 1, clamp + 1], inside the staged
// 70 x 22; the Sobel of an image pixel reads positions one further out, inside the 68 x 20; the suppression reads
// magnitudes one around the tile, inside the 66 x 18.
template <int CH>
__global__ __launch_bounds__(kBlock) void k_dm_class(const unsigned char* __restrict__ src, const MImg* __restrict__ imgs,
                                                     const MTile* __restrict__ tiles, const int* __restrict__ cuts,
                                                     int pre_blur, int low, int high, unsigned char* __restrict__ cls) {
  constexpr int GW = kTW + 6, GH = kTH + 6, BW = kTW + 4, BH = kTH + 4, MW = kTW + 2, MH = kTH + 2;
  __shared__ unsigned char tab[256];
  __shared__ unsigned char sg[GH][GW + 2];
  __shared__ unsigned char sb[BH][BW];
  __shared__ unsigned short sm[MH][MW];
  const int tid = threadIdx.x;
  const MTile t = tiles[blockIdx.x];
  const MImg im = imgs[t.img];
  const int w = (int)im.w, h = (int)im.h, x0 = t.tx * kTW, y0 = t.ty * kTH;
  tab[tid] = (unsigned char)cbh_stretch_px(cuts[2 * t.img], cuts[2 * t.img + 1], (unsigned)tid);
  __syncthreads();
  const unsigned char* s = src + im.off;
  for (int k = tid; k < GW * GH; k += kBlock) {
    const int ry = k / GW, rx = k - ry * GW;
    const int y = clampi(y0 - 3 + ry, h - 1), x = clampi(x0 - 3 + rx, w - 1);
    const unsigned char* p = s + (size_t)y * im.stride + (size_t)x * CH;
    sg[ry][rx] = CH == 1 ? tab[p[0]] : cbh_gray_px(tab[p[0]], tab[p[1]], tab[p[2]]);
  }
  __syncthreads();
  for (int k = tid; k < BW * BH; k += kBlock) {
    const int by = k / BW, bx = k - by * BW;
    const int cy = clampi(y0 - 2 + by, h - 1), cx = clampi(x0 - 2 + bx, w - 1);
    int v;
    if (pre_blur) {
      const int ya = reflect101(cy - 1, h) - (y0 - 3), yb = cy - (y0 - 3), yc = reflect101(cy + 1, h) - (y0 - 3);
      const int xa = reflect101(cx - 1, w) - (x0 - 3), xb = cx - (x0 - 3), xc = reflect101(cx + 1, w) - (x0 - 3);
      const int sum = (sg[ya][xa] + 2 * sg[ya][xb] + sg[ya][xc]) + 2 * (sg[yb][xa] + 2 * sg[yb][xb] + sg[yb][xc]) +
                      (sg[yc][xa] + 2 * sg[yc][xb] + sg[yc][xc]);
      v = (sum + 8) >> 4;
    } else {
      v = sg[cy - (y0 - 3)][cx - (x0 - 3)];
    }
    sb[by][bx] = (unsigned char)v;
  }
  __syncthreads();
  // sb[Y - (y0 - 2)][X - (x0 - 2)] is the blurred grey at the clamped position: BORDER_REPLICATE for the Sobel
  for (int k = tid; k < MW * MH; k += kBlock) {
    const int my = k / MW, mx = k - my * MW;
    const int X = x0 - 1 + mx, Y = y0 - 1 + my;
    int m = 0;
    if (X >= 0 && X < w && Y >= 0 && Y < h) {
      const unsigned char *a = sb[my], *b = sb[my + 1], *c = sb[my + 2];
      const int dx = (a[mx + 2] + 2 * b[mx + 2] + c[mx + 2]) - (a[mx] + 2 * b[mx] + c[mx]);
      const int dy = (c[mx] + 2 * c[mx + 1] + c[mx + 2]) - (a[mx] + 2 * a[mx + 1] + a[mx + 2]);
      m = abs(dx) + abs(dy);
    }
    sm[my][mx] = (unsigned short)m;
  }
  __syncthreads();
  unsigned char* out = cls + im.plane;
#pragma unroll
  for (int q = 0; q < kTW * kTH / kBlock; ++q) {
    const int py = (tid >> 6) + 4 * q, px = tid & 63;
    const int X = x0 + px, Y = y0 + py;
    if (X >= w || Y >= h) continue;
    const int my = py + 1, mx = px + 1;
    const unsigned char *a = sb[my], *b = sb[my + 1], *c = sb[my + 2];
    const int dx = (a[mx + 2] + 2 * b[mx + 2] + c[mx + 2]) - (a[mx] + 2 * b[mx] + c[mx]);
    const int dy = (c[mx] + 2 * c[mx + 1] + c[mx + 2]) - (a[mx] + 2 * a[mx + 1] + a[mx + 2]);
    const int m = sm[my][mx];
    int kind = 0;
    if (m > low) {
      const int ax = abs(dx), ay = abs(dy) << 15;
      const int t22 = ax * 13573, t67 = t22 + (ax << 16);
      bool keep;
      if (ay < t22) {
        keep = m > sm[my][mx - 1] && m >= sm[my][mx + 1];
      } else if (ay > t67) {
        keep = m > sm[my - 1][mx] && m >= sm[my + 1][mx];
      } else {
        const int sgn = (dx ^ dy) < 0 ? -1 : 1;
        keep = m > sm[my - 1][mx - sgn] && m > sm[my + 1][mx + sgn];
      }
      if (keep) kind = m > high ? 2 : 1;
    }
    out[(size_t)Y * w + X] = (unsigned char)kind;
  }
}

// ---- the hysteresis ------------------------------------------------------------------------------------------------------
// st[1 + y][1 + x] = class of tile pixel (x, y); the halo is 0 outside the image.  Thread tid owns pixels (tid & 63,
// (tid >> 6) + 4 q), q = 0 .. 15, and is the only one that writes them, in LDS and in global memory.
__global__ __launch_bounds__(kBlock) void k_dm_hyst(const MImg* __restrict__ imgs, const MTile* __restrict__ tiles,
                                                    unsigned char* cls, unsigned* __restrict__ flag) {
  constexpr int SW = kHT + 2;
  __shared__ unsigned char st[SW][SW + 2];
  const int tid = threadIdx.x;
  const MTile t = tiles[blockIdx.x];
  const MImg im = imgs[t.img];
  const int w = (int)im.w, h = (int)im.h, x0 = t.tx * kHT, y0 = t.ty * kHT;
  unsigned char* plane = cls + im.plane;
  for (int k = tid; k < SW * SW; k += kBlock) {
    const int ry = k / SW, rx = k - ry * SW;
    const int X = x0 - 1 + rx, Y = y0 - 1 + ry;
    st[ry][rx] = (X >= 0 && X < w && Y >= 0 && Y < h) ? plane[(size_t)Y * w + X] : 0;
  }
  __syncthreads();
  const int px = (tid & 63) + 1, py0 = (tid >> 6) + 1;
  unsigned cand = 0;  // bit q: my pixel q is a candidate
#pragma unroll
  for (int q = 0; q < 16; ++q) cand |= (st[py0 + 4 * q][px] == 1 ? 1u : 0u) << q;
  if (!__syncthreads_or(cand != 0)) return;
  unsigned promoted = 0;
  for (int round = 0; round < kHT * kHT; ++round) {  // (a round that promotes nothing ends the loop; each other one promotes a pixel)
    unsigned now = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (!(cand >> q & 1)) continue;
      const int y = py0 + 4 * q;
      const bool strong = st[y - 1][px - 1] == 2 || st[y - 1][px] == 2 || st[y - 1][px + 1] == 2 || st[y][px - 1] == 2 ||
                          st[y][px + 1] == 2 || st[y + 1][px - 1] == 2 || st[y + 1][px] == 2 || st[y + 1][px + 1] == 2;
      now |= (strong ? 1u : 0u) << q;
    }
    __syncthreads();  // every read of this round is done
#pragma unroll
    for (int q = 0; q < 16; ++q)
      if (now >> q & 1) st[py0 + 4 * q][px] = 2;
    cand &= ~now, promoted |= now;
    if (!__syncthreads_or(now != 0)) break;
  }
  if (promoted) {
#pragma unroll
    for (int q = 0; q < 16; ++q)
      if (promoted >> q & 1) plane[(size_t)(y0 + py0 - 1 + 4 * q) * w + (x0 + px - 1)] = 2;  // (a candidate lies in the image)
    *flag = 1u;
  }
}

// ---- step 4 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_dm_edges(const MImg* __restrict__ imgs, const MTile* __restrict__ tiles,
                                                     const unsigned char* __restrict__ cls, int post_blur,
                                                     unsigned char* __restrict__ edges) {
  const int tid = threadIdx.x;
  const MTile t = tiles[blockIdx.x];
  const MImg im = imgs[t.img];
  const int w = (int)im.w, h = (int)im.h;
  const unsigned char* c = cls + im.plane;
  unsigned char* out = edges + im.plane;
#pragma unroll
  for (int q = 0; q < kTW * kTH / kBlock; ++q) {
    const int X = t.tx * kTW + (tid & 63), Y = t.ty * kTH + (tid >> 6) + 4 * q;
    if (X >= w || Y >= h) continue;
    int v;
    if (post_blur) {
      const size_t ya = (size_t)reflect101(Y - 1, h) * w, yb = (size_t)Y * w, yc = (size_t)reflect101(Y + 1, h) * w;
      const int xa = reflect101(X - 1, w), xc = reflect101(X + 1, w);
      const int n = ((c[ya + xa] == 2) + 2 * (c[ya + X] == 2) + (c[ya + xc] == 2)) +
                    2 * ((c[yb + xa] == 2) + 2 * (c[yb + X] == 2) + (c[yb + xc] == 2)) +
                    ((c[yc + xa] == 2) + 2 * (c[yc + X] == 2) + (c[yc + xc] == 2));
      v = (n * 255 + 8) >> 4;
    } else {
      v = c[(size_t)Y * w + X] == 2 ? 255 : 0;
    }
    out[(size_t)Y * w + X] = (unsigned char)v;
  }
}

// ---- step 5: the counts -----------------------------------------------------------------------------------------------------
// A non-zero pixel (row i, column j) votes at 2 j (angle 0), 2 i (angle 2) and rint(float(j * tabCos[n]) + float(i *
// tabSin[n])) for the diagonals n = 1, 3, all relative to (numrho - 1) / 2.  Rows and columns read the diagonal bins 2 i
// and 2 j alone, so an even diagonal bin d is counted at d / 2 and an odd one is not counted.
__global__ __launch_bounds__(kBlock) void k_dm_votes(const MImg* __restrict__ imgs, const MTile* __restrict__ tiles,
                                                     const unsigned char* __restrict__ edges, float tc1, float ts1, float tc3,
                                                     float ts3, unsigned* __restrict__ acc) {
  __shared__ unsigned colc[kTW];
  const int tid = threadIdx.x;
  const MTile t = tiles[blockIdx.x];
  const MImg im = imgs[t.img];
  const int w = (int)im.w, h = (int)im.h;
  if (tid < kTW) colc[tid] = 0;
  __syncthreads();
  const unsigned char* e = edges + im.plane;
  unsigned *rows = acc + im.acc, *cols = rows + h, *d45 = cols + w, *d135 = d45 + max(w, h);
  const int X = t.tx * kTW + (tid & 63);
  unsigned mine = 0;
#pragma unroll
  for (int q = 0; q < kTW * kTH / kBlock; ++q) {
    const int Y = t.ty * kTH + (tid >> 6) + 4 * q;
    const bool nz = X < w && Y < h && e[(size_t)Y * w + X] != 0;
    const unsigned long long b = __ballot(nz);
    if ((tid & 63) == 0 && b) atomicAdd(&rows[Y], (unsigned)__popcll(b));  // (b != 0: the wave's row lies in the image)
    if (nz) {
      ++mine;
      const float fj = (float)X, fi = (float)Y;
      const float a1 = fj * tc1, b1 = fi * ts1, a3 = fj * tc3, b3 = fi * ts3;
      const int r1 = (int)rintf(a1 + b1), r3 = (int)rintf(a3 + b3);
      if (r1 >= 0 && !(r1 & 1) && (r1 >> 1) < max(w, h)) atomicAdd(&d45[r1 >> 1], 1u);
      if (r3 >= 0 && !(r3 & 1) && (r3 >> 1) < h) atomicAdd(&d135[r3 >> 1], 1u);
    }
  }
  if (mine) atomicAdd(&colc[tid & 63], mine);
  __syncthreads();
  if (tid < kTW && colc[tid]) atomicAdd(&cols[t.tx * kTW + tid], colc[tid]);  // (a counted column lies in the image)
}

// ---- the host side: parameters -----------------------------------------------------------------------------------------------
int inval(const char* why) {
  set_last_error_text(why);
  return CBH_E_INVAL;
}
int params_ok(const cbh_demosaic_params* p) {
  if (!p) return inval("demosaic: params is NULL");
  if (!(p->clip_pct >= 0.0f) || !std::isfinite(p->clip_pct)) return inval("demosaic: clip_pct is negative or not finite");
  if (!std::isfinite(p->hough_thresh_factor) || !std::isfinite(p->max_aspect) || !std::isfinite(p->min_aspect))
    return inval("demosaic: a factor or an aspect bound is not finite");
  // a negative crop_margin would put cells outside their image, a spacing below 1 lets selectLines pair a line with itself
  if (p->crop_margin < 0 || p->min_grid_spacing < 1) return inval("demosaic: crop_margin is negative or min_grid_spacing below 1");
  if ((p->pre_blur != 0 && p->pre_blur != 3) || (p->post_blur != 0 && p->post_blur != 3) || p->hough_rho != 0.5f ||
      p->hough_theta != 45.0f) {
    set_last_error_text("demosaic: only blur kernels 0 and 3, hough_rho 0.5 and hough_theta 45 are implemented");
    return CBH_E_UNSUPPORTED;
  }
  return CBH_OK;
}
int tables_ok(size_t n, const uint64_t* off, const uint32_t* w, const uint32_t* h, const uint32_t* stride, int channels,
              bool host, size_t bytes) {
  for (size_t i = 0; i < n; ++i) {
    if (!(w[i] >= 1 && h[i] >= 1 && w[i] <= kMaxSide && h[i] <= kMaxSide && stride[i] >= w[i] * (uint32_t)channels))
      return inval("demosaic: an image has a side of 0 or above 32767, or rows shorter than its pixels");
    if (host && image_end(off[i], w[i], h[i], stride[i], channels) > bytes)
      return inval("demosaic: an image ends outside its buffer");
  }
  return CBH_OK;
}

// ---- steps 6 and 7 ------------------------------------------------------------------------------------------------------------
// selectLines (:1552-1617) as it stands: `cols` bounds the doubled spacing in both directions, and d2 is the distance
// from the grid's last line to lines[prev], which the loop itself keeps at 0
std::vector<int> select_lines(const std::vector<int>& lines, int cols, int min_size, int margin) {
  std::vector<int> max_grid, grid, accepted;
  const int n = (int)lines.size();
  for (int k = 0; k < n - 2; ++k)
    for (int i = k + 1; i < n - 1; ++i) {
      const int grid_size = lines[i] - lines[k];
      if (grid_size < min_size) continue;
      grid.assign({lines[k], lines[i]});
      accepted.clear();
      for (int m = 1; m < 3; ++m) {
        const int s = m * grid_size;
        if (s > cols) break;
        accepted.push_back(s);
      }
      for (int m = 1; m < 3; ++m) {
        const int s = grid_size / m;
        if (s < min_size) break;
        accepted.push_back(s);
      }
      int prev = i, last;
      do {
        last = prev;
        for (int j = prev + 1; j < n; ++j) {
          const int d = lines[j] - lines[prev];
          for (int s : accepted) {
            if (s >= d - margin && s < d + margin) {
              const int d2 = grid.back() - lines[prev];
              if (d2 > 0) {
                if (std::abs(d2 - grid_size) < std::abs(d - grid_size)) continue;
                grid.pop_back();
              }
              grid.push_back(lines[j]);
              prev = j;
              goto find_next_line;
            }
          }
        }
      find_next_line:;
      } while (prev > last);
      if (max_grid.empty() || grid.size() > max_grid.size() ||
          (grid.size() == max_grid.size() && grid.back() - grid.front() > max_grid.back() - max_grid.front()))
        max_grid = grid;
    }
  return max_grid;
}
std::vector<int> grid_of(std::vector<int> lines, int side, int cols, int min_size, int margin) {
  lines.push_back(0);
  lines.push_back(side);
  std::sort(lines.begin(), lines.end());
  return select_lines(lines, cols, min_size, margin);
}
struct Rect {
  int x, y, w, h;
};
void grid_rects(std::vector<int> hg, std::vector<int> vg, int w, int h, int crop, std::vector<Rect>* out) {
  if (hg.empty()) hg = {0, h};
  if (vg.empty()) vg = {0, w};
  if (hg.size() < 3 && vg.size() < 3) {
    out->push_back({0, 0, w, h});
    return;
  }
  int y0 = hg[0];
  for (size_t i = 1; i < hg.size(); ++i) {
    int x0 = vg[0];
    for (size_t j = 1; j < vg.size(); ++j) {
      out->push_back({x0 + crop, y0 + crop, vg[j] - x0 - 2 * crop, hg[i] - y0 - 2 * crop});
      x0 = vg[j];
    }
    y0 = hg[i];
  }
}

// ---- one pass over a list of views: steps 1-5 ----------------------------------------------------------------------------------
struct View {
  uint64_t off;
  uint32_t w, h, stride;
};
struct PassOut {
  void* d_edges = nullptr;            // NULL, or where the edge maps go (packed, view after view)
  void* d_cls = nullptr;              // NULL, or where the class maps before the hysteresis go
  std::vector<std::vector<int>>*hor = nullptr, *ver = nullptr;  // NULL, or the positions per view, ascending
  unsigned passes = 0;                // launches of k_dm_hyst
};

template <int CH>
void launch_class(const uint8_t* src, const MImg* di, const MTile* dt, size_t nt, const int* cuts, const cbh_demosaic_params& p,
                  unsigned char* cls, hipStream_t s) {
  hipLaunchKernelGGL(k_dm_class<CH>, dim3((unsigned)nt), dim3(kBlock), 0, s, src, di, dt, cuts, p.pre_blur,
                     std::min(p.canny1, p.canny2), std::max(p.canny1, p.canny2), cls);
}

int run_pass(const void* d_src, const std::vector<View>& views, int channels, const cbh_demosaic_params& p, float factor,
             PassOut* out, int device, hipStream_t s) {
  const size_t n = views.size();
  if (n == 0) return CBH_OK;
  std::vector<MImg> imgs(n);
  std::vector<MTile> t16, t64;
  std::vector<uint64_t> off(n);
  std::vector<uint32_t> vw(n), vh(n), vs(n);
  uint64_t plane = 0, acc = 0, largest = 0;
  for (size_t i = 0; i < n; ++i) {
    const View& v = views[i];
    imgs[i] = {v.off, plane, acc, v.w, v.h, v.stride, 0};
    off[i] = v.off, vw[i] = v.w, vh[i] = v.h, vs[i] = v.stride;
    plane += (uint64_t)v.w * v.h;
    acc += (uint64_t)v.w + 2ull * v.h + std::max(v.w, v.h);
    largest = std::max<uint64_t>(largest, (uint64_t)v.w * v.h);
    for (unsigned ty = 0; ty < (v.h + kTH - 1) / kTH; ++ty)
      for (unsigned tx = 0; tx < (v.w + kTW - 1) / kTW; ++tx) t16.push_back({(unsigned)i, (unsigned short)tx, (unsigned short)ty});
    for (unsigned ty = 0; ty < (v.h + kHT - 1) / kHT; ++ty)
      for (unsigned tx = 0; tx < (v.w + kHT - 1) / kHT; ++tx) t64.push_back({(unsigned)i, (unsigned short)tx, (unsigned short)ty});
  }
  if (t16.size() > 0x7fffffffu) return inval("demosaic: more than 2^31 tiles in one call");
  Scratch scratch(s);
  MImg* di = nullptr;
  MTile *d16 = nullptr, *d64 = nullptr;
  int* cuts = nullptr;
  unsigned char *cls = nullptr, *edges = (unsigned char*)out->d_edges;
  unsigned *dacc = nullptr, *flag = nullptr;
  const bool votes = out->hor || out->ver;
  hipError_t e = upload(scratch, &di, imgs, s);
  if (e == hipSuccess) e = upload(scratch, &d16, t16, s);
  if (e == hipSuccess) e = upload(scratch, &d64, t64, s);
  if (e == hipSuccess) e = scratch.get(&cuts, n * 2 * sizeof(int));
  if (e == hipSuccess) e = scratch.get(&cls, plane);
  if (e == hipSuccess && !edges) e = scratch.get(&edges, plane);
  if (e == hipSuccess && votes) e = scratch.get(&dacc, acc * sizeof(unsigned));
  if (e == hipSuccess) e = scratch.get(&flag, sizeof(unsigned));
  // (every way out waits for the stream: the host tables above must outlive their copies)
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);
    return fail("demosaic", e);
  }
  // step 1: the cuts (synchronises the stream)
  int rc = cbh_auto_contrast_dev(d_src, n, off.data(), vw.data(), vh.data(), vs.data(), channels, p.clip_pct, nullptr, cuts,
                                 nullptr, device, s);
  if (rc != CBH_OK) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  const uint8_t* src = (const uint8_t*)d_src;
  if (channels == 1) launch_class<1>(src, di, d16, t16.size(), cuts, p, cls, s);
  else if (channels == 3) launch_class<3>(src, di, d16, t16.size(), cuts, p, cls, s);
  else launch_class<4>(src, di, d16, t16.size(), cuts, p, cls, s);
  e = hipGetLastError();
  if (e == hipSuccess && out->d_cls) e = hipMemcpyAsync(out->d_cls, cls, plane, hipMemcpyDeviceToDevice, s);
  // the hysteresis: a launch that sets the flag has promoted at least one pixel, so `largest` + 1 launches always suffice
  for (uint64_t pass = 0; e == hipSuccess && pass <= largest; ++pass) {
    unsigned changed = 0;
    e = hipMemsetAsync(flag, 0, sizeof(unsigned), s);
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(k_dm_hyst, dim3((unsigned)t64.size()), dim3(kBlock), 0, s, di, d64, cls, flag);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&changed, flag, sizeof(unsigned), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    ++out->passes;
    if (!changed) break;
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_dm_edges, dim3((unsigned)t16.size()), dim3(kBlock), 0, s, di, d16, cls, p.post_blur, edges);
    e = hipGetLastError();
  }
  std::vector<unsigned> hacc;
  if (e == hipSuccess && votes) {
    // the tables of cv::HoughLines: theta accumulated in float32, cos and sin in f64, times 1 / rho
    const float theta = (float)((double)p.hough_theta * 3.1415926535897932384626433832795 / 180.0);
    float ang = 0.0f, tc[4], ts[4];
    for (int k = 0; k < 4; ++k) {
      tc[k] = (float)(std::cos((double)ang) * 2.0), ts[k] = (float)(std::sin((double)ang) * 2.0);
      ang = ang + theta;
    }
    hacc.resize(acc);
    e = hipMemsetAsync(dacc, 0, acc * sizeof(unsigned), s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_dm_votes, dim3((unsigned)t16.size()), dim3(kBlock), 0, s, di, d16, edges, tc[1], ts[1], tc[3], ts[3],
                         dacc);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hacc.data(), dacc, acc * sizeof(unsigned), hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail("demosaic", e);
  if (!votes) return CBH_OK;
  // the local-maximum rule at the bins rows and columns land on.  Row i sits at bin r = 2 i + (numrho - 1) / 2 of angle 2:
  // its neighbours r - 1 and r + 1 are never voted for, angle 1 must stay below it and angle 3 must not exceed it.  Column j
  // sits at the same bin of angle 0: there is no angle -1, and angle 1 must not exceed it.
  if (out->hor) out->hor->assign(n, {});
  if (out->ver) out->ver->assign(n, {});
  for (size_t i = 0; i < n; ++i) {
    const int w = (int)views[i].w, h = (int)views[i].h;
    const unsigned *rows = hacc.data() + imgs[i].acc, *cols = rows + h, *d45 = cols + w, *d135 = d45 + std::max(w, h);
    const int numrho = 4 * (w + h) + 2;
    const int th = (int)((float)w * factor), tv = (int)((float)h * factor);
    auto position = [numrho](int k) {
      const int r = 2 * k + (numrho - 1) / 2;
      const float rho = ((float)r - (float)(numrho - 1) * 0.5f) * 0.5f;
      return (int)rho;
    };
    for (int y = 0; y < h && out->hor; ++y) {
      const long long a = rows[y];
      if (a > th && a > 0 && a > (long long)d45[y] && a >= (long long)d135[y]) {
        const int pos = position(y);
        if (pos >= p.h_margin && pos < h - p.h_margin) (*out->hor)[i].push_back(pos);
      }
    }
    for (int x = 0; x < w && out->ver; ++x) {
      const long long a = cols[x];
      if (a > tv && a > 0 && a >= (long long)d45[x]) {
        const int pos = position(x);
        if (pos >= p.v_margin && pos < w - p.v_margin) (*out->ver)[i].push_back(pos);
      }
    }
  }
  return CBH_OK;
}

// ---- step 8: the whole, level by level -------------------------------------------------------------------------------------------
// A node is an image (level 0) or a rectangle that is subdivided: a view of the original pixels.  Its rectangles are
// relative to it; child[k] is the node that replaces rectangle k, or -1.
struct Node {
  size_t img;
  int ax, ay, w, h;
  std::vector<Rect> rects;
  std::vector<long> child;
};
void flatten(const std::vector<Node>& nodes, size_t k, std::vector<Rect>* out) {
  const Node& nd = nodes[k];
  for (size_t r = 0; r < nd.rects.size(); ++r) {
    if (nd.child[r] >= 0) flatten(nodes, (size_t)nd.child[r], out);  // (a subdivision always answers with a rectangle)
    else out->push_back({nd.ax + nd.rects[r].x, nd.ay + nd.rects[r].y, nd.rects[r].w, nd.rects[r].h});
  }
}

int demosaic_all(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                 const uint32_t* img_row_stride, int channels, const cbh_demosaic_params& p, std::vector<std::vector<Rect>>* res,
                 int device, hipStream_t s) {
  std::vector<Node> nodes(n);
  std::vector<size_t> todo(n);
  for (size_t i = 0; i < n; ++i) nodes[i] = {i, 0, 0, (int)img_w[i], (int)img_h[i], {}, {}}, todo[i] = i;
  float factor = p.hough_thresh_factor;
  while (!todo.empty()) {
    std::vector<View> views(todo.size());
    for (size_t k = 0; k < todo.size(); ++k) {
      const Node& nd = nodes[todo[k]];
      views[k] = {img_off[nd.img] + (uint64_t)nd.ay * img_row_stride[nd.img] + (uint64_t)nd.ax * channels, (uint32_t)nd.w,
                  (uint32_t)nd.h, img_row_stride[nd.img]};
    }
    std::vector<std::vector<int>> hor, ver;
    PassOut out;
    out.hor = &hor, out.ver = &ver;
    const int rc = run_pass(d_imgs, views, channels, p, factor, &out, device, s);
    if (rc != CBH_OK) return rc;
    std::vector<size_t> next;
    for (size_t k = 0; k < todo.size(); ++k) {
      const size_t me = todo[k];
      const int w = nodes[me].w, h = nodes[me].h;
      std::vector<Rect> rects;
      grid_rects(grid_of(hor[k], h, w, p.min_grid_spacing, p.grid_tolerance),
                 grid_of(ver[k], w, w, p.min_grid_spacing, p.grid_tolerance), w, h, p.crop_margin, &rects);
      std::vector<long> child(rects.size(), -1);
      for (size_t r = 0; r < rects.size() && rects.size() >= 2; ++r) {
        // a side below 1, or a cell that is not inside its node (the reference would assert or throw), or one that is
        // the whole node (the reference would recurse without end): not subdivided.  Every child is therefore a smaller
        // view inside its parent, which bounds the levels and keeps every view inside the caller's image
        const Rect& c = rects[r];
        if (c.w < 1 || c.h < 1 || c.x < 0 || c.y < 0 || c.x + c.w > w || c.y + c.h > h || (c.w == w && c.h == h)) continue;
        const float aspect = (float)rects[r].w / (float)rects[r].h;
        if (aspect > p.max_aspect || aspect < p.min_aspect) {
          child[r] = (long)nodes.size();
          next.push_back(nodes.size());
          nodes.push_back({nodes[me].img, nodes[me].ax + rects[r].x, nodes[me].ay + rects[r].y, rects[r].w, rects[r].h, {}, {}});
        }
      }
      nodes[me].rects = std::move(rects), nodes[me].child = std::move(child);
    }
    todo = std::move(next);
    factor = 0.95f;  // a subimage has no borders of its own (:1675-1677)
  }
  res->assign(n, {});
  for (size_t i = 0; i < n; ++i) flatten(nodes, i, &(*res)[i]);
  return CBH_OK;
}

int batch_args(size_t n, int channels, const cbh_demosaic_params* p) {
  if (!channels_ok(channels)) return inval("demosaic: the channel count is not 1, 3 or 4");
  if (n > kMaxBatch) return inval("demosaic: more than 2^20 images");
  return params_ok(p);
}

}  // namespace
}  // namespace cbh

extern "C" {

void cbh_demosaic_default_params(cbh_demosaic_params* p) {
  if (!p) return;
  p->clip_pct = 10.0f, p->pre_blur = 3, p->canny1 = 50, p->canny2 = 0, p->post_blur = 3, p->h_margin = 0, p->v_margin = 0;
  p->hough_rho = 0.5f, p->hough_theta = 45.0f, p->hough_thresh_factor = 0.8f;
  p->min_grid_spacing = 96, p->grid_tolerance = 4, p->crop_margin = 2, p->max_aspect = 2.5f, p->min_aspect = 0.5f;
}

int cbh_grid_select(const int32_t* lines, size_t n_lines, int side, int cols, int min_grid_spacing, int grid_tolerance,
                    int32_t* grid, size_t* n_grid) {
  using namespace cbh;
  if ((n_lines && !lines) || !grid || !n_grid || side < 1 || side > (int)kMaxSide || cols < 1 || cols > (int)kMaxSide ||
      n_lines > kMaxSide + 1)
    return CBH_E_INVAL;
  for (size_t i = 0; i < n_lines; ++i)
    if (lines[i] < 0 || lines[i] > side) return CBH_E_INVAL;
  const std::vector<int> g = grid_of(std::vector<int>(lines, lines + n_lines), side, cols, min_grid_spacing, grid_tolerance);
  std::copy(g.begin(), g.end(), grid);
  *n_grid = g.size();
  return CBH_OK;
}

int cbh_grid_rects(const int32_t* hgrid, size_t n_h, const int32_t* vgrid, size_t n_v, int w, int h, int crop_margin,
                   int32_t* rects, size_t rects_cap, size_t* n_rects) {
  using namespace cbh;
  if ((n_h && !hgrid) || (n_v && !vgrid) || !n_rects || w < 1 || h < 1 || w > (int)kMaxSide || h > (int)kMaxSide ||
      n_h > kMaxSide + 2 || n_v > kMaxSide + 2 || (rects_cap && !rects))
    return CBH_E_INVAL;
  std::vector<Rect> r;
  grid_rects(std::vector<int>(hgrid, hgrid + n_h), std::vector<int>(vgrid, vgrid + n_v), w, h, crop_margin, &r);
  *n_rects = r.size();
  if (r.size() > rects_cap) return CBH_E_OVERFLOW;
  for (size_t k = 0; k < r.size(); ++k) rects[4 * k] = r[k].x, rects[4 * k + 1] = r[k].y, rects[4 * k + 2] = r[k].w, rects[4 * k + 3] = r[k].h;
  return CBH_OK;
}

int cbh_edge_maps_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                      const uint32_t* img_row_stride, int channels, const cbh_demosaic_params* params, void* d_edges,
                      void* d_classes, uint32_t* passes, int device, void* stream) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  int rc = batch_args(n, channels, params);
  if (rc != CBH_OK) return rc;
  if (passes) *passes = 0;
  if (n == 0) return CBH_OK;
  if (!d_imgs || !img_off || !img_w || !img_h || !img_row_stride || !d_edges) return inval("edge maps: a required pointer is NULL");
  if ((rc = tables_ok(n, img_off, img_w, img_h, img_row_stride, channels, false, 0)) != CBH_OK) return rc;
  std::vector<View> views(n);
  for (size_t i = 0; i < n; ++i) views[i] = {img_off[i], img_w[i], img_h[i], img_row_stride[i]};
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  PassOut out;
  out.d_edges = d_edges, out.d_cls = d_classes;
  rc = run_pass(d_imgs, views, channels, *params, params->hough_thresh_factor, &out, device, (hipStream_t)stream);
  if (passes) *passes = out.passes;
  return rc;
}

int cbh_grid_lines_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                       const uint32_t* img_row_stride, int channels, const cbh_demosaic_params* params, int32_t* hor,
                       uint32_t* hor_first, int32_t* ver, uint32_t* ver_first, int device, void* stream) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  int rc = batch_args(n, channels, params);
  if (rc != CBH_OK) return rc;
  if (!hor_first || !ver_first) return inval("grid lines: a required pointer is NULL");
  hor_first[0] = ver_first[0] = 0;
  if (n == 0) return CBH_OK;
  if (!d_imgs || !img_off || !img_w || !img_h || !img_row_stride || !hor || !ver) return inval("grid lines: a required pointer is NULL");
  if ((rc = tables_ok(n, img_off, img_w, img_h, img_row_stride, channels, false, 0)) != CBH_OK) return rc;
  std::vector<View> views(n);
  for (size_t i = 0; i < n; ++i) views[i] = {img_off[i], img_w[i], img_h[i], img_row_stride[i]};
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  std::vector<std::vector<int>> h, v;
  PassOut out;
  out.hor = &h, out.ver = &v;
  rc = run_pass(d_imgs, views, channels, *params, params->hough_thresh_factor, &out, device, (hipStream_t)stream);
  if (rc != CBH_OK) return rc;
  for (size_t i = 0; i < n; ++i) {
    std::copy(h[i].begin(), h[i].end(), hor + hor_first[i]);
    std::copy(v[i].begin(), v[i].end(), ver + ver_first[i]);
    hor_first[i + 1] = hor_first[i] + (uint32_t)h[i].size(), ver_first[i + 1] = ver_first[i] + (uint32_t)v[i].size();
  }
  return CBH_OK;
}

int cbh_demosaic_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                     const uint32_t* img_row_stride, int channels, const cbh_demosaic_params* params, int32_t* rects,
                     size_t rects_cap, uint32_t* rect_first, int device, void* stream) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  int rc = batch_args(n, channels, params);
  if (rc != CBH_OK) return rc;
  if (!rect_first) return inval("demosaic: rect_first is NULL");
  rect_first[0] = 0;
  if (n == 0) return CBH_OK;
  if (!d_imgs || !img_off || !img_w || !img_h || !img_row_stride || (rects_cap && !rects))
    return inval("demosaic: a required pointer is NULL");
  if ((rc = tables_ok(n, img_off, img_w, img_h, img_row_stride, channels, false, 0)) != CBH_OK) return rc;
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  std::vector<std::vector<Rect>> res;
  rc = demosaic_all(d_imgs, n, img_off, img_w, img_h, img_row_stride, channels, *params, &res, device, (hipStream_t)stream);
  if (rc != CBH_OK) return rc;
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) total += res[i].size();
  if (total > 0xffffffffull) return inval("demosaic: more than 2^32 rectangles");
  for (size_t i = 0; i < n; ++i) rect_first[i + 1] = rect_first[i] + (uint32_t)res[i].size();
  if (total > rects_cap) {
    set_last_error_text("demosaic: rects_cap is below rect_first[n]");
    return CBH_E_OVERFLOW;
  }
  for (size_t i = 0; i < n; ++i)
    for (size_t k = 0; k < res[i].size(); ++k) {
      int32_t* q = rects + 4 * ((size_t)rect_first[i] + k);
      q[0] = res[i][k].x, q[1] = res[i][k].y, q[2] = res[i][k].w, q[3] = res[i][k].h;
    }
  return CBH_OK;
}

int cbh_demosaic(const uint8_t* imgs, size_t imgs_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                 const uint32_t* img_h, const uint32_t* img_row_stride, int channels, const cbh_demosaic_params* params,
                 int32_t* rects, size_t rects_cap, uint32_t* rect_first, int device) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  int rc = batch_args(n, channels, params);
  if (rc != CBH_OK) return rc;
  if (!rect_first) return inval("demosaic: rect_first is NULL");
  rect_first[0] = 0;
  if (n == 0) return CBH_OK;
  if (!imgs || !img_off || !img_w || !img_h || !img_row_stride || (rects_cap && !rects))
    return inval("demosaic: a required pointer is NULL");
  if ((rc = tables_ok(n, img_off, img_w, img_h, img_row_stride, channels, true, imgs_bytes)) != CBH_OK) return rc;
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  Staging st("demosaic");
  uint8_t* d_imgs;
  st.alloc(&d_imgs, imgs_bytes);
  st.up(d_imgs, imgs, imgs_bytes);
  rc = st.status();
  if (rc != CBH_OK) return rc;
  return cbh_demosaic_dev(d_imgs, n, img_off, img_w, img_h, img_row_stride, channels, params, rects, rects_cap, rect_first,
                          device, st.s);
}

}  // extern "C"
