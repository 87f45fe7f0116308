// tmatch.hip -- the steps of TemplateMatcher::match between its descriptor match and its score
// (src/templatematcher.cpp:264-333) for a batch of candidates of one template, without leaving the device:
//   estimateRigidTransform(tmplPoints, matchPoints, false) twice (:264, :309), cv::transform of the template's corners and
//   the roi (:284-300), invertAffineTransform + warpAffine(INTER_AREA, BORDER_CONSTANT, (0,0,0,255)) (:331-333);
//   cbh_template_match_dev then hands the patches to cbh_template_hashes_dev (prestage.hip, :334-372) and takes hamm64.
//
// UNPINNED.  OpenCV is not available to this repository: what follows restates estimateRigidTransform / getRTMatrix /
// invertAffineTransform / warpAffine / remap's bilinear fixed-point path as recalled from OpenCV 2.4.13, and stays unpinned
// until tools/pin_with_opencv.sh has written tests/golden/opencv_tmatch.npz.  This file is the ONE place of the
// restatement on the device side (tests/template_match_rules.py is the one on the test side); the eigen-solver behind
// DECOMP_EIG is this project's own cyclic Jacobi (jacobi_solve below), which differs from OpenCV's in sweep order only.
//
//   k_ransac      one wave per point-pair list (a candidate is two lists: the points as they are and divided by
//                 candScale).  The RNG, the draws, the three-point fit and the 4 x 4 solve are wave-uniform (every lane
//                 computes the same doubles); the inlier test is lane-parallel, 64 points per step; the sums of the final fit
//                 run over the good pairs in ascending order: ballot + prefix popcount compacts a step's terms into LDS,
//                 lanes 0..6 add one accumulator each, entry by entry.  Lists of up to kLdsPoints pairs are drawn from an LDS
//                 copy (a degenerate list makes 250 000 dependent draws), longer ones from global memory.
//   k_tm_prepare  one lane per candidate: both inversions, the 2^30 domain check, the corners and the roi
//   k_warp<CH>    one lane per four consecutive output pixels of the packed patches (flat over the whole batch, so every
//                 lane's store is one aligned 4 * CH byte vector store and a wave writes 256 * CH contiguous bytes); the
//                 coordinate integers adelta / bdelta are recomputed per pixel in double, X0 / Y0 per lane and row, four taps
//                 of CH bytes are gathered.  Gather-bound: a wave's taps follow a line through the candidate image.
// The grouped chain's tail (template_match_pairs_tail, a template per candidate) launches the same kernels and, for the
// warp and the mask, tmpairs.hip's ragged forms; warp_px.h holds the pixel both warps share.
// The file is built with -ffp-contract=off (Makefile): every float / double operation rounds once, as in the model.
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#include <algorithm>
#include <vector>

#include "cbh_index.h"
#include "cbh_runs.h"
#include "cbh_staging.h"
#include "warp_px.h"

namespace cbh {
namespace {

constexpr int kRansacIters = 500;   // RANSAC_MAX_ITERS, outer and inner
constexpr int kLdsPoints = 2048;    // most pairs of one list kept in LDS (32 KB); a launch reserves what its lists need
constexpr int kWarpBlock = 256;
constexpr double kDomain = 1073741824.0 - 64.0;  // the coordinate integers stay below 2^30

int g_tmatch_chunk_mb = 1024;  // "tmatch_chunk_mb"

struct RProblem {
  unsigned long long first;  // first pair of the list in a_xy / b_xy
  unsigned count;
  float b_div;               // B is divided by this in float (1: as it is; x / 1.0f == x)
};

// ---- getRTMatrix(fullAffine = false): x = V diag(1 / lambda) V^T b by cyclic Jacobi ---------------------------------
// s = { sa00, sa02, sa03, sb0, sb1, sb2, sb3 }, n = pairs; out = { m0, -m1, m2, m1, m0, m3 }
__device__ __forceinline__ void jacobi_solve(const double (&s)[7], double n, double (&out)[6]) {
  double a[4][4] = {{s[0], 0.0, s[1], s[2]}, {0.0, s[0], -s[2], s[1]}, {s[1], -s[2], n, 0.0}, {s[2], s[1], 0.0, n}};
  double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  const double b[4] = {s[3], s[4], s[5], s[6]};
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = a[p][q], g = fabs(apq);
        if (g == 0.0) continue;
        if (fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[q][q]) + g == fabs(a[q][q])) {
          a[p][q] = a[q][p] = 0.0;
          continue;
        }
        rotated = true;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        a[p][p] = a[p][p] - t * apq;
        a[q][q] = a[q][q] + t * apq;
        a[p][q] = a[q][p] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k != p && k != q) {
            const double akp = a[k][p], akq = a[k][q];
            a[k][p] = a[p][k] = c * akp - sn * akq;
            a[k][q] = a[q][k] = sn * akp + c * akq;
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - sn * vkq;
          v[k][q] = sn * vkp + c * vkq;
        }
      }
    }
    if (!rotated) break;
  }
  const double cut = 2.0 * DBL_EPSILON * (((fabs(a[0][0]) + fabs(a[1][1])) + fabs(a[2][2])) + fabs(a[3][3]));
  double y[4], x[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double d = ((v[0][j] * b[0] + v[1][j] * b[1]) + v[2][j] * b[2]) + v[3][j] * b[3];
    y[j] = d * (a[j][j] <= cut ? 0.0 : 1.0 / a[j][j]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = ((v[i][0] * y[0] + v[i][1] * y[1]) + v[i][2] * y[2]) + v[i][3] * y[3];
  out[0] = x[0], out[1] = -x[1], out[2] = x[2], out[3] = x[1], out[4] = x[0], out[5] = x[3];
}

// the seven terms of the flagged lanes' pairs go to LDS in lane order; lanes 0..6 add one accumulator each in that order
__device__ __forceinline__ void add_terms(double (*sT)[64], bool flag, float2 a, float2 b, double& acc, int lane) {
  const unsigned long long mask = __ballot(flag);
  const int pos = __popcll(mask & ((1ull << lane) - 1ull)), cnt = __popcll(mask);
  if (flag) {
    // products and their two-term sums in float, then widened
    const float t0 = a.x * a.x + a.y * a.y, t3 = a.x * b.x + a.y * b.y, t4 = a.x * b.y - a.y * b.x;
    sT[0][pos] = (double)t0, sT[1][pos] = (double)a.x, sT[2][pos] = (double)a.y, sT[3][pos] = (double)t3;
    sT[4][pos] = (double)t4, sT[5][pos] = (double)b.x, sT[6][pos] = (double)b.y;
  }
  __syncthreads();
  if (lane < 7)
    for (int j = 0; j < cnt; ++j) acc += sT[lane][j];
  __syncthreads();
}

__device__ __forceinline__ void solve_from_acc(double acc, double n, double (&m)[6]) {
  double s[7];
#pragma unroll
  for (int t = 0; t < 7; ++t) s[t] = __shfl(acc, t);
  jacobi_solve(s, n, m);
}

__device__ __forceinline__ bool near_collinear(float2 p0, float2 p1, float2 p2) {
  const double dx1 = (double)(p1.x - p0.x), dy1 = (double)(p1.y - p0.y);  // differences in float, the rest in double
  const double dx2 = (double)(p2.x - p0.x), dy2 = (double)(p2.y - p0.y);
  return fabs(dx1 * dy2 - dy1 * dx2) < 0.01 * sqrt(dx1 * dx1 + dy1 * dy1) * sqrt(dx2 * dx2 + dy2 * dy2);
}

struct Points {
  const float2 *ga, *gb;  // the list in global memory
  const float2* lds;      // its LDS copy: the A points, then from lds_points the B points (already divided)
  unsigned lds_points;
  bool cached;
  float div;
  __device__ __forceinline__ float2 a(unsigned i) const { return cached ? lds[i] : ga[i]; }
  __device__ __forceinline__ float2 b(unsigned i) const {
    if (cached) return lds[lds_points + i];
    const float2 p = gb[i];
    return make_float2(p.x / div, p.y / div);
  }
};

struct Draw {
  unsigned long long state;
  unsigned draws;
  __device__ __forceinline__ unsigned next() {
    state = (unsigned long long)(unsigned)state * 4164903690ull + (state >> 32);
    ++draws;
    return (unsigned)state;
  }
};

// draw number I of an outer iteration: up to kRansacIters tries; false when they run out
template <int I>
__device__ __forceinline__ bool draw_point(const Points& P, unsigned count, Draw& rng, unsigned (&idx)[3], float2 (&pa)[3],
                                           float2 (&pb)[3]) {
  for (int k1 = 0; k1 < kRansacIters; ++k1) {
    const unsigned id = rng.next() % count;
    const float2 qa = P.a(id), qb = P.b(id);
    bool bad = false;
#pragma unroll
    for (int j = 0; j < I; ++j)
      bad = bad || idx[j] == id || fabsf(qa.x - pa[j].x) + fabsf(qa.y - pa[j].y) < FLT_EPSILON ||
            fabsf(qb.x - pb[j].x) + fabsf(qb.y - pb[j].y) < FLT_EPSILON;
    if (bad) continue;
    if (I == 2 && (near_collinear(pa[0], pa[1], qa) || near_collinear(pb[0], pb[1], qb))) continue;
    idx[I] = id, pa[I] = qa, pb[I] = qb;
    return true;
  }
  return false;
}

__device__ __forceinline__ bool is_good(const double (&m)[6], float2 a, float2 b, double thr) {
  const double ax = a.x, ay = a.y, bx = b.x, by = b.y;
  return fabs(m[0] * ax + m[1] * ay + m[2] - bx) + fabs(m[3] * ax + m[4] * ay + m[5] - by) < thr;
}

__global__ __launch_bounds__(64) void k_ransac(const float2* __restrict__ a_xy, const float2* __restrict__ b_xy,
                                               const RProblem* __restrict__ probs, double* __restrict__ m_out,
                                               unsigned char* __restrict__ found_out, cbh_rigid_detail* __restrict__ detail,
                                               unsigned lds_points) {
  extern __shared__ float2 s_points[];  // 2 * lds_points: the A points, then the B points, of a list that fits
  float2 *const sA = s_points, *const sB = s_points + lds_points;
  __shared__ double sT[7][64];
  const int lane = (int)threadIdx.x;
  const RProblem pr = probs[blockIdx.x];
  const unsigned count = pr.count;
  Points P{a_xy + pr.first, b_xy + pr.first, s_points, lds_points, count <= lds_points, pr.b_div};
  double m[6] = {0, 0, 0, 0, 0, 0};
  int found = 0, iterations = 0, good_count = 0;
  Draw rng{0xFFFFFFFFFFFFFFFFull, 0u};  // cv::RNG rng((uint64)-1), fresh per call
  if (count >= 3) {
    // boundingRect(B) for float points: floor of the extremes, width = x1 - x0 + 1
    float lox = INFINITY, loy = INFINITY, hix = -INFINITY, hiy = -INFINITY;
    for (unsigned i = lane; i < count; i += 64) {
      const float2 pa = P.ga[i], g = P.gb[i], pb = make_float2(g.x / pr.b_div, g.y / pr.b_div);
      if (P.cached) sA[i] = pa, sB[i] = pb;
      lox = fminf(lox, pb.x), hix = fmaxf(hix, pb.x), loy = fminf(loy, pb.y), hiy = fmaxf(hiy, pb.y);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      lox = fminf(lox, __shfl_xor(lox, d)), hix = fmaxf(hix, __shfl_xor(hix, d));
      loy = fminf(loy, __shfl_xor(loy, d)), hiy = fmaxf(hiy, __shfl_xor(hiy, d));
    }
    __syncthreads();
    const double bw = (double)floorf(hix) - (double)floorf(lox) + 1.0, bh = (double)floorf(hiy) - (double)floorf(loy) + 1.0;
    const double thr = fmax(bw, bh) * 0.05, half = (double)count * 0.5;
    while (iterations < kRansacIters) {
      ++iterations;
      unsigned idx[3] = {0, 0, 0};
      float2 pa[3], pb[3];
      pa[0] = pa[1] = pa[2] = pb[0] = pb[1] = pb[2] = make_float2(0.f, 0.f);
      if (!draw_point<0>(P, count, rng, idx, pa, pb)) continue;
      if (!draw_point<1>(P, count, rng, idx, pa, pb)) continue;
      if (!draw_point<2>(P, count, rng, idx, pa, pb)) continue;
      double acc = 0.0;
      // lane l < 3 takes pair l (selected by value: a selected address would keep the arrays in scratch memory)
      const float2 a0 = pa[0], a1 = pa[1], a2 = pa[2], b0 = pb[0], b1 = pb[1], b2 = pb[2];
      const float2 la = make_float2(lane == 0 ? a0.x : lane == 1 ? a1.x : a2.x, lane == 0 ? a0.y : lane == 1 ? a1.y : a2.y);
      const float2 lb = make_float2(lane == 0 ? b0.x : lane == 1 ? b1.x : b2.x, lane == 0 ? b0.y : lane == 1 ? b1.y : b2.y);
      add_terms(sT, lane < 3, la, lb, acc, lane);
      solve_from_acc(acc, 3.0, m);
      unsigned good = 0;
      for (unsigned base = 0; base < count; base += 64) {
        const unsigned i = base + lane;
        const bool in = i < count;
        const unsigned ii = in ? i : 0u;
        good += (unsigned)__popcll(__ballot(in && is_good(m, P.a(ii), P.b(ii), thr)));
      }
      if ((double)good >= half) {
        // the final fit over the good pairs, in ascending order
        acc = 0.0;
        for (unsigned base = 0; base < count; base += 64) {
          const unsigned i = base + lane;
          const bool in = i < count;
          const unsigned ii = in ? i : 0u;
          const float2 qa = P.a(ii), qb = P.b(ii);
          add_terms(sT, in && is_good(m, qa, qb, thr), qa, qb, acc, lane);
        }
        solve_from_acc(acc, (double)good, m);
        found = 1, good_count = (int)good;
        break;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) m_out[(size_t)blockIdx.x * 6 + k] = found ? m[k] : 0.0;
    found_out[blockIdx.x] = (unsigned char)found;
    if (detail) {
      cbh_rigid_detail d;
      d.iterations = iterations, d.good_count = good_count, d.draws = rng.draws, d.reserved = 0;
      detail[blockIdx.x] = d;
    }
  }
}

// ---- invertAffineTransform, warpAffine's own inversion, the domain, the corners and the roi ---------------------------
// m / found: entry i * m_step of the estimate arrays (the chain keeps two estimates per candidate)
__global__ __launch_bounds__(64) void k_tm_prepare(const double* __restrict__ m_in, const unsigned char* __restrict__ found,
                                                   unsigned m_step, unsigned n, int tw, int th,
                                                   const float* __restrict__ scale, double* __restrict__ wm,
                                                   unsigned char* __restrict__ ok, int* __restrict__ roi,
                                                   const PPatch* __restrict__ ragged) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (ragged) tw = (int)ragged[i].tw, th = (int)ragged[i].th;  // the grouped chain: every candidate has its own template
  const double* M = m_in + (size_t)i * m_step * 6;
  double w[6] = {0, 0, 0, 0, 0, 0};
  bool good = found[(size_t)i * m_step] != 0;
  if (good) {
    // invertAffineTransform
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1.0 / D : 0.0;
    const double A11 = M[4] * D, A22 = M[0] * D, A12 = -M[1] * D, A21 = -M[3] * D;
    const double b1 = -A11 * M[2] - A12 * M[5], b2 = -A21 * M[2] - A22 * M[5];
    // warpAffine without WARP_INVERSE_MAP inverts again, in its own form
    double E = A11 * A22 - A12 * A21;
    E = E != 0 ? 1.0 / E : 0.0;
    w[0] = A22 * E, w[4] = A11 * E, w[1] = A12 * -E, w[3] = A21 * -E;
    w[2] = -w[0] * b1 - w[1] * b2, w[5] = -w[3] * b1 - w[4] * b2;
    // where the coordinate integers would reach 2^30 the reference is undefined: no transform (NaN fails too)
#pragma unroll
    for (int r = 0; r < 6; r += 3) {
      const double ax = fabs(w[r] * (double)(tw - 1) * 1024.0);
      const double bx = fmax(fabs(w[r + 2] * 1024.0), fabs((w[r + 1] * (double)(th - 1) + w[r + 2]) * 1024.0));
      if (!(ax + bx < kDomain)) good = false;
    }
  }
  ok[i] = good ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) wm[(size_t)i * 6 + k] = good ? w[k] : 0.0;
  if (roi) {
    // cv::transform of (0,0) (w,0) (w,h) (0,h) with the matrix converted to float; int(x / candScale), float division
    const float sc = scale ? scale[i] : 1.f;
    float mf[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) mf[k] = (float)M[k];
    const float cx[4] = {0.f, (float)tw, (float)tw, 0.f}, cy[4] = {0.f, 0.f, (float)th, (float)th};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float qx = (cx[c] * mf[0] + cy[c] * mf[1] + mf[2]) / sc, qy = (cx[c] * mf[3] + cy[c] * mf[4] + mf[5]) / sc;
      roi[(size_t)i * 8 + 2 * c] = good ? (int)qx : 0;
      roi[(size_t)i * 8 + 2 * c + 1] = good ? (int)qy : 0;
    }
  }
}

// out: packed patches of candidates i0 .. (flat bytes, 4 * CH per lane); total = pixels of this launch
template <int CH>
__global__ __launch_bounds__(kWarpBlock) void k_warp(const unsigned char* __restrict__ imgs, const WImage* __restrict__ images,
                                                     const double* __restrict__ wm, const unsigned char* __restrict__ ok,
                                                     unsigned tw, unsigned th, unsigned long long total,
                                                     unsigned char* __restrict__ out) {
  const unsigned long long p0 = ((unsigned long long)blockIdx.x * kWarpBlock + threadIdx.x) * 4ull;
  if (p0 >= total) return;
  const unsigned npx = tw * th;
  unsigned img, r;
  if (total <= 0xffffffffull) {  // (every launch of queue_warp but a 2^32-pixel one: a 32-bit division)
    img = (unsigned)p0 / npx, r = (unsigned)p0 % npx;
  } else {
    img = (unsigned)(p0 / npx), r = (unsigned)(p0 % npx);
  }
  unsigned y = r / tw, x = r % tw;
  unsigned words[CH] = {};
  const int live = (int)min(4ull, total - p0);
  int X0, Y0;  // of the row the lane is in: once per lane, and again where its four pixels cross into the next row
  row_start(wm + (size_t)img * 6, (int)y, X0, Y0);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < live) {
      unsigned px[CH] = {};
      if (ok[img]) warp_pixel<CH>(imgs, images[img], wm + (size_t)img * 6, (int)x, X0, Y0, px);
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int b = k * CH + c;
        words[b >> 2] |= px[c] << (8 * (b & 3));
      }
      if (++x == tw) {
        x = 0;
        if (++y == th) y = 0, ++img;
        if (k + 1 < live) row_start(wm + (size_t)img * 6, (int)y, X0, Y0);
      }
    }
  }
  unsigned char* dst = out + p0 * CH;
  if (live == 4) {
    if constexpr (CH == 4) {
      *reinterpret_cast<uint4*>(dst) = make_uint4(words[0], words[1], words[2], words[3]);
    } else {
#pragma unroll
      for (int c = 0; c < CH; ++c) reinterpret_cast<unsigned*>(dst)[c] = words[c];
    }
  } else {
    for (int b = 0; b < live * CH; ++b) dst[b] = (unsigned char)(words[b >> 2] >> (8 * (b & 3)));
  }
}

// one lane per candidate: the result record of the chain
__global__ __launch_bounds__(64) void k_tm_finish(const double* __restrict__ m, const unsigned char* __restrict__ found,
                                                  const cbh_rigid_detail* __restrict__ detail,
                                                  const unsigned char* __restrict__ ok, const int* __restrict__ roi,
                                                  const unsigned long long* __restrict__ cand_hash,
                                                  const unsigned long long* __restrict__ tmpl_hash, unsigned n,
                                                  cbh_template_result* __restrict__ out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cbh_template_result r = {};
  r.iterations = detail[2 * i].iterations, r.good_count = detail[2 * i].good_count;
  r.score = INT_MAX;  // :233, :258, :271
  if (ok[i]) {
    r.found = 1, r.tx_found = found[2 * i + 1];
#pragma unroll
    for (int k = 0; k < 6; ++k) r.m[k] = m[(size_t)i * 12 + k], r.tx[k] = m[(size_t)i * 12 + 6 + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) r.roi[k] = roi[(size_t)i * 8 + k];
    r.cand_hash = cand_hash[i], r.tmpl_hash = tmpl_hash[i];
    r.score = __popcll(r.cand_hash ^ r.tmpl_hash);
  }
  out[i] = r;
}

bool lists_ok(const uint64_t* first, size_t n) {
  if (first[0] != 0) return false;
  for (size_t i = 0; i < n; ++i)
    if (first[i + 1] < first[i] || first[i + 1] - first[i] > 0x7fffffffull) return false;
  return first[n] < (1ull << 40);
}

// queues the RANSAC of `np` lists: list j = pairs first[j / per] .. first[j / per + 1], `per` lists per entry of first (the
// chain: 2, the second with B divided by scale[j / 2]).  The table is host memory: the caller synchronises.
int queue_ransac(Scratch& scratch, std::vector<RProblem>& probs, const float* d_a, const float* d_b, const uint64_t* first,
                 size_t n, int per, const float* scale, double* d_m, unsigned char* d_found, cbh_rigid_detail* d_detail,
                 hipStream_t s) {
  probs.resize(n * per);
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < per; ++k)
      probs[i * per + k] = {first[i], (unsigned)(first[i + 1] - first[i]), k ? scale[i] : 1.f};
  RProblem* d_probs = nullptr;
  const hipError_t e = upload(scratch, &d_probs, probs, s);
  if (e != hipSuccess) return fail("rigid transform tables", e);
  // LDS for the longest list of the launch, up to kLdsPoints pairs (a 100-pair batch keeps its occupancy); longer lists
  // are drawn from global memory
  unsigned lds_points = 1;
  for (const RProblem& p : probs) lds_points = std::max(lds_points, std::min(p.count, (unsigned)kLdsPoints));
  hipLaunchKernelGGL(k_ransac, dim3((unsigned)probs.size()), dim3(64), 2 * lds_points * sizeof(float2), s, (const float2*)d_a,
                     (const float2*)d_b, d_probs, d_m, d_found, d_detail, lds_points);
  return CBH_OK;
}

// queues k_tm_prepare's products -> the patches of n candidates; images is host memory: the caller synchronises
int queue_warp(Scratch& scratch, std::vector<WImage>& images, const uint8_t* d_imgs, size_t n, const uint64_t* img_off,
               const uint32_t* img_w, const uint32_t* img_h, const uint32_t* img_row_stride, int channels,
               const double* d_wm, const unsigned char* d_ok, int tw, int th, uint8_t* d_patches, hipStream_t s) {
  images.resize(n);
  for (size_t i = 0; i < n; ++i) images[i] = {img_off[i], img_w[i], img_h[i], img_row_stride[i], 0u};
  WImage* d_images = nullptr;
  const hipError_t e = upload(scratch, &d_images, images, s);
  if (e != hipSuccess) return fail("warp tables", e);
  const size_t npx = (size_t)tw * th;
  // launches of at most 2^32 pixels, a multiple of four candidates each (the stores stay aligned)
  const size_t per = std::max<size_t>(4, (((size_t)1 << 32) / npx) & ~(size_t)3);
  for (size_t i0 = 0; i0 < n; i0 += per) {
    const size_t m = std::min(per, n - i0);
    const unsigned long long total = (unsigned long long)m * npx;
    const unsigned blocks = (unsigned)((total + 4ull * kWarpBlock - 1) / (4ull * kWarpBlock));
    uint8_t* out = d_patches + i0 * npx * channels;
#define CBH_WARP(CH)                                                                                                    \
  hipLaunchKernelGGL(k_warp<CH>, dim3(blocks), dim3(kWarpBlock), 0, s, d_imgs, d_images + i0, d_wm + i0 * 6, d_ok + i0, \
                     (unsigned)tw, (unsigned)th, total, out)
    if (channels == 1)
      CBH_WARP(1);
    else if (channels == 3)
      CBH_WARP(3);
    else
      CBH_WARP(4);
#undef CBH_WARP
  }
  return CBH_OK;
}

size_t tmatch_budget() { return (size_t)std::max(g_tmatch_chunk_mb, 1) << 20; }

// the ragged warp of n candidates; images / patches are host memory: the caller synchronises
int queue_warp_ragged(Scratch& scratch, std::vector<WImage>& images, const std::vector<PPatch>& patches,
                      const PPatch* d_patches_tab, const uint8_t* d_imgs, const uint64_t* img_off, const uint32_t* img_w,
                      const uint32_t* img_h, const uint32_t* img_row_stride, int channels, const double* d_wm,
                      const unsigned char* d_ok, uint8_t* d_out, hipStream_t s) {
  const size_t n = patches.size();
  images.resize(n);
  for (size_t i = 0; i < n; ++i) images[i] = {img_off[i], img_w[i], img_h[i], img_row_stride[i], 0u};
  WImage* d_images = nullptr;
  const hipError_t e = upload(scratch, &d_images, images, s);
  if (e != hipSuccess) return fail("warp tables", e);
  for (size_t i0 = 0; i0 < n; i0 += 65535) {
    const size_t m = std::min<size_t>(65535, n - i0);
    unsigned long long most = 1;
    for (size_t i = i0; i < i0 + m; ++i) most = std::max(most, (unsigned long long)patches[i].tw * patches[i].th);
    const dim3 grid((unsigned)std::min<unsigned long long>((most + 4 * kWarpBlock - 1) / (4 * kWarpBlock), 4096), (unsigned)m);
    launch_warp_ragged(channels, grid, s, d_imgs, d_images + i0, d_wm + i0 * 6, d_ok + i0, d_patches_tab + i0, d_out);
  }
  return CBH_OK;
}

}  // namespace

// cbh_template_match_dev for candidates that each have a template of their own (tmimages.hip's grouped chain): candidate i
// is matched against the tg[i].tw x tg[i].th template at d_tmpl_base + tg[i].off.  One RANSAC launch, one prepare, one
// ragged warp and one ragged mask for all of them; the hashes keep their per-geometry launch plan -- one launch_dcthash
// pair per run of consecutive candidates with the same template size, queued back to back (launch_dcthash takes arena
// scratch per call but neither synchronises nor reaches the driver once a geometry's tables exist).  res is host memory
// and complete on return: the one wait of this function.
int template_match_pairs_tail(const uint8_t* d_tmpl_base, const TmplGeom* tg, const uint8_t* d_imgs, size_t n,
                              const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                              const uint32_t* img_row_stride, int channels, const float* d_tmpl_xy, const float* d_match_xy,
                              const uint64_t* first, const float* cand_scale, cbh_template_result* res, unsigned* hash_launches,
                              hipStream_t s) {
  if (n == 0) return CBH_OK;
  if (!lists_ok(first, n)) return CBH_E_INVAL;
  std::vector<PPatch> patches(n);
  size_t patch_bytes = 0, gray_bytes = 0;
  for (size_t i = 0; i < n; ++i) {
    patches[i] = {patch_bytes, tg[i].off, gray_bytes, tg[i].tw, tg[i].th, tg[i].stride, 0u};
    patch_bytes += ((size_t)tg[i].tw * tg[i].th * channels + 15) & ~(size_t)15;
    gray_bytes += (size_t)tg[i].tw * tg[i].th;  // (packed: a run of one size is what launch_dcthash takes)
  }
  Scratch scratch(s), tables(s);
  std::vector<RProblem> probs;
  std::vector<WImage> images;
  double *d_m = nullptr, *d_wm = nullptr;
  unsigned char *d_found = nullptr, *d_ok = nullptr, *d_gray = nullptr;
  cbh_rigid_detail* d_detail = nullptr;
  int* d_roi = nullptr;
  float* d_scale = nullptr;
  unsigned long long* d_hash = nullptr;
  uint8_t* d_p = nullptr;
  cbh_template_result* d_res = nullptr;
  PPatch* d_tab = nullptr;
  hipError_t e = scratch.get(&d_m, n * 12 * sizeof(double));
  if (e == hipSuccess) e = scratch.get(&d_wm, n * 6 * sizeof(double));
  if (e == hipSuccess) e = scratch.get(&d_found, n * 2);
  if (e == hipSuccess) e = scratch.get(&d_ok, n);
  if (e == hipSuccess) e = scratch.get(&d_detail, n * 2 * sizeof(cbh_rigid_detail));
  if (e == hipSuccess) e = scratch.get(&d_roi, n * 8 * sizeof(int));
  if (e == hipSuccess) e = scratch.get(&d_hash, n * 2 * sizeof(unsigned long long));
  if (e == hipSuccess) e = scratch.get(&d_p, patch_bytes);
  if (e == hipSuccess) e = scratch.get(&d_gray, 2 * gray_bytes);
  if (e == hipSuccess) e = scratch.get(&d_res, n * sizeof(cbh_template_result));
  if (e == hipSuccess) e = upload(tables, &d_scale, cand_scale, n, s);
  if (e == hipSuccess) e = upload(tables, &d_tab, patches, s);
  int rc = e == hipSuccess ? CBH_OK : fail("template match pairs scratch", e);
  if (rc == CBH_OK)
    rc = queue_ransac(tables, probs, d_tmpl_xy, d_match_xy, first, n, 2, cand_scale, d_m, d_found, d_detail, s);
  if (rc == CBH_OK) {
    hipLaunchKernelGGL(k_tm_prepare, dim3(((unsigned)n + 63) / 64), dim3(64), 0, s, d_m, d_found, 2u, (unsigned)n, 0, 0,
                       d_scale, d_wm, d_ok, d_roi, (const PPatch*)d_tab);
    rc = queue_warp_ragged(tables, images, patches, d_tab, d_imgs, img_off, img_w, img_h, img_row_stride, channels, d_wm, d_ok,
                           d_p, s);
  }
  if (rc == CBH_OK) {
    unsigned char *cg = d_gray, *tgray = d_gray + gray_bytes;
    for (size_t i0 = 0; i0 < n; i0 += 65535) {
      const size_t m = std::min<size_t>(65535, n - i0);
      unsigned long long most = 1;
      for (size_t i = i0; i < i0 + m; ++i) most = std::max(most, (unsigned long long)patches[i].tw * patches[i].th);
      launch_tm_mask_ragged(dim3((unsigned)std::min<unsigned long long>(1024, (most + 255) / 256), (unsigned)m), s, d_p,
                            d_tmpl_base, d_tab + i0, channels, cg, tgray);
    }
    if ((e = hipGetLastError()) != hipSuccess) rc = fail("template match pairs", e);
    for (size_t i0 = 0; i0 < n && rc == CBH_OK;) {
      const size_t px = (size_t)tg[i0].tw * tg[i0].th;
      const size_t per = std::max<size_t>(1, std::min<size_t>(65535, ((size_t)1 << 30) / px));  // (cbh_template_hashes_dev's)
      size_t i1 = i0 + 1;
      while (i1 < n && i1 - i0 < per && tg[i1].tw == tg[i0].tw && tg[i1].th == tg[i0].th) ++i1;
      const size_t g0 = (size_t)patches[i0].gray_off;
      rc = launch_dcthash(cg + g0, i1 - i0, (int)tg[i0].tw, (int)tg[i0].th, tg[i0].tw, px, (uint64_t*)d_hash + i0, s);
      if (rc == CBH_OK)
        rc = launch_dcthash(tgray + g0, i1 - i0, (int)tg[i0].tw, (int)tg[i0].th, tg[i0].tw, px, (uint64_t*)d_hash + n + i0, s);
      if (hash_launches) *hash_launches += 2;
      i0 = i1;
    }
  }
  if (rc == CBH_OK) {
    hipLaunchKernelGGL(k_tm_finish, dim3(((unsigned)n + 63) / 64), dim3(64), 0, s, d_m, d_found, d_detail, d_ok, d_roi, d_hash,
                       d_hash + n, (unsigned)n, d_res);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(res, d_res, n * sizeof(cbh_template_result), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) rc = fail("template match pairs", e);
  }
  e = hipStreamSynchronize(s);  // the results; and the host tables are leaving
  if (rc == CBH_OK && e != hipSuccess) rc = fail("template match pairs", e);
  return rc;
}

void set_tmatch_chunk_mb(int v) {
  if (v > 0) g_tmatch_chunk_mb = v;
}
int get_tmatch_chunk_mb() { return g_tmatch_chunk_mb; }

}  // namespace cbh

extern "C" {

int cbh_estimate_rigid_dev(const void* d_a_xy, const void* d_b_xy, size_t n, const uint64_t* first, void* d_m,
                           void* d_found, void* d_detail, int device, void* stream) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) return CBH_OK;
  if (!first || !d_m || !d_found || n > (1u << 24) || !cbh::lists_ok(first, n) || (first[n] && (!d_a_xy || !d_b_xy)))
    return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  cbh::Scratch scratch(s);
  std::vector<cbh::RProblem> probs;
  int rc = cbh::queue_ransac(scratch, probs, (const float*)d_a_xy, (const float*)d_b_xy, first, n, 1, nullptr, (double*)d_m,
                             (unsigned char*)d_found, (cbh_rigid_detail*)d_detail, s);
  if (rc != CBH_OK) return rc;
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the host table must outlive its copy
  return e == hipSuccess ? CBH_OK : cbh::fail("rigid transform", e);
}

int cbh_estimate_rigid(const float* a_xy, const float* b_xy, size_t n, const uint64_t* first, double* m, uint8_t* found,
                       cbh_rigid_detail* detail, int device) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) return CBH_OK;
  if (!first || !m || !found || n > (1u << 24) || !cbh::lists_ok(first, n) || (first[n] && (!a_xy || !b_xy)))
    return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  const size_t pts = std::max<size_t>(first[n], 1) * 2 * sizeof(float);
  cbh::Staging st("rigid transform");
  float *d_a, *d_b;
  double* d_m;
  uint8_t* d_found;
  cbh_rigid_detail* d_detail = nullptr;
  st.alloc(&d_a, pts);
  st.alloc(&d_b, pts);
  st.alloc(&d_m, n * 6 * sizeof(double));
  st.alloc(&d_found, n);
  if (detail) st.alloc(&d_detail, n * sizeof(cbh_rigid_detail));
  if (first[n]) st.up(d_a, a_xy, first[n] * 8), st.up(d_b, b_xy, first[n] * 8);
  int rc = st.status();
  if (rc == CBH_OK) rc = cbh_estimate_rigid_dev(d_a, d_b, n, first, d_m, d_found, d_detail, device, st.s);
  if (rc != CBH_OK) return rc;
  st.down(m, d_m, n * 6 * sizeof(double));
  st.down(found, d_found, n);
  if (detail) st.down(detail, d_detail, n * sizeof(cbh_rigid_detail));
  st.sync();
  return st.status();
}

int cbh_warp_affine_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                        const uint32_t* img_row_stride, int channels, const void* d_m, const void* d_found, int tw, int th,
                        void* d_patches, void* d_warped, int device, void* stream) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) return CBH_OK;
  if (!d_imgs || !img_off || !img_w || !img_h || !img_row_stride || !d_m || !d_found || !d_patches ||
      !cbh::channels_ok(channels) || tw < 1 || th < 1 || tw > 32767 || th > 32767 || n > (1u << 24) ||
      ((uintptr_t)d_patches & 15))
    return CBH_E_INVAL;
  for (size_t i = 0; i < n; ++i)
    if (!cbh::image_ok(img_w[i], img_h[i], img_row_stride[i], channels)) return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  cbh::Scratch scratch(s);
  double* d_wm = nullptr;
  unsigned char* d_ok = nullptr;
  hipError_t e = scratch.get(&d_wm, n * 6 * sizeof(double));
  if (e == hipSuccess) e = scratch.get(&d_ok, n);
  if (e != hipSuccess) return cbh::fail("warp scratch", e);
  hipLaunchKernelGGL(cbh::k_tm_prepare, dim3(((unsigned)n + 63) / 64), dim3(64), 0, s, (const double*)d_m,
                     (const unsigned char*)d_found, 1u, (unsigned)n, tw, th, (const float*)nullptr, d_wm, d_ok, (int*)nullptr,
                     (const cbh::PPatch*)nullptr);
  std::vector<cbh::WImage> images;
  int rc = cbh::queue_warp(scratch, images, (const uint8_t*)d_imgs, n, img_off, img_w, img_h, img_row_stride, channels, d_wm,
                           d_ok, tw, th, (uint8_t*)d_patches, s);
  if (rc != CBH_OK) return rc;
  e = hipGetLastError();
  if (e == hipSuccess && d_warped) e = hipMemcpyAsync(d_warped, d_ok, n, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the host table must outlive its copy
  return e == hipSuccess ? CBH_OK : cbh::fail("warp", e);
}

int cbh_warp_affine_ragged_dev(const void* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                               const uint32_t* img_h, const uint32_t* img_row_stride, int channels, const void* d_m,
                               const void* d_found, const uint32_t* tw, const uint32_t* th, const uint64_t* patch_off,
                               void* d_patches, void* d_warped, int device, void* stream) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) return CBH_OK;
  if (!d_imgs || !img_off || !img_w || !img_h || !img_row_stride || !d_m || !d_found || !tw || !th || !patch_off ||
      !d_patches || !cbh::channels_ok(channels) || n > (1u << 24) || ((uintptr_t)d_patches & 15))
    return CBH_E_INVAL;
  std::vector<cbh::PPatch> patches(n);
  for (size_t i = 0; i < n; ++i) {
    if (!cbh::image_ok(img_w[i], img_h[i], img_row_stride[i], channels) || tw[i] < 1 || th[i] < 1 || tw[i] > 32767 ||
        th[i] > 32767 || (patch_off[i] & 15))
      return CBH_E_INVAL;
    patches[i] = {patch_off[i], 0ull, 0ull, tw[i], th[i], 0u, 0u};
  }
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  cbh::Scratch scratch(s);
  double* d_wm = nullptr;
  unsigned char* d_ok = nullptr;
  cbh::PPatch* d_tab = nullptr;
  hipError_t e = scratch.get(&d_wm, n * 6 * sizeof(double));
  if (e == hipSuccess) e = scratch.get(&d_ok, n);
  if (e == hipSuccess) e = cbh::upload(scratch, &d_tab, patches, s);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);  // the table's copy may be queued
    return cbh::fail("warp scratch", e);
  }
  hipLaunchKernelGGL(cbh::k_tm_prepare, dim3(((unsigned)n + 63) / 64), dim3(64), 0, s, (const double*)d_m,
                     (const unsigned char*)d_found, 1u, (unsigned)n, 0, 0, (const float*)nullptr, d_wm, d_ok, (int*)nullptr,
                     (const cbh::PPatch*)d_tab);
  std::vector<cbh::WImage> images;
  int rc = cbh::queue_warp_ragged(scratch, images, patches, d_tab, (const uint8_t*)d_imgs, img_off, img_w, img_h, img_row_stride,
                                  channels, d_wm, d_ok, (uint8_t*)d_patches, s);
  e = hipGetLastError();
  if (rc == CBH_OK && e == hipSuccess && d_warped) e = hipMemcpyAsync(d_warped, d_ok, n, hipMemcpyDeviceToDevice, s);
  const hipError_t e2 = hipStreamSynchronize(s);  // the host tables must outlive their copies
  if (rc != CBH_OK) return rc;
  if (e == hipSuccess) e = e2;
  return e == hipSuccess ? CBH_OK : cbh::fail("ragged warp", e);
}

int cbh_template_match_dev(const void* d_tmpl, int tw, int th, size_t tmpl_row_stride, int tmpl_channels, const void* d_imgs,
                           size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                           const uint32_t* img_row_stride, int channels, const void* d_tmpl_xy, const void* d_match_xy,
                           const uint64_t* first, const float* cand_scale, void* d_results, void* d_patches, int device,
                           void* stream) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) return CBH_OK;
  if (!d_tmpl || !d_imgs || !img_off || !img_w || !img_h || !img_row_stride || !first || !cand_scale || !d_results ||
      !cbh::channels_ok(channels) || !cbh::channels_ok(tmpl_channels) || tw < 1 || th < 1 || tw > 32767 || th > 32767 ||
      tmpl_row_stride < (size_t)tw * tmpl_channels || n > (1u << 24) || ((uintptr_t)d_patches & 15) ||
      !cbh::lists_ok(first, n) || (first[n] && (!d_tmpl_xy || !d_match_xy)))
    return CBH_E_INVAL;
  for (size_t i = 0; i < n; ++i)
    if (!cbh::image_ok(img_w[i], img_h[i], img_row_stride[i], channels) || !(cand_scale[i] > 0.f) || std::isinf(cand_scale[i]))
      return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  const size_t patch = (size_t)tw * th * channels;
  // groups of candidates whose patches fit "tmatch_chunk_mb" of scratch (a multiple of four, so that a caller's patches
  // stay aligned)
  const size_t per = d_patches ? n : std::max<size_t>(4, (cbh::tmatch_budget() / patch) & ~(size_t)3);
  std::vector<cbh::RProblem> probs;
  std::vector<cbh::WImage> images;
  std::vector<uint64_t> rel;
  for (size_t i0 = 0; i0 < n; i0 += per) {
    const size_t m = std::min(per, n - i0);
    cbh::Scratch scratch(s);
    double *d_m = nullptr, *d_wm = nullptr;
    unsigned char *d_found = nullptr, *d_ok = nullptr;
    cbh_rigid_detail* d_detail = nullptr;
    int* d_roi = nullptr;
    float* d_scale = nullptr;
    unsigned long long* d_hash = nullptr;
    uint8_t* d_p = d_patches ? (uint8_t*)d_patches + i0 * patch : nullptr;
    hipError_t e = scratch.get(&d_m, m * 12 * sizeof(double));
    if (e == hipSuccess) e = scratch.get(&d_wm, m * 6 * sizeof(double));
    if (e == hipSuccess) e = scratch.get(&d_found, m * 2);
    if (e == hipSuccess) e = scratch.get(&d_ok, m);
    if (e == hipSuccess) e = scratch.get(&d_detail, m * 2 * sizeof(cbh_rigid_detail));
    if (e == hipSuccess) e = scratch.get(&d_roi, m * 8 * sizeof(int));
    if (e == hipSuccess) e = scratch.get(&d_scale, m * sizeof(float));
    if (e == hipSuccess) e = scratch.get(&d_hash, m * 2 * sizeof(unsigned long long));
    if (e == hipSuccess && !d_p) e = scratch.get(&d_p, m * patch);
    if (e == hipSuccess) e = hipMemcpyAsync(d_scale, cand_scale + i0, m * sizeof(float), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return cbh::fail("template match scratch", e);
    rel.assign(first + i0, first + i0 + m + 1);
    for (uint64_t& v : rel) v -= first[i0];
    int rc = cbh::queue_ransac(scratch, probs, (const float*)d_tmpl_xy + 2 * first[i0], (const float*)d_match_xy + 2 * first[i0],
                               rel.data(), m, 2, cand_scale + i0, d_m, d_found, d_detail, s);
    if (rc != CBH_OK) {
      (void)hipStreamSynchronize(s);  // the copy of the caller's scales is queued
      return rc;
    }
    hipLaunchKernelGGL(cbh::k_tm_prepare, dim3(((unsigned)m + 63) / 64), dim3(64), 0, s, d_m, d_found, 2u, (unsigned)m, tw, th,
                       d_scale, d_wm, d_ok, d_roi, (const cbh::PPatch*)nullptr);
    rc = cbh::queue_warp(scratch, images, (const uint8_t*)d_imgs, m, img_off + i0, img_w + i0, img_h + i0, img_row_stride + i0,
                         channels, d_wm, d_ok, tw, th, d_p, s);
    if (rc == CBH_OK && (e = hipGetLastError()) != hipSuccess) rc = cbh::fail("template match", e);
    if (rc != CBH_OK) {
      (void)hipStreamSynchronize(s);  // the host tables of this group are still being read
      return rc;
    }
    // a non-blocking stream of our own would not be ordered with the NULL stream: the hashes run on `s` as well; with
    // s == NULL cbh_template_hashes_dev synchronises itself
    rc = cbh_template_hashes_dev(d_p, m, tw, th, (size_t)tw * channels, patch, channels, d_tmpl, tmpl_row_stride,
                                 tmpl_channels, d_hash, d_hash + m, device, s);
    if (rc != CBH_OK) {
      (void)hipStreamSynchronize(s);  // the host tables of this group are still being read
      return rc;
    }
    hipLaunchKernelGGL(cbh::k_tm_finish, dim3(((unsigned)m + 63) / 64), dim3(64), 0, s, d_m, d_found, d_detail, d_ok, d_roi,
                       d_hash, d_hash + m, (unsigned)m, (cbh_template_result*)d_results + i0);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // the host tables must outlive their copies
    if (e != hipSuccess) return cbh::fail("template match", e);
  }
  return CBH_OK;
}

int cbh_template_match(const uint8_t* tmpl, int tw, int th, size_t tmpl_row_stride, int tmpl_channels, const uint8_t* imgs,
                       size_t imgs_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                       const uint32_t* img_row_stride, int channels, const float* tmpl_xy, const float* match_xy,
                       const uint64_t* first, const float* cand_scale, cbh_template_result* results, uint8_t* patches,
                       int device) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) return CBH_OK;
  if (!tmpl || !imgs || !img_off || !img_w || !img_h || !img_row_stride || !first || !cand_scale || !results ||
      !cbh::channels_ok(channels) || !cbh::channels_ok(tmpl_channels) || tw < 1 || th < 1 || tw > 32767 || th > 32767 ||
      tmpl_row_stride < (size_t)tw * tmpl_channels || n > (1u << 24) || !cbh::lists_ok(first, n) ||
      (first[n] && (!tmpl_xy || !match_xy)))
    return CBH_E_INVAL;
  std::vector<uint64_t> end(n);
  for (size_t i = 0; i < n; ++i) {
    if (!cbh::image_ok(img_w[i], img_h[i], img_row_stride[i], channels) || !(cand_scale[i] > 0.f) || std::isinf(cand_scale[i]))
      return CBH_E_INVAL;
    end[i] = cbh::image_end(img_off[i], img_w[i], img_h[i], img_row_stride[i], channels);
    if (end[i] > imgs_bytes) return CBH_E_INVAL;
  }
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  // uploads of at most "tmatch_chunk_mb" each: runs of candidates whose image bytes span no more than that, and whose
  // patches fit it as well (at least one candidate, then multiples of four)
  const size_t budget = cbh::tmatch_budget(), patch = (size_t)tw * th * channels;
  const std::vector<cbh::Run> runs =
      cbh::make_runs(n, img_off, end.data(), budget, std::max<size_t>(4, (budget / patch) & ~(size_t)3));
  size_t span = 0, most_m = 0;
  for (const cbh::Run& r : runs) span = std::max<size_t>(span, r.hi - r.lo), most_m = std::max(most_m, r.m);
  const size_t tspan = (size_t)(th - 1) * tmpl_row_stride + (size_t)tw * tmpl_channels;
  const size_t pts = std::max<size_t>(first[n], 1) * 2 * sizeof(float);
  cbh::Staging st("template match");
  uint8_t *d_imgs, *d_tmpl, *d_patches = nullptr;
  float *d_a, *d_b;
  cbh_template_result* d_res;
  st.alloc(&d_imgs, span);
  st.alloc(&d_tmpl, tspan);
  st.alloc(&d_a, pts);
  st.alloc(&d_b, pts);
  st.alloc(&d_res, n * sizeof(cbh_template_result));
  if (patches) st.alloc(&d_patches, most_m * patch);
  st.up(d_tmpl, tmpl, tspan);
  if (first[n]) st.up(d_a, tmpl_xy, first[n] * 8), st.up(d_b, match_xy, first[n] * 8);
  int rc = st.status();
  std::vector<uint64_t> off, rel;
  for (size_t k = 0; k < runs.size() && rc == CBH_OK; ++k) {
    const cbh::Run& r = runs[k];
    cbh::rebase(r, img_off, &off);
    rel.assign(first + r.i0, first + r.i0 + r.m + 1);
    for (uint64_t& v : rel) v -= first[r.i0];
    // (the run before has finished: cbh_template_match_dev synchronises the stream before it returns)
    st.up(d_imgs, imgs + r.lo, r.hi - r.lo);
    if ((rc = st.status()) != CBH_OK) break;
    rc = cbh_template_match_dev(d_tmpl, tw, th, tmpl_row_stride, tmpl_channels, d_imgs, r.m, off.data(), img_w + r.i0,
                                img_h + r.i0, img_row_stride + r.i0, channels, d_a + 2 * first[r.i0], d_b + 2 * first[r.i0],
                                rel.data(), cand_scale + r.i0, d_res + r.i0, d_patches, device, st.s);
    if (rc == CBH_OK && patches) {  // before the next run warps into d_patches
      st.down(patches + r.i0 * patch, d_patches, r.m * patch);
      st.sync();
      rc = st.status();
    }
  }
  if (rc != CBH_OK) return rc;
  st.down(results, d_res, n * sizeof(cbh_template_result));
  st.sync();
  return st.status();
}

}  // extern "C"
