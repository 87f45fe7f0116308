// tmpairs.hip -- the kernels the grouped template match adds (cbh_template_match_pairs: TemplateMatcher::match for a batch
// of result groups, where every candidate has a template of its own).  The chain that launches them is tmimages.hip's
// run_pairs and tmatch.hip's template_match_pairs_tail; everything else they run is the single-template chain's kernels.
//   k_tm_match_pairs<EMIT>  tmimages.hip's k_tm_match with the train set read per candidate from a table
//   k_warp_ragged<CH>       tmatch.hip's k_warp with a patch size and a patch offset per candidate (warp_px.h's pixel)
//   k_tm_mask_ragged        prestage.hip's k_tm_mask with the template per candidate
// Built with -ffp-contract=off (Makefile), as tmatch.hip is: every float / double operation rounds once, as in the model.
#include <cstdint>

#include "cbh_internal.h"
#include "warp_px.h"

namespace cbh {
namespace {

constexpr int kBlock = kTmMatchBlock;
constexpr int kTrainPiece = kTmTrainPiece;
constexpr int kWarpBlock = 256;

// ---- the descriptor match against per-candidate train sets -----------------------------------------------------------
// k_tm_match's grid, key layout and count / emit contract (tmimages.hip): candidate cand0 + blockIdx.y, query row
// blockIdx.x * kBlock + threadIdx.x; the candidate's train rows are tsets[candidate].n rows from row tsets[candidate].base
// of `train`.  blockIdx.y is the candidate, so the choice is uniform per block and the LDS staging is k_tm_match's.
// The single-template launch keeps its own kernel: read in the ISA, both forms take the same registers (66 VGPRs counting,
// 42 emitting, 5 waves per SIMD by the 32 KB of LDS, no scratch) -- the table costs one dependent scalar load in front of
// the first staging loop and nothing per row -- so sharing one kernel would gain nothing, and keeping k_tm_match as it
// was leaves the code the existing entry runs untouched while the two entries are compared with each other.
template <bool EMIT>
__global__ __launch_bounds__(kBlock) void k_tm_match_pairs(const uint4* __restrict__ train_rows,
                                                           const TSet* __restrict__ tsets, const uint4* __restrict__ desc,
                                                           const unsigned* __restrict__ counts, unsigned kp_cap,
                                                           unsigned max_dist, unsigned cand0, unsigned* __restrict__ qcount,
                                                           const unsigned* __restrict__ qoff,
                                                           const unsigned long long* __restrict__ first,
                                                           unsigned long long base, unsigned g0,
                                                           unsigned long long* __restrict__ keys, unsigned long long cap) {
  __shared__ uint4 s_train[kTrainPiece * 2];
  const unsigned cand = cand0 + blockIdx.y;
  const unsigned rows = min(counts[cand], kp_cap);
  if (blockIdx.x * kBlock >= rows) return;  // (the whole block: no lane of it has a query)
  const TSet ts = tsets[cand];
  const uint4* __restrict__ train = train_rows + (size_t)ts.base * 2;
  const unsigned n_train = ts.n;
  const unsigned row = blockIdx.x * kBlock + threadIdx.x;
  const bool valid = row < rows;
  const size_t slot = (size_t)cand * kp_cap + (valid ? row : 0u);
  const uint4 qa = desc[slot * 2], qb = desc[slot * 2 + 1];
  unsigned cnt = 0;
  unsigned long long pos = 0, qkey = 0;
  if (EMIT) {
    pos = first[cand] - base + qoff[slot];
    qkey = (unsigned long long)((cand - g0) * kp_cap + row) << 41;
  }
  for (unsigned t0 = 0; t0 < n_train; t0 += kTrainPiece) {
    const unsigned piece = min((unsigned)kTrainPiece, n_train - t0);
    __syncthreads();
    for (unsigned k = threadIdx.x; k < piece * 2; k += kBlock) s_train[k] = train[(size_t)t0 * 2 + k];
    __syncthreads();
    if (!valid) continue;
    for (unsigned t = 0; t < piece; ++t) {
      const uint4 a = s_train[2 * t], b = s_train[2 * t + 1];
      const unsigned d = __popc(qa.x ^ a.x) + __popc(qa.y ^ a.y) + __popc(qa.z ^ a.z) + __popc(qa.w ^ a.w) +
                         __popc(qb.x ^ b.x) + __popc(qb.y ^ b.y) + __popc(qb.z ^ b.z) + __popc(qb.w ^ b.w);
      if (d <= max_dist) {
        if (EMIT) {
          if (pos < cap) keys[pos] = qkey | (unsigned long long)d << 32 | (t0 + t);
          ++pos;
        } else {
          ++cnt;
        }
      }
    }
  }
  if (!EMIT && valid) qcount[slot] = cnt;
}

// ---- the ragged warp -----------------------------------------------------------------------------------------------------
// The ragged form: candidate blockIdx.y warps into its own tw x th patch at out + patch_off (16-byte aligned).  A lane keeps
// k_warp's shape -- four consecutive pixels, row_start once and again where they cross a row, whole-dword stores -- but its
// pixel index runs inside ONE patch: no lane writes outside it, and the tail of a patch whose pixel count is not a
// multiple of four leaves as bytes.
template <int CH>
__global__ __launch_bounds__(kWarpBlock) void k_warp_ragged(const unsigned char* __restrict__ imgs,
                                                            const WImage* __restrict__ images, const double* __restrict__ wm,
                                                            const unsigned char* __restrict__ ok,
                                                            const PPatch* __restrict__ patches, unsigned char* __restrict__ out) {
  const unsigned img = blockIdx.y;
  const PPatch pt = patches[img];
  const unsigned tw = pt.tw, th = pt.th, total = tw * th;  // sides up to 32767: below 2^30
  const double* M = wm + (size_t)img * 6;
  const bool warped = ok[img] != 0;
  const WImage im = images[img];
  for (unsigned p0 = (blockIdx.x * kWarpBlock + threadIdx.x) * 4u; p0 < total; p0 += gridDim.x * kWarpBlock * 4u) {
    unsigned y = p0 / tw, x = p0 - y * tw;
    unsigned words[CH] = {};
    const int live = (int)min(4u, total - p0);
    int X0, Y0;
    row_start(M, (int)y, X0, Y0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < live) {
        unsigned px[CH] = {};
        if (warped) warp_pixel<CH>(imgs, im, M, (int)x, X0, Y0, px);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int b = k * CH + c;
          words[b >> 2] |= px[c] << (8 * (b & 3));
        }
        if (++x == tw) {
          x = 0, ++y;
          if (k + 1 < live) row_start(M, (int)y, X0, Y0);
        }
      }
    }
    unsigned char* dst = out + pt.patch_off + (size_t)p0 * CH;
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
}

// ---- the mask ------------------------------------------------------------------------------------------------------------
// prestage.hip's k_tm_mask (src/templatematcher.cpp:334-364) with the template per candidate: candidate blockIdx.y's patch
// against ITS template -> the two grey planes (pitch tw) at gray_off of cand_gray / tmpl_gray.  One channel count for both.
__device__ __forceinline__ unsigned tm_gray(unsigned b, unsigned g, unsigned r) {
  return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14;
}
__global__ __launch_bounds__(256) void k_tm_mask_ragged(const unsigned char* __restrict__ patch_base,
                                                        const unsigned char* __restrict__ tmpl_base,
                                                        const PPatch* __restrict__ patches, int ch,
                                                        unsigned char* __restrict__ cand_gray,
                                                        unsigned char* __restrict__ tmpl_gray) {
  const PPatch pt = patches[blockIdx.y];
  const unsigned total = pt.tw * pt.th;
  const unsigned char* c = patch_base + pt.patch_off;
  const unsigned char* tm = tmpl_base + pt.tmpl_off;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned y = i / pt.tw, x = i - y * pt.tw;
    const unsigned char* p = c + (size_t)i * ch;
    const unsigned char* t = tm + (size_t)y * pt.tstride + (size_t)x * ch;
    unsigned g = ch == 1 ? p[0] : tm_gray(p[0], p[1], p[2]);
    const unsigned m = g != 0u ? 255u : 0u;
    unsigned tg;
    if (ch == 1) {
      tg = t[0] & m;
    } else if (ch == 3) {
      tg = tm_gray(t[0] & m, t[1] & m, t[2] & m);
    } else {
      const unsigned a = t[3];
      tg = tm_gray(((t[0] * a) >> 8) & m, ((t[1] * a) >> 8) & m, ((t[2] * a) >> 8) & m);
      g = (g * a) >> 8;
    }
    cand_gray[pt.gray_off + i] = (unsigned char)g;
    tmpl_gray[pt.gray_off + i] = (unsigned char)tg;
  }
}

}  // namespace

void launch_tm_match_pairs(bool emit, unsigned tiles, unsigned m, hipStream_t s, const uint8_t* d_train, const TSet* d_tsets,
                           const uint8_t* d_desc, const uint32_t* d_counts, unsigned kp_cap, unsigned max_dist, unsigned cand0,
                           unsigned* d_qcount, const unsigned* d_qoff, const unsigned long long* d_first,
                           unsigned long long base, unsigned g0, unsigned long long* d_keys, unsigned long long cap) {
  if (emit)
    hipLaunchKernelGGL(k_tm_match_pairs<true>, dim3(tiles, m), dim3(kBlock), 0, s, (const uint4*)d_train, d_tsets,
                       (const uint4*)d_desc, d_counts, kp_cap, max_dist, cand0, d_qcount, d_qoff, d_first, base, g0, d_keys, cap);
  else
    hipLaunchKernelGGL(k_tm_match_pairs<false>, dim3(tiles, m), dim3(kBlock), 0, s, (const uint4*)d_train, d_tsets,
                       (const uint4*)d_desc, d_counts, kp_cap, max_dist, cand0, d_qcount, d_qoff, d_first, base, g0, d_keys, cap);
}

void launch_warp_ragged(int channels, dim3 grid, hipStream_t s, const uint8_t* d_imgs, const WImage* d_images,
                        const double* d_wm, const unsigned char* d_ok, const PPatch* d_patches, uint8_t* d_out) {
  if (channels == 1)
    hipLaunchKernelGGL(k_warp_ragged<1>, grid, dim3(kWarpBlock), 0, s, d_imgs, d_images, d_wm, d_ok, d_patches, d_out);
  else if (channels == 3)
    hipLaunchKernelGGL(k_warp_ragged<3>, grid, dim3(kWarpBlock), 0, s, d_imgs, d_images, d_wm, d_ok, d_patches, d_out);
  else
    hipLaunchKernelGGL(k_warp_ragged<4>, grid, dim3(kWarpBlock), 0, s, d_imgs, d_images, d_wm, d_ok, d_patches, d_out);
}

void launch_tm_mask_ragged(dim3 grid, hipStream_t s, const uint8_t* d_patches, const uint8_t* d_tmpl_base,
                           const PPatch* d_tab, int channels, uint8_t* d_cand_gray, uint8_t* d_tmpl_gray) {
  hipLaunchKernelGGL(k_tm_mask_ragged, grid, dim3(256), 0, s, d_patches, d_tmpl_base, d_tab, channels, d_cand_gray,
                     d_tmpl_gray);
}

}  // namespace cbh
