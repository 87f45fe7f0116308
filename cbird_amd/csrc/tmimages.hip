// tmimages.hip -- TemplateMatcher::match (src/templatematcher.cpp:105-374) from the decoded images to the score for one
// template and a batch of candidates, without a host round trip between the upload and the results:
//   k_resize_ragged<CH>  sizeScaleFactor (src/cvutil.cpp:1951-1956: cv::resize INTER_LANCZOS4) of ragged 1 / 3 / 4 channel
//                        images, each to its own size.  k_resize_lanczos4's arithmetic (prestage.hip: 8 x 8 clamped taps,
//                        the host-built 11-bit tables, (v + 2^21) >> 22, saturate) applied to every channel; integer
//                        throughout, so the bytes do not depend on evaluation order.  One lane makes four consecutive output
//                        pixels: a tap's pixel is addressed once for all its channels, the x weights are read once per
//                        pixel, and the 4 * CH result bytes leave as whole dwords (the tail of an image, which is not a
//                        multiple of four pixels, as bytes: no lane writes outside its image).
//   k_gray_ragged        cvtColor(BGR2GRAY / BGRA2GRAY) (cbh_gray_px) of ragged images, what ORB applies to a colour input
//   k_tm_match<EMIT>     BFMatcher(NORM_HAMMING).radiusMatch (:134, :217) of every candidate's descriptor rows against the
//                        template's: the train rows are staged in LDS in pieces of kTrainPiece, every lane keeps one query row
//                        in registers and reads the train rows as broadcasts.  A counting pass, an exclusive scan
//                        (k_tm_scan_queries, k_tm_scan_first), then the emitting pass writes 64-bit keys
//                        query << 41 | distance << 32 | train row at their final candidate's range; records.hip's radix sort
//                        puts them into the contract's order (candidate, query row, distance, train row).  No capacity is
//                        guessed and nothing is retried.
//   k_tm_gather          :241-250 from the ordered keys and the kp_after tables: the tmplPoints / matchPoints lists
// and cbh_template_match_images(_dev), the chain resize -> grey -> ORB -> match -> gather -> cbh_template_match_dev.
// cbh_template_match_pairs(_dev) is the same chain for (template image, candidate image) pairs over one image table --
// Database::similar's call of the matcher once per needle (src/database.cpp:1418) as one call: run_pairs below, with
// tmpairs.hip's kernels where a candidate has a template of its own and tmatch.hip's template_match_pairs_tail.
//
// UNPINNED, as tmatch.hip and orb.hip are: OpenCV is not available to this repository; the estimate, the warp and ORB are
// restated as recalled.  The resize, the grey conversion and the match are integer arithmetic checked against the oracle.
#include <climits>
#include <cmath>
#include <cstdint>

#include <algorithm>
#include <map>
#include <vector>

#include "cbh_index.h"
#include "cbh_runs.h"
#include "cbh_staging.h"
#include "gray_px.h"

namespace cbh {
namespace {

constexpr int kBlock = kTmMatchBlock;
constexpr int kTrainPiece = kTmTrainPiece;  // train rows in LDS at a time (32 KB); any number of rows, piece by piece
constexpr int kQueryBits = 23;     // of a key's query field (the record layout of hamm256_scan.hip)
constexpr unsigned long long kGroupKeys = 1ull << 26;  // keys sorted at a time (512 MB), unless one candidate has more

struct RImage {
  unsigned long long src_off, dst_off;
  unsigned w, h, stride, dw, dh;
  unsigned xtab, ytab;  // first entries of its x / y tables (offsets; the weights start at 8 x that)
  unsigned copy;        // 1: same size, the bytes as they are (a candidate the chain does not resize)
};

template <int CH>
__device__ __forceinline__ void resize_pixel(const unsigned char* __restrict__ img, const RImage& im,
                                             const int* __restrict__ ofs, const short* __restrict__ coef, unsigned dx,
                                             unsigned dy, unsigned (&px)[CH]) {
  if (im.copy) {
    const unsigned char* p = img + (size_t)dy * im.stride + (size_t)dx * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) px[c] = p[c];
    return;
  }
  const int sx0 = ofs[im.xtab + dx] - 3, sy0 = ofs[im.ytab + dy] - 3;
  const short* xa = coef + ((size_t)im.xtab + dx) * 8;
  const short* yb = coef + ((size_t)im.ytab + dy) * 8;
  int a[8], cx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = xa[j];
    cx[j] = min(max(sx0 + j, 0), (int)im.w - 1) * CH;
  }
  int v[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) v[c] = 0;
#pragma unroll 2
  for (int k = 0; k < 8; ++k) {
    const unsigned char* S = img + (size_t)min(max(sy0 + k, 0), (int)im.h - 1) * im.stride;
    int D[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) D[c] = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if constexpr (CH == 4) {
        unsigned t;
        __builtin_memcpy(&t, S + cx[j], 4);  // (rows of a ragged batch need not be dword aligned)
#pragma unroll
        for (int c = 0; c < 4; ++c) D[c] += (int)((t >> (8 * c)) & 255u) * a[j];
      } else {
#pragma unroll
        for (int c = 0; c < CH; ++c) D[c] += (int)S[cx[j] + c] * a[j];
      }
    }
    const int b = yb[k];
#pragma unroll
    for (int c = 0; c < CH; ++c) v[c] += D[c] * b;
  }
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int r = (v[c] + (1 << 21)) >> 22;
    px[c] = (unsigned)(r < 0 ? 0 : r > 255 ? 255 : r);
  }
}

// the 4 * CH bytes of four consecutive pixels at out + p0 * CH (dword aligned: the image starts on 16 bytes, p0 on four
// pixels); `live` < 4 at the end of an image
template <int CH>
__device__ __forceinline__ void store_pixels(unsigned char* __restrict__ out, unsigned p0, int live,
                                             const unsigned (&words)[CH]) {
  unsigned char* dst = out + (size_t)p0 * CH;
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

// grid (x, images): image blockIdx.y, four output pixels per lane
template <int CH>
__global__ __launch_bounds__(kBlock) void k_resize_ragged(const unsigned char* __restrict__ src,
                                                          const RImage* __restrict__ images, const int* __restrict__ ofs,
                                                          const short* __restrict__ coef, unsigned char* __restrict__ dst) {
  const RImage im = images[blockIdx.y];
  const unsigned total = im.dw * im.dh;  // sides up to 32767: below 2^30
  const unsigned char* img = src + im.src_off;
  unsigned char* out = dst + im.dst_off;
  for (unsigned p0 = (blockIdx.x * kBlock + threadIdx.x) * 4u; p0 < total; p0 += gridDim.x * kBlock * 4u) {
    const int live = (int)min(4u, total - p0);
    unsigned dy = p0 / im.dw, dx = p0 - dy * im.dw;
    unsigned words[CH] = {};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < live) {
        unsigned px[CH];
        resize_pixel<CH>(img, im, ofs, coef, dx, dy, px);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int b = k * CH + c;
          words[b >> 2] |= px[c] << (8 * (b & 3));
        }
        if (++dx == im.dw) dx = 0, ++dy;
      }
    }
    store_pixels<CH>(out, p0, live, words);
  }
}

// grey planes (pitch = width) at dst_off of images of CH = 3 / 4 channels; RImage: dw / dh / the tables unused
template <int CH>
__global__ __launch_bounds__(kBlock) void k_gray_ragged(const unsigned char* __restrict__ src,
                                                        const RImage* __restrict__ images, unsigned char* __restrict__ dst) {
  const RImage im = images[blockIdx.y];
  const unsigned total = im.w * im.h;
  const unsigned char* img = src + im.src_off;
  unsigned char* out = dst + im.dst_off;
  for (unsigned p0 = (blockIdx.x * kBlock + threadIdx.x) * 4u; p0 < total; p0 += gridDim.x * kBlock * 4u) {
    const int live = (int)min(4u, total - p0);
    unsigned y = p0 / im.w, x = p0 - y * im.w;
    unsigned words[1] = {0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < live) {
        const unsigned char* p = img + (size_t)y * im.stride + (size_t)x * CH;
        words[0] |= (unsigned)cbh_gray_px(p[0], p[1], p[2]) << (8 * k);
        if (++x == im.w) x = 0, ++y;
      }
    }
    store_pixels<1>(out, p0, live, words);
  }
}

// ---- the descriptor match -----------------------------------------------------------------------------------------------
// grid (query tiles, candidates of this launch): candidate cand0 + blockIdx.y, query row blockIdx.x * kBlock + threadIdx.x.
// EMIT false: qcount[slot] = pairs of the query within max_dist.  EMIT true: their keys, in train order, from
// first[candidate] - base + qoff[slot] on (slot = candidate * kp_cap + row); a key at or past `cap` is not written
template <bool EMIT>
__global__ __launch_bounds__(kBlock) void k_tm_match(const uint4* __restrict__ train, unsigned n_train,
                                                     const uint4* __restrict__ desc, const unsigned* __restrict__ counts,
                                                     unsigned kp_cap, unsigned max_dist, unsigned cand0,
                                                     unsigned* __restrict__ qcount, const unsigned* __restrict__ qoff,
                                                     const unsigned long long* __restrict__ first, unsigned long long base,
                                                     unsigned g0, unsigned long long* __restrict__ keys,
                                                     unsigned long long cap) {
  __shared__ uint4 s_train[kTrainPiece * 2];
  const unsigned cand = cand0 + blockIdx.y;
  const unsigned rows = min(counts[cand], kp_cap);
  if (blockIdx.x * kBlock >= rows) return;  // (the whole block: no lane of it has a query)
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

// inclusive scan of one value per thread of a 256-thread block; *total = the block's sum
template <class T>
__device__ __forceinline__ T block_scan(T v, T* s_w, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) s_w[wave] = x;
  __syncthreads();
  T off = 0;
  for (int w = 0; w < wave; ++w) off += s_w[w];
  *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  __syncthreads();
  return x + off;
}

// one block per candidate: qoff[slot] = pairs of the candidate's earlier query rows, total[candidate] = all its pairs
__global__ __launch_bounds__(kBlock) void k_tm_scan_queries(const unsigned* __restrict__ qcount,
                                                            const unsigned* __restrict__ counts, unsigned kp_cap,
                                                            unsigned cand0, unsigned* __restrict__ qoff,
                                                            unsigned long long* __restrict__ total) {
  __shared__ unsigned s_w[4];
  const unsigned cand = cand0 + blockIdx.x;
  const unsigned rows = min(counts[cand], kp_cap);
  unsigned carry = 0;  // (kp_cap x train rows stays below 2^32: checked by the callers)
  for (unsigned r0 = 0; r0 < rows; r0 += kBlock) {
    const unsigned row = r0 + threadIdx.x;
    const size_t slot = (size_t)cand * kp_cap + row;
    const unsigned v = row < rows ? qcount[slot] : 0u;
    unsigned sum;
    const unsigned incl = block_scan(v, s_w, &sum);
    if (row < rows) qoff[slot] = carry + incl - v;
    carry += sum;
  }
  if (threadIdx.x == 0) total[cand] = carry;
}

// one block: first[0] = 0, first[i + 1] = first[i] + total[i]
__global__ __launch_bounds__(kBlock) void k_tm_scan_first(const unsigned long long* __restrict__ total, unsigned n,
                                                          unsigned long long* __restrict__ first) {
  __shared__ unsigned long long s_w[4];
  unsigned long long carry = 0;
  if (threadIdx.x == 0) first[0] = 0;
  for (unsigned i0 = 0; i0 < n; i0 += kBlock) {
    const unsigned i = i0 + threadIdx.x;
    const unsigned long long v = i < n ? total[i] : 0ull;
    unsigned long long sum;
    const unsigned long long incl = block_scan(v, s_w, &sum);
    if (i < n) first[i + 1] = carry + incl;
    carry += sum;
  }
}

// the ordered keys of candidates g0 .. -> entries base .. of the point lists (and of the records)
__global__ __launch_bounds__(kBlock) void k_tm_gather(const unsigned long long* __restrict__ keys, unsigned long long cnt,
                                                      unsigned long long base, unsigned g0, unsigned kp_cap,
                                                      const float2* __restrict__ tmpl_xy, const float2* __restrict__ cand_xy,
                                                      float2* __restrict__ tmpl_pts, float2* __restrict__ match_pts,
                                                      cbh_dmatch* __restrict__ records, const TSet* __restrict__ tsets) {
  const unsigned long long r = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  if (r >= cnt) return;
  const unsigned long long key = keys[r];
  const unsigned q = (unsigned)(key >> 41), d = (unsigned)(key >> 32) & 0x1ffu, t = (unsigned)key;
  const unsigned cand = g0 + q / kp_cap, row = q % kp_cap;
  tmpl_pts[base + r] = tmpl_xy[(tsets ? (size_t)tsets[cand].base : 0) + t];  // (the grouped chain: its own template's)
  match_pts[base + r] = cand_xy[(size_t)cand * kp_cap + row];
  if (records) {
    cbh_dmatch m;
    m.query_idx = (int)row, m.train_idx = (int)t, m.distance = (int)d;
    records[base + r] = m;
  }
}

// ---- resize / grey launchers.  The tables they upload live in `keep` (host memory the caller holds until it has
// synchronised the stream) and in `scratch` ----------------------------------------------------------------------------
struct ResizeTables {
  std::vector<RImage> images;
  std::vector<int> ofs;
  std::vector<short> coef;
};

// copy: NULL, or per image 1 = same size and no filter
int queue_resize(Scratch& scratch, ResizeTables& keep, const uint8_t* d_src, size_t n, const uint64_t* off, const uint32_t* w,
                 const uint32_t* h, const uint32_t* stride, int channels, const uint64_t* dst_off, const uint32_t* dw,
                 const uint32_t* dh, const uint8_t* copy, uint8_t* d_dst, hipStream_t s) {
  keep.images.resize(n);
  keep.ofs.clear(), keep.coef.clear();
  std::map<std::pair<uint32_t, uint32_t>, unsigned> made;  // (ssize, dsize) -> first entry: each pair built once
  std::vector<int> o;
  std::vector<short> c;
  auto table = [&](uint32_t ssize, uint32_t dsize) {
    auto it = made.find({ssize, dsize});
    if (it != made.end()) return it->second;
    const unsigned at = (unsigned)keep.ofs.size();
    lanczos4_table((int)ssize, (int)dsize, &o, &c);
    keep.ofs.insert(keep.ofs.end(), o.begin(), o.end());
    keep.coef.insert(keep.coef.end(), c.begin(), c.end());
    made[{ssize, dsize}] = at;
    return at;
  };
  unsigned long long most = 0;
  for (size_t i = 0; i < n; ++i) {
    const bool cp = copy && copy[i];
    keep.images[i] = {off[i], dst_off[i], w[i], h[i], stride[i], dw[i], dh[i], cp ? 0u : table(w[i], dw[i]),
                      cp ? 0u : table(h[i], dh[i]), cp ? 1u : 0u};
    most = std::max<unsigned long long>(most, (unsigned long long)dw[i] * dh[i]);
  }
  if (keep.ofs.empty()) keep.ofs.assign(1, 0), keep.coef.assign(8, 0);
  RImage* d_images = nullptr;
  int* d_ofs = nullptr;
  short* d_coef = nullptr;
  hipError_t e = upload(scratch, &d_images, keep.images, s);
  if (e == hipSuccess) e = upload(scratch, &d_ofs, keep.ofs, s);
  if (e == hipSuccess) e = upload(scratch, &d_coef, keep.coef, s);
  if (e != hipSuccess) return fail("ragged resize tables", e);
  const unsigned gx = (unsigned)std::min<unsigned long long>((most + 4 * kBlock - 1) / (4 * kBlock), 4096);
  for (size_t i0 = 0; i0 < n; i0 += 65535) {
    const dim3 grid(gx, (unsigned)std::min<size_t>(65535, n - i0));
    if (channels == 1)
      hipLaunchKernelGGL(k_resize_ragged<1>, grid, dim3(kBlock), 0, s, d_src, d_images + i0, d_ofs, d_coef, d_dst);
    else if (channels == 3)
      hipLaunchKernelGGL(k_resize_ragged<3>, grid, dim3(kBlock), 0, s, d_src, d_images + i0, d_ofs, d_coef, d_dst);
    else
      hipLaunchKernelGGL(k_resize_ragged<4>, grid, dim3(kBlock), 0, s, d_src, d_images + i0, d_ofs, d_coef, d_dst);
  }
  e = hipGetLastError();
  return e == hipSuccess ? CBH_OK : fail("ragged resize", e);
}

int queue_gray(Scratch& scratch, std::vector<RImage>& keep, const uint8_t* d_src, size_t n, const uint64_t* off,
               const uint32_t* w, const uint32_t* h, const uint32_t* stride, int channels, const uint64_t* dst_off,
               uint8_t* d_dst, hipStream_t s) {
  keep.resize(n);
  unsigned long long most = 0;
  for (size_t i = 0; i < n; ++i) {
    keep[i] = {off[i], dst_off[i], w[i], h[i], stride[i], w[i], h[i], 0u, 0u, 0u};
    most = std::max<unsigned long long>(most, (unsigned long long)w[i] * h[i]);
  }
  RImage* d_images = nullptr;
  hipError_t e = upload(scratch, &d_images, keep, s);
  if (e != hipSuccess) return fail("ragged grey tables", e);
  const unsigned gx = (unsigned)std::min<unsigned long long>((most + 4 * kBlock - 1) / (4 * kBlock), 4096);
  for (size_t i0 = 0; i0 < n; i0 += 65535) {
    const dim3 grid(gx, (unsigned)std::min<size_t>(65535, n - i0));
    if (channels == 3)
      hipLaunchKernelGGL(k_gray_ragged<3>, grid, dim3(kBlock), 0, s, d_src, d_images + i0, d_dst);
    else
      hipLaunchKernelGGL(k_gray_ragged<4>, grid, dim3(kBlock), 0, s, d_src, d_images + i0, d_dst);
  }
  e = hipGetLastError();
  return e == hipSuccess ? CBH_OK : fail("ragged grey", e);
}

// ---- match + gather -----------------------------------------------------------------------------------------------------
struct MatchState {  // what the counting pass leaves for the emitting pass (blocks of the caller's Scratch)
  unsigned *d_qcount = nullptr, *d_qoff = nullptr;
  unsigned long long *d_total = nullptr, *d_first = nullptr;
};

bool match_shape_ok(size_t n_train, size_t n, int kp_cap, int max_dist) {
  return n <= (1u << 24) && kp_cap >= 1 && kp_cap <= (1 << kQueryBits) && max_dist >= 0 && max_dist <= 256 &&
         n_train <= (1u << 20) && (unsigned long long)kp_cap * std::max<size_t>(n_train, 1) < (1ull << 32);
}

// counting pass + scans; `first` (host, n + 1) is complete when this returns (it synchronises the stream)
int match_count(Scratch& scratch, MatchState& st, const uint8_t* d_train, size_t n_train, const uint8_t* d_desc,
                const uint32_t* d_counts, size_t n, int kp_cap, int max_dist, uint64_t* first, hipStream_t s,
                const TSet* d_tsets = nullptr) {
  if (n_train == 0) {
    std::fill(first, first + n + 1, (uint64_t)0);
    return CBH_OK;
  }
  const size_t slots = n * (size_t)kp_cap;
  hipError_t e = scratch.get(&st.d_qcount, slots * sizeof(unsigned));
  if (e == hipSuccess) e = scratch.get(&st.d_qoff, slots * sizeof(unsigned));
  if (e == hipSuccess) e = scratch.get(&st.d_total, n * sizeof(unsigned long long));
  if (e == hipSuccess) e = scratch.get(&st.d_first, (n + 1) * sizeof(unsigned long long));
  if (e != hipSuccess) return fail("descriptor match scratch", e);
  const unsigned tiles = ((unsigned)kp_cap + kBlock - 1) / kBlock;
  for (size_t i0 = 0; i0 < n; i0 += 65535) {
    const unsigned m = (unsigned)std::min<size_t>(65535, n - i0);
    if (d_tsets)  // the grouped chain: a train set per candidate (tmpairs.hip)
      launch_tm_match_pairs(false, tiles, m, s, d_train, d_tsets, d_desc, d_counts, (unsigned)kp_cap, (unsigned)max_dist,
                            (unsigned)i0, st.d_qcount, nullptr, nullptr, 0ull, 0u, nullptr, 0ull);
    else
      hipLaunchKernelGGL(k_tm_match<false>, dim3(tiles, m), dim3(kBlock), 0, s, (const uint4*)d_train, (unsigned)n_train,
                         (const uint4*)d_desc, d_counts, (unsigned)kp_cap, (unsigned)max_dist, (unsigned)i0, st.d_qcount,
                         (const unsigned*)nullptr, (const unsigned long long*)nullptr, 0ull, 0u,
                         (unsigned long long*)nullptr, 0ull);
  }
  for (size_t i0 = 0; i0 < n; i0 += 1u << 20)
    hipLaunchKernelGGL(k_tm_scan_queries, dim3((unsigned)std::min<size_t>(1u << 20, n - i0)), dim3(kBlock), 0, s, st.d_qcount,
                       d_counts, (unsigned)kp_cap, (unsigned)i0, st.d_qoff, st.d_total);
  hipLaunchKernelGGL(k_tm_scan_first, dim3(1), dim3(kBlock), 0, s, st.d_total, (unsigned)n, st.d_first);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(first, st.d_first, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return e == hipSuccess ? CBH_OK : fail("descriptor match count", e);
}

// emitting pass, the sort and the gather for first[n] pairs (the lists have room for them)
int match_emit(const MatchState& st, const uint8_t* d_train, size_t n_train, const float* d_tmpl_xy, const uint8_t* d_desc,
               const float* d_xy, const uint32_t* d_counts, size_t n, int kp_cap, int max_dist, const uint64_t* first,
               cbh_dmatch* d_records, float* d_tmpl_pts, float* d_match_pts, hipStream_t s,
               const TSet* d_tsets = nullptr) {
  if (first[n] == 0) return CBH_OK;
  const unsigned tiles = ((unsigned)kp_cap + kBlock - 1) / kBlock;
  const size_t most = std::min<size_t>(65535, ((size_t)1 << kQueryBits) / (size_t)kp_cap);
  for (size_t g0 = 0; g0 < n;) {
    size_t g1 = g0 + 1;
    while (g1 < n && g1 - g0 < most && first[g1 + 1] - first[g0] <= kGroupKeys) ++g1;
    const unsigned long long cnt = first[g1] - first[g0];
    if (cnt) {
      Scratch scratch(s);
      unsigned long long* d_keys = nullptr;
      hipError_t e = scratch.get(&d_keys, cnt * sizeof(unsigned long long));
      if (e != hipSuccess) return fail("descriptor match keys", e);
      if (d_tsets)
        launch_tm_match_pairs(true, tiles, (unsigned)(g1 - g0), s, d_train, d_tsets, d_desc, d_counts, (unsigned)kp_cap,
                              (unsigned)max_dist, (unsigned)g0, nullptr, st.d_qoff, st.d_first, (unsigned long long)first[g0],
                              (unsigned)g0, d_keys, cnt);
      else
        hipLaunchKernelGGL(k_tm_match<true>, dim3(tiles, (unsigned)(g1 - g0)), dim3(kBlock), 0, s, (const uint4*)d_train,
                           (unsigned)n_train, (const uint4*)d_desc, d_counts, (unsigned)kp_cap, (unsigned)max_dist, (unsigned)g0,
                           (unsigned*)nullptr, (const unsigned*)st.d_qoff, (const unsigned long long*)st.d_first,
                           (unsigned long long)first[g0], (unsigned)g0, d_keys, cnt);
      if ((e = hipGetLastError()) != hipSuccess) return fail("descriptor match", e);
      int bits = 0;
      while (((size_t)1 << bits) < (g1 - g0) * (size_t)kp_cap) ++bits;
      const int rc = sort_keys_u64(d_keys, (size_t)cnt, 41 + bits, s);
      if (rc != CBH_OK) return rc;
      hipLaunchKernelGGL(k_tm_gather, dim3((unsigned)((cnt + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_keys, cnt,
                         (unsigned long long)first[g0], (unsigned)g0, (unsigned)kp_cap, (const float2*)d_tmpl_xy,
                         (const float2*)d_xy, (float2*)d_tmpl_pts, (float2*)d_match_pts, d_records, d_tsets);
      if ((e = hipGetLastError()) != hipSuccess) return fail("point gather", e);
    }
    g0 = g1;
  }
  return CBH_OK;
}

// ---- the chain ----------------------------------------------------------------------------------------------------------
bool params_ok(const cbh_tm_params* p) {
  return p && p->needle_features >= 0 && p->needle_features <= 100000 && p->haystack_features >= 0 &&
         p->haystack_features <= 100000 && p->cv_thresh >= 0 && p->cv_thresh <= 256 && p->tm_scale_pct >= 0;
}

// :182-192 and sizeScaleFactor's sizes: *dw == 0 or *dh == 0 where cv::resize would throw
void cand_target(int tw, int th, int w, int h, int pct, float* scale, int* dw, int* dh, bool* resized) {
  *scale = 1.f, *dw = w, *dh = h, *resized = false;
  if ((long long)th * tw < (long long)h * w) {
    const int cSize = std::max(w, h), tSize = std::max(th, tw);
    const int maxSize = (int)(tSize * pct / 100.0);
    if (cSize > maxSize) {
      *scale = (float)maxSize / cSize;
      *dw = (int)(w * *scale), *dh = (int)(h * *scale);
      *resized = true;
    }
  }
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// ORB of m grey images with room that grows until every count fits (cbird_amd/orb.py's loop); the outputs are blocks of
// `scratch`, counts (host, m) complete on return.  Synchronises the stream.
struct OrbOut {
  cbh_keypoint* d_kp = nullptr;
  float* d_after = nullptr;
  uint8_t* d_desc = nullptr;
  uint32_t* d_counts = nullptr;
  int kp_cap = 0;
};
int orb_until_it_fits(std::vector<std::unique_ptr<Scratch>>& held, OrbOut& o, const uint8_t* d_gray, size_t m,
                      const uint64_t* off, const uint32_t* w, const uint32_t* h, const uint32_t* stride, int nfeatures,
                      uint32_t* counts, hipStream_t s) {
  int cap = nfeatures + 64;
  for (;;) {
    held.emplace_back(new Scratch(s));
    Scratch& scratch = *held.back();
    const size_t slots = m * (size_t)cap;
    hipError_t e = scratch.get(&o.d_kp, slots * sizeof(cbh_keypoint));
    if (e == hipSuccess) e = scratch.get(&o.d_after, slots * 2 * sizeof(float));
    if (e == hipSuccess) e = scratch.get(&o.d_desc, slots * 32);
    if (e == hipSuccess) e = scratch.get(&o.d_counts, m * sizeof(uint32_t));
    if (e != hipSuccess) return fail("template match ORB scratch", e);
    int rc = launch_orb(d_gray, m, off, w, h, stride, nfeatures, cap, o.d_kp, o.d_after, o.d_desc, o.d_counts, s);
    if (rc != CBH_OK) return rc;
    e = hipMemcpyAsync(counts, o.d_counts, m * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail("template match ORB", e);
    const uint32_t most = *std::max_element(counts, counts + m);
    o.kp_cap = cap;
    if (most <= (uint32_t)cap) return CBH_OK;
    held.pop_back();  // (behind the kernels that used it) and again with the room the counts ask for
    cap = (int)most;
  }
}

// the template's side of a call: its grey view and its ORB output, made once and used by every group
struct Template {
  const uint8_t* d_img;
  int tw, th, channels;
  size_t stride;
  std::vector<std::unique_ptr<Scratch>> held;
  OrbOut orb;
  uint32_t count = 0;
};

int prepare_template(Template& t, const cbh_tm_params* p, hipStream_t s) {
  const uint64_t off = 0;
  const uint32_t w = (uint32_t)t.tw, h = (uint32_t)t.th;
  uint32_t stride = (uint32_t)t.stride;
  const uint8_t* d_gray = t.d_img;
  std::vector<RImage> keep;
  if (t.channels != 1) {
    t.held.emplace_back(new Scratch(s));
    uint8_t* g = nullptr;
    hipError_t e = t.held.back()->get(&g, (size_t)w * h);
    if (e != hipSuccess) return fail("template grey", e);
    int rc = queue_gray(*t.held.back(), keep, t.d_img, 1, &off, &w, &h, &stride, t.channels, &off, g, s);
    if (rc != CBH_OK) {
      (void)hipStreamSynchronize(s);
      return rc;
    }
    d_gray = g, stride = w;
  }
  int rc = orb_until_it_fits(t.held, t.orb, d_gray, 1, &off, &w, &h, &stride, p->needle_features, &t.count, s);
  (void)hipStreamSynchronize(s);  // `keep` is leaving
  return rc;
}

cbh_tm_image_result blank_result() {
  cbh_tm_image_result r = {};
  r.r.score = INT_MAX;
  r.cand_scale = 1.f;
  return r;
}

// candidates i0 .. i0 + m of a call: everything from the resize to the statuses.  d_patches: NULL, or the patches of
// these m candidates.  Returns with the stream synchronised.
int run_group(const Template& t, const uint8_t* d_imgs, size_t m, const uint64_t* img_off, const uint32_t* img_w,
              const uint32_t* img_h, const uint32_t* img_row_stride, const cbh_tm_params* p, cbh_tm_image_result* results,
              uint8_t* d_patches, int device, hipStream_t s) {
  const int ch = t.channels;
  const size_t patch = (size_t)t.tw * t.th * ch;
  // 1. scales and target sizes; `live` = the candidates that go on (all but the empty resizes)
  std::vector<uint32_t> live;
  std::vector<uint64_t> src_off, woff, goff;
  std::vector<uint32_t> sw, sh, sst, ww, wh, wst;
  std::vector<uint8_t> copy;
  std::vector<float> scale;
  size_t work_bytes = 0, gray_bytes = 0;
  for (size_t i = 0; i < m; ++i) {
    cbh_tm_image_result& r = results[i];
    r = blank_result();
    int dw, dh;
    bool resized;
    cand_target(t.tw, t.th, (int)img_w[i], (int)img_h[i], p->tm_scale_pct, &r.cand_scale, &dw, &dh, &resized);
    r.w = dw, r.h = dh;
    if (t.count == 0) {
      r.status = CBH_TM_NO_TEMPLATE_KEYPOINTS;  // :127-130, before any candidate is looked at
      r.cand_scale = 1.f, r.w = (int)img_w[i], r.h = (int)img_h[i];
      continue;
    }
    if (dw <= 0 || dh <= 0) {
      r.status = CBH_TM_EMPTY_RESIZE;
      continue;
    }
    if (dw > 8192 || dh > 8192) return CBH_E_INVAL;  // ORB's limit (cbh_orb_dev)
    live.push_back((uint32_t)i);
    src_off.push_back(img_off[i]), sw.push_back(img_w[i]), sh.push_back(img_h[i]), sst.push_back(img_row_stride[i]);
    ww.push_back((uint32_t)dw), wh.push_back((uint32_t)dh), wst.push_back((uint32_t)dw * ch);
    copy.push_back(resized ? 0 : 1), scale.push_back(r.cand_scale);
    woff.push_back(work_bytes), goff.push_back(gray_bytes);
    work_bytes += align16((size_t)dw * dh * ch), gray_bytes += align16((size_t)dw * dh);
  }
  const size_t k = live.size();
  // the warp stores 16-byte vectors: a group that starts inside the caller's patches off that grid, or that skips
  // candidates, warps into scratch and copies
  const bool staged = d_patches && (k != m || ((uintptr_t)d_patches & 15));
  if (d_patches && k != m) {
    hipError_t e = hipMemsetAsync(d_patches, 0, m * patch, s);
    if (e != hipSuccess) return fail("template match patches", e);
  }
  if (k == 0) {
    hipError_t e = hipStreamSynchronize(s);
    return e == hipSuccess ? CBH_OK : fail("template match", e);
  }
  Scratch scratch(s);
  ResizeTables rkeep;
  std::vector<RImage> gkeep;
  std::vector<std::unique_ptr<Scratch>> held;
  std::vector<uint32_t> counts(k);
  std::vector<uint64_t> first(k + 1);
  std::vector<cbh_template_result> res(k);
  uint8_t *d_work = nullptr, *d_gray = nullptr, *d_p = nullptr;
  cbh_template_result* d_res = nullptr;
  float *d_tp = nullptr, *d_mp = nullptr;
  OrbOut orb;
  MatchState st;
  int rc = CBH_OK;
  hipError_t e = scratch.get(&d_work, work_bytes);
  if (e == hipSuccess && ch != 1) e = scratch.get(&d_gray, gray_bytes);
  if (e == hipSuccess) e = scratch.get(&d_res, k * sizeof(cbh_template_result));
  if (e == hipSuccess && staged) e = scratch.get(&d_p, k * patch);
  if (e != hipSuccess) return fail("template match images scratch", e);
  // 3. the working images: resized, or copied as they are, packed at 16-byte offsets
  rc = queue_resize(scratch, rkeep, d_imgs, k, src_off.data(), sw.data(), sh.data(), sst.data(), ch, woff.data(), ww.data(),
                    wh.data(), copy.data(), d_work, s);
  // 2b. their grey views
  if (rc == CBH_OK && ch != 1)
    rc = queue_gray(scratch, gkeep, d_work, k, woff.data(), ww.data(), wh.data(), wst.data(), ch, goff.data(), d_gray, s);
  // 4. ORB on all of them
  if (rc == CBH_OK)
    rc = orb_until_it_fits(held, orb, ch == 1 ? d_work : d_gray, k, ch == 1 ? woff.data() : goff.data(), ww.data(), wh.data(),
                           ww.data(), p->haystack_features, counts.data(), s);
  // 5. match, gather, score
  if (rc == CBH_OK)
    rc = match_shape_ok(t.count, k, orb.kp_cap, p->cv_thresh) ? CBH_OK : CBH_E_INVAL;
  if (rc == CBH_OK)
    rc = match_count(scratch, st, t.orb.d_desc, t.count, orb.d_desc, orb.d_counts, k, orb.kp_cap, p->cv_thresh, first.data(),
                     s);
  if (rc == CBH_OK) {
    const size_t pts = std::max<uint64_t>(first[k], 1) * 2 * sizeof(float);
    if ((e = scratch.get(&d_tp, pts)) != hipSuccess || (e = scratch.get(&d_mp, pts)) != hipSuccess)
      rc = fail("template match point lists", e);
  }
  if (rc == CBH_OK)
    rc = match_emit(st, t.orb.d_desc, t.count, t.orb.d_after, orb.d_desc, orb.d_after, orb.d_counts, k, orb.kp_cap,
                    p->cv_thresh, first.data(), nullptr, d_tp, d_mp, s);
  if (rc == CBH_OK)
    rc = cbh_template_match_dev(t.d_img, t.tw, t.th, t.stride, ch, d_work, k, woff.data(), ww.data(), wh.data(), wst.data(), ch,
                                d_tp, d_mp, first.data(), scale.data(), d_res, staged ? d_p : d_patches,
                                device, s);
  if (rc == CBH_OK) {
    e = hipMemcpyAsync(res.data(), d_res, k * sizeof(cbh_template_result), hipMemcpyDeviceToHost, s);
    for (size_t j = 0; j < k && e == hipSuccess && d_p; ++j)
      e = hipMemcpyAsync(d_patches + live[j] * patch, d_p + j * patch, patch, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) rc = fail("template match images fetch", e);
  }
  e = hipStreamSynchronize(s);  // the host tables of this group are leaving
  if (rc == CBH_OK && e != hipSuccess) rc = fail("template match images", e);
  if (rc != CBH_OK) return rc;
  // 6. the statuses: the exits of the reference's loop, in its order
  for (size_t j = 0; j < k; ++j) {
    cbh_tm_image_result& r = results[live[j]];
    r.r = res[j];
    r.n_keypoints = counts[j];
    r.n_matches = (uint32_t)std::min<uint64_t>(first[j + 1] - first[j], 0xffffffffu);
    r.status = counts[j] == 0      ? CBH_TM_NO_KEYPOINTS
               : r.n_matches == 0  ? CBH_TM_NO_MATCHES
               : r.n_matches < 3   ? CBH_TM_FEW_POINTS
               : !r.r.found        ? CBH_TM_NO_TRANSFORM
                                   : CBH_TM_SCORED;
  }
  return CBH_OK;
}

bool images_args_ok(const void* tmpl, int tw, int th, size_t tstride, const void* imgs, const uint64_t* off,
                    const uint32_t* w, const uint32_t* h, const uint32_t* stride, size_t n, int channels,
                    const cbh_tm_params* p, const void* results) {
  if (!tmpl || !imgs || !off || !w || !h || !stride || !results || !channels_ok(channels) || !params_ok(p) || tw < 1 ||
      th < 1 || tw > 8192 || th > 8192 || tstride < (size_t)tw * channels || tstride > 0xffffffffull || n > (1u << 24))
    return false;
  for (size_t i = 0; i < n; ++i)
    if (!image_ok(w[i], h[i], stride[i], channels)) return false;
  return true;
}

// runs of candidates whose bytes span at most "tmatch_chunk_mb" (at least one candidate, at most 32768)
std::vector<Run> candidate_runs(size_t n, const uint64_t* off, const uint32_t* w, const uint32_t* h, const uint32_t* stride,
                                int channels) {
  std::vector<uint64_t> end(n);
  for (size_t i = 0; i < n; ++i) end[i] = image_end(off[i], w[i], h[i], stride[i], channels);
  return make_runs(n, off, end.data(), (uint64_t)std::max(get_tmatch_chunk_mb(), 1) << 20, 32768);
}

// ---- the grouped chain: (template image, candidate image) pairs over one image table --------------------------------
// Device-event times of the stages of the last grouped call, kept only while cbh_tm_pairs_stage_ms has asked for them.
struct StageClock {
  bool on = false;
  double ms[5] = {0, 0, 0, 0, 0};  // grey, ORB of the templates, ORB of the candidates, match + gather, estimate to score
  unsigned sizes = 0, hash_launches = 0;
};
StageClock g_clock;
struct StageTimer {  // brackets one stage with two events; read (a host wait) only when the clock is on
  hipStream_t s;
  int stage;
  hipEvent_t a = nullptr, b = nullptr;
  StageTimer(hipStream_t stream, int st) : s(stream), stage(st) {
    if (g_clock.on && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) (void)hipEventRecord(a, s);
  }
  void stop() {
    if (!a || !b) return;
    float ms = 0.f;
    if (hipEventRecord(b, s) == hipSuccess && hipEventSynchronize(b) == hipSuccess &&
        hipEventElapsedTime(&ms, a, b) == hipSuccess)
      g_clock.ms[stage] += ms;
  }
  ~StageTimer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

struct PairRef {
  uint32_t tmpl, cand, out;  // indexes of the image table; results[out]
};

// m pairs whose equal templates are adjacent: the distinct templates go through grey and ONE ragged ORB, the candidates
// through resize / grey / ONE ragged ORB, then one grouped match and template_match_pairs_tail.  The host waits are the
// two ORB counts, `first` and the results, whatever the number of templates.  Returns with the stream synchronised.
int run_pairs(const uint8_t* d_imgs, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
              const uint32_t* img_row_stride, int ch, const PairRef* pairs, size_t m, const cbh_tm_params* p,
              cbh_tm_image_result* results, hipStream_t s) {
  // 1. the distinct templates
  std::vector<uint32_t> slot(m);
  std::vector<uint64_t> toff, tgoff;
  std::vector<uint32_t> tw, th, tst, tgst;
  size_t tgray_bytes = 0;
  for (size_t j = 0; j < m; ++j) {
    if (j == 0 || pairs[j].tmpl != pairs[j - 1].tmpl) {
      const uint32_t t = pairs[j].tmpl;
      toff.push_back(img_off[t]), tw.push_back(img_w[t]), th.push_back(img_h[t]), tst.push_back(img_row_stride[t]);
      tgoff.push_back(tgray_bytes), tgst.push_back(img_w[t]);
      tgray_bytes += align16((size_t)img_w[t] * img_h[t]);
    }
    slot[j] = (uint32_t)toff.size() - 1;
  }
  const size_t G = toff.size();
  Scratch tscratch(s);
  std::vector<RImage> tkeep;
  std::vector<std::unique_ptr<Scratch>> theld;
  std::vector<uint32_t> tcounts(G);
  OrbOut torb;
  int rc = CBH_OK;
  hipError_t e = hipSuccess;
  {
    uint8_t* d_tgray = nullptr;
    StageTimer grey(s, 0);
    if (ch != 1) {
      if ((e = tscratch.get(&d_tgray, tgray_bytes)) != hipSuccess) return fail("template match pairs grey", e);
      rc = queue_gray(tscratch, tkeep, d_imgs, G, toff.data(), tw.data(), th.data(), tst.data(), ch, tgoff.data(), d_tgray, s);
    }
    grey.stop();
    StageTimer orb(s, 1);
    if (rc == CBH_OK)
      rc = orb_until_it_fits(theld, torb, ch == 1 ? d_imgs : d_tgray, G, ch == 1 ? toff.data() : tgoff.data(), tw.data(),
                             th.data(), ch == 1 ? tst.data() : tgst.data(), p->needle_features, tcounts.data(), s);
    orb.stop();
    if (rc != CBH_OK) {
      (void)hipStreamSynchronize(s);  // `tkeep` is leaving
      return rc;
    }
  }
  // 2. scales and target sizes per pair; `live` = the pairs that go on
  std::vector<uint32_t> live;
  std::vector<uint64_t> src_off, woff, goff;
  std::vector<uint32_t> sw, sh, sst, ww, wh, wst;
  std::vector<uint8_t> copy;
  std::vector<float> scale;
  std::vector<TSet> tsets;
  std::vector<TmplGeom> geom;
  size_t work_bytes = 0, gray_bytes = 0, n_train = 0;
  for (size_t j = 0; j < m; ++j) {
    cbh_tm_image_result& r = results[pairs[j].out];
    const uint32_t c = pairs[j].cand, g = slot[j];
    r = blank_result();
    int dw, dh;
    bool resized;
    cand_target((int)tw[g], (int)th[g], (int)img_w[c], (int)img_h[c], p->tm_scale_pct, &r.cand_scale, &dw, &dh, &resized);
    r.w = dw, r.h = dh;
    if (tcounts[g] == 0) {
      r.status = CBH_TM_NO_TEMPLATE_KEYPOINTS;
      r.cand_scale = 1.f, r.w = (int)img_w[c], r.h = (int)img_h[c];
      continue;
    }
    if (dw <= 0 || dh <= 0) {
      r.status = CBH_TM_EMPTY_RESIZE;
      continue;
    }
    if (dw > 8192 || dh > 8192) return CBH_E_INVAL;  // ORB's limit (the stream is idle: orb_until_it_fits waited)
    live.push_back((uint32_t)j);
    src_off.push_back(img_off[c]), sw.push_back(img_w[c]), sh.push_back(img_h[c]), sst.push_back(img_row_stride[c]);
    ww.push_back((uint32_t)dw), wh.push_back((uint32_t)dh), wst.push_back((uint32_t)dw * ch);
    copy.push_back(resized ? 0 : 1), scale.push_back(r.cand_scale);
    woff.push_back(work_bytes), goff.push_back(gray_bytes);
    work_bytes += align16((size_t)dw * dh * ch), gray_bytes += align16((size_t)dw * dh);
    tsets.push_back({(unsigned)(g * (size_t)torb.kp_cap), tcounts[g]});
    geom.push_back({toff[g], tw[g], th[g], tst[g]});
    n_train = std::max<size_t>(n_train, tcounts[g]);
  }
  const size_t k = live.size();
  if (k == 0) return CBH_OK;
  if (G * (size_t)torb.kp_cap >= (1ull << 32)) return CBH_E_INVAL;  // (a TSet's base is 32 bits)
  Scratch scratch(s);
  ResizeTables rkeep;
  std::vector<RImage> gkeep;
  std::vector<std::unique_ptr<Scratch>> held;
  std::vector<uint32_t> counts(k);
  std::vector<uint64_t> first(k + 1);
  std::vector<cbh_template_result> res(k);
  uint8_t *d_work = nullptr, *d_gray = nullptr;
  float *d_tp = nullptr, *d_mp = nullptr;
  TSet* d_tsets = nullptr;
  OrbOut orb;
  MatchState st;
  e = scratch.get(&d_work, work_bytes);
  if (e == hipSuccess && ch != 1) e = scratch.get(&d_gray, gray_bytes);
  if (e == hipSuccess) e = upload(scratch, &d_tsets, tsets, s);
  if (e != hipSuccess) rc = fail("template match pairs scratch", e);
  {
    StageTimer grey(s, 0);
    if (rc == CBH_OK)
      rc = queue_resize(scratch, rkeep, d_imgs, k, src_off.data(), sw.data(), sh.data(), sst.data(), ch, woff.data(), ww.data(),
                        wh.data(), copy.data(), d_work, s);
    if (rc == CBH_OK && ch != 1)
      rc = queue_gray(scratch, gkeep, d_work, k, woff.data(), ww.data(), wh.data(), wst.data(), ch, goff.data(), d_gray, s);
    grey.stop();
  }
  {
    StageTimer t(s, 2);
    if (rc == CBH_OK)
      rc = orb_until_it_fits(held, orb, ch == 1 ? d_work : d_gray, k, ch == 1 ? woff.data() : goff.data(), ww.data(), wh.data(),
                             ww.data(), p->haystack_features, counts.data(), s);
    t.stop();
  }
  {
    StageTimer t(s, 3);
    if (rc == CBH_OK) rc = match_shape_ok(n_train, k, orb.kp_cap, p->cv_thresh) ? CBH_OK : CBH_E_INVAL;
    if (rc == CBH_OK)
      rc = match_count(scratch, st, torb.d_desc, n_train, orb.d_desc, orb.d_counts, k, orb.kp_cap, p->cv_thresh, first.data(), s,
                       d_tsets);
    if (rc == CBH_OK) {
      const size_t pts = std::max<uint64_t>(first[k], 1) * 2 * sizeof(float);
      if ((e = scratch.get(&d_tp, pts)) != hipSuccess || (e = scratch.get(&d_mp, pts)) != hipSuccess)
        rc = fail("template match pairs point lists", e);
    }
    if (rc == CBH_OK)
      rc = match_emit(st, torb.d_desc, n_train, torb.d_after, orb.d_desc, orb.d_after, orb.d_counts, k, orb.kp_cap, p->cv_thresh,
                      first.data(), nullptr, d_tp, d_mp, s, d_tsets);
    t.stop();
  }
  {
    StageTimer t(s, 4);
    if (rc == CBH_OK)
      rc = template_match_pairs_tail(d_imgs, geom.data(), d_work, k, woff.data(), ww.data(), wh.data(), wst.data(), ch, d_tp,
                                     d_mp, first.data(), scale.data(), res.data(), g_clock.on ? &g_clock.hash_launches : nullptr,
                                     s);
    t.stop();
  }
  e = hipStreamSynchronize(s);  // the host tables of this chunk are leaving
  if (rc == CBH_OK && e != hipSuccess) rc = fail("template match pairs", e);
  if (rc != CBH_OK) return rc;
  if (g_clock.on)
    for (size_t j = 0; j < k; ++j)
      if (j == 0 || geom[j].tw != geom[j - 1].tw || geom[j].th != geom[j - 1].th) ++g_clock.sizes;
  for (size_t j = 0; j < k; ++j) {
    cbh_tm_image_result& r = results[pairs[live[j]].out];
    r.r = res[j];
    r.n_keypoints = counts[j];
    r.n_matches = (uint32_t)std::min<uint64_t>(first[j + 1] - first[j], 0xffffffffu);
    r.status = counts[j] == 0      ? CBH_TM_NO_KEYPOINTS
               : r.n_matches == 0  ? CBH_TM_NO_MATCHES
               : r.n_matches < 3   ? CBH_TM_FEW_POINTS
               : !r.r.found        ? CBH_TM_NO_TRANSFORM
                                   : CBH_TM_SCORED;
  }
  return CBH_OK;
}

bool pairs_args_ok(const void* imgs, size_t n_imgs, const uint64_t* off, const uint32_t* w, const uint32_t* h,
                   const uint32_t* stride, int channels, const uint32_t* pt, const uint32_t* pc, size_t n_pairs,
                   const cbh_tm_params* p, const void* results) {
  if (!imgs || !off || !w || !h || !stride || !pt || !pc || !results || !channels_ok(channels) || !params_ok(p) ||
      n_imgs > (1u << 24) || n_pairs > (1u << 24))
    return false;
  for (size_t i = 0; i < n_imgs; ++i)
    if (!image_ok(w[i], h[i], stride[i], channels)) return false;
  for (size_t j = 0; j < n_pairs; ++j)
    if (pt[j] >= n_imgs || pc[j] >= n_imgs || w[pt[j]] > 8192 || h[pt[j]] > 8192) return false;  // ORB's limit: the template
  return true;
}

// The caller's pairs in the order the chain works in -- by template size (runs of one hash geometry), then template, then
// the caller's order -- cut into chunks whose working set (the templates once, each pair's candidate image and its
// patch) stays within "tmatch_chunk_mb": make_runs over the running sum of those bytes.
struct PairPlan {
  std::vector<PairRef> pairs;
  std::vector<Run> runs;
};
PairPlan plan_pairs(const uint32_t* w, const uint32_t* h, const uint32_t* stride, int channels, const uint32_t* pt,
                    const uint32_t* pc, size_t n_pairs) {
  PairPlan plan;
  plan.pairs.resize(n_pairs);
  for (size_t j = 0; j < n_pairs; ++j) plan.pairs[j] = {pt[j], pc[j], (uint32_t)j};
  std::sort(plan.pairs.begin(), plan.pairs.end(), [&](const PairRef& a, const PairRef& b) {
    if (w[a.tmpl] != w[b.tmpl]) return w[a.tmpl] < w[b.tmpl];
    if (h[a.tmpl] != h[b.tmpl]) return h[a.tmpl] < h[b.tmpl];
    if (a.tmpl != b.tmpl) return a.tmpl < b.tmpl;
    return a.out < b.out;
  });
  std::vector<uint64_t> lo(n_pairs), hi(n_pairs);
  uint64_t at = 0;
  for (size_t j = 0; j < n_pairs; ++j) {
    const PairRef& r = plan.pairs[j];
    lo[j] = at;
    at += (uint64_t)h[r.cand] * stride[r.cand] + (uint64_t)w[r.tmpl] * h[r.tmpl] * channels;
    if (j == 0 || plan.pairs[j - 1].tmpl != r.tmpl) at += (uint64_t)h[r.tmpl] * stride[r.tmpl];
    hi[j] = at;
  }
  plan.runs = make_runs(n_pairs, lo.data(), hi.data(), (uint64_t)std::max(get_tmatch_chunk_mb(), 1) << 20, 32768);
  return plan;
}

}  // namespace
}  // namespace cbh

extern "C" {

int cbh_tm_pairs_stage_ms(int on, double* ms5, uint32_t* sizes, uint32_t* hash_launches) {
  if (ms5) std::copy(cbh::g_clock.ms, cbh::g_clock.ms + 5, ms5);
  if (sizes) *sizes = cbh::g_clock.sizes;
  if (hash_launches) *hash_launches = cbh::g_clock.hash_launches;
  cbh::g_clock = cbh::StageClock();
  cbh::g_clock.on = on != 0;
  return CBH_OK;
}

int cbh_template_match_pairs_dev(const void* d_imgs, size_t n_imgs, const uint64_t* img_off, const uint32_t* img_w,
                                 const uint32_t* img_h, const uint32_t* img_row_stride, int channels,
                                 const uint32_t* pair_tmpl, const uint32_t* pair_cand, size_t n_pairs,
                                 const cbh_tm_params* params, cbh_tm_image_result* results, int device, void* stream) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n_pairs == 0) return CBH_OK;
  if (!cbh::pairs_args_ok(d_imgs, n_imgs, img_off, img_w, img_h, img_row_stride, channels, pair_tmpl, pair_cand, n_pairs,
                          params, results))
    return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  const cbh::PairPlan plan = cbh::plan_pairs(img_w, img_h, img_row_stride, channels, pair_tmpl, pair_cand, n_pairs);
  for (const cbh::Run& r : plan.runs) {
    const int rc = cbh::run_pairs((const uint8_t*)d_imgs, img_off, img_w, img_h, img_row_stride, channels,
                                  plan.pairs.data() + r.i0, r.m, params, results, s);
    if (rc != CBH_OK) return rc;
  }
  return CBH_OK;
}

int cbh_template_match_pairs(const uint8_t* imgs, size_t imgs_bytes, size_t n_imgs, const uint64_t* img_off,
                             const uint32_t* img_w, const uint32_t* img_h, const uint32_t* img_row_stride, int channels,
                             const uint32_t* pair_tmpl, const uint32_t* pair_cand, size_t n_pairs,
                             const cbh_tm_params* params, cbh_tm_image_result* results, int device) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n_pairs == 0) return CBH_OK;
  if (!cbh::pairs_args_ok(imgs, n_imgs, img_off, img_w, img_h, img_row_stride, channels, pair_tmpl, pair_cand, n_pairs, params,
                          results))
    return CBH_E_INVAL;
  for (size_t i = 0; i < n_imgs; ++i)
    if (cbh::image_end(img_off[i], img_w[i], img_h[i], img_row_stride[i], channels) > imgs_bytes) return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  const cbh::PairPlan plan = cbh::plan_pairs(img_w, img_h, img_row_stride, channels, pair_tmpl, pair_cand, n_pairs);
  // What a chunk uploads: the images its pairs name, each once.  They go up in ascending host order, and neighbours
  // (the next one starts within 64 bytes of the bytes taken so far: a packed table) in ONE copy that keeps their distances;
  // the copies are packed at 16-byte offsets.  `upload` false: only the bytes the chunk needs on the device.
  std::vector<uint64_t> off(n_imgs);
  std::vector<uint32_t> seen(n_imgs, 0xffffffffu), ids;
  auto span = [&](uint32_t i) {
    return (size_t)(cbh::image_end(img_off[i], img_w[i], img_h[i], img_row_stride[i], channels) - img_off[i]);
  };
  cbh::Staging st("template match pairs");
  uint8_t* d_imgs = nullptr;
  auto lay_out = [&](size_t k, bool upload) {
    const cbh::Run& r = plan.runs[k];
    const uint32_t mark = (uint32_t)(2 * k + (upload ? 1 : 0));
    ids.clear();
    for (size_t j = r.i0; j < r.i0 + r.m; ++j)
      for (uint32_t i : {plan.pairs[j].tmpl, plan.pairs[j].cand})
        if (seen[i] != mark) seen[i] = mark, ids.push_back(i);
    std::sort(ids.begin(), ids.end(), [&](uint32_t x, uint32_t y) { return img_off[x] < img_off[y]; });
    size_t at = 0;
    for (size_t a = 0; a < ids.size();) {
      const uint64_t lo = img_off[ids[a]];
      uint64_t hi = lo + span(ids[a]);
      size_t b = a + 1;
      while (b < ids.size() && img_off[ids[b]] <= hi + 64) hi = std::max<uint64_t>(hi, img_off[ids[b]] + span(ids[b])), ++b;
      if (upload) {
        for (size_t c = a; c < b; ++c) off[ids[c]] = at + (img_off[ids[c]] - lo);
        st.up(d_imgs + at, imgs + lo, (size_t)(hi - lo));
      }
      at += cbh::align16((size_t)(hi - lo));
      a = b;
    }
    return at;
  };
  size_t most = 0;
  for (size_t k = 0; k < plan.runs.size(); ++k) most = std::max(most, lay_out(k, false));
  st.alloc(&d_imgs, most);
  int rc = st.status();
  for (size_t k = 0; k < plan.runs.size() && rc == CBH_OK; ++k) {
    const cbh::Run& r = plan.runs[k];
    // (the chunk before has finished: run_pairs returns with the stream synchronised)
    lay_out(k, true);
    if ((rc = st.status()) != CBH_OK) break;
    rc = cbh::run_pairs(d_imgs, off.data(), img_w, img_h, img_row_stride, channels, plan.pairs.data() + r.i0, r.m, params,
                        results, st.s);
  }
  return rc;
}

int cbh_tm_match_points_pairs_dev(const void* d_tmpl_desc, const void* d_tmpl_xy, const uint64_t* tmpl_first, size_t n_tmpl,
                                  const uint32_t* tmpl_of, const void* d_desc, const void* d_xy, const void* d_counts,
                                  size_t n, int kp_cap, int max_dist, void* d_records, void* d_tmpl_pts, void* d_match_pts,
                                  size_t points_cap, uint64_t* first, int device, void* stream) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) {
    if (first) first[0] = 0;
    return CBH_OK;
  }
  if (!first || !d_desc || !d_xy || !d_counts || !tmpl_first || !tmpl_of || n_tmpl == 0 || n_tmpl > (1u << 24) ||
      (points_cap && (!d_tmpl_pts || !d_match_pts)) || tmpl_first[0] != 0)
    return CBH_E_INVAL;
  size_t n_train = 0;
  for (size_t g = 0; g < n_tmpl; ++g) {
    if (tmpl_first[g + 1] < tmpl_first[g] || tmpl_first[g + 1] >= (1ull << 32)) return CBH_E_INVAL;
    n_train = std::max<size_t>(n_train, tmpl_first[g + 1] - tmpl_first[g]);
  }
  if ((tmpl_first[n_tmpl] && (!d_tmpl_desc || !d_tmpl_xy)) || !cbh::match_shape_ok(n_train, n, kp_cap, max_dist))
    return CBH_E_INVAL;
  std::vector<cbh::TSet> tsets(n);
  for (size_t i = 0; i < n; ++i) {
    if (tmpl_of[i] >= n_tmpl) return CBH_E_INVAL;
    tsets[i] = {(unsigned)tmpl_first[tmpl_of[i]], (unsigned)(tmpl_first[tmpl_of[i] + 1] - tmpl_first[tmpl_of[i]])};
  }
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  cbh::Scratch scratch(s);
  cbh::MatchState st;
  cbh::TSet* d_tsets = nullptr;
  hipError_t e = cbh::upload(scratch, &d_tsets, tsets, s);
  int rc = e == hipSuccess ? CBH_OK : cbh::fail("descriptor match tables", e);
  // (n_train = 0 fills `first` with zeros without a launch: every train set is empty)
  if (rc == CBH_OK)
    rc = cbh::match_count(scratch, st, (const uint8_t*)d_tmpl_desc, n_train, (const uint8_t*)d_desc, (const uint32_t*)d_counts, n,
                          kp_cap, max_dist, first, s, d_tsets);
  if (rc == CBH_OK && first[n] > points_cap) rc = CBH_E_OVERFLOW;  // `first` is complete; nothing has been written
  if (rc == CBH_OK)
    rc = cbh::match_emit(st, (const uint8_t*)d_tmpl_desc, n_train, (const float*)d_tmpl_xy, (const uint8_t*)d_desc,
                         (const float*)d_xy, (const uint32_t*)d_counts, n, kp_cap, max_dist, first, (cbh_dmatch*)d_records,
                         (float*)d_tmpl_pts, (float*)d_match_pts, s, d_tsets);
  e = hipStreamSynchronize(s);  // the host table must outlive its copy
  if (rc == CBH_OK && e != hipSuccess) rc = cbh::fail("descriptor match", e);
  return rc;
}

int cbh_resize_lanczos4_ragged_dev(const void* d_src, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                                   const uint32_t* img_h, const uint32_t* img_row_stride, int channels,
                                   const uint64_t* dst_off, const uint32_t* dst_w, const uint32_t* dst_h, void* d_dst,
                                   int device, void* stream) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) return CBH_OK;
  if (!d_src || !img_off || !img_w || !img_h || !img_row_stride || !dst_off || !dst_w || !dst_h || !d_dst ||
      !cbh::channels_ok(channels) || n > (1u << 24) || ((uintptr_t)d_dst & 15))
    return CBH_E_INVAL;
  for (size_t i = 0; i < n; ++i)
    if (!cbh::image_ok(img_w[i], img_h[i], img_row_stride[i], channels) || dst_w[i] < 1 || dst_h[i] < 1 ||
        dst_w[i] > 32767 || dst_h[i] > 32767 || (dst_off[i] & 15))
      return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  cbh::Scratch scratch(s);
  cbh::ResizeTables keep;
  int rc = cbh::queue_resize(scratch, keep, (const uint8_t*)d_src, n, img_off, img_w, img_h, img_row_stride, channels, dst_off,
                             dst_w, dst_h, nullptr, (uint8_t*)d_dst, s);
  hipError_t e = hipStreamSynchronize(s);  // the host tables must outlive their copies
  if (rc == CBH_OK && e != hipSuccess) rc = cbh::fail("ragged resize", e);
  return rc;
}

int cbh_bgr2gray_ragged_dev(const void* d_src, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                            const uint32_t* img_row_stride, int channels, const uint64_t* dst_off, void* d_dst, int device,
                            void* stream) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) return CBH_OK;
  if (!d_src || !img_off || !img_w || !img_h || !img_row_stride || !dst_off || !d_dst || (channels != 3 && channels != 4) ||
      n > (1u << 24) || ((uintptr_t)d_dst & 15))
    return CBH_E_INVAL;
  for (size_t i = 0; i < n; ++i)
    if (!cbh::image_ok(img_w[i], img_h[i], img_row_stride[i], channels) || (dst_off[i] & 15)) return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  cbh::Scratch scratch(s);
  std::vector<cbh::RImage> keep;
  int rc = cbh::queue_gray(scratch, keep, (const uint8_t*)d_src, n, img_off, img_w, img_h, img_row_stride, channels, dst_off,
                           (uint8_t*)d_dst, s);
  hipError_t e = hipStreamSynchronize(s);  // the host table must outlive its copy
  if (rc == CBH_OK && e != hipSuccess) rc = cbh::fail("ragged grey", e);
  return rc;
}

int cbh_tm_match_points_dev(const void* d_tmpl_desc, const void* d_tmpl_xy, size_t n_train, const void* d_desc,
                            const void* d_xy, const void* d_counts, size_t n, int kp_cap, int max_dist, void* d_records,
                            void* d_tmpl_pts, void* d_match_pts, size_t points_cap, uint64_t* first, int device,
                            void* stream) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) {
    if (first) first[0] = 0;
    return CBH_OK;
  }
  if (!first || !d_desc || !d_xy || !d_counts || (n_train && (!d_tmpl_desc || !d_tmpl_xy)) ||
      (points_cap && (!d_tmpl_pts || !d_match_pts)) || !cbh::match_shape_ok(n_train, n, kp_cap, max_dist))
    return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  cbh::Scratch scratch(s);
  cbh::MatchState st;
  int rc = cbh::match_count(scratch, st, (const uint8_t*)d_tmpl_desc, n_train, (const uint8_t*)d_desc,
                            (const uint32_t*)d_counts, n, kp_cap, max_dist, first, s);
  if (rc != CBH_OK) return rc;
  if (first[n] > points_cap) return CBH_E_OVERFLOW;  // `first` is complete; nothing has been written to the lists
  rc = cbh::match_emit(st, (const uint8_t*)d_tmpl_desc, n_train, (const float*)d_tmpl_xy, (const uint8_t*)d_desc,
                       (const float*)d_xy, (const uint32_t*)d_counts, n, kp_cap, max_dist, first, (cbh_dmatch*)d_records,
                       (float*)d_tmpl_pts, (float*)d_match_pts, s);
  hipError_t e = hipStreamSynchronize(s);
  if (rc == CBH_OK && e != hipSuccess) rc = cbh::fail("descriptor match", e);
  return rc;
}

int cbh_template_match_images_dev(const void* d_tmpl, int tw, int th, size_t tmpl_row_stride, const void* d_imgs, size_t n,
                                  const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                                  const uint32_t* img_row_stride, int channels, const cbh_tm_params* params,
                                  cbh_tm_image_result* results, void* d_patches, int device, void* stream) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) return CBH_OK;
  if (!cbh::images_args_ok(d_tmpl, tw, th, tmpl_row_stride, d_imgs, img_off, img_w, img_h, img_row_stride, n, channels,
                           params, results) ||
      ((uintptr_t)d_patches & 15))
    return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  cbh::Template t{(const uint8_t*)d_tmpl, tw, th, channels, tmpl_row_stride};
  int rc = cbh::prepare_template(t, params, s);
  if (rc != CBH_OK) return rc;
  const size_t patch = (size_t)tw * th * channels;
  for (const cbh::Run& r : cbh::candidate_runs(n, img_off, img_w, img_h, img_row_stride, channels)) {
    rc = cbh::run_group(t, (const uint8_t*)d_imgs, r.m, img_off + r.i0, img_w + r.i0, img_h + r.i0, img_row_stride + r.i0,
                        params, results + r.i0, d_patches ? (uint8_t*)d_patches + r.i0 * patch : nullptr, device, s);
    if (rc != CBH_OK) return rc;
  }
  return CBH_OK;
}

int cbh_template_match_images(const uint8_t* tmpl, int tw, int th, size_t tmpl_row_stride, const uint8_t* imgs,
                              size_t imgs_bytes, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                              const uint32_t* img_h, const uint32_t* img_row_stride, int channels,
                              const cbh_tm_params* params, cbh_tm_image_result* results, uint8_t* patches, int device) {
  if (!cbh::device_usable(device)) return CBH_E_NODEVICE;
  if (n == 0) return CBH_OK;
  if (!cbh::images_args_ok(tmpl, tw, th, tmpl_row_stride, imgs, img_off, img_w, img_h, img_row_stride, n, channels, params,
                           results))
    return CBH_E_INVAL;
  for (size_t i = 0; i < n; ++i)
    if (cbh::image_end(img_off[i], img_w[i], img_h[i], img_row_stride[i], channels) > imgs_bytes) return CBH_E_INVAL;
  cbh::DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  const std::vector<cbh::Run> runs = cbh::candidate_runs(n, img_off, img_w, img_h, img_row_stride, channels);
  size_t span = 0, most_m = 0;
  for (const cbh::Run& r : runs) span = std::max<size_t>(span, r.hi - r.lo), most_m = std::max(most_m, r.m);
  const size_t tspan = (size_t)(th - 1) * tmpl_row_stride + (size_t)tw * channels;
  const size_t patch = (size_t)tw * th * channels;
  cbh::Staging st("template match images");
  uint8_t *d_imgs, *d_tmpl, *d_patches = nullptr;
  st.alloc(&d_imgs, span);
  st.alloc(&d_tmpl, tspan);
  if (patches) st.alloc(&d_patches, most_m * patch);
  st.up(d_tmpl, tmpl, tspan);
  int rc = st.status();
  if (rc != CBH_OK) return rc;
  cbh::Template t{d_tmpl, tw, th, channels, tmpl_row_stride};
  rc = cbh::prepare_template(t, params, st.s);
  std::vector<uint64_t> off;
  for (size_t k = 0; k < runs.size() && rc == CBH_OK; ++k) {
    const cbh::Run& r = runs[k];
    cbh::rebase(r, img_off, &off);
    // (the run before has finished: run_group returns with the stream synchronised)
    st.up(d_imgs, imgs + r.lo, r.hi - r.lo);
    if ((rc = st.status()) != CBH_OK) break;
    rc = cbh::run_group(t, d_imgs, r.m, off.data(), img_w + r.i0, img_h + r.i0, img_row_stride + r.i0, params,
                        results + r.i0, d_patches, device, st.s);
    if (rc == CBH_OK && patches) {  // before the next run warps into d_patches
      st.down(patches + r.i0 * patch, d_patches, r.m * patch);
      st.sync();
      rc = st.status();
    }
  }
  (void)hipStreamSynchronize(st.s);  // before the template's scratch goes back
  return rc;
}

}  // extern "C"
