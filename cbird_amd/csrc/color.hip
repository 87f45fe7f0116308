// color.hip -- ColorDescIndex (src/colordescindex.{h,cpp}) and ColorDescriptor::distance
// (src/cvutil.cpp:682-749) on gfx950.
//
// Reference: a descriptor is 32 x {L,u,v,w : u16} + numColors : u8 (258 bytes, src/cvutil.h:57-113);
// find() is a linear scan of distance(target, desc[i]) over the whole index (colordescindex.cpp:250-278):
//   skip when either side has 0 colours or the counts differ by more than 2 (:683-684);
//   a := the side with more colours (:697-706); score = 1 + sum_{i<numA} min_{j<numB} |a_i - b_j|_2 in
//   float, colours decompressed as l=L*100/65535, u=U*354/65535-134, v=V*262/65535-140 (cvutil.h:83-87);
//   Match(id, int(score)) for id != 0, in index order.
//
// Layout: the index is stored decompressed and planar -- l/u/v[32][capacity] f32, num[capacity] u8 -- so that a
// wave reads each colour plane with unit stride (the 258-byte AoS record would give every lane its own cache
// line).  k_color_dist: one lane per haystack descriptor; the needle's (<= 32) colours are wave-uniform SGPR
// operands.  Per colour pair 3 sub, 3 mul, 2 add in the reference's association order (no FMA contraction:
// the library is built with -ffp-contract=off), one running minimum per needle colour and one per haystack
// colour (either side can be "a"); sqrtf is monotonic, so it is applied to the 32 minima instead of the 1024
// pair distances (bit-identical result), then summed in index order starting from 1.0f.

#include <atomic>
#include <cfloat>
#include <map>

#include "cbh_index.h"

namespace {

constexpr int kNC = 32;  // ColorDescriptor::NUM_DESC_COLORS
constexpr size_t kDescBytes = 258;

struct alignas(16) NeedleF {  // 400 bytes: k_color_dist3 reads the components as float4
  float l[kNC], u[kNC], v[kNC];
  int num;
};

// Launch geometry of the distance kernels: blockIdx.x = NEEDLE (fastest), blockIdx.y/z = haystack tile.  The
// workgroups that run together then share one tile: it comes from HBM once per XCD instead of once per needle (with
// the tile fastest, 64 needles re-streamed a 384 MB index 64 times -- 1.8 TB/s of traffic that held every variant of
// the kernel at ~14 ms whatever its instruction mix).
__device__ __forceinline__ uint32_t color_tile() { return blockIdx.y + blockIdx.z * 32768u; }



// Two haystack descriptors per lane on the packed-f32 ALU (v_pk_add_f32 / v_pk_mul_f32 work on two
// independent floats per lane and issue like one VALU op): per colour pair 3 pk sub + 3 pk mul + 2 pk add
// for both descriptors, then the minima per half.  Same operations in the same order as k_color_dist (no
// contraction: products and sums are rounded separately), so results are bit-identical; missing haystack
// colours are loaded as 1e18 so their distance (~3e36, finite) can never win a minimum -- one select less.
typedef float f2 __attribute__((ext_vector_type(2)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

// Missing colours on EITHER side are 1e18 in L (host: decompress_pad; device: the index planes are padded the
// same way), so a pair with a missing colour has a distance of ~1e36 (finite) that never wins a minimum and the
// loop needs no selects.  Squared distances are non-negative finite floats, whose order is the order of their
// bit patterns as unsigned integers: the minima are v_min_u32 / v_min3_u32 (no NaN canonicalisation ops).
__global__ __launch_bounds__(256) void k_color_dist2(const float* __restrict__ L, const float* __restrict__ U,
                                                     const float* __restrict__ V,
                                                     const unsigned char* __restrict__ num, size_t stride,
                                                     uint32_t n, const NeedleF* __restrict__ needles,
                                                     int* __restrict__ out /* [nq][n] */) {
  const uint32_t i0 = (color_tile() * blockDim.x + threadIdx.x) * 2u;  // descriptors i0, i0 + 1 (stride is even)
  const NeedleF& nd = needles[blockIdx.x];                             // wave-uniform, colours >= num padded
  const int nn = nd.num;
  const int hn0 = i0 < n ? (int)num[i0] : 0, hn1 = i0 + 1 < n ? (int)num[i0 + 1] : 0;
  const int hmax = max(hn0, hn1);
  constexpr uint32_t kBig = 0x7f7fffffu;  // FLT_MAX
  u2 rowmin[kNC];
#pragma unroll
  for (int p = 0; p < kNC; ++p) rowmin[p] = u2{kBig, kBig};
  f2 colacc = {1.0f, 1.0f};
  for (int h = 0; h < kNC; ++h) {
    if (__ballot(h < hmax) == 0ull) break;  // no lane of this wave has that many colours
    f2 hl = {1e18f, 1e18f}, hu = {0.f, 0.f}, hv = {0.f, 0.f};
    if (i0 < n) {  // planes are padded to an even capacity and with 1e18 beyond every descriptor's colours
      hl = *reinterpret_cast<const f2*>(L + (size_t)h * stride + i0);
      hu = *reinterpret_cast<const f2*>(U + (size_t)h * stride + i0);
      hv = *reinterpret_cast<const f2*>(V + (size_t)h * stride + i0);
    }
    u2 colmin = {kBig, kBig};
#pragma unroll
    for (int p = 0; p < kNC; p += 2) {
      const f2 dl0 = f2{nd.l[p], nd.l[p]} - hl, du0 = f2{nd.u[p], nd.u[p]} - hu, dv0 = f2{nd.v[p], nd.v[p]} - hv;
      const f2 dl1 = f2{nd.l[p + 1], nd.l[p + 1]} - hl, du1 = f2{nd.u[p + 1], nd.u[p + 1]} - hu,
               dv1 = f2{nd.v[p + 1], nd.v[p + 1]} - hv;
      const f2 e0 = dl0 * dl0 + du0 * du0 + dv0 * dv0;
      const f2 e1 = dl1 * dl1 + du1 * du1 + dv1 * dv1;
      const u2 b0 = __builtin_bit_cast(u2, e0), b1 = __builtin_bit_cast(u2, e1);
      rowmin[p] = u2{min(rowmin[p].x, b0.x), min(rowmin[p].y, b0.y)};
      rowmin[p + 1] = u2{min(rowmin[p + 1].x, b1.x), min(rowmin[p + 1].y, b1.y)};
      colmin = u2{min(min(colmin.x, b0.x), b1.x), min(min(colmin.y, b0.y), b1.y)};  // v_min3_u32
    }
    // (scalar copies first: __builtin_bit_cast on a vector-element lvalue reads element 0 with this clang)
    const uint32_t cm0 = colmin.x, cm1 = colmin.y;
    if (h < hn0) colacc.x += sqrtf(__builtin_bit_cast(float, cm0));  // haystack side is "a" (more colours)
    if (h < hn1) colacc.y += sqrtf(__builtin_bit_cast(float, cm1));
  }
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const uint32_t i = i0 + (uint32_t)e;
    const int hn = e ? hn1 : hn0;
    int result = -1;
    if (i < n && nn != 0 && hn != 0 && abs(nn - hn) <= 2) {
      float score;
      if (nn < hn) {
        score = e ? colacc.y : colacc.x;
      } else {
        score = 1.0f;
#pragma unroll
        for (int p = 0; p < kNC; ++p)
          if (p < nn) {
            const uint32_t rm = e ? rowmin[p].y : rowmin[p].x;
            score += sqrtf(__builtin_bit_cast(float, rm));
          }
      }
      result = (int)score;
    }
    if (i < n) out[(size_t)blockIdx.x * n + i] = result;
  }
}

// k_color_dist3 (default): the same arithmetic shaped for the VALU's fast path.  tools/ubench/pk_f32_rate.hip on the
// MI355X: a wave issues one VALU instruction every ~4.3-5 cycles, and a SIMD interleaves TWO waves, so plain
// v_sub/v_mul/v_add_f32 and v_min3_u32 on VGPR operands retire every ~2.15 cycles per SIMD with 2, 4, 6 or 8 resident
// waves -- but every 2.8 with 3 (an odd wave has no partner), every 4.1 when an operand is an SGPR (k_color_dist,
// k_color_dist2 keep the needle in SGPRs), and the packed forms (v_pk_*_f32) every 4.2 for two floats per lane, i.e.
// no gain.  So: needle colours in VGPRs, 32-bit ops, and an EVEN occupancy.  All 96 needle components + 32 running
// minima do not fit 128 VGPRs (4 waves), so the needle is taken in two halves of 16 colours: a lane owns one haystack
// descriptor, walks its colours two at a time against the 16 needle colours of the half (3 sub + 3 mul + 2 add per
// pair, one v_min3_u32 per needle colour for its running minimum, one per two needle colours for each haystack
// colour's), and parks the haystack-side minima of the first half in LDS ([colour][lane], conflict-free) for the
// second half to finish.  40 KB of LDS per workgroup also pins the occupancy at 4 workgroups per CU = 4 waves per
// SIMD.  Operation order per distance and per sum is k_color_dist's (minima are order-independent; the two sums run
// over ascending colour index), so the results are bit-identical.  RAW: also the float distance (FLT_MAX where the
// reference's distance() returns FLT_MAX).
// FMA ("color_fma" 1, never the default): dl^2 + du^2 + dv^2 as one multiply and two fused multiply-adds -- 6
// floating-point instructions per colour pair instead of 8.  The squared distance then carries one rounding instead of
// three, so a distance can differ from ColorDescriptor::distance's (src/cvutil.cpp:700-735: plain float expressions,
// which GCC does not contract across statements at cbird's -O2) in its last bits: within north_star's 1e-5 on the float,
// but int(score) is not guaranteed to match at an integer boundary.  tools/bench_configs.py reports the rate both ways and
// how many scores move.
constexpr int kHalf = kNC / 2;
template <bool RAW, bool FMA>
__global__ __launch_bounds__(256) void k_color_dist3(const float* __restrict__ L, const float* __restrict__ U,
                                                     const float* __restrict__ V,
                                                     const unsigned char* __restrict__ num, size_t stride,
                                                     uint32_t n, const NeedleF* __restrict__ needles,
                                                     int* __restrict__ out /* [nq][n] */,
                                                     float* __restrict__ raw /* [nq][n] or null */) {
  __shared__ uint32_t s_cmin[kNC + 8][256];  // +8 rows: 33 KB -> 40 KB, at most 4 workgroups per CU
  const uint32_t i = color_tile() * blockDim.x + threadIdx.x;
  const NeedleF& nd = needles[blockIdx.x];  // wave-uniform, colours >= num padded with 1e18
  const int nn = nd.num;
  const int hn = i < n ? (int)num[i] : 0;
  const uint32_t ii = i < n ? i : 0;  // (lanes past the end read descriptor 0 and write nothing)
  constexpr uint32_t kBig = 0x7f7fffffu;  // FLT_MAX
  unsigned zero;
  asm volatile("v_mov_b32 %0, 0" : "=v"(zero));  // an index the compiler cannot prove uniform: vector loads below
  const float4* np4 = reinterpret_cast<const float4*>(&nd) + zero;
  float colacc = 1.0f, rowacc = 1.0f;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    // this half's 48 needle components straight into VGPRs (every lane reads the same bytes: broadcast lines)
    float nl[kHalf], nu[kHalf], nv[kHalf];
#pragma unroll
    for (int p = 0; p < kHalf / 4; ++p) {
      const float4 a = np4[half * (kHalf / 4) + p], b = np4[kNC / 4 + half * (kHalf / 4) + p],
                   c = np4[2 * (kNC / 4) + half * (kHalf / 4) + p];
      nl[4 * p] = a.x, nl[4 * p + 1] = a.y, nl[4 * p + 2] = a.z, nl[4 * p + 3] = a.w;
      nu[4 * p] = b.x, nu[4 * p + 1] = b.y, nu[4 * p + 2] = b.z, nu[4 * p + 3] = b.w;
      nv[4 * p] = c.x, nv[4 * p + 1] = c.y, nv[4 * p + 2] = c.z, nv[4 * p + 3] = c.w;
    }
    uint32_t rowmin[kHalf];
#pragma unroll
    for (int p = 0; p < kHalf; ++p) rowmin[p] = kBig;
    // planes are padded with 1e18 beyond every descriptor's colours: no guards in the loop.  The next step's six
    // values are requested before this step's arithmetic.
    float al = L[ii], au = U[ii], av = V[ii];
    float bl = L[stride + ii], bu = U[stride + ii], bv = V[stride + ii];
    for (int h = 0; h < kNC; h += 2) {
      if (__ballot(h < hn) == 0ull) break;  // no lane of this wave has that many colours
      const int hnx = h + 2 < kNC ? h + 2 : h;  // (the last step re-reads its own colours: harmless)
      const float xal = L[(size_t)hnx * stride + ii], xau = U[(size_t)hnx * stride + ii],
                  xav = V[(size_t)hnx * stride + ii];
      const float xbl = L[(size_t)(hnx + 1) * stride + ii], xbu = U[(size_t)(hnx + 1) * stride + ii],
                  xbv = V[(size_t)(hnx + 1) * stride + ii];
      uint32_t cmin_a = kBig, cmin_b = kBig;
      if (half) cmin_a = s_cmin[h][threadIdx.x], cmin_b = s_cmin[h + 1][threadIdx.x];
#pragma unroll
      for (int p = 0; p < kHalf; p += 2) {
        uint32_t da[2], db[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float dl = nl[p + e] - al, du = nu[p + e] - au, dv = nv[p + e] - av;
          const float el = nl[p + e] - bl, eu = nu[p + e] - bu, ev = nv[p + e] - bv;
          const float d2a = FMA ? __builtin_fmaf(dv, dv, __builtin_fmaf(du, du, dl * dl)) : dl * dl + du * du + dv * dv;
          const float d2b = FMA ? __builtin_fmaf(ev, ev, __builtin_fmaf(eu, eu, el * el)) : el * el + eu * eu + ev * ev;
          da[e] = __builtin_bit_cast(uint32_t, d2a);
          db[e] = __builtin_bit_cast(uint32_t, d2b);
          rowmin[p + e] = min(min(rowmin[p + e], da[e]), db[e]);  // v_min3_u32
        }
        cmin_a = min(min(cmin_a, da[0]), da[1]);
        cmin_b = min(min(cmin_b, db[0]), db[1]);
      }
      if (half == 0) {
        s_cmin[h][threadIdx.x] = cmin_a, s_cmin[h + 1][threadIdx.x] = cmin_b;  // own column only: no barrier needed
      } else {
        if (h < hn) colacc += sqrtf(__builtin_bit_cast(float, cmin_a));  // haystack side is "a" (more colours)
        if (h + 1 < hn) colacc += sqrtf(__builtin_bit_cast(float, cmin_b));
      }
      al = xal, au = xau, av = xav, bl = xbl, bu = xbu, bv = xbv;
    }
#pragma unroll
    for (int p = 0; p < kHalf; ++p)  // needle side is "a": sum over needle colours in index order, across the halves
      if (half * kHalf + p < nn) rowacc += sqrtf(__builtin_bit_cast(float, rowmin[p]));
  }
  if (i >= n) return;
  int result = -1;
  float score = FLT_MAX;
  if (nn != 0 && hn != 0 && abs(nn - hn) <= 2) {
    score = nn < hn ? colacc : rowacc;
    result = (int)score;
  }
  out[(size_t)blockIdx.x * n + i] = result;
  if (RAW) raw[(size_t)blockIdx.x * n + i] = score;
}

// key = score<<32 | id for entries that match (score >= 0, id != 0), ~0 otherwise
__global__ __launch_bounds__(256) void k_color_keys(const int* __restrict__ score,
                                                    const uint32_t* __restrict__ ids, uint32_t n,
                                                    unsigned long long* __restrict__ keys) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = score[i];
  const uint32_t id = ids[i];
  keys[i] = (s >= 0 && id != 0) ? (((unsigned long long)(uint32_t)s << 32) | id) : ~0ull;
}


// ---- top-k per needle without sorting the whole score row (find_batch) -----------------------------------
// Scores are small integers, so the k-th smallest score can be found exactly with a histogram; only entries at
// or under it are collected and ordered on the host.  The k best of ~10^6 entries lie within a few hundred of
// the minimum, so the histogram is a 2048-bin window above the per-needle minimum score (k_color_min), kept in
// LDS per block and flushed once (one pass of global atomics over ALL scores took 5 ms per 64 needles; this
// takes 0.2 ms).  A k-th score beyond the window, or more ties than kCandCap, falls back to the full sort.
constexpr int kWin = 2048;
constexpr uint32_t kCandCap = 4096;  // per needle; more ties than this -> the full-sort path

__global__ __launch_bounds__(256) void k_color_min(const int* __restrict__ score, const uint32_t* __restrict__ ids,
                                                   uint32_t n, int* __restrict__ smin /* [nq], init INT_MAX */) {
  const uint32_t q = blockIdx.y;
  const int* sc = score + (size_t)q * n;
  int m = 0x7fffffff;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const int s = sc[i];
    if (s >= 0 && ids[i] != 0) m = min(m, s);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && m != 0x7fffffff) atomicMin(&smin[q], m);
}

__global__ __launch_bounds__(256) void k_color_hist(const int* __restrict__ score,
                                                    const uint32_t* __restrict__ ids, uint32_t n,
                                                    const int* __restrict__ smin,
                                                    uint32_t* __restrict__ hist /* [nq][kWin] */,
                                                    uint32_t* __restrict__ valid /* [nq] */) {
  __shared__ uint32_t sh[kWin];
  const uint32_t q = blockIdx.y;
  const int* sc = score + (size_t)q * n;
  const int base = smin[q];
  for (int b = threadIdx.x; b < kWin; b += 256) sh[b] = 0;
  __syncthreads();
  uint32_t local = 0;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const int s = sc[i];
    if (s >= 0 && ids[i] != 0) {
      ++local;
      const int d = s - base;
      if (d < kWin) atomicAdd(&sh[d], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kWin; b += 256)
    if (sh[b]) atomicAdd(&hist[(size_t)q * kWin + b], sh[b]);
  if (local) atomicAdd(&valid[q], local);  // compiler aggregates per wave
}

// thr[q] = k-th smallest score when it lies inside the window, else INT_MAX (collect everything -> fallback)
__global__ __launch_bounds__(256) void k_color_thresh(const uint32_t* __restrict__ hist, uint32_t k,
                                                      const int* __restrict__ smin, int* __restrict__ thr) {
  __shared__ uint32_t part[256];
  const uint32_t q = blockIdx.x, t = threadIdx.x;
  const uint32_t* h = hist + (size_t)q * kWin + t * (kWin / 256);
  uint32_t sum = 0;
  for (int b = 0; b < kWin / 256; ++b) sum += h[b];
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    int bin = -1;
    for (uint32_t j = 0; j < 256 && bin < 0; ++j) {
      if (run + part[j] >= k) {
        const uint32_t* hs = hist + (size_t)q * kWin + j * (kWin / 256);
        uint32_t c = run;
        for (int b = 0; b < kWin / 256; ++b) {
          c += hs[b];
          if (c >= k) {
            bin = (int)j * (kWin / 256) + b;
            break;
          }
        }
      }
      run += part[j];
    }
    thr[q] = bin >= 0 ? smin[q] + bin : 0x7fffffff;
  }
}

__global__ __launch_bounds__(256) void k_color_collect(const int* __restrict__ score,
                                                       const uint32_t* __restrict__ ids, uint32_t n,
                                                       const int* __restrict__ thr,
                                                       unsigned long long* __restrict__ cand /* [nq][kCandCap] */,
                                                       uint32_t* __restrict__ ncand /* [nq] */) {
  const uint32_t q = blockIdx.y;
  const int* sc = score + (size_t)q * n;
  const int T = thr[q];
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const int s = sc[i];
    const uint32_t id = ids[i];
    if (s >= 0 && id != 0 && s <= T) {
      const uint32_t slot = atomicAdd(&ncand[q], 1u);
      if (slot < kCandCap) cand[(size_t)q * kCandCap + slot] = ((unsigned long long)(uint32_t)s << 32) | id;
    }
  }
}

// distance kernels: k_color_dist2 (two descriptors per lane on packed f32; the default: 12.1 ms per 64 needles x 1M
// descriptors) and k_color_dist3 (32-bit ops on VGPR operands at 4 waves per SIMD: 12.5 ms; the one that can also hand
// out the raw floats, and the fused-square form of "color_fma").  Both sit at the VALU issue ceiling of this arithmetic
// (no FMA: the reference's rounding order) once the launch geometry lets concurrent workgroups share haystack tiles.
// (Round 1's one-descriptor-per-lane k_color_dist, 14.1 ms, is in the history: r05's "color_pk" 0.)
int g_color_fma = 0;  // "color_fma": 1 = k_color_dist3 with fused squares (faster, NOT bit-identical; see the kernel)

void decompress(const uint8_t* desc, NeedleF* out) {  // DescriptorColor::get, cvutil.h:83-87
  for (int c = 0; c < kNC; ++c) {
    uint16_t l, u, v;
    memcpy(&l, desc + c * 8 + 0, 2);
    memcpy(&u, desc + c * 8 + 2, 2);
    memcpy(&v, desc + c * 8 + 4, 2);
    out->l[c] = l * 100.0f / 65535;
    out->u[c] = u * 354.0f / 65535 - 134.0f;
    out->v[c] = v * 262.0f / 65535 - 140.0f;
  }
  out->num = desc[256];
  // colours the reference's loops never visit (index >= numColors): far away, so that a distance involving one
  // of them (~1e36, finite) can never be a minimum -- lets k_color_dist2 run without per-colour guards
  for (int c = out->num < kNC ? out->num : kNC; c < kNC; ++c) {
    out->l[c] = 1e18f;
    out->u[c] = 0.f;
    out->v[c] = 0.f;
  }
}

// "color_chunk_scores": the most score elements (needles x entries) one chunk of cbh_color_find_batch,
// cbh_color_find_all_batch or cbh_color_distances may hold; 0 (default) = 2^28 / 2^27 / 2^27.  At least one needle per
// chunk.  Forced (tests): the second and later chunks of the needle loops on a small index.  Results do not depend on it.
std::atomic<int> g_color_chunk_scores{0};
// "color_full_sorts" / "color_window_cuts": needles of cbh_color_find_batch that went through color_full_sort_one / were
// answered from the candidate list (needles without a match, and k == 0, count as neither)
std::atomic<long long> g_color_full_sorts{0}, g_color_window_cuts{0};

// ---- cbh_color_sort_similar ---------------------------------------------------------------------------------------------
// "color_sort_table_kb": KiB of score tables one group of sets may hold, 0 (default) = kSortTableBytes.  Forced (tests):
// several groups on small sets, and a set that does not fit.  Results do not depend on it.
constexpr uint64_t kSortTableBytes = 2ull << 30;
static_assert((uint64_t)CBH_COLOR_SORT_SIMILAR_MAX * CBH_COLOR_SORT_SIMILAR_MAX * 2 <= kSortTableBytes,
              "the largest set's table has to fit the default budget");
static_assert(CBH_COLOR_SORT_SIMILAR_MAX <= CBH_SORT_SIMILAR_MAX, "the chain's limit");
std::atomic<int> g_color_sort_table_kb{0}, g_color_sort_timing{0};
std::atomic<long long> g_color_sort_stat[3];  // the last call's groups, table fill in us, chain in us (timing on)

// int scores of rows [r0, r0 + m) of one set (k_color_dist*: [m][n], -1 = no match) into the set's table: uint16_t rows of
// `stride` scores (a multiple of 8), 0xFFFF = no match and in the padding.  A score is (int)(1.0f + up to 32 distances of
// at most sqrt(100^2 + 354^2 + 262^2) = 451.7 between decompressed colours, src/cvutil.h:83-87) <= 14 454 < 0xFFFF.
__global__ __launch_bounds__(256) void k_color_table(const int* __restrict__ score, uint32_t m, uint32_t n, uint32_t stride,
                                                     uint32_t* __restrict__ rows /* [m][stride / 2] */) {
  const uint32_t half = stride / 2;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)m * half) return;
  const uint32_t r = (uint32_t)(t / half), c = (uint32_t)(t % half) * 2;
  const int a = c < n ? score[(size_t)r * n + c] : -1, b = c + 1 < n ? score[(size_t)r * n + c + 1] : -1;
  rows[t] = (a < 0 ? 0xffffu : (uint32_t)a) | (b < 0 ? 0xffffu : (uint32_t)b) << 16;
}

// an item without a live entry in the index: no colours, so that no needle matches it (its in_index flag is 0 as well)
__global__ __launch_bounds__(256) void k_color_absent(const uint8_t* __restrict__ attr, uint32_t n,
                                                      unsigned char* __restrict__ num) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && !(attr[i] & 1)) num[i] = 0;
}

// needles per chunk of a loop whose default budget is `dflt` score elements
size_t color_chunk(size_t nq, size_t n, size_t dflt) {
  const int forced = g_color_chunk_scores.load();
  return std::max<size_t>(1, std::min<size_t>(nq, (forced > 0 ? (size_t)forced : dflt) / n));
}

}  // namespace

namespace cbh {
void set_color_fma(int on) { g_color_fma = on ? 1 : 0; }
int set_color_chunk_scores(int v) {
  if (v < 0) return CBH_E_INVAL;
  g_color_chunk_scores.store(v);
  return CBH_OK;
}
int get_color_chunk_scores() { return g_color_chunk_scores.load(); }
long long get_color_full_sorts() { return g_color_full_sorts.load(); }
long long get_color_window_cuts() { return g_color_window_cuts.load(); }
int set_color_sort_table_kb(int v) {
  if (v < 0) return CBH_E_INVAL;
  g_color_sort_table_kb.store(v);
  return CBH_OK;
}
int get_color_sort_table_kb() { return g_color_sort_table_kb.load(); }
void set_color_sort_timing(int on) { g_color_sort_timing.store(on ? 1 : 0); }
long long get_color_sort_stat(int which) { return which >= 0 && which < 3 ? g_color_sort_stat[which].load() : 0; }
}  // namespace cbh

struct cbh_color {
  int device = 0;
  size_t n = 0, cap = 0;
  float *dL = nullptr, *dU = nullptr, *dV = nullptr;  // [32][cap]
  unsigned char* d_num = nullptr;
  uint32_t* d_ids = nullptr;
  std::vector<uint8_t> host_desc;  // AoS copy for findIndexData / slice (258 B each)
  std::vector<uint32_t> host_ids;
  std::mutex mu;
  hipStream_t stream = nullptr;
  NeedleF* d_needles = nullptr;
  size_t needles_cap = 0;
  int* d_scores = nullptr;
  size_t scores_cap = 0;
  unsigned long long *d_keys = nullptr, *d_keys_alt = nullptr;
  void* d_tmp = nullptr;
  size_t keys_cap = 0, tmp_bytes = 0;
  // find_batch top-k scratch
  uint32_t *d_hist = nullptr, *d_ncand = nullptr, *d_valid = nullptr;
  int *d_thr = nullptr, *d_smin = nullptr;
  unsigned long long* d_cand = nullptr;
  size_t topk_cap = 0;
};

namespace {

int grow_index(cbh_color* c, size_t need) {
  if (need <= c->cap) return CBH_OK;
  const size_t ncap = (std::max<size_t>(need, c->cap + c->cap / 2 + 4096) + 1) & ~(size_t)1;  // even: pair loads
  float *nL = nullptr, *nU = nullptr, *nV = nullptr;
  unsigned char* nn = nullptr;
  uint32_t* ni = nullptr;
  CBH_HIP(hipMalloc(&nL, ncap * kNC * 4));
  CBH_HIP(hipMalloc(&nU, ncap * kNC * 4));
  CBH_HIP(hipMalloc(&nV, ncap * kNC * 4));
  CBH_HIP(hipMalloc(&nn, ncap));
  CBH_HIP(hipMalloc(&ni, ncap * 4));
  if (c->n) {
    CBH_HIP(hipMemcpy2D(nL, ncap * 4, c->dL, c->cap * 4, c->n * 4, kNC, hipMemcpyDeviceToDevice));
    CBH_HIP(hipMemcpy2D(nU, ncap * 4, c->dU, c->cap * 4, c->n * 4, kNC, hipMemcpyDeviceToDevice));
    CBH_HIP(hipMemcpy2D(nV, ncap * 4, c->dV, c->cap * 4, c->n * 4, kNC, hipMemcpyDeviceToDevice));
    CBH_HIP(hipMemcpy(nn, c->d_num, c->n, hipMemcpyDeviceToDevice));
    CBH_HIP(hipMemcpy(ni, c->d_ids, c->n * 4, hipMemcpyDeviceToDevice));
  }
  for (void* p : {(void*)c->dL, (void*)c->dU, (void*)c->dV, (void*)c->d_num, (void*)c->d_ids})
    if (p) (void)hipFree(p);
  c->dL = nL;
  c->dU = nU;
  c->dV = nV;
  c->d_num = nn;
  c->d_ids = ni;
  c->cap = ncap;
  return CBH_OK;
}

// upload host descriptors [first, first+m) into the planar device arrays
int upload(cbh_color* c, size_t first, size_t m) {
  std::vector<float> pl((size_t)kNC * m), pu((size_t)kNC * m), pv((size_t)kNC * m);
  std::vector<unsigned char> pn(m);
  NeedleF f;
  for (size_t i = 0; i < m; ++i) {
    decompress(c->host_desc.data() + (first + i) * kDescBytes, &f);
    for (int k = 0; k < kNC; ++k) {
      pl[(size_t)k * m + i] = f.l[k];
      pu[(size_t)k * m + i] = f.u[k];
      pv[(size_t)k * m + i] = f.v[k];
    }
    pn[i] = (unsigned char)f.num;
  }
  CBH_HIP(hipMemcpy2D(c->dL + first, c->cap * 4, pl.data(), m * 4, m * 4, kNC, hipMemcpyHostToDevice));
  CBH_HIP(hipMemcpy2D(c->dU + first, c->cap * 4, pu.data(), m * 4, m * 4, kNC, hipMemcpyHostToDevice));
  CBH_HIP(hipMemcpy2D(c->dV + first, c->cap * 4, pv.data(), m * 4, m * 4, kNC, hipMemcpyHostToDevice));
  CBH_HIP(hipMemcpy(c->d_num + first, pn.data(), m, hipMemcpyHostToDevice));
  CBH_HIP(hipMemcpy(c->d_ids + first, c->host_ids.data() + first, m * 4, hipMemcpyHostToDevice));
  return CBH_OK;
}

int ensure_scratch(cbh_color* c, size_t nq, bool keys) {
  if (!c->stream) CBH_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  if (nq > c->needles_cap) {
    if (c->d_needles) (void)hipFree(c->d_needles);
    c->d_needles = nullptr;
    CBH_HIP(hipMalloc(&c->d_needles, nq * sizeof(NeedleF)));
    c->needles_cap = nq;
  }
  if (nq * c->n > c->scores_cap) {
    if (c->d_scores) (void)hipFree(c->d_scores);
    c->d_scores = nullptr;
    CBH_HIP(hipMalloc(&c->d_scores, nq * c->n * 4));
    c->scores_cap = nq * c->n;
  }
  if (keys && c->n > c->keys_cap) {
    for (void* p : {(void*)c->d_keys, (void*)c->d_keys_alt, c->d_tmp})
      if (p) (void)hipFree(p);
    c->d_keys = c->d_keys_alt = nullptr;
    c->d_tmp = nullptr;
    CBH_HIP(hipMalloc(&c->d_keys, c->n * 8));
    CBH_HIP(hipMalloc(&c->d_keys_alt, c->n * 8));
    c->tmp_bytes = cbh::sort_records_scratch_bytes(c->n);
    CBH_HIP(hipMalloc(&c->d_tmp, c->tmp_bytes ? c->tmp_bytes : 16));
    c->keys_cap = c->n;
  }
  return CBH_OK;
}

// scores of nq needles against the whole index -> c->d_scores [nq][n] (enqueued on c->stream); d_raw: also the float
// distances (k_color_dist3 only)
// the distance kernel the knobs choose, nq needles against n descriptors in planes of `cap` entries (cap even, padded)
int launch_dist(const float* dL, const float* dU, const float* dV, const unsigned char* d_num, size_t cap, size_t n,
                const NeedleF* d_needles, size_t nq, int* d_scores, float* d_raw, hipStream_t stream) {
  if (d_raw || g_color_fma) {
    const unsigned tiles = (unsigned)((n + 255) / 256);
    dim3 grid((unsigned)nq, std::min(tiles, 32768u), (tiles + 32767u) / 32768u), block(256);
#define CBH_DIST3(RAW_, FMA_)                                                                                         \
  hipLaunchKernelGGL((k_color_dist3<RAW_, FMA_>), grid, block, 0, stream, dL, dU, dV, d_num, cap, (uint32_t)n, d_needles, \
                     d_scores, d_raw)
    if (g_color_fma) {
      if (d_raw) CBH_DIST3(true, true); else CBH_DIST3(false, true);
    } else {
      if (d_raw) CBH_DIST3(true, false); else CBH_DIST3(false, false);
    }
#undef CBH_DIST3
  } else {  // (cap is always even: ensure_cap)
    const unsigned tiles = (unsigned)((n + 511) / 512);
    dim3 grid((unsigned)nq, std::min(tiles, 32768u), (tiles + 32767u) / 32768u), block(256);
    hipLaunchKernelGGL(k_color_dist2, grid, block, 0, stream, dL, dU, dV, d_num, cap, (uint32_t)n, d_needles, d_scores);
  }
  CBH_HIP(hipGetLastError());
  return CBH_OK;
}

int run_dist(cbh_color* c, const uint8_t* needle_descs, size_t nq, float* d_raw = nullptr) {
  std::vector<NeedleF> nf(nq);
  for (size_t q = 0; q < nq; ++q) decompress(needle_descs + q * kDescBytes, &nf[q]);
  CBH_HIP(hipMemcpyAsync(c->d_needles, nf.data(), nq * sizeof(NeedleF), hipMemcpyHostToDevice, c->stream));
  CBH_HIP(hipStreamSynchronize(c->stream));  // nf is a stack-lifetime buffer
  return launch_dist(c->dL, c->dU, c->dV, c->d_num, c->cap, c->n, c->d_needles, nq, c->d_scores, d_raw, c->stream);
}

}  // namespace

extern "C" {

cbh_color* cbh_color_create(int device) {
  cbh::clear_last_error();
  if (!cbh::device_usable(device)) return (cbh_color*)cbh::fail_handle(CBH_E_NODEVICE, "cbh_color_create: no usable gfx950 device at that ordinal");
  cbh_color* c = new (std::nothrow) cbh_color;
  if (!c) return (cbh_color*)cbh::fail_handle(CBH_E_NOMEM, "cbh_color_create: host allocation failed");
  c->device = device;
  return c;
}

void cbh_color_destroy(cbh_color* c) {
  if (!c) return;
  cbh::combiner_drop(c);  // combine.hip: the queue of cbh_*_find_coalesced callers
  cbh::DeviceGuard g(c->device);
  for (void* p : {(void*)c->dL, (void*)c->dU, (void*)c->dV, (void*)c->d_num, (void*)c->d_ids, (void*)c->d_needles,
                  (void*)c->d_scores, (void*)c->d_keys, (void*)c->d_keys_alt, c->d_tmp, (void*)c->d_hist,
                  (void*)c->d_thr, (void*)c->d_smin, (void*)c->d_ncand, (void*)c->d_valid, (void*)c->d_cand})
    if (p) (void)hipFree(p);
  if (c->stream) cbh::stream_destroy(c->stream);
  delete c;
}

/* add()/load(): append n (mediaId, ColorDescriptor) entries (colordescindex.cpp:123-168, 201-213) */
int cbh_color_add(cbh_color* c, const uint32_t* ids, const void* descs, size_t n) {
  if (!c || (n && (!ids || !descs))) return CBH_E_INVAL;
  if (n == 0) return CBH_OK;
  cbh::DeviceGuard g(c->device);
  if (!g.ok) return CBH_E_NODEVICE;
  std::lock_guard<std::mutex> lk(c->mu);
  const size_t first = c->n;
  int rc = grow_index(c, first + n);
  if (rc) return rc;  // (before the host copies grow: a refused add leaves nothing behind for the next one to upload)
  c->host_desc.insert(c->host_desc.end(), (const uint8_t*)descs, (const uint8_t*)descs + n * kDescBytes);
  c->host_ids.insert(c->host_ids.end(), ids, ids + n);
  c->n = first + n;
  return upload(c, first, n);
}

/* remove(): id 0 and cleared descriptor in place (:215-229) */
int cbh_color_remove(cbh_color* c, const uint32_t* ids, size_t n) {
  if (!c || (n && !ids)) return CBH_E_INVAL;
  if (c->n == 0 || n == 0) return CBH_OK;  // `if (!isLoaded()) return;`
  cbh::DeviceGuard g(c->device);
  if (!g.ok) return CBH_E_NODEVICE;
  std::lock_guard<std::mutex> lk(c->mu);
  std::vector<uint32_t> rm(ids, ids + n);
  std::sort(rm.begin(), rm.end());
  for (size_t i = 0; i < c->n; ++i)
    if (std::binary_search(rm.begin(), rm.end(), c->host_ids[i])) {
      c->host_ids[i] = 0;
      memset(c->host_desc.data() + i * kDescBytes, 0, kDescBytes);
      int rc = upload(c, i, 1);
      if (rc) return rc;
    }
  return CBH_OK;
}

/* slice() (colordescindex.cpp:231-248): the entries whose id is listed, in index order.  The host copies are filtered on
 * the host; the device planes are gathered from the parent's by position (slice.hip: k_slice_color) -- no descriptor is
 * decompressed or uploaded again. */
static int color_slice(cbh_color* c, const std::vector<uint32_t>& want, cbh_color* out) {
  cbh::DeviceGuard g(c->device);
  if (!g.ok) return CBH_E_NODEVICE;
  std::lock_guard<std::mutex> lk(c->mu);
  std::vector<uint32_t> pos;
  for (size_t i = 0; i < c->n; ++i)
    if (std::binary_search(want.begin(), want.end(), c->host_ids[i])) pos.push_back((uint32_t)i);
  const size_t m = pos.size();
  if (m) {
    out->host_ids.resize(m);
    out->host_desc.resize(m * kDescBytes);
    for (size_t j = 0; j < m; ++j) {
      out->host_ids[j] = c->host_ids[pos[j]];
      memcpy(out->host_desc.data() + j * kDescBytes, c->host_desc.data() + (size_t)pos[j] * kDescBytes, kDescBytes);
    }
    // a multiple of 4: even, as the pair loads need it, and every plane 16-byte aligned for the gather's stores.  The
    // planes fit exactly; a later add() lands in the slack or grows them (grow_index copies by the old pitch)
    const size_t cap = (m + 3) & ~(size_t)3;
    CBH_HIP(hipMalloc(&out->dL, cap * kNC * 4));
    CBH_HIP(hipMalloc(&out->dU, cap * kNC * 4));
    CBH_HIP(hipMalloc(&out->dV, cap * kNC * 4));
    CBH_HIP(hipMalloc(&out->d_num, cap));
    CBH_HIP(hipMalloc(&out->d_ids, cap * 4));
    out->cap = cap;
    if (!c->stream) CBH_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    cbh::Scratch scratch(c->stream);
    uint32_t* d_pos = nullptr;
    int rc = CBH_OK;
    hipError_t e = scratch.get(&d_pos, m * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pos, pos.data(), m * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
      rc = cbh::launch_slice_color(c->dL, c->dU, c->dV, c->d_num, c->d_ids, c->cap, d_pos, m, out->dL, out->dU, out->dV,
                                   out->d_num, out->d_ids, cap, c->stream);
    const hipError_t drained = hipStreamSynchronize(c->stream);  // on every path: pos is read by the copy
    if (rc) return rc;
    CBH_HIP(e);
    CBH_HIP(drained);
    out->n = m;
  }
  cbh::note_slice_on_device();
  return CBH_OK;
}

cbh_color* cbh_color_slice(const cbh_color* c, const uint32_t* ids, size_t n) {
  cbh::clear_last_error();
  if (!c || (n && !ids)) return (cbh_color*)cbh::fail_handle(CBH_E_INVAL, "cbh_color_slice: no index, or a count without ids");
  std::vector<uint32_t> want(ids, ids + (ids ? n : 0));
  std::sort(want.begin(), want.end());
  cbh_color* out = cbh_color_create(c->device);
  if (!out) return nullptr;  // (the create call has set the code)
  if (const int rc = color_slice(const_cast<cbh_color*>(c), want, out)) {
    cbh_color_destroy(out);
    return (cbh_color*)cbh::fail_handle(rc, nullptr);
  }
  return out;
}

size_t cbh_color_count(const cbh_color* c) { return c ? c->n : 0; }
int cbh_color_is_loaded(const cbh_color* c) { return c && c->n > 0; }  // `_count > 0` (:114)
size_t cbh_color_memory_usage(const cbh_color* c) { return c ? (kDescBytes + 4) * c->n : 0; }  // (:118-121)

/* findIndexData (:231-239): first entry with that id */
int cbh_color_find_index_data(const cbh_color* c, uint32_t id, void* out_desc) {
  if (!c || !out_desc) return CBH_E_INVAL;
  for (size_t i = 0; i < c->n; ++i)
    if (c->host_ids[i] == id) {
      memcpy(out_desc, c->host_desc.data() + i * kDescBytes, kDescBytes);
      return 1;
    }
  return 0;
}

int cbh_color_download(const cbh_color* c, uint32_t* ids, void* descs, size_t cap) {
  if (!c) return CBH_E_INVAL;
  const size_t m = std::min(cap, c->n);
  if (ids) memcpy(ids, c->host_ids.data(), m * 4);
  if (descs) memcpy(descs, c->host_desc.data(), m * kDescBytes);
  return CBH_OK;
}

/* find() (:250-278): every entry with a finite distance and id != 0, index order, score = int(distance) */
int cbh_color_find(cbh_color* c, const void* needle_desc, cbh_match* out, size_t cap, size_t* n_out) {
  if (!c || !needle_desc || !n_out || (cap && !out)) return CBH_E_INVAL;
  *n_out = 0;
  if (((const uint8_t*)needle_desc)[256] == 0 || c->n == 0) return CBH_OK;  // no colours (:259-266)
  cbh::DeviceGuard g(c->device);
  if (!g.ok) return CBH_E_NODEVICE;
  std::lock_guard<std::mutex> lk(c->mu);
  int rc = ensure_scratch(c, 1, false);
  if (rc) return rc;
  rc = run_dist(c, (const uint8_t*)needle_desc, 1);
  if (rc) return rc;
  std::vector<int> sc(c->n);
  CBH_HIP(hipMemcpyAsync(sc.data(), c->d_scores, c->n * 4, hipMemcpyDeviceToHost, c->stream));
  CBH_HIP(hipStreamSynchronize(c->stream));
  size_t m = 0;
  for (size_t i = 0; i < c->n; ++i)
    if (sc[i] >= 0 && c->host_ids[i] != 0) {
      if (m < cap) out[m] = cbh_match{c->host_ids[i], sc[i]};
      ++m;
    }
  *n_out = m;
  return CBH_OK;
}

/* find() for nq needles in one pass: needle q's matches (all of them, index order, as cbh_color_find returns them) at
 * out[out_offsets[q] .. out_offsets[q+1]); CBH_E_OVERFLOW with out_offsets complete when cap is too small */
int cbh_color_find_all_batch(cbh_color* c, const void* needle_descs, size_t nq, cbh_match* out, size_t cap,
                             uint64_t* out_offsets) {
  if (!c || !out_offsets || (nq && !needle_descs) || (cap && !out)) return CBH_E_INVAL;
  for (size_t q = 0; q <= nq; ++q) out_offsets[q] = 0;
  if (nq == 0 || c->n == 0) return CBH_OK;
  cbh::DeviceGuard g(c->device);
  if (!g.ok) return CBH_E_NODEVICE;
  std::lock_guard<std::mutex> lk(c->mu);
  const size_t chunk = color_chunk(nq, c->n, (size_t)1 << 27);
  int rc = ensure_scratch(c, chunk, false);
  if (rc) return rc;
  std::vector<int> sc(chunk * c->n);
  uint64_t pos = 0;
  for (size_t q0 = 0; q0 < nq; q0 += chunk) {
    const size_t m = std::min(chunk, nq - q0);
    rc = run_dist(c, (const uint8_t*)needle_descs + q0 * kDescBytes, m);
    if (rc) return rc;
    CBH_HIP(hipMemcpyAsync(sc.data(), c->d_scores, m * c->n * 4, hipMemcpyDeviceToHost, c->stream));
    CBH_HIP(hipStreamSynchronize(c->stream));
    for (size_t q = 0; q < m; ++q) {
      out_offsets[q0 + q] = pos;
      if (((const uint8_t*)needle_descs)[(q0 + q) * kDescBytes + 256] == 0) continue;  // no colours (:259-266)
      const int* s = sc.data() + q * c->n;
      for (size_t i = 0; i < c->n; ++i)
        if (s[i] >= 0 && c->host_ids[i] != 0) {
          if (pos < cap) out[pos] = cbh_match{c->host_ids[i], s[i]};
          ++pos;
        }
    }
  }
  out_offsets[nq] = pos;
  return pos > cap ? CBH_E_OVERFLOW : CBH_OK;
}

/* ColorDescriptor::distance (cvutil.cpp:682-749) of nq needles against every index entry, as floats: out[q*n + i];
 * FLT_MAX where the reference returns FLT_MAX (no colours on a side, or the colour counts differ by more than 2).
 * Entry i is the i-th descriptor added, whatever its id. */
int cbh_color_distances(cbh_color* c, const void* needle_descs, size_t nq, float* out) {
  if (!c || (nq && (!needle_descs || !out))) return CBH_E_INVAL;
  if (nq == 0 || c->n == 0) return CBH_OK;
  cbh::DeviceGuard g(c->device);
  if (!g.ok) return CBH_E_NODEVICE;
  std::lock_guard<std::mutex> lk(c->mu);
  const size_t chunk = color_chunk(nq, c->n, (size_t)1 << 27);
  int rc = ensure_scratch(c, chunk, false);
  if (rc) return rc;
  float* d_raw = nullptr;
  CBH_HIP(hipMalloc(&d_raw, chunk * c->n * sizeof(float)));
  for (size_t q0 = 0; q0 < nq && !rc; q0 += chunk) {
    const size_t m = std::min(chunk, nq - q0);
    rc = run_dist(c, (const uint8_t*)needle_descs + q0 * kDescBytes, m, d_raw);
    if (rc) break;
    hipError_t e = hipMemcpyAsync(out + q0 * c->n, d_raw, m * c->n * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
      cbh::set_last_error("color distances", e);
      rc = CBH_E_HIP;
    }
  }
  (void)hipFree(d_raw);
  return rc;
}

/* find() for many needles + the sort/cut of searchIndex (database.cpp:1729-1735): out[q*k..] = first
 * min(counts[q], k) matches in (score, id) order, counts[q] = all matches */
// one needle through the full sort (ties beyond kCandCap, or k > kCandCap)
static int color_full_sort_one(cbh_color* c, size_t q_in_chunk, int k, cbh_match* out_q, uint32_t valid) {
  hipLaunchKernelGGL(k_color_keys, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream,
                     c->d_scores + q_in_chunk * c->n, c->d_ids, (uint32_t)c->n, c->d_keys);
  unsigned long long* sorted = nullptr;
  int rc_s = cbh::sort_keys64_db(c->d_keys, c->d_keys_alt, c->n, 64, c->d_tmp, c->tmp_bytes, c->stream, &sorted);
  if (rc_s) return rc_s;
  const size_t take = std::min<size_t>(std::min<size_t>((size_t)k, c->n), valid);
  std::vector<unsigned long long> head(take);
  if (take) CBH_HIP(hipMemcpyAsync(head.data(), sorted, take * 8, hipMemcpyDeviceToHost, c->stream));
  CBH_HIP(hipStreamSynchronize(c->stream));
  for (size_t j = 0; j < take; ++j) out_q[j] = cbh_match{(uint32_t)head[j], (int32_t)(head[j] >> 32)};
  return CBH_OK;
}

int cbh_color_find_batch(cbh_color* c, const void* needle_descs, size_t nq, int k, cbh_match* out,
                         uint32_t* counts) {
  if (!c || k < 0 || (nq && (!needle_descs || !counts || (k && !out)))) return CBH_E_INVAL;
  if (nq == 0) return CBH_OK;
  memset(counts, 0, nq * 4);
  if (k) memset(out, 0, nq * (size_t)k * sizeof(cbh_match));
  if (c->n == 0) return CBH_OK;
  cbh::DeviceGuard g(c->device);
  if (!g.ok) return CBH_E_NODEVICE;
  std::lock_guard<std::mutex> lk(c->mu);
  const size_t chunk = color_chunk(nq, c->n, (size_t)1 << 28);  // <= 1 GiB of scores
  int rc = ensure_scratch(c, chunk, true);
  if (rc) return rc;
  if (chunk > c->topk_cap) {
    for (void* p : {(void*)c->d_hist, (void*)c->d_thr, (void*)c->d_smin, (void*)c->d_ncand, (void*)c->d_valid,
                    (void*)c->d_cand})
      if (p) (void)hipFree(p);
    c->d_hist = c->d_ncand = c->d_valid = nullptr;
    c->d_thr = c->d_smin = nullptr;
    c->d_cand = nullptr;
    c->topk_cap = 0;
    CBH_HIP(hipMalloc(&c->d_hist, chunk * kWin * 4));
    CBH_HIP(hipMalloc(&c->d_thr, chunk * 4));
    CBH_HIP(hipMalloc(&c->d_smin, chunk * 4));
    CBH_HIP(hipMalloc(&c->d_ncand, chunk * 4));
    CBH_HIP(hipMalloc(&c->d_valid, chunk * 4));
    CBH_HIP(hipMalloc(&c->d_cand, chunk * (size_t)kCandCap * 8));
    c->topk_cap = chunk;
  }
  const bool topk = k >= 1 && (uint32_t)k <= kCandCap;
  std::vector<uint32_t> h_valid, h_ncand;
  std::vector<unsigned long long> h_cand;
  for (size_t q0 = 0; q0 < nq; q0 += chunk) {
    const size_t m = std::min(chunk, nq - q0);
    rc = run_dist(c, (const uint8_t*)needle_descs + q0 * kDescBytes, m);
    if (rc) return rc;
    // number of matches and, exactly, the k-th smallest score of every needle
    CBH_HIP(hipMemsetAsync(c->d_hist, 0, m * kWin * 4, c->stream));
    CBH_HIP(hipMemsetAsync(c->d_valid, 0, m * 4, c->stream));
    CBH_HIP(hipMemsetAsync(c->d_ncand, 0, m * 4, c->stream));
    CBH_HIP(hipMemsetAsync(c->d_smin, 0x7f, m * 4, c->stream));  // 0x7f7f7f7f: above every score
    const unsigned gx = (unsigned)std::min<size_t>((c->n + 255) / 256, 128);
    hipLaunchKernelGGL(k_color_min, dim3(gx, (unsigned)m), dim3(256), 0, c->stream, c->d_scores, c->d_ids,
                       (uint32_t)c->n, c->d_smin);
    hipLaunchKernelGGL(k_color_hist, dim3(gx, (unsigned)m), dim3(256), 0, c->stream, c->d_scores, c->d_ids,
                       (uint32_t)c->n, c->d_smin, c->d_hist, c->d_valid);
    h_valid.resize(m);
    CBH_HIP(hipMemcpyAsync(h_valid.data(), c->d_valid, m * 4, hipMemcpyDeviceToHost, c->stream));
    if (topk) {
      hipLaunchKernelGGL(k_color_thresh, dim3((unsigned)m), dim3(256), 0, c->stream, c->d_hist, (uint32_t)k,
                         c->d_smin, c->d_thr);
      hipLaunchKernelGGL(k_color_collect, dim3(gx, (unsigned)m), dim3(256), 0, c->stream, c->d_scores, c->d_ids,
                         (uint32_t)c->n, c->d_thr, c->d_cand, c->d_ncand);
      h_ncand.resize(m);
      h_cand.resize(m * (size_t)kCandCap);
      CBH_HIP(hipMemcpyAsync(h_ncand.data(), c->d_ncand, m * 4, hipMemcpyDeviceToHost, c->stream));
      CBH_HIP(hipGetLastError());
      CBH_HIP(hipStreamSynchronize(c->stream));
      for (size_t q = 0; q < m; ++q)  // only the filled part of every candidate list
        if (h_ncand[q] && h_ncand[q] <= kCandCap)
          CBH_HIP(hipMemcpyAsync(h_cand.data() + q * kCandCap, c->d_cand + q * kCandCap, (size_t)h_ncand[q] * 8,
                                 hipMemcpyDeviceToHost, c->stream));
    }
    CBH_HIP(hipStreamSynchronize(c->stream));
    for (size_t q = 0; q < m; ++q) {
      counts[q0 + q] = h_valid[q];
      if (k == 0 || h_valid[q] == 0) continue;
      cbh_match* oq = out + (q0 + q) * (size_t)k;
      if (topk && h_ncand[q] <= kCandCap) {
        unsigned long long* cq = h_cand.data() + q * kCandCap;
        std::sort(cq, cq + h_ncand[q]);  // (score, id): Database::searchIndex order with ties by id
        const size_t take = std::min<size_t>((size_t)k, h_ncand[q]);
        for (size_t j = 0; j < take; ++j) oq[j] = cbh_match{(uint32_t)cq[j], (int32_t)(cq[j] >> 32)};
        g_color_window_cuts++;
      } else {
        rc = color_full_sort_one(c, q, k, oq, h_valid[q]);
        if (rc) return rc;
        g_color_full_sorts++;
      }
    }
  }
  return CBH_OK;
}

}  // extern "C"

// ---- -sort-similar with AlgoColor: the tables on the device, then sortsimilar_table.hip's chain ------------------------
namespace {

int cs_fail(int code, const char* why) {
  cbh::set_last_error_text(why);
  return code;
}

struct StreamDrain {  // host vectors feed asynchronous copies: no way out of the call before the stream has run dry
  hipStream_t s;
  ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

constexpr uint32_t kNoPos = 0xffffffffu;

// under c->mu.  first0: set_first rebased to 0; perm[g]: the caller's place (from the batch's first item) of the item
// that is g-th when every set is in ascending id order
int color_sort_similar(cbh_color* c, const uint32_t* ids, const uint8_t* needle_descs, const uint32_t* dir_id,
                       const uint8_t* under, const std::vector<uint64_t>& first0, const std::vector<uint32_t>& perm,
                       uint64_t budget_scores, const cbh_sort_table_params* p, uint32_t* out_ids,
                       cbh_sort_similar_result* out) {
  const size_t n_sets = first0.size() - 1, total = perm.size();
  // where the index holds the listed ids: one pass over the index, as slice() makes it
  std::vector<uint32_t> want(ids, ids + total);
  std::sort(want.begin(), want.end());
  want.erase(std::unique(want.begin(), want.end()), want.end());
  std::vector<uint32_t> where(want.size(), kNoPos);
  for (size_t i = 0; i < c->n; ++i) {
    const uint32_t id = c->host_ids[i];
    if (id == 0) continue;  // removed (:272-273)
    const auto it = std::lower_bound(want.begin(), want.end(), id);
    if (it == want.end() || *it != id) continue;
    if (where[it - want.begin()] != kNoPos) return cs_fail(CBH_E_UNSUPPORTED, "color sort similar: the index holds an id twice");
    where[it - want.begin()] = (uint32_t)i;
  }
  // every set in id order: ids, attributes, index positions (sets start at multiples of 4: the gather's loads), needles
  std::vector<uint32_t> s_id(total), s_dir(p->filter_parent ? total : 0), first_pos(n_sets);
  std::vector<uint64_t> pos_first(n_sets + 1, 0), sorted_first(n_sets);
  for (size_t s = 0; s < n_sets; ++s) pos_first[s + 1] = pos_first[s] + ((first0[s + 1] - first0[s] + 3) & ~(uint64_t)3);
  std::vector<uint32_t> pos(std::max<uint64_t>(pos_first[n_sets], 4), 0);
  std::vector<uint8_t> s_attr(total);
  std::vector<NeedleF> nf(total);
  static const uint8_t kNoDesc[kDescBytes] = {0};
  for (size_t s = 0; s < n_sets; ++s)
    for (uint64_t g = first0[s]; g < first0[s + 1]; ++g) {
      const uint32_t src = perm[g], id = ids[src];
      const uint32_t at = where[std::lower_bound(want.begin(), want.end(), id) - want.begin()];
      s_id[g] = id;
      s_attr[g] = (uint8_t)((at != kNoPos ? 1 : 0) | (under && under[src] ? 2 : 0));
      if (p->filter_parent) s_dir[g] = dir_id[src];
      if (src == first0[s]) first_pos[s] = (uint32_t)(g - first0[s]);
      pos[pos_first[s] + (g - first0[s])] = at != kNoPos ? at : 0;
      const uint8_t* own = needle_descs ? needle_descs + (size_t)src * kDescBytes : nullptr;
      decompress(own && own[256] > 0 ? own : at != kNoPos ? c->host_desc.data() + (size_t)at * kDescBytes : kNoDesc, &nf[g]);
    }

  if (!c->stream) CBH_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  hipStream_t st = c->stream;
  StreamDrain drain{st};
  cbh::Scratch scratch(st);
  uint32_t *d_id, *d_dir = nullptr, *d_first_pos, *d_pos, *d_out_ids;
  uint8_t* d_attr;
  uint64_t *d_first, *d_sorted_first;
  NeedleF* d_needles;
  cbh_sort_similar_result* d_out;
  CBH_HIP(scratch.get(&d_id, total * 4));
  CBH_HIP(scratch.get(&d_attr, total));
  if (p->filter_parent) CBH_HIP(scratch.get(&d_dir, total * 4));
  CBH_HIP(scratch.get(&d_first_pos, n_sets * 4));
  CBH_HIP(scratch.get(&d_first, (n_sets + 1) * 8));
  CBH_HIP(scratch.get(&d_sorted_first, n_sets * 8));
  CBH_HIP(scratch.get(&d_pos, pos.size() * 4));
  CBH_HIP(scratch.get(&d_needles, total * sizeof(NeedleF)));
  CBH_HIP(scratch.get(&d_out_ids, total * 4));
  CBH_HIP(scratch.get(&d_out, n_sets * sizeof(cbh_sort_similar_result)));
  // groups of consecutive sets whose tables fit the budget; sorted_first counts from each group's own block
  std::vector<size_t> group_end;
  for (size_t g0 = 0; g0 < n_sets;) {
    size_t g1 = g0;
    uint64_t scores = 0;
    while (g1 < n_sets) {
      const uint64_t n = first0[g1 + 1] - first0[g1], t = n * cbh::sort_table_row_stride((uint32_t)n);
      if (g1 > g0 && scores + t > budget_scores) break;
      scores += t, ++g1;
    }
    (void)cbh::sort_table_layout(first0.data() + g0, g1 - g0, sorted_first.data() + g0);
    group_end.push_back(g1);
    g0 = g1;
  }
  CBH_HIP(hipMemcpyAsync(d_id, s_id.data(), total * 4, hipMemcpyHostToDevice, st));
  CBH_HIP(hipMemcpyAsync(d_attr, s_attr.data(), total, hipMemcpyHostToDevice, st));
  if (d_dir) CBH_HIP(hipMemcpyAsync(d_dir, s_dir.data(), total * 4, hipMemcpyHostToDevice, st));
  CBH_HIP(hipMemcpyAsync(d_first_pos, first_pos.data(), n_sets * 4, hipMemcpyHostToDevice, st));
  CBH_HIP(hipMemcpyAsync(d_first, first0.data(), (n_sets + 1) * 8, hipMemcpyHostToDevice, st));
  CBH_HIP(hipMemcpyAsync(d_sorted_first, sorted_first.data(), n_sets * 8, hipMemcpyHostToDevice, st));
  CBH_HIP(hipMemcpyAsync(d_pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, st));
  CBH_HIP(hipMemcpyAsync(d_needles, nf.data(), total * sizeof(NeedleF), hipMemcpyHostToDevice, st));

  const bool timing = g_color_sort_timing.load() != 0;
  float fill_ms = 0.f, chain_ms = 0.f;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  if (timing)
    for (hipEvent_t& e : ev) CBH_HIP(hipEventCreate(&e));
  int rc = CBH_OK;
  size_t g0 = 0;
  for (size_t g1 : group_end) {
    uint32_t largest = 0;
    uint64_t chunk_scores = 1;
    for (size_t s = g0; s < g1; ++s) {
      const uint32_t n = (uint32_t)(first0[s + 1] - first0[s]);
      largest = std::max(largest, n);
      if (n) chunk_scores = std::max<uint64_t>(chunk_scores, (uint64_t)color_chunk(n, n, (size_t)1 << 24) * n);
    }
    const uint64_t group_scores = cbh::sort_table_layout(first0.data() + g0, g1 - g0, sorted_first.data() + g0);
    const size_t cap = ((size_t)largest + 3) & ~(size_t)3;
    cbh::Scratch gs(st);
    uint16_t* table;
    float *pl, *pu, *pv;
    unsigned char* pnum;
    uint32_t* pids;
    int* d_scores;
    hipError_t e = gs.get(&table, group_scores * 2);
    if (e == hipSuccess) e = gs.get(&pl, std::max<size_t>(cap, 4) * kNC * 4);
    if (e == hipSuccess) e = gs.get(&pu, std::max<size_t>(cap, 4) * kNC * 4);
    if (e == hipSuccess) e = gs.get(&pv, std::max<size_t>(cap, 4) * kNC * 4);
    if (e == hipSuccess) e = gs.get(&pnum, std::max<size_t>(cap, 4));
    if (e == hipSuccess) e = gs.get(&pids, std::max<size_t>(cap, 4) * 4);
    if (e == hipSuccess) e = gs.get(&d_scores, chunk_scores * 4);
    if (e == hipSuccess && timing) e = hipEventRecord(ev[0], st);
    if (e != hipSuccess) {
      rc = cbh::fail("color sort similar: a group's scratch", e);
      break;
    }
    for (size_t s = g0; s < g1 && rc == CBH_OK && c->n > 0; ++s) {
      const uint32_t n = (uint32_t)(first0[s + 1] - first0[s]);
      if (n < 2) continue;  // no queries
      const uint32_t stride = cbh::sort_table_row_stride(n);
      const size_t cap_s = ((size_t)n + 3) & ~(size_t)3;
      rc = cbh::launch_slice_color(c->dL, c->dU, c->dV, c->d_num, c->d_ids, c->cap, d_pos + pos_first[s], n, pl, pu, pv,
                                   pnum, pids, cap_s, st);
      if (rc) break;
      hipLaunchKernelGGL(k_color_absent, dim3((n + 255) / 256), dim3(256), 0, st, d_attr + first0[s], n, pnum);
      const size_t chunk = color_chunk(n, n, (size_t)1 << 24);
      for (size_t r0 = 0; r0 < n && rc == CBH_OK; r0 += chunk) {
        const size_t m = std::min<size_t>(chunk, n - r0);
        rc = launch_dist(pl, pu, pv, pnum, cap_s, n, d_needles + first0[s] + r0, m, d_scores, nullptr, st);
        if (rc) break;
        const size_t words = m * (stride / 2);
        hipLaunchKernelGGL(k_color_table, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, d_scores, (uint32_t)m, n,
                           stride, reinterpret_cast<uint32_t*>(table + sorted_first[s] + r0 * stride));
      }
    }
    if (rc == CBH_OK && (e = hipGetLastError()) != hipSuccess) rc = cbh::fail("color sort similar: the table fill", e);
    if (rc != CBH_OK) break;
    if (timing) (void)hipEventRecord(ev[1], st);
    rc = cbh::launch_sort_table_chain(table, d_sorted_first + g0, d_id, d_attr, d_dir, d_first_pos + g0, d_first + g0, 0,
                                      g1 - g0, largest, p, d_out_ids, d_out + g0, st);
    if (rc != CBH_OK) break;
    if (timing) {
      float a = 0.f, b = 0.f;
      (void)hipEventRecord(ev[2], st);
      if (hipEventSynchronize(ev[2]) == hipSuccess && hipEventElapsedTime(&a, ev[0], ev[1]) == hipSuccess &&
          hipEventElapsedTime(&b, ev[1], ev[2]) == hipSuccess)
        fill_ms += a, chain_ms += b;
    }
    g0 = g1;
  }
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  if (rc != CBH_OK) return rc;
  if (total) CBH_HIP(hipMemcpyAsync(out_ids, d_out_ids, total * 4, hipMemcpyDeviceToHost, st));
  CBH_HIP(hipMemcpyAsync(out, d_out, n_sets * sizeof(cbh_sort_similar_result), hipMemcpyDeviceToHost, st));
  CBH_HIP(hipStreamSynchronize(st));
  g_color_sort_stat[0].store((long long)group_end.size());
  g_color_sort_stat[1].store(timing ? (long long)(fill_ms * 1000.f) : 0);
  g_color_sort_stat[2].store(timing ? (long long)(chain_ms * 1000.f) : 0);
  return CBH_OK;
}

}  // namespace

extern "C" int cbh_color_sort_similar(cbh_color* c, const uint32_t* ids, const void* needle_descs, const uint32_t* dir_id,
                                      const uint8_t* under_prefix, const uint64_t* set_first, size_t n_sets,
                                      const cbh_sort_table_params* params, uint32_t* out_ids,
                                      cbh_sort_similar_result* out) {
  if (!c) return CBH_E_INVAL;
  int rc = cbh::sort_table_params_ok(params, dir_id, under_prefix);
  if (rc != CBH_OK) return rc;
  if (n_sets == 0) return CBH_OK;
  if (!set_first || !out) return cs_fail(CBH_E_INVAL, "color sort similar: a required pointer is NULL");
  const int kb = g_color_sort_table_kb.load();
  const uint64_t budget_scores = (kb > 0 ? (uint64_t)kb * 1024 : kSortTableBytes) / 2;
  for (size_t s = 0; s < n_sets; ++s) {
    if (set_first[s + 1] < set_first[s]) return cs_fail(CBH_E_INVAL, "color sort similar: set_first is not ascending");
    const uint64_t n = set_first[s + 1] - set_first[s];
    if (n > CBH_COLOR_SORT_SIMILAR_MAX)
      return cs_fail(CBH_E_UNSUPPORTED, "color sort similar: a set above CBH_COLOR_SORT_SIMILAR_MAX items");
    if (n * cbh::sort_table_row_stride((uint32_t)n) > budget_scores)
      return cs_fail(CBH_E_UNSUPPORTED, "color sort similar: a set's table does not fit \"color_sort_table_kb\"");
  }
  const uint64_t base = set_first[0], total = set_first[n_sets] - base;
  if (n_sets > 0xfffffff0ull || total > 0xfffffff0ull)
    return cs_fail(CBH_E_INVAL, "color sort similar: more than 2^32 sets or items in one call");
  if (total && (!ids || !out_ids)) return cs_fail(CBH_E_INVAL, "color sort similar: a required pointer is NULL");
  if (total == 0) {
    memset(out, 0, n_sets * sizeof(cbh_sort_similar_result));
    return CBH_OK;
  }
  // every set in ascending id order, on the host: positions then order like ids
  std::vector<uint64_t> first0(n_sets + 1);
  for (size_t s = 0; s <= n_sets; ++s) first0[s] = set_first[s] - base;
  std::vector<uint32_t> perm(total);
  for (uint64_t i = 0; i < total; ++i) perm[i] = (uint32_t)i;
  const uint32_t* id0 = ids + base;
  for (size_t s = 0; s < n_sets; ++s) {
    std::sort(perm.begin() + first0[s], perm.begin() + first0[s + 1], [&](uint32_t a, uint32_t b) { return id0[a] < id0[b]; });
    for (uint64_t g = first0[s]; g < first0[s + 1]; ++g) {
      if (id0[perm[g]] == 0) return cs_fail(CBH_E_INVAL, "color sort similar: an item has id 0");
      if (g > first0[s] && id0[perm[g]] == id0[perm[g - 1]])
        return cs_fail(CBH_E_INVAL, "color sort similar: an id occurs twice in one set");
    }
  }
  cbh::DeviceGuard g(c->device);
  if (!g.ok) return CBH_E_NODEVICE;
  std::lock_guard<std::mutex> lk(c->mu);
  return color_sort_similar(c, id0, needle_descs ? (const uint8_t*)needle_descs + base * kDescBytes : nullptr,
                            dir_id ? dir_id + base : nullptr, under_prefix ? under_prefix + base : nullptr, first0, perm,
                            budget_scores, params, out_ids + base, out);
}
