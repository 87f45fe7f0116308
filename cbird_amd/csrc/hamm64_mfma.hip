// hamm64_mfma.hip -- K3m: the all-pairs 64-bit Hamming threshold scan on the gfx950 matrix cores.
//
// Same contract as k_hamm64_scan (hamm64_scan.hip): every pair with
//   hamm64(q, hash[i]) < thresh  &&  id[i] != 0  &&  q != 0
// (src/dcthashindex.cpp:196-217, hamm64 = popcountll(a ^ b), src/hamm.h:24-26) is appended as
// a cbh_record.  Only the arithmetic differs.
//
// Why the matrix cores.  PMC shows the VALU scan is bound by integer-VALU issue (one
// v_bcnt_u32_b32 per 32 bits per pair), not by memory: 0.8 GB of HBM traffic per 10^12 pairs.
// The distance is also a dot product of sign vectors (fp4_sign.h),
//   dot(s(a), s(b)) = 64 - 2 * hamm64(a, b),
// +-1.0 are exact in FP4, so ONE v_mfma_scale_f32_32x32x64_f8f6f4 (K = 64 = one hash) yields
// the exact distances of 32 haystack rows x 32 needles: 1024 pairs in ~32 matrix-core cycles,
// against ~8.3 (prefilter) / 14.3 (full) VALU cycles per 64 pairs.  All sums are small integers,
// so the f32 accumulation is exact and results stay bit-identical.  The VALU shares its issue port with the MFMAs, so
// every kernel here packs several needle tiles' results into one accumulator register (MX block scales put each tile
// in a bit field of its own) and reduces registers with one cheap operation before it looks at any of them.
//
// Structure.  A workgroup is 4 waves; each wave keeps its haystack tiles (32 rows each) expanded to FP4 in VGPRs and
// streams needle operands -- expanded once per call by k_expand_needles into the scratch NeedleScratch describes --
// through 16-byte buffer loads that the 4 waves share in L1/L2 (needle_loop: one double-buffered loop for every kernel).
// Which kernel runs is decided in hamm64_scan.hip and handed to launch_hamm64_scan_mfma as a ScanVariant:
//   * the prefilters (prefilter_body over a description Pre32 / Pre48 / Pre16: k_hamm64_mfma<true>, k_hamm64_mfma48,
//     k_hamm64_mfma16) compare a shorter word that bounds the distance from below, four needle tiles per accumulator,
//     and re-check the rare candidates on all 64 bits.  A description states the word, its operands and its MFMA chain;
//     candidate events, drain, re-check and records are written once;
//   * Full is FULL3 (k_hamm64_mfma3, thresholds <= 64): three needle tiles per accumulator on all 64 bits, and FULL2
//     (k_hamm64_mfma<false>, threshold 65 only): two.  They share the tile load, the queue entry format and the record tail.
// Every kernel parks its records in wave-private LDS and appends them with one atomic (out_push / out_flush): every
// append to the result block moves its counter, ONE address for the whole device, and the L2 takes ~10 ns per atomic on
// one address whatever its operand -- 10^6 self matches of a self-join are 10 ms of serial atomics beside a 9-16 ms scan
// (profiles/r06_adaptive_ab_before.jsonl).  How the variants came about, and what was tried and dropped: NOTES.md.
#include <algorithm>
#include <mutex>
#include <vector>

#include "cbh_internal.h"
#include "fp4_sign.h"

namespace cbh {
namespace {

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef unsigned v4u_t __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kHT = 8;  // haystack tiles a wave keeps in registers (256 rows)
constexpr int kG = 2;   // tiles per accumulator group
// the MX block scale 2^e (E8M0 127 + e) in every byte of a scale operand
constexpr int e8m0(int e) { return (int)((uint32_t)(127 + e) * 0x01010101u); }

// ---- the expanded-needle scratch -----------------------------------------------------------------------------------------
// Four regions of uint4 (16 bytes) over nq_pad needles, nq rounded up to kNeedlePad with hash 0:
//   words  2 per needle: needle j -> the FP4 expansions of its low and high word at [2j], [2j + 1] (FULL2, FULL3)
//   fold   1 per needle: of the prefilter word lo ^ hi (Pre32)
//   pre48  per quadruple of needle tiles P Q R S (128 needles) the B operands of its three MFMAs, 64 lanes each.  Lane
//          (c, K block kb) of MFMA m holds sub-blocks 2 (2m + kb) and 2 (2m + kb) + 1 of the twelve  P.E0 P.E1 P.E2 Q.E0
//          ... S.E2  of column c's four needles: sub-block s belongs to needle tile s / 3 and is its word's sub-block
//          s % 3 (pre48_sub), at +-0.5 except Q.E0, R.E1, S.E0 (s = 3, 7, 9) at +-4 -- the complement of the haystack's
//          magnitudes (Pre48)
//   pre16  per quadruple ONE B operand of 64 lanes: lane (c, K block kb) = fold16 of needle c of tile 2 kb at +-0.5 |
//          fold16 of needle c of tile 2 kb + 1 at +-4 (Pre16)
constexpr uint32_t kNeedlePad = 384;
constexpr uint32_t kNeedleBytes = 80;  // of scratch per padded needle
struct NeedleScratch {
  uint32_t nq_pad;
  __host__ __device__ constexpr uint32_t words() const { return 0u; }
  __host__ __device__ constexpr uint32_t fold() const { return 2u * nq_pad; }
  __host__ __device__ constexpr uint32_t pre48() const { return 3u * nq_pad; }
  __host__ __device__ constexpr uint32_t pre16() const { return pre48() + nq_pad / 128u * 192u; }
  __host__ __device__ constexpr uint32_t total() const { return pre16() + nq_pad / 128u * 64u; }
};
static_assert(kNeedlePad % 64u == 0 && kNeedlePad % 96u == 0 && kNeedlePad % 128u == 0,
              "whole pairs, triples and quadruples of needle tiles");
static_assert(NeedleScratch{kNeedlePad}.total() * 16u == kNeedlePad * kNeedleBytes &&
                  NeedleScratch{5u * kNeedlePad}.total() * 16u == 5u * kNeedlePad * kNeedleBytes,
              "the regions add up to kNeedleBytes per padded needle");

__global__ __launch_bounds__(256) void k_expand_needles(const uint64_t* __restrict__ q, uint32_t nq,
                                                        uint32_t nq_pad, uint4* __restrict__ qx) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // one thread per output uint4
  const NeedleScratch L{nq_pad};
  if (i >= L.total()) return;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(q);
  if (i < L.fold()) {
    qx[i] = fp4_expand32((i >> 1) < nq ? w[i] : 0u);
  } else if (i < L.pre48()) {
    const uint32_t j = i - L.fold();
    qx[i] = fp4_expand32(j < nq ? w[2u * j] ^ w[2u * j + 1u] : 0u);
  } else if (i < L.pre16()) {
    const uint32_t u = i - L.pre48(), quad = u / 192u, m = (u % 192u) >> 6, c = u & 31u, kb = (u >> 5) & 1u;
    uint2 o[2];
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
      const uint32_t s = 2u * (2u * m + kb) + k, j = quad * 128u + (s / 3u) * 32u + c;
      const uint32_t lo = j < nq ? w[2u * j] : 0u, hi = j < nq ? w[2u * j + 1u] : 0u;
      o[k] = fp4_expand16(pre48_sub(lo, hi, s % 3u), s == 3u || s == 7u || s == 9u ? kFp4Four : kFp4Half);
    }
    qx[i] = make_uint4(o[0].x, o[0].y, o[1].x, o[1].y);
  } else {
    const uint32_t u = i - L.pre16(), c = u & 31u, kb = (u >> 5) & 1u;
    const uint32_t j0 = (u >> 6) * 128u + kb * 64u + c, j1 = j0 + 32u;
    const uint2 lo = fp4_expand16(j0 < nq ? fold16(w[2u * j0], w[2u * j0 + 1u]) : 0u, kFp4Half);
    const uint2 hi = fp4_expand16(j1 < nq ? fold16(w[2u * j1], w[2u * j1 + 1u]) : 0u, kFp4Four);
    qx[i] = make_uint4(lo.x, lo.y, hi.x, hi.y);
  }
}

// ---- what every kernel shares ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t as_u32(float f) { return __builtin_bit_cast(uint32_t, f); }
// The queues below are wave-private and the LDS executes one wave's instructions in order, so a
// ds_read issued after a ds_write of another lane of the same wave sees it: only the COMPILER must
// be kept from reordering or caching LDS accesses across the hand-over points (a compiler-level memory
// clobber; `volatile` would make it wait for every outstanding needle prefetch at each access).
__device__ __forceinline__ void wave_order() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}
// wave compaction: base + the number of lanes below this one that are set in the ballot m
__device__ __forceinline__ uint32_t wave_rank(uint64_t m, uint32_t base = 0u) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, base));
}
// inclusive prefix sum of v over the 64 lanes (all active): six v_add_u32 with a DPP operand -- four shifts inside each
// row of 16 lanes, then the last lane of rows 0 | 2 onto rows 1 | 3 and lane 31 onto rows 2 and 3.  (DPP controls
// row_shr:n = 0x110 + n, row_bcast:15 = 0x142, row_bcast:31 = 0x143; lanes that a shift or a row mask leaves without a
// source add the `old` operand, 0.)
__device__ __forceinline__ uint32_t wave_prefix_sum(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
  return v;
}
// C/D layout of the 32x32 MFMA: column = lane & 31 -> needle, accumulator register g of `lane` -> this haystack row of
// the tile.  Register 16 t + g of a group of tiles counts on into tile t: the result gains 32 t.
__device__ __forceinline__ uint32_t cd_row(uint32_t g, uint32_t lane) { return (g & 3u) + 8u * (g >> 2) + 4u * (lane >> 5); }

struct HitParams {
  uint32_t thresh, n, nq, keep0;
  const uint64_t* q;
  const uint32_t* ids;
  cbh_record* rec;
  unsigned long long cap;
  unsigned long long* total;
  const uint2* hay;      // raw slot hashes, read only for the optional equal-bits filter
  const uint2* qmask;    // optional: bits of (needle ^ slot) that must be zero
};

// ---- records: parked per wave, appended with one atomic ---------------------------------------------------------------
// s_out = 2 * kOutCap words of the wave's LDS, nout = records parked (wave-uniform; callers keep it in an SGPR).
// All of these functions must be reached by the WHOLE wave (uniform control flow: they ballot).
constexpr uint32_t kOutCap = 128;
// (not inlined, the flush costs the prefilter kernel 144 bytes of scratch around the call and 1.5 ms per launch)
__device__ __forceinline__ void out_flush(uint32_t* s_out, uint32_t& nout, const HitParams& hp) {
  if (nout == 0) return;
  wave_order();
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(hp.total, (unsigned long long)nout);
  const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
  const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
  base = ((unsigned long long)bhi << 32) | blo;
  for (uint32_t k = lane; k < nout; k += 64u) {
    const uint2 r = *reinterpret_cast<const uint2*>(&s_out[2u * k]);
    if (base + k < hp.cap) hp.rec[base + k] = ((cbh_record)r.y << 32) | r.x;  // (past cap: counted, not stored)
  }
  wave_order();
  nout = 0;
}
// every lane with `has` contributes the record  needle qidx << 39 | dist << 32 | id
__device__ __forceinline__ void out_push(uint32_t* s_out, uint32_t& nout, bool has, uint32_t qidx, uint32_t dist,
                                         uint32_t id, const HitParams& hp) {
  const uint64_t m = __builtin_amdgcn_ballot_w64(has);
  if (m == 0) return;
  const uint32_t c = (uint32_t)__popcll(m);
  if (nout + c > kOutCap) out_flush(s_out, nout, hp);
  if (has) *reinterpret_cast<uint2*>(&s_out[2u * wave_rank(m, nout)]) = make_uint2(id, (qidx << 7) | dist);
  nout += c;
}

// the reference's approximate structures compare a needle only with entries sharing its low bits
__device__ __forceinline__ bool mask_ok(const HitParams& hp, uint32_t row, uint32_t qi, uint64_t nv) {
  if (!hp.qmask) return true;
  const uint2 hv = hp.hay[row], mk = hp.qmask[qi];
  return (((hv.x ^ (uint32_t)nv) & mk.x) | ((hv.y ^ (uint32_t)(nv >> 32)) & mk.y)) == 0;
}
// the record tail: a lane whose pair (slot `row`, needle qi = nv) is `under` the threshold parks its record if the slot
// exists, the call's mask lets the pair through and the slot has an id (or the caller keeps id 0)
__device__ __forceinline__ void out_match(uint32_t* s_out, uint32_t& nout, bool under, uint32_t row, uint32_t qi,
                                          uint64_t nv, uint32_t dist, const HitParams& hp) {
  bool has = false;
  uint32_t id = 0;
  if (under && row < hp.n && mask_ok(hp, row, qi, nv)) {
    id = hp.ids[row];
    has = id != 0 || hp.keep0;
  }
  out_push(s_out, nout, has, qi, dist, id, hp);
}

// ---- the needle loop ------------------------------------------------------------------------------------------------------
// A wave's needle operands are 1024-byte blocks (64 lanes x 16 bytes at byte `voff` of the block) in a row behind
// `base`; step s of `nsteps` takes blocks [N s, N s + N), each clamped to block `last` (a lone last pair of Pre32).
// Two steps per trip with explicit double buffers: the loads of the next step are in flight while the MFMAs of the
// current one run, and no register moves next -> current or vector address updates are spent on the prefetch, in
// kernels bound by what the VALU issues beside the MFMAs (NOTES 11).  Raw buffer loads: descriptor base, scalar
// byte offset of the block, constant per-lane offset; a block index chosen by s_min_u32, so that all loads are issued
// back to back (a select became vector code).
template <int N, class Step>
__device__ __forceinline__ void needle_loop(const uint4* base, uint32_t voff, uint32_t nsteps, uint32_t last, Step&& step) {
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(base), 0, (int)0xffffffffu, 0x27000);
  auto load = [&](uint32_t s, uint4 (&o)[N]) __attribute__((always_inline)) {
#pragma unroll
    for (uint32_t m = 0; m < (uint32_t)N; ++m) {
      const v4u_t v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, (int)(min(s * N + m, last) * 1024u), 0);
      o[m] = make_uint4(v.x, v.y, v.z, v.w);
    }
  };
  uint4 x[N], y[N];
  load(0, x);
#pragma unroll 1
  for (uint32_t s = 0; s < nsteps; s += 2) {  // (two call sites of step(): its cold paths are large)
    load(min(s + 1, nsteps - 1), y);
    step(s, x);
    if (s + 1 < nsteps) {
      load(min(s + 2, nsteps - 1), x);
      step(s + 1, y);
    }
  }
}
constexpr uint32_t kNoClamp = 0xffffffffu;  // `last` of a stream whose blocks all exist

// ---- the prefilters -------------------------------------------------------------------------------------------------------
// A step takes a QUADRUPLE of needle tiles (pairs p, p + 1: 128 needles) against the wave's resident haystack tiles and
// leaves FOUR prefilter-word distances per accumulator register, as 6-bit fields at bits 0, 6, 12, 18: field f holds
// bias + (a multiple of) the dot product of needle tile f, biased by C0 so that "candidate" is bit 5 of the field; the top
// field's flag is the carry into the f32 exponent (bit 23 of the pattern: the exponent goes from 150 to 151).  Every
// element of field f ends with weight 64^f / 2.  The +-0.5 products are exact at an accumulator of 2^23 because the
// hardware adds the 32 products of a block (an integer) before it meets the accumulator -- checked on 4.3e9 results
// incl. 1e7 hits by tools/ubench/mfma_half_exact.hip.  OR-ing accumulators preserves "some flag is set": one result VGPR
// answers 256 prefilter comparisons.
constexpr uint32_t kFlagMaskPre = (1u << 5) | (1u << 11) | (1u << 17) | (1u << 23);
constexpr uint32_t kFieldOnes = 1u + (1u << 6) + (1u << 12) + (1u << 18);  // a bias in every field

// The candidate path.  A candidate costs the matrix pipe nothing but a handful of VALU slots when it is FOUND and
// is re-checked LATER, 64 at a time:
//   * the event: every lane whose OR of a group's flags is not clear appends ONE descriptor {flag bits of the two
//     reduction chains, lane | group | step} to the wave's pending list -- a ballot, an mbcnt and one ds_write_b64 for
//     all hit lanes of the group at once, no global memory access, no difference between one hit lane and sixty-four.
//     The lane does NOT find out which of its 32 accumulator registers held the flag (that took parking them in LDS and
//     reading them back -- most of what a candidate used to cost, NOTES 11);
//   * when 64 descriptors are pending at the end of a step (and at the end of the wave's needle chunk) the wave drains
//     the list: the descriptors become work items, one per flagged chain and candidate field, and the items are worked
//     off 64 at a time, one per lane -- its needle from global memory (64 lanes' loads in flight together), then ALL 17
//     or 15 haystack rows of its chain from LDS against it on their 32-bit fold, three instructions a row, and the rows
//     that survive on all 64 bits; real matches go to the wave's record buffer.  Every (row, needle) pair belongs to
//     one (lane, group, step), one chain and one field, so a match is emitted once.
// (An immediate scalar re-check -- s_load + s_bcnt1 per candidate -- was built first: no VALU at all, but every event
//  stalled the wave for a scalar-cache miss, 15.9 ms at threshold 6; NOTES 11.)
// The wave's words: pending list (2 words per descriptor) | record buffer | item list (1 word per item).
// Pending descriptors.  A group adds at most one per lane, a step has kHT / kG groups, a drain keeps npend & 63: a step
// that starts with <= 63 ends with <= 63 + 4 x 64 = 319, so the list is drained between steps only.
constexpr uint32_t kPendCap = 320;                          // descriptors the pending list holds
constexpr uint32_t kOutOff = 2u * kPendCap;                 // word offset of the record buffer
constexpr uint32_t kItemOff = kOutOff + 2u * kOutCap;       // word offset of the drain's item list
constexpr uint32_t kItemCap = 63u + 64u * 8u;               // items: the kept remainder + two chains x four fields of 64 descriptors
constexpr uint32_t kPreQueue = kItemOff + kItemCap + 1u;    // the prefilter kernels' words per wave
static_assert(kPendCap >= 63u + (kHT / kG) * 64u, "pending list: every lane of every group of a step");
static_assert(kG == 2, "a descriptor names the two reduction chains of a group of 32 registers");

// OR of accumulator registers [A, B) of a group (register r = tile r / 16, element r % 16), three and then two per
// v_or3_b32
template <int A, int B, int G>
__device__ __forceinline__ uint32_t or_regs(const v16f (&c)[G]) {
  static_assert(B - A >= 3, "range");
  uint32_t o = as_u32(c[A >> 4][A & 15]) | as_u32(c[(A + 1) >> 4][(A + 1) & 15]) | as_u32(c[(A + 2) >> 4][(A + 2) & 15]);
#pragma unroll
  for (int r = A + 3; r < B; r += 2)
    o |= as_u32(c[r >> 4][r & 15]) | (r + 1 < B ? as_u32(c[(r + 1) >> 4][(r + 1) & 15]) : 0u);
  return o;
}

#define CBH_SCALED_MFMA(A, B, C, SCALE_B) __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, C, 4, 4, 0, kScaleOne, 0, SCALE_B)

// One description per prefilter word, everything prefilter_body does not share:
//   kTiles     haystack tiles a wave keeps resident
//   kOps       16-byte needle operands per lane and step = MFMAs chained into one accumulator
//   operands() where its operand blocks start in the needle scratch: 1024 bytes each, kOps per quadruple
//   last_op()  the last block a wave whose chunk starts at pair p0 may read, relative to its first
//   hay()      the A operand of haystack row hv in K block `half`
//   bias()     what C0 puts into every field at threshold t
//   scale()    the B block scale of MFMA m in K block `half`
//   chain()    the group's kOps x kG MFMAs: tiles a[t0], a[t0 + 1] against the step's operands b, C0 -> c
//
// Pre32 (small thresholds while candidates are rare): the FOLD f(x) = lo(x) ^ hi(x).  Bit i of f(a) ^ f(b) is the XOR of
// bits i and i + 32 of a ^ b, so popc(f(a) ^ f(b)) <= popc(a ^ b) -- a lower bound on the distance that looks at all 64
// bits.  (The low word alone is also a lower bound, but the low-frequency coefficients of images agree far more often
// than chance; on image-derived hashes the fold passes 2-3x fewer false candidates -- exactly the rate of uniform random
// words -- NOTES 11.)  The block scale is per lane and K block, so lanes 0-31 (K 0..31) carry the folds of one needle
// tile and lanes 32-63 (K 32..63) the folds of the next, against the haystack's folds in both K blocks: ONE MFMA = 2048
// fold distances.  MFMA 0 carries tiles 0 | 1 with block scales 2^-1 | 2^5, MFMA 1 tiles 2 | 3 with 2^11 | 2^17; with
// b = thresh - 1 field i holds 16 + b + dot_i / 2 = 32 + b - d_i in [b, 32 + b]:  d_i <= b  <=>  bit 5.
// Its operands are addressed by PAIR: block p is pair p's 64 folds.  The chunk length is even, only the call's last pair
// can be single -- its partner slot is fed the same block again (the clamp) and its candidates fall out at qi >= nq.
struct Pre32 {
  static constexpr int kTiles = kHT, kOps = 2;
  static constexpr uint32_t operands(NeedleScratch L) { return L.fold(); }
  static __device__ __forceinline__ uint32_t last_op(uint32_t n_pairs, uint32_t p0) { return n_pairs - 1u - p0; }
  static __device__ __forceinline__ v8i hay(uint2 hv, uint32_t) { return fp4_operand(fp4_expand32(hv.x ^ hv.y)); }
  static __device__ __forceinline__ uint32_t bias(uint32_t t) { return 16u + (t - 1u); }
  static __device__ __forceinline__ int scale(int m, uint32_t half) {
    return m == 0 ? (half ? e8m0(5) : e8m0(-1)) : (half ? e8m0(17) : e8m0(11));
  }
  static __device__ __forceinline__ void chain(const v8i (&a)[kTiles], int t0, const v8i (&b)[kOps], const v16f& c0,
                                               const int (&sc)[kOps], v16f (&c)[kG]) {
#pragma unroll
    for (int t = 0; t < kG; ++t) c[t] = CBH_SCALED_MFMA(a[t0 + t], b[0], c0, sc[0]);
#pragma unroll
    for (int t = 0; t < kG; ++t) c[t] = CBH_SCALED_MFMA(a[t0 + t], b[1], c[t], sc[1]);
  }
};

// Pre48 (thresholds where the fold's candidates drown Pre32: 8 on image hashes): a 48-bit word -- 16 folds and 32 plain
// bits in three sub-blocks E0 E1 E2 of 16 (pre48_sub), a tighter lower bound whose candidates are a hundred times rarer
// -- for three MFMAs per quadruple P Q R S: 3/4 of FULL3's matrix work.  A haystack row is four sub-blocks of 16 elements
// per lane (8 VGPRs): K block 0 holds Y = (E0, E1, E2, E0 at +-4), K block 1 holds X = (E2, E0 at +-4, E1, E2), everything
// else at +-0.5.  MFMA m multiplies the haystack's sub-blocks m, m + 1 (operand registers [2m, 2m + 4) of the tile's
// eight: overlapping windows, which the compiler turns into three copies made once per wave, outside the loop) with
// needle sub-blocks 4m .. 4m + 3 (NeedleScratch):
//     K block 0 (Y)                         K block 1 (X)
//   0 P.E0 P.E1            x 2              P.E2 | Q.E0 (4 x 4)     x 2
//   1 Q.E1 Q.E2            x 2^7            R.E0 R.E1               x 2^10   (one side at 4, the other at 0.5)
//   2 R.E2 | S.E0 (4 x 4)  x 2^13           S.E1 S.E2               x 2^19
// A compare spans one scale block and a half; inside a split block the two fields differ by 0.5 * 0.5 against 4 * 4,
// a factor of 64 = one field.  Field f gains 24 - h_f (h_f = the 48-bit distance) on the 8 + thresh that C0 puts there:
// 32 + thresh - h_f, bit 5 set <=> h_f <= thresh.  One more than Pre32's bias: a field of h > 32 + thresh goes negative
// and borrows one from the field above, which then reads h <= thresh - 1 -- still every true match (h <= hamm64 <
// thresh); the wrapped field itself reads as flagged, a false candidate the re-check drops.  The top field S arrives whole
// in the last MFMA, so the accumulator stays inside [2^23, 2^24) until then.
// 6 tiles per wave at 3 workgroups per CU: the three windows of a tile's eight registers end up as three copies of
// four, the compiler does not overlap operand tuples: 12 VGPRs per tile.  With 8 tiles the kernel takes 185 VGPRs, two
// waves per SIMD, and runs 14.65 ms per 10^12 pairs against 14.0 (profiles/r08_lib_ab_ht6_over_ht8.json).
struct Pre48 {
  static constexpr int kTiles = 6, kOps = 3;
  static constexpr uint32_t operands(NeedleScratch L) { return L.pre48(); }
  static __device__ __forceinline__ uint32_t last_op(uint32_t, uint32_t) { return kNoClamp; }  // whole quadruples
  static __device__ __forceinline__ v8i hay(uint2 hv, uint32_t half) {
    const uint32_t e0 = pre48_sub(hv.x, hv.y, 0), e1 = pre48_sub(hv.x, hv.y, 1), e2 = pre48_sub(hv.x, hv.y, 2);
    const uint2 s0 = fp4_expand16(half ? e2 : e0, kFp4Half);
    const uint2 s1 = fp4_expand16(half ? e0 : e1, half ? kFp4Four : kFp4Half);
    const uint2 s2 = fp4_expand16(half ? e1 : e2, kFp4Half);
    const uint2 s3 = fp4_expand16(half ? e2 : e0, half ? kFp4Half : kFp4Four);
    return v8i{(int)s0.x, (int)s0.y, (int)s1.x, (int)s1.y, (int)s2.x, (int)s2.y, (int)s3.x, (int)s3.y};
  }
  static __device__ __forceinline__ uint32_t bias(uint32_t t) { return 8u + t; }
  static __device__ __forceinline__ int scale(int m, uint32_t half) {
    return m == 0 ? e8m0(1) : m == 1 ? (half ? e8m0(10) : e8m0(7)) : (half ? e8m0(19) : e8m0(13));
  }
  static __device__ __forceinline__ void chain(const v8i (&a)[kTiles], int t0, const v8i (&b)[kOps], const v16f& c0,
                                               const int (&sc)[kOps], v16f (&c)[kG]) {
#pragma unroll
    for (int m = 0; m < kOps; ++m)
#pragma unroll
      for (int t = 0; t < kG; ++t) {
        const v8i& h = a[t0 + t];
        c[t] = CBH_SCALED_MFMA((v8i{h[2 * m], h[2 * m + 1], h[2 * m + 2], h[2 * m + 3], 0, 0, 0, 0}), b[m], m ? c[t] : c0, sc[m]);
      }
  }
};

// Pre16 (threshold 1 of unrelated hashes; wherever its candidates are rare enough, thresholds <= 8): the 16-bit word
// fold16 (fp4_sign.h), ONE MFMA per quadruple, half of Pre32's matrix work, for candidates at the rate of 16-bit words
// (1.5e-5 per pair at threshold 1, 2.6e-4 at 2).  Both operands split each scale block of 32 elements by magnitude:
// sub-block 0 at +-0.5, sub-block 1 at +-4 (the haystack: fold16 at +-0.5 | the same at +-4, in both K blocks), so a
// block's sum is  0.25 dot(tile 2 kb) + 16 dot(tile 2 kb + 1)  with dot = 16 - 2 d16, and the B block scales 2 | 2^13
// put the four tiles at 0.5, 32, 2^11, 2^17 = 64^f / 2: field f gains 8 - d16_f on the 24 + b that C0 puts there,
// 32 + b - d16_f in [16 + b, 32 + b] -- no field goes negative, bit 5 set <=> d16_f <= b.
// C0 < 2^24 needs 24 + b < 32: thresholds 1..8 (launch_hamm64_scan_mfma refuses the rest).
struct Pre16 {
  static constexpr int kTiles = kHT, kOps = 1;
  static constexpr uint32_t operands(NeedleScratch L) { return L.pre16(); }
  static __device__ __forceinline__ uint32_t last_op(uint32_t, uint32_t) { return kNoClamp; }  // whole quadruples
  static __device__ __forceinline__ v8i hay(uint2 hv, uint32_t) {
    const uint32_t f = fold16(hv.x, hv.y);
    const uint2 s0 = fp4_expand16(f, kFp4Half), s1 = fp4_expand16(f, kFp4Four);
    return v8i{(int)s0.x, (int)s0.y, (int)s1.x, (int)s1.y, 0, 0, 0, 0};
  }
  static __device__ __forceinline__ uint32_t bias(uint32_t t) { return 24u + (t - 1u); }
  static __device__ __forceinline__ int scale(int, uint32_t half) { return half ? e8m0(13) : e8m0(1); }
  static __device__ __forceinline__ void chain(const v8i (&a)[kTiles], int t0, const v8i (&b)[kOps], const v16f& c0,
                                               const int (&sc)[kOps], v16f (&c)[kG]) {
#pragma unroll
    for (int t = 0; t < kG; ++t) c[t] = CBH_SCALED_MFMA(a[t0 + t], b[0], c0, sc[0]);
  }
};

#define CBH_MFMA_PARAMS                                                                                              \
  const uint2 *__restrict__ hay, const uint32_t *__restrict__ ids, uint32_t n, const uint64_t *__restrict__ q,       \
      const uint4 *__restrict__ qx, uint32_t nq, uint32_t n_pairs, uint32_t pairs_per_chunk, uint32_t thresh,        \
      cbh_record *__restrict__ rec, unsigned long long cap, unsigned long long *__restrict__ total, uint32_t keep0,  \
      const uint2 *__restrict__ qmask, const uint4 *__restrict__ qf
#define CBH_MFMA_ARGS hay, ids, n, q, qx, nq, n_pairs, pairs_per_chunk, thresh, rec, cap, total, keep0, qmask, qf

// The prefilter kernel over description V; qf = the needle scratch at V::operands().  (Pre32 and Pre16 at 4 workgroups
// per CU: 128 VGPRs; bound by VALU issue, and a fourth wave per SIMD hides more of it -- same box, compiled for 1 / 2 / 3 /
// 4: 10.8 / 10.8 / 10.1 / 9.8 ms.)
template <class V>
__device__ __forceinline__ void prefilter_body(CBH_MFMA_PARAMS) {
  constexpr int HT = V::kTiles, G = kG;
  __shared__ __attribute__((aligned(16))) uint32_t s_queue_[kWaves][kPreQueue];
  __shared__ __attribute__((aligned(16))) uint2 s_hay_[kWaves][HT * 32];  // raw hashes for the re-check
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // uniform, and known to be
  const uint32_t r = lane & 31u, half = lane >> 5;
  const uint32_t tile0 = (blockIdx.x * kWaves + wave) * HT;
  if (tile0 * 32u >= n) return;  // whole wave past the end (no workgroup barriers in this kernel)
  uint32_t* s_queue = s_queue_[wave];
  uint2* s_hay = s_hay_[wave];
  uint32_t* s_out = s_queue + kOutOff;
  uint32_t nout = 0;  // records parked in s_out (wave-uniform)

  v8i a[HT];
#pragma unroll
  for (int t = 0; t < HT; ++t) {
    const uint32_t row = (tile0 + t) * 32u + r;
    const uint2 hv = row < n ? hay[row] : make_uint2(0u, 0u);
    a[t] = V::hay(hv, half);
    if (half == 0) s_hay[t * 32 + r] = hv;
  }
  wave_order();
  v16f c0;
#pragma unroll
  for (int g = 0; g < 16; ++g) c0[g] = 8388608.0f + (float)(V::bias(thresh) * kFieldOnes);
  asm volatile("" : "+v"(c0));  // keep C0 resident: otherwise it is rebuilt (16 v_mov) every trip
  int scale[V::kOps];
#pragma unroll
  for (int m = 0; m < V::kOps; ++m) {
    scale[m] = V::scale(m, half);
    asm volatile("" : "+v"(scale[m]));
  }

  const uint32_t p0 = blockIdx.y * pairs_per_chunk;  // (even: launch_hamm64_scan_mfma)
  const uint32_t p1 = min(n_pairs, p0 + pairs_per_chunk);
  const HitParams hp = {thresh, n, nq, keep0, q, ids, rec, cap, total, hay, qmask};

  uint32_t npend = 0;  // descriptors waiting in s_queue (wave-uniform)
  uint32_t nitem = 0;  // work items waiting in s_item (wave-uniform)
  uint32_t* s_item = s_queue + kItemOff;
  // One ITEM per lane: a descriptor's flagged chain x candidate field = 17 or 15 haystack rows against ONE needle, on all
  // 64 bits.  (One DESCRIPTOR per lane made every pass run at the pace of its unluckiest lane: a top-field carry makes all
  // four fields of its chain candidates, a quarter of all candidates sit in the top field, so some lane of 64 nearly always
  // held four or more and the wave walked the rows four times for a mean of 1.75 candidates per lane.)
  // Whole batches of 64 only -- the newest items; the < 64 oldest wait for company, and for the chunk's end, as the
  // descriptors do: a batch costs its global-memory round trip and its row walk whether one lane works in it or all.
  auto work = [&](uint32_t idx, bool live) {
    const uint32_t it = s_item[idx];
    const uint32_t f = it & 3u, ch = (it >> 2) & 1u, L = (it >> 3) & 63u, pp = p0 + 2u * (it >> 11);
    // register rr of the group is wave row  row0 + cd_row(rr, L): a quad of registers is four rows in a row, and the
    // next quad starts eight rows on
    const uint32_t row0 = ((it >> 9) & 3u) * 64u;
    const uint32_t qi = pp * 64u + (L & 31u) + 32u * f;  // the needle of field f
    // all lanes' loads in flight together; a null needle (and one past nq: the padding, the partner of a lone last pair)
    // matches nothing
    const uint64_t nv = live && qi < hp.nq ? hp.q[qi] : 0;
    const uint32_t qlo = (uint32_t)nv, qhi = (uint32_t)(nv >> 32), qfold = qlo ^ qhi;
    // Bit k of the chain's row masks is register 16 ch + k of the group.  Chain 0 = registers 0..16 (quads 0..3 and the
    // first of quad 4): 17 bits; chain 1 = 17..31 (the rest of quad 4, quads 5..7): bits 1..15.
    const uint32_t rows = nv == 0 ? 0u : ch ? 0x0000fffeu : 0x0001ffffu;
    const uint2* hq = s_hay + row0 + cd_row(16u * ch, L);  // quad i of the chain: hq[8 i .. 8 i + 3]
    // First the FOLD of every row, all 64 bits only for the survivors: popc(fold(row) ^ fold(needle)) <= hamm64(row,
    // needle) whichever word raised the flag, and all but about one row of a flagged chain differ from the needle in
    // about 16 of the 32 fold bits.  Three instructions per row: the three-input xor, v_bcnt_u32_b32 onto 2^31 - thresh
    // (bit 31 of the sum <=> popc >= thresh) and v_alignbit_b32, which shifts that bit into the mask from below -- rows
    // go in from the last to the first, so row k ends in bit k.
    const uint32_t far0 = 0x80000000u - hp.thresh;
    uint32_t far = 0;  // bit k: row k is out on its fold alone
    auto shift_in = [&](uint32_t lo, uint32_t hi) __attribute__((always_inline)) {
      // (the builtin: written as lo ^ hi ^ qfold the compiler emits two v_xor_b32; 0x96 is the truth table of a ^ b ^ c)
      far = __builtin_amdgcn_alignbit(far, (uint32_t)__popc(__builtin_amdgcn_bitop3_b32(lo, hi, qfold, 0x96)) + far0, 31u);
    };
    {  // register 16, chain 0's seventeenth row; chain 1 reads its row 0 in that place, which `rows` leaves out
      const uint2 h = hq[ch ? 0u : 32u];
      shift_in(h.x, h.y);
    }
#pragma unroll
    for (int i = 3; i >= 0; --i) {
      const uint4* h4 = reinterpret_cast<const uint4*>(hq + 8 * i);
      const uint4 x = h4[0], y = h4[1];
      shift_in(y.z, y.w);
      shift_in(y.x, y.y);
      shift_in(x.z, x.w);
      shift_in(x.x, x.y);
    }
    // the survivors, lane by lane: a flagged chain usually has one, a carried chain's unflagged fields none
    uint32_t hit = 0;
    for (uint32_t sv = ~far & rows; sv != 0; sv &= sv - 1u) {
      const uint32_t k = (uint32_t)__builtin_ctz(sv);
      const uint2 hv = hq[k + (k & 0x1cu)];  // 8 (k >> 2) + (k & 3)
      if (__popc(hv.x ^ qlo) + __popc(hv.y ^ qhi) < hp.thresh) hit |= 1u << k;
    }
    hit <<= 16u * ch;  // as registers of the group
    // a needle can match several rows of a chain (duplicates): one record per lane and round; the loop is uniform -- the
    // record buffer ballots
    while (__builtin_amdgcn_ballot_w64(hit != 0) != 0) {
      const uint32_t wr = row0 + cd_row((uint32_t)__builtin_ctz(hit | 0x80000000u), L);
      const uint2 hv = s_hay[wr];
      out_match(s_out, nout, hit != 0, tile0 * 32u + wr, qi, nv, __popc(hv.x ^ qlo) + __popc(hv.y ^ qhi), hp);
      hit &= hit - 1u;
    }
  };
  // the pending descriptors -> items, 64 descriptors at a time (at most 8 items each behind the <= 63 kept: kItemCap),
  // and the full batches worked off; all: the kept descriptors and items too (the end of the wave's needle chunk)
  auto drain = [&](bool all) {
    wave_order();
    const uint32_t keep = all ? 0u : (npend & 63u);
    uint32_t k0 = keep;
    for (;;) {  // (one site of work(): its code is large)
      if (nitem < 64u && k0 < npend) {
        const uint2 e = *reinterpret_cast<const uint2*>(&s_queue[2u * min(k0 + lane, npend - 1u)]);
        // candidates: bit 4 c + f = field f in the rows of chain c (flag bits of chain c at 5 + c, 11 + c, 17 + c,
        // 23 + c).  A carry into the exponent (top field flagged) leaves the lower fields of that register unreadable,
        // and the OR cannot say which register it was: all four fields are candidates in that chain's rows.
        // (the four flags, six bits apart, brought together by ONE 24-bit multiply: 1 + 2^5 + 2^10 + 2^15 lands them on
        //  bits 15..18 and every other partial product on a bit of its own outside those, so nothing carries)
        uint32_t cm = 0;
#pragma unroll
        for (uint32_t c = 0; c < 2; ++c) {
          const uint32_t nb = ((((e.x >> (5u + c)) & 0x41041u) * 0x8421u) >> 15) & 0xfu;
          cm |= (nb > 7u ? 0xfu : nb) << (4u * c);
        }
        if (k0 + lane >= npend) cm = 0;
        // item = {lane | group | step} << 3 | chain << 2 | field.  A lane lists its own descriptor's items, one behind
        // the other from where the lanes below it end: one prefix sum of the per-lane counts for the wave, then a loop
        // over the lane's set bits (one turn for most lanes, four behind a carry).
        const uint32_t cnt = (uint32_t)__popc(cm), upto = wave_prefix_sum(cnt);
        uint32_t* dst = s_item + nitem + (upto - cnt);
        for (const uint32_t item0 = e.y << 3; cm != 0; cm &= cm - 1u) *dst++ = item0 | (uint32_t)__builtin_ctz(cm);
        nitem += (uint32_t)__builtin_amdgcn_readlane((int)upto, 63);
        k0 += 64u;
        wave_order();
        continue;
      }
      uint32_t idx;
      bool live = true;
      if (nitem >= 64u) {
        nitem -= 64u;
        idx = nitem + lane;
      } else if (all && nitem != 0) {
        idx = min(lane, nitem - 1u);
        live = lane < nitem;
        nitem = 0;
      } else {
        break;
      }
      work(idx, live);
      wave_order();
    }
    npend = keep;
  };

  // the group's flags.  Flag bits survive OR: v_or3_b32 takes two more registers per op (plain VGPR-only ops, cheaper to
  // issue than a packed max); two chains of 17 and 15 registers: 8 + 7 v_or3_b32 (16 + 16 would take 8 + 8)
  auto detect = [&](const v16f (&c)[G], const uint32_t group, const uint32_t step) __attribute__((always_inline)) {
    constexpr int R = G * 16;
    constexpr int RA = R / 2 + 1;
    const uint32_t half0 = or_regs<0, RA, G>(c), half1 = or_regs<RA, R, G>(c);
    const uint32_t flags = (half0 | half1) & kFlagMaskPre;
    const uint64_t hm = __builtin_amdgcn_ballot_w64(flags != 0);
    if (hm != 0) {
      // wave-uniform from here: some lane holds a candidate (one group in ~10 at threshold 5, every other at 6).
      // Every hit lane appends {flag bits of chain 0 | those of chain 1 one bit higher, lane | group | step}.
      // (the lane id through an opaque copy: the compiler otherwise hoists this path's lane-derived values out of the
      // chunk loop, runs out of its 128 registers and SPILLS them)
      static_assert(R == 32, "two chains of 17 and 15 registers");
      uint32_t ln = lane;
      asm volatile("" : "+v"(ln));
      if (flags != 0)
        *reinterpret_cast<uint2*>(&s_queue[2u * wave_rank(hm, npend)]) =
            make_uint2((half0 & kFlagMaskPre) | ((half1 & kFlagMaskPre) << 1), ln | (group << 6) | (step << 8));
      npend += (uint32_t)__popcll(hm);
      // (drained at the end of the step: 4 x 64 descriptors fit behind the <= 63 a drain leaves, and the drain's code
      //  sits once per step instead of once per group, profiles/r06_pre_drain_sites_ab.json)
    }
  };

  // step s of the chunk: the quadruple of pairs p0 + 2 s, p0 + 2 s + 1 against the HT resident haystack tiles, G tiles
  // at a time: kOps * G MFMAs in flight, G * 16 accumulator registers live.  A lone last pair's quadruple is whole in the
  // scratch (Pre32: its clamp; the others: padding needles, hash 0, dropped at qi >= nq).
  needle_loop<V::kOps>(qf + (size_t)(p0 >> 1) * (V::kOps * 64u), lane * 16u, (p1 - p0 + 1u) >> 1, V::last_op(n_pairs, p0),
                       [&](const uint32_t s, const uint4 (&nn)[V::kOps]) __attribute__((always_inline)) {
    v8i b[V::kOps];
#pragma unroll
    for (int m = 0; m < V::kOps; ++m) b[m] = fp4_operand(nn[m]);
#pragma unroll
    for (int t0 = 0; t0 < HT; t0 += G) {
      v16f c[G];
      V::chain(a, t0, b, c0, scale, c);
      detect(c, (uint32_t)(t0 / G), s);
    }
    if (npend >= 64u) drain(false);
  });
  if (npend | nitem) drain(true);
  out_flush(s_out, nout, hp);
}

template <bool PRE>
__global__ void k_hamm64_mfma(CBH_MFMA_PARAMS);
template <>
__global__ __launch_bounds__(kThreads, 4) void k_hamm64_mfma<true>(CBH_MFMA_PARAMS) { prefilter_body<Pre32>(CBH_MFMA_ARGS); }
__global__ __launch_bounds__(kThreads, 3) void k_hamm64_mfma48(CBH_MFMA_PARAMS) { prefilter_body<Pre48>(CBH_MFMA_ARGS); }
__global__ __launch_bounds__(kThreads, 4) void k_hamm64_mfma16(CBH_MFMA_PARAMS) { prefilter_body<Pre16>(CBH_MFMA_ARGS); }

// ---- FULL2 and FULL3: all 64 bits, two or three needle tiles per accumulator ------------------------------------------------
// Lane (r, half) holds word `half` of row r of each of the wave's kHT tiles
__device__ __forceinline__ void load_hay_words(const uint2* __restrict__ hay, uint32_t n, uint32_t tile0, v8i (&a)[kHT]) {
  const uint32_t r = threadIdx.x & 31u, half = (threadIdx.x >> 5) & 1u;
#pragma unroll
  for (int t = 0; t < kHT; ++t) {
    const uint32_t row = (tile0 + t) * 32u + r;
    const uint2 hv = row < n ? hay[row] : make_uint2(0u, 0u);
    a[t] = fp4_operand(fp4_expand32(half ? hv.y : hv.x));
  }
}
// A flagged tile's results go through a wave-private queue: the lanes that hold them list
//   dist << 12 | field << 10 | g << 6 | lane
// (ballot + wave_rank, the count in an SGPR), then the whole wave works the list off, one entry per lane: register g of
// `lane` is row cd_row of the tile, its field the needle 32 field + (lane & 31) of the step's, and out_match the tail.

// FULL2 (threshold 65 only, where every pair matches): K = the 64 bits of one hash; tile B is a second MFMA accumulated
// onto tile A's with the block scale 2^15, on C0 = 2^23 + 0x4040 + 64 * 2^15.  In [2^23, 2^24) one f32 ulp is 1, so the
// mantissa holds  (0x4040 + dotA) + 2^15 * (64 + dotB)  exactly, i.e. the f32 bit pattern is
//   hi16 = 0x4B00 + (64 + dotB) / 2 = 0x4B40 - distB,   lo16 = 0x4040 + dotA = 0x4080 - 2 distA
// (dotB even => bit 15 is 0): two distances per register, each half monotone in its distance.  Both halves are positive
// normal f16 bit patterns, so v_pk_maximum3_f16 takes the per-half maximum of three registers at once: 4 ops per MFMA,
// and one compare of the reduced maxima against per-threshold keys says whether a group holds anything.
constexpr uint32_t kLoZero2 = 0x4080u, kHiZero2 = 0x4B40u;  // lo16, hi16 at distance 0
__device__ __forceinline__ h2 as_h2(float f) { return __builtin_bit_cast(h2, f); }
__device__ __forceinline__ h2 pkmax3(h2 a, h2 b, h2 c) {
  return __builtin_elementwise_maximum(__builtin_elementwise_maximum(a, b), c);  // v_pk_maximum3_f16
}
// cold path (inlined once per haystack tile of the step's call site): one tile's 16 accumulators of pair p;
// lo16 << 16 >= lo_key  <=>  distA < thresh,  pattern >= hi_key  <=>  distB < thresh
__device__ __forceinline__ void handle_tile2(const v16f& c, uint32_t row0, uint32_t p, uint32_t lo_key, uint32_t hi_key,
                                             const HitParams& hp, uint32_t* s_queue, uint32_t* s_out, uint32_t& nout) {
  const uint32_t lane = threadIdx.x & 63u;
  {  // quick reject of the tile that did not cause the group's hit
    h2 m0 = {0, 0}, m1 = {0, 0};
#pragma unroll
    for (int g = 0; g < 16; g += 4) {
      m0 = pkmax3(m0, as_h2(c[g]), as_h2(c[g + 1]));
      m1 = pkmax3(m1, as_h2(c[g + 2]), as_h2(c[g + 3]));
    }
    const uint32_t tb = __builtin_bit_cast(uint32_t, __builtin_elementwise_maximum(m0, m1));
    if (__builtin_amdgcn_ballot_w64((tb << 16) >= lo_key || tb >= hi_key) == 0) return;
  }
  uint32_t cnt = 0;  // wave-uniform
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const uint32_t bits = as_u32(c[g]);
    const bool fh = bits >= hi_key;
    const bool fl = (bits << 16) >= lo_key;
    if (__builtin_amdgcn_ballot_w64(fh || fl) == 0) continue;  // scalar branch, rarely not taken
    const uint64_t mh = __builtin_amdgcn_ballot_w64(fh);
    if (fh) s_queue[wave_rank(mh, cnt)] = ((kHiZero2 - (bits >> 16)) << 12) | (1u << 10) | ((uint32_t)g << 6) | lane;
    cnt += (uint32_t)__popcll(mh);
    const uint64_t ml = __builtin_amdgcn_ballot_w64(fl);
    if (fl) s_queue[wave_rank(ml, cnt)] = (((kLoZero2 - (bits & 0xffffu)) >> 1) << 12) | ((uint32_t)g << 6) | lane;
    cnt += (uint32_t)__popcll(ml);
  }
  wave_order();
  for (uint32_t k0 = 0; k0 < cnt; k0 += 64u) {
    const uint32_t k = k0 + lane;
    const uint32_t e = s_queue[min(k, cnt - 1u)];
    const uint32_t src = e & 63u, g = (e >> 6) & 15u, field = (e >> 10) & 1u, d = e >> 12;
    const uint32_t row = row0 + cd_row(g, src);
    const uint32_t qi = p * 64u + field * 32u + (src & 31u);
    // (the needle load under its branch: at this threshold the loop is the kernel, and FULL3's select form below, which
    //  compiles to a branch around the load as well, ran 0.03 % slower here -- earlier_calls.select_form and t65_variants
    //  in profiles/r11_refactor_lib_ab.json, NOTES 25)
    bool under = false;
    uint64_t nv = 0;
    if (k < cnt && row < hp.n && qi < hp.nq) {
      nv = hp.q[qi];
      under = nv != 0 && d < hp.thresh;
    }
    out_match(s_out, nout, under, row, qi, nv, d, hp);
  }
  wave_order();
}

template <>
__global__ __launch_bounds__(kThreads, 1) void k_hamm64_mfma<false>(CBH_MFMA_PARAMS) {
  constexpr int HT = kHT, G = kG;
  constexpr uint32_t kQueue = 2048;  // words per wave: two entries per register of a tile
  __shared__ uint32_t s_queue_[kWaves][kQueue];
  __shared__ uint32_t s_out_[kWaves][2 * kOutCap];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile0 = (blockIdx.x * kWaves + wave) * HT;
  if (tile0 * 32u >= n) return;  // whole wave past the end (no workgroup barriers in this kernel)
  uint32_t* s_queue = s_queue_[wave];
  uint32_t* s_out = s_out_[wave];
  uint32_t nout = 0;  // records parked in s_out (wave-uniform)

  v8i a[HT];
  load_hay_words(hay, n, tile0, a);
  v16f c0;
#pragma unroll
  for (int g = 0; g < 16; ++g) c0[g] = 8388608.0f + 16448.0f + 2097152.0f;  // 2^23 + 0x4040 + 64 * 2^15
  asm volatile("" : "+v"(c0));  // keep C0 resident: otherwise it is rebuilt (16 v_mov) every trip
  const uint32_t lo_key = (kLoZero2 - 2u * (thresh - 1u)) << 16, hi_key = (kHiZero2 - (thresh - 1u)) << 16;
  const HitParams hp = {thresh, n, nq, keep0, q, ids, rec, cap, total, hay, qmask};

  const uint32_t p0 = blockIdx.y * pairs_per_chunk;
  const uint32_t p1 = min(n_pairs, p0 + pairs_per_chunk);
  // pair p = needles [64p, 64p + 64): tile A = first 32, tile B = last 32, one block each; lane (c, half) reads word
  // `half` of needle c
  needle_loop<2>(qx + (size_t)p0 * 128u, (2u * (lane & 31u) + (lane >> 5)) * 16u, p1 - p0, kNoClamp,
                 [&](const uint32_t s, const uint4 (&nn)[2]) __attribute__((always_inline)) {
    const v8i bA = fp4_operand(nn[0]), bB = fp4_operand(nn[1]);
#pragma unroll
    for (int t0 = 0; t0 < HT; t0 += G) {
      v16f c[G];
#pragma unroll
      for (int t = 0; t < G; ++t) c[t] = CBH_SCALED_MFMA(a[t0 + t], bA, c0, kScaleOne);
#pragma unroll
      for (int t = 0; t < G; ++t) c[t] = CBH_SCALED_MFMA(a[t0 + t], bB, c[t], e8m0(15));
      // packed per-half maximum of the group's G * 16 results: 8 v_pk_maximum3_f16 per tile
      h2 m0 = {0, 0}, m1 = {0, 0};
#pragma unroll
      for (int t = 0; t < G; ++t)
#pragma unroll
        for (int g = 0; g < 16; g += 4) {
          m0 = pkmax3(m0, as_h2(c[t][g]), as_h2(c[t][g + 1]));
          m1 = pkmax3(m1, as_h2(c[t][g + 2]), as_h2(c[t][g + 3]));
        }
      const uint32_t mb = __builtin_bit_cast(uint32_t, __builtin_elementwise_maximum(m0, m1));
      if (__builtin_amdgcn_ballot_w64((mb << 16) >= lo_key || mb >= hi_key) != 0) {
        // wave-uniform from here: something in this group is under the threshold
#pragma unroll
        for (int t = 0; t < G; ++t)
          handle_tile2(c[t], (tile0 + t0 + t) * 32u, p0 + s, lo_key, hi_key, hp, s_queue, s_out, nout);
      }
    }
  });
  out_flush(s_out, nout, hp);
}
#undef CBH_MFMA_PARAMS
#undef CBH_MFMA_ARGS

// FULL3: detection by OR instead of maximum.
// The VALU reduction shares the issue port with the MFMAs (measured: an FP4 32x32x64 MFMA blocks it ~24 of
// its ~40 cycles, every VALU op adds 4), so fewer reduction ops per MFMA is the lever.  With w = 64 - dist
// and b = thresh - 1 the accumulator is built as
//   2^23 + 2 * sum_{i<3} 2^(7i) * (w_i + b)        (B scales 2^0, 2^7, 2^14; C0 carries 2^23 + the b terms)
// i.e. three 7-bit fields (w + b <= 127 for thresh <= 64), and  dist_i < thresh  <=>  w_i + b >= 64  <=>
// bit 6 of field i = bit 7 + 7i of the f32 pattern.  OR-ing registers keeps "some flag bit is set", so
// v_or3_b32 reduces two registers per op for THREE MFMAs' worth of results: 2.7 VALU ops per MFMA instead
// of 4, which makes the kernel matrix-core bound.
constexpr uint32_t kFlagMask3 = (1u << 7) | (1u << 14) | (1u << 21);

__device__ __forceinline__ void handle_tile3(const v16f& c, uint32_t row0, uint32_t p3, const HitParams& hp,
                                             uint32_t* s_queue, uint32_t* s_out, uint32_t& nout) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t any = 0;
#pragma unroll
  for (int g = 0; g < 16; ++g) any |= as_u32(c[g]);
  if (__builtin_amdgcn_ballot_w64((any & kFlagMask3) != 0) == 0) return;  // the other tile of the group
  const uint32_t b = hp.thresh - 1u;
  // one pass per field: the queue holds 16 registers x 64 lanes (4 KB per wave, so that LDS never limits the waves per
  // SIMD); the records of a tile come out field by field -- their order in the block is free
#pragma unroll 1
  for (uint32_t f = 0; f < 3; ++f) {
    uint32_t cnt = 0;  // wave-uniform
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const uint32_t bits = as_u32(c[g]);
      const bool fl = (bits >> (7u + 7u * f)) & 1u;
      const uint64_t m = __builtin_amdgcn_ballot_w64(fl);
      if (m == 0) continue;
      if (fl)
        s_queue[wave_rank(m, cnt)] = ((64u + b - ((bits >> (1u + 7u * f)) & 0x7fu)) << 12) | (f << 10) | ((uint32_t)g << 6) | lane;
      cnt += (uint32_t)__popcll(m);
    }
    wave_order();
    for (uint32_t k0 = 0; k0 < cnt; k0 += 64u) {
      const uint32_t k = k0 + lane;
      const uint32_t e = s_queue[min(k, cnt - 1u)];
      const uint32_t src = e & 63u, g = (e >> 6) & 15u, field = (e >> 10) & 3u, d = e >> 12;
      const uint32_t row = row0 + cd_row(g, src);
      const uint32_t qi = p3 * 96u + field * 32u + (src & 31u);
      const uint64_t nv = (k < cnt && row < hp.n && qi < hp.nq) ? hp.q[qi] : 0;
      out_match(s_out, nout, nv != 0, row, qi, nv, d, hp);
    }
    wave_order();
  }
}

// (2 workgroups per CU as the minimum: with at most 256 registers per lane the compiler keeps the accumulators in
//  VGPRs -- given 512 it puts them in AGPRs and adds a v_accvgpr_read_b32 for every register the OR reduction touches,
//  71 instead of 39 VALU instructions per six MFMAs; compiled for 4 workgroups per CU it spills: 35 ms.)
__global__ __launch_bounds__(kThreads, 2) void k_hamm64_mfma3(
    const uint2* __restrict__ hay, const uint32_t* __restrict__ ids, uint32_t n,
    const uint64_t* __restrict__ q, const uint4* __restrict__ qx, uint32_t nq, uint32_t n_triples,
    uint32_t triples_per_chunk, uint32_t thresh, cbh_record* __restrict__ rec,
    unsigned long long cap, unsigned long long* __restrict__ total, uint32_t keep0,
    const uint2* __restrict__ qmask) {
  constexpr int HT = kHT, G = kG;
  __shared__ uint32_t s_queue_[kWaves][16 * 64];
  __shared__ uint32_t s_out_[kWaves][2 * kOutCap];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile0 = (blockIdx.x * kWaves + wave) * HT;
  if (tile0 * 32u >= n) return;
  uint32_t* s_queue = s_queue_[wave];
  uint32_t* s_out = s_out_[wave];
  uint32_t nout = 0;

  v8i a[HT];
  load_hay_words(hay, n, tile0, a);
  // C0 = 2^23 + (64 + 2b) * (1 + 2^7 + 2^14): every field starts at 2 * (32 + b) and gains dot_i = 2 * (w_i - 32)
  const uint32_t b = thresh - 1u;
  v16f c0;
#pragma unroll
  for (int g = 0; g < 16; ++g) c0[g] = 8388608.0f + (float)((64u + 2u * b) * 16513u);
  asm volatile("" : "+v"(c0));
  const HitParams hp = {thresh, n, nq, keep0, q, ids, rec, cap, total, hay, qmask};

  const uint32_t p0 = blockIdx.y * triples_per_chunk;
  const uint32_t p1 = min(n_triples, p0 + triples_per_chunk);
  // triple p = needles [96p, 96p + 96): three tiles of 32, one block each; lane (c, half) reads word `half` of needle c
  needle_loop<3>(qx + (size_t)p0 * 192u, (2u * (lane & 31u) + (lane >> 5)) * 16u, p1 - p0, kNoClamp,
                 [&](const uint32_t s, const uint4 (&nn)[3]) __attribute__((always_inline)) {
    const v8i b0 = fp4_operand(nn[0]), b1 = fp4_operand(nn[1]), b2 = fp4_operand(nn[2]);
#pragma unroll
    for (int t0 = 0; t0 < HT; t0 += G) {
      v16f c[G];
#pragma unroll
      for (int t = 0; t < G; ++t) c[t] = CBH_SCALED_MFMA(a[t0 + t], b0, c0, kScaleOne);
#pragma unroll
      for (int t = 0; t < G; ++t) c[t] = CBH_SCALED_MFMA(a[t0 + t], b1, c[t], e8m0(7));
#pragma unroll
      for (int t = 0; t < G; ++t) c[t] = CBH_SCALED_MFMA(a[t0 + t], b2, c[t], e8m0(14));
      // one v_or3_b32 per two result registers, the last register and the mask in one v_bitop3_b32
      if (__builtin_amdgcn_ballot_w64((or_regs<0, G * 16, G>(c) & kFlagMask3) != 0) != 0) {
#pragma unroll
        for (int t = 0; t < G; ++t) handle_tile3(c[t], (tile0 + t0 + t) * 32u, p0 + s, hp, s_queue, s_out, nout);
      }
    }
  });
  out_flush(s_out, nout, hp);
}

// ---- the probe: candidate and true-match rates of THIS launch's data (the route in hamm64_scan.hip weighs them) --------
// k_fold_probe counts, on kProbeS x kProbeS (slot, needle) samples, the pairs whose fold distance and whose 64-bit distance
// are under each threshold up to kProbeT, and those the 48-bit prefilter would flag.
constexpr uint32_t kProbeS = 2048;     // samples per side
constexpr int kProbeT = kProbeMaxThresh;  // thresholds 1..8 are counted (the prefilter never pays beyond: 1e-3 per pair at 8)

// grid (sq / 256, sh / 64): thread = one needle sample against 64 slot samples; counts[t - 1] += pairs with fold
// distance < t, counts[kProbeT + t - 1] += pairs with 64-bit distance < t, counts[2 kProbeT + t - 1] += pairs with 48-bit
// distance <= t or > 32 + t, counts[3 kProbeT + t - 1] += pairs with fold16 distance < t.  The samples are pseudo-random rows / needles
// (a 32-bit mix of the sample number): evenly spaced ones meet the diagonal of a self-join far more often than its share
// -- a shard of 125 000 slots against its index's 10^6 needles counted 256 self matches among 4.2 x 10^6 sampled pairs,
// sixty times their true rate, which is how dht 7 first came to take the prefilter on a sharded handle.
__device__ __forceinline__ uint32_t probe_mix(uint32_t x) {
  x = ((x >> 16) ^ x) * 0x45d9f3bu;
  x = ((x >> 16) ^ x) * 0x45d9f3bu;
  return (x >> 16) ^ x;
}
__global__ __launch_bounds__(256) void k_fold_probe(const uint2* __restrict__ hay, uint32_t n, const uint2* __restrict__ q,
                                                    uint32_t nq, uint32_t sh, uint32_t sq, uint32_t* __restrict__ counts) {
  __shared__ uint2 s_h[64];
  __shared__ uint32_t s_cnt[4 * kProbeT];
  const uint32_t t = threadIdx.x;
  if (t < 64) {
    const uint32_t i = blockIdx.y * 64u + t;
    s_h[t] = i < sh ? hay[sh == n ? i : probe_mix(i) % n] : make_uint2(0u, 0u);
  }
  if (t < 4 * kProbeT) s_cnt[t] = 0;
  __syncthreads();
  const uint32_t j = blockIdx.x * 256u + t;
  const uint32_t nslots = min(64u, sh - blockIdx.y * 64u);
  uint32_t cnt[kProbeT] = {}, cnt64[kProbeT] = {}, cnt48[kProbeT] = {}, cnt16[kProbeT] = {};
  if (j < sq) {
    const uint2 nv = q[sq == nq ? j : probe_mix(j ^ 0x9e3779b9u) % nq];
    const uint32_t f = nv.x ^ nv.y;
    for (uint32_t k = 0; k < nslots; ++k) {
      const uint2 hv = s_h[k];
      const uint32_t d = (uint32_t)__popc(f ^ hv.x ^ hv.y);
#pragma unroll
      for (int th = 0; th < kProbeT; ++th) cnt[th] += d < (uint32_t)(th + 1) ? 1u : 0u;
      // the 48-bit prefilter word's candidates: distance <= threshold, or a field that wraps (its flag rule, see the kernel)
      const uint32_t d48 = (uint32_t)__popc((f ^ hv.x ^ hv.y) & 0xffffu) + (uint32_t)__popc((nv.x ^ hv.x) >> 16) +
                           (uint32_t)__popc((nv.y ^ hv.y) >> 16);
#pragma unroll
      for (int th = 0; th < kProbeT; ++th) cnt48[th] += d48 <= (uint32_t)(th + 1) || d48 > (uint32_t)(th + 33) ? 1u : 0u;
      const uint32_t x32 = f ^ hv.x ^ hv.y, d16 = (uint32_t)__popc((x32 ^ (x32 >> 16)) & 0xffffu);  // (fold16, fp4_sign.h)
#pragma unroll
      for (int th = 0; th < kProbeT; ++th) cnt16[th] += d16 < (uint32_t)(th + 1) ? 1u : 0u;
      if (d < (uint32_t)kProbeT) {  // (rare: a true match is a candidate first)
        const uint32_t d64 = (uint32_t)__popc(nv.x ^ hv.x) + (uint32_t)__popc(nv.y ^ hv.y);
#pragma unroll
        for (int th = 0; th < kProbeT; ++th) cnt64[th] += d64 < (uint32_t)(th + 1) ? 1u : 0u;
      }
    }
  }
#pragma unroll
  for (int th = 0; th < 4 * kProbeT; ++th) {
    uint32_t v = th < kProbeT ? cnt[th % kProbeT] : th < 2 * kProbeT ? cnt64[th % kProbeT]
                 : th < 3 * kProbeT ? cnt48[th % kProbeT] : cnt16[th % kProbeT];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((t & 63u) == 0 && v) atomicAdd(&s_cnt[th], v);
  }
  __syncthreads();
  if (t < 4 * kProbeT && s_cnt[t]) atomicAdd(&counts[t], s_cnt[t]);
}

// ---- self-test: the FP4 values and block scales PRE48 multiplies with ----------------------------------------------------
// One MFMA per (code a, code b, block scale, element count 1 | 16, K block): `cnt` elements of code a against as many of
// code b in that K block, everything else 0, C = 0; out = cnt * a * b * scale as the hardware returns it.
// (codes and scales by selects: a table indexed at run time would have to live in device memory)
__device__ __forceinline__ uint32_t selftest_fp4_code(uint32_t i) {  // 0.5, -0.5, 1, -1, 4, -4
  return ((i >> 1) == 0 ? kFp4Half : (i >> 1) == 1 ? 0x2u : kFp4Four) | ((i & 1u) << 3);
}
__global__ __launch_bounds__(64) void k_selftest_fp4(float* __restrict__ out) {
  const uint32_t lane = threadIdx.x, half = lane >> 5;
  for (uint32_t i = 0; i < 720u; ++i) {
    const uint32_t kb = i & 1u, ci = (i >> 1) & 1u, k = (i >> 2) % 5u, ib = (i / 20u) % 6u, ia = i / 120u;
    const uint32_t fa = selftest_fp4_code(ia) * (ci ? 0x11111111u : 1u), fb = selftest_fp4_code(ib) * (ci ? 0x11111111u : 1u);
    const bool on = half == kb;
    const v8i a = {on ? (int)fa : 0, on && ci ? (int)fa : 0, 0, 0, 0, 0, 0, 0};
    const v8i b = {on ? (int)fb : 0, on && ci ? (int)fb : 0, 0, 0, 0, 0, 0, 0};
    int sc = k == 0 ? e8m0(1) : k == 1 ? e8m0(7) : k == 2 ? e8m0(10) : k == 3 ? e8m0(13) : e8m0(19);
    asm volatile("" : "+v"(sc));
    v16f c = {};
    c = CBH_SCALED_MFMA(a, b, c, sc);
    asm volatile("" : "+v"(c));  // the MFMA stays in front of the branch: it needs the operands of all 64 lanes
    if (lane == 0) out[i] = c[0];
  }
}

// pinned words for the probe's answer: a free list (a slot is in use only inside one synchronous probe)
std::mutex g_probe_mu;
std::vector<uint32_t*> g_probe_free;
uint32_t* probe_slot_get() {
  {
    std::lock_guard<std::mutex> lk(g_probe_mu);
    if (!g_probe_free.empty()) {
      uint32_t* p = g_probe_free.back();
      g_probe_free.pop_back();
      return p;
    }
  }
  uint32_t* p = nullptr;
  if (hipHostMalloc(&p, 4 * kProbeT * sizeof(uint32_t)) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}
void probe_slot_put(uint32_t* p) {
  std::lock_guard<std::mutex> lk(g_probe_mu);
  g_probe_free.push_back(p);
}

#undef CBH_SCALED_MFMA

}  // namespace

bool probe_fold_rates(const uint64_t* d_hashes, size_t n, const uint64_t* d_q, size_t nq, int thresh, hipStream_t stream,
                      double* r_cand, double* r_true, double* r_cand48, double* r_cand16) {
  Scratch scratch(stream);
  uint32_t* d_cnt = nullptr;
  if (scratch.get(&d_cnt, 4 * kProbeT * sizeof(uint32_t)) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  uint32_t* h_cnt = probe_slot_get();
  bool ok = h_cnt != nullptr;
  const uint32_t sh = (uint32_t)std::min<size_t>(n, kProbeS), sq = (uint32_t)std::min<size_t>(nq, kProbeS);
  if (ok) {
    ok = hipMemsetAsync(d_cnt, 0, 4 * kProbeT * sizeof(uint32_t), stream) == hipSuccess;
    if (ok) {
      hipLaunchKernelGGL(k_fold_probe, dim3((sq + 255u) / 256u, (sh + 63u) / 64u), dim3(256), 0, stream,
                         reinterpret_cast<const uint2*>(d_hashes), (uint32_t)n, reinterpret_cast<const uint2*>(d_q),
                         (uint32_t)nq, sh, sq, d_cnt);
      ok = hipGetLastError() == hipSuccess &&
           hipMemcpyAsync(h_cnt, d_cnt, 4 * kProbeT * sizeof(uint32_t), hipMemcpyDeviceToHost, stream) == hipSuccess &&
           hipStreamSynchronize(stream) == hipSuccess;
    }
  }
  if (ok) {
    const double pairs = (double)sh * (double)sq;
    *r_cand = (double)h_cnt[thresh - 1] / pairs;
    *r_true = (double)h_cnt[kProbeT + thresh - 1] / pairs;
    *r_cand48 = (double)h_cnt[2 * kProbeT + thresh - 1] / pairs;
    *r_cand16 = (double)h_cnt[3 * kProbeT + thresh - 1] / pairs;
  } else {
    (void)hipGetLastError();
  }
  if (h_cnt) probe_slot_put(h_cnt);
  return ok;
}

int selftest_fp4_products(float* d_out, hipStream_t stream) {
  hipLaunchKernelGGL(k_selftest_fp4, dim3(1), dim3(64), 0, stream, d_out);
  CBH_HIP(hipGetLastError());
  return CBH_OK;
}

static NeedleScratch needle_scratch(size_t nq) { return {(uint32_t)((nq + kNeedlePad - 1) / kNeedlePad) * kNeedlePad}; }

int expand_needles_for_scan(const uint64_t* d_q, size_t nq, hipStream_t stream, uint4** qx_out) {
  *qx_out = nullptr;
  if (nq == 0 || nq > CBH_MAX_QUERIES_PER_CALL) return CBH_OK;
  const NeedleScratch L = needle_scratch(nq);
  uint4* qx = nullptr;
  CBH_HIP(malloc_async((void**)&qx, (size_t)L.total() * sizeof(uint4), stream));
  hipLaunchKernelGGL(k_expand_needles, dim3((L.total() + 255u) / 256u), dim3(256), 0, stream, d_q, (uint32_t)nq, L.nq_pad, qx);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    (void)free_async(qx, stream);
    CBH_HIP(e);
  }
  *qx_out = qx;
  return CBH_OK;
}

int launch_hamm64_scan_mfma(const uint64_t* d_hashes, const uint32_t* d_ids, size_t n, const uint64_t* d_q, size_t nq,
                            int thresh, cbh_record* d_rec, size_t cap, unsigned long long* d_total, hipStream_t stream,
                            ScanVariant variant, const ScanOpts& o) {
  if (variant == ScanVariant::Auto || thresh > max_thresh(variant)) return CBH_E_INVAL;  // (its fields overflow)
  const uint4* qx = o.qx;
  uint4* qx_own = nullptr;
  if (!qx) {
    int rc = expand_needles_for_scan(d_q, nq, stream, &qx_own);
    if (rc) return rc;
    qx = qx_own;
  }
  // launches that run side by side on this device (the shards of a sharded handle): the workgroups that fill the machine are
  // theirs together -- a shard of 125 000 slots alone cut its needles into chunks of 128 pairs to reach 8192 workgroups and
  // paid the shorter chunks' per-chunk costs (3 % of the sweep) for parallelism its seven siblings already supplied
  const uint32_t sib = std::max(1u, o.siblings);
  // K over `items` needle pairs or triples, cut into chunks by scan_chunk(.., start, floor, multiple)
  auto launch = [&](auto K, int tiles, uint32_t items, uint32_t start, uint32_t floor, uint32_t multiple, auto... operands) {
    const uint32_t rows_per_wg = 32u * (uint32_t)tiles * kWaves, wgs = (uint32_t)((n + rows_per_wg - 1) / rows_per_wg);
    const uint32_t per_chunk = scan_chunk((uint64_t)wgs * sib, items, start, floor, multiple);
    hipLaunchKernelGGL(K, dim3(wgs, (items + per_chunk - 1) / per_chunk), dim3(kThreads), 0, stream,
                       reinterpret_cast<const uint2*>(d_hashes), d_ids, (uint32_t)n, d_q, qx, (uint32_t)nq, items, per_chunk,
                       (uint32_t)thresh, d_rec, (unsigned long long)cap, d_total, (uint32_t)o.keep_id0,
                       reinterpret_cast<const uint2*>(o.d_qmask), operands...);
  };
  const uint32_t n_pairs = (uint32_t)((nq + 63) / 64), n_triples = (uint32_t)((nq + 95) / 96);
  const NeedleScratch L = needle_scratch(nq);
  // A prefilter: 512 pairs = 32768 needles per chunk -- a wave drains its pending candidates at the end of its chunk,
  // mostly a short list: at threshold 6 chunks of 512 / 1024 pairs run 12.63 ms against 12.98 with 256 and 13.35 with 64.
  // Whole quadruples (even: a step takes two pairs).
  auto prefilter = [&](auto K, auto V) { launch(K, V.kTiles, n_pairs, 512u, 16u, 2u, qx + V.operands(L)); };
  switch (variant) {
    case ScanVariant::Pre32: prefilter(k_hamm64_mfma<true>, Pre32{}); break;
    case ScanVariant::Pre48: prefilter(k_hamm64_mfma48, Pre48{}); break;
    case ScanVariant::Pre16: prefilter(k_hamm64_mfma16, Pre16{}); break;
    default:
      // FULL3: each wave amortises its tile expansion over >= 11 needle-tile triples (172 triples = 16512 needles per chunk:
      // 16.05 ms against 16.25-16.3 with 2-4x that, tools/ab/scan_chunk_ab.py); FULL2, threshold 65: pairs
      if (thresh <= 64) launch(k_hamm64_mfma3, kHT, n_triples, 172u, 11u, 1u);
      else launch(k_hamm64_mfma<false>, kHT, n_pairs, 256u, 16u, 2u, (const uint4*)nullptr);
  }
  hipError_t e = hipGetLastError();
  if (qx_own) (void)cbh::free_async(qx_own, stream);
  CBH_HIP(e);
  return CBH_OK;
}

}  // namespace cbh
