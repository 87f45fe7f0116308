// vsegments.hip -- where one video lies inside another: the frame-number offsets at which a source video's frames are
// found in a destination video, one segment per offset, for a batch of ordered pairs.
//
// The coverage map (vcoverage.hip) gives every source frame its nearest destination frame ANYWHERE; a black frame or a
// static scene matches wherever the destination has one.  The reference's wish list asks for the next step (doc/
// cbird-devel.md, Search: "refine video search matches using neighboring hashes").  The rules are in include/cbird_hip.h
// at cbh_video_segments; the views, span and the match predicate are coverage's (cbh_vviews.h builds both).
//
//   host            the two views of every distinct video, uploaded once; per pair the offset domain [omin, omin + n_off)
//                   from the first and last frame numbers of its two views (cbh_vviews.h: vseg_range), a difference array
//                   of n_off + 1 words; pairs in groups whose arrays fit "vseg_budget_mb" together; a tile table block ->
//                   (pair, 256 source frames).  Then per group and round: memset, k_vs_support, k_vs_pick, k_vs_members,
//                   queued without a host wait -- a pair that is finished turns its blocks into no-ops.
//   k_vs_support    a lane owns one live source frame and sees the WHOLE destination, 256 entries (hash, frame) per LDS
//                   stage, double buffered, every lane reading the same address (a broadcast).  Per comparison two xor,
//                   two v_bcnt and a share of a minimum; one branch per 8 entries, only a match goes further.  Destination frames rise, so a lane's match
//                   offsets rise: the interval [o - tol, o + tol] of a match extends the lane's running interval while
//                   they touch, in registers, and a finished interval is flushed as +1 at its start and -1 one past its
//                   end by integer atomicAdd.  A lane is the only one that sees its frame, so the frame counts once per
//                   offset; integer adds commute, so the array does not depend on any order.
//   k_vs_pick       one block per pair: a prefix sum over the array, 2048 words a step, for the maximum support; a
//                   second one for the runs of it -- a run starts where the support is the maximum and the difference
//                   word is not 0, and ends in front of the next such word -- each run's centre, and the minimum of
//                   |c| << 1 | (c >= 0).  Below min_frames the pair is finished.
//   k_vs_members    the comparisons again: a live lane keeps the minimum of |offset - c| << 32 | distance << 24 | entry
//                   over its matches within tol of c, writes its map entry and leaves the live set; a wave reduces its
//                   members to four atomics on the segment's record.
//   k_vs_finish     one wave per pair: span sums over the map, lane r completes segment r, the monotone flag from 16 x 16
//                   lane comparisons, the summary.
// Bounds: frame numbers that fall inside a used video are refused (CBH_E_INVAL) before anything is launched, so the first
// and last frame of a view are its minimum and maximum and every index a kernel forms lies inside its array; the flush
// checks the end of its interval against n_off all the same.
#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "cbh_index.h"
#include "cbh_staging.h"
#include "cbh_vviews.h"

namespace cbh {
namespace {

constexpr int kThreads = 256;
constexpr int kStage = 256;           // destination entries per LDS stage: one per thread
constexpr int kBatch = 8;            // destination entries a lane compares between two branches
constexpr int kPickPer = 8;          // words of a difference array one thread of k_vs_pick takes a step
constexpr int kPickStep = kPickPer * kThreads;

std::atomic<int> g_vseg_budget_mb{256};  // "vseg_budget_mb": what the difference arrays of one group of pairs may take

struct VsPair {
  uint32_t s_begin, s_n;  // the source view of the pair's source video
  uint32_t d_begin, d_n;  // the destination view of its destination video
  unsigned long long map_off;   // its first map entry
  unsigned long long diff_off;  // its difference array in the group's block, in words
  int32_t omin;                 // the offset of word 0
  uint32_t n_off;               // offsets in the domain; 0 = nothing to do
};
struct VsTile {
  uint32_t pair, s0;  // sources [s0, s0 + 256) of the pair
};

int vs_inval(const char* why) {
  set_last_error_text(why);
  return CBH_E_INVAL;
}

__global__ __launch_bounds__(kThreads) void k_vs_init(const int32_t* __restrict__ src_frame,
                                                     const VsPair* __restrict__ pairs, const VsTile* __restrict__ tiles,
                                                     cbh_vsegment_frame* __restrict__ map) {
  const VsTile t = tiles[blockIdx.x];
  const VsPair p = pairs[t.pair];
  const uint32_t i = t.s0 + threadIdx.x;
  if (i < p.s_n) map[p.map_off + i] = cbh_vsegment_frame{src_frame[p.s_begin + i], -1, 65, -1};
}

// What the two comparison kernels share: the destination of the pair, 256 entries a stage through LDS, `on_match(frame,
// distance, entry)` for every entry under the lane's threshold (0 for a lane without a live frame).
template <class F>
__device__ inline void for_each_match(const VsPair& p, const uint64_t* __restrict__ dst_hash,
                                      const int32_t* __restrict__ dst_frame, uint64_t h, int lane_thresh, bool wave_has,
                                      uint64_t (*stage_h)[kStage], int32_t (*stage_f)[kStage], F on_match) {
  const uint32_t tid = threadIdx.x;
  const uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
  const uint64_t* dh = dst_hash + p.d_begin;
  const int32_t* df = dst_frame + p.d_begin;
  uint32_t pos = 0;
  stage_h[0][tid] = tid < p.d_n ? dh[tid] : 0;
  stage_f[0][tid] = tid < p.d_n ? df[tid] : 0;
  __syncthreads();
  int buf = 0;
  while (pos < p.d_n) {
    const uint32_t cnt = min((uint32_t)kStage, p.d_n - pos), npos = pos + kStage;
    uint64_t nh = 0;
    int32_t nf = 0;
    if (npos + tid < p.d_n) nh = dh[npos + tid], nf = df[npos + tid];
    if (wave_has) {
      // 8 entries a step: their LDS reads are in flight together and ONE branch asks whether any of them matches -- with
      // a wave per SIMD nothing else hides a read, and a branch per entry left every read's latency in the open
      uint32_t k = 0;
      for (; k + kBatch <= cnt; k += kBatch) {
        int d[kBatch], nearest = 64;
#pragma unroll
        for (int q = 0; q < kBatch; ++q) {
          const uint64_t e = stage_h[buf][k + q];
          d[q] = __builtin_popcount(lo ^ (uint32_t)e) + __builtin_popcount(hi ^ (uint32_t)(e >> 32));
          nearest = min(nearest, d[q]);
        }
        if (nearest < lane_thresh) {
#pragma unroll
          for (int q = 0; q < kBatch; ++q)  // in entry order: the callers rely on rising frames
            if (d[q] < lane_thresh) on_match(stage_f[buf][k + q], d[q], pos + k + q);
        }
      }
      for (; k < cnt; ++k) {
        const uint64_t e = stage_h[buf][k];
        const int d = __builtin_popcount(lo ^ (uint32_t)e) + __builtin_popcount(hi ^ (uint32_t)(e >> 32));
        if (d < lane_thresh) on_match(stage_f[buf][k], d, pos + k);
      }
    }
    if (npos < p.d_n) stage_h[buf ^ 1][tid] = nh, stage_f[buf ^ 1][tid] = nf;
    __syncthreads();  // the other buffer is full, and nobody reads this one any more
    buf ^= 1;
    pos = npos;
  }
}

__global__ __launch_bounds__(kThreads) void k_vs_support(const uint64_t* __restrict__ src_hash,
                                                        const int32_t* __restrict__ src_frame,
                                                        const uint64_t* __restrict__ dst_hash,
                                                        const int32_t* __restrict__ dst_frame,
                                                        const VsPair* __restrict__ pairs, const VsTile* __restrict__ tiles,
                                                        const int32_t* __restrict__ finished,
                                                        const cbh_vsegment_frame* __restrict__ map, int thresh, int tol,
                                                        int32_t* __restrict__ diff) {
  __shared__ uint64_t stage_h[2][kStage];
  __shared__ int32_t stage_f[2][kStage];
  const VsTile t = tiles[blockIdx.x];
  if (finished[t.pair]) return;  // (the whole block)
  const VsPair p = pairs[t.pair];
  const uint32_t i = t.s0 + threadIdx.x;
  const bool live = i < p.s_n && map[p.map_off + i].segment < 0;
  const uint64_t h = live ? src_hash[p.s_begin + i] : 0;
  const uint32_t fs = live ? (uint32_t)src_frame[p.s_begin + i] : 0;
  // word of the first offset of a match's interval: (fd - fs - tol) - omin, in wrapping arithmetic -- the true value lies
  // in [0, n_off - 2 tol)
  const uint32_t base = fs + (uint32_t)p.omin + (uint32_t)tol, width = 2u * (uint32_t)tol;
  int32_t* d = diff + p.diff_off;
  const uint32_t n_off = p.n_off;
  uint32_t a = 0, b = 0;
  bool open = false;
  auto flush = [&]() {
    if (a <= b && b < n_off) atomicAdd(&d[a], 1), atomicAdd(&d[b + 1], -1);
  };
  for_each_match(p, dst_hash, dst_frame, h, live ? thresh : 0, __ballot(live) != 0, stage_h, stage_f,
                 [&](int32_t fd, int, uint32_t) {
                   const uint32_t u = (uint32_t)fd - base;
                   if (open && u <= b + 1) {  // touches the running interval: offsets rise, so it only grows upward
                     b = u + width;
                   } else {
                     if (open) flush();
                     a = u, b = u + width, open = true;
                   }
                 });
  if (open) flush();
}

__device__ inline int wave_incl_sum(int v, uint32_t lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(v, o);
    if ((int)lane >= o) v += up;
  }
  return v;
}
__device__ inline int wave_incl_max(int v, uint32_t lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(v, o);
    if ((int)lane >= o) v = max(v, up);
  }
  return v;
}
// exclusive scans over the block's 256 threads; *total = the whole block's.  Two barriers each; `part` is 4 words of LDS
__device__ inline int block_excl_sum(int v, int* part, int* total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int inc = wave_incl_sum(v, lane);
  __syncthreads();  // the last reader of part[] is done
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    const int x = part[w];
    if (w < (int)wave) before += x;
    all += x;
  }
  *total = all;
  return before + inc - v;
}
__device__ inline int block_excl_max(int v, int* part, int* total) {  // values >= -1
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int inc = wave_incl_max(v, lane);
  int excl = __shfl_up(inc, 1);
  if (lane == 0) excl = -1;
  __syncthreads();
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  int all = -1;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    const int x = part[w];
    if (w < (int)wave) excl = max(excl, x);
    all = max(all, x);
  }
  *total = all;
  return excl;
}

// Round `round` of the pairs [p0, p0 + gridDim.x): rule 2 on the difference array the support kernel left.
__global__ __launch_bounds__(kThreads) void k_vs_pick(const VsPair* __restrict__ pairs, uint32_t p0,
                                                     const int32_t* __restrict__ diff, int round, int min_frames,
                                                     int max_segments, int32_t* __restrict__ finished,
                                                     int32_t* __restrict__ n_segments, cbh_vsegment* __restrict__ segs) {
  __shared__ int part[kThreads / 64];
  __shared__ int wave_best[kThreads / 64];
  __shared__ unsigned long long wave_key[kThreads / 64];
  const uint32_t pi = p0 + blockIdx.x, tid = threadIdx.x;
  if (finished[pi]) return;  // (the whole block)
  const VsPair p = pairs[pi];
  const int32_t* d = diff + p.diff_off;
  const uint32_t n = p.n_off;

  // the maximum support
  int carry = 0, best = 0;
  for (uint32_t step = 0; step < n; step += kPickStep) {
    const uint32_t o0 = step + kPickPer * tid;
    int s[kPickPer];
#pragma unroll
    for (int q = 0; q < kPickPer; ++q) s[q] = o0 + q < n ? d[o0 + q] : 0;
#pragma unroll
    for (int q = 1; q < kPickPer; ++q) s[q] += s[q - 1];
    int total;
    const int before = carry + block_excl_sum(s[kPickPer - 1], part, &total);
#pragma unroll
    for (int q = 0; q < kPickPer; ++q) best = max(best, before + s[q]);
    carry += total;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
  if ((tid & 63) == 0) wave_best[tid >> 6] = best;
  __syncthreads();
  const int m = max(max(wave_best[0], wave_best[1]), max(wave_best[2], wave_best[3]));
  if (m < min_frames) {  // (min_frames >= 1: a pair without a match left ends here too)
    if (tid == 0) finished[pi] = 1;
    return;
  }

  // its runs: the run that ends at offset word `hi` began at the last start at or before it
  unsigned long long key = ~0ull;
  int last_start = -1;
  carry = 0;
  for (uint32_t step = 0; step < n; step += kPickStep) {
    const uint32_t o0 = step + kPickPer * tid;
    int raw[kPickPer + 1], s[kPickPer];
#pragma unroll
    for (int q = 0; q <= kPickPer; ++q) raw[q] = o0 + q < n ? d[o0 + q] : 0;
    s[0] = raw[0];
#pragma unroll
    for (int q = 1; q < kPickPer; ++q) s[q] = s[q - 1] + raw[q];
    int total, starts;
    const int before = carry + block_excl_sum(s[kPickPer - 1], part, &total);
    carry += total;
    bool at_max[kPickPer];
    int mine = -1;
#pragma unroll
    for (int q = 0; q < kPickPer; ++q) {
      at_max[q] = o0 + q < n && before + s[q] == m;
      if (at_max[q] && (o0 + q == 0 || raw[q] != 0)) mine = (int)(o0 + q);
    }
    int cur = max(last_start, block_excl_max(mine, part, &starts));
    last_start = max(last_start, starts);
#pragma unroll
    for (int q = 0; q < kPickPer; ++q) {
      if (!at_max[q]) continue;
      const uint32_t o = o0 + q;
      if (o == 0 || raw[q] != 0) cur = (int)o;
      if (o + 1 == n || raw[q + 1] != 0) {
        const long long c = (2ll * p.omin + cur + (long long)o) >> 1;  // floor toward minus infinity
        key = min(key, (unsigned long long)(c < 0 ? -c : c) << 1 | (c >= 0));
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned long long)__shfl_xor((long long)key, o));
  if ((tid & 63) == 0) wave_key[tid >> 6] = key;
  __syncthreads();
  if (tid == 0) {
    key = min(min(wave_key[0], wave_key[1]), min(wave_key[2], wave_key[3]));
    const long long mag = (long long)(key >> 1);
    segs[(size_t)pi * max_segments + round].offset = (int32_t)((key & 1) ? mag : -mag);
    n_segments[pi] = round + 1;
  }
}

__device__ inline long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(kThreads) void k_vs_members(const uint64_t* __restrict__ src_hash,
                                                        const int32_t* __restrict__ src_frame,
                                                        const int32_t* __restrict__ src_span,
                                                        const uint64_t* __restrict__ dst_hash,
                                                        const int32_t* __restrict__ dst_frame,
                                                        const VsPair* __restrict__ pairs, const VsTile* __restrict__ tiles,
                                                        const int32_t* __restrict__ finished, int thresh, int tol, int round,
                                                        int max_segments, cbh_vsegment_frame* __restrict__ map,
                                                        cbh_vsegment* __restrict__ segs, uint32_t* __restrict__ first_i,
                                                        uint32_t* __restrict__ last_i) {
  __shared__ uint64_t stage_h[2][kStage];
  __shared__ int32_t stage_f[2][kStage];
  const VsTile t = tiles[blockIdx.x];
  if (finished[t.pair]) return;  // (the whole block)
  const VsPair p = pairs[t.pair];
  const size_t seg = (size_t)t.pair * max_segments + round;
  const uint32_t i = t.s0 + threadIdx.x;
  const bool live = i < p.s_n && map[p.map_off + i].segment < 0;
  const uint64_t h = live ? src_hash[p.s_begin + i] : 0;
  const int32_t sf = live ? src_frame[p.s_begin + i] : 0;
  // (fd - fs - c) + tol in wrapping arithmetic: the true value is below 2^31 either way, and within [0, 2 tol] for a member
  const uint32_t base = (uint32_t)sf + (uint32_t)segs[seg].offset - (uint32_t)tol, width = 2u * (uint32_t)tol;
  unsigned long long best = ~0ull;
  for_each_match(p, dst_hash, dst_frame, h, live ? thresh : 0, __ballot(live) != 0, stage_h, stage_f,
                 [&](int32_t fd, int dist, uint32_t j) {
                   const uint32_t u = (uint32_t)fd - base;
                   if (u <= width) {
                     const uint32_t apart = u < (uint32_t)tol ? (uint32_t)tol - u : u - (uint32_t)tol;
                     best = min(best, (unsigned long long)apart << 32 | (uint32_t)dist << 24 | j);
                   }
                 });
  const bool member = best != ~0ull;
  if (member)
    map[p.map_off + i] = cbh_vsegment_frame{sf, dst_frame[p.d_begin + ((uint32_t)best & (kMostVideoEntries - 1))],
                                            (int32_t)((uint32_t)best >> 24), round};
  const unsigned long long who = __ballot(member);
  if (!who) return;  // (the whole wave)
  const long long spans = wave_sum_ll(member ? src_span[p.s_begin + i] : 0);
  const uint32_t lane = threadIdx.x & 63;
  if (lane == 0) {  // lanes hold rising frames: the first and the last set bit
    atomicAdd(&segs[seg].n_frames, __popcll(who));
    atomicAdd((unsigned long long*)&segs[seg].span_sum, (unsigned long long)spans);
    atomicMin(&first_i[seg], i + (uint32_t)(__ffsll(who) - 1));
    atomicMax(&last_i[seg], i + (uint32_t)(63 - __clzll(who)));
  }
}

__global__ __launch_bounds__(kThreads) void k_vs_finish(const int32_t* __restrict__ src_span,
                                                       const VsPair* __restrict__ pairs, uint32_t n_pairs,
                                                       const int32_t* __restrict__ n_segments, int max_segments,
                                                       const cbh_vsegment_frame* __restrict__ map,
                                                       const uint32_t* __restrict__ first_i,
                                                       const uint32_t* __restrict__ last_i, cbh_vsegment* __restrict__ segs,
                                                       cbh_vsegments* __restrict__ sums) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t pi = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (pi >= n_pairs) return;  // (whole waves: no barrier below)
  const VsPair p = pairs[pi];
  long long total = 0, aligned = 0;
  int n_aligned = 0;
  for (uint32_t at = 0; at < p.s_n; at += 64) {
    const uint32_t i = at + lane;
    const long long span = i < p.s_n ? src_span[p.s_begin + i] : 0;
    const bool in = i < p.s_n && map[p.map_off + i].segment >= 0;
    total += span, aligned += in ? span : 0, n_aligned += in;
  }
  total = wave_sum_ll(total), aligned = wave_sum_ll(aligned), n_aligned = (int)wave_sum_ll(n_aligned);
  const int n_seg = n_segments[pi];
  // lane r completes segment r
  int src_first = 0, dst_first = 0, dst_last = 0;
  long long placed = 0;
  if ((int)lane < n_seg) {
    const size_t seg = (size_t)pi * max_segments + lane;
    // (a segment has a member, so both are frames of the pair; min() keeps the reads inside the map come what may)
    const cbh_vsegment_frame a = map[p.map_off + min(first_i[seg], p.s_n - 1)], b = map[p.map_off + min(last_i[seg], p.s_n - 1)];
    segs[seg].src_first = a.src_frame, segs[seg].src_last = b.src_frame;
    segs[seg].dst_first = a.dst_frame, segs[seg].dst_last = b.dst_frame;
    src_first = a.src_frame, dst_first = a.dst_frame, dst_last = b.dst_frame;
    placed = (long long)a.src_frame + segs[seg].offset;
  }
  // monotone: of two segments the one that comes first in the source (the earlier found of two equals) lies no later
  bool falls = false;
  for (int r = 0; r < n_seg; ++r) {
    const int other_first = __shfl(src_first, r);
    const long long other_placed = __shfl(placed, r);
    if ((int)lane < n_seg && (src_first < other_first || (src_first == other_first && (int)lane < r)))
      falls |= placed > other_placed;
  }
  const bool monotone = __ballot(falls) == 0;
  if (lane != 0) return;
  cbh_vsegments s;
  s.src_frames_total = total, s.src_frames_aligned = aligned;
  s.n_src = (int32_t)p.s_n, s.n_dst = (int32_t)p.d_n, s.n_segments = n_seg, s.n_aligned = n_aligned;
  s.monotone = monotone;
  s.src_in = n_seg ? src_first : -1, s.dst_in = n_seg ? dst_first : -1;
  s.len = n_seg ? (int32_t)((long long)dst_last - dst_first + 1) : 0;
  sums[pi] = s;
}

size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

int video_segments(int device, const int32_t* frames, const uint64_t* hashes, const uint64_t* voff, size_t n_videos,
                   const uint32_t* pairs, size_t n_pairs, int thresh, int skip, int tol, int min_frames, int max_segments,
                   cbh_vsegments* summaries, cbh_vsegment* segments, cbh_vsegment_frame* map, size_t map_cap,
                   uint64_t* map_offsets) {
  std::vector<uint8_t> as_src(n_videos, 0), as_dst(n_videos, 0);
  for (size_t k = 0; k < n_pairs; ++k) {
    if (pairs[2 * k] >= n_videos || pairs[2 * k + 1] >= n_videos) return vs_inval("video segments: a pair names a video outside the table");
    as_src[pairs[2 * k]] = 1, as_dst[pairs[2 * k + 1]] = 1;
  }
  VideoViews vv;
  {
    std::string why;
    const int rc = build_video_views("video segments", frames, hashes, voff, n_videos, as_src, as_dst, skip, true, &vv, &why);
    if (rc != CBH_OK) {
      set_last_error_text(why.c_str());
      return rc;
    }
  }

  // the map's layout and every offset domain are known before anything runs
  const uint64_t budget = (uint64_t)g_vseg_budget_mb.load() << 20;
  std::vector<VsPair> ptab(n_pairs);
  std::vector<VsegRange> ranges(n_pairs);
  std::vector<int32_t> finished(n_pairs, 0);
  uint64_t need = 0;
  for (size_t k = 0; k < n_pairs; ++k) {
    const VideoView &a = vv.views[pairs[2 * k]], &b = vv.views[pairs[2 * k + 1]];
    if (a.s_n && b.d_n) {
      const int rc = vseg_range(vv.sf[a.s_begin], vv.sf[a.s_begin + a.s_n - 1], vv.df[b.d_begin],
                                vv.df[b.d_begin + b.d_n - 1], tol, budget, &ranges[k]);
      if (rc == CBH_E_NOMEM) set_last_error_text("video segments: the offsets of one pair alone exceed \"vseg_budget_mb\"");
      if (rc == CBH_E_UNSUPPORTED) set_last_error_text("video segments: an offset outside 32 bits");
      if (rc != CBH_OK) return rc;
    } else {
      finished[k] = 1;
    }
    ptab[k] = VsPair{a.s_begin, a.s_n, b.d_begin, b.d_n, need, 0, ranges[k].omin, ranges[k].n_off};
    if (map_offsets) map_offsets[k] = need;
    need += a.s_n;
  }
  if (map_offsets) map_offsets[n_pairs] = need;
  if (map && need > map_cap) return CBH_E_OVERFLOW;

  const std::vector<size_t> group = vseg_groups(ranges, budget);  // the first pair of every group, then n_pairs
  uint64_t most_words = 0;
  for (size_t g = 0; g + 1 < group.size(); ++g) {
    uint64_t words = 0;
    for (size_t k = group[g]; k < group[g + 1]; ++k) ptab[k].diff_off = words, words += ranges[k].words;
    most_words = std::max(most_words, words);
  }
  // tiles: 256 source frames of one pair are one block; the tiles of a pair, and so of a group, lie together
  std::vector<VsTile> ttab;
  std::vector<size_t> tile_of(n_pairs + 1, 0);  // the first tile of every pair
  {
    uint64_t n_tiles = 0;
    for (const VsPair& p : ptab) n_tiles += (p.s_n + kThreads - 1) / kThreads;
    if (n_tiles >= 0x7fffffffull) {
      set_last_error_text("video segments: more than 2^31 tiles in one call");
      return CBH_E_UNSUPPORTED;
    }
    ttab.reserve((size_t)n_tiles);
    for (size_t k = 0; k < n_pairs; ++k) {
      tile_of[k] = ttab.size();
      for (uint32_t s0 = 0; s0 < ptab[k].s_n; s0 += kThreads) ttab.push_back(VsTile{(uint32_t)k, s0});
    }
    tile_of[n_pairs] = ttab.size();
  }

  const size_t ns = vv.sh.size(), nd = vv.dh.size(), n_segs = n_pairs * (size_t)max_segments;
  const size_t src_bytes = round16(ns * 8) + round16(ns * 4) + round16(ns * 4);
  const size_t dst_bytes = round16(nd * 8) + round16(nd * 4);
  const size_t tab_bytes = round16(n_pairs * sizeof(VsPair)) + round16(ttab.size() * sizeof(VsTile));
  // the state of the rounds: finished and n_segments per pair, first and last member per segment
  const size_t state_bytes = 2 * round16(n_pairs * 4) + 2 * round16(n_segs * 4);

  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  Staging st("video segments");
  uint8_t *d_src, *d_dst, *d_tab, *d_state;
  int32_t* d_diff;
  cbh_vsegments* d_sums;
  cbh_vsegment* d_segs;
  cbh_vsegment_frame* d_map;
  st.alloc(&d_src, std::max<size_t>(src_bytes, 16));
  st.alloc(&d_dst, std::max<size_t>(dst_bytes, 16));
  st.alloc(&d_tab, tab_bytes);
  st.alloc(&d_state, state_bytes);
  st.alloc(&d_diff, std::max<uint64_t>(most_words, 4) * 4);
  st.alloc(&d_sums, n_pairs * sizeof(cbh_vsegments));
  st.alloc(&d_segs, n_segs * sizeof(cbh_vsegment));
  st.alloc(&d_map, std::max<uint64_t>(need, 1) * sizeof(cbh_vsegment_frame));
  int rc = st.status();
  if (rc != CBH_OK) return rc;
  if (ns) {
    st.up(d_src, vv.sh.data(), ns * 8);
    st.up(d_src + round16(ns * 8), vv.sf.data(), ns * 4);
    st.up(d_src + round16(ns * 8) + round16(ns * 4), vv.ss.data(), ns * 4);
  }
  if (nd) {
    st.up(d_dst, vv.dh.data(), nd * 8);
    st.up(d_dst + round16(nd * 8), vv.df.data(), nd * 4);
  }
  st.up(d_tab, ptab.data(), n_pairs * sizeof(VsPair));
  if (!ttab.empty()) st.up(d_tab + round16(n_pairs * sizeof(VsPair)), ttab.data(), ttab.size() * sizeof(VsTile));
  int32_t* d_finished = (int32_t*)d_state;
  int32_t* d_nseg = (int32_t*)(d_state + round16(n_pairs * 4));
  uint32_t* d_first = (uint32_t*)(d_state + 2 * round16(n_pairs * 4));
  uint32_t* d_last = (uint32_t*)(d_state + 2 * round16(n_pairs * 4) + round16(n_segs * 4));
  st.up(d_finished, finished.data(), n_pairs * 4);
  if ((rc = st.status()) != CBH_OK) return rc;
  CBH_HIP(hipMemsetAsync(d_nseg, 0, round16(n_pairs * 4), st.s));
  CBH_HIP(hipMemsetAsync(d_first, 0xff, round16(n_segs * 4), st.s));
  CBH_HIP(hipMemsetAsync(d_last, 0, round16(n_segs * 4), st.s));
  CBH_HIP(hipMemsetAsync(d_segs, 0, n_segs * sizeof(cbh_vsegment), st.s));
  const uint64_t* d_sh = (const uint64_t*)d_src;
  const int32_t* d_sf = (const int32_t*)(d_src + round16(ns * 8));
  const int32_t* d_ss = (const int32_t*)(d_src + round16(ns * 8) + round16(ns * 4));
  const uint64_t* d_dh = (const uint64_t*)d_dst;
  const int32_t* d_df = (const int32_t*)(d_dst + round16(nd * 8));
  const VsPair* d_pairs = (const VsPair*)d_tab;
  const VsTile* d_tiles = (const VsTile*)(d_tab + round16(n_pairs * sizeof(VsPair)));
  if (!ttab.empty()) {
    hipLaunchKernelGGL(k_vs_init, dim3((unsigned)ttab.size()), dim3(kThreads), 0, st.s, d_sf, d_pairs, d_tiles, d_map);
    CBH_HIP(hipGetLastError());
  }
  for (size_t gi = 0; gi + 1 < group.size(); ++gi) {
    const size_t p0 = group[gi], p1 = group[gi + 1];
    const unsigned blocks = (unsigned)(tile_of[p1] - tile_of[p0]);
    uint64_t words = 0;
    for (size_t k = p0; k < p1; ++k) words += ranges[k].words;
    if (!blocks || !words) continue;  // no pair of the group has both frames and entries
    const VsTile* tiles = d_tiles + tile_of[p0];
    for (int round = 0; round < max_segments; ++round) {  // no host wait: a finished pair's blocks return at once
      CBH_HIP(hipMemsetAsync(d_diff, 0, words * 4, st.s));
      hipLaunchKernelGGL(k_vs_support, dim3(blocks), dim3(kThreads), 0, st.s, d_sh, d_sf, d_dh, d_df, d_pairs, tiles,
                         d_finished, d_map, thresh, tol, d_diff);
      hipLaunchKernelGGL(k_vs_pick, dim3((unsigned)(p1 - p0)), dim3(kThreads), 0, st.s, d_pairs, (uint32_t)p0, d_diff, round,
                         min_frames, max_segments, d_finished, d_nseg, d_segs);
      hipLaunchKernelGGL(k_vs_members, dim3(blocks), dim3(kThreads), 0, st.s, d_sh, d_sf, d_ss, d_dh, d_df, d_pairs, tiles,
                         d_finished, thresh, tol, round, max_segments, d_map, d_segs, d_first, d_last);
      CBH_HIP(hipGetLastError());
    }
  }
  const unsigned per_block = kThreads / 64;
  hipLaunchKernelGGL(k_vs_finish, dim3((unsigned)((n_pairs + per_block - 1) / per_block)), dim3(kThreads), 0, st.s, d_ss,
                     d_pairs, (uint32_t)n_pairs, d_nseg, max_segments, d_map, d_first, d_last, d_segs, d_sums);
  CBH_HIP(hipGetLastError());
  st.down(summaries, d_sums, n_pairs * sizeof(cbh_vsegments));
  st.down(segments, d_segs, n_segs * sizeof(cbh_vsegment));
  if (map && need) st.down(map, d_map, need * sizeof(cbh_vsegment_frame));
  st.sync();
  return st.status();
}

}  // namespace

int set_vseg_budget_mb(int v) {
  if (v < 1 || v > 4096) return CBH_E_INVAL;
  g_vseg_budget_mb.store(v);
  return CBH_OK;
}
int get_vseg_budget_mb() { return g_vseg_budget_mb.load(); }

}  // namespace cbh

extern "C" {

int cbh_video_segments(int device, const int32_t* frames, const uint64_t* hashes, const uint64_t* video_offsets,
                       size_t n_videos, const uint32_t* pairs, size_t n_pairs, int thresh, int skip_frames, int tol,
                       int min_frames, int max_segments, cbh_vsegments* summaries, cbh_vsegment* segments,
                       cbh_vsegment_frame* map, size_t map_cap, uint64_t* map_offsets) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  if (skip_frames < 0) return vs_inval("video segments: skip_frames below 0");
  if (tol < 0) return vs_inval("video segments: tol below 0");
  if (min_frames < 1) return vs_inval("video segments: min_frames below 1");
  if (max_segments < 1 || max_segments > CBH_VSEGMENTS_MAX) return vs_inval("video segments: max_segments outside 1..16");
  if (map && !map_offsets) return vs_inval("video segments: a map without map_offsets");
  if (n_pairs == 0) {
    if (map_offsets) map_offsets[0] = 0;
    return CBH_OK;
  }
  if (n_pairs >= 0x7fffffffull / CBH_VSEGMENTS_MAX) return vs_inval("video segments: 2^27 pairs or more");
  if (!pairs || !summaries || !segments || !video_offsets) return vs_inval("video segments: a required pointer is NULL");
  if (n_videos && video_offsets[n_videos] > video_offsets[0] && (!frames || !hashes))
    return vs_inval("video segments: frames or hashes is NULL");
  try {
    return video_segments(device, frames, hashes, video_offsets, n_videos, pairs, n_pairs, thresh, skip_frames, tol,
                          min_frames, max_segments, summaries, segments, map, map_cap, map_offsets);
  } catch (const std::bad_alloc&) {
    set_last_error_text("video segments: host allocation failed");
    return CBH_E_NOMEM;
  }
}

}  // extern "C"
