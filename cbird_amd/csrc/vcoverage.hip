// vcoverage.hip -- the coverage map of video pairs: for every stored frame of a source video the nearest frame of a
// destination video, and per pair a summary that says whether the destination contains the source and where not.
//
// findVideo (src/dctvideoindex.cpp:399-657) builds "needle frame -> closest frame" for every matched video, collapses
// it into one MatchRange and percentNear, and drops it; the reference's wish list asks for the map itself
// (doc/cbird-devel.md, Search: "video coverage map to tell if one clip includes all frames of another clip").  The rules
// (include/cbird_hip.h has them in full): source frames as findVideo searches them (the unconditional trim, :431),
// destination entries as insertHashes stores them (5-bit detail rule, conditional trim, :89-95), nearest = the minimum
// of distance << 24 | entry, covered = distance < thresh.
//
//   host          one source view (hash, frame, span) and one destination view (hash, frame) per distinct video, each
//                 uploaded once however many pairs name it; a pair table; a tile table block -> (pair, source tile,
//                 destination chunk), so that a ragged batch and one huge pair both fill the device
//   k_vc_map<R>   256 threads; every lane keeps R source hashes and R running minima in registers, wave w owning the
//                 sources [64 R w, 64 R (w + 1)) of the tile (a short video leaves whole waves idle, not lanes of every
//                 wave).  The chunk's destination hashes pass through LDS 256 at a time, double buffered: one barrier
//                 per stage, the next stage's global load in flight behind the compares.  Every lane reads the SAME LDS
//                 address (a broadcast, no bank conflict).  Per comparison two xor, two v_bcnt (the second accumulating),
//                 one v_lshl_or for the key, one v_min_u32.  No cross-lane step: partial minima of the chunks of one
//                 pair meet by atomicMin on the pair's key words, one word per source frame.
//   k_vc_finish   one wave per pair walks the finished keys 64 frames at a time in frame order: key -> (frame,
//                 distance) into the map when the caller wants it, and the summary from ballots, two wave scans and a
//                 wave-uniform walk over the runs of uncovered frames; what crosses a step is carried in scalars.
// What bounds k_vc_map: 6 VALU operations per comparison at 4 cycles per wave instruction (tools/ubench/valu_rate.hip:
// v_bcnt and anything with an SGPR source), 64 comparisons per instruction: 1024 SIMDs x 2.4 GHz x 64 / 24 = 6.5e12
// comparisons per second.  DESIGN.md has the measured fraction.
#include <algorithm>
#include <new>
#include <vector>

#include "cbh_index.h"
#include "cbh_staging.h"
#include "cbh_vviews.h"

namespace cbh {
namespace {

constexpr int kThreads = 256;
constexpr int kStage = 256;                // destination hashes per LDS stage: one per thread
constexpr uint32_t kNoKey = 0xffffffffu;   // no destination entry seen (a real key is at most 64 << 24 | 2^24 - 1)
constexpr uint32_t kMostEntries = kMostVideoEntries;  // the entry field of a key (cbh_vviews.h)
constexpr int kFrameMargin = 15;           // findVideo's frameMargin (:593)

std::atomic<int> g_vcover_chunk{0};     // "vcover_chunk": destination entries per block, 0 = by the size of the batch
std::atomic<int> g_vcover_tile{1024};   // "vcover_tile": source frames per block, 256 x {1, 2, 4, 8}

struct VcPair {
  uint32_t s_begin, s_n;  // the source view of the pair's source video
  uint32_t d_begin, d_n;  // the destination view of its destination video
  unsigned long long key_off;  // its first key word = its first map entry
};
struct VcTile {
  uint32_t pair, s0, d0, d1;  // sources [s0, s0 + 256 R) against entries [d0, d1) of the pair
};

int vc_inval(const char* why) {
  set_last_error_text(why);
  return CBH_E_INVAL;
}

template <int R>
__global__ __launch_bounds__(kThreads) void k_vc_map(const uint64_t* __restrict__ src_hash,
                                                    const uint64_t* __restrict__ dst_hash,
                                                    const VcPair* __restrict__ pairs, const VcTile* __restrict__ tiles,
                                                    uint32_t* __restrict__ keys) {
  __shared__ uint64_t stage[2][kStage];
  const VcTile t = tiles[blockIdx.x];
  const VcPair p = pairs[t.pair];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t w0 = t.s0 + wave * (64 * R);  // this wave's first source
  const bool wave_has = w0 < p.s_n;
  uint32_t lo[R], hi[R], best[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t i = w0 + r * 64 + lane;
    const uint64_t h = i < p.s_n ? src_hash[p.s_begin + i] : 0;
    lo[r] = (uint32_t)h, hi[r] = (uint32_t)(h >> 32), best[r] = kNoKey;
  }
  const uint64_t* dh = dst_hash + p.d_begin;
  uint32_t pos = t.d0;
  stage[0][tid] = pos + tid < t.d1 ? dh[pos + tid] : 0;
  __syncthreads();
  int buf = 0;
  while (pos < t.d1) {
    const uint32_t cnt = min((uint32_t)kStage, t.d1 - pos), npos = pos + kStage;
    uint64_t nxt = 0;
    if (npos + tid < t.d1) nxt = dh[npos + tid];
    if (wave_has) {
#pragma unroll 4
      for (uint32_t k = 0; k < cnt; ++k) {
        const uint64_t e = stage[buf][k];
        const uint32_t elo = (uint32_t)e, ehi = (uint32_t)(e >> 32), j = pos + k;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const uint32_t d = __builtin_popcount(lo[r] ^ elo) + __builtin_popcount(hi[r] ^ ehi);
          best[r] = min(best[r], d << 24 | j);
        }
      }
    }
    if (npos < t.d1) stage[buf ^ 1][tid] = nxt;
    __syncthreads();  // the other buffer is full, and nobody reads this one any more
    buf ^= 1;
    pos = npos;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t i = w0 + r * 64 + lane;
    if (i < p.s_n && best[r] != kNoKey) atomicMin(&keys[p.key_off + i], best[r]);
  }
}

__device__ inline long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ inline int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ inline int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

__global__ __launch_bounds__(kThreads) void k_vc_finish(const uint64_t* __restrict__ src_hash,
                                                       const int32_t* __restrict__ src_frame,
                                                       const int32_t* __restrict__ src_span,
                                                       const int32_t* __restrict__ dst_frame,
                                                       const VcPair* __restrict__ pairs, uint32_t n_pairs,
                                                       const uint32_t* __restrict__ keys, int thresh,
                                                       cbh_vcover* __restrict__ sums, cbh_vcover_frame* __restrict__ map) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t pi = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (pi >= n_pairs) return;  // (whole waves: no barrier below)
  const VcPair p = pairs[pi];
  // what crosses a step of 64 frames; all of it is equal in every lane
  int n_cov = 0, n_low = 0, adj = 0, last_dst = 0;  // `int lastFrame = 0` (:608)
  int first_src = -1, first_dst = -1, last_src = -1, dmin = INT32_MAX, dmax = INT32_MIN;
  long long total = 0, cov_total = 0, run_len = 0, best_len = 0;
  int run_begin = 0, best_begin = 0;
  bool run_open = false;
  for (uint32_t base = 0; base < p.s_n; base += 64) {
    const uint32_t i = base + lane;
    const bool valid = i < p.s_n;
    const uint32_t key = valid ? keys[p.key_off + i] : kNoKey;
    const uint64_t h = valid ? src_hash[p.s_begin + i] : 0;
    const int sf = valid ? src_frame[p.s_begin + i] : 0;
    const long long span = valid ? src_span[p.s_begin + i] : 0;
    const bool none = key == kNoKey;
    const int d = none ? 65 : (int)(key >> 24);
    const int df = none ? -1 : dst_frame[p.d_begin + (key & (kMostEntries - 1))];
    if (map && valid) map[p.key_off + i] = cbh_vcover_frame{sf, df, d};
    const bool cov = valid && d < thresh;
    const unsigned long long vmask = __ballot(valid), cmask = __ballot(cov);
    const int pc = __popcll(h);
    n_low += __popcll(__ballot(valid && (pc < 5 || 64 - pc < 5)));

    // percentNear: a covered frame is adjacent when its match lies within frameMargin of the previous covered one's
    const unsigned long long below = cmask & ((1ull << lane) - 1);
    const int prev_lane = below ? 63 - __clzll(below) : 0;
    const int got = __shfl(df, prev_lane);
    const int prev_dst = below ? got : last_dst;
    const long long apart = (long long)df - prev_dst;
    adj += __popcll(__ballot(cov && (apart < 0 ? -apart : apart) < kFrameMargin));
    if (cmask) {
      const int fl = __ffsll(cmask) - 1, ll = 63 - __clzll(cmask);
      if (n_cov == 0) first_src = __shfl(sf, fl), first_dst = __shfl(df, fl);
      last_src = __shfl(sf, ll), last_dst = __shfl(df, ll);
      dmin = min(dmin, wave_min_i(cov ? df : INT32_MAX));
      dmax = max(dmax, wave_max_i(cov ? df : INT32_MIN));
    }
    n_cov += __popcll(cmask);
    cov_total += wave_sum(cov ? span : 0);

    // spans: an inclusive scan, so that a run of frames is a difference of two of its values
    long long scan = span;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long up = __shfl_up(scan, o);
      if ((int)lane >= o) scan += up;
    }
    total += __shfl(scan, 63);

    // the runs of uncovered frames of this step, in order; one may come in from the step before and one may go out
    const unsigned long long umask = vmask & ~cmask;
    if (run_open && !(umask & 1)) {
      if (run_len > best_len) best_len = run_len, best_begin = run_begin;
      run_open = false;
    }
    unsigned long long rem = umask;
    while (rem) {
      const int a = __ffsll(rem) - 1;                            // first frame of the run
      const unsigned long long stop = ~(umask | ((1ull << a) - 1));  // bits at or above a that are not uncovered
      const int e = stop ? __ffsll(stop) - 1 : 64;               // one past its last frame
      const long long upto = __shfl(scan, e - 1), before = __shfl(scan, a ? a - 1 : 0);
      const long long sum = upto - (a ? before : 0);
      const int begin = __shfl(sf, a);
      if (a == 0 && run_open) {
        run_len += sum;
      } else {
        run_open = true, run_begin = begin, run_len = sum;
      }
      if (e < 64 && ((vmask >> e) & 1)) {  // a covered frame ends it here
        if (run_len > best_len) best_len = run_len, best_begin = run_begin;
        run_open = false;
      }
      rem = e < 64 ? rem & ~((1ull << e) - 1) : 0;
    }
  }
  if (run_open && run_len > best_len) best_len = run_len, best_begin = run_begin;
  if (lane != 0) return;
  cbh_vcover s;
  s.src_frames_total = total, s.src_frames_covered = cov_total, s.gap_len = best_len;
  s.n_src = (int32_t)p.s_n, s.n_dst = (int32_t)p.d_n, s.n_covered = n_cov, s.n_low_detail = n_low;
  s.near_percent = n_cov ? adj * 100 / n_cov : 0;
  s.src_in = first_src, s.dst_in = first_dst;
  s.len = n_cov ? max(last_src - first_src, last_dst - first_dst) : 0;
  s.dst_min = n_cov ? dmin : -1, s.dst_max = n_cov ? dmax : -1;
  s.gap_begin = best_len ? best_begin : 0;
  s.reserved = 0;
  sums[pi] = s;
}

template <int R>
void launch_map(unsigned blocks, hipStream_t s, const uint64_t* sh, const uint64_t* dh, const VcPair* pairs,
                const VcTile* tiles, uint32_t* keys) {
  hipLaunchKernelGGL(k_vc_map<R>, dim3(blocks), dim3(kThreads), 0, s, sh, dh, pairs, tiles, keys);
}

size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

int video_coverage(int device, const int32_t* frames, const uint64_t* hashes, const uint64_t* voff, size_t n_videos,
                   const uint32_t* pairs, size_t n_pairs, int thresh, int skip, cbh_vcover* summaries,
                   cbh_vcover_frame* map, size_t map_cap, uint64_t* map_offsets) {
  std::vector<uint8_t> as_src(n_videos, 0), as_dst(n_videos, 0);
  for (size_t k = 0; k < n_pairs; ++k) {
    if (pairs[2 * k] >= n_videos || pairs[2 * k + 1] >= n_videos) return vc_inval("video coverage: a pair names a video outside the table");
    as_src[pairs[2 * k]] = 1, as_dst[pairs[2 * k + 1]] = 1;
  }
  VideoViews vv;
  {
    std::string why;
    const int rc = build_video_views("video coverage", frames, hashes, voff, n_videos, as_src, as_dst, skip, false, &vv, &why);
    if (rc != CBH_OK) {
      set_last_error_text(why.c_str());
      return rc;
    }
  }
  const std::vector<VideoView>& views = vv.views;
  const std::vector<uint64_t>&sh = vv.sh, &dh = vv.dh;
  const std::vector<int32_t>&sf = vv.sf, &ss = vv.ss, &df = vv.df;

  // the map's layout is known before anything runs: one entry per considered source frame
  std::vector<VcPair> ptab(n_pairs);
  uint64_t need = 0;
  for (size_t k = 0; k < n_pairs; ++k) {
    const VideoView &a = views[pairs[2 * k]], &b = views[pairs[2 * k + 1]];
    ptab[k] = VcPair{a.s_begin, a.s_n, b.d_begin, b.d_n, need};
    if (map_offsets) map_offsets[k] = need;
    need += a.s_n;
  }
  if (map_offsets) map_offsets[n_pairs] = need;
  if (map && need > map_cap) return CBH_E_OVERFLOW;

  // tiles: every (source tile, destination chunk) of every pair is one block
  const uint32_t tile = (uint32_t)g_vcover_tile.load();
  uint32_t chunk = (uint32_t)g_vcover_chunk.load();
  auto count_tiles = [&](uint32_t c) {
    uint64_t t = 0;
    for (const VcPair& p : ptab) t += (uint64_t)((p.s_n + tile - 1) / tile) * ((p.d_n + c - 1) / c);
    return t;
  };
  if (chunk == 0)  // shorter chunks while the batch leaves compute units without a block
    for (chunk = 4096; chunk > 256 && count_tiles(chunk) < 2048; chunk /= 2) {
    }
  const uint64_t n_tiles = count_tiles(chunk);
  if (n_tiles >= 0x7fffffffull) {
    set_last_error_text("video coverage: more than 2^31 tiles in one call");
    return CBH_E_UNSUPPORTED;
  }
  std::vector<VcTile> ttab;
  ttab.reserve((size_t)n_tiles);
  for (size_t k = 0; k < n_pairs; ++k)
    for (uint32_t s0 = 0; s0 < ptab[k].s_n; s0 += tile)
      for (uint32_t d0 = 0; d0 < ptab[k].d_n; d0 += chunk)
        ttab.push_back(VcTile{(uint32_t)k, s0, d0, (uint32_t)std::min<uint64_t>(ptab[k].d_n, (uint64_t)d0 + chunk)});

  // three device blocks: the source views, the destination views, the tables; the arrays go up from where they are
  const size_t ns = sh.size(), nd = dh.size();
  const size_t src_bytes = round16(ns * 8) + round16(ns * 4) + round16(ns * 4);
  const size_t dst_bytes = round16(nd * 8) + round16(nd * 4);
  const size_t tab_bytes = round16(n_pairs * sizeof(VcPair)) + round16(ttab.size() * sizeof(VcTile));

  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  Staging st("video coverage");
  uint8_t *d_src, *d_dst, *d_tab;
  uint32_t* d_keys;
  cbh_vcover* d_sums;
  cbh_vcover_frame* d_map = nullptr;
  st.alloc(&d_src, std::max<size_t>(src_bytes, 16));
  st.alloc(&d_dst, std::max<size_t>(dst_bytes, 16));
  st.alloc(&d_tab, tab_bytes);
  st.alloc(&d_keys, std::max<uint64_t>(need, 1) * 4);
  st.alloc(&d_sums, n_pairs * sizeof(cbh_vcover));
  if (map) st.alloc(&d_map, std::max<uint64_t>(need, 1) * sizeof(cbh_vcover_frame));
  int rc = st.status();
  if (rc != CBH_OK) return rc;
  if (ns) {
    st.up(d_src, sh.data(), ns * 8);
    st.up(d_src + round16(ns * 8), sf.data(), ns * 4);
    st.up(d_src + round16(ns * 8) + round16(ns * 4), ss.data(), ns * 4);
  }
  if (nd) {
    st.up(d_dst, dh.data(), nd * 8);
    st.up(d_dst + round16(nd * 8), df.data(), nd * 4);
  }
  st.up(d_tab, ptab.data(), n_pairs * sizeof(VcPair));
  if (!ttab.empty()) st.up(d_tab + round16(n_pairs * sizeof(VcPair)), ttab.data(), ttab.size() * sizeof(VcTile));
  if ((rc = st.status()) != CBH_OK) return rc;
  const uint64_t* d_sh = (const uint64_t*)d_src;
  const int32_t* d_sf = (const int32_t*)(d_src + round16(ns * 8));
  const int32_t* d_ss = (const int32_t*)(d_src + round16(ns * 8) + round16(ns * 4));
  const uint64_t* d_dh = (const uint64_t*)d_dst;
  const int32_t* d_df = (const int32_t*)(d_dst + round16(nd * 8));
  const VcPair* d_pairs = (const VcPair*)d_tab;
  const VcTile* d_tiles = (const VcTile*)(d_tab + round16(n_pairs * sizeof(VcPair)));
  if (need) CBH_HIP(hipMemsetAsync(d_keys, 0xff, need * 4, st.s));
  if (!ttab.empty()) {
    const unsigned blocks = (unsigned)ttab.size();
    switch (tile / kThreads) {
      case 1: launch_map<1>(blocks, st.s, d_sh, d_dh, d_pairs, d_tiles, d_keys); break;
      case 2: launch_map<2>(blocks, st.s, d_sh, d_dh, d_pairs, d_tiles, d_keys); break;
      case 4: launch_map<4>(blocks, st.s, d_sh, d_dh, d_pairs, d_tiles, d_keys); break;
      default: launch_map<8>(blocks, st.s, d_sh, d_dh, d_pairs, d_tiles, d_keys); break;
    }
    CBH_HIP(hipGetLastError());
  }
  const unsigned per_block = kThreads / 64;
  hipLaunchKernelGGL(k_vc_finish, dim3((unsigned)((n_pairs + per_block - 1) / per_block)), dim3(kThreads), 0, st.s, d_sh, d_sf,
                     d_ss, d_df, d_pairs, (uint32_t)n_pairs, d_keys, thresh, d_sums, d_map);
  CBH_HIP(hipGetLastError());
  st.down(summaries, d_sums, n_pairs * sizeof(cbh_vcover));
  if (map && need) st.down(map, d_map, need * sizeof(cbh_vcover_frame));
  st.sync();
  return st.status();
}

}  // namespace

int set_vcover_chunk(int v) {
  if (v < 0 || v > (int)kMostEntries) return CBH_E_INVAL;
  g_vcover_chunk.store(v);
  return CBH_OK;
}
int get_vcover_chunk() { return g_vcover_chunk.load(); }
int set_vcover_tile(int v) {
  if (v != 256 && v != 512 && v != 1024 && v != 2048) return CBH_E_INVAL;
  g_vcover_tile.store(v);
  return CBH_OK;
}
int get_vcover_tile() { return g_vcover_tile.load(); }

}  // namespace cbh

extern "C" {

int cbh_video_coverage(int device, const int32_t* frames, const uint64_t* hashes, const uint64_t* video_offsets,
                       size_t n_videos, const uint32_t* pairs, size_t n_pairs, int thresh, int skip_frames,
                       cbh_vcover* summaries, cbh_vcover_frame* map, size_t map_cap, uint64_t* map_offsets) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  if (skip_frames < 0) return vc_inval("video coverage: skip_frames below 0");
  if (map && !map_offsets) return vc_inval("video coverage: a map without map_offsets");
  if (n_pairs == 0) {
    if (map_offsets) map_offsets[0] = 0;
    return CBH_OK;
  }
  if (n_pairs >= 0x7fffffffull) return vc_inval("video coverage: 2^31 pairs or more");
  if (!pairs || !summaries || !video_offsets) return vc_inval("video coverage: a required pointer is NULL");
  if (n_videos && video_offsets[n_videos] > video_offsets[0] && (!frames || !hashes))
    return vc_inval("video coverage: frames or hashes is NULL");
  try {
    return video_coverage(device, frames, hashes, video_offsets, n_videos, pairs, n_pairs, thresh, skip_frames, summaries,
                          map, map_cap, map_offsets);
  } catch (const std::bad_alloc&) {
    set_last_error_text("video coverage: host allocation failed");
    return CBH_E_NOMEM;
  }
}

}  // extern "C"
