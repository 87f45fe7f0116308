// merge.hip -- cbird's -merge A B (src/main.cpp:1582-1652): every item of selection B put into selection A next to its
// closest match.  The DCT stage of the reference's cascade for ALL needles in one launch, and the placement on the host.
//
// The reference runs, per needle b_k in B's order, the lambda multiSearch (:1587-1615: maxMatches = 2, Engine::query,
// "if match.score is >= threshold, use the next algorithm" with thresholds {12, 1000, 1000, INT_MAX}) inside
// params.set = A followed by b_0 .. b_k with inSet (:1619-1625), and then inserts the needle next to matches[0]
// (:1628-1650).  The set of needle k is fixed by the order of B, never by an earlier answer -- the set grows by appended
// needles, it never holds the mutated A -- so the queries are independent and only the placement is sequential.
//
//   k_ss_keys     sortsimilar_common.h, one set: key = id, value = the item's place in the caller's arrays (A then B)
//   (radix sort)  records.hip: the union in ascending id order, so that a POSITION orders like the id
//   k_mg_gather   hashes / attributes / dir_id into that order; seen[pos] = the item's sequence number -- 0 for an item
//                 of A, j + 1 for b_j -- or kNone for an item the index does not hold; where each needle went
//   k_merge_find  one wave per needle, kWaves waves per workgroup, no __syncthreads() and no communication between
//                 waves.  Needle b_k sees item i iff seen[i] <= k and i is not the needle.  A query is a minimum of
//                 distance << 24 | position over what the needle sees (ties by position = by id, the project's rule):
//                 the lanes stride over the union's hashes in global memory, the wave takes the minimum by DPP, and
//                 successive minima ("smallest key above the last") as many as k_sort_similar's `want`.  Lane 0 then
//                 applies searchIndex + filterMatch (src/database.cpp:1691-1757, 1209-1247) as thread 0 of
//                 k_sort_similar does and writes match[k] (the match's place in the caller's arrays, kNone without
//                 one) and score[k].
// What bounds it: n_b * (n_a + n_b) popcounts per minimum, 12 bytes per item read from L2 (8 of hash, 4 of seen); at
// a few needles the launch and the sort in front of it.
#include <algorithm>
#include <vector>

#include "cbh_index.h"
#include "cbh_staging.h"

namespace cbh {
namespace {

#include "sortsimilar_common.h"  // kNone, kMostKeys, k_ss_keys, wave_min

constexpr int kWaves = 4;                      // needles (waves) per workgroup
constexpr uint32_t kMostItems = 1u << 24;      // the position field of a key

struct MgParams {
  int thresh, max_thresh, min_matches, max_matches, filter_parent, path_mode;
  int never;  // min_matches > max_matches: 1 + kept > min_matches cannot hold, every query fails
};

int mg_inval(const char* why) {
  set_last_error_text(why);
  return CBH_E_INVAL;
}

// attr: bit 0 = in the index, bit 1 = under the path prefix
__global__ __launch_bounds__(256) void k_mg_gather(const unsigned long long* __restrict__ keys,
                                                   const uint32_t* __restrict__ vals, const uint64_t* __restrict__ hashes,
                                                   const uint8_t* __restrict__ in_index, const uint32_t* __restrict__ dir_id,
                                                   const uint8_t* __restrict__ under, uint32_t n_a, uint32_t total,
                                                   uint64_t* __restrict__ s_hash, uint32_t* __restrict__ s_seen,
                                                   uint8_t* __restrict__ s_attr, uint32_t* __restrict__ s_dir,
                                                   uint32_t* __restrict__ needle_pos, uint32_t* __restrict__ status) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const uint32_t src = vals[g];
  if (g > 0 && keys[g - 1] == keys[g]) atomicOr(status, 2u);  // the same id twice in A + B
  const bool held = in_index ? in_index[src] != 0 : true;
  s_hash[g] = hashes[src];
  s_seen[g] = held ? (src < n_a ? 0u : src - n_a + 1) : kNone;
  s_attr[g] = (uint8_t)((held ? 1 : 0) | (under ? (under[src] != 0) << 1 : 0));
  if (s_dir) s_dir[g] = dir_id[src];
  if (src >= n_a) needle_pos[src - n_a] = g;
}

__global__ __launch_bounds__(64 * kWaves) void k_merge_find(const uint64_t* __restrict__ hash,
                                                            const uint32_t* __restrict__ seen,
                                                            const uint8_t* __restrict__ attr, const uint32_t* __restrict__ dir,
                                                            const uint32_t* __restrict__ place,
                                                            const uint32_t* __restrict__ needle_pos, uint32_t total,
                                                            uint32_t n_b, MgParams p, uint32_t* __restrict__ out_match,
                                                            int32_t* __restrict__ out_score) {
  __shared__ uint32_t wave_keys[kWaves][kMostKeys];  // lane 0 of each wave: the minima of its query
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t k = blockIdx.x * kWaves + wave;
  if (k >= n_b) return;
  uint32_t* keys = wave_keys[wave];
  const uint32_t np = needle_pos[k];
  const uint64_t hq = hash[np];
  const bool self = attr[np] & 1;

  const bool filters = p.filter_parent != 0 || p.path_mode != 0;
  // no candidate at or beyond this distance can ever count
  const uint32_t reach = (uint32_t)((p.max_thresh > 0 && p.thresh < p.max_thresh) ? p.max_thresh : p.thresh);
  // how many minima decide this query: k_sort_similar's `want`
  int want = max(1, p.min_matches + (self ? 0 : 1));
  if (filters) want = max(want, p.max_matches);
  if (hq == 0 || p.never) want = 0;  // a needle without a hash finds nothing (src/dcthashindex.cpp:196-200)
  int got = 0;
  uint32_t above = 0;  // only keys >= above
  while (got < want) {
    uint32_t best = kNone;
    for (uint32_t i = lane; i < total; i += 64) {
      if (seen[i] > k || i == np) continue;  // not in this needle's set (:1619-1625), outside the index, or itself
      const uint32_t d = (uint32_t)__popcll(hq ^ hash[i]);
      const uint32_t key = d << 24 | i;
      if (d < reach && key >= above) best = min(best, key);
    }
    best = wave_min(best);
    if (best == kNone) break;
    if (lane == 0) keys[got] = best;
    ++got;
    above = best + 1;
  }
  if (lane != 0) return;

  // searchIndex: raise the threshold while too few match, never past max_thresh (:1703-1725)
  int t = p.thresh, cnt = 0;
  while (cnt < got && (int)(keys[cnt] >> 24) < t) ++cnt;
  if (p.max_thresh > 0)
    while (cnt + ((self && t > 0) ? 1 : 0) <= p.min_matches && t + 1 <= p.max_thresh) {
      ++t;
      while (cnt < got && (int)(keys[cnt] >> 24) < t) ++cnt;
    }
  // the first max_matches in (distance, id) order, then filterMatch on them (:1217-1245)
  uint32_t kept = 0, answer = kNone;
  int32_t score = -1;
  const uint32_t cut = (uint32_t)min(cnt, p.max_matches);
  for (uint32_t c = 0; c < cut; ++c) {
    const uint32_t pos = keys[c] & 0xffffffu;
    if (p.path_mode && (((p.path_mode == 2) ? 1u : 0u) ^ ((attr[pos] >> 1) & 1u)) == 0) continue;
    if (p.filter_parent && dir[pos] == dir[np]) continue;
    if (kept++ == 0) answer = pos, score = (int32_t)(keys[c] >> 24);
  }
  const bool ok = kept > 0 && (long long)kept + 1 > (long long)p.min_matches;
  out_match[k] = ok ? place[answer] : kNone;
  out_score[k] = ok ? score : -1;
}

int params_ok(const cbh_merge_params* p, const void* dir_id, const void* under_prefix) {
  if (!p) return mg_inval("merge find: params is NULL");
  if (p->max_matches < 1 || p->max_matches > 55) return mg_inval("merge find: max_matches outside 1..55");
  if (p->thresh < 0 || p->thresh > 65 || p->max_thresh < 0 || p->max_thresh > 65)
    return mg_inval("merge find: a threshold outside 0..65");
  if (p->path_mode < 0 || p->path_mode > 2) return mg_inval("merge find: path_mode outside 0..2");
  if (p->filter_parent && !dir_id) return mg_inval("merge find: filter_parent without dir_id");
  if (p->path_mode && !under_prefix) return mg_inval("merge find: path_mode without under_prefix");
  return CBH_OK;
}

// everything on the device, the arrays holding A then B; total = n_a + n_b, 0 < total < kMostItems
int merge_find_dev(const uint64_t* d_hashes, const uint32_t* d_ids, const uint8_t* d_in_index, const uint32_t* d_dir,
                   const uint8_t* d_under, uint32_t n_a, uint32_t n_b, const cbh_merge_params* p, uint32_t* d_match,
                   int32_t* d_score, hipStream_t s) {
  const uint32_t total = n_a + n_b;
  Scratch scratch(s);
  unsigned long long* keys;
  uint32_t *vals, *s_seen, *s_dir = nullptr, *needle_pos, *status;
  uint64_t* s_hash;
  uint8_t* s_attr;
  CBH_HIP(scratch.get(&keys, (size_t)total * 8));
  CBH_HIP(scratch.get(&vals, (size_t)total * 4));
  CBH_HIP(scratch.get(&s_hash, (size_t)total * 8));
  CBH_HIP(scratch.get(&s_seen, (size_t)total * 4));
  CBH_HIP(scratch.get(&s_attr, (size_t)total));
  if (p->filter_parent) CBH_HIP(scratch.get(&s_dir, (size_t)total * 4));
  CBH_HIP(scratch.get(&needle_pos, (size_t)std::max(n_b, 1u) * 4));
  CBH_HIP(scratch.get(&status, 4));
  CBH_HIP(hipMemsetAsync(status, 0, 4, s));
  const unsigned blocks = (total + 255) / 256;
  // one set: the search for an item's set has nothing to read, set_first stays NULL
  hipLaunchKernelGGL(k_ss_keys, dim3(blocks), dim3(256), 0, s, d_ids, (const uint64_t*)nullptr, 1u, (uint64_t)0, total, keys,
                     vals, status);
  CBH_HIP(hipGetLastError());
  if (int rc = sort_pairs_u64_u32(keys, vals, total, 32, s)) return rc;
  hipLaunchKernelGGL(k_mg_gather, dim3(blocks), dim3(256), 0, s, keys, vals, d_hashes, d_in_index, d_dir, d_under, n_a, total,
                     s_hash, s_seen, s_attr, s_dir, needle_pos, status);
  CBH_HIP(hipGetLastError());
  uint32_t h_status = 0;
  CBH_HIP(hipMemcpyAsync(&h_status, status, 4, hipMemcpyDeviceToHost, s));
  CBH_HIP(hipStreamSynchronize(s));
  if (h_status & 1) return mg_inval("merge find: an item has id 0");
  if (h_status & 2) return mg_inval("merge find: an id occurs twice in A and B");
  if (n_b == 0) return CBH_OK;

  const MgParams k{p->thresh, p->max_thresh, p->min_matches, p->max_matches, p->filter_parent, p->path_mode,
                   p->min_matches > p->max_matches};
  hipLaunchKernelGGL(k_merge_find, dim3((n_b + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, s, s_hash, s_seen, s_attr, s_dir,
                     vals, needle_pos, total, n_b, k, d_match, d_score);
  CBH_HIP(hipGetLastError());
  return CBH_OK;
}

}  // namespace
}  // namespace cbh

extern "C" {

int cbh_merge_find(const uint64_t* hashes, const uint32_t* ids, const uint8_t* in_index, const uint32_t* dir_id,
                   const uint8_t* under_prefix, size_t n_a, size_t n_b, const cbh_merge_params* params, uint32_t* out_match,
                   int32_t* out_score, int device) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  int rc = params_ok(params, dir_id, under_prefix);
  if (rc != CBH_OK) return rc;
  const size_t total = n_a + n_b;
  if (total < n_a || total >= kMostItems) {
    set_last_error_text("merge find: A and B together hold 2^24 items or more");
    return CBH_E_UNSUPPORTED;
  }
  if (total == 0) return CBH_OK;
  if (!hashes || !ids || (n_b && (!out_match || !out_score))) return mg_inval("merge find: a required pointer is NULL");
  for (size_t i = 0; i < total; ++i)
    if (ids[i] == 0) return mg_inval("merge find: an item has id 0");
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  Staging st("merge find");
  uint64_t* d_hashes;
  uint32_t *d_ids, *d_dir = nullptr, *d_match;
  uint8_t *d_in = nullptr, *d_under = nullptr;
  int32_t* d_score;
  const size_t nb1 = std::max<size_t>(n_b, 1);
  st.alloc(&d_hashes, total * 8);
  st.alloc(&d_ids, total * 4);
  if (in_index) st.alloc(&d_in, total);
  if (params->filter_parent) st.alloc(&d_dir, total * 4);
  if (params->path_mode) st.alloc(&d_under, total);
  st.alloc(&d_match, nb1 * 4);
  st.alloc(&d_score, nb1 * 4);
  st.up(d_hashes, hashes, total * 8);
  st.up(d_ids, ids, total * 4);
  if (d_in) st.up(d_in, in_index, total);
  if (d_dir) st.up(d_dir, dir_id, total * 4);
  if (d_under) st.up(d_under, under_prefix, total);
  rc = st.status();
  if (rc == CBH_OK)
    rc = merge_find_dev(d_hashes, d_ids, d_in, d_dir, d_under, (uint32_t)n_a, (uint32_t)n_b, params, d_match, d_score, st.s);
  if (rc != CBH_OK) return rc;
  if (n_b) {
    st.down(out_match, d_match, n_b * 4);
    st.down(out_score, d_score, n_b * 4);
  }
  st.sync();
  return st.status();
}

// The placement (:1628-1650) on a doubly linked list of places in the caller's arrays: A in its order, then every needle
// in B's order in front of its match -- behind it only when the match has a neighbour on both sides and the needle is
// strictly nearer to the one behind (`if (after < before) pos++`, :1643-1648).
int cbh_merge_place(const uint64_t* hashes, size_t n_a, size_t n_b, const uint32_t* match, uint32_t* out_order,
                    uint8_t* out_status, size_t* n_out) {
  using namespace cbh;
  const size_t total = n_a + n_b;
  if (total < n_a || total >= 0xffffffffull) return mg_inval("merge place: more than 2^32 items");
  if (n_out) *n_out = 0;
  if (total == 0) return CBH_OK;
  if (!hashes || !out_order || (n_b && (!match || !out_status))) return mg_inval("merge place: a required pointer is NULL");
  for (size_t k = 0; k < n_b; ++k)
    if (match[k] != kNone && match[k] >= total) return mg_inval("merge place: a match outside A and B");
  std::vector<uint32_t> prev(total, kNone), next(total, kNone);
  std::vector<uint8_t> placed(total, 0);
  uint32_t head = n_a ? 0u : kNone;
  for (size_t i = 0; i < n_a; ++i) {
    placed[i] = 1;
    if (i > 0) prev[i] = (uint32_t)(i - 1);
    if (i + 1 < n_a) next[i] = (uint32_t)(i + 1);
  }
  size_t len = n_a;
  for (size_t k = 0; k < n_b; ++k) {
    const uint32_t me = (uint32_t)(n_a + k), m = match[k];
    if (m == kNone) {
      out_status[k] = CBH_MERGE_NO_MATCH;  // qCritical("no match"), the needle is dropped (:1631-1634)
      continue;
    }
    if (!placed[m]) {
      out_status[k] = CBH_MERGE_MATCH_UNPLACED;  // the reference's Q_ASSERT (:1640); here the needle is dropped
      continue;
    }
    uint32_t before = prev[m], behind = m;  // the needle goes between `before` and `behind`
    if (prev[m] != kNone && next[m] != kNone &&
        __builtin_popcountll(hashes[me] ^ hashes[next[m]]) < __builtin_popcountll(hashes[me] ^ hashes[prev[m]]))
      before = m, behind = next[m];
    prev[me] = before, next[me] = behind;
    prev[behind] = me;
    if (before == kNone)
      head = me;
    else
      next[before] = me;
    placed[me] = 1;
    out_status[k] = CBH_MERGE_PLACED;
    ++len;
  }
  size_t w = 0;
  for (uint32_t i = head; i != kNone; i = next[i]) out_order[w++] = i;
  if (n_out) *n_out = len;
  return CBH_OK;
}

}  // extern "C"
