// sortsimilar.hip -- cbird's -sort-similar (src/main.cpp:1523-1580) for a ragged batch of selections, each chain of
// dependent queries kept on the device.
//
// The reference orders a selection so that every item is followed by its nearest remaining neighbour: for i in 0..n-2
// and j in 0..min(lookBehind, len(sorted))-1 it runs Engine::query of sorted[len-1-j] inside the set unsorted + needle
// and inserts the first match at len-j (no break after an insert, len re-read every pass, failing queries counted).
// Every query's haystack depends on the previous answer, so no batch of finds can replay it; one workgroup per selection
// can: it holds the selection, walks the loop and needs no other workgroup.
//
//   k_ss_keys     one thread per item: key = set << 32 | id, value = the item's place in the caller's arrays
//   (radix sort)  records.hip: every set in ascending id order, so that the POSITION inside a set orders like the id
//   k_ss_gather   hashes / ids / attributes into that order; where the caller's first item of each set went
//   k_sort_similar<LDS>
//                 grid = sets, one workgroup of 64..1024 threads per set, no communication between workgroups and no
//                 waiting on memory: __syncthreads() and trip counts fixed by n.  A query is a minimum of
//                 distance << 24 | position over the unsorted items (ties by position = by id, the project's rule,
//                 SURVEY section 7.2): every lane over its strided items, the wave by DPP, 16 partials through LDS.
//                 Thread 0 then applies searchIndex + filterMatch (src/database.cpp:1691-1757, 1209-1247) to the
//                 minima found so far, inserts, and publishes the next needle.  min_matches <= 1 without a filter and a
//                 needle in the index needs ONE minimum per query; otherwise successive minima ("smallest key above the
//                 last") up to max(max_matches, min_matches + 1) of them.
//                 LDS = true: sets up to 16 384 items keep their hashes in LDS (128 KiB dynamic) -- a query reads 8
//                 bytes per unsorted item from LDS and nothing from memory.  LDS = false: up to CBH_SORT_SIMILAR_MAX
//                 items read them from global memory (512 KiB at most: L2).  Both: 16 KiB of bitmaps (unsorted and in
//                 the index, in the index) + 0.5 KiB of state.  Hashes cannot be poisoned instead: thresholds up to 65
//                 are legal, so no hash value is out of every needle's reach.
//                 Once a whole i iteration has inserted nothing the state cannot change any more: the queries of the
//                 remaining iterations all fail and are added in closed form.
// What bounds a query: at 1 000 items the two barriers and the LDS round trip of the partials, not the popcounts; at
// 16 384 items 16 LDS reads per lane and pass.
#include <algorithm>
#include <vector>

#include "cbh_index.h"
#include "cbh_staging.h"

namespace cbh {
namespace {

#include "sortsimilar_common.h"  // kNone, kMostKeys, kTail, k_ss_keys, wave_min, ss_inval, sets_ok

constexpr uint32_t kLdsItems = 16384;  // largest set whose hashes stay in LDS

struct SsParams {
  int thresh, max_thresh, min_matches, max_matches, filter_parent, path_mode, look_behind;
  int never;  // min_matches > max_matches: 1 + kept > min_matches cannot hold, every query fails
};

// attr: bit 0 = in the index, bit 1 = under the path prefix
__global__ __launch_bounds__(256) void k_ss_gather(const unsigned long long* __restrict__ keys,
                                                   const uint32_t* __restrict__ vals, const uint64_t* __restrict__ hashes,
                                                   const uint8_t* __restrict__ in_index, const uint32_t* __restrict__ dir_id,
                                                   const uint8_t* __restrict__ under, const uint64_t* __restrict__ set_first,
                                                   uint64_t base, uint32_t total, uint64_t* __restrict__ s_hash,
                                                   uint32_t* __restrict__ s_id, uint8_t* __restrict__ s_attr,
                                                   uint32_t* __restrict__ s_dir, uint32_t* __restrict__ first_pos,
                                                   uint32_t* __restrict__ status) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const unsigned long long key = keys[g];
  const uint32_t set = (uint32_t)(key >> 32), src = vals[g];
  if (g > 0 && keys[g - 1] == key) atomicOr(status, 2u);  // the same id twice in one set
  s_hash[g] = hashes[base + src];
  s_id[g] = (uint32_t)key;
  s_attr[g] = (uint8_t)((in_index ? (in_index[base + src] != 0) : 1) | (under ? (under[base + src] != 0) << 1 : 0));
  if (s_dir) s_dir[g] = dir_id[base + src];
  if (base + src == set_first[set]) first_pos[set] = g - (uint32_t)(set_first[set] - base);
}

// out_ids doubles as the list of positions while the workgroup runs; the last step turns positions into ids.
template <bool LDS>
__global__ __launch_bounds__(1024) void k_sort_similar(const uint64_t* __restrict__ g_hash, const uint32_t* __restrict__ g_id,
                                                       const uint8_t* __restrict__ g_attr, const uint32_t* __restrict__ g_dir,
                                                       const uint32_t* __restrict__ first_pos,
                                                       const uint64_t* __restrict__ set_first, uint64_t base, SsParams p,
                                                       uint32_t* __restrict__ out_ids,
                                                       cbh_sort_similar_result* __restrict__ out) {
  extern __shared__ uint64_t lds_hash[];          // LDS: the set's hashes
  __shared__ uint32_t avail[CBH_SORT_SIMILAR_MAX / 32];   // unsorted and in the index: the candidates
  __shared__ uint32_t indexed[CBH_SORT_SIMILAR_MAX / 32];  // in the index (a needle outside it does not count itself)
  __shared__ uint32_t part[2][16];                // the waves' minima, by the parity of the pass
  __shared__ uint32_t needle_of[2];               // the needle's position (kNone: done), by the parity of the query
  __shared__ uint32_t keys[kMostKeys];            // thread 0: the minima of this query
  __shared__ uint32_t tail[kTail + 1];            // thread 0: the last entries of `sorted`
  __shared__ uint32_t final_len;

  const uint32_t set = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const uint64_t first = set_first[set];
  const uint32_t n = (uint32_t)(set_first[set + 1] - first);
  if (LDS ? n > kLdsItems : n <= kLdsItems) return;  // the other variant's set
  const size_t off = (size_t)(first - base);
  uint32_t* order = out_ids + first;
  if (n < 2) {
    if (tid == 0) {
      if (n == 1) order[0] = g_id[off];
      out[set] = cbh_sort_similar_result{n, 0u, 0u, 0u};
    }
    return;
  }
  const uint64_t* hash = LDS ? lds_hash : g_hash + off;
  const uint8_t* attr = g_attr + off;
  const uint32_t start = first_pos[set];
  if (LDS)
    for (uint32_t i = tid; i < n; i += T) lds_hash[i] = g_hash[off + i];
  for (uint32_t w = tid; w < (n + 31) / 32; w += T) {
    uint32_t bits = 0;
    const uint32_t m = min(32u, n - w * 32);
    for (uint32_t b = 0; b < m; ++b) bits |= (uint32_t)(attr[w * 32 + b] & 1) << b;
    indexed[w] = bits;
    avail[w] = (start >> 5) == w ? bits & ~(1u << (start & 31)) : bits;
  }
  if (tid == 0) needle_of[0] = start;

  const bool filters = p.filter_parent != 0 || p.path_mode != 0;
  // no candidate at or beyond this distance can ever count
  const uint32_t reach = (uint32_t)((p.max_thresh > 0 && p.thresh < p.max_thresh) ? p.max_thresh : p.thresh);
  // thread 0's view of the reference's loop
  uint32_t len = 1, held = 1, i_iter = 0, j = 0, queries = 0, not_found = 0, behind = 0;
  bool inserted = false;
  if (tid == 0) tail[0] = start;
  uint32_t pass = 0;

  for (uint32_t q = 0;; ++q) {
    __syncthreads();
    const uint32_t np = needle_of[q & 1];
    if (np == kNone) break;
    const uint64_t hq = hash[np];
    const bool self = (indexed[np >> 5] >> (np & 31)) & 1;
    // how many minima decide this query: enough to tell whether the count passes min_matches (the needle counts itself
    // when it is in the index), and with a filter the max_matches that filterMatch looks at
    int want = max(1, p.min_matches + (self ? 0 : 1));
    if (filters) want = max(want, p.max_matches);
    if (hq == 0 || p.never) want = 0;  // a needle without a hash finds nothing (src/dcthashindex.cpp:196-200)
    int got = 0;
    uint32_t above = 0;  // only keys >= above
    while (got < want) {
      uint32_t best = kNone;
      for (uint32_t i = tid; i < n; i += T) {
        if (!((avail[i >> 5] >> (i & 31)) & 1)) continue;
        const uint32_t d = (uint32_t)__popcll(hq ^ hash[i]);
        const uint32_t key = d << 24 | i;
        if (d < reach && key >= above) best = min(best, key);
      }
      best = wave_min(best);
      if ((tid & 63) == 0) part[pass & 1][tid >> 6] = best;
      __syncthreads();
      best = kNone;
      for (uint32_t w = 0; w < (T + 63) / 64; ++w) best = min(best, part[pass & 1][w]);
      ++pass;
      if (best == kNone) break;
      if (tid == 0) keys[got] = best;
      ++got;
      above = best + 1;
    }
    if (tid != 0) continue;

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
    const uint32_t cut = (uint32_t)min(cnt, p.max_matches);
    for (uint32_t k = 0; k < cut; ++k) {
      const uint32_t c = keys[k] & 0xffffffu;
      if (p.path_mode && (((p.path_mode == 2) ? 1u : 0u) ^ ((attr[c] >> 1) & 1u)) == 0) continue;
      if (p.filter_parent && g_dir[off + c] == g_dir[off + np]) continue;
      if (kept++ == 0) answer = c;
    }
    ++queries;
    if (kept > 0 && (long long)kept + 1 > (long long)p.min_matches) {
      // sorted.insert(len - j, answer): only the last kTail entries can move, older ones are final
      if (held == kTail) {
        order[len - kTail] = tail[0];
        for (uint32_t k = 0; k + 1 < kTail; ++k) tail[k] = tail[k + 1];
        held = kTail - 1;
      }
      for (uint32_t k = held; k > held - j; --k) tail[k] = tail[k - 1];
      tail[held - j] = answer;
      ++held, ++len;
      avail[answer >> 5] &= ~(1u << (answer & 31));
      inserted = true;
      if (j > 0) ++behind;
    } else {
      ++not_found;
    }
    // the next (i, j); `min(lookBehind, sorted.count())` is read again with the new length (:1547)
    uint32_t next = kNone;
    ++j;
    if (j < min((uint32_t)p.look_behind, len)) {
      next = tail[held - 1 - j];
    } else if (!inserted) {
      const uint32_t rest = (n - 2 - i_iter) * min((uint32_t)p.look_behind, len);  // nothing can change any more
      queries += rest, not_found += rest;
    } else if (++i_iter + 1 < n) {
      j = 0, inserted = false;
      next = tail[held - 1];
    }
    needle_of[(q + 1) & 1] = next;
  }

  if (tid == 0) {
    for (uint32_t k = 0; k < held; ++k) order[len - held + k] = tail[k];
    out[set] = cbh_sort_similar_result{len, queries, not_found, behind};
    final_len = len;
  }
  __syncthreads();
  const uint32_t sorted = final_len;
  for (uint32_t k = tid; k < n; k += T) order[k] = k < sorted ? g_id[off + order[k]] : 0u;
}

int params_ok(const cbh_sort_similar_params* p, const void* dir_id, const void* under_prefix) {
  if (!p) return ss_inval("sort similar: params is NULL");
  if (p->look_behind < 1 || p->look_behind > kTail) return ss_inval("sort similar: look_behind outside 1..8");
  if (p->max_matches < 1 || p->max_matches > 55) return ss_inval("sort similar: max_matches outside 1..55");
  if (p->thresh < 0 || p->thresh > 65 || p->max_thresh > 65) return ss_inval("sort similar: a threshold outside 0..65");
  if (p->path_mode < 0 || p->path_mode > 2) return ss_inval("sort similar: path_mode outside 0..2");
  if (p->filter_parent && !dir_id) return ss_inval("sort similar: filter_parent without dir_id");
  if (p->path_mode && !under_prefix) return ss_inval("sort similar: path_mode without under_prefix");
  return CBH_OK;
}

// everything on the device; h_first = set_first on the host, checked by sets_ok
int sort_similar_dev(const uint64_t* d_hashes, const uint32_t* d_ids, const uint8_t* d_in_index, const uint32_t* d_dir,
                     const uint8_t* d_under, const uint64_t* d_first, const uint64_t* h_first, size_t n_sets,
                     uint32_t largest, const cbh_sort_similar_params* p, uint32_t* d_out_ids,
                     cbh_sort_similar_result* d_out, hipStream_t s) {
  const uint64_t base = h_first[0];
  const uint32_t total = (uint32_t)(h_first[n_sets] - base);
  if (total == 0) {
    CBH_HIP(hipMemsetAsync(d_out, 0, n_sets * sizeof(cbh_sort_similar_result), s));
    return CBH_OK;
  }
  Scratch scratch(s);
  unsigned long long* keys;
  uint32_t *vals, *s_id, *s_dir = nullptr, *first_pos, *status;
  uint64_t* s_hash;
  uint8_t* s_attr;
  CBH_HIP(scratch.get(&keys, (size_t)total * 8));
  CBH_HIP(scratch.get(&vals, (size_t)total * 4));
  CBH_HIP(scratch.get(&s_hash, (size_t)total * 8));
  CBH_HIP(scratch.get(&s_id, (size_t)total * 4));
  CBH_HIP(scratch.get(&s_attr, (size_t)total));
  if (p->filter_parent) CBH_HIP(scratch.get(&s_dir, (size_t)total * 4));
  CBH_HIP(scratch.get(&first_pos, n_sets * 4));
  CBH_HIP(scratch.get(&status, 4));
  CBH_HIP(hipMemsetAsync(status, 0, 4, s));
  const unsigned blocks = (total + 255) / 256;
  hipLaunchKernelGGL(k_ss_keys, dim3(blocks), dim3(256), 0, s, d_ids, d_first, (uint32_t)n_sets, base, total, keys, vals,
                     status);
  CBH_HIP(hipGetLastError());
  int set_bits = 1;
  while (set_bits < 32 && ((uint64_t)1 << set_bits) < n_sets) ++set_bits;
  if (int rc = sort_pairs_u64_u32(keys, vals, total, 32 + set_bits, s)) return rc;
  hipLaunchKernelGGL(k_ss_gather, dim3(blocks), dim3(256), 0, s, keys, vals, d_hashes, d_in_index, d_dir, d_under, d_first,
                     base, total, s_hash, s_id, s_attr, s_dir, first_pos, status);
  CBH_HIP(hipGetLastError());
  uint32_t h_status = 0;
  CBH_HIP(hipMemcpyAsync(&h_status, status, 4, hipMemcpyDeviceToHost, s));
  CBH_HIP(hipStreamSynchronize(s));
  if (h_status & 1) return ss_inval("sort similar: an item has id 0");
  if (h_status & 2) return ss_inval("sort similar: an id occurs twice in one set");

  SsParams k{p->thresh, p->max_thresh, p->min_matches, p->max_matches, p->filter_parent, p->path_mode, p->look_behind,
             p->min_matches > p->max_matches};
  bool small = false, large = false;
  for (size_t i = 0; i < n_sets; ++i) (h_first[i + 1] - h_first[i] > kLdsItems ? large : small) = true;
  const unsigned threads = std::min(1024u, std::max(64u, (largest + 63) / 64 * 64));
  if (small) {
    const size_t smem = (size_t)std::min(largest, kLdsItems) * 8;
    if (smem > 48 * 1024)
      CBH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sort_similar<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(k_sort_similar<true>, dim3((unsigned)n_sets), dim3(std::min(threads, 1024u)), smem, s, s_hash, s_id,
                       s_attr, s_dir, first_pos, d_first, base, k, d_out_ids, d_out);
    CBH_HIP(hipGetLastError());
  }
  if (large) {
    hipLaunchKernelGGL(k_sort_similar<false>, dim3((unsigned)n_sets), dim3(1024), 0, s, s_hash, s_id, s_attr, s_dir,
                       first_pos, d_first, base, k, d_out_ids, d_out);
    CBH_HIP(hipGetLastError());
  }
  return CBH_OK;
}

}  // namespace
}  // namespace cbh

extern "C" {

int cbh_sort_similar_dev(const void* d_hashes, const void* d_ids, const void* d_in_index, const void* d_dir_id,
                         const void* d_under_prefix, const void* d_set_first, size_t n_sets,
                         const cbh_sort_similar_params* params, void* d_out_ids, void* d_out, int device, void* stream) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  int rc = params_ok(params, d_dir_id, d_under_prefix);
  if (rc != CBH_OK) return rc;
  if (n_sets == 0) return CBH_OK;
  if (!d_set_first || !d_out) return ss_inval("sort similar: a required pointer is NULL");
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  hipStream_t s = (hipStream_t)stream;
  std::vector<uint64_t> h_first(n_sets + 1);
  CBH_HIP(hipMemcpyAsync(h_first.data(), d_set_first, (n_sets + 1) * 8, hipMemcpyDeviceToHost, s));
  CBH_HIP(hipStreamSynchronize(s));
  uint32_t largest = 0;
  if ((rc = sets_ok(h_first.data(), n_sets, &largest)) != CBH_OK) return rc;
  if (h_first[n_sets] > h_first[0] && (!d_hashes || !d_ids || !d_out_ids))
    return ss_inval("sort similar: a required pointer is NULL");
  return sort_similar_dev((const uint64_t*)d_hashes, (const uint32_t*)d_ids, (const uint8_t*)d_in_index,
                          (const uint32_t*)d_dir_id, (const uint8_t*)d_under_prefix, (const uint64_t*)d_set_first,
                          h_first.data(), n_sets, largest, params, (uint32_t*)d_out_ids, (cbh_sort_similar_result*)d_out, s);
}

int cbh_sort_similar(const uint64_t* hashes, const uint32_t* ids, const uint8_t* in_index, const uint32_t* dir_id,
                     const uint8_t* under_prefix, const uint64_t* set_first, size_t n_sets,
                     const cbh_sort_similar_params* params, uint32_t* out_ids, cbh_sort_similar_result* out, int device) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  int rc = params_ok(params, dir_id, under_prefix);
  if (rc != CBH_OK) return rc;
  if (n_sets == 0) return CBH_OK;
  if (!set_first || !out) return ss_inval("sort similar: a required pointer is NULL");
  uint32_t largest = 0;
  if ((rc = sets_ok(set_first, n_sets, &largest)) != CBH_OK) return rc;
  const uint64_t base = set_first[0], total = set_first[n_sets] - base;
  if (total && (!hashes || !ids || !out_ids)) return ss_inval("sort similar: a required pointer is NULL");
  for (uint64_t i = 0; i < total; ++i)
    if (ids[base + i] == 0) return ss_inval("sort similar: an item has id 0");
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  // the device copies hold the batch's items only: set_first goes up rebased to 0
  std::vector<uint64_t> first0(set_first, set_first + n_sets + 1);
  for (uint64_t& f : first0) f -= base;
  Staging st("sort similar");
  uint64_t *d_hashes, *d_first;
  uint32_t *d_ids, *d_dir = nullptr, *d_out_ids;
  uint8_t *d_in = nullptr, *d_under = nullptr;
  cbh_sort_similar_result* d_out;
  const size_t cnt = std::max<uint64_t>(total, 1);
  st.alloc(&d_hashes, cnt * 8);
  st.alloc(&d_ids, cnt * 4);
  if (in_index) st.alloc(&d_in, cnt);
  if (params->filter_parent) st.alloc(&d_dir, cnt * 4);
  if (params->path_mode) st.alloc(&d_under, cnt);
  st.alloc(&d_first, (n_sets + 1) * 8);
  st.alloc(&d_out_ids, cnt * 4);
  st.alloc(&d_out, n_sets * sizeof(cbh_sort_similar_result));
  if (total) {
    st.up(d_hashes, hashes + base, total * 8);
    st.up(d_ids, ids + base, total * 4);
    if (d_in) st.up(d_in, in_index + base, total);
    if (d_dir) st.up(d_dir, dir_id + base, total * 4);
    if (d_under) st.up(d_under, under_prefix + base, total);
  }
  st.up(d_first, first0.data(), (n_sets + 1) * 8);
  rc = st.status();
  if (rc == CBH_OK)
    rc = sort_similar_dev(d_hashes, d_ids, d_in, d_dir, d_under, d_first, first0.data(), n_sets, largest, params, d_out_ids,
                          d_out, st.s);
  if (rc != CBH_OK) return rc;
  if (total) st.down(out_ids + base, d_out_ids, total * 4);
  st.down(out, d_out, n_sets * sizeof(cbh_sort_similar_result));
  st.sync();
  return st.status();
}

}  // extern "C"
