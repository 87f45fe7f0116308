// sortsimilar_table.hip -- cbird's -sort-similar (src/main.cpp:1523-1580) over a TABLE of pair scores, for every index
// whose score of a pair does not depend on what else is in the slice (the colour index: color.hip fills the table).
//
// The loop is the one sortsimilar.hip restates (sorted / unsorted, look_behind passes whose bound is read again on every
// pass, no break after a hit, failing passes counted, items never reached dropped, the closed form once a whole i
// iteration has inserted nothing); what differs is the candidate rule: the score of (needle r, candidate c) is
// table[r][c], a uint16_t, 0xFFFF = no match; no thresholds, no escalation.
//
//   k_ss_keys       sortsimilar_common.h: key = set << 32 | id, value = the item's place in the caller's arrays
//   (radix sort)    records.hip: every set in ascending id order, so that the POSITION inside a set orders like the id
//   k_st_gather     ids / attributes into that order; where the caller's first item of each set went; an id twice
//   k_st_permute    the table's rows and columns into that order, rows padded to a multiple of 8 scores (16 bytes)
//   k_sort_similar_table
//                   grid = sets, one workgroup of 64..1024 threads per set, no communication between workgroups and no
//                   waiting on memory: __syncthreads() and trip counts fixed by n.  A query is a minimum of
//                   score << 16 | position over the candidates (ties by position = by id): a lane takes 8 scores with
//                   one 16-byte load -- skipped when none of the 8 items is a candidate any more -- the wave reduces by
//                   DPP, the waves' partials go through LDS.  Thread 0 applies the max_matches cut, path_mode /
//                   filter_parent and the min_matches acceptance to the minima found so far, inserts, and publishes the
//                   next needle.  min_matches <= 1 without a filter needs ONE minimum per query; otherwise successive
//                   minima ("smallest key above the last"), at most max(max_matches, min_matches + 1) of them.
//                   LDS: 8 KiB bitmap (unsorted and in the index) + 0.5 KiB of state.  Rows are read from global memory
//                   (128 KiB at most: L2) and never staged.
// What bounds a query: the two barriers and the L2 round trip of the row's loads; the arithmetic is 8 compares per load.
#include <algorithm>
#include <vector>

#include "cbh_index.h"
#include "cbh_staging.h"

namespace cbh {
namespace {

#include "sortsimilar_common.h"  // kNone, kMostKeys, kTail, k_ss_keys, wave_min, ss_inval, sets_ok

static_assert(CBH_SORT_SIMILAR_MAX <= 65536, "a position has to fit the key's low 16 bits");

struct StParams {
  int min_matches, max_matches, filter_parent, path_mode, look_behind;
  // how many minima decide a query: enough to tell whether 1 + kept passes min_matches, and with a filter the
  // max_matches that filterMatch looks at; 0 when min_matches > max_matches: 1 + kept > min_matches cannot hold, every
  // query fails.  The needle is not unsorted, so it never takes one of these places
  int want;
};

StParams st_params(const cbh_sort_table_params* p) {
  int want = std::max(1, p->min_matches);
  if (p->filter_parent || p->path_mode) want = std::max(want, p->max_matches);
  if (p->min_matches > p->max_matches) want = 0;
  return StParams{p->min_matches, p->max_matches, p->filter_parent, p->path_mode, p->look_behind, want};
}

// attr: bit 0 = in the index, bit 1 = under the path prefix
__global__ __launch_bounds__(256) void k_st_gather(const unsigned long long* __restrict__ keys,
                                                   const uint32_t* __restrict__ vals, const uint8_t* __restrict__ in_index,
                                                   const uint32_t* __restrict__ dir_id, const uint8_t* __restrict__ under,
                                                   const uint64_t* __restrict__ set_first, uint64_t base, uint32_t total,
                                                   uint32_t* __restrict__ s_id, uint8_t* __restrict__ s_attr,
                                                   uint32_t* __restrict__ s_dir, uint32_t* __restrict__ first_pos,
                                                   uint32_t* __restrict__ status) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const unsigned long long key = keys[g];
  const uint32_t set = (uint32_t)(key >> 32), src = vals[g];
  if (g > 0 && keys[g - 1] == key) atomicOr(status, 2u);  // the same id twice in one set
  s_id[g] = (uint32_t)key;
  s_attr[g] = (uint8_t)((in_index ? (in_index[base + src] != 0) : 1) | (under ? (under[base + src] != 0) << 1 : 0));
  if (s_dir) s_dir[g] = dir_id[base + src];
  if (base + src == set_first[set]) first_pos[set] = g - (uint32_t)(set_first[set] - base);
}

// one workgroup per row of the sorted tables (grid-stride over the batch's items): sorted[i][j] = caller[src(i)][src(j)]
__global__ __launch_bounds__(256) void k_st_permute(const unsigned long long* __restrict__ keys,
                                                    const uint32_t* __restrict__ vals, const uint16_t* __restrict__ scores,
                                                    const uint64_t* __restrict__ table_first,
                                                    const uint64_t* __restrict__ set_first, uint64_t base, uint32_t total,
                                                    const uint64_t* __restrict__ sorted_first,
                                                    uint16_t* __restrict__ sorted) {
  for (uint32_t g = blockIdx.x; g < total; g += gridDim.x) {
    const uint32_t set = (uint32_t)(keys[g] >> 32);
    const uint32_t first = (uint32_t)(set_first[set] - base), n = (uint32_t)(set_first[set + 1] - set_first[set]);
    const uint32_t stride = sort_table_row_stride(n);
    const uint16_t* src = scores + table_first[set] + (size_t)(vals[g] - first) * n;
    uint16_t* dst = sorted + sorted_first[set] + (size_t)(g - first) * stride;
    for (uint32_t j = threadIdx.x; j < stride; j += 256) dst[j] = j < n ? src[vals[first + j] - first] : (uint16_t)0xffff;
  }
}

// out_ids doubles as the list of positions while the workgroup runs; the last step turns positions into ids.
// table: set s at sorted_first[s] (a multiple of 8 scores from a 16-byte aligned base), n rows of sort_table_row_stride(n) scores
__global__ __launch_bounds__(1024) void k_sort_similar_table(const uint16_t* __restrict__ table,
                                                             const uint64_t* __restrict__ sorted_first,
                                                             const uint32_t* __restrict__ g_id,
                                                             const uint8_t* __restrict__ g_attr,
                                                             const uint32_t* __restrict__ g_dir,
                                                             const uint32_t* __restrict__ first_pos,
                                                             const uint64_t* __restrict__ set_first, uint64_t base,
                                                             StParams p, uint32_t* __restrict__ out_ids,
                                                             cbh_sort_similar_result* __restrict__ out) {
  __shared__ uint32_t avail[CBH_SORT_SIMILAR_MAX / 32];  // unsorted and in the index: the candidates
  __shared__ uint32_t part[2][16];                       // the waves' minima, by the parity of the pass
  __shared__ uint32_t needle_of[2];                      // the needle's position (kNone: done), by the parity of the query
  __shared__ uint32_t keys[kMostKeys];                   // thread 0: the minima of this query
  __shared__ uint32_t tail[kTail + 1];                   // thread 0: the last entries of `sorted`
  __shared__ uint32_t final_len;

  const uint32_t set = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const uint64_t first = set_first[set];
  const uint32_t n = (uint32_t)(set_first[set + 1] - first);
  const size_t off = (size_t)(first - base);
  uint32_t* order = out_ids + first;
  if (n < 2) {
    if (tid == 0) {
      if (n == 1) order[0] = g_id[off];
      out[set] = cbh_sort_similar_result{n, 0u, 0u, 0u};
    }
    return;
  }
  const uint8_t* attr = g_attr + off;
  const uint32_t start = first_pos[set];
  const uint32_t stride = sort_table_row_stride(n);
  const uint16_t* rows = table + sorted_first[set];
  for (uint32_t w = tid; w < (n + 31) / 32; w += T) {
    uint32_t bits = 0;
    const uint32_t m = min(32u, n - w * 32);
    for (uint32_t b = 0; b < m; ++b) bits |= (uint32_t)(attr[w * 32 + b] & 1) << b;
    avail[w] = (start >> 5) == w ? bits & ~(1u << (start & 31)) : bits;
  }
  if (tid == 0) needle_of[0] = start;

  // thread 0's view of the reference's loop
  uint32_t len = 1, held = 1, i_iter = 0, j = 0, queries = 0, not_found = 0, behind = 0;
  bool inserted = false;
  if (tid == 0) tail[0] = start;
  uint32_t pass = 0;

  for (uint32_t q = 0;; ++q) {
    __syncthreads();
    const uint32_t np = needle_of[q & 1];
    if (np == kNone) break;
    const uint4* row = reinterpret_cast<const uint4*>(rows + (size_t)np * stride);
    int got = 0;
    uint32_t above = 0;  // only keys >= above
    while (got < p.want) {
      // The minimum is taken over key - above (mod 2^32), with all ones where the item is no candidate: keys under
      // `above` wrap to 2^32 - above or more, "no match" keys (score 0xFFFF) stay at 0xFFFF0000 - above or more, and every
      // key that counts lies under that -- one test after the reduction instead of three compares per score.
      uint32_t best = kNone;
      for (uint32_t k = tid; k < stride / 8; k += T) {
        const uint32_t bits = (avail[k >> 2] >> ((k & 3) * 8)) & 0xffu;  // items 8k .. 8k + 7
        if (bits == 0) continue;
        const uint4 v = row[k];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t e = 0; e < 8; ++e) {
          const uint32_t key = ((e & 1) ? (w[e >> 1] & 0xffff0000u) : (w[e >> 1] << 16)) | (k * 8 + e);
          best = min(best, (key - above) | (((bits >> e) & 1u) - 1u));
        }
      }
      best = wave_min(best);
      if ((tid & 63) == 0) part[pass & 1][tid >> 6] = best;
      __syncthreads();
      best = kNone;
      for (uint32_t w = 0; w < (T + 63) / 64; ++w) best = min(best, part[pass & 1][w]);
      ++pass;
      if (best >= 0xffff0000u - above) break;
      best += above;
      if (tid == 0) keys[got] = best;
      ++got;
      above = best + 1;
    }
    if (tid != 0) continue;

    // the first max_matches in (score, id) order, then filterMatch on them (src/database.cpp:1217-1245)
    uint32_t kept = 0, answer = kNone;
    const uint32_t cut = (uint32_t)min(got, p.max_matches);
    for (uint32_t k = 0; k < cut; ++k) {
      const uint32_t c = keys[k] & 0xffffu;
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

// everything on the device, the table in the caller's item order; h_first = set_first on the host, checked by sets_ok
int sort_table_dev(const uint16_t* d_scores, const uint64_t* d_table_first, const uint32_t* d_ids, const uint8_t* d_in_index,
                   const uint32_t* d_dir, const uint8_t* d_under, const uint64_t* d_first, const uint64_t* h_first,
                   size_t n_sets, uint32_t largest, const cbh_sort_table_params* p, uint32_t* d_out_ids,
                   cbh_sort_similar_result* d_out, hipStream_t s) {
  const uint64_t base = h_first[0];
  const uint32_t total = (uint32_t)(h_first[n_sets] - base);
  if (total == 0) {
    CBH_HIP(hipMemsetAsync(d_out, 0, n_sets * sizeof(cbh_sort_similar_result), s));
    return CBH_OK;
  }
  std::vector<uint64_t> h_sorted_first(n_sets);
  const uint64_t table_scores = sort_table_layout(h_first, n_sets, h_sorted_first.data());
  Scratch scratch(s);
  unsigned long long* keys;
  uint32_t *vals, *s_id, *s_dir = nullptr, *first_pos, *status;
  uint8_t* s_attr;
  uint64_t* sorted_first;
  uint16_t* sorted;
  CBH_HIP(scratch.get(&keys, (size_t)total * 8));
  CBH_HIP(scratch.get(&vals, (size_t)total * 4));
  CBH_HIP(scratch.get(&s_id, (size_t)total * 4));
  CBH_HIP(scratch.get(&s_attr, (size_t)total));
  if (p->filter_parent) CBH_HIP(scratch.get(&s_dir, (size_t)total * 4));
  CBH_HIP(scratch.get(&first_pos, n_sets * 4));
  CBH_HIP(scratch.get(&status, 4));
  CBH_HIP(scratch.get(&sorted_first, n_sets * 8));
  CBH_HIP(scratch.get(&sorted, (size_t)table_scores * 2));
  CBH_HIP(hipMemsetAsync(status, 0, 4, s));
  const unsigned blocks = (total + 255) / 256;
  hipLaunchKernelGGL(k_ss_keys, dim3(blocks), dim3(256), 0, s, d_ids, d_first, (uint32_t)n_sets, base, total, keys, vals,
                     status);
  CBH_HIP(hipGetLastError());
  int set_bits = 1;
  while (set_bits < 32 && ((uint64_t)1 << set_bits) < n_sets) ++set_bits;
  if (int rc = sort_pairs_u64_u32(keys, vals, total, 32 + set_bits, s)) return rc;
  hipLaunchKernelGGL(k_st_gather, dim3(blocks), dim3(256), 0, s, keys, vals, d_in_index, d_dir, d_under, d_first, base,
                     total, s_id, s_attr, s_dir, first_pos, status);
  CBH_HIP(hipGetLastError());
  uint32_t h_status = 0;
  CBH_HIP(hipMemcpyAsync(sorted_first, h_sorted_first.data(), n_sets * 8, hipMemcpyHostToDevice, s));
  CBH_HIP(hipMemcpyAsync(&h_status, status, 4, hipMemcpyDeviceToHost, s));
  CBH_HIP(hipStreamSynchronize(s));
  if (h_status & 1) return ss_inval("sort similar: an item has id 0");
  if (h_status & 2) return ss_inval("sort similar: an id occurs twice in one set");
  hipLaunchKernelGGL(k_st_permute, dim3(std::min(total, 1u << 20)), dim3(256), 0, s, keys, vals, d_scores, d_table_first,
                     d_first, base, total, sorted_first, sorted);
  CBH_HIP(hipGetLastError());
  return launch_sort_table_chain(sorted, sorted_first, s_id, s_attr, s_dir, first_pos, d_first, base, n_sets, largest, p,
                                 d_out_ids, d_out, s);
}

}  // namespace

int sort_table_params_ok(const cbh_sort_table_params* p, const void* dir_id, const void* under_prefix) {
  if (!p) return ss_inval("sort similar: params is NULL");
  if (p->look_behind < 1 || p->look_behind > kTail) return ss_inval("sort similar: look_behind outside 1..8");
  if (p->max_matches < 1 || p->max_matches > 55) return ss_inval("sort similar: max_matches outside 1..55");
  if (p->path_mode < 0 || p->path_mode > 2) return ss_inval("sort similar: path_mode outside 0..2");
  if (p->filter_parent && !dir_id) return ss_inval("sort similar: filter_parent without dir_id");
  if (p->path_mode && !under_prefix) return ss_inval("sort similar: path_mode without under_prefix");
  return CBH_OK;
}

uint64_t sort_table_layout(const uint64_t* h_first, size_t n_sets, uint64_t* h_sorted_first) {
  uint64_t at = 0;
  for (size_t i = 0; i < n_sets; ++i) {
    const uint64_t n = h_first[i + 1] - h_first[i];
    h_sorted_first[i] = at;
    at += n * sort_table_row_stride((uint32_t)n);
  }
  return std::max<uint64_t>(at, 8);
}

int launch_sort_table_chain(const uint16_t* d_sorted, const uint64_t* d_sorted_first, const uint32_t* s_id,
                            const uint8_t* s_attr, const uint32_t* s_dir, const uint32_t* first_pos, const uint64_t* d_first,
                            uint64_t base, size_t n_sets, uint32_t largest, const cbh_sort_table_params* p,
                            uint32_t* d_out_ids, cbh_sort_similar_result* d_out, hipStream_t s) {
  if (n_sets == 0) return CBH_OK;
  const StParams k = st_params(p);
  // a lane takes 8 scores per load: a wave per 512 items, at most 1024 threads
  const unsigned threads = std::min(1024u, std::max(64u, (sort_table_row_stride(largest) / 8 + 63) / 64 * 64));
  hipLaunchKernelGGL(k_sort_similar_table, dim3((unsigned)n_sets), dim3(threads), 0, s, d_sorted, d_sorted_first, s_id,
                     s_attr, s_dir, first_pos, d_first, base, k, d_out_ids, d_out);
  CBH_HIP(hipGetLastError());
  return CBH_OK;
}

}  // namespace cbh

extern "C" {

int cbh_sort_similar_table_dev(const void* d_scores, const void* d_table_first, const void* d_ids, const void* d_in_index,
                               const void* d_dir_id, const void* d_under_prefix, const void* d_set_first, size_t n_sets,
                               const cbh_sort_table_params* params, void* d_out_ids, void* d_out, int device, void* stream) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  int rc = sort_table_params_ok(params, d_dir_id, d_under_prefix);
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
  if (h_first[n_sets] > h_first[0] && (!d_scores || !d_table_first || !d_ids || !d_out_ids))
    return ss_inval("sort similar: a required pointer is NULL");
  return sort_table_dev((const uint16_t*)d_scores, (const uint64_t*)d_table_first, (const uint32_t*)d_ids,
                        (const uint8_t*)d_in_index, (const uint32_t*)d_dir_id, (const uint8_t*)d_under_prefix,
                        (const uint64_t*)d_set_first, h_first.data(), n_sets, largest, params, (uint32_t*)d_out_ids,
                        (cbh_sort_similar_result*)d_out, s);
}

int cbh_sort_similar_table(const uint16_t* scores, const uint64_t* table_first, const uint32_t* ids, const uint8_t* in_index,
                           const uint32_t* dir_id, const uint8_t* under_prefix, const uint64_t* set_first, size_t n_sets,
                           const cbh_sort_table_params* params, uint32_t* out_ids, cbh_sort_similar_result* out, int device) {
  using namespace cbh;
  if (!device_usable(device)) return CBH_E_NODEVICE;
  int rc = sort_table_params_ok(params, dir_id, under_prefix);
  if (rc != CBH_OK) return rc;
  if (n_sets == 0) return CBH_OK;
  if (!set_first || !out) return ss_inval("sort similar: a required pointer is NULL");
  uint32_t largest = 0;
  if ((rc = sets_ok(set_first, n_sets, &largest)) != CBH_OK) return rc;
  const uint64_t base = set_first[0], total = set_first[n_sets] - base;
  if (total && (!scores || !table_first || !ids || !out_ids)) return ss_inval("sort similar: a required pointer is NULL");
  for (uint64_t i = 0; i < total; ++i)
    if (ids[base + i] == 0) return ss_inval("sort similar: an item has id 0");
  DeviceGuard g(device);
  if (!g.ok) return CBH_E_NODEVICE;
  // the device copies hold the batch's items and tables only: set_first and table_first go up rebased to 0, in one block
  // (set_first's n_sets + 1 entries, then table_first's n_sets)
  uint64_t lo = ~0ull, hi = 0;
  for (size_t s = 0; s < n_sets; ++s) {
    const uint64_t n = set_first[s + 1] - set_first[s];
    if (n == 0) continue;
    lo = std::min(lo, table_first[s]);
    hi = std::max(hi, table_first[s] + n * n);
  }
  if (lo > hi) lo = hi = 0;
  std::vector<uint64_t> first0(2 * n_sets + 1);
  for (size_t s = 0; s <= n_sets; ++s) first0[s] = set_first[s] - base;
  for (size_t s = 0; s < n_sets; ++s) first0[n_sets + 1 + s] = set_first[s + 1] > set_first[s] ? table_first[s] - lo : 0;
  Staging st("sort similar table");
  uint16_t* d_scores;
  uint64_t* d_first;
  uint32_t *d_ids, *d_dir = nullptr, *d_out_ids;
  uint8_t *d_in = nullptr, *d_under = nullptr;
  cbh_sort_similar_result* d_out;
  const size_t cnt = std::max<uint64_t>(total, 1);
  st.alloc(&d_scores, std::max<uint64_t>(hi - lo, 8) * 2);
  st.alloc(&d_ids, cnt * 4);
  if (in_index) st.alloc(&d_in, cnt);
  if (params->filter_parent) st.alloc(&d_dir, cnt * 4);
  if (params->path_mode) st.alloc(&d_under, cnt);
  st.alloc(&d_first, first0.size() * 8);
  st.alloc(&d_out_ids, cnt * 4);
  st.alloc(&d_out, n_sets * sizeof(cbh_sort_similar_result));
  if (total) {
    st.up(d_scores, scores + lo, (hi - lo) * 2);
    st.up(d_ids, ids + base, total * 4);
    if (d_in) st.up(d_in, in_index + base, total);
    if (d_dir) st.up(d_dir, dir_id + base, total * 4);
    if (d_under) st.up(d_under, under_prefix + base, total);
  }
  st.up(d_first, first0.data(), first0.size() * 8);
  rc = st.status();
  if (rc == CBH_OK)
    rc = sort_table_dev(d_scores, d_first + n_sets + 1, d_ids, d_in, d_dir, d_under, d_first, first0.data(), n_sets, largest,
                        params, d_out_ids, d_out, st.s);
  if (rc != CBH_OK) return rc;
  if (total) st.down(out_ids + base, d_out_ids, total * 4);
  st.down(out, d_out, n_sets * sizeof(cbh_sort_similar_result));
  st.sync();
  return st.status();
}

}  // extern "C"
