// sortsimilar_common.h -- internal: what the two -sort-similar chains share (sortsimilar.hip: 64-bit hashes;
// sortsimilar_table.hip: a table of scores).  Include inside `namespace cbh { namespace {`, after cbh_index.h.
#pragma once

constexpr uint32_t kNone = 0xffffffffu;
constexpr int kMostKeys = 56;  // max(max_matches <= 55, min_matches + 1 <= 56)
constexpr int kTail = 8;       // look_behind <= 8: the entries of `sorted` a pass can still read or move

__global__ __launch_bounds__(256) void k_ss_keys(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ set_first,
                                                 uint32_t n_sets, uint64_t base, uint32_t total,
                                                 unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals,
                                                 uint32_t* __restrict__ status) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  uint32_t lo = 0, hi = n_sets;  // last set whose first is <= base + g (empty sets in front of it share that first)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (set_first[mid] <= base + g)
      lo = mid;
    else
      hi = mid;
  }
  const uint32_t id = ids[base + g];
  if (id == 0) atomicOr(status, 1u);
  keys[g] = (unsigned long long)lo << 32 | id;
  vals[g] = g;
}

// minimum over the 64 lanes, in every lane.  row_shr:n = 0x110 + n inside each row of 16 lanes, then row_bcast:15
// (0x142) onto rows 1 | 3 and row_bcast:31 (0x143) onto rows 2 and 3 (wave_prefix_sum in hamm64_mfma.hip has the same
// ladder); lanes without a source take `old`, the identity.  Lane 63 ends with the whole wave's minimum.
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)kNone, (int)v, 0x111, 0xf, 0xf, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)kNone, (int)v, 0x112, 0xf, 0xf, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)kNone, (int)v, 0x114, 0xf, 0xf, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)kNone, (int)v, 0x118, 0xf, 0xf, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)kNone, (int)v, 0x142, 0xa, 0xf, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)kNone, (int)v, 0x143, 0xc, 0xf, false));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

int ss_inval(const char* why) {
  set_last_error_text(why);
  return CBH_E_INVAL;
}

// set_first on the host: ascending, every set within CBH_SORT_SIMILAR_MAX, the batch within 32-bit positions
int sets_ok(const uint64_t* set_first, size_t n_sets, uint32_t* largest) {
  *largest = 0;
  for (size_t s = 0; s < n_sets; ++s) {
    if (set_first[s + 1] < set_first[s]) return ss_inval("sort similar: set_first is not ascending");
    const uint64_t n = set_first[s + 1] - set_first[s];
    if (n > CBH_SORT_SIMILAR_MAX) {
      set_last_error_text("sort similar: a set above CBH_SORT_SIMILAR_MAX items");
      return CBH_E_UNSUPPORTED;
    }
    *largest = std::max(*largest, (uint32_t)n);
  }
  if (n_sets > 0xfffffff0ull || set_first[n_sets] - set_first[0] > 0xfffffff0ull)
    return ss_inval("sort similar: more than 2^32 sets or items in one call");
  return CBH_OK;
}
