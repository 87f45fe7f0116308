// clusters.hip -- "which of my files are the same picture?" as a partition of a DctHashIndex: the connected components
// of its match graph (single-linkage clusters at dctThresh), exact, in one pass over the edges.
//
// Nodes are the live entries (id != 0, hash != 0), edges the pairs with popcount(h_i ^ h_j) < thresh -- find()'s
// predicate (src/dcthashindex.cpp:210-217).  The reference has no counterpart: its only tool for making sets out of
// -similar's groups is Media::mergeGroupList (src/media.cpp:300-324), which is neither transitive nor better than
// quadratic in the number of groups.
//
// Host flow (cluster_core): the node table = live (id, hash) pairs in ascending id order (one pair sort, records.hip), so
// that a node's NUMBER is the rank of its id and the smallest node of a component is its smallest id; then the table's
// hashes go through scan_all as needles, "cluster_chunk" of them per scan, and every chunk's records are consumed by
// k_cl_hook and dropped.  A chunk with more than "cluster_max_records" records is halved and scanned again.
//
//   k_cl_slots    one thread per slot: key = id (live) or 2^32 (not), value = slot; counts the live slots per wave
//   k_cl_table    one thread per sorted key: the table's ids and hashes; flags an id that two live slots hold
//   k_cl_init     parent[i] = i, nearest[i] = 0xFF
//   k_cl_hook     one thread per record (needle node i = chunk base + query, haystack node j = binary search of the
//                 record's id in the table).  Lowers nearest[i] (test, then atomicMin), and for j < i -- every edge
//                 is reported from both ends, the larger end unites -- walks to both roots (reads only) and hooks the
//                 larger root under the smaller with old = atomicMin(&parent[hi], lo).  old != hi: another thread hooked
//                 hi first; go on with the pair (old, lo).  parent[x] <= x always and values only ever decrease, so there
//                 are no cycles, a walk ends, and the larger endpoint of the pair strictly decreases from one round to the
//                 next: the trip count is bounded by the data, no thread ever waits for another.  No path compression
//                 here: a racing plain store could undo an atomicMin.
//   k_cl_flatten  parent[i] = root(i), after every chunk (so that walks stay short) -- no atomicMin runs beside it
//   k_cl_labels   ids / label = id of the root / nearest as bytes, for the caller
//   k_cl_sizes    size[root] += the lanes of the wave under that root (one add per wave and root)
//   k_cl_tile_sums / k_cl_tile_offsets / k_cl_emit
//                 exclusive scan of (1, size) over the roots of components with >= min_members nodes, packed in one u64
//                 (tiles of 1024 nodes, a one-workgroup pass over the tile sums): a cluster's number and first member
//                 slot; k_cl_emit also writes every kept node's key root << 32 | node
//   (radix sort)  those keys: clusters in ascending first id, members in ascending id
//   k_cl_members  cbh_match{id, nearest} per sorted key
// What bounds the call: the scans.  Per record the rest costs one binary search in the id table (L2 resident up to a few
// million nodes) and at most one atomicMin per round of the union.
#include <algorithm>
#include <atomic>
#include <vector>

#include "cbh_index.h"

namespace cbh {
namespace {

std::atomic<int> g_cluster_chunk{1 << 20};        // "cluster_chunk": needle nodes per scan
std::atomic<int> g_cluster_max_records{1 << 26};  // "cluster_max_records": records one scan may materialise (512 MB)
std::atomic<int> g_cluster_timing{0};             // "cluster_timing": 1 = time the stages apart with events
std::atomic<long long> g_cluster_us[3] = {{0}, {0}, {0}};  // the last successful call's table / hook + flatten / emit

constexpr uint32_t kNoNeighbour = 0xffu;
constexpr int kTile = 1024;  // nodes per workgroup of the scan passes: 256 threads x 4

int cl_fail(int code, const char* why) {
  set_last_error_text(why);
  return code;
}

__device__ __forceinline__ uint32_t cl_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// parent[x] <= x, so the walk ends at the first x that is its own parent
__device__ __forceinline__ uint32_t cl_root(const uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = cl_load(parent + x);
    if (p == x) return x;
    x = p;
  }
}

// status[0] = live slots, status[1] = 1 once an id is held twice
__global__ __launch_bounds__(256) void k_cl_slots(const uint64_t* __restrict__ hashes, const uint32_t* __restrict__ ids,
                                                  uint32_t n_slots, unsigned long long* __restrict__ keys,
                                                  uint32_t* __restrict__ vals, uint32_t* __restrict__ status) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  bool live = false;
  if (g < n_slots) {
    const uint32_t id = ids[g];
    live = id != 0 && hashes[g] != 0;
    keys[g] = live ? (unsigned long long)id : 1ull << 32;
    vals[g] = g;
  }
  const unsigned long long m = __ballot(live);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(status, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(256) void k_cl_table(const unsigned long long* __restrict__ keys,
                                                  const uint32_t* __restrict__ vals, const uint64_t* __restrict__ hashes,
                                                  uint32_t n_slots, uint32_t* __restrict__ t_id,
                                                  uint64_t* __restrict__ t_hash, uint32_t* __restrict__ status) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= n_slots) return;
  const unsigned long long key = keys[g];
  if (key >> 32) return;  // not live: sorted behind every node
  if (g > 0 && keys[g - 1] == key) atomicOr(status + 1, 1u);
  t_id[g] = (uint32_t)key;
  t_hash[g] = hashes[vals[g]];
}

__global__ __launch_bounds__(256) void k_cl_init(uint32_t* __restrict__ parent, uint32_t* __restrict__ nearest,
                                                 uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  parent[i] = i;
  nearest[i] = kNoNeighbour;
}

__global__ __launch_bounds__(256) void k_cl_hook(const cbh_record* __restrict__ rec, unsigned long long total,
                                                 uint32_t base, const uint32_t* __restrict__ t_id,
                                                 const uint64_t* __restrict__ t_hash, uint32_t n, uint32_t* parent,
                                                 uint32_t* nearest) {
  const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const cbh_record r = rec[t];
  const uint32_t i = base + CBH_REC_QUERY(r), id = CBH_REC_ID(r), d = (uint32_t)CBH_REC_DIST(r);
  if (i >= n) return;
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (t_id[mid] < id)
      lo = mid + 1;
    else
      hi = mid;
  }
  const uint32_t j = lo;
  if (j >= n || t_id[j] != id || j == i) return;
  // (a slot whose hash is 0 keeps its id and can still match a needle; it is no node, and its distance is not the node's)
  if ((uint32_t)__popcll(t_hash[i] ^ t_hash[j]) != d) return;
  if (cl_load(nearest + i) > d) atomicMin(nearest + i, d);
  if (j > i) return;  // the same edge comes again with j as the needle
  uint32_t a = i, b = j;
  for (;;) {
    a = cl_root(parent, a);
    b = cl_root(parent, b);
    if (a == b) break;
    const uint32_t big = max(a, b), small = min(a, b);
    const uint32_t old = atomicMin(parent + big, small);
    if (old == big) break;  // big was a root and now hangs under small
    a = old, b = small;     // someone hooked big first: old < big still has to meet small
  }
}

__global__ __launch_bounds__(256) void k_cl_flatten(uint32_t* parent, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  __hip_atomic_store(parent + i, cl_root(parent, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_cl_labels(const uint32_t* __restrict__ t_id, const uint32_t* __restrict__ parent,
                                                   const uint32_t* __restrict__ nearest, uint32_t n,
                                                   uint32_t* __restrict__ ids, uint32_t* __restrict__ label,
                                                   uint8_t* __restrict__ near8) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  ids[i] = t_id[i];
  label[i] = t_id[parent[i]];
  near8[i] = (uint8_t)nearest[i];
}

__global__ __launch_bounds__(256) void k_cl_sizes(const uint32_t* __restrict__ parent, uint32_t n,
                                                  uint32_t* __restrict__ size) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  bool todo = i < n;
  const uint32_t root = todo ? parent[i] : 0u;
  // the lanes of a wave that share a root add once: a large component is ONE address, and a million single adds to it
  // took as long as the scan (11.5 ns each).  At most 64 rounds, one per distinct root in the wave; the ballots are
  // wave-uniform, so every lane leaves the loop in the same round
  for (;;) {
    const unsigned long long left = __ballot(todo);
    if (!left) break;
    const uint32_t leader = (uint32_t)__ffsll(left) - 1u;
    const uint32_t r = (uint32_t)__shfl((int)root, (int)leader);
    const bool mine = todo && root == r;
    const unsigned long long same = __ballot(mine);
    if (lane == leader) atomicAdd(size + r, (uint32_t)__popcll(same));
    if (mine) todo = false;
  }
}

// what node i adds to the scan: (1 cluster, size members) for the root of a kept component
__device__ __forceinline__ unsigned long long cl_weight(const uint32_t* __restrict__ parent,
                                                        const uint32_t* __restrict__ size, uint32_t i, uint32_t n,
                                                        uint32_t min_members) {
  if (i >= n || parent[i] != i) return 0ull;
  const uint32_t sz = size[i];
  return sz >= min_members ? (1ull << 32 | sz) : 0ull;
}

// exclusive sum over the 256 threads of a workgroup; *total = the sum of all
__device__ __forceinline__ unsigned long long cl_block_excl(unsigned long long v, unsigned long long* sh,
                                                            unsigned long long* total) {
  const uint32_t t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const unsigned long long add = t >= d ? sh[t - d] : 0ull;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  *total = sh[255];
  const unsigned long long incl = sh[t];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(256) void k_cl_tile_sums(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ size,
                                                      uint32_t n, uint32_t min_members,
                                                      unsigned long long* __restrict__ tile_sum) {
  __shared__ unsigned long long sh[256];
  const uint32_t first = blockIdx.x * kTile + threadIdx.x * 4;
  unsigned long long v = 0, total;
  for (uint32_t k = 0; k < 4; ++k) v += cl_weight(parent, size, first + k, n, min_members);
  (void)cl_block_excl(v, sh, &total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one workgroup: tile_sum[t] becomes the sum of the tiles before t, tile_sum[n_tiles] the sum of all
__global__ __launch_bounds__(256) void k_cl_tile_offsets(unsigned long long* tile_sum, uint32_t n_tiles) {
  __shared__ unsigned long long sh[256];
  unsigned long long carry = 0;
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += 256) {
    const uint32_t t = t0 + threadIdx.x;
    const unsigned long long v = t < n_tiles ? tile_sum[t] : 0ull;
    unsigned long long total;
    const unsigned long long ex = cl_block_excl(v, sh, &total);
    if (t < n_tiles) tile_sum[t] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) tile_sum[n_tiles] = carry;
}

__global__ __launch_bounds__(256) void k_cl_emit(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ size,
                                                 uint32_t n, uint32_t min_members,
                                                 const unsigned long long* __restrict__ tile_off,
                                                 uint64_t* __restrict__ out_first, unsigned long long* __restrict__ keys) {
  __shared__ unsigned long long sh[256];
  const uint32_t first = blockIdx.x * kTile + threadIdx.x * 4;
  unsigned long long w[4], v = 0, total;
  for (uint32_t k = 0; k < 4; ++k) v += w[k] = cl_weight(parent, size, first + k, n, min_members);
  unsigned long long ex = cl_block_excl(v, sh, &total) + tile_off[blockIdx.x];
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t i = first + k;
    if (i >= n) break;
    if (w[k]) out_first[ex >> 32] = ex & 0xffffffffull;
    ex += w[k];
    const uint32_t root = parent[i];
    // a node outside every cluster sorts behind all of them: label n is nobody's
    keys[i] = (unsigned long long)(size[root] >= min_members ? root : n) << 32 | i;
  }
}

__global__ __launch_bounds__(256) void k_cl_members(const unsigned long long* __restrict__ keys, uint32_t members,
                                                    const uint32_t* __restrict__ t_id, const uint32_t* __restrict__ nearest,
                                                    cbh_match* __restrict__ out) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= members) return;
  const uint32_t node = (uint32_t)keys[p];
  out[p] = cbh_match{t_id[node], (int32_t)nearest[node]};
}

inline unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

// event pairs of a call that times its stages ("cluster_timing"); every method is a no-op without it
struct StageClock {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double us[3] = {0, 0, 0};
  bool on = false;
  int init() {
    if (!g_cluster_timing.load()) return CBH_OK;
    CBH_HIP(hipEventCreate(&e0));
    CBH_HIP(hipEventCreate(&e1));
    on = true;
    return CBH_OK;
  }
  int start(hipStream_t s) {
    if (on) CBH_HIP(hipEventRecord(e0, s));
    return CBH_OK;
  }
  int stop(int stage, hipStream_t s) {
    if (!on) return CBH_OK;
    CBH_HIP(hipEventRecord(e1, s));
    CBH_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    CBH_HIP(hipEventElapsedTime(&ms, e0, e1));
    us[stage] += (double)ms * 1000.0;
    return CBH_OK;
  }
  void publish() const {
    for (int k = 0; k < 3; ++k) g_cluster_us[k].store(on ? (long long)(us[k] + 0.5) : 0);
  }
  ~StageClock() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

// the device state of one call: the node table and the forest, in blocks of the call's scratch
struct Forest {
  uint32_t n = 0;  // nodes
  uint32_t *t_id = nullptr, *parent = nullptr, *nearest = nullptr;
  uint64_t* t_hash = nullptr;
};

// the live (id, hash) pairs of the handle in ascending id order.  Synchronises `s`.
int build_table(cbh_idx64* idx, Scratch& keep, Forest* F, hipStream_t s) {
  const size_t n_slots = idx->n;
  F->n = 0;
  if (n_slots == 0) return CBH_OK;
  if (n_slots > 0xfffffff0ull) return cl_fail(CBH_E_UNSUPPORTED, "clusters: more than 2^32 slots");
  Scratch scratch(s);  // what only the build needs
  const uint64_t* d_hashes = idx->d_hashes;
  const uint32_t* d_ids = idx->d_ids;
  if (idx->shards) {
    uint64_t* gh;
    uint32_t* gi;
    CBH_HIP(scratch.get(&gh, n_slots * 8));
    CBH_HIP(scratch.get(&gi, n_slots * 4));
    if (int rc = sharded_gather_dev(idx, gh, gi, s)) return rc;
    d_hashes = gh, d_ids = gi;
  }
  unsigned long long* keys;
  uint32_t *vals, *status;
  CBH_HIP(scratch.get(&keys, n_slots * 8));
  CBH_HIP(scratch.get(&vals, n_slots * 4));
  CBH_HIP(scratch.get(&status, 8));
  CBH_HIP(keep.get(&F->t_id, n_slots * 4));
  CBH_HIP(keep.get(&F->t_hash, n_slots * 8));
  CBH_HIP(hipMemsetAsync(status, 0, 8, s));
  hipLaunchKernelGGL(k_cl_slots, dim3(blocks_of(n_slots)), dim3(256), 0, s, d_hashes, d_ids, (uint32_t)n_slots, keys, vals,
                     status);
  CBH_HIP(hipGetLastError());
  if (int rc = sort_pairs_u64_u32(keys, vals, n_slots, 33, s)) return rc;
  hipLaunchKernelGGL(k_cl_table, dim3(blocks_of(n_slots)), dim3(256), 0, s, keys, vals, d_hashes, (uint32_t)n_slots,
                     F->t_id, F->t_hash, status);
  CBH_HIP(hipGetLastError());
  uint32_t h_status[2] = {0, 0};
  CBH_HIP(hipMemcpyAsync(h_status, status, 8, hipMemcpyDeviceToHost, s));
  CBH_HIP(hipStreamSynchronize(s));
  if (h_status[1])
    return cl_fail(CBH_E_UNSUPPORTED, "clusters: two live entries hold the same id (not a DctHashIndex)");
  F->n = h_status[0];
  return CBH_OK;
}

// table, scans, unions: leaves F with parent[i] = the smallest node of i's component
int cluster_core(cbh_idx64* idx, Workspace* ws, int thresh, Scratch& keep, Forest* F, cbh_cluster_stats* st,
                 StageClock* clock, hipStream_t s) {
  int rc = clock->start(s);
  if (rc || (rc = build_table(idx, keep, F, s)) || (rc = clock->stop(0, s))) return rc;
  const uint32_t n = F->n;
  st->nodes = n;
  if (n == 0) return CBH_OK;
  CBH_HIP(keep.get(&F->parent, (size_t)n * 4));
  CBH_HIP(keep.get(&F->nearest, (size_t)n * 4));
  hipLaunchKernelGGL(k_cl_init, dim3(blocks_of(n)), dim3(256), 0, s, F->parent, F->nearest, n);
  CBH_HIP(hipGetLastError());
  if (thresh <= 0) return CBH_OK;  // no pair is closer than 0
  const uint32_t chunk = (uint32_t)g_cluster_chunk.load();
  const size_t max_records = (size_t)g_cluster_max_records.load();
  struct Range {
    uint32_t base, len;
  };
  std::vector<Range> todo;  // a stack, first range on top
  for (uint32_t base = (n - 1) / chunk * chunk;; base -= chunk) {
    todo.push_back(Range{base, std::min(chunk, n - base)});
    if (base == 0) break;
  }
  while (!todo.empty()) {
    const Range r = todo.back();
    todo.pop_back();
    unsigned long long total = 0;
    rc = scan_all(idx, ws, F->t_hash + r.base, r.len, thresh, s, &total, ScanOpts{}, max_records);
    // (scan_all lets a result through that fits the block the workspace already has: the limit holds whatever an earlier
    // call left there, so that chunks and rescans depend on the contents and the knobs alone)
    if (rc == CBH_OK && total > max_records) rc = CBH_E_OVERFLOW;
    if (rc == CBH_E_OVERFLOW) {
      if (r.len == 1) return cl_fail(CBH_E_OVERFLOW, "clusters: one entry has more matches than \"cluster_max_records\"");
      const uint32_t half = r.len / 2;
      todo.push_back(Range{r.base + half, r.len - half});
      todo.push_back(Range{r.base, half});
      st->rescans++;
      continue;
    }
    if (rc) return rc;
    st->chunks++;
    st->records += total;
    if ((rc = clock->start(s))) return rc;
    if (total) {
      hipLaunchKernelGGL(k_cl_hook, dim3(blocks_of((size_t)total)), dim3(256), 0, s, ws->d_rec, total, r.base, F->t_id,
                         F->t_hash, n, F->parent, F->nearest);
      CBH_HIP(hipGetLastError());
      hipLaunchKernelGGL(k_cl_flatten, dim3(blocks_of(n)), dim3(256), 0, s, F->parent, n);
      CBH_HIP(hipGetLastError());
    }
    if ((rc = clock->stop(1, s))) return rc;
  }
  return CBH_OK;
}

int args_ok(const cbh_idx64* idx, int thresh) {
  if (!idx) return cl_fail(CBH_E_INVAL, "clusters: the handle is NULL");
  if (thresh < 0 || thresh > 65) return cl_fail(CBH_E_INVAL, "clusters: thresh outside 0..65");
  return CBH_OK;
}

// the workspace goes back to its pool idle, and without the record block of a clique
int settle(Workspace* ws, cbh_idx64* idx, hipStream_t s, int rc) {
  const hipError_t e = hipStreamSynchronize(s);
  ws->shrink_records(std::max<size_t>(idx->rec_cap_default, (size_t)1 << 22));
  if (rc == CBH_OK && e != hipSuccess) rc = fail("hipStreamSynchronize(clusters)", e);
  return rc;
}

// labels into device arrays of `cap` entries on the handle's device
int labels_dev(cbh_idx64* idx, Workspace* ws, int thresh, uint32_t* d_ids, uint32_t* d_label, uint8_t* d_nearest, size_t cap,
               size_t* n_out, cbh_cluster_stats* stats, hipStream_t s) {
  cbh_cluster_stats st = {};
  StageClock clock;
  Scratch keep(s);
  Forest F;
  int rc = clock.init();
  if (rc || (rc = cluster_core(idx, ws, thresh, keep, &F, &st, &clock, s))) return rc;
  *n_out = F.n;
  const uint32_t m = (uint32_t)std::min<size_t>(F.n, cap);
  if (m) {
    if ((rc = clock.start(s))) return rc;
    if (m == F.n) {
      hipLaunchKernelGGL(k_cl_labels, dim3(blocks_of(m)), dim3(256), 0, s, F.t_id, F.parent, F.nearest, m, d_ids, d_label,
                         d_nearest);
      CBH_HIP(hipGetLastError());
    } else {  // a caller asking for the count, or for the first few: the kernel writes whole arrays, so copy
      uint32_t *a, *b;
      uint8_t* c;
      CBH_HIP(keep.get(&a, (size_t)F.n * 4));
      CBH_HIP(keep.get(&b, (size_t)F.n * 4));
      CBH_HIP(keep.get(&c, (size_t)F.n));
      hipLaunchKernelGGL(k_cl_labels, dim3(blocks_of(F.n)), dim3(256), 0, s, F.t_id, F.parent, F.nearest, F.n, a, b, c);
      CBH_HIP(hipGetLastError());
      CBH_HIP(hipMemcpyAsync(d_ids, a, (size_t)m * 4, hipMemcpyDeviceToDevice, s));
      CBH_HIP(hipMemcpyAsync(d_label, b, (size_t)m * 4, hipMemcpyDeviceToDevice, s));
      CBH_HIP(hipMemcpyAsync(d_nearest, c, (size_t)m, hipMemcpyDeviceToDevice, s));
    }
    if ((rc = clock.stop(2, s))) return rc;
  }
  if (stats) *stats = st;
  clock.publish();
  return CBH_OK;
}

}  // namespace

int set_cluster_chunk(int v) {
  if (v < 1 || (unsigned)v > CBH_MAX_QUERIES_PER_CALL) return CBH_E_INVAL;
  g_cluster_chunk.store(v);
  return CBH_OK;
}
int get_cluster_chunk() { return g_cluster_chunk.load(); }
int set_cluster_max_records(int v) {
  if (v < 1) return CBH_E_INVAL;
  g_cluster_max_records.store(v);
  return CBH_OK;
}
int get_cluster_max_records() { return g_cluster_max_records.load(); }
void set_cluster_timing(int on) { g_cluster_timing.store(on != 0); }
long long get_cluster_stat(int which) { return g_cluster_us[which].load(); }

}  // namespace cbh

extern "C" {

int cbh_idx64_cluster_labels_dev(cbh_idx64* idx, int thresh, void* d_ids, void* d_label, void* d_nearest, size_t cap,
                                 size_t* n_out, cbh_cluster_stats* stats, void* stream) {
  using namespace cbh;
  clear_last_error();
  int rc = args_ok(idx, thresh);
  if (rc) return rc;
  if (!n_out || (cap && (!d_ids || !d_label || !d_nearest))) return cl_fail(CBH_E_INVAL, "clusters: a required pointer is NULL");
  *n_out = 0;
  DeviceGuard g(idx->device);
  if (!g.ok) return CBH_E_NODEVICE;
  WsLease L(idx, &rc);
  if (!L.ws) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : L.ws->stream;
  rc = labels_dev(idx, L.ws, thresh, (uint32_t*)d_ids, (uint32_t*)d_label, (uint8_t*)d_nearest, cap, n_out, stats, s);
  return settle(L.ws, idx, s, rc);
}

int cbh_idx64_cluster_labels(cbh_idx64* idx, int thresh, uint32_t* ids, uint32_t* label, uint8_t* nearest, size_t cap,
                             size_t* n_out, cbh_cluster_stats* stats) {
  using namespace cbh;
  clear_last_error();
  int rc = args_ok(idx, thresh);
  if (rc) return rc;
  if (!n_out || (cap && (!ids || !label || !nearest))) return cl_fail(CBH_E_INVAL, "clusters: a required pointer is NULL");
  *n_out = 0;
  DeviceGuard g(idx->device);
  if (!g.ok) return CBH_E_NODEVICE;
  WsLease L(idx, &rc);
  if (!L.ws) return rc;
  hipStream_t s = L.ws->stream;
  auto run = [&]() -> int {
    Scratch out(s);
    const size_t m = std::min(cap, idx->n);  // never more nodes than slots
    uint32_t *d_ids = nullptr, *d_label = nullptr;
    uint8_t* d_near = nullptr;
    if (m) {
      CBH_HIP(out.get(&d_ids, m * 4));
      CBH_HIP(out.get(&d_label, m * 4));
      CBH_HIP(out.get(&d_near, m));
    }
    int r = labels_dev(idx, L.ws, thresh, d_ids, d_label, d_near, m, n_out, stats, s);
    if (r) return r;
    const size_t w = std::min(m, *n_out);
    if (w) {
      CBH_HIP(hipMemcpyAsync(ids, d_ids, w * 4, hipMemcpyDeviceToHost, s));
      CBH_HIP(hipMemcpyAsync(label, d_label, w * 4, hipMemcpyDeviceToHost, s));
      CBH_HIP(hipMemcpyAsync(nearest, d_near, w, hipMemcpyDeviceToHost, s));
      CBH_HIP(hipStreamSynchronize(s));  // (the scratch goes back behind the copies)
    }
    return CBH_OK;
  };
  return settle(L.ws, idx, s, run());
}

int cbh_idx64_clusters(cbh_idx64* idx, int thresh, int min_members, uint64_t* out_first, size_t cap_clusters,
                       cbh_match* out_members, size_t cap_members, size_t* n_clusters, size_t* n_members,
                       cbh_cluster_stats* stats) {
  using namespace cbh;
  clear_last_error();
  int rc = args_ok(idx, thresh);
  if (rc) return rc;
  if (min_members < 2) return cl_fail(CBH_E_INVAL, "clusters: min_members below 2");
  if (!n_clusters || !n_members || !out_first || (cap_members && !out_members))
    return cl_fail(CBH_E_INVAL, "clusters: a required pointer is NULL");
  *n_clusters = *n_members = 0;
  DeviceGuard g(idx->device);
  if (!g.ok) return CBH_E_NODEVICE;
  WsLease L(idx, &rc);
  if (!L.ws) return rc;
  hipStream_t s = L.ws->stream;
  auto run = [&]() -> int {
    cbh_cluster_stats st = {};
    StageClock clock;
    Scratch keep(s);
    Forest F;
    int r = clock.init();
    if (r || (r = cluster_core(idx, L.ws, thresh, keep, &F, &st, &clock, s))) return r;
    const uint32_t n = F.n;
    unsigned long long sums = 0;  // clusters << 32 | members
    uint64_t* d_first = nullptr;
    cbh_match* d_members = nullptr;
    if (n >= 2 && thresh > 0) {
      if ((r = clock.start(s))) return r;
      const uint32_t tiles = (n + kTile - 1) / kTile;
      uint32_t* size;
      unsigned long long *tile_sum, *keys;
      CBH_HIP(keep.get(&size, (size_t)n * 4));
      CBH_HIP(keep.get(&tile_sum, ((size_t)tiles + 1) * 8));
      CBH_HIP(keep.get(&keys, (size_t)n * 8));
      CBH_HIP(keep.get(&d_first, ((size_t)n / 2 + 2) * 8));
      CBH_HIP(keep.get(&d_members, (size_t)n * sizeof(cbh_match)));
      CBH_HIP(hipMemsetAsync(size, 0, (size_t)n * 4, s));
      hipLaunchKernelGGL(k_cl_sizes, dim3(blocks_of(n)), dim3(256), 0, s, F.parent, n, size);
      CBH_HIP(hipGetLastError());
      hipLaunchKernelGGL(k_cl_tile_sums, dim3(tiles), dim3(256), 0, s, F.parent, size, n, (uint32_t)min_members, tile_sum);
      CBH_HIP(hipGetLastError());
      hipLaunchKernelGGL(k_cl_tile_offsets, dim3(1), dim3(256), 0, s, tile_sum, tiles);
      CBH_HIP(hipGetLastError());
      hipLaunchKernelGGL(k_cl_emit, dim3(tiles), dim3(256), 0, s, F.parent, size, n, (uint32_t)min_members, tile_sum, d_first,
                         keys);
      CBH_HIP(hipGetLastError());
      int bits = 1;
      while (bits < 32 && ((uint64_t)1 << bits) <= n) ++bits;  // labels 0..n
      if ((r = sort_keys_u64(keys, n, 32 + bits, s))) return r;
      CBH_HIP(hipMemcpyAsync(&sums, tile_sum + tiles, 8, hipMemcpyDeviceToHost, s));
      CBH_HIP(hipStreamSynchronize(s));
      const uint32_t members = (uint32_t)sums;
      if (members) {
        hipLaunchKernelGGL(k_cl_members, dim3(blocks_of(members)), dim3(256), 0, s, keys, members, F.t_id, F.nearest,
                           d_members);
        CBH_HIP(hipGetLastError());
      }
      if ((r = clock.stop(2, s))) return r;
    }
    const size_t clusters = (size_t)(sums >> 32), members = (size_t)(sums & 0xffffffffull);
    st.clusters = clusters, st.members = members;
    *n_clusters = clusters, *n_members = members;
    if (stats) *stats = st;
    clock.publish();
    if (clusters > cap_clusters || members > cap_members) return CBH_E_OVERFLOW;
    if (clusters) CBH_HIP(hipMemcpyAsync(out_first, d_first, clusters * 8, hipMemcpyDeviceToHost, s));
    if (members) CBH_HIP(hipMemcpyAsync(out_members, d_members, members * sizeof(cbh_match), hipMemcpyDeviceToHost, s));
    CBH_HIP(hipStreamSynchronize(s));
    out_first[clusters] = members;  // (out_first has cap_clusters + 1 entries)
    return CBH_OK;
  };
  return settle(L.ws, idx, s, run());
}

}  // extern "C"
