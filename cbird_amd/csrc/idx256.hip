// idx256.hip -- CvFeaturesIndex (src/cvfeaturesindex.{h,cpp}): 256-bit ORB/BRIEF descriptors, k nearest
// neighbours in Hamming space, brute force on gfx950.
//
// Reference: all descriptors live in one N x 32-byte matrix (cvfeaturesindex.h:73); find() asks a FLANN LSH
// index for the 10 nearest rows of every needle descriptor (cvfeaturesindex.cpp:497), keeps distance <
// cvThresh (:508), maps row -> mediaId through the first-row map (:511-516, removed media have id 0 and are
// skipped AFTER the knn cut, :518), and scores each media by median distance * 1000 / votes (:564-596).
// LSH is approximate; this is the exact search it approximates (results are a superset).
//
// Since the k nearest are only ever used below a threshold, the search is a threshold scan (launch_hamm256_scan,
// hamm256_scan.hip: the popcount kernel or the matrix cores).  Records q<<41 | dist<<32 | row are then ordered and cut
// at k per needle descriptor.
//
//   rows   Rows256: rows on one device and what a scan of them needs.  A plain handle has one; a sharded handle one per
//          shard, and its own holds no rows but receives the shards' records.
//   call   Call256 owns one search: the handle's device and mutex, and a Run256 per Rows256 it puts work on.
//   scan   rounds over the runs that have to scan (launch_round, collect_round), the same for both handle kinds;
//          gather_shards is the sharded-only finish.
//   cut    sorted_records leaves the ordered records in the handle's own block; knn256 cuts them at k, radius256 downloads them.

#include <map>
#include <optional>

#include "cbh_index.h"

namespace {

// first k records of every needle descriptor from the sorted list: (row, dist)
__global__ __launch_bounds__(256) void k_select256(const unsigned long long* __restrict__ rec, size_t n,
                                                   uint32_t nq, int k, uint32_t* __restrict__ out_row,
                                                   uint16_t* __restrict__ out_dist,
                                                   uint32_t* __restrict__ counts) {
  const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
  if (qi >= nq) return;
  auto lower = [&](unsigned long long key) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
      size_t mid = (lo + hi) >> 1;
      if (rec[mid] < key)
        lo = mid + 1;
      else
        hi = mid;
    }
    return lo;
  };
  const size_t a = lower((unsigned long long)qi << 41);
  const size_t b = lower(((unsigned long long)qi + 1) << 41);
  const size_t cnt = b - a;
  counts[qi] = cnt > 0xffffffffull ? 0xffffffffu : (uint32_t)cnt;
  for (int j = 0; j < k; ++j) {  // places past the count are zeroed (the buffers are reused between calls)
    const unsigned long long r = (size_t)j < cnt ? rec[a + (size_t)j] : 0ull;
    out_row[(size_t)qi * k + j] = (uint32_t)r;
    out_dist[(size_t)qi * k + j] = (uint16_t)((r >> 32) & 0x1ff);
  }
}

int sig_bits256(size_t nq) {
  int b = 0;
  while (b < 23 && ((size_t)1 << b) < nq) ++b;
  return 41 + b;
}

// a grow-only device array of `need` elements of `each` bytes (what it held is not kept)
template <class T>
int regrow(T** p, size_t* cap, size_t need, size_t each) {
  if (need <= *cap) return CBH_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  CBH_HIP(hipMalloc(p, need * each));
  *cap = need;
  return CBH_OK;
}

// rows on one device and what a scan of them needs (every function: on `device`, the caller has made it current)
struct Rows256 {
  int device = 0;
  uint8_t* d_rows = nullptr;  // n x 32 B
  size_t n = 0, cap = 0;
  hipStream_t stream = nullptr;
  uint8_t* d_q = nullptr;  // the needles of a call
  size_t q_cap = 0;
  unsigned long long* d_rec = nullptr;
  size_t rec_cap = 0;
  unsigned long long *d_total = nullptr, *h_total = nullptr;  // h_total: pinned
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  cbh::XBuf x[2];  // exchange buffers of a shard (cbh_shard.h)

  int ensure_scan(size_t nq, size_t rec_need) {
    if (!stream) {
      CBH_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
      CBH_HIP(hipMalloc(&d_total, 8));
      CBH_HIP(hipHostMalloc(&h_total, 8));
      CBH_HIP(hipEventCreate(&ev0));
      CBH_HIP(hipEventCreate(&ev1));
    }
    const int rc = regrow(&d_rec, &rec_cap, rec_need, 8);
    return rc ? rc : regrow(&d_q, &q_cap, nq, 32);
  }
  int append(const uint8_t* rows, size_t n_rows) {
    if (n + n_rows > cap) {
      size_t ncap = std::max<size_t>(n + n_rows, cap + cap / 2 + 65536);
      uint8_t* nr = nullptr;
      CBH_HIP(hipMalloc(&nr, ncap * 32));
      if (n) CBH_HIP(hipMemcpy(nr, d_rows, n * 32, hipMemcpyDeviceToDevice));
      if (d_rows) (void)hipFree(d_rows);
      d_rows = nr;
      cap = ncap;
    }
    CBH_HIP(hipMemcpy(d_rows + n * 32, rows, n_rows * 32, hipMemcpyHostToDevice));
    n += n_rows;
    return CBH_OK;
  }
  void release() {
    for (cbh::XBuf& b : x) b.release();
    for (void* p : {(void*)d_rows, (void*)d_rec, (void*)d_total, (void*)d_q})
      if (p) (void)hipFree(p);
    if (h_total) (void)hipHostFree(h_total);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) cbh::stream_destroy(stream);
  }
};

}  // namespace

struct Shards256;  // below: the shards of a CvFeaturesIndex that spans several shards / devices
struct cbh_idx256 {
  bool loaded = false;
  Shards256* shards = nullptr;  // cbh_idx256_create_sharded: this handle keeps the maps, the shards the rows
  Rows256 own;                  // a plain handle: the rows.  A sharded one: no rows, the block that receives the shards' records
  size_t n = 0;                 // rows in all (a plain handle: own.n)
  // _indexMap (cvfeaturesindex.h:77): first row -> mediaId (0 = removed), ascending; sentinel (n, 0)
  std::vector<uint32_t> first_row{0};
  std::vector<uint32_t> media_id{0};
  std::map<uint32_t, uint32_t> id_to_first;  // _idMap
  std::mutex mu;                             // one search at a time per index
  // sort and cut scratch beside own.d_rec
  unsigned long long* d_alt = nullptr;
  void* d_tmp = nullptr;
  size_t alt_cap = 0, tmp_bytes = 0;
  uint32_t *d_out_row = nullptr, *d_counts = nullptr;  // k_select256's outputs
  uint16_t* d_out_dist = nullptr;
  size_t row_cap = 0, dist_cap = 0, counts_cap = 0;
  double scan_ms = 0;
  uint64_t scan_pairs = 0, scan_launches = 0;

  uint32_t media_of_row(uint32_t row) const {  // upper_bound(index) - 1 (:514-516)
    auto it = std::upper_bound(first_row.begin(), first_row.end(), row);
    if (it == first_row.begin()) return 0;
    return media_id[(size_t)(it - first_row.begin()) - 1];
  }
  // the ping-pong buffer and radix scratch for own.rec_cap records; nq x k places for the cut (a radius search: none)
  int ensure_cut(size_t nq, int k) {
    const size_t places = nq * (size_t)k;
    int rc = CBH_OK;
    if (alt_cap < own.rec_cap) {  // (the two grow together)
      tmp_bytes = 0;
      rc = regrow(&d_tmp, &tmp_bytes, std::max<size_t>(cbh::sort_records_scratch_bytes(own.rec_cap), 16), 1);
      if (!rc) rc = regrow(&d_alt, &alt_cap, own.rec_cap, 8);
    }
    if (!rc) rc = regrow(&d_out_row, &row_cap, places, 4);
    if (!rc) rc = regrow(&d_out_dist, &dist_cap, places, 2);
    return rc ? rc : regrow(&d_counts, &counts_cap, nq, 4);
  }
};

// ---- one CvFeaturesIndex over several shards / GPUs (cbh_idx256_create_sharded) ------------------------------------
// Sharded BY IMAGE: a media's descriptor rows stay together on one shard; the handle keeps the
// first-row -> mediaId maps in GLOBAL row numbers exactly as the one-device index does, the shards hold rows only.
// Rows arrive media by media (add), so a shard takes media until it has received kShardRun rows, then the emptiest
// shard takes over: the global row order is the add order, a shard's rows are runs of it (a segment table per shard).
// A search scans every shard on its own device and stream, rewrites the LOCAL row of every record to the global one
// (k_rows_to_global: the tie-break of the knn is (distance, global row), and the maps are global), brings the records
// to the handle's own block with ShardComm::exchange (cbh_shard.h: copies inside a device, ncclAllGather between devices)
// and sorts / cuts / scores there as the one-device index does.
struct Shards256 {
  cbh::ShardComm comm;
  std::vector<Rows256> shard;
  struct Seg {
    uint32_t shard;
    size_t local, global, len;
  };
  std::vector<Seg> segs;  // in global order
  size_t cur = 0, cur_run = 0;
  static constexpr size_t kShardRun = 16384;
  // per shard: the segment table on its device (local start ascending, global - local), rebuilt when rows were added
  std::vector<uint32_t*> d_seg_local;
  std::vector<long long*> d_seg_delta;
  std::vector<uint32_t> n_seg;
  bool dirty = true;

  // the shard the next media goes to: the current one until it has had its run, then the emptiest
  size_t next_shard() {
    if (cur_run >= kShardRun) {
      size_t best = 0;
      for (size_t s = 1; s < shard.size(); ++s)
        if (shard[s].n < shard[best].n) best = s;
      cur = best;
      cur_run = 0;
    }
    return cur;
  }
  // n_rows rows went to shard `cur` at its row `local`, as global rows from `global`
  void note_rows(size_t local, size_t global, size_t n_rows) {
    if (!segs.empty() && segs.back().shard == cur && segs.back().local + segs.back().len == local &&
        segs.back().global + segs.back().len == global)
      segs.back().len += n_rows;
    else
      segs.push_back(Seg{(uint32_t)cur, local, global, n_rows});
    cur_run += n_rows;
    dirty = true;
  }
};

namespace {

__global__ __launch_bounds__(256) void k_rows_to_global(unsigned long long* __restrict__ rec, unsigned long long n,
                                                        const uint32_t* __restrict__ seg_local,
                                                        const long long* __restrict__ seg_delta, uint32_t nseg) {
  const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
  if (i >= n) return;
  const unsigned long long r = rec[i];
  const uint32_t row = (uint32_t)r;
  uint32_t lo = 0, hi = nseg;  // last segment whose local start is <= row
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (seg_local[mid] <= row)
      lo = mid;
    else
      hi = mid;
  }
  rec[i] = (r & 0xffffffff00000000ull) | (uint32_t)((long long)row + seg_delta[lo]);
}

// a block for a counted result and, beside the handle's own block, its sort scratch (no memory for it: the result does
// not fit, CBH_E_OVERFLOW)
int grow_for_result(cbh_idx256* ix, Rows256* r, unsigned long long records) {
  int rc = r->ensure_scan(0, (size_t)records + 1024);
  if (!rc && r == &ix->own) rc = ix->ensure_cut(0, 0);
  return rc == CBH_E_NOMEM ? CBH_E_OVERFLOW : rc;
}

int upload_segments(Shards256* S) {
  if (!S->dirty) return CBH_OK;
  for (size_t s = 0; s < S->shard.size(); ++s) {
    std::vector<uint32_t> loc;
    std::vector<long long> delta;
    for (const Shards256::Seg& g : S->segs)
      if (g.shard == s) {  // (global order is also local order inside a shard)
        loc.push_back((uint32_t)g.local);
        delta.push_back((long long)g.global - (long long)g.local);
      }
    cbh::DeviceGuard dg(S->shard[s].device);
    if (!dg.ok) return CBH_E_NODEVICE;
    if (S->d_seg_local[s]) (void)hipFree(S->d_seg_local[s]);
    if (S->d_seg_delta[s]) (void)hipFree(S->d_seg_delta[s]);
    S->d_seg_local[s] = nullptr, S->d_seg_delta[s] = nullptr;
    S->n_seg[s] = (uint32_t)loc.size();
    if (loc.empty()) continue;
    CBH_HIP(hipMalloc(&S->d_seg_local[s], loc.size() * 4));
    CBH_HIP(hipMalloc(&S->d_seg_delta[s], loc.size() * 8));
    CBH_HIP(hipMemcpy(S->d_seg_local[s], loc.data(), loc.size() * 4, hipMemcpyHostToDevice));
    CBH_HIP(hipMemcpy(S->d_seg_delta[s], delta.data(), delta.size() * 8, hipMemcpyHostToDevice));
  }
  S->dirty = false;
  return CBH_OK;
}

// One Rows256 for the length of one call.  `drained`: nothing this call put on its stream can still be running.  Two
// operations touch it: work(), through which every enqueue goes, clears it; saw_drained(), where the host saw that, sets it.
struct Run256 {
  Rows256* r = nullptr;
  bool todo = false;             // has to scan in the next round
  unsigned long long count = 0;  // records its last scan counted
  bool drained = true;           // (the index's streams are idle when its mutex is taken)
  hipStream_t work() { return drained = false, r->stream; }
  void saw_drained() { drained = true; }
};

// What one search holds: the handle's device and mutex, and the runs.  run[0 .. n_scan) scan: the shards, or a plain
// handle's own rows; root() is the handle's own block, where the records end up (a plain handle: the same run).
struct Call256 {
  cbh_idx256* ix;
  Shards256* S;
  const uint8_t* needles;  // host memory
  size_t nq;
  int thresh;
  cbh::DeviceGuard g;
  std::lock_guard<std::mutex> lk;
  std::vector<Run256> run;
  size_t n_scan;
  Call256(cbh_idx256* i, const uint8_t* q, size_t nq_, int t)
      : ix(i), S(i->shards), needles(q), nq(nq_), thresh(t), g(i->own.device), lk(i->mu),
        run(S ? S->shard.size() + 1 : 1), n_scan(S ? S->shard.size() : 1) {
    for (size_t s = 0; S && s < n_scan; ++s) run[s].r = &S->shard[s];
    run.back().r = &ix->own;
  }
  Run256& root() { return run.back(); }
  // Every stream not known drained is synchronised; only then the members go: the mutex is released, and the caller's
  // host buffers may follow.  (On the paths that succeed everything has been seen drained and nothing is synchronised here.)
  ~Call256() {
    for (Run256& u : run)
      if (!u.drained) {
        cbh::DeviceGuard dg(u.r->device);
        (void)hipStreamSynchronize(u.r->stream);
      }
  }
};

// the device of a scanning run for a scope: a shard's own; a plain handle's rows are on the device the call holds already
struct RunDevice {
  std::optional<cbh::DeviceGuard> g;
  RunDevice(const Call256& K, const Run256& u) { if (K.S) g.emplace(u.r->device); }
  bool ok() const { return !g || g->ok; }
};

// the handle's own block and cut scratch, the segment tables, and on every run with rows: room for the needles and a first
// record block (2^22 records, split over the shards), the needles, todo
int begin_scan(Call256& K, size_t out_nq, int out_k) {
  cbh_idx256* ix = K.ix;
  int rc = ix->own.ensure_scan(K.nq, std::max<size_t>(ix->own.rec_cap, (size_t)1 << 22));
  if (!rc) rc = ix->ensure_cut(out_nq, out_k);
  if (!rc && K.S) rc = upload_segments(K.S);
  if (rc) return rc;
  const size_t first_block = std::max<size_t>(65536, ((size_t)1 << 22) / K.n_scan);
  for (size_t s = 0; s < K.n_scan; ++s) {
    Run256& u = K.run[s];
    if (!u.r->n) continue;
    RunDevice dev(K, u);
    if (!dev.ok()) return CBH_E_NODEVICE;
    if (K.S && (rc = u.r->ensure_scan(K.nq, std::max(u.r->rec_cap, first_block)))) return rc;
    CBH_HIP(hipMemcpyAsync(u.r->d_q, K.needles, K.nq * 32, hipMemcpyHostToDevice, u.work()));
    u.todo = true;
  }
  return CBH_OK;
}

// every run that has to scan: counter, scan, count back, on its own stream
int launch_round(Call256& K, int attempt) {
  for (size_t s = 0; s < K.n_scan; ++s) {
    Run256& u = K.run[s];
    if (!u.todo) continue;
    Rows256* r = u.r;
    RunDevice dev(K, u);
    if (!dev.ok()) return CBH_E_NODEVICE;
    hipStream_t st = u.work();
    CBH_HIP(hipMemsetAsync(r->d_total, 0, 8, st));
    CBH_HIP(hipEventRecord(r->ev0, st));
    const int rc = cbh::launch_hamm256_scan(r->d_rows, r->n, r->d_q, K.nq, K.thresh, r->d_rec, r->rec_cap, r->d_total, st);
    if (rc) return rc;
    CBH_HIP(hipEventRecord(r->ev1, st));
    CBH_HIP(hipMemcpyAsync(r->h_total, r->d_total, 8, hipMemcpyDeviceToHost, st));
    if (K.S) K.S->comm.n_scans++, K.S->comm.n_rescans += attempt ? 1 : 0;
  }
  return CBH_OK;
}

// waits for the round; a run whose count outgrew its block grows the block (the count plus 1024) and has to scan again,
// up to three attempts.  *slowest: the longest kernel time of the round in ms, < 0 if none could be read.
int collect_round(Call256& K, int attempt, float* slowest) {
  *slowest = -1.f;
  for (size_t s = 0; s < K.n_scan; ++s) {
    Run256& u = K.run[s];
    if (!u.todo) continue;
    Rows256* r = u.r;
    RunDevice dev(K, u);
    if (!dev.ok()) return CBH_E_NODEVICE;
    CBH_HIP(hipStreamSynchronize(r->stream));
    u.saw_drained();
    u.count = *r->h_total;
    float ms = 0;
    if (hipEventElapsedTime(&ms, r->ev0, r->ev1) == hipSuccess) *slowest = std::max(*slowest, ms);
    u.todo = false;
    if (u.count <= r->rec_cap) continue;
    if (attempt >= 2) return CBH_E_OVERFLOW;
    const int rc = grow_for_result(K.ix, r, u.count);
    if (rc) return rc;
    u.todo = true;
  }
  return CBH_OK;
}

// The rounds, and what cbh_idx256_get_stats counts of them.  A plain handle counts every attempt as a scan of its own: its
// kernel time (when it could be read), n * nq pairs, one launch.  A sharded handle counts the call once: the sum over the
// rounds of the slowest shard, n * nq pairs, one launch (the shards' launches are cbh_shard_stats' scans / rescans).
int scan_rounds(Call256& K) {
  cbh_idx256* ix = K.ix;
  float call_ms = 0;
  auto count_scan = [&](float ms) { ix->scan_ms += ms, ix->scan_pairs += (uint64_t)ix->n * K.nq, ix->scan_launches++; };
  auto any_todo = [&] { return std::any_of(K.run.begin(), K.run.begin() + K.n_scan, [](const Run256& u) { return u.todo; }); };
  for (int attempt = 0; any_todo(); ++attempt) {  // (collect_round ends the third)
    float ms = 0;
    int rc = launch_round(K, attempt);
    if (!rc) rc = collect_round(K, attempt, &ms);
    if (rc) return rc;
    if (K.S)
      call_ms += std::max(ms, 0.f);
    else if (ms >= 0)
      count_scan(ms);
  }
  if (K.S) count_scan(call_ms);
  return CBH_OK;
}

// sharded only: local rows -> global rows on every shard, then the exchange into the handle's own block (grown to the sum
// of the counts), and both sides of it finished
int gather_shards(Call256& K, unsigned long long* total) {
  cbh_idx256* ix = K.ix;
  Shards256* S = K.S;
  unsigned long long sum = 0;
  for (size_t s = 0; s < K.n_scan; ++s) sum += K.run[s].count;
  if (sum > ix->own.rec_cap) {
    cbh::DeviceGuard dg(ix->own.device);
    if (!dg.ok) return CBH_E_NODEVICE;
    const int rc = grow_for_result(ix, &ix->own, sum);
    if (rc) return rc;
  }
  std::vector<cbh::ShardPart> parts(K.n_scan);
  for (size_t s = 0; s < K.n_scan; ++s) {
    Run256& u = K.run[s];
    Rows256* r = u.r;
    cbh::DeviceGuard dg(r->device);
    if (!dg.ok) return CBH_E_NODEVICE;
    if (u.count) {
      hipLaunchKernelGGL(k_rows_to_global, dim3((unsigned)((u.count + 255) / 256)), dim3(256), 0, u.work(), r->d_rec, u.count,
                         S->d_seg_local[s], S->d_seg_delta[s], S->n_seg[s]);
      CBH_HIP(hipGetLastError());
    }
    if (!r->stream) {  // an empty shard that never scanned still takes part in a collective
      const int rc = r->ensure_scan(1, 1024);
      if (rc) return rc;
    }
    parts[s] = cbh::ShardPart{S->comm.dev_pos_of_shard(s), u.work(), r->d_rec, u.count, nullptr, 0, r->ev1, r->x, r->h_total};
  }
  cbh::DeviceGuard dg(ix->own.device);
  if (!dg.ok) return CBH_E_NODEVICE;
  const int rc = S->comm.exchange(parts, K.root().work(), ix->own.d_rec);
  if (rc) return rc;
  CBH_HIP(hipStreamSynchronize(ix->own.stream));
  K.root().saw_drained();
  for (size_t s = 0; s < K.n_scan; ++s) {  // the shards' side of a collective has finished too before their buffers are reused
    cbh::DeviceGuard dg2(K.run[s].r->device);
    if (!dg2.ok) return CBH_E_NODEVICE;
    CBH_HIP(hipStreamSynchronize(K.run[s].r->stream));
    K.run[s].saw_drained();
  }
  *total = sum;
  return CBH_OK;
}

// Every record of the call's needles under its threshold, in (needle, distance, row) order, in the handle's own block, on
// its stream; *total of them.  out_nq x out_k: the places the caller's cut needs (ensure_cut).
int sorted_records(Call256& K, size_t out_nq, int out_k, unsigned long long* total) {
  cbh_idx256* ix = K.ix;
  if (!K.g.ok) return CBH_E_NODEVICE;
  int rc = begin_scan(K, out_nq, out_k);
  if (!rc) rc = scan_rounds(K);
  if (rc) return rc;
  *total = K.run[0].count;
  if (K.S && (rc = gather_shards(K, total))) return rc;
  if (*total > 1) {
    unsigned long long* sorted = nullptr;
    hipStream_t st = K.root().work();
    if ((rc = cbh::sort_keys64_db(ix->own.d_rec, ix->d_alt, (size_t)*total, (unsigned)sig_bits256(K.nq), ix->d_tmp,
                                  ix->tmp_bytes, st, &sorted)))
      return rc;
    if (sorted != ix->own.d_rec)
      CBH_HIP(hipMemcpyAsync(ix->own.d_rec, sorted, *total * 8, hipMemcpyDeviceToDevice, st));
  }
  return CBH_OK;
}

// knn (k per needle descriptor, below thresh) for nq needle rows in host memory: row/dist [nq*k] in (distance, row) order,
// zero past the count; counts[nq] (full number under thresh)
int knn256(cbh_idx256* ix, const uint8_t* needles, size_t nq, int k, int thresh, uint32_t* row, uint16_t* dist,
           uint32_t* counts) {
  if (k > 0 && nq) {
    memset(row, 0, nq * (size_t)k * 4);
    memset(dist, 0, nq * (size_t)k * 2);
  }
  if (nq) memset(counts, 0, nq * 4);
  if (nq == 0 || ix->n == 0 || thresh <= 0 || k <= 0) return CBH_OK;  // (nothing to scan: the zeros are the answer)
  if (nq >= (1u << 23)) return CBH_E_INVAL;
  Call256 K(ix, needles, nq, thresh);
  unsigned long long total = 0;
  const int rc = sorted_records(K, nq, k, &total);
  if (rc) return rc;
  hipStream_t st = K.root().work();
  hipLaunchKernelGGL(k_select256, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, ix->own.d_rec, (size_t)total,
                     (uint32_t)nq, k, ix->d_out_row, ix->d_out_dist, ix->d_counts);
  CBH_HIP(hipGetLastError());
  CBH_HIP(hipMemcpyAsync(row, ix->d_out_row, nq * (size_t)k * 4, hipMemcpyDeviceToHost, st));
  CBH_HIP(hipMemcpyAsync(dist, ix->d_out_dist, nq * (size_t)k * 2, hipMemcpyDeviceToHost, st));
  CBH_HIP(hipMemcpyAsync(counts, ix->d_counts, nq * 4, hipMemcpyDeviceToHost, st));
  CBH_HIP(hipStreamSynchronize(st));
  K.root().saw_drained();
  return CBH_OK;
}

// radius search: every record, in (needle, distance, row) order.  `rec` is the caller's: it outlives the call's copies.
int radius256(cbh_idx256* ix, const uint8_t* needles, size_t nq, int thresh, std::vector<unsigned long long>* rec) {
  rec->clear();
  if (nq == 0 || ix->n == 0 || thresh <= 0) return CBH_OK;
  if (nq >= (1u << 23)) return CBH_E_INVAL;
  Call256 K(ix, needles, nq, thresh);
  unsigned long long total = 0;
  const int rc = sorted_records(K, 0, 0, &total);
  if (rc) return rc;
  rec->resize((size_t)total);
  hipStream_t st = K.root().work();
  if (total) CBH_HIP(hipMemcpyAsync(rec->data(), ix->own.d_rec, total * 8, hipMemcpyDeviceToHost, st));
  CBH_HIP(hipStreamSynchronize(st));
  K.root().saw_drained();
  return CBH_OK;
}

// votes and scores of one needle image (cvfeaturesindex.cpp:499-596) from a knn table that already carries the
// mediaId of every candidate (0 = deleted/removed item, :518)
void score_media(const uint32_t* media, const uint16_t* dist, const uint32_t* counts, size_t d0, size_t d1, int k,
                 std::vector<cbh_match>* out) {
  std::map<uint32_t, std::vector<int>> matches;  // QMap<uint32_t, Match_>: ascending mediaId
  for (size_t j = d0; j < d1; ++j) {
    const uint32_t len = std::min<uint32_t>((uint32_t)k, counts[j]);
    for (uint32_t t = 0; t < len; ++t) {
      const uint32_t mediaId = media[j * (size_t)k + t];
      if (!mediaId) continue;
      matches[mediaId].push_back((int)dist[j * (size_t)k + t]);
    }
  }
  for (auto& kv : matches) {
    std::vector<int>& scores = kv.second;
    std::sort(scores.begin(), scores.end());
    int score;
    const size_t middle = scores.size() / 2;
    if (scores.size() < 2)
      score = scores[0];
    else if (scores.size() % 2 == 0)
      score = (scores[middle - 1] + scores[middle]) / 2;
    else
      score = scores[middle];
    score = score * 1000 / (int)scores.size();
    out->push_back(cbh_match{kv.first, score});
  }
}

void score256(const cbh_idx256* ix, const uint32_t* row, const uint16_t* dist, const uint32_t* counts, size_t d0,
              size_t d1, int k, std::vector<cbh_match>* out) {
  std::vector<uint32_t> media((d1 - d0) * (size_t)k, 0);
  for (size_t j = d0; j < d1; ++j) {
    const uint32_t len = std::min<uint32_t>((uint32_t)k, counts[j]);
    for (uint32_t t = 0; t < len; ++t) media[(j - d0) * (size_t)k + t] = ix->media_of_row(row[j * (size_t)k + t]);
  }
  score_media(media.data(), dist + d0 * (size_t)k, counts + d0, 0, d1 - d0, k, out);
}

// per-needle results, score(i, &res) for needle i, packed into out (cap places) and out_offsets (n_needles + 1 entries)
template <class Score>
int pack_matches(size_t n_needles, Score score, cbh_match* out, size_t cap, uint64_t* out_offsets) {
  uint64_t pos = 0;
  for (size_t i = 0; i < n_needles; ++i) {
    out_offsets[i] = pos;
    std::vector<cbh_match> res;
    score(i, &res);
    for (auto& m : res) {
      if (pos < cap) out[pos] = m;
      ++pos;
    }
  }
  out_offsets[n_needles] = pos;
  return pos > cap ? CBH_E_OVERFLOW : CBH_OK;
}

}  // namespace

extern "C" {

cbh_idx256* cbh_idx256_create(int device) {
  cbh::clear_last_error();
  if (!cbh::device_usable(device)) return (cbh_idx256*)cbh::fail_handle(CBH_E_NODEVICE, "cbh_idx256_create: no usable gfx950 device at that ordinal");
  cbh_idx256* ix = new (std::nothrow) cbh_idx256;
  if (!ix) return (cbh_idx256*)cbh::fail_handle(CBH_E_NOMEM, "cbh_idx256_create: host allocation failed");
  ix->own.device = device;
  return ix;
}

cbh_idx256* cbh_idx256_create_sharded(uint32_t device_mask, int shards_per_device) {
  cbh::clear_last_error();
  Shards256* S = new (std::nothrow) Shards256;
  if (!S) return (cbh_idx256*)cbh::fail_handle(CBH_E_NOMEM, "cbh_idx256_create_sharded: host allocation failed");
  if (!S->comm.init(device_mask, shards_per_device)) {
    delete S;
    return (cbh_idx256*)cbh::fail_handle(CBH_E_INVAL, "cbh_idx256_create_sharded: empty mask, a device of the mask is not usable, or shards_per_device out of range");
  }
  cbh_idx256* ix = new (std::nothrow) cbh_idx256;
  if (!ix) {
    delete S;
    return (cbh_idx256*)cbh::fail_handle(CBH_E_NOMEM, "cbh_idx256_create_sharded: host allocation failed");
  }
  ix->own.device = S->comm.devices[0];
  ix->shards = S;
  const size_t R = S->comm.shard_count();
  S->shard.resize(R);
  for (size_t s = 0; s < R; ++s) S->shard[s].device = S->comm.device_of_shard(s);
  S->d_seg_local.assign(R, nullptr);
  S->d_seg_delta.assign(R, nullptr);
  S->n_seg.assign(R, 0);
  return ix;
}

int cbh_idx256_shard_count(const cbh_idx256* ix) { return !ix ? 0 : ix->shards ? (int)ix->shards->shard.size() : 1; }

size_t cbh_idx256_shard_rows(const cbh_idx256* ix, int i) {
  if (!ix) return 0;
  if (!ix->shards) return i == 0 ? ix->n : 0;
  return i >= 0 && (size_t)i < ix->shards->shard.size() ? ix->shards->shard[(size_t)i].n : 0;
}

int cbh_idx256_shard_stats(const cbh_idx256* ix, cbh_shard_stats* out) {
  if (!ix || !out) return CBH_E_INVAL;
  memset(out, 0, sizeof *out);
  out->shards = 1, out->devices = 1;
  if (!ix->shards) return CBH_OK;
  const Shards256* S = ix->shards;
  out->shards = (uint32_t)S->shard.size();
  out->devices = (uint32_t)S->comm.devices.size();
  out->device_mask = S->comm.mask;
  out->segments = S->segs.size();
  out->scans = S->comm.n_scans.load();
  out->rescans = S->comm.n_rescans.load();
  out->collectives = S->comm.n_collectives.load();
  out->peer_copies = S->comm.n_peer_copies.load();
  out->local_copies = S->comm.n_local_copies.load();
  return CBH_OK;
}

void cbh_idx256_destroy(cbh_idx256* ix) {
  if (!ix) return;
  cbh::combiner_drop(ix);  // combine.hip: the queue of cbh_*_find_coalesced callers
  if (Shards256* S = ix->shards) {
    S->comm.destroy_comms();
    for (size_t s = 0; s < S->shard.size(); ++s) {
      cbh::DeviceGuard g(S->shard[s].device);
      if (S->d_seg_local[s]) (void)hipFree(S->d_seg_local[s]);
      if (S->d_seg_delta[s]) (void)hipFree(S->d_seg_delta[s]);
      S->shard[s].release();
    }
    delete S;
  }
  cbh::DeviceGuard g(ix->own.device);
  ix->own.release();
  for (void* p : {(void*)ix->d_alt, (void*)ix->d_tmp, (void*)ix->d_out_row, (void*)ix->d_out_dist, (void*)ix->d_counts})
    if (p) (void)hipFree(p);
  delete ix;
}

/* add(): append one media's descriptor rows (cvfeaturesindex.cpp:122-150); n_rows == 0 is skipped with no
 * map entry ("no descriptors for ..."), as in the reference.  load() is add() per `matrix` row. */
int cbh_idx256_add(cbh_idx256* ix, uint32_t media_id, const uint8_t* rows, size_t n_rows) {
  if (!ix) return CBH_E_INVAL;
  ix->loaded = true;
  if (n_rows == 0) return CBH_OK;
  if (!rows) return CBH_E_INVAL;
  if (ix->n + n_rows > 0xfffffff0ull) return CBH_E_INVAL;
  std::lock_guard<std::mutex> lk(ix->mu);
  Shards256* S = ix->shards;  // the rows go to a shard, the maps stay here in global row numbers
  Rows256& dst = S ? S->shard[S->next_shard()] : ix->own;
  const size_t local = dst.n;
  cbh::DeviceGuard g(dst.device);
  if (!g.ok) return CBH_E_NODEVICE;
  const int rc = dst.append(rows, n_rows);
  if (rc) return rc;
  if (S) S->note_rows(local, ix->n, n_rows);
  // _idMap[mid] = numDesc; _indexMap[numDesc] = mid; sentinel (numDesc + rows) -> 0
  ix->first_row.back() = (uint32_t)ix->n;
  ix->media_id.back() = media_id;
  ix->id_to_first[media_id] = (uint32_t)ix->n;
  ix->n += n_rows;
  ix->first_row.push_back((uint32_t)ix->n);
  ix->media_id.push_back(0);
  return CBH_OK;
}

/* remove(): the media's map entry becomes id 0; its descriptors stay in the matrix (:152-165) */
int cbh_idx256_remove(cbh_idx256* ix, const uint32_t* ids, size_t n) {
  if (!ix || (n && !ids)) return CBH_E_INVAL;
  std::lock_guard<std::mutex> lk(ix->mu);
  for (size_t i = 0; i < n; ++i) {
    auto it = ix->id_to_first.find(ids[i]);
    if (it == ix->id_to_first.end()) continue;
    auto p = std::lower_bound(ix->first_row.begin(), ix->first_row.end() - 1, it->second);
    if (p != ix->first_row.end() - 1 && *p == it->second) ix->media_id[(size_t)(p - ix->first_row.begin())] = 0;
  }
  return CBH_OK;
}

int cbh_idx256_is_loaded(const cbh_idx256* ix) { return ix && ix->loaded; }
size_t cbh_idx256_count(const cbh_idx256* ix) { return ix ? ix->n : 0; }  // _descriptors.rows (:103)
size_t cbh_idx256_memory_usage(const cbh_idx256* ix) { return ix ? ix->n * 32 * 2 : 0; }  // (:105-120)

/* descriptorsForMediaId (:421-436): row range of one media (0,0 when unknown) */
int cbh_idx256_rows_of(const cbh_idx256* ix, uint32_t media_id, size_t* first, size_t* count) {
  if (!ix || !first || !count) return CBH_E_INVAL;
  *first = *count = 0;
  auto it = ix->id_to_first.find(media_id);
  if (it == ix->id_to_first.end()) return CBH_OK;
  auto p = std::lower_bound(ix->first_row.begin(), ix->first_row.end(), it->second);
  *first = it->second;
  *count = (size_t)(*(p + 1) - *p);
  return CBH_OK;
}

int cbh_idx256_download_rows(const cbh_idx256* ix, size_t first, size_t count, uint8_t* out) {
  if (!ix || (count && !out) || first + count > ix->n) return CBH_E_INVAL;
  if (!count) return CBH_OK;
  if (ix->shards) {  // the range may span runs on several shards
    for (const Shards256::Seg& sg : ix->shards->segs) {
      const size_t a = std::max(first, sg.global), b = std::min(first + count, sg.global + sg.len);
      if (a >= b) continue;
      const Rows256& c = ix->shards->shard[sg.shard];
      cbh::DeviceGuard g(c.device);
      if (!g.ok) return CBH_E_NODEVICE;
      CBH_HIP(hipMemcpy(out + (a - first) * 32, c.d_rows + (sg.local + (a - sg.global)) * 32, (b - a) * 32,
                        hipMemcpyDeviceToHost));
    }
    return CBH_OK;
  }
  cbh::DeviceGuard g(ix->own.device);
  if (!g.ok) return CBH_E_NODEVICE;
  CBH_HIP(hipMemcpy(out, ix->own.d_rows + first * 32, count * 32, hipMemcpyDeviceToHost));
  return CBH_OK;
}

/* slice() (cvfeaturesindex.cpp:285-309): the rows of the listed media in ascending id order, as add() media by media
 * would build them -- the same maps, the same rows in the same global order and, on a sharded parent, the same shards.
 * A media takes the rows cbh_idx256_rows_of reports (a removed media too: _idMap keeps it); ids without rows are skipped.
 * The host plans one row range per kept media from the maps; the rows move on the device (slice.hip: k_slice_rows),
 * and rows that change ordinal travel as one staged contiguous block per (source shard, destination shard). */
extern "C++" {
namespace {

struct Move256 {  // the kept media that go from one source Rows256 to one destination Rows256, in id order
  const Rows256* src = nullptr;
  Rows256 *dst = nullptr, *via = nullptr;  // via: the new handle's Rows256 on the source's device (its stream does the source side)
  std::vector<uint32_t> dstf, srcf, len;
  std::vector<uint32_t> table, table2;  // as launch_slice_rows256 takes them (kept until the copies have run)
  size_t rows = 0;
};

// arena blocks and the streams they were used on: the blocks go back, then the streams are drained -- on every return
struct Held256 {
  std::vector<std::pair<void*, Rows256*>> blocks;
  std::vector<Rows256*> used;
  template <class T>
  int take(T** p, size_t bytes, Rows256* on) {  // (on->device is current)
    void* q = nullptr;
    *p = nullptr;
    CBH_HIP(cbh::malloc_async(&q, std::max<size_t>(bytes, 16), on->stream));
    blocks.emplace_back(q, on);
    *p = static_cast<T*>(q);
    return CBH_OK;
  }
  int use(Rows256* r) {  // (r->device is current)
    if (std::find(used.begin(), used.end(), r) != used.end()) return CBH_OK;
    const int rc = r->ensure_scan(0, 0);
    if (!rc) used.push_back(r);
    return rc;
  }
  ~Held256() {
    for (auto& b : blocks) {
      cbh::DeviceGuard g(b.second->device);  // (a cache over its budget records an event on the block's stream)
      (void)cbh::free_async(b.first, b.second->stream);
    }
    for (Rows256* r : used) {
      cbh::DeviceGuard g(r->device);
      (void)hipStreamSynchronize(r->stream);
    }
  }
};

// pk | dst firsts | src firsts, n + 1 words each (the last pk = the row count); `packed` replaces one side by pk
void make_table(const Move256& m, int packed_side, std::vector<uint32_t>* t) {
  const size_t k = m.len.size();
  t->assign(3 * (k + 1), 0);
  uint32_t at = 0;
  for (size_t i = 0; i < k; ++i) {
    (*t)[i] = at;
    (*t)[(k + 1) + i] = packed_side == 1 ? at : m.dstf[i];
    (*t)[2 * (k + 1) + i] = packed_side == 2 ? at : m.srcf[i];
    at += m.len[i];
  }
  (*t)[k] = at;
}

int slice256(cbh_idx256* ix, const std::vector<uint32_t>& ids, cbh_idx256* out) {
  std::lock_guard<std::mutex> lk(ix->mu);
  Shards256 *S = ix->shards, *T = out->shards;
  const size_t R = S ? S->shard.size() : 1;
  std::vector<Move256> moves(R * R);  // [source shard * R + destination shard]
  // plan: the maps of the new handle and where every kept media's rows come from and go to
  for (uint32_t id : ids) {
    size_t first = 0, cnt = 0;
    cbh_idx256_rows_of(ix, id, &first, &cnt);
    if (!cnt) continue;
    size_t s = 0, src_local = first, d = 0;
    if (S) {
      auto g = std::upper_bound(S->segs.begin(), S->segs.end(), first,
                                [](size_t row, const Shards256::Seg& sg) { return row < sg.global; });
      --g;  // (the run that holds the media's first row holds all of them: a media is appended in one piece)
      s = g->shard, src_local = g->local + (first - g->global);
      d = T->next_shard();
    }
    Rows256& dst = T ? T->shard[d] : out->own;
    Move256& m = moves[s * R + d];
    m.src = S ? &S->shard[s] : &ix->own;
    m.dst = &dst;
    m.via = T ? &T->shard[s] : &out->own;
    m.dstf.push_back((uint32_t)dst.n), m.srcf.push_back((uint32_t)src_local), m.len.push_back((uint32_t)cnt);
    m.rows += cnt;
    if (T) T->note_rows(dst.n, out->n, cnt);
    dst.n += cnt;
    out->first_row.back() = (uint32_t)out->n;
    out->media_id.back() = id;
    out->id_to_first[id] = (uint32_t)out->n;
    out->n += cnt;
    out->first_row.push_back((uint32_t)out->n);
    out->media_id.push_back(0);
    out->loaded = true;
  }
  // room for the rows, exactly
  for (size_t d = 0; d < R; ++d) {
    Rows256& dst = T ? T->shard[d] : out->own;
    if (!dst.n) continue;
    cbh::DeviceGuard g(dst.device);
    if (!g.ok) return CBH_E_NODEVICE;
    CBH_HIP(hipMalloc(&dst.d_rows, dst.n * 32));
    dst.cap = dst.n;
  }
  Held256 H;
  int rc;
  for (Move256& m : moves) {
    if (!m.rows) continue;
    const size_t k = m.len.size();
    uint32_t* d_table = nullptr;
    cbh::DeviceGuard g(m.src->device);
    if (!g.ok) return CBH_E_NODEVICE;
    if ((rc = H.use(m.via))) return rc;
    hipStream_t st = m.via->stream;
    const bool across = m.dst->device != m.src->device;
    make_table(m, across ? 1 : 0, &m.table);
    if ((rc = H.take(&d_table, m.table.size() * 4, m.via))) return rc;
    CBH_HIP(hipMemcpyAsync(d_table, m.table.data(), m.table.size() * 4, hipMemcpyHostToDevice, st));
    if (!across) {  // (the moves of a call fill disjoint rows of a destination: no order between their streams)
      if ((rc = cbh::launch_slice_rows256(m.src->d_rows, m.dst->d_rows, d_table, k, m.rows, st))) return rc;
      continue;
    }
    // gather into a contiguous block here, carry it across, scatter it there
    uint8_t *stage = nullptr, *landed = nullptr;
    uint32_t* d_table2 = nullptr;
    if ((rc = H.take(&stage, m.rows * 32, m.via))) return rc;
    if ((rc = cbh::launch_slice_rows256(m.src->d_rows, stage, d_table, k, m.rows, st))) return rc;
    {
      cbh::DeviceGuard gd(m.dst->device);
      if (!gd.ok) return CBH_E_NODEVICE;
      if ((rc = H.use(m.dst))) return rc;
      if ((rc = H.take(&landed, m.rows * 32, m.dst)) || (rc = H.take(&d_table2, m.table.size() * 4, m.dst))) return rc;
      CBH_HIP(hipEventRecord(m.dst->ev0, m.dst->stream));  // (what the landing block was used for before has finished)
    }
    CBH_HIP(hipStreamWaitEvent(st, m.dst->ev0, 0));
    CBH_HIP(hipMemcpyPeerAsync(landed, m.dst->device, stage, m.src->device, m.rows * 32, st));
    CBH_HIP(hipEventRecord(m.via->ev1, st));
    if (T) T->comm.n_peer_copies++;
    cbh::DeviceGuard gd(m.dst->device);
    if (!gd.ok) return CBH_E_NODEVICE;
    make_table(m, 2, &m.table2);
    CBH_HIP(hipMemcpyAsync(d_table2, m.table2.data(), m.table2.size() * 4, hipMemcpyHostToDevice, m.dst->stream));
    CBH_HIP(hipStreamWaitEvent(m.dst->stream, m.via->ev1, 0));
    if ((rc = cbh::launch_slice_rows256(landed, m.dst->d_rows, d_table2, k, m.rows, m.dst->stream))) return rc;
  }
  for (Rows256* r : H.used) {
    cbh::DeviceGuard g(r->device);
    if (!g.ok) return CBH_E_NODEVICE;
    CBH_HIP(hipStreamSynchronize(r->stream));
  }
  cbh::note_slice_on_device();
  return CBH_OK;
}

}  // namespace
}  // extern "C++"

cbh_idx256* cbh_idx256_slice(const cbh_idx256* ix, const uint32_t* ids, size_t n) {
  cbh::clear_last_error();
  if (!ix || (n && !ids)) return (cbh_idx256*)cbh::fail_handle(CBH_E_INVAL, "cbh_idx256_slice: no index, or a count without ids");
  std::vector<uint32_t> want(ids, ids + (ids ? n : 0));
  std::sort(want.begin(), want.end());
  want.erase(std::unique(want.begin(), want.end()), want.end());
  cbh_idx256* out = ix->shards ? cbh_idx256_create_sharded(ix->shards->comm.mask, ix->shards->comm.per_device)
                               : cbh_idx256_create(ix->own.device);
  if (!out) return nullptr;  // (the create call has set the code)
  if (const int rc = slice256(const_cast<cbh_idx256*>(ix), want, out)) {
    cbh_idx256_destroy(out);
    return (cbh_idx256*)cbh::fail_handle(rc, nullptr);
  }
  return out;
}

/* exact knnSearch(needles, k) restricted to distance < thresh: out_row/out_dist [nq*k] in (distance, row)
 * order, counts[nq] = number of rows under thresh (may exceed k) */
int cbh_idx256_knn(cbh_idx256* ix, const uint8_t* needles, size_t nq, int k, int thresh, uint32_t* out_row,
                   uint16_t* out_dist, uint32_t* counts) {
  if (!ix || (nq && (!needles || !out_row || !out_dist || !counts))) return CBH_E_INVAL;
  return knn256(ix, needles, nq, k, thresh, out_row, out_dist, counts);
}

/* knn + the mediaId of every candidate row (0 = removed): the shard-local step of the multi-GPU path, where the
 * first-row -> mediaId map is local to the shard */
int cbh_idx256_knn_media(cbh_idx256* ix, const uint8_t* needles, size_t nq, int k, int thresh, uint32_t* out_row,
                         uint16_t* out_dist, uint32_t* out_media, uint32_t* counts) {
  if (!ix || (nq && (!needles || !out_row || !out_dist || !out_media || !counts))) return CBH_E_INVAL;
  int rc = cbh_idx256_knn(ix, needles, nq, k, thresh, out_row, out_dist, counts);
  if (rc) return rc;
  for (size_t j = 0; j < nq; ++j) {
    const uint32_t len = std::min<uint32_t>((uint32_t)std::max(k, 0), counts[j]);
    for (uint32_t t = 0; t < (uint32_t)std::max(k, 0); ++t)
      out_media[j * (size_t)k + t] = t < len ? ix->media_of_row(out_row[j * (size_t)k + t]) : 0u;
  }
  return CBH_OK;
}

/* the scoring half of find() (:499-596) on a knn table with mediaIds (host code): what every rank runs on the
 * merged candidate lists in the multi-GPU path */
int cbh_cvfeatures_score(const uint32_t* media, const uint16_t* dist, const uint32_t* counts, const uint64_t* offsets,
                         size_t n_needles, int k, cbh_match* out, size_t cap, uint64_t* out_offsets) {
  if (!offsets || !out_offsets || (cap && !out) || k <= 0) return CBH_E_INVAL;
  if (n_needles && offsets[n_needles] && (!media || !dist || !counts)) return CBH_E_INVAL;
  auto score = [&](size_t i, std::vector<cbh_match>* res) {
    score_media(media, dist, counts, (size_t)offsets[i], (size_t)offsets[i + 1], k, res);
  };
  return pack_matches(n_needles, score, out, cap, out_offsets);
}

/* CvFeaturesIndex::find (:438-604) for one needle with n_desc descriptor rows */
int cbh_idx256_find(cbh_idx256* ix, const uint8_t* needle_rows, size_t n_desc, int thresh, int k, cbh_match* out,
                    size_t cap, size_t* n_out) {
  if (!ix || !n_out || (cap && !out) || (n_desc && !needle_rows)) return CBH_E_INVAL;
  *n_out = 0;
  const size_t places = n_desc * (size_t)std::max(k, 0);
  std::vector<uint32_t> row(places), cnt(n_desc);
  std::vector<uint16_t> dist(places);
  int rc = knn256(ix, needle_rows, n_desc, k, thresh, row.data(), dist.data(), cnt.data());
  if (rc) return rc;
  std::vector<cbh_match> res;
  score256(ix, row.data(), dist.data(), cnt.data(), 0, n_desc, k, &res);
  *n_out = res.size();
  for (size_t i = 0; i < res.size() && i < cap; ++i) out[i] = res[i];
  return CBH_OK;
}

int cbh_idx256_find_batch(cbh_idx256* ix, const uint8_t* needle_rows, const uint64_t* offsets, size_t n_needles,
                          int thresh, int k, cbh_match* out, size_t cap, uint64_t* out_offsets) {
  if (!ix || !offsets || !out_offsets || (cap && !out)) return CBH_E_INVAL;
  const size_t nq = n_needles ? (size_t)offsets[n_needles] : 0;
  const size_t places = nq * (size_t)std::max(k, 0);
  std::vector<uint32_t> row(places), cnt(nq);
  std::vector<uint16_t> dist(places);
  int rc = knn256(ix, needle_rows, nq, k, thresh, row.data(), dist.data(), cnt.data());
  if (rc) return rc;
  auto score = [&](size_t i, std::vector<cbh_match>* res) {
    score256(ix, row.data(), dist.data(), cnt.data(), (size_t)offsets[i], (size_t)offsets[i + 1], k, res);
  };
  return pack_matches(n_needles, score, out, cap, out_offsets);
}

/* cv::BFMatcher(NORM_HAMMING).radiusMatch(queryDescriptors, matches, maxDistance) against the rows of the index as
 * the train set (src/templatematcher.cpp:134,217): every (query, train) pair with distance <= max_dist, grouped by
 * query in ascending (distance, train row) order -- OpenCV sorts each query's list by distance and leaves equal
 * distances in unspecified order.  out_first[q] .. out_first[q+1] delimit query q's matches (nq + 1 entries). */
int cbh_idx256_radius_match(cbh_idx256* ix, const uint8_t* queries, size_t nq, int max_dist, cbh_dmatch* out,
                            size_t cap, uint64_t* out_first) {
  if (!ix || !out_first || (nq && !queries) || (cap && !out)) return CBH_E_INVAL;
  if (max_dist < 0) max_dist = -1;
  if (max_dist > 256) max_dist = 256;
  std::vector<unsigned long long> rec;
  int rc = radius256(ix, queries, nq, max_dist + 1, &rec);
  if (rc) return rc;
  size_t p = 0;
  for (size_t q = 0; q < nq; ++q) {
    out_first[q] = p;
    while (p < rec.size() && (size_t)(rec[p] >> 41) == q) {
      if (p < cap) out[p] = cbh_dmatch{(int32_t)q, (int32_t)(uint32_t)rec[p], (int32_t)((rec[p] >> 32) & 0x1ff)};
      ++p;
    }
  }
  out_first[nq] = p;
  return p > cap ? CBH_E_OVERFLOW : CBH_OK;
}

int cbh_idx256_get_stats(const cbh_idx256* ix, cbh_stats* out) {
  if (!ix || !out) return CBH_E_INVAL;
  out->scan_launches = ix->scan_launches;
  out->scan_pairs = ix->scan_pairs;
  out->scan_ms = ix->scan_ms;
  return CBH_OK;
}

}  // extern "C"
