// cbh_internal.h -- shared declarations between the host shim and the kernel launchers.
// 64-bit threshold searches: every caller goes through launch_hamm64_scan (hamm64_scan.hip), the one place that decides
// between the bucketed join, the popcount kernel and the matrix-core kernels; those modules launch what they are told.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "cbird_hip.h"

namespace cbh {

void combiner_drop(const void* handle);  // combine.hip
void set_last_error(const char* where, hipError_t e);
void set_last_error_text(const char* text);  // non-HIP failures (RCCL)
// The thread's error state is per call for the entry points that return a handle: clear_last_error() on entry, and every
// NULL return goes through fail_handle(code, why) so that cbh_last_error_code() names THIS failure, never an older one.
void clear_last_error();
void set_last_error_code(int code);  // keeps the text (a successful fall-back leaves its note, not an error code)
void* fail_handle(int code, const char* why);  // sets code + text (text kept if `why` is null and a text exists), returns nullptr

// ---- stream-ordered scratch memory (cbird_hip.hip) ------------------------------------------------------------------
// malloc_async(&p, bytes, stream) takes a block and free_async(p, stream) gives it back behind the last kernel that uses
// it (the contract of hipMallocAsync / hipFreeAsync).  Launchers do both through the Scratch guard below; only blocks
// that outlive the function that takes them are freed by hand (DESIGN.md names them).
// The source is the library's own arena: hipMalloc'ed blocks cached per (device, stream), reused only by the stream that
// freed them; bounded ("pool_live_keep_mb" per live stream, "pool_keep_mb" for blocks that outlive theirs, 32 stream
// caches, cbh_trim).  (ROCm's hipMallocAsync pools hand out memory that is still in use on this stack:
// tools/ubench/pool_cross_stream.hip.)
hipError_t malloc_async(void** p, size_t bytes, hipStream_t s);
hipError_t free_async(void* p, hipStream_t s);
// for streams the library creates itself: synchronise, hand the cached blocks to the device's orphan list, destroy
void stream_destroy(hipStream_t s);
void set_pool_keep_mb(int mb);
void set_pool_live_keep_mb(int mb);
int trim_pools(int device, unsigned long long* released_bytes);
// The scratch of one launcher: every block taken through get() goes back with free_async on the same stream when the
// guard leaves scope -- behind the kernels that were queued, and on every early return (a later allocation that fails,
// a launch error) as well as at the end.
struct Scratch {
  hipStream_t s;
  void* blocks[16];
  int n = 0;
  explicit Scratch(hipStream_t stream) : s(stream) {}
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  template <class T>
  hipError_t get(T** p, size_t bytes) {
    void* q = nullptr;
    *p = nullptr;
    if (n >= 16) return hipErrorInvalidValue;
    hipError_t e = malloc_async(&q, bytes, s);
    if (e != hipSuccess) return e;
    blocks[n++] = q;
    *p = static_cast<T*>(q);
    return hipSuccess;
  }
  ~Scratch() {
    while (n > 0) (void)free_async(blocks[--n], s);
  }
};

// ---- fault injection (cbird_hip.hip; tests/test_error_paths.py) ------------------------------------------------------
// Every allocation the library makes -- scratch through malloc_async, index / table memory through hipMalloc, pinned
// words through hipHostMalloc -- first passes fault_gate().  cbh_set_tuning("fault_alloc_after", n) arms it: the n-th
// allocation from now (0 = the next one) fails ONCE with hipErrorOutOfMemory, then the gate disarms itself;
// cbh_get_tuning("fault_alloc_after") reads what is left (-1 = disarmed or fired).  The arena's own calls into the
// driver are written (hipMalloc)(...) and pass "fault_driver_oom" instead (the trim-and-retry path).
hipError_t fault_gate();
hipError_t fault_gate_driver();
void set_fault_alloc_after(int n);
void set_fault_driver_oom(int n);
void set_fault_alloc_sticky(int v);
void set_fault_rccl(int v);  // sharded.hip: 1 = behave as if librccl could not be loaded
long get_fault_alloc_after();
unsigned long get_fault_fired();
unsigned long get_alloc_calls();
int arena_counter(const char* name, long long* value);
hipError_t persistent_malloc(void** p, size_t bytes);
void set_fault_persist_oom(int n);  // "fault_persist_oom": the n-th persistent allocation is refused by the "driver" once
template <class T>
static inline hipError_t gated_malloc(T** p, size_t bytes) {
  hipError_t e = fault_gate();
  if (e != hipSuccess) {
    *p = nullptr;
    return e;
  }
  return persistent_malloc((void**)p, bytes);  // cbird_hip.hip: gives the scratch arena's caches back before it fails
}
template <class T>
static inline hipError_t gated_host_malloc(T** p, size_t bytes, unsigned flags = hipHostMallocDefault) {
  hipError_t e = fault_gate();
  if (e != hipSuccess) {
    *p = nullptr;
    return e;
  }
  return (hipHostMalloc)(p, bytes, flags);
}
#define hipMalloc(...) ::cbh::gated_malloc(__VA_ARGS__)
#define hipHostMalloc(...) ::cbh::gated_host_malloc(__VA_ARGS__)

// the code the C-ABI returns for a failed HIP call; fail() also leaves the error text
inline int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? CBH_E_NOMEM : CBH_E_HIP; }
inline int fail(const char* where, hipError_t e) {
  set_last_error(where, e);
  return hip_code(e);
}
#define CBH_HIP(call)                                     \
  do {                                                    \
    hipError_t e_ = (call);                               \
    if (e_ != hipSuccess) return ::cbh::fail(#call, e_);  \
  } while (0)

// a host table into a block of the launcher's scratch (at least one element's worth, so that an empty table still has an
// address).  The copy reads the host memory when the stream gets to it: the caller keeps it until it has synchronised
template <class T>
hipError_t upload(Scratch& scratch, T** d, const T* h, size_t count, hipStream_t s) {
  hipError_t e = scratch.get(d, std::max<size_t>(count, 1) * sizeof(T));
  if (e == hipSuccess && count) e = hipMemcpyAsync(*d, h, count * sizeof(T), hipMemcpyHostToDevice, s);
  return e;
}
template <class T>
hipError_t upload(Scratch& scratch, T** d, const std::vector<T>& h, hipStream_t s) {
  return upload(scratch, d, h.data(), h.size(), s);
}

// ---- the 64-bit threshold search: hamm64_scan.hip decides, hamm64_join.hip / hamm64_mfma.hip launch what they are told --
struct JoinCache;    // the resident slot tables of one index, below (hamm64_join.hip)
struct JoinTables;
struct JoinNeedles;
// Which matrix-core kernel takes a launch (hamm64_mfma.hip), and the largest threshold each can take: the prefilters keep a
// biased distance in a 6-bit field (Pre32: bias 16 + t - 1 against 32 bits; Pre48: 8 + t, which leaves that much room;
// Pre16: 24 + t - 1 has to stay under 32), Full is the three-field kernel up to 64 and the two-field one at 65.
// The values are what "scan_pre16" / "scan_pre48" and recorded profiles mean by them.
enum class ScanVariant : int { Auto = -1, Full = 0, Pre32 = 1, Pre48 = 2, Pre16 = 3 };
constexpr int max_thresh(ScanVariant v) {
  return v == ScanVariant::Pre32 ? 32 : v == ScanVariant::Pre48 ? 16 : v == ScanVariant::Pre16 ? 8 : 65;
}
// What a caller says about a search besides its shape.
struct ScanOpts {
  bool keep_id0 = false;              // also emit slots whose id is 0 (DctFeaturesIndex top-10 cut)
  // one u64 per needle: also require ((q[j] ^ hashes[i]) & qmask[j]) == 0 -- the reference's approximate structures only
  // compare a needle with the entries that share its low bits (HammingTree leaf, src/tree/hammingtree.h:244-252; RadixMap
  const uint64_t* d_qmask = nullptr;  // bucket, src/tree/radix.h:135-141)
  // a needle hash of 0 is a needle like any other: findVideo and DctFeaturesIndex::find hand every hash to the tree
  // (src/dctvideoindex.cpp:437, src/dctfeaturesindex.cpp:293); only DctHashIndex::find returns nothing for it.  The scan
  // kernels skip such needles, so the callers that hold one set this and launch_hamm64_scan adds their records in a
  // pass of its own (k_zero_needle_scan)
  bool zero_needles = false;
  // a call made of several launches against the same needles (the shards of a sharded handle):
  ScanVariant pre = ScanVariant::Auto;  // the kernel choice made once for the whole call (scan_pick_pre); Auto: the launch's own
  unsigned siblings = 1;              // launches running side by side on this device
  const uint4* qx = nullptr;          // the needles expanded once on this device (expand_needles_for_scan)
  // the bucketed join (hamm64_join.hip): the resident slot tables of the handle whose slots these are, and the slot in
  // which the launch leaves its reference to the tables it read -- the caller drops it once the stream has finished the
  // launch's kernels.  Both or neither; without them the join prepares the slots' side per call from the scratch arena
  JoinCache* join = nullptr;
  std::shared_ptr<const JoinTables>* join_hold = nullptr;
  const JoinNeedles* join_needles = nullptr;  // the needles' side prepared once on this device (join_prepare_needles)
};
// Appends one record per (query j, slot i) with popc(q[j]^hashes[i]) < thresh, ids[i] != 0,
// q[j] != 0 (ScanOpts::zero_needles: q[j] == 0 as well).  *d_total += number of such pairs; records with slot index >= cap
// are dropped.
// Runs the bucketed join, the popcount kernel or the matrix-core scan: the route at the end of hamm64_scan.hip.
int launch_hamm64_scan(const uint64_t* d_hashes, const uint32_t* d_ids, size_t n,
                       const uint64_t* d_q, size_t nq, int thresh, cbh_record* d_rec, size_t cap,
                       unsigned long long* d_total, hipStream_t stream, const ScanOpts& opts = {});
// For a call made of several launches: would a launch of n slots run the matrix-core scan; and the prefilter choice for
// the whole call, probed on one launch's n slots of the call's n_total (ScanOpts::pre)
bool scan_takes_mfma(size_t n, size_t nq, int thresh);
ScanVariant scan_pick_pre(const uint64_t* d_hashes, size_t n, size_t n_total, const uint64_t* d_q, size_t nq, int thresh,
                          hipStream_t stream);
// Needles (pairs, triples) per blockIdx.y chunk of a scan launch that has `wgs` workgroups per chunk: halved (rounding up)
// from the start value `c` while above `floor` and the launch has fewer than 8192 workgroups -- enough to fill 256 CUs several times
// over, while each workgroup still amortises its tile load over `floor` items; then at most 65535 chunks, in whole
// `multiple`s
inline uint32_t scan_chunk(uint64_t wgs, size_t items, uint32_t c, uint32_t floor, uint32_t multiple) {
  while (c > floor && wgs * ((items + c - 1) / c) < 8192) c = (c + 1) / 2;
  if ((items + c - 1) / c > 65535) c = (uint32_t)(((items + 65534) / 65535 + multiple - 1) / multiple) * multiple;
  return c;
}
// the knobs and read-backs behind cbh_set_tuning / cbh_get_tuning (include/cbird_hip.h documents each)
int set_scan_mfma(int mode);  // 0..4; CBH_E_INVAL (knob unchanged) for anything else
int get_scan_mfma();
void set_scan_pre_max(int t);
void set_scan_pre_rate(int e9);
void set_scan_pre48(int v);
int set_scan_pre16(int v);  // -1, 0, 1; CBH_E_INVAL (knob unchanged) for anything else
long long get_scan_pre_mask();
long long get_scan_pre48_mask();
long long get_scan_pre16_mask();
long long get_scan_probes();
long long get_scan_probe_rate_e9();
long long get_scan_probe_true_e9();
long long get_scan_probe_rate48_e9();
long long get_scan_probe_rate16_e9();

// ---- the lone needle (Engine::query / -similar-to: one find() at a time) ---------------------------------------------
// One kernel launch and no copies: the needle travels as a kernel argument, matches go straight into a pinned, coherent
// host block, the last workgroup to finish publishes the count and a sequence number that the host polls for
// (hipStreamSynchronize costs ~6.5 us even on a drained stream; the plain path's needle upload, counter reset, two
// read-backs and synchronisation were 26 us per find, ~25 us PER SHARD on a sharded handle).
struct LoneBlock {
  volatile unsigned long long done;  // the call's sequence number, written last
  unsigned long long count;          // matches found (may exceed kRecs: then the caller takes the general path)
  static constexpr unsigned kRecs = 512;
  cbh_record recs[kRecs];            // dist << 32 | id (needle index 0), unordered
};
// d_state: two zeroed words of device memory owned by the caller's workspace (the kernel leaves them zeroed)
int launch_find_one(const uint64_t* d_hashes, const uint32_t* d_ids, size_t n, uint64_t q, int thresh, unsigned* d_state,
                    LoneBlock* h_block, unsigned long long seq, hipStream_t stream);
// spin until the block carries `seq`, with no time limit; every 4096 polls ask whether the stream is still busy: once it
// is idle without `seq`, or the query fails, CBH_E_HIP (only the failed query sets an error text).  CBH_OK / CBH_E_HIP
int wait_find_one(const LoneBlock* h_block, unsigned long long seq, hipStream_t stream);

// ---- hamm64_mfma.hip: the same scan on the matrix cores (FP4 sign dot products) --------
// variant: never Auto; CBH_E_INVAL for a threshold beyond max_thresh(variant)
int launch_hamm64_scan_mfma(const uint64_t* d_hashes, const uint32_t* d_ids, size_t n, const uint64_t* d_q, size_t nq,
                            int thresh, cbh_record* d_rec, size_t cap, unsigned long long* d_total, hipStream_t stream,
                            ScanVariant variant, const ScanOpts& opts);
// the needles of a call in the matrix-core kernels' operand layout, made ONCE for several launches against the same needles
// on one device (the shards of a sharded handle): *qx = malloc_async on `stream`, to be handed to every launch as
// ScanOpts::qx (launches on other streams wait for an event of `stream`) and given back with free_async once they have
// all finished
int expand_needles_for_scan(const uint64_t* d_q, size_t nq, hipStream_t stream, uint4** qx);
// k_fold_probe: the rates of fold-distance candidates and of true matches under `thresh` (<= kProbeMaxThresh) among a
// sample of the launch's pairs -- one host round trip; false if it could not run
constexpr int kProbeMaxThresh = 8;
// (r_cand48: candidates of the 48-bit prefilter word, 48-bit distance <= thresh or > 32 + thresh; r_cand16: of the 16-bit
// one, fold16 distance < thresh)
bool probe_fold_rates(const uint64_t* d_hashes, size_t n, const uint64_t* d_q, size_t nq, int thresh, hipStream_t stream,
                      double* r_cand, double* r_true, double* r_cand48, double* r_cand16);
// the 720 products of cbh_selftest_fp4_products into device memory
int selftest_fp4_products(float* d_out, hipStream_t stream);
// ---- hamm64_join.hip: the same search as a bucketed join (multi-index hashing), thresholds <= kJoinMaxThresh -----------
constexpr int kJoinMaxThresh = 8;
long long get_scan_joins();  // calls the join has answered so far (cbh_get_tuning "scan_joins")
long long get_join_needle_preps();  // needle sides prepared so far (cbh_get_tuning "join_needle_preps")
int set_join_resident(int v);     // "join_resident": 0 only handles opted in by cbh_idx64_join_prepare keep tables, 1 all
int set_join_resident_mb(int v);  // "join_resident_mb": what the tables of one index may hold, all plans together
int get_join_resident();
int get_join_resident_mb();
// The slots' side of one join plan (m = max(4, thresh) chunks), which depends on the index contents alone: the chunk
// values' histogram, its exclusive scans and the m chunk-ordered copies of the slots.  Immutable once published and
// reference counted: the index holds one reference, every launch that reads them another until its kernels are done, so a
// mutation only ever drops the index's (the rule of coalesce.hip's retired snapshots).
struct JoinTables {
  int m = 0, device = 0;
  size_t n = 0, bytes = 0;
  uint32_t *hist_h = nullptr, *start_h = nullptr, *hid = nullptr;
  uint64_t* hx = nullptr;
  JoinTables() = default;
  JoinTables(const JoinTables&) = delete;
  JoinTables& operator=(const JoinTables&) = delete;
  ~JoinTables();
};
// What an index owns of them (cbh_idx64::join; every shard of a sharded handle has its own).  plan[m] is current by
// construction: every path that changes the contents calls drop_all().
struct JoinCache {
  std::mutex mu;  // building and dropping; two first calls build once
  std::shared_ptr<const JoinTables> plan[kJoinMaxThresh + 1];
  std::atomic<bool> opted{false};  // cbh_idx64_join_prepare / _release
  std::atomic<uint64_t> builds{0}, hits{0}, drops{0}, failed_builds{0}, bytes{0};
  bool enabled() const { return opted.load() || get_join_resident() != 0; }
  std::shared_ptr<const JoinTables> current(int m);
  // the tables of plan m, built now if they are not there: nullptr (failure counted, *rc = CBH_E_NOMEM, error text set) when
  // memory or the budget does not allow them -- everything is allocated before anything is published.  Synchronises `stream`.
  std::shared_ptr<const JoinTables> get_or_build(int m, const uint64_t* d_hashes, const uint32_t* d_ids, size_t n, int device,
                                                 hipStream_t stream, int* rc);
  void drop_all();  // load, load_dev, add, remove, remove_ids_only, a shard's redistribution, release, destroy
  uint32_t plans();
};
// The needles' side of plans 5..8 (histogram -> start_q, the m chunk-ordered copies qx / qidx): independent of the slots,
// so a sharded call prepares it once per device (ScanOpts::join_needles).  The blocks are malloc_async on `stream`;
// launches on other streams wait for an event of it, and free() gives them back once they have all finished.
struct JoinNeedles {
  int m = 0;
  size_t nq = 0;
  uint32_t *start_q = nullptr, *qidx = nullptr;
  uint64_t* qx = nullptr;
  hipStream_t stream = nullptr;
  void free();
};
int join_prepare_needles(const uint64_t* d_q, size_t nq, int thresh, hipStream_t stream, JoinNeedles* out);
// would a launch of this shape go to the join at all (the route's answer)
bool scan_routes_to_join(size_t n, size_t nq, int thresh, bool masked);
// CBH_OK = done; CBH_E_UNSUPPORTED = the scan is cheaper for this call (decided from the exact candidate count against
// scan_ms_estimate unless `force`), or its jobs do not fit a grid: nothing written, the caller may scan.  No needle masks.
// Of `o`: keep_id0, join / join_hold, join_needles.
int launch_hamm64_join(const uint64_t* d_hashes, const uint32_t* d_ids, size_t n, const uint64_t* d_q, size_t nq,
                       int thresh, cbh_record* d_rec, size_t cap, unsigned long long* d_total, hipStream_t stream,
                       const ScanOpts& o, bool force, double scan_ms_estimate);

// ---- the 256-bit threshold scan: hamm256_scan.hip decides, hamm256_mfma.hip launches what it is told -------------------
// "scan256_kernels": which kernels 256-bit launches have used since the mask was last cleared (cbh_set_tuning(.., 0)).
// Noted by launch_hamm256_scan and nowhere else.
enum Scan256Kernel : int {
  kS256Scan = 1 << 0,     // k_hamm256_scan<8,4>
  kS256Mfma2 = 1 << 1,    // k_hamm256_mfma<6,3,2>
  kS256Mfma4 = 1 << 2,    // k_hamm256_mfma<6,3,4>
  kS256Mfma3 = 1 << 3,    // k_hamm256_mfma3<12,2>
  kS256Small4 = 1 << 4,   // k_hamm256_small<4>
  kS256Small8 = 1 << 5,   // k_hamm256_small<8>
  kS256Small16 = 1 << 6,  // k_hamm256_small<16>
};
// the kernel of a launch of n rows x nq needle descriptors, and the descriptor count its expanded needles are padded to
// (0: k_hamm256_scan reads the needles as they are)
struct Route256 {
  Scan256Kernel kernel;
  uint32_t nq_pad;
};
Route256 route256(size_t n, size_t nq, int thresh);
// Appends one record q << 41 | dist << 32 | row per (needle descriptor q, row) with popcount(xor of the 32 bytes) < thresh.
// *d_total += number of such pairs; records with slot index >= cap are dropped.
int launch_hamm256_scan(const uint8_t* d_rows, size_t n, const uint8_t* d_q, size_t nq, int thresh,
                        unsigned long long* d_rec, size_t cap, unsigned long long* d_total, hipStream_t stream);
int set_scan256_small(int v);  // stationary-needle kernel for <= 512 needle descriptors: 0 / 1; else CBH_E_INVAL, knob unchanged
int set_scan256_mfma(int v);   // 0..2 (2 = force for any size); else CBH_E_INVAL, knob unchanged
int get_scan256_small();
int get_scan256_mfma();
long long get_scan256_kernels();
void clear_scan256_kernels();
// hamm256_mfma.hip: the needles in the matrix-core kernels' operand layout (qx: nq_pad x 128 bytes), and one of its kernels
// on them
void expand_needles256(const uint8_t* d_q, size_t nq, uint32_t nq_pad, uint4* qx, hipStream_t stream);
int launch_hamm256_mfma(Scan256Kernel kernel, const uint8_t* d_rows, size_t n, const uint4* qx, const uint8_t* d_q,
                        size_t nq, int thresh, unsigned long long* d_rec, size_t cap, unsigned long long* d_total,
                        hipStream_t stream);

// ---- setters behind cbh_set_tuning (include/cbird_hip.h documents every knob) ---------------------------------------
void set_hash_mfma(int v);         // dcthash.hip "hash_mfma": 256 x 256 tiles on k_dcthash_256_band (non-zero) or k_dcthash_256 (0)
void set_hash_band_area(int v);    // dcthash.hip "hash_band_area": k_band_area for fractional ratios up to 1920 columns (1) or never (0)
void set_hash_stream(int v);       // dcthash.hip "hash_stream": k_blur_area_regs on strips -- 0 never, 1 by batch size, >= 2 always, of v steps
void set_hash_fuse(int v);         // dcthash.hip "hash_fuse": vertical INTER_AREA pass + tile inside k_blur_area_regs (0 never, 1 auto, 2 always)
void set_kp_blur_side(int v);      // kphash.hip "kp_blur_side": largest keypoint square whose blurred copy stays in LDS (default 112)
void set_kp_lds_side(int v);       // kphash.hip "kp_lds_side": largest keypoint square processed in LDS (default 134)
extern int g_fdct_host_vote, g_video_host_reduce;  // fdct.hip: 0 = device for batches / host for one needle, 1 = host, 2 = device
void set_orb_retain_order(int v);  // orb.hip: 1 (default) retainBest in libstdc++'s order, 0 canonical (ties kept, raster order)
void set_cd_chunk_mb(int v);       // colordesc_create.hip "color_create_chunk_mb": MB of scratch one launch may take
int set_cd_group(int v);           // colordesc_create.hip "color_create_group": images per wave of k_cdw_round, 0 (by size) / 1 / 2 / 4 / 8 / 16 / 21; else CBH_E_INVAL, knob unchanged
int get_cd_group();
int get_cd_group_last();           // "color_create_group_last": images per wave of the most recent chunk launch (0 = none yet)
void set_quality_chunk_mb(int v);  // quality.hip "quality_chunk_mb": MB one upload / one group's working planes may take
int get_quality_chunk_mb();
int get_quality_strip_rows();      // "quality_strip_rows": rows one thread of the quality kernels walks
void set_tmatch_chunk_mb(int v);   // tmatch.hip "tmatch_chunk_mb": MB one upload / one group's patches may take
int get_tmatch_chunk_mb();
int get_diff_block_pixels();       // diffimage.hip "diff_block_pixels": pixels of one grid a workgroup of its passes takes
void set_color_fma(int on);        // color.hip "color_fma": fused squares in k_color_dist3 (default off: not bit-identical)
int set_color_chunk_scores(int v);  // color.hip "color_chunk_scores": most score elements per chunk of the needle loops, 0 (default) = 2^28 / 2^27 / 2^27; < 0: CBH_E_INVAL, knob unchanged
int get_color_chunk_scores();
long long get_color_full_sorts();   // "color_full_sorts": needles cbh_color_find_batch has sent through color_full_sort_one
long long get_color_window_cuts();  // "color_window_cuts": needles it has answered from the candidate list
int set_color_sort_table_kb(int v);  // color.hip "color_sort_table_kb": KiB of score tables one group of cbh_color_sort_similar may hold, 0 (default) = 2 GiB; < 0: CBH_E_INVAL
int get_color_sort_table_kb();
void set_color_sort_timing(int on);  // "color_sort_timing": 1 = cbh_color_sort_similar times its table fill and its chain with events
long long get_color_sort_stat(int which);  // 0 "color_sort_groups", 1 "color_sort_fill_us", 2 "color_sort_chain_us": the last call's
int set_cluster_chunk(int v);  // clusters.hip "cluster_chunk": needle nodes per scan of cbh_idx64_clusters, 1..2^25 (default 2^20); else CBH_E_INVAL
int get_cluster_chunk();
int set_cluster_max_records(int v);  // "cluster_max_records": records one of its scans may materialise (default 2^26); < 1: CBH_E_INVAL
int get_cluster_max_records();
void set_cluster_timing(int on);  // "cluster_timing": 1 = the cluster calls time their stages apart with events
long long get_cluster_stat(int which);  // 0 "cluster_table_us", 1 "cluster_hook_us", 2 "cluster_emit_us": the last call's
int set_vcover_chunk(int v);  // vcoverage.hip "vcover_chunk": destination entries per workgroup of cbh_video_coverage, 0 (default) = by the batch, 1..2^24; else CBH_E_INVAL
int get_vcover_chunk();
int set_vcover_tile(int v);  // "vcover_tile": source frames per workgroup, 256 / 512 / 1024 (default) / 2048; else CBH_E_INVAL
int get_vcover_tile();
int set_vseg_budget_mb(int v);  // vsegments.hip "vseg_budget_mb": what the difference arrays of one group of pairs of cbh_video_segments may take, 1..4096 (default 256); else CBH_E_INVAL
int get_vseg_budget_mb();

// ---- sortsimilar_table.hip: the -sort-similar chain over tables of scores -------------------------------------------
// A set of n items in ascending id order has its table as n rows of sort_table_row_stride(n) scores (16-byte rows, the
// padding is never a candidate); sort_table_layout gives every set's first score in one block (multiples of 8 from 0)
// and returns the block's size in scores (at least 8).
__host__ __device__ inline uint32_t sort_table_row_stride(uint32_t n) { return (n + 7u) & ~7u; }
uint64_t sort_table_layout(const uint64_t* h_first, size_t n_sets, uint64_t* h_sorted_first);
int sort_table_params_ok(const cbh_sort_table_params* p, const void* dir_id, const void* under_prefix);
// the chain alone: tables, ids, attributes (bit 0 in the index, bit 1 under the prefix) and dir ids already in ascending
// id order per set, item i of set s at d_first[s] - base + i; first_pos[s] = where the set's first item went;
// d_out_ids / d_out as cbh_sort_similar_dev.  d_sorted 16-byte aligned.
int launch_sort_table_chain(const uint16_t* d_sorted, const uint64_t* d_sorted_first, const uint32_t* s_id,
                            const uint8_t* s_attr, const uint32_t* s_dir, const uint32_t* first_pos, const uint64_t* d_first,
                            uint64_t base, size_t n_sets, uint32_t largest, const cbh_sort_table_params* p,
                            uint32_t* d_out_ids, cbh_sort_similar_result* d_out, hipStream_t s);

// ---- records.hip ----------------------------------------------------------------------
// Ascending u64 sort of n records in place (uses d_alt as the ping-pong buffer and d_tmp as
// scratch; sizes from sort_records_scratch_bytes).
size_t sort_records_scratch_bytes(size_t n);
int sort_keys64_db(unsigned long long* d_keys, unsigned long long* d_alt, size_t n, unsigned end_bit, void* d_tmp,
                   size_t tmp_bytes, hipStream_t stream, unsigned long long** sorted);  // any 64-bit keys, double buffer
int launch_sort_records(cbh_record* d_rec, cbh_record* d_alt, size_t n, size_t nq, void* d_tmp,
                        size_t tmp_bytes, hipStream_t stream);
int launch_select_records(const cbh_record* d_sorted, size_t n, size_t nq, int k, cbh_match* d_out,
                          uint32_t* d_counts, hipStream_t stream);
int launch_remove_ids(uint64_t* d_hashes, uint32_t* d_ids, size_t n, const uint32_t* d_sorted_rm,
                      size_t n_rm, hipStream_t stream, int zero_hash = 1);

// ---- topk.hip: K4 counting select over { count, records[cap] } blocks ---------------------------
constexpr int kTopkMaxK = 64;  // larger cuts take the radix sort (records.hip)
size_t topk_scratch_bytes(size_t nq, size_t total_cap);
int topk_scratch_init(void* d_scratch, size_t nq, hipStream_t stream);
int launch_records_group(const unsigned long long* d_blocks, unsigned nb, size_t stride, size_t cap, size_t nq,
                         unsigned* d_status, void* d_scratch, const unsigned** d_off, const unsigned long long** d_seg,
                         hipStream_t stream);
int launch_records_topk(const unsigned long long* d_blocks, unsigned nb, size_t stride, size_t cap, size_t nq, int k,
                        cbh_match* d_out, uint32_t* d_counts, unsigned* d_status, void* d_scratch,
                        hipStream_t stream);

// ---- slice.hip: Index::slice() on the device (row-range copy, planar gather) -------------------------------------
// 32-byte rows by ranges: d_table = 3 x (n_ranges + 1) words: packed firsts (from 0; the last = total_rows), dst firsts,
// src firsts
int launch_slice_rows256(const uint8_t* d_src, uint8_t* d_dst, const uint32_t* d_table, size_t n_ranges,
                         size_t total_rows, hipStream_t stream);
// entries d_pos[0..m) of the colour planes [32][src_cap] into entries 0..m of planes [32][dst_cap]; dst_cap is a
// multiple of 4 and entries m..dst_cap are written as padding (1e18 in L, no colours, id 0)
int launch_slice_color(const float* sL, const float* sU, const float* sV, const unsigned char* s_num,
                       const uint32_t* s_ids, size_t src_cap, const uint32_t* d_pos, size_t m, float* dL, float* dU,
                       float* dV, unsigned char* d_num, uint32_t* d_ids, size_t dst_cap, hipStream_t stream);
void note_slice_on_device();         // one more slice call succeeded on this route (with or without a launch) ...
long long get_slices_on_device();    // ... cbh_get_tuning "slices_on_device"

// ---- reduce.hip: K5 (fdct votes) and K8 (video closest-frame + adjacency) on the device ---------
struct cbh_nmatch {   // one DctFeaturesIndex result of needle image `needle`
  uint32_t needle, id;
  int32_t score;
};
struct cbh_nvmatch {  // one DctVideoIndex::findVideo result of needle video `needle`
  uint32_t needle;
  cbh_vmatch m;
};
int sort_keys_u64(unsigned long long* d_keys, size_t n, int end_bit, hipStream_t s);      // (records.hip: in place, arena scratch)
int sort_pairs_u64_u32(unsigned long long* d_keys, uint32_t* d_vals, size_t n, int end_bit, hipStream_t s);
int launch_fdct_vote(const cbh_match* d_top, const uint32_t* d_counts, const uint32_t* d_qneedle, size_t nq, int k,
                     const uint32_t* d_needle_id, size_t n_needles, std::vector<cbh_nmatch>* h_out, hipStream_t s);
int launch_video_reduce(const unsigned* d_off, const unsigned long long* d_seg, size_t total, size_t nq,
                        const uint32_t* d_egroup, const int32_t* d_eframe, const uint32_t* d_vmedia,
                        const uint32_t* d_qneedle, const int32_t* d_qframe, const uint32_t* d_needle_id, int filter_self,
                        int min_matched, int min_near, std::vector<cbh_nvmatch>* h_out, hipStream_t s);

// ---- frames.hip: K9, findFrame for a chunk of image needles (nearest frame per video, one sort, no host ordering) ----
// d_rec: `total` unordered scan records of `nq` needles, re-keyed and sorted between d_rec and d_alt (d_tmp / tmp_bytes: the
// sort's scratch, Workspace::ensure_sort); h_src_in: NULL or nq values.  h_out: one match per (needle, video) run, in
// (needle, video index) order; h_off[0 .. nq]: first run of every needle.  CBH_E_OVERFLOW for total >= 2^32.
int launch_frame_reduce(unsigned long long* d_rec, unsigned long long* d_alt, size_t total, size_t nq, void* d_tmp,
                        size_t tmp_bytes, const uint32_t* d_evidx, const int32_t* d_eframe, const uint32_t* d_vmedia,
                        const int32_t* h_src_in, std::vector<cbh_vmatch>* h_out, std::vector<uint32_t>* h_off,
                        hipStream_t s);

// ---- dcthash.hip (whole images), kphash.hip (rectangles, keypoint squares) -------------
// view: the images are w x h sub-rectangles at (ox, oy) of pw x ph parents starting at d_imgs -- cv::blur on a
// cv::Mat view takes its border pixels from the parent (dctHash64 after autocrop(), src/cvutil.cpp:1397-1401)
struct HashView {
  int pw, ph, ox, oy;
};
int launch_dcthash(const uint8_t* d_imgs, size_t n, int w, int h, size_t row_stride,
                   size_t img_stride, uint64_t* d_out, hipStream_t stream,
                   uint8_t* d_tiles = nullptr, const HashView* view = nullptr);
// The per-geometry steps of the callers that hash autocropped images (cbh_regions.h plans their launches).  rect: the
// kept region {left, top, right, bottom} that the n grey w x h images at d_gray share.
// dctHash64 of the kept VIEW: the blur sees the cropped-away margins (a view that is the whole image is none)
inline int launch_dcthash_kept(const uint8_t* d_gray, size_t n, int w, int h, size_t row_stride, size_t img_stride,
                               const int* rect, uint64_t* d_out, hipStream_t stream) {
  const HashView view{w, h, rect[0], rect[1]};
  return launch_dcthash(d_gray, n, rect[2] - rect[0], rect[3] - rect[1], row_stride, img_stride, d_out, stream, nullptr,
                        &view);
}
// prestage.hip: sizeLongestSide(kept region, size) packed at d_dst (a view: cv::resize does not look outside it).
// *dw x *dh: the size of each; 0 x 0 and nothing launched where the reference throws
int resize_kept(const uint8_t* d_gray, size_t n, size_t row_stride, size_t img_stride, const int* rect, int size,
                uint8_t* d_dst, int device, hipStream_t stream, int* dw, int* dh);
// prestage.hip: the kept regions of n grey images on the host (rects, n x 4), which has synchronised `stream` when they
// come from autocrop (range >= 0, through d_rects); range < 0: the whole frames
int fetch_kept_regions(const uint8_t* d_gray, size_t n, int w, int h, size_t row_stride, size_t img_stride, int range,
                       int* d_rects, int* rects, int device, hipStream_t stream);
// rectangles of images hashed one after the other, optionally in place (Media::makeKeyPointHashes); also the path of
// images with a side < 32
struct RectImageDesc {
  unsigned long long off;  // first byte of the image in the batch buffer
  int w, h;
  unsigned row_stride;
  unsigned first, count;   // its rectangles: rects[4*first .. 4*(first+count))
};
int launch_keypoint_hashes(uint8_t* d_base, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                           const uint32_t* img_h, const uint32_t* img_row_stride, const float* kp,
                           const uint32_t* kp_first, uint64_t* d_out, uint32_t* out_first, hipStream_t stream);
int launch_rect_hashes(uint8_t* d_base, const std::vector<RectImageDesc>& images, const std::vector<int>& rects,
                       int write_back, uint64_t* d_out, hipStream_t stream, uint8_t* d_tiles = nullptr);

// ---- orb.hip: ORB keypoints + rBRIEF descriptors (Media::makeKeyPoints / makeKeyPointDescriptors) ------------------
int orb_set_pattern(const int8_t* xy);
int launch_orb(const uint8_t* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
               const uint32_t* img_row_stride, int nfeatures, int kp_cap, cbh_keypoint* d_kp, float* d_kp_after,
               uint8_t* d_desc, uint32_t* d_counts, hipStream_t s);
int launch_orb_describe(const uint8_t* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                        const uint32_t* img_h, const uint32_t* img_row_stride, const cbh_keypoint* kp,
                        const uint32_t* kp_first, cbh_keypoint* out_kp, uint8_t* out_desc, uint32_t* out_first,
                        hipStream_t s);

// ---- tmpairs.hip: the kernels the grouped template match adds, launched from tmimages.hip and tmatch.hip ---------------
constexpr int kTmMatchBlock = 256;     // k_tm_match / k_tm_match_pairs: threads per block, one query row each
constexpr int kTmTrainPiece = 1024;    // ... and the train rows they stage in LDS at a time (32 KB)
struct TSet {                          // a candidate's train set: n rows from row `base` of the templates' descriptor rows
  unsigned base, n;
};
struct WImage;  // warp_px.h
struct PPatch;
// k_tm_match's launch (grid (tiles, m), candidates cand0 ..) with the train set per candidate
void launch_tm_match_pairs(bool emit, unsigned tiles, unsigned m, hipStream_t s, const uint8_t* d_train, const TSet* d_tsets,
                           const uint8_t* d_desc, const uint32_t* d_counts, unsigned kp_cap, unsigned max_dist, unsigned cand0,
                           unsigned* d_qcount, const unsigned* d_qoff, const unsigned long long* d_first,
                           unsigned long long base, unsigned g0, unsigned long long* d_keys, unsigned long long cap);
// grid (x, candidates): candidate blockIdx.y of the tables warps into its own patch / is masked by its own template
void launch_warp_ragged(int channels, dim3 grid, hipStream_t s, const uint8_t* d_imgs, const WImage* d_images,
                        const double* d_wm, const unsigned char* d_ok, const PPatch* d_patches, uint8_t* d_out);
void launch_tm_mask_ragged(dim3 grid, hipStream_t s, const uint8_t* d_patches, const uint8_t* d_tmpl_base,
                           const PPatch* d_tab, int channels, uint8_t* d_cand_gray, uint8_t* d_tmpl_gray);

// ---- tmatch.hip: estimate -> prepare -> ragged warp -> mask -> hashes -> records for candidates that each have their own
// template (the tail of tmimages.hip's grouped chain).  tg (host, n): candidate i's template, bytes at d_tmpl_base + off.
// res (host, n) is complete on return; *hash_launches (optional) is advanced by the launch_dcthash calls made.
struct TmplGeom {
  uint64_t off;
  uint32_t tw, th, stride;
};
int template_match_pairs_tail(const uint8_t* d_tmpl_base, const TmplGeom* tg, const uint8_t* d_imgs, size_t n,
                              const uint64_t* img_off, const uint32_t* img_w, const uint32_t* img_h,
                              const uint32_t* img_row_stride, int channels, const float* d_tmpl_xy, const float* d_match_xy,
                              const uint64_t* first, const float* cand_scale, cbh_template_result* res, unsigned* hash_launches,
                              hipStream_t s);

// ---- prestage.hip: the fixed-point Lanczos-4 tables of cv::resize (dsize offsets, dsize x 8 weights), built on the host --
void lanczos4_table(int ssize, int dsize, std::vector<int>* ofs, std::vector<short>* coef);

// ---- colordesc_create.hip: ColorDescriptor::create for a batch --------------------------------------------------
int launch_color_descriptors(const uint8_t* d_imgs, size_t n, const uint64_t* img_off, const uint32_t* img_w,
                             const uint32_t* img_h, const uint32_t* img_row_stride, int channels, uint8_t* d_descs,
                             uint8_t* d_ok, hipStream_t s);

}  // namespace cbh
