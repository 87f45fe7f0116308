// sharded.hip -- one index over several shards / several GPUs, inside ONE process, behind the same C-ABI handle.
//
// cbird is one process: Engine::Engine registers each Index once (src/engine.cpp:38-45) and Database::similar fans
// find() out from a thread pool (src/database.cpp:1400-1432).  A drop-in that wants all GPUs of the node therefore has
// to shard INSIDE the handle -- cbh_idx64_create_sharded(device_mask, shards_per_device) returns a cbh_idx64 that every
// other entry point accepts -- not in a torchrun harness (cbird_amd/dist.py keeps that form for bench.py --gpus N).
//
// Layout: the haystack is row-sharded, shard s of R owns the slots [s*n/R, (s+1)*n/R) of a load in load
// order (add() appends to the emptiest shard and the global order is kept as a segment list); needles are replicated.
// A threshold search over a union of shards is the union of the per-shard results, so there is exactly one sharded
// primitive: scan_all (cbh_index.h) -- "all records of these needles, in the root workspace's { count, records }
// block".  Everything above it (the K4 cut, fdct votes, video reduce, searchIndex escalation, the coalescer's self-join)
// runs unchanged on the root device over the merged block.
//
//   scan      in phases over one ShardRun per shard; sharded_scan_all is the loop that calls them:
//             plan       once per call.  The shards of the root device are DIRECT: they append straight into the root block
//                        through its one counter -- no block, count read-back, synchronisation or copy of their own --
//                        unless the exchange is the collective, whose send buffers are the devices' own blocks
//             launch     every shard that has to run scans on its own device and stream behind an event of the root stream;
//                        a shard that is not direct fills its own block { u64 count; records[cap] }
//             collect    the direct shards share one wait on the root stream and one read of its counter; any other shard
//                        synchronises and reads its own, and if its block overflowed it alone grows it and runs again
//             settle     a root block too small for the sum grows, and the direct shards run again
//             finish     statistics, the exchange below for the shards that are not direct, word 0 = total
//   exchange  ShardComm::exchange (cbh_shard.h; shared with the sharded CvFeaturesIndex, idx256.hip) --
//             inside a device: device-to-device copies of exactly count_s records behind each other;
//             between devices: ONE grouped ncclAllGather of the per-device blocks, sized to the fullest device
//             (1 + max count words) -- librccl called directly (ncclCommInitAll, one communicator per device, all
//             in this process), found with dlopen so that a single-GPU user never loads it;
//             "shard_exchange" = 1 replaces the collective by hipMemcpyPeerAsync straight into the root block
//   merge     the D gathered blocks are compacted into the root block; word 0 = total
//
// One GPU per box is all this pool offers, so the inter-device leg runs here with one rank ("shard_force_rccl" = 1:
// a one-device index still goes through ncclAllGather), and everything else -- ragged shards, overflow-redo, removal,
// order of a merged result -- with R logical shards on one device (tests/test_sharded_capi.py, tests/cpp).
#include <dlfcn.h>
#include <rccl/rccl.h>

#include "cbh_index.h"

namespace cbh {

namespace {

struct Rccl {
  void* handle = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*GetVersion)(int*) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string why;  // when it could not be loaded
};

// librccl.so.1: the copy already mapped in this process if there is one (PyTorch ships its own), else the system's
Rccl* rccl() {
  static Rccl* r = [] {
    Rccl* x = new Rccl;
    for (const char* name : {"librccl.so.1", "librccl.so"}) {
      x->handle = dlopen(name, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
      if (x->handle) break;
    }
    if (!x->handle)
      for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        x->handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (x->handle) break;
      }
    if (!x->handle) {
      const char* e = dlerror();
      x->why = e ? e : "librccl not found";
      return x;
    }
#define CBH_SYM(field, name)                                         \
  x->field = reinterpret_cast<decltype(x->field)>(dlsym(x->handle, name)); \
  if (!x->field) x->why = std::string("librccl lacks ") + name
    CBH_SYM(CommInitAll, "ncclCommInitAll");
    CBH_SYM(CommDestroy, "ncclCommDestroy");
    CBH_SYM(AllGather, "ncclAllGather");
    CBH_SYM(GroupStart, "ncclGroupStart");
    CBH_SYM(GroupEnd, "ncclGroupEnd");
    CBH_SYM(GetErrorString, "ncclGetErrorString");
    CBH_SYM(GetVersion, "ncclGetVersion");
#undef CBH_SYM
    // the copy found may be the one another library of this process brought along (PyTorch ships its own): use it only
    // when it is the API generation this file was compiled against (same major version as <rccl/rccl.h>)
    int v = 0;
    if (x->why.empty() && (x->GetVersion(&v) != ncclSuccess || v / 10000 != NCCL_VERSION_CODE / 10000))
      x->why = "librccl version " + std::to_string(v) + " does not match the headers (" + std::to_string(NCCL_VERSION_CODE) + ")";
    return x;
  }();
  return r;
}

int g_force_rccl = 0;  // "shard_force_rccl": the collective also at one device (transport test on a one-GPU box)
// "shard_exchange": 1 = copies of exactly count_s records into the root block (default: only the root device consumes
// the records, an all-gather would put D times the bytes on the links), 0 = grouped ncclAllGather of the device blocks
int g_exchange = 1;
int g_fault_rccl = 0;  // "fault_rccl": librccl treated as absent

int ensure_comms(ShardComm* C) {  // under coll_mu
  if (!C->comms.empty()) return CBH_OK;
  if (C->comms_tried) return CBH_E_UNSUPPORTED;
  C->comms_tried = true;
  if (g_fault_rccl) {
    set_last_error_text("RCCL unavailable: fault_rccl");
    return CBH_E_UNSUPPORTED;
  }
  Rccl* r = rccl();
  if (!r->handle || !r->why.empty()) {
    set_last_error_text(("RCCL unavailable: " + r->why).c_str());
    return CBH_E_UNSUPPORTED;
  }
  std::vector<ncclComm_t> c(C->devices.size());
  ncclResult_t e = r->CommInitAll(c.data(), (int)C->devices.size(), C->devices.data());
  if (e != ncclSuccess) {
    set_last_error_text((std::string("ncclCommInitAll: ") + r->GetErrorString(e)).c_str());
    return CBH_E_HIP;
  }
  for (ncclComm_t x : c) C->comms.push_back((void*)x);
  return CBH_OK;
}

}  // namespace

void set_shard_force_rccl(int v) { g_force_rccl = v; }
void set_shard_exchange(int v) { g_exchange = v; }
void set_fault_rccl(int v) { g_fault_rccl = v; }

bool ShardComm::init(uint32_t device_mask, int shards_per_device) {
  if (device_mask == 0 || shards_per_device < 0 || shards_per_device > 64) return false;
  devices.clear();
  for (int d = 0; d < 32; ++d)
    if (device_mask & (1u << d)) {
      if (!device_usable(d)) return false;  // a device of the mask is not there: no silent narrowing
      devices.push_back(d);
    }
  per_device = std::max(1, shards_per_device);
  mask = device_mask;
  // direct xGMI copies where the platform allows them (RCCL opens its own).  A refusal is not an error: only copies
  // cross devices (no kernel dereferences a peer pointer), and hipMemcpyPeerAsync stages through the host without it.
  if (devices.size() > 1)
    for (int a : devices) {
      DeviceGuard g(a);
      for (int b : devices)
        if (a != b) {
          int can = 0;
          if (hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(b, 0);
        }
      (void)hipGetLastError();  // "already enabled" is not an error worth keeping
    }
  return true;
}

void ShardComm::destroy_comms() {
  if (comms.empty()) return;
  Rccl* r = rccl();
  for (size_t d = 0; d < comms.size(); ++d) {
    DeviceGuard g(devices[d]);
    (void)r->CommDestroy((ncclComm_t)comms[d]);
  }
  comms.clear();
}

int ShardComm::exchange(std::vector<ShardPart>& parts, hipStream_t root_stream, unsigned long long* d_dst,
                        bool* went_collective, unsigned long long root_prefilled) {
  const size_t R = parts.size(), D = devices.size();
  const int root = devices[0];
  bool collective = g_exchange == 0 && (D > 1 || g_force_rccl);
  if (collective) {
    // no communicator (librccl absent or of another generation, ncclCommInitAll refused): the copies below give the
    // same block; said once per index in cbh_last_error and on stderr, counted in cbh_shard_stats.collective_fallbacks
    std::lock_guard<std::mutex> lk(coll_mu);
    if (ensure_comms(this) != CBH_OK) {
      collective = false;
      if (!n_fallbacks.fetch_add(1))
        fprintf(stderr, "cbird_hip: sharded index exchanges by device copies, not ncclAllGather (%s)\n", cbh_last_error());
      set_last_error_code(CBH_OK);  // absorbed: the note stays in cbh_last_error, the call has not failed
    }
  }
  // per-device totals, the place of every shard inside its device's run, and of every device in the destination
  std::vector<unsigned long long> dev_total(D, 0), shard_off(R, 0), dev_off(D, 0);
  dev_total[0] = root_prefilled;  // (copies only: records the root device's shards appended in place, ahead of everything)
  for (size_t s = 0; s < R; ++s) {
    shard_off[s] = dev_total[(size_t)parts[s].dev_pos];
    dev_total[(size_t)parts[s].dev_pos] += parts[s].count;
  }
  for (size_t d = 1; d < D; ++d) dev_off[d] = dev_off[d - 1] + dev_total[d - 1];
  std::vector<size_t> first_of(D, R);  // first shard of a device: its stream carries the device's part of a collective
  for (size_t s = R; s-- > 0;) first_of[(size_t)parts[s].dev_pos] = s;
  int rc;
  if (went_collective) *went_collective = collective;
  if (!collective) {
    // every shard copies exactly its records to their final place on the root device
    for (size_t s = 0; s < R; ++s) {
      ShardPart& P = parts[s];
      if (!P.count) continue;
      const int dev = devices[(size_t)P.dev_pos];
      DeviceGuard g(dev);
      if (!g.ok) return CBH_E_NODEVICE;
      unsigned long long* dst = d_dst + dev_off[(size_t)P.dev_pos] + shard_off[s];
      if (dev == root) {
        CBH_HIP(hipMemcpyAsync(dst, P.d_rec, P.count * 8, hipMemcpyDeviceToDevice, P.stream));
        n_local_copies++;
      } else {
        CBH_HIP(hipMemcpyPeerAsync(dst, root, P.d_rec, dev, P.count * 8, P.stream));
        n_peer_copies++;
      }
      CBH_HIP(hipEventRecord(P.ev, P.stream));
    }
    DeviceGuard g(root);
    for (size_t s = 0; s < R; ++s)
      if (parts[s].count) CBH_HIP(hipStreamWaitEvent(root_stream, parts[s].ev, 0));
    return CBH_OK;
  }
  unsigned long long m = 0;
  for (size_t d = 0; d < D; ++d) m = std::max(m, dev_total[d]);
  const size_t words = 1 + (size_t)m;
  std::vector<const void*> send(D, nullptr);
  std::vector<void*> recv(D, nullptr);
  for (size_t d = 0; d < D; ++d) {
    const size_t f = first_of[d];
    if (f == R) return CBH_E_INVAL;  // a device without a shard
    ShardPart& F = parts[f];
    DeviceGuard g(devices[d]);
    if (!g.ok) return CBH_E_NODEVICE;
    if ((rc = F.x[1].ensure(D * words * 8))) return rc;
    recv[d] = F.x[1].p;
    if (per_device == 1 && F.own_block && F.own_cap + 1 >= words) {
      send[d] = F.own_block;  // a single shard's block is the device block as it stands: word 0 = count (written by
      continue;               // the scan kernel), and it is at least `words` long
    }
    if ((rc = F.x[0].ensure(words * 8))) return rc;
    unsigned long long* B = (unsigned long long*)F.x[0].p;
    send[d] = B;
    *F.h_word = dev_total[d];
    CBH_HIP(hipMemcpyAsync(B, F.h_word, 8, hipMemcpyHostToDevice, F.stream));
    for (size_t s = 0; s < R; ++s) {
      ShardPart& P = parts[s];
      if ((size_t)P.dev_pos != d || !P.count) continue;
      CBH_HIP(hipMemcpyAsync(B + 1 + shard_off[s], P.d_rec, P.count * 8, hipMemcpyDeviceToDevice, P.stream));
      n_local_copies++;
      if (s != f) {
        CBH_HIP(hipEventRecord(P.ev, P.stream));
        CBH_HIP(hipStreamWaitEvent(F.stream, P.ev, 0));
      }
    }
  }
  {
    std::lock_guard<std::mutex> lk(coll_mu);
    if (comms.empty()) return CBH_E_UNSUPPORTED;  // (destroyed under our feet: an index being torn down)
    Rccl* r = rccl();
    ncclResult_t e = r->GroupStart();
    for (size_t d = 0; d < D && e == ncclSuccess; ++d) {
      DeviceGuard g(devices[d]);
      e = r->AllGather(send[d], recv[d], words, ncclUint64, (ncclComm_t)comms[d], parts[first_of[d]].stream);
    }
    ncclResult_t e2 = r->GroupEnd();
    if (e == ncclSuccess) e = e2;
    if (e != ncclSuccess) {
      set_last_error_text((std::string("ncclAllGather: ") + r->GetErrorString(e)).c_str());
      return CBH_E_HIP;
    }
    n_collectives++;
  }
  DeviceGuard g(root);
  ShardPart& Rt = parts[first_of[0]];
  const unsigned long long* G = (const unsigned long long*)Rt.x[1].p;
  for (size_t d = 0; d < D; ++d)
    if (dev_total[d])
      CBH_HIP(hipMemcpyAsync(d_dst + dev_off[d], G + d * words + 1, dev_total[d] * 8, hipMemcpyDeviceToDevice, Rt.stream));
  CBH_HIP(hipEventRecord(Rt.ev, Rt.stream));
  CBH_HIP(hipStreamWaitEvent(root_stream, Rt.ev, 0));
  return CBH_OK;
}

struct ShardSet {
  ShardComm comm;
  std::vector<cbh_idx64*> child;  // plain single-device indexes; child[s]->device == comm.device_of_shard(s)
  // global slot order: segment g covers parent slots [global, global+len) = child[shard] slots [local, local+len)
  struct Seg {
    uint32_t shard;
    size_t local, global, len;
  };
  std::vector<Seg> segs;
};

void shardset_free(ShardSet* S) {
  if (!S) return;
  S->comm.destroy_comms();
  for (cbh_idx64* c : S->child) cbh_idx64_destroy(c);
  delete S;
}

namespace {

constexpr size_t kKeepXBufBytes = (size_t)64 << 20;  // exchange buffers above this go back after the call
constexpr size_t kKeepShardRecs = (size_t)1 << 22;   // a shard's record block above this (32 MB) likewise

// One shard for the length of one call.  `drained`: nothing this call put on the shard's stream can still be running.  Two
// operations touch it: work(), through which every enqueue goes, clears it; saw_drained(), where the host saw that, sets it.
struct ShardRun {
  cbh_idx64* c = nullptr;        // the child index
  Workspace* ws = nullptr;       // leased from it
  bool direct = false;           // lives on the root device: appends into the root block through the root counter
  bool todo = false;             // has to scan in the next round (a lone find: launched, not yet collected)
  unsigned long long count = 0;  // records in its own block (the direct shards' are ScanCall::direct_count)
  const uint64_t *q = nullptr, *qmask = nullptr;  // needles and masks on its own device
  bool drained = true;           // (a workspace is idle when it is leased)
  std::shared_ptr<const JoinTables> join_hold;  // the join tables its launch read: let go with the lease, behind the stream
  hipStream_t work() { return drained = false, ws->stream; }
  void saw_drained() { drained = true; }
};

// what one call holds: a workspace per shard, and the needles expanded for the root device's shards (scans only)
struct ShardLeases {
  std::vector<ShardRun> run;
  uint4* qx_root = nullptr;  // the shards read it on their own streams; allocated on the root stream
  JoinNeedles jn_root;       // likewise the join's needle side (join_prepare_needles); m == 0: none
  hipStream_t root_stream;
  int root;
  ShardLeases(cbh_idx64* idx, hipStream_t st) : run(idx->shards->child.size()), root_stream(st), root(idx->device) {
    for (size_t s = 0; s < run.size(); ++s) run[s].c = idx->shards->child[s];
  }
  int acquire_all() {
    for (ShardRun& r : run) {
      DeviceGuard g(r.c->device);
      if (!g.ok) return CBH_E_NODEVICE;
      int rc = CBH_OK;
      r.ws = r.c->acquire(&rc);
      if (!r.ws) return rc ? rc : CBH_E_NOMEM;
    }
    return CBH_OK;
  }
  // In this order: every shard stream not known drained is synchronised, so that its workspace, shrunk, goes back idle to
  // its pool; only then qx_root, which those streams may have been reading, is freed on the root stream.  (On the paths
  // that succeed the root stream has waited for the shards and nothing is synchronised here.)
  ~ShardLeases() {
    for (ShardRun& r : run)
      if (r.ws) {
        DeviceGuard g(r.c->device);
        // (6.5 us per synchronisation even on a drained stream: a lone find() on 8 shards spent 52 of its 230 us here)
        if (!r.drained) (void)hipStreamSynchronize(r.ws->stream);
        // one large result (a self-join attempt) must not leave every shard holding a block of that size for good
        r.ws->shrink_records(std::max<size_t>(r.c->rec_cap_default, kKeepShardRecs));
        for (XBuf& x : r.ws->x)
          if (x.bytes > kKeepXBufBytes) x.release();
        r.c->give_back(r.ws);
      }
    if (qx_root || jn_root.m) {
      DeviceGuard g(root);
      if (qx_root) (void)free_async(qx_root, root_stream);
      jn_root.free();
    }
  }
};

// the arguments of one sharded_scan_all, what plan_scan decides once for it, and the tallies of its rounds
struct ScanCall {
  cbh_idx64* idx;
  Workspace* ws;  // the root workspace: the merged block ends up in it
  const uint64_t* d_q;
  size_t nq, max_records;
  int thresh;
  hipStream_t stream;
  unsigned long long* total;
  ScanOpts opts;  // the caller's; plan_scan adds the siblings and the prefilter choice
  ShardLeases L;
  ShardComm& C;  // (an aggregate: sharded_scan_all fills it down to here)
  bool timed = false, any_direct = false;
  unsigned long long direct_count = 0;  // records the direct shards have appended to the root block
  float scan_ms = 0.f;
  bool pending(bool direct_only = false) const {
    return std::any_of(L.run.begin(), L.run.end(), [=](const ShardRun& r) { return r.todo && (r.direct || !direct_only); });
  }
  unsigned long long sum() const {  // as far as the shards have reported
    unsigned long long t = direct_count;
    for (const ShardRun& r : L.run) t += r.count;
    return t;
  }
};

// plan: what is decided once per call
int plan_scan(ScanCall& K) {
  const bool collective = g_exchange == 0 && (K.C.devices.size() > 1 || g_force_rccl);
  for (ShardRun& r : K.L.run) {
    r.todo = r.c->n != 0;
    r.direct = !collective && r.todo && r.c->device == K.L.root;
    K.any_direct = K.any_direct || r.direct;
    r.q = K.d_q, r.qmask = K.opts.d_qmask;
  }
  // kernel timing (cbh_idx64_get_stats) only where it can matter: a handful of needles is launch-bound, every HIP call counts
  K.timed = K.nq >= 256;
  // prefilter or three-field kernel: one probe for the whole call, on the slots of a shard that lives where the needles
  // are (every shard probing for itself cost a stream synchronisation per shard and threshold); and ONE expansion of the
  // needles into the matrix-core operand layout for all the shards of the root device (80 bytes per padded needle)
  K.opts.siblings = (unsigned)K.C.per_device;
  // the bucketed join at thresholds 5..8 on shards that keep their slot tables: ONE needle side (histogram, starts, the
  // chunk-ordered copies) for all the shards of the root device, which then run their jobs kernel and their joins only.
  // No memory for it: every shard prepares its own, as a handle that keeps no tables does.
  for (const ShardRun& r : K.L.run)
    if (r.c->device == K.L.root && r.c->n != 0 && K.thresh >= 5 && r.c->join.enabled() &&
        scan_routes_to_join(r.c->n, K.nq, K.thresh, K.opts.d_qmask != nullptr)) {
      DeviceGuard g(K.L.root);
      const int rc = join_prepare_needles(K.d_q, K.nq, K.thresh, K.stream, &K.L.jn_root);
      if (rc == CBH_E_NOMEM) {
        K.L.jn_root.m = 0;
        cbh_clear_error();
      } else if (rc) {
        K.L.jn_root.m = 0;
        return rc;
      }
      break;
    }
  for (const ShardRun& r : K.L.run)
    if (r.c->device == K.L.root && r.c->n != 0 && scan_takes_mfma(r.c->n, K.nq, K.thresh)) {
      DeviceGuard g(K.L.root);
      K.opts.pre = scan_pick_pre(r.c->d_hashes, r.c->n, K.idx->n, K.d_q, K.nq, K.thresh, K.stream);
      return expand_needles_for_scan(K.d_q, K.nq, K.stream, &K.L.qx_root);
    }
  return CBH_OK;
}

// launch a round
int launch_round(ScanCall& K, int attempt) {
  const bool direct_now = K.pending(true);
  DeviceGuard on_root(K.L.root);
  if (direct_now) CBH_HIP(hipMemsetAsync(K.ws->d_total, 0, sizeof(unsigned long long), K.stream));
  // the needles (and masks, the expansion, the zeroed counter) are complete on the root device
  if (attempt == 0 || direct_now) CBH_HIP(hipEventRecord(K.ws->ev0, K.stream));
  for (ShardRun& r : K.L.run) {
    if (!r.todo) continue;
    cbh_idx64* c = r.c;
    Workspace* cw = r.ws;
    DeviceGuard g(c->device);
    if (!g.ok) return CBH_E_NODEVICE;
    hipStream_t cs = r.work();
    int rc;
    if (attempt == 0 || r.direct) CBH_HIP(hipStreamWaitEvent(cs, K.ws->ev0, 0));
    if (attempt == 0) {         // the shard's first run
      if (c->device != K.L.root) {  // replicate the needles: one peer copy per shard and call (8 B per needle)
        if ((rc = Workspace::grow(&cw->d_q, &cw->q_cap, K.nq))) return rc;
        CBH_HIP(hipMemcpyPeerAsync(cw->d_q, c->device, K.d_q, K.L.root, K.nq * sizeof(uint64_t), cs));
        r.q = cw->d_q;
        if (r.qmask) {
          if ((rc = Workspace::grow(&cw->d_qmask, &cw->qmask_cap, K.nq))) return rc;
          CBH_HIP(hipMemcpyPeerAsync(cw->d_qmask, c->device, r.qmask, K.L.root, K.nq * sizeof(uint64_t), cs));
          r.qmask = cw->d_qmask;
        }
        K.C.n_peer_copies++;
      }
      if (!r.direct && (rc = cw->ensure_records(std::max<size_t>(c->rec_cap_default, 1024)))) return rc;
    }
    if (!r.direct) CBH_HIP(hipMemsetAsync(cw->d_total, 0, sizeof(unsigned long long), cs));
    if (K.timed) CBH_HIP(hipEventRecord(cw->ev0, cs));
    Workspace* into = r.direct ? K.ws : cw;
    ScanOpts o = K.opts;
    o.d_qmask = r.qmask;
    o.qx = c->device == K.L.root ? K.L.qx_root : nullptr;
    o.join = &c->join, o.join_hold = &r.join_hold;
    o.join_needles = c->device == K.L.root && K.L.jn_root.m ? &K.L.jn_root : nullptr;
    rc = launch_hamm64_scan(c->d_hashes, c->d_ids, c->n, r.q, K.nq, K.thresh, into->d_rec, into->rec_cap, into->d_total, cs, o);
    if (rc) return rc;
    if (K.timed || r.direct) CBH_HIP(hipEventRecord(cw->ev1, cs));
    if (!r.direct)
      CBH_HIP(hipMemcpyAsync(cw->h_total, cw->d_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, cs));
    K.C.n_scans++;
    if (attempt) K.C.n_rescans++;
  }
  return CBH_OK;
}

// collect a round; *worst = the slowest kernel of the round
int collect_round(ScanCall& K, float* worst) {
  float ms = 0.f;
  if (K.pending(true)) {
    DeviceGuard g(K.L.root);
    for (const ShardRun& r : K.L.run)
      if (r.todo && r.direct) CBH_HIP(hipStreamWaitEvent(K.stream, r.ws->ev1, 0));
    CBH_HIP(hipMemcpyAsync(K.ws->h_total, K.ws->d_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, K.stream));
    CBH_HIP(hipStreamSynchronize(K.stream));
    K.direct_count = *K.ws->h_total;
    for (ShardRun& r : K.L.run) {
      if (!r.todo || !r.direct) continue;
      if (K.timed && hipEventElapsedTime(&ms, r.ws->ev0, r.ws->ev1) == hipSuccess) *worst = std::max(*worst, ms);
      r.todo = false;
      r.saw_drained();  // its stream's last operation is the event the root stream waited for, and that stream is drained
    }
  }
  for (ShardRun& r : K.L.run) {
    if (!r.todo) continue;
    Workspace* cw = r.ws;
    DeviceGuard g(r.c->device);
    CBH_HIP(hipStreamSynchronize(cw->stream));
    r.saw_drained();
    r.count = *cw->h_total;
    if (K.timed && hipEventElapsedTime(&ms, cw->ev0, cw->ev1) == hipSuccess) *worst = std::max(*worst, ms);
    r.todo = false;
    if (r.count > cw->rec_cap) {
      if (K.sum() > K.max_records && K.sum() > K.ws->rec_cap) {  // the merged result cannot fit anyway
        *K.total = K.sum();
        return CBH_E_OVERFLOW;
      }
      if (int rc = grow_for_result(cw, r.count)) return rc;
      r.todo = true;
    }
  }
  return CBH_OK;
}

// settle the root block, once every shard has reported
int settle_root_block(ScanCall& K) {
  const unsigned long long sum = K.sum();
  if (sum <= K.ws->rec_cap) return CBH_OK;
  *K.total = sum;
  if (sum > K.max_records) return CBH_E_OVERFLOW;  // nobody grows for it
  DeviceGuard g(K.L.root);
  CBH_HIP(hipStreamSynchronize(K.stream));
  if (int rc = grow_for_result(K.ws, sum)) return rc;  // (a new block: what the direct shards appended is gone)
  for (ShardRun& r : K.L.run) r.todo = r.direct;
  K.direct_count = 0;
  return CBH_OK;
}

// finish
int finish_scan(ScanCall& K) {
  count_scan(K.idx, K.nq, K.scan_ms);
  const unsigned long long sum = K.sum(), remote = sum - K.direct_count;
  *K.total = sum;
  if (sum > K.ws->rec_cap) return CBH_E_OVERFLOW;
  // all of it is in place, the counter holds the sum, and every shard that ran has been seen drained
  if (!remote && K.any_direct) return CBH_OK;
  std::vector<ShardPart> parts(K.L.run.size());
  for (size_t s = 0; s < parts.size(); ++s) {
    ShardRun& r = K.L.run[s];
    Workspace* w = r.ws;  // (its d_total heads the shard's own block { count, records[rec_cap] })
    parts[s] = ShardPart{K.C.dev_pos_of_shard(s), r.work(), reinterpret_cast<const unsigned long long*>(w->d_rec), r.count,
                         w->d_total, w->rec_cap, w->ev1, w->x, w->h_total};
  }
  bool by_collective = true;
  int rc = K.C.exchange(parts, K.stream, reinterpret_cast<unsigned long long*>(K.ws->d_rec), &by_collective, K.direct_count);
  if (rc) return rc;
  DeviceGuard g(K.L.root);
  *K.ws->h_total = sum;
  CBH_HIP(hipMemcpyAsync(K.ws->d_total, K.ws->h_total, sizeof(unsigned long long), hipMemcpyHostToDevice, K.stream));
  CBH_HIP(hipStreamSynchronize(K.stream));  // scan_all's contract: the block is complete on return
  // Copies: a shard stream's last operation is its record copy + event, which `stream` waited for before the synchronisation
  // just done.  (A collective may leave the peers' halves of the all-gather in flight: synchronised when the leases end.)
  if (!by_collective)
    for (ShardRun& r : K.L.run) r.saw_drained();
  return CBH_OK;
}

}  // namespace

int sharded_scan_all(cbh_idx64* idx, Workspace* ws, const uint64_t* d_q, size_t nq, int thresh, hipStream_t stream,
                     unsigned long long* total, const ScanOpts& opts, size_t max_records) {
  *total = 0;
  // the root block must exist whatever happens (consumers read word 0)
  int rc = ws->ensure_records(first_record_block(idx, max_records));
  if (rc) return rc;
  if (nq == 0 || idx->n == 0 || thresh <= 0) {
    CBH_HIP(hipMemsetAsync(ws->d_total, 0, sizeof(unsigned long long), stream));
    CBH_HIP(hipStreamSynchronize(stream));
    return CBH_OK;
  }
  ScanCall K{idx, ws, d_q, nq, max_records, thresh, stream, total, opts, ShardLeases(idx, stream), idx->shards->comm};
  if ((rc = K.L.acquire_all()) || (rc = plan_scan(K))) return rc;
  for (int attempt = 0; attempt < 4 && K.pending(); ++attempt) {
    float worst = 0.f;
    if ((rc = launch_round(K, attempt)) || (rc = collect_round(K, &worst))) return rc;
    K.scan_ms += worst;  // the shards run side by side: a round costs what its slowest shard costs
    if (!K.pending() && (rc = settle_root_block(K))) return rc;
  }
  return K.pending() ? CBH_E_OVERFLOW : finish_scan(K);
}

// The lone needle on a sharded handle (cbh_idx64_find): one launch_find_one per shard, issued back to back from this thread,
// then one poll per shard -- no needle copies, no event waits, no counter resets, no read-backs, no stream synchronisation
// (what made a find() on 8 shards cost 203 us against 26 on the plain index).  *fits = every shard's matches fitted its
// LoneBlock (then *recs holds them all, unordered); otherwise the caller takes the general path.
int sharded_find_one(cbh_idx64* idx, uint64_t q, int thresh, std::vector<cbh_record>* recs, bool* fits) {
  *fits = false;
  recs->clear();
  ShardLeases L(idx, nullptr);
  int rc = L.acquire_all();
  if (rc) return rc;
  for (ShardRun& r : L.run) {
    if (r.c->n == 0) continue;
    DeviceGuard g(r.c->device);
    if (!g.ok) return CBH_E_NODEVICE;
    Workspace* cw = r.ws;
    hipStream_t cs = r.work();  // (ensure_lone's first call already puts a memset there)
    if ((rc = cw->ensure_lone())) return rc;
    rc = launch_find_one(r.c->d_hashes, r.c->d_ids, r.c->n, q, thresh, cw->d_lone, cw->h_lone, ++cw->lone_seq, cs);
    if (rc) return rc;
    r.todo = true;
    idx->shards->comm.n_scans++;
  }
  bool all_fit = true;
  for (ShardRun& r : L.run) {
    if (!r.todo) continue;
    Workspace* cw = r.ws;  // (leased to this call alone: lone_seq is still this call's number)
    DeviceGuard g(r.c->device);
    if ((rc = wait_find_one(cw->h_lone, cw->lone_seq, cw->stream))) return rc;
    r.saw_drained();  // its kernel has published its result: nothing of this call is left on the stream
    const unsigned long long t = cw->h_lone->count;
    if (t > LoneBlock::kRecs) all_fit = false;
    else if (all_fit) recs->insert(recs->end(), cw->h_lone->recs, cw->h_lone->recs + t);
  }
  *fits = all_fit;
  if (!all_fit) recs->clear();
  return CBH_OK;
}

int sharded_download(const cbh_idx64* idx, uint64_t* hashes, uint32_t* ids, size_t cap) {
  const ShardSet* S = idx->shards;
  for (const ShardSet::Seg& g : S->segs) {
    if (g.global >= cap) continue;
    const size_t m = std::min(g.len, cap - g.global);
    const cbh_idx64* c = S->child[g.shard];
    DeviceGuard dg(c->device);
    if (!dg.ok) return CBH_E_NODEVICE;
    if (hashes) CBH_HIP(hipMemcpy(hashes + g.global, c->d_hashes + g.local, m * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (ids) CBH_HIP(hipMemcpy(ids + g.global, c->d_ids + g.local, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  return CBH_OK;
}

int sharded_gather_dev(const cbh_idx64* idx, uint64_t* d_hashes, uint32_t* d_ids, hipStream_t stream) {
  const ShardSet* S = idx->shards;
  bool drained = false;
  for (const ShardSet::Seg& g : S->segs) {
    const cbh_idx64* c = S->child[g.shard];
    if (c->device == idx->device) {
      CBH_HIP(hipMemcpyAsync(d_hashes + g.global, c->d_hashes + g.local, g.len * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
      CBH_HIP(hipMemcpyAsync(d_ids + g.global, c->d_ids + g.local, g.len * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    } else {
      // (the copy does not run on `stream`: whatever `stream` still does with the destination blocks comes first)
      if (!drained) CBH_HIP(hipStreamSynchronize(stream));
      drained = true;
      CBH_HIP(hipMemcpyPeer(d_hashes + g.global, idx->device, c->d_hashes + g.local, c->device, g.len * sizeof(uint64_t)));
      CBH_HIP(hipMemcpyPeer(d_ids + g.global, idx->device, c->d_ids + g.local, c->device, g.len * sizeof(uint32_t)));
    }
  }
  return CBH_OK;
}

// load: shard s of R takes [s*n/R, (s+1)*n/R) (cbird_amd/dist.py shard_range); src on the host, or on the
// root device (load_dev)
int sharded_load(cbh_idx64* idx, const void* hashes, const void* ids, size_t n, bool on_device, hipStream_t stream) {
  ShardSet* S = idx->shards;
  const size_t R = S->child.size();
  S->segs.clear();
  idx->n = 0;
  if (n && (!hashes || !ids)) return CBH_E_INVAL;
  if (n > 0xfffffff0ull) return CBH_E_INVAL;
  if (on_device && stream) CBH_HIP(hipStreamSynchronize(stream));  // the source arrays are complete
  for (size_t s = 0; s < R; ++s) {
    const size_t a = s * n / R, b = (s + 1) * n / R;
    cbh_idx64* c = S->child[s];
    const uint64_t* h = (const uint64_t*)hashes + a;
    const uint32_t* i = (const uint32_t*)ids + a;
    int rc;
    if (!on_device) {
      rc = cbh_idx64_load(c, h, i, b - a);
    } else if (c->device == idx->device) {
      rc = cbh_idx64_load_dev(c, h, i, b - a, nullptr);
    } else {
      DeviceGuard g(c->device);
      if (!g.ok) return CBH_E_NODEVICE;
      c->n = 0;
      c->contents_changed();
      c->loaded = true;
      rc = c->reserve(b - a);
      if (!rc && b > a) {
        CBH_HIP(hipMemcpyPeer(c->d_hashes, c->device, h, idx->device, (b - a) * sizeof(uint64_t)));
        CBH_HIP(hipMemcpyPeer(c->d_ids, c->device, i, idx->device, (b - a) * sizeof(uint32_t)));
        c->n = b - a;
      }
    }
    if (rc) return rc;
    if (b > a) S->segs.push_back(ShardSet::Seg{(uint32_t)s, 0, a, b - a});
  }
  idx->n = n;
  return CBH_OK;
}

// add(): the reference appends and rebuilds its tree (src/dcthashindex.cpp:158-173); here the batch goes to the shard
// that holds the fewest slots, the parent's slot order continues
int sharded_add(cbh_idx64* idx, const uint64_t* hashes, const uint32_t* ids, size_t n) {
  ShardSet* S = idx->shards;
  if (n == 0) return CBH_OK;
  if (!hashes || !ids) return CBH_E_INVAL;
  if (idx->n + n > 0xfffffff0ull) return CBH_E_INVAL;
  size_t best = 0;
  for (size_t s = 1; s < S->child.size(); ++s)
    if (S->child[s]->n < S->child[best]->n) best = s;
  cbh_idx64* c = S->child[best];
  const size_t local = c->n;
  int rc = c->loaded ? cbh_idx64_add(c, hashes, ids, n) : cbh_idx64_load(c, hashes, ids, n);
  if (rc) return rc;
  if (!S->segs.empty() && S->segs.back().shard == best && S->segs.back().local + S->segs.back().len == local &&
      S->segs.back().global + S->segs.back().len == idx->n)
    S->segs.back().len += n;
  else
    S->segs.push_back(ShardSet::Seg{(uint32_t)best, local, idx->n, n});
  idx->n += n;
  return CBH_OK;
}

int sharded_remove(cbh_idx64* idx, const uint32_t* ids, size_t n, int zero_hash) {
  for (cbh_idx64* c : idx->shards->child) {
    int rc = zero_hash ? cbh_idx64_remove(c, ids, n) : cbh_idx64_remove_ids_only(c, ids, n);
    if (rc) return rc;
  }
  return CBH_OK;
}

}  // namespace cbh

extern "C" {

cbh_idx64* cbh_idx64_create_sharded(uint32_t device_mask, int shards_per_device) {
  clear_last_error();
  cbh_idx64* idx = new (std::nothrow) cbh_idx64;
  ShardSet* S = new (std::nothrow) ShardSet;
  if (!idx || !S) {
    delete idx;
    delete S;
    return (cbh_idx64*)fail_handle(CBH_E_NOMEM, "cbh_idx64_create_sharded: host allocation failed");
  }
  if (!S->comm.init(device_mask, shards_per_device)) {
    delete idx;
    delete S;
    return (cbh_idx64*)fail_handle(CBH_E_INVAL, "cbh_idx64_create_sharded: empty mask, a device of the mask is not usable, or shards_per_device out of range");
  }
  idx->device = S->comm.devices[0];
  idx->shards = S;
  const size_t R = S->comm.shard_count();
  for (size_t s = 0; s < R; ++s) {
    cbh_idx64* c = cbh_idx64_create(S->comm.device_of_shard(s));
    if (!c) {
      cbh_idx64_destroy(idx);
      return nullptr;
    }
    c->rec_cap_default = std::max<size_t>(65536, idx->rec_cap_default / R);
    S->child.push_back(c);
  }
  return idx;
}

uint32_t cbh_idx64_device_mask(const cbh_idx64* idx) {
  return !idx ? 0 : idx->shards ? idx->shards->comm.mask : (1u << idx->device);
}

int cbh_idx64_shards_per_device(const cbh_idx64* idx) { return !idx ? 0 : idx->shards ? idx->shards->comm.per_device : 1; }

int cbh_idx64_shard_count(const cbh_idx64* idx) { return !idx ? 0 : idx->shards ? (int)idx->shards->child.size() : 1; }

cbh_idx64* cbh_idx64_shard(cbh_idx64* idx, int i) {
  if (!idx) return nullptr;
  if (!idx->shards) return i == 0 ? idx : nullptr;
  if (i < 0 || (size_t)i >= idx->shards->child.size()) return nullptr;
  return idx->shards->child[(size_t)i];
}

int cbh_idx64_shard_stats(const cbh_idx64* idx, cbh_shard_stats* out) {
  if (!idx || !out) return CBH_E_INVAL;
  memset(out, 0, sizeof *out);
  if (!idx->shards) {
    out->shards = 1, out->devices = 1;
    return CBH_OK;
  }
  const ShardSet* S = idx->shards;
  out->shards = (uint32_t)S->child.size();
  out->devices = (uint32_t)S->comm.devices.size();
  out->device_mask = S->comm.mask;
  out->scans = S->comm.n_scans.load();
  out->rescans = S->comm.n_rescans.load();
  out->collectives = S->comm.n_collectives.load();
  out->peer_copies = S->comm.n_peer_copies.load();
  out->local_copies = S->comm.n_local_copies.load();
  out->collective_fallbacks = S->comm.n_fallbacks.load();
  out->segments = S->segs.size();
  return CBH_OK;
}

}  // extern "C"
