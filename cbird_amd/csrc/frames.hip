// frames.hip -- K9: DctVideoIndex::findFrame (src/dctvideoindex.cpp:291-387) for a chunk of image needles on the device.
//
// Input: the unordered scan records of the chunk, needle (25) | distance (7) | entry position + 1 (32).  The entries of
// the search structure are stored in video order (video.hip build()), so position order is video order and the whole
// reduction is linear in the records:
//   k_frame_keys     rotates every record in place to  needle (25) | position + 1 (32) | distance (7)
//   sort_keys64_db   one ascending sort: the records of a (needle, video) pair become one contiguous RUN, and the runs
//                    stand in the output order -- ascending needle, then ascending video index, the QMap order of :353-366
//   k_frame_heads    a record is a run head when its (needle, video index) differs from its predecessor's; an inclusive
//                    scan of the head flags numbers the runs
//   k_frame_winners  one thread per record, a segmented min-scan of  distance << 32 | position + 1  over the 64 lanes of
//                    a wave: smallest distance, among equals the earliest entry -- what the reference's in-order walk with
//                    `match.distance < it->distance` keeps (:355-364).  Only the last lane a run has inside a wave
//                    writes: a plain store when the run begins and ends in that wave, else ONE 64-bit atomicMin on
//                    best[run] (preset to all ones).  No record walks its run or its needle's segment, so a needle that
//                    hits a static stretch of video (runs of thousands of records) costs what any other record costs
//   k_frame_emit     the head of run r writes out[r]; k_frame_offsets finds every needle's first run by a binary search
// The result is compact, ordered and deterministic: the host sorts nothing.
#include <rocprim/device/device_scan.hpp>

#include "cbh_internal.h"

namespace cbh {
namespace {

constexpr unsigned kNoRun = 0xffffffffu;

__device__ __forceinline__ uint32_t key_needle(unsigned long long k) { return (uint32_t)(k >> 39); }
__device__ __forceinline__ uint32_t key_id(unsigned long long k) { return (uint32_t)(k >> 7); }  // entry position + 1

__global__ __launch_bounds__(256) void k_frame_keys(unsigned long long* __restrict__ rec, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const unsigned long long r = rec[i];
  rec[i] = ((r >> 39) << 39) | ((r & 0xffffffffull) << 7) | ((r >> 32) & 0x7f);
}

__global__ __launch_bounds__(256) void k_frame_heads(const unsigned long long* __restrict__ keys, size_t total,
                                                     const uint32_t* __restrict__ evidx, uint32_t* __restrict__ flags) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  bool head = true;
  if (i > 0) {
    const unsigned long long k = keys[i], p = keys[i - 1];
    head = key_needle(k) != key_needle(p) || evidx[key_id(k) - 1] != evidx[key_id(p) - 1];
  }
  flags[i] = head ? 1u : 0u;
}

// runno[i] = number of heads in [0, i]: the run of record i is runno[i] - 1
__global__ __launch_bounds__(256) void k_frame_winners(const unsigned long long* __restrict__ keys,
                                                       const uint32_t* __restrict__ runno, size_t total,
                                                       unsigned long long* __restrict__ best) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const unsigned lane = threadIdx.x & 63;
  const bool live = i < total;  // (every lane stays for the shuffles)
  unsigned run = kNoRun, prev = kNoRun, next = kNoRun;
  unsigned long long val = ~0ull;
  if (live) {
    const unsigned long long k = keys[i];
    val = ((k & 0x7f) << 32) | (unsigned long long)key_id(k);
    run = runno[i] - 1;
    if (i > 0) prev = runno[i - 1] - 1;
    if (i + 1 < total) next = runno[i + 1] - 1;
  }
  // inclusive segmented minimum: runs are contiguous, so a lane `d` below in the same run means every lane between is
#pragma unroll
  for (unsigned d = 1; d < 64; d <<= 1) {
    const unsigned long long ov = __shfl_up(val, d);
    const unsigned orun = __shfl_up(run, d);
    if (lane >= d && orun == run) val = min(val, ov);
  }
  const unsigned run0 = __shfl(run, 0);
  const int head0 = __shfl((int)(prev != run), 0);  // does the wave's first record begin its run
  if (!live) return;
  if (lane != 63 && next == run) return;  // not the last lane of its run inside this wave
  const bool begins_here = run != run0 || head0, ends_here = next != run;
  if (begins_here && ends_here)
    best[run] = val;
  else
    atomicMin(&best[run], val);
}

__global__ __launch_bounds__(256) void k_frame_emit(const unsigned long long* __restrict__ keys,
                                                    const uint32_t* __restrict__ runno, size_t total,
                                                    const unsigned long long* __restrict__ best,
                                                    const uint32_t* __restrict__ evidx, const int32_t* __restrict__ eframe,
                                                    const uint32_t* __restrict__ vmedia,
                                                    const int32_t* __restrict__ src_in, cbh_vmatch* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const unsigned run = runno[i] - 1;
  if (i > 0 && runno[i - 1] - 1 == run) return;  // not a head
  const unsigned long long b = best[run];
  const uint32_t pos = (uint32_t)(b & 0xffffffffull) - 1;
  const int32_t src = src_in ? src_in[key_needle(keys[i])] : 0;
  cbh_vmatch m;
  m.id = vmedia[evidx[pos]];
  m.score = (int32_t)(b >> 32);
  m.src_in = src < 0 ? 0 : src;  // (:372-376)
  m.dst_in = eframe[pos];
  m.len = 1;
  out[run] = m;
}

// off[j], j = 0..nq: the run of the first record whose needle is >= j (a head: its predecessor's needle is smaller)
__global__ __launch_bounds__(256) void k_frame_offsets(const unsigned long long* __restrict__ keys,
                                                       const uint32_t* __restrict__ runno, size_t total, unsigned nq,
                                                       uint32_t* __restrict__ off) {
  const unsigned j = blockIdx.x * 256 + threadIdx.x;
  if (j > nq) return;
  size_t lo = 0, hi = total;
  while (lo < hi) {
    const size_t mid = (lo + hi) >> 1;
    if (key_needle(keys[mid]) < j)
      lo = mid + 1;
    else
      hi = mid;
  }
  off[j] = lo < total ? runno[lo] - 1 : runno[total - 1];
}

}  // namespace

// d_rec: `total` (1 .. 2^32 - 1) unordered scan records of `nq` needles; d_alt / d_tmp: the sort's second buffer and
// scratch (Workspace::ensure_sort).  d_evidx / d_eframe: entry -> video index / frame, d_vmedia: video index -> media id.
// h_src_in: NULL (every needle 0) or nq values.  On return h_out holds one match per run and h_off[0 .. nq] the first run
// of every needle (h_off[nq] = the number of runs).  Synchronises `s`.
int launch_frame_reduce(unsigned long long* d_rec, unsigned long long* d_alt, size_t total, size_t nq, void* d_tmp,
                        size_t tmp_bytes, const uint32_t* d_evidx, const int32_t* d_eframe, const uint32_t* d_vmedia,
                        const int32_t* h_src_in, std::vector<cbh_vmatch>* h_out, std::vector<uint32_t>* h_off,
                        hipStream_t s) {
  h_out->clear();
  h_off->assign(nq + 1, 0);
  if (total == 0 || nq == 0) return CBH_OK;
  if (total >= (1ull << 32) || nq > CBH_MAX_QUERIES_PER_CALL) return CBH_E_OVERFLOW;
  uint32_t *flags = nullptr, *runno = nullptr, *off = nullptr;
  int32_t* d_src_in = nullptr;
  void* scan_tmp = nullptr;
  size_t scan_bytes = 0;
  CBH_HIP(rocprim::inclusive_scan(nullptr, scan_bytes, flags, runno, total, rocprim::plus<uint32_t>(), s));
  Scratch scratch(s);
  CBH_HIP(scratch.get(&flags, total * 4));
  CBH_HIP(scratch.get(&runno, total * 4));
  CBH_HIP(scratch.get(&scan_tmp, scan_bytes ? scan_bytes : 16));
  CBH_HIP(scratch.get(&off, (nq + 1) * 4));
  if (h_src_in) CBH_HIP(upload(scratch, &d_src_in, h_src_in, nq, s));
  const unsigned g = (unsigned)((total + 255) / 256);
  hipLaunchKernelGGL(k_frame_keys, dim3(g), dim3(256), 0, s, d_rec, total);
  unsigned end_bit = 39;
  while (end_bit < 64 && ((size_t)1 << (end_bit - 39)) < nq) ++end_bit;
  unsigned long long* keys = nullptr;
  if (int rc = sort_keys64_db(d_rec, d_alt, total, end_bit, d_tmp, tmp_bytes, s, &keys)) return rc;
  hipLaunchKernelGGL(k_frame_heads, dim3(g), dim3(256), 0, s, keys, total, d_evidx, flags);
  CBH_HIP(rocprim::inclusive_scan(scan_tmp, scan_bytes, flags, runno, total, rocprim::plus<uint32_t>(), s));
  hipLaunchKernelGGL(k_frame_offsets, dim3((unsigned)((nq + 1 + 255) / 256)), dim3(256), 0, s, keys, runno, total,
                     (unsigned)nq, off);
  CBH_HIP(hipGetLastError());
  CBH_HIP(hipMemcpyAsync(h_off->data(), off, (nq + 1) * 4, hipMemcpyDeviceToHost, s));
  CBH_HIP(hipStreamSynchronize(s));
  const size_t n_runs = (*h_off)[nq];
  if (n_runs == 0 || n_runs > total) return CBH_E_HIP;  // (total > 0: there is at least the first record's run)
  unsigned long long* best = nullptr;
  cbh_vmatch* out = nullptr;
  CBH_HIP(scratch.get(&best, n_runs * 8));
  CBH_HIP(scratch.get(&out, n_runs * sizeof(cbh_vmatch)));
  CBH_HIP(hipMemsetAsync(best, 0xff, n_runs * 8, s));
  hipLaunchKernelGGL(k_frame_winners, dim3(g), dim3(256), 0, s, keys, runno, total, best);
  hipLaunchKernelGGL(k_frame_emit, dim3(g), dim3(256), 0, s, keys, runno, total, best, d_evidx, d_eframe, d_vmedia,
                     d_src_in, out);
  CBH_HIP(hipGetLastError());
  h_out->resize(n_runs);
  CBH_HIP(hipMemcpyAsync(h_out->data(), out, n_runs * sizeof(cbh_vmatch), hipMemcpyDeviceToHost, s));
  CBH_HIP(hipStreamSynchronize(s));
  return CBH_OK;
}

}  // namespace cbh
