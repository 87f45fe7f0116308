// hamm256_scan.hip -- the 256-bit threshold scan of CvFeaturesIndex (idx256.hip): the popcount kernel, and the one place
// that decides which kernel a launch runs on.  Every caller goes through launch_hamm256_scan; route256() is the decision,
// hamm256_mfma.hip launches what it is told.
//
// k_hamm256_scan has the shape of k_hamm64_scan: each lane keeps H rows (first 128 bits, 4 VGPRs per row) in
// registers, needles are wave-uniform SGPR operands.  Since the k nearest are only ever used below a threshold,
// it is a threshold scan: the first 128 bits give a sound lower bound (4 xor + 4 bcnt per pair, min3 over
// pairs), and only slots whose bound drops under the threshold load their second half and evaluate all 256 bits.
#include <atomic>

#include "cbh_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kH = 8;
constexpr int kQB = 4;

__device__ __forceinline__ uint32_t min3u(uint32_t a, uint32_t b, uint32_t c) { return min(min(a, b), c); }

__device__ __forceinline__ uint32_t popc128(uint4 a, uint4 b) {
  return __popc(a.x ^ b.x) + __popc(a.y ^ b.y) + __popc(a.z ^ b.z) + __popc(a.w ^ b.w);
}

template <int H, int QB>
__global__ __launch_bounds__(kThreads) void k_hamm256_scan(
    const uint4* __restrict__ rows /* 2 x uint4 per row */, uint32_t n, const uint4* __restrict__ q, uint32_t nq,
    uint32_t q_chunk, uint32_t thresh, unsigned long long* __restrict__ rec, unsigned long long cap,
    unsigned long long* __restrict__ total) {
  const uint32_t base_idx = blockIdx.x * (uint32_t)(kThreads * H) + threadIdx.x;
  uint4 h[H];
#pragma unroll
  for (int j = 0; j < H; ++j) {
    const uint32_t idx = base_idx + (uint32_t)j * kThreads;
    h[j] = idx < n ? rows[(size_t)idx * 2] : make_uint4(0u, 0u, 0u, 0u);
  }
  const uint32_t q0 = blockIdx.y * q_chunk;
  const uint32_t q1 = min(nq, q0 + q_chunk);
  for (uint32_t qb = q0; qb < q1; qb += QB) {
    uint4 cur[QB];
#pragma unroll
    for (int i = 0; i < QB; ++i) cur[i] = q[(size_t)min(qb + i, q1 - 1) * 2];  // wave-uniform -> SMEM
    uint32_t acc[H];
#pragma unroll
    for (int j = 0; j < H; ++j) acc[j] = 0xffffu;
#pragma unroll
    for (int i = 0; i < QB; i += 2) {
#pragma unroll
      for (int j = 0; j < H; ++j) acc[j] = min3u(acc[j], popc128(h[j], cur[i]), popc128(h[j], cur[i + 1]));
    }
    uint32_t m = acc[0];
#pragma unroll
    for (int j = 1; j < H; ++j) m = min(m, acc[j]);
    if (m < thresh) {
#pragma unroll
      for (int j = 0; j < H; ++j) {
        if (acc[j] < thresh) {
          const uint32_t idx = base_idx + (uint32_t)j * kThreads;
          if (idx < n) {
            const uint4 h2 = rows[(size_t)idx * 2 + 1];
#pragma unroll 1
            for (uint32_t qi = qb; qi < min(qb + QB, q1); ++qi) {
              const uint32_t d = popc128(h[j], q[(size_t)qi * 2]) + popc128(h2, q[(size_t)qi * 2 + 1]);
              if (d < thresh) {
                const unsigned long long slot = atomicAdd(total, 1ull);
                if (slot < cap)
                  rec[slot] = ((unsigned long long)qi << 41) | ((unsigned long long)d << 32) | idx;
              }
            }
          }
        }
      }
    }
  }
}

}  // namespace

namespace cbh {
namespace {

int launch_popcount(const uint8_t* d_rows, size_t n, const uint8_t* d_q, size_t nq, int thresh,
                    unsigned long long* d_rec, size_t cap, unsigned long long* d_total, hipStream_t stream) {
  const uint32_t tile = kThreads * kH;
  const uint32_t tiles = (uint32_t)((n + tile - 1) / tile);
  uint32_t q_chunk = 4096;
  while (q_chunk > 256 && (uint64_t)tiles * ((nq + q_chunk - 1) / q_chunk) < 8192) q_chunk >>= 1;
  uint32_t chunks = (uint32_t)((nq + q_chunk - 1) / q_chunk);
  if (chunks > 65535) {
    q_chunk = (uint32_t)((nq + 65534) / 65535);
    q_chunk = (q_chunk + kQB - 1) / kQB * kQB;
    chunks = (uint32_t)((nq + q_chunk - 1) / q_chunk);
  }
  hipLaunchKernelGGL((k_hamm256_scan<kH, kQB>), dim3(tiles, chunks), dim3(kThreads), 0, stream,
                     reinterpret_cast<const uint4*>(d_rows), (uint32_t)n, reinterpret_cast<const uint4*>(d_q),
                     (uint32_t)nq, q_chunk, (uint32_t)thresh, d_rec, (unsigned long long)cap, d_total);
  CBH_HIP(hipGetLastError());
  return CBH_OK;
}

int g_scan256_small = 1;  // "scan256_small": the stationary-needle kernel for <= 512 needle descriptors (default on)
int g_scan256_mfma = 1;   // "scan256_mfma": 0 never, 1 from 64 needle descriptors and 4096 rows, 2 always (tests)
constexpr int kPre128MaxThresh = 40;  // thresholds up to this take a first-128-bit prefilter variant
std::atomic<long long> g_scan256_kernels{0};  // "scan256_kernels": Scan256Kernel bits of the launches since the last clear

}  // namespace

int set_scan256_mfma(int v) {
  if (v < 0 || v > 2) return CBH_E_INVAL;
  g_scan256_mfma = v;
  return CBH_OK;
}
int set_scan256_small(int v) {
  if (v != 0 && v != 1) return CBH_E_INVAL;
  g_scan256_small = v;
  return CBH_OK;
}
int get_scan256_mfma() { return g_scan256_mfma; }
int get_scan256_small() { return g_scan256_small; }
long long get_scan256_kernels() { return g_scan256_kernels.load(); }
void clear_scan256_kernels() { g_scan256_kernels.store(0); }

// The decision, a pure function of the launch's shape and the two knobs (tests/scan256_layout.py: route() is its model).
// Thresholds the matrix-core kernels cannot hold (cbh_idx256_knn passes any) stay on the popcount kernel.
Route256 route256(size_t n, size_t nq, int thresh) {
  const bool forced = g_scan256_mfma == 2;
  if (thresh < 1 || thresh > 257 || !g_scan256_mfma || (!forced && !(nq >= 64 && n >= 4096))) return {kS256Scan, 0};
  const uint32_t n_tiles = (uint32_t)((nq + 31) / 32);
  const bool pre128 = thresh <= kPre128MaxThresh;
  // k_hamm256_small: its buffer descriptor spans n * 32 bytes; needle tiles are padded to the template's count
  if (g_scan256_small && pre128 && n_tiles <= 16 && n <= ((size_t)1 << 27) - 64) {
    if (n_tiles <= 4) return {kS256Small4, 4 * 32};
    if (n_tiles <= 8) return {kS256Small8, 8 * 32};
    return {kS256Small16, 16 * 32};
  }
  if (pre128 && n_tiles >= 3) return {kS256Mfma3, (n_tiles + 2u) / 3u * 96u};  // whole triples
  // fewer than three needle tiles, or thresholds beyond the prefilter's range: one tile per accumulator
  return {pre128 ? kS256Mfma2 : kS256Mfma4, n_tiles * 32u};
}

int launch_hamm256_scan(const uint8_t* d_rows, size_t n, const uint8_t* d_q, size_t nq, int thresh,
                        unsigned long long* d_rec, size_t cap, unsigned long long* d_total, hipStream_t stream) {
  if (n == 0 || nq == 0 || thresh <= 0) return CBH_OK;
  if (n > 0xfffffff0ull || nq >= (1u << 23)) return CBH_E_INVAL;
  const Route256 r = route256(n, nq, thresh);
  g_scan256_kernels.fetch_or((long long)r.kernel);
  if (r.kernel == kS256Scan) return launch_popcount(d_rows, n, d_q, nq, thresh, d_rec, cap, d_total, stream);
  // the padding descriptors are zero (k_expand_needles256); the kernels drop them at qi >= nq in the hit path
  Scratch scratch(stream);
  uint4* qx = nullptr;
  CBH_HIP(scratch.get(&qx, (size_t)r.nq_pad * 128u));
  expand_needles256(d_q, nq, r.nq_pad, qx, stream);
  return launch_hamm256_mfma(r.kernel, d_rows, n, qx, d_q, nq, thresh, d_rec, cap, d_total, stream);
}

}  // namespace cbh
