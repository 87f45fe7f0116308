// fp4_sign.h -- shared by the matrix-core Hamming kernels (hamm64_mfma.hip, hamm256_mfma.hip).
//
// Hamming distance as a dot product: with s(x)_k = +1 if bit k of x is set, else -1,
//   dot(s(a), s(b)) over K bits = K - 2 * popcount(a ^ b).
// +-1.0 are exact in FP4 (E2M1: +1.0 = 0x2, -1.0 = 0xA), products and partial sums are small
// integers, so v_mfma_scale_f32_32x32x64_f8f6f4 with FP4 operands and unit block scales returns
// exact distances of 32 x 32 pairs per 64 bits of K.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cbh {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kScaleOne = 0x7f7f7f7f;  // E8M0 127 = 2^0 in every byte

// 32 bits -> 32 FP4 sign nibbles: bit k -> nibble k = 0x2 (+1.0) if set, 0xA (-1.0) if clear
__device__ __forceinline__ uint4 fp4_expand32(uint32_t w) {
  uint32_t o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t x = (w >> (8 * d)) & 0xffu;
    x = (x | (x << 12)) & 0x000f000fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = (x | (x << 3)) & 0x11111111u;
    o[d] = 0xaaaaaaaau ^ (x << 3);
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// The same with a magnitude other than 1: 16 bits -> 16 nibbles  sign | mag,  mag = the E2M1 code without its sign.
// 0.5 (the one subnormal) and 4.0 are what the 48-bit prefilter of hamm64_mfma.hip tells two fields of one scale
// block apart by: 0.5 * 0.5 against 4 * 4 is a ratio of 64.
constexpr uint32_t kFp4Half = 0x1u;  // 0.5
constexpr uint32_t kFp4Four = 0x6u;  // 4.0
__device__ __forceinline__ uint2 fp4_expand16(uint32_t w, uint32_t mag) {
  uint32_t o[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    uint32_t x = (w >> (8 * d)) & 0xffu;
    x = (x | (x << 12)) & 0x000f000fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = (x | (x << 3)) & 0x11111111u;
    o[d] = (0x88888888u | (mag * 0x11111111u)) ^ (x << 3);
  }
  return make_uint2(o[0], o[1]);
}

// The 48-bit prefilter word of a 64-bit hash (lo, hi), as three sub-blocks of 16 elements: E0 = the folds
// bit i ^ bit i + 32 for i < 16 (the lowest-frequency coefficients against their partners), E1 = bits 16..31,
// E2 = bits 48..63 as they are.  popc over the three sub-blocks of a ^ b is a lower bound on hamm64(a, b): every set
// element needs a set bit of a ^ b of its own (the fold argument at the top of hamm64_mfma.hip).
__host__ __device__ __forceinline__ uint32_t pre48_sub(uint32_t lo, uint32_t hi, uint32_t k) {
  return k == 0 ? (lo ^ hi) & 0xffffu : k == 1 ? lo >> 16 : hi >> 16;
}

// The 16-bit prefilter word: the 32-bit fold lo ^ hi folded once more, bit i = the XOR of bits i, i + 16, i + 32, i + 48.
// A set bit of fold16(a) ^ fold16(b) needs an odd number of set bits among those four of a ^ b, so its popcount is a lower
// bound on hamm64(a, b) by the same argument.  One scale block split by magnitude (0.5 x 0.5 against 4 x 4) holds two such
// words: the threshold-1 prefilter of hamm64_mfma.hip compares four needle tiles in ONE MFMA.
__host__ __device__ __forceinline__ uint32_t fold16(uint32_t lo, uint32_t hi) {
  const uint32_t f = lo ^ hi;
  return (f ^ (f >> 16)) & 0xffffu;
}

// FP4 operand of the f8f6f4 MFMA: the first 4 of the 8 operand dwords are used
__device__ __forceinline__ v8i fp4_operand(uint4 e) {
  return v8i{(int)e.x, (int)e.y, (int)e.z, (int)e.w, 0, 0, 0, 0};
}

}  // namespace cbh
