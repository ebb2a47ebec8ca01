// Device helpers shared by the attention aggregation kernels (gat.hip,
// gatv2.hip): typed vector loads/stores, LeakyReLU, the attention-dropout
// hash and the fixed-order wave reductions. Everything is force-inlined, so
// each .hip gets exactly the code it had when these lived in its own
// anonymous namespace.
#pragma once

#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace attn_util {

constexpr int kWave = 64;

using int32x4 = __attribute__((ext_vector_type(4))) int;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__hip_bfloat16 v) {
  return __bfloat162float(v);
}
template <typename T>
__device__ __forceinline__ T from_f32(float v);
template <>
__device__ __forceinline__ float from_f32<float>(float v) {
  return v;
}
template <>
__device__ __forceinline__ __hip_bfloat16 from_f32<__hip_bfloat16>(float v) {
  return __float2bfloat16(v);
}

// one lane's VEC elements move as ONE 2/4/8/16-byte access (hipcc does not
// merge scalar bf16 accesses by itself)
template <int BYTES>
struct raw_vec;
template <>
struct raw_vec<2> {
  using type = unsigned short;
};
template <>
struct raw_vec<4> {
  using type = unsigned int;
};
template <>
struct raw_vec<8> {
  using type = __attribute__((ext_vector_type(2))) unsigned int;
};
template <>
struct raw_vec<16> {
  using type = __attribute__((ext_vector_type(4))) unsigned int;
};

template <typename T, int VEC>
__device__ __forceinline__ void ld_vec(const T* p, float (&v)[VEC]) {
  using R = typename raw_vec<sizeof(T) * VEC>::type;
  const R r = *reinterpret_cast<const R*>(p);
  T tmp[VEC];
  __builtin_memcpy(tmp, &r, sizeof(R));
#pragma unroll
  for (int k = 0; k < VEC; ++k) v[k] = to_f32(tmp[k]);
}

template <typename T, int VEC>
__device__ __forceinline__ void st_vec(T* p, const float (&v)[VEC]) {
  using R = typename raw_vec<sizeof(T) * VEC>::type;
  T tmp[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) tmp[k] = from_f32<T>(v[k]);
  R r;
  __builtin_memcpy(&r, tmp, sizeof(R));
  __builtin_nontemporal_store(r, reinterpret_cast<R*>(p));
}

__device__ __forceinline__ float leaky(float s, float slope) {
  return s > 0.f ? s : slope * s;
}

// Attention-dropout keep bit of (edge u -> v, head h): stateless, 32-bit
// arithmetic only (mod 2^32). The pre-mix is linear so that each kernel
// hoists the term of its fixed endpoint: drop_base() once per (row, lane),
// then one multiply-add and the murmur3 finaliser per edge. Ids are hashed
// as uint32 (no sign extension). ops.gat_dropout_keep is the bit-identical
// torch mirror.
constexpr uint32_t kDropMulU = 0x9E3779B1u;
constexpr uint32_t kDropMulV = 0x85EBCA77u;
constexpr uint32_t kDropMulH = 0xC2B2AE3Du;

__device__ __forceinline__ uint32_t drop_base(uint32_t fixed_id,
                                              uint32_t fixed_mul, uint32_t h,
                                              uint32_t key) {
  return fixed_id * fixed_mul + h * kDropMulH + key;
}

__device__ __forceinline__ uint32_t drop_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// dropout weight of one edge: scale = 1 / (1 - p) if kept, else 0
__device__ __forceinline__ float drop_weight(uint32_t id, uint32_t mul,
                                             uint32_t base, uint32_t thr,
                                             float scale) {
  return drop_mix(id * mul + base) >= thr ? scale : 0.f;
}

// fixed-order butterfly sum: every lane ends with the same total
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
  return x;
}

// host side: launch geometry and alignment of the wave-per-row kernels
inline int64_t grid_for(int64_t nwaves, int threads) {
  int64_t blocks = (nwaves * kWave + threads - 1) / threads;
  // cap the grid; the grid-stride loops cover the rest
  blocks = std::min<int64_t>(blocks, 8 * 65536);
  return blocks == 0 ? 1 : blocks;
}

inline bool aligned_to(const void* p, int64_t bytes) {
  return reinterpret_cast<uintptr_t>(p) % bytes == 0;
}

}  // namespace attn_util
