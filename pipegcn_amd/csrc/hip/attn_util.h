// Shared by the attention aggregation kernels (gat.hip, gatv2.hip).
// Device side: typed vector loads/stores, LeakyReLU, the attention-dropout
// hash, the fixed-order wave reduction, the wave-per-pair preamble (wave_ids)
// and the walk over one row's edges (for_edges). Everything there is
// force-inlined, so each .hip gets exactly the code it had when these lived
// in its own anonymous namespace. Host side: the checks that keep an
// under-sized tensor from becoming an out-of-bounds gather; each takes the
// op's name for its messages. kWave, int32x4, to_f32, grid_for and
// aligned_to come from hip_util.h.
#pragma once

#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace attn_util {

using f32x4 = __attribute__((ext_vector_type(4))) float;

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

// The wave of a (row, chunk) or (row, head group) pair loop: a kernel walks
// pairs wave_global, wave_global + nwaves, ... The one place where the
// scalar-register wave index of spmm_csr_kernel would go (docs/ROADMAP.md).
struct WaveIds {
  int64_t wave_global;
  int lane;
  int64_t nwaves;
};

// Called as wave_ids(). The launch geometry arrives through default
// arguments because those are evaluated in the calling kernel: read inside a
// device function, blockDim loses the kernel's uniform-block-size guarantee
// and costs a dependent load at every wave's start.
__device__ __forceinline__ WaveIds wave_ids(unsigned block = blockIdx.x,
                                            unsigned block_dim = blockDim.x,
                                            unsigned thread = threadIdx.x,
                                            unsigned grid_dim = gridDim.x) {
  return {(static_cast<int64_t>(block) * block_dim + thread) / kWave,
          static_cast<int>(thread & (kWave - 1)),
          (static_cast<int64_t>(grid_dim) * block_dim) / kWave};
}

// Walk the edges [e, e_end) of one row: peel until e is 4-aligned, then read
// four indices with one dwordx4 and hand them on U at a time (U gathers in
// flight), then the tail one by one. fn(integral_constant<int, N>, ids).
template <int U, typename Fn>
__device__ __forceinline__ void for_edges(const int32_t* __restrict__ indices,
                                          int64_t e, int64_t e_end, Fn&& fn) {
  for (; e < e_end && (e & 3); ++e) {
    const int32_t one[1] = {indices[e]};
    fn(std::integral_constant<int, 1>{}, one);
  }
  for (; e + 4 <= e_end; e += 4) {
    const int32x4 q = __builtin_nontemporal_load(
        reinterpret_cast<const int32x4*>(indices + e));
    const int32_t ids[4] = {q[0], q[1], q[2], q[3]};
#pragma unroll
    for (int b = 0; b < 4; b += U) {
      int32_t part[U];
#pragma unroll
      for (int i = 0; i < U; ++i) part[i] = ids[b + i];
      fn(std::integral_constant<int, U>{}, part);
    }
  }
  for (; e < e_end; ++e) {
    const int32_t one[1] = {indices[e]};
    fn(std::integral_constant<int, 1>{}, one);
  }
}

// ---------------------------------------------------------------------------
// host side: `op` ("gat" / "gatv2") prefixes every message
// ---------------------------------------------------------------------------

// the attention dropout's folded key, keep threshold and 1 / (1 - p).
// thr == 0 keeps every edge.
struct DropArgs {
  uint32_t key;
  uint32_t thr;
  float scale;
};

inline DropArgs drop_args(const char* op, int64_t key, int64_t thr,
                          double scale) {
  TORCH_CHECK(key >= 0 && key <= 0xFFFFFFFFll && thr >= 0 &&
                  thr <= 0xFFFFFFFFll,
              op, ": drop_key and drop_thr are 32-bit values");
  return {static_cast<uint32_t>(key), static_cast<uint32_t>(thr),
          static_cast<float>(scale)};
}

inline const int32_t* row_order_ptr(const char* op,
                                    const torch::Tensor& row_order,
                                    int64_t num_rows) {
  if (!row_order.defined() || row_order.numel() == 0) return nullptr;
  TORCH_CHECK(row_order.is_cuda() && row_order.is_contiguous() &&
                  row_order.numel() == num_rows &&
                  row_order.scalar_type() == torch::kInt,
              op, ": row_order must be a contiguous int32[num_rows]");
  return row_order.data_ptr<int32_t>();
}

inline void check_graph(const char* op, const torch::Tensor& indptr,
                        const torch::Tensor& indices) {
  TORCH_CHECK(indptr.is_cuda() && indices.is_cuda(), op,
              ": graph tensors must be on the device");
  TORCH_CHECK(indptr.scalar_type() == torch::kLong &&
                  indices.scalar_type() == torch::kInt,
              op, ": indptr int64 / indices int32");
  TORCH_CHECK(indptr.is_contiguous() && indices.is_contiguous() &&
                  indptr.numel() >= 1,
              op, ": graph tensors must be contiguous");
  // for_edges reads indices four at a time with one dwordx4
  TORCH_CHECK(aligned_to(indices.data_ptr(), 16), op,
              ": indices must be 16-byte aligned");
}

// a per-node per-head fp32 table with at least `rows` rows
inline void check_node_table(const char* op, const torch::Tensor& x,
                             int64_t rows, int64_t H, const char* name) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() &&
                  x.scalar_type() == torch::kFloat,
              op, ": ", name, " must be a contiguous fp32 [nodes, H] tensor");
  TORCH_CHECK(x.size(1) == H, op, ": ", name, " has ", x.size(1),
              " heads, expected ", H);
  TORCH_CHECK(x.size(0) >= rows, op, ": ", name, " has ", x.size(0),
              " rows but the graph references ", rows);
}

// a [nodes, F] feature tensor (fp32 or bf16) with at least `rows` rows
inline void check_features(const char* op, const torch::Tensor& x,
                           int64_t rows, int64_t H, const char* name) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous(), op, ": ",
              name, " must be a contiguous [nodes, F] tensor");
  TORCH_CHECK(x.scalar_type() == torch::kFloat ||
                  x.scalar_type() == torch::kBFloat16,
              op, ": ", name, " must be fp32 or bf16");
  TORCH_CHECK(H >= 1 && x.size(1) >= H && x.size(1) % H == 0, op, ": ", name,
              " width F=", x.size(1), " is not H*D for H=", H);
  TORCH_CHECK(x.size(0) >= rows, op, ": ", name, " has ", x.size(0),
              " rows but the graph references ", rows,
              " (an under-sized tensor would be an out-of-bounds gather)");
}

}  // namespace attn_util
