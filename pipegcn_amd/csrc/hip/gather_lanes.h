// Shared by the wave-per-(row, chunk) gathers that are not sums (spmm_max.hip,
// spmm_pna.hip). Device side: int32 / fp32 lane accesses next to
// attn_util::ld_vec, and the wave preamble with its index in a scalar
// register. Host side: the lane width, the dtype dispatch and the launch
// geometry. Everything device-side is force-inlined.
#pragma once

#include "../common.h"
#include "attn_util.h"
#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

namespace gather_lanes {

using attn_util::raw_vec;

// 4-byte elements (int32 ids, fp32 state), VEC per lane: one 4/8/16-byte
// access, or two 16-byte ones for VEC = 8 (they are 4 bytes per element
// whatever the features' dtype is)
template <typename W, int VEC>
__device__ __forceinline__ void ld_words(const W* p, W (&v)[VEC]) {
  static_assert(sizeof(W) == 4);
  constexpr int N = VEC < 4 ? VEC : 4;
  using R = typename raw_vec<4 * N>::type;
#pragma unroll
  for (int b = 0; b < VEC; b += N) {
    const R r = *reinterpret_cast<const R*>(p + b);
    __builtin_memcpy(&v[b], &r, sizeof(R));
  }
}

template <typename W, int VEC>
__device__ __forceinline__ void st_words(W* p, const W (&v)[VEC]) {
  static_assert(sizeof(W) == 4);
  constexpr int N = VEC < 4 ? VEC : 4;
  using R = typename raw_vec<4 * N>::type;
#pragma unroll
  for (int b = 0; b < VEC; b += N) {
    R r;
    __builtin_memcpy(&r, &v[b], sizeof(R));
    __builtin_nontemporal_store(r, reinterpret_cast<R*>(p + b));
  }
}

template <int VEC>
__device__ __forceinline__ void ld_ids(const int32_t* p, int32_t (&v)[VEC]) {
  ld_words<int32_t, VEC>(p, v);
}

template <int VEC>
__device__ __forceinline__ void st_ids(int32_t* p, const int32_t (&v)[VEC]) {
  st_words<int32_t, VEC>(p, v);
}

// The wave of a (row, chunk) pair loop with its index in a scalar register,
// as spmm_csr_kernel forms it: row, edge cursor and node ids are then
// wave-uniform for the compiler too. The geometry arrives through default
// arguments for the reason given at attn_util::wave_ids.
struct UniformWave {
  int64_t wave_global;
  int lane;
  int64_t nwaves;
};

__device__ __forceinline__ UniformWave uniform_wave(
    unsigned block = blockIdx.x, unsigned block_dim = blockDim.x,
    unsigned thread = threadIdx.x, unsigned grid_dim = gridDim.x) {
  const int wave_in_block =
      __builtin_amdgcn_readfirstlane(static_cast<int>(thread) / kWave);
  const int64_t waves_per_block = block_dim / kWave;
  return {static_cast<int64_t>(block) * waves_per_block + wave_in_block,
          static_cast<int>(thread & (kWave - 1)),
          static_cast<int64_t>(grid_dim) * waves_per_block};
}

// pick_vec's width, narrowed until every pointer takes the lane access:
// `elems` hold `elem_size`-byte elements, `words` 4-byte ones (16 bytes at
// the most per access); null pointers are skipped
inline int lane_vec(const char* op, int64_t F, int64_t num_rows,
                    int64_t elem_size,
                    std::initializer_list<const void*> elems,
                    std::initializer_list<const void*> words) {
  int vec = pick_vec(F, num_rows, elem_size);
  auto fits = [&](int v) {
    for (const void* p : elems)
      if (p && !aligned_to(p, v * elem_size)) return false;
    for (const void* p : words)
      if (p && !aligned_to(p, std::min(4 * v, 16))) return false;
    return true;
  };
  while (vec > 1 && !fits(vec)) vec /= 2;
  TORCH_CHECK(F % vec == 0 && vec * elem_size <= 16, op, ": lane width ", vec,
              " does not fit rows of ", F, " elements");
  return vec;
}

template <typename T>
const T* cptr(const torch::Tensor& x) {
  return reinterpret_cast<const T*>(x.data_ptr());
}
template <typename T>
T* mptr(torch::Tensor& x) {
  return reinterpret_cast<T*>(x.data_ptr());
}

// fn(T{}, VEC as an integral constant) for x's element type and a lane width
// that lane_vec returned
template <typename Fn>
void dispatch(const torch::Tensor& x, int vec, Fn&& fn) {
  dispatch_vec(vec, [&](auto v) {
    if (x.scalar_type() == torch::kBFloat16) {
      fn(__hip_bfloat16{}, v);
    } else if constexpr (v.value <= 4) {
      fn(float{}, v);
    }
  });
}

struct Launch {
  int64_t nchunks;
  dim3 grid, block;
};

inline Launch launch_of(int64_t num_rows, int64_t F, int vec) {
  constexpr int threads = 256;  // whole waves: the kernels keep the wave
  static_assert(threads % kWave == 0);  // index in a scalar register
  const int64_t nchunks = (F + kWave * vec - 1) / (kWave * vec);
  return {nchunks, dim3(grid_for(num_rows * nchunks, threads)),
          dim3(threads)};
}

}  // namespace gather_lanes
