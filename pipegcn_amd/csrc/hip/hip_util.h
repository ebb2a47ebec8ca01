// Pieces shared by the .hip sources: error checks, the current stream, the
// wave width, element-type and index-vector helpers, the launch geometry of
// the wave-per-row kernels, the MFMA 32x32 fp32 accumulator layout and the
// vector-width dispatch.
// Each .hip still includes <hip/hip_runtime.h> itself: the build's source
// translation step writes a *_hip.hip copy of any file that does not name it.
#pragma once

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#define HIP_CHECK(expr)                                                  \
  do {                                                                   \
    hipError_t _e = (expr);                                              \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e)); \
  } while (0)

inline hipStream_t current_stream() {
  return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

// call right after a kernel launch: surfaces a bad launch configuration
inline void check_launch() { HIP_CHECK(hipGetLastError()); }

constexpr int kWave = 64;

// four int32 indices read with one dwordx4
using int32x4 = __attribute__((ext_vector_type(4))) int;

// element-type helper: compute in fp32 whatever T (fp32 or bf16) is stored
__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__hip_bfloat16 v) {
  return __bfloat162float(v);
}

// blocks of `threads` threads that give `nwaves` waves one (row, chunk) pair
// each
inline int64_t grid_for(int64_t nwaves, int threads) {
  int64_t blocks = (nwaves * kWave + threads - 1) / threads;
  // cap the grid; the grid-stride loops cover the rest
  blocks = std::min<int64_t>(blocks, 8 * 65536);
  return blocks == 0 ? 1 : blocks;
}

inline bool aligned_to(const void* p, int64_t bytes) {
  return reinterpret_cast<uintptr_t>(p) % bytes == 0;
}

// Accumulator of one v_mfma_f32_32x32x2_f32 fragment: 16 fp32 per lane.
using f32x16 = __attribute__((__vector_size__(16 * sizeof(float)))) float;

// C/D layout of the 32x32 MFMA shapes (shape-determined): lane l holds
// column l&31; its register `reg` (0..15) holds the row below, where
// lane_hi = l>>5. Registers come in groups of 4 consecutive rows; groups are
// 8 rows apart and the upper half-wave is offset by 4.
__device__ __forceinline__ int mfma32_c_row(int reg, int lane_hi) {
  return (reg & 3) + 8 * (reg >> 2) + 4 * lane_hi;
}

// Run fn(std::integral_constant<int, V>{}) for the V in {8, 4, 2, 1} equal to
// vec (anything else runs V = 1), so a runtime width picks a template width.
template <typename Fn>
void dispatch_vec(int vec, Fn&& fn) {
  switch (vec) {
    case 8:
      fn(std::integral_constant<int, 8>{});
      break;
    case 4:
      fn(std::integral_constant<int, 4>{});
      break;
    case 2:
      fn(std::integral_constant<int, 2>{});
      break;
    default:
      fn(std::integral_constant<int, 1>{});
  }
}
