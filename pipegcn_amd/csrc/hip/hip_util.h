// Pieces shared by the .hip sources: error checks, the current stream,
// the MFMA 32x32 fp32 accumulator layout and the vector-width dispatch.
// Each .hip still includes <hip/hip_runtime.h> itself: the build's source
// translation step writes a *_hip.hip copy of any file that does not name it.
#pragma once

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

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
