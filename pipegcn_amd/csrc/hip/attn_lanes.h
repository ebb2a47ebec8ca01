// The lane layout shared by the attention kernels whose score is a head-wide
// dot over gathered rows (gatv2.hip, dot_attn.hip). Device side: the DPP
// segment butterflies, the LaneMap and the row loads/stores built on it.
// Host side: the layout choice, its dispatch over the compiled instances and
// the one launch of a wave-per-(row, head group) kernel. As in attn_util.h
// everything on the device side is force-inlined, so each .hip gets exactly
// the code it had when these lived in gatv2.hip's anonymous namespace.
//
// Lane layout. A head's D features are cut into G = D / VEC groups of VEC
// elements (VEC | D: one lane access is one aligned 4..16-byte load). A wave
// is split into 64 / SEG segments of SEG lanes; each segment owns one head
// and lane sl of it holds groups sl, sl + SEG, ... (NV of them), so a wave's
// loads of one row are contiguous. SEG < 64 packs 8, 4 or 2 narrow heads
// (G <= 8, 16, 32) into a wave; the dot is a butterfly over SEG lanes: DPP
// exchanges inside a row of 16 lanes, shuffles across rows. Heads up to
// 64 * NV * VEC <= 1024 wide fit.
#pragma once

#include "attn_util.h"
#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <type_traits>

namespace attn_lanes {

using namespace attn_util;

// finite stand-in for -inf: exp(kNegBig - s) is 0, not NaN
constexpr float kNegBig = -1e30f;
// widest head the lane layout holds: 64 lanes x 16 elements
constexpr int64_t kMaxHeadDim = 1024;

using f32x2 = __attribute__((ext_vector_type(2))) float;

// edges whose gathered rows are in flight together: four at up to 4 elements
// per lane (as the SpMM), fewer when a lane already issues 8 or 16 loads
template <int E>
constexpr int kUnroll = E <= 4 ? 4 : (E <= 8 ? 2 : 1);

// One DPP lane exchange inside a row of 16 lanes: a VALU operand modifier,
// not an LDS round trip like __shfl_xor's ds_bpermute.
template <int CTRL>
__device__ __forceinline__ float dpp(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(
      0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
constexpr int kQuadXor1 = 0xB1;     // quad_perm [1,0,3,2]
constexpr int kQuadXor2 = 0x4E;     // quad_perm [2,3,0,1]
constexpr int kHalfMirror = 0x141;  // lane i <- lane 7 - i of its 8
constexpr int kRowMirror = 0x140;   // lane i <- lane 15 - i of its 16

// Fixed-order sum over 8 lanes: after the two quad steps a quad's lanes
// agree, so the mirror partner carries the other quad's sum.
__device__ __forceinline__ float oct_sum(float x) {
  x += dpp<kQuadXor1>(x);
  x += dpp<kQuadXor2>(x);
  x += dpp<kHalfMirror>(x);
  return x;
}

// fixed-order sum over the SEG lanes of a segment: every lane of it ends
// with the same total. Rows of 16 reduce by DPP, rows combine by shuffles.
template <int SEG>
__device__ __forceinline__ float seg_sum(float x) {
  x = oct_sum(x);
  if constexpr (SEG >= 16) x += dpp<kRowMirror>(x);
#pragma unroll
  for (int off = 16; off < SEG; off <<= 1) x += __shfl_xor(x, off, kWave);
  return x;
}

// Two segment sums for the price of one plus two exchanges: the first step
// leaves a's partial sums in the lower half of the segment and b's in the
// upper half, the halves reduce separately, the last step swaps the totals.
template <int SEG>
__device__ __forceinline__ void seg_sum2(float& a, float& b, int lane) {
  const bool hi = lane & (SEG / 2);
  float keep = hi ? b : a;
  const float send = hi ? a : b;
  float other;
  if constexpr (SEG == 8) {
    keep += dpp<kHalfMirror>(send);
    keep += dpp<kQuadXor1>(keep);
    keep += dpp<kQuadXor2>(keep);
    other = dpp<kHalfMirror>(keep);
  } else if constexpr (SEG == 16) {
    keep += dpp<kRowMirror>(send);
    keep = oct_sum(keep);
    other = dpp<kRowMirror>(keep);
  } else {
    keep += __shfl_xor(send, SEG / 2, kWave);
    keep = seg_sum<SEG / 2>(keep);
    other = __shfl_xor(keep, SEG / 2, kWave);
  }
  a = hi ? other : keep;
  b = hi ? keep : other;
}

// Where this lane's NV groups of head `h` start inside a [*, F] row, and
// which of them exist. A lane of a segment whose head is past H owns nothing
// but still takes part in the butterflies.
template <int VEC, int NV, int SEG>
struct LaneMap {
  int off[NV];
  bool ok[NV];
  int64_t h;  // clamped to a valid head for the per-head scalar loads
  bool head_ok;

  __device__ __forceinline__ LaneMap(int lane, int64_t hgroup, int64_t H,
                                     int64_t D) {
    const int sl = lane & (SEG - 1);
    h = hgroup * (kWave / SEG) + lane / SEG;
    head_ok = h < H;
    if (!head_ok) h = H - 1;
    const int G = static_cast<int>(D / VEC);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int grp = k * SEG + sl;
      ok[k] = head_ok && grp < G;
      off[k] = static_cast<int>(h * D) + (ok[k] ? grp : 0) * VEC;
    }
  }
};

// this lane's E = NV * VEC elements of one row; groups it does not own are 0
template <typename T, int VEC, int NV, int SEG>
__device__ __forceinline__ void ld_row(const T* row,
                                       const LaneMap<VEC, NV, SEG>& lm,
                                       float (&v)[NV * VEC]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float t[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) t[j] = 0.f;
    if (lm.ok[k]) ld_vec<T, VEC>(row + lm.off[k], t);
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[k * VEC + j] = t[j];
  }
}

template <typename T, int VEC, int NV, int SEG>
__device__ __forceinline__ void st_row(T* row,
                                       const LaneMap<VEC, NV, SEG>& lm,
                                       const float (&v)[NV * VEC]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float t[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) t[j] = v[k * VEC + j];
    if (lm.ok[k]) st_vec<T, VEC>(row + lm.off[k], t);
  }
}

// ---------------------------------------------------------------------------
// host side: `op` ("gatv2" / "dot") prefixes every message
// ---------------------------------------------------------------------------

// The lane layout of one head width (file header). 4-element accesses need
// D % 4 == 0, 16-byte (fp32) / 8-byte (bf16) aligned bases and at least 8
// groups (the narrowest segment); narrower heads fill their segment with
// single elements instead.
struct Layout {
  int vec, nv, seg;
};

// `ptrs` are the bases of the [*, F] element rows; `f32_ptr` (may be null)
// is an fp32 row read with the same lane map, which wants 16 bytes.
inline Layout pick_layout(const char* op, int64_t D, int64_t elem_size,
                          const void* f32_ptr,
                          std::initializer_list<const void*> ptrs) {
  TORCH_CHECK(D >= 1 && D <= kMaxHeadDim, op, ": head width D=", D,
              " exceeds the supported ", kMaxHeadDim);
  bool wide = D % 4 == 0 && D >= 32 && aligned_to(f32_ptr, 16);
  for (const void* p : ptrs) wide = wide && aligned_to(p, 4 * elem_size);
  Layout l;
  l.vec = wide ? 4 : 1;
  const int64_t G = D / l.vec;
  l.seg = G <= 8 ? 8 : (G <= 16 ? 16 : (G <= 32 ? 32 : 64));
  if (l.vec == 1 && l.seg == 8) l.seg = 16;  // 1-wide: compiled from 16 up
  l.nv = 1;
  while (static_cast<int64_t>(l.nv) * kWave < G) l.nv *= 2;
  return l;
}

// fn(VEC, NV, SEG as integral constants) for the compiled layouts
template <typename Fn>
void dispatch_layout(const char* op, const Layout& l, Fn&& fn) {
#define ATTN_LANES_CASE(V, N, S)                                 \
  if (l.vec == V && l.nv == N && l.seg == S) {                   \
    fn(std::integral_constant<int, V>{},                         \
       std::integral_constant<int, N>{},                         \
       std::integral_constant<int, S>{});                        \
    return;                                                      \
  }
  ATTN_LANES_CASE(1, 1, 16)
  ATTN_LANES_CASE(1, 1, 32)
  ATTN_LANES_CASE(1, 1, 64)
  ATTN_LANES_CASE(1, 2, 64)
  ATTN_LANES_CASE(1, 4, 64)
  ATTN_LANES_CASE(1, 8, 64)
  ATTN_LANES_CASE(1, 16, 64)
  ATTN_LANES_CASE(4, 1, 8)
  ATTN_LANES_CASE(4, 1, 16)
  ATTN_LANES_CASE(4, 1, 32)
  ATTN_LANES_CASE(4, 1, 64)
  ATTN_LANES_CASE(4, 2, 64)
  ATTN_LANES_CASE(4, 4, 64)
#undef ATTN_LANES_CASE
  TORCH_CHECK(false, op, ": no kernel for layout vec=", l.vec, " nv=", l.nv,
              " seg=", l.seg);
}

template <typename T>
const T* cptr(const torch::Tensor& x) {
  return reinterpret_cast<const T*>(x.data_ptr());
}
template <typename T>
T* mptr(torch::Tensor& x) {
  return reinterpret_cast<T*>(x.data_ptr());
}

// fn(T{}) for the element type T of x (fp32 or bf16: check_features)
template <typename Fn>
void dispatch_dtype(const torch::Tensor& x, Fn&& fn) {
  if (x.scalar_type() == torch::kBFloat16)
    fn(__hip_bfloat16{});
  else
    fn(float{});
}

// One launch of a wave-per-(row, head group) kernel over `indptr`'s rows in
// layout `l`: the grid, the launch and its check. F = H * D is the width of
// the rows the lane map indexes. kernel_of(VEC, NV, SEG as integral
// constants) returns the instance; `mid` are the kernel's arguments between
// the graph and the sizes, `param` its one float between the sizes and the
// dropout (GATv2's slope, the dot kernels' score scale): the kernels share
// what comes before and after.
template <typename KernelOf, typename... Mid>
void launch(const char* op, const Layout& l, const torch::Tensor& indptr,
            const torch::Tensor& indices, int64_t F, int64_t H, float param,
            DropArgs drop, KernelOf&& kernel_of, Mid... mid) {
  const int64_t num_rows = indptr.numel() - 1, D = F / H;
  dispatch_layout(op, l, [&](auto vec_c, auto nv_c, auto seg_c) {
    constexpr int SEG = decltype(seg_c)::value;
    const int64_t hpw = kWave / SEG, nhg = (H + hpw - 1) / hpw;
    const int threads = 256;
    hipLaunchKernelGGL(kernel_of(vec_c, nv_c, seg_c),
                       dim3(grid_for(num_rows * nhg, threads)), dim3(threads),
                       0, current_stream(), indptr.data_ptr<int64_t>(),
                       indices.data_ptr<int32_t>(), mid..., num_rows, F, H, D,
                       nhg, param, drop.key, drop.thr, drop.scale);
  });
  check_launch();
}

// kernel_of for launch(): the <T, VEC, NV, SEG> instance of a kernel template
#define ATTN_LANES_KERNEL_OF(kernel, T)                                \
  [](auto vec_c, auto nv_c, auto seg_c) {                              \
    return kernel<T, decltype(vec_c)::value, decltype(nv_c)::value,    \
                  decltype(seg_c)::value>;                             \
  }

}  // namespace attn_lanes
