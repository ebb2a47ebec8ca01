// GATv2 (dynamic attention) aggregation for gfx950: attention weights are
// never stored.
//
//   x_uvf  = zl[u,f] + zr[v,f]
//   s_uvh  = sum_{f in head h} a[h,f] * leaky_relu(x_uvf)
//   alpha  = exp(s_uvh - lse[v,h])              (lse >= row max: no overflow)
//   out[v] = sum_u w_uvh * alpha_uvh * zl[u]
//
// The score is a head-wide dot over D features of BOTH endpoints, so it does
// not reduce to two per-node scalars as GAT's el[u] + er[v] does (gat.hip):
// every pass gathers the rows it needs and recomputes s with a fixed-order
// butterfly. Nothing of size nnz exists in forward or backward, and the
// transpose pass walks the prebuilt CSC without atomics (docs/DESIGN.md).
//
//  - gatv2_fwd     : over the CSR, gathers zl[u]. Online softmax (running
//                    max, sum, acc[]), so ONE gather pass emits out and lse.
//  - gatv2_bwd_dst : over the CSR, gathers zl[u]; emits d_zr[v] and the
//                    per-node pa[v] whose column sum is d_a.
//  - gatv2_bwd_src : over the CSC, gathers g[v], zr[v] and (lse, t)[v];
//                    emits d_zl[u].
//
// With t[v,h] = <g[v,h,:], out[v,h,:]> and, per edge,
//   gz    = <g[v,h,:], zl[u,h,:]>
//   delta = alpha * (w * gz - t[v,h])
//   q_f   = delta * a[h,f] * leaky_relu'(x_f)
// the gradients are d_zl[u] = sum_v (w*alpha*g[v] + q), d_zr[v] = sum_u q and
// pa[v,f] = sum_u delta * leaky_relu(x_f). w is 1, or with attention dropout
// keep(key, u, v, h) / (1 - p) from gat.hip's endpoint hash (attn_util.h);
// the softmax itself (lse) is never masked.
//
// Lane layout. A head's D features are cut into G = D / VEC groups of VEC
// elements (VEC | D: one lane access is one aligned 4..16-byte load). A wave
// is split into 64 / SEG segments of SEG lanes; each segment owns one head
// and lane sl of it holds groups sl, sl + SEG, ... (NV of them), so a wave's
// loads of one row are contiguous. SEG < 64 packs 8, 4 or 2 narrow heads
// (G <= 8, 16, 32) into a wave; the dot is a butterfly over SEG lanes: DPP
// exchanges inside a row of 16 lanes, shuffles across rows. Heads up to
// 64 * NV * VEC <= 1024 wide fit; launchers refuse wider ones.
//
// One fixed set of lanes walks a row's edges in CSR/CSC order and all
// reductions are fixed-order butterflies: results are bitwise reproducible
// and independent of row_order.
//
// Compiler resource report (profiles/README.md, "GATv2 aggregation"): no
// instance uses scratch at the plain 256-thread launch bound, so no instance
// carries a waves-per-SIMD bound of its own; the widest (16 elements per
// lane) run at reduced occupancy by their register count alone.

#include "../common.h"
#include "attn_util.h"
#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <vector>

namespace {

// ld_vec / st_vec, leaky, the drop_* hash, wave_ids, for_edges and the
// host-side input checks are shared with gat.hip
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
// Forward over the CSR: out[r,h,:] = sum_e w * alpha * zl[u_e,h,:] and
// lse[r,h], from one gather of zl[u_e] per edge. Online softmax: (m, sum,
// acc[]) are rescaled once per batch of U edges. The denominator takes every
// edge; only acc sees the dropout weight. Rows without edges get 0 and 0.
// ---------------------------------------------------------------------------
template <typename T, int VEC, int NV, int SEG>
__global__ void __launch_bounds__(256) gatv2_fwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ zl, const T* __restrict__ zr,
    const float* __restrict__ attn, const int32_t* __restrict__ row_order,
    T* __restrict__ out, float* __restrict__ lse, int64_t num_rows, int64_t F,
    int64_t H, int64_t D, int64_t nhg, float slope, uint32_t key,
    uint32_t thr, float scale) {
  constexpr int E = NV * VEC;
  const WaveIds wv = wave_ids();
  const int lane = wv.lane;
  const int64_t npairs = num_rows * nhg;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nhg;
    if (row_order) r = row_order[r];
    const LaneMap<VEC, NV, SEG> lm(lane, pair % nhg, H, D);
    float a[E], zrv[E], acc[E];
    ld_row<float, VEC, NV, SEG>(attn, lm, a);
    ld_row<T, VEC, NV, SEG>(zr + r * F, lm, zrv);
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = 0.f;
    float m = kNegBig, sum = 0.f;
    const uint32_t base = drop_base(static_cast<uint32_t>(r), kDropMulV,
                                    static_cast<uint32_t>(lm.h), key);

    const int64_t e_begin = indptr[r], e_end = indptr[r + 1];
    auto batch = [&](auto n_c, const auto& uu) {
      constexpr int N = decltype(n_c)::value;
      float v[N][E], s[N];
#pragma unroll
      for (int i = 0; i < N; ++i)
        ld_row<T, VEC, NV, SEG>(zl + static_cast<int64_t>(uu[i]) * F, lm,
                                v[i]);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        float p = 0.f;
#pragma unroll
        for (int k = 0; k < E; ++k) p += a[k] * leaky(v[i][k] + zrv[k], slope);
        s[i] = p;
      }
#pragma unroll
      for (int i = 0; i < N; ++i) s[i] = seg_sum<SEG>(s[i]);
      float mn = m;
#pragma unroll
      for (int i = 0; i < N; ++i) mn = fmaxf(mn, s[i]);
      const float c = expf(m - mn);
      m = mn;
      sum *= c;
#pragma unroll
      for (int k = 0; k < E; ++k) acc[k] *= c;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        float p = expf(s[i] - mn);
        sum += p;
        if (thr)
          p *= drop_weight(static_cast<uint32_t>(uu[i]), kDropMulU, base, thr,
                           scale);
#pragma unroll
        for (int k = 0; k < E; ++k) acc[k] += p * v[i][k];
      }
    };
    for_edges<kUnroll<E>>(indices, e_begin, e_end, batch);

    const bool any = e_end > e_begin;
    const float inv = any ? 1.f / sum : 0.f;
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] *= inv;
    st_row<T, VEC, NV, SEG>(out + r * F, lm, acc);
    if (lm.head_ok && (lane & (SEG - 1)) == 0)
      lse[r * H + lm.h] = any ? m + logf(sum) : 0.f;
  }
}

// ---------------------------------------------------------------------------
// Backward over the CSR (row = destination v): gathers zl[u] per edge.
//   d_zr[v,f] = sum_u delta * a[h,f] * leaky_relu'(x_f)
//   pa[v,f]   = sum_u delta * leaky_relu(x_f)            (fp32; d_a = colsum)
// Rows without edges get zeros.
// ---------------------------------------------------------------------------
template <typename T, int VEC, int NV, int SEG>
__global__ void __launch_bounds__(256) gatv2_bwd_dst_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ g, const T* __restrict__ zl,
    const T* __restrict__ zr, const float* __restrict__ attn,
    const float* __restrict__ lse, const float* __restrict__ t,
    const int32_t* __restrict__ row_order, T* __restrict__ d_zr,
    float* __restrict__ pa, int64_t num_rows, int64_t F, int64_t H, int64_t D,
    int64_t nhg, float slope, uint32_t key, uint32_t thr, float scale) {
  constexpr int E = NV * VEC;
  const WaveIds wv = wave_ids();
  const int lane = wv.lane;
  const int64_t npairs = num_rows * nhg;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nhg;
    if (row_order) r = row_order[r];
    const LaneMap<VEC, NV, SEG> lm(lane, pair % nhg, H, D);
    float a[E], zrv[E], gv[E], dzr[E], pav[E];
    ld_row<float, VEC, NV, SEG>(attn, lm, a);
    ld_row<T, VEC, NV, SEG>(zr + r * F, lm, zrv);
    ld_row<T, VEC, NV, SEG>(g + r * F, lm, gv);
#pragma unroll
    for (int k = 0; k < E; ++k) dzr[k] = pav[k] = 0.f;
    const float lse_v = lse[r * H + lm.h];
    const float t_v = t[r * H + lm.h];
    const uint32_t base = drop_base(static_cast<uint32_t>(r), kDropMulV,
                                    static_cast<uint32_t>(lm.h), key);

    auto batch = [&](auto n_c, const auto& uu) {
      constexpr int N = decltype(n_c)::value;
      float v[N][E], s[N], gz[N];
#pragma unroll
      for (int i = 0; i < N; ++i)
        ld_row<T, VEC, NV, SEG>(zl + static_cast<int64_t>(uu[i]) * F, lm,
                                v[i]);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        float p = 0.f, q = 0.f;
#pragma unroll
        for (int k = 0; k < E; ++k) {
          p += a[k] * leaky(v[i][k] + zrv[k], slope);
          q += gv[k] * v[i][k];
        }
        s[i] = p;
        gz[i] = q;
      }
#pragma unroll
      for (int i = 0; i < N; ++i) seg_sum2<SEG>(s[i], gz[i], lane);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float alpha = expf(s[i] - lse_v);
        const float w =
            thr ? drop_weight(static_cast<uint32_t>(uu[i]), kDropMulU, base,
                              thr, scale)
                : 1.f;
        const float delta = alpha * (w * gz[i] - t_v);
#pragma unroll
        for (int k = 0; k < E; ++k) {
          const float x = v[i][k] + zrv[k];
          dzr[k] += delta * a[k] * (x > 0.f ? 1.f : slope);
          pav[k] += delta * leaky(x, slope);
        }
      }
    };
    for_edges<kUnroll<E>>(indices, indptr[r], indptr[r + 1], batch);

    st_row<T, VEC, NV, SEG>(d_zr + r * F, lm, dzr);
    st_row<float, VEC, NV, SEG>(pa + r * F, lm, pav);
  }
}

// ---------------------------------------------------------------------------
// Backward over the CSC (row = source u, columns = destinations v): gathers
// g[v], zr[v] and dst_state[v,h] = (lse, t) per edge.
//   d_zl[u,f] = sum_v (w*alpha*g[v,f] + delta * a[h,f] * leaky_relu'(x_f))
// Sources without edges get zeros.
// ---------------------------------------------------------------------------
template <typename T, int VEC, int NV, int SEG>
__global__ void __launch_bounds__(256) gatv2_bwd_src_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ g, const T* __restrict__ zl,
    const T* __restrict__ zr, const float* __restrict__ attn,
    const f32x2* __restrict__ dst_state,
    const int32_t* __restrict__ row_order, T* __restrict__ d_zl,
    int64_t num_rows, int64_t F, int64_t H, int64_t D, int64_t nhg,
    float slope, uint32_t key, uint32_t thr, float scale) {
  constexpr int E = NV * VEC;
  const WaveIds wv = wave_ids();
  const int lane = wv.lane;
  const int64_t npairs = num_rows * nhg;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nhg;
    if (row_order) r = row_order[r];
    const LaneMap<VEC, NV, SEG> lm(lane, pair % nhg, H, D);
    float a[E], zlu[E], acc[E];
    ld_row<float, VEC, NV, SEG>(attn, lm, a);
    ld_row<T, VEC, NV, SEG>(zl + r * F, lm, zlu);
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = 0.f;
    const uint32_t base = drop_base(static_cast<uint32_t>(r), kDropMulU,
                                    static_cast<uint32_t>(lm.h), key);

    auto batch = [&](auto n_c, const auto& vv) {
      constexpr int N = decltype(n_c)::value;
      float gv[N][E], zrv[N][E], s[N], gz[N];
      f32x2 st[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int64_t v = vv[i];
        st[i] = dst_state[v * H + lm.h];
        ld_row<T, VEC, NV, SEG>(g + v * F, lm, gv[i]);
        ld_row<T, VEC, NV, SEG>(zr + v * F, lm, zrv[i]);
      }
#pragma unroll
      for (int i = 0; i < N; ++i) {
        float p = 0.f, q = 0.f;
#pragma unroll
        for (int k = 0; k < E; ++k) {
          p += a[k] * leaky(zlu[k] + zrv[i][k], slope);
          q += gv[i][k] * zlu[k];
        }
        s[i] = p;
        gz[i] = q;
      }
#pragma unroll
      for (int i = 0; i < N; ++i) seg_sum2<SEG>(s[i], gz[i], lane);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float alpha = expf(s[i] - st[i][0]);
        const float w =
            thr ? drop_weight(static_cast<uint32_t>(vv[i]), kDropMulV, base,
                              thr, scale)
                : 1.f;
        const float delta = alpha * (w * gz[i] - st[i][1]);
        const float wa = w * alpha;
#pragma unroll
        for (int k = 0; k < E; ++k) {
          const float x = zlu[k] + zrv[i][k];
          acc[k] += wa * gv[i][k] + delta * a[k] * (x > 0.f ? 1.f : slope);
        }
      }
    };
    for_edges<kUnroll<E>>(indices, indptr[r], indptr[r + 1], batch);

    st_row<T, VEC, NV, SEG>(d_zl + r * F, lm, acc);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// the shared host checks (attn_util.h), with this op's name in the messages
constexpr const char* kOp = "gatv2";

// a [nodes, F] feature tensor whose heads fit the lane layout
void check_features(const torch::Tensor& x, int64_t rows, int64_t H,
                    const char* name) {
  attn_util::check_features(kOp, x, rows, H, name);
  TORCH_CHECK(x.size(1) / H <= kMaxHeadDim, "gatv2: head width D=",
              x.size(1) / H, " exceeds the supported ", kMaxHeadDim);
}

void check_same(const torch::Tensor& x, const torch::Tensor& like,
                const char* name) {
  TORCH_CHECK(x.size(1) == like.size(1) &&
                  x.scalar_type() == like.scalar_type(),
              "gatv2: ", name, " must agree with zl in width and dtype");
}

void check_attn(const torch::Tensor& attn, int64_t H, int64_t D) {
  TORCH_CHECK(attn.is_cuda() && attn.is_contiguous() &&
                  attn.scalar_type() == torch::kFloat && attn.dim() == 2 &&
                  attn.size(0) == H && attn.size(1) == D,
              "gatv2: attn must be a contiguous fp32 [H, D] = [", H, ", ", D,
              "] tensor");
}

// The lane layout of one head width (file header). 4-element accesses need
// D % 4 == 0, 16-byte (fp32) / 8-byte (bf16) aligned bases and at least 8
// groups (the narrowest segment); narrower heads fill their segment with
// single elements instead.
struct Layout {
  int vec, nv, seg;
};

Layout pick_layout(int64_t D, int64_t elem_size, const torch::Tensor& attn,
                   std::initializer_list<const void*> ptrs) {
  TORCH_CHECK(D >= 1 && D <= kMaxHeadDim, "gatv2: head width D=", D,
              " exceeds the supported ", kMaxHeadDim);
  bool wide = D % 4 == 0 && D >= 32 && aligned_to(attn.data_ptr(), 16);
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
void dispatch_layout(const Layout& l, Fn&& fn) {
#define GATV2_CASE(V, N, S)                                      \
  if (l.vec == V && l.nv == N && l.seg == S) {                   \
    fn(std::integral_constant<int, V>{},                         \
       std::integral_constant<int, N>{},                         \
       std::integral_constant<int, S>{});                        \
    return;                                                      \
  }
  GATV2_CASE(1, 1, 16)
  GATV2_CASE(1, 1, 32)
  GATV2_CASE(1, 1, 64)
  GATV2_CASE(1, 2, 64)
  GATV2_CASE(1, 4, 64)
  GATV2_CASE(1, 8, 64)
  GATV2_CASE(1, 16, 64)
  GATV2_CASE(4, 1, 8)
  GATV2_CASE(4, 1, 16)
  GATV2_CASE(4, 1, 32)
  GATV2_CASE(4, 1, 64)
  GATV2_CASE(4, 2, 64)
  GATV2_CASE(4, 4, 64)
#undef GATV2_CASE
  TORCH_CHECK(false, "gatv2: no kernel for layout vec=", l.vec,
              " nv=", l.nv, " seg=", l.seg);
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

// One launch of a wave-per-(row, head group) kernel over `indptr`'s rows:
// the lane layout from the head width and the alignment of `ptrs`, the grid,
// the launch and its check. kernel_of(VEC, NV, SEG as integral constants)
// returns the instance; `mid` are the kernel's arguments between the graph
// and the sizes (the three kernels share what comes before and after).
template <typename KernelOf, typename... Mid>
void launch(const torch::Tensor& indptr, const torch::Tensor& indices,
            const torch::Tensor& zl, int64_t H, const torch::Tensor& attn,
            std::initializer_list<const void*> ptrs, float slope,
            DropArgs drop, KernelOf&& kernel_of, Mid... mid) {
  const int64_t num_rows = indptr.numel() - 1, F = zl.size(1), D = F / H;
  const Layout l = pick_layout(D, zl.element_size(), attn, ptrs);
  dispatch_layout(l, [&](auto vec_c, auto nv_c, auto seg_c) {
    constexpr int SEG = decltype(seg_c)::value;
    const int64_t hpw = kWave / SEG, nhg = (H + hpw - 1) / hpw;
    const int threads = 256;
    hipLaunchKernelGGL(kernel_of(vec_c, nv_c, seg_c),
                       dim3(grid_for(num_rows * nhg, threads)), dim3(threads),
                       0, current_stream(), indptr.data_ptr<int64_t>(),
                       indices.data_ptr<int32_t>(), mid..., num_rows, F, H, D,
                       nhg, slope, drop.key, drop.thr, drop.scale);
  });
  check_launch();
}

// kernel_of for launch(): the <T, VEC, NV, SEG> instance of a kernel template
#define GATV2_KERNEL_OF(kernel, T)                                     \
  [](auto vec_c, auto nv_c, auto seg_c) {                              \
    return kernel<T, decltype(vec_c)::value, decltype(nv_c)::value,    \
                  decltype(seg_c)::value>;                             \
  }

}  // namespace

std::vector<torch::Tensor> gatv2_fwd_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor zl,
    torch::Tensor zr, torch::Tensor attn, torch::Tensor row_order,
    int64_t num_cols, int64_t H, double slope, int64_t drop_key,
    int64_t drop_thr, double drop_scale) {
  check_graph(kOp, indptr, indices);
  const DropArgs drop = drop_args(kOp, drop_key, drop_thr, drop_scale);
  const int64_t num_rows = indptr.numel() - 1;
  check_features(zl, num_cols, H, "zl");
  check_features(zr, num_rows, H, "zr");
  check_same(zr, zl, "zr");
  const int64_t F = zl.size(1);
  check_attn(attn, H, F / H);
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto out = torch::empty({num_rows, F}, zl.options());
  auto lse = torch::empty({num_rows, H}, attn.options());
  if (num_rows == 0) return {out, lse};
  dispatch_dtype(zl, [&](auto tag) {
    using T = decltype(tag);
    launch(indptr, indices, zl, H, attn,
           {zl.data_ptr(), zr.data_ptr(), out.data_ptr()},
           static_cast<float>(slope), drop,
           GATV2_KERNEL_OF(gatv2_fwd_kernel, T), cptr<T>(zl), cptr<T>(zr),
           attn.data_ptr<float>(), rop, mptr<T>(out), lse.data_ptr<float>());
  });
  return {out, lse};
}

std::vector<torch::Tensor> gatv2_bwd_dst_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor g,
    torch::Tensor zl, torch::Tensor zr, torch::Tensor attn, torch::Tensor lse,
    torch::Tensor t, torch::Tensor row_order, int64_t num_cols, int64_t H,
    double slope, int64_t drop_key, int64_t drop_thr, double drop_scale) {
  check_graph(kOp, indptr, indices);
  const DropArgs drop = drop_args(kOp, drop_key, drop_thr, drop_scale);
  const int64_t num_rows = indptr.numel() - 1;
  check_features(zl, num_cols, H, "zl");
  check_features(zr, num_rows, H, "zr");
  check_features(g, num_rows, H, "g");
  check_same(zr, zl, "zr");
  check_same(g, zl, "g");
  const int64_t F = zl.size(1);
  check_attn(attn, H, F / H);
  check_node_table(kOp, lse, num_rows, H, "lse");
  check_node_table(kOp, t, num_rows, H, "t");
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto d_zr = torch::empty({num_rows, F}, zl.options());
  auto pa = torch::empty({num_rows, F}, attn.options());
  if (num_rows == 0) return {d_zr, pa};
  dispatch_dtype(zl, [&](auto tag) {
    using T = decltype(tag);
    launch(indptr, indices, zl, H, attn,
           {zl.data_ptr(), zr.data_ptr(), g.data_ptr(), d_zr.data_ptr()},
           static_cast<float>(slope), drop,
           GATV2_KERNEL_OF(gatv2_bwd_dst_kernel, T), cptr<T>(g), cptr<T>(zl),
           cptr<T>(zr), attn.data_ptr<float>(), lse.data_ptr<float>(),
           t.data_ptr<float>(), rop, mptr<T>(d_zr), pa.data_ptr<float>());
  });
  return {d_zr, pa};
}

torch::Tensor gatv2_bwd_src_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor g,
    torch::Tensor zl, torch::Tensor zr, torch::Tensor attn, torch::Tensor lse,
    torch::Tensor t, torch::Tensor row_order, int64_t num_cols, int64_t H,
    double slope, int64_t drop_key, int64_t drop_thr, double drop_scale) {
  // indptr/indices are the CSC: rows = source nodes, columns = destinations
  check_graph(kOp, indptr, indices);
  const DropArgs drop = drop_args(kOp, drop_key, drop_thr, drop_scale);
  const int64_t num_rows = indptr.numel() - 1;
  check_features(zl, num_rows, H, "zl");
  check_features(zr, num_cols, H, "zr");
  check_features(g, num_cols, H, "g");
  check_same(zr, zl, "zr");
  check_same(g, zl, "g");
  const int64_t F = zl.size(1);
  check_attn(attn, H, F / H);
  check_node_table(kOp, lse, num_cols, H, "lse");
  check_node_table(kOp, t, num_cols, H, "t");
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto d_zl = torch::empty({num_rows, F}, zl.options());
  if (num_rows == 0) return d_zl;
  // (lse, t) per destination and head: one 8-byte gather per edge
  auto dst_state = torch::stack({lse.narrow(0, 0, num_cols),
                                 t.narrow(0, 0, num_cols)},
                                2)
                       .contiguous();
  TORCH_CHECK(aligned_to(dst_state.data_ptr(), 8));
  dispatch_dtype(zl, [&](auto tag) {
    using T = decltype(tag);
    launch(indptr, indices, zl, H, attn,
           {zl.data_ptr(), zr.data_ptr(), g.data_ptr(), d_zl.data_ptr()},
           static_cast<float>(slope), drop,
           GATV2_KERNEL_OF(gatv2_bwd_src_kernel, T), cptr<T>(g), cptr<T>(zl),
           cptr<T>(zr), attn.data_ptr<float>(),
           reinterpret_cast<const f32x2*>(dst_state.data_ptr<float>()), rop,
           mptr<T>(d_zl));
  });
  return d_zl;
}
