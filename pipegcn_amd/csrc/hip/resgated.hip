// Residual gated graph conv aggregation (Bresson & Laurent 2017; PyG's
// ResGatedGraphConv, the message function of GatedGCN) for gfx950, and its
// backward (docs/DESIGN.md, "Residual gated aggregation"). Per column c, over
// the edges u -> v of row v (parallel edges counted):
//
//   s_uv[c]  = sigmoid(k[v,c] + Q[u,c])              qv[u] = [Q[u] | V[u]]
//   out[v,c] = inv_deg[v] * sum_u s_uv[c] * V[u,c]   (inv_deg absent: the sum)
//
// The weight is a per-channel gate, not normalised over the neighbourhood, so
// no pass needs a row statistic: each one recomputes the gate from the rows it
// gathers and nothing of size nnz exists in forward or backward. Q and V of a
// source are the two halves of ONE record of width 2F (dot_attn.hip's kv): a
// source's two loads hit adjacent memory and both gradients come back as one
// [nodes, 2F] tensor.
//
//  - resgated_dst<false> : forward over the CSR. The lane holds its columns of
//      k[v]; per edge it loads its slices of Q[u] and V[u] (base qv + u * 2F,
//      second half at + F), forms the gate and does one FMA.
//  - resgated_dst<true>  : backward A over the CSR, the same walk and gathers:
//      d_k[v] = inv_deg[v] g[v] * sum_u s (1 - s) V[u].
//  - resgated_prep       : dst[v] = [k[v] | gs[v]], gs = inv_deg[v] g[v]: the
//      destination-side record of backward B, one pass over [num_dst, F].
//  - resgated_src        : backward B over the CSC (row = source u, columns =
//      destinations v). The lane holds Q[u] and V[u]; per entry it gathers
//      the one record dst[v]:
//        dV += s gs        t += s (1 - s) gs        dQ = V[u] * t
//      stored as the two halves of d_qv[u]. Gathering k[v] and g[v] as two
//      rows with a scalar inv_deg[v] was measured 2-8 % slower, the prep
//      pass included (profiles/README.md).
//
// The gate. With kLog2e folded into the held row, each gate is one v_exp_f32
// and one v_rcp_f32: s = 1 / (1 + exp2(-(k + q) log2e)). Where |k + q| is
// large exp2 gives 0 or +inf, the reciprocal exactly 1 or 0, and s (1 - s)
// exactly 0: never NaN. (e / (1 + e)^2 would be inf / inf there.)
//
// Scheduling is spmm_softmax.hip's: one wave per (row, chunk of 64 * VEC
// columns), the wave index in a scalar register, grid-stride over row_order,
// four edges in flight (for_edges<4>) with all their loads issued before the
// first use, non-temporal stores, no LDS and no atomics. One fixed lane owns a
// column and walks the row in stored order: results are bitwise reproducible
// and independent of row_order. VEC divides F, so the record's second half
// takes the same lane access as its first (the host checks both pointers).
//
// Compiler resource report: profiles/README.md, "Residual gated aggregation".
// No instance uses scratch.

#include "../common.h"
#include "attn_util.h"
#include "gather_lanes.h"
#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace {

using namespace attn_util;
using namespace gather_lanes;

constexpr float kNegLog2e = -1.44269504088896340736f;
constexpr int kThreads = 256;  // launch_of's block
constexpr int kInFlight = 4;   // edges whose two row loads are issued together

// sigmoid(z) from x = -z * log2(e): exactly 1 where exp2 underflows, exactly
// 0 where it overflows (file header)
__device__ __forceinline__ float gate_of(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x));
}

// ---------------------------------------------------------------------------
// Over the CSR (row = destination v, columns = sources u). DK = false is the
// forward: out[v] = scale_v * sum_u s V[u]. DK = true is backward A:
// d_k[v] = scale_v g[v] * sum_u s (1 - s) V[u]. scale_v = inv_deg[v], or 1
// without inv_deg. Rows without edges get zeros.
// ---------------------------------------------------------------------------
template <typename T, int VEC, bool DK>
__global__ void __launch_bounds__(kThreads) resgated_dst_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ k, const T* __restrict__ qv,
    const T* __restrict__ g, const float* __restrict__ inv_deg,
    const int32_t* __restrict__ row_order, T* __restrict__ out,
    int64_t num_rows, int64_t F, int64_t nchunks) {
  const UniformWave wv = uniform_wave();
  const int64_t npairs = num_rows * nchunks;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nchunks;
    if (row_order) r = row_order[r];
    // VEC divides F (host check): a lane is all inside the row or all past it
    const int64_t f0 = pair % nchunks * (kWave * VEC) + wv.lane * VEC;
    if (f0 >= F) continue;

    float nk[VEC], acc[VEC];
    ld_vec<T, VEC>(k + r * F + f0, nk);
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      nk[c] *= kNegLog2e;
      acc[c] = 0.f;
    }

    const T* rec0 = qv + f0;
    auto batch = [&](auto n_c, const auto& uu) {
      constexpr int NB = decltype(n_c)::value;
      float qq[NB][VEC], vv[NB][VEC];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const T* rec = rec0 + static_cast<int64_t>(uu[i]) * (2 * F);
        ld_vec<T, VEC>(rec, qq[i]);
        ld_vec<T, VEC>(rec + F, vv[i]);
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
          const float s = gate_of(fmaf(qq[i][c], kNegLog2e, nk[c]));
          acc[c] = fmaf(DK ? s * (1.f - s) : s, vv[i][c], acc[c]);
        }
      }
    };
    for_edges<kInFlight>(indices, indptr[r], indptr[r + 1], batch);

    const float scale = inv_deg ? inv_deg[r] : 1.f;  // wave-uniform
    if constexpr (DK) {
      float gv[VEC];
      ld_vec<T, VEC>(g + r * F + f0, gv);
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[c] *= scale * gv[c];
    } else {
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[c] *= scale;
    }
    st_vec<T, VEC>(out + r * F + f0, acc);
  }
}

// ---------------------------------------------------------------------------
// Destination records of backward B: dst[v] = [k[v] | inv_deg[v] g[v]], one
// pass over [num_rows, F] that also folds inv_deg in.
// ---------------------------------------------------------------------------
template <typename T, int VEC>
__global__ void __launch_bounds__(kThreads) resgated_prep_kernel(
    const T* __restrict__ k, const T* __restrict__ g,
    const float* __restrict__ inv_deg, T* __restrict__ dst, int64_t num_rows,
    int64_t F, int64_t nchunks) {
  const UniformWave wv = uniform_wave();
  const int64_t npairs = num_rows * nchunks;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    const int64_t r = pair / nchunks;
    const int64_t f0 = pair % nchunks * (kWave * VEC) + wv.lane * VEC;
    if (f0 >= F) continue;
    float kk[VEC], gs[VEC];
    ld_vec<T, VEC>(k + r * F + f0, kk);
    ld_vec<T, VEC>(g + r * F + f0, gs);
    const float scale = inv_deg ? inv_deg[r] : 1.f;  // wave-uniform
#pragma unroll
    for (int c = 0; c < VEC; ++c) gs[c] *= scale;
    T* o = dst + r * (2 * F) + f0;
    st_vec<T, VEC>(o, kk);
    st_vec<T, VEC>(o + F, gs);
  }
}

// ---------------------------------------------------------------------------
// Backward B over the CSC (row = source u, columns = destinations v): holds
// the record qv[u], gathers the record dst[v] = [k[v] | gs[v]] per entry;
// writes d_qv[u] = [dQ | dV]. Source rows without entries get zeros.
// ---------------------------------------------------------------------------
template <typename T, int VEC>
__global__ void __launch_bounds__(kThreads) resgated_src_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ dst, const T* __restrict__ qv,
    const int32_t* __restrict__ row_order, T* __restrict__ d_qv,
    int64_t num_rows, int64_t F, int64_t nchunks) {
  const UniformWave wv = uniform_wave();
  const int64_t npairs = num_rows * nchunks;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nchunks;
    if (row_order) r = row_order[r];
    const int64_t f0 = pair % nchunks * (kWave * VEC) + wv.lane * VEC;
    if (f0 >= F) continue;

    float nq[VEC], vu[VEC], dv[VEC], t[VEC];
    const T* held = qv + r * (2 * F) + f0;
    ld_vec<T, VEC>(held, nq);
    ld_vec<T, VEC>(held + F, vu);
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      nq[c] *= kNegLog2e;
      dv[c] = t[c] = 0.f;
    }

    const T* rec0 = dst + f0;
    auto batch = [&](auto n_c, const auto& dd) {
      constexpr int NB = decltype(n_c)::value;
      float kk[NB][VEC], gs[NB][VEC];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const T* rec = rec0 + static_cast<int64_t>(dd[i]) * (2 * F);
        ld_vec<T, VEC>(rec, kk[i]);
        ld_vec<T, VEC>(rec + F, gs[i]);
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
          const float s = gate_of(fmaf(kk[i][c], kNegLog2e, nq[c]));
          dv[c] = fmaf(s, gs[i][c], dv[c]);
          t[c] = fmaf(s * (1.f - s), gs[i][c], t[c]);
        }
      }
    };
    for_edges<kInFlight>(indices, indptr[r], indptr[r + 1], batch);

#pragma unroll
    for (int c = 0; c < VEC; ++c) t[c] *= vu[c];
    T* o = d_qv + r * (2 * F) + f0;
    st_vec<T, VEC>(o, t);
    st_vec<T, VEC>(o + F, dv);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

constexpr const char* kOp = "resgated";

// qv / d_qv: [>= rows, 2F] records of k's dtype, Q in the first F columns
void check_qv(const torch::Tensor& qv, const torch::Tensor& k, int64_t rows) {
  check_features(kOp, qv, rows, 2, "qv");
  TORCH_CHECK(qv.size(1) == 2 * k.size(1) &&
                  qv.scalar_type() == k.scalar_type(),
              kOp, ": qv must be [nodes, 2F] = [Q | V] of k's dtype, got width ",
              qv.size(1), " for F=", k.size(1));
}

// null without inv_deg (the plain sum); else fp32 [>= rows] on the device
const float* inv_deg_ptr(const torch::Tensor& inv_deg, int64_t rows) {
  if (!inv_deg.defined() || inv_deg.numel() == 0) return nullptr;
  TORCH_CHECK(inv_deg.is_cuda() && inv_deg.is_contiguous() &&
                  inv_deg.dim() == 1 &&
                  inv_deg.scalar_type() == torch::kFloat &&
                  inv_deg.numel() >= rows,
              kOp, ": inv_deg must be a contiguous fp32 vector with one entry "
                   "per destination (", rows, ")");
  return inv_deg.data_ptr<float>();
}

// the record's second half, F elements into the row
const void* half_of(const torch::Tensor& rec, int64_t F) {
  return static_cast<const char*>(rec.data_ptr()) + F * rec.element_size();
}

// forward (g undefined) or backward A over the CSR
torch::Tensor run_dst(const torch::Tensor& indptr,
                      const torch::Tensor& indices, const torch::Tensor* g,
                      const torch::Tensor& k, const torch::Tensor& qv,
                      const torch::Tensor& inv_deg,
                      const torch::Tensor& row_order, int64_t num_cols) {
  check_graph(kOp, indptr, indices);
  const int64_t num_rows = indptr.numel() - 1;
  check_features(kOp, k, num_rows, 1, "k");
  check_qv(qv, k, num_cols);
  const int64_t F = k.size(1);
  if (g) {
    check_features(kOp, *g, num_rows, 1, "g");
    TORCH_CHECK(g->size(1) == F && g->scalar_type() == k.scalar_type(), kOp,
                ": g must agree with k in width and dtype");
  }
  const float* ip = inv_deg_ptr(inv_deg, num_rows);
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto out = torch::empty({num_rows, F}, k.options());
  if (num_rows == 0) return out;
  const int vec = lane_vec(kOp, F, num_rows, k.element_size(),
                           {k.data_ptr(), qv.data_ptr(), half_of(qv, F),
                            g ? g->data_ptr() : nullptr, out.data_ptr()},
                           {});
  const Launch l = launch_of(num_rows, F, vec);
  dispatch(k, vec, [&](auto tag, auto v) {
    using T = decltype(tag);
    constexpr int V = decltype(v)::value;
    auto run = [&](auto kern, const T* gp) {
      hipLaunchKernelGGL(kern, l.grid, l.block, 0, current_stream(),
                         indptr.data_ptr<int64_t>(),
                         indices.data_ptr<int32_t>(), cptr<T>(k), cptr<T>(qv),
                         gp, ip, rop, mptr<T>(out), num_rows, F, l.nchunks);
    };
    if (g)
      run(HIP_KERNEL_NAME(resgated_dst_kernel<T, V, true>), cptr<T>(*g));
    else
      run(HIP_KERNEL_NAME(resgated_dst_kernel<T, V, false>), nullptr);
  });
  check_launch();
  return out;
}

}  // namespace

torch::Tensor resgated_fwd_hip(torch::Tensor indptr, torch::Tensor indices,
                               torch::Tensor k, torch::Tensor qv,
                               torch::Tensor inv_deg, torch::Tensor row_order,
                               int64_t num_cols) {
  return run_dst(indptr, indices, nullptr, k, qv, inv_deg, row_order,
                 num_cols);
}

torch::Tensor resgated_bwd_dst_hip(torch::Tensor indptr, torch::Tensor indices,
                                   torch::Tensor g, torch::Tensor k,
                                   torch::Tensor qv, torch::Tensor inv_deg,
                                   torch::Tensor row_order, int64_t num_cols) {
  return run_dst(indptr, indices, &g, k, qv, inv_deg, row_order, num_cols);
}

torch::Tensor resgated_bwd_src_hip(torch::Tensor indptr, torch::Tensor indices,
                                   torch::Tensor g, torch::Tensor k,
                                   torch::Tensor qv, torch::Tensor inv_deg,
                                   torch::Tensor row_order, int64_t num_cols) {
  // indptr/indices are the CSC: rows = source nodes, columns = destinations
  check_graph(kOp, indptr, indices);
  const int64_t num_rows = indptr.numel() - 1;
  check_features(kOp, k, num_cols, 1, "k");
  check_features(kOp, g, num_cols, 1, "g");
  TORCH_CHECK(g.size(1) == k.size(1) && g.scalar_type() == k.scalar_type(),
              kOp, ": g must agree with k in width and dtype");
  check_qv(qv, k, num_rows);
  const int64_t F = k.size(1);
  const float* ip = inv_deg_ptr(inv_deg, num_cols);
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto d_qv = torch::empty({num_rows, 2 * F}, qv.options());
  if (num_rows == 0) return d_qv;
  // [k | inv_deg g] per destination: one record gather per entry
  auto dst = torch::empty({num_cols, 2 * F}, k.options());
  const int vec = lane_vec(kOp, F, num_rows, k.element_size(),
                           {k.data_ptr(), g.data_ptr(), dst.data_ptr(),
                            half_of(dst, F), qv.data_ptr(), half_of(qv, F),
                            d_qv.data_ptr(), half_of(d_qv, F)},
                           {});
  const Launch lp = launch_of(num_cols, F, vec);
  const Launch l = launch_of(num_rows, F, vec);
  dispatch(k, vec, [&](auto tag, auto v) {
    using T = decltype(tag);
    constexpr int V = decltype(v)::value;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(resgated_prep_kernel<T, V>), lp.grid,
                       lp.block, 0, current_stream(), cptr<T>(k), cptr<T>(g),
                       ip, mptr<T>(dst), num_cols, F, lp.nchunks);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(resgated_src_kernel<T, V>), l.grid,
                       l.block, 0, current_stream(),
                       indptr.data_ptr<int64_t>(), indices.data_ptr<int32_t>(),
                       cptr<T>(dst), cptr<T>(qv), rop, mptr<T>(d_qv), num_rows,
                       F, l.nchunks);
  });
  check_launch();
  return d_qv;
}
