// GCNII propagation (Chen et al. 2020, "Simple and Deep Graph Convolutional
// Networks"; PyG's GCN2Conv) for gfx950, and its backward (docs/DESIGN.md,
// "GCNII propagation"). With d = deg^{-1/2} over all local rows and the edges
// u -> v of row v (parallel edges counted):
//
//   P[v] = (1 - alpha) d[v] sum_u d[u] h[u]  +  alpha h0[v]
//
// The identity mapping out = (1 - beta) P + beta P W^T is a GEMM and stays
// outside; these kernels are the symmetric-normalised gather with the initial
// residual in its epilogue, so that no [N, F] pass runs beside it.
//
//  - gcn2_gather<SRC, true>  : forward over the CSR. The lane loads its
//      columns of h0[v] first, so that the load is in flight under the edge
//      walk, sums d[u] h[u] (SRC: one scalar d[u] per edge) or rows that the
//      caller scaled already (!SRC), and stores
//      fma((1 - alpha) d[v], acc, alpha h0[v]) once. A row without edges
//      gives alpha h0[v].
//  - gcn2_prep               : one pass over dP [num_dst, F]:
//      gs[v] = (1 - alpha) d[v] dP[v], the row the transposed gather reads,
//      and dh0[v] += alpha dP[v] in place into an fp32 buffer that all GCNII
//      layers of a step share (one read of dP, one write, one
//      read-modify-write).
//  - gcn2_gather<false, false> : backward over the CSC (row = source u):
//      dh[u] = d[u] sum_v gs[v]. No atomics, nothing of size nnz.
//
// The sum takes the edges in the dense SpMM's order and grouping (peel to a
// 4-aligned edge, then four per step, then the tail), so alpha = 0 is that
// kernel's result with both scales up to how the compiler contracts the
// products (not bit for bit: measured). The epilogue is one fma, so alpha = 1
// returns h0 bit for bit (0 * acc + h0).
//
// Scheduling is resgated.hip's: one wave per (row, chunk of 64 * VEC
// columns), the wave index in a scalar register, grid-stride over row_order,
// four edges in flight (for_edges<4>) with all their loads issued before the
// first use, non-temporal stores, no LDS and no atomics. One fixed lane owns a
// column and walks the row in stored order: results are bitwise reproducible
// and independent of row_order. VEC divides F.
//
// Compiler resource report: profiles/README.md, "GCNII propagation".

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

constexpr int kThreads = 256;  // launch_of's block
constexpr int kInFlight = 4;   // edges whose row loads are issued together

// ---------------------------------------------------------------------------
// out[r] = c_acc d_row[r] * sum_{e in row r} (SRC ? d_col[id_e] : 1) x[id_e]
//          (+ c_h0 h0[r] when H0)
// Forward: CSR rows, c_acc = 1 - alpha, c_h0 = alpha. Backward: CSC rows,
// x = gs, c_acc = 1.
// ---------------------------------------------------------------------------
template <typename T, int VEC, bool SRC, bool H0>
__global__ void __launch_bounds__(kThreads) gcn2_gather_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ x, const T* __restrict__ h0,
    const float* __restrict__ d_row, const float* __restrict__ d_col,
    const int32_t* __restrict__ row_order, T* __restrict__ out,
    int64_t num_rows, int64_t F, int64_t nchunks, float c_acc, float c_h0) {
  const UniformWave wv = uniform_wave();
  const int64_t npairs = num_rows * nchunks;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nchunks;
    if (row_order) r = row_order[r];
    // VEC divides F (host check): a lane is all inside the row or all past it
    const int64_t f0 = pair % nchunks * (kWave * VEC) + wv.lane * VEC;
    if (f0 >= F) continue;

    [[maybe_unused]] float res[VEC];
    float acc[VEC];
    if constexpr (H0) ld_vec<T, VEC>(h0 + r * F + f0, res);
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc[c] = 0.f;

    const T* x0 = x + f0;
    auto batch = [&](auto n_c, const auto& uu) {
      constexpr int NB = decltype(n_c)::value;
      float s[NB], v[NB][VEC];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        s[i] = SRC ? d_col[uu[i]] : 1.f;  // wave-uniform: a scalar load
        ld_vec<T, VEC>(x0 + static_cast<int64_t>(uu[i]) * F, v[i]);
      }
      // the dense SpMM's grouping: the batch is summed first, then added
#pragma unroll
      for (int c = 0; c < VEC; ++c) {
        if constexpr (NB == 4) {
          acc[c] += SRC ? s[0] * v[0][c] + s[1] * v[1][c] + s[2] * v[2][c] +
                              s[3] * v[3][c]
                        : v[0][c] + v[1][c] + v[2][c] + v[3][c];
        } else {
#pragma unroll
          for (int i = 0; i < NB; ++i) acc[c] += s[i] * v[i][c];
        }
      }
    };
    for_edges<kInFlight>(indices, indptr[r], indptr[r + 1], batch);

    const float scale = c_acc * d_row[r];  // wave-uniform
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      if constexpr (H0)
        acc[c] = fmaf(scale, acc[c], c_h0 * res[c]);
      else
        acc[c] *= scale;
    }
    st_vec<T, VEC>(out + r * F + f0, acc);
  }
}

// ---------------------------------------------------------------------------
// gs[v] = c_gs d[v] dP[v]; with ACC, dh0[v] += c_h0 dP[v] in fp32, in place.
// ---------------------------------------------------------------------------
template <typename T, int VEC, bool ACC>
__global__ void __launch_bounds__(kThreads) gcn2_prep_kernel(
    const T* __restrict__ dp, const float* __restrict__ d,
    T* __restrict__ gs, float* __restrict__ dh0, int64_t num_rows, int64_t F,
    int64_t nchunks, float c_gs, float c_h0) {
  const UniformWave wv = uniform_wave();
  const int64_t npairs = num_rows * nchunks;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    const int64_t r = pair / nchunks;
    const int64_t f0 = pair % nchunks * (kWave * VEC) + wv.lane * VEC;
    if (f0 >= F) continue;
    float g[VEC], run[VEC];
    ld_vec<T, VEC>(dp + r * F + f0, g);
    if constexpr (ACC) {
      ld_words<float, VEC>(dh0 + r * F + f0, run);
#pragma unroll
      for (int c = 0; c < VEC; ++c) run[c] = fmaf(c_h0, g[c], run[c]);
      st_words<float, VEC>(dh0 + r * F + f0, run);
    }
    const float scale = c_gs * d[r];  // wave-uniform
#pragma unroll
    for (int c = 0; c < VEC; ++c) g[c] *= scale;
    st_vec<T, VEC>(gs + r * F + f0, g);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

constexpr const char* kOp = "gcn2";

// fp32 [>= rows] on the device
const float* deg_ptr(const torch::Tensor& d, int64_t rows, const char* name) {
  TORCH_CHECK(d.is_cuda() && d.is_contiguous() && d.dim() == 1 &&
                  d.scalar_type() == torch::kFloat && d.numel() >= rows,
              kOp, ": ", name, " must be a contiguous fp32 vector with at "
              "least ", rows, " entries (an under-sized one would be an "
              "out-of-bounds read)");
  return d.data_ptr<float>();
}

// the gather over `indptr/indices` of rows of x [>= num_cols, F]; h0 null in
// the backward
torch::Tensor run_gather(const torch::Tensor& indptr,
                         const torch::Tensor& indices, const torch::Tensor& x,
                         const torch::Tensor* h0, const torch::Tensor& d_row,
                         const torch::Tensor& d_col,
                         const torch::Tensor& row_order, int64_t num_cols,
                         float c_acc, float c_h0) {
  check_graph(kOp, indptr, indices);
  const int64_t num_rows = indptr.numel() - 1;
  check_features(kOp, x, num_cols, 1, h0 ? "h" : "gs");
  const int64_t F = x.size(1);
  if (h0) {
    check_features(kOp, *h0, num_rows, 1, "h0");
    TORCH_CHECK(h0->size(1) == F && h0->scalar_type() == x.scalar_type(), kOp,
                ": h0 must agree with h in width and dtype");
  }
  const float* dr = deg_ptr(d_row, num_rows, "the row-side degree scale");
  const bool src = d_col.defined() && d_col.numel() > 0;
  const float* dc =
      src ? deg_ptr(d_col, num_cols, "the column-side degree scale") : nullptr;
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto out = torch::empty({num_rows, F}, x.options());
  if (num_rows == 0) return out;
  const int vec = lane_vec(kOp, F, num_rows, x.element_size(),
                           {x.data_ptr(), h0 ? h0->data_ptr() : nullptr,
                            out.data_ptr()},
                           {});
  const Launch l = launch_of(num_rows, F, vec);
  dispatch(x, vec, [&](auto tag, auto v) {
    using T = decltype(tag);
    constexpr int V = decltype(v)::value;
    auto run = [&](auto kern) {
      hipLaunchKernelGGL(kern, l.grid, l.block, 0, current_stream(),
                         indptr.data_ptr<int64_t>(),
                         indices.data_ptr<int32_t>(), cptr<T>(x),
                         h0 ? cptr<T>(*h0) : nullptr, dr, dc, rop,
                         mptr<T>(out), num_rows, F, l.nchunks, c_acc, c_h0);
    };
    if (!h0)
      run(HIP_KERNEL_NAME(gcn2_gather_kernel<T, V, false, false>));
    else if (src)
      run(HIP_KERNEL_NAME(gcn2_gather_kernel<T, V, true, true>));
    else
      run(HIP_KERNEL_NAME(gcn2_gather_kernel<T, V, false, true>));
  });
  check_launch();
  return out;
}

float check_alpha(double alpha) {
  TORCH_CHECK(alpha >= 0.0 && alpha <= 1.0, kOp, ": alpha=", alpha,
              " is outside [0, 1]");
  return static_cast<float>(alpha);
}

}  // namespace

torch::Tensor gcn2_fwd_hip(torch::Tensor indptr, torch::Tensor indices,
                           torch::Tensor h, torch::Tensor h0,
                           torch::Tensor d_dst, torch::Tensor d_src,
                           torch::Tensor row_order, int64_t num_cols,
                           double alpha) {
  check_alpha(alpha);
  return run_gather(indptr, indices, h, &h0, d_dst, d_src, row_order,
                    num_cols, static_cast<float>(1.0 - alpha),
                    static_cast<float>(alpha));
}

torch::Tensor gcn2_bwd_prep_hip(torch::Tensor dp, torch::Tensor d_dst,
                                double alpha, torch::Tensor dh0) {
  const float a = check_alpha(alpha);
  check_features(kOp, dp, 0, 1, "dP");
  const int64_t num_rows = dp.size(0), F = dp.size(1);
  const float* dd = deg_ptr(d_dst, num_rows, "d_dst");
  const bool acc = dh0.defined() && dh0.numel() > 0;
  if (acc)
    TORCH_CHECK(dh0.is_cuda() && dh0.is_contiguous() && dh0.dim() == 2 &&
                    dh0.scalar_type() == torch::kFloat &&
                    dh0.size(0) >= num_rows && dh0.size(1) == F,
                kOp, ": dh0 must be a contiguous fp32 [>= ", num_rows, ", ", F,
                "] buffer");
  auto gs = torch::empty_like(dp);
  if (num_rows == 0) return gs;
  const int vec = lane_vec(kOp, F, num_rows, dp.element_size(),
                           {dp.data_ptr(), gs.data_ptr()},
                           {acc ? dh0.data_ptr() : nullptr});
  const Launch l = launch_of(num_rows, F, vec);
  dispatch(dp, vec, [&](auto tag, auto v) {
    using T = decltype(tag);
    constexpr int V = decltype(v)::value;
    auto run = [&](auto kern) {
      hipLaunchKernelGGL(kern, l.grid, l.block, 0, current_stream(),
                         cptr<T>(dp), dd, mptr<T>(gs),
                         acc ? dh0.data_ptr<float>() : nullptr, num_rows, F,
                         l.nchunks, static_cast<float>(1.0 - alpha), a);
    };
    if (acc)
      run(HIP_KERNEL_NAME(gcn2_prep_kernel<T, V, true>));
    else
      run(HIP_KERNEL_NAME(gcn2_prep_kernel<T, V, false>));
  });
  check_launch();
  return gs;
}

torch::Tensor gcn2_bwd_hip(torch::Tensor indptr, torch::Tensor indices,
                           torch::Tensor gs, torch::Tensor d_src,
                           torch::Tensor row_order, int64_t num_cols) {
  // indptr/indices are the CSC: rows = source nodes, columns = destinations
  return run_gather(indptr, indices, gs, nullptr, d_src, torch::Tensor(),
                    row_order, num_cols, 1.f, 0.f);
}
