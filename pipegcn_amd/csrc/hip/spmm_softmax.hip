// Softmax aggregation (DeeperGCN / GENConv: Li et al. 2020; PyG's
// SoftmaxAggregation(learn=True)) for gfx950, and its backward
// (docs/DESIGN.md, "Softmax aggregation"). Per column c, over the d edges of
// row r (parallel edges counted):
//
//   out[r, c] = sum_u softmax_u(beta * x[u, c]) * x[u, c]
//
// Every column has a softmax of its own: the score is the gathered value
// itself, so one gather of each neighbour row serves score and value. beta is
// one learned fp32 scalar, read by the kernels through a device pointer (no
// host read). Rows without edges give 0. All arithmetic is fp32; NaN and
// infinite inputs are unspecified.
//
// The exponentials are taken in base 2: the kernels hold bl = beta * log2(e)
// and form weights as exp2(bl * x + c), where c = -(bl * K) and K is the
// running extremum of x over the row: its maximum where bl >= 0, its minimum
// where bl < 0 (the sign of beta is wave-uniform, so the choice is a scalar
// branch). The exponent is never above 0 but for its last rounding.
//
//  - spmm_softmax_fwd : over the CSR, one wave per (row, chunk of 64 * VEC
//      columns). Per lane and column: K, c, Z = sum exp2(bl x_u + c) and
//      N = sum exp2(bl x_u + c) x_u; out = N / Z. Edges come four at a time
//      (for_edges<4>), all four row loads issued before the first use; a batch
//      takes its extremum first and rescales Z and N once by
//      exp2(c_new - c_old), which is exactly 1 while the extremum stands: 5
//      exponentials per 4 edges. WITH_STATE also writes
//        lse fp32 [num_rows, F] = log2(Z) - c, IN BASE 2: the weight of edge
//            u -> r is exp2(bl * x_u - lse_r); 0 on rows without edges;
//        out32 fp32 [num_rows, F], for bf16 x only: out before its rounding
//            (for fp32 x, out is that tensor).
//  - spmm_softmax_bwd : over the CSC WITH repeated entries (row = source j,
//      columns = destinations i), so multiplicity counts. The lane holds x_j;
//      per entry it gathers g_i, lse_i and out_i (three rows) and forms
//        w = exp2(bl x_j - lse_i)   gw = g_i w   t = x_j - out_i
//        A += gw                    B += gw t
//      then dx_j = A + beta B, and x_j B is the lane's share of dbeta.
//      Those shares are summed in a fixed order: over the lane's columns and
//      (row, chunk) pairs, over the wave by a butterfly, over the block's
//      waves through LDS by thread 0, one partial per block.
//  - dbeta_sum        : one block adds the [grid] partials in a fixed order.
//
// One fixed lane owns a column and walks the row in stored order, so out and
// grad_x are bitwise reproducible and independent of row_order; dbeta is
// reproducible for a given graph, row_order and launch geometry. No atomics.
//
// Compiler resource report: profiles/README.md, "Softmax aggregation".
// No instance uses scratch.

#include "../common.h"
#include "attn_util.h"
#include "gather_lanes.h"
#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>
#include <vector>

namespace {

using namespace attn_util;
using namespace gather_lanes;

constexpr float kLog2e = 1.44269504088896340736f;
constexpr int kThreads = 256;  // launch_of's block
constexpr int kWavesPerBlock = kThreads / kWave;

// Every fused multiply-add below is written as fmaf and the compiler forms
// none of its own, so the WITH_STATE instances and the plain ones agree bit
// for bit (see spmm_pna.hip).
#pragma clang fp contract(off)

// v_exp_f32: the exponents here are <= 0 (but for a rounding), a result
// below the normal range may flush to 0
__device__ __forceinline__ float exp2_fast(float v) {
  return __builtin_amdgcn_exp2f(v);
}

template <bool POS>
__device__ __forceinline__ float extremum(float a, float b) {
  return POS ? fmaxf(a, b) : fminf(a, b);
}

// ---------------------------------------------------------------------------
// forward over the CSR (row = destination r, columns = sources u)
// ---------------------------------------------------------------------------
template <typename T, int VEC, bool WITH_STATE>
__global__ void __launch_bounds__(kThreads) spmm_softmax_fwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ x, const float* __restrict__ beta,
    const int32_t* __restrict__ row_order, T* __restrict__ out,
    float* __restrict__ lse, float* __restrict__ out32, int64_t num_rows,
    int64_t F, int64_t nchunks) {
  const UniformWave wv = uniform_wave();
  const int64_t npairs = num_rows * nchunks;
  const float bl = *beta * kLog2e;  // a scalar load: wave-uniform

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nchunks;
    if (row_order) r = row_order[r];
    // VEC divides F (host check): a lane is all inside the row or all past it
    const int64_t f0 = pair % nchunks * (kWave * VEC) + wv.lane * VEC;
    if (f0 >= F) continue;

    float o[VEC], l[VEC];
    const int64_t e_begin = indptr[r];
    const int64_t e_end = indptr[r + 1];
    if (e_begin == e_end) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k] = l[k] = 0.f;
    } else {
      // the first edge starts the state, so no infinity enters (beta may be
      // 0); it is weighted by the same formula as every later edge
      float K[VEC], c[VEC], Z[VEC], N[VEC];
      ld_vec<T, VEC>(x + static_cast<int64_t>(indices[e_begin]) * F + f0, K);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        c[k] = -(bl * K[k]);
        Z[k] = exp2_fast(fmaf(bl, K[k], c[k]));
        N[k] = Z[k] * K[k];
      }

      auto walk = [&](auto pos_c) {
        constexpr bool POS = decltype(pos_c)::value;
        auto batch = [&](auto n_c, const auto& uu) {
          constexpr int NB = decltype(n_c)::value;
          float v[NB][VEC];
#pragma unroll
          for (int i = 0; i < NB; ++i)
            ld_vec<T, VEC>(x + static_cast<int64_t>(uu[i]) * F + f0, v[i]);
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            float kn = K[k];
#pragma unroll
            for (int i = 0; i < NB; ++i) kn = extremum<POS>(kn, v[i][k]);
            const float cn = -(bl * kn);
            // exactly 1 while the extremum stands
            const float rs = exp2_fast(cn - c[k]);
            float z = Z[k] * rs;
            float n = N[k] * rs;
#pragma unroll
            for (int i = 0; i < NB; ++i) {
              const float e = exp2_fast(fmaf(bl, v[i][k], cn));
              z += e;
              n = fmaf(e, v[i][k], n);
            }
            K[k] = kn;
            c[k] = cn;
            Z[k] = z;
            N[k] = n;
          }
        };
        for_edges<4>(indices, e_begin + 1, e_end, batch);
      };
      if (bl >= 0.f)
        walk(std::true_type{});
      else
        walk(std::false_type{});

#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        o[k] = N[k] / Z[k];
        l[k] = log2f(Z[k]) - c[k];
      }
    }

    st_vec<T, VEC>(out + r * F + f0, o);
    if constexpr (WITH_STATE) {
      st_words<float, VEC>(lse + r * F + f0, l);
      if constexpr (!std::is_same_v<T, float>)
        st_words<float, VEC>(out32 + r * F + f0, o);
    }
  }
}

// ---------------------------------------------------------------------------
// backward over the CSC with repeated entries (row = source j, columns =
// destinations i): three row gathers per entry, g[i], lse[i] and out32[i]
// ---------------------------------------------------------------------------
template <typename T, int VEC>
__global__ void __launch_bounds__(kThreads) spmm_softmax_bwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ g, const float* __restrict__ lse,
    const float* __restrict__ out32, const T* __restrict__ x,
    const float* __restrict__ beta, const int32_t* __restrict__ row_order,
    T* __restrict__ grad_x, float* __restrict__ partial, int64_t num_rows,
    int64_t F, int64_t nchunks) {
  __shared__ float wave_part[kWavesPerBlock];
  const UniformWave wv = uniform_wave();
  const int64_t npairs = num_rows * nchunks;
  const float bv = *beta;
  const float bl = bv * kLog2e;
  // the widest lane gathers 80 bytes per entry: two entries in flight hold
  // what four hold at the narrower widths
  constexpr int U = VEC == 8 ? 2 : 4;

  float db = 0.f;  // this lane's share of dbeta, over all its pairs
  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nchunks;
    if (row_order) r = row_order[r];
    const int64_t f0 = pair % nchunks * (kWave * VEC) + wv.lane * VEC;
    if (f0 >= F) continue;

    float xv[VEC], A[VEC], B[VEC];
    ld_vec<T, VEC>(x + r * F + f0, xv);
#pragma unroll
    for (int k = 0; k < VEC; ++k) A[k] = B[k] = 0.f;

    auto batch = [&](auto n_c, const auto& ii) {
      constexpr int NB = decltype(n_c)::value;
      float gg[NB][VEC], ll[NB][VEC], oo[NB][VEC];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int64_t at = static_cast<int64_t>(ii[i]) * F + f0;
        ld_vec<T, VEC>(g + at, gg[i]);
        ld_words<float, VEC>(lse + at, ll[i]);
        ld_words<float, VEC>(out32 + at, oo[i]);
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          // <= 1 but for a rounding: no overflow is possible
          const float w = exp2_fast(fmaf(bl, xv[k], -ll[i][k]));
          const float gw = gg[i][k] * w;
          A[k] += gw;
          B[k] = fmaf(gw, xv[k] - oo[i][k], B[k]);
        }
      }
    };
    for_edges<U>(indices, indptr[r], indptr[r + 1], batch);

    float dx[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      dx[k] = fmaf(bv, B[k], A[k]);
      db = fmaf(xv[k], B[k], db);
    }
    st_vec<T, VEC>(grad_x + r * F + f0, dx);
  }

  // lanes -> wave -> block, each step in a fixed order
  db = wave_sum(db);
  if (wv.lane == 0) wave_part[threadIdx.x / kWave] = db;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = wave_part[0];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) s += wave_part[w];
    partial[blockIdx.x] = s;
  }
}

// dbeta = the sum of the per-block partials: thread t adds partials t,
// t + 256, ... in that order, then a tree over LDS
__global__ void __launch_bounds__(kThreads) dbeta_sum_kernel(
    const float* __restrict__ partial, int64_t n, float* __restrict__ dbeta) {
  __shared__ float s[kThreads];
  float a = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) a += partial[i];
  s[threadIdx.x] = a;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) dbeta[0] = s[0];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

constexpr const char* kOp = "spmm_softmax";

const float* beta_ptr(const torch::Tensor& beta) {
  TORCH_CHECK(beta.is_cuda() && beta.numel() == 1 &&
                  beta.scalar_type() == torch::kFloat,
              kOp, ": beta must be one fp32 value on the device");
  return beta.data_ptr<float>();
}

// a contiguous fp32 [>= rows, F] table
void check_state(const torch::Tensor& t, int64_t rows, int64_t F,
                 const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 2 && t.is_contiguous() &&
                  t.scalar_type() == torch::kFloat,
              kOp, ": ", name, " must be a contiguous fp32 [rows, ", F,
              "] tensor");
  TORCH_CHECK(t.size(0) >= rows && t.size(1) == F, kOp, ": ", name, " is [",
              t.size(0), ", ", t.size(1), "] but the graph references ", rows,
              " rows of width ", F);
}

}  // namespace

std::vector<torch::Tensor> spmm_softmax_fwd_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor x,
    torch::Tensor beta, torch::Tensor row_order, int64_t num_cols,
    bool with_state) {
  check_graph(kOp, indptr, indices);
  const int64_t num_rows = indptr.numel() - 1;
  check_features(kOp, x, num_cols, 1, "x");
  const float* bp = beta_ptr(beta);
  const int64_t F = x.size(1);
  const bool bf16 = x.scalar_type() == torch::kBFloat16;
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto out = torch::empty({num_rows, F}, x.options());
  torch::Tensor lse, out32;
  if (with_state) {
    lse = torch::empty({num_rows, F}, x.options().dtype(torch::kFloat));
    if (bf16) out32 = torch::empty_like(lse);
  }
  if (num_rows > 0 && F > 0) {
    const int vec = lane_vec(
        kOp, F, num_rows, x.element_size(), {x.data_ptr(), out.data_ptr()},
        {with_state ? lse.data_ptr() : nullptr,
         out32.defined() ? out32.data_ptr() : nullptr});
    const Launch l = launch_of(num_rows, F, vec);
    dispatch(x, vec, [&](auto tag, auto v) {
      using T = decltype(tag);
      constexpr int V = decltype(v)::value;
      auto run = [&](auto kern, float* lp, float* op) {
        hipLaunchKernelGGL(kern, l.grid, l.block, 0, current_stream(),
                           indptr.data_ptr<int64_t>(),
                           indices.data_ptr<int32_t>(), cptr<T>(x), bp, rop,
                           mptr<T>(out), lp, op, num_rows, F, l.nchunks);
      };
      if (with_state)
        run(HIP_KERNEL_NAME(spmm_softmax_fwd_kernel<T, V, true>),
            lse.data_ptr<float>(),
            out32.defined() ? out32.data_ptr<float>() : nullptr);
      else
        run(HIP_KERNEL_NAME(spmm_softmax_fwd_kernel<T, V, false>), nullptr,
            nullptr);
    });
    check_launch();
  }
  if (!with_state) return {out};
  if (bf16) return {out, lse, out32};
  return {out, lse};
}

std::vector<torch::Tensor> spmm_softmax_bwd_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor g,
    torch::Tensor lse, torch::Tensor out32, torch::Tensor x,
    torch::Tensor beta, torch::Tensor row_order, int64_t num_cols) {
  // indptr/indices are the CSC: rows = sources, columns = destinations
  check_graph(kOp, indptr, indices);
  const int64_t num_rows = indptr.numel() - 1;
  check_features(kOp, g, num_cols, 1, "g");
  const int64_t F = g.size(1);
  check_state(lse, num_cols, F, "lse");
  check_state(out32, num_cols, F, "out32");
  check_features(kOp, x, num_rows, 1, "x");
  TORCH_CHECK(x.size(1) == F && x.scalar_type() == g.scalar_type(), kOp,
              ": x must be [rows, ", F, "] of g's dtype");
  const float* bp = beta_ptr(beta);
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto grad_x = torch::empty({num_rows, F}, x.options());
  if (num_rows == 0 || F == 0)
    return {grad_x, torch::zeros({1}, lse.options())};
  auto dbeta = torch::empty({1}, lse.options());
  const int vec = lane_vec(kOp, F, num_rows, g.element_size(),
                           {g.data_ptr(), x.data_ptr(), grad_x.data_ptr()},
                           {lse.data_ptr(), out32.data_ptr()});
  const Launch l = launch_of(num_rows, F, vec);
  // every block writes its partial, whether or not it had a pair
  auto partial = torch::empty({static_cast<int64_t>(l.grid.x)}, lse.options());
  dispatch(g, vec, [&](auto tag, auto v) {
    using T = decltype(tag);
    constexpr int V = decltype(v)::value;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spmm_softmax_bwd_kernel<T, V>), l.grid,
                       l.block, 0, current_stream(),
                       indptr.data_ptr<int64_t>(),
                       indices.data_ptr<int32_t>(), cptr<T>(g),
                       lse.data_ptr<float>(), out32.data_ptr<float>(),
                       cptr<T>(x), bp, rop, mptr<T>(grad_x),
                       partial.data_ptr<float>(), num_rows, F, l.nchunks);
  });
  check_launch();
  hipLaunchKernelGGL(dbeta_sum_kernel, dim3(1), dim3(kThreads), 0,
                     current_stream(), partial.data_ptr<float>(),
                     static_cast<int64_t>(l.grid.x), dbeta.data_ptr<float>());
  check_launch();
  return {grad_x, dbeta};
}
