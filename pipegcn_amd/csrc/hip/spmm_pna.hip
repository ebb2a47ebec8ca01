// Multi-aggregation (PNA: Corso et al. 2020) for gfx950: mean, maximum,
// minimum and standard deviation of a neighbourhood from ONE gather of each
// neighbour row, and its backward (docs/DESIGN.md, "Multi-aggregation
// (PNA)").
//
//   out[r] = [ x[r] | mean | max | min | std ]        [num_rows, 5F], x's dtype
//
// over the d edges of row r (parallel edges counted), per column:
//   K    = x at the row's first edge: the initial max and min, and the SHIFT
//   S1   = sum (x_u - K)          S2 = sum (x_u - K)^2
//   m    = S1 / d                 mean = K + m
//   var  = S2 / d - m^2           std  = sqrt(max(var, 0) + 1e-5)
//   max, min with their source ids by spmm_max's contract: strict > / strict <
//   in stored order, so the first edge that attains the extremum keeps it.
// Rows without edges give zeros in the four statistic blocks. All arithmetic
// is fp32; NaN inputs are unspecified.
//
// The shift keeps S2 / d - m^2 from cancelling when |mean| >> std: the sums
// then hold deviations from a row member instead of raw values.
//
// State (WITH_STATE, for the backward):
//   arg  int32 [num_rows, 2F] = [arg_max | arg_min], -1 on rows without edges
//   stat fp32  [num_rows, 2F] = [mean | rstd], rstd = 1 / (d * std), and 0
//        where var <= 0 (relu's gradient at 0) or the row has no edges
//
//  - spmm_pna_fwd : over the CSR, one wave per (row, chunk of 64 * VEC
//                   columns) as spmm_max_fwd_kernel; 7 * VEC accumulators per
//                   lane plus 4 * VEC loaded values.
//  - pna_bwd_prep : elementwise, PQ = [P | Q] fp32 [num_in, 2F] with
//                   Q = g_std * rstd, P = g_mean / d - Q * mean. The dense
//                   SpMM over the CSC then gives Tt = [sum P | sum Q] per
//                   source: the mean's and the std's gradient is
//                   sum P + x_u * sum Q, with the multiplicity of parallel
//                   edges.
//  - spmm_pna_bwd : over the CSC WITHOUT repeated entries, as
//                   spmm_max_bwd_kernel: adds g_max / g_min where arg_max /
//                   arg_min name this source, then Tt's term and g_self.
//
// One fixed lane owns a column and walks the row in stored order, so results
// are bitwise reproducible and independent of row_order.
//
// Compiler resource report: profiles/README.md, "Multi-aggregation (PNA)".
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

constexpr float kEps = 1e-5f;  // PyG's PNAConv

// Every fused multiply-add below is written as fmaf and the compiler forms
// none of its own: left to itself it fuses s2 += dv * dv in some copies of
// the edge loop and not in others, and differently in the WITH_STATE
// instances, so the two forwards would not agree bit for bit.
#pragma clang fp contract(off)

// ---------------------------------------------------------------------------
// forward over the CSR (row = destination r, columns = sources u)
// ---------------------------------------------------------------------------
template <typename T, int VEC, bool WITH_STATE>
__global__ void __launch_bounds__(256) spmm_pna_fwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ x, const int32_t* __restrict__ row_order,
    T* __restrict__ out, int32_t* __restrict__ arg, float* __restrict__ stat,
    int64_t num_rows, int64_t F, int64_t nchunks) {
  const UniformWave wv = uniform_wave();
  const int64_t npairs = num_rows * nchunks;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nchunks;
    if (row_order) r = row_order[r];
    // VEC divides F (host check): a lane is all inside the row or all past
    // it, and the block offsets k * F keep its alignment
    const int64_t f0 = pair % nchunks * (kWave * VEC) + wv.lane * VEC;
    if (f0 >= F) continue;
    T* const orow = out + r * 5 * F + f0;

    // destination r is row r of x
    float self[VEC];
    ld_vec<T, VEC>(x + r * F + f0, self);
    st_vec<T, VEC>(orow, self);

    float mean[VEC], best[VEC], lo[VEC], sd[VEC], rstd[VEC];
    int32_t bid[VEC], lid[VEC];
    const int64_t e_begin = indptr[r];
    const int64_t e_end = indptr[r + 1];
    if (e_begin == e_end) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        mean[k] = best[k] = lo[k] = sd[k] = rstd[k] = 0.f;
        bid[k] = lid[k] = -1;
      }
    } else {
      const int32_t first = indices[e_begin];
      float K[VEC], s1[VEC], s2[VEC];
      ld_vec<T, VEC>(x + static_cast<int64_t>(first) * F + f0, K);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        best[k] = lo[k] = K[k];
        bid[k] = lid[k] = first;
        s1[k] = s2[k] = 0.f;  // the first edge's deviation from K is 0
      }

      auto batch = [&](auto n_c, const auto& uu) {
        constexpr int N = decltype(n_c)::value;
        float v[N][VEC];
#pragma unroll
        for (int i = 0; i < N; ++i)
          ld_vec<T, VEC>(x + static_cast<int64_t>(uu[i]) * F + f0, v[i]);
        // in stored order, strict comparisons: the first edge that attains
        // an extremum keeps it
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            const float dv = v[i][k] - K[k];
            s1[k] += dv;
            s2[k] = fmaf(dv, dv, s2[k]);
            const bool gt = v[i][k] > best[k];
            const bool lt = v[i][k] < lo[k];
            best[k] = gt ? v[i][k] : best[k];
            lo[k] = lt ? v[i][k] : lo[k];
            if constexpr (WITH_STATE) {
              bid[k] = gt ? uu[i] : bid[k];
              lid[k] = lt ? uu[i] : lid[k];
            }
          }
        }
      };
      for_edges<4>(indices, e_begin + 1, e_end, batch);

      const float d = static_cast<float>(e_end - e_begin);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float m = s1[k] / d;
        const float var = fmaf(-m, m, s2[k] / d);
        mean[k] = K[k] + m;
        sd[k] = sqrtf(fmaxf(var, 0.f) + kEps);
        rstd[k] = var > 0.f ? 1.f / (d * sd[k]) : 0.f;
      }
    }

    st_vec<T, VEC>(orow + F, mean);
    st_vec<T, VEC>(orow + 2 * F, best);
    st_vec<T, VEC>(orow + 3 * F, lo);
    st_vec<T, VEC>(orow + 4 * F, sd);
    if constexpr (WITH_STATE) {
      const int64_t at = r * 2 * F + f0;
      st_ids<VEC>(arg + at, bid);
      st_ids<VEC>(arg + at + F, lid);
      st_words<float, VEC>(stat + at, mean);
      st_words<float, VEC>(stat + at + F, rstd);
    }
  }
}

// ---------------------------------------------------------------------------
// backward, step 1: PQ = [P | Q] per destination row, elementwise
// ---------------------------------------------------------------------------

// (row, chunk) pairs a wave has in flight: all loads of a round are issued
// before the first use, as the other elementwise kernels do
constexpr int kPrepInFlight = 2;

template <typename T, int VEC>
__global__ void __launch_bounds__(256) pna_bwd_prep_kernel(
    const int64_t* __restrict__ indptr, const T* __restrict__ g,
    const float* __restrict__ stat, float* __restrict__ pq, int64_t num_rows,
    int64_t F, int64_t nchunks) {
  const UniformWave wv = uniform_wave();
  const int64_t npairs = num_rows * nchunks;

  for (int64_t p0 = wv.wave_global; p0 < npairs;
       p0 += kPrepInFlight * wv.nwaves) {
    float gm[kPrepInFlight][VEC], gs[kPrepInFlight][VEC];
    float mean[kPrepInFlight][VEC], rstd[kPrepInFlight][VEC];
    float inv_d[kPrepInFlight];
    int64_t at[kPrepInFlight];
    bool on[kPrepInFlight];
    // no load sits behind a branch: a pair past the end or a lane past the
    // row reads the last valid place instead and stores nothing
#pragma unroll
    for (int j = 0; j < kPrepInFlight; ++j) {
      const int64_t pair = p0 + j * wv.nwaves;
      const int64_t pc = min(pair, npairs - 1);
      const int64_t row = pc / nchunks;
      const int64_t f0 = pc % nchunks * (kWave * VEC) + wv.lane * VEC;
      on[j] = pair < npairs && f0 < F;
      const int64_t fc = min(f0, F - VEC);
      const T* grow = g + row * 5 * F + fc;
      at[j] = row * 2 * F + fc;
      ld_vec<T, VEC>(grow + F, gm[j]);
      ld_vec<T, VEC>(grow + 4 * F, gs[j]);
      ld_words<float, VEC>(stat + at[j], mean[j]);
      ld_words<float, VEC>(stat + at[j] + F, rstd[j]);
      const int64_t d = indptr[row + 1] - indptr[row];
      inv_d[j] = d > 0 ? 1.f / static_cast<float>(d) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < kPrepInFlight; ++j) {
      if (!on[j]) continue;
      float P[VEC], Q[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        Q[k] = gs[j][k] * rstd[j][k];
        P[k] = fmaf(-Q[k], mean[j][k], gm[j][k] * inv_d[j]);
      }
      st_words<float, VEC>(pq + at[j], P);
      st_words<float, VEC>(pq + at[j] + F, Q);
    }
  }
}

// ---------------------------------------------------------------------------
// backward, step 3, over a CSC without repeated entries (row = source u,
// columns = destinations r): four row gathers per entry, g_max[r], g_min[r],
// arg_max[r] and arg_min[r]
// ---------------------------------------------------------------------------
template <typename T, int VEC>
__global__ void __launch_bounds__(256) spmm_pna_bwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ g, const int32_t* __restrict__ arg,
    const float* __restrict__ tt, const T* __restrict__ x,
    const int32_t* __restrict__ row_order, T* __restrict__ grad_x,
    int64_t num_rows, int64_t num_in, int64_t F, int64_t nchunks) {
  const UniformWave wv = uniform_wave();
  const int64_t npairs = num_rows * nchunks;
  // the widest lane gathers 96 bytes per entry: two entries in flight hold
  // what four hold at the narrower widths
  constexpr int U = VEC == 8 ? 2 : 4;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nchunks;
    if (row_order) r = row_order[r];
    const int64_t f0 = pair % nchunks * (kWave * VEC) + wv.lane * VEC;
    if (f0 >= F) continue;
    const int32_t u = static_cast<int32_t>(r);

    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;

    auto batch = [&](auto n_c, const auto& rr) {
      constexpr int N = decltype(n_c)::value;
      float gmax[N][VEC], gmin[N][VEC];
      int32_t amax[N][VEC], amin[N][VEC];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const T* grow = g + static_cast<int64_t>(rr[i]) * 5 * F + f0;
        const int32_t* arow = arg + static_cast<int64_t>(rr[i]) * 2 * F + f0;
        ld_vec<T, VEC>(grow + 2 * F, gmax[i]);
        ld_vec<T, VEC>(grow + 3 * F, gmin[i]);
        ld_ids<VEC>(arow, amax[i]);
        ld_ids<VEC>(arow + F, amin[i]);
      }
#pragma unroll
      for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          acc[k] += amax[i][k] == u ? gmax[i][k] : 0.f;
          acc[k] += amin[i][k] == u ? gmin[i][k] : 0.f;
        }
      }
    };
    for_edges<U>(indices, indptr[r], indptr[r + 1], batch);

    // the moments' part: sum P + x_u * sum Q
    float sp[VEC], sq[VEC], xv[VEC];
    ld_words<float, VEC>(tt + r * 2 * F + f0, sp);
    ld_words<float, VEC>(tt + r * 2 * F + F + f0, sq);
    ld_vec<T, VEC>(x + r * F + f0, xv);
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] += fmaf(xv[k], sq[k], sp[k]);
    if (r < num_in) {  // a destination is a source of its own self block
      float gself[VEC];
      ld_vec<T, VEC>(g + r * 5 * F + f0, gself);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] += gself[k];
    }

    st_vec<T, VEC>(grad_x + r * F + f0, acc);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

constexpr const char* kOp = "spmm_pna";

// a contiguous [>= rows, width] table of 4-byte elements
void check_table(const torch::Tensor& t, torch::ScalarType dtype,
                 int64_t rows, int64_t width, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 2 && t.is_contiguous() &&
                  t.scalar_type() == dtype,
              kOp, ": ", name, " must be a contiguous ",
              dtype == torch::kInt ? "int32" : "fp32", " [rows, ", width,
              "] tensor");
  TORCH_CHECK(t.size(0) >= rows && t.size(1) == width, kOp, ": ", name,
              " is [", t.size(0), ", ", t.size(1),
              "] but the graph references ", rows, " rows of width ", width);
}

// g [>= rows, 5F] -> F
int64_t check_grad(const torch::Tensor& g, int64_t rows) {
  check_features(kOp, g, rows, 1, "g");
  TORCH_CHECK(g.size(1) > 0 && g.size(1) % 5 == 0, kOp, ": g has ", g.size(1),
              " columns, expected 5 * F");
  return g.size(1) / 5;
}

}  // namespace

std::vector<torch::Tensor> spmm_pna_fwd_hip(torch::Tensor indptr,
                                            torch::Tensor indices,
                                            torch::Tensor x,
                                            torch::Tensor row_order,
                                            int64_t num_cols,
                                            bool with_state) {
  check_graph(kOp, indptr, indices);
  const int64_t num_rows = indptr.numel() - 1;
  // the self block reads x[r] for every destination r as well
  check_features(kOp, x, std::max(num_cols, num_rows), 1, "x");
  const int64_t F = x.size(1);
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto out = torch::empty({num_rows, 5 * F}, x.options());
  torch::Tensor arg, stat;
  if (with_state) {
    arg = torch::empty({num_rows, 2 * F}, x.options().dtype(torch::kInt));
    stat = torch::empty({num_rows, 2 * F}, x.options().dtype(torch::kFloat));
  }
  if (num_rows > 0 && F > 0) {
    const int vec = lane_vec(
        kOp, F, num_rows, x.element_size(), {x.data_ptr(), out.data_ptr()},
        {with_state ? arg.data_ptr() : nullptr,
         with_state ? stat.data_ptr() : nullptr});
    const Launch l = launch_of(num_rows, F, vec);
    dispatch(x, vec, [&](auto tag, auto v) {
      using T = decltype(tag);
      constexpr int V = decltype(v)::value;
      auto run = [&](auto kern, int32_t* ap, float* sp) {
        hipLaunchKernelGGL(kern, l.grid, l.block, 0, current_stream(),
                           indptr.data_ptr<int64_t>(),
                           indices.data_ptr<int32_t>(), cptr<T>(x), rop,
                           mptr<T>(out), ap, sp, num_rows, F, l.nchunks);
      };
      if (with_state)
        run(HIP_KERNEL_NAME(spmm_pna_fwd_kernel<T, V, true>),
            arg.data_ptr<int32_t>(), stat.data_ptr<float>());
      else
        run(HIP_KERNEL_NAME(spmm_pna_fwd_kernel<T, V, false>), nullptr,
            nullptr);
    });
    check_launch();
  }
  if (with_state) return {out, arg, stat};
  return {out};
}

torch::Tensor pna_bwd_prep_hip(torch::Tensor indptr, torch::Tensor g,
                               torch::Tensor stat) {
  TORCH_CHECK(indptr.is_cuda() && indptr.is_contiguous() &&
                  indptr.scalar_type() == torch::kLong && indptr.numel() >= 1,
              kOp, ": indptr must be a contiguous int64 device tensor");
  const int64_t num_rows = indptr.numel() - 1;
  const int64_t F = check_grad(g, num_rows);
  check_table(stat, torch::kFloat, num_rows, 2 * F, "stat");
  auto pq = torch::empty({num_rows, 2 * F}, stat.options());
  if (num_rows == 0) return pq;
  const int vec = lane_vec(kOp, F, num_rows, g.element_size(), {g.data_ptr()},
                           {stat.data_ptr(), pq.data_ptr()});
  const Launch l = launch_of(
      (num_rows + kPrepInFlight - 1) / kPrepInFlight, F, vec);
  dispatch(g, vec, [&](auto tag, auto v) {
    using T = decltype(tag);
    constexpr int V = decltype(v)::value;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pna_bwd_prep_kernel<T, V>), l.grid,
                       l.block, 0, current_stream(),
                       indptr.data_ptr<int64_t>(), cptr<T>(g),
                       stat.data_ptr<float>(), pq.data_ptr<float>(), num_rows,
                       F, l.nchunks);
  });
  check_launch();
  return pq;
}

torch::Tensor spmm_pna_bwd_hip(torch::Tensor indptr, torch::Tensor indices,
                               torch::Tensor g, torch::Tensor arg,
                               torch::Tensor tt, torch::Tensor x,
                               torch::Tensor row_order, int64_t num_cols) {
  // indptr/indices are the simple CSC: rows = sources, columns = destinations
  check_graph(kOp, indptr, indices);
  const int64_t num_rows = indptr.numel() - 1;
  const int64_t F = check_grad(g, num_cols);
  check_table(arg, torch::kInt, num_cols, 2 * F, "arg");
  check_table(tt, torch::kFloat, num_rows, 2 * F, "tt");
  check_features(kOp, x, num_rows, 1, "x");
  TORCH_CHECK(x.size(1) == F && x.scalar_type() == g.scalar_type(), kOp,
              ": x must be [rows, ", F, "] of g's dtype");
  // the self block: sources below num_cols are the destinations
  TORCH_CHECK(num_cols <= num_rows, kOp, ": ", num_cols,
              " destinations but ", num_rows, " sources");
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto grad_x = torch::empty({num_rows, F}, x.options());
  if (num_rows == 0) return grad_x;
  const int vec = lane_vec(kOp, F, num_rows, g.element_size(),
                           {g.data_ptr(), x.data_ptr(), grad_x.data_ptr()},
                           {arg.data_ptr(), tt.data_ptr()});
  const Launch l = launch_of(num_rows, F, vec);
  dispatch(g, vec, [&](auto tag, auto v) {
    using T = decltype(tag);
    constexpr int V = decltype(v)::value;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spmm_pna_bwd_kernel<T, V>), l.grid,
                       l.block, 0, current_stream(),
                       indptr.data_ptr<int64_t>(),
                       indices.data_ptr<int32_t>(), cptr<T>(g),
                       arg.data_ptr<int32_t>(), tt.data_ptr<float>(),
                       cptr<T>(x), rop, mptr<T>(grad_x), num_rows, num_cols,
                       F, l.nchunks);
  });
  check_launch();
  return grad_x;
}
