// Beta gate of the graph transformer layer (UniMP's TransformerConv with
// beta=True), gfx950:
//
//   beta_v = sigmoid(<a, r_v> + <b, m_v>)          one scalar per node
//   out_v  = beta_v * r_v + (1 - beta_v) * m_v
//
// r is the skip projection, m the attention aggregate. a = w_r + w_d and
// b = w_m - w_d fold the layer's [1, 3F] weight over [r | m | r - m]; the
// fold and its gradient are torch's (ops.gated_residual), the kernels see the
// two fp32 [F] vectors only. Storage is fp32 or bf16, arithmetic fp32.
//
// Work split: one 64-lane wave per row, grid-stride over rows. A lane owns
// FIXED columns: chunk c gives it the VEC columns from c * 64 * VEC +
// lane * VEC on, moved as one access. A wave holds a PANEL of NCH chunks
// (NCH * VEC <= 16 columns per lane, so up to 1024 columns) of r and m in
// registers: it loads them once, reduces the logit with a shuffle butterfly
// and writes the mix from the held registers, so up to F = 1024 every input
// element is read exactly once. a and b for the panel are loaded once per
// wave, outside the row loop.
//
// Wider rows run one pass over the rows per panel: the columns outside the
// held panel are streamed for the row's dot product only, in ascending chunk
// order in every pass, so each pass forms bit for bit the same scalar. Such a
// row is read once per panel (twice up to F = 2048).
//
// Backward, with d = r - m, t_v = <g_v, d_v>, s_v = t_v beta_v (1 - beta_v):
//
//   d_r = beta g + s a            d_m = (1 - beta) g + s b
//   da  = sum_v s_v r_v           db  = sum_v s_v m_v
//
// da and db need no cross-lane work: a lane's columns are the same for every
// row its wave visits, so it accumulates s_v r_v[k] and s_v m_v[k] in
// registers across its rows. The waves of a block then combine through LDS in
// wave order, the block writes one [2F] fp32 partial, and gate_sum_kernel
// adds the partials in block order. There are no atomics: for a given (N, F)
// the launch geometry and every summation order are fixed, so da and db are
// bitwise reproducible. That needs a fixed, small grid: kGateMaxBlocks. Its
// value (1024 blocks of 256 threads) is a starting point and has NOT been
// tuned; see profiles/README.md, "Beta gate".

#include "../common.h"
#include "attn_util.h"
#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

namespace {

using attn_util::ld_vec;
using attn_util::st_vec;
using attn_util::wave_ids;
using attn_util::wave_sum;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
// columns of one row a lane holds in registers: a panel is 64 * 16 columns
constexpr int kHeld = 16;
// grid cap of the backward (unmeasured, see the header)
constexpr int64_t kGateMaxBlocks = 1024;
// gate_sum_kernel: 64 columns x kSumSegs runs of consecutive blocks
constexpr int kSumSegs = 8;

// VEC fp32 values of a / b / a partial row, in accesses of 16 bytes at most
template <int VEC>
__device__ __forceinline__ void ld_f32(const float* p, float (&v)[VEC]) {
  if constexpr (VEC <= 4) {
    ld_vec<float, VEC>(p, v);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; k += 4) {
      float q[4];
      ld_vec<float, 4>(p + k, q);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[k + i] = q[i];
    }
  }
}

template <int VEC>
__device__ __forceinline__ void st_f32(float* p, const float (&v)[VEC]) {
  if constexpr (VEC <= 4) {
    st_vec<float, VEC>(p, v);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; k += 4) {
      const float q[4] = {v[k], v[k + 1], v[k + 2], v[k + 3]};
      st_vec<float, 4>(p + k, q);
    }
  }
}

// the panel's slice of a and b, zero past the row's end
template <int VEC, int NCH>
__device__ __forceinline__ void ld_panel_ab(const float* __restrict__ a,
                                            const float* __restrict__ b,
                                            int c0, int lane, int F,
                                            float (&av)[NCH][VEC],
                                            float (&bv)[NCH][VEC]) {
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int f = (c0 + j) * (kWave * VEC) + lane * VEC;
#pragma unroll
    for (int k = 0; k < VEC; ++k) av[j][k] = bv[j][k] = 0.f;
    if (f < F) {
      ld_f32<VEC>(a + f, av[j]);
      ld_f32<VEC>(b + f, bv[j]);
    }
  }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

template <typename T, int VEC, int NCH>
__global__ __launch_bounds__(kThreads) void gate_fwd_kernel(
    const T* __restrict__ r, const T* __restrict__ m,
    const float* __restrict__ a, const float* __restrict__ b,
    T* __restrict__ out, float* __restrict__ beta, int64_t N, int F) {
  constexpr int CH = kWave * VEC;
  const auto ids = wave_ids();
  const int lane = ids.lane;
  const int nchunks = (F + CH - 1) / CH;

  // this lane's share of <a, r> + <b, m> over chunk c, from memory
  auto stream = [&](const T* rr, const T* mr, int c, float& part) {
    const int f = c * CH + lane * VEC;
    if (f >= F) return;
    float rv[VEC], mv[VEC], av[VEC], bv[VEC];
    ld_vec<T, VEC>(rr + f, rv);
    ld_vec<T, VEC>(mr + f, mv);
    ld_f32<VEC>(a + f, av);
    ld_f32<VEC>(b + f, bv);
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      part = fmaf(bv[k], mv[k], fmaf(av[k], rv[k], part));
  };

  for (int c0 = 0; c0 < nchunks; c0 += NCH) {  // one pass when F <= 1024
    float av[NCH][VEC], bv[NCH][VEC];
    ld_panel_ab<VEC, NCH>(a, b, c0, lane, F, av, bv);

    for (int64_t row = ids.wave_global; row < N; row += ids.nwaves) {
      const T* rr = r + row * F;
      const T* mr = m + row * F;
      float rv[NCH][VEC], mv[NCH][VEC];
      float part = 0.f;
      for (int c = 0; c < c0; ++c) stream(rr, mr, c, part);
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int f = (c0 + j) * CH + lane * VEC;
        if (f < F) {
          ld_vec<T, VEC>(rr + f, rv[j]);
          ld_vec<T, VEC>(mr + f, mv[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int f = (c0 + j) * CH + lane * VEC;
        if (f < F) {
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            part = fmaf(bv[j][k], mv[j][k], fmaf(av[j][k], rv[j][k], part));
        }
      }
      for (int c = c0 + NCH; c < nchunks; ++c) stream(rr, mr, c, part);

      const float bt = 1.f / (1.f + expf(-wave_sum(part)));
      if (c0 == 0 && lane == 0) beta[row] = bt;
      T* orow = out + row * F;
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int f = (c0 + j) * CH + lane * VEC;
        if (f < F) {
          float o[VEC];
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            o[k] = fmaf(bt, rv[j][k] - mv[j][k], mv[j][k]);
          st_vec<T, VEC>(orow + f, o);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------

template <typename T, int VEC, int NCH>
__global__ __launch_bounds__(kThreads) void gate_bwd_kernel(
    const T* __restrict__ g, const T* __restrict__ r, const T* __restrict__ m,
    const float* __restrict__ a, const float* __restrict__ b,
    const float* __restrict__ beta, T* __restrict__ d_r, T* __restrict__ d_m,
    float* __restrict__ partial, int64_t N, int F) {
  constexpr int CH = kWave * VEC;
  // the accumulators of waves 1.. of the block, [wave - 1][da | db][slot][lane]
  __shared__ float lds[kWaves - 1][2][NCH * VEC][kWave];
  const auto ids = wave_ids();
  const int lane = ids.lane;
  const int wave = threadIdx.x / kWave;
  const int nchunks = (F + CH - 1) / CH;

  // this lane's share of <g, r - m> over chunk c, from memory
  auto stream = [&](int64_t row, int c, float& part) {
    const int f = c * CH + lane * VEC;
    if (f >= F) return;
    float gv[VEC], rv[VEC], mv[VEC];
    ld_vec<T, VEC>(g + row * F + f, gv);
    ld_vec<T, VEC>(r + row * F + f, rv);
    ld_vec<T, VEC>(m + row * F + f, mv);
#pragma unroll
    for (int k = 0; k < VEC; ++k) part = fmaf(gv[k], rv[k] - mv[k], part);
  };

  for (int c0 = 0; c0 < nchunks; c0 += NCH) {  // one pass when F <= 1024
    float av[NCH][VEC], bv[NCH][VEC];
    ld_panel_ab<VEC, NCH>(a, b, c0, lane, F, av, bv);
    float acc_a[NCH][VEC] = {};
    float acc_b[NCH][VEC] = {};

    for (int64_t row = ids.wave_global; row < N; row += ids.nwaves) {
      const float bt = beta[row];
      float gv[NCH][VEC], rv[NCH][VEC], mv[NCH][VEC];
      float part = 0.f;
      for (int c = 0; c < c0; ++c) stream(row, c, part);
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int f = (c0 + j) * CH + lane * VEC;
        if (f < F) {
          ld_vec<T, VEC>(g + row * F + f, gv[j]);
          ld_vec<T, VEC>(r + row * F + f, rv[j]);
          ld_vec<T, VEC>(m + row * F + f, mv[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int f = (c0 + j) * CH + lane * VEC;
        if (f < F) {
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            part = fmaf(gv[j][k], rv[j][k] - mv[j][k], part);
        }
      }
      for (int c = c0 + NCH; c < nchunks; ++c) stream(row, c, part);

      const float s = wave_sum(part) * bt * (1.f - bt);
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int f = (c0 + j) * CH + lane * VEC;
        if (f < F) {
          float dr[VEC], dm[VEC];
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            dr[k] = fmaf(s, av[j][k], bt * gv[j][k]);
            dm[k] = fmaf(s, bv[j][k], (1.f - bt) * gv[j][k]);
            acc_a[j][k] = fmaf(s, rv[j][k], acc_a[j][k]);
            acc_b[j][k] = fmaf(s, mv[j][k], acc_b[j][k]);
          }
          st_vec<T, VEC>(d_r + row * F + f, dr);
          st_vec<T, VEC>(d_m + row * F + f, dm);
        }
      }
    }

    // block partial: wave 0 adds waves 1, 2, 3 in that order
    if (wave > 0) {
#pragma unroll
      for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          lds[wave - 1][0][j * VEC + k][lane] = acc_a[j][k];
          lds[wave - 1][1][j * VEC + k][lane] = acc_b[j][k];
        }
    }
    __syncthreads();
    if (wave == 0) {
      float* prow = partial + static_cast<int64_t>(blockIdx.x) * 2 * F;
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int f = (c0 + j) * CH + lane * VEC;
        if (f < F) {
#pragma unroll
          for (int w = 0; w < kWaves - 1; ++w)
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
              acc_a[j][k] += lds[w][0][j * VEC + k][lane];
              acc_b[j][k] += lds[w][1][j * VEC + k][lane];
            }
          st_f32<VEC>(prow + f, acc_a[j]);
          st_f32<VEC>(prow + F + f, acc_b[j]);
        }
      }
    }
    __syncthreads();  // the next panel writes the LDS again
  }
}

// dab[col] = sum over the blocks' partials of partial[blk][col], col < cols =
// 2F. threadIdx.y picks one of kSumSegs runs of consecutive blocks; a thread
// adds its run in block order and thread (x, 0) adds the runs in run order.
__global__ __launch_bounds__(kWave* kSumSegs) void gate_sum_kernel(
    const float* __restrict__ partial, float* __restrict__ dab, int nblk,
    int cols) {
  __shared__ float runs[kSumSegs][kWave];
  const int col = blockIdx.x * kWave + threadIdx.x;
  const int per = (nblk + kSumSegs - 1) / kSumSegs;
  const int lo = threadIdx.y * per;
  const int hi = min(lo + per, nblk);
  float s = 0.f;
  if (col < cols)
    for (int i = lo; i < hi; ++i)
      s += partial[static_cast<int64_t>(i) * cols + col];
  runs[threadIdx.y][threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.y == 0 && col < cols) {
    float total = runs[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < kSumSegs; ++q) total += runs[q][threadIdx.x];
    dab[col] = total;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// r (and m, g alike): a contiguous fp32 or bf16 [N, F] device tensor
void check_rows(const torch::Tensor& x, const char* name) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous(), "gate: ",
              name, " must be a contiguous [N, F] device tensor");
  TORCH_CHECK(x.scalar_type() == torch::kFloat ||
                  x.scalar_type() == torch::kBFloat16,
              "gate: ", name, " must be fp32 or bf16");
  // column offsets are int
  TORCH_CHECK(x.size(1) < (int64_t{1} << 30), "gate: ", name, " is too wide");
}

void check_like(const torch::Tensor& x, const torch::Tensor& r,
                const char* name) {
  check_rows(x, name);
  TORCH_CHECK(x.sizes() == r.sizes() && x.scalar_type() == r.scalar_type() &&
                  x.device() == r.device(),
              "gate: ", name, " must have r's shape, dtype and device");
}

// a / b: fp32 [F]; beta: fp32 [N]
void check_vector(const torch::Tensor& x, const torch::Tensor& r, int64_t n,
                  const char* name) {
  TORCH_CHECK(x.is_cuda() && x.device() == r.device() && x.dim() == 1 &&
                  x.is_contiguous() && x.scalar_type() == torch::kFloat &&
                  x.size(0) == n,
              "gate: ", name, " must be a contiguous fp32 [", n,
              "] tensor on r's device");
}

// Widest lane access (16 bytes at most) that F and every base address allow:
// rows start at multiples of F elements, so F % vec == 0 keeps them aligned.
// `rows` are of elem bytes per element, `vectors` are fp32.
int pick_gate_vec(int64_t F, int64_t elem,
                  std::initializer_list<const void*> rows,
                  std::initializer_list<const void*> vectors) {
  int vec = static_cast<int>(16 / elem);
  auto fits = [&](int v) {
    if (F % v) return false;
    for (const void* p : rows)
      if (!aligned_to(p, v * elem)) return false;
    for (const void* p : vectors)
      if (!aligned_to(p, std::min(v, 4) * 4)) return false;
    return true;
  };
  while (vec > 1 && !fits(vec)) vec >>= 1;
  return vec;
}

// fn(T tag, VEC, NCH) for the instance that serves (dtype, vec, F): NCH is
// the power of two that covers the row, or the full panel for F > 1024
template <typename T, int VEC, typename Fn>
void dispatch_chunks(int nch, Fn&& fn) {
  auto run = [&](auto n) {
    if constexpr (decltype(n)::value * VEC <= kHeld)
      fn(T{}, std::integral_constant<int, VEC>{}, n);
  };
  switch (nch) {
    case 1:
      run(std::integral_constant<int, 1>{});
      break;
    case 2:
      run(std::integral_constant<int, 2>{});
      break;
    case 4:
      run(std::integral_constant<int, 4>{});
      break;
    case 8:
      run(std::integral_constant<int, 8>{});
      break;
    default:
      run(std::integral_constant<int, 16>{});
  }
}

template <typename Fn>
void dispatch_gate(const torch::Tensor& r, int vec, Fn&& fn) {
  const int64_t chunks = (r.size(1) + kWave * vec - 1) / (kWave * vec);
  int nch = 1;
  while (nch < chunks && nch * vec < kHeld) nch <<= 1;
  const bool bf16 = r.scalar_type() == torch::kBFloat16;
  dispatch_vec(vec, [&](auto v) {
    constexpr int VEC = decltype(v)::value;
    if (bf16)
      dispatch_chunks<__hip_bfloat16, VEC>(nch, fn);
    else if constexpr (VEC <= 4)
      dispatch_chunks<float, VEC>(nch, fn);
  });
}

template <typename T>
const T* cptr(const torch::Tensor& x) {
  return reinterpret_cast<const T*>(x.data_ptr());
}
template <typename T>
T* mptr(torch::Tensor& x) {
  return reinterpret_cast<T*>(x.data_ptr());
}

}  // namespace

std::vector<torch::Tensor> gate_fwd_hip(torch::Tensor r, torch::Tensor m,
                                        torch::Tensor a, torch::Tensor b) {
  check_rows(r, "r");
  check_like(m, r, "m");
  const int64_t N = r.size(0);
  const int64_t F = r.size(1);
  check_vector(a, r, F, "a");
  check_vector(b, r, F, "b");
  auto out = torch::empty_like(r);
  auto beta = torch::empty({N}, r.options().dtype(torch::kFloat));
  if (N == 0) return {out, beta};
  if (F == 0) return {out, beta.fill_(0.5f)};  // sigmoid of an empty sum
  const int vec = pick_gate_vec(
      F, r.element_size(), {r.data_ptr(), m.data_ptr(), out.data_ptr()},
      {a.data_ptr(), b.data_ptr()});
  const int64_t blocks = grid_for(N, kThreads);
  dispatch_gate(r, vec, [&](auto tag, auto v, auto n) {
    using T = decltype(tag);
    hipLaunchKernelGGL(
        HIP_KERNEL_NAME(gate_fwd_kernel<T, decltype(v)::value,
                                        decltype(n)::value>),
        dim3(blocks), dim3(kThreads), 0, current_stream(), cptr<T>(r),
        cptr<T>(m), a.data_ptr<float>(), b.data_ptr<float>(), mptr<T>(out),
        beta.data_ptr<float>(), N, static_cast<int>(F));
  });
  check_launch();
  return {out, beta};
}

std::vector<torch::Tensor> gate_bwd_hip(torch::Tensor g, torch::Tensor r,
                                        torch::Tensor m, torch::Tensor a,
                                        torch::Tensor b, torch::Tensor beta) {
  check_rows(r, "r");
  check_like(m, r, "m");
  check_like(g, r, "g");
  const int64_t N = r.size(0);
  const int64_t F = r.size(1);
  check_vector(a, r, F, "a");
  check_vector(b, r, F, "b");
  check_vector(beta, r, N, "beta");
  auto d_r = torch::empty_like(r);
  auto d_m = torch::empty_like(r);
  auto dab = torch::empty({2, F}, r.options().dtype(torch::kFloat));
  if (N == 0 || F == 0) {
    dab.zero_();
    return {d_r, d_m, dab[0], dab[1]};
  }
  // the grid is a function of N alone: da / db are reproducible
  const int64_t blocks =
      std::min<int64_t>((N + kWaves - 1) / kWaves, kGateMaxBlocks);
  auto partial =
      torch::empty({blocks, 2 * F}, r.options().dtype(torch::kFloat));
  const int vec = pick_gate_vec(
      F, r.element_size(),
      {g.data_ptr(), r.data_ptr(), m.data_ptr(), d_r.data_ptr(),
       d_m.data_ptr()},
      {a.data_ptr(), b.data_ptr(), partial.data_ptr()});
  auto stream = current_stream();
  dispatch_gate(r, vec, [&](auto tag, auto v, auto n) {
    using T = decltype(tag);
    hipLaunchKernelGGL(
        HIP_KERNEL_NAME(gate_bwd_kernel<T, decltype(v)::value,
                                        decltype(n)::value>),
        dim3(blocks), dim3(kThreads), 0, stream, cptr<T>(g), cptr<T>(r),
        cptr<T>(m), a.data_ptr<float>(), b.data_ptr<float>(),
        beta.data_ptr<float>(), mptr<T>(d_r), mptr<T>(d_m),
        partial.data_ptr<float>(), N, static_cast<int>(F));
  });
  check_launch();
  hipLaunchKernelGGL(gate_sum_kernel, dim3((2 * F + kWave - 1) / kWave),
                     dim3(kWave, kSumSegs), 0, stream,
                     partial.data_ptr<float>(), dab.data_ptr<float>(),
                     static_cast<int>(blocks), static_cast<int>(2 * F));
  check_launch();
  return {d_r, d_m, dab[0], dab[1]};
}
