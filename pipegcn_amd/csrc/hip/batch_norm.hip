// Fused SyncBatchNorm [+ReLU] for gfx950: the four [N, F] passes of
// ops.sync_batch_norm_relu. Storage is fp32 or bf16, all arithmetic and every
// statistic is fp32.
//
//   bn_stats      one read of x        -> sum x, sum x^2            [2, F]
//   bn_apply      one read of x        -> y = [relu]((x - mean) / std * w + b)
//   bn_bwd_stats  one read of dy, x    -> sum g', sum g' x_hat      [2, F]
//   bn_bwd_apply  one read of dy, x    -> dx = (w / n) / std *
//                                             (n g' - dbias - x_hat dweight)
//
// with x_hat = (x - mean) / std and g' = dy where the ReLU let the element
// through, else 0. Nothing of size [N, F] is kept between forward and
// backward but x itself: x_hat and the mask are recomputed by bn_pre(), the
// ONE function every kernel calls, from the same fp32 inputs, so forward and
// backward always agree on the mask. The mask is taken on the fp32
// pre-activation, before y is rounded to the storage dtype.
//
// Work split, the same in all four kernels. A row is P = F / VEC packets of
// VEC columns (one 16-byte access where F and the addresses allow, else 8, 4
// or 2 bytes). A block of 256 threads owns a contiguous stripe of rows. A
// thread owns ONE packet for the whole stripe, so its per-column constants
// (mean, 1 / std, w, b, ...) are loaded once and its column sums live in
// registers. When P < 256 the block splits into G = 256 / P row groups:
// group g takes rows r0 + g, r0 + g + G, ... of the stripe, so consecutive
// groups read consecutive rows and every thread works whatever F is (F = 64
// fp32: 16 packets, 16 groups). When P > 256 (fp32 F > 1024) the block
// walks the row in chunks of 256 packets, one pass over the stripe each. A
// thread issues the loads of kRows1 (one input) or kRows2 (two inputs) of
// its rows before it uses them, in row order.
//
// Column sums are deterministic. A thread adds its rows in row order; the
// groups of a block combine through LDS in group order 0..G-1; the block
// writes one fp32 partial [2, F]; bn_sum_kernel adds the partials of
// consecutive blocks in index order within kSumSegs runs and the runs in run
// order. No atomics: for a given (N, F, dtype) every order is fixed.

#include "../common.h"
#include "attn_util.h"
#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

namespace {

using attn_util::ld_vec;
using attn_util::st_vec;

constexpr int kThreads = 256;
// rows whose loads a thread keeps in flight: kernels with one / two inputs
constexpr int kRows1 = 8;
constexpr int kRows2 = 4;
// Grid cap. The partials are [blocks, 2, F] fp32, so it also bounds the
// second phase. 1024 blocks of 256 threads are 4 per CU; not tuned.
constexpr int64_t kMaxBlocks = 1024;
// bn_sum_kernel: 64 columns x kSumSegs runs of consecutive blocks
constexpr int kSumSegs = 8;
constexpr int kSumInFlight = 8;

// How a block is laid over its stripe (see the header).
struct Geom {
  int tp;      // threads of one row group = packets of one chunk
  int groups;  // row groups per block
  int64_t rows_per_blk;
  int64_t blocks;
};

// A thread's place in the block: group g, packet p of the chunk.
struct Place {
  int g;
  int p;
  bool active;  // false for the threads past groups * tp
  int64_t r0, r1;
};

__device__ __forceinline__ Place place(int tp, int groups,
                                       int64_t rows_per_blk, int64_t N,
                                       unsigned thread = threadIdx.x,
                                       unsigned block = blockIdx.x) {
  Place q;
  q.g = static_cast<int>(thread) / tp;
  q.p = static_cast<int>(thread) - q.g * tp;
  q.active = q.g < groups;
  q.r0 = static_cast<int64_t>(block) * rows_per_blk;
  q.r1 = min(q.r0 + rows_per_blk, N);
  return q;
}

// The pre-activation and x_hat of one element. Every kernel goes through
// here with the same (mean, rstd, w, b), so the sign of `pre` -- the ReLU
// mask -- is the same bit in the forward and in both backward kernels.
__device__ __forceinline__ float bn_pre(float x, float mean, float rstd,
                                        float w, float b, float& x_hat) {
  x_hat = (x - mean) * rstd;
  return fmaf(x_hat, w, b);
}

// per-column constants of a thread's packet: loaded once per chunk
template <int VEC>
struct Cols {
  float mean[VEC], rstd[VEC], w[VEC], b[VEC];
};

template <int VEC>
__device__ __forceinline__ Cols<VEC> ld_cols(const float* __restrict__ mean,
                                             const float* __restrict__ std,
                                             const float* __restrict__ w,
                                             const float* __restrict__ b,
                                             int f) {
  Cols<VEC> c;
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    c.mean[k] = mean[f + k];
    c.rstd[k] = 1.f / std[f + k];
    c.w[k] = w[f + k];
    c.b[k] = b[f + k];
  }
  return c;
}

// Rows r, r + step, ... < r1 of NIN tensors at columns f..f+VEC: the loads of
// ROWS rows are issued together, then fn(row, v[NIN][VEC]) runs in row order.
template <typename T, int VEC, int ROWS, int NIN, typename Fn>
__device__ __forceinline__ void stream_rows(const T* const (&in)[NIN],
                                            int64_t r, int64_t r1,
                                            int64_t step, int64_t F, int f,
                                            Fn&& fn) {
  for (; r + (ROWS - 1) * step < r1; r += ROWS * step) {
    float v[ROWS][NIN][VEC];
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
      for (int i = 0; i < NIN; ++i)
        ld_vec<T, VEC>(in[i] + (r + j * step) * F + f, v[j][i]);
#pragma unroll
    for (int j = 0; j < ROWS; ++j) fn(r + j * step, v[j]);
  }
  for (; r < r1; r += step) {
    float v[NIN][VEC];
#pragma unroll
    for (int i = 0; i < NIN; ++i) ld_vec<T, VEC>(in[i] + r * F + f, v[i]);
    fn(r, v);
  }
}

// The block's two column sums from its threads' (s0, s1): the groups are
// added in group order through LDS and group 0 writes partial[blk][0 | 1][f].
// Every thread of the block must call it (it synchronises).
template <int VEC>
__device__ __forceinline__ void block_partial(float (&lds)[2 * VEC][kThreads],
                                              float (&s0)[VEC],
                                              float (&s1)[VEC],
                                              const Place& q, bool on, int tp,
                                              int groups, int f, int F,
                                              float* __restrict__ partial) {
  if (groups > 1) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      lds[k][threadIdx.x] = s0[k];
      lds[VEC + k][threadIdx.x] = s1[k];
    }
    __syncthreads();
    if (q.g == 0 && on) {
      for (int gg = 1; gg < groups; ++gg) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          s0[k] += lds[k][gg * tp + q.p];
          s1[k] += lds[VEC + k][gg * tp + q.p];
        }
      }
    }
    // groups > 1 means one chunk: the LDS is not written again
  }
  if (q.g == 0 && on) {
    float* row = partial + static_cast<int64_t>(blockIdx.x) * 2 * F + f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      row[k] = s0[k];
      row[F + k] = s1[k];
    }
  }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void bn_stats_kernel(
    const T* __restrict__ x, float* __restrict__ partial, int64_t N, int F,
    int tp, int groups, int64_t rows_per_blk) {
  __shared__ float lds[2 * VEC][kThreads];
  const Place q = place(tp, groups, rows_per_blk, N);
  const int P = F / VEC;
  for (int c0 = 0; c0 < P; c0 += tp) {  // one trip unless P > 256
    const bool on = q.active && c0 + q.p < P;
    const int f = (c0 + q.p) * VEC;
    float s[VEC] = {}, s2[VEC] = {};
    if (on) {
      const T* const in[1] = {x};
      stream_rows<T, VEC, kRows1, 1>(
          in, q.r0 + q.g, q.r1, groups, F, f,
          [&](int64_t, const float(&v)[1][VEC]) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
              s[k] += v[0][k];
              s2[k] = fmaf(v[0][k], v[0][k], s2[k]);
            }
          });
    }
    block_partial<VEC>(lds, s, s2, q, on, tp, groups, f, F, partial);
  }
}

template <typename T, int VEC, bool RELU>
__global__ __launch_bounds__(kThreads) void bn_apply_kernel(
    const T* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ std, const float* __restrict__ w,
    const float* __restrict__ b, T* __restrict__ y, int64_t N, int F, int tp,
    int groups, int64_t rows_per_blk) {
  const Place q = place(tp, groups, rows_per_blk, N);
  const int P = F / VEC;
  if (!q.active) return;
  for (int c0 = q.p; c0 < P; c0 += tp) {
    const int f = c0 * VEC;
    const Cols<VEC> c = ld_cols<VEC>(mean, std, w, b, f);
    const T* const in[1] = {x};
    stream_rows<T, VEC, kRows1, 1>(
        in, q.r0 + q.g, q.r1, groups, F, f,
        [&](int64_t row, const float(&v)[1][VEC]) {
          float o[VEC];
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            float x_hat;
            const float pre =
                bn_pre(v[0][k], c.mean[k], c.rstd[k], c.w[k], c.b[k], x_hat);
            o[k] = RELU && !(pre > 0.f) ? 0.f : pre;
          }
          st_vec<T, VEC>(y + row * F + f, o);
        });
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------

template <typename T, int VEC, bool RELU>
__global__ __launch_bounds__(kThreads) void bn_bwd_stats_kernel(
    const T* __restrict__ dy, const T* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ std,
    const float* __restrict__ w, const float* __restrict__ b,
    float* __restrict__ partial, int64_t N, int F, int tp, int groups,
    int64_t rows_per_blk) {
  __shared__ float lds[2 * VEC][kThreads];
  const Place q = place(tp, groups, rows_per_blk, N);
  const int P = F / VEC;
  for (int c0 = 0; c0 < P; c0 += tp) {
    const bool on = q.active && c0 + q.p < P;
    const int f = (c0 + q.p) * VEC;
    float db[VEC] = {}, dw[VEC] = {};
    if (on) {
      const Cols<VEC> c = ld_cols<VEC>(mean, std, w, b, f);
      const T* const in[2] = {dy, x};
      stream_rows<T, VEC, kRows2, 2>(
          in, q.r0 + q.g, q.r1, groups, F, f,
          [&](int64_t, const float(&v)[2][VEC]) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
              float x_hat;
              const float pre =
                  bn_pre(v[1][k], c.mean[k], c.rstd[k], c.w[k], c.b[k], x_hat);
              const float g = RELU && !(pre > 0.f) ? 0.f : v[0][k];
              db[k] += g;
              dw[k] = fmaf(g, x_hat, dw[k]);
            }
          });
    }
    block_partial<VEC>(lds, db, dw, q, on, tp, groups, f, F, partial);
  }
}

// dsum: fp32 [2, F] = dbias, dweight (summed over every rank)
template <typename T, int VEC, bool RELU>
__global__ __launch_bounds__(kThreads) void bn_bwd_apply_kernel(
    const T* __restrict__ dy, const T* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ std,
    const float* __restrict__ w, const float* __restrict__ b,
    const float* __restrict__ dsum, float n, T* __restrict__ dx, int64_t N,
    int F, int tp, int groups, int64_t rows_per_blk) {
  const Place q = place(tp, groups, rows_per_blk, N);
  const int P = F / VEC;
  if (!q.active) return;
  for (int c0 = q.p; c0 < P; c0 += tp) {
    const int f = c0 * VEC;
    const Cols<VEC> c = ld_cols<VEC>(mean, std, w, b, f);
    float coef[VEC], db[VEC], dw[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      coef[k] = (c.w[k] / n) / std[f + k];
      db[k] = dsum[f + k];
      dw[k] = dsum[F + f + k];
    }
    const T* const in[2] = {dy, x};
    stream_rows<T, VEC, kRows2, 2>(
        in, q.r0 + q.g, q.r1, groups, F, f,
        [&](int64_t row, const float(&v)[2][VEC]) {
          float o[VEC];
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            float x_hat;
            const float pre =
                bn_pre(v[1][k], c.mean[k], c.rstd[k], c.w[k], c.b[k], x_hat);
            const float g = RELU && !(pre > 0.f) ? 0.f : v[0][k];
            o[k] = coef[k] * (n * g - db[k] - x_hat * dw[k]);
          }
          st_vec<T, VEC>(dx + row * F + f, o);
        });
  }
}

// out[col] = sum over the blocks of partial[blk][col], col < cols = 2F.
// threadIdx.y picks one of kSumSegs runs of consecutive blocks; a thread adds
// its run in block order (kSumInFlight loads at a time) and thread (x, 0)
// adds the runs in run order.
__global__ __launch_bounds__(kWave* kSumSegs) void bn_sum_kernel(
    const float* __restrict__ partial, float* __restrict__ out, int nblk,
    int cols) {
  __shared__ float runs[kSumSegs][kWave];
  const int col = blockIdx.x * kWave + threadIdx.x;
  const int per = (nblk + kSumSegs - 1) / kSumSegs;
  const int lo = threadIdx.y * per;
  const int hi = min(lo + per, nblk);
  float s = 0.f;
  if (col < cols) {
    int i = lo;
    for (; i + kSumInFlight <= hi; i += kSumInFlight) {
      float v[kSumInFlight];
#pragma unroll
      for (int j = 0; j < kSumInFlight; ++j)
        v[j] = partial[static_cast<int64_t>(i + j) * cols + col];
#pragma unroll
      for (int j = 0; j < kSumInFlight; ++j) s += v[j];
    }
    for (; i < hi; ++i) s += partial[static_cast<int64_t>(i) * cols + col];
  }
  runs[threadIdx.y][threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.y == 0 && col < cols) {
    float total = runs[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < kSumSegs; ++k) total += runs[k][threadIdx.x];
    out[col] = total;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

void check_rows(const torch::Tensor& x, const char* name) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous(),
              "batch_norm: ", name,
              " must be a contiguous [N, F] device tensor");
  TORCH_CHECK(x.scalar_type() == torch::kFloat ||
                  x.scalar_type() == torch::kBFloat16,
              "batch_norm: ", name, " must be fp32 or bf16");
  // column offsets are int
  TORCH_CHECK(x.size(1) >= 1 && x.size(1) < (int64_t{1} << 30),
              "batch_norm: ", name, " needs 1 <= F < 2^30");
}

void check_like(const torch::Tensor& x, const torch::Tensor& ref,
                const char* name) {
  check_rows(x, name);
  TORCH_CHECK(x.sizes() == ref.sizes() &&
                  x.scalar_type() == ref.scalar_type() &&
                  x.device() == ref.device(),
              "batch_norm: ", name, " must have x's shape, dtype and device");
}

// mean / std / w / b: fp32 [F]; dsum: fp32 [2, F] (numel 2F)
void check_vector(const torch::Tensor& v, const torch::Tensor& x, int64_t n,
                  const char* name) {
  TORCH_CHECK(v.is_cuda() && v.device() == x.device() && v.is_contiguous() &&
                  v.scalar_type() == torch::kFloat && v.numel() == n,
              "batch_norm: ", name, " must be a contiguous fp32 tensor of ",
              n, " elements on x's device");
}

void check_cols(const torch::Tensor& x, const torch::Tensor& mean,
                const torch::Tensor& std, const torch::Tensor& w,
                const torch::Tensor& b) {
  const int64_t F = x.size(1);
  check_vector(mean, x, F, "mean");
  check_vector(std, x, F, "std");
  check_vector(w, x, F, "weight");
  check_vector(b, x, F, "bias");
}

// Widest packet (16 bytes at most) that F and every [N, F] base address
// allow: rows start at multiples of F elements, so F % vec == 0 keeps every
// packet aligned. The fp32 [F] vectors are read a scalar at a time.
int pick_bn_vec(int64_t F, int64_t elem,
                std::initializer_list<const void*> rows) {
  int vec = static_cast<int>(16 / elem);
  auto fits = [&](int v) {
    if (F % v) return false;
    for (const void* p : rows)
      if (!aligned_to(p, v * elem)) return false;
    return true;
  };
  while (vec > 1 && !fits(vec)) vec >>= 1;
  return vec;
}

// rows_in_flight: kRows1 or kRows2, so that a small input still spreads over
// several blocks instead of leaving one to do it all
Geom geom(int64_t N, int64_t F, int vec, int rows_in_flight) {
  Geom g;
  const int64_t P = F / vec;
  g.tp = static_cast<int>(std::min<int64_t>(P, kThreads));
  g.groups = kThreads / g.tp;
  const int64_t per_step = static_cast<int64_t>(g.groups) * rows_in_flight;
  const int64_t want =
      std::min<int64_t>(kMaxBlocks, (N + per_step - 1) / per_step);
  g.rows_per_blk = (N + want - 1) / want;
  g.blocks = (N + g.rows_per_blk - 1) / g.rows_per_blk;
  return g;
}

// fn(T tag, integral_constant VEC) for the instance of (dtype, vec)
template <typename Fn>
void dispatch_bn(const torch::Tensor& x, int vec, Fn&& fn) {
  const bool bf16 = x.scalar_type() == torch::kBFloat16;
  dispatch_vec(vec, [&](auto v) {
    if (bf16)
      fn(__hip_bfloat16{}, v);
    else if constexpr (decltype(v)::value <= 4)
      fn(float{}, v);
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

// second phase: partial [blocks, 2, F] -> out [2, F]
void sum_partials(const torch::Tensor& partial, torch::Tensor& out,
                  int64_t blocks, int64_t F, hipStream_t stream) {
  hipLaunchKernelGGL(bn_sum_kernel, dim3((2 * F + kWave - 1) / kWave),
                     dim3(kWave, kSumSegs), 0, stream,
                     partial.data_ptr<float>(), out.data_ptr<float>(),
                     static_cast<int>(blocks), static_cast<int>(2 * F));
  check_launch();
}

}  // namespace

torch::Tensor bn_stats_hip(torch::Tensor x) {
  check_rows(x, "x");
  const int64_t N = x.size(0), F = x.size(1);
  const auto f32 = x.options().dtype(torch::kFloat);
  if (N == 0) return torch::zeros({2, F}, f32);
  const int vec = pick_bn_vec(F, x.element_size(), {x.data_ptr()});
  const Geom g = geom(N, F, vec, kRows1);
  auto partial = torch::empty({g.blocks, 2, F}, f32);
  auto out = torch::empty({2, F}, f32);
  auto stream = current_stream();
  dispatch_bn(x, vec, [&](auto tag, auto v) {
    using T = decltype(tag);
    hipLaunchKernelGGL(
        HIP_KERNEL_NAME(bn_stats_kernel<T, decltype(v)::value>),
        dim3(g.blocks), dim3(kThreads), 0, stream, cptr<T>(x),
        partial.data_ptr<float>(), N, static_cast<int>(F), g.tp, g.groups,
        g.rows_per_blk);
  });
  check_launch();
  sum_partials(partial, out, g.blocks, F, stream);
  return out;
}

torch::Tensor bn_apply_hip(torch::Tensor x, torch::Tensor mean,
                           torch::Tensor std, torch::Tensor w,
                           torch::Tensor b, bool relu) {
  check_rows(x, "x");
  check_cols(x, mean, std, w, b);
  const int64_t N = x.size(0), F = x.size(1);
  auto y = torch::empty_like(x);
  if (N == 0) return y;
  const int vec =
      pick_bn_vec(F, x.element_size(), {x.data_ptr(), y.data_ptr()});
  const Geom g = geom(N, F, vec, kRows1);
  dispatch_bn(x, vec, [&](auto tag, auto v) {
    using T = decltype(tag);
    constexpr int VEC = decltype(v)::value;
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(g.blocks), dim3(kThreads), 0,
                         current_stream(), cptr<T>(x), mean.data_ptr<float>(),
                         std.data_ptr<float>(), w.data_ptr<float>(),
                         b.data_ptr<float>(), mptr<T>(y), N,
                         static_cast<int>(F), g.tp, g.groups, g.rows_per_blk);
    };
    if (relu)
      launch(HIP_KERNEL_NAME(bn_apply_kernel<T, VEC, true>));
    else
      launch(HIP_KERNEL_NAME(bn_apply_kernel<T, VEC, false>));
  });
  check_launch();
  return y;
}

torch::Tensor bn_bwd_stats_hip(torch::Tensor dy, torch::Tensor x,
                               torch::Tensor mean, torch::Tensor std,
                               torch::Tensor w, torch::Tensor b, bool relu) {
  check_rows(x, "x");
  check_like(dy, x, "dy");
  check_cols(x, mean, std, w, b);
  const int64_t N = x.size(0), F = x.size(1);
  const auto f32 = x.options().dtype(torch::kFloat);
  if (N == 0) return torch::zeros({2, F}, f32);
  const int vec =
      pick_bn_vec(F, x.element_size(), {x.data_ptr(), dy.data_ptr()});
  const Geom g = geom(N, F, vec, kRows2);
  auto partial = torch::empty({g.blocks, 2, F}, f32);
  auto out = torch::empty({2, F}, f32);
  auto stream = current_stream();
  dispatch_bn(x, vec, [&](auto tag, auto v) {
    using T = decltype(tag);
    constexpr int VEC = decltype(v)::value;
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(g.blocks), dim3(kThreads), 0, stream,
                         cptr<T>(dy), cptr<T>(x), mean.data_ptr<float>(),
                         std.data_ptr<float>(), w.data_ptr<float>(),
                         b.data_ptr<float>(), partial.data_ptr<float>(), N,
                         static_cast<int>(F), g.tp, g.groups, g.rows_per_blk);
    };
    if (relu)
      launch(HIP_KERNEL_NAME(bn_bwd_stats_kernel<T, VEC, true>));
    else
      launch(HIP_KERNEL_NAME(bn_bwd_stats_kernel<T, VEC, false>));
  });
  check_launch();
  sum_partials(partial, out, g.blocks, F, stream);
  return out;
}

torch::Tensor bn_bwd_apply_hip(torch::Tensor dy, torch::Tensor x,
                               torch::Tensor mean, torch::Tensor std,
                               torch::Tensor w, torch::Tensor b,
                               torch::Tensor dsum, double whole_size,
                               bool relu) {
  check_rows(x, "x");
  check_like(dy, x, "dy");
  check_cols(x, mean, std, w, b);
  const int64_t N = x.size(0), F = x.size(1);
  check_vector(dsum, x, 2 * F, "dsum");
  auto dx = torch::empty_like(dy);
  if (N == 0) return dx;
  const int vec = pick_bn_vec(F, x.element_size(),
                              {x.data_ptr(), dy.data_ptr(), dx.data_ptr()});
  const Geom g = geom(N, F, vec, kRows2);
  dispatch_bn(x, vec, [&](auto tag, auto v) {
    using T = decltype(tag);
    constexpr int VEC = decltype(v)::value;
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(g.blocks), dim3(kThreads), 0,
                         current_stream(), cptr<T>(dy), cptr<T>(x),
                         mean.data_ptr<float>(), std.data_ptr<float>(),
                         w.data_ptr<float>(), b.data_ptr<float>(),
                         dsum.data_ptr<float>(),
                         static_cast<float>(whole_size), mptr<T>(dx), N,
                         static_cast<int>(F), g.tp, g.groups, g.rows_per_blk);
    };
    if (relu)
      launch(HIP_KERNEL_NAME(bn_bwd_apply_kernel<T, VEC, true>));
    else
      launch(HIP_KERNEL_NAME(bn_bwd_apply_kernel<T, VEC, false>));
  });
  check_launch();
  return dx;
}
