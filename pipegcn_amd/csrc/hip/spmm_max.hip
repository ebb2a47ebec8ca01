// Max aggregation for gfx950: the (max, arg-max) reduction over a
// neighbourhood and its backward. The first aggregation pair here that is not
// a sum (docs/DESIGN.md, "Max aggregation").
//
//   out[r,c] = max over the edges e of row r of z[indices[e], c]
//   arg[r,c] = source id of the FIRST edge of row r, in stored order, that
//              attains it: initialised from the row's first edge, updated on
//              strict >. Rows without edges give out = 0, arg = -1.
//   grad_z[u,c] = sum of g[r,c] over the destinations r with arg[r,c] == u
//
// The comparison is in fp32 and the result is one of the inputs, so out is
// exact in fp32 and bf16. NaN inputs are unspecified.
//
//  - spmm_max_fwd : over the CSR, gathers z[u]; one wave per (row, chunk of
//                   64 * VEC columns) as spmm_csr_kernel: same loads, a
//                   compare-select in place of the add. WITH_ARG = false drops
//                   the ids and the arg store for calls that need no gradient.
//  - spmm_max_bwd : over a CSC WITHOUT repeated entries (rows = sources u),
//                   gathers g[r] and arg[r] per entry and adds g where
//                   arg == u. No atomics; with a repeated entry the match
//                   would count that destination twice, hence the simple CSC
//                   (HaloGraph.csc_simple).
//
// One fixed lane owns a column and walks the row in stored order, so results
// are bitwise reproducible and independent of row_order.
//
// The lane width starts from pick_vec's byte preference (kernels.hip), which
// was measured for the mean SpMM and not re-measured for these kernels. It
// always divides F, so a lane's VEC columns are all inside the row or all
// past it: the tail chunk needs the lane guard only.
//
// Compiler resource report: profiles/README.md, "Max aggregation". No
// instance uses scratch.

#include "../common.h"
#include "attn_util.h"
#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>
#include <vector>

namespace {

// ld_vec / st_vec, for_edges and the host-side input checks are shared with
// the attention kernels
using namespace attn_util;

// int32 ids, VEC per lane: one 4/8/16-byte access, or two 16-byte ones for
// VEC = 8 (arg is 4 bytes per element whatever z's dtype is)
template <int VEC>
__device__ __forceinline__ void ld_ids(const int32_t* p, int32_t (&v)[VEC]) {
  constexpr int W = VEC < 4 ? VEC : 4;
  using R = typename raw_vec<4 * W>::type;
#pragma unroll
  for (int b = 0; b < VEC; b += W) {
    const R r = *reinterpret_cast<const R*>(p + b);
    __builtin_memcpy(&v[b], &r, sizeof(R));
  }
}

template <int VEC>
__device__ __forceinline__ void st_ids(int32_t* p, const int32_t (&v)[VEC]) {
  constexpr int W = VEC < 4 ? VEC : 4;
  using R = typename raw_vec<4 * W>::type;
#pragma unroll
  for (int b = 0; b < VEC; b += W) {
    R r;
    __builtin_memcpy(&r, &v[b], sizeof(R));
    __builtin_nontemporal_store(r, reinterpret_cast<R*>(p + b));
  }
}

// The wave of a (row, chunk) pair loop with its index in a scalar register,
// as spmm_csr_kernel forms it: row, edge cursor and node ids are then
// wave-uniform for the compiler too. The geometry arrives through default
// arguments for the reason given at attn_util::wave_ids.
struct UniformWave {
  int64_t wave_global;
  int lane;
  int64_t nwaves;
};

__device__ __forceinline__ UniformWave uniform_wave(
    unsigned block = blockIdx.x, unsigned block_dim = blockDim.x,
    unsigned thread = threadIdx.x, unsigned grid_dim = gridDim.x) {
  const int wave_in_block =
      __builtin_amdgcn_readfirstlane(static_cast<int>(thread) / kWave);
  const int64_t waves_per_block = block_dim / kWave;
  return {static_cast<int64_t>(block) * waves_per_block + wave_in_block,
          static_cast<int>(thread & (kWave - 1)),
          static_cast<int64_t>(grid_dim) * waves_per_block};
}

// ---------------------------------------------------------------------------
// forward over the CSR (row = destination r, columns = sources u)
// ---------------------------------------------------------------------------
template <typename T, int VEC, bool WITH_ARG>
__global__ void __launch_bounds__(256) spmm_max_fwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ z, const int32_t* __restrict__ row_order,
    T* __restrict__ out, int32_t* __restrict__ arg, int64_t num_rows,
    int64_t F, int64_t nchunks) {
  const UniformWave wv = uniform_wave();
  const int64_t npairs = num_rows * nchunks;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nchunks;
    if (row_order) r = row_order[r];
    // VEC divides F (host check): a lane is all inside the row or all past it
    const int64_t f0 = pair % nchunks * (kWave * VEC) + wv.lane * VEC;
    if (f0 >= F) continue;

    float best[VEC];
    int32_t bid[VEC];
    const int64_t e_begin = indptr[r];
    const int64_t e_end = indptr[r + 1];
    if (e_begin == e_end) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        best[k] = 0.f;
        bid[k] = -1;
      }
    } else {
      // the contract's initial value is the first edge, not -inf: a row of
      // -inf still names its first source
      const int32_t first = indices[e_begin];
      ld_vec<T, VEC>(z + static_cast<int64_t>(first) * F + f0, best);
#pragma unroll
      for (int k = 0; k < VEC; ++k) bid[k] = first;

      auto batch = [&](auto n_c, const auto& uu) {
        constexpr int N = decltype(n_c)::value;
        float v[N][VEC];
#pragma unroll
        for (int i = 0; i < N; ++i)
          ld_vec<T, VEC>(z + static_cast<int64_t>(uu[i]) * F + f0, v[i]);
        // in stored order, strict >: the first edge that attains the
        // maximum keeps it
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            const bool gt = v[i][k] > best[k];
            best[k] = gt ? v[i][k] : best[k];
            if constexpr (WITH_ARG) bid[k] = gt ? uu[i] : bid[k];
          }
        }
      };
      for_edges<4>(indices, e_begin + 1, e_end, batch);
    }

    st_vec<T, VEC>(out + r * F + f0, best);
    if constexpr (WITH_ARG) st_ids<VEC>(arg + r * F + f0, bid);
  }
}

// ---------------------------------------------------------------------------
// backward over a CSC without repeated entries (row = source u, columns =
// destinations r): two row gathers per entry, g[r] and arg[r]
// ---------------------------------------------------------------------------
template <typename T, int VEC>
__global__ void __launch_bounds__(256) spmm_max_bwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ g, const int32_t* __restrict__ arg,
    const int32_t* __restrict__ row_order, T* __restrict__ grad_z,
    int64_t num_rows, int64_t F, int64_t nchunks) {
  const UniformWave wv = uniform_wave();
  const int64_t npairs = num_rows * nchunks;

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
      float gv[N][VEC];
      int32_t av[N][VEC];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int64_t at = static_cast<int64_t>(rr[i]) * F + f0;
        ld_vec<T, VEC>(g + at, gv[i]);
        ld_ids<VEC>(arg + at, av[i]);
      }
#pragma unroll
      for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          acc[k] += av[i][k] == u ? gv[i][k] : 0.f;
      }
    };
    for_edges<4>(indices, indptr[r], indptr[r + 1], batch);

    st_vec<T, VEC>(grad_z + r * F + f0, acc);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

constexpr const char* kOp = "spmm_max";

void check_arg(const torch::Tensor& arg, int64_t rows, int64_t F) {
  TORCH_CHECK(arg.is_cuda() && arg.dim() == 2 && arg.is_contiguous() &&
                  arg.scalar_type() == torch::kInt,
              kOp, ": arg must be a contiguous int32 [rows, F] tensor");
  TORCH_CHECK(arg.size(0) >= rows && arg.size(1) == F, kOp, ": arg is [",
              arg.size(0), ", ", arg.size(1), "] but the graph references ",
              rows, " rows of width ", F);
}

// pick_vec's width, narrowed until every pointer takes the lane access:
// `elems` hold `elem_size`-byte elements, `ids` int32 (16 bytes at the most
// per access)
int lane_vec(int64_t F, int64_t num_rows, int64_t elem_size,
             std::initializer_list<const void*> elems, const void* ids) {
  int vec = pick_vec(F, num_rows, elem_size);
  auto fits = [&](int v) {
    for (const void* p : elems)
      if (!aligned_to(p, v * elem_size)) return false;
    return ids == nullptr || aligned_to(ids, std::min(4 * v, 16));
  };
  while (vec > 1 && !fits(vec)) vec /= 2;
  TORCH_CHECK(F % vec == 0 && vec * elem_size <= 16, kOp, ": lane width ",
              vec, " does not fit rows of ", F, " elements");
  return vec;
}

template <typename T>
const T* cptr(const torch::Tensor& x) {
  return reinterpret_cast<const T*>(x.data_ptr());
}
template <typename T>
T* mptr(torch::Tensor& x) {
  return reinterpret_cast<T*>(x.data_ptr());
}

// fn(T{}, VEC as an integral constant) for x's element type and a lane width
// that lane_vec returned
template <typename Fn>
void dispatch(const torch::Tensor& x, int vec, Fn&& fn) {
  dispatch_vec(vec, [&](auto v) {
    if (x.scalar_type() == torch::kBFloat16) {
      fn(__hip_bfloat16{}, v);
    } else if constexpr (v.value <= 4) {
      fn(float{}, v);
    }
  });
}

struct Launch {
  int64_t nchunks;
  dim3 grid, block;
};

Launch launch_of(int64_t num_rows, int64_t F, int vec) {
  constexpr int threads = 256;  // whole waves: the kernels keep the wave
  static_assert(threads % kWave == 0);  // index in a scalar register
  const int64_t nchunks = (F + kWave * vec - 1) / (kWave * vec);
  return {nchunks, dim3(grid_for(num_rows * nchunks, threads)),
          dim3(threads)};
}

}  // namespace

std::vector<torch::Tensor> spmm_max_fwd_hip(torch::Tensor indptr,
                                            torch::Tensor indices,
                                            torch::Tensor z,
                                            torch::Tensor row_order,
                                            int64_t num_cols, bool with_arg) {
  check_graph(kOp, indptr, indices);
  const int64_t num_rows = indptr.numel() - 1;
  check_features(kOp, z, num_cols, 1, "z");
  const int64_t F = z.size(1);
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto out = torch::empty({num_rows, F}, z.options());
  torch::Tensor arg;
  if (with_arg)
    arg = torch::empty({num_rows, F}, z.options().dtype(torch::kInt));
  if (num_rows > 0) {
    const int vec =
        lane_vec(F, num_rows, z.element_size(),
                 {z.data_ptr(), out.data_ptr()},
                 with_arg ? arg.data_ptr() : nullptr);
    const Launch l = launch_of(num_rows, F, vec);
    dispatch(z, vec, [&](auto tag, auto v) {
      using T = decltype(tag);
      constexpr int V = decltype(v)::value;
      auto run = [&](auto kern, int32_t* ap) {
        hipLaunchKernelGGL(kern, l.grid, l.block, 0, current_stream(),
                           indptr.data_ptr<int64_t>(),
                           indices.data_ptr<int32_t>(), cptr<T>(z), rop,
                           mptr<T>(out), ap, num_rows, F, l.nchunks);
      };
      if (with_arg)
        run(HIP_KERNEL_NAME(spmm_max_fwd_kernel<T, V, true>),
            arg.data_ptr<int32_t>());
      else
        run(HIP_KERNEL_NAME(spmm_max_fwd_kernel<T, V, false>), nullptr);
    });
    check_launch();
  }
  if (with_arg) return {out, arg};
  return {out};
}

torch::Tensor spmm_max_bwd_hip(torch::Tensor indptr, torch::Tensor indices,
                               torch::Tensor g, torch::Tensor arg,
                               torch::Tensor row_order, int64_t num_cols) {
  // indptr/indices are the simple CSC: rows = sources, columns = destinations
  check_graph(kOp, indptr, indices);
  const int64_t num_rows = indptr.numel() - 1;
  check_features(kOp, g, num_cols, 1, "g");
  const int64_t F = g.size(1);
  check_arg(arg, num_cols, F);
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto grad_z = torch::empty({num_rows, F}, g.options());
  if (num_rows == 0) return grad_z;
  const int vec = lane_vec(F, num_rows, g.element_size(),
                           {g.data_ptr(), grad_z.data_ptr()}, arg.data_ptr());
  const Launch l = launch_of(num_rows, F, vec);
  dispatch(g, vec, [&](auto tag, auto v) {
    using T = decltype(tag);
    constexpr int V = decltype(v)::value;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spmm_max_bwd_kernel<T, V>), l.grid,
                       l.block, 0, current_stream(),
                       indptr.data_ptr<int64_t>(),
                       indices.data_ptr<int32_t>(), cptr<T>(g),
                       arg.data_ptr<int32_t>(), rop, mptr<T>(grad_z),
                       num_rows, F, l.nchunks);
  });
  check_launch();
  return grad_z;
}
