// Edge dropout (DropEdge) for the mean / GCN aggregation on gfx950: a masked
// variant of spmm_csr_kernel (kernels.hip; docs/DESIGN.md, "Edge dropout").
//
//   out[r,:] = dst_scale[r] * scale *
//              sum over the KEPT edges e of row r of
//                  src_scale[indices[e]] * feat[indices[e],:]
//
// keep(e) is the attention-dropout hash of the edge's endpoints with one head
// (attn_util.h: drop_base / drop_mix; ops.edge_drop_keep is the torch mirror),
// recomputed here per edge and never stored. Over the CSR the row is the
// destination v and the gathered id the source u; over the CSC it is the other
// way round, so the caller hands the two pre-mix multipliers in the order
// (row, gathered id) and both passes draw the same bit for the same edge.
//
// Same scheduling shape as spmm_csr_kernel: one wave per (row, chunk of
// 64 * VEC columns), grid-stride, optional row_order, wave index in a scalar
// register. Row, edge cursor, ids, hash and keep bit are therefore
// wave-uniform and live on the scalar unit; the vector unit sees the gathers
// and the adds only.
//
// A dropped edge issues no gather. The kept ids are compacted: they enter a
// four-slot scalar queue, and whenever it is full the wave issues four gathers
// back to back and adds v0 + v1 + v2 + v3, as the dense kernel does per four
// edges. The 0-3 ids left after the row are gathered once, outside the loop.
// (A per-edge "load or not" would make the compiler wait for each load on its
// own, one memory round trip per edge.)
//
// Summation order: the kept edges in stored order, in groups of four counted
// in KEPT order. It depends neither on row_order nor on where the row starts
// in `indices`. A row whose edges are all dropped stores zeros.
//
// n_live (HAS_LIVE) is spmm_csr_kernel's redirect of dead rows: the id is
// hashed as stored and gathered as min(id, *n_live).
//
// The lane width is pick_vec's (kernels.hip), narrowed to the pointers'
// alignment; it always divides F, so a lane's VEC columns are all inside the
// row or all past it and the tail chunk needs the lane guard only.

#include "../common.h"
#include "attn_util.h"
#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace {

using namespace attn_util;

template <typename T, int VEC, bool HAS_SRC_SCALE, bool HAS_LIVE>
__global__ void __launch_bounds__(256) spmm_drop_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ feat, const float* __restrict__ dst_scale,
    const float* __restrict__ src_scale, const int32_t* __restrict__ row_order,
    T* __restrict__ out, int64_t num_rows, int64_t F, int64_t nchunks,
    const int32_t* __restrict__ n_live, uint32_t mul_row, uint32_t mul_col,
    uint32_t key, uint32_t thr, float scale) {
  static_assert(!(HAS_SRC_SCALE && HAS_LIVE),
                "the redirect would also redirect the scale's index");
  int32_t live = 0;
  if constexpr (HAS_LIVE) live = max(*n_live, 0);
  // the wave index in a scalar register (spmm_csr_kernel's convention)
  const int wave_in_block =
      __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) / kWave);
  const int64_t waves_per_block = blockDim.x / kWave;
  const int64_t wave_global =
      static_cast<int64_t>(blockIdx.x) * waves_per_block + wave_in_block;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * waves_per_block;
  const int64_t npairs = num_rows * nchunks;

  for (int64_t pair = wave_global; pair < npairs; pair += nwaves) {
    int64_t r = pair / nchunks;
    if (row_order) r = row_order[r];
    const int64_t f0 = pair % nchunks * (kWave * VEC) + lane * VEC;
    if (f0 >= F) continue;

    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;

    // N gathers back to back, then one sum in the order given
    auto gather = [&](auto n_c, const int32_t (&ids)[4]) {
      constexpr int N = decltype(n_c)::value;
      float s[N];
      float v[N][VEC];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        s[i] = HAS_SRC_SCALE ? src_scale[ids[i]] : 1.f;
        const int64_t u = HAS_LIVE ? min(ids[i], live) : ids[i];
        ld_vec<T, VEC>(feat + u * F + f0, v[i]);
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float t = HAS_SRC_SCALE ? s[0] * v[0][k] : v[0][k];
#pragma unroll
        for (int i = 1; i < N; ++i)
          t += HAS_SRC_SCALE ? s[i] * v[i][k] : v[i][k];
        acc[k] += t;
      }
    };

    // the queue of kept ids, oldest first once it is full: with qn < 4 in it
    // they are q[4 - qn .. 3]
    int32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    int qn = 0;
    const uint32_t base =
        drop_base(static_cast<uint32_t>(r), mul_row, 0u, key);
    auto push = [&](int32_t id) {
      if (drop_mix(static_cast<uint32_t>(id) * mul_col + base) >= thr) {
        q0 = q1;
        q1 = q2;
        q2 = q3;
        q3 = id;
        if (++qn == 4) {
          const int32_t ids[4] = {q0, q1, q2, q3};
          gather(std::integral_constant<int, 4>{}, ids);
          qn = 0;
        }
      }
    };

    int64_t e = indptr[r];
    const int64_t e_end = indptr[r + 1];
    // peel until e is 4-aligned, then FOUR ids with ONE dwordx4, then the tail
    for (; e < e_end && (e & 3); ++e) push(indices[e]);
    for (; e + 4 <= e_end; e += 4) {
      const int32x4 uu = *reinterpret_cast<const int32x4*>(indices + e);
      push(uu[0]);
      push(uu[1]);
      push(uu[2]);
      push(uu[3]);
    }
    for (; e < e_end; ++e) push(indices[e]);

    // the last 0-3 kept ids
    if (qn == 3) {
      const int32_t ids[4] = {q1, q2, q3, 0};
      gather(std::integral_constant<int, 3>{}, ids);
    } else if (qn == 2) {
      const int32_t ids[4] = {q2, q3, 0, 0};
      gather(std::integral_constant<int, 2>{}, ids);
    } else if (qn == 1) {
      const int32_t ids[4] = {q3, 0, 0, 0};
      gather(std::integral_constant<int, 1>{}, ids);
    }

    const float s = (dst_scale ? dst_scale[r] : 1.f);
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = acc[k] * s * scale;
    st_vec<T, VEC>(out + r * F + f0, acc);
  }
}

constexpr const char* kOp = "spmm_drop";

}  // namespace

void spmm_drop_hip(torch::Tensor indptr, torch::Tensor indices,
                   torch::Tensor feat, torch::Tensor dst_scale,
                   torch::Tensor src_scale, torch::Tensor row_order,
                   torch::Tensor out, torch::Tensor n_live, bool transposed,
                   int64_t drop_key, int64_t drop_thr, double drop_scale) {
  // spmm_csr_hip's checks
  TORCH_CHECK(feat.is_cuda() && out.is_cuda(), kOp, ": device tensors");
  const bool bf16 = feat.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || feat.scalar_type() == torch::kFloat, kOp,
              ": fp32 or bf16 only");
  TORCH_CHECK(out.scalar_type() == feat.scalar_type());
  TORCH_CHECK(feat.dim() == 2 && out.dim() == 2 && feat.is_contiguous() &&
              out.is_contiguous());
  check_graph(kOp, indptr, indices);
  const int64_t num_rows = out.size(0);
  const int64_t num_src = feat.size(0);
  const int64_t F = feat.size(1);
  TORCH_CHECK(out.size(1) == F && indptr.numel() == num_rows + 1);
  const float* dsp = nullptr;
  if (dst_scale.defined() && dst_scale.numel() > 0) {
    TORCH_CHECK(dst_scale.is_cuda() && dst_scale.is_contiguous() &&
                dst_scale.numel() == num_rows);
    TORCH_CHECK(dst_scale.scalar_type() == torch::kFloat);
    dsp = dst_scale.data_ptr<float>();
  }
  const float* ssp = nullptr;
  if (src_scale.defined() && src_scale.numel() > 0) {
    TORCH_CHECK(src_scale.is_cuda() && src_scale.is_contiguous() &&
                src_scale.numel() == num_src);
    TORCH_CHECK(src_scale.scalar_type() == torch::kFloat);
    ssp = src_scale.data_ptr<float>();
  }
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  const int32_t* nlp = nullptr;
  if (n_live.defined() && n_live.numel() > 0) {
    TORCH_CHECK(n_live.is_cuda() && n_live.numel() == 1 &&
                    n_live.scalar_type() == torch::kInt,
                kOp, ": n_live is one int32 in device memory");
    TORCH_CHECK(ssp == nullptr, kOp,
                ": n_live and src_scale do not combine (the redirect would "
                "pick another row's scale)");
    nlp = n_live.data_ptr<int32_t>();
  }
  const DropArgs drop = drop_args(kOp, drop_key, drop_thr, drop_scale);
  if (num_rows == 0 || F == 0) return;

  // the row's endpoint first: destination over the CSR, source over the CSC
  const uint32_t mul_row = transposed ? kDropMulU : kDropMulV;
  const uint32_t mul_col = transposed ? kDropMulV : kDropMulU;

  const int64_t elem = bf16 ? 2 : 4;
  int vec = pick_vec(F, num_rows, elem);
  while (vec > 1 && !(aligned_to(feat.data_ptr(), vec * elem) &&
                      aligned_to(out.data_ptr(), vec * elem)))
    vec /= 2;
  TORCH_CHECK(F % vec == 0 && vec * elem <= 16, kOp, ": lane width ", vec,
              " does not fit rows of ", F, " elements");

  constexpr int threads = 256;  // whole waves: the kernel keeps the wave
  static_assert(threads % kWave == 0);  // index in a scalar register
  const int64_t nchunks = (F + kWave * vec - 1) / (kWave * vec);
  const dim3 grid(grid_for(num_rows * nchunks, threads));
  auto stream = current_stream();

  dispatch_vec(vec, [&](auto v) {
    constexpr int V = decltype(v)::value;
    auto run = [&](auto tag) {
      using T = decltype(tag);
      if constexpr (V * sizeof(T) <= 16) {
        auto launch = [&](auto kern) {
          hipLaunchKernelGGL(
              kern, grid, dim3(threads), 0, stream,
              indptr.data_ptr<int64_t>(), indices.data_ptr<int32_t>(),
              reinterpret_cast<const T*>(feat.data_ptr()), dsp, ssp, rop,
              reinterpret_cast<T*>(out.data_ptr()), num_rows, F, nchunks, nlp,
              mul_row, mul_col, drop.key, drop.thr, drop.scale);
        };
        if (nlp)
          launch(HIP_KERNEL_NAME(spmm_drop_kernel<T, V, false, true>));
        else if (ssp)
          launch(HIP_KERNEL_NAME(spmm_drop_kernel<T, V, true, false>));
        else
          launch(HIP_KERNEL_NAME(spmm_drop_kernel<T, V, false, false>));
      }
    };
    if (bf16)
      run(__hip_bfloat16{});
    else
      run(float{});
  });
  check_launch();
}
