// Hand-written HIP/CDNA4 (gfx950) kernels for the pipegcn_amd hot path.
//
// These replace the reference's DGL CUDA gSpMM (copy_src+sum, invoked at
// /root/reference/module/layer.py:47-49), its index gather/scatter
// (/root/reference/helper/feature_buffer.py:176,215-217) and the EMA
// smoothing correction (/root/reference/helper/feature_buffer.py:189-191).
//
// Design (MI355X-first, see /opt/skills/guides/cdna_hip_programming.md):
//  - wavefront = 64 lanes; feature dim is mapped across lanes with float4/2/1
//    vector loads so each wave issues 1 KiB coalesced reads of a neighbor row.
//  - SpMM is a bandwidth/gather-bound op: one wave owns one (dst-row, feature
//    chunk); the edge loop is unrolled 4x to keep 4 gathers in flight per
//    lane, rows are walked in descending-degree order (LPT scheduling — see
//    pick_vec/profiles), and occupancy stays high (tiny VGPR footprint) so
//    TLP hides HBM latency. The degree-divide epilogue is fused (scale
//    argument); kernels are dtype-templated (fp32, bf16-with-fp32-accumulate).
//  - The backward (transpose) SpMM is the same kernel run over the CSC of the
//    halo graph, built once at setup — no atomics anywhere on the hot path.

#include "../common.h"
#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <vector>

namespace {

// element-type helpers: compute in fp32 (to_f32, hip_util.h), store in T
// (fp32 or bf16)
__device__ __forceinline__ void st_nt(float* p, float v) {
  __builtin_nontemporal_store(v, p);
}
__device__ __forceinline__ void st_nt(__hip_bfloat16* p, float v) {
  union {
    __hip_bfloat16 b;
    unsigned short u;
  } cv;
  cv.b = __float2bfloat16(v);
  __builtin_nontemporal_store(cv.u, reinterpret_cast<unsigned short*>(p));
}
__device__ __forceinline__ void st(float* p, float v) { *p = v; }
__device__ __forceinline__ void st(__hip_bfloat16* p, float v) {
  *p = __float2bfloat16(v);
}

// a fp32 value as a store to T and a load back would leave it
__device__ __forceinline__ float rounded(float v, const float*) { return v; }
__device__ __forceinline__ float rounded(float v, const __hip_bfloat16*) {
  return __bfloat162float(__float2bfloat16(v));
}

// ---------------------------------------------------------------------------
// CSR SpMM: out[r, fchunk] = scale[r] * sum_e feat[indices[e], fchunk]
// One wave per (row, chunk) pair, grid-stride. VEC in {8, 4, 2, 1}.
// ---------------------------------------------------------------------------

// What the EPI instances do to a finished sum before they store it (the
// fused layer backward; docs/DESIGN.md, "Fused layer backward"):
//   v = acc + (r < n_add ? add_rows[r, c] : 0)     when add_rows is set
//   v = bit(r * F + c) of drop_mask ? v * drop_scale : 0   when drop_mask is
// add_rows has add_stride elements between rows (a column slice of a wider
// tensor); drop_mask is the bit mask dropout_fwd_kernel wrote over the
// flattened [num_rows, F] tensor, so at an F that is no multiple of 8 a byte
// straddles two rows. Every step rounds to T as the three kernels it
// replaces did (this kernel's store, the accumulate, dropout_bwd_kernel), so
// the result is theirs bit for bit.
struct SpmmEpilogue {
  const void* add_rows;
  int64_t add_stride;
  int64_t n_add;
  const uint8_t* drop_mask;
  float drop_scale;
};

template <typename T>
__device__ __forceinline__ float spmm_epilogue(const SpmmEpilogue& ep,
                                               float acc, int64_t r,
                                               int64_t c, int64_t F) {
  const T* tag = nullptr;
  float v = rounded(acc, tag);
  if (ep.add_rows != nullptr) {
    // rows past n_add add the +0.0 the padded accumulate added: a sum that
    // rounded to -0.0 comes out +0.0 there too
    const float a = r < ep.n_add ? to_f32(static_cast<const T*>(
                                       ep.add_rows)[r * ep.add_stride + c])
                                 : 0.f;
    v = rounded(v + a, tag);
  }
  if (ep.drop_mask != nullptr) {
    const int64_t i = r * F + c;
    const bool keep = (ep.drop_mask[i >> 3] >> (i & 7)) & 1;
    v = keep ? rounded(v * ep.drop_scale, tag) : 0.f;
  }
  return v;
}

// Chunk-inner order (consecutive waves take the chunks of one row): sweeping
// one column panel at a time to keep it cache-resident measured slower at
// every shape (42.7 -> 49.8 ms at F=602; profiles/README.md).
// 4 gathers in flight per lane are enough: 8 measured neutral and a wave that
// walks a whole row 2x slower — wave-level parallelism, not per-wave depth,
// hides the gather latency (profiles/README.md, negative results).
// HAS_SRC_SCALE fuses a per-source-row scale (the transpose/backward SpMM's
// D^{-1} pre-scale) into the gather.
//
// HAS_LIVE (the last layer's backward; docs/DESIGN.md, "Dead gradient rows"):
// the rows of feat from *n_live on are all zero. Every gathered id u becomes
// min(u, *n_live) — one scalar min per edge, the ids being wave-uniform — so
// the loads of dead rows all hit the one zero row n_live, which stays in
// L1/L2, and never reach HBM. Same loads, same order, same adds: the result
// is bitwise that of the plain kernel.
//
// EPI: the add / dropout epilogue above, instead of dst_scale. A template
// flag, so the instances launched without an epilogue are the code they were.
template <typename T, int VEC, bool HAS_SRC_SCALE, bool HAS_LIVE, bool EPI>
__global__ void spmm_csr_kernel(const int64_t* __restrict__ indptr,
                                const int32_t* __restrict__ indices,
                                const T* __restrict__ feat,
                                const float* __restrict__ dst_scale,
                                const float* __restrict__ src_scale,
                                const int32_t* __restrict__ row_order,
                                T* __restrict__ out, int64_t num_rows,
                                int64_t F, int64_t nchunks,
                                const int32_t* __restrict__ n_live,
                                SpmmEpilogue ep) {
  static_assert(!(HAS_SRC_SCALE && HAS_LIVE),
                "the redirect would also redirect the scale's index");
  // read once per wave (a scalar load); max() only keeps a corrupt count
  // from forming a negative row address
  int32_t live = 0;
  if constexpr (HAS_LIVE) live = max(*n_live, 0);
  // the id as gathered: itself, or the zero row for a dead one
  auto node = [&](int32_t u) -> int64_t {
    return HAS_LIVE ? min(u, live) : u;
  };
  // the wave index in a scalar register: row, edge cursor and node ids are
  // then wave-uniform for the compiler too (spmm_packed.hip has the convention)
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
    const int64_t chunk = pair % nchunks;
    // LPT scheduling: rows pre-sorted by degree descending — the heavy
    // (lognormal-tail) rows start first, light rows backfill
    if (row_order) r = row_order[r];
    const int64_t f0 = chunk * (kWave * VEC) + lane * VEC;
    if (f0 >= F) continue;
    const bool full = (f0 + VEC <= F);

    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;

    const int64_t e_begin = indptr[r];
    const int64_t e_end = indptr[r + 1];
    int64_t e = e_begin;

    if (full) {
      // peel until e is 4-aligned so the unrolled loop can read FOUR int32
      // indices with ONE dwordx4 — per 4 edges the VMEM stream is then
      // 1 index load + 4 row gathers instead of 8 instructions (the gather
      // path is instruction-rate-limited at small F; profiles/README.md).
      for (; e < e_end && (e & 3); ++e) {
        const int64_t u = node(indices[e]);
        const float s = HAS_SRC_SCALE ? src_scale[u] : 1.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          acc[k] += s * to_f32(feat[u * F + f0 + k]);
      }
      for (; e + 4 <= e_end; e += 4) {
        const int32x4 uu = *reinterpret_cast<const int32x4*>(indices + e);
        const int64_t u0 = node(uu[0]);
        const int64_t u1 = node(uu[1]);
        const int64_t u2 = node(uu[2]);
        const int64_t u3 = node(uu[3]);
        float s0 = 1.f, s1 = 1.f, s2 = 1.f, s3 = 1.f;
        if (HAS_SRC_SCALE) {
          s0 = src_scale[u0];
          s1 = src_scale[u1];
          s2 = src_scale[u2];
          s3 = src_scale[u3];
        }
        float v0[VEC], v1[VEC], v2[VEC], v3[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) v0[k] = to_f32(feat[u0 * F + f0 + k]);
#pragma unroll
        for (int k = 0; k < VEC; ++k) v1[k] = to_f32(feat[u1 * F + f0 + k]);
#pragma unroll
        for (int k = 0; k < VEC; ++k) v2[k] = to_f32(feat[u2 * F + f0 + k]);
#pragma unroll
        for (int k = 0; k < VEC; ++k) v3[k] = to_f32(feat[u3 * F + f0 + k]);
        if (HAS_SRC_SCALE) {
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            acc[k] += s0 * v0[k] + s1 * v1[k] + s2 * v2[k] + s3 * v3[k];
        } else {
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            acc[k] += v0[k] + v1[k] + v2[k] + v3[k];
        }
      }
      for (; e < e_end; ++e) {
        const int64_t u = node(indices[e]);
        const float s = HAS_SRC_SCALE ? src_scale[u] : 1.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          acc[k] += s * to_f32(feat[u * F + f0 + k]);
      }
      if constexpr (EPI) {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          st_nt(out + r * F + f0 + k,
                spmm_epilogue<T>(ep, acc[k], r, f0 + k, F));
      } else {
        const float s = dst_scale ? dst_scale[r] : 1.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k) st_nt(out + r * F + f0 + k, acc[k] * s);
      }
    } else {
      // ragged tail chunk: scalar guarded
      for (; e < e_end; ++e) {
        const int64_t u = node(indices[e]);
        const float s = HAS_SRC_SCALE ? src_scale[u] : 1.f;
        for (int k = 0; k < VEC && f0 + k < F; ++k)
          acc[k] += s * to_f32(feat[u * F + f0 + k]);
      }
      if constexpr (EPI) {
        for (int k = 0; k < VEC && f0 + k < F; ++k)
          st(out + r * F + f0 + k,
             spmm_epilogue<T>(ep, acc[k], r, f0 + k, F));
      } else {
        const float s = dst_scale ? dst_scale[r] : 1.f;
        for (int k = 0; k < VEC && f0 + k < F; ++k)
          st(out + r * F + f0 + k, acc[k] * s);
      }
    }
  }
}

template <typename T, int VEC>
void launch_spmm(const int64_t* indptr, const int32_t* indices,
                 const T* feat, const float* dst_scale,
                 const float* src_scale, const int32_t* row_order,
                 const int32_t* n_live, const SpmmEpilogue* epi, T* out,
                 int64_t num_rows, int64_t F, hipStream_t stream) {
  const int64_t nchunks = (F + kWave * VEC - 1) / (kWave * VEC);
  constexpr int threads = 256;  // 4 whole waves: the kernel keeps the
  static_assert(threads % kWave == 0);  // wave index in a scalar register
  const int64_t blocks = grid_for(num_rows * nchunks, threads);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, stream, indptr,
                       indices, feat, dst_scale, src_scale, row_order, out,
                       num_rows, F, nchunks, n_live,
                       epi ? *epi : SpmmEpilogue{});
  };
  // spmm_csr_hip refuses n_live with src_scale, and an epilogue with dst_scale
  if (epi) {
    if (n_live)
      launch(HIP_KERNEL_NAME(spmm_csr_kernel<T, VEC, false, true, true>));
    else if (src_scale)
      launch(HIP_KERNEL_NAME(spmm_csr_kernel<T, VEC, true, false, true>));
    else
      launch(HIP_KERNEL_NAME(spmm_csr_kernel<T, VEC, false, false, true>));
  } else if (n_live) {
    launch(HIP_KERNEL_NAME(spmm_csr_kernel<T, VEC, false, true, false>));
  } else if (src_scale) {
    launch(HIP_KERNEL_NAME(spmm_csr_kernel<T, VEC, true, false, false>));
  } else {
    launch(HIP_KERNEL_NAME(spmm_csr_kernel<T, VEC, false, false, false>));
  }
  check_launch();
}

// ---------------------------------------------------------------------------
// Row gather / scatter-add. One wave per (row, chunk).
// ---------------------------------------------------------------------------

template <typename T, int VEC, bool SCATTER_ADD>
__global__ void rowcopy_kernel(const T* __restrict__ src,
                               const int64_t* __restrict__ idx,
                               T* __restrict__ dst, int64_t nrows,
                               int64_t F, int64_t nchunks) {
  const int64_t wave_global =
      (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t nwaves =
      (static_cast<int64_t>(gridDim.x) * blockDim.x) / kWave;
  const int64_t npairs = nrows * nchunks;
  for (int64_t pair = wave_global; pair < npairs; pair += nwaves) {
    const int64_t i = pair / nchunks;
    const int64_t f0 = pair % nchunks * (kWave * VEC) + lane * VEC;
    if (f0 >= F) continue;
    const int64_t j = idx[i];
    if (f0 + VEC <= F) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if (SCATTER_ADD)
          st(dst + j * F + f0 + k, to_f32(dst[j * F + f0 + k]) +
                                       to_f32(src[i * F + f0 + k]));
        else
          dst[i * F + f0 + k] = src[j * F + f0 + k];
      }
    } else {
      for (int k = 0; f0 + k < F; ++k) {
        if (SCATTER_ADD)
          st(dst + j * F + f0 + k, to_f32(dst[j * F + f0 + k]) +
                                       to_f32(src[i * F + f0 + k]));
        else
          dst[i * F + f0 + k] = src[j * F + f0 + k];
      }
    }
  }
}

template <typename T, int VEC, bool SCATTER_ADD>
void launch_rowcopy(const T* src, const int64_t* idx, T* dst,
                    int64_t nrows, int64_t F, hipStream_t stream) {
  const int64_t nchunks = (F + kWave * VEC - 1) / (kWave * VEC);
  const int threads = 256;
  const int64_t blocks = grid_for(nrows * nchunks, threads);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rowcopy_kernel<T, VEC, SCATTER_ADD>),
                     dim3(blocks), dim3(threads), 0, stream, src, idx, dst,
                     nrows, F, nchunks);
  check_launch();
}

// ---------------------------------------------------------------------------
// EMA: avg = m * avg + (1 - m) * x   (flat elementwise, float4)
// ---------------------------------------------------------------------------

__global__ void ema_kernel(float* __restrict__ avg,
                           const float* __restrict__ x, float m, int64_t n) {
  const int64_t i4 = (static_cast<int64_t>(blockIdx.x) * blockDim.x +
                      threadIdx.x) * 4;
  if (i4 + 4 <= n) {
    float4 a = *reinterpret_cast<float4*>(avg + i4);
    const float4 b = *reinterpret_cast<const float4*>(x + i4);
    a.x = m * a.x + (1.f - m) * b.x;
    a.y = m * a.y + (1.f - m) * b.y;
    a.z = m * a.z + (1.f - m) * b.z;
    a.w = m * a.w + (1.f - m) * b.w;
    *reinterpret_cast<float4*>(avg + i4) = a;
  } else {
    for (int64_t i = i4; i < n; ++i) avg[i] = m * avg[i] + (1.f - m) * x[i];
  }
}

// ---------------------------------------------------------------------------
// Column sum: out[n] = sum_m x[m, n]  (bias/BN reductions — ROCm eager
// .sum(0) runs at ~130 GB/s on tall tensors). Two-phase: blocks accumulate
// row stripes into partials [nblk, F]; a tiny second pass (torch) reduces.
// ---------------------------------------------------------------------------

// rows whose loads a thread issues before it adds them: the adds stay in row
// order, so the sum is the one a row at a time gives, bit for bit, and the
// loads no longer wait for one another
constexpr int kColsumRows = 16;

template <int VEC>
__global__ void colsum_partial_kernel(const float* __restrict__ x,
                                      float* __restrict__ partials,
                                      int64_t M, int64_t F,
                                      int64_t rows_per_blk) {
  const int64_t blk = blockIdx.x;
  const int64_t r0 = blk * rows_per_blk;
  const int64_t r1 = min(r0 + rows_per_blk, M);
  // 256 threads cover F columns in VEC-wide strides
  for (int64_t f0 = static_cast<int64_t>(threadIdx.x) * VEC; f0 < F;
       f0 += 256 * VEC) {
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    if (f0 + VEC <= F) {
      int64_t r = r0;
      for (; r + kColsumRows <= r1; r += kColsumRows) {
        float v[kColsumRows][VEC];
#pragma unroll
        for (int j = 0; j < kColsumRows; ++j)
#pragma unroll
          for (int k = 0; k < VEC; ++k) v[j][k] = x[(r + j) * F + f0 + k];
#pragma unroll
        for (int j = 0; j < kColsumRows; ++j)
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] += v[j][k];
      }
      for (; r < r1; ++r) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] += x[r * F + f0 + k];
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) partials[blk * F + f0 + k] = acc[k];
    } else {
      for (int64_t r = r0; r < r1; ++r)
        for (int k = 0; f0 + k < F; ++k) acc[k] += x[r * F + f0 + k];
      for (int k = 0; f0 + k < F; ++k) partials[blk * F + f0 + k] = acc[k];
    }
  }
}

}  // namespace

// declared in common.h: spmm_max.hip starts from the same preference
int pick_vec(int64_t F, int64_t num_rows, int64_t elem_size) {
  // With LPT row scheduling handling load balance, width is a pure
  // throughput choice. Measured on MI355X (profiles/README.md): 8 B lane
  // loads win at F=256 fp32 (VEC2 15.4 ms vs VEC1 15.7 / VEC4 16.0) and
  // F=256 bf16 (VEC4); 16 B is within ~3%; 4 B loses up to 40% for bf16.
  // Preference: 8 B, then 16 B, then 4 B — first width dividing F.
  if (const char* e = std::getenv("PIPEGCN_SPMM_VEC")) {
    int v = std::atoi(e);
    if ((v == 8 || v == 4 || v == 2 || v == 1) && F % v == 0 &&
        v * elem_size <= 16)
      return v;
  }
  // row count flips the 8B/16B preference: 2.45M-row graphs (products)
  // measured 16B 6% faster at F=256, 233k-row (reddit) 8B 4% faster.
  const bool big = num_rows >= (1 << 20);
  const std::initializer_list<int> pref =
      big ? std::initializer_list<int>{16, 8, 4}
          : std::initializer_list<int>{8, 16, 4};
  for (int bytes : pref) {
    if (bytes < elem_size) continue;
    const int v = bytes / static_cast<int>(elem_size);
    if (F % v == 0) return v;
  }
  return 1;
}

template <typename T>
void spmm_dispatch(torch::Tensor& indptr, torch::Tensor& indices,
                   torch::Tensor& feat, const float* dsp, const float* ssp,
                   const int32_t* rop, const int32_t* nlp,
                   const SpmmEpilogue* epi, torch::Tensor& out,
                   int64_t num_rows, int64_t F, int vec, hipStream_t stream) {
  const T* fp = reinterpret_cast<const T*>(feat.data_ptr());
  T* op = reinterpret_cast<T*>(out.data_ptr());
  const int64_t* ip = indptr.data_ptr<int64_t>();
  const int32_t* xp = indices.data_ptr<int32_t>();
  dispatch_vec(vec, [&](auto v) {
    launch_spmm<T, v.value>(ip, xp, fp, dsp, ssp, rop, nlp, epi, op, num_rows,
                            F, stream);
  });
}

void spmm_csr_hip(torch::Tensor indptr, torch::Tensor indices,
                  torch::Tensor feat, torch::Tensor dst_scale,
                  torch::Tensor src_scale, torch::Tensor row_order,
                  torch::Tensor out, torch::Tensor n_live,
                  torch::Tensor add_rows, int64_t n_add,
                  torch::Tensor drop_mask, double drop_scale) {
  TORCH_CHECK(feat.is_cuda() && out.is_cuda(), "spmm_csr_hip: device tensors");
  const bool bf16 = feat.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || feat.scalar_type() == torch::kFloat,
              "spmm: fp32 or bf16 only");
  TORCH_CHECK(out.scalar_type() == feat.scalar_type());
  TORCH_CHECK(feat.is_contiguous() && out.is_contiguous());
  TORCH_CHECK(indptr.scalar_type() == torch::kLong &&
              indices.scalar_type() == torch::kInt);
  const int64_t num_rows = out.size(0);
  const int64_t num_src = feat.size(0);
  const int64_t F = feat.size(1);
  TORCH_CHECK(out.size(1) == F && indptr.numel() == num_rows + 1);
  const float* dsp = nullptr;
  if (dst_scale.defined() && dst_scale.numel() > 0) {
    TORCH_CHECK(dst_scale.is_contiguous() && dst_scale.numel() == num_rows);
    TORCH_CHECK(dst_scale.scalar_type() == torch::kFloat);
    dsp = dst_scale.data_ptr<float>();
  }
  const float* ssp = nullptr;
  if (src_scale.defined() && src_scale.numel() > 0) {
    TORCH_CHECK(src_scale.is_contiguous() && src_scale.numel() == num_src);
    TORCH_CHECK(src_scale.scalar_type() == torch::kFloat);
    ssp = src_scale.data_ptr<float>();
  }
  const int32_t* rop = nullptr;
  if (row_order.defined() && row_order.numel() > 0) {
    TORCH_CHECK(row_order.is_contiguous() && row_order.numel() == num_rows &&
                row_order.scalar_type() == torch::kInt);
    rop = row_order.data_ptr<int32_t>();
  }
  const int32_t* nlp = nullptr;
  if (n_live.defined() && n_live.numel() > 0) {
    TORCH_CHECK(n_live.is_cuda() && n_live.numel() == 1 &&
                    n_live.scalar_type() == torch::kInt,
                "spmm: n_live is one int32 in device memory");
    TORCH_CHECK(ssp == nullptr,
                "spmm: n_live and src_scale do not combine (the redirect "
                "would pick another row's scale)");
    nlp = n_live.data_ptr<int32_t>();
  }
  SpmmEpilogue ep{};
  if (add_rows.defined() && add_rows.numel() > 0) {
    TORCH_CHECK(add_rows.is_cuda() && add_rows.dim() == 2 &&
                    add_rows.scalar_type() == feat.scalar_type() &&
                    add_rows.size(1) == F &&
                    (F == 1 || add_rows.stride(1) == 1),
                "spmm: add_rows is [n_add, F] in feat's dtype, rows "
                "contiguous");
    TORCH_CHECK(n_add >= 0 && n_add <= add_rows.size(0),
                "spmm: n_add exceeds add_rows");
    TORCH_CHECK(add_rows.size(0) <= 1 || add_rows.stride(0) >= F,
                "spmm: add_rows rows overlap");
    ep.add_rows = add_rows.data_ptr();
    ep.add_stride = add_rows.stride(0);
    ep.n_add = n_add;
  }
  if (drop_mask.defined() && drop_mask.numel() > 0) {
    TORCH_CHECK(drop_mask.is_cuda() && drop_mask.is_contiguous() &&
                    drop_mask.scalar_type() == torch::kUInt8 &&
                    drop_mask.numel() >= (num_rows * F + 7) / 8,
                "spmm: drop_mask holds one bit per output element (uint8)");
    ep.drop_mask = drop_mask.data_ptr<uint8_t>();
    ep.drop_scale = static_cast<float>(drop_scale);
  }
  const bool has_epi = ep.add_rows != nullptr || ep.drop_mask != nullptr;
  TORCH_CHECK(!(has_epi && dsp != nullptr),
              "spmm: the add/dropout epilogue and dst_scale do not combine "
              "(acc * scale + add would round once)");
  const SpmmEpilogue* epi = has_epi ? &ep : nullptr;
  auto stream = current_stream();
  const int vec = pick_vec(F, num_rows, bf16 ? 2 : 4);
  if (bf16)
    spmm_dispatch<__hip_bfloat16>(indptr, indices, feat, dsp, ssp, rop, nlp,
                                  epi, out, num_rows, F, vec, stream);
  else
    spmm_dispatch<float>(indptr, indices, feat, dsp, ssp, rop, nlp, epi, out,
                         num_rows, F, vec, stream);
}

template <typename T, bool SCATTER_ADD>
void rowcopy_dispatch(torch::Tensor& src, torch::Tensor& idx,
                      torch::Tensor& dst, int64_t n, int64_t F,
                      int vec, hipStream_t stream) {
  const T* sp = reinterpret_cast<const T*>(src.data_ptr());
  T* dp = reinterpret_cast<T*>(dst.data_ptr());
  const int64_t* ixp = idx.data_ptr<int64_t>();
  dispatch_vec(vec, [&](auto v) {
    launch_rowcopy<T, v.value, SCATTER_ADD>(sp, ixp, dp, n, F, stream);
  });
}

void gather_rows_hip(torch::Tensor src, torch::Tensor idx, torch::Tensor out) {
  TORCH_CHECK(src.is_cuda() && idx.is_cuda() && out.is_cuda());
  const bool bf16 = src.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || src.scalar_type() == torch::kFloat);
  TORCH_CHECK(out.scalar_type() == src.scalar_type() &&
              idx.scalar_type() == torch::kLong);
  TORCH_CHECK(src.is_contiguous() && out.is_contiguous());
  const int64_t F = src.size(1);
  const int64_t n = idx.numel();
  TORCH_CHECK(out.size(0) == n && out.size(1) == F);
  auto stream = current_stream();
  const int vec = pick_vec(F, 0, bf16 ? 2 : 4);
  if (bf16)
    rowcopy_dispatch<__hip_bfloat16, false>(src, idx, out, n, F, vec, stream);
  else
    rowcopy_dispatch<float, false>(src, idx, out, n, F, vec, stream);
}

void scatter_add_rows_hip(torch::Tensor dst, torch::Tensor idx,
                          torch::Tensor src) {
  // Contract: idx entries are unique (one boundary peer at a time) — rows
  // are written by exactly one wave, so no atomics are needed.
  TORCH_CHECK(dst.is_cuda() && idx.is_cuda() && src.is_cuda());
  const bool bf16 = dst.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || dst.scalar_type() == torch::kFloat);
  TORCH_CHECK(src.scalar_type() == dst.scalar_type() &&
              idx.scalar_type() == torch::kLong);
  TORCH_CHECK(src.is_contiguous() && dst.is_contiguous());
  const int64_t F = dst.size(1);
  const int64_t n = idx.numel();
  TORCH_CHECK(src.size(0) == n && src.size(1) == F);
  auto stream = current_stream();
  const int vec = pick_vec(F, 0, bf16 ? 2 : 4);
  if (bf16)
    rowcopy_dispatch<__hip_bfloat16, true>(src, idx, dst, n, F, vec, stream);
  else
    rowcopy_dispatch<float, true>(src, idx, dst, n, F, vec, stream);
}

torch::Tensor colsum_hip(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kFloat);
  const int64_t M = x.size(0), F = x.size(1);
  // enough blocks to fill the chip; each handles a contiguous row stripe
  const int64_t nblk = std::min<int64_t>(2048, (M + 255) / 256);
  const int64_t rows_per_blk = (M + nblk - 1) / nblk;
  auto partials = torch::empty({nblk, F}, x.options());
  auto stream = current_stream();
  // widths 4, 2, 1 only: an 8-wide colsum is never picked
  dispatch_vec(F % 4 == 0 ? 4 : (F % 2 == 0 ? 2 : 1), [&](auto v) {
    if constexpr (v.value <= 4)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(colsum_partial_kernel<v.value>),
                         dim3(nblk), dim3(256), 0, stream,
                         x.data_ptr<float>(), partials.data_ptr<float>(), M,
                         F, rows_per_blk);
  });
  check_launch();
  return partials.sum(0);
}

void ema_update_hip(torch::Tensor avg, torch::Tensor x, double momentum) {
  TORCH_CHECK(avg.is_cuda() && x.is_cuda());
  TORCH_CHECK(avg.is_contiguous() && x.is_contiguous());
  TORCH_CHECK(avg.numel() == x.numel());
  const int64_t n = avg.numel();
  const int threads = 256;
  int64_t blocks = (n + 4 * threads - 1) / (4 * threads);
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL(ema_kernel, dim3(blocks), dim3(threads), 0,
                     current_stream(), avg.data_ptr<float>(),
                     x.data_ptr<float>(), static_cast<float>(momentum), n);
  check_launch();
}
