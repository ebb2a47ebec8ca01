// Packed-row gather for the forward SpMM (fp32): skip the zeros that dropout
// and ReLU put into the SpMM input one kernel earlier.
//
// pack_rows_kernel rewrites a dense [N, F] tensor as one fixed-stride record
// per row (layout: PackedLayout in common.h, docs/DESIGN.md "Packed rows"):
//
//   header  W = ceil(F / 32) entries of 8 B: {uint32 mask, uint32 prefix}
//           mask bit b of entry w is set when column 32 w + b is non-zero
//           (v != 0.f: both zeros dropped, NaN and +-Inf kept); prefix is the
//           number of non-zero columns before column 32 w
//   values  the row's non-zero values, contiguous, in column order, starting
//           16-byte aligned after the header
//
// Row u starts at u * stride (a multiple of 128 B, so no offsets array); only
// the header and the leading nnz_u value slots are meaningful, which is where
// the byte saving comes from.
//
// spmm_packed_kernel is spmm_csr_kernel<float, VEC, false> with the row
// gather replaced: same (row, chunk) decomposition, row_order, peel / 4-edge
// group / tail and the same accumulation expressions per column, so the
// result is bitwise the dense kernel's at any lane width (a skipped column
// contributes 0.f where the dense kernel loaded a zero; docs/DESIGN.md has
// the argument).

#include "../common.h"
#include "hip_util.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int kWave = 64;

using int32x4 = __attribute__((ext_vector_type(4))) int;

// ---------------------------------------------------------------------------
// Pack: one wave per row, 64 columns (two header entries) per step.
// ---------------------------------------------------------------------------

__global__ void pack_rows_kernel(const float* __restrict__ x,
                                 uint32_t* __restrict__ packed, int64_t N,
                                 int64_t F, int64_t stride_words,
                                 int64_t hdr_words) {
  const int64_t wave_global =
      (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t nwaves =
      (static_cast<int64_t>(gridDim.x) * blockDim.x) / kWave;
  const uint64_t below = (1ull << lane) - 1ull;

  for (int64_t u = wave_global; u < N; u += nwaves) {
    const float* row = x + u * F;
    uint32_t* rec = packed + u * stride_words;
    float* vals = reinterpret_cast<float*>(rec + hdr_words);
    uint32_t base = 0;
    for (int64_t c0 = 0; c0 < F; c0 += kWave) {
      const int64_t c = c0 + lane;
      const float v = c < F ? row[c] : 0.f;
      const bool nz = v != 0.f;
      const uint64_t bal = __ballot(nz);
      if (nz) vals[base + __popcll(bal & below)] = v;
      const uint32_t lo = static_cast<uint32_t>(bal);
      const int64_t w = c0 >> 5;
      if (lane == 0) {
        rec[2 * w] = lo;
        rec[2 * w + 1] = base;
      }
      if (lane == 32 && c0 + 32 < F) {
        rec[2 * w + 2] = static_cast<uint32_t>(bal >> 32);
        rec[2 * w + 3] = base + __popc(lo);
      }
      base += __popcll(bal);
    }
  }
}

// ---------------------------------------------------------------------------
// Packed gather of the VEC consecutive columns f0 .. f0+VEC-1 of one record.
// f0 is a multiple of VEC and VEC divides 32, so they share one header entry.
// Columns at or past F have clear mask bits and so read as 0.f: a chunk that
// runs past the end of the row needs no guard here.
// ---------------------------------------------------------------------------

struct PackedRef {
  const uint32_t* base;  // all records
  int64_t stride_words;
  int64_t hdr_words;
};

// where a lane's values sit in one record, and which of its columns are set
struct Slot {
  const float* src;
  uint32_t m;
};

// the dependent half: one 8-byte header load, then the address arithmetic
__device__ __forceinline__ uint2 load_header(const PackedRef& p, int64_t u,
                                             int64_t f0) {
  return *reinterpret_cast<const uint2*>(p.base + u * p.stride_words +
                                         2 * (f0 >> 5));
}

__device__ __forceinline__ Slot locate(const PackedRef& p, int64_t u,
                                       int64_t f0, uint2 h) {
  const uint32_t bit = static_cast<uint32_t>(f0) & 31u;
  const uint32_t rank = h.y + __popc(h.x & ((1u << bit) - 1u));
  return {reinterpret_cast<const float*>(p.base + u * p.stride_words +
                                         p.hdr_words) + rank,
          h.x >> bit};
}

__device__ __forceinline__ Slot locate(const PackedRef& p, int64_t u,
                                       int64_t f0) {
  return locate(p, u, f0, load_header(p, u, f0));
}

// ONE VEC-wide value load at the rank of the first owned column, issued
// unconditionally: the columns a lane owns that are non-zero sit in
// consecutive slots from there. A lane whose bits are all clear reads the
// slots of the next non-zero column, which its neighbours fetch anyway, or
// the row's slack past the last value (PackedLayout keeps 32 B of it); it
// uses none of what it read. The loaded slots live in a vector value, never
// in an array: indexed by slot, an array would be put into scratch.
template <int VEC>
using Vals = float __attribute__((ext_vector_type(VEC)));

template <int VEC>
__device__ __forceinline__ Vals<VEC> fetch(const Slot& s) {
  Vals<VEC> w;
  // 4-byte aligned only: the target reads unaligned multi-dword loads
  __builtin_memcpy(&w, s.src, sizeof(float) * VEC);
  return w;
}

// v[k] = column k's value or 0.f; a set column's slot is the number of set
// bits below it
template <int VEC>
__device__ __forceinline__ void place(uint32_t m, const Vals<VEC>& w,
                                      float (&v)[VEC]) {
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const uint32_t slot = __popc(m & ((1u << k) - 1u));
    float pick = w[0];
#pragma unroll
    for (int j = 1; j <= k; ++j) pick = slot == j ? w[j] : pick;
    v[k] = ((m >> k) & 1u) ? pick : 0.f;
  }
}

// the sums are spmm_csr_kernel's, term for term: keep them so
template <int VEC>
__device__ __forceinline__ void add_edge(const PackedRef& p, int64_t u,
                                         int64_t f0, float (&acc)[VEC]) {
  float v[VEC];
  const Slot s = locate(p, u, f0);
  place<VEC>(s.m, fetch<VEC>(s), v);
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] += v[k];
}

template <int VEC>
__device__ __forceinline__ void add_group(
    uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3, const Vals<VEC>& w0,
    const Vals<VEC>& w1, const Vals<VEC>& w2, const Vals<VEC>& w3,
    float (&acc)[VEC]) {
  float v0[VEC], v1[VEC], v2[VEC], v3[VEC];
  place<VEC>(m0, w0, v0);
  place<VEC>(m1, w1, v1);
  place<VEC>(m2, w2, v2);
  place<VEC>(m3, w3, v3);
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] += v0[k] + v1[k] + v2[k] + v3[k];
}

// One wave per (row, chunk of 64 * VEC columns), grid-stride, as the dense
// kernel. The 4-edge groups are software-pipelined: the next group's header
// loads (and the index load two groups ahead) are issued under the current
// group's value loads, so a group exposes one memory latency instead of three
// (8.7 against 11.3 ms at F=256, a quarter non-zero; profiles/README.md).
template <int VEC>
__global__ void spmm_packed_kernel(const int64_t* __restrict__ indptr,
                                   const int32_t* __restrict__ indices,
                                   const uint32_t* __restrict__ packed,
                                   int64_t stride_words, int64_t hdr_words,
                                   const float* __restrict__ dst_scale,
                                   const int32_t* __restrict__ row_order,
                                   float* __restrict__ out, int64_t num_rows,
                                   int64_t F, int64_t nchunks) {
  const int64_t wave_global =
      (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t nwaves =
      (static_cast<int64_t>(gridDim.x) * blockDim.x) / kWave;
  const int64_t npairs = num_rows * nchunks;
  const PackedRef p{packed, stride_words, hdr_words};

  for (int64_t pair = wave_global; pair < npairs; pair += nwaves) {
    int64_t r = pair / nchunks;
    const int64_t chunk = pair % nchunks;
    if (row_order) r = row_order[r];
    const int64_t f0 = chunk * (kWave * VEC) + lane * VEC;
    if (f0 >= F) continue;

    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;

    const int64_t e_begin = indptr[r];
    const int64_t e_end = indptr[r + 1];
    int64_t e = e_begin;

    for (; e < e_end && (e & 3); ++e) add_edge<VEC>(p, indices[e], f0, acc);
    if (e + 4 <= e_end) {
      const int32x4 uu = __builtin_nontemporal_load(
          reinterpret_cast<const int32x4*>(indices + e));
      Slot s0 = locate(p, uu[0], f0);
      Slot s1 = locate(p, uu[1], f0);
      Slot s2 = locate(p, uu[2], f0);
      Slot s3 = locate(p, uu[3], f0);
      // indices of the group after this one (this one again if it is the
      // last: the address stays inside the row)
      int32x4 un = __builtin_nontemporal_load(reinterpret_cast<const int32x4*>(
          indices + (e + 8 <= e_end ? e + 4 : e)));
      while (e + 8 <= e_end) {
        const int32x4 un2 =
            __builtin_nontemporal_load(reinterpret_cast<const int32x4*>(
                indices + (e + 12 <= e_end ? e + 8 : e)));
        const Vals<VEC> w0 = fetch<VEC>(s0);
        const Vals<VEC> w1 = fetch<VEC>(s1);
        const Vals<VEC> w2 = fetch<VEC>(s2);
        const Vals<VEC> w3 = fetch<VEC>(s3);
        const uint2 h0 = load_header(p, un[0], f0);
        const uint2 h1 = load_header(p, un[1], f0);
        const uint2 h2 = load_header(p, un[2], f0);
        const uint2 h3 = load_header(p, un[3], f0);
        // keep the header loads above the wait for the values
        __builtin_amdgcn_sched_barrier(0);
        add_group<VEC>(s0.m, s1.m, s2.m, s3.m, w0, w1, w2, w3, acc);
        s0 = locate(p, un[0], f0, h0);
        s1 = locate(p, un[1], f0, h1);
        s2 = locate(p, un[2], f0, h2);
        s3 = locate(p, un[3], f0, h3);
        un = un2;
        e += 4;
      }
      const Vals<VEC> w0 = fetch<VEC>(s0);
      const Vals<VEC> w1 = fetch<VEC>(s1);
      const Vals<VEC> w2 = fetch<VEC>(s2);
      const Vals<VEC> w3 = fetch<VEC>(s3);
      add_group<VEC>(s0.m, s1.m, s2.m, s3.m, w0, w1, w2, w3, acc);
      e += 4;
    }
    for (; e < e_end; ++e) add_edge<VEC>(p, indices[e], f0, acc);

    const float s = dst_scale ? dst_scale[r] : 1.f;
    if (f0 + VEC <= F) {
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        __builtin_nontemporal_store(acc[k] * s, out + r * F + f0 + k);
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        if (f0 + k < F) out[r * F + f0 + k] = acc[k] * s;
    }
  }
}

}  // namespace

PackedLayout packed_layout(int64_t F) {
  PackedLayout l;
  l.mask_words = (F + 31) / 32;
  // header padded so the values start 16-byte aligned
  l.hdr_words = (2 * l.mask_words + 3) / 4 * 4;
  // 8 slack words: the widest value load may start at slot nnz <= F
  l.stride_words = (l.hdr_words + F + 8 + 31) / 32 * 32;
  return l;
}

void pack_rows_hip(torch::Tensor x, torch::Tensor packed) {
  TORCH_CHECK(x.is_cuda() && packed.is_cuda(), "pack_rows: device tensors");
  TORCH_CHECK(x.scalar_type() == torch::kFloat && x.dim() == 2 &&
                  x.is_contiguous(),
              "pack_rows: contiguous fp32 [N, F]");
  const int64_t N = x.size(0), F = x.size(1);
  const PackedLayout l = packed_layout(F);
  TORCH_CHECK(packed.scalar_type() == torch::kInt && packed.dim() == 2 &&
                  packed.is_contiguous() && packed.size(0) == N &&
                  packed.size(1) == l.stride_words,
              "pack_rows: packed must be int32 [N, stride_words]");
  const int threads = 256;  // 4 waves, one row each
  int64_t blocks = (N * kWave + threads - 1) / threads;
  blocks = std::min<int64_t>(blocks, 8 * 65536);
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL(pack_rows_kernel, dim3(blocks), dim3(threads), 0,
                     current_stream(), x.data_ptr<float>(),
                     reinterpret_cast<uint32_t*>(packed.data_ptr<int32_t>()),
                     N, F, l.stride_words, l.hdr_words);
  check_launch();
}

void spmm_packed_hip(torch::Tensor indptr, torch::Tensor indices,
                     torch::Tensor packed, int64_t F, torch::Tensor dst_scale,
                     torch::Tensor row_order, torch::Tensor out) {
  TORCH_CHECK(packed.is_cuda() && out.is_cuda(),
              "spmm_packed: device tensors");
  const PackedLayout l = packed_layout(F);
  TORCH_CHECK(packed.scalar_type() == torch::kInt && packed.dim() == 2 &&
                  packed.is_contiguous() && packed.size(1) == l.stride_words,
              "spmm_packed: packed must be int32 [N, stride_words] of "
              "pack_rows for this F");
  TORCH_CHECK(out.scalar_type() == torch::kFloat && out.is_contiguous() &&
              out.dim() == 2 && out.size(1) == F);
  TORCH_CHECK(indptr.scalar_type() == torch::kLong &&
              indices.scalar_type() == torch::kInt);
  const int64_t num_rows = out.size(0);
  TORCH_CHECK(indptr.numel() == num_rows + 1);
  const float* dsp = nullptr;
  if (dst_scale.defined() && dst_scale.numel() > 0) {
    TORCH_CHECK(dst_scale.is_contiguous() && dst_scale.numel() == num_rows);
    TORCH_CHECK(dst_scale.scalar_type() == torch::kFloat);
    dsp = dst_scale.data_ptr<float>();
  }
  const int32_t* rop = nullptr;
  if (row_order.defined() && row_order.numel() > 0) {
    TORCH_CHECK(row_order.is_contiguous() && row_order.numel() == num_rows &&
                row_order.scalar_type() == torch::kInt);
    rop = row_order.data_ptr<int32_t>();
  }
  auto stream = current_stream();
  const int64_t* ip = indptr.data_ptr<int64_t>();
  const int32_t* xp = indices.data_ptr<int32_t>();
  const uint32_t* pp =
      reinterpret_cast<const uint32_t*>(packed.data_ptr<int32_t>());
  float* op = out.data_ptr<float>();
  // lane width: the narrowest that covers the row in one chunk, at most 4.
  // Unlike the dense kernel's, it need not divide F (values are read
  // unaligned, and columns past F read as zero), and wider is faster here:
  // the gather is bound by (row, chunk) visits, not bytes. At F=256, a
  // quarter non-zero: 4 -> 8.7 ms, 2 -> 16.0 ms, dense 15.4 ms; 8 loses to
  // its own selects (18.7 ms) (profiles/README.md).
  const int vec = F > 128 ? 4 : (F > 64 ? 2 : 1);
  dispatch_vec(vec, [&](auto v) {
    constexpr int VEC = v.value;
    if constexpr (VEC <= 4) {
      const int64_t nchunks = (F + kWave * VEC - 1) / (kWave * VEC);
      const int threads = 256;  // 4 waves
      const int64_t npairs = num_rows * nchunks;
      int64_t blocks = (npairs * kWave + threads - 1) / threads;
      blocks = std::min<int64_t>(blocks, 8 * 65536);
      if (blocks == 0) blocks = 1;
      hipLaunchKernelGGL(HIP_KERNEL_NAME(spmm_packed_kernel<VEC>),
                         dim3(blocks), dim3(threads), 0, stream, ip, xp, pp,
                         l.stride_words, l.hdr_words, dsp, rop, op, num_rows,
                         F, nchunks);
    }
  });
  check_launch();
}
