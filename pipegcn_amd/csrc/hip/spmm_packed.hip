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
// the argument). What differs from the dense kernel besides the gather: the
// values a wave shares (row, edge cursor, node ids, record bases) are held in
// scalar registers and the loaded slots are placed with bit-selects, since
// the parent of this form was bound by its vector instructions, 98 % VALU
// busy (profiles/README.md, "Packed gather: wave-uniform index path").

#include "../common.h"
#include "hip_util.h"

#include <hip/hip_runtime.h>

namespace {

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

// Wave-uniform convention: a wave owns one (row, chunk), so the row, its edge
// range, the edge cursor, the node ids and every record's base address are
// the same in all 64 lanes. They are kept in scalar registers (the wave index
// goes through readfirstlane, from which the compiler derives the rest), the
// loops branch on scalar conditions, and a lane adds only its own part: a
// 32-bit byte offset into the record, so the loads take the scalar-base plus
// vector-offset form.

// byte address of record u: a 32 x 32 -> 64-bit product (u * stride exceeds
// 2^32 bytes at papers100M scale)
__device__ __forceinline__ const char* record(const uint32_t* packed,
                                              int32_t u,
                                              uint32_t stride_bytes) {
  return reinterpret_cast<const char*>(packed) +
         static_cast<uint64_t>(static_cast<uint32_t>(u)) * stride_bytes;
}

// what a lane keeps per pair: where its header entry sits in any record,
// which bit of it is its first column, and where the values start
struct Lane {
  uint32_t hdr_off;   // byte offset of the header entry of column f0
  uint32_t bit;       // f0 & 31
  uint32_t vals_off;  // byte offset of value slot 0
};

// where a lane's values sit in one record (byte offset), and which of its
// columns are set
struct Slot {
  uint32_t off;
  uint32_t m;
};

// the dependent half: one 8-byte header load, then the address arithmetic
__device__ __forceinline__ uint2 load_header(const char* rec,
                                             uint32_t hdr_off) {
  return *reinterpret_cast<const uint2*>(rec + hdr_off);
}

// The header offset is the same for every record. Hoisted out of a loop, its
// widening to 64 bits turns every header load into a 64-bit vector add plus a
// load from a vector address; passed through this once per iteration, the
// widening stays next to the loads, which then take scalar base + offset.
__device__ __forceinline__ uint32_t pinned(uint32_t off) {
  asm volatile("" : "+v"(off));
  return off;
}

__device__ __forceinline__ Slot locate(const Lane& l, uint2 h) {
  const uint32_t rank = h.y + __popc(h.x & ((1u << l.bit) - 1u));
  return {l.vals_off + 4u * rank, h.x >> l.bit};
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
__device__ __forceinline__ Vals<VEC> fetch(const char* rec, const Slot& s) {
  Vals<VEC> w;
  // 4-byte aligned only: the target reads unaligned multi-dword loads
  __builtin_memcpy(&w, rec + s.off, sizeof(float) * VEC);
  return w;
}

// v[k] = column k's value or 0.f. The loaded slots are a queue: column k, if
// set, takes its head and the queue moves up one. Moves are on the bit
// patterns, under an all-ones / all-zeros word per column: one bit-field
// extract, then one bit-select per move, 14 vector instructions per edge at
// VEC = 4 where compares and selects on the slot number took 27. The extract
// is spelled as the instruction: written in C++ the compiler turns the masks
// back into compares and selects (profiles/README.md).
//
// This and pinned() above steer the instruction selection of one compiler.
// To re-check after a toolchain change, compile this file with -O3
// --offload-arch=gfx950 --offload-device-only -S and count the v_*
// instructions of the innermost loop of spmm_packed_kernel<4> (the basic
// block with four global_load_dwordx4 and four global_load_dwordx2): 83,
// among them 16 v_bfe_i32 and 24 bit-selects (v_bfi_b32 or v_bitop3_b32),
// the loads in the form "v, v_off, s[base:base+1]", no v_cmp and no
// v_lshl_add_u64. 134 means the
// masks were folded into selects again, 89 that the header loads went back
// to vector addresses; <2> and <1> count 42 and 30.
template <int K>
__device__ __forceinline__ uint32_t column_mask(uint32_t m) {
  uint32_t on;
  asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(on) : "v"(m), "n"(K));
  return on;
}

template <int VEC, int K = 0>
__device__ __forceinline__ void place_from(uint32_t m, uint32_t (&q)[VEC],
                                           float (&v)[VEC]) {
  if constexpr (K < VEC) {
    const uint32_t on = column_mask<K>(m);
    v[K] = __uint_as_float(q[0] & on);
#pragma unroll
    for (int j = 0; j + 1 < VEC - K; ++j)
      q[j] = (q[j + 1] & on) | (q[j] & ~on);
    place_from<VEC, K + 1>(m, q, v);
  }
}

template <int VEC>
__device__ __forceinline__ void place(uint32_t m, const Vals<VEC>& w,
                                      float (&v)[VEC]) {
  uint32_t q[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) q[j] = __float_as_uint(w[j]);
  place_from<VEC>(m, q, v);
}

// the sums are spmm_csr_kernel's, term for term: keep them so
template <int VEC>
__device__ __forceinline__ void add_edge(const char* rec, const Lane& l,
                                         float (&acc)[VEC]) {
  float v[VEC];
  const Slot s = locate(l, load_header(rec, l.hdr_off));
  place<VEC>(s.m, fetch<VEC>(rec, s), v);
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
// (8.7 against 11.3 ms at F=256, a quarter non-zero, before the index path
// went scalar; profiles/README.md).
// The block is whole waves (the host asserts it), so the wave index is
// uniform; see the convention above for what follows from that.
template <int VEC>
__global__ void spmm_packed_kernel(const int64_t* __restrict__ indptr,
                                   const int32_t* __restrict__ indices,
                                   const uint32_t* __restrict__ packed,
                                   int64_t stride_words, int64_t hdr_words,
                                   const float* __restrict__ dst_scale,
                                   const int32_t* __restrict__ row_order,
                                   float* __restrict__ out, int64_t num_rows,
                                   int64_t F, int64_t nchunks) {
  const int wave_in_block =
      __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) / kWave);
  const int64_t waves_per_block = blockDim.x / kWave;
  const int64_t wave_global =
      static_cast<int64_t>(blockIdx.x) * waves_per_block + wave_in_block;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * waves_per_block;
  const int64_t npairs = num_rows * nchunks;
  const uint32_t stride_bytes = static_cast<uint32_t>(stride_words) * 4u;

  for (int64_t pair = wave_global; pair < npairs; pair += nwaves) {
    int64_t r = pair / nchunks;
    const int64_t chunk = pair % nchunks;
    if (row_order) r = row_order[r];
    const int64_t f0 = chunk * (kWave * VEC) + lane * VEC;
    // lane 0 always passes: the uniform values below come from live lanes
    if (f0 >= F) continue;
    const Lane l{static_cast<uint32_t>(f0 >> 5) * 8u,
                 static_cast<uint32_t>(f0) & 31u,
                 static_cast<uint32_t>(hdr_words) * 4u};

    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;

    const int64_t e_begin = indptr[r];
    const int64_t e_end = indptr[r + 1];
    int64_t e = e_begin;

    // The trip counts are unsigned and only tested for (in)equality or in 32
    // bits: that is what the scalar unit compares (a 64-bit "less than" would
    // go to the vector unit). peel: the edges before the next multiple of 4,
    // or the whole row if it ends sooner.
    const uint64_t deg = static_cast<uint64_t>(e_end - e_begin);
    uint32_t peel = static_cast<uint32_t>(-e_begin) & 3u;
    if ((deg >> 2) == 0 && static_cast<uint32_t>(deg) < peel)
      peel = static_cast<uint32_t>(deg);
    for (uint32_t i = 0; i != peel; ++i, ++e)
      add_edge<VEC>(record(packed, indices[e], stride_bytes), l, acc);
    // whole groups left, this one included
    uint64_t g = static_cast<uint64_t>(e_end - e) >> 2;
    if (g != 0) {
      const int32x4 uu = *reinterpret_cast<const int32x4*>(indices + e);
      const char* r0 = record(packed, uu[0], stride_bytes);
      const char* r1 = record(packed, uu[1], stride_bytes);
      const char* r2 = record(packed, uu[2], stride_bytes);
      const char* r3 = record(packed, uu[3], stride_bytes);
      Slot s0 = locate(l, load_header(r0, l.hdr_off));
      Slot s1 = locate(l, load_header(r1, l.hdr_off));
      Slot s2 = locate(l, load_header(r2, l.hdr_off));
      Slot s3 = locate(l, load_header(r3, l.hdr_off));
      // indices of the group after this one (this one again if it is the
      // last: the address stays inside the row)
      int32x4 un = *reinterpret_cast<const int32x4*>(
          indices + (g != 1 ? e + 4 : e));
      for (; g != 1; --g) {
        const int32x4 un2 = *reinterpret_cast<const int32x4*>(
            indices + (g != 2 ? e + 8 : e));
        const Vals<VEC> w0 = fetch<VEC>(r0, s0);
        const Vals<VEC> w1 = fetch<VEC>(r1, s1);
        const Vals<VEC> w2 = fetch<VEC>(r2, s2);
        const Vals<VEC> w3 = fetch<VEC>(r3, s3);
        r0 = record(packed, un[0], stride_bytes);
        r1 = record(packed, un[1], stride_bytes);
        r2 = record(packed, un[2], stride_bytes);
        r3 = record(packed, un[3], stride_bytes);
        const uint32_t ho = pinned(l.hdr_off);
        const uint2 h0 = load_header(r0, ho);
        const uint2 h1 = load_header(r1, ho);
        const uint2 h2 = load_header(r2, ho);
        const uint2 h3 = load_header(r3, ho);
        // keep the header loads above the wait for the values
        __builtin_amdgcn_sched_barrier(0);
        add_group<VEC>(s0.m, s1.m, s2.m, s3.m, w0, w1, w2, w3, acc);
        s0 = locate(l, h0);
        s1 = locate(l, h1);
        s2 = locate(l, h2);
        s3 = locate(l, h3);
        un = un2;
        e += 4;
      }
      const Vals<VEC> w0 = fetch<VEC>(r0, s0);
      const Vals<VEC> w1 = fetch<VEC>(r1, s1);
      const Vals<VEC> w2 = fetch<VEC>(r2, s2);
      const Vals<VEC> w3 = fetch<VEC>(r3, s3);
      add_group<VEC>(s0.m, s1.m, s2.m, s3.m, w0, w1, w2, w3, acc);
      e += 4;
    }
    const uint32_t tail = static_cast<uint32_t>(e_end - e) & 3u;
    for (uint32_t i = 0; i != tail; ++i, ++e)
      add_edge<VEC>(record(packed, indices[e], stride_bytes), l, acc);

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
  hipLaunchKernelGGL(pack_rows_kernel, dim3(grid_for(N, threads)),
                     dim3(threads), 0,
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
  // the cost is per (row, chunk) visit of a wave, not per byte. At F=256, a
  // quarter non-zero, with the index math still per lane: 4 -> 8.7 ms, 2 ->
  // 16.0 ms, dense 15.4 ms, 8 lost to its own selects (18.7 ms); 4 is at
  // 6.7 ms now (profiles/README.md).
  const int vec = F > 128 ? 4 : (F > 64 ? 2 : 1);
  dispatch_vec(vec, [&](auto v) {
    constexpr int VEC = v.value;
    if constexpr (VEC <= 4) {
      const int64_t nchunks = (F + kWave * VEC - 1) / (kWave * VEC);
      constexpr int threads = 256;  // 4 whole waves: the kernel keeps the
      static_assert(threads % kWave == 0);  // wave index in a scalar register
      hipLaunchKernelGGL(HIP_KERNEL_NAME(spmm_packed_kernel<VEC>),
                         dim3(grid_for(num_rows * nchunks, threads)),
                         dim3(threads), 0, stream, ip, xp, pp, l.stride_words,
                         l.hdr_words, dsp, rop, op, num_rows, F, nchunks);
    }
  });
  check_launch();
}
