// Packed-row gather for the forward SpMM, bf16: spmm_packed.hip's idea (skip
// the zeros that dropout and ReLU put into the SpMM input) with a record, a
// value fetch and a placement designed for 2-byte values.
//
// pack_rows_bf16_kernel rewrites a dense bf16 [N, F] tensor as one
// fixed-stride record per row (layout: packed_layout(F, 2) in common.h,
// docs/DESIGN.md "Packed rows, bf16"):
//
//   header  W = ceil(F / 64) entries of 12 B: {uint32 mask_lo, uint32
//           mask_hi, uint32 prefix}. Bit b of the 64-bit mask of entry w is
//           set when column 64 w + b is non-zero (v != 0 on the bf16 value:
//           both zeros dropped, NaN and +-Inf kept); prefix is the number of
//           non-zero columns before column 64 w. 12 B per 64 columns is 9.4 %
//           of a dense bf16 row; the fp32 header (8 B per 32) would be 12.5 %.
//   values  the row's non-zero values, 2 bytes each, contiguous, in column
//           order, starting 16-byte aligned after the header; 3 words of
//           slack follow the F-th slot
//
// spmm_packed_bf16_kernel is spmm_csr_kernel<bf16, VEC, false> with the row
// gather replaced: same (row, chunk) decomposition, row_order, peel / 4-edge
// group / tail, fp32 accumulation expressions per column, acc * scale and one
// rounding to bf16, so the result is bitwise the dense kernel's at any lane
// width (a skipped column contributes 0.f where the dense kernel loaded a
// zero). The wave-uniform convention (scalar wave index, record bases and
// loop conditions, software-pipelined header loads) is spmm_packed.hip's.
//
// A lane owns VEC = 4 or 8 columns as VEC / 4 quads. Per quad and edge:
//   fetch  the quad's first value is slot `rank` of the record, at 2-byte
//          granularity. The lane loads the three 4-byte-aligned words from
//          word rank / 2 on (never a 2-byte-aligned multi-word load) and
//          funnel-shifts them by (rank & 1) * 16 into a 64-bit queue of four
//          bf16, head in the low bits.
//   place  column k, if its mask bit is set, takes the head as bits << 16 (an
//          fp32) and the queue moves down 16 bits: one variable 64-bit shift
//          per column, all in registers.
// The second quad of VEC = 8 starts at rank + popcount(first quad's bits): two
// 3-word loads instead of one 5-word window, which keeps every queue at 64
// bits and the slack at 3 words.

#include "../common.h"
#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

// This file's device code is built without the packed fp32 instructions
// (v_pk_add_f32 and kin): every function from here on carries the target
// attribute, in the device pass only. Functions of the HIP headers do not
// carry it and would stay calls, so the device code below uses the compiler
// builtins they wrap (popcount, ballot, bit_cast, the __bf16 conversion).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

// ---------------------------------------------------------------------------
// Pack: one wave per row, 64 columns (one header entry) per step.
// ---------------------------------------------------------------------------

__global__ void pack_rows_bf16_kernel(const uint16_t* __restrict__ x,
                                      uint32_t* __restrict__ packed,
                                      int64_t N, int64_t F,
                                      int64_t stride_words,
                                      int64_t hdr_words) {
  const int64_t wave_global =
      (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t nwaves =
      (static_cast<int64_t>(gridDim.x) * blockDim.x) / kWave;
  const uint64_t below = (1ull << lane) - 1ull;

  for (int64_t u = wave_global; u < N; u += nwaves) {
    const uint16_t* row = x + u * F;
    uint32_t* rec = packed + u * stride_words;
    uint16_t* vals = reinterpret_cast<uint16_t*>(rec + hdr_words);
    uint32_t base = 0;
    for (int64_t c0 = 0; c0 < F; c0 += kWave) {
      const int64_t c = c0 + lane;
      const uint16_t v = c < F ? row[c] : 0;
      const bool nz = (v & 0x7fffu) != 0;  // v != 0: -0.0 out, NaN and Inf in
      const uint64_t bal = __builtin_amdgcn_ballot_w64(nz);
      if (nz) vals[base + __builtin_popcountll(bal & below)] = v;
      if (lane == 0) {
        uint32_t* h = rec + 3 * (c0 >> 6);
        h[0] = static_cast<uint32_t>(bal);
        h[1] = static_cast<uint32_t>(bal >> 32);
        h[2] = base;
      }
      base += __builtin_popcountll(bal);
    }
  }
}

// ---------------------------------------------------------------------------
// Packed gather of the VEC consecutive columns f0 .. f0+VEC-1 of one record.
// f0 is a multiple of VEC and VEC divides 64, so they share one header entry.
// Columns at or past F have clear mask bits and so read as 0.f: a chunk that
// runs past the end of the row needs no guard here.
// ---------------------------------------------------------------------------

// byte address of record u: a 32 x 32 -> 64-bit product (u * stride exceeds
// 2^32 bytes at papers100M scale)
__device__ __forceinline__ const char* record(const uint32_t* packed,
                                              int32_t u,
                                              uint32_t stride_bytes) {
  return reinterpret_cast<const char*>(packed) +
         static_cast<uint64_t>(static_cast<uint32_t>(u)) * stride_bytes;
}

using u32x3 = uint32_t __attribute__((ext_vector_type(3)));

// what a lane keeps per pair
struct Lane {
  uint32_t hdr_off;   // byte offset of the header entry of column f0
  uint32_t below_lo;  // the entry's columns before f0, as mask bits
  uint32_t below_hi;
  uint32_t shift;     // f0 & 31: where f0 sits in its half of the mask
  bool upper;         // f0 & 32: which half that is
  uint32_t vals_off;  // byte offset of value slot 0
};

// where a lane's quads start in one record (byte offsets of their first
// value, 2-byte granular), and which of its columns are set
template <int VEC>
struct Slot {
  uint32_t off[VEC / 4];
  uint32_t m;
};

// the dependent half: one 12-byte header load, then the address arithmetic
__device__ __forceinline__ u32x3 load_header(const char* rec,
                                             uint32_t hdr_off) {
  u32x3 h;
  __builtin_memcpy(&h, rec + hdr_off, 12);
  return h;
}

// spmm_packed.hip's pinned(): keeps the widening of the header offset next to
// the loads, which then take scalar base + vector offset
__device__ __forceinline__ uint32_t pinned(uint32_t off) {
  asm volatile("" : "+v"(off));
  return off;
}

template <int VEC>
__device__ __forceinline__ Slot<VEC> locate(const Lane& l, u32x3 h) {
  Slot<VEC> s;
  const uint32_t rank = h.z + __builtin_popcount(h.x & l.below_lo) +
                        __builtin_popcount(h.y & l.below_hi);
  s.m = (l.upper ? h.y : h.x) >> l.shift;
  s.off[0] = l.vals_off + 2u * rank;
  if constexpr (VEC == 8)
    s.off[1] = s.off[0] + 2u * __builtin_popcount(s.m & 0xfu);
  return s;
}

// The three aligned words that cover a quad's four slots, loaded
// unconditionally. A quad whose bits are all clear reads the slots of the
// next non-zero column or the record's slack (3 words after the F-th slot:
// rank <= F, so the load ends at or before word F / 2 + 2); it uses none of
// what it read. The words live in vector values, never in an array indexed
// by slot, which would be put into scratch.
template <int VEC>
struct Vals {
  u32x3 w[VEC / 4];
};

template <int VEC>
__device__ __forceinline__ Vals<VEC> fetch(const char* rec,
                                           const Slot<VEC>& s) {
  Vals<VEC> v;
#pragma unroll
  for (int q = 0; q < VEC / 4; ++q)
    __builtin_memcpy(&v.w[q], rec + (s.off[q] & ~3u), 12);
  return v;
}

// all ones or all zeros from bit K of m; spelled as the instruction so the
// masks are not folded back into compares and selects (spmm_packed.hip)
template <int K>
__device__ __forceinline__ uint32_t column_mask(uint32_t m) {
  uint32_t on;
  asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(on) : "v"(m), "n"(K));
  return on;
}

// v[4 Q + k] = column 4 Q + k's value or 0.f, for the quad Q
template <int VEC, int Q, int K = 0>
__device__ __forceinline__ void place_from(uint32_t m, uint64_t q,
                                           float (&v)[VEC]) {
  if constexpr (K < 4) {
    const uint32_t on = column_mask<4 * Q + K>(m);
    v[4 * Q + K] = __builtin_bit_cast(
        float, (static_cast<uint32_t>(q) << 16) & on);
    place_from<VEC, Q, K + 1>(m, q >> (on & 16u), v);
  }
}

template <int VEC>
__device__ __forceinline__ void place(const Slot<VEC>& s, const Vals<VEC>& w,
                                      float (&v)[VEC]) {
#pragma unroll
  for (int q = 0; q < VEC / 4; ++q) {
    // (rank & 1) * 16 is off * 8 in the five bits the funnel shift reads
    const uint32_t sh = s.off[q] << 3;
    const uint32_t lo = __builtin_amdgcn_alignbit(w.w[q].y, w.w[q].x, sh);
    const uint32_t hi = __builtin_amdgcn_alignbit(w.w[q].z, w.w[q].y, sh);
    const uint64_t queue = (static_cast<uint64_t>(hi) << 32) | lo;
    if (q == 0)
      place_from<VEC, 0>(s.m, queue, v);
    else
      place_from<VEC, VEC / 4 - 1>(s.m, queue, v);
  }
}

// the sums are spmm_csr_kernel's, term for term: keep them so
template <int VEC>
__device__ __forceinline__ void add_edge(const char* rec, const Lane& l,
                                         float (&acc)[VEC]) {
  float v[VEC];
  const Slot<VEC> s = locate<VEC>(l, load_header(rec, l.hdr_off));
  place<VEC>(s, fetch<VEC>(rec, s), v);
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] += v[k];
}

template <int VEC>
__device__ __forceinline__ void add_group(
    const Slot<VEC>& s0, const Slot<VEC>& s1, const Slot<VEC>& s2,
    const Slot<VEC>& s3, const Vals<VEC>& w0, const Vals<VEC>& w1,
    const Vals<VEC>& w2, const Vals<VEC>& w3, float (&acc)[VEC]) {
  float v0[VEC], v1[VEC], v2[VEC], v3[VEC];
  place<VEC>(s0, w0, v0);
  place<VEC>(s1, w1, v1);
  place<VEC>(s2, w2, v2);
  place<VEC>(s3, w3, v3);
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] += v0[k] + v1[k] + v2[k] + v3[k];
}

// the dense kernel's store: one rounding of the fp32 product to bf16, the
// conversion __float2bfloat16 makes
__device__ __forceinline__ void store_bf16(uint16_t* p, float v,
                                           bool nontemporal) {
  const uint16_t u = __builtin_bit_cast(uint16_t, static_cast<__bf16>(v));
  if (nontemporal)
    __builtin_nontemporal_store(u, p);
  else
    *p = u;
}

// One wave per (row, chunk of 64 * VEC columns), grid-stride, the 4-edge
// groups software-pipelined as in spmm_packed_kernel: the next group's header
// loads (and the index load two groups ahead) are issued under the current
// group's value loads. The block is whole waves (the host asserts it).
template <int VEC>
__global__ void spmm_packed_bf16_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const uint32_t* __restrict__ packed, int64_t stride_words,
    int64_t hdr_words, const float* __restrict__ dst_scale,
    const int32_t* __restrict__ row_order, uint16_t* __restrict__ out,
    int64_t num_rows, int64_t F, int64_t nchunks) {
  static_assert(VEC == 4 || VEC == 8, "a lane owns one or two quads");
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
    const uint64_t below = (1ull << (static_cast<uint32_t>(f0) & 63u)) - 1ull;
    const Lane l{static_cast<uint32_t>(f0 >> 6) * 12u,
                 static_cast<uint32_t>(below),
                 static_cast<uint32_t>(below >> 32),
                 static_cast<uint32_t>(f0) & 31u,
                 (static_cast<uint32_t>(f0) & 32u) != 0,
                 static_cast<uint32_t>(hdr_words) * 4u};

    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;

    const int64_t e_begin = indptr[r];
    const int64_t e_end = indptr[r + 1];
    int64_t e = e_begin;

    // trip counts unsigned and compared for (in)equality or in 32 bits, as
    // the scalar unit compares. peel: the edges before the next multiple of
    // 4, or the whole row if it ends sooner.
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
      Slot<VEC> s0 = locate<VEC>(l, load_header(r0, l.hdr_off));
      Slot<VEC> s1 = locate<VEC>(l, load_header(r1, l.hdr_off));
      Slot<VEC> s2 = locate<VEC>(l, load_header(r2, l.hdr_off));
      Slot<VEC> s3 = locate<VEC>(l, load_header(r3, l.hdr_off));
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
        const u32x3 h0 = load_header(r0, ho);
        const u32x3 h1 = load_header(r1, ho);
        const u32x3 h2 = load_header(r2, ho);
        const u32x3 h3 = load_header(r3, ho);
        // keep the header loads above the wait for the values
        __builtin_amdgcn_sched_barrier(0);
        add_group<VEC>(s0, s1, s2, s3, w0, w1, w2, w3, acc);
        s0 = locate<VEC>(l, h0);
        s1 = locate<VEC>(l, h1);
        s2 = locate<VEC>(l, h2);
        s3 = locate<VEC>(l, h3);
        un = un2;
        e += 4;
      }
      const Vals<VEC> w0 = fetch<VEC>(r0, s0);
      const Vals<VEC> w1 = fetch<VEC>(r1, s1);
      const Vals<VEC> w2 = fetch<VEC>(r2, s2);
      const Vals<VEC> w3 = fetch<VEC>(r3, s3);
      add_group<VEC>(s0, s1, s2, s3, w0, w1, w2, w3, acc);
      e += 4;
    }
    const uint32_t tail = static_cast<uint32_t>(e_end - e) & 3u;
    for (uint32_t i = 0; i != tail; ++i, ++e)
      add_edge<VEC>(record(packed, indices[e], stride_bytes), l, acc);

    const float s = dst_scale ? dst_scale[r] : 1.f;
    if (f0 + VEC <= F) {
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        store_bf16(out + r * F + f0 + k, acc[k] * s, true);
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        if (f0 + k < F) store_bf16(out + r * F + f0 + k, acc[k] * s, false);
    }
  }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

void pack_rows_bf16_hip(torch::Tensor x, torch::Tensor packed) {
  TORCH_CHECK(x.is_cuda() && packed.is_cuda(), "pack_rows: device tensors");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && x.dim() == 2 &&
                  x.is_contiguous(),
              "pack_rows: contiguous bf16 [N, F]");
  const int64_t N = x.size(0), F = x.size(1);
  const PackedLayout l = packed_layout(F, 2);
  TORCH_CHECK(packed.scalar_type() == torch::kInt && packed.dim() == 2 &&
                  packed.is_contiguous() && packed.size(0) == N &&
                  packed.size(1) == l.stride_words,
              "pack_rows: packed must be int32 [N, stride_words]");
  const int threads = 256;  // 4 waves, one row each
  hipLaunchKernelGGL(pack_rows_bf16_kernel, dim3(grid_for(N, threads)),
                     dim3(threads), 0, current_stream(),
                     reinterpret_cast<const uint16_t*>(x.data_ptr()),
                     reinterpret_cast<uint32_t*>(packed.data_ptr<int32_t>()),
                     N, F, l.stride_words, l.hdr_words);
  check_launch();
}

void spmm_packed_bf16_hip(torch::Tensor indptr, torch::Tensor indices,
                          torch::Tensor packed, int64_t F,
                          torch::Tensor dst_scale, torch::Tensor row_order,
                          torch::Tensor out, int64_t vec) {
  TORCH_CHECK(packed.is_cuda() && out.is_cuda(),
              "spmm_packed: device tensors");
  const PackedLayout l = packed_layout(F, 2);
  TORCH_CHECK(packed.scalar_type() == torch::kInt && packed.dim() == 2 &&
                  packed.is_contiguous() && packed.size(1) == l.stride_words,
              "spmm_packed: packed must be int32 [N, stride_words] of "
              "pack_rows for this F and bf16");
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16 && out.is_contiguous() &&
                  out.dim() == 2 && out.size(1) == F,
              "spmm_packed: out must be contiguous bf16 [num_rows, F]");
  TORCH_CHECK(indptr.scalar_type() == torch::kLong &&
                  indices.scalar_type() == torch::kInt,
              "spmm_packed: indptr int64, indices int32");
  TORCH_CHECK(vec == 0 || vec == 4 || vec == 8,
              "spmm_packed: the bf16 lane width is 4 or 8 (0: by F)");
  const int64_t num_rows = out.size(0);
  TORCH_CHECK(indptr.numel() == num_rows + 1,
              "spmm_packed: indptr must have num_rows + 1 entries");
  const float* dsp = nullptr;
  if (dst_scale.defined() && dst_scale.numel() > 0) {
    TORCH_CHECK(dst_scale.is_contiguous() && dst_scale.numel() == num_rows &&
                    dst_scale.scalar_type() == torch::kFloat,
                "spmm_packed: dst_scale must be contiguous fp32 [num_rows]");
    dsp = dst_scale.data_ptr<float>();
  }
  const int32_t* rop = nullptr;
  if (row_order.defined() && row_order.numel() > 0) {
    TORCH_CHECK(row_order.is_contiguous() && row_order.numel() == num_rows &&
                    row_order.scalar_type() == torch::kInt,
                "spmm_packed: row_order must be contiguous int32 [num_rows]");
    rop = row_order.data_ptr<int32_t>();
  }
  auto stream = current_stream();
  const int64_t* ip = indptr.data_ptr<int64_t>();
  const int32_t* xp = indices.data_ptr<int32_t>();
  const uint32_t* pp =
      reinterpret_cast<const uint32_t*>(packed.data_ptr<int32_t>());
  uint16_t* op = reinterpret_cast<uint16_t*>(out.data_ptr());
  // lane width: 4 at every F. The gather is bound by its vector instructions,
  // whose count goes with the column slots visited, not with the (row, chunk)
  // visits: F = 602 is 3 chunks of 256 at 4 and 2 chunks of 512 at 8, and 4
  // measured 18.3 against 20.3 ms at a quarter non-zero; at F = 256 (one
  // chunk either way, half the lanes idle at 8) 6.9 against 10.3 ms
  // (profiles/README.md, "Packed-row forward SpMM, bf16").
  if (vec == 0) vec = 4;
  dispatch_vec(static_cast<int>(vec), [&](auto v) {
    constexpr int VEC = v.value;
    if constexpr (VEC == 4 || VEC == 8) {
      const int64_t nchunks = (F + kWave * VEC - 1) / (kWave * VEC);
      constexpr int threads = 256;  // 4 whole waves: the kernel keeps the
      static_assert(threads % kWave == 0);  // wave index in a scalar register
      hipLaunchKernelGGL(HIP_KERNEL_NAME(spmm_packed_bf16_kernel<VEC>),
                         dim3(grid_for(num_rows * nchunks, threads)),
                         dim3(threads), 0, stream, ip, xp, pp, l.stride_words,
                         l.hdr_words, dsp, rop, op, num_rows, F, nchunks);
    }
  });
  check_launch();
}
