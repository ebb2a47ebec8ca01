// GAT edge-softmax aggregation for gfx950: attention weights are never stored.
//
//   s_uv     = el[u,h] + er[v,h]
//   alpha_uv = exp(leaky_relu(s_uv) - lse[v,h])    (lse >= row max: no
//                                                   overflow)
//   c_uv     = alpha_uv * leaky_relu'(s_uv)
//
// Every kernel recomputes alpha from PER-NODE state (el, er, lse), so nothing
// of size nnz exists in forward or backward, and the transpose pass walks the
// prebuilt CSC without an edge-id permutation or atomics (docs/DESIGN.md).
//
//  - gat_row_stats     : lse[v,h], one wave per destination row
//  - gat_aggregate_fwd : out[v] = sum_u alpha*z[u]  (+ zc = sum_u c*z[u] and
//                        csum = sum_u c when gradients are needed)
//  - gat_aggregate_bwd : over the CSC: dz[u] = sum_v alpha*g[v] and
//                        d_el[u,h] = z[u,h,:].(sum_v c*g[v,h,:])
//                                    - sum_v c*t[v,h]
//
// Attention dropout (p > 0) is applied AFTER the softmax, so alpha, c and lse
// are unchanged and gat_row_stats is untouched. With w_uvh = keep(key, u, v,
// h) / (1 - p), a bit recomputed per edge and head from a 32-bit hash of the
// ENDPOINTS (the CSR and CSC passes see an edge at different positions):
//
//   out[v]    = sum_u w*alpha*z[u]        dz[u] = sum_v w*alpha*g[v]
//   zc[v]     = sum_u w*c*z[u]            gc    = sum_v w*c*g[v]
//   t[v,h]    = <g[v,h], out[v,h]>        (the dropped out)
//   csum[v,h] = sum_u c  and  sum_v c*t[v,h]  use the UNMASKED c
//
// i.e. the masked weight goes into every accumulator that multiplies a
// gathered row, the unmasked c into the two scalar sums: with
// dL/ds_uv = c_uv * (w_uv * <g[v], z[u]> - t[v]) both d_er = <g, zc> - t*csum
// and d_el keep their form. Duplicate (u, v) edges share one bit per head.
//
// The two aggregate kernels keep spmm_csr_kernel's scheduling shape (one wave
// per (row, feature chunk), LPT row order, aligned dwordx4 index load, four
// gathers in flight). A lane's VEC elements always belong to ONE head (VEC
// divides D), so its edge weight is one scalar. Each row's edges are walked
// in CSR order by one wave: results are bitwise reproducible and independent
// of row_order.
//
// Both aggregate kernels spell the edge walk out (one_edge plus the 4-way
// body) where gatv2.hip passes one generic lambda to for_edges. Ported to
// that form the forward spills in two instances and the backward's two
// 1-element dropout instances fuse other products of the 4-edge sums into
// FMAs, a last-bit change of dz and d_el (profiles/README.md, "Shared
// attention scaffolding"). Keep one_edge and the unrolled body in step: same
// weights, csum / ct from the unmasked c, masking after that.

#include "../common.h"
#include "attn_util.h"
#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

// ld_vec / st_vec, leaky, the drop_* hash, wave_sum, wave_ids and the
// host-side input checks are shared with gatv2.hip
using namespace attn_util;

// heads handled per sweep over a row's edges in gat_row_stats
constexpr int kHeadBlk = 4;
// finite stand-in for -inf: (kNegBig - kNegBig) is 0, not NaN
constexpr float kNegBig = -1e30f;
// second __launch_bounds__ argument (waves per SIMD) of the aggregate
// kernels: at most 64 VGPRs, the occupancy spmm_csr_kernel runs at
constexpr int kWavesPerSimd = 8;

// The backward holds two accumulators plus four gathered rows. Its 4-wide
// instance does not fit 64 VGPRs without scratch, so it is bounded at 5 waves
// per SIMD and compiles to 76-80 VGPRs (6 waves) — measured faster than
// staying 2-wide at 8 waves:
// 17.2 vs 20.0 ms fp32, 9.7 vs 18.8 ms bf16 on the Reddit shape at F=256;
// bf16 8-wide at 4 waves lost to 4-wide (11.2 ms). profiles/README.md.
//
// The attention-dropout (DROP) instances add the hash to the per-edge work.
// Three of them spill at the bounds above (16-32 B/lane of scratch) and get
// one wave less, which removes the scratch: the 4-wide forward with zc/csum
// (both dtypes) and the fp32 2-wide backward.
template <int VEC, bool AUX, bool DROP>
constexpr int kFwdWaves =
    (AUX && DROP && VEC >= 4) ? kWavesPerSimd - 1 : kWavesPerSimd;
template <typename T, int VEC, bool DROP>
constexpr int kBwdWaves =
    VEC > 2 ? 5
            : (DROP && VEC == 2 && sizeof(T) == 4 ? kWavesPerSimd - 1
                                                  : kWavesPerSimd);

// alpha and c = alpha * leaky_relu'(s) of one edge and head
__device__ __forceinline__ void edge_weight(float s, float lse, float slope,
                                            float& a, float& c) {
  a = expf(leaky(s, slope) - lse);
  c = s > 0.f ? a : slope * a;
}

// ---------------------------------------------------------------------------
// lse[r,h] = log sum_{u in N(r)} exp(leaky_relu(el[u,h] + er[r,h]))
// One wave per row; lanes stride over the row's edges with a running
// (max, sum-exp) per head, merged by a fixed-order butterfly. Rows without
// edges get 0.
// ---------------------------------------------------------------------------
__global__ void gat_row_stats_kernel(const int64_t* __restrict__ indptr,
                                     const int32_t* __restrict__ indices,
                                     const float* __restrict__ el,
                                     const float* __restrict__ er,
                                     float* __restrict__ lse,
                                     int64_t num_rows, int64_t H,
                                     float slope) {
  const WaveIds wv = wave_ids();
  const int lane = wv.lane;

  for (int64_t r = wv.wave_global; r < num_rows; r += wv.nwaves) {
    const int64_t e_begin = indptr[r];
    const int64_t e_end = indptr[r + 1];
    for (int64_t h0 = 0; h0 < H; h0 += kHeadBlk) {
      float m[kHeadBlk], s[kHeadBlk], erv[kHeadBlk];
#pragma unroll
      for (int k = 0; k < kHeadBlk; ++k) {
        m[k] = kNegBig;
        s[k] = 0.f;
        erv[k] = h0 + k < H ? er[r * H + h0 + k] : 0.f;
      }
      for (int64_t e = e_begin + lane; e < e_end; e += kWave) {
        const int64_t u = indices[e];
#pragma unroll
        for (int k = 0; k < kHeadBlk; ++k) {
          if (h0 + k < H) {
            const float x = leaky(el[u * H + h0 + k] + erv[k], slope);
            if (x > m[k]) {
              s[k] = s[k] * expf(m[k] - x) + 1.f;
              m[k] = x;
            } else {
              s[k] += expf(x - m[k]);
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < kHeadBlk; ++k) {
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
          const float mo = __shfl_xor(m[k], off, kWave);
          const float so = __shfl_xor(s[k], off, kWave);
          const float mn = fmaxf(m[k], mo);
          s[k] = s[k] * expf(m[k] - mn) + so * expf(mo - mn);
          m[k] = mn;
        }
        if (lane == 0 && h0 + k < H)
          lse[r * H + h0 + k] = e_end > e_begin ? m[k] + logf(s[k]) : 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Forward: out[r, f] = sum_e alpha(u_e, r, f / D) * z[u_e, f]
// AUX also emits zc[r, f] = sum_e c * z[u_e, f] and csum[r, h] = sum_e c from
// the same gathers (second accumulator, different scalar weight).
// F = H * D and VEC | D, so every lane with f0 < F owns VEC whole elements of
// one head — there is no ragged tail.
// DROP multiplies a and the zc weight by the edge's dropout weight; csum
// keeps the unmasked c (file header).
// ---------------------------------------------------------------------------
template <typename T, int VEC, bool AUX, bool DROP>
__global__ void __launch_bounds__(256, (kFwdWaves<VEC, AUX, DROP>))
gat_aggregate_fwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ z, const float* __restrict__ el,
    const float* __restrict__ er, const float* __restrict__ lse,
    const int32_t* __restrict__ row_order, T* __restrict__ out,
    T* __restrict__ zc, float* __restrict__ csum, int64_t num_rows, int64_t F,
    int64_t H, int64_t D, int64_t nchunks, float slope, uint32_t key,
    uint32_t thr, float scale) {
  const WaveIds wv = wave_ids();
  const int lane = wv.lane;
  const int64_t npairs = num_rows * nchunks;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nchunks;
    const int64_t chunk = pair % nchunks;
    if (row_order) r = row_order[r];
    const int64_t f0 = chunk * (kWave * VEC) + lane * VEC;
    if (f0 >= F) continue;
    const int64_t h = f0 / D;
    const float er_v = er[r * H + h];
    const float lse_v = lse[r * H + h];
    const float* elh = el + h;
    const T* zf = z + f0;
    uint32_t base = 0;
    if constexpr (DROP)
      base = drop_base(static_cast<uint32_t>(r), kDropMulV,
                       static_cast<uint32_t>(h), key);

    float acc[VEC], accc[VEC];
    float cs = 0.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = accc[k] = 0.f;

    auto one_edge = [&](int64_t e) {
      const int64_t u = indices[e];
      float a, c, v[VEC];
      ld_vec<T, VEC>(zf + u * F, v);
      edge_weight(elh[u * H] + er_v, lse_v, slope, a, c);
      if constexpr (DROP) {
        // csum takes the unmasked c, then a and c are masked in place
        if (AUX) cs += c;
        const float w = drop_weight(static_cast<uint32_t>(u), kDropMulU, base,
                                    thr, scale);
        a *= w;
        c *= w;
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] += a * v[k];
      if (AUX) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) accc[k] += c * v[k];
        if constexpr (!DROP) cs += c;
      }
    };

    const int64_t e_end = indptr[r + 1];
    int64_t e = indptr[r];
    // peel until e is 4-aligned: the unrolled loop reads four indices with
    // one dwordx4 and keeps four row gathers in flight (as the SpMM does)
    for (; e < e_end && (e & 3); ++e) one_edge(e);
    for (; e + 4 <= e_end; e += 4) {
      const int32x4 uu = __builtin_nontemporal_load(
          reinterpret_cast<const int32x4*>(indices + e));
      const int64_t u0 = uu[0], u1 = uu[1], u2 = uu[2], u3 = uu[3];
      const float x0 = elh[u0 * H], x1 = elh[u1 * H], x2 = elh[u2 * H],
                  x3 = elh[u3 * H];
      float v0[VEC], v1[VEC], v2[VEC], v3[VEC];
      ld_vec<T, VEC>(zf + u0 * F, v0);
      ld_vec<T, VEC>(zf + u1 * F, v1);
      ld_vec<T, VEC>(zf + u2 * F, v2);
      ld_vec<T, VEC>(zf + u3 * F, v3);
      float a0, a1, a2, a3, c0, c1, c2, c3;
      edge_weight(x0 + er_v, lse_v, slope, a0, c0);
      edge_weight(x1 + er_v, lse_v, slope, a1, c1);
      edge_weight(x2 + er_v, lse_v, slope, a2, c2);
      edge_weight(x3 + er_v, lse_v, slope, a3, c3);
      if constexpr (DROP) {
        if (AUX) cs += c0 + c1 + c2 + c3;
        const float w0 = drop_weight(uu[0], kDropMulU, base, thr, scale);
        const float w1 = drop_weight(uu[1], kDropMulU, base, thr, scale);
        const float w2 = drop_weight(uu[2], kDropMulU, base, thr, scale);
        const float w3 = drop_weight(uu[3], kDropMulU, base, thr, scale);
        a0 *= w0, a1 *= w1, a2 *= w2, a3 *= w3;
        c0 *= w0, c1 *= w1, c2 *= w2, c3 *= w3;
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        acc[k] += a0 * v0[k] + a1 * v1[k] + a2 * v2[k] + a3 * v3[k];
      if (AUX) {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          accc[k] += c0 * v0[k] + c1 * v1[k] + c2 * v2[k] + c3 * v3[k];
        if constexpr (!DROP) cs += c0 + c1 + c2 + c3;
      }
    }
    for (; e < e_end; ++e) one_edge(e);

    st_vec<T, VEC>(out + r * F + f0, acc);
    if (AUX) {
      st_vec<T, VEC>(zc + r * F + f0, accc);
      // every lane of a head holds the same cs; its first lane writes it
      if (f0 % D == 0) csum[r * H + h] = cs;
    }
  }
}

// ---------------------------------------------------------------------------
// Backward over the CSC (row = source u, columns = destinations v):
//   dz[u, f]   = sum_v alpha * g[v, f]
//   gc[f]      = sum_v c * g[v, f]                    (registers only)
//   d_el[u, h] = sum_{f in head h} gc[f] * z[u, f]  -  sum_v c * t[v, h]
// The per-head dot is one fixed-order wave reduction per head the chunk
// touches, written to d_el_part[u, chunk, h]; the launcher sums the chunk
// axis (a head may span several chunks). d_el_part must be zero-filled.
// dst_state[v, h] = (er, lse, t, 0): the three per-destination scalars of an
// edge arrive in ONE 16-byte gather instead of three 4-byte ones.
// DROP multiplies the dz and gc weights by the edge's dropout weight; the
// sum_v c*t term keeps the unmasked c (file header).
// ---------------------------------------------------------------------------
template <typename T, int VEC, bool DROP>
__global__ void __launch_bounds__(256, (kBwdWaves<T, VEC, DROP>))
gat_aggregate_bwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ g, const T* __restrict__ z,
    const float* __restrict__ el, const f32x4* __restrict__ dst_state,
    const int32_t* __restrict__ row_order, T* __restrict__ dz,
    float* __restrict__ d_el_part, int64_t num_rows, int64_t F, int64_t H,
    int64_t D, int64_t nchunks, float slope, uint32_t key, uint32_t thr,
    float scale) {
  const WaveIds wv = wave_ids();
  const int lane = wv.lane;
  const int64_t npairs = num_rows * nchunks;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nchunks;
    const int64_t chunk = pair % nchunks;
    if (row_order) r = row_order[r];
    const int64_t c_begin = chunk * (kWave * VEC);
    const int64_t f0 = c_begin + lane * VEC;
    // no early exit: every lane takes part in the reductions below
    const bool active = f0 < F;
    const int64_t h = active ? f0 / D : 0;
    float partial = 0.f;

    if (active) {
      const float el_u = el[r * H + h];
      const T* gf = g + f0;
      uint32_t base = 0;
      if constexpr (DROP)
        base = drop_base(static_cast<uint32_t>(r), kDropMulU,
                         static_cast<uint32_t>(h), key);
      float acc[VEC], gc[VEC];
      float ct = 0.f;
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = gc[k] = 0.f;

      auto one_edge = [&](int64_t e) {
        const int64_t v = indices[e];
        float a, c, gv[VEC];
        ld_vec<T, VEC>(gf + v * F, gv);
        const f32x4 d = dst_state[v * H + h];
        edge_weight(el_u + d[0], d[1], slope, a, c);
        ct += c * d[2];
        if constexpr (DROP) {
          const float w = drop_weight(static_cast<uint32_t>(v), kDropMulV,
                                      base, thr, scale);
          a *= w;
          c *= w;
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          acc[k] += a * gv[k];
          gc[k] += c * gv[k];
        }
      };

      const int64_t e_end = indptr[r + 1];
      int64_t e = indptr[r];
      for (; e < e_end && (e & 3); ++e) one_edge(e);
      for (; e + 4 <= e_end; e += 4) {
        const int32x4 vv = __builtin_nontemporal_load(
            reinterpret_cast<const int32x4*>(indices + e));
        const f32x4 d0 = dst_state[vv[0] * H + h];
        const f32x4 d1 = dst_state[vv[1] * H + h];
        const f32x4 d2 = dst_state[vv[2] * H + h];
        const f32x4 d3 = dst_state[vv[3] * H + h];
        float g0[VEC], g1[VEC], g2[VEC], g3[VEC];
        ld_vec<T, VEC>(gf + static_cast<int64_t>(vv[0]) * F, g0);
        ld_vec<T, VEC>(gf + static_cast<int64_t>(vv[1]) * F, g1);
        ld_vec<T, VEC>(gf + static_cast<int64_t>(vv[2]) * F, g2);
        ld_vec<T, VEC>(gf + static_cast<int64_t>(vv[3]) * F, g3);
        float a0, a1, a2, a3, c0, c1, c2, c3;
        edge_weight(el_u + d0[0], d0[1], slope, a0, c0);
        edge_weight(el_u + d1[0], d1[1], slope, a1, c1);
        edge_weight(el_u + d2[0], d2[1], slope, a2, c2);
        edge_weight(el_u + d3[0], d3[1], slope, a3, c3);
        ct += c0 * d0[2] + c1 * d1[2] + c2 * d2[2] + c3 * d3[2];
        if constexpr (DROP) {
          const float w0 = drop_weight(vv[0], kDropMulV, base, thr, scale);
          const float w1 = drop_weight(vv[1], kDropMulV, base, thr, scale);
          const float w2 = drop_weight(vv[2], kDropMulV, base, thr, scale);
          const float w3 = drop_weight(vv[3], kDropMulV, base, thr, scale);
          a0 *= w0, a1 *= w1, a2 *= w2, a3 *= w3;
          c0 *= w0, c1 *= w1, c2 *= w2, c3 *= w3;
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          acc[k] += a0 * g0[k] + a1 * g1[k] + a2 * g2[k] + a3 * g3[k];
          gc[k] += c0 * g0[k] + c1 * g1[k] + c2 * g2[k] + c3 * g3[k];
        }
      }
      for (; e < e_end; ++e) one_edge(e);

      st_vec<T, VEC>(dz + r * F + f0, acc);
      float zu[VEC];
      ld_vec<T, VEC>(z + r * F + f0, zu);
#pragma unroll
      for (int k = 0; k < VEC; ++k) partial += gc[k] * zu[k];
      // sum_v c*t is the same in every lane of a head: its first lane
      // subtracts it once
      if (f0 % D == 0) partial -= ct;
    }

    const int64_t c_last = min(F, c_begin + kWave * VEC) - 1;
    const int64_t h_hi = c_last / D;
    for (int64_t hh = c_begin / D; hh <= h_hi; ++hh) {
      const float tot = wave_sum(active && h == hh ? partial : 0.f);
      if (lane == 0) d_el_part[(r * nchunks + chunk) * H + hh] = tot;
    }
  }
}

// The keep bit on explicit id tensors (one thread per edge, all heads): lets
// the device hash be compared with its torch mirror without building a graph.
__global__ void gat_dropout_keep_kernel(const int32_t* __restrict__ u,
                                        const int32_t* __restrict__ v,
                                        bool* __restrict__ keep, int64_t n,
                                        int64_t H, uint32_t key,
                                        uint32_t thr) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       i < n; i += stride) {
    const uint32_t ui = static_cast<uint32_t>(u[i]);
    const uint32_t vi = static_cast<uint32_t>(v[i]);
    for (int64_t h = 0; h < H; ++h) {
      // the forward's hoisting: v and h fixed, u per edge
      const uint32_t base =
          drop_base(vi, kDropMulV, static_cast<uint32_t>(h), key);
      keep[i * H + h] = drop_mix(ui * kDropMulU + base) >= thr;
    }
  }
}

// Widest compiled instances (compiler resource remarks,
// profiles/README.md): none uses scratch. bf16 forward-with-aux stops at 4
// elements to stay within kWavesPerSimd's 64 VGPRs; the backward at 4.
template <typename T, bool AUX, bool DROP>
constexpr int kFwdMaxVec = (AUX && sizeof(T) == 2) ? 4 : 16 / sizeof(T);
constexpr int kBwdMaxVec = 4;

// low word of splitmix64(seed): the 32-bit key of one call's masks
uint32_t drop_fold_seed(int64_t seed) {
  uint64_t x = static_cast<uint64_t>(seed) + 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return static_cast<uint32_t>(x);
}

// thr = min(round(p * 2^32), 2^32 - 1); an edge is kept when hash >= thr
uint32_t drop_threshold(double p) {
  const double t = std::floor(p * 4294967296.0 + 0.5);
  return t >= 4294967295.0 ? 0xFFFFFFFFu : static_cast<uint32_t>(t);
}

// Widest lane access (<= 16 B, <= max_vec elements) whose element count
// divides the head width D, so a lane never straddles two heads. Unlike the
// SpMM (8 B preferred) the per-edge exp is paid once per lane whatever the
// width, so wider is better.
int gat_pick_vec(int64_t D, int64_t elem_size, int max_vec,
                 std::initializer_list<const void*> ptrs) {
  for (int v = std::min(max_vec, static_cast<int>(16 / elem_size)); v > 1;
       v >>= 1) {
    if (D % v) continue;
    bool ok = true;
    for (const void* p : ptrs) ok = ok && aligned_to(p, v * elem_size);
    if (ok) return v;
  }
  return 1;
}

// the shared host checks (attn_util.h), with this op's name in the messages
constexpr const char* kOp = "gat";

}  // namespace

torch::Tensor gat_row_stats_hip(torch::Tensor indptr, torch::Tensor indices,
                                torch::Tensor el, torch::Tensor er,
                                int64_t num_cols, double slope) {
  check_graph(kOp, indptr, indices);
  const int64_t num_rows = indptr.numel() - 1;
  TORCH_CHECK(er.dim() == 2, "gat: er must be [num_rows, H]");
  const int64_t H = er.size(1);
  TORCH_CHECK(H >= 1, "gat: at least one head");
  check_node_table(kOp, er, num_rows, H, "er");
  check_node_table(kOp, el, num_cols, H, "el");
  auto lse = torch::empty({num_rows, H}, er.options());
  const int threads = 256;
  hipLaunchKernelGGL(gat_row_stats_kernel, dim3(grid_for(num_rows, threads)),
                     dim3(threads), 0, current_stream(),
                     indptr.data_ptr<int64_t>(), indices.data_ptr<int32_t>(),
                     el.data_ptr<float>(), er.data_ptr<float>(),
                     lse.data_ptr<float>(), num_rows, H,
                     static_cast<float>(slope));
  check_launch();
  return lse;
}

template <typename T>
static void fwd_dispatch(const torch::Tensor& indptr,
                         const torch::Tensor& indices, const torch::Tensor& z,
                         const torch::Tensor& el, const torch::Tensor& er,
                         const torch::Tensor& lse, const int32_t* rop,
                         torch::Tensor& out, torch::Tensor& zc,
                         torch::Tensor& csum, int64_t num_rows, int64_t F,
                         int64_t H, bool with_aux, float slope,
                         DropArgs drop) {
  const int64_t D = F / H;
  const T* zp = reinterpret_cast<const T*>(z.data_ptr());
  T* op = reinterpret_cast<T*>(out.data_ptr());
  T* zcp = with_aux ? reinterpret_cast<T*>(zc.data_ptr()) : nullptr;
  float* csp = with_aux ? csum.data_ptr<float>() : nullptr;
  auto stream = current_stream();
  auto run = [&](auto aux_c, auto drop_c) {
    constexpr bool AUX = decltype(aux_c)::value;
    constexpr bool DROP = decltype(drop_c)::value;
    const int vec =
        gat_pick_vec(D, sizeof(T), kFwdMaxVec<T, AUX, DROP>, {zp, op, zcp});
    dispatch_vec(vec, [&](auto v) {
      constexpr int VEC = decltype(v)::value;
      if constexpr (VEC <= kFwdMaxVec<T, AUX, DROP>) {
        const int64_t nchunks = (F + kWave * VEC - 1) / (kWave * VEC);
        const int threads = 256;
        hipLaunchKernelGGL(
            HIP_KERNEL_NAME(gat_aggregate_fwd_kernel<T, VEC, AUX, DROP>),
            dim3(grid_for(num_rows * nchunks, threads)), dim3(threads), 0,
            stream, indptr.data_ptr<int64_t>(), indices.data_ptr<int32_t>(),
            zp, el.data_ptr<float>(), er.data_ptr<float>(),
            lse.data_ptr<float>(), rop, op, zcp, csp, num_rows, F, H, D,
            nchunks, slope, drop.key, drop.thr, drop.scale);
      }
    });
  };
  const bool dropping = drop.thr > 0;
  if (with_aux && dropping)
    run(std::true_type{}, std::true_type{});
  else if (with_aux)
    run(std::true_type{}, std::false_type{});
  else if (dropping)
    run(std::false_type{}, std::true_type{});
  else
    run(std::false_type{}, std::false_type{});
  check_launch();
}

std::vector<torch::Tensor> gat_aggregate_fwd_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor z,
    torch::Tensor el, torch::Tensor er, torch::Tensor lse,
    torch::Tensor row_order, int64_t num_cols, int64_t H, double slope,
    bool with_aux, int64_t drop_key, int64_t drop_thr, double drop_scale) {
  check_graph(kOp, indptr, indices);
  const DropArgs drop = drop_args(kOp, drop_key, drop_thr, drop_scale);
  const int64_t num_rows = indptr.numel() - 1;
  check_features(kOp, z, num_cols, H, "z");
  const int64_t F = z.size(1);
  check_node_table(kOp, el, num_cols, H, "el");
  check_node_table(kOp, er, num_rows, H, "er");
  check_node_table(kOp, lse, num_rows, H, "lse");
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto out = torch::empty({num_rows, F}, z.options());
  torch::Tensor zc, csum;
  if (with_aux) {
    zc = torch::empty({num_rows, F}, z.options());
    csum = torch::empty({num_rows, H}, er.options());
  }
  if (z.scalar_type() == torch::kBFloat16)
    fwd_dispatch<__hip_bfloat16>(indptr, indices, z, el, er, lse, rop, out, zc,
                                 csum, num_rows, F, H, with_aux,
                                 static_cast<float>(slope), drop);
  else
    fwd_dispatch<float>(indptr, indices, z, el, er, lse, rop, out, zc, csum,
                        num_rows, F, H, with_aux, static_cast<float>(slope),
                        drop);
  if (!with_aux) return {out};
  return {out, zc, csum};
}

template <typename T>
static torch::Tensor bwd_dispatch(
    const torch::Tensor& indptr, const torch::Tensor& indices,
    const torch::Tensor& g, const torch::Tensor& z, const torch::Tensor& el,
    const torch::Tensor& dst_state, const int32_t* rop, torch::Tensor& dz,
    int64_t num_rows, int64_t F, int64_t H, float slope, DropArgs drop) {
  const int64_t D = F / H;
  const T* gp = reinterpret_cast<const T*>(g.data_ptr());
  const T* zp = reinterpret_cast<const T*>(z.data_ptr());
  T* dzp = reinterpret_cast<T*>(dz.data_ptr());
  const int vec =
      gat_pick_vec(D, sizeof(T), kBwdMaxVec, {gp, zp, dzp});
  auto stream = current_stream();
  torch::Tensor part;
  dispatch_vec(vec, [&](auto v) {
    constexpr int VEC = decltype(v)::value;
    if constexpr (VEC <= kBwdMaxVec) {
      const int64_t nchunks = (F + kWave * VEC - 1) / (kWave * VEC);
      // zero-filled: a chunk writes only the heads it touches
      part = torch::zeros({num_rows, nchunks, H}, el.options());
      const int threads = 256;
      auto launch = [&](auto kern) {
        hipLaunchKernelGGL(
            kern, dim3(grid_for(num_rows * nchunks, threads)), dim3(threads),
            0, stream, indptr.data_ptr<int64_t>(),
            indices.data_ptr<int32_t>(), gp, zp, el.data_ptr<float>(),
            reinterpret_cast<const f32x4*>(dst_state.data_ptr<float>()), rop,
            dzp, part.data_ptr<float>(), num_rows, F, H, D, nchunks, slope,
            drop.key, drop.thr, drop.scale);
      };
      if (drop.thr > 0)
        launch(HIP_KERNEL_NAME(gat_aggregate_bwd_kernel<T, VEC, true>));
      else
        launch(HIP_KERNEL_NAME(gat_aggregate_bwd_kernel<T, VEC, false>));
    }
  });
  check_launch();
  // fixed-order sum over the (few) chunks a head spans
  return part.size(1) == 1 ? part.select(1, 0) : part.sum(1);
}

std::vector<torch::Tensor> gat_aggregate_bwd_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor g,
    torch::Tensor z, torch::Tensor el, torch::Tensor er, torch::Tensor lse,
    torch::Tensor t, torch::Tensor row_order, int64_t num_cols, int64_t H,
    double slope, int64_t drop_key, int64_t drop_thr, double drop_scale) {
  // indptr/indices are the CSC: rows = source nodes, columns = destinations
  check_graph(kOp, indptr, indices);
  const DropArgs drop = drop_args(kOp, drop_key, drop_thr, drop_scale);
  const int64_t num_rows = indptr.numel() - 1;
  check_features(kOp, g, num_cols, H, "g");
  check_features(kOp, z, num_rows, H, "z");
  const int64_t F = z.size(1);
  TORCH_CHECK(g.size(1) == F && g.scalar_type() == z.scalar_type(),
              "gat: g and z must agree in width and dtype");
  check_node_table(kOp, el, num_rows, H, "el");
  check_node_table(kOp, er, num_cols, H, "er");
  check_node_table(kOp, lse, num_cols, H, "lse");
  check_node_table(kOp, t, num_cols, H, "t");
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto dz = torch::empty({num_rows, F}, z.options());
  // (er, lse, t, 0) per destination and head — node-sized, 16-byte aligned
  auto dst_state =
      torch::stack({er.narrow(0, 0, num_cols), lse.narrow(0, 0, num_cols),
                    t.narrow(0, 0, num_cols),
                    torch::zeros({num_cols, H}, t.options())},
                   2)
          .contiguous();
  TORCH_CHECK(aligned_to(dst_state.data_ptr(), 16));
  torch::Tensor d_el;
  if (z.scalar_type() == torch::kBFloat16)
    d_el = bwd_dispatch<__hip_bfloat16>(indptr, indices, g, z, el, dst_state,
                                        rop, dz, num_rows, F, H,
                                        static_cast<float>(slope), drop);
  else
    d_el = bwd_dispatch<float>(indptr, indices, g, z, el, dst_state, rop, dz,
                               num_rows, F, H, static_cast<float>(slope),
                               drop);
  return {dz, d_el};
}

torch::Tensor gat_dropout_keep_hip(torch::Tensor u, torch::Tensor v, int64_t H,
                                   int64_t seed, double p) {
  TORCH_CHECK(u.is_cuda() && v.is_cuda() && u.is_contiguous() &&
                  v.is_contiguous() && u.scalar_type() == torch::kInt &&
                  v.scalar_type() == torch::kInt && u.dim() == 1 &&
                  v.dim() == 1 && u.numel() == v.numel(),
              "gat_dropout_keep: u and v must be contiguous int32 [n] device "
              "tensors of one length");
  TORCH_CHECK(H >= 1, "gat_dropout_keep: at least one head");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "gat_dropout_keep: p must be in [0, 1)");
  const int64_t n = u.numel();
  auto keep = torch::empty({n, H}, u.options().dtype(torch::kBool));
  if (n == 0) return keep;
  const int threads = 256;
  const int64_t blocks =
      std::min<int64_t>((n + threads - 1) / threads, 8 * 65536);
  hipLaunchKernelGGL(gat_dropout_keep_kernel, dim3(blocks), dim3(threads), 0,
                     current_stream(), u.data_ptr<int32_t>(),
                     v.data_ptr<int32_t>(), keep.data_ptr<bool>(), n, H,
                     drop_fold_seed(seed), drop_threshold(p));
  check_launch();
  return keep;
}
