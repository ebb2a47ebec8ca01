// Scaled dot-product attention aggregation (UniMP's TransformerConv) for
// gfx950: attention weights are never stored.
//
//   s_uvh  = c * <q[v,h,:], K[u,h,:]>              kv[u] = [K[u] | V[u]]
//   alpha  = exp(s_uvh - lse[v,h])                 (lse >= row max: no overflow)
//   agg[v] = sum_u w_uvh * alpha_uvh * V[u,h,:]
//
// The third member of the attention family (gat.hip, gatv2.hip). The score is
// a dot of a row the wave HOLDS (q[v] over the CSR, K[u] over the CSC) with a
// row it GATHERS, and the aggregated row V[u] is another tensor than the
// scored row K[u]. K and V of one source are the two halves of ONE record
// kv[u] of width 2F: a source's two loads hit adjacent memory, and the
// gradient of both comes back as one [nodes, 2F] tensor, so the projection
// that produced kv has ONE backward GEMM. As in GATv2 nothing of size nnz
// exists in forward or backward: every pass recomputes s from the rows it
// gathers, and the transpose pass walks the prebuilt CSC without atomics
// (docs/DESIGN.md, "Dot-product attention aggregation").
//
//  - dot_fwd     : over the CSR, gathers kv[u]. Online softmax (running max,
//                  sum, acc[]), so ONE gather pass emits agg and lse. V does
//                  not depend on the score: the K and V loads of all edges in
//                  flight are issued before the first wait.
//  - dot_bwd_dst : over the CSR, gathers kv[u]; emits d_q[v].
//  - dot_bwd_src : over the CSC, gathers q[v], g[v] and (lse, t)[v]; emits
//                  d_kv[u] = [d_K[u] | d_V[u]].
//
// With t[v,h] = <g[v,h,:], agg[v,h,:]> and, per edge,
//   gz    = <g[v,h,:], V[u,h,:]>
//   delta = alpha * (w * gz - t[v,h])
// the gradients are
//   d_q[v] = c * sum_u delta * K[u]     d_K[u] = c * sum_v delta * q[v]
//   d_V[u] = sum_v w * alpha * g[v]
// w is 1, or with attention dropout keep(key, u, v, h) / (1 - p) from the
// endpoint hash of attn_util.h; the softmax itself (lse) is never masked.
// The held row carries c (q[v] * c over the CSR, K[u] * c over the CSC), so
// the per-edge score is a plain dot; s and gz share one butterfly (seg_sum2).
//
// Scheduling is that of gatv2.hip: one wave per (row, head group),
// grid-stride over row_order, the lane layout of attn_lanes.h, for_edges
// with its aligned dwordx4 index load, non-temporal stores, no atomics and no
// LDS. One fixed set of lanes walks a row's edges in CSR/CSC order and all
// reductions are fixed-order butterflies: results are bitwise reproducible
// and independent of row_order.
//
// Edges in flight. Every pass gathers TWO rows per edge (K and V, or q and
// g), 2 * NV loads per lane, where GATv2's CSR passes gather one: kEdges
// keeps about eight loads per lane and at most 32 gathered registers in
// flight (4 edges at one load group per row, 2 at two, 1 above).
//
// Compiler resource report (profiles/README.md, "Dot-product attention
// aggregation"): no instance uses scratch at the plain 256-thread launch
// bound, up to the 1024-wide head of the lane layout.

#include "../common.h"
#include "hip_util.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <vector>

// This file's device code is built without the packed fp32 instructions
// (v_pk_fma_f32 and kin): every function from here on, the shared attention
// headers' included, carries the target attribute, in the device pass only.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "attn_lanes.h"
#include "attn_util.h"

namespace {

using namespace attn_lanes;

// edges whose two gathered rows are in flight together (file header)
template <int NV>
constexpr int kEdges = NV == 1 ? 4 : (NV == 2 ? 2 : 1);

// <a, b> over this lane's elements (the segment sum is the caller's)
template <int E>
__device__ __forceinline__ float dot_part(const float (&a)[E],
                                          const float (&b)[E]) {
  float p = 0.f;
#pragma unroll
  for (int k = 0; k < E; ++k) p += a[k] * b[k];
  return p;
}

// ---------------------------------------------------------------------------
// Forward over the CSR: agg[r,h,:] = sum_e w * alpha * V[u_e,h,:] and
// lse[r,h], from one gather of the record kv[u_e] per edge. Online softmax:
// (m, sum, acc[]) are rescaled once per batch of edges in flight. The
// denominator takes every edge; only acc sees the dropout weight. Rows
// without edges get 0 and 0. F is the width of q and agg; kv rows are 2F.
// ---------------------------------------------------------------------------
template <typename T, int VEC, int NV, int SEG>
__global__ void __launch_bounds__(256) dot_fwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ q, const T* __restrict__ kv,
    const int32_t* __restrict__ row_order, T* __restrict__ agg,
    float* __restrict__ lse, int64_t num_rows, int64_t F, int64_t H, int64_t D,
    int64_t nhg, float c, uint32_t key, uint32_t thr, float scale) {
  constexpr int E = NV * VEC;
  const WaveIds wv = wave_ids();
  const int lane = wv.lane;
  const int64_t npairs = num_rows * nhg;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nhg;
    if (row_order) r = row_order[r];
    const LaneMap<VEC, NV, SEG> lm(lane, pair % nhg, H, D);
    float qv[E], acc[E];
    ld_row<T, VEC, NV, SEG>(q + r * F, lm, qv);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      qv[k] *= c;
      acc[k] = 0.f;
    }
    float m = kNegBig, sum = 0.f;
    const uint32_t base = drop_base(static_cast<uint32_t>(r), kDropMulV,
                                    static_cast<uint32_t>(lm.h), key);

    const int64_t e_begin = indptr[r], e_end = indptr[r + 1];
    auto batch = [&](auto n_c, const auto& uu) {
      constexpr int N = decltype(n_c)::value;
      float kk[N][E], vv[N][E], s[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const T* rec = kv + static_cast<int64_t>(uu[i]) * (2 * F);
        ld_row<T, VEC, NV, SEG>(rec, lm, kk[i]);
        ld_row<T, VEC, NV, SEG>(rec + F, lm, vv[i]);
      }
#pragma unroll
      for (int i = 0; i < N; ++i) s[i] = dot_part<E>(qv, kk[i]);
#pragma unroll
      for (int i = 0; i < N; ++i) s[i] = seg_sum<SEG>(s[i]);
      float mn = m;
#pragma unroll
      for (int i = 0; i < N; ++i) mn = fmaxf(mn, s[i]);
      const float resc = expf(m - mn);
      m = mn;
      sum *= resc;
#pragma unroll
      for (int k = 0; k < E; ++k) acc[k] *= resc;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        float p = expf(s[i] - mn);
        sum += p;
        if (thr)
          p *= drop_weight(static_cast<uint32_t>(uu[i]), kDropMulU, base, thr,
                           scale);
#pragma unroll
        for (int k = 0; k < E; ++k) acc[k] += p * vv[i][k];
      }
    };
    for_edges<kEdges<NV>>(indices, e_begin, e_end, batch);

    const bool any = e_end > e_begin;
    const float inv = any ? 1.f / sum : 0.f;
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] *= inv;
    st_row<T, VEC, NV, SEG>(agg + r * F, lm, acc);
    if (lm.head_ok && (lane & (SEG - 1)) == 0)
      lse[r * H + lm.h] = any ? m + logf(sum) : 0.f;
  }
}

// ---------------------------------------------------------------------------
// Backward over the CSR (row = destination v): gathers kv[u] per edge.
//   d_q[v,h,:] = c * sum_u delta * K[u,h,:]
// Rows without edges get zeros.
// ---------------------------------------------------------------------------
template <typename T, int VEC, int NV, int SEG>
__global__ void __launch_bounds__(256) dot_bwd_dst_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ g, const T* __restrict__ q,
    const T* __restrict__ kv, const float* __restrict__ lse,
    const float* __restrict__ t, const int32_t* __restrict__ row_order,
    T* __restrict__ d_q, int64_t num_rows, int64_t F, int64_t H, int64_t D,
    int64_t nhg, float c, uint32_t key, uint32_t thr, float scale) {
  constexpr int E = NV * VEC;
  const WaveIds wv = wave_ids();
  const int lane = wv.lane;
  const int64_t npairs = num_rows * nhg;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nhg;
    if (row_order) r = row_order[r];
    const LaneMap<VEC, NV, SEG> lm(lane, pair % nhg, H, D);
    float qv[E], gv[E], dq[E];
    ld_row<T, VEC, NV, SEG>(q + r * F, lm, qv);
    ld_row<T, VEC, NV, SEG>(g + r * F, lm, gv);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      qv[k] *= c;
      dq[k] = 0.f;
    }
    const float lse_v = lse[r * H + lm.h];
    const float t_v = t[r * H + lm.h];
    const uint32_t base = drop_base(static_cast<uint32_t>(r), kDropMulV,
                                    static_cast<uint32_t>(lm.h), key);

    auto batch = [&](auto n_c, const auto& uu) {
      constexpr int N = decltype(n_c)::value;
      float kk[N][E], vv[N][E], s[N], gz[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const T* rec = kv + static_cast<int64_t>(uu[i]) * (2 * F);
        ld_row<T, VEC, NV, SEG>(rec, lm, kk[i]);
        ld_row<T, VEC, NV, SEG>(rec + F, lm, vv[i]);
      }
#pragma unroll
      for (int i = 0; i < N; ++i) {
        s[i] = dot_part<E>(qv, kk[i]);
        gz[i] = dot_part<E>(gv, vv[i]);
      }
#pragma unroll
      for (int i = 0; i < N; ++i) seg_sum2<SEG>(s[i], gz[i], lane);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float alpha = expf(s[i] - lse_v);
        const float w =
            thr ? drop_weight(static_cast<uint32_t>(uu[i]), kDropMulU, base,
                              thr, scale)
                : 1.f;
        const float delta = alpha * (w * gz[i] - t_v);
#pragma unroll
        for (int k = 0; k < E; ++k) dq[k] += delta * kk[i][k];
      }
    };
    for_edges<kEdges<NV>>(indices, indptr[r], indptr[r + 1], batch);

#pragma unroll
    for (int k = 0; k < E; ++k) dq[k] *= c;
    st_row<T, VEC, NV, SEG>(d_q + r * F, lm, dq);
  }
}

// ---------------------------------------------------------------------------
// Backward over the CSC (row = source u, columns = destinations v): holds
// the record kv[u], gathers q[v], g[v] and dst_state[v,h] = (lse, t) per
// entry.
//   d_K[u,h,:] = c * sum_v delta * q[v,h,:]
//   d_V[u,h,:] = sum_v w * alpha * g[v,h,:]
// stored as the two halves of d_kv[u]. Sources without edges get zeros.
// ---------------------------------------------------------------------------
template <typename T, int VEC, int NV, int SEG>
__global__ void __launch_bounds__(256) dot_bwd_src_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ g, const T* __restrict__ q,
    const T* __restrict__ kv, const f32x2* __restrict__ dst_state,
    const int32_t* __restrict__ row_order, T* __restrict__ d_kv,
    int64_t num_rows, int64_t F, int64_t H, int64_t D, int64_t nhg, float c,
    uint32_t key, uint32_t thr, float scale) {
  constexpr int E = NV * VEC;
  const WaveIds wv = wave_ids();
  const int lane = wv.lane;
  const int64_t npairs = num_rows * nhg;

  for (int64_t pair = wv.wave_global; pair < npairs; pair += wv.nwaves) {
    int64_t r = pair / nhg;
    if (row_order) r = row_order[r];
    const LaneMap<VEC, NV, SEG> lm(lane, pair % nhg, H, D);
    float ku[E], vu[E], dk[E], dv[E];
    const T* rec = kv + r * (2 * F);
    ld_row<T, VEC, NV, SEG>(rec, lm, ku);
    ld_row<T, VEC, NV, SEG>(rec + F, lm, vu);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      ku[k] *= c;
      dk[k] = dv[k] = 0.f;
    }
    const uint32_t base = drop_base(static_cast<uint32_t>(r), kDropMulU,
                                    static_cast<uint32_t>(lm.h), key);

    auto batch = [&](auto n_c, const auto& dd) {
      constexpr int N = decltype(n_c)::value;
      float qv[N][E], gv[N][E], s[N], gz[N];
      f32x2 st[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int64_t v = dd[i];
        st[i] = dst_state[v * H + lm.h];
        ld_row<T, VEC, NV, SEG>(q + v * F, lm, qv[i]);
        ld_row<T, VEC, NV, SEG>(g + v * F, lm, gv[i]);
      }
#pragma unroll
      for (int i = 0; i < N; ++i) {
        s[i] = dot_part<E>(qv[i], ku);
        gz[i] = dot_part<E>(gv[i], vu);
      }
#pragma unroll
      for (int i = 0; i < N; ++i) seg_sum2<SEG>(s[i], gz[i], lane);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float alpha = expf(s[i] - st[i][0]);
        const float w =
            thr ? drop_weight(static_cast<uint32_t>(dd[i]), kDropMulV, base,
                              thr, scale)
                : 1.f;
        const float delta = alpha * (w * gz[i] - st[i][1]);
        const float wa = w * alpha;
#pragma unroll
        for (int k = 0; k < E; ++k) {
          dk[k] += delta * qv[i][k];
          dv[k] += wa * gv[i][k];
        }
      }
    };
    for_edges<kEdges<NV>>(indices, indptr[r], indptr[r + 1], batch);

#pragma unroll
    for (int k = 0; k < E; ++k) dk[k] *= c;
    T* out = d_kv + r * (2 * F);
    st_row<T, VEC, NV, SEG>(out, lm, dk);
    st_row<T, VEC, NV, SEG>(out + F, lm, dv);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// the shared host checks (attn_util.h), with this op's name in the messages
constexpr const char* kOp = "dot";

// q / g: a [nodes, F] tensor whose heads fit the lane layout
void check_rows(const torch::Tensor& x, int64_t rows, int64_t H,
                const char* name) {
  check_features(kOp, x, rows, H, name);
  TORCH_CHECK(x.size(1) / H <= kMaxHeadDim, "dot: head width D=",
              x.size(1) / H, " exceeds the supported ", kMaxHeadDim);
}

// kv: [nodes, 2F] records of q's dtype, K in the first F columns
void check_kv(const torch::Tensor& kv, const torch::Tensor& q, int64_t rows,
              int64_t H) {
  check_features(kOp, kv, rows, 2 * H, "kv");
  TORCH_CHECK(kv.size(1) == 2 * q.size(1) &&
                  kv.scalar_type() == q.scalar_type(),
              "dot: kv must be [nodes, 2F] = [K | V] of q's dtype, got width ",
              kv.size(1), " for F=", q.size(1));
}

void check_same(const torch::Tensor& x, const torch::Tensor& like,
                const char* name) {
  TORCH_CHECK(x.size(1) == like.size(1) &&
                  x.scalar_type() == like.scalar_type(),
              "dot: ", name, " must agree with q in width and dtype");
}

}  // namespace

std::vector<torch::Tensor> dot_fwd_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor q,
    torch::Tensor kv, torch::Tensor row_order, int64_t num_cols, int64_t H,
    double scale, int64_t drop_key, int64_t drop_thr, double drop_scale) {
  check_graph(kOp, indptr, indices);
  const DropArgs drop = drop_args(kOp, drop_key, drop_thr, drop_scale);
  const int64_t num_rows = indptr.numel() - 1;
  check_rows(q, num_rows, H, "q");
  check_kv(kv, q, num_cols, H);
  const int64_t F = q.size(1);
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto agg = torch::empty({num_rows, F}, q.options());
  auto lse = torch::empty({num_rows, H}, q.options().dtype(torch::kFloat));
  if (num_rows == 0) return {agg, lse};
  // kv + F shares kv's alignment class: 4 | D makes 4 | F
  const Layout l = pick_layout(kOp, F / H, q.element_size(), nullptr,
                               {q.data_ptr(), kv.data_ptr(), agg.data_ptr()});
  dispatch_dtype(q, [&](auto tag) {
    using T = decltype(tag);
    launch(kOp, l, indptr, indices, F, H, static_cast<float>(scale), drop,
           ATTN_LANES_KERNEL_OF(dot_fwd_kernel, T), cptr<T>(q), cptr<T>(kv),
           rop, mptr<T>(agg), lse.data_ptr<float>());
  });
  return {agg, lse};
}

torch::Tensor dot_bwd_dst_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor g,
    torch::Tensor q, torch::Tensor kv, torch::Tensor lse, torch::Tensor t,
    torch::Tensor row_order, int64_t num_cols, int64_t H, double scale,
    int64_t drop_key, int64_t drop_thr, double drop_scale) {
  check_graph(kOp, indptr, indices);
  const DropArgs drop = drop_args(kOp, drop_key, drop_thr, drop_scale);
  const int64_t num_rows = indptr.numel() - 1;
  check_rows(q, num_rows, H, "q");
  check_rows(g, num_rows, H, "g");
  check_same(g, q, "g");
  check_kv(kv, q, num_cols, H);
  const int64_t F = q.size(1);
  check_node_table(kOp, lse, num_rows, H, "lse");
  check_node_table(kOp, t, num_rows, H, "t");
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto d_q = torch::empty({num_rows, F}, q.options());
  if (num_rows == 0) return d_q;
  const Layout l = pick_layout(
      kOp, F / H, q.element_size(), nullptr,
      {q.data_ptr(), g.data_ptr(), kv.data_ptr(), d_q.data_ptr()});
  dispatch_dtype(q, [&](auto tag) {
    using T = decltype(tag);
    launch(kOp, l, indptr, indices, F, H, static_cast<float>(scale), drop,
           ATTN_LANES_KERNEL_OF(dot_bwd_dst_kernel, T), cptr<T>(g),
           cptr<T>(q), cptr<T>(kv), lse.data_ptr<float>(),
           t.data_ptr<float>(), rop, mptr<T>(d_q));
  });
  return d_q;
}

torch::Tensor dot_bwd_src_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor g,
    torch::Tensor q, torch::Tensor kv, torch::Tensor lse, torch::Tensor t,
    torch::Tensor row_order, int64_t num_cols, int64_t H, double scale,
    int64_t drop_key, int64_t drop_thr, double drop_scale) {
  // indptr/indices are the CSC: rows = source nodes, columns = destinations
  check_graph(kOp, indptr, indices);
  const DropArgs drop = drop_args(kOp, drop_key, drop_thr, drop_scale);
  const int64_t num_rows = indptr.numel() - 1;
  check_rows(q, num_cols, H, "q");
  check_rows(g, num_cols, H, "g");
  check_same(g, q, "g");
  check_kv(kv, q, num_rows, H);
  const int64_t F = q.size(1);
  check_node_table(kOp, lse, num_cols, H, "lse");
  check_node_table(kOp, t, num_cols, H, "t");
  const int32_t* rop = row_order_ptr(kOp, row_order, num_rows);
  auto d_kv = torch::empty({num_rows, 2 * F}, kv.options());
  if (num_rows == 0) return d_kv;
  // (lse, t) per destination and head: one 8-byte gather per entry
  auto dst_state = torch::stack({lse.narrow(0, 0, num_cols),
                                 t.narrow(0, 0, num_cols)},
                                2)
                       .contiguous();
  TORCH_CHECK(aligned_to(dst_state.data_ptr(), 8));
  const Layout l = pick_layout(
      kOp, F / H, q.element_size(), nullptr,
      {q.data_ptr(), g.data_ptr(), kv.data_ptr(), d_kv.data_ptr()});
  dispatch_dtype(q, [&](auto tag) {
    using T = decltype(tag);
    launch(kOp, l, indptr, indices, F, H, static_cast<float>(scale), drop,
           ATTN_LANES_KERNEL_OF(dot_bwd_src_kernel, T), cptr<T>(g),
           cptr<T>(q), cptr<T>(kv),
           reinterpret_cast<const f32x2*>(dst_state.data_ptr<float>()), rop,
           mptr<T>(d_kv));
  });
  return d_kv;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
