// Common declarations shared between the host graph core and the HIP kernel
// launchers of pipegcn_amd._C.
//
// The native layer replaces the reference's external stacks (DGL C++/CUDA SpMM,
// METIS partitioning, Gloo staging; see /root/reference SURVEY §2.2) with
// MI355X-native C++/HIP code compiled for gfx950 only.
#pragma once

#include <torch/extension.h>

#include <cstdint>
#include <vector>

// ---------------------------------------------------------------------------
// Host-side graph core (graph_core.cpp)
// ---------------------------------------------------------------------------

// Build a CSR adjacency over destination rows from a COO edge list.
//   u, v : int64/int32 CPU tensors of equal length E (edge u -> v)
//   num_rows : number of destination nodes (rows)
// Returns (indptr int64[num_rows+1], indices int32[E]) where
// indices[indptr[r]:indptr[r+1]] are the sources of row r (unsorted within row).
std::vector<torch::Tensor> build_csr(torch::Tensor u, torch::Tensor v,
                                     int64_t num_rows);

// Multi-way graph partitioner (replaces METIS; BFS-grown balanced seeds +
// boundary refinement). Operates on an undirectedized CSR of the full graph.
//   indptr int64[N+1], indices int32[E] (CSR over rows = nodes)
//   nparts : number of partitions
//   objective : 0 = edge cut, 1 = communication volume ("vol")
//   balance_slack : allowed imbalance, e.g. 0.05
// Returns int32[N] partition assignment.
torch::Tensor partition_graph_cpu(torch::Tensor indptr, torch::Tensor indices,
                                  int64_t nparts, int64_t objective,
                                  double balance_slack, int64_t n_refine_passes,
                                  int64_t seed);

// CPU CSR SpMM: out[r, :] = scale[r] * sum_{c in row r} feat[indices[c], :]
// scale may be an undefined tensor (no scaling). feat float32 [num_src, F].
torch::Tensor spmm_cpu(torch::Tensor indptr, torch::Tensor indices,
                       torch::Tensor feat, torch::Tensor dst_scale,
                       torch::Tensor src_scale, int64_t num_rows);

// Max aggregation on the CPU (the contract: docs/DESIGN.md, "Max
// aggregation"). out[r,c] = max over the edges of row r of z[indices[e],c],
// arg[r,c] = the source id of the first edge, in stored order, that attains
// it (initialised from the first edge, updated on strict >); rows without
// edges give 0 and -1. z fp32 [num_src, F]. -> {out} or, with_arg, {out, arg}.
std::vector<torch::Tensor> max_aggregate_cpu(torch::Tensor indptr,
                                             torch::Tensor indices,
                                             torch::Tensor z, int64_t num_rows,
                                             bool with_arg);
// grad_z[u,c] = sum of g[r,c] over the rows r with arg[r,c] == u: a scatter
// of g by arg, serial over r inside each column block (deterministic, every
// destination counted once). g fp32 [rows, F], arg int32 [rows, F] with
// entries in [-1, num_src). -> fp32 [num_src, F].
torch::Tensor max_aggregate_bwd_cpu(torch::Tensor g, torch::Tensor arg,
                                    int64_t num_src);

// The CSR with each row's repeated entries removed (rows come out sorted),
// parallel over rows. -> {indptr, indices, removed}: removed is a bool scalar
// tensor; when it is false the first two are the inputs themselves.
std::vector<torch::Tensor> csr_simple(torch::Tensor indptr,
                                      torch::Tensor indices);

// ---------------------------------------------------------------------------
// HIP kernel launchers (hip/*.hip) — gfx950 only.
// ---------------------------------------------------------------------------

// Elements per lane access of the wave-per-(row, chunk) gathers for rows of F
// elements of elem_size bytes: 8-byte accesses first (16-byte first from 2^20
// rows on), PIPEGCN_SPMM_VEC overrides. Always divides F. (hip/kernels.hip)
int pick_vec(int64_t F, int64_t num_rows, int64_t elem_size = 4);

// Max aggregation (hip/spmm_max.hip): max_aggregate_cpu's contract for fp32 or
// bf16 z [>= num_cols, F]; comparison in fp32, the result is one of the
// inputs. -> {out} or, with_arg, {out, arg int32 [num_rows, F]}.
std::vector<torch::Tensor> spmm_max_fwd_hip(torch::Tensor indptr,
                                            torch::Tensor indices,
                                            torch::Tensor z,
                                            torch::Tensor row_order,
                                            int64_t num_cols, bool with_arg);
// Its backward; indptr/indices/row_order are a CSC WITHOUT repeated entries
// (rows = sources u, columns = destinations r < num_cols): grad_z[u,c] = sum
// over the entries r of row u of g[r,c] where arg[r,c] == u, fp32 accumulate.
// g fp32 or bf16 [>= num_cols, F], arg int32 of the same shape.
// -> [num_rows, F] in g's dtype.
torch::Tensor spmm_max_bwd_hip(torch::Tensor indptr, torch::Tensor indices,
                               torch::Tensor g, torch::Tensor arg,
                               torch::Tensor row_order, int64_t num_cols);

// out[r,:] = scale[r] * sum_{e in [indptr[r], indptr[r+1])} feat[indices[e],:]
// All tensors on device. feat fp32 [num_src, F], out fp32 [num_rows, F].
// n_live (optional: undefined or empty is none; not with src_scale): one int32
// in device memory, read by the kernel. The caller guarantees that the rows of
// feat from *n_live on are all zero; their gathers are then redirected to row
// *n_live. The result is bitwise the one without it.
// Epilogue (optional, not with dst_scale): add_rows [>= n_add, F] in feat's
// dtype, unit column stride and any row stride, is added to output rows
// r < n_add; drop_mask, the uint8 bit mask dropout_fwd_hip writes over a
// [num_rows, F] tensor, then zeroes the elements whose bit is clear and
// multiplies the others by drop_scale. Bitwise dropout_bwd_hip of the eager
// sum of the plain result and the zero-padded add_rows.
void spmm_csr_hip(torch::Tensor indptr, torch::Tensor indices,
                  torch::Tensor feat, torch::Tensor dst_scale,
                  torch::Tensor src_scale, torch::Tensor row_order,
                  torch::Tensor out, torch::Tensor n_live = {},
                  torch::Tensor add_rows = {}, int64_t n_add = 0,
                  torch::Tensor drop_mask = {}, double drop_scale = 1.0);

// scaled[r,:] = g[r,:] * inv[r] (for bf16, inv rounded to bf16 first, as the
// eager product rounds it), and in the same pass *n_live = 1 + the largest r
// with any scaled[r,c] != 0, or 0 (both zeros are zero, NaN and Inf are not).
// g fp32 or bf16 [N, F] with unit column stride (rows may be strided), inv
// fp32 [N]; scaled is contiguous, n_live one int32, zeroed here.
void scale_rows_live_hip(torch::Tensor g, torch::Tensor inv,
                         torch::Tensor scaled, torch::Tensor n_live);

// Edge dropout (csrc/hip/spmm_drop.hip): spmm_csr_hip over the kept edges
// only, times drop_scale = 1 / (1 - p). The edge of row r and gathered id c
// is kept when the attention-dropout hash with one head (hip/attn_util.h) of
// (u, v) = (c, r), or (r, c) if `transposed` (the CSC pass), is at least
// drop_thr; drop_key and drop_thr are 32-bit values, drop_thr == 0 keeps
// every edge. A dropped edge issues no gather. The other arguments and their
// checks are spmm_csr_hip's; indices must be 16-byte aligned.
void spmm_drop_hip(torch::Tensor indptr, torch::Tensor indices,
                   torch::Tensor feat, torch::Tensor dst_scale,
                   torch::Tensor src_scale, torch::Tensor row_order,
                   torch::Tensor out, torch::Tensor n_live, bool transposed,
                   int64_t drop_key, int64_t drop_thr, double drop_scale);

// Packed rows (csrc/hip/spmm_packed.hip): one fixed-stride record per row of a
// fp32 [N, F] tensor, in 4-byte words: mask_words header entries {uint32 mask,
// uint32 exclusive prefix count} (one per 32 columns), padding up to hdr_words
// (a multiple of 4), then the row's non-zero values in column order. Row u
// starts at word u * stride_words (a multiple of 32).
struct PackedLayout {
  int64_t mask_words;
  int64_t hdr_words;
  int64_t stride_words;
};
PackedLayout packed_layout(int64_t F);
// packed: int32 [N, stride_words], written for every row of x (fp32 [N, F]);
// padding and the value slots past a row's non-zero count stay unwritten.
void pack_rows_hip(torch::Tensor x, torch::Tensor packed);
// spmm_csr_hip over packed rows (fp32, no src_scale): bitwise the result of
// the dense kernel on the tensor the rows were packed from. The caller
// guarantees that every column index is below packed.size(0).
void spmm_packed_hip(torch::Tensor indptr, torch::Tensor indices,
                     torch::Tensor packed, int64_t F, torch::Tensor dst_scale,
                     torch::Tensor row_order, torch::Tensor out);

// out[i,:] = src[idx[i],:]
void gather_rows_hip(torch::Tensor src, torch::Tensor idx, torch::Tensor out);

// dst[idx[i],:] += src[i,:]. Contract: idx entries are unique — one wave
// owns each row and no atomics are used, so duplicates would race.
void scatter_add_rows_hip(torch::Tensor dst, torch::Tensor idx,
                          torch::Tensor src);

// avg = momentum * avg + (1 - momentum) * x
void ema_update_hip(torch::Tensor avg, torch::Tensor x, double momentum);

// out[n] = sum_m x[m, n] — fast column reduction for bias/BN grads.
torch::Tensor colsum_hip(torch::Tensor x);

// Fused dropout with a bitpacked mask (1 bit/elem): y = mask ? x/(1-p) : 0.
// mask uint8[(n+7)/8]; seed drives a counter-based RNG (reproducible).
void dropout_fwd_hip(torch::Tensor x, torch::Tensor y, torch::Tensor mask,
                     double p, int64_t seed);
void dropout_bwd_hip(torch::Tensor dy, torch::Tensor mask, torch::Tensor dx,
                     double p);

// Fused LayerNorm [+ReLU]: y = [relu](w * xhat + b), xhat/rstd saved for
// backward (wave-per-row, fp32 statistics, F <= 1024).
void layer_norm_relu_fwd_hip(torch::Tensor x, torch::Tensor w,
                             torch::Tensor b, double eps, bool relu,
                             torch::Tensor y, torch::Tensor xhat,
                             torch::Tensor rstd);
// fused dual data gradient: {g @ w1, g @ w2} via MFMA
// (csrc/hip/dual_dgrad.hip)
std::vector<torch::Tensor> dual_dgrad_hip(torch::Tensor g, torch::Tensor w1,
                                          torch::Tensor w2);

// fused dual weight gradient: {g^T x1 [, g^T x2]} via MFMA split-M
// (csrc/hip/wgrad.hip); pass an undefined x2 for the single-wgrad case
std::vector<torch::Tensor> dual_wgrad_hip(torch::Tensor g, torch::Tensor x1,
                                          torch::Tensor x2);

// dw_part/db_part: fp32 [nwaves, F] per-wave partials (column-sum on host).
void layer_norm_relu_bwd_hip(torch::Tensor dy, torch::Tensor xhat,
                             torch::Tensor rstd, torch::Tensor w,
                             torch::Tensor b, bool relu, torch::Tensor dx,
                             torch::Tensor dw_part, torch::Tensor db_part);

// GAT edge-softmax aggregation (csrc/hip/gat.hip). Attention weights are
// recomputed from per-node state, alpha_uv = exp(leaky_relu(el[u] + er[v]) -
// lse[v]); nothing of size nnz is allocated. z/g/out/zc/dz are fp32 or bf16
// [nodes, F] with F = H * D; el/er/lse/csum/t/d_el are fp32 [nodes, H].
// num_cols is the number of nodes the column indices may reference.
//
// lse[v,h] = log sum_{u in N(v)} exp(leaky_relu(el[u,h] + er[v,h])); rows
// without edges get 0.
torch::Tensor gat_row_stats_hip(torch::Tensor indptr, torch::Tensor indices,
                                torch::Tensor el, torch::Tensor er,
                                int64_t num_cols, double slope);
// -> {out} or, with_aux, {out, zc, csum}: out[v] = sum_u alpha_uv z[u],
// zc[v] = sum_u c_uv z[u], csum[v,h] = sum_u c_uv, c = alpha * leaky_relu'.
//
// Attention dropout: drop_thr > 0 multiplies alpha in out/dz and c in zc/gc
// by keep(drop_key, u, v, h) * drop_scale, where keep = hash >= drop_thr is
// recomputed per edge and head from the endpoint ids (gat.hip); csum and the
// backward's sum_v c*t stay unmasked. drop_key and drop_thr are 32-bit
// values, drop_scale = 1 / (1 - p). drop_thr == 0 is today's code path.
std::vector<torch::Tensor> gat_aggregate_fwd_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor z,
    torch::Tensor el, torch::Tensor er, torch::Tensor lse,
    torch::Tensor row_order, int64_t num_cols, int64_t H, double slope,
    bool with_aux, int64_t drop_key, int64_t drop_thr, double drop_scale);
// Transpose pass; indptr/indices/row_order are the CSC (rows = sources).
// t[v,h] = g[v,h,:] . out[v,h,:]. -> {dz, d_el}.
std::vector<torch::Tensor> gat_aggregate_bwd_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor g,
    torch::Tensor z, torch::Tensor el, torch::Tensor er, torch::Tensor lse,
    torch::Tensor t, torch::Tensor row_order, int64_t num_cols, int64_t H,
    double slope, int64_t drop_key, int64_t drop_thr, double drop_scale);
// keep[i, h] of the edge u[i] -> v[i] (int32 ids, hashed as uint32) for the
// 62-bit seed and rate p, computed by the kernels' device function: a probe
// for comparing it with ops.gat_dropout_keep. -> bool [n, H].
torch::Tensor gat_dropout_keep_hip(torch::Tensor u, torch::Tensor v, int64_t H,
                                   int64_t seed, double p);

// GATv2 (dynamic attention) aggregation (csrc/hip/gatv2.hip):
//   s_uvh = sum_{f in head h} attn[h,f] * leaky_relu(zl[u,f] + zr[v,f]),
//   alpha = softmax_u(s), out[v] = sum_u w * alpha * zl[u].
// Every pass recomputes s from the gathered rows; nothing of size nnz is
// allocated. zl/zr/g/out/d_zl/d_zr are fp32 or bf16 [nodes, F] with F = H * D
// and D <= 1024; attn is fp32 [H, D]; lse/t are fp32 [nodes, H]. The drop_*
// arguments are those of gat_aggregate_fwd_hip (drop_thr == 0: no dropout).
// -> {out, lse}; rows without edges get 0 and 0.
std::vector<torch::Tensor> gatv2_fwd_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor zl,
    torch::Tensor zr, torch::Tensor attn, torch::Tensor row_order,
    int64_t num_cols, int64_t H, double slope, int64_t drop_key,
    int64_t drop_thr, double drop_scale);
// Destination-side backward over the CSR, t[v,h] = g[v,h,:] . out[v,h,:].
// -> {d_zr, pa}: pa is fp32 [num_rows, F] and d_attn is its column sum.
std::vector<torch::Tensor> gatv2_bwd_dst_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor g,
    torch::Tensor zl, torch::Tensor zr, torch::Tensor attn, torch::Tensor lse,
    torch::Tensor t, torch::Tensor row_order, int64_t num_cols, int64_t H,
    double slope, int64_t drop_key, int64_t drop_thr, double drop_scale);
// Source-side backward; indptr/indices/row_order are the CSC (rows =
// sources, num_cols = destinations). -> d_zl [num_rows, F].
torch::Tensor gatv2_bwd_src_hip(
    torch::Tensor indptr, torch::Tensor indices, torch::Tensor g,
    torch::Tensor zl, torch::Tensor zr, torch::Tensor attn, torch::Tensor lse,
    torch::Tensor t, torch::Tensor row_order, int64_t num_cols, int64_t H,
    double slope, int64_t drop_key, int64_t drop_thr, double drop_scale);

// Fused dual GEMM for the GraphSAGE layer forward:
//   out[M,N] = x1[M,K] @ w1[N,K]^T + x2[M,K] @ w2[N,K]^T + bias[N]
// fp32, MFMA (v_mfma_f32_32x32x2_f32). Weights in torch Linear layout [N,K],
// not pre-transposed; an empty bias tensor means no bias.
void sage_dual_gemm_hip(torch::Tensor x1, torch::Tensor x2, torch::Tensor w1,
                        torch::Tensor w2, torch::Tensor bias,
                        torch::Tensor out);
