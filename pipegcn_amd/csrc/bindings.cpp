// pybind bindings + device dispatch for pipegcn_amd._C.
//
// On device tensors every op goes to the hand-written gfx950 HIP kernels in
// hip/kernels.hip — there is NO silent eager fallback on GPU: if this
// extension is missing on a GPU box, the Python ops raise (see
// pipegcn_amd/ops/__init__.py). CPU tensors use the native C++ paths in
// graph_core.cpp (used by the CPU test tier and rank-0 full-graph eval).

#include "common.h"

#include <optional>

static torch::Tensor spmm(torch::Tensor indptr, torch::Tensor indices,
                          torch::Tensor feat, torch::Tensor dst_scale,
                          torch::Tensor src_scale, torch::Tensor row_order,
                          int64_t num_rows,
                          std::optional<torch::Tensor> n_live,
                          std::optional<torch::Tensor> add_rows,
                          int64_t n_add,
                          std::optional<torch::Tensor> drop_mask,
                          double drop_scale) {
  if (feat.is_cuda()) {
    auto out = torch::empty({num_rows, feat.size(1)}, feat.options());
    spmm_csr_hip(indptr, indices, feat, dst_scale, src_scale, row_order,
                 out, n_live.value_or(torch::Tensor()),
                 add_rows.value_or(torch::Tensor()), n_add,
                 drop_mask.value_or(torch::Tensor()), drop_scale);
    return out;
  }
  TORCH_CHECK(!add_rows.has_value() && !drop_mask.has_value(),
              "spmm: the add/dropout epilogue is the GPU path");
  // n_live only saves the GPU kernel memory traffic: the CPU result is the
  // same with or without it
  if (feat.scalar_type() == torch::kBFloat16) {
    // CPU tier computes in fp32 (the CPU path serves tests + rank-0 eval)
    return spmm_cpu(indptr, indices, feat.to(torch::kFloat), dst_scale,
                    src_scale, num_rows)
        .to(torch::kBFloat16);
  }
  return spmm_cpu(indptr, indices, feat, dst_scale, src_scale, num_rows);
}

// GPU-only: ops.spmm_drop composes the CPU path from torch ops
static torch::Tensor spmm_drop(torch::Tensor indptr, torch::Tensor indices,
                               torch::Tensor feat, torch::Tensor dst_scale,
                               torch::Tensor src_scale,
                               torch::Tensor row_order, int64_t num_rows,
                               bool transposed, int64_t drop_key,
                               int64_t drop_thr, double drop_scale,
                               std::optional<torch::Tensor> n_live) {
  TORCH_CHECK(feat.is_cuda() && feat.dim() == 2,
              "spmm_drop is the GPU path");
  auto out = torch::empty({num_rows, feat.size(1)}, feat.options());
  spmm_drop_hip(indptr, indices, feat, dst_scale, src_scale, row_order, out,
                n_live.value_or(torch::Tensor()), transposed, drop_key,
                drop_thr, drop_scale);
  return out;
}

// -> [out] or, with_arg, [out, arg]
static std::vector<torch::Tensor> spmm_max(torch::Tensor indptr,
                                           torch::Tensor indices,
                                           torch::Tensor z,
                                           torch::Tensor row_order,
                                           int64_t num_rows, int64_t num_cols,
                                           bool with_arg) {
  TORCH_CHECK(indptr.numel() == num_rows + 1,
              "spmm_max: indptr must hold num_rows + 1 entries");
  if (z.is_cuda())
    return spmm_max_fwd_hip(indptr, indices, z, row_order, num_cols, with_arg);
  TORCH_CHECK(z.dim() == 2 && z.size(0) >= num_cols, "spmm_max: z has ",
              z.size(0), " rows but the graph references ", num_cols);
  if (z.scalar_type() == torch::kBFloat16) {
    // the CPU tier compares in fp32; the maximum is one of the inputs, so
    // the way back to bf16 is exact
    auto res = max_aggregate_cpu(indptr, indices, z.to(torch::kFloat),
                                 num_rows, with_arg);
    res[0] = res[0].to(torch::kBFloat16);
    return res;
  }
  return max_aggregate_cpu(indptr, indices, z, num_rows, with_arg);
}

// GPU: gather over the simple CSC (rows = the num_src sources). CPU: a
// scatter of g by arg, which needs no graph (pass empty tensors).
static torch::Tensor spmm_max_bwd(torch::Tensor indptr, torch::Tensor indices,
                                  torch::Tensor g, torch::Tensor arg,
                                  torch::Tensor row_order, int64_t num_src,
                                  int64_t num_cols) {
  if (g.is_cuda()) {
    TORCH_CHECK(indptr.numel() == num_src + 1,
                "spmm_max_bwd: indptr must hold num_src + 1 entries");
    return spmm_max_bwd_hip(indptr, indices, g, arg, row_order, num_cols);
  }
  if (g.scalar_type() == torch::kBFloat16)
    return max_aggregate_bwd_cpu(g.to(torch::kFloat), arg, num_src)
        .to(torch::kBFloat16);
  return max_aggregate_bwd_cpu(g, arg, num_src);
}

// GPU-only (ops._SpmmMean.backward multiplies eagerly on the CPU)
static std::vector<torch::Tensor> scale_rows_live(torch::Tensor g,
                                                  torch::Tensor inv) {
  TORCH_CHECK(g.is_cuda() && g.dim() == 2,
              "scale_rows_live is the GPU path");
  if (g.size(0) > 1 && g.size(1) > 1 && g.stride(1) != 1) g = g.contiguous();
  auto scaled = torch::empty({g.size(0), g.size(1)}, g.options());
  auto n_live = torch::empty({1}, g.options().dtype(torch::kInt));
  scale_rows_live_hip(g, inv, scaled, n_live);
  return {scaled, n_live};
}

// GPU-only: ops.pack_rows_reference is the torch mirror of the layout
static torch::Tensor pack_rows(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2, "pack_rows is the GPU path");
  auto packed = torch::empty({x.size(0), packed_layout(x.size(1)).stride_words},
                             x.options().dtype(torch::kInt));
  pack_rows_hip(x, packed);
  return packed;
}

static torch::Tensor spmm_packed(torch::Tensor indptr, torch::Tensor indices,
                                 torch::Tensor packed, int64_t F,
                                 torch::Tensor dst_scale,
                                 torch::Tensor row_order, int64_t num_rows) {
  TORCH_CHECK(packed.is_cuda(), "spmm_packed is the GPU path");
  auto out = torch::empty({num_rows, F},
                          packed.options().dtype(torch::kFloat));
  spmm_packed_hip(indptr, indices, packed, F, dst_scale, row_order, out);
  return out;
}

static torch::Tensor gather_rows(torch::Tensor src, torch::Tensor idx) {
  if (src.is_cuda()) {
    auto out = torch::empty({idx.numel(), src.size(1)}, src.options());
    gather_rows_hip(src, idx, out);
    return out;
  }
  return src.index_select(0, idx);
}

static void gather_rows_out(torch::Tensor src, torch::Tensor idx,
                            torch::Tensor out) {
  if (src.is_cuda()) {
    gather_rows_hip(src, idx, out);
  } else {
    torch::index_select_out(out, src, 0, idx);
  }
}

static void scatter_add_rows(torch::Tensor dst, torch::Tensor idx,
                             torch::Tensor src) {
  if (dst.is_cuda()) {
    scatter_add_rows_hip(dst, idx, src);
  } else {
    dst.index_add_(0, idx, src);
  }
}

static torch::Tensor sage_dual_gemm(torch::Tensor x1, torch::Tensor x2,
                                    torch::Tensor w1, torch::Tensor w2,
                                    torch::Tensor bias) {
  if (x1.is_cuda()) {
    auto out = torch::empty({x1.size(0), w1.size(0)}, x1.options());
    sage_dual_gemm_hip(x1, x2, w1, w2, bias, out);
    return out;
  }
  auto out = torch::mm(x1, w1.t());
  out.addmm_(x2, w2.t());
  if (bias.defined() && bias.numel() > 0) out.add_(bias);
  return out;
}

static torch::Tensor colsum(torch::Tensor x) {
  if (x.is_cuda()) {
    if (x.scalar_type() == torch::kBFloat16)
      return colsum_hip(x.to(torch::kFloat)).to(torch::kBFloat16);
    return colsum_hip(x);
  }
  return x.sum(0);
}

// GPU-only fused ops (the Python wrappers fall back to eager torch on CPU)

static std::vector<torch::Tensor> dropout_fwd(torch::Tensor x, double p,
                                              int64_t seed) {
  TORCH_CHECK(x.is_cuda(), "fused dropout is the GPU path");
  auto y = torch::empty_like(x);
  auto mask = torch::empty({(x.numel() + 7) / 8},
                           x.options().dtype(torch::kUInt8));
  dropout_fwd_hip(x, y, mask, p, seed);
  return {y, mask};
}

static torch::Tensor dropout_bwd(torch::Tensor dy, torch::Tensor mask,
                                 double p) {
  auto dx = torch::empty_like(dy);
  dropout_bwd_hip(dy.contiguous(), mask, dx, p);
  return dx;
}

static std::vector<torch::Tensor> layer_norm_relu_fwd(torch::Tensor x,
                                                      torch::Tensor w,
                                                      torch::Tensor b,
                                                      double eps, bool relu) {
  TORCH_CHECK(x.is_cuda(), "fused layer_norm_relu is the GPU path");
  auto y = torch::empty_like(x);
  auto xhat = torch::empty_like(x);
  auto rstd = torch::empty({x.size(0)}, x.options().dtype(torch::kFloat));
  layer_norm_relu_fwd_hip(x.contiguous(), w, b, eps, relu, y, xhat, rstd);
  return {y, xhat, rstd};
}

static std::vector<torch::Tensor> layer_norm_relu_bwd(
    torch::Tensor dy, torch::Tensor xhat, torch::Tensor rstd,
    torch::Tensor w, torch::Tensor b, bool relu) {
  auto dx = torch::empty_like(dy);
  const int64_t N = dy.size(0);
  const int64_t F = dy.size(1);
  const int64_t nblk = std::min<int64_t>(1024, (N + 3) / 4);
  auto dw_part = torch::empty({nblk * 4, F},
                              dy.options().dtype(torch::kFloat));
  auto db_part = torch::empty_like(dw_part);
  layer_norm_relu_bwd_hip(dy.contiguous(), xhat, rstd, w, b, relu, dx,
                          dw_part, db_part);
  return {dx, colsum_hip(dw_part), colsum_hip(db_part)};
}

static void ema_update(torch::Tensor avg, torch::Tensor x, double momentum) {
  if (avg.is_cuda()) {
    ema_update_hip(avg, x, momentum);
  } else {
    avg.mul_(momentum).add_(x, 1.0 - momentum);
  }
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "pipegcn_amd native core (gfx950 HIP kernels + host graph ops)";
  m.def("build_csr", &build_csr, "COO -> CSR (counting sort by dst)");
  m.def("partition_graph", &partition_graph_cpu,
        "BFS-grown + refined k-way partitioner (cut/vol objective)");
  // n_live and the add/dropout epilogue trail with defaults: calls without
  // them run what they ran before
  m.def("spmm", &spmm, "CSR SpMM with fused scale epilogue (fwd & transpose)",
        py::arg("indptr"), py::arg("indices"), py::arg("feat"),
        py::arg("dst_scale"), py::arg("src_scale"), py::arg("row_order"),
        py::arg("num_rows"), py::arg("n_live") = py::none(),
        py::arg("add_rows") = py::none(), py::arg("n_add") = 0,
        py::arg("drop_mask") = py::none(), py::arg("drop_scale") = 1.0);
  m.def("spmm_drop", &spmm_drop,
        "CSR SpMM over the edges the edge-dropout hash keeps, times "
        "drop_scale",
        py::arg("indptr"), py::arg("indices"), py::arg("feat"),
        py::arg("dst_scale"), py::arg("src_scale"), py::arg("row_order"),
        py::arg("num_rows"), py::arg("transposed"), py::arg("drop_key"),
        py::arg("drop_thr"), py::arg("drop_scale"),
        py::arg("n_live") = py::none());
  m.def("csr_simple", &csr_simple,
        "CSR without repeated entries in a row -> (indptr, indices, removed)");
  m.def("spmm_max", &spmm_max,
        "max aggregation over the CSR -> [out] or [out, arg]",
        py::arg("indptr"), py::arg("indices"), py::arg("z"),
        py::arg("row_order"), py::arg("num_rows"), py::arg("num_cols"),
        py::arg("with_arg"));
  m.def("spmm_max_bwd", &spmm_max_bwd,
        "grad_z of the max aggregation (GPU: over the simple CSC)",
        py::arg("indptr"), py::arg("indices"), py::arg("g"), py::arg("arg"),
        py::arg("row_order"), py::arg("num_src"), py::arg("num_cols"));
  m.def("scale_rows_live", &scale_rows_live,
        "g * inv per row -> (scaled, n_live = 1 + last non-zero row, int32)");
  m.def("pack_rows", &pack_rows,
        "fp32 [N, F] -> packed rows int32 [N, stride_words]");
  m.def("spmm_packed", &spmm_packed,
        "CSR SpMM over packed rows (fp32, dst_scale epilogue)");
  m.def("gather_rows", &gather_rows, "out[i,:] = src[idx[i],:]");
  m.def("gather_rows_out", &gather_rows_out,
        "gather into a preallocated out buffer");
  m.def("scatter_add_rows", &scatter_add_rows, "dst[idx[i],:] += src[i,:]");
  m.def("ema_update", &ema_update, "avg = m*avg + (1-m)*x");
  m.def("colsum", &colsum, "out[n] = sum_m x[m,n]");
  m.def("sage_dual_gemm", &sage_dual_gemm,
        "out = x1 @ w1^T + x2 @ w2^T + bias (MFMA fp32, fused)");
  m.def("dual_dgrad", &dual_dgrad_hip,
        "gx1 = g w1, gx2 = g w2 fused MFMA dgrad");
  m.def("dual_wgrad", &dual_wgrad_hip,
        "gw1 = g^T x1 [, gw2 = g^T x2] fused MFMA split-M wgrad");
  m.def("dropout_fwd", &dropout_fwd,
        "fused dropout, bitpacked mask -> (y, mask)");
  m.def("dropout_bwd", &dropout_bwd, "dx = mask ? dy/(1-p) : 0");
  m.def("layer_norm_relu_fwd", &layer_norm_relu_fwd,
        "fused LayerNorm[+ReLU] -> (y, xhat, rstd)");
  m.def("layer_norm_relu_bwd", &layer_norm_relu_bwd,
        "-> (dx, dweight, dbias)");
  // GPU-only: ops.gat_aggregate composes the CPU path from torch ops
  m.def("gat_row_stats", &gat_row_stats_hip,
        "per-destination log-sum-exp of the GAT edge scores -> lse");
  // the attention-dropout arguments trail with defaults: drop_thr = 0 is no
  // dropout, so calls without them run exactly what they ran before
  m.def("gat_aggregate_fwd", &gat_aggregate_fwd_hip,
        "edge-softmax aggregation -> (out[, zc, csum])", py::arg("indptr"),
        py::arg("indices"), py::arg("z"), py::arg("el"), py::arg("er"),
        py::arg("lse"), py::arg("row_order"), py::arg("num_cols"),
        py::arg("num_heads"), py::arg("slope"), py::arg("with_aux"),
        py::arg("drop_key") = 0, py::arg("drop_thr") = 0,
        py::arg("drop_scale") = 1.0);
  m.def("gat_aggregate_bwd", &gat_aggregate_bwd_hip,
        "transpose edge-softmax aggregation over the CSC -> (dz, d_el)",
        py::arg("indptr"), py::arg("indices"), py::arg("g"), py::arg("z"),
        py::arg("el"), py::arg("er"), py::arg("lse"), py::arg("t"),
        py::arg("row_order"), py::arg("num_cols"), py::arg("num_heads"),
        py::arg("slope"), py::arg("drop_key") = 0, py::arg("drop_thr") = 0,
        py::arg("drop_scale") = 1.0);
  m.def("gat_dropout_keep", &gat_dropout_keep_hip,
        "attention-dropout keep bits of explicit (u, v) ids -> bool [n, H]",
        py::arg("u"), py::arg("v"), py::arg("num_heads"), py::arg("seed"),
        py::arg("p"));
  m.def("gatv2_fwd", &gatv2_fwd_hip,
        "GATv2 dynamic-attention aggregation over the CSR -> (out, lse)",
        py::arg("indptr"), py::arg("indices"), py::arg("zl"), py::arg("zr"),
        py::arg("attn"), py::arg("row_order"), py::arg("num_cols"),
        py::arg("num_heads"), py::arg("slope"), py::arg("drop_key") = 0,
        py::arg("drop_thr") = 0, py::arg("drop_scale") = 1.0);
  m.def("gatv2_bwd_dst", &gatv2_bwd_dst_hip,
        "GATv2 backward over the CSR -> (d_zr, pa)", py::arg("indptr"),
        py::arg("indices"), py::arg("g"), py::arg("zl"), py::arg("zr"),
        py::arg("attn"), py::arg("lse"), py::arg("t"), py::arg("row_order"),
        py::arg("num_cols"), py::arg("num_heads"), py::arg("slope"),
        py::arg("drop_key") = 0, py::arg("drop_thr") = 0,
        py::arg("drop_scale") = 1.0);
  m.def("gatv2_bwd_src", &gatv2_bwd_src_hip,
        "GATv2 backward over the CSC -> d_zl", py::arg("indptr"),
        py::arg("indices"), py::arg("g"), py::arg("zl"), py::arg("zr"),
        py::arg("attn"), py::arg("lse"), py::arg("t"), py::arg("row_order"),
        py::arg("num_cols"), py::arg("num_heads"), py::arg("slope"),
        py::arg("drop_key") = 0, py::arg("drop_thr") = 0,
        py::arg("drop_scale") = 1.0);
  m.attr("with_hip") = true;
}
