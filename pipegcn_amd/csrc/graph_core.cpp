// Host-side graph core: CSR construction and de-duplication, CPU SpMM, CPU
// max aggregation, and the multi-way graph partitioner.
//
// This replaces the reference's external native layers:
//  - DGL's C++ COO->CSR graph machinery (used via dgl.graph/heterograph at
//    /root/reference/train.py:206-229)
//  - METIS k-way partitioning invoked through
//    dgl.distributed.partition_graph (/root/reference/helper/utils.py:143).
// The partitioner here is our own implementation (METIS is not available in
// this environment): BFS-grown balanced regions + boundary (KL/FM-style)
// refinement with an edge-cut or communication-volume objective, matching the
// reference's `--partition-obj {cut,vol}` surface.

#include "common.h"

#include <ATen/Parallel.h>

#include <algorithm>
#include <deque>
#include <random>

namespace {

template <typename T>
inline const T* data_of(const torch::Tensor& t) {
  return t.data_ptr<T>();
}

}  // namespace

std::vector<torch::Tensor> build_csr(torch::Tensor u, torch::Tensor v,
                                     int64_t num_rows) {
  TORCH_CHECK(u.device().is_cpu() && v.device().is_cpu(),
              "build_csr expects CPU tensors");
  TORCH_CHECK(u.numel() == v.numel(), "u/v length mismatch");
  u = u.contiguous().to(torch::kLong);
  v = v.contiguous().to(torch::kLong);
  const int64_t E = u.numel();
  auto indptr = torch::zeros({num_rows + 1}, torch::kLong);
  auto indices = torch::empty({E}, torch::kInt);
  const int64_t* up = data_of<int64_t>(u);
  const int64_t* vp = data_of<int64_t>(v);
  int64_t* ip = indptr.data_ptr<int64_t>();
  int32_t* xp = indices.data_ptr<int32_t>();

  // counting sort by destination row
  for (int64_t e = 0; e < E; ++e) {
    TORCH_CHECK(vp[e] >= 0 && vp[e] < num_rows, "dst out of range");
    ip[vp[e] + 1]++;
  }
  for (int64_t r = 0; r < num_rows; ++r) ip[r + 1] += ip[r];
  std::vector<int64_t> cursor(ip, ip + num_rows);
  for (int64_t e = 0; e < E; ++e) {
    xp[cursor[vp[e]]++] = static_cast<int32_t>(up[e]);
  }
  return {indptr, indices};
}

torch::Tensor spmm_cpu(torch::Tensor indptr, torch::Tensor indices,
                       torch::Tensor feat, torch::Tensor dst_scale,
                       torch::Tensor src_scale, int64_t num_rows) {
  TORCH_CHECK(feat.dim() == 2 && feat.scalar_type() == torch::kFloat,
              "spmm_cpu: feat must be fp32 [N,F]");
  feat = feat.contiguous();
  const int64_t F = feat.size(1);
  auto out = torch::zeros({num_rows, F}, feat.options());
  const int64_t* ip = indptr.data_ptr<int64_t>();
  const int32_t* xp = indices.data_ptr<int32_t>();
  const float* fp = feat.data_ptr<float>();
  float* op = out.data_ptr<float>();
  const bool has_scale = dst_scale.defined() && dst_scale.numel() > 0;
  auto dsc = has_scale ? dst_scale.contiguous() : dst_scale;
  const float* sp = has_scale ? dsc.data_ptr<float>() : nullptr;
  const bool has_src = src_scale.defined() && src_scale.numel() > 0;
  auto ssc = has_src ? src_scale.contiguous() : src_scale;
  const float* ssp = has_src ? ssc.data_ptr<float>() : nullptr;

  at::parallel_for(0, num_rows, 64, [&](int64_t begin, int64_t end) {
    for (int64_t r = begin; r < end; ++r) {
      float* orow = op + r * F;
      for (int64_t e = ip[r]; e < ip[r + 1]; ++e) {
        const float* frow = fp + static_cast<int64_t>(xp[e]) * F;
        const float sv = ssp ? ssp[xp[e]] : 1.f;
        for (int64_t k = 0; k < F; ++k) orow[k] += sv * frow[k];
      }
      if (has_scale) {
        const float s = sp[r];
        for (int64_t k = 0; k < F; ++k) orow[k] *= s;
      }
    }
  });
  return out;
}

std::vector<torch::Tensor> max_aggregate_cpu(torch::Tensor indptr,
                                             torch::Tensor indices,
                                             torch::Tensor z, int64_t num_rows,
                                             bool with_arg) {
  TORCH_CHECK(z.dim() == 2 && z.scalar_type() == torch::kFloat,
              "max_aggregate_cpu: z must be fp32 [N,F]");
  TORCH_CHECK(indptr.scalar_type() == torch::kLong &&
                  indices.scalar_type() == torch::kInt &&
                  indptr.numel() == num_rows + 1,
              "max_aggregate_cpu: indptr int64[num_rows+1] / indices int32");
  z = z.contiguous();
  indptr = indptr.contiguous();
  indices = indices.contiguous();
  const int64_t F = z.size(1);
  auto out = torch::zeros({num_rows, F}, z.options());
  torch::Tensor arg;
  if (with_arg)
    arg = torch::full({num_rows, F}, -1, z.options().dtype(torch::kInt));
  const int64_t* ip = data_of<int64_t>(indptr);
  const int32_t* xp = data_of<int32_t>(indices);
  const float* zp = data_of<float>(z);
  float* op = out.data_ptr<float>();
  int32_t* ap = with_arg ? arg.data_ptr<int32_t>() : nullptr;
  const int64_t num_src = z.size(0);
  if (indices.numel() > 0)
    TORCH_CHECK(indices.min().item<int32_t>() >= 0 &&
                    indices.max().item<int32_t>() < num_src,
                "max_aggregate_cpu: z has ", num_src,
                " rows but the graph references more");

  at::parallel_for(0, num_rows, 64, [&](int64_t begin, int64_t end) {
    for (int64_t r = begin; r < end; ++r) {
      if (ip[r] == ip[r + 1]) continue;  // out = 0, arg = -1
      float* orow = op + r * F;
      int32_t* arow = ap ? ap + r * F : nullptr;
      // the first edge initialises, later ones replace on strict >
      const int32_t first = xp[ip[r]];
      const float* frow = zp + static_cast<int64_t>(first) * F;
      for (int64_t k = 0; k < F; ++k) orow[k] = frow[k];
      if (arow)
        for (int64_t k = 0; k < F; ++k) arow[k] = first;
      for (int64_t e = ip[r] + 1; e < ip[r + 1]; ++e) {
        const int32_t u = xp[e];
        const float* zrow = zp + static_cast<int64_t>(u) * F;
        if (arow) {
          for (int64_t k = 0; k < F; ++k) {
            if (zrow[k] > orow[k]) {
              orow[k] = zrow[k];
              arow[k] = u;
            }
          }
        } else {
          for (int64_t k = 0; k < F; ++k)
            orow[k] = zrow[k] > orow[k] ? zrow[k] : orow[k];
        }
      }
    }
  });
  if (with_arg) return {out, arg};
  return {out};
}

torch::Tensor max_aggregate_bwd_cpu(torch::Tensor g, torch::Tensor arg,
                                    int64_t num_src) {
  TORCH_CHECK(g.dim() == 2 && g.scalar_type() == torch::kFloat,
              "max_aggregate_bwd_cpu: g must be fp32 [rows,F]");
  TORCH_CHECK(arg.scalar_type() == torch::kInt && arg.sizes() == g.sizes(),
              "max_aggregate_bwd_cpu: arg must be int32 of g's shape");
  g = g.contiguous();
  arg = arg.contiguous();
  const int64_t rows = g.size(0), F = g.size(1);
  auto grad = torch::zeros({num_src, F}, g.options());
  if (arg.numel() > 0)
    TORCH_CHECK(arg.min().item<int32_t>() >= -1 &&
                    arg.max().item<int32_t>() < num_src,
                "max_aggregate_bwd_cpu: arg names a row outside [0, ", num_src,
                ")");
  const float* gp = data_of<float>(g);
  const int32_t* ap = data_of<int32_t>(arg);
  float* dp = grad.data_ptr<float>();
  // a block of columns belongs to one thread, which walks the rows in order:
  // no two threads add into the same element and the sums have a fixed order
  constexpr int64_t kBlock = 16;
  at::parallel_for(0, (F + kBlock - 1) / kBlock, 1,
                   [&](int64_t begin, int64_t end) {
    const int64_t c0 = begin * kBlock, c1 = std::min(end * kBlock, F);
    for (int64_t r = 0; r < rows; ++r) {
      for (int64_t c = c0; c < c1; ++c) {
        const int32_t u = ap[r * F + c];
        if (u >= 0) dp[static_cast<int64_t>(u) * F + c] += gp[r * F + c];
      }
    }
  });
  return grad;
}

std::vector<torch::Tensor> csr_simple(torch::Tensor indptr,
                                      torch::Tensor indices) {
  TORCH_CHECK(indptr.device().is_cpu() && indices.device().is_cpu(),
              "csr_simple expects CPU tensors");
  TORCH_CHECK(indptr.scalar_type() == torch::kLong &&
                  indices.scalar_type() == torch::kInt && indptr.numel() >= 1,
              "csr_simple: indptr int64 / indices int32");
  indptr = indptr.contiguous();
  indices = indices.contiguous();
  const int64_t num_rows = indptr.numel() - 1;
  const int64_t* ip = data_of<int64_t>(indptr);
  TORCH_CHECK(ip[0] == 0 && ip[num_rows] == indices.numel(),
              "csr_simple: indptr does not span indices");

  // each row sorted and made unique at the row's old start, its new length
  // in counts[r + 1]
  auto sorted = indices.clone();
  auto counts = torch::zeros({num_rows + 1}, torch::kLong);
  int32_t* sp = sorted.data_ptr<int32_t>();
  int64_t* cp = counts.data_ptr<int64_t>();
  at::parallel_for(0, num_rows, 256, [&](int64_t begin, int64_t end) {
    for (int64_t r = begin; r < end; ++r) {
      std::sort(sp + ip[r], sp + ip[r + 1]);
      cp[r + 1] = std::unique(sp + ip[r], sp + ip[r + 1]) - (sp + ip[r]);
    }
  });
  for (int64_t r = 0; r < num_rows; ++r) cp[r + 1] += cp[r];
  const bool removed = cp[num_rows] != indices.numel();
  if (!removed) return {indptr, indices, torch::tensor(false)};

  auto simple = torch::empty({cp[num_rows]}, torch::kInt);
  int32_t* op = simple.data_ptr<int32_t>();
  at::parallel_for(0, num_rows, 256, [&](int64_t begin, int64_t end) {
    for (int64_t r = begin; r < end; ++r)
      std::copy(sp + ip[r], sp + ip[r] + (cp[r + 1] - cp[r]), op + cp[r]);
  });
  return {counts, simple, torch::tensor(true)};
}

// The multilevel k-way partitioner lives in partitioner.cpp.
