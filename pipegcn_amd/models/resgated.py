"""Residual gated graph conv model (Bresson & Laurent 2017; PyG's
ResGatedGraphConv, the message function of GatedGCN in "Benchmarking GNNs")
— a capability extension over the reference, which has no gated model.

Layer, at width F = out_feats:

    k  = h[:num_in] W_k^T + b_k      on destination rows only
    qv = h W_qv^T                    on ALL local rows (inner + halo)
    Q = qv[:, :F], V = qv[:, F:]
    s_uv[c] = sigmoid(k[v,c] + Q[u,c])                 (per channel)
    m[v] = inv_deg[v] * sum over u in N(v) of s_uv * V[u]
    out[v] = m[v] + h[v] W_skip^T + b_skip

The edge weight is a per-channel sigmoid gate and is not normalised over the
neighbourhood; repeated edges count as often as they occur. `linear_k`
carries the bias of the gate's pre-activation, so a bias on Q would only add
to it and none exists; `linear_qv` has no bias at all, like the transformer's
`linear_kv`, so the value has none either. There are no edge features
(docs/ROADMAP.md).

Deviation from PyG: m is the MEAN of the gated messages, PyG sums them.
inv_deg = 1 / in_deg.clamp(min=1) is the degree GraphSAGE's mean uses: in
training from the `in_deg` argument, in evaluation from
`graph.in_degrees()`. The benchmark graphs have mean degrees in the hundreds
and every other unnormalised sum in this project is followed by a degree
division. `ops.resgated_aggregate(..., inv_deg=None)` is PyG's sum.

The aggregation is `ops.resgated_aggregate` (csrc/hip/resgated.hip): the gate
is recomputed per edge from the gathered rows wherever it is needed, so no
[nnz, F] tensor exists on the GPU in forward or backward (docs/DESIGN.md,
"Residual gated aggregation"). Q and V come from ONE projection so that its
backward is one GEMM over the kernels' single d_qv. Only h, at the layer's
input width, crosses the halo: gradients reach the halo rows through d_qv
into `linear_qv`, and `ctx.buffer.update` stays the only distributed seam.
"""
from __future__ import annotations

import math

from torch import nn

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import FullGraph, HaloGraph
from pipegcn_amd.models.sage import GNNBase


class ResGatedLayer(nn.Module):
    def __init__(self, in_feats, out_feats):
        super().__init__()
        self.linear_k = nn.Linear(in_feats, out_feats, bias=True)
        self.linear_qv = nn.Linear(in_feats, 2 * out_feats, bias=False)
        self.linear_skip = nn.Linear(in_feats, out_feats, bias=True)
        self.reset_parameters()

    def reset_parameters(self):
        # the project's uniform +-1/sqrt(fan_in), in registration order
        stdv = 1.0 / math.sqrt(self.linear_k.weight.size(1))
        for p in self.parameters():
            p.data.uniform_(-stdv, stdv)

    def forward(self, graph, feat, in_deg=None):
        qv = ops.linear(feat, self.linear_qv)
        if self.training:
            assert isinstance(graph, HaloGraph)
            root = feat[: graph.num_in]
            inv_deg = (1.0 / in_deg.clamp(min=1.0)).contiguous()
            agg = ops.resgated_aggregate(
                graph, ops.linear(root, self.linear_k), qv, inv_deg)
        else:
            # eval: full homogeneous graph, degrees from the graph itself
            assert isinstance(graph, FullGraph) and in_deg is None
            root = feat
            inv_deg = (1.0 / graph.in_degrees().clamp(min=1.0)).contiguous()
            agg = ops.resgated_aggregate_csr(
                graph.csr, ops.linear(root, self.linear_k), qv, inv_deg)
        return agg + ops.linear(root, self.linear_skip)


class ResGated(GNNBase):
    """Same structure as Transformer: conv layers then linear tail,
    norm+ReLU between layers, `ctx.buffer.update` as the only distributed
    seam."""

    def __init__(self, layer_size, activation, use_pp=False, dropout=0.5,
                 norm="layer", train_size=None, n_linear=0):
        if use_pp:
            raise NotImplementedError("--use-pp supports graphsage only "
                                      "(reference parity)")
        super().__init__(layer_size, activation, dropout, norm, train_size,
                         n_linear)

    def make_conv(self, i, in_feats, out_feats):
        return ResGatedLayer(in_feats, out_feats)
