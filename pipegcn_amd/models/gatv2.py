"""GATv2 model (dynamic multi-head attention, Brody et al., ICLR'22) — a
capability extension over the reference, which has no attention model.

Layer, H heads of width D = out_feats / H, LeakyReLU slope 0.2:

    zl = h W_l^T                 on ALL local rows (inner + halo)
    zr = h[:num_in] W_r^T        on destination rows only
    s_uvh = <a[h], leaky_relu(zl[u,h,:] + zr[v,h,:])>
    alpha = softmax over u in N(v) of s_uvh            (per head)
    out[v] = sum_u alpha_uv zl[u] + b

GAT applies the nonlinearity to a sum of two per-node scalars, so its
ranking of the sources is the same for every destination; here it sits
inside the dot product, and the ranking depends on the destination.

In training, `attn_drop` > 0 drops each alpha_uv (per head) with that
probability and scales the rest by 1 / (1 - attn_drop); evaluation never
drops. The mask is the GAT one: a hash of the edge's endpoints and a per-call
seed drawn from torch's host generator, recomputed inside the kernels.

The aggregation is `ops.gatv2_aggregate` (csrc/hip/gatv2.hip): the score is
recomputed per edge from the gathered rows wherever it is needed, so no
[nnz, H] or [nnz, H, D] tensor exists on the GPU in forward or backward
(docs/DESIGN.md). Gradients reach the halo rows of h through d_zl into
`linear_l`; the buffer's existing backward path ships them, so
`ctx.buffer.update` stays the only distributed seam.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import FullGraph, HaloGraph
from pipegcn_amd.models.gat import NEGATIVE_SLOPE
from pipegcn_amd.models.sage import GNNBase


class GATv2Layer(nn.Module):
    def __init__(self, in_feats, out_feats, num_heads=1, bias=True,
                 attn_drop=0.0):
        super().__init__()
        if not 0.0 <= attn_drop < 1.0:
            raise ValueError(f"attn_drop={attn_drop} is outside [0, 1)")
        self.attn_drop = attn_drop
        if num_heads < 1 or out_feats % num_heads != 0:
            raise ValueError(
                f"GATv2 layer width {out_feats} is not divisible by "
                f"{num_heads} heads (--n-hidden must be a multiple of "
                "--n-heads)")
        self.num_heads = num_heads
        self.head_dim = out_feats // num_heads
        self.linear_l = nn.Linear(in_feats, out_feats, bias=False)
        self.linear_r = nn.Linear(in_feats, out_feats, bias=False)
        self.attn = nn.Parameter(torch.empty(num_heads, self.head_dim))
        self.bias = nn.Parameter(torch.empty(out_feats)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        # the project's uniform +-1/sqrt(fan_in); fan_in = D for attn
        stdv = 1.0 / math.sqrt(self.linear_l.weight.size(1))
        self.linear_l.weight.data.uniform_(-stdv, stdv)
        self.linear_r.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.uniform_(-stdv, stdv)
        stdv_a = 1.0 / math.sqrt(self.head_dim)
        self.attn.data.uniform_(-stdv_a, stdv_a)

    def forward(self, graph, feat, in_deg=None):
        zl = self.linear_l(feat)
        if self.training:
            assert isinstance(graph, HaloGraph)
            zr = self.linear_r(feat[: graph.num_in])
            out = ops.gatv2_aggregate(graph, zl, zr, self.attn,
                                      self.num_heads, NEGATIVE_SLOPE,
                                      self.attn_drop)
        else:
            # eval: full homogeneous graph, every node is a destination
            assert isinstance(graph, FullGraph)
            zr = self.linear_r(feat)
            out = ops.gatv2_aggregate_csr(graph.csr, zl, zr, self.attn,
                                          self.num_heads, NEGATIVE_SLOPE)
        if self.bias is None:
            return out
        return ops.add_bias(out, self.bias)


class GATv2(GNNBase):
    """Same structure as GAT: conv layers then linear tail, norm+ReLU
    between layers, `ctx.buffer.update` as the only distributed seam.

    Hidden conv layers use `n_heads` heads, concatenated; a conv layer that
    is the model's last layer uses a single head (its width is n_class).
    """

    def __init__(self, layer_size, activation, use_pp=False, dropout=0.5,
                 norm="layer", train_size=None, n_linear=0, n_heads=1,
                 attn_drop=0.0):
        if use_pp:
            raise NotImplementedError("--use-pp supports graphsage only "
                                      "(reference parity)")
        super().__init__(layer_size, activation, dropout, norm, train_size,
                         n_linear, n_heads=n_heads, attn_drop=attn_drop)

    def make_conv(self, i, in_feats, out_feats, n_heads, attn_drop):
        heads = 1 if i == self.n_layers - 1 else n_heads
        return GATv2Layer(in_feats, out_feats, num_heads=heads,
                          attn_drop=attn_drop)
