"""GAT model (multi-head attention aggregation) — a capability extension over
the reference, which has no attention model (its `create_model` supports
only graphsage).

Layer, H heads of width D = out_feats / H, LeakyReLU slope 0.2:

    z     = h W^T                         on ALL local rows (inner + halo)
    el[u] = <z[u,h,:], a_l[h]>,  er[v] = <z[v,h,:], a_r[h]>
    alpha = softmax over u in N(v) of leaky_relu(el[u] + er[v])   (per head)
    out[v] = sum_u alpha_uv z[u] + b

In training, `attn_drop` > 0 drops each alpha_uv (per head) with that
probability and scales the rest by 1 / (1 - attn_drop); evaluation never
drops. The mask is recomputed inside the kernels from a hash of the edge's
endpoints and a per-call seed drawn from torch's host generator.

The aggregation is `ops.gat_aggregate` (csrc/hip/gat.hip): alpha is
recomputed from per-node state wherever it is needed, so no [nnz, H] tensor
exists on the GPU in forward or backward (docs/DESIGN.md). Gradients reach
the halo rows of h through z and el; the buffer's existing backward path
ships them, so `ctx.buffer.update` stays the only distributed seam.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import FullGraph, HaloGraph
from pipegcn_amd.models.sage import GNNBase

NEGATIVE_SLOPE = 0.2


class GATLayer(nn.Module):
    def __init__(self, in_feats, out_feats, num_heads=1, bias=True,
                 attn_drop=0.0):
        super().__init__()
        if not 0.0 <= attn_drop < 1.0:
            raise ValueError(f"attn_drop={attn_drop} is outside [0, 1)")
        self.attn_drop = attn_drop
        if num_heads < 1 or out_feats % num_heads != 0:
            raise ValueError(
                f"GAT layer width {out_feats} is not divisible by "
                f"{num_heads} heads (--n-hidden must be a multiple of "
                "--n-heads)")
        self.num_heads = num_heads
        self.head_dim = out_feats // num_heads
        self.linear = nn.Linear(in_feats, out_feats, bias=False)
        self.attn_l = nn.Parameter(torch.empty(num_heads, self.head_dim))
        self.attn_r = nn.Parameter(torch.empty(num_heads, self.head_dim))
        self.bias = nn.Parameter(torch.empty(out_feats)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        # the project's uniform +-1/sqrt(fan_in); fan_in = D for a_l / a_r
        stdv = 1.0 / math.sqrt(self.linear.weight.size(1))
        self.linear.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.uniform_(-stdv, stdv)
        stdv_a = 1.0 / math.sqrt(self.head_dim)
        self.attn_l.data.uniform_(-stdv_a, stdv_a)
        self.attn_r.data.uniform_(-stdv_a, stdv_a)

    def _scores(self, z, attn):
        return (z.view(z.shape[0], self.num_heads, self.head_dim)
                * attn).sum(-1)

    def forward(self, graph, feat, in_deg=None):
        z = self.linear(feat)
        el = self._scores(z, self.attn_l)
        if self.training:
            assert isinstance(graph, HaloGraph)
            er = self._scores(z[: graph.num_in], self.attn_r)
            out = ops.gat_aggregate(graph, z, el, er, self.num_heads,
                                    NEGATIVE_SLOPE, self.attn_drop)
        else:
            # eval: full homogeneous graph, every node is a destination
            assert isinstance(graph, FullGraph)
            er = self._scores(z, self.attn_r)
            out = ops.gat_aggregate_csr(graph.csr, z, el, er,
                                        self.num_heads, NEGATIVE_SLOPE)
        if self.bias is None:
            return out
        return ops.add_bias(out, self.bias)


class GAT(GNNBase):
    """Same structure as GCN: conv layers then linear tail, norm+ReLU
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
        return GATLayer(in_feats, out_feats, num_heads=heads,
                        attn_drop=attn_drop)
