"""Graph transformer model (UniMP's TransformerConv, Shi et al., IJCAI'21:
scaled dot-product attention over the neighbourhood) — a capability
extension over the reference, which has no attention model.

Layer, H heads of width D = out_feats / H:

    q  = h[:num_in] W_q^T + b_q      on destination rows only
    kv = h W_kv^T                    on ALL local rows (inner + halo); a key
                                     bias would cancel in the softmax
    K = kv[:, :F], V = kv[:, F:]
    s_uvh = <q[v,h,:], K[u,h,:]> / sqrt(D)
    alpha = softmax over u in N(v) of s_uvh            (per head)
    m[v] = sum_u alpha_uv V[u],  r[v] = h[v] W_skip^T + b_skip
    out[v] = m[v] + r[v]

Unlike GAT and GATv2 the aggregated row V[u] is another projection than the
scored row K[u], and the destination's own features enter through the root
weight `linear_skip` and not through a self-loop. There are no edge features
(docs/ROADMAP.md).

With `beta=True` (the published UniMP setting) a learned gate mixes the two
terms instead of adding them:

    beta[v] = sigmoid([r[v] | m[v] | r[v] - m[v]] W_beta^T)    one scalar
    out[v]  = beta[v] r[v] + (1 - beta[v]) m[v]

through `ops.gated_residual` (csrc/hip/gate.hip): one fused pass forward and
one backward, no eager [N, F] op between the aggregation and the output.

In training, `attn_drop` > 0 drops each alpha_uv (per head) with that
probability and scales the rest by 1 / (1 - attn_drop); evaluation never
drops. The mask is the GAT one: a hash of the edge's endpoints and a per-call
seed drawn from torch's host generator, recomputed inside the kernels.

The aggregation is `ops.dot_aggregate` (csrc/hip/dot_attn.hip): the score is
recomputed per edge from the gathered rows wherever it is needed, so no
[nnz, H] or [nnz, H, D] tensor exists on the GPU in forward or backward
(docs/DESIGN.md). K and V come from ONE projection so that its backward is
one GEMM over the kernels' single d_kv. Gradients reach the halo rows of h
through d_kv into `linear_kv`; the buffer's existing backward path ships
them, so `ctx.buffer.update` stays the only distributed seam.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import FullGraph, HaloGraph
from pipegcn_amd.models.sage import GNNBase


class TransformerLayer(nn.Module):
    def __init__(self, in_feats, out_feats, num_heads=1, attn_drop=0.0,
                 beta=False):
        super().__init__()
        if not 0.0 <= attn_drop < 1.0:
            raise ValueError(f"attn_drop={attn_drop} is outside [0, 1)")
        self.attn_drop = attn_drop
        if num_heads < 1 or out_feats % num_heads != 0:
            raise ValueError(
                f"Transformer layer width {out_feats} is not divisible by "
                f"{num_heads} heads (--n-hidden must be a multiple of "
                "--n-heads)")
        self.num_heads = num_heads
        self.head_dim = out_feats // num_heads
        self.linear_q = nn.Linear(in_feats, out_feats, bias=True)
        self.linear_kv = nn.Linear(in_feats, 2 * out_feats, bias=False)
        self.linear_skip = nn.Linear(in_feats, out_feats, bias=True)
        # without the gate no parameter exists and no draw is made
        self.linear_beta = (nn.Linear(3 * out_feats, 1, bias=False)
                            if beta else None)
        self.reset_parameters()

    def reset_parameters(self):
        # the project's uniform +-1/sqrt(fan_in); the gate, registered last,
        # is drawn last with its own fan-in of 3 * out_feats
        stdv = 1.0 / math.sqrt(self.linear_q.weight.size(1))
        for name, p in self.named_parameters():
            if name.startswith("linear_beta"):
                stdv = 1.0 / math.sqrt(p.size(1))
            p.data.uniform_(-stdv, stdv)

    def forward(self, graph, feat, in_deg=None):
        kv = ops.linear(feat, self.linear_kv)
        if self.training:
            assert isinstance(graph, HaloGraph)
            root = feat[: graph.num_in]
            agg = ops.dot_aggregate(graph, ops.linear(root, self.linear_q),
                                    kv, self.num_heads,
                                    attn_drop=self.attn_drop)
        else:
            # eval: full homogeneous graph, every node is a destination
            assert isinstance(graph, FullGraph)
            root = feat
            agg = ops.dot_aggregate_csr(graph.csr,
                                        ops.linear(root, self.linear_q), kv,
                                        self.num_heads)
        skip = ops.linear(root, self.linear_skip)
        if self.linear_beta is None:
            return agg + skip
        return ops.gated_residual(skip, agg, self.linear_beta.weight)


class Transformer(GNNBase):
    """Same structure as GAT and GATv2: conv layers then linear tail,
    norm+ReLU between layers, `ctx.buffer.update` as the only distributed
    seam.

    Hidden conv layers use `n_heads` heads, concatenated; a conv layer that
    is the model's last layer uses a single head (its width is n_class).
    `beta` gates every conv layer, that one included.
    """

    def __init__(self, layer_size, activation, use_pp=False, dropout=0.5,
                 norm="layer", train_size=None, n_linear=0, n_heads=1,
                 attn_drop=0.0, beta=False):
        if use_pp:
            raise NotImplementedError("--use-pp supports graphsage only "
                                      "(reference parity)")
        super().__init__(layer_size, activation, dropout, norm, train_size,
                         n_linear, n_heads=n_heads, attn_drop=attn_drop,
                         beta=beta)

    def make_conv(self, i, in_feats, out_feats, n_heads, attn_drop, beta):
        heads = 1 if i == self.n_layers - 1 else n_heads
        return TransformerLayer(in_feats, out_feats, num_heads=heads,
                                attn_drop=attn_drop, beta=beta)
