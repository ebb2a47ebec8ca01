"""GCNII model (Chen et al. 2020, "Simple and Deep Graph Convolutional
Networks"; PyG's GCN2Conv) — a capability extension over the reference: the
one model here that can go deep, through an initial residual and an identity
mapping.

GCNII layer l = 1, 2, ... at width F = in_feats = out_feats:

    P[v]   = (1 - alpha) d[v] sum over u in N(v) of d[u] h[u] + alpha H0[v]
    out[v] = (1 - beta_l) P[v] + beta_l P[v] W_l^T
    beta_l = log(lambda / l + 1)
    d      = rsqrt(in_deg.clamp(min=1)) over ALL local rows, as GCNLayer

Self-loops are already in the graphs and repeated edges count as often as
they occur. W_l is square and has no bias.

Deviation from the paper: its input map is a plain Linear; here layer 0 is
the existing `GCNLayer(n_feat, n_hidden)` and H0 is its output after norm and
activation, on inner rows. Conv layer i owns halo exchange slot i at width
`layer_size[i]`, so with a graph conv in front the buffer needs no change
(docs/ROADMAP.md has the Linear input map). Layers 1 .. n_layers - n_linear -
1 are GCNII layers, with the usual dropout before each and norm + ReLU after;
the linear tail (n_linear >= 1) maps to the classes.

The propagation is `ops.gcn2_propagate` (csrc/hip/gcn2.hip): one gather with
the initial residual in its epilogue, and a backward whose one elementwise
pass also adds alpha dP into a running fp32 buffer that all GCNII layers of
the step share; H0 receives that buffer's sum once (docs/DESIGN.md, "GCNII
propagation"). H0 is read on destination rows only, so nothing new crosses
the halo and `ctx.buffer.update` stays the only distributed seam.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import FullGraph, HaloGraph
from pipegcn_amd.models.gcn import GCNLayer
from pipegcn_amd.models.sage import GNNBase
from pipegcn_amd.parallel import context as ctx


class _H0Grad(torch.autograd.Function):
    """Identity on H0 whose backward adds the step's running dh0 buffer.
    Every GCNII layer takes H0 from here, so autograd runs this node after
    all of them, when the buffer holds their whole sum."""

    @staticmethod
    def forward(ctx_, h0, dh0):
        ctx_.dh0, ctx_.dtype = dh0, h0.dtype
        ctx_.set_materialize_grads(False)
        return h0.view_as(h0)

    @staticmethod
    def backward(ctx_, g):
        # g: what reached H0 beside the buffer (it is also layer 1's input);
        # the sum is formed in fp32 and rounded once
        total = ctx_.dh0 if g is None else ctx_.dh0 + g
        return total.to(ctx_.dtype), None


class GCN2Layer(nn.Module):
    """One GCNII layer; `index` l >= 1 sets beta_l = log(lam / l + 1)."""

    def __init__(self, feats, index, alpha=0.1, lam=0.5):
        super().__init__()
        if index < 1:
            raise ValueError(f"GCN2Layer: index={index} counts from 1")
        self.alpha = float(alpha)
        self.beta = math.log(lam / index + 1.0)
        self.linear = nn.Linear(feats, feats, bias=False)
        stdv = 1.0 / math.sqrt(feats)
        self.linear.weight.data.uniform_(-stdv, stdv)

    def forward(self, graph, feat, h0, deg=None, dh0=None):
        if self.training:
            assert isinstance(graph, HaloGraph)
            d = torch.rsqrt(deg.clamp(min=1.0)).contiguous()
            p = ops.gcn2_propagate(graph, feat.contiguous(), h0, d,
                                   self.alpha, dh0=dh0)
        else:
            assert isinstance(graph, FullGraph) and deg is None
            d = torch.rsqrt(graph.in_degrees().clamp(min=1.0)).contiguous()
            p = ops.gcn2_propagate_csr(graph.csr, feat.contiguous(), h0, d, d,
                                       self.alpha)
        return ops.gcn2_mix(p, self.linear.weight, self.beta)


class GCN2(GNNBase):
    """GCNLayer, GCNII layers, linear tail; norm+ReLU between layers,
    `ctx.buffer.update` as the only distributed seam. `in_deg` must cover ALL
    local nodes (inner + halo), as for GCN."""

    def __init__(self, layer_size, activation, use_pp=False, dropout=0.5,
                 norm="layer", train_size=None, n_linear=1, alpha=0.1,
                 lam=0.5):
        if use_pp:
            raise NotImplementedError("--use-pp supports graphsage only "
                                      "(reference parity)")
        n_conv = len(layer_size) - 1 - n_linear
        if n_linear < 1 or n_conv < 2:
            raise ValueError(
                "gcn2 needs --n-linear >= 1 and at least two conv layers "
                f"(got {n_conv} conv, {n_linear} linear): the GCNII layers "
                "are square and the linear tail maps to the classes")
        if len(set(layer_size[1:n_conv + 1])) != 1:
            raise ValueError("gcn2: the GCNII layers must be square, got "
                             f"widths {layer_size[1:n_conv + 1]}")
        super().__init__(layer_size, activation, dropout, norm, train_size,
                         n_linear, alpha=alpha, lam=lam)

    def make_conv(self, i, in_feats, out_feats, alpha, lam):
        if i == 0:
            return GCNLayer(in_feats, out_feats)
        return GCN2Layer(out_feats, i, alpha, lam)

    def forward(self, g, feat, in_deg=None):
        h, h0, dh0 = feat, None, None
        for i in range(self.n_layers):
            if i < self.n_layers - self.n_linear:
                if self.training:
                    h = ctx.buffer.update(i, h)
                h = self._drop(h)
                if i == 0:
                    h = self.layers[0](g, h, in_deg)
                else:
                    h = self.layers[i](g, h, h0, in_deg, dh0)
            else:
                h = ops.linear(self._drop(h), self.layers[i])
            if i < self.n_layers - 1:
                h = self._norm_act(i, h)
            if i == 0:
                h0 = h.contiguous()
                if self.training and h0.is_cuda and h0.requires_grad:
                    # the step's running dh0: every GCNII layer's backward
                    # adds into it, H0 receives the sum once
                    dh0 = torch.zeros(h0.shape, dtype=torch.float32,
                                      device=h0.device)
                    h0 = _H0Grad.apply(h0, dh0)
                h = h0
        return h
