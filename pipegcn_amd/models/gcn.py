"""GCN model (symmetric-normalized aggregation) — a capability extension
over the reference (whose `create_model` supports only graphsage,
/root/reference/train.py:192-197); the north star names the "GraphSAGE/GCN
layer hot path".

Layer: H' = D^{-1/2} (A+I) D^{-1/2} H W + b, computed by the SAME gfx950
SpMM kernel with BOTH fused scales (dst_scale = deg(dst)^{-1/2},
src_scale = deg(src)^{-1/2}); self-loops are already present in the graphs
(datasets.py normalization). The src scale needs the in-degrees of HALO
nodes, fetched once at setup (trainer.exchange_halo_values).
"""
from __future__ import annotations

import math

import torch
from torch import nn

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import FullGraph, HaloGraph
from pipegcn_amd.models.sage import GNNBase, check_edge_drop


class _SpmmSym(torch.autograd.Function):
    """sym-normalized aggregation; backward is the transpose with the
    scales swapped (S = D_dst^{-1/2} A D_src^{-1/2};
    S^T = D_src^{-1/2} A^T D_dst^{-1/2}).

    drop = (key, thr, scale) of one edge-dropout draw (`ops.edge_drop_args`),
    or None: both passes then run the masked kernel over the same kept
    edges, with the same choice between their two branches."""

    @staticmethod
    def forward(ctx_, graph: HaloGraph, feat, inv_sqrt_dst, inv_sqrt_all,
                drop=None):
        ctx_.graph, ctx_.drop = graph, drop
        ctx_.save_for_backward(inv_sqrt_dst, inv_sqrt_all)
        if drop is not None:
            if graph.csr.nnz > feat.numel():
                return ops.spmm_drop(
                    graph.csr,
                    feat * inv_sqrt_all.unsqueeze(1).to(feat.dtype),
                    inv_sqrt_dst, drop=drop)
            return ops.spmm_drop(graph.csr, feat, inv_sqrt_dst,
                                 src_scale=inv_sqrt_all, drop=drop)
        # source-side scale: streaming row-multiply on dense graphs,
        # fused per-edge gather on sparse-wide ones (cost model in
        # _SpmmMean.backward)
        if graph.csr.nnz > feat.numel():
            return ops.spmm(graph.csr,
                            feat * inv_sqrt_all.unsqueeze(1).to(feat.dtype),
                            inv_sqrt_dst)
        return ops.spmm(graph.csr, feat, inv_sqrt_dst,
                        src_scale=inv_sqrt_all)

    @staticmethod
    def backward(ctx_, grad_out):
        inv_sqrt_dst, inv_sqrt_all = ctx_.saved_tensors
        g, drop = ctx_.graph, ctx_.drop
        if drop is not None:
            if g.csc.nnz > grad_out.numel():
                grad_feat = ops.spmm_drop(
                    g.csc,
                    grad_out * inv_sqrt_dst.unsqueeze(1).to(grad_out.dtype),
                    inv_sqrt_all, drop=drop, transposed=True)
            else:
                grad_feat = ops.spmm_drop(g.csc, grad_out.contiguous(),
                                          inv_sqrt_all,
                                          src_scale=inv_sqrt_dst, drop=drop,
                                          transposed=True)
        elif g.csc.nnz > grad_out.numel():
            grad_feat = ops.spmm(
                g.csc,
                grad_out * inv_sqrt_dst.unsqueeze(1).to(grad_out.dtype),
                inv_sqrt_all)
        else:
            grad_feat = ops.spmm(g.csc, grad_out.contiguous(),
                                 inv_sqrt_all, src_scale=inv_sqrt_dst)
        return None, grad_feat, None, None, None


class GCNLayer(nn.Module):
    """`edge_drop` > 0: DropEdge in training, as in GraphSAGELayer; the
    degrees on both sides stay the full-graph constants."""

    def __init__(self, in_feats, out_feats, bias=True, edge_drop=0.0):
        super().__init__()
        self.edge_drop = check_edge_drop(edge_drop)
        self.linear = nn.Linear(in_feats, out_feats, bias=bias)
        stdv = 1.0 / math.sqrt(self.linear.weight.size(1))
        self.linear.weight.data.uniform_(-stdv, stdv)
        if bias:
            self.linear.bias.data.uniform_(-stdv, stdv)

    def forward(self, graph, feat, deg=None):
        if self.training:
            assert isinstance(graph, HaloGraph)
            inv_sqrt_all = torch.rsqrt(deg.clamp(min=1.0)).contiguous()
            drop = ops.edge_drop_args("GCNLayer", self.edge_drop)
            ah = _SpmmSym.apply(graph, feat,
                                inv_sqrt_all[: graph.num_in].contiguous(),
                                inv_sqrt_all, drop if drop[1] > 0 else None)
            return ops.linear(ah, self.linear)
        assert isinstance(graph, FullGraph) and deg is None
        d = torch.rsqrt(graph.in_degrees().clamp(min=1.0)).contiguous()
        ah = ops.spmm(graph.csr, feat, d, src_scale=d)
        return self.linear(ah)


class GCN(GNNBase):
    """Same structure as GraphSAGE: conv layers then linear tail, norm+ReLU
    between layers, `ctx.buffer.update` as the only distributed seam.

    `in_deg` passed to forward must cover ALL local nodes (inner + halo) —
    the trainer assembles it via the one-shot halo degree exchange.
    """

    def __init__(self, layer_size, activation, use_pp=False, dropout=0.5,
                 norm="layer", train_size=None, n_linear=0, edge_drop=0.0):
        if use_pp:
            raise NotImplementedError("--use-pp supports graphsage only "
                                      "(reference parity)")
        super().__init__(layer_size, activation, dropout, norm, train_size,
                         n_linear, edge_drop=check_edge_drop(edge_drop))
        self.edge_drop = edge_drop

    def make_conv(self, i, in_feats, out_feats, edge_drop):
        return GCNLayer(in_feats, out_feats, edge_drop=edge_drop)
