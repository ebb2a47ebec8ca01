"""GraphSAGE model + layer on the native SpMM.

Reimplements /root/reference/module/layer.py and module/model.py on our
HaloGraph/FullGraph CSR structures and hand-written gfx950 SpMM:

 - training path: mean aggregation over the bipartite halo graph with the
   degree-divide fused into the SpMM epilogue, then
   linear1(feat[:num_dst]) + linear2(ah)   (layer.py:44-51);
 - use_pp first layer collapses to one GEMM on [feat ‖ mean_agg]
   (layer.py:41-42);
 - eval path: full homogeneous graph, degrees from the graph (layer.py:52-62);
 - init: uniform ±1/sqrt(fan_in) (layer.py:24-36);
 - `aggregator="pool"`: GraphSAGE's max-pooling aggregator (SAGEPoolLayer),
   an extension over the reference, which has the mean only.
"""
from __future__ import annotations

import math
import os

import torch
from torch import nn

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import FullGraph, HaloGraph
from pipegcn_amd.models.sync_bn import SyncBatchNorm
from pipegcn_amd.parallel import context as ctx


def check_edge_drop(edge_drop):
    if not 0.0 <= edge_drop < 1.0:
        raise ValueError(f"edge_drop={edge_drop} is outside [0, 1)")
    return edge_drop


class GraphSAGELayer(nn.Module):
    """`edge_drop` > 0 removes each edge with that probability in training,
    redrawn at every call, and scales the kept sum by 1 / (1 - edge_drop)
    (docs/DESIGN.md, "Edge dropout"); evaluation never drops. A use_pp
    layer aggregates nothing in training, so it drops nothing."""

    def __init__(self, in_feats, out_feats, bias=True, use_pp=False,
                 edge_drop=0.0):
        super().__init__()
        self.use_pp = use_pp
        self.edge_drop = check_edge_drop(edge_drop)
        if use_pp:
            self.linear = nn.Linear(2 * in_feats, out_feats, bias=bias)
        else:
            self.linear1 = nn.Linear(in_feats, out_feats, bias=bias)
            self.linear2 = nn.Linear(in_feats, out_feats, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        def init(lin):
            stdv = 1.0 / math.sqrt(lin.weight.size(1))
            lin.weight.data.uniform_(-stdv, stdv)
            if lin.bias is not None:
                lin.bias.data.uniform_(-stdv, stdv)

        if self.use_pp:
            init(self.linear)
        else:
            init(self.linear1)
            init(self.linear2)

    def _can_fuse(self, feat):
        return (self.training and not self.use_pp and self.edge_drop == 0
                and feat.is_cuda)

    def fuses_dropout(self, feat):
        """Whether the model should hand this layer the tensor BEFORE feature
        dropout together with the rate (`forward(..., dropout=p)`), so that
        the training forward runs as the one fused node
        (`ops.sage_mean_layer`). PIPEGCN_SAGE_FUSED=0 keeps the three
        separate ops everywhere. The caller asks once per layer call."""
        return (self._can_fuse(feat)
                and os.environ.get("PIPEGCN_SAGE_FUSED", "1") != "0")

    def forward(self, graph, feat, in_deg=None, dropout=None):
        """dropout=None: feat is the layer's input as it is (the three
        separate ops in training). dropout=p, p >= 0: feat is the tensor
        before feature dropout and the fused node applies the rate p."""
        if dropout is not None and not self._can_fuse(feat):
            raise ValueError("GraphSAGELayer: only the fused training path "
                             "(GPU, mean aggregation, no edge dropout, not "
                             "use_pp) applies feature dropout itself")
        if self.training:
            if self.use_pp:
                return self.linear(feat)
            assert isinstance(graph, HaloGraph)
            inv_deg = (1.0 / in_deg.clamp(min=1.0)).contiguous()
            if dropout is not None:
                return ops.sage_mean_layer(graph, feat, inv_deg,
                                           self.linear1, self.linear2,
                                           p=dropout)
            if self.edge_drop > 0:
                ah = ops.spmm_mean(graph, feat, inv_deg,
                                   edge_drop=self.edge_drop)
            else:
                ah = ops.spmm_mean(graph, feat, inv_deg)
            x1 = feat[: graph.num_in]
            if feat.is_cuda:
                # hand-written MFMA fused dual GEMM (one output pass)
                return ops.sage_dual_linear(x1, ah, self.linear1,
                                            self.linear2)
            return self.linear1(x1) + self.linear2(ah)
        # eval: full homogeneous graph, degrees from the graph itself
        assert isinstance(graph, FullGraph) and in_deg is None
        degs = graph.in_degrees().clamp(min=1.0)
        ah = ops.spmm(graph.csr, feat, (1.0 / degs).contiguous())
        if self.use_pp:
            return self.linear(torch.cat((feat, ah), dim=1))
        return self.linear1(feat) + self.linear2(ah)


class SAGEPoolLayer(nn.Module):
    """GraphSAGE's max-pooling aggregator: every neighbour is projected and
    rectified, the element-wise maximum over the neighbourhood joins the
    node's own row:

        z = relu(linear_pool(h))          on ALL local rows (inner + halo)
        m[v] = max over u in N(v) of z[u]
        out = linear1(h[:num_dst]) + linear2(m)

    `ops.spmm_max` is the aggregation (csrc/hip/spmm_max.hip). The halo
    exchange carries h at the layer's input width, as for the mean layer.
    """

    def __init__(self, in_feats, out_feats, bias=True):
        super().__init__()
        self.linear_pool = nn.Linear(in_feats, in_feats, bias=True)
        self.linear1 = nn.Linear(in_feats, out_feats, bias=bias)
        self.linear2 = nn.Linear(in_feats, out_feats, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.linear_pool, self.linear1, self.linear2):
            stdv = 1.0 / math.sqrt(lin.weight.size(1))
            lin.weight.data.uniform_(-stdv, stdv)
            if lin.bias is not None:
                lin.bias.data.uniform_(-stdv, stdv)

    def forward(self, graph, feat, in_deg=None):
        z = torch.relu(ops.linear(feat, self.linear_pool))
        if self.training:
            assert isinstance(graph, HaloGraph)
            m = ops.spmm_max(graph, z)
            x1 = feat[: graph.num_in]
            if feat.is_cuda:
                return ops.sage_dual_linear(x1, m, self.linear1,
                                            self.linear2)
            return self.linear1(x1) + self.linear2(m)
        # eval: full homogeneous graph, every node is a destination
        assert isinstance(graph, FullGraph)
        m = ops.spmm_max_csr(graph.csr, z)
        return self.linear1(feat) + self.linear2(m)


class GNNBase(nn.Module):
    """Conv layers, then `n_linear` linear layers, with norm + activation
    between layers; `ctx.buffer.update` is the only distributed seam.

    A model subclasses this with `make_conv(i, in_feats, out_feats, **conv)`,
    which builds conv layer i from the keyword arguments the subclass handed
    to this constructor. Layer i is built before norm i, so the parameter
    draws and the state_dict keys (`layers.N.*`, `norm.N.*`) follow the layer
    index.
    """

    def __init__(self, layer_size, activation, dropout=0.5, norm="layer",
                 train_size=None, n_linear=0, **conv):
        super().__init__()
        self.n_layers = len(layer_size) - 1
        self.layers = nn.ModuleList()
        self.activation = activation
        self.n_linear = n_linear
        self.use_norm = norm is not None
        if self.use_norm:
            self.norm = nn.ModuleList()
        self.dropout = nn.Dropout(p=dropout)
        for i in range(self.n_layers):
            if i < self.n_layers - n_linear:
                self.layers.append(self.make_conv(i, layer_size[i],
                                                  layer_size[i + 1], **conv))
            else:
                self.layers.append(nn.Linear(layer_size[i],
                                             layer_size[i + 1]))
            if i < self.n_layers - 1 and self.use_norm:
                if norm == "layer":
                    self.norm.append(
                        nn.LayerNorm(layer_size[i + 1],
                                     elementwise_affine=True))
                elif norm == "batch":
                    self.norm.append(SyncBatchNorm(layer_size[i + 1],
                                                   train_size))

    def make_conv(self, i, in_feats, out_feats, **conv):
        raise NotImplementedError

    def _exchanges_input(self, i):
        """Whether conv layer i's training input goes through the halo
        exchange of `ctx.buffer.update`."""
        return True

    def forward(self, g, feat, in_deg=None):
        h = feat
        for i in range(self.n_layers):
            if i < self.n_layers - self.n_linear:
                if self.training and self._exchanges_input(i):
                    h = ctx.buffer.update(i, h)
                layer = self.layers[i]
                if (isinstance(layer, GraphSAGELayer)
                        and layer.fuses_dropout(h)):
                    # the layer's one node drops h itself
                    h = layer(g, h, in_deg, dropout=self.dropout.p)
                else:
                    h = self._drop(h)
                    h = layer(g, h, in_deg)
            else:
                h = self._drop(h)
                h = ops.linear(h, self.layers[i])
            if i < self.n_layers - 1:
                h = self._norm_act(i, h)
        return h

    def _drop(self, h):
        """Dropout: fused bitmask kernel on GPU, eager elsewhere."""
        if self.training and h.is_cuda and self.dropout.p > 0:
            return ops.fused_dropout(h, self.dropout.p)
        return self.dropout(h)

    def _norm_act(self, i, h):
        """Inter-layer norm + activation: fused LayerNorm+ReLU on GPU."""
        if h.is_cuda and self.use_norm and isinstance(self.norm[i],
                                                      nn.LayerNorm):
            fuse_relu = self.activation is torch.nn.functional.relu
            h = ops.layer_norm_relu(h, self.norm[i], relu=fuse_relu)
            return h if fuse_relu else self.activation(h)
        if self.use_norm:
            h = self.norm[i](h)
        return self.activation(h)


AGGREGATORS = ("mean", "pool")


class GraphSAGE(GNNBase):
    def __init__(self, layer_size, activation, use_pp, dropout=0.5,
                 norm="layer", train_size=None, n_linear=0,
                 aggregator="mean", edge_drop=0.0):
        if aggregator not in AGGREGATORS:
            raise ValueError(f"unknown aggregator {aggregator!r}: one of "
                             f"{', '.join(AGGREGATORS)}")
        if use_pp and aggregator == "pool":
            # layer 0's neighbourhood term passes through a learned
            # projection, so there is nothing to precompute
            raise NotImplementedError(
                "--use-pp does not combine with --aggregator pool")
        if check_edge_drop(edge_drop) > 0 and aggregator == "pool":
            # a masked max gather does not exist (docs/ROADMAP.md)
            raise NotImplementedError(
                "--edge-drop does not combine with --aggregator pool")
        super().__init__(layer_size, activation, dropout, norm, train_size,
                         n_linear, use_pp=use_pp, aggregator=aggregator,
                         edge_drop=edge_drop)
        self.use_pp = use_pp
        self.aggregator = aggregator
        self.edge_drop = edge_drop

    def make_conv(self, i, in_feats, out_feats, use_pp, aggregator,
                  edge_drop):
        if aggregator == "pool":
            return SAGEPoolLayer(in_feats, out_feats)
        # use_pp applies to the first layer only: its input already holds
        # [feat ‖ mean_agg], precomputed once
        return GraphSAGELayer(in_feats, out_feats, use_pp=use_pp and i == 0,
                              edge_drop=edge_drop)

    def _exchanges_input(self, i):
        # a use_pp first layer aggregates nothing, so it fetches no halo rows
        return i > 0 or not self.use_pp
