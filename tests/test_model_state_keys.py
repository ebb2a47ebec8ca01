"""The state_dict layout of the four models: key order and shapes, one small
configuration each. Checkpoints are loaded by key, so the layer / norm
numbering that GNNBase builds must not move. The lists are the output of the
models as they were before the shared constructor loop."""
import pytest
import torch.nn.functional as F

from pipegcn_amd.models.gat import GAT
from pipegcn_amd.models.gatv2 import GATv2
from pipegcn_amd.models.gcn import GCN
from pipegcn_amd.models.sage import GraphSAGE

LAYER_SIZE = [12, 8, 8, 3]

LAYER_NORMS = [
    ("norm.0.weight", (8,)),
    ("norm.0.bias", (8,)),
    ("norm.1.weight", (8,)),
    ("norm.1.bias", (8,)),
]

CASES = {
    # use_pp: the first layer only is the single [feat ‖ mean_agg] GEMM
    "graphsage": (
        lambda: GraphSAGE(LAYER_SIZE, F.relu, True, norm="layer", n_linear=1),
        [
            ("layers.0.linear.weight", (8, 24)),
            ("layers.0.linear.bias", (8,)),
            ("layers.1.linear1.weight", (8, 8)),
            ("layers.1.linear1.bias", (8,)),
            ("layers.1.linear2.weight", (8, 8)),
            ("layers.1.linear2.bias", (8,)),
            ("layers.2.weight", (3, 8)),
            ("layers.2.bias", (3,)),
        ] + LAYER_NORMS),
    "gcn": (
        lambda: GCN(LAYER_SIZE, F.relu, False, norm="batch", n_linear=1,
                    train_size=10),
        [
            ("layers.0.linear.weight", (8, 12)),
            ("layers.0.linear.bias", (8,)),
            ("layers.1.linear.weight", (8, 8)),
            ("layers.1.linear.bias", (8,)),
            ("layers.2.weight", (3, 8)),
            ("layers.2.bias", (3,)),
            ("norm.0.weight", (8,)),
            ("norm.0.bias", (8,)),
            ("norm.0.running_mean", (8,)),
            ("norm.0.running_var", (8,)),
            ("norm.1.weight", (8,)),
            ("norm.1.bias", (8,)),
            ("norm.1.running_mean", (8,)),
            ("norm.1.running_var", (8,)),
        ]),
    # the last conv layer has one head whatever n_heads is
    "gat": (
        lambda: GAT(LAYER_SIZE, F.relu, False, norm="layer", n_linear=0,
                    n_heads=4),
        [
            ("layers.0.attn_l", (4, 2)),
            ("layers.0.attn_r", (4, 2)),
            ("layers.0.bias", (8,)),
            ("layers.0.linear.weight", (8, 12)),
            ("layers.1.attn_l", (4, 2)),
            ("layers.1.attn_r", (4, 2)),
            ("layers.1.bias", (8,)),
            ("layers.1.linear.weight", (8, 8)),
            ("layers.2.attn_l", (1, 3)),
            ("layers.2.attn_r", (1, 3)),
            ("layers.2.bias", (3,)),
            ("layers.2.linear.weight", (3, 8)),
        ] + LAYER_NORMS),
    "gatv2": (
        lambda: GATv2(LAYER_SIZE, F.relu, False, norm="layer", n_linear=1,
                      n_heads=2),
        [
            ("layers.0.attn", (2, 4)),
            ("layers.0.bias", (8,)),
            ("layers.0.linear_l.weight", (8, 12)),
            ("layers.0.linear_r.weight", (8, 12)),
            ("layers.1.attn", (2, 4)),
            ("layers.1.bias", (8,)),
            ("layers.1.linear_l.weight", (8, 8)),
            ("layers.1.linear_r.weight", (8, 8)),
            ("layers.2.weight", (3, 8)),
            ("layers.2.bias", (3,)),
        ] + LAYER_NORMS),
}


@pytest.mark.parametrize("model", sorted(CASES))
def test_state_dict_keys_and_shapes(model):
    make, want = CASES[model]
    got = [(k, tuple(v.shape)) for k, v in make().state_dict().items()]
    assert got == want
