"""Edge dropout in the models: GraphSAGE-mean and GCN layers, create_model,
the CLI flag, the launcher, and the GPU training path against the CPU one.

The graph is the small one of tests/test_spmm_live_rows.py (140 inner, 300
local nodes). `ctx.buffer` is replaced by a stand-in that appends fixed halo
rows: nothing here is about the exchange.

GPU against CPU: atol = rtol = 1e-3, tests/test_ops.py's policy for paths
through the dense layers.
"""
import functools
import math
import re

import pytest
import torch
import torch.nn.functional as F

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import FullGraph, HaloGraph
from pipegcn_amd.models.gcn import GCN
from pipegcn_amd.models.sage import GraphSAGE
from pipegcn_amd.parallel import context as ctx
from tests.test_distributed import make_args
from tests.test_launcher import run_main
from tests.test_spmm_live_rows import NUM_OUT, NUM_SRC, _edges

N_FEAT, N_HIDDEN, N_CLASS = 12, 16, 5
LAYERS = [N_FEAT, N_HIDDEN, N_CLASS]


@functools.lru_cache(maxsize=None)
def edges():
    return _edges(NUM_OUT, NUM_SRC, 30, 7)


@functools.lru_cache(maxsize=None)
def halo_graph(device="cpu"):
    hg = HaloGraph.from_edges(*edges(), NUM_OUT, NUM_SRC)
    return hg if device == "cpu" else hg.to(device)


@functools.lru_cache(maxsize=None)
def full_graph():
    return FullGraph.from_coo(*edges(), NUM_SRC)


class FixedHalo:
    """ctx.buffer's update(): the inner rows followed by constant halo rows."""

    def update(self, layer, feat):
        g = torch.Generator().manual_seed(50 + layer)
        halo = torch.randn(NUM_SRC - NUM_OUT, feat.shape[1], generator=g)
        return torch.cat((feat, halo.to(feat)))


@pytest.fixture
def fixed_halo(monkeypatch):
    monkeypatch.setattr(ctx, "buffer", FixedHalo())


def _feat(width=N_FEAT):
    return torch.randn(NUM_OUT, width,
                       generator=torch.Generator().manual_seed(1))


def _degrees(model_name):
    """in_deg as the trainer hands it over: inner nodes for GraphSAGE, all
    local nodes for GCN."""
    deg = halo_graph().csr.row_degrees()
    if model_name == "graphsage":
        return deg
    return torch.cat((deg, torch.full((NUM_SRC - NUM_OUT,), 3.0)))


def _model(model_name, edge_drop, layers=LAYERS, **kw):
    torch.manual_seed(3)
    if model_name == "graphsage":
        return GraphSAGE(layers, F.relu, kw.pop("use_pp", False),
                         dropout=0.0, edge_drop=edge_drop, **kw)
    return GCN(layers, F.relu, dropout=0.0, edge_drop=edge_drop, **kw)


# ------------------------------------------------------------------ CPU tier


@pytest.mark.parametrize("model_name", ["graphsage", "gcn"])
def test_train_drops_eval_does_not(model_name, fixed_halo):
    plain, drop = _model(model_name, 0.0), _model(model_name, 0.5)
    assert list(plain.state_dict()) == list(drop.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(),
                                                 drop.state_dict().values()))
    assert all(layer.edge_drop == 0.5 for layer in drop.layers)

    full = torch.randn(NUM_SRC, N_FEAT,
                       generator=torch.Generator().manual_seed(2))
    plain.eval(), drop.eval()
    state = torch.get_rng_state()
    with torch.no_grad():
        assert torch.equal(plain(full_graph(), full),
                           drop(full_graph(), full))
    assert torch.equal(torch.get_rng_state(), state)

    plain.train(), drop.train()
    hg, deg = halo_graph(), _degrees(model_name)
    base = plain(hg, _feat(), deg)
    assert torch.equal(torch.get_rng_state(), state)  # no draw when off
    torch.manual_seed(9)
    a = drop(hg, _feat(), deg)
    b = drop(hg, _feat(), deg)  # the next draws
    torch.manual_seed(9)
    c = drop(hg, _feat(), deg)
    assert torch.equal(a, c)
    assert not torch.equal(a, b)
    assert not torch.allclose(a, base, atol=1e-3)
    a.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in drop.parameters())


@pytest.mark.parametrize("model_name", ["graphsage", "gcn"])
def test_rate_is_validated(model_name):
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="edge_drop"):
            _model(model_name, bad)


def test_use_pp_drops_from_layer_one_on(fixed_halo, monkeypatch):
    layers = [N_FEAT, N_HIDDEN, N_HIDDEN, N_CLASS]
    model = _model("graphsage", 0.5, layers, use_pp=True)
    assert model.layers[0].use_pp and not model.layers[1].use_pp
    seen = []
    real = ops.spmm_mean

    def spy(graph, feat, inv_deg, edge_drop=0.0, seed=None):
        seen.append((feat.shape[1], edge_drop))
        return real(graph, feat, inv_deg, edge_drop, seed)

    monkeypatch.setattr(ops, "spmm_mean", spy)
    model.train()
    # layer 0 reads the precomputed [feat || mean], undropped
    out = model(halo_graph(), _feat(2 * N_FEAT), _degrees("graphsage"))
    out.sum().backward()
    assert seen == [(N_HIDDEN, 0.5), (N_HIDDEN, 0.5)]


def test_create_model_wires_and_rejects():
    from pipegcn_amd import trainer

    for model in ("graphsage", "gcn"):
        m = trainer.create_model(LAYERS, make_args(model=model,
                                                   edge_drop=0.3))
        assert all(layer.edge_drop == 0.3 for layer in m.layers)
        m = trainer.create_model(LAYERS, make_args(model=model))
        assert all(layer.edge_drop == 0.0 for layer in m.layers)
    for kw in (dict(aggregator="pool"), dict(model="gat"),
               dict(model="gatv2")):
        with pytest.raises(NotImplementedError, match="--edge-drop"):
            trainer.create_model(LAYERS, make_args(edge_drop=0.3, **kw))
        trainer.create_model(LAYERS, make_args(**kw))  # fine without
    with pytest.raises(NotImplementedError, match="--edge-drop"):
        GraphSAGE(LAYERS, F.relu, use_pp=False, aggregator="pool",
                  edge_drop=0.3)


def test_cli_flag():
    from pipegcn_amd.cli import create_parser

    assert create_parser([]).edge_drop == 0.0
    assert create_parser(["--edge-drop", "0.25"]).edge_drop == 0.25
    assert create_parser(["--edge_drop", "0.5"]).edge_drop == 0.5
    for bad in ("1.0", "-0.1", "2"):
        with pytest.raises(SystemExit):
            create_parser(["--edge-drop", bad])


@pytest.mark.parametrize("model_name", ["graphsage", "gcn"])
def test_main_edge_drop_pipelined(tmp_path, model_name):
    out = run_main(tmp_path, ["--model", model_name, "--edge-drop", "0.5",
                              "--enable-pipeline", "--no-eval"])
    # the two ranks' lines may share a line
    losses = [float(x) for x in re.findall(r"\| Loss ([-+.0-9einfa]+)", out)]
    assert len(losses) == 2, out  # both ranks, at the tenth epoch
    assert all(math.isfinite(x) for x in losses), losses


# ------------------------------------------------------------------ GPU tier


def _fwd_bwd(model_name, device, k):
    model = _model(model_name, 0.5).to(device)
    model.train()
    hg = halo_graph(device)
    x = _feat().to(device).requires_grad_(True)
    torch.manual_seed(k)
    logits = model(hg, x, _degrees(model_name).to(device))
    g = torch.randn(NUM_OUT, N_CLASS,
                    generator=torch.Generator().manual_seed(4))
    logits.backward(g.to(device))
    return logits.detach().cpu(), x.grad.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("model_name", ["graphsage", "gcn"])
def test_gpu_model_matches_cpu(model_name, fixed_halo):
    for k in (0, 1):
        cpu_logits, cpu_grad = _fwd_bwd(model_name, "cpu", k)
        gpu_logits, gpu_grad = _fwd_bwd(model_name, "cuda", k)
        assert torch.allclose(gpu_logits, cpu_logits, atol=1e-3, rtol=1e-3), \
            (k, (gpu_logits - cpu_logits).abs().max())
        assert torch.allclose(gpu_grad, cpu_grad, atol=1e-3, rtol=1e-3), \
            (k, (gpu_grad - cpu_grad).abs().max())
    a, _ = _fwd_bwd(model_name, "cpu", 0)
    b, _ = _fwd_bwd(model_name, "cpu", 1)
    assert not torch.equal(a, b)
