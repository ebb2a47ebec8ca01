"""GCNII model: parser, refusals, state dict, beta_l, one CPU training step
against plain float64 torch layers; on the GPU, the step against the CPU's."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_distributed import make_args
from tests.test_launcher import run_main

SIZES = [12, 8, 8, 8, 3]  # GCN layer, two GCNII layers, one linear


def _create(**kw):
    from pipegcn_amd import trainer

    kw.setdefault("n_linear", 1)
    return trainer.create_model(SIZES, make_args(model="gcn2", **kw))


def test_parser_defaults_and_spellings():
    from pipegcn_amd.cli import create_parser

    a = create_parser(["--model", "gcn2"])
    assert (a.model, a.gcn2_alpha, a.gcn2_lambda) == ("gcn2", 0.1, 0.5)
    for argv in (["--gcn2-alpha", "0.2", "--gcn2-lambda", "1.5"],
                 ["--gcn2_alpha", "0.2", "--gcn2_lambda", "1.5"]):
        a = create_parser(argv)
        assert (a.gcn2_alpha, a.gcn2_lambda) == (0.2, 1.5)


@pytest.mark.parametrize("kw,match", [
    (dict(use_pp=True), "--use-pp supports graphsage only"),
    (dict(edge_drop=0.2), "--edge-drop does not combine with --model gcn2"),
    (dict(beta_gate=True), "--beta-gate supports --model transformer only"),
    (dict(aggregator="pool"), "--aggregator pool supports graphsage only"),
    (dict(n_linear=0), "n-linear >= 1"),
])
def test_gcn2_refusals(kw, match):
    exc = ValueError if "n_linear" in kw else NotImplementedError
    with pytest.raises(exc, match=match):
        _create(**kw)


def test_state_dict_and_betas():
    from pipegcn_amd.models.gcn2 import GCN2Layer

    model = _create(gcn2_lambda=0.5)
    want = {f"norm.{i}.{p}": (8,) for i in (0, 1, 2)
            for p in ("weight", "bias")}
    want.update({"layers.0.linear.weight": (8, 12),
                 "layers.0.linear.bias": (8,), "layers.3.bias": (3,),
                 "layers.1.linear.weight": (8, 8), "layers.3.weight": (3, 8),
                 "layers.2.linear.weight": (8, 8)})
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == want
    for l in (1, 2):
        assert (type(model.layers[l]), model.layers[l].alpha) == (GCN2Layer,
                                                                  0.1)
        assert model.layers[l].beta == pytest.approx(math.log(0.5 / l + 1))
        assert model.layers[l].linear.weight.abs().max() <= 8 ** -0.5


def _step(device, seed=7):
    """One training step, dropout 0 -> (model, data, logits, {name: grad})."""
    from pipegcn_amd.graph.csr import HaloGraph
    from pipegcn_amd.parallel import context as ctx
    from pipegcn_amd.parallel.buffer import Buffer

    n = 150
    gen = torch.Generator().manual_seed(3)
    u, v = torch.randint(0, n, (2, 1200), generator=gen)
    feat = torch.randn(n, SIZES[0], generator=gen)
    label = torch.arange(n) % SIZES[-1]
    deg = torch.bincount(v, minlength=n).float()
    ctx.buffer = Buffer()
    ctx.buffer.init_buffer(n, n, [None], [None], SIZES[:3], device=device)
    torch.manual_seed(seed)
    model = _create(dropout=0.0, gcn2_alpha=0.2).to(device).train()
    graph = HaloGraph.from_edges(u, v, n, n).to(device)
    logits = model(graph, feat.to(device), deg.to(device))
    F.cross_entropy(logits, label.to(device), reduction="sum").backward()
    ctx.buffer.shutdown()
    grads = {k: p.grad.cpu() for k, p in model.named_parameters()}
    return model, (u, v, feat, label, deg), logits.detach().cpu(), grads


def _agree(logits, grads, ref_logits, ref_grads):
    assert torch.allclose(logits.double(), ref_logits.double(), atol=1e-4,
                          rtol=1e-4)
    assert set(grads) == set(ref_grads)
    for k, ref in ref_grads.items():
        err = (grads[k].double() - ref.double()).abs().max() / ref.abs().max()
        assert err < 1e-4, (k, err.item())


def test_gcn2_cpu_step_matches_plain_torch():
    model, (u, v, feat, label, deg), logits, grads = _step("cpu")
    p = {k: t.detach().double().requires_grad_(True)
         for k, t in model.named_parameters()}
    d = deg.double().clamp(min=1).rsqrt().unsqueeze(1)

    def prop(h):  # D^{-1/2} A D^{-1/2} h
        return d * torch.zeros_like(h).index_add(0, v, (d * h)[u])

    def act(i, h):
        return F.relu(F.layer_norm(h, (8,), p[f"norm.{i}.weight"],
                                   p[f"norm.{i}.bias"]))

    h = h0 = act(0, F.linear(prop(feat.double()), p["layers.0.linear.weight"],
                             p["layers.0.linear.bias"]))
    for l in (1, 2):
        P = 0.8 * prop(h) + 0.2 * h0
        beta = math.log(0.5 / l + 1)
        h = act(l, (1 - beta) * P
                + beta * P @ p[f"layers.{l}.linear.weight"].t())
    ref = F.linear(h, p["layers.3.weight"], p["layers.3.bias"])
    F.cross_entropy(ref, label, reduction="sum").backward()
    _agree(logits, grads, ref.detach(), {k: t.grad for k, t in p.items()})


@pytest.mark.gpu
def test_gcn2_gpu_step_matches_cpu():
    """tests/test_transformer_model.py's bound for the same comparison, which
    the residual gated model test mirrors."""
    _agree(*_step("cuda")[2:], *_step("cpu")[2:])


@pytest.mark.gpu
def test_main_gcn2_trains_and_saves_checkpoint(tmp_path):
    out = run_main(tmp_path, ["--model", "gcn2", "--n-partitions", "1",
                              "--n-epochs", "2", "--n-layers", "4",
                              "--n-linear", "1", "--log-every", "1"])
    assert "nan" not in out and "model saved" in out
    ckpt = tmp_path / "model" / "synth-tiny-1-metis-vol-trans_final.pth.tar"
    sd = torch.load(ckpt, weights_only=True)
    assert sd["layers.1.linear.weight"].shape == (8, 8)
