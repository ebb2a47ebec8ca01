"""GraphSAGE with the PNA multi-aggregator (SAGEPNALayer): arguments and
construction, --use-pp, train path versus eval path, the launcher (CPU) and
the layer on the GPU against the same module in float64 on the CPU. The CPU
op computes in fp32, so the float64 run forms the layer's input densely
(tests/test_spmm_pna_ops.py's formulas) and applies the module's linear."""
import pytest
import torch

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import FullGraph, HaloGraph
from pipegcn_amd.models.sage import GraphSAGE, SAGEPNALayer
from tests.test_distributed import make_args
from tests.test_launcher import run_main

N, F_IN, F_OUT = 120, 64, 32


def whole_graph():
    """One random graph as the training structure and as the eval one."""
    gen = torch.Generator().manual_seed(21)
    u = torch.randint(0, N, (900,), generator=gen)
    v = torch.randint(1, N, (900,), generator=gen)  # node 0 has no in-edges
    return (HaloGraph.from_edges(u, v, N, N), FullGraph.from_coo(u, v, N),
            torch.randn(N, F_IN, generator=gen))


def dense_pna64(hg, x):
    """[x | mean | max | min | std] in float64 with autograd; the extrema
    are read at the CPU op's args (the first-edge rule, checked against an
    independent reference in tests/test_spmm_pna_ops.py)."""
    csr = hg.csr
    rows = torch.repeat_interleave(torch.arange(N), csr.indptr.diff())
    cnt = torch.zeros(N, N, dtype=torch.float64)
    cnt.index_put_((rows, csr.indices.long()),
                   torch.ones(rows.numel(), dtype=torch.float64),
                   accumulate=True)
    d = cnt.sum(1, keepdim=True)
    has, dc = d > 0, d.clamp(min=1.0)
    mean = cnt @ x / dc
    dev = x.unsqueeze(0) - mean.unsqueeze(1)
    var = (cnt.unsqueeze(2) * dev * dev).sum(1) / dc
    std = torch.sqrt(torch.relu(var) + 1e-5) * has
    arg = ops.spmm_pna_csr(csr, x.detach().float(), with_state=True)[1]
    hi, lo = (x.gather(0, a.long().clamp(min=0)) * has
              for a in arg.split(F_IN, dim=1))
    return torch.cat((x, mean, hi, lo, std), dim=1)


def test_cli_and_construction():
    from pipegcn_amd import trainer
    from pipegcn_amd.cli import create_parser

    assert create_parser(["--aggregator", "pna"]).aggregator == "pna"
    model = trainer.create_model([16, 8, 3], make_args(aggregator="pna"))
    assert all(isinstance(l, SAGEPNALayer) for l in model.layers)
    assert model.layers[0].linear.weight.shape == (8, 5 * 16)
    assert set(model.state_dict()) == {
        f"{m}.{p}" for m in ("layers.0.linear", "layers.1.linear", "norm.0")
        for p in ("weight", "bias")}
    assert model.layers[0].linear.weight.abs().max() <= 1 / (5 * 16) ** 0.5
    with pytest.raises(NotImplementedError, match="--edge-drop does not "
                                                  "combine with "
                                                  "--aggregator pna"):
        trainer.create_model([16, 8, 3],
                             make_args(aggregator="pna", edge_drop=0.1))
    with pytest.raises(NotImplementedError, match="--aggregator pna"):
        GraphSAGE([16, 8, 3], torch.relu, use_pp=False, aggregator="pna",
                  edge_drop=0.1)
    for model_name in ("gcn", "gat", "gatv2", "transformer"):
        with pytest.raises(NotImplementedError, match="--aggregator pna "
                                                      "supports graphsage"):
            trainer.create_model([16, 8, 3], make_args(model=model_name,
                                                       aggregator="pna"))
    mean = GraphSAGE([16, 8, 3], torch.relu, use_pp=False, aggregator="mean")
    assert set(mean.state_dict()) == set(
        GraphSAGE([16, 8, 3], torch.relu, use_pp=False).state_dict())


def test_use_pp_first_layer_equals_the_plain_one():
    import types

    from pipegcn_amd import trainer

    hg, _, feat = whole_graph()
    rp = types.SimpleNamespace(graph=hg, num_all=N, ndata=dict(feat=feat))
    pre = trainer.precompute(rp, make_args(use_pp=True, aggregator="pna"))
    assert pre.shape == (N, 5 * F_IN)
    plain = SAGEPNALayer(F_IN, F_OUT)
    pp = SAGEPNALayer(F_IN, F_OUT, use_pp=True)
    pp.load_state_dict(plain.state_dict())
    assert torch.allclose(pp(hg, pre), plain(hg, feat), atol=1e-5, rtol=1e-5)
    model = GraphSAGE([F_IN, 8, 3], torch.relu, use_pp=True,
                      aggregator="pna")
    assert model.layers[0].use_pp and not model.layers[1].use_pp
    assert not model._exchanges_input(0) and model._exchanges_input(1)


def test_train_path_equals_eval_path():
    hg, fg, feat = whole_graph()
    layer = SAGEPNALayer(F_IN, F_OUT)
    train = layer(hg, feat)
    assert torch.allclose(layer.eval()(fg, feat), train, atol=1e-5, rtol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_pna_layer_gpu_matches_cpu_float64(dtype):
    """Output, weight gradient and input gradient with the tolerances of
    tests/test_spmm_pna_ops.py."""
    hg, _, feat = whole_graph()
    torch.manual_seed(4)
    ref = SAGEPNALayer(F_IN, F_OUT)
    gout = torch.randn(N, F_OUT)
    if dtype == torch.bfloat16:
        feat, gout = feat.bfloat16().float(), gout.bfloat16().float()
        ref = ref.bfloat16().float()  # the rounded weights, held exactly
    gpu = SAGEPNALayer(F_IN, F_OUT).to("cuda", dtype)
    gpu.load_state_dict(ref.state_dict())
    ref = ref.double()
    got, want = [], []
    for layer, x, g, res in (
            (ref, feat.double(), gout.double(), want),
            (gpu, feat.to("cuda", dtype), gout.to("cuda", dtype), got)):
        x.requires_grad_(True)
        out = (layer(hg.to("cuda"), x) if layer is gpu
               else layer.linear(dense_pna64(hg, x)))
        out.backward(g)
        res += [out.detach(), layer.linear.weight.grad, x.grad]
    for a, b, name in zip(got, want, ("out", "weight grad", "input grad")):
        assert a.dtype == dtype
        err = (a.double().cpu() - b).abs().max()
        print(name, dtype, "max err", err.item(), "of", b.abs().max().item())
        if dtype == torch.float32:
            assert torch.allclose(a.double().cpu(), b, atol=1e-4, rtol=1e-4)
        else:
            assert err / b.abs().max() < 0.02


def test_main_pna_pipelined(tmp_path):
    out = run_main(tmp_path, ["--aggregator", "pna", "--enable-pipeline",
                              "--no-eval"])
    assert "Epoch" in out and "nan" not in out and "inf" not in out
