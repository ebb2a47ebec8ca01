"""GraphSAGE with the softmax aggregator (SAGESoftmaxLayer), CPU and GPU.
Workers and bounds are tests/test_sage_pool_model.py's with this aggregator."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from pipegcn_amd import trainer
from pipegcn_amd.graph.csr import FullGraph, HaloGraph
from pipegcn_amd.models.sage import (GraphSAGE, GraphSAGELayer,
                                     SAGESoftmaxLayer)
from pipegcn_amd.parallel import context as ctx
from pipegcn_amd.parallel.buffer import Buffer
from pipegcn_amd.parallel.reducer import Reducer
from tests.conftest import run_distributed
from tests.test_distributed import _prepare_partitions, make_args
from tests.test_launcher import run_main


def test_cli_construction_and_state_dict():
    from pipegcn_amd.cli import create_parser

    assert create_parser(["--aggregator", "softmax"]).aggregator == "softmax"
    model = trainer.create_model([16, 8, 3], make_args(aggregator="softmax"))
    assert all(isinstance(l, SAGESoftmaxLayer) for l in model.layers)
    sd = model.state_dict()
    want = {f"layers.{i}.{lin}.{p}" for i in range(2)
            for lin in ("linear1", "linear2") for p in ("weight", "bias")}
    want |= {"layers.0.beta", "layers.1.beta", "norm.0.weight", "norm.0.bias"}
    assert set(sd) == want
    assert sd["layers.0.linear2.weight"].shape == (8, 16)
    for beta in (sd["layers.0.beta"], sd["layers.1.beta"]):
        assert beta.dtype == torch.float32 and beta.tolist() == [1.0]
    assert model.bfloat16().layers[0].beta.dtype == torch.float32
    assert model.layers[0].linear1.weight.dtype == torch.bfloat16
    # GraphSAGELayer's draws in its order; beta draws nothing
    torch.manual_seed(11)
    a = SAGESoftmaxLayer(16, 8)
    torch.manual_seed(11)
    b = GraphSAGELayer(16, 8)
    for lin in ("linear1", "linear2"):
        assert torch.equal(getattr(a, lin).weight, getattr(b, lin).weight)
        assert torch.equal(getattr(a, lin).bias, getattr(b, lin).bias)


def test_refusals():
    use_pp = "--use-pp does not combine with --aggregator softmax"
    edge_drop = "--edge-drop does not combine with --aggregator softmax"
    with pytest.raises(NotImplementedError, match=use_pp):
        GraphSAGE([8, 8, 3], torch.relu, use_pp=True, aggregator="softmax")
    with pytest.raises(NotImplementedError, match=use_pp):
        trainer.precompute(None, make_args(use_pp=True, aggregator="softmax"))
    with pytest.raises(NotImplementedError, match=edge_drop):
        GraphSAGE([8, 8, 3], torch.relu, use_pp=False, aggregator="softmax",
                  edge_drop=0.1)
    with pytest.raises(NotImplementedError, match=edge_drop):
        trainer.create_model([8, 8, 3], make_args(aggregator="softmax",
                                                  edge_drop=0.1))
    other = "--aggregator softmax supports graphsage only"
    for model in ("gcn", "gat", "gatv2", "transformer"):
        with pytest.raises(NotImplementedError, match=other):
            trainer.create_model([8, 8, 3], make_args(model=model,
                                                      aggregator="softmax"))


def test_train_path_equals_eval_path():
    n = 120
    gen = torch.Generator().manual_seed(21)
    u = torch.randint(0, n, (900,), generator=gen)
    v = torch.randint(1, n, (900,), generator=gen)  # node 0 has no in-edges
    feat = torch.randn(n, 64, generator=gen)
    layer = SAGESoftmaxLayer(64, 32)
    layer.beta.data.fill_(-0.6)
    train = layer(HaloGraph.from_edges(u, v, n, n), feat)
    evald = layer.eval()(FullGraph.from_coo(u, v, n), feat)
    assert torch.allclose(evald, train, atol=1e-5, rtol=1e-5)


def _cpu_worker(rank, world, tmpdir):
    import torch.distributed as dist

    from pipegcn_amd.graph.datasets import data_stats

    os.chdir(tmpdir)
    ctx.buffer, ctx.reducer = Buffer(), Reducer()
    (u, v, n, ndata), part = _prepare_partitions(
        os.path.join(tmpdir, f"p{world}"), world)
    args = make_args(n_partitions=world, enable_pipeline=False,
                     aggregator="softmax")
    args.n_feat, args.n_class, args.n_train = data_stats(ndata)
    t = torch.tensor(trainer.run(part, args, device="cpu")["losses"])
    dist.all_reduce(t)
    return t.tolist()


def test_softmax_2part_matches_1part(tmp_path):
    two = run_distributed(_cpu_worker, 2, args=(str(tmp_path),))[0]
    one = run_distributed(_cpu_worker, 1, args=(str(tmp_path),))[0]
    for a, b in zip(one, two):
        assert abs(a - b) / max(abs(a), 1e-9) < 2e-3, (one, two)
    assert two[-1] < two[0]


def test_main_softmax_pipelined_with_eval(tmp_path):
    out = run_main(tmp_path, ["--aggregator", "softmax", "--enable-pipeline"])
    assert "Epoch" in out and "nan" not in out and "Validation Acc" in out


def _fwd_bwd(device):
    """A 2-layer model on the small partition -> (logits, {name: grad})."""
    from pipegcn_amd.graph.halo import build_runtime_partition
    from pipegcn_amd.graph.synthetic import synth_partition

    part = synth_partition("small", 0, 1, seed=0)
    rp = build_runtime_partition(part, device=device)
    layer_size = trainer.get_layer_size(part.n_feat, 32, part.n_class, 2)
    ctx.buffer = Buffer()
    ctx.buffer.init_buffer(rp.num_in, rp.num_all, rp.boundary,
                           rp.recv_shape, layer_size[:2], device=device)
    torch.manual_seed(7)
    model = GraphSAGE(layer_size, F.relu, use_pp=False, dropout=0.0,
                      norm="layer", train_size=part.n_train,
                      aggregator="softmax").to(device)
    model.train()
    logits = model(rp.graph, rp.ndata["feat"], rp.ndata["in_degree"])
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(
        logits[: rp.num_train], rp.ndata["label"][: rp.num_train])
    loss.backward()
    ctx.buffer.shutdown()
    return (logits.detach().cpu(),
            {k: p.grad.cpu() for k, p in model.named_parameters()})


def _gpu_vs_cpu_worker(rank, world):
    cpu_logits, cpu_grads = _fwd_bwd("cpu")
    gpu_logits, gpu_grads = _fwd_bwd("cuda:0")
    assert torch.allclose(gpu_logits, cpu_logits, atol=1e-4, rtol=1e-4), \
        (gpu_logits - cpu_logits).abs().max()
    assert set(cpu_grads) == set(gpu_grads)
    assert {"layers.0.beta", "layers.1.beta"} <= set(cpu_grads)
    for k, ref in cpu_grads.items():
        err = (gpu_grads[k] - ref).abs().max() / ref.abs().max()
        print(f"{k}: rel-to-max err {err:.3e}")
        assert err < 1e-4, (k, err.item())
    return True


@pytest.mark.gpu
def test_softmax_gpu_matches_cpu():
    run_distributed(_gpu_vs_cpu_worker, 1, timeout=600)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_gpu_softmax_two_rank_training(tmp_path, dtype):
    from tests.test_gpu_distributed import _train_gpu_worker

    worker = functools.partial(_train_gpu_worker, aggregator="softmax",
                               dtype=dtype)
    run_distributed(worker, 2, args=(str(tmp_path),), timeout=900)
