"""GraphSAGE with the max-pooling aggregator: distributed equivalence,
launcher, argument errors, state-dict keys (CPU) and the GPU training path
(two ranks on one device, GPU vs CPU gradients)."""
import functools
import os

import pytest
import torch

from tests.conftest import run_distributed
from tests.test_distributed import _prepare_partitions, make_args
from tests.test_launcher import run_main

# ------------------------------------------------ 2-part versus 1-part (CPU)


def _pool_worker(rank, world, tmpdir):
    from pipegcn_amd import trainer
    from pipegcn_amd.graph.datasets import data_stats
    from pipegcn_amd.parallel import context as ctx
    from pipegcn_amd.parallel.buffer import Buffer
    from pipegcn_amd.parallel.reducer import Reducer

    import torch.distributed as dist

    os.chdir(tmpdir)
    ctx.buffer = Buffer()
    ctx.reducer = Reducer()
    (u, v, n, ndata), part = _prepare_partitions(
        os.path.join(tmpdir, f"p{world}"), world)
    args = make_args(n_partitions=world, enable_pipeline=False,
                     aggregator="pool")
    args.n_feat, args.n_class, args.n_train = data_stats(ndata)
    s = trainer.run(part, args, device="cpu")
    t = torch.tensor(s["losses"])
    dist.all_reduce(t)
    return t.tolist()


def test_pool_2part_matches_1part(tmp_path):
    two = run_distributed(_pool_worker, 2, args=(str(tmp_path),))[0]
    one = run_distributed(_pool_worker, 1, args=(str(tmp_path),))[0]
    for a, b in zip(one, two):
        assert abs(a - b) / max(abs(a), 1e-9) < 2e-3, (one, two)
    assert two[-1] < two[0]


# ------------------------------------------------------------ launcher (CPU)


def test_main_pool_pipelined(tmp_path):
    out = run_main(tmp_path, ["--aggregator", "pool", "--enable-pipeline",
                              "--no-eval"])
    assert "Epoch" in out and "nan" not in out


def test_main_pool_with_eval(tmp_path):
    out = run_main(tmp_path, ["--aggregator", "pool", "--enable-pipeline"])
    assert "Validation Accuracy" in out
    assert "model saved" in out
    ckpt = tmp_path / "model" / "synth-tiny-2-metis-vol-trans_final.pth.tar"
    sd = torch.load(ckpt, weights_only=True)
    assert "layers.0.linear_pool.weight" in sd
    assert sd["layers.1.linear_pool.weight"].shape == (8, 8)  # n_hidden^2


# ------------------------------------------------- errors and keys (CPU)


def test_parser_default_and_choices():
    from pipegcn_amd.cli import create_parser

    assert create_parser([]).aggregator == "mean"
    assert create_parser(["--aggregator", "pool"]).aggregator == "pool"
    with pytest.raises(SystemExit):
        create_parser(["--aggregator", "lstm"])


def test_pool_use_pp_is_rejected_by_the_constructor():
    from pipegcn_amd import trainer
    from pipegcn_amd.models.sage import GraphSAGE

    with pytest.raises(NotImplementedError, match="--use-pp does not "
                                                  "combine with "
                                                  "--aggregator pool"):
        GraphSAGE([8, 8, 3], torch.relu, use_pp=True, aggregator="pool")
    with pytest.raises(NotImplementedError, match="--aggregator pool"):
        trainer.create_model([8, 8, 3],
                             make_args(use_pp=True, aggregator="pool"))
    with pytest.raises(ValueError, match="unknown aggregator"):
        GraphSAGE([8, 8, 3], torch.relu, use_pp=False, aggregator="lstm")


def test_pool_use_pp_is_rejected_by_precompute():
    from pipegcn_amd import trainer

    # refused before the partition is looked at
    with pytest.raises(NotImplementedError, match="--use-pp does not "
                                                  "combine with "
                                                  "--aggregator pool"):
        trainer.precompute(None, make_args(use_pp=True, aggregator="pool"))


@pytest.mark.parametrize("model", ["gcn", "gat", "gatv2"])
def test_pool_with_other_models_is_rejected(model):
    from pipegcn_amd import trainer

    with pytest.raises(NotImplementedError, match="--aggregator pool "
                                                  "supports graphsage only"):
        trainer.create_model([8, 8, 3],
                             make_args(model=model, aggregator="pool"))
    # the default leaves them alone
    trainer.create_model([8, 8, 3], make_args(model=model))


def test_pool_state_dict_keys_and_init_order():
    import math

    from pipegcn_amd import trainer
    from pipegcn_amd.models.sage import SAGEPoolLayer

    model = trainer.create_model([16, 8, 8, 3],
                                 make_args(aggregator="pool", n_linear=1))
    assert all(isinstance(l, SAGEPoolLayer) for l in model.layers[:2])
    assert isinstance(model.layers[2], torch.nn.Linear)
    want = {f"layers.{i}.{lin}.{p}" for i in range(2)
            for lin in ("linear_pool", "linear1", "linear2")
            for p in ("weight", "bias")}
    want |= {"layers.2.weight", "layers.2.bias"}
    want |= {f"norm.{i}.{p}" for i in range(2) for p in ("weight", "bias")}
    assert set(model.state_dict()) == want
    assert model.layers[0].linear_pool.weight.shape == (16, 16)
    assert model.layers[0].linear1.weight.shape == (8, 16)

    # +-1/sqrt(fan_in), drawn in the order pool, linear1, linear2
    layer = SAGEPoolLayer(16, 8)
    torch.manual_seed(11)
    layer.reset_parameters()
    torch.manual_seed(11)
    stdv = 1.0 / math.sqrt(16)
    for lin in (layer.linear_pool, layer.linear1, layer.linear2):
        w = torch.empty_like(lin.weight).uniform_(-stdv, stdv)
        b = torch.empty_like(lin.bias).uniform_(-stdv, stdv)
        assert torch.equal(lin.weight.data, w)
        assert torch.equal(lin.bias.data, b)


def test_mean_model_is_unchanged_by_the_argument():
    """aggregator="mean" builds what the model built before: same layers,
    same parameter draws."""
    from pipegcn_amd.models.sage import GraphSAGE, GraphSAGELayer

    torch.manual_seed(3)
    a = GraphSAGE([16, 8, 3], torch.relu, use_pp=False)
    torch.manual_seed(3)
    b = GraphSAGE([16, 8, 3], torch.relu, use_pp=False, aggregator="mean")
    assert all(isinstance(l, GraphSAGELayer) for l in a.layers)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


# ----------------------------------------------- GPU: 2 ranks on one device


def _pool_gpu_worker(rank, world, tmpdir, dtype):
    from tests.test_gpu_distributed import _train_gpu_worker

    return _train_gpu_worker(rank, world, tmpdir, aggregator="pool",
                             dtype=dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_gpu_pool_two_rank_training(tmp_path, dtype):
    run_distributed(functools.partial(_pool_gpu_worker, dtype=dtype), 2,
                    args=(str(tmp_path),), timeout=900)


# ------------------------------------------------------------ GPU versus CPU


def _fwd_bwd(device):
    """One forward+backward of a 2-layer pool model (dropout 0) on the small
    synthetic partition -> (logits, {name: grad})."""
    import torch.nn.functional as F

    from pipegcn_amd.graph.halo import build_runtime_partition
    from pipegcn_amd.graph.synthetic import synth_partition
    from pipegcn_amd.models.sage import GraphSAGE
    from pipegcn_amd.parallel import context as ctx
    from pipegcn_amd.parallel.buffer import Buffer
    from pipegcn_amd.trainer import get_layer_size

    part = synth_partition("small", 0, 1, seed=0)
    rp = build_runtime_partition(part, device=device)
    layer_size = get_layer_size(part.n_feat, 32, part.n_class, 2)
    ctx.buffer = Buffer()
    ctx.buffer.init_buffer(rp.num_in, rp.num_all, rp.boundary,
                           rp.recv_shape, layer_size[:2], device=device)
    torch.manual_seed(7)
    model = GraphSAGE(layer_size, F.relu, use_pp=False, dropout=0.0,
                      norm="layer", train_size=part.n_train,
                      aggregator="pool").to(device)
    model.train()
    logits = model(rp.graph, rp.ndata["feat"], rp.ndata["in_degree"])
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(
        logits[: rp.num_train], rp.ndata["label"][: rp.num_train])
    loss.backward()
    ctx.buffer.shutdown()
    return (logits.detach().cpu(),
            {k: p.grad.cpu() for k, p in model.named_parameters()})


def _pool_gpu_vs_cpu_worker(rank, world):
    cpu_logits, cpu_grads = _fwd_bwd("cpu")
    gpu_logits, gpu_grads = _fwd_bwd("cuda:0")
    assert torch.allclose(gpu_logits, cpu_logits, atol=1e-4, rtol=1e-4), \
        (gpu_logits - cpu_logits).abs().max()
    assert set(cpu_grads) == set(gpu_grads)
    assert "layers.0.linear_pool.weight" in cpu_grads
    for k, ref in cpu_grads.items():
        err = (gpu_grads[k] - ref).abs().max() / ref.abs().max()
        print(f"{k}: rel-to-max err {err:.3e}")
        assert err < 1e-4, (k, err.item())
    return True


@pytest.mark.gpu
def test_pool_gpu_matches_cpu():
    run_distributed(_pool_gpu_vs_cpu_worker, 1, timeout=600)
