"""GATv2 model: distributed equivalence, launcher, argument errors (CPU) and
the GPU training path (two ranks on one device, GPU vs CPU gradients)."""
import functools
import os

import pytest
import torch

from tests.conftest import run_distributed
from tests.test_distributed import _prepare_partitions, make_args
from tests.test_launcher import run_main

# ------------------------------------------------ 2-part versus 1-part (CPU)


def _gatv2_worker(rank, world, tmpdir, n_heads=None):
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
    kw = dict(n_partitions=world, enable_pipeline=False, model="gatv2")
    if n_heads is not None:  # None: the namespace has no n_heads at all
        kw["n_heads"] = n_heads
    args = make_args(**kw)
    args.n_feat, args.n_class, args.n_train = data_stats(ndata)
    s = trainer.run(part, args, device="cpu")
    t = torch.tensor(s["losses"])
    dist.all_reduce(t)
    return t.tolist()


@pytest.mark.parametrize("n_heads", [None, 4])
def test_gatv2_2part_matches_1part(tmp_path, n_heads):
    worker = functools.partial(_gatv2_worker, n_heads=n_heads)
    two = run_distributed(worker, 2, args=(str(tmp_path),))[0]
    one = run_distributed(worker, 1, args=(str(tmp_path),))[0]
    for a, b in zip(one, two):
        assert abs(a - b) / max(abs(a), 1e-9) < 2e-3, (one, two)
    assert two[-1] < two[0]


# ------------------------------------------------------------ launcher (CPU)


def test_main_gatv2_pipelined(tmp_path):
    out = run_main(tmp_path, ["--model", "gatv2", "--n-heads", "2",
                              "--enable-pipeline", "--no-eval"])
    assert "Epoch" in out and "nan" not in out


def test_main_gatv2_with_eval(tmp_path):
    out = run_main(tmp_path, ["--model", "gatv2", "--n-heads", "2",
                              "--enable-pipeline"])
    assert "Validation Accuracy" in out
    assert "model saved" in out
    ckpt = tmp_path / "model" / "synth-tiny-2-metis-vol-trans_final.pth.tar"
    sd = torch.load(ckpt, weights_only=True)
    for key in ("layers.0.linear_l.weight", "layers.0.linear_r.weight",
                "layers.0.attn"):
        assert key in sd, key
    assert sd["layers.0.attn"].shape == (2, 4)  # n_heads x (n_hidden / 2)
    assert sd["layers.1.attn"].shape[0] == 1  # last conv layer: one head


def test_main_gatv2_attn_drop(tmp_path):
    out = run_main(tmp_path, ["--model", "gatv2", "--n-heads", "2",
                              "--attn-drop", "0.3", "--enable-pipeline",
                              "--no-eval"])
    assert "Epoch" in out and "nan" not in out


# -------------------------------------------------------------- errors (CPU)


def test_gatv2_use_pp_is_rejected():
    from pipegcn_amd.models.gatv2 import GATv2

    with pytest.raises(NotImplementedError, match="--use-pp supports "
                                                  "graphsage only"):
        GATv2([8, 8, 3], torch.relu, use_pp=True)
    # the same through the trainer's model factory (--model gatv2 --use-pp)
    from pipegcn_amd import trainer

    with pytest.raises(NotImplementedError, match="graphsage only"):
        trainer.create_model([8, 8, 3], make_args(model="gatv2", use_pp=True))


def test_gatv2_heads_must_divide_hidden():
    from pipegcn_amd import trainer

    args = make_args(model="gatv2", n_hidden=10, n_heads=4)
    with pytest.raises(ValueError, match="not divisible by 4 heads"):
        trainer.create_model([16, 10, 10, 3], args)
    # the last conv layer uses one head, so any n_class is fine
    model = trainer.create_model(
        [16, 12, 12, 3], make_args(model="gatv2", n_hidden=12, n_heads=4))
    assert [l.num_heads for l in model.layers] == [4, 4, 1]
    assert model.layers[0].attn_drop == 0.0
    model = trainer.create_model(
        [16, 12, 3], make_args(model="gatv2", n_hidden=12, n_heads=4,
                               attn_drop=0.25))
    assert [l.attn_drop for l in model.layers] == [0.25, 0.25]


# ----------------------------------------------- GPU: 2 ranks on one device


def _gatv2_gpu_worker(rank, world, tmpdir, dtype):
    from tests.test_gpu_distributed import _train_gpu_worker

    return _train_gpu_worker(rank, world, tmpdir, model="gatv2", n_heads=4,
                             dtype=dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_gpu_gatv2_two_rank_training(tmp_path, dtype):
    run_distributed(functools.partial(_gatv2_gpu_worker, dtype=dtype), 2,
                    args=(str(tmp_path),), timeout=900)


# ------------------------------------------------------------ GPU versus CPU


def _fwd_bwd(device):
    """One forward+backward of a 2-layer GATv2 (4 heads, dropout 0) on the
    small synthetic partition -> (logits, {name: grad})."""
    import torch.nn.functional as F

    from pipegcn_amd.graph.halo import build_runtime_partition
    from pipegcn_amd.graph.synthetic import synth_partition
    from pipegcn_amd.models.gatv2 import GATv2
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
    model = GATv2(layer_size, F.relu, dropout=0.0, norm="layer",
                  train_size=part.n_train, n_heads=4).to(device)
    model.train()
    logits = model(rp.graph, rp.ndata["feat"])
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(
        logits[: rp.num_train], rp.ndata["label"][: rp.num_train])
    loss.backward()
    ctx.buffer.shutdown()
    return (logits.detach().cpu(),
            {k: p.grad.cpu() for k, p in model.named_parameters()})


def _gatv2_gpu_vs_cpu_worker(rank, world):
    cpu_logits, cpu_grads = _fwd_bwd("cpu")
    gpu_logits, gpu_grads = _fwd_bwd("cuda:0")
    assert torch.allclose(gpu_logits, cpu_logits, atol=1e-4, rtol=1e-4), \
        (gpu_logits - cpu_logits).abs().max()
    assert set(cpu_grads) == set(gpu_grads) and "layers.0.attn" in cpu_grads
    for k, ref in cpu_grads.items():
        err = (gpu_grads[k] - ref).abs().max() / ref.abs().max()
        print(f"{k}: rel-to-max err {err:.3e}")
        assert err < 1e-4, (k, err.item())
    return True


@pytest.mark.gpu
def test_gatv2_gpu_matches_cpu():
    run_distributed(_gatv2_gpu_vs_cpu_worker, 1, timeout=600)
