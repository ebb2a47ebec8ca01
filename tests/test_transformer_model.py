"""Transformer (dot-product attention) model: distributed equivalence,
launcher, argument errors (CPU) and GPU vs CPU gradients of one training
step; mirrors tests/test_gatv2_model.py."""
import os

import pytest
import torch

from tests.conftest import run_distributed
from tests.test_distributed import _prepare_partitions, make_args
from tests.test_launcher import run_main

KEYS = ("linear_q.weight", "linear_q.bias", "linear_kv.weight",
        "linear_skip.weight", "linear_skip.bias")


def _worker(rank, world, tmpdir):
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
                     model="transformer", n_heads=4)
    args.n_feat, args.n_class, args.n_train = data_stats(ndata)
    s = trainer.run(part, args, device="cpu")
    t = torch.tensor(s["losses"])
    dist.all_reduce(t)
    return t.tolist()


def test_transformer_2part_matches_1part(tmp_path):
    two = run_distributed(_worker, 2, args=(str(tmp_path),))[0]
    one = run_distributed(_worker, 1, args=(str(tmp_path),))[0]
    for a, b in zip(one, two):
        assert abs(a - b) / max(abs(a), 1e-9) < 2e-3, (one, two)
    assert two[-1] < two[0]


def test_main_transformer_attn_drop_saves_checkpoint(tmp_path):
    out = run_main(tmp_path, ["--model", "transformer", "--n-heads", "2",
                              "--attn-drop", "0.3", "--enable-pipeline"])
    assert "Epoch" in out and "nan" not in out
    assert "model saved" in out
    ckpt = tmp_path / "model" / "synth-tiny-2-metis-vol-trans_final.pth.tar"
    sd = torch.load(ckpt, weights_only=True)
    for i in (0, 1):
        for key in KEYS:
            assert f"layers.{i}.{key}" in sd, (i, key)
    n_hidden = sd["layers.0.linear_q.weight"].shape[0]
    assert sd["layers.0.linear_kv.weight"].shape[0] == 2 * n_hidden


def test_transformer_refuses_use_pp_and_edge_drop():
    from pipegcn_amd import trainer
    from pipegcn_amd.models.transformer import Transformer

    with pytest.raises(NotImplementedError, match="graphsage only"):
        Transformer([8, 8, 3], torch.relu, use_pp=True)
    with pytest.raises(NotImplementedError, match="graphsage only"):
        trainer.create_model([8, 8, 3],
                             make_args(model="transformer", use_pp=True))
    with pytest.raises(NotImplementedError,
                       match="--edge-drop does not combine with --model "
                             "transformer"):
        trainer.create_model([8, 8, 3],
                             make_args(model="transformer", edge_drop=0.2))
    model = trainer.create_model(
        [16, 12, 12, 3], make_args(model="transformer", n_hidden=12,
                                   n_heads=4, attn_drop=0.25))
    assert [l.num_heads for l in model.layers] == [4, 4, 1]
    assert [l.attn_drop for l in model.layers] == [0.25] * 3


# ------------------------------------------------------------ GPU versus CPU


def _fwd_bwd(device):
    """One training forward+backward of a 2-layer Transformer (4 heads,
    feature dropout 0, attention dropout 0.3 from one torch seed) on the
    small synthetic partition -> (logits, {name: grad})."""
    import torch.nn.functional as F

    from pipegcn_amd.graph.halo import build_runtime_partition
    from pipegcn_amd.graph.synthetic import synth_partition
    from pipegcn_amd.models.transformer import Transformer
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
    model = Transformer(layer_size, F.relu, dropout=0.0, norm="layer",
                        train_size=part.n_train, n_heads=4,
                        attn_drop=0.3).to(device)
    model.train()
    logits = model(rp.graph, rp.ndata["feat"])
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
    assert "layers.0.linear_kv.weight" in cpu_grads
    for k, ref in cpu_grads.items():
        err = (gpu_grads[k] - ref).abs().max() / ref.abs().max()
        print(f"{k}: rel-to-max err {err:.3e}")
        assert err < 1e-4, (k, err.item())
    return True


@pytest.mark.gpu
def test_transformer_gpu_matches_cpu():
    run_distributed(_gpu_vs_cpu_worker, 1, timeout=600)
