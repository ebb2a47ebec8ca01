"""Transformer with --beta-gate: parameters, wiring, CLI, distributed
equivalence, launcher (CPU); GPU vs CPU gradients of one training step."""
import os

import pytest
import torch

from tests.conftest import run_distributed
from tests.test_distributed import _prepare_partitions, make_args
from tests.test_launcher import run_main


def _model(seed=11, **kw):
    from pipegcn_amd.models.transformer import Transformer

    torch.manual_seed(seed)
    # 3 conv layers of widths 12, 12, 5; the last one has a single head
    return Transformer([16, 12, 12, 5], torch.relu, n_heads=4, **kw)


def test_gate_adds_one_weight_per_conv_layer_and_nothing_without_it():
    plain, off, on = _model(), _model(beta=False), _model(beta=True)
    sd_plain, sd_off, sd_on = (m.state_dict() for m in (plain, off, on))
    assert list(sd_off) == list(sd_plain)  # same keys, same draws
    assert all(torch.equal(sd_off[k], v) for k, v in sd_plain.items())
    new = {k: tuple(v.shape) for k, v in sd_on.items() if k not in sd_plain}
    assert new == {f"layers.{i}.linear_beta.weight": (1, 3 * out)
                   for i, out in enumerate((12, 12, 5))}
    for layer in on.layers:
        bound = 1 / (3 * layer.linear_skip.out_features) ** 0.5
        assert layer.linear_beta.weight.abs().max() <= bound


def test_create_model_and_parser_wire_beta_gate():
    from pipegcn_amd import trainer
    from pipegcn_amd.cli import create_parser

    base = ["--dataset", "synth-tiny", "--model", "transformer"]
    assert create_parser(base).beta_gate is False
    assert create_parser(base + ["--beta-gate"]).beta_gate is True
    on = trainer.create_model([8, 8, 3], make_args(model="transformer",
                                                   beta_gate=True))
    off = trainer.create_model([8, 8, 3], make_args(model="transformer"))
    assert all(l.linear_beta is not None for l in on.layers)
    assert all(l.linear_beta is None for l in off.layers)
    for model in ("graphsage", "gcn", "gat", "gatv2"):
        with pytest.raises(NotImplementedError,
                           match="--beta-gate supports --model transformer "
                                 "only"):
            trainer.create_model([8, 8, 3], make_args(model=model,
                                                      beta_gate=True))


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
                     model="transformer", n_heads=4, beta_gate=True)
    args.n_feat, args.n_class, args.n_train = data_stats(ndata)
    s = trainer.run(part, args, device="cpu")
    t = torch.tensor(s["losses"])
    dist.all_reduce(t)
    return t.tolist()


def test_gated_transformer_2part_matches_1part(tmp_path):
    two = run_distributed(_worker, 2, args=(str(tmp_path),))[0]
    one = run_distributed(_worker, 1, args=(str(tmp_path),))[0]
    for a, b in zip(one, two):
        assert abs(a - b) / max(abs(a), 1e-9) < 2e-3, (one, two)
    assert two[-1] < two[0]


def test_main_beta_gate_saves_checkpoint(tmp_path):
    out = run_main(tmp_path, ["--model", "transformer", "--n-heads", "2",
                              "--beta-gate", "--enable-pipeline"])
    assert "nan" not in out and "Validation Accuracy" in out
    assert "model saved" in out
    ckpt = tmp_path / "model" / "synth-tiny-2-metis-vol-trans_final.pth.tar"
    sd = torch.load(ckpt, weights_only=True)
    n_hidden = sd["layers.0.linear_q.weight"].shape[0]
    n_class = sd["layers.1.linear_q.weight"].shape[0]
    assert sd["layers.0.linear_beta.weight"].shape == (1, 3 * n_hidden)
    assert sd["layers.1.linear_beta.weight"].shape == (1, 3 * n_class)


def _fwd_bwd(device):
    """tests/test_transformer_model.py's training step with the gate on."""
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
                        train_size=part.n_train, n_heads=4, attn_drop=0.3,
                        beta=True).to(device)
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
    assert torch.allclose(gpu_logits, cpu_logits, atol=1e-4, rtol=1e-4)
    assert "layers.1.linear_beta.weight" in gpu_grads
    for k, ref in cpu_grads.items():
        err = (gpu_grads[k] - ref).abs().max() / ref.abs().max()
        assert err < 1e-4, (k, err.item())
    return True


@pytest.mark.gpu
def test_gated_transformer_gpu_matches_cpu():
    run_distributed(_gpu_vs_cpu_worker, 1, timeout=600)
