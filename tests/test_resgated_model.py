"""Residual gated graph conv model: wiring, refusals, state dict, launcher and
distributed equivalence (CPU); GPU training in fp32 and bf16. Mirrors
tests/test_transformer_model.py."""
import functools
import os

import pytest
import torch

from tests.conftest import run_distributed
from tests.test_distributed import _prepare_partitions, make_args
from tests.test_launcher import run_main

KEYS = ("linear_k.weight", "linear_k.bias", "linear_qv.weight",
        "linear_skip.weight", "linear_skip.bias")


def test_parser_create_model_and_state_dict():
    from pipegcn_amd import trainer
    from pipegcn_amd.cli import create_parser
    from pipegcn_amd.models.resgated import ResGated, ResGatedLayer

    assert create_parser(["--model", "resgated"]).model == "resgated"
    model = trainer.create_model(
        [12, 8, 8, 3], make_args(model="resgated", n_hidden=8, n_heads=3,
                                 attn_drop=0.5))  # neither is read
    assert isinstance(model, ResGated)
    assert all(isinstance(l, ResGatedLayer) for l in model.layers)
    want = {f"norm.{i}.{p}": (8,) for i in (0, 1) for p in ("weight", "bias")}
    for i, (fin, fout) in enumerate(((12, 8), (8, 8), (8, 3))):
        shapes = ((fout, fin), (fout,), (2 * fout, fin), (fout, fin), (fout,))
        want.update({f"layers.{i}.{key}": s for key, s in zip(KEYS, shapes)})
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == want
    assert all(p.abs().max() <= 12 ** -0.5
               for p in model.layers[0].parameters())


def test_resgated_refusals():
    from pipegcn_amd import trainer
    from pipegcn_amd.models.resgated import ResGated

    def create(**kw):
        return trainer.create_model([8, 8, 3], make_args(model="resgated",
                                                         **kw))

    with pytest.raises(NotImplementedError, match="graphsage only"):
        ResGated([8, 8, 3], torch.relu, use_pp=True)
    with pytest.raises(NotImplementedError, match="graphsage only"):
        create(use_pp=True)
    with pytest.raises(NotImplementedError, match="graphsage only"):
        trainer.precompute(None, make_args(model="resgated", use_pp=True))
    with pytest.raises(NotImplementedError,
                       match="--edge-drop does not combine with --model "
                             "resgated"):
        create(edge_drop=0.2)
    with pytest.raises(NotImplementedError,
                       match="--beta-gate supports --model transformer only"):
        create(beta_gate=True)
    with pytest.raises(NotImplementedError,
                       match="--aggregator pool supports graphsage only"):
        create(aggregator="pool")


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
                     model="resgated")
    args.n_feat, args.n_class, args.n_train = data_stats(ndata)
    s = trainer.run(part, args, device="cpu")
    t = torch.tensor(s["losses"])
    dist.all_reduce(t)
    return t.tolist()


def test_resgated_2part_matches_1part(tmp_path):
    two = run_distributed(_worker, 2, args=(str(tmp_path),))[0]
    one = run_distributed(_worker, 1, args=(str(tmp_path),))[0]
    for a, b in zip(one, two):
        assert abs(a - b) / max(abs(a), 1e-9) < 2e-3, (one, two)
    assert two[-1] < two[0]


def test_main_resgated_pipelined_saves_checkpoint(tmp_path):
    out = run_main(tmp_path, ["--model", "resgated", "--enable-pipeline"])
    assert "Epoch" in out and "nan" not in out
    assert "Validation Accuracy" in out and "model saved" in out
    ckpt = tmp_path / "model" / "synth-tiny-2-metis-vol-trans_final.pth.tar"
    sd = torch.load(ckpt, weights_only=True)
    for i in (0, 1):
        for key in KEYS:
            assert f"layers.{i}.{key}" in sd, (i, key)
    n_hidden = sd["layers.0.linear_k.weight"].shape[0]
    assert sd["layers.0.linear_qv.weight"].shape[0] == 2 * n_hidden


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_resgated_gpu_training(tmp_path, dtype):
    """The loss is finite and falls (the worker asserts both)."""
    from tests.test_gpu_distributed import _train_gpu_worker

    worker = functools.partial(_train_gpu_worker, model="resgated",
                               dtype=dtype)
    run_distributed(worker, 1, args=(str(tmp_path),), timeout=900)
