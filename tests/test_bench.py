"""bench.py contract tests — the driver launches this file directly
(`python bench.py --gpus N --steps K --warmup W`) and parses ONE JSON
line; breakage here silently kills the round-end benchmark."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup",
            "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"]


def _run(args, timeout=240):
    r = subprocess.run([sys.executable, "bench.py", "--shape", "small",
                        "--steps", "2", "--warmup", "1"] + args,
                       cwd=REPO, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def test_bench_json_contract():
    d = _run([])
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is False
    assert d["data"] == "synthetic"
    assert d["config"]["parallelism"] == "graph-partition dp1"
    assert d["value"] > 0


@pytest.mark.parametrize("extra", [["--model", "gcn"],
                                   ["--use-pp"],
                                   ["--no-pipeline"],
                                   ["--feat-corr", "--grad-corr"],
                                   ["--norm", "batch"]])
def test_bench_variants(extra):
    d = _run(extra)
    assert d["value"] > 0


def _load_dump(d):
    import numpy as np

    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dump"))
    res = _run(["--full", "--dump-outputs", d])
    return res, _load_dump(d)


def test_bench_dump_outputs_contract(dumped):
    """--dump-outputs writes the last timed step's results as float .npy
    files within the 64 MB budget; --full is accepted and keeps the line."""
    import numpy as np

    res, arrs = dumped
    for k in REQUIRED:
        assert k in res, k
    assert res["steps"] == 2
    assert {"logits.npy", "loss.npy"} <= set(arrs)
    assert any(f.startswith("param.") for f in arrs)
    assert all(f.endswith(".npy") for f in arrs)
    for f, a in arrs.items():
        assert a.dtype in (np.float32, np.float64), (f, a.dtype)
        assert np.isfinite(a).all(), f
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 2**20
    assert arrs["logits.npy"].ndim == 2
    assert arrs["logits.npy"].shape[1] == res["config"]["n_class"]
    assert arrs["loss.npy"].size == 1


def test_bench_dump_outputs_repeatable(dumped, tmp_path):
    """Same arguments -> same inputs: a second run reproduces the dump (up
    to fp32 reduction-order noise over the 3 epochs run)."""
    import numpy as np

    _, first = dumped
    _run(["--dump-outputs", str(tmp_path)])
    second = _load_dump(str(tmp_path))
    assert set(first) == set(second)
    for f in first:
        assert first[f].shape == second[f].shape, f
        np.testing.assert_allclose(second[f], first[f], rtol=1e-3,
                                   atol=1e-4, err_msg=f)


def test_bench_dump_outputs_budget(tmp_path):
    """Outputs over the budget are cut to a fixed row subset per array."""
    import numpy as np
    import torch

    sys.path.insert(0, REPO)
    try:
        import bench
    finally:
        sys.path.remove(REPO)
    big = torch.arange(3 * 2**20 * 8, dtype=torch.float32).reshape(-1, 8)
    small = torch.ones(5, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path),
                       {"big": big, "small": small, "s": big.sum()})
    a = _load_dump(str(tmp_path))
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_BUDGET_BYTES
    assert a["big.npy"].dtype == np.float32
    assert a["small.npy"].dtype == np.float64
    assert a["big.npy"].shape[1] == 8 and a["big.npy"].shape[0] > 2**20
    # rows are an evenly strided, run-independent pick starting at row 0
    assert a["big.npy"][0, 0] == 0.0
    assert np.all(np.diff(a["big.npy"][:, 0]) > 0)


def test_bench_world2_gloo():
    """The exact launch pattern the driver uses for N>1, pinned to CPU/gloo
    so it runs the same on a host with fewer GPUs than ranks (the default
    device is cuda:<local rank> wherever a GPU is visible)."""
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29591", "bench.py", "--gpus", "2", "--shape",
         "small", "--steps", "2", "--warmup", "1", "--device", "cpu"],
        cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2
    assert d["config"]["boundary_comm_overlap_pct"] is not None
