"""Multi-aggregation (PNA): ops.spmm_pna / ops.spmm_pna_csr on the CPU path
and on the gfx950 kernels (csrc/hip/spmm_pna.hip).

The reference is written here, dense and float64, independent of the library:
a counts matrix cnt[n_dst, n_src], mean = cnt x / d, the variance CENTRED
(sum cnt (x - mean)^2 / d), std = sqrt(relu(var) + 1e-5), max and min by a
masked reduction, and the expected args by the first-edge rule of
tests/test_spmm_max_ops.py. The reference gradient is float64 autograd through
self, mean and std plus index_put_(accumulate=True) of g_max / g_min by the
expected args.

self, max, min and both args are compared EXACTLY on every dtype. mean, std
and grad_x: fp32 atol = rtol = 1e-4 (the project's SpMM tolerance), bf16 max
error over the reference's max-norm < 0.02 (test_spmm_bf16_gpu's bound).

Kinds of input: randn; tie (integers in [-3, 3]: extrema attained many times
and through parallel edges); offset (1000 + randn), FORWARD ONLY: an
unshifted S2 / d - mean^2 cannot pass it. Its backward is excluded on
purpose: the gradient through mean and std is formed as sum P + x * sum Q,
which cancels when |mean| >> std (docs/DESIGN.md, "Multi-aggregation (PNA)").
"""
import dataclasses
import functools

import pytest
import torch

from pipegcn_amd import ops
from tests.test_gat_ops import EMPTY_ROWS, N_DST, N_SRC, edges, graph

# one ragged element per lane | one exact chunk | the widest lane load |
# multi-chunk with a ragged tail and unaligned block offsets k * 602
WIDTHS = [41, 64, 256, 602]
KINDS = ["randn", "tie"]
GPU_DTYPES = [torch.float32, torch.bfloat16]
EMPTY = list(EMPTY_ROWS)


@functools.lru_cache(maxsize=None)
def case(F, kind, bf16=False):
    """Seeded inputs and the dense float64 reference, computed once per
    (width, kind, dtype) and shared read-only."""
    gen = torch.Generator().manual_seed(9000 + F + len(kind))
    if kind == "tie":
        x = torch.randint(-3, 4, (N_SRC, F), generator=gen).float()
    else:
        x = torch.randn(N_SRC, F, generator=gen)
        if kind == "offset":
            x = x + 1000.0
    g = torch.randn(N_DST, 5, F, generator=gen)
    if bf16:
        x, g = x.bfloat16().float(), g.bfloat16().float()
    u, v = edges()
    cnt = torch.zeros(N_DST, N_SRC, dtype=torch.float64)
    cnt.index_put_((v, u), torch.ones(u.numel(), dtype=torch.float64),
                   accumulate=True)
    d = cnt.sum(1, keepdim=True)
    has, dc, mask = d > 0, d.clamp(min=1.0), (cnt > 0).unsqueeze(2)
    out = torch.zeros(N_DST, 5, F, dtype=torch.float64)
    dx = torch.zeros(N_SRC, F, dtype=torch.float64)
    inf = torch.tensor(float("inf"), dtype=torch.float64)
    for c0 in range(0, F, 64):  # columns are independent: 64 at a time
        cols = slice(c0, c0 + 64)
        xc = x[:, cols].double().requires_grad_(True)
        mean = cnt @ xc / dc
        dev = xc.unsqueeze(0) - mean.unsqueeze(1)  # [n_dst, n_src, cols]
        var = (cnt.unsqueeze(2) * dev * dev).sum(1) / dc
        std = torch.sqrt(torch.relu(var) + 1e-5) * has
        diff = [xc[:N_DST], mean, std]
        dx[:, cols] = torch.autograd.grad(
            diff, xc, [g[:, k, cols].double() for k in (0, 1, 4)])[0]
        xm = xc.detach().unsqueeze(0)
        for k, t in zip((0, 1, 4), diff):
            out[:, k, cols] = t.detach()
        out[:, 2, cols] = torch.where(mask, xm, -inf).max(1).values
        out[:, 3, cols] = torch.where(mask, xm, inf).min(1).values
    out[EMPTY, 1:] = 0.0
    # the first edge of each row, in stored order, that equals the extremum
    csr = graph("cpu").csr
    arg = torch.full((N_DST, 2, F), -1, dtype=torch.int32)
    for r in range(N_DST):
        ids = csr.indices[csr.indptr[r]:csr.indptr[r + 1]].long()
        for k in (0, 1):
            if ids.numel():
                hit = x[ids].double() == out[r, 2 + k]  # [deg, F]
                assert hit.any(0).all()
                arg[r, k] = ids[hit.int().argmax(0)].int()
    ext = torch.zeros(N_SRC, F, dtype=torch.float64)
    for k in (0, 1):
        rows, cols = (arg[:, k] >= 0).nonzero(as_tuple=True)
        ext.index_put_((arg[rows, k, cols].long(), cols),
                       g[rows, 2 + k, cols].double(), accumulate=True)
    return dict(x=x, g=g.reshape(N_DST, 5 * F), out=out, dx=dx + ext,
                arg=arg.reshape(N_DST, 2 * F), nonempty=has.squeeze(1))


def _close(got, want, dtype):
    got = got.double().cpu()
    if dtype == torch.float32:
        assert torch.allclose(got, want, atol=1e-4, rtol=1e-4), \
            (got - want).abs().max()
    else:
        err = (got - want).abs().max() / want.abs().max()
        assert err < 0.02, err


def _run(device, dtype, F, kind, backward=True):
    c = case(F, kind, dtype == torch.bfloat16)
    hg = graph(device)
    x = c["x"].to(device=device, dtype=dtype).requires_grad_(backward)
    out = ops.spmm_pna(hg, x)
    assert out.dtype == dtype and out.shape == (N_DST, 5 * F)
    o = out.detach().double().cpu().view(N_DST, 5, F)
    for k in (0, 2, 3):  # self, max, min: one of the inputs
        assert torch.equal(o[:, k], c["out"][:, k]), k
    for k in (1, 4):
        print(kind, F, dtype, "mean" if k == 1 else "std", "max err",
              (o[:, k] - c["out"][:, k]).abs().max().item())
        _close(o[:, k], c["out"][:, k], dtype)
    assert (o[EMPTY, 1:] == 0).all()

    out2, arg, stat = ops.spmm_pna_csr(hg.csr, x.detach(), with_state=True)
    assert arg.dtype == torch.int32 and stat.dtype == torch.float32
    assert torch.equal(arg.cpu(), c["arg"])
    assert (arg[EMPTY] == -1).all() and (stat[EMPTY] == 0).all()
    assert torch.equal(out2, out.detach())
    # the forwards that keep no state: same out
    assert torch.equal(ops.spmm_pna_csr(hg.csr, x.detach()), out.detach())
    with torch.no_grad():
        assert torch.equal(ops.spmm_pna(hg, x), out.detach())
    if backward:
        g = c["g"].to(device=device, dtype=dtype)
        out.backward(g)
        assert x.grad.dtype == dtype and x.grad.shape == x.shape
        print(kind, F, dtype, "grad_x max err",
              (x.grad.double().cpu() - c["dx"]).abs().max().item())
        _close(x.grad, c["dx"], dtype)
    if backward and kind == "tie":
        # the extrema part alone: every destination lands exactly once
        g = g.view(N_DST, 5, F).clone()
        g[:, (0, 1, 4)] = 0
        x.grad = None
        ops.spmm_pna(hg, x).backward(g.view(N_DST, 5 * F))
        want = g[c["nonempty"].to(device)][:, 2:4].double().sum((0, 1)).cpu()
        _close(x.grad.double().sum(0), want, dtype)
    return out2, arg, stat


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", WIDTHS)
def test_spmm_pna_cpu(F, kind):
    _run("cpu", torch.float32, F, kind)


@pytest.mark.parametrize("F", [41, 256])
def test_spmm_pna_offset_forward_cpu(F):
    _run("cpu", torch.float32, F, "offset", backward=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", GPU_DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", WIDTHS)
def test_spmm_pna_gpu(F, dtype, kind):
    arg = _run("cuda", dtype, F, kind)[1]
    # GPU and CPU args are identical
    x = case(F, kind, dtype == torch.bfloat16)["x"]
    cpu_arg = ops.spmm_pna_csr(graph("cpu").csr, x, with_state=True)[1]
    assert torch.equal(arg.cpu(), cpu_arg)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [41, 256])
def test_spmm_pna_offset_forward_gpu(F):
    _run("cuda", torch.float32, F, "offset", backward=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,vec", [(torch.float32, 4), (torch.float32, 1),
                                       (torch.bfloat16, 8),
                                       (torch.bfloat16, 2)],
                         ids=["fp32-16B", "fp32-4B", "bf16-16B", "bf16-4B"])
def test_spmm_pna_gpu_lane_widths(monkeypatch, dtype, vec, kind):
    """The lane widths that pick_vec's preference does not reach on a graph
    this small."""
    monkeypatch.setenv("PIPEGCN_SPMM_VEC", str(vec))
    _run("cuda", dtype, 256, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", GPU_DTYPES, ids=["fp32", "bf16"])
def test_spmm_pna_gpu_natural_row_order(dtype):
    x = case(602, "tie", dtype == torch.bfloat16)["x"].to("cuda", dtype)
    csr = graph("cuda").csr
    nat = dataclasses.replace(csr, row_order=None)
    for a, b in zip(ops.spmm_pna_csr(csr, x, with_state=True),
                    ops.spmm_pna_csr(nat, x, with_state=True)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("device", ["cpu", pytest.param(
    "cuda", marks=pytest.mark.gpu)])
def test_spmm_pna_undersized_x_raises_before_launch(device):
    hg = graph(device)
    x = torch.randn(N_SRC - 1, 64, device=device)
    with pytest.raises(ValueError, match="spmm_pna: x has 299 rows but the "
                                         "graph references 300"):
        ops.spmm_pna(hg, x)
    with pytest.raises(ValueError, match="out-of-bounds GPU gather"):
        ops.spmm_pna_csr(hg.csr, x)
