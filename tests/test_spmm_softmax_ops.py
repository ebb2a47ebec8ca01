"""Softmax aggregation: ops.spmm_softmax / ops.spmm_softmax_csr on the CPU
path and on the gfx950 kernels (csrc/hip/spmm_softmax.hip).

The reference is written here, dense and float64, independent of the library:
a counts matrix cnt[n_dst, n_src], the masked softmax of beta * x per column
with weights cnt, out = sum w x / sum w (zeros on empty rows), grad_x and
grad_beta from float64 autograd. out and grad_x: fp32 atol = rtol = 1e-4 (the
project's SpMM tolerance), bf16 max error over the reference's max-norm < 0.02
(test_spmm_bf16_gpu's bound). grad_beta: |got - want| <= tol * S, S the
float64 sum of the absolute per-(edge, column) terms |g w (x_j - out_i) x_j|,
the sum that cancels; tol = 1e-4 (fp32) or 0.02 (bf16). Kind big: x scaled so
that max |beta * x| is tests/test_gat_ops.py's BIG_SCORE = 90; exp(90)
overflows fp32, so a kernel without the running maximum, or with a wrong
rescale, cannot pass.
"""
import dataclasses
import functools

import pytest
import torch

from pipegcn_amd import ops
from tests.test_gat_ops import (BIG_SCORE, EMPTY_ROWS, N_DST, N_SRC, edges,
                                graph)

# ragged lane | one exact chunk | the widest lane load | chunks + ragged tail
WIDTHS = [41, 64, 256, 602]
CASES = [("randn", 1.0), ("randn", -0.7), ("randn", 0.0), ("big", 1.0),
         ("big", -1.0)]
GPU_DTYPES = [torch.float32, torch.bfloat16]
EMPTY = list(EMPTY_ROWS)


@functools.lru_cache(maxsize=None)
def case(F, kind, beta, bf16=False):
    """Inputs and the dense float64 reference, computed once and shared."""
    gen = torch.Generator().manual_seed(7000 + F + len(kind))
    x = torch.randn(N_SRC, F, generator=gen)
    if kind == "big":
        x = x * (BIG_SCORE / abs(beta) / x.abs().max())
    g = torch.randn(N_DST, F, generator=gen)
    if bf16:
        x, g = x.bfloat16().float(), g.bfloat16().float()
    u, v = edges()
    cnt = torch.zeros(N_DST, N_SRC, dtype=torch.float64)
    cnt.index_put_((v, u), torch.ones(u.numel(), dtype=torch.float64),
                   accumulate=True)
    has = cnt.sum(1) > 0
    mask, cw = (cnt > 0).unsqueeze(2), cnt.unsqueeze(2)
    ninf = torch.tensor(float("-inf"), dtype=torch.float64)
    b = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    out = torch.zeros(N_DST, F, dtype=torch.float64)
    dx = torch.zeros(N_SRC, F, dtype=torch.float64)
    dbeta, scale = 0.0, 0.0
    for c0 in range(0, F, 64):  # columns are independent: 64 at a time
        cols = slice(c0, c0 + 64)
        xc = x[:, cols].double().requires_grad_(True)
        gc = g[:, cols].double()
        s = torch.where(mask, (b * xc).unsqueeze(0), ninf)
        m = torch.where(has.view(-1, 1, 1), s.detach().amax(1, keepdim=True),
                        torch.zeros(()).double())
        w = cw * torch.exp(s - m)  # [n_dst, n_src, cols], 0 off the graph
        w = w / torch.where(has.view(-1, 1, 1), w.sum(1, keepdim=True),
                            torch.ones(()).double())
        oc = (w * xc.unsqueeze(0)).sum(1)
        gx, gb = torch.autograd.grad(oc, (xc, b), gc)
        out[:, cols], dx[:, cols] = oc.detach(), gx
        dbeta += gb.item()
        t = xc.detach().unsqueeze(0) - oc.detach().unsqueeze(1)
        scale += (gc.unsqueeze(1) * w.detach() * t
                  * xc.detach().unsqueeze(0)).abs().sum().item()
    assert (out[EMPTY] == 0).all()
    return dict(x=x, g=g, out=out, dx=dx, dbeta=dbeta, scale=scale)


def _close(got, want, dtype):
    err = (got.double().cpu() - want).abs()
    if dtype == torch.float32:  # allclose with atol = rtol = 1e-4
        assert (err <= 1e-4 + 1e-4 * want.abs()).all(), err.max()
    else:
        assert err.max() / want.abs().max() < 0.02, err.max()


def _run(device, dtype, F, kind, beta, hg=None):
    c = case(F, kind, beta, dtype == torch.bfloat16)
    hg = hg or graph(device)
    x = c["x"].to(device=device, dtype=dtype).requires_grad_(True)
    b = torch.tensor([beta], device=device, requires_grad=True)
    out = ops.spmm_softmax(hg, x, b)
    assert out.dtype == dtype and out.shape == (N_DST, F)
    _close(out.detach(), c["out"], dtype)
    assert (out.detach()[EMPTY] == 0).all()
    assert torch.equal(ops.spmm_softmax_csr(hg.csr, x.detach(), b.detach()),
                       out.detach())
    with torch.no_grad():
        assert torch.equal(ops.spmm_softmax(hg, x, b), out.detach())
    if beta == 0.0:
        inv_deg = 1.0 / hg.csr.row_degrees().clamp(min=1.0)
        _close(ops.spmm_mean(hg, x.detach(), inv_deg), c["out"], dtype)
    out.backward(c["g"].to(device=device, dtype=dtype))
    assert (x.grad.dtype, x.grad.shape) == (dtype, x.shape)
    assert (b.grad.dtype, b.grad.shape) == (torch.float32, (1,))
    tol = 1e-4 if dtype == torch.float32 else 0.02
    print(kind, beta, F, dtype, "grad_beta", b.grad.item(), "want",
          c["dbeta"], "bound", tol * c["scale"])
    _close(x.grad, c["dx"], dtype)
    assert abs(b.grad.item() - c["dbeta"]) <= tol * c["scale"]
    return out.detach(), x.grad, b.grad


@pytest.mark.parametrize("kind,beta", CASES)
@pytest.mark.parametrize("F", WIDTHS)
def test_spmm_softmax_cpu(F, kind, beta):
    _run("cpu", torch.float32, F, kind, beta)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,beta", CASES)
@pytest.mark.parametrize("dtype", GPU_DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", WIDTHS)
def test_spmm_softmax_gpu(F, dtype, kind, beta):
    _run("cuda", dtype, F, kind, beta)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,beta", [("randn", 1.0), ("big", -1.0)])
@pytest.mark.parametrize("dtype,vec", [(torch.float32, 4), (torch.float32, 1),
                                       (torch.bfloat16, 8),
                                       (torch.bfloat16, 2)],
                         ids=["fp32-16B", "fp32-4B", "bf16-16B", "bf16-4B"])
def test_spmm_softmax_gpu_lane_widths(monkeypatch, dtype, vec, kind, beta):
    monkeypatch.setenv("PIPEGCN_SPMM_VEC", str(vec))
    _run("cuda", dtype, 256, kind, beta)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", GPU_DTYPES, ids=["fp32", "bf16"])
def test_spmm_softmax_gpu_natural_row_order(dtype):
    # grad_beta's order of summation follows the row order: tolerance only
    hg = graph("cuda")
    nat = dataclasses.replace(
        hg, csr=dataclasses.replace(hg.csr, row_order=None),
        csc=dataclasses.replace(hg.csc, row_order=None))
    a, b = (_run("cuda", dtype, 602, "randn", -0.7, hg=g) for g in (hg, nat))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("device", ["cpu", pytest.param(
    "cuda", marks=pytest.mark.gpu)])
def test_spmm_softmax_undersized_x_raises_before_launch(device):
    hg = graph(device)
    x = torch.randn(N_SRC - 1, 64, device=device)
    beta = torch.ones(1, device=device)
    with pytest.raises(ValueError, match="spmm_softmax: x has 299 rows but "
                                         "the graph references 300"):
        ops.spmm_softmax(hg, x, beta)
    with pytest.raises(ValueError, match="out-of-bounds GPU gather"):
        ops.spmm_softmax_csr(hg.csr, x, beta)
