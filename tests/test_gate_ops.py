"""Beta gate: ops.gated_residual on the CPU path and on the gfx950 kernels
(csrc/hip/gate.hip) against the published formula in float64.

Tolerance of the GPU tests, per output: max abs error <= 4 x the error of the
eager composition in the working precision (fp32 torch ops on the same
inputs; for bf16 storage fp32 math from the bf16 inputs, rounded once) + one
unit in the last place of the output's dtype at the output's max magnitude
(the factor covers another summation order in the dot and the column sums).

Measured, max abs error against float64 as eager/kernel (eager on the CPU,
kernel on an MI355X; every output and slice: profiles/README.md, "Beta gate"):
  (N, F)   dtype  out              beta             d_r, d_m (max)   dw slices (max)
  1x1      fp32   6.6e-09/6.6e-09  1.8e-09/1.8e-09  7.0e-09/7.0e-09  3.2e-08/2.8e-08
  1x1      bf16   1.6e-03/1.6e-03  1.0e-08/1.0e-08  8.4e-04/8.4e-04  1.7e-08/2.4e-08
  3x41     fp32   1.6e-07/1.6e-07  3.6e-08/3.6e-08  1.9e-07/1.2e-07  1.2e-06/2.2e-06
  3x41     bf16   3.8e-03/3.8e-03  3.2e-08/3.2e-08  5.3e-03/5.3e-03  9.8e-07/1.6e-06
  257x64   fp32   3.7e-07/3.9e-07  7.9e-08/8.4e-08  3.1e-07/3.9e-07  5.5e-05/1.6e-05
  257x64   bf16   7.8e-03/7.8e-03  7.3e-08/8.0e-08  7.7e-03/7.7e-03  5.6e-05/2.0e-05
  130x256  fp32   4.6e-07/4.0e-07  1.1e-07/7.6e-08  3.8e-07/3.1e-07  5.8e-05/2.8e-05
  130x256  bf16   7.8e-03/7.8e-03  9.2e-08/8.2e-08  7.8e-03/7.8e-03  6.3e-05/3.7e-05
  66x1024  fp32   7.4e-07/4.6e-07  1.1e-07/9.0e-08  4.9e-07/4.0e-07  1.1e-04/5.0e-05
  66x1024  bf16   7.8e-03/7.8e-03  1.7e-07/6.6e-08  7.7e-03/7.7e-03  1.0e-04/5.3e-05
  66x1100  fp32   8.8e-07/5.9e-07  1.8e-07/9.1e-08  6.3e-07/3.6e-07  7.4e-05/5.8e-05
  66x1100  bf16   7.8e-03/7.8e-03  1.4e-07/8.4e-08  7.7e-03/7.7e-03  1.2e-04/6.6e-05
  20011x64 fp32   7.4e-07/5.9e-07  1.1e-07/9.1e-08  4.9e-07/5.0e-07  4.5e-03/3.4e-04
  20011x64 bf16   1.5e-02/1.5e-02  1.0e-07/1.2e-07  7.8e-03/7.8e-03  5.6e-03/3.9e-04
"""
import functools

import pytest
import torch

from pipegcn_amd import native, ops

# (N, F): smallest | VEC 1, partial wave, n_class wide | one chunk, rows > a
# block's waves | several held chunks | the register-resident limit | past
# it, partial last chunk | rows > waves in flight for any cap <= 4096 blocks
SHAPES = [(1, 1), (3, 41), (257, 64), (130, 256), (66, 1024), (66, 1100),
          (20011, 64)]
OUTPUTS = ("out", "beta", "d_r", "d_m", "dw_r", "dw_m", "dw_d")


def _published(r, m, w, g):
    """The layer as the paper writes it -> the OUTPUTS, by autograd."""
    r, m, w = (t.detach().clone().requires_grad_() for t in (r, m, w))
    beta = torch.sigmoid(torch.cat([r, m, r - m], 1) @ w.T)
    out = beta * r + (1 - beta) * m
    out.backward(g)
    return dict(zip(OUTPUTS, (out.detach(), beta.detach()[:, 0], r.grad,
                              m.grad, *w.grad.view(3, -1))))


def _folded(r, m, w, g, run):
    """The OUTPUTS of the folded form, out = run(r, m, w); beta comes from
    the forward kernel on the GPU and from torch ops on the CPU."""
    r, m, w = (t.detach().clone().requires_grad_() for t in (r, m, w))
    out = run(r, m, w)
    out.backward(g.to(out.dtype))
    w_r, w_m, w_d = w.detach().float().view(3, -1)
    a, b = w_r + w_d, w_m - w_d
    if r.is_cuda:
        beta = native().gate_fwd(r.detach(), m.detach(), a, b)[1]
    else:
        beta = torch.sigmoid(r.detach() @ a + m.detach() @ b)
    res = dict(zip(OUTPUTS, (out.detach(), beta, r.grad, m.grad,
                             *w.grad.view(3, -1))))
    return {k: v.cpu() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def case(N, F, dtype):
    """Seeded inputs, the float64 reference and the eager composition's
    errors, computed once per case and shared read-only."""
    gen = torch.Generator().manual_seed(1000 * N + F)
    r, m, g = (torch.randn(N, F, generator=gen).to(dtype).float()
               for _ in range(3))
    w = (torch.rand(1, 3 * F, generator=gen) * 2 - 1) / (3 * F) ** 0.5
    ref = _published(r.double(), m.double(), w.double(), g.double())
    eager = _folded(r, m, w, g, lambda r, m, w: ops._gate_mix(
        r, m, w[0, :F] + w[0, 2 * F:], w[0, F:2 * F] - w[0, 2 * F:]))
    for k in ("out", "d_r", "d_m"):  # the one rounding of the storage dtype
        eager[k] = eager[k].to(dtype)
    err = {k: (eager[k].double() - ref[k]).abs().max().item() for k in OUTPUTS}
    return (r, m, w, g), ref, err


def test_gated_residual_cpu_matches_published_formula():
    gen = torch.Generator().manual_seed(5)
    r, m, g = (torch.randn(37, 41, dtype=torch.float64, generator=gen)
               for _ in range(3))
    w = torch.rand(1, 123, dtype=torch.float64, generator=gen) - 0.5
    ref = _published(r, m, w, g)
    r, m, w = (t.clone().requires_grad_() for t in (r, m, w))
    out = ops.gated_residual(r, m, w)
    out.backward(g)
    assert out.dtype == torch.float64
    for got, key in ((out, "out"), (r.grad, "d_r"), (m.grad, "d_m")):
        assert torch.allclose(got, ref[key], rtol=1e-12, atol=1e-13), key
    dw = torch.cat([ref["dw_r"], ref["dw_m"], ref["dw_d"]])
    assert torch.allclose(w.grad[0], dw, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("r,m,w", [
    (torch.randn(4, 6), torch.randn(4, 5), torch.randn(1, 18)),
    (torch.randn(4, 6), torch.randn(4, 6).double(), torch.randn(1, 18)),
    (torch.randn(4, 6), torch.randn(4, 6), torch.randn(3, 6)),
    (torch.randn(6), torch.randn(6), torch.randn(1, 18)),
], ids=["m_shape", "m_dtype", "w_shape", "r_1d"])
def test_gated_residual_rejects_mismatches(r, m, w):
    with pytest.raises(ValueError, match="gated_residual"):
        ops.gated_residual(r, m, w)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,F", SHAPES)
def test_gate_gpu_matches_float64(N, F, dtype):
    (r, m, w, g), ref, eager_err = case(N, F, dtype)
    got = _folded(r.to("cuda", dtype), m.to("cuda", dtype), w.cuda(), g.cuda(),
                  ops.gated_residual)
    assert got["out"].dtype == got["d_r"].dtype == dtype
    assert got["beta"].dtype == got["dw_r"].dtype == torch.float32
    bad = []
    for k in OUTPUTS:
        err = (got[k].double() - ref[k]).abs().max().item()
        ulp = torch.finfo(got[k].dtype).eps * ref[k].abs().max().item()
        print(f"{N}x{F} {dtype} {k}: eager {eager_err[k]:.3e} kernel "
              f"{err:.3e} bound {4 * eager_err[k] + ulp:.3e}")
        if not err <= 4 * eager_err[k] + ulp:
            bad.append((k, err, eager_err[k], ulp))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("N,F", [(20011, 64), (130, 256)])
def test_gate_weight_gradient_is_bitwise_reproducible(N, F):
    (r, m, w, g), _, _ = case(N, F, torch.float32)
    runs = [_folded(r.cuda(), m.cuda(), w.cuda(), g.cuda(),
                    ops.gated_residual) for _ in range(2)]
    for k in ("dw_r", "dw_m", "dw_d"):
        assert torch.equal(runs[0][k], runs[1][k]), k


@pytest.mark.gpu
def test_gate_gpu_without_rows():
    r = torch.zeros(0, 64, device="cuda", requires_grad=True)
    w = torch.ones(1, 192, device="cuda", requires_grad=True)
    out = ops.gated_residual(r, torch.zeros(0, 64, device="cuda"), w)
    out.sum().backward()
    assert out.shape == r.grad.shape == (0, 64)
    assert w.grad.shape == (1, 192) and not w.grad.any()
