"""ops.gcn2_propagate / _csr on the CPU path and on the gfx950 kernels
(csrc/hip/gcn2.hip), against the formula in float64 with index_add_.
Tolerances are tests/test_resgated_ops.py's: fp32 atol = rtol = 1e-4, bf16
max error over the reference's max-norm < 0.02 with the inputs rounded to
bf16 first. The running dh0 buffer is fp32 at both dtypes: the fp32 bound.
"""
import functools

import pytest
import torch

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import HaloGraph

N_SRC, N_DST, ALPHA = 300, 200, 0.3
# the 4-edge batch boundary on both sides, an empty row, a long row
DEGS = (0, 1, 3, 4, 5, 8, 70)
# narrowest lane | one full wave | a tail off the lane width | two chunks
WIDTHS = [4, 64, 130, 256]
BRANCHES = pytest.mark.parametrize("per_edge", [True, False])  # or prescaled


@functools.lru_cache(maxsize=None)
def edges():
    """Row v has DEGS[v % 7] edges from sources below N_SRC - 1 (the last
    source has none); one edge of row 2 is repeated."""
    gen = torch.Generator().manual_seed(0)
    deg = torch.tensor(DEGS)[torch.arange(N_DST) % len(DEGS)]
    v = torch.repeat_interleave(torch.arange(N_DST), deg)
    u = torch.randint(0, N_SRC - 1, (v.numel(),), generator=gen)
    u[1] = u[2]  # row 2's first two edges (row 0 has none, row 1 has one)
    # d over ALL local rows: the in-degree inside, any degree on the halo
    in_deg = torch.cat((deg, torch.randint(1, 50, (N_SRC - N_DST,),
                                           generator=gen))).float()
    return u, v, torch.rsqrt(in_deg.clamp(min=1.0))


@functools.lru_cache(maxsize=None)
def graph(device):
    return HaloGraph.from_edges(*edges()[:2], N_DST, N_SRC).to(device)


@functools.lru_cache(maxsize=None)
def case(F, bf16=False, alpha=ALPHA):
    """Inputs and the float64 reference, computed once and shared."""
    gen = torch.Generator().manual_seed(7000 + F)
    h = torch.randn(N_SRC, F, generator=gen)
    h0, g, buf = (torch.randn(N_DST, F, generator=gen) for _ in "abc")
    if bf16:
        h, h0, g = (t.bfloat16().float() for t in (h, h0, g))
    u, v, d = edges()
    d64 = d.double().unsqueeze(1)
    agg = torch.zeros(N_DST, F, dtype=torch.float64).index_add_(
        0, v, d64[u] * h.double()[u])
    P = (1 - alpha) * d64[:N_DST] * agg + alpha * h0.double()
    gs = (1 - alpha) * d64[:N_DST] * g.double()
    dh = d64 * torch.zeros(N_SRC, F, dtype=torch.float64).index_add_(
        0, u, gs[v])
    return dict(h=h, h0=h0, g=g, buf=buf, d=d, P=P, dh=dh,
                dh0=alpha * g.double())


def _close(name, got, want, dtype):
    err = (got.double().cpu() - want).abs()
    if dtype == torch.bfloat16:
        assert err.max() / want.abs().max() < 0.02, (name, err.max())
    else:
        assert (err <= 1e-4 + 1e-4 * want.abs()).all(), (name, err.max())


def _run(device, dtype, F, per_edge=None):
    c, hg = case(F, dtype == torch.bfloat16), graph(device)
    # fresh leaves: the cached case tensors are shared and stay untouched
    h, h0 = (c[n].to(device=device, dtype=dtype).clone().requires_grad_(True)
             for n in ("h", "h0"))
    d = c["d"].to(device)
    # starts non-zero: a kernel that stores where it should add fails
    buf = c["buf"].to(device).clone() if h.is_cuda else None
    P = ops.gcn2_propagate(hg, h, h0, d, ALPHA, dh0=buf, per_edge=per_edge)
    assert P.dtype == dtype and P.shape == (N_DST, F)
    assert torch.equal(ops.gcn2_propagate_csr(
        hg.csr, h.detach(), h0.detach(), d[:N_DST].contiguous(), d, ALPHA,
        per_edge=per_edge), P.detach())
    P.backward(c["g"].to(device=device, dtype=dtype))
    assert (h.grad.dtype, h.grad.shape) == (dtype, h.shape)
    _close("P", P.detach(), c["P"], dtype)
    _close("dh", h.grad, c["dh"], dtype)
    assert (h.grad[N_SRC - 1] == 0).all()  # the source without edges
    if buf is None:
        _close("dh0", h0.grad, c["dh0"], dtype)
    else:
        assert h0.grad is None and buf.dtype == torch.float32
        _close("dh0", buf, c["buf"].double() + c["dh0"], torch.float32)


@pytest.mark.parametrize("F", WIDTHS)
def test_gcn2_cpu(F):
    _run("cpu", torch.float32, F)


@pytest.mark.gpu
@BRANCHES
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", WIDTHS)
def test_gcn2_gpu(F, dtype, per_edge):
    _run("cuda", dtype, F, per_edge)


@pytest.mark.gpu
@BRANCHES
def test_gcn2_gpu_alpha_edges(per_edge):
    """alpha = 0 is the dense SpMM with both scales (the same products, fma
    contraction may differ: the fp32 bound); alpha = 1 is h0 bit for bit;
    without a running buffer h0's gradient is a plain alpha * dP."""
    c, hg = case(130), graph("cuda")
    h, h0, d, g = (c[n].cuda() for n in ("h", "h0", "d", "g"))
    d_dst = d[:N_DST].contiguous()
    want = (ops.spmm(hg.csr, h, d_dst, src_scale=d) if per_edge
            else ops.spmm(hg.csr, h * d.unsqueeze(1), d_dst))
    _close("alpha=0", ops.gcn2_propagate(hg, h, h0, d, 0.0,
                                         per_edge=per_edge),
           want.double().cpu(), torch.float32)
    assert torch.equal(ops.gcn2_propagate(hg, h, h0, d, 1.0,
                                          per_edge=per_edge), h0)
    h0 = h0.clone().requires_grad_(True)
    ops.gcn2_propagate(hg, h, h0, d, ALPHA, per_edge=per_edge).backward(g)
    _close("dh0", h0.grad, c["dh0"], torch.float32)


@pytest.mark.parametrize("device", ["cpu", pytest.param(
    "cuda", marks=pytest.mark.gpu)])
def test_gcn2_argument_errors_raise_before_launch(device):
    hg = graph(device)
    h, h0 = (torch.randn(n, 64, device=device) for n in (N_SRC, N_DST))
    d = edges()[2].to(device)
    for fn in (lambda *a: ops.gcn2_propagate(hg, *a, d, ALPHA),
               lambda *a: ops.gcn2_propagate_csr(hg.csr, *a, d, d, ALPHA)):
        with pytest.raises(ValueError, match="h has 299 rows but the graph "
                                             ".*out-of-bounds GPU gather"):
            fn(h[:-1], h0)
        with pytest.raises(ValueError, match="200 destination nodes"):
            fn(h, h0[:-1])
        with pytest.raises(ValueError, match="fp32 or bf16"):
            fn(h.double(), h0.double())
