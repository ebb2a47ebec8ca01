"""Residual gated aggregation: ops.resgated_aggregate / _csr on the CPU path
and on the gfx950 kernels (csrc/hip/resgated.hip).

The reference is written here, dense and float64, independent of the library:
a counts matrix cnt[n_dst, n_src] and
out[v] = inv_deg[v] * sum_u cnt[v,u] sigmoid(k[v] + Q[u]) V[u], a column block
at a time; d_k and d_qv from float64 autograd. Kind big: k and Q scaled so
that max |k + Q| over the edges is tests/test_gat_ops.py's BIG_SCORE = 90;
exp(90) overflows fp32, so a gate or an s (1 - s) formed from e / (1 + e)^2
gives NaN there.

Tolerances: fp32 atol = rtol = 1e-4, bf16 max error over the reference's
max-norm < 0.02 with the inputs rounded to bf16 first. d_k and dQ are sums of
signed products; a plain fp32 torch evaluation of their closed form on the
edge list stays inside the fp32 bound at every case here (worst max error
against float64: 8.5e-6), so no case needed tests/test_gat_ops.py's 4x
yardstick and none uses it.
"""
import dataclasses
import functools

import pytest
import torch

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import HaloGraph
from tests.test_gat_ops import (BIG_SCORE, EMPTY_ROWS, N_DST, N_SRC, edges,
                                graph)

# ragged 4-byte lanes | one exact chunk | the preferred lane load | chunks, a
# ragged tail and a half-row that is 8- but not 16-byte aligned
WIDTHS = [41, 64, 256, 602]
KINDS = ["randn", "big"]
GPU_DTYPES = [torch.float32, torch.bfloat16]
EMPTY = list(EMPTY_ROWS)
FREE_SRC = 4  # sources past N_SRC that no edge references (`wide_graph`)


@functools.lru_cache(maxsize=None)
def wide_graph(device):
    """test_gat_ops's edges over FREE_SRC more sources: CSC rows without
    entries."""
    u, v = edges()
    return HaloGraph.from_edges(u, v, N_DST, N_SRC + FREE_SRC).to(device)


def _inv_deg(mean):
    deg = torch.bincount(edges()[1], minlength=N_DST).float()
    return (1.0 / deg.clamp(min=1.0)) if mean else None


@functools.lru_cache(maxsize=None)
def case(F, kind, mean, bf16=False):
    """Inputs and the dense float64 reference, computed once and shared."""
    gen = torch.Generator().manual_seed(9000 + F + len(kind))
    k = torch.randn(N_DST, F, generator=gen)
    qv = torch.randn(N_SRC, 2 * F, generator=gen)
    g = torch.randn(N_DST, F, generator=gen)
    u, v = edges()
    if kind == "big":
        c = BIG_SCORE / (k[v] + qv[u, :F]).abs().max()
        k, qv = k * c, torch.cat((qv[:, :F] * c, qv[:, F:]), 1)
    if bf16:
        k, qv, g = (t.bfloat16().float() for t in (k, qv, g))
    cnt = torch.zeros(N_DST, N_SRC, dtype=torch.float64)
    cnt.index_put_((v, u), torch.ones(u.numel(), dtype=torch.float64),
                   accumulate=True)
    inv = _inv_deg(mean)
    scale = (inv.double() if mean else torch.ones(N_DST).double()).view(-1, 1)
    out, d_k = (torch.zeros(N_DST, F, dtype=torch.float64) for _ in "ab")
    d_qv = torch.zeros(N_SRC, 2 * F, dtype=torch.float64)
    for c0 in range(0, F, 64):  # columns are independent: 64 at a time
        cols = slice(c0, min(c0 + 64, F))
        kc, qc, vc = (t.double().requires_grad_(True) for t in (
            k[:, cols], qv[:, cols], qv[:, F + cols.start:F + cols.stop]))
        s = torch.sigmoid(kc.unsqueeze(1) + qc.unsqueeze(0))
        oc = (cnt.unsqueeze(2) * s * vc.unsqueeze(0)).sum(1) * scale
        gk, gq, gv = torch.autograd.grad(oc, (kc, qc, vc), g[:, cols].double())
        out[:, cols], d_k[:, cols] = oc.detach(), gk
        d_qv[:, cols], d_qv[:, F + cols.start:F + cols.stop] = gq, gv
    assert (out[EMPTY] == 0).all() and torch.isfinite(d_qv).all()
    return dict(k=k, qv=qv, g=g, inv=inv, out=out, d_k=d_k, d_qv=d_qv)


def _close(name, got, want, dtype):
    err = (got.double().cpu() - want).abs()
    if dtype == torch.bfloat16:
        assert err.max() / want.abs().max() < 0.02, (name, err.max())
    else:
        assert (err <= 1e-4 + 1e-4 * want.abs()).all(), (name, err.max())


def _run(device, dtype, F, kind, mean, hg=None):
    c = case(F, kind, mean, dtype == torch.bfloat16)
    hg = hg or graph(device)
    # fresh leaves: the cached case tensors are shared and stay untouched
    k, qv = (c[n].to(device=device, dtype=dtype).clone().requires_grad_(True)
             for n in ("k", "qv"))
    if hg.num_all > N_SRC:
        qv = torch.cat((qv.detach(), torch.ones(
            hg.num_all - N_SRC, 2 * F, device=device, dtype=dtype))
        ).requires_grad_(True)
    inv = c["inv"].to(device) if mean else None
    out = ops.resgated_aggregate(hg, k, qv, inv)
    assert out.dtype == dtype and out.shape == (N_DST, F)
    assert torch.equal(ops.resgated_aggregate_csr(
        hg.csr, k.detach(), qv.detach(), inv), out.detach())
    with torch.no_grad():
        assert torch.equal(ops.resgated_aggregate(hg, k, qv, inv),
                           out.detach())
    out.backward(c["g"].to(device=device, dtype=dtype))
    d_k, d_qv = k.grad, qv.grad
    assert (d_k.dtype, d_k.shape) == (dtype, k.shape)
    assert (d_qv.dtype, d_qv.shape) == (dtype, qv.shape)
    for t in (out, d_k, d_qv):
        assert torch.isfinite(t).all()
    assert (out.detach()[EMPTY] == 0).all() and (d_k[EMPTY] == 0).all()
    assert (d_qv[N_SRC:] == 0).all()
    _close("out", out.detach(), c["out"], dtype)
    _close("d_k", d_k, c["d_k"], dtype)
    _close("dQ", d_qv[:N_SRC, :F], c["d_qv"][:, :F], dtype)
    _close("dV", d_qv[:N_SRC, F:], c["d_qv"][:, F:], dtype)
    return out.detach(), d_k, d_qv


@pytest.mark.parametrize("mean", [True, False], ids=["mean", "sum"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", WIDTHS)
def test_resgated_cpu(F, kind, mean):
    _run("cpu", torch.float32, F, kind, mean)


@pytest.mark.gpu
@pytest.mark.parametrize("mean", [True, False], ids=["mean", "sum"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", GPU_DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", WIDTHS)
def test_resgated_gpu(F, dtype, kind, mean):
    first = _run("cuda", dtype, F, kind, mean)
    again = _run("cuda", dtype, F, kind, mean)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,vec", [(torch.float32, 4), (torch.float32, 1),
                                       (torch.bfloat16, 8),
                                       (torch.bfloat16, 2)],
                         ids=["fp32-16B", "fp32-4B", "bf16-16B", "bf16-4B"])
def test_resgated_gpu_lane_widths(monkeypatch, dtype, vec):
    monkeypatch.setenv("PIPEGCN_SPMM_VEC", str(vec))
    _run("cuda", dtype, 256, "big", True)


@pytest.mark.parametrize("device", ["cpu", pytest.param(
    "cuda", marks=pytest.mark.gpu)])
def test_resgated_sources_without_entries_and_natural_row_order(device):
    """CSC rows without entries give exact zeros, and neither they nor the
    row order change any other row."""
    base = _run(device, torch.float32, 602, "randn", True)
    hg = wide_graph(device)
    nat = dataclasses.replace(
        hg, csr=dataclasses.replace(hg.csr, row_order=None),
        csc=dataclasses.replace(hg.csc, row_order=None))
    for g in (hg, nat):
        out, d_k, d_qv = _run(device, torch.float32, 602, "randn", True, hg=g)
        assert torch.equal(out, base[0]) and torch.equal(d_k, base[1])
        assert torch.equal(d_qv[:N_SRC], base[2])


@pytest.mark.parametrize("device", ["cpu", pytest.param(
    "cuda", marks=pytest.mark.gpu)])
def test_resgated_shape_errors_raise_before_launch(device):
    hg = graph(device)
    k = torch.randn(N_DST, 64, device=device)
    qv = torch.randn(N_SRC, 128, device=device)
    for fn in (lambda *a: ops.resgated_aggregate(hg, *a),
               lambda *a: ops.resgated_aggregate_csr(hg.csr, *a)):
        with pytest.raises(ValueError, match="resgated_aggregate: qv has 299 "
                                             "rows but the graph references "
                                             "300"):
            fn(k, qv[:-1])
        with pytest.raises(ValueError, match=r"resgated_aggregate: qv must "
                                             r"be \[nodes, 2F\]"):
            fn(k, qv[:, :127].contiguous())
        with pytest.raises(ValueError, match="resgated_aggregate: k has 199 "
                                             "rows"):
            fn(k[:-1], qv)
        with pytest.raises(ValueError, match="contiguous and of one dtype"):
            fn(k, qv.bfloat16())
        with pytest.raises(ValueError, match="contiguous and of one dtype"):
            fn(k.t().contiguous().t(), qv)
