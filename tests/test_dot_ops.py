"""Dot-product attention aggregation: ops.dot_aggregate on the CPU path and on
the gfx950 kernels (csrc/hip/dot_attn.hip) against a float64 reference.

The graph is the constructed one of tests/test_gat_ops.py (two empty rows, a
degree-1 row, a 261-edge row starting off a 4-edge boundary, duplicates).

The reference is written here and is independent of the library's CPU path:
a DENSE per-destination softmax over [n_dst, n_src] scores per head (edge
multiplicities as weights) differentiated by torch autograd in float64.

Tolerances:
 - agg: atol = rtol = 1e-4, the project's fp32 SpMM tolerance
   (tests/test_ops.py).
 - d_q, d_kv are differences of like-sized sums, so their error is set by the
   summation, not by the result's size. The yardstick is a plain fp32 torch
   evaluation of the closed form on the edge list (`_eager`); the code under
   test may have 4x its max error against float64, the factor and method of
   tests/test_gat_ops.py and tests/test_gatv2_ops.py.
 - bf16: max error relative to the reference's max-norm < 0.02, the bound of
   test_spmm_bf16_gpu.
"""
import dataclasses
import functools

import pytest
import torch

from pipegcn_amd import native, ops
from pipegcn_amd.graph.csr import HaloGraph
from tests.test_gat_ops import EMPTY_ROWS, N_DST, N_SRC, edges, graph

CAP = ops.DOT_MAX_HEAD_DIM
# (H, D), one per compiled lane layout (VEC, NV, SEG): (1,1,64) | (1,1,16) |
# (4,1,8) | (4,1,32) | (1,8,64) | (1,16,64) | (4,1,16) | (4,1,64) | (1,1,32) |
# (1,2,64) | (1,4,64) | (4,2,64) | (4,4,64), the widest head | the widest
# that is no multiple of 4
SHAPES = [(1, 41), (4, 16), (8, 32), (3, 100), (2, 301), (1, 602), (5, 64),
          (1, 256), (3, 30), (2, 101), (1, 201), (1, 512), (1, CAP),
          (1, CAP - 1)]
# q is scaled so the largest score is exactly this: exp(90) overflows fp32,
# so a missing max-subtraction cannot pass
BIG_SCORE = 90.0
DROP_P, DROP_SEED = 0.5, 1234
GRADS = ("d_q", "d_kv")


def _heads(q, kv, H):
    """q, K, V as [nodes, H, D] views."""
    F = q.shape[1]
    return (q.view(N_DST, H, -1), kv[:, :F].reshape(N_SRC, H, -1),
            kv[:, F:].reshape(N_SRC, H, -1))


def _dense_attention(q, kv, H, w=None):
    """float64 dense softmax -> agg, autograd-capable."""
    u, v = edges()
    cnt = torch.zeros(N_DST, N_SRC, dtype=torch.float64)
    cnt.index_put_((v, u), torch.ones(u.numel(), dtype=torch.float64),
                   accumulate=True)
    qh, kh, vh = _heads(q, kv, H)
    outs = []
    for h in range(H):
        s = (qh[:, h] @ kh[:, h].T) / qh.shape[2] ** 0.5
        s = torch.where(cnt > 0, s, torch.full_like(s, -float("inf")))
        top = s.detach().max(1).values
        top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
        e = cnt * torch.exp(s - top.unsqueeze(1))
        den = e.sum(1)
        alpha = e / torch.where(den > 0, den, torch.ones_like(den)).unsqueeze(1)
        if w is not None:
            alpha = alpha * w[:, :, h]
        outs.append(alpha @ vh[:, h])
    return torch.cat(outs, 1)


@functools.lru_cache(maxsize=None)
def case(H, D, big=False, bf16=False, p=0.0):
    """Seeded inputs and the float64 dense reference, computed once per shape
    and shared (read-only) by every test that needs them."""
    gen = torch.Generator().manual_seed(1000 * H + D)
    q = torch.randn(N_DST, H * D, generator=gen)
    kv = torch.randn(N_SRC, 2 * H * D, generator=gen)
    g = torch.randn(N_DST, H * D, generator=gen)
    if big:
        u, v = edges()
        qh, kh, _ = _heads(q.double(), kv.double(), H)
        s = (qh[v] * kh[u]).sum(-1) / D ** 0.5
        q = (q.double() * (BIG_SCORE / s.max())).float()
    if bf16:
        q, kv, g = (t.to(torch.bfloat16).float() for t in (q, kv, g))
    w = None
    if p > 0:  # w_uvh = keep / (1 - p) for every (v, u) pair
        vv = torch.arange(N_DST).repeat_interleave(N_SRC)
        uu = torch.arange(N_SRC).repeat(N_DST)
        keep = ops.gat_dropout_keep(uu, vv, H, DROP_SEED, p)
        w = keep.view(N_DST, N_SRC, H).double() / (1.0 - p)
    q64, kv64 = (t.double().requires_grad_(True) for t in (q, kv))
    agg = _dense_attention(q64, kv64, H, w)
    d_q, d_kv = torch.autograd.grad(agg, (q64, kv64), g.double())
    ref = dict(agg=agg.detach(), d_q=d_q, d_kv=d_kv)
    for t in ref.values():
        assert torch.isfinite(t).all()
    return dict(q=q, kv=kv, g=g, ref=ref)


def _eager(c, H, p=0.0):
    """The two gradients from the closed form in plain fp32 torch ops on the
    edge list: the yardstick for the summation error."""
    u, v = edges()
    qh, kh, vh = _heads(c["q"], c["kv"], H)
    gh = c["g"].view(N_DST, H, -1)
    scale = 1.0 / qh.shape[2] ** 0.5
    s = (qh[v] * kh[u]).sum(-1) * scale
    top = torch.zeros(N_DST, H).scatter_reduce(
        0, v.unsqueeze(1).expand_as(s), s, "amax", include_self=False)
    den = torch.zeros(N_DST, H).index_add(0, v, torch.exp(s - top[v]))
    alpha = torch.exp(s - (top + torch.log(den.clamp(min=1e-38)))[v])
    w = torch.ones_like(alpha)
    if p > 0:
        w = ops.gat_dropout_keep(u, v, H, DROP_SEED, p).float() / (1.0 - p)
    wa = (w * alpha).unsqueeze(-1)
    t = (gh * torch.zeros_like(gh).index_add(0, v, wa * vh[u])).sum(-1)
    delta = (alpha * (w * (gh[v] * vh[u]).sum(-1) - t[v])).unsqueeze(-1)
    d_q = scale * torch.zeros_like(qh).index_add(0, v, delta * kh[u])
    d_k = scale * torch.zeros_like(kh).index_add(0, u, delta * qh[v])
    d_v = torch.zeros_like(vh).index_add(0, u, wa * gh[v])
    return dict(d_q=d_q.reshape(N_DST, -1),
                d_kv=torch.cat((d_k.reshape(N_SRC, -1),
                                d_v.reshape(N_SRC, -1)), 1))


def _run(c, H, device, dtype=torch.float32, hg=None, p=0.0):
    hg = hg if hg is not None else graph(device)
    # fresh leaves: the cached case tensors are shared and stay untouched
    q, kv = (c[k].to(device=device, dtype=dtype).clone().requires_grad_(True)
             for k in ("q", "kv"))
    agg = ops.dot_aggregate(hg, q, kv, H, attn_drop=p,
                            seed=DROP_SEED if p > 0 else None)
    agg.backward(c["g"].to(device=device, dtype=dtype))
    return dict(agg=agg.detach(), d_q=q.grad, d_kv=kv.grad)


def _err(a, ref):
    return (a.double().cpu() - ref).abs().max().item()


def _check(device, H, D, big=False, p=0.0):
    c = case(H, D, big, False, p)
    ref = c["ref"]
    got = _run(c, H, device, p=p)
    for t in got.values():
        assert torch.isfinite(t).all()
    assert (got["agg"][list(EMPTY_ROWS)] == 0).all(), "empty rows: zero"
    assert (got["d_q"][list(EMPTY_ROWS)] == 0).all()
    assert torch.allclose(got["agg"].double().cpu(), ref["agg"], atol=1e-4,
                          rtol=1e-4), _err(got["agg"], ref["agg"])
    eager = _eager(c, H, p=p)
    for name in GRADS:
        e_eager, e_got = _err(eager[name], ref[name]), _err(got[name],
                                                            ref[name])
        print(f"{device} H={H} D={D} big={big} p={p} {name}: eager fp32 err "
              f"{e_eager:.3e}, got {e_got:.3e}")
        assert e_got <= 4 * e_eager, (name, e_got, e_eager)


@pytest.mark.parametrize("H,D", SHAPES)
def test_dot_aggregate_cpu(H, D):
    _check("cpu", H, D)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", SHAPES)
def test_dot_aggregate_gpu(H, D):
    _check("cuda", H, D)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", [(4, 16), (2, 301)])
def test_dot_aggregate_large_scores_gpu(H, D):
    _check("cuda", H, D, big=True)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", [(4, 16), (2, 301)])
def test_dot_attn_dropout_gpu(H, D):
    """d_kv comes from the CSC pass: it matches only if that pass draws the
    bits the CSR pass (and ops.gat_dropout_keep) drew."""
    _check("cuda", H, D, p=DROP_P)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", [(4, 16), (8, 32)])
def test_dot_aggregate_bf16_gpu(H, D):
    c = case(H, D, bf16=True)
    got = _run(c, H, "cuda", torch.bfloat16)
    for name, t in got.items():
        assert t.dtype == torch.bfloat16, name
        ref = c["ref"][name]
        err = _err(t, ref) / ref.abs().max().item()
        print(f"bf16 H={H} D={D} {name}: rel err {err:.3e}")
        assert err < 0.02, (name, err)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, DROP_P])
@pytest.mark.parametrize("H,D", [(4, 16), (2, 301)])
def test_dot_row_order_gpu(H, D, p):
    """Bitwise equal with or without the LPT row order: each row's edges are
    walked in CSR/CSC order by a fixed set of lanes."""
    c = case(H, D)
    hg = graph("cuda")
    assert hg.csr.row_order is not None and hg.csc.row_order is not None
    natural = HaloGraph(dataclasses.replace(hg.csr, row_order=None),
                        dataclasses.replace(hg.csc, row_order=None),
                        hg.num_in, hg.num_all)
    lpt, plain = _run(c, H, "cuda", p=p), _run(c, H, "cuda", hg=natural, p=p)
    for k in lpt:
        assert torch.equal(lpt[k], plain[k]), k


@pytest.mark.gpu
def test_dot_guards_gpu():
    """Each refused before any launch; the native entry guards itself too."""
    c = case(4, 16)
    hg = graph("cuda")
    q, kv = c["q"].cuda(), c["kv"].cuda()
    with pytest.raises(ValueError, match="2F"):
        ops.dot_aggregate(hg, q, kv[:, :64].contiguous(), 4)
    with pytest.raises(ValueError, match="destination"):
        ops.dot_aggregate(hg, q[:100], kv, 4)
    with pytest.raises(ValueError, match="out-of-bounds"):
        ops.dot_aggregate(hg, q, kv[:100], 4)
    wide_q = torch.zeros(N_DST, CAP + 1, device="cuda")
    wide_kv = torch.zeros(N_SRC, 2 * CAP + 2, device="cuda")
    with pytest.raises(ValueError, match="head width"):
        ops.dot_aggregate(hg, wide_q, wide_kv, 1)
    csr = hg.csr
    with pytest.raises(RuntimeError, match="exceeds"):
        native().dot_fwd(csr.indptr, csr.indices, wide_q, wide_kv,
                         torch.Tensor(), csr.num_cols, 1, 1.0)
    with pytest.raises(RuntimeError, match="rows"):
        native().dot_fwd(csr.indptr, csr.indices, q, kv[:100].contiguous(),
                         torch.Tensor(), csr.num_cols, 4, 0.25)
