"""GATv2 dynamic-attention aggregation: ops.gatv2_aggregate on the CPU path
and on the gfx950 kernels (csrc/hip/gatv2.hip) against a float64 reference.

The graph is the constructed one of tests/test_gat_ops.py (two empty rows, a
degree-1 row, a 261-edge row starting off a 4-edge boundary, duplicates).

The reference is written here and is independent of the library's CPU path:
a DENSE per-destination softmax over [n_dst, n_src] scores per head (edge
multiplicities as weights) differentiated by torch autograd in float64.

Tolerances:
 - out and lse: atol = rtol = 1e-4, the project's fp32 SpMM tolerance
   (tests/test_ops.py).
 - d_zl, d_zr, d_a are differences of like-sized sums, so their error is set
   by the summation, not by the result's size. The yardstick is a plain fp32
   torch evaluation of the closed form on the edge list (`_eager`); the code
   under test may have 4x its max error against float64, the factor
   tests/test_gat_ops.py uses.
 - bf16: max error relative to the reference's max-norm < 0.02, the bound of
   test_spmm_bf16_gpu.
"""
import dataclasses
import functools

import pytest
import torch

from pipegcn_amd import native, ops
from pipegcn_amd.graph.csr import HaloGraph
from tests.test_gat_ops import (EMPTY_ROWS, N_DST, N_SRC, SLOPE, edges,
                                graph)

# (H, D): one element per lane, ragged | four heads per wave | 4-wide, eight
# heads per wave | 4-wide, two heads per wave, odd head count | 5 and 10
# elements per lane
SHAPES = [(1, 41), (4, 16), (8, 32), (3, 100), (2, 301), (1, 602)]
# every other compiled lane layout, up to the widest supported head: 4-wide
# with 4 heads per wave | one | two | four groups per lane; 1-wide with two |
# four | sixteen groups per lane, and two heads per wave
LAYOUT_SHAPES = [(5, 64), (1, 256), (1, 512), (1, 1024), (2, 101), (1, 201),
                 (1, 1023), (3, 30)]
# attn is scaled so the largest score is exactly this: exp(90) overflows
# fp32, so a missing max-subtraction cannot pass
BIG_SCORE = 90.0
DROP_P, DROP_SEED = 0.5, 1234
GRADS = ("d_zl", "d_zr", "d_a")


def _keep_dense(H, p, seed):
    """w_uvh = keep / (1 - p) for every (v, u) pair: [n_dst, n_src, H]."""
    vv = torch.arange(N_DST).repeat_interleave(N_SRC)
    uu = torch.arange(N_SRC).repeat(N_DST)
    keep = ops.gat_dropout_keep(uu, vv, H, seed, p)
    return keep.view(N_DST, N_SRC, H).double() / (1.0 - p)


def _dense_attention(zl, zr, a, H, w=None):
    """float64 dense softmax -> (out, lse), autograd-capable."""
    u, v = edges()
    cnt = torch.zeros(N_DST, N_SRC, dtype=torch.float64)
    cnt.index_put_((v, u), torch.ones(u.numel(), dtype=torch.float64),
                   accumulate=True)
    mask = cnt > 0
    zlh, zrh = zl.view(N_SRC, H, -1), zr.view(N_DST, H, -1)
    outs, lses = [], []
    for h in range(H):
        x = zlh[:, h].unsqueeze(0) + zrh[:, h].unsqueeze(1)
        s = torch.nn.functional.leaky_relu(x, SLOPE) @ a[h]
        s = torch.where(mask, s, torch.full_like(s, -float("inf")))
        top = s.detach().max(1).values
        top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
        e = cnt * torch.exp(s - top.unsqueeze(1))
        den = e.sum(1)
        nonempty = den > 0
        safe = torch.where(nonempty, den, torch.ones_like(den))
        alpha = e / safe.unsqueeze(1)
        lses.append(torch.where(nonempty, top + torch.log(safe),
                                torch.zeros_like(den)))
        if w is not None:
            alpha = alpha * w[:, :, h]
        outs.append(alpha @ zlh[:, h])
    return torch.cat(outs, 1), torch.stack(lses, 1)


def _inputs(H, D, big, bf16):
    gen = torch.Generator().manual_seed(1000 * H + D)
    zl = torch.randn(N_SRC, H * D, generator=gen)
    zr = torch.randn(N_DST, H * D, generator=gen)
    a = torch.randn(H, D, generator=gen) / D ** 0.5
    g = torch.randn(N_DST, H * D, generator=gen)
    if big:
        u, v = edges()
        x = zl.view(N_SRC, H, D)[u] + zr.view(N_DST, H, D)[v]
        s = (torch.nn.functional.leaky_relu(x.double(), SLOPE)
             * a.double()).sum(-1)
        a = (a.double() * (BIG_SCORE / s.max())).float()
    if bf16:
        zl, zr, a, g = (t.to(torch.bfloat16).float() for t in (zl, zr, a, g))
    return dict(zl=zl, zr=zr, a=a, g=g)


@functools.lru_cache(maxsize=None)
def case(H, D, big=False, bf16=False, p=0.0):
    """Seeded inputs and the float64 dense reference, computed once per shape
    and shared (read-only) by every test that needs them."""
    c = _inputs(H, D, big, bf16)
    zl, zr, a = (c[k].double().requires_grad_(True)
                 for k in ("zl", "zr", "a"))
    w = _keep_dense(H, p, DROP_SEED) if p > 0 else None
    out, lse = _dense_attention(zl, zr, a, H, w)
    d_zl, d_zr, d_a = torch.autograd.grad(out, (zl, zr, a), c["g"].double())
    ref = dict(out=out, lse=lse, d_zl=d_zl, d_zr=d_zr, d_a=d_a)
    ref = {k: t.detach() for k, t in ref.items()}
    for t in ref.values():
        assert torch.isfinite(t).all()
    c["ref"] = ref
    return c


def _eager(c, H, dtype=torch.float32, p=0.0):
    """out, lse and the three gradients from the issue's closed form in plain
    torch ops on the edge list. In fp32 it is the yardstick for the
    summation error; in float64 the reference of the extra layout shapes."""
    u, v = edges()
    zl, zr, a, g = (c[k].to(dtype) for k in ("zl", "zr", "a", "g"))
    zlh, zrh = zl.view(N_SRC, H, -1), zr.view(N_DST, H, -1)
    gh = g.view(N_DST, H, -1)
    x = zlh[u] + zrh[v]
    lk = torch.nn.functional.leaky_relu(x, SLOPE)
    s = (lk * a).sum(-1)
    top = torch.zeros(N_DST, H, dtype=dtype).scatter_reduce(
        0, v.unsqueeze(1).expand_as(s), s, "amax", include_self=False)
    den = torch.zeros(N_DST, H, dtype=dtype).index_add(
        0, v, torch.exp(s - top[v]))
    lse = torch.where(den > 0, top + torch.log(den.clamp(min=1e-38)),
                      torch.zeros_like(den))
    alpha = torch.exp(s - lse[v])
    w = torch.ones_like(alpha)
    if p > 0:
        w = ops.gat_dropout_keep(u, v, H, DROP_SEED, p).to(dtype) / (1.0 - p)
    wa = (w * alpha).unsqueeze(-1)
    out = torch.zeros(N_DST, H, zlh.shape[2], dtype=dtype).index_add(
        0, v, wa * zlh[u])
    t = (gh * out).sum(-1)
    delta = alpha * (w * (gh[v] * zlh[u]).sum(-1) - t[v])
    q = delta.unsqueeze(-1) * a * torch.where(x > 0, 1.0, SLOPE).to(dtype)
    d_zl = torch.zeros_like(zlh).index_add(0, u, wa * gh[v] + q)
    d_zr = torch.zeros_like(zrh).index_add(0, v, q)
    d_a = (delta.unsqueeze(-1) * lk).sum(0)
    return dict(out=out.reshape(N_DST, -1), lse=lse,
                d_zl=d_zl.reshape(N_SRC, -1), d_zr=d_zr.reshape(N_DST, -1),
                d_a=d_a)


def _run(c, H, device, dtype=torch.float32, hg=None, p=0.0):
    hg = hg if hg is not None else graph(device)
    # fresh leaves: the cached case tensors are shared and stay untouched
    zl, zr, a = (c[k].to(device=device, dtype=dtype).clone()
                 .requires_grad_(True) for k in ("zl", "zr", "a"))
    out = ops.gatv2_aggregate(hg, zl, zr, a, H, SLOPE, attn_drop=p,
                              seed=DROP_SEED if p > 0 else None)
    out.backward(c["g"].to(device=device, dtype=dtype))
    return dict(out=out.detach(), d_zl=zl.grad, d_zr=zr.grad, d_a=a.grad)


def _close(a, ref):
    return torch.allclose(a.double().cpu(), ref, atol=1e-4, rtol=1e-4)


def _err(a, ref):
    return (a.double().cpu() - ref).abs().max().item()


def _check(device, H, D, big=False, p=0.0, ref=None):
    c = case(H, D, big, False, p) if ref is None else ref
    ref = c["ref"]
    got = _run(c, H, device, p=p)
    for t in got.values():
        assert torch.isfinite(t).all()
    assert (got["out"][list(EMPTY_ROWS)] == 0).all(), "empty rows: zero"
    assert (got["d_zr"][list(EMPTY_ROWS)] == 0).all()
    assert _close(got["out"], ref["out"]), _err(got["out"], ref["out"])
    eager = _eager(c, H, p=p)
    for name in GRADS:
        e_eager, e_got = _err(eager[name], ref[name]), _err(got[name],
                                                            ref[name])
        print(f"{device} H={H} D={D} big={big} p={p} {name}: eager fp32 err "
              f"{e_eager:.3e}, got {e_got:.3e}")
        # Measured max abs error against float64 as "eager fp32 / kernel on
        # MI355X / CPU path" ("-": GPU-only shape), unit-normal inputs unless
        # "s90" (scores scaled to 90) or "p.5" (attention dropout 0.5):
        #   shape        d_zl                         d_zr                         d_a
        #   (1,41)       7.15e-07 6.92e-07 3.40e-07   3.89e-07 3.08e-07 2.53e-07   1.22e-05 1.90e-05 1.14e-05
        #   (4,16)       9.34e-07 1.19e-06 5.87e-07   5.77e-07 4.72e-07 4.08e-07   1.03e-05 1.75e-05 8.63e-06
        #   (8,32)       7.56e-07 1.19e-06 6.35e-07   9.37e-07 1.09e-06 5.23e-07   1.99e-05 3.50e-05 1.09e-05
        #   (3,100)      7.18e-07 1.04e-06 6.78e-07   7.79e-07 7.60e-07 3.70e-07   2.40e-05 3.99e-05 2.10e-05
        #   (2,301)      7.70e-07 1.12e-06 7.09e-07   5.55e-07 6.24e-07 5.46e-07   5.03e-05 8.53e-05 3.94e-05
        #   (1,602)      1.22e-06 1.10e-06 9.06e-07   9.33e-07 1.20e-06 4.35e-07   7.73e-05 9.23e-05 6.16e-05
        #   (4,16)s90    1.76e-04 1.68e-04 1.21e-04   1.66e-04 1.04e-04 6.85e-05   1.96e-04 7.43e-05 3.47e-05
        #   (2,301)s90   3.31e-04 7.29e-04 1.43e-04   3.03e-04 6.29e-04 1.03e-04   6.70e-04 5.09e-04 1.63e-04
        #   (4,16)p.5    1.13e-06 1.41e-06 1.36e-06   9.91e-07 1.01e-06 1.14e-06   1.93e-05 1.66e-05 1.12e-05
        #   (2,301)p.5   1.23e-06 2.11e-06 1.11e-06   1.08e-06 1.22e-06 5.62e-07   5.45e-05 9.76e-05 4.06e-05
        #   (5,64)       1.92e-06 1.44e-06 -          6.27e-07 7.00e-07 -          2.80e-05 3.36e-05 -
        #   (1,256)      5.45e-07 8.06e-07 -          4.92e-07 8.87e-07 -          3.87e-05 5.28e-05 -
        #   (1,512)      6.25e-07 5.92e-07 -          4.15e-07 4.64e-07 -          6.38e-05 8.11e-05 -
        #   (1,1024)     7.32e-07 8.72e-07 -          6.56e-07 4.64e-07 -          1.11e-04 1.51e-04 -
        #   (2,101)      6.53e-07 9.38e-07 -          6.93e-07 5.35e-07 -          2.58e-05 4.65e-05 -
        #   (1,201)      5.99e-07 6.23e-07 -          5.85e-07 4.32e-07 -          4.67e-05 4.57e-05 -
        #   (1,1023)     9.52e-07 1.19e-06 -          1.32e-06 4.98e-07 -          1.13e-04 1.60e-04 -
        #   (3,30)       6.45e-07 7.66e-07 -          5.29e-07 4.02e-07 -          1.42e-05 1.27e-05 -
        # Worst kernel/eager ratio 2.20 (d_zl at (2,301)s90); the bound is 4.
        assert e_got <= 4 * e_eager, (name, e_got, e_eager)


@pytest.mark.parametrize("H,D", SHAPES)
def test_gatv2_aggregate_cpu(H, D):
    _check("cpu", H, D)


@pytest.mark.parametrize("H,D", [(4, 16), (2, 301)])
def test_gatv2_aggregate_large_scores_cpu(H, D):
    _check("cpu", H, D, big=True)


@pytest.mark.parametrize("H,D", [(4, 16), (2, 301)])
def test_gatv2_attn_dropout_cpu(H, D):
    _check("cpu", H, D, p=DROP_P)


def test_gatv2_dropout_zero_draws_nothing_cpu():
    _draws_nothing("cpu")


def test_gatv2_csr_ignores_dropout_cpu():
    _csr_path("cpu", 4, 16)


def test_gatv2_shape_errors_cpu():
    _shape_errors("cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", SHAPES)
def test_gatv2_aggregate_gpu(H, D):
    _check("cuda", H, D)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", [(4, 16), (2, 301)])
def test_gatv2_aggregate_large_scores_gpu(H, D):
    _check("cuda", H, D, big=True)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", [(4, 16), (2, 301)])
def test_gatv2_attn_dropout_gpu(H, D):
    _check("cuda", H, D, p=DROP_P)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", LAYOUT_SHAPES)
def test_gatv2_lane_layouts_gpu(H, D):
    """The lane layouts the issue's shapes do not reach, D = 1024 included.
    The reference is the closed form on the edge list in float64 (the dense
    one would need [n_dst, n_src, 1024] temporaries)."""
    c = _inputs(H, D, False, False)
    c["ref"] = _eager(c, H, torch.float64)
    _check("cuda", H, D, ref=c)


@pytest.mark.gpu
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("H,D", SHAPES)
def test_gatv2_forward_state_gpu(H, D, big):
    """lse next to out, and the forward-only instance (eval)."""
    c = case(H, D, big)
    ref = c["ref"]
    csr = graph("cuda").csr
    zl, zr, a = c["zl"].cuda(), c["zr"].cuda(), c["a"].cuda()
    out, lse = ops._gatv2_forward_hip(csr, zl, zr, a, H, SLOPE)
    for name, t in (("lse", lse), ("out", out)):
        assert torch.isfinite(t).all(), name
        assert (t[list(EMPTY_ROWS)] == 0).all(), name
        assert _close(t, ref[name]), (name, _err(t, ref[name]))
    _csr_path("cuda", H, D, big)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", [(4, 16), (8, 32)])
def test_gatv2_aggregate_bf16_gpu(H, D):
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
def test_gatv2_reproducible_gpu(H, D, p):
    """Bitwise equal run to run, and with or without the LPT row order: each
    row's edges are walked in CSR/CSC order by a fixed set of lanes."""
    c = case(H, D)
    hg = graph("cuda")
    first = _run(c, H, "cuda", p=p)
    again = _run(c, H, "cuda", p=p)
    natural = HaloGraph(dataclasses.replace(hg.csr, row_order=None),
                        dataclasses.replace(hg.csc, row_order=None),
                        hg.num_in, hg.num_all)
    unordered = _run(c, H, "cuda", hg=natural, p=p)
    for k in first:
        assert torch.equal(first[k], again[k]), k
        assert torch.equal(first[k], unordered[k]), k


@pytest.mark.gpu
def test_gatv2_unreferenced_rows_gpu():
    """Rows of zl past the graph's sources get a zero gradient."""
    c = case(4, 16)
    hg = graph("cuda")
    zl = torch.cat((c["zl"], torch.ones(7, 64))).cuda().requires_grad_(True)
    zr, a = c["zr"].cuda(), c["a"].cuda()
    ops.gatv2_aggregate(hg, zl, zr, a, 4, SLOPE).backward(c["g"].cuda())
    assert zl.grad.shape == zl.shape and (zl.grad[N_SRC:] == 0).all()
    assert _close(zl.grad[:N_SRC], c["ref"]["d_zl"])


@pytest.mark.gpu
def test_gatv2_dropout_zero_draws_nothing_gpu():
    _draws_nothing("cuda")


@pytest.mark.gpu
def test_gatv2_no_nnz_sized_allocation_gpu():
    """Forward + backward allocate nothing of size nnz: every legitimate
    output and saved tensor is per-node (< 2 MB in total at this shape), one
    fp32 value per edge would be 4 MB."""
    n_src, n_dst, nnz, H, D = 3000, 2000, 1_000_000, 4, 8
    gen = torch.Generator().manual_seed(3)
    u = torch.randint(0, n_src, (nnz,), generator=gen)
    v = torch.randint(0, n_dst, (nnz,), generator=gen)
    hg = HaloGraph.from_edges(u, v, n_dst, n_src).to("cuda")
    zl = torch.randn(n_src, H * D, generator=gen).cuda().requires_grad_(True)
    zr = torch.randn(n_dst, H * D, generator=gen).cuda().requires_grad_(True)
    a = torch.randn(H, D, generator=gen).cuda().requires_grad_(True)
    g = torch.randn(n_dst, H * D, generator=gen).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    resident = torch.cuda.memory_allocated()
    out = ops.gatv2_aggregate(hg, zl, zr, a, H, SLOPE)
    out.backward(g)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - resident
    print(f"peak growth {grew} B, one nnz-sized fp32 tensor {4 * nnz} B")
    for t in (zl.grad, zr.grad, a.grad):
        assert torch.isfinite(t).all()
    assert grew < 4 * nnz, grew


@pytest.mark.gpu
def test_gatv2_shape_errors_gpu():
    _shape_errors("cuda")
    c = case(4, 16)
    hg = graph("cuda")
    csr = hg.csr
    zl, zr, a = c["zl"].cuda(), c["zr"].cuda(), c["a"].cuda()
    # past the head-width cap: the wrapper, then the native entry itself
    wide_l = torch.zeros(N_SRC, 1025, device="cuda")
    wide_r = torch.zeros(N_DST, 1025, device="cuda")
    wide_a = torch.zeros(1, 1025, device="cuda")
    with pytest.raises(ValueError, match="head width"):
        ops.gatv2_aggregate(hg, wide_l, wide_r, wide_a, 1)
    with pytest.raises(RuntimeError, match="exceeds"):
        native().gatv2_fwd(csr.indptr, csr.indices, wide_l, wide_r, wide_a,
                           torch.Tensor(), csr.num_cols, 1, SLOPE)
    # the native entry points guard themselves too (TORCH_CHECK)
    lse = torch.zeros(N_DST, 4, device="cuda")
    with pytest.raises(RuntimeError, match="rows"):
        native().gatv2_fwd(csr.indptr, csr.indices, zl[:100].contiguous(),
                           zr, a, torch.Tensor(), csr.num_cols, 4, SLOPE)
    with pytest.raises(RuntimeError, match="H\\*D"):
        native().gatv2_fwd(csr.indptr, csr.indices, zl[:, :63].contiguous(),
                           zr[:, :63].contiguous(), a, torch.Tensor(),
                           csr.num_cols, 4, SLOPE)
    with pytest.raises(RuntimeError, match="attn"):
        native().gatv2_fwd(csr.indptr, csr.indices, zl, zr,
                           a[:2].contiguous(), torch.Tensor(), csr.num_cols,
                           4, SLOPE)
    with pytest.raises(RuntimeError, match="rows"):
        native().gatv2_bwd_dst(csr.indptr, csr.indices, zr, zl, zr, a,
                               lse[:100], lse, torch.Tensor(), csr.num_cols,
                               4, SLOPE)
    csc = hg.csc
    with pytest.raises(RuntimeError, match="rows"):
        native().gatv2_bwd_src(csc.indptr, csc.indices, zr[:100].contiguous(),
                               zl, zr, a, lse, lse, torch.Tensor(),
                               csc.num_cols, 4, SLOPE)


def _draws_nothing(device):
    c = case(4, 16)
    hg = graph(device)
    zl, zr, a = (c[k].to(device) for k in ("zl", "zr", "a"))
    state = torch.get_rng_state()
    ops.gatv2_aggregate(hg, zl, zr, a, 4, SLOPE, attn_drop=0.0)
    assert torch.equal(torch.get_rng_state(), state)
    ops.gatv2_aggregate(hg, zl, zr, a, 4, SLOPE, attn_drop=0.5)
    assert not torch.equal(torch.get_rng_state(), state)


def _csr_path(device, H, D, big=False):
    """gatv2_aggregate_csr: forward only, no dropout argument at all, equal
    to the undropped reference; empty rows exactly 0."""
    c = case(H, D, big)
    csr = graph(device).csr
    zl, zr, a = (c[k].to(device) for k in ("zl", "zr", "a"))
    zl = zl.clone().requires_grad_(True)  # the cached tensor stays a plain one
    out = ops.gatv2_aggregate_csr(csr, zl, zr, a, H, SLOPE)
    assert not out.requires_grad
    assert (out[list(EMPTY_ROWS)] == 0).all()
    assert _close(out, c["ref"]["out"]), _err(out, c["ref"]["out"])


def _shape_errors(device):
    c = case(4, 16)
    hg = graph(device)
    zl, zr, a = (c[k].to(device) for k in ("zl", "zr", "a"))
    with pytest.raises(ValueError, match="out-of-bounds"):
        ops.gatv2_aggregate(hg, zl[:100], zr, a, 4)
    with pytest.raises(ValueError, match="destination"):
        ops.gatv2_aggregate(hg, zl, zr[:100], a, 4)
    with pytest.raises(ValueError, match="attn must be"):
        ops.gatv2_aggregate(hg, zl, zr, a[:2], 4)
    with pytest.raises(ValueError, match="num_heads"):
        ops.gatv2_aggregate(hg, zl[:, :63], zr[:, :63], a, 4)
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError, match="attn_drop"):
            ops.gatv2_aggregate(hg, zl, zr, a, 4, attn_drop=bad)
    with pytest.raises(ValueError, match="out-of-bounds"):
        ops.gatv2_aggregate_csr(hg.csr, zl[:100], zr, a, 4)
