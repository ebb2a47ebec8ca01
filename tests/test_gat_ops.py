"""GAT edge-softmax aggregation: ops.gat_aggregate on the CPU path and on the
gfx950 kernels (csrc/hip/gat.hip) against a float64 reference.

The reference is written here and is independent of the library's CPU path:
a DENSE per-destination softmax over an [n_dst, n_src, H] score tensor (edge
multiplicities as weights) differentiated by torch autograd in float64.

Tolerances:
 - out, dz (and lse, zc, csum): atol = rtol = 1e-4, the project's fp32 SpMM
   tolerance (tests/test_ops.py).
 - d_el, d_er are differences of two like-sized sums, so their error is set
   by the summation, not by the result's size. The yardstick is a plain fp32
   torch evaluation of the SAME closed form on the same inputs (`_eager32`);
   the code under test may have 4x its max error against float64 — only the
   summation order differs, anything larger is a bug.
 - bf16: max error relative to the reference's max-norm < 0.02, the bound of
   test_spmm_bf16_gpu.
"""
import dataclasses
import functools

import pytest
import torch

from pipegcn_amd import native, ops
from pipegcn_amd.graph.csr import HaloGraph

SLOPE = 0.2
N_SRC, N_DST = 300, 200
EMPTY_ROWS = (5, 199)
DEG1_ROW = 7
LONG_ROW, LONG_DEG = 11, 261
# (H, D): thin VEC 1 | F = 64 | F = 256, one full chunk | head width
# divisible by 4 with a ragged F | F = 602, multi-chunk, odd head width
SHAPES = [(1, 41), (4, 16), (8, 32), (3, 100), (2, 301)]
# raw scores are scaled so the largest is exactly this: exp(90) overflows
# fp32, so a missing max-subtraction cannot pass
BIG_SCORE = 90.0


@functools.lru_cache(maxsize=None)
def edges():
    """tests/test_ops.py's random graph plus the constructed rows."""
    g = torch.Generator().manual_seed(0)
    u = torch.randint(0, N_SRC, (4000,), generator=g)
    v = torch.randint(0, N_DST, (4000,), generator=g)
    special = torch.tensor(EMPTY_ROWS + (DEG1_ROW, LONG_ROW))
    keep = ~torch.isin(v, special)
    u, v = u[keep], v[keep]
    # the long row must start off a 4-edge boundary so that the peel, the
    # unrolled and the tail loop all run on it (261 = 1 or 2 or 3 peeled +
    # 64 x 4 + tail); pad the row before it if needed
    start = int((v < LONG_ROW).sum())
    pad = 1 if start % 4 == 0 else 0
    u = torch.cat((u, torch.tensor([17]),
                   torch.randint(0, N_SRC, (LONG_DEG,), generator=g),
                   torch.randint(0, N_SRC, (pad,), generator=g)))
    v = torch.cat((v, torch.tensor([DEG1_ROW]),
                   torch.full((LONG_DEG,), LONG_ROW),
                   torch.full((pad,), LONG_ROW - 1)))
    return u, v


@functools.lru_cache(maxsize=None)
def graph(device):
    u, v = edges()
    return HaloGraph.from_edges(u, v, N_DST, N_SRC).to(device)


def test_constructed_rows():
    hg = graph("cpu")
    deg = hg.csr.indptr[1:] - hg.csr.indptr[:-1]
    assert all(deg[r] == 0 for r in EMPTY_ROWS)
    assert deg[DEG1_ROW] == 1 and deg[LONG_ROW] == LONG_DEG
    assert hg.csr.indptr[LONG_ROW] % 4 != 0


def _dense_attention(z, el, er, H):
    """float64 dense softmax -> (out, lse, zc, csum), autograd-capable."""
    u, v = edges()
    cnt = torch.zeros(N_DST, N_SRC, dtype=torch.float64)
    cnt.index_put_((v, u), torch.ones(u.numel(), dtype=torch.float64),
                   accumulate=True)
    mask = (cnt > 0).unsqueeze(-1)
    s = el.unsqueeze(0) + er.unsqueeze(1)  # [n_dst, n_src, H]
    e = torch.nn.functional.leaky_relu(s, SLOPE)
    e = torch.where(mask, e, torch.full_like(e, -float("inf")))
    top = e.detach().max(1).values
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
    w = cnt.unsqueeze(-1) * torch.exp(e - top.unsqueeze(1))
    den = w.sum(1)
    nonempty = den > 0
    alpha = w / torch.where(nonempty, den, torch.ones_like(den)).unsqueeze(1)
    zh = z.view(N_SRC, H, -1)
    out = torch.einsum("vuh,uhd->vhd", alpha, zh).reshape(N_DST, -1)
    c = alpha * torch.where(s > 0, 1.0, SLOPE)
    zc = torch.einsum("vuh,uhd->vhd", c, zh).reshape(N_DST, -1)
    lse = torch.where(nonempty, top + torch.log(
        torch.where(nonempty, den, torch.ones_like(den))),
        torch.zeros_like(den))
    return out, lse, zc, c.sum(1)


@functools.lru_cache(maxsize=None)
def case(H, D, big=False, bf16=False):
    """Seeded inputs and the float64 reference, computed once per shape and
    shared (read-only) by every test that needs them."""
    gen = torch.Generator().manual_seed(1000 * H + D)
    z = torch.randn(N_SRC, H * D, generator=gen)
    el = torch.randn(N_SRC, H, generator=gen)
    er = torch.randn(N_DST, H, generator=gen)
    g = torch.randn(N_DST, H * D, generator=gen)
    if big:
        u, v = edges()
        k = BIG_SCORE / (el[u] + er[v]).max()
        el, er = el * k, er * k
    if bf16:
        z, el, er, g = (t.to(torch.bfloat16).float() for t in (z, el, er, g))
    z64, el64, er64 = (t.double().requires_grad_(True) for t in (z, el, er))
    out, lse, zc, csum = _dense_attention(z64, el64, er64, H)
    dz, d_el, d_er = torch.autograd.grad(out, (z64, el64, er64), g.double())
    ref = dict(out=out, lse=lse, zc=zc, csum=csum, dz=dz, d_el=d_el,
               d_er=d_er)
    ref = {k: t.detach() for k, t in ref.items()}
    for t in ref.values():
        assert torch.isfinite(t).all()
    return dict(z=z, el=el, er=er, g=g, ref=ref)


def _eager32(c, H):
    """d_el, d_er from the issue's closed form in plain fp32 torch ops on
    the edge list — the yardstick for the summation error."""
    u, v = edges()
    z, el, er, g = c["z"], c["el"], c["er"], c["g"]
    s = el[u] + er[v]
    e = torch.nn.functional.leaky_relu(s, SLOPE)
    top = torch.zeros(N_DST, H).scatter_reduce(
        0, v.unsqueeze(1).expand_as(e), e, "amax", include_self=False)
    den = torch.zeros(N_DST, H).index_add(0, v, torch.exp(e - top[v]))
    lse = top + torch.log(den.clamp(min=1e-38))
    alpha = torch.exp(e - lse[v])
    cw = alpha * torch.where(s > 0, 1.0, SLOPE)
    zh, gh = z.view(N_SRC, H, -1), g.view(N_DST, H, -1)
    out = torch.zeros(N_DST, H, zh.shape[2]).index_add(
        0, v, alpha.unsqueeze(-1) * zh[u])
    zc = torch.zeros_like(out).index_add(0, v, cw.unsqueeze(-1) * zh[u])
    csum = torch.zeros(N_DST, H).index_add(0, v, cw)
    t = (gh * out).sum(-1)
    gc = torch.zeros_like(zh).index_add(0, u, cw.unsqueeze(-1) * gh[v])
    d_el = (zh * gc).sum(-1) - torch.zeros(N_SRC, H).index_add(
        0, u, cw * t[v])
    d_er = (gh * zc).sum(-1) - t * csum
    return d_el, d_er


def _run(c, H, device, dtype=torch.float32, hg=None):
    hg = hg if hg is not None else graph(device)
    # fresh leaves: the cached case tensors are shared and stay untouched
    z, el, er = (c[k].to(device=device, dtype=dtype).clone()
                 .requires_grad_(True) for k in ("z", "el", "er"))
    out = ops.gat_aggregate(hg, z, el, er, H, SLOPE)
    out.backward(c["g"].to(device=device, dtype=dtype))
    return out.detach(), z.grad, el.grad, er.grad


def _close(a, ref):
    return torch.allclose(a.double().cpu(), ref, atol=1e-4, rtol=1e-4)


def _err(a, ref):
    return (a.double().cpu() - ref).abs().max().item()


def _check(device, H, D, big):
    c = case(H, D, big)
    ref = c["ref"]
    out, dz, d_el, d_er = _run(c, H, device)
    for t in (out, dz, d_el, d_er):
        assert torch.isfinite(t).all()
    assert (out[list(EMPTY_ROWS)] == 0).all(), "empty rows must be zero"
    assert _close(out, ref["out"]), _err(out, ref["out"])
    assert _close(dz, ref["dz"]), _err(dz, ref["dz"])
    eager_el, eager_er = _eager32(c, H)
    for name, got, eager in (("d_el", d_el, eager_el),
                             ("d_er", d_er, eager_er)):
        e_eager, e_got = _err(eager, ref[name]), _err(got, ref[name])
        print(f"{device} H={H} D={D} big={big} {name}: eager fp32 err "
              f"{e_eager:.3e}, got {e_got:.3e}")
        # Measured max abs error against float64 as "eager fp32 / kernel on
        # MI355X / CPU path", unit-normal inputs unless "s90" (scores
        # scaled to 90):
        #   shape      d_el                       d_er
        #   (1,41)     1.08e-6 1.40e-6 1.07e-6    1.43e-6 1.91e-6 8.90e-7
        #   (4,16)     1.04e-6 1.27e-6 1.59e-6    1.53e-6 1.41e-6 9.39e-7
        #   (8,32)     2.89e-6 2.10e-6 1.88e-6    3.70e-6 2.07e-6 1.28e-6
        #   (3,100)    3.56e-6 4.02e-6 3.60e-6    3.45e-6 2.81e-6 2.37e-6
        #   (2,301)    3.39e-6 5.92e-6 4.01e-6    3.93e-6 5.87e-6 3.12e-6
        #   (4,16)s90  3.47e-5 3.52e-5 4.10e-6    2.05e-5 2.05e-5 1.99e-6
        #   (2,301)s90 1.35e-4 1.41e-4 3.04e-5    8.39e-5 8.39e-5 7.26e-6
        # Worst kernel/eager ratio 1.74 (d_el at (2,301)); the bound is 4.
        assert e_got <= 4 * e_eager, (name, e_got, e_eager)


@pytest.mark.parametrize("H,D", SHAPES)
def test_gat_aggregate_cpu(H, D):
    _check("cpu", H, D, big=False)


@pytest.mark.parametrize("H,D", [(4, 16), (2, 301)])
def test_gat_aggregate_large_scores_cpu(H, D):
    _check("cpu", H, D, big=True)


def test_gat_shape_errors_cpu():
    _shape_errors("cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", SHAPES)
def test_gat_aggregate_gpu(H, D):
    _check("cuda", H, D, big=False)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", [(4, 16), (2, 301)])
def test_gat_aggregate_large_scores_gpu(H, D):
    _check("cuda", H, D, big=True)


@pytest.mark.gpu
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("H,D", SHAPES)
def test_gat_forward_state_gpu(H, D, big):
    """lse, zc and csum — the per-node state the backward is built from."""
    c = case(H, D, big)
    ref = c["ref"]
    csr = graph("cuda").csr
    lse, out, zc, csum = ops._gat_forward_hip(
        csr, c["z"].cuda(), c["el"].cuda(), c["er"].cuda(), H, SLOPE, True)
    for name, t in (("lse", lse), ("out", out), ("zc", zc), ("csum", csum)):
        assert torch.isfinite(t).all(), name
        assert (t[list(EMPTY_ROWS)] == 0).all(), name
        assert _close(t, ref[name]), (name, _err(t, ref[name]))
    # the forward-only variant (eval): the kernel compiled without zc/csum
    out2 = ops.gat_aggregate_csr(csr, c["z"].cuda(), c["el"].cuda(),
                                 c["er"].cuda(), H, SLOPE)
    assert (out2[list(EMPTY_ROWS)] == 0).all()
    assert _close(out2, ref["out"]), _err(out2, ref["out"])


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", [(4, 16), (8, 32)])
def test_gat_aggregate_bf16_gpu(H, D):
    c = case(H, D, bf16=True)
    out, dz, d_el, d_er = _run(c, H, "cuda", torch.bfloat16)
    for name, t in (("out", out), ("dz", dz), ("d_el", d_el),
                    ("d_er", d_er)):
        assert t.dtype == torch.bfloat16, name
        ref = c["ref"][name]
        err = _err(t, ref) / ref.abs().max().item()
        print(f"bf16 H={H} D={D} {name}: rel err {err:.3e}")
        assert err < 0.02, (name, err)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", [(4, 16), (2, 301)])
def test_gat_reproducible_gpu(H, D):
    """Bitwise equal run to run, and with or without the LPT row order:
    each row's edges are walked in CSR order by one wave."""
    c = case(H, D)
    hg = graph("cuda")
    first = _run(c, H, "cuda")
    again = _run(c, H, "cuda")
    natural = HaloGraph(dataclasses.replace(hg.csr, row_order=None),
                        dataclasses.replace(hg.csc, row_order=None),
                        hg.num_in, hg.num_all)
    unordered = _run(c, H, "cuda", hg=natural)
    for a, b, n in zip(first, again, unordered):
        assert torch.equal(a, b)
        assert torch.equal(a, n)


@pytest.mark.gpu
def test_gat_no_nnz_sized_allocation_gpu():
    """Forward + backward allocate nothing of size nnz: every legitimate
    output and saved tensor is per-node (< 2 MB in total at this shape), one
    fp32 value per edge would be 4 MB."""
    n_src, n_dst, nnz, H, D = 3000, 2000, 1_000_000, 4, 8
    gen = torch.Generator().manual_seed(3)
    u = torch.randint(0, n_src, (nnz,), generator=gen)
    v = torch.randint(0, n_dst, (nnz,), generator=gen)
    hg = HaloGraph.from_edges(u, v, n_dst, n_src).to("cuda")
    z = torch.randn(n_src, H * D, generator=gen).cuda().requires_grad_(True)
    el = torch.randn(n_src, H, generator=gen).cuda().requires_grad_(True)
    er = torch.randn(n_dst, H, generator=gen).cuda().requires_grad_(True)
    g = torch.randn(n_dst, H * D, generator=gen).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    resident = torch.cuda.memory_allocated()
    out = ops.gat_aggregate(hg, z, el, er, H, SLOPE)
    out.backward(g)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - resident
    print(f"peak growth {grew} B, one nnz-sized fp32 tensor {4 * nnz} B")
    assert torch.isfinite(z.grad).all() and torch.isfinite(el.grad).all()
    assert grew < 4 * nnz, grew


@pytest.mark.gpu
def test_gat_shape_errors_gpu():
    _shape_errors("cuda")
    # the native entry points guard themselves too (TORCH_CHECK)
    c = case(4, 16)
    csr = graph("cuda").csr
    z, el, er = c["z"].cuda(), c["el"].cuda(), c["er"].cuda()
    with pytest.raises(RuntimeError, match="rows"):
        native().gat_aggregate_fwd(
            csr.indptr, csr.indices, z[:100].contiguous(), el, er,
            torch.zeros_like(er), torch.Tensor(), csr.num_cols, 4, SLOPE,
            False)
    with pytest.raises(RuntimeError, match="rows"):
        native().gat_row_stats(csr.indptr, csr.indices, el[:100], er,
                               csr.num_cols, SLOPE)
    with pytest.raises(RuntimeError, match="H\\*D"):
        native().gat_aggregate_fwd(
            csr.indptr, csr.indices, z[:, :63].contiguous(), el, er,
            torch.zeros_like(er), torch.Tensor(), csr.num_cols, 4, SLOPE,
            False)


def _shape_errors(device):
    c = case(4, 16)
    hg = graph(device)
    z, el, er = (c[k].to(device) for k in ("z", "el", "er"))
    with pytest.raises(ValueError, match="out-of-bounds"):
        ops.gat_aggregate(hg, z[:100], el[:100], er, 4)
    with pytest.raises(ValueError, match="num_heads"):
        ops.gat_aggregate(hg, z[:, :63], el, er, 4)
    with pytest.raises(ValueError, match="el/er"):
        ops.gat_aggregate(hg, z, el[:, :2], er[:, :2], 4)
