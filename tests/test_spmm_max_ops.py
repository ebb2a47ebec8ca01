"""Max aggregation: ops.spmm_max / ops.spmm_max_csr on the CPU path and on
the gfx950 kernels (csrc/hip/spmm_max.hip).

The reference is written here and is independent of the library's CPU path:
a DENSE masked maximum over an [n_dst, n_src] adjacency mask, per column. The
expected arg is the first edge of the row, in csr.indices order, whose value
equals that maximum.

The maximum is one of the inputs, so out and arg are compared EXACTLY, in
fp32 and in bf16. The backward is a sum and is compared against a float64
`index_put_(accumulate=True)` of g by the expected arg:
 - fp32: atol = rtol = 1e-4, the SpMM tolerance of tests/test_ops.py;
 - bf16: max error over the reference's max-norm < 0.02, the bound of
   test_spmm_bf16_gpu.

Two kinds of input: randn, and a TIE input of small integers on which most
maxima are attained by several nodes and by parallel edges. On the tie input
the column sums of grad_z must equal those of g over the non-empty rows: a
destination counted once per parallel edge cannot pass that.
"""
import dataclasses
import functools

import pytest
import torch

from pipegcn_amd import native, ops
from tests.test_gat_ops import EMPTY_ROWS, N_DST, N_SRC, edges, graph

# one ragged element per lane | one exact chunk | the widest lane load |
# multi-chunk with a ragged tail, twice (fp32 8-byte lanes, bf16 4-byte)
WIDTHS = [41, 64, 256, 300, 602]
KINDS = ["randn", "tie"]
GPU_DTYPES = [torch.float32, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def case(F, kind, bf16=False):
    """Seeded inputs and the dense reference, computed once per (width,
    kind, dtype) and shared read-only: z, g (rounded to bf16 values for the
    bf16 runs), out, arg and the float64 grad_z."""
    gen = torch.Generator().manual_seed(7000 + F + (1 if kind == "tie" else 0))
    if kind == "tie":
        z = torch.randint(-3, 4, (N_SRC, F), generator=gen).float()
    else:
        z = torch.randn(N_SRC, F, generator=gen)
    g = torch.randn(N_DST, F, generator=gen)
    if bf16:
        z, g = z.bfloat16().float(), g.bfloat16().float()
    u, v = edges()
    mask = torch.zeros(N_DST, N_SRC, dtype=torch.bool)
    mask[v, u] = True
    nonempty = mask.any(1)
    out = torch.empty(N_DST, F)
    for c0 in range(0, F, 64):  # [n_dst, n_src, 64] at a time
        zc = z[:, c0:c0 + 64].t().unsqueeze(0)  # [1, cols, n_src]
        m = torch.where(mask.unsqueeze(1), zc,
                        torch.full_like(zc, -float("inf")))
        out[:, c0:c0 + 64] = m.max(2).values
    out[~nonempty] = 0.0
    # the first edge of each row, in stored order, that equals the maximum
    csr = graph("cpu").csr
    arg = torch.full((N_DST, F), -1, dtype=torch.int32)
    for r in range(N_DST):
        ids = csr.indices[csr.indptr[r]:csr.indptr[r + 1]].long()
        if ids.numel() == 0:
            continue
        hit = z[ids] == out[r]  # [deg, F]
        assert hit.any(0).all()
        arg[r] = ids[hit.int().argmax(0)].int()
    rows, cols = (arg >= 0).nonzero(as_tuple=True)
    dz = torch.zeros(N_SRC, F, dtype=torch.float64)
    dz.index_put_((arg[rows, cols].long(), cols), g[rows, cols].double(),
                  accumulate=True)
    return dict(z=z, g=g, out=out, arg=arg, dz=dz, nonempty=nonempty)


def _check_grad(got, c, dtype):
    got = got.double().cpu()
    if dtype == torch.float32:
        assert torch.allclose(got, c["dz"], atol=1e-4, rtol=1e-4), \
            (got - c["dz"]).abs().max()
    else:
        err = (got - c["dz"]).abs().max() / c["dz"].abs().max()
        assert err < 0.02, err
    # every destination's gradient lands exactly once
    want = c["g"][c["nonempty"]].double().sum(0)
    have = got.sum(0)
    if dtype == torch.float32:
        assert torch.allclose(have, want, atol=1e-4, rtol=1e-4), \
            (have - want).abs().max()
    else:
        err = (have - want).abs().max() / want.abs().max()
        assert err < 0.02, err


def _run(device, dtype, F, kind):
    c = case(F, kind, dtype == torch.bfloat16)
    hg = graph(device)
    z = c["z"].to(device=device, dtype=dtype).requires_grad_(True)
    out = ops.spmm_max(hg, z)
    assert out.dtype == dtype and out.shape == (N_DST, F)
    assert torch.equal(out.detach().float().cpu(), c["out"])
    assert (out.detach()[list(EMPTY_ROWS)] == 0).all()
    out.backward(c["g"].to(device=device, dtype=dtype))
    assert z.grad.dtype == dtype and z.grad.shape == z.shape
    _check_grad(z.grad, c, dtype)

    out2, arg = ops.spmm_max_csr(hg.csr, z.detach(), with_arg=True)
    assert arg.dtype == torch.int32
    assert torch.equal(arg.cpu(), c["arg"])
    assert (arg[list(EMPTY_ROWS)] == -1).all()
    assert torch.equal(out2, out.detach())
    # the forward that drops arg: same out
    assert torch.equal(ops.spmm_max_csr(hg.csr, z.detach()), out.detach())
    with torch.no_grad():
        assert torch.equal(ops.spmm_max(hg, z), out.detach())
    return arg.cpu()


def test_graph_has_parallel_edges():
    u, v = edges()
    pairs = torch.unique(v * N_SRC + u)
    assert u.numel() == 4177 and pairs.numel() == 3988


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", WIDTHS)
def test_spmm_max_cpu(F, kind):
    _run("cpu", torch.float32, F, kind)


def test_spmm_max_cpu_bf16():
    _run("cpu", torch.bfloat16, 64, "tie")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", GPU_DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", WIDTHS)
def test_spmm_max_gpu(F, dtype, kind):
    gpu_arg = _run("cuda", dtype, F, kind)
    # GPU and CPU arg are identical
    z = case(F, kind, dtype == torch.bfloat16)["z"]
    cpu_arg = ops.spmm_max_csr(graph("cpu").csr, z, with_arg=True)[1]
    assert torch.equal(gpu_arg, cpu_arg)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,vec", [(torch.float32, 4), (torch.float32, 1),
                                       (torch.bfloat16, 8),
                                       (torch.bfloat16, 2)],
                         ids=["fp32-16B", "fp32-4B", "bf16-16B", "bf16-4B"])
def test_spmm_max_gpu_lane_widths(monkeypatch, dtype, vec):
    """The lane widths that pick_vec's preference does not reach on a graph
    this small: 16-byte accesses (bf16: arg in two 16-byte halves) and
    single dwords."""
    monkeypatch.setenv("PIPEGCN_SPMM_VEC", str(vec))
    _run("cuda", dtype, 256, "tie")
    _run("cuda", dtype, 256, "randn")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", GPU_DTYPES, ids=["fp32", "bf16"])
def test_spmm_max_gpu_natural_row_order(dtype):
    """Both GPU passes with row_order absent."""
    F = 300
    c = case(F, "tie", dtype == torch.bfloat16)
    hg = graph("cuda")
    z = c["z"].to(device="cuda", dtype=dtype)
    nat = dataclasses.replace(hg.csr, row_order=None)
    out, arg = ops.spmm_max_csr(nat, z, with_arg=True)
    assert torch.equal(out.float().cpu(), c["out"])
    assert torch.equal(arg.cpu(), c["arg"])
    csc = hg.csc_simple()
    dz = native().spmm_max_bwd(csc.indptr, csc.indices,
                               c["g"].to(device="cuda", dtype=dtype), arg,
                               torch.Tensor(), csc.num_rows, csc.num_cols)
    _check_grad(dz, c, dtype)


def test_spmm_max_undersized_z_raises_cpu():
    hg = graph("cpu")
    z = torch.randn(N_SRC - 1, 64)
    with pytest.raises(ValueError, match="spmm_max: z has 299 rows but the "
                                         "graph references 300"):
        ops.spmm_max(hg, z)
    with pytest.raises(ValueError, match="out-of-bounds GPU gather"):
        ops.spmm_max_csr(hg.csr, z)


@pytest.mark.gpu
def test_spmm_max_undersized_raises_before_launch_gpu():
    hg = graph("cuda")
    csr, z = hg.csr, torch.randn(N_SRC - 1, 64, device="cuda")
    with pytest.raises(ValueError, match="spmm_max: z has 299 rows"):
        ops.spmm_max(hg, z)
    # the native wrappers check for themselves
    with pytest.raises(RuntimeError, match="z has 299 rows"):
        native().spmm_max(csr.indptr, csr.indices, z, torch.Tensor(),
                          csr.num_rows, csr.num_cols, True)
    csc = hg.csc_simple()
    g = torch.randn(N_DST, 64, device="cuda")
    arg = torch.zeros(N_DST - 1, 64, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="arg is"):
        native().spmm_max_bwd(csc.indptr, csc.indices, g, arg, torch.Tensor(),
                              csc.num_rows, csc.num_cols)
    with pytest.raises(RuntimeError, match="g has 199 rows"):
        native().spmm_max_bwd(csc.indptr, csc.indices, g[:-1].contiguous(),
                              arg, torch.Tensor(), csc.num_rows, csc.num_cols)
    torch.cuda.synchronize()


def test_spmm_max_grad_of_unreferenced_rows_is_zero():
    """Rows of z past the graph's sources get a zero gradient."""
    hg = graph("cpu")
    z = torch.randn(N_SRC + 3, 41, requires_grad=True)
    ops.spmm_max(hg, z).sum().backward()
    assert z.grad.shape == z.shape and (z.grad[N_SRC:] == 0).all()


@pytest.mark.gpu
def test_spmm_max_grad_of_unreferenced_rows_is_zero_gpu():
    hg = graph("cuda")
    z = torch.randn(N_SRC + 3, 41, device="cuda", requires_grad=True)
    ops.spmm_max(hg, z).sum().backward()
    assert z.grad.shape == z.shape and (z.grad[N_SRC:] == 0).all()
    assert z.grad.sum().item() == pytest.approx(
        41 * (N_DST - len(EMPTY_ROWS)), rel=1e-5)
