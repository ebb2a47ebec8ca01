"""Packed-row forward SpMM for bf16: the layout mirror, the packing kernel and
the packed gather, bit for bit against the mirror and the dense bf16 kernel
(docs/DESIGN.md, "Packed rows, bf16"), and against an fp64 sum."""
import functools

import pytest
import torch

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import CSR, HaloGraph

NUM_DST, NUM_SRC = 300, 400
# below one header entry, odd (a whole non-zero row reaches the slack), the
# narrow widths, one chunk, several chunks with a last lane that straddles F
WIDTHS = [4, 41, 100, 256, 602]
DENSITIES = [0.0, 0.25, 0.5, 1.0]
BF16 = torch.bfloat16


@functools.lru_cache(None)
def _edges():
    """Degrees 0..9 in turn (every alignment of the peel, the 4-edge group
    and the tail), then random 0..30, and one row of 200 edges."""
    g = torch.Generator().manual_seed(11)
    deg = torch.cat((torch.arange(100) % 10,
                     torch.randint(0, 31, (NUM_DST - 100,), generator=g)))
    deg[150] = 200
    v = torch.repeat_interleave(torch.arange(NUM_DST), deg)
    u = torch.randint(0, NUM_SRC, (v.numel(),), generator=g)
    return u, v


@functools.lru_cache(None)
def _graph():
    return HaloGraph.from_edges(*_edges(), NUM_DST, NUM_SRC).to("cuda")


@functools.lru_cache(None)
def _input(F, density, finite=False):
    """bf16 [NUM_SRC, F] with about `density` non-zeros. Strictly between 0
    and 1 it also carries an all-zero row, an all-non-zero row, a -0.0
    (dropped) and, unless `finite`, a NaN and an Inf (both kept)."""
    g = torch.Generator().manual_seed(1000 * F + int(100 * density))
    x = torch.randn(NUM_SRC, F, generator=g).to(BF16)
    x[x == 0] = 1.0
    x = x * (torch.rand(NUM_SRC, F, generator=g) < density)
    if 0.0 < density < 1.0:
        x[0] = 0.0
        x[1] = torch.arange(1, F + 1).to(BF16)
        x[2, 0] = -0.0
        x[5, F // 2] = -0.0
        if not finite:
            x[3, F - 1] = float("nan")
            x[4, 1] = float("inf")
    return x


def _bits(t):
    return t.contiguous().view(torch.int16)


def _scale(g):
    return (1.0 / g.csr.row_degrees().clamp(min=1.0)).contiguous()


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("density", DENSITIES)
def test_mirror_roundtrip(F, density):
    W, hdr, stride = ops.packed_row_layout(F, BF16)
    assert W == (F + 63) // 64 and hdr % 4 == 0 and hdr >= 3 * W
    # a 3-word load from word F // 2 stays inside the 128-byte-strided record
    assert stride % 32 == 0 and stride >= hdr + F // 2 + 3
    assert ops.packed_row_layout(F) == ops.packed_row_layout(F, torch.float32)
    x = _input(F, density)
    packed = ops.pack_rows_reference(x)
    assert packed.shape == (NUM_SRC, stride) and packed.dtype == torch.int32
    back = ops.unpack_rows_reference(packed, F, BF16)
    zero = x == 0
    assert back.dtype == BF16 and torch.equal(back == 0, zero)
    assert torch.equal(_bits(back)[~zero], _bits(x)[~zero])
    assert not _bits(back)[zero].any()  # -0.0 reads back as +0.0
    # header against the definition: 64-bit mask and exclusive prefix count
    nz = torch.zeros(NUM_SRC, W * 64, dtype=torch.long)
    nz[:, :F] = ~zero
    nz = nz.view(NUM_SRC, W, 64)
    mask = (packed[:, 0:3 * W:3].long() & 0xFFFFFFFF) \
        | (packed[:, 1:3 * W:3].long() << 32)
    assert torch.equal(mask, (nz << torch.arange(64)).sum(-1))
    assert torch.equal(packed[:, 2:3 * W:3].long(),
                       nz.sum(-1).cumsum(-1) - nz.sum(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("density", DENSITIES)
def test_pack_kernel_matches_mirror(F, density):
    x = _input(F, density)
    ref = ops.pack_rows_reference(x)
    dev = ops.pack_rows(x.cuda()).cpu()
    assert dev.shape == ref.shape and dev.dtype == torch.int32
    # the words the layout defines: header entries, then nnz 2-byte slots
    W, hdr, stride = ops.packed_row_layout(F, BF16)
    nnz = (x != 0).sum(1, keepdim=True)
    assert torch.equal(dev[:, :3 * W], ref[:, :3 * W])
    slot = torch.arange(2 * (stride - hdr)).unsqueeze(0)
    keep = slot < nnz
    assert torch.equal(_bits(dev[:, hdr:])[keep], _bits(ref[:, hdr:])[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("density", DENSITIES)
def test_gather_bitwise_dense(F, density):
    g = _graph()
    x = _input(F, density).cuda()
    plain = CSR(g.csr.indptr, g.csr.indices, g.csr.num_rows, g.csr.num_cols,
                None)
    for csr in (g.csr, plain):
        for s in (None, _scale(g)):
            ref = ops.spmm(csr, x, s)
            out = ops.spmm_packed(csr, x, s)
            assert out.dtype == BF16 and out.shape == ref.shape
            assert torch.equal(_bits(out), _bits(ref)), (
                F, density, csr.row_order is not None, s is not None)
    if 0.0 < density < 1.0:
        assert torch.isnan(ref).any()  # the kept NaN reached the output


@pytest.mark.gpu
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("density", DENSITIES)
def test_gather_against_fp64(F, density):
    """|out - ref| <= 2^-8 * scale * sum_u |x_u|: the one rounding to bf16 is
    at most 2^-9 relative, the fp32 accumulation over at most 200 edges adds
    less than 200 * 2^-24 of the absolute sum."""
    g = _graph()
    x = _input(F, density, finite=True)
    u, v = _edges()
    scale = _scale(g).cpu().double().unsqueeze(1)
    rows = x.double()[u]
    ref = torch.zeros(NUM_DST, F, dtype=torch.float64).index_add_(0, v, rows)
    mag = torch.zeros(NUM_DST, F, dtype=torch.float64).index_add_(
        0, v, rows.abs())
    out = ops.spmm_packed(g.csr, x.cuda(), _scale(g)).cpu().double()
    err = (out - ref * scale).abs()
    print(f"F={F} density={density}: max err / bound = "
          f"{(err / (2.0 ** -8 * scale * mag).clamp(min=1e-300)).max():.3f}")
    assert (err <= 2.0 ** -8 * scale * mag).all()


@pytest.mark.gpu
def test_routing_is_bitwise_neutral(monkeypatch):
    F = 256
    routed = ops._spmm_packed_width(F, BF16)
    g = _graph()
    inv = _scale(g)
    x = _input(F, 0.25, finite=True).cuda()
    grad = torch.randn(NUM_DST, F, generator=torch.Generator().manual_seed(
        3)).to(BF16).cuda()
    calls = []
    real = ops.spmm_packed
    monkeypatch.setattr(
        ops, "spmm_packed",
        lambda *a, **k: calls.append(1) or real(*a, **k))
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("PIPEGCN_SPMM_PACKED", flag)
        xi = x.clone().requires_grad_(True)
        out = ops.spmm_mean(g, xi, inv)
        out.backward(grad)
        res[flag] = (out.detach(), xi.grad)
        # 0 pins the dense kernel; 1 goes packed where the table says so
        assert len(calls) == (int(routed) if flag == "1" else 0)
    assert torch.equal(_bits(res["0"][0]), _bits(res["1"][0]))
    assert torch.equal(_bits(res["0"][1]), _bits(res["1"][1]))
    assert torch.equal(_bits(real(g.csr, x, inv)), _bits(res["0"][0]))


def test_refusals_cpu():
    with pytest.raises(ValueError, match="fp32 or bf16"):
        ops.pack_rows_reference(torch.zeros(4, 8, dtype=torch.float16))
    with pytest.raises(ValueError, match="fp32 or bf16"):
        ops.packed_row_layout(8, torch.float16)


@pytest.mark.gpu
def test_refusals_gpu():
    csr = _graph().csr
    with pytest.raises(ValueError, match="fp32 or bf16"):
        ops.spmm_packed(csr, torch.zeros(NUM_SRC, 8, dtype=torch.float16,
                                         device="cuda"))
    with pytest.raises(ValueError, match="fp32 or bf16"):
        ops.pack_rows(torch.zeros(4, 8, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError, match="source nodes"):
        ops.spmm_packed(csr, torch.zeros(NUM_SRC - 1, 256, dtype=BF16,
                                         device="cuda"))
