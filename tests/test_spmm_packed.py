"""Packed-row forward SpMM: the row layout, the packing kernel and the packed
gather, each checked bit for bit (the packed path must not change a single
bit of what the dense kernel computes; docs/DESIGN.md, "Packed rows")."""
import os
import subprocess
import sys

import pytest
import torch

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import CSR, HaloGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NUM_DST, NUM_SRC = 300, 400
WIDTHS = [4, 41, 100, 256, 602]
DENSITIES = [0.0, 0.25, 0.5, 1.0]


def _edges(num_src):
    """~3k edges into NUM_DST rows: degrees 0..9 in turn (every alignment of
    the peel, the 4-edge group and the tail), then random 0..30, and one row
    of 200 edges."""
    g = torch.Generator().manual_seed(11)
    deg = torch.cat((torch.arange(100) % 10,
                     torch.randint(0, 31, (NUM_DST - 100,), generator=g)))
    deg[150] = 200
    v = torch.repeat_interleave(torch.arange(NUM_DST), deg)
    u = torch.randint(0, num_src, (v.numel(),), generator=g)
    return u, v


_GRAPHS = {}


def _graph(num_src=NUM_SRC):
    """Shared halo-shaped graph (more source rows than destination rows)."""
    if num_src not in _GRAPHS:
        _GRAPHS[num_src] = HaloGraph.from_edges(*_edges(num_src), NUM_DST,
                                                num_src)
    return _GRAPHS[num_src]


def _input(F, density, n=NUM_SRC):
    """fp32 [n, F] with about `density` non-zeros. Strictly between 0 and 1
    it also carries an all-zero row, an all-non-zero row, a -0.0 (dropped),
    a NaN and an Inf (both kept)."""
    g = torch.Generator().manual_seed(1000 * F + int(100 * density))
    x = torch.randn(n, F, generator=g)
    x[x == 0] = 1.0
    x = x * (torch.rand(n, F, generator=g) < density)
    if 0.0 < density < 1.0:
        x[0] = 0.0
        x[1] = torch.arange(1, F + 1, dtype=torch.float32)
        x[2, 0] = -0.0
        x[3, F - 1] = float("nan")
        x[4, 1] = float("inf")
        x[5, F // 2] = -0.0
    return x


def _bits(t):
    return t.contiguous().view(torch.int32)


def _meaningful(ref, F):
    """The words of a packed buffer the layout defines: the header entries
    and each row's leading nnz value slots."""
    W, hdr, stride = ops.packed_row_layout(F)
    nnz = (ref[:, 0:2 * W:2].long() & 0xFFFFFFFF)
    nnz = sum(((nnz >> b) & 1) for b in range(32)).sum(1, keepdim=True)
    col = torch.arange(stride).unsqueeze(0)
    return (col < 2 * W) | ((col >= hdr) & (col < hdr + nnz))


# ------------------------------------------------------------ layout (CPU)


@pytest.mark.parametrize("F", WIDTHS)
def test_layout_roundtrip(F):
    W, hdr, stride = ops.packed_row_layout(F)
    assert W == (F + 31) // 32
    assert hdr % 4 == 0 and hdr >= 2 * W          # values 16-byte aligned
    assert stride % 32 == 0 and stride >= hdr + F + 8
    for density in DENSITIES:
        x = _input(F, density)
        packed = ops.pack_rows_reference(x)
        assert packed.shape == (NUM_SRC, stride)
        back = ops.unpack_rows_reference(packed, F)
        # bitwise, up to the sign of a dropped zero
        zero = x == 0
        assert torch.equal(back == 0, zero)
        assert torch.equal(_bits(back)[~zero], _bits(x)[~zero])
        assert not _bits(back)[zero].any()


def test_layout_against_plain_loop():
    """The vectorised mirror against the definition, element by element."""
    F = 41
    x = _input(F, 0.5)[:8]
    W, hdr, stride = ops.packed_row_layout(F)
    packed = ops.pack_rows_reference(x)
    for r in range(x.shape[0]):
        rank = 0
        for w in range(W):
            mask = 0
            assert packed[r, 2 * w + 1].item() == rank
            for b in range(32):
                c = 32 * w + b
                if c < F and x[r, c].item() != 0.0:
                    mask |= 1 << b
                    assert packed[r, hdr + rank].item() == \
                        _bits(x)[r, c].item()
                    rank += 1
            assert packed[r, 2 * w].item() & 0xFFFFFFFF == mask


def test_guard_rows():
    """Fewer feature rows than the graph references: refused before any
    launch (the check precedes every device call)."""
    csr = _graph().csr
    with pytest.raises(ValueError, match="source nodes"):
        ops.spmm_packed(csr, torch.zeros(NUM_SRC - 1, 8))


# ------------------------------------------------------------ kernels (GPU)


@pytest.mark.gpu
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("density", DENSITIES)
def test_pack_kernel_matches_mirror(F, density):
    x = _input(F, density)
    ref = ops.pack_rows_reference(x)
    dev = ops.pack_rows(x.cuda()).cpu()
    assert dev.shape == ref.shape and dev.dtype == torch.int32
    keep = _meaningful(ref, F)
    assert torch.equal(dev[keep], ref[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("density", DENSITIES)
def test_spmm_packed_bitwise(F, density):
    g = _graph().to("cuda")
    x = _input(F, density).cuda()
    scale = (1.0 / g.csr.row_degrees().clamp(min=1.0)).contiguous()
    plain = CSR(g.csr.indptr, g.csr.indices, g.csr.num_rows, g.csr.num_cols,
                None)
    for csr in (g.csr, plain):
        for s in (None, scale):
            ref = ops.spmm(csr, x, s)
            out = ops.spmm_packed(csr, x, s)
            assert out.shape == ref.shape
            assert torch.equal(_bits(out), _bits(ref)), (
                F, density, csr.row_order is not None, s is not None)
    if 0.0 < density < 1.0:
        assert torch.isnan(ref).any()  # the kept NaN reached the output


@pytest.mark.gpu
def test_guard_rows_gpu():
    csr = _graph().to("cuda").csr
    with pytest.raises(ValueError, match="source nodes"):
        ops.spmm_packed(csr, torch.zeros(NUM_SRC - 1, 256, device="cuda"))


def _count_packed(monkeypatch):
    calls = []
    real = ops.spmm_packed

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "spmm_packed", counted)
    return calls


@pytest.mark.gpu
def test_autograd_packed_equals_dense(monkeypatch):
    g = _graph().to("cuda")
    inv = (1.0 / g.csr.row_degrees().clamp(min=1.0)).contiguous()
    x = _input(256, 0.25).cuda()
    grad = torch.randn(NUM_DST, 256, generator=torch.Generator().manual_seed(
        3)).cuda()
    calls = _count_packed(monkeypatch)
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("PIPEGCN_SPMM_PACKED", flag)
        xi = x.clone().requires_grad_(True)
        out = ops.spmm_mean(g, xi, inv)
        out.backward(grad)
        res[flag] = (out.detach(), xi.grad)
        assert len(calls) == int(flag)  # 0 pins dense, 1 routes F=256 packed
    assert torch.equal(_bits(res["0"][0]), _bits(res["1"][0]))
    assert torch.equal(_bits(res["0"][1]), _bits(res["1"][1]))


# --------------------------------------------------------- model level (GPU)


def _model_step():
    """One training step of a 3-layer GraphSAGE 100 -> 64 -> 64 -> 7
    (LayerNorm, dropout 0.5) on the small graph -> ({name: tensor}, number
    of packed SpMM calls). A single partition has no halo, so the graph is
    the shared one with its sources folded into the destination rows."""
    import torch.nn.functional as F

    from pipegcn_amd.models.sage import GraphSAGE
    from pipegcn_amd.parallel import context as ctx
    from pipegcn_amd.parallel.buffer import Buffer

    calls = []
    real = ops.spmm_packed

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    ops.spmm_packed = counted
    try:
        graph = _graph(NUM_DST).to("cuda")
        layer_size = [100, 64, 64, 7]
        ctx.buffer = Buffer()
        ctx.buffer.init_buffer(NUM_DST, NUM_DST, [None], [None],
                               layer_size[:3], device="cuda")
        torch.manual_seed(5)
        model = GraphSAGE(layer_size, F.relu, use_pp=False, dropout=0.5,
                          norm="layer", train_size=NUM_DST).cuda()
        model.train()
        feat = _input(100, 1.0, NUM_DST).cuda()
        in_deg = graph.csr.row_degrees()
        label = (torch.arange(NUM_DST) % 7).cuda()
        logits = model(graph, feat, in_deg)
        loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, label)
        loss.backward()
        ctx.buffer.shutdown()
        out = {"logits": logits.detach().cpu(), "loss": loss.detach().cpu()}
        for k, p in model.named_parameters():
            out["grad." + k] = p.grad.cpu()
        return out, len(calls)
    finally:
        ops.spmm_packed = real


@pytest.mark.gpu
def test_model_step_packed_equals_dense(tmp_path, monkeypatch):
    monkeypatch.setenv("PIPEGCN_SPMM_PACKED", "0")
    dense, n_dense = _model_step()
    assert n_dense == 0
    path = str(tmp_path / "packed.pt")
    env = dict(os.environ, PIPEGCN_SPMM_PACKED="1", PYTHONPATH=ROOT)
    subprocess.run([sys.executable, os.path.abspath(__file__), path],
                   cwd=ROOT, env=env, check=True, timeout=300)
    packed, n_packed = torch.load(path)
    assert n_packed == 3  # every layer's forward gather went packed
    assert set(packed) == set(dense) and len(dense) == 2 + 16
    for k, ref in dense.items():
        assert torch.equal(_bits(packed[k]), _bits(ref)), k


if __name__ == "__main__":
    torch.save(_model_step(), sys.argv[1])
