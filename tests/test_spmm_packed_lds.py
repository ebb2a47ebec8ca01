"""The LDS-staged packed gather (spmm_packed_lds_kernel, 4 columns per lane,
three chunks, 512 < F <= 768): the leading B bytes of every record are copied
blind into two LDS slots and header and values are read from there; lanes
whose value slots lie past B take the dependent load. B is derived on the
device from the mean payload of the packed rows, in whole 128-byte lines up
to a cap. Every comparison is bitwise against the dense `ops.spmm` on the same
input, and against the register-fed packed kernel (PIPEGCN_SPMM_PACKED_LDS=0).
The one-chunk widths 129, 200, 256 and the two-chunk 257 are not routed to the
staged kernel (one chunk lost a measured cell and was removed): there both
settings run the register-fed kernel, and the cases hold the routing to
that."""
import pytest
import torch

from pipegcn_amd import native, ops
from pipegcn_amd.graph.csr import CSR, HaloGraph

NUM_DST, NUM_SRC = 200, 300
FORCED = [0, 1, 2, 3, 4, 5, 7, 8, 9, 70]
SINGLE = [129, 200, 256]
MULTI = [257, 513, 600, 602, 768]
POISON = 0x7FC00000


def _bits(t):
    return t.contiguous().view(torch.int32)


def _line_ends(F):
    """Non-zero counts at which a record's last value slot ends exactly at a
    128-byte line: whatever B the kernel derives (a whole number of lines),
    one of these rows ends at byte B and its neighbour 4 bytes past it."""
    _, hdr, stride = ops.packed_row_layout(F)
    ends = range((4 * hdr // 128 + 1) * 128, 4 * stride + 1, 128)
    return [n for n in ((e - 4 * hdr) // 4 for e in ends) if 0 < n < F]


_G = {}


def _graph():
    """200 rows over 300 sources: the forced degrees four times over (a
    repeat holds 109 edges, so each degree starts once at every alignment:
    every peel, -e_begin & 3, and every tail length occurs, also for the
    degree-70 rows of 16-17 whole groups); the rest random 0..12. The last
    source row is referenced."""
    if not _G:
        g = torch.Generator().manual_seed(17)
        rep = torch.tensor(FORCED)
        head = rep.repeat(4)
        deg = torch.cat((head, torch.randint(
            0, 13, (NUM_DST - head.numel(),), generator=g)))
        v = torch.repeat_interleave(torch.arange(NUM_DST), deg)
        u = torch.randint(0, NUM_SRC, (v.numel(),), generator=g)
        u[:80] = torch.arange(80)          # the planted rows are gathered
        u[-1] = NUM_SRC - 1                # the buffer's final record is read
        hg = HaloGraph.from_edges(u, v, NUM_DST, NUM_SRC)
        indptr = hg.csr.indptr
        d = indptr[1:] - indptr[:-1]
        assert torch.equal(d, deg)
        for want in FORCED:
            assert (d == want).any(), want
        start = indptr[:-1]
        peel = torch.minimum((-start) & 3, d)
        tail = (d - peel) & 3
        whole = d >= 8
        assert set(((-start) & 3)[whole].tolist()) == {0, 1, 2, 3}
        assert set(tail[whole].tolist()) == {0, 1, 2, 3}
        assert set(((-start) & 3)[d == 70].tolist()) == {0, 1, 2, 3}
        assert int(hg.csr.indices.max()) == NUM_SRC - 1
        perm = torch.randperm(NUM_DST, generator=g).to(torch.int32)
        _G["hg"] = hg
        _G["perm"] = perm
    return _G["hg"], _G["perm"]


def _input(F, density):
    """fp32 [NUM_SRC, F] with about `density` non-zeros. Planted: dense and
    empty rows alternating (rows 6..9), for every 128-byte line a row whose
    last value slot ends at it and one that ends 4 bytes past it (rows 12
    on), NaN, +-Inf (kept), -0.0 (dropped)."""
    g = torch.Generator().manual_seed(1000 * F + int(100 * density))
    x = torch.randn(NUM_SRC, F, generator=g)
    x[x == 0] = 1.0
    x = x * (torch.rand(NUM_SRC, F, generator=g) < density)
    full = torch.arange(1, F + 1, dtype=torch.float32)
    x[6], x[7], x[8], x[9] = full, 0.0, -full, 0.0
    row = 12
    for fit in _line_ends(F):
        for n in (fit, fit + 1):
            x[row] = 0.0
            x[row, F - n:] = full[:n]
            row += 1
    assert 12 < row <= 80
    if 0.0 < density < 1.0:
        x[0, F - 1] = float("nan")
        x[1, 1] = float("inf")
        x[2, F // 2] = float("-inf")
        x[3, 0] = -0.0
        x[4, F - 2] = -0.0
    return x


def _variants(hg, perm):
    scale = (1.0 / hg.csr.row_degrees().clamp(min=1.0)).contiguous().cuda()
    csr = hg.csr.to("cuda")
    plain = CSR(csr.indptr, csr.indices, csr.num_rows, csr.num_cols, None)
    ordered = CSR(csr.indptr, csr.indices, csr.num_rows, csr.num_cols,
                  perm.cuda())
    return [(c, s) for c in (plain, ordered) for s in (None, scale)]


def _packed(c, packed, F, s):
    return native().spmm_packed(
        c.indptr, c.indices, packed, F, s if s is not None else torch.Tensor(),
        c.row_order if c.row_order is not None else torch.Tensor(),
        c.num_rows)


def _poisoned(x):
    """pack_rows(x) as it is after the buffer held quiet NaNs everywhere:
    the words the pack pass does not write (header padding, slots past a
    row's non-zeros, the slack) are poison."""
    F = x.shape[1]
    W, hdr, stride = ops.packed_row_layout(F)
    packed = native().pack_rows(x)
    nnz = (x != 0).sum(1, keepdim=True)
    col = torch.arange(stride, device=x.device).unsqueeze(0)
    written = (col < 2 * W) | ((col >= hdr) & (col < hdr + nnz))
    return torch.where(written, packed,
                       torch.full_like(packed, POISON)).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("F", SINGLE + MULTI)
@pytest.mark.parametrize("density", [0.0, 0.25, 0.5, 1.0])
def test_staged_equals_dense_and_packed(F, density, monkeypatch):
    hg, perm = _graph()
    x = _input(F, density).cuda()
    poisoned = _poisoned(x)
    packed = native().pack_rows(x)
    for c, s in _variants(hg, perm):
        ref = _bits(ops.spmm(c, x, s))
        monkeypatch.setenv("PIPEGCN_SPMM_PACKED_LDS", "0")
        old = _bits(_packed(c, packed, F, s))
        monkeypatch.setenv("PIPEGCN_SPMM_PACKED_LDS", "1")
        new = _bits(_packed(c, packed, F, s))
        poison = _bits(_packed(c, poisoned, F, s))
        via_ops = _bits(ops.spmm_packed(c, x, s))
        key = (F, density, c.row_order is not None, s is not None)
        assert torch.equal(old, ref), key
        assert torch.equal(new, ref), key
        assert torch.equal(poison, ref), key
        assert torch.equal(via_ops, ref), key
    if 0.0 < density < 1.0:
        out = ops.spmm(c, x, s)
        assert torch.isnan(out).any() and torch.isinf(out).any()


@pytest.mark.gpu
def test_launcher_rejects_a_mismatched_buffer():
    """The bound B <= cap <= stride rests on the buffer having the stride of
    this F: the launcher refuses any other before it launches (the check the
    register-fed kernel already relied on). The launcher's own checks of the
    cap and of the LDS size are defensive: no input reaches them."""
    hg, _ = _graph()
    c = hg.csr.to("cuda")
    packed = native().pack_rows(torch.zeros(NUM_SRC, 600, device="cuda"))
    with pytest.raises(RuntimeError, match="stride_words"):
        _packed(c, packed, 700, None)
    with pytest.raises(RuntimeError, match="stride_words"):
        _packed(c, packed[:, :-32].contiguous(), 600, None)


def _model_step():
    """One training step of GraphSAGE 602 -> 64 -> 64 -> 7 (LayerNorm,
    dropout 0.5) on a small graph (the `small` synthetic shape has 100
    features, too narrow for the staged gather): layer 0's forward SpMM is
    three chunks wide."""
    import torch.nn.functional as F

    from pipegcn_amd.models.sage import GraphSAGE
    from pipegcn_amd.parallel import context as ctx
    from pipegcn_amd.parallel.buffer import Buffer

    n = NUM_DST
    g = torch.Generator().manual_seed(3)
    deg = torch.randint(0, 13, (n,), generator=g)
    v = torch.repeat_interleave(torch.arange(n), deg)
    u = torch.randint(0, n, (v.numel(),), generator=g)
    graph = HaloGraph.from_edges(u, v, n, n).to("cuda")
    layer_size = [602, 64, 64, 7]
    ctx.buffer = Buffer()
    ctx.buffer.init_buffer(n, n, [None], [None], layer_size[:3],
                           device="cuda")
    torch.manual_seed(5)
    model = GraphSAGE(layer_size, F.relu, use_pp=False, dropout=0.5,
                      norm="layer", train_size=n).cuda()
    model.train()
    feat = torch.randn(n, 602, generator=g).cuda()
    label = (torch.arange(n) % 7).cuda()
    logits = model(graph, feat, graph.csr.row_degrees())
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, label)
    loss.backward()
    ctx.buffer.shutdown()
    out = {"logits": logits.detach().cpu()}
    for k, p in model.named_parameters():
        out["grad." + k] = p.grad.cpu()
    return out


@pytest.mark.gpu
def test_model_step_staged_equals_packed(monkeypatch):
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("PIPEGCN_SPMM_PACKED_LDS", flag)
        res[flag] = _model_step()
    assert res["0"].keys() == res["1"].keys() and len(res["0"]) > 4
    for k in res["0"]:
        assert torch.equal(_bits(res["0"][k]), _bits(res["1"][k])), k
