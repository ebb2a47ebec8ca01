"""Dead gradient rows in the backward SpMM: the fused row scale that counts the
live rows, and the dense gather that redirects the dead ones to one zero row.
Both must leave every bit of the result as it was (docs/DESIGN.md, "Dead
gradient rows")."""
import pytest
import torch

from pipegcn_amd import native, ops
from pipegcn_amd.graph.csr import HaloGraph

NUM_OUT, NUM_SRC = 140, 300
WIDTHS = [1, 41, 64, 100, 256, 602]
MID = 150
N_LIVE = [0, 1, MID, NUM_SRC - 1, NUM_SRC]
DTYPES = [torch.float32, torch.bfloat16]


def _edges(num_out, num_src, max_rand_deg, seed):
    """Degrees 0, 1, 3, 4, 5, 7, 8, 9 (and 2, 6) in turn for the first 100
    rows, so the peel, the 4-edge group and the tail start at every offset
    mod 4 and meet every position; then random degrees, and one long row.
    Source ids are uniform, so live and dead ids mix at every position."""
    g = torch.Generator().manual_seed(seed)
    pattern = torch.tensor([0, 1, 3, 4, 5, 7, 8, 9, 2, 6])
    deg = torch.cat((pattern.repeat(10),
                     torch.randint(0, max_rand_deg + 1, (num_out - 100,),
                                   generator=g)))
    deg[120] = 200
    v = torch.repeat_interleave(torch.arange(num_out), deg)
    u = torch.randint(0, num_src, (v.numel(),), generator=g)
    return u, v


_CACHE = {}


def _graph():
    """Shared: NUM_OUT output rows gathering from NUM_SRC source rows."""
    if "graph" not in _CACHE:
        hg = HaloGraph.from_edges(*_edges(NUM_OUT, NUM_SRC, 30, 7), NUM_OUT,
                                  NUM_SRC)
        offs = hg.csr.indptr[:-1]
        assert {int(o) % 4 for o in offs} == {0, 1, 2, 3}
        _CACHE["graph"] = hg
    return _CACHE["graph"]


def _input(F, n_live, dtype):
    """[NUM_SRC, F] whose rows from n_live on are zero, some of them -0.0;
    row n_live - 1 is non-zero. Among the live rows: NaN, +-Inf, and an
    all-zero row (live, because a later row is not)."""
    key = ("input", F, n_live, dtype)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(100 * F + n_live)
        x = torch.randn(NUM_SRC, F, generator=g)
        x[x == 0] = 1.0
        if n_live >= 8:
            x[2] = 0.0
            x[3] = -0.0
            x[4, F - 1] = float("nan")
            x[5, 0] = float("inf")
            x[6, F // 2] = float("-inf")
        x[n_live:] = 0.0
        x[n_live::2] = -0.0          # every other dead row: all -0.0
        if n_live + 1 < NUM_SRC:
            x[n_live + 1, F - 1] = -0.0   # a +0.0 row that ends in -0.0
        _CACHE[key] = x.to(dtype)
    return _CACHE[key]


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _count(n, device="cuda"):
    return torch.tensor([n], dtype=torch.int32, device=device)


def _scale():
    if "scale" not in _CACHE:
        _CACHE["scale"] = 1.0 / _graph().csr.row_degrees().clamp(min=1.0)
    return _CACHE["scale"]


# -------------------------------------------------- the redirecting gather


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", WIDTHS)
def test_redirect_bitwise(F, dtype):
    csr = _graph().csr.to("cuda")
    for n_live in N_LIVE:
        x = _input(F, n_live, dtype).cuda()
        for scale in (None, _scale().cuda()):
            plain = ops.spmm(csr, x, scale)
            got = ops.spmm(csr, x, scale, n_live=_count(n_live))
            assert torch.equal(_bits(got), _bits(plain)), (F, n_live)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,vec", [(torch.float32, 4), (torch.float32, 2),
                                       (torch.float32, 1),
                                       (torch.bfloat16, 8),
                                       (torch.bfloat16, 4),
                                       (torch.bfloat16, 2),
                                       (torch.bfloat16, 1)])
def test_redirect_every_lane_width(dtype, vec, monkeypatch):
    """The widths pick_vec does not choose by itself at these shapes."""
    csr = _graph().csr.to("cuda")
    monkeypatch.setenv("PIPEGCN_SPMM_VEC", str(vec))
    for n_live in N_LIVE:
        x = _input(256, n_live, dtype).cuda()
        plain = ops.spmm(csr, x, None)
        got = ops.spmm(csr, x, None, n_live=_count(n_live))
        assert torch.equal(_bits(got), _bits(plain)), n_live


@pytest.mark.gpu
def test_redirect_natural_row_order():
    """Without the degree-sorted row order (what the autotune may pick)."""
    csr = _graph().csr.to("cuda")
    x = _input(64, MID, torch.float32).cuda()
    none = torch.Tensor()
    plain = native().spmm(csr.indptr, csr.indices, x, none, none, none,
                          csr.num_rows)
    got = native().spmm(csr.indptr, csr.indices, x, none, none, none,
                        csr.num_rows, _count(MID))
    assert torch.equal(_bits(got), _bits(plain))
    assert torch.equal(_bits(plain), _bits(ops.spmm(csr, x, None)))


@pytest.mark.gpu
def test_redirect_refuses_src_scale():
    """The redirect would read another row's scale: refused, not ignored."""
    csr = _graph().csr.to("cuda")
    x = _input(64, MID, torch.float32).cuda()
    with pytest.raises(RuntimeError, match="src_scale"):
        ops.spmm(csr, x, None, src_scale=torch.ones(NUM_SRC, device="cuda"),
                 n_live=_count(MID))


# ------------------------------------------------ the scale-and-count pass


def _inv(n=NUM_SRC):
    g = torch.Generator().manual_seed(3)
    return 1.0 / torch.randint(1, 500, (n,), generator=g).float()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", WIDTHS)
def test_scale_rows_live(F, dtype):
    inv = _inv().cuda()
    for n_live in N_LIVE:
        x = _input(F, n_live, dtype).cuda()
        scaled, count = ops.scale_rows_live(x, inv)
        eager = x * inv.unsqueeze(1).to(dtype)
        assert scaled.is_contiguous() and scaled.dtype == dtype
        assert torch.equal(_bits(scaled), _bits(eager)), (F, n_live)
        assert count.dtype == torch.int32 and count.numel() == 1
        assert count.item() == n_live, (F, n_live)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_scale_rows_live_edge_inputs(dtype):
    F = 100
    inv = _inv().cuda()
    # all zero, of both signs
    z = torch.zeros(NUM_SRC, F, dtype=dtype, device="cuda")
    z[::3] = -0.0
    scaled, count = ops.scale_rows_live(z, inv)
    assert count.item() == 0
    assert torch.equal(_bits(scaled), _bits(z * inv.unsqueeze(1).to(dtype)))
    # the last row alone is live, through one NaN / one Inf in its last column
    for v in (float("nan"), float("inf")):
        x = z.clone()
        x[NUM_SRC - 1, F - 1] = v
        assert ops.scale_rows_live(x, inv)[1].item() == NUM_SRC
    # a dead row ending in -0.0 after the last live one
    x = z.clone()
    x[10, 0] = 1.0
    x[11, F - 1] = -0.0
    assert ops.scale_rows_live(x, inv)[1].item() == 11
    # liveness is that of the product: a row that underflows to zero is dead
    x = z.clone()
    x[10, 0] = 1.0
    x[20] = 1e-30
    tiny = inv.clone()
    tiny[20] = 1e-30
    scaled, count = ops.scale_rows_live(x, tiny)
    assert count.item() == 11
    assert torch.equal(_bits(scaled), _bits(x * tiny.unsqueeze(1).to(dtype)))
    # more rows than one pass of the grid, one row, no row
    big = torch.zeros(40000, 8, dtype=dtype, device="cuda")
    big[39990, 3] = 2.0
    assert ops.scale_rows_live(big, torch.ones(40000, device="cuda"))[1] \
        .item() == 39991
    one = torch.ones(1, F, dtype=dtype, device="cuda")
    scaled, count = ops.scale_rows_live(one, inv[:1])
    assert count.item() == 1
    assert torch.equal(_bits(scaled), _bits(one * inv[:1].to(dtype)))
    scaled, count = ops.scale_rows_live(one[:0], inv[:0])
    assert count.item() == 0 and scaled.shape == (0, F)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("F,lo,width", [(41, 41, 82), (64, 64, 128),
                                        (100, 3, 108)])
def test_scale_rows_live_strided_rows(F, lo, width, dtype):
    """A column slice, as the last layer's backward hands over its gradient
    (the right half of one [rows, 2F] product), read in place: odd stride,
    a stride and start that allow the widest loads, a misaligned start."""
    inv = _inv().cuda()
    wide = torch.randn(NUM_SRC, width, device="cuda").to(dtype)
    wide[MID:, lo:lo + F] = 0.0
    x = wide[:, lo:lo + F]
    assert not x.is_contiguous()
    scaled, count = ops.scale_rows_live(x, inv)
    assert scaled.is_contiguous()
    assert torch.equal(_bits(scaled), _bits(x * inv.unsqueeze(1).to(dtype)))
    assert count.item() == MID


# ------------------------------------------------------------ autograd path


def _halo_graph():
    """300 inner and 340 source nodes, dense enough (nnz > rows * F) that
    _SpmmMean.backward takes its pre-scale branch."""
    if "halo" not in _CACHE:
        _CACHE["halo"] = HaloGraph.from_edges(*_edges(300, 340, 120, 9),
                                              300, 340)
    return _CACHE["halo"]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("n_live", [0, 1, 198, 300])
def test_spmm_mean_backward_bitwise(n_live, dtype, monkeypatch):
    hg = _halo_graph().to("cuda")
    F = 24
    g = torch.Generator().manual_seed(n_live)
    feat0 = torch.randn(hg.num_all, F, generator=g).to(dtype).cuda()
    inv_deg = (1.0 / hg.csr.row_degrees().clamp(min=1.0)).cuda()
    # the right half of a wider product, with an all-zero tail
    wide = torch.randn(hg.num_in, 2 * F, generator=g).to(dtype).cuda()
    wide[n_live:] = 0.0
    grad = wide[:, F:]
    assert hg.csc.nnz > grad.numel()

    handed = []
    real_spmm = ops.spmm

    def spy(csr, feat, scale=None, src_scale=None, n_live=None):
        handed.append(n_live)
        return real_spmm(csr, feat, scale, src_scale, n_live)

    monkeypatch.setattr(ops, "spmm", spy)

    def run():
        feat = feat0.clone().requires_grad_(True)
        ops.spmm_mean(hg, feat, inv_deg).backward(grad)
        return feat.grad

    got = run()
    assert handed[-1] is not None and handed[-1].item() == n_live
    monkeypatch.setenv("PIPEGCN_SPMM_LIVE", "0")
    withheld = run()
    assert handed[-1] is None
    assert torch.equal(_bits(got), _bits(withheld))
    # and both are the product the backward always was
    none = torch.Tensor()
    csc = hg.csc
    ref = native().spmm(csc.indptr, csc.indices,
                        grad * inv_deg.unsqueeze(1).to(dtype), none, none,
                        csc.row_order, csc.num_rows)
    assert torch.equal(_bits(got), _bits(ref))


# ----------------------------------------------------------------- CPU tier


def test_spmm_mean_backward_cpu_unchanged():
    """The CPU path keeps the eager pre-scale: its gradient is the transpose
    product of g * inv_deg, bit for bit, and matches the dense definition."""
    hg = _halo_graph()
    F = 24
    g = torch.Generator().manual_seed(5)
    feat = torch.randn(hg.num_all, F, generator=g, requires_grad=True)
    inv_deg = 1.0 / hg.csr.row_degrees().clamp(min=1.0)
    grad = torch.randn(hg.num_in, F, generator=g)
    grad[198:] = 0.0
    assert hg.csc.nnz > grad.numel()
    out = ops.spmm_mean(hg, feat, inv_deg)
    out.backward(grad)

    ref = ops.spmm(hg.csc, grad * inv_deg.unsqueeze(1), None)
    assert torch.equal(_bits(feat.grad), _bits(ref))

    u, v = _edges(300, 340, 120, 9)
    A = torch.zeros(hg.num_in, hg.num_all, dtype=torch.float64)
    A.index_put_((v, u), torch.ones(v.numel(), dtype=torch.float64),
                 accumulate=True)
    dense = A.t() @ (grad.double() * inv_deg.double().unsqueeze(1))
    # fp32 sums of at most 300 products of O(1) terms against fp64
    assert torch.allclose(feat.grad.double(), dense, rtol=1e-5, atol=1e-5)
    # n_live is a GPU matter: on the CPU it changes nothing
    assert torch.equal(
        _bits(ops.spmm(hg.csc, grad * inv_deg.unsqueeze(1), None,
                       n_live=torch.tensor([198], dtype=torch.int32))),
        _bits(ref))
