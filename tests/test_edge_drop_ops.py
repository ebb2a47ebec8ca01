"""Edge dropout (DropEdge) in the mean / GCN aggregation: the keep mirror,
ops.spmm_drop on the CPU path and on the masked gfx950 kernel, and
ops.spmm_mean(edge_drop=...) under autograd (docs/DESIGN.md, "Edge dropout").

The graph is the small one of tests/test_spmm_live_rows.py: 140 destinations,
300 sources, degrees 0-9 in turn (rows start at every offset mod 4), one row of
200 edges, 81 duplicate edges. The reference is written here: a float64 dense
[140, 300] matrix of kept-edge counts built from the mirror, times the scales
and 1 / (1 - p); its transpose for the CSC pass; torch autograd for gradients.

Tolerances:
 - exact cases (integer inputs in [-4, 4], power-of-two scales, p in {0.5,
   0.75}): every partial sum is an integer times a power of two below 2^24,
   exact in fp32, so any correct kernel gives the float64 reference rounded
   once to the dtype, bit for bit;
 - random floats, fp32: atol = rtol = 1e-4 (tests/test_ops.py's SpMM policy);
 - random floats, bf16: max error over the reference's max-norm < 0.02 (the
   GAT tests' policy).
"""
import functools

import pytest
import torch

from pipegcn_amd import native, ops
from pipegcn_amd.graph.csr import HaloGraph
from tests.test_spmm_live_rows import NUM_OUT, NUM_SRC, _edges

SEED = 1234
WIDTHS = [1, 41, 64, 100, 256, 602]
DTYPES = [torch.float32, torch.bfloat16]
LONG_ROW = 120


@functools.lru_cache(maxsize=None)
def edges():
    return _edges(NUM_OUT, NUM_SRC, 30, 7)


@functools.lru_cache(maxsize=None)
def graph(device="cpu"):
    hg = HaloGraph.from_edges(*edges(), NUM_OUT, NUM_SRC)
    return hg if device == "cpu" else hg.to(device)


@functools.lru_cache(maxsize=None)
def kept_counts(p, seed=SEED):
    """float64 [NUM_OUT, NUM_SRC]: how many kept u -> v edges there are."""
    u, v = edges()
    keep = ops.edge_drop_keep(u, v, seed, p)
    A = torch.zeros(NUM_OUT, NUM_SRC, dtype=torch.float64)
    A.index_put_((v, u), keep.double(), accumulate=True)
    return A


def reference(x, p, transposed=False, scale=None, src_scale=None, seed=SEED):
    """float64 result of spmm_drop on the CSR, or on the CSC if transposed;
    autograd-capable in x."""
    A = kept_counts(p, seed)
    A = A.t() if transposed else A
    x = x.double()
    if src_scale is not None:
        x = x * src_scale.double().unsqueeze(1)
    out = A @ x
    if scale is not None:
        out = out * scale.double().unsqueeze(1)
    return out / (1.0 - p)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _shape(transposed):
    """(rows, cols) of the matrix spmm_drop walks."""
    return (NUM_SRC, NUM_OUT) if transposed else (NUM_OUT, NUM_SRC)


def _matrix(hg, transposed):
    return hg.csc if transposed else hg.csr


@functools.lru_cache(maxsize=None)
def pow2_scales(n):
    """Powers of two, 2^0 .. 2^-3 in turn."""
    return torch.tensor([2.0 ** -(i % 4) for i in range(n)])


@functools.lru_cache(maxsize=None)
def int_input(n, F):
    g = torch.Generator().manual_seed(31 * n + F)
    return torch.randint(-4, 5, (n, F), generator=g).float()


@functools.lru_cache(maxsize=None)
def float_input(n, F):
    g = torch.Generator().manual_seed(17 * n + F)
    return torch.randn(n, F, generator=g)


SCALINGS = ["none", "dst", "dst+src"]


def _scales(kind, rows, cols, device="cpu"):
    s = pow2_scales(rows).to(device) if kind != "none" else None
    ss = pow2_scales(cols).flip(0).contiguous().to(device) \
        if kind == "dst+src" else None
    return s, ss


# ------------------------------------------------------- the mask (CPU tier)


def test_mask_has_the_cases_the_tests_need():
    """What the other tests rely on at SEED, asserted so that a changed hash
    cannot hollow them out."""
    u, v = edges()
    ones = torch.ones(u.numel())
    deg = torch.zeros(NUM_OUT).index_add(0, v, ones)
    out_deg = torch.zeros(NUM_SRC).index_add(0, u, ones)
    assert deg[LONG_ROW] == 200
    pairs = u * NUM_OUT + v
    assert pairs.numel() - pairs.unique().numel() == 81

    def stats(p):
        k = ops.edge_drop_keep(u, v, SEED, p).float()
        kept = torch.zeros(NUM_OUT).index_add(0, v, k)
        out_kept = torch.zeros(NUM_SRC).index_add(0, u, k)
        groups = k.view(-1, 4).sum(1)  # nnz = 1288 = 4 * 322
        return {
            "dst_all_dropped": int(((kept == 0) & (deg > 0)).sum()),
            "dst_all_kept": int(((kept == deg) & (deg > 0)).sum()),
            "groups": [int((groups == i).sum()) for i in range(5)],
            "src_all_dropped": int(((out_kept == 0) & (out_deg > 0)).sum()),
            "long_row": int(kept[LONG_ROW]),
        }

    half = stats(0.5)
    assert half == {"dst_all_dropped": 10, "dst_all_kept": 10,
                    "groups": [15, 89, 96, 92, 30], "src_all_dropped": 36,
                    "long_row": 113}, half
    most = stats(0.9)
    assert most["dst_all_dropped"] == 57 and most["src_all_dropped"] == 190
    assert most["long_row"] == 26


def test_keep_is_the_one_head_attention_hash():
    u, v = edges()
    for p in (0.1, 0.5, 0.9):
        for seed in (0, SEED, 2 ** 62 - 2):
            k = ops.edge_drop_keep(u, v, seed, p)
            assert k.dtype == torch.bool and k.shape == (u.numel(),)
            assert torch.equal(
                k, ops.gat_dropout_keep(u, v, 1, seed, p)[:, 0])
    assert ops.edge_drop_keep(u, v, SEED, 0.0).all()
    with pytest.raises(ValueError):
        ops.edge_drop_keep(u, v, SEED, 1.0)
    with pytest.raises(ValueError):
        ops.edge_drop_keep(u, v, SEED, -0.1)


def test_keep_depends_on_endpoints_only():
    u, v = edges()
    k = ops.edge_drop_keep(u, v, SEED, 0.5)
    assert torch.equal(k, ops.edge_drop_keep(u.int(), v.int(), SEED, 0.5))
    perm = torch.randperm(u.numel(),
                          generator=torch.Generator().manual_seed(0))
    assert torch.equal(k[perm],
                       ops.edge_drop_keep(u[perm], v[perm], SEED, 0.5))
    # (u, v) is ordered: the CSC pass must not hash (v, u)
    assert not torch.equal(k, ops.edge_drop_keep(v, u, SEED, 0.5))


# ------------------------------------------------------ the op (CPU tier)


@pytest.mark.parametrize("transposed", [False, True], ids=["csr", "csc"])
def test_spmm_drop_cpu(transposed):
    hg = graph()
    rows, cols = _shape(transposed)
    for F in (1, 41, 64):
        x = float_input(cols, F)
        for p in (0.1, 0.5, 0.9):
            for kind in SCALINGS:
                s, ss = _scales(kind, rows, cols)
                got = ops.spmm_drop(_matrix(hg, transposed), x, s, ss, p=p,
                                    seed=SEED, transposed=transposed)
                ref = reference(x, p, transposed, s, ss)
                assert got.dtype == torch.float32
                assert torch.allclose(got.double(), ref, atol=1e-4,
                                      rtol=1e-4), (F, p, kind)
    # p = 0 keeps everything and is the plain product
    x = float_input(cols, 41)
    assert torch.allclose(
        ops.spmm_drop(_matrix(hg, transposed), x, p=0.0,
                      transposed=transposed),
        ops.spmm(_matrix(hg, transposed), x), atol=1e-5, rtol=1e-5)
    with pytest.raises(ValueError):
        ops.spmm_drop(_matrix(hg, transposed), x, p=1.0)
    # bf16 computes in fp32 and rounds once
    got = ops.spmm_drop(_matrix(hg, transposed), x.bfloat16(), p=0.5,
                        seed=SEED, transposed=transposed)
    ref = reference(x.bfloat16(), 0.5, transposed)
    assert got.dtype == torch.bfloat16
    assert (got.double() - ref).abs().max() / ref.abs().max() < 0.02


def _inv_deg(hg):
    return 1.0 / hg.csr.row_degrees().clamp(min=1.0)


def _mean_reference(x, inv_deg, grad, p, seed=SEED):
    """float64 out and d out / d x contracted with grad, by autograd."""
    x64 = x.double().requires_grad_(True)
    out = reference(x64, p, False, inv_deg, seed=seed)
    out.backward(grad.double())
    return out.detach(), x64.grad


@pytest.mark.parametrize("F", [1, 64])
def test_spmm_mean_edge_drop_cpu(F):
    """F = 1 takes the backward's pre-scale branch (nnz > numel), F = 64 the
    fused src_scale gather."""
    hg = graph()
    inv_deg = _inv_deg(hg)
    grad = float_input(NUM_OUT, F)
    assert (hg.csc.nnz > grad.numel()) == (F == 1)
    for p in (0.5, 0.9):
        x = float_input(NUM_SRC, F).clone().requires_grad_(True)
        out = ops.spmm_mean(hg, x, inv_deg, edge_drop=p, seed=SEED)
        out.backward(grad)
        ref_out, ref_grad = _mean_reference(x.detach(), inv_deg, grad, p)
        assert torch.allclose(out.double(), ref_out, atol=1e-4, rtol=1e-4)
        assert torch.allclose(x.grad.double(), ref_grad, atol=1e-4,
                              rtol=1e-4)


def test_edge_drop_zero_is_todays_path():
    hg = graph()
    inv_deg = _inv_deg(hg)
    x = float_input(NUM_SRC, 41)
    state = torch.get_rng_state()
    plain = ops.spmm_mean(hg, x, inv_deg)
    got = ops.spmm_mean(hg, x, inv_deg, edge_drop=0.0)
    assert torch.equal(_bits(got), _bits(plain))
    assert torch.equal(_bits(ops.spmm_mean(hg, x, inv_deg, 0.0, SEED)),
                       _bits(plain))
    assert torch.equal(torch.get_rng_state(), state)
    with pytest.raises(ValueError):
        ops.spmm_mean(hg, x, inv_deg, edge_drop=1.0)


def test_seed_comes_from_the_host_generator():
    hg = graph()
    inv_deg = _inv_deg(hg)
    x = float_input(NUM_SRC, 41)
    torch.manual_seed(5)
    drawn = int(torch.randint(0, 2 ** 62, (1,)).item())
    after_one_draw = torch.get_rng_state()
    torch.manual_seed(5)
    a = ops.spmm_mean(hg, x, inv_deg, edge_drop=0.5)
    assert torch.equal(torch.get_rng_state(), after_one_draw)
    assert torch.equal(a, ops.spmm_mean(hg, x, inv_deg, edge_drop=0.5,
                                        seed=drawn))
    b = ops.spmm_mean(hg, x, inv_deg, edge_drop=0.5)  # the next draw
    assert not torch.equal(a, b)
    torch.manual_seed(5)
    assert torch.equal(a, ops.spmm_mean(hg, x, inv_deg, edge_drop=0.5))
    # an explicit seed draws nothing
    state = torch.get_rng_state()
    ops.spmm_mean(hg, x, inv_deg, edge_drop=0.5, seed=SEED)
    assert torch.equal(torch.get_rng_state(), state)


# ------------------------------------------------------ the kernel (GPU)


def _exact_case(hg, F, dtype, transposed, kind, p):
    rows, cols = _shape(transposed)
    x = int_input(cols, F)
    s, ss = _scales(kind, rows, cols)
    ref = reference(x, p, transposed, s, ss).to(dtype)
    got = ops.spmm_drop(_matrix(hg, transposed), x.to(dtype).cuda(),
                        s.cuda() if s is not None else None,
                        ss.cuda() if ss is not None else None, p=p,
                        seed=SEED, transposed=transposed).cpu()
    assert got.dtype == dtype and got.shape == ref.shape
    diff = (got.double() - ref.double()).abs().max().item()
    assert torch.equal(got, ref), (F, dtype, transposed, kind, p, diff)
    A = kept_counts(p)
    dead = ((A.t() if transposed else A).sum(1) == 0)
    assert (got[dead] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", WIDTHS)
def test_kernel_exact(F, dtype):
    hg = graph("cuda")
    for transposed in (False, True):
        for kind in SCALINGS:
            for p in (0.5, 0.75):
                _exact_case(hg, F, dtype, transposed, kind, p)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,vec", [(torch.float32, 4), (torch.float32, 2),
                                       (torch.float32, 1),
                                       (torch.bfloat16, 8),
                                       (torch.bfloat16, 4),
                                       (torch.bfloat16, 2),
                                       (torch.bfloat16, 1)])
def test_kernel_exact_every_lane_width(dtype, vec, monkeypatch):
    """The widths pick_vec does not choose by itself at these shapes."""
    hg = graph("cuda")
    monkeypatch.setenv("PIPEGCN_SPMM_VEC", str(vec))
    for transposed in (False, True):
        for kind in SCALINGS:
            _exact_case(hg, 256, dtype, transposed, kind, 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_kernel_row_order_and_seed(dtype):
    hg = graph("cuda")
    none = torch.Tensor()
    for transposed in (False, True):
        m = _matrix(hg, transposed)
        assert m.row_order is not None
        rows, cols = _shape(transposed)
        for F in (41, 256):
            x = float_input(cols, F).to(dtype).cuda()
            key, thr, scale = ops.edge_drop_args("test", 0.5, SEED)
            lpt = ops.spmm_drop(m, x, p=0.5, seed=SEED,
                                transposed=transposed)
            nat = native().spmm_drop(m.indptr, m.indices, x, none, none,
                                     none, m.num_rows, transposed, key, thr,
                                     scale)
            assert torch.equal(_bits(lpt), _bits(nat)), (transposed, F)
            again = ops.spmm_drop(m, x, p=0.5, seed=SEED,
                                  transposed=transposed)
            assert torch.equal(_bits(lpt), _bits(again))
            other = ops.spmm_drop(m, x, p=0.5, seed=SEED + 1,
                                  transposed=transposed)
            assert not torch.equal(_bits(lpt), _bits(other))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_kernel_n_live(dtype):
    hg = graph("cuda")
    for F in (1, 41, 256):
        for n_live in (0, 1, 150, NUM_SRC - 1, NUM_SRC):
            x = float_input(NUM_SRC, F).clone()
            x[n_live:] = 0.0
            x[n_live::2] = -0.0
            x = x.to(dtype).cuda()
            count = torch.tensor([n_live], dtype=torch.int32, device="cuda")
            for scale in (None, _inv_deg(hg).cuda()):
                plain = ops.spmm_drop(hg.csr, x, scale, p=0.5, seed=SEED)
                got = ops.spmm_drop(hg.csr, x, scale, p=0.5, seed=SEED,
                                    n_live=count)
                assert torch.equal(_bits(got), _bits(plain)), (F, n_live)


@pytest.mark.gpu
def test_kernel_n_live_refuses_src_scale():
    hg = graph("cuda")
    x = float_input(NUM_SRC, 64).cuda()
    with pytest.raises(RuntimeError, match="src_scale"):
        ops.spmm_drop(hg.csr, x, None, torch.ones(NUM_SRC, device="cuda"),
                      p=0.5, seed=SEED,
                      n_live=torch.tensor([150], dtype=torch.int32,
                                          device="cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", WIDTHS)
def test_kernel_random_floats(F, dtype):
    hg = graph("cuda")
    for transposed in (False, True):
        rows, cols = _shape(transposed)
        x = float_input(cols, F).to(dtype)
        s = 1.0 / torch.arange(1, rows + 1).float()
        ss = 1.0 / torch.arange(1, cols + 1).float().sqrt()
        for p in (0.1, 0.5, 0.9):
            for sc, ssc in ((None, None), (s, None), (s, ss)):
                got = ops.spmm_drop(
                    _matrix(hg, transposed), x.cuda(),
                    sc.cuda() if sc is not None else None,
                    ssc.cuda() if ssc is not None else None, p=p, seed=SEED,
                    transposed=transposed).cpu()
                ref = reference(x, p, transposed, sc, ssc)
                if dtype == torch.float32:
                    assert torch.allclose(got.double(), ref, atol=1e-4,
                                          rtol=1e-4), (transposed, p)
                else:
                    err = (got.double() - ref).abs().max() / ref.abs().max()
                    assert err < 0.02, (transposed, p, err.item())


@pytest.mark.gpu
@pytest.mark.parametrize("F,prescale", [(1, True), (64, False)])
def test_spmm_mean_edge_drop_gpu(F, prescale, monkeypatch):
    """At F = 1 csc.nnz = 1288 > grad.numel() = 140: the backward pre-scales
    and hands the live-row count on. At F = 64, 8960 > 1288: it takes the
    fused src_scale gather."""
    hg = graph("cuda")
    inv_deg = _inv_deg(graph())
    grad = float_input(NUM_OUT, F)
    assert (hg.csc.nnz > grad.numel()) == prescale

    calls = []
    real = ops.scale_rows_live

    def counting(g, inv):
        calls.append(tuple(g.shape))
        return real(g, inv)

    monkeypatch.setattr(ops, "scale_rows_live", counting)
    x = float_input(NUM_SRC, F).cuda().requires_grad_(True)
    out = ops.spmm_mean(hg, x, inv_deg.cuda(), edge_drop=0.5, seed=SEED)
    out.backward(grad.cuda())
    assert len(calls) == (1 if prescale else 0)
    ref_out, ref_grad = _mean_reference(x.detach().cpu(), inv_deg, grad, 0.5)
    assert torch.allclose(out.detach().cpu().double(), ref_out, atol=1e-4,
                          rtol=1e-4)
    assert torch.allclose(x.grad.cpu().double(), ref_grad, atol=1e-4,
                          rtol=1e-4)


@pytest.mark.gpu
def test_undersized_feat_raises_before_any_launch(monkeypatch):
    hg = graph("cuda")

    def boom(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(native(), "spmm_drop", boom)
    x = float_input(NUM_SRC, 64).cuda()
    with pytest.raises(ValueError, match="under-sized"):
        ops.spmm_drop(hg.csr, x[: NUM_SRC - 1], p=0.5, seed=SEED)
    with pytest.raises(ValueError, match="under-sized"):
        ops.spmm_drop(hg.csc, x[: NUM_OUT - 1], p=0.5, seed=SEED,
                      transposed=True)
    with pytest.raises(ValueError, match="under-sized"):
        ops.spmm_mean(hg, x[: NUM_SRC - 1],
                      _inv_deg(graph()).cuda(), edge_drop=0.5, seed=SEED)
