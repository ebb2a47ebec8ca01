"""GAT attention dropout: the keep hash (torch mirror and device function),
ops.gat_aggregate(attn_drop=...) on the CPU path and on the gfx950 kernels,
and the model / CLI plumbing.

The graph, shapes and seeded inputs are those of tests/test_gat_ops.py. The
reference is written here: that file's float64 dense softmax, its alpha
multiplied by the mirror's [n_dst, n_src, H] keep mask and by 1 / (1 - p),
differentiated by torch autograd.

Tolerances (the existing file's policy):
 - out, dz: atol = rtol = 1e-4.
 - d_el, d_er: at most 4x the max error of a plain fp32 torch evaluation of
   the same closed form (`_eager32_drop`) against float64.
 - bf16: max error over the reference's max-norm < 0.02.
 - mirror statistics: 5 sigma of the binomial, never a measured figure.
"""
import dataclasses
import functools
import math

import pytest
import torch

from pipegcn_amd import native, ops
from pipegcn_amd.graph.csr import FullGraph, HaloGraph
from tests.conftest import run_distributed
from tests.test_gat_ops import (DEG1_ROW, EMPTY_ROWS, N_DST, N_SRC,
                                SHAPES, SLOPE, case, edges, graph)
from tests.test_launcher import run_main

SEED = 1234
GRID_H = 8


def _grid(device="cpu"):
    """Every (u, v) of the 300 x 200 node grid, v-major: [n_dst * n_src]."""
    v, u = torch.meshgrid(torch.arange(N_DST, device=device),
                          torch.arange(N_SRC, device=device), indexing="ij")
    return u.reshape(-1), v.reshape(-1)


# ----------------------------------------------------------- mirror (CPU)


@pytest.mark.parametrize("p", [0.1, 0.6, 0.9])
@pytest.mark.parametrize("seed", [0, SEED, 2 ** 62 - 2])
def test_mirror_statistics(p, seed):
    u, v = _grid()
    k0 = ops.gat_dropout_keep(u, v, GRID_H, seed, p)
    k1 = ops.gat_dropout_keep(u, v, GRID_H, seed + 1, p)
    assert k0.dtype == torch.bool and k0.shape == (u.numel(), GRID_H)
    n = k0.numel()
    assert n == 480_000
    sd = math.sqrt(p * (1 - p) / n)
    rate = k0.double().mean().item()
    print(f"p={p} seed={seed}: keep rate z = {(rate - (1 - p)) / sd:+.2f}")
    assert abs(rate - (1 - p)) <= 5 * sd
    sd_h = math.sqrt(p * (1 - p) / (n / GRID_H))
    for h in range(GRID_H):
        rate_h = k0[:, h].double().mean().item()
        assert abs(rate_h - (1 - p)) <= 5 * sd_h, (h, rate_h)
    e = (1 - p) ** 2 + p ** 2
    sd_e = math.sqrt(e * (1 - e) / n)
    agree = (k0 == k1).double().mean().item()
    print(f"  seeds s, s+1 agreement z = {(agree - e) / sd_e:+.2f}")
    assert abs(agree - e) <= 5 * sd_e
    sd_eh = math.sqrt(e * (1 - e) / (n / GRID_H))
    for h0 in range(GRID_H):
        for h1 in range(h0 + 1, GRID_H):
            agree_h = (k0[:, h0] == k0[:, h1]).double().mean().item()
            assert abs(agree_h - e) <= 5 * sd_eh, (h0, h1, agree_h)


def test_mirror_endpoints_not_position():
    """A function of (seed, u, v, h) only: any id dtype, any order, and
    duplicate edges share their bits."""
    u, v = edges()
    k = ops.gat_dropout_keep(u, v, 4, SEED, 0.6)
    assert torch.equal(k, ops.gat_dropout_keep(u.int(), v.int(), 4, SEED, 0.6))
    perm = torch.randperm(u.numel(), generator=torch.Generator().manual_seed(0))
    assert torch.equal(k[perm],
                       ops.gat_dropout_keep(u[perm], v[perm], 4, SEED, 0.6))
    assert ops.gat_dropout_keep(u, v, 4, SEED, 0.0).all()
    with pytest.raises(ValueError):
        ops.gat_dropout_keep(u, v, 4, SEED, 1.0)


# ------------------------------------------------- the float64 reference


def _dense_drop(z, el, er, H, p, seed):
    """test_gat_ops._dense_attention's softmax with alpha masked: float64,
    autograd-capable -> out."""
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
    gu, gv = _grid()
    keep = ops.gat_dropout_keep(gu, gv, H, seed, p).view(N_DST, N_SRC, H)
    alpha = alpha * keep.double() / (1.0 - p)
    zh = z.view(N_SRC, H, -1)
    return torch.einsum("vuh,uhd->vhd", alpha, zh).reshape(N_DST, -1)


@functools.lru_cache(maxsize=None)
def drop_case(H, D, p, seed=SEED, big=False, bf16=False):
    """test_gat_ops.case's inputs with the dropped float64 reference,
    computed once per (shape, p, seed) and shared read-only."""
    c = case(H, D, big, bf16)
    z64, el64, er64 = (c[k].double().requires_grad_(True)
                       for k in ("z", "el", "er"))
    out = _dense_drop(z64, el64, er64, H, p, seed)
    dz, d_el, d_er = torch.autograd.grad(out, (z64, el64, er64),
                                         c["g"].double())
    ref = dict(out=out.detach(), dz=dz, d_el=d_el, d_er=d_er)
    for t in ref.values():
        assert torch.isfinite(t).all()
    return dict(z=c["z"], el=c["el"], er=c["er"], g=c["g"], ref=ref)


def _eager32_drop(c, H, p, seed):
    """d_el, d_er from the closed form with dropout in plain fp32 torch ops
    on the edge list — the yardstick for the summation error. The masked
    weight multiplies every gathered row; csum and sum_v c*t are unmasked."""
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
    w = ops.gat_dropout_keep(u, v, H, seed, p).float() * (1.0 / (1.0 - p))
    zh, gh = z.view(N_SRC, H, -1), g.view(N_DST, H, -1)
    out = torch.zeros(N_DST, H, zh.shape[2]).index_add(
        0, v, (w * alpha).unsqueeze(-1) * zh[u])
    zc = torch.zeros_like(out).index_add(0, v, (w * cw).unsqueeze(-1) * zh[u])
    csum = torch.zeros(N_DST, H).index_add(0, v, cw)
    t = (gh * out).sum(-1)
    gc = torch.zeros_like(zh).index_add(0, u, (w * cw).unsqueeze(-1) * gh[v])
    d_el = (zh * gc).sum(-1) - torch.zeros(N_SRC, H).index_add(
        0, u, cw * t[v])
    d_er = (gh * zc).sum(-1) - t * csum
    return d_el, d_er


def _run(c, H, device, p, seed=SEED, dtype=torch.float32, hg=None):
    hg = hg if hg is not None else graph(device)
    z, el, er = (c[k].to(device=device, dtype=dtype).clone()
                 .requires_grad_(True) for k in ("z", "el", "er"))
    out = ops.gat_aggregate(hg, z, el, er, H, SLOPE, attn_drop=p, seed=seed)
    out.backward(c["g"].to(device=device, dtype=dtype))
    return out.detach(), z.grad, el.grad, er.grad


def _close(a, ref):
    return torch.allclose(a.double().cpu(), ref, atol=1e-4, rtol=1e-4)


def _err(a, ref):
    return (a.double().cpu() - ref).abs().max().item()


def _check(device, H, D, p, big=False):
    c = drop_case(H, D, p, big=big)
    ref = c["ref"]
    out, dz, d_el, d_er = _run(c, H, device, p)
    for t in (out, dz, d_el, d_er):
        assert torch.isfinite(t).all()
    assert (out[list(EMPTY_ROWS)] == 0).all(), "empty rows must be zero"
    assert _close(out, ref["out"]), _err(out, ref["out"])
    assert _close(dz, ref["dz"]), _err(dz, ref["dz"])
    eager_el, eager_er = _eager32_drop(c, H, p, SEED)
    for name, got, eager in (("d_el", d_el, eager_el),
                             ("d_er", d_er, eager_er)):
        e_eager, e_got = _err(eager, ref[name]), _err(got, ref[name])
        print(f"{device} H={H} D={D} p={p} big={big} {name}: eager fp32 err "
              f"{e_eager:.3e}, got {e_got:.3e}")
        # Measured max abs error against float64 as "eager fp32 / kernel on
        # MI355X / CPU path", seed 1234, unit-normal inputs unless "s90":
        #   shape, p        d_el                       d_er
        #   (1,41) .6       2.19e-6 1.87e-6 2.15e-6    2.86e-6 2.38e-6 1.34e-6
        #   (4,16) .6       1.65e-6 2.23e-6 2.23e-6    2.10e-6 2.61e-6 1.34e-6
        #   (8,32) .6       2.72e-6 3.80e-6 2.45e-6    3.23e-6 2.66e-6 2.67e-6
        #   (3,100) .6      4.85e-6 8.42e-6 5.16e-6    5.60e-6 3.92e-6 3.58e-6
        #   (2,301) .6      6.68e-6 5.56e-6 5.04e-6    8.64e-6 1.24e-5 7.17e-6
        #   (4,16) .9       4.81e-6 5.66e-6 1.97e-6    3.55e-6 5.38e-6 3.11e-6
        #   (2,301) .9      2.27e-5 1.85e-5 1.36e-5    2.34e-5 1.91e-5 3.17e-5
        #   (4,16) .6 s90   7.32e-5 7.32e-5 -          5.25e-5 5.25e-5 -
        # Worst kernel/eager ratio 1.74 (d_el at (3,100), p = 0.6), worst
        # CPU-path/eager ratio 2.0 (d_er at (2,301), p = 0.9, where the
        # eager figure on that host was 1.58e-5); the bound is 4.
        assert e_got <= 4 * e_eager, (name, e_got, e_eager)


# --------------------------------------------------------- op on the CPU


@pytest.mark.parametrize("p", [0.6, 0.9])
@pytest.mark.parametrize("H,D", SHAPES)
def test_gat_dropout_cpu(H, D, p):
    _check("cpu", H, D, p)


def _deg1_seeds(H, p):
    """The first seed that keeps and the first that drops head 0 of
    DEG1_ROW's only edge, found by evaluating the mirror."""
    hg = graph("cpu")
    src = hg.csr.indices[hg.csr.indptr[DEG1_ROW]].view(1).long()
    dst = torch.tensor([DEG1_ROW])
    kept = dropped = None
    for seed in range(64):
        bit = bool(ops.gat_dropout_keep(src, dst, H, seed, p)[0, 0])
        if bit and kept is None:
            kept = seed
        if not bit and dropped is None:
            dropped = seed
    return src, dst, kept, dropped


def _deg1_check(device):
    H, D, p = 4, 16, 0.6
    src, dst, kept, dropped = _deg1_seeds(H, p)
    assert kept is not None and dropped is not None
    assert ops.gat_dropout_keep(src, dst, H, kept, p)[0, 0]
    assert not ops.gat_dropout_keep(src, dst, H, dropped, p)[0, 0]
    c = case(H, D)
    # kept: alpha = 1 on a degree-1 row, so the head is z[src] / (1 - p)
    out = _run(c, H, device, p, seed=kept)[0].cpu()
    want = c["z"][src[0], :D] / (1 - p)
    assert torch.allclose(out[DEG1_ROW, :D], want, atol=1e-5, rtol=1e-5)
    out, dz, d_el, d_er = _run(c, H, device, p, seed=dropped)
    assert (out[DEG1_ROW, :D] == 0).all(), "dropped head must be exactly 0"
    assert (out[list(EMPTY_ROWS)] == 0).all()
    for t in (out, dz, d_el, d_er):
        assert torch.isfinite(t).all()


def test_gat_dropout_degree1_row_cpu():
    _deg1_check("cpu")


def _p0_and_validation(device):
    c = case(4, 16)
    hg = graph(device)

    def run(**kw):
        z, el, er = (c[k].to(device).clone().requires_grad_(True)
                     for k in ("z", "el", "er"))
        out = ops.gat_aggregate(hg, z, el, er, 4, SLOPE, **kw)
        out.backward(c["g"].to(device))
        return out.detach(), z.grad, el.grad, er.grad

    plain = run()
    state = torch.get_rng_state()
    zero = run(attn_drop=0.0)
    assert torch.equal(state, torch.get_rng_state()), \
        "attn_drop == 0 must not draw from the generator"
    for a, b in zip(plain, zero):
        assert torch.equal(a, b)
    run(attn_drop=0.5)  # seed=None draws exactly as fused_dropout does
    assert not torch.equal(state, torch.get_rng_state())
    z, el, er = (c[k].to(device) for k in ("z", "el", "er"))
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError, match="attn_drop"):
            ops.gat_aggregate(hg, z, el, er, 4, SLOPE, attn_drop=bad)


def test_gat_dropout_p0_and_validation_cpu():
    _p0_and_validation("cpu")


# ------------------------------------------------------ model and CLI (CPU)


def _layer_graphs():
    u, v = edges()
    keep = u < N_DST  # a square graph for the eval path
    full = FullGraph.from_coo(u[keep], v[keep], N_DST)
    halo = HaloGraph.from_edges(u, v, N_DST, N_SRC)
    return halo, full


def test_gat_layer_attn_drop_train_and_eval():
    from pipegcn_amd.models.gat import GAT, GATLayer

    halo, full = _layer_graphs()
    torch.manual_seed(0)
    drop = GATLayer(12, 16, num_heads=4, attn_drop=0.6)
    plain = GATLayer(12, 16, num_heads=4)
    plain.load_state_dict(drop.state_dict())
    x = torch.randn(N_SRC, 12)
    drop.eval(), plain.eval()
    with torch.no_grad():
        assert torch.equal(drop(full, x[:N_DST]), plain(full, x[:N_DST]))
    drop.train(), plain.train()
    torch.manual_seed(5)
    a = drop(halo, x)
    b = drop(halo, x)  # no reseed: another mask
    torch.manual_seed(5)
    a2 = drop(halo, x)
    assert torch.equal(a, a2)
    assert not torch.equal(a, b)
    assert not torch.equal(a, plain(halo, x))
    with pytest.raises(ValueError, match="attn_drop"):
        GATLayer(12, 16, num_heads=4, attn_drop=1.0)
    model = GAT([12, 16, 16, 3], torch.relu, n_heads=4, attn_drop=0.6)
    assert [l.attn_drop for l in model.layers] == [0.6, 0.6, 0.6]


def test_cli_attn_drop():
    from pipegcn_amd import trainer
    from pipegcn_amd.cli import create_parser
    from tests.test_distributed import make_args

    assert create_parser([]).attn_drop == 0.0
    assert create_parser(["--attn-drop", "0.6"]).attn_drop == 0.6
    assert create_parser(["--attn_drop", "0.25"]).attn_drop == 0.25
    model = trainer.create_model(
        [16, 8, 8, 3], make_args(model="gat", n_hidden=8, n_heads=2,
                                 attn_drop=0.6))
    assert all(l.attn_drop == 0.6 for l in model.layers)
    # a namespace without the attribute (older callers) means no dropout
    model = trainer.create_model([16, 8, 8, 3],
                                 make_args(model="gat", n_hidden=8))
    assert all(l.attn_drop == 0.0 for l in model.layers)


def test_main_gat_attn_drop(tmp_path):
    out = run_main(tmp_path, ["--model", "gat", "--n-heads", "2",
                              "--attn-drop", "0.6", "--enable-pipeline"])
    assert "Epoch" in out and "nan" not in out
    assert "Validation Accuracy" in out
    assert "model saved" in out


# ------------------------------------------------------------------- GPU


@pytest.mark.gpu
def test_probe_matches_mirror_gpu():
    u, v = _grid("cuda")
    for seed in (SEED, 2 ** 62 - 1):
        for p in (0.1, 0.6):
            got = native().gat_dropout_keep(u.int(), v.int(), GRID_H, seed, p)
            want = ops.gat_dropout_keep(u, v, GRID_H, seed, p)
            assert got.dtype == torch.bool and got.shape == want.shape
            assert torch.equal(got, want), (seed, p)
    # ids up to 2^31 - 1 hash as uint32, without sign extension
    ids = torch.tensor([0, 1, 65536, 2 ** 31 - 1], device="cuda")
    u, v = (t.reshape(-1) for t in torch.meshgrid(ids, ids, indexing="ij"))
    for seed in (SEED, SEED + 1):
        got = native().gat_dropout_keep(u.int(), v.int(), GRID_H, seed, 0.5)
        assert torch.equal(got, ops.gat_dropout_keep(u, v, GRID_H, seed, 0.5))
        assert torch.equal(got.cpu(), ops.gat_dropout_keep(
            u.cpu(), v.cpu(), GRID_H, seed, 0.5))


@pytest.mark.gpu
@pytest.mark.parametrize("H,D,p", [(H, D, 0.6) for H, D in SHAPES]
                         + [(4, 16, 0.9), (2, 301, 0.9)])
def test_gat_dropout_gpu(H, D, p):
    _check("cuda", H, D, p)


@pytest.mark.gpu
def test_gat_dropout_large_scores_gpu():
    _check("cuda", 4, 16, 0.6, big=True)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", [(4, 16), (8, 32)])
def test_gat_dropout_bf16_gpu(H, D):
    c = drop_case(H, D, 0.6, bf16=True)
    out, dz, d_el, d_er = _run(c, H, "cuda", 0.6, dtype=torch.bfloat16)
    for name, t in (("out", out), ("dz", dz), ("d_el", d_el),
                    ("d_er", d_er)):
        assert t.dtype == torch.bfloat16, name
        ref = c["ref"][name]
        err = _err(t, ref) / ref.abs().max().item()
        print(f"bf16 H={H} D={D} p=0.6 {name}: rel err {err:.3e}")
        assert err < 0.02, (name, err)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", [(4, 16), (2, 301)])
def test_gat_dropout_reproducible_gpu(H, D):
    c = case(H, D)
    hg = graph("cuda")
    first = _run(c, H, "cuda", 0.6)
    again = _run(c, H, "cuda", 0.6)
    natural = HaloGraph(dataclasses.replace(hg.csr, row_order=None),
                        dataclasses.replace(hg.csc, row_order=None),
                        hg.num_in, hg.num_all)
    unordered = _run(c, H, "cuda", 0.6, hg=natural)
    for a, b, n in zip(first, again, unordered):
        assert torch.equal(a, b)
        assert torch.equal(a, n)
    other = _run(c, H, "cuda", 0.6, seed=SEED + 1)
    assert not torch.equal(first[0], other[0])
    # the CPU path draws the same mask for the same seed
    cpu = _run(c, H, "cpu", 0.6)
    assert torch.allclose(first[0].cpu(), cpu[0], atol=1e-4, rtol=1e-4), \
        (first[0].cpu() - cpu[0]).abs().max()


@pytest.mark.gpu
def test_gat_dropout_degree1_row_gpu():
    _deg1_check("cuda")


@pytest.mark.gpu
def test_gat_dropout_p0_and_validation_gpu():
    _p0_and_validation("cuda")


@pytest.mark.gpu
def test_gat_dropout_no_nnz_sized_allocation_gpu():
    """Dropout allocates nothing more than the p = 0 call (plus 64 KiB of
    slack): a one-bit-per-edge-and-head mask would be 500 KB here."""
    n_src, n_dst, nnz, H, D = 3000, 2000, 1_000_000, 4, 8
    gen = torch.Generator().manual_seed(3)
    u = torch.randint(0, n_src, (nnz,), generator=gen)
    v = torch.randint(0, n_dst, (nnz,), generator=gen)
    hg = HaloGraph.from_edges(u, v, n_dst, n_src).to("cuda")
    z0 = torch.randn(n_src, H * D, generator=gen).cuda()
    el0 = torch.randn(n_src, H, generator=gen).cuda()
    er0 = torch.randn(n_dst, H, generator=gen).cuda()
    g = torch.randn(n_dst, H * D, generator=gen).cuda()

    def growth(p):
        z, el, er = (t.clone().requires_grad_(True) for t in (z0, el0, er0))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        resident = torch.cuda.memory_allocated()
        out = ops.gat_aggregate(hg, z, el, er, H, SLOPE, attn_drop=p,
                                seed=SEED)
        out.backward(g)
        torch.cuda.synchronize()
        grew = torch.cuda.max_memory_allocated() - resident
        assert torch.isfinite(z.grad).all() and torch.isfinite(el.grad).all()
        return grew

    growth(0.0)  # warm: the first call of a process may allocate workspaces
    base, dropped = growth(0.0), growth(0.6)
    print(f"peak growth p=0: {base} B, p=0.6: {dropped} B")
    assert dropped <= base + 64 * 1024, (dropped, base)


def _model_fwd_bwd(device):
    """tests/test_gat_model.py's comparison with attn_drop = 0.6: the seeds
    come from the host generator, so both devices draw the same masks."""
    import torch.nn.functional as F

    from pipegcn_amd.graph.halo import build_runtime_partition
    from pipegcn_amd.graph.synthetic import synth_partition
    from pipegcn_amd.models.gat import GAT
    from pipegcn_amd.parallel import context as ctx
    from pipegcn_amd.parallel.buffer import Buffer
    from pipegcn_amd.trainer import get_layer_size

    part = synth_partition("small", 0, 1, seed=0)
    rp = build_runtime_partition(part, device=device)
    layer_size = get_layer_size(part.n_feat, 32, part.n_class, 2)
    ctx.buffer = Buffer()
    ctx.buffer.init_buffer(rp.num_in, rp.num_all, rp.boundary,
                           rp.recv_shape, layer_size[:2], device=device)
    torch.manual_seed(7)
    model = GAT(layer_size, F.relu, dropout=0.0, norm="layer",
                train_size=part.n_train, n_heads=4,
                attn_drop=0.6).to(device)
    model.train()
    logits = model(rp.graph, rp.ndata["feat"])
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(
        logits[: rp.num_train], rp.ndata["label"][: rp.num_train])
    loss.backward()
    ctx.buffer.shutdown()
    return (logits.detach().cpu(),
            {k: p.grad.cpu() for k, p in model.named_parameters()})


def _model_gpu_vs_cpu_worker(rank, world):
    cpu_logits, cpu_grads = _model_fwd_bwd("cpu")
    gpu_logits, gpu_grads = _model_fwd_bwd("cuda:0")
    assert torch.allclose(gpu_logits, cpu_logits, atol=1e-4, rtol=1e-4), \
        (gpu_logits - cpu_logits).abs().max()
    assert set(cpu_grads) == set(gpu_grads) and "layers.0.attn_l" in cpu_grads
    for k, ref in cpu_grads.items():
        err = (gpu_grads[k] - ref).abs().max() / ref.abs().max()
        print(f"{k}: rel-to-max err {err:.3e}")
        assert err < 1e-4, (k, err.item())
    return True


@pytest.mark.gpu
def test_gat_dropout_model_gpu_matches_cpu():
    run_distributed(_model_gpu_vs_cpu_worker, 1, timeout=600)
