"""The fused backward of the GraphSAGE mean layer (docs/DESIGN.md, "Fused
layer backward"): the add / dropout epilogue of the transpose SpMM, the one
autograd node that uses it, the dgrads gated on who wants them, and the column
sum that keeps several rows in flight. Everything is compared bit for bit with
the unfused composition run in the same test; colsum with the outputs the
kernel gave before it was changed (tests/golden/colsum_*.npy)."""
import os

import numpy as np
import pytest
import torch

from pipegcn_amd import native, ops
from pipegcn_amd.graph.csr import HaloGraph

NUM_IN, NUM_ALL = 37, 48
DEGREES = [0, 1, 3, 4, 5, 9]  # empty, peel only, one group, group plus tail
WIDTHS = [8, 20, 130]
DTYPES = [torch.float32, torch.bfloat16]
P = 0.3  # 1 / (1 - p) is no power of two: the multiply rounds
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_CACHE = {}


def _halo_graph(extra_deg=0):
    """48 source rows (37 inner, 11 halo) whose out-degrees run through
    DEGREES (+ extra_deg), to uniform inner destinations."""
    key = ("graph", extra_deg)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(11)
        deg = torch.tensor(DEGREES).repeat(NUM_ALL // len(DEGREES)) + extra_deg
        u = torch.repeat_interleave(torch.arange(NUM_ALL), deg)
        v = torch.randint(0, NUM_IN, (u.numel(),), generator=g)
        hg = HaloGraph.from_edges(u, v, NUM_IN, NUM_ALL)
        assert sorted(set(hg.csc.row_degrees().long().tolist())) == [
            d + extra_deg for d in DEGREES]
        _CACHE[key] = hg
    return _CACHE[key]


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _rand(rows, cols, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, cols, generator=g).to(dtype).cuda()


def _mask(F, p=P, seed=77):
    """The bit mask dropout_fwd writes over a [NUM_ALL, F] tensor."""
    _, mask = native().dropout_fwd(
        torch.ones(NUM_ALL, F, device="cuda"), p, seed)
    assert mask.numel() == (NUM_ALL * F + 7) // 8
    return mask


def _unfused(plain, add, mask, p=P):
    """What autograd made of the transpose SpMM's output: the accumulate
    with the zero-padded self term, then dropout_bwd."""
    out = plain
    if add is not None:
        pad = torch.zeros_like(plain)
        pad[: add.shape[0]] = add
        out = plain + pad
    if mask is not None:
        out = native().dropout_bwd(out, mask, p)
    return out


def _epilogue_cases(F, dtype):
    """(name, spmm kwargs, feat) of the kernel instances the epilogue must
    serve: plain, src_scale, n_live."""
    feat = _rand(NUM_IN, F, 1, dtype)
    dead = feat.clone()
    dead[20:] = 0.0
    n_live = torch.tensor([20], dtype=torch.int32, device="cuda")
    src_scale = (torch.rand(NUM_IN, generator=torch.Generator().manual_seed(
        2)) + 0.5).cuda()
    return [("plain", {}, feat), ("src_scale", dict(src_scale=src_scale),
                                  feat), ("n_live", dict(n_live=n_live),
                                          dead)]


def _check_epilogue(F, dtype):
    csc = _halo_graph().csc.to("cuda")
    add = _rand(NUM_IN, F, 3, dtype)
    wide = _rand(NUM_IN, 2 * F + 3, 4, dtype)
    sliced = wide[:, 3:F + 3]  # a column slice: row stride 2F + 3
    assert not sliced.is_contiguous()
    mask = _mask(F)
    scale = ops.dropout_scale(P)
    for name, kw, feat in _epilogue_cases(F, dtype):
        plain = ops.spmm(csc, feat, None, **kw)
        assert plain.shape == (NUM_ALL, F)
        for a in (add, sliced):
            # add and mask: rows 37..47 get no self term (n_add < num_rows)
            got = ops.spmm(csc, feat, None, add_rows=a, n_add=NUM_IN,
                           drop_mask=mask, drop_scale=scale, **kw)
            assert torch.equal(_bits(got), _bits(_unfused(plain, a, mask))), \
                (name, F, "add+mask")
            # add only; n_add defaults to add_rows' rows
            got = ops.spmm(csc, feat, None, add_rows=a, **kw)
            assert torch.equal(_bits(got), _bits(_unfused(plain, a, None))), \
                (name, F, "add")
        # fewer self rows than add_rows holds
        got = ops.spmm(csc, feat, None, add_rows=add, n_add=5, **kw)
        assert torch.equal(_bits(got), _bits(_unfused(plain, add[:5], None)))
        # mask only
        got = ops.spmm(csc, feat, None, drop_mask=mask, drop_scale=scale,
                       **kw)
        assert torch.equal(_bits(got), _bits(_unfused(plain, None, mask))), \
            (name, F, "mask")
        # neither: the kernel it always was
        none = torch.Tensor()
        got = native().spmm(csc.indptr, csc.indices, feat, none,
                            kw.get("src_scale", none), csc.row_order,
                            csc.num_rows, kw.get("n_live"), None, 0, None,
                            1.0)
        assert torch.equal(_bits(got), _bits(plain)), (name, F, "neither")


# --------------------------------------------------------------- epilogue op


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", WIDTHS)
def test_epilogue_bitwise(F, dtype):
    _check_epilogue(F, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("vec", [1, 2, 4, 8])
def test_epilogue_forced_lane_widths(vec, dtype, monkeypatch):
    """The widths pick_vec does not choose by itself, where it accepts them:
    a forced width that does not divide F or exceeds 16 bytes per lane falls
    back to the default. So F = 8 runs 1, 2, 4 (and 8 in bf16), F = 20 runs 1,
    2, 4, and F = 130 runs 1 and 2, where its last chunk is a short one of
    full lanes. No width ever leaves a lane half inside a row: the kernel's
    guarded branch for that is not reachable through pick_vec."""
    monkeypatch.setenv("PIPEGCN_SPMM_VEC", str(vec))
    for F in WIDTHS:
        _check_epilogue(F, dtype)


@pytest.mark.gpu
def test_epilogue_mask_bytes_straddle_rows():
    """At F = 20 a mask byte covers the end of one row and the start of the
    next; the kept set must be dropout_fwd's, element for element."""
    F = 20
    csc = _halo_graph().csc.to("cuda")
    y, mask = native().dropout_fwd(torch.ones(NUM_ALL, F, device="cuda"),
                                   0.5, 123)
    feat = _rand(NUM_IN, F, 9)
    plain = ops.spmm(csc, feat, None)
    got = ops.spmm(csc, feat, None, drop_mask=mask, drop_scale=2.0)
    assert torch.equal(got, torch.where(y != 0, plain * 2.0,
                                        torch.zeros_like(plain)))
    assert 0 < (y == 0).sum() < y.numel()


@pytest.mark.gpu
def test_epilogue_refuses_dst_scale_and_bad_arguments():
    csc = _halo_graph().csc.to("cuda")
    feat, add = _rand(NUM_IN, 8, 1), _rand(NUM_IN, 8, 3)
    dst = torch.ones(NUM_ALL, device="cuda")
    none = torch.Tensor()
    with pytest.raises(ValueError, match="scale"):
        ops.spmm(csc, feat, dst, add_rows=add)
    with pytest.raises(ValueError, match="scale"):
        ops.spmm(csc, feat, dst, drop_mask=_mask(8), drop_scale=2.0)
    with pytest.raises(RuntimeError, match="dst_scale"):
        native().spmm(csc.indptr, csc.indices, feat, dst, none,
                      csc.row_order, csc.num_rows, None, add, NUM_IN, None,
                      1.0)
    # checked before any launch: out-of-bounds reads otherwise
    with pytest.raises(RuntimeError, match="n_add"):
        ops.spmm(csc, feat, None, add_rows=add, n_add=NUM_IN + 1)
    with pytest.raises(RuntimeError, match="drop_mask"):
        ops.spmm(csc, feat, None, drop_mask=_mask(8)[:-1], drop_scale=2.0)
    with pytest.raises(RuntimeError, match="add_rows"):
        ops.spmm(csc, feat, None, add_rows=_rand(NUM_IN, 9, 3))
    with pytest.raises(RuntimeError, match="add_rows"):
        ops.spmm(csc, feat, None, add_rows=add.bfloat16())


def test_epilogue_is_gpu_only():
    hg = _halo_graph()
    feat = torch.zeros(NUM_IN, 8)
    with pytest.raises(ValueError, match="GPU"):
        ops.spmm(hg.csc, feat, None, add_rows=feat)


def test_dropout_scale_is_the_kernels():
    assert ops.dropout_scale(0.5) == 2.0
    assert ops.dropout_scale(0.0) == 1.0
    p16 = int(0.3 * 65536.0 + 0.5)
    want = np.float32(1.0) / (np.float32(1.0) - np.float32(p16)
                              / np.float32(65536.0))
    assert ops.dropout_scale(0.3) == float(want)


# --------------------------------------------------------------------- layer


def _layer_case(n_in, n_out, dtype=torch.float32, extra_deg=0):
    hg = _halo_graph(extra_deg).to("cuda")
    torch.manual_seed(n_in * 100 + n_out)
    lin1 = torch.nn.Linear(n_in, n_out).cuda().to(dtype)
    lin2 = torch.nn.Linear(n_in, n_out).cuda().to(dtype)
    h = _rand(NUM_ALL, n_in, 5, dtype)
    grad = _rand(NUM_IN, n_out, 6, dtype)
    inv_deg = (1.0 / hg.csr.row_degrees().clamp(min=1.0)).contiguous()
    return hg, lin1, lin2, h, grad, inv_deg


def _run_layer(fused, p, hg, lin1, lin2, h, grad, inv_deg, need_h=True):
    for lin in (lin1, lin2):
        lin.weight.grad = lin.bias.grad = None
    h = h.clone().requires_grad_(need_h)
    torch.manual_seed(21)
    if fused:
        out = ops.sage_mean_layer(hg, h, inv_deg, lin1, lin2, p)
    else:
        feat = ops.fused_dropout(h, p) if p > 0 else h
        ah = ops.spmm_mean(hg, feat, inv_deg)
        out = ops.sage_dual_linear(feat[: hg.num_in], ah, lin1, lin2)
    state = torch.get_rng_state()
    out.backward(grad)
    return dict(out=out.detach(), gh=h.grad, gw1=lin1.weight.grad,
                gw2=lin2.weight.grad, gb1=lin1.bias.grad,
                gb2=lin2.bias.grad, rng=state)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        elif k == "rng":
            assert torch.equal(a[k], b[k]), k
        else:
            assert torch.equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("n_in,n_out", [(20, 64), (64, 64), (64, 7)])
def test_layer_node_equals_three_ops(n_in, n_out, p):
    """MFMA forward and dgrad at (20, 64) and (64, 64), the rocBLAS pair and
    the one cat-GEMM (whose column slice is add_rows) at (64, 7)."""
    case = _layer_case(n_in, n_out)
    _same(_run_layer(True, p, *case), _run_layer(False, p, *case))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_layer_node_prescale_branch(dtype, monkeypatch):
    """A graph dense enough (nnz > rows * F) for the pre-scale branch of the
    transpose, where the epilogue rides on the n_live instance; and bf16."""
    case = _layer_case(20, 64, dtype, extra_deg=20)
    assert case[0].csc.nnz > NUM_IN * 20
    live = []
    real = ops.scale_rows_live

    def counting(*a):
        live.append(1)
        return real(*a)

    monkeypatch.setattr(ops, "scale_rows_live", counting)
    fused = _run_layer(True, 0.5, *case)
    assert len(live) == 1
    _same(fused, _run_layer(False, 0.5, *case))
    # the sparse graph takes the src_scale branch in bf16 too
    case = _layer_case(20, 64, dtype)
    _same(_run_layer(True, 0.5, *case), _run_layer(False, 0.5, *case))


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_layer_node_frees_its_activations_once(p):
    """The node lets go of its activations in the backward (they would
    otherwise outlive the transpose SpMM, at the step's memory peak), so a
    second backward through a retained graph is refused, not wrong."""
    hg, lin1, lin2, h, grad, inv_deg = _layer_case(20, 64)
    h = h.clone().requires_grad_(True)
    out = ops.sage_mean_layer(hg, h, inv_deg, lin1, lin2, p)
    out.backward(grad, retain_graph=True)
    with pytest.raises(RuntimeError, match="second"):
        out.backward(grad)


# -------------------------------------------------------------------- gating


def _count_dgrads(monkeypatch):
    calls = []
    real = ops._sage_dgrad

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "_sage_dgrad", counted)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,n_out", [(20, 64), (64, 7)])
def test_no_dgrad_for_a_constant_input(n_in, n_out, monkeypatch):
    calls = _count_dgrads(monkeypatch)
    case = _layer_case(n_in, n_out)
    for fused in (True, False):
        ref = _run_layer(fused, 0.5, *case)
        assert len(calls) == 1
        got = _run_layer(fused, 0.5, *case, need_h=False)
        assert len(calls) == 1  # no dgrad at all
        assert got["gh"] is None
        ref["gh"] = None
        _same(got, ref)
        calls.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,n_out", [(20, 64), (64, 7), (300, 64)])
def test_dual_linear_one_input_needs_grad(n_in, n_out, monkeypatch):
    """(300, 64): wide K, the rocBLAS branch at a layer-0 width."""
    calls = _count_dgrads(monkeypatch)
    torch.manual_seed(n_in + n_out)
    lin1 = torch.nn.Linear(n_in, n_out).cuda()
    lin2 = torch.nn.Linear(n_in, n_out).cuda()
    x1, x2 = _rand(NUM_IN, n_in, 7), _rand(NUM_IN, n_in, 8)
    grad = _rand(NUM_IN, n_out, 9)

    def run(need1, need2):
        a = x1.clone().requires_grad_(need1)
        b = x2.clone().requires_grad_(need2)
        for lin in (lin1, lin2):
            lin.weight.grad = lin.bias.grad = None
        ops.sage_dual_linear(a, b, lin1, lin2).backward(grad)
        return (a.grad, b.grad, lin1.weight.grad, lin2.weight.grad,
                lin1.bias.grad)

    both = run(True, True)
    for need1, need2 in ((True, False), (False, True)):
        got = run(need1, need2)
        assert (got[0] is None) == (not need1)
        assert (got[1] is None) == (not need2)
        for g, ref in zip(got, both):
            if g is not None:
                assert torch.equal(_bits(g), _bits(ref))
    assert len(calls) == 3
    none = run(False, False)
    assert len(calls) == 3 and none[0] is None and none[1] is None
    for g, ref in zip(none[2:], both[2:]):
        assert torch.equal(_bits(g), _bits(ref))


@pytest.mark.gpu
def test_linear_colsum_gated(monkeypatch):
    calls = []
    real = ops._mm_dgrad

    def counted(g, w):
        calls.append(1)
        return real(g, w)

    monkeypatch.setattr(ops, "_mm_dgrad", counted)
    torch.manual_seed(4)
    lin = torch.nn.Linear(20, 7).cuda()
    x0, grad = _rand(NUM_IN, 20, 7), _rand(NUM_IN, 7, 9)

    def run(need):
        x = x0.clone().requires_grad_(need)
        lin.weight.grad = lin.bias.grad = None
        ops.linear(x, lin).backward(grad)
        return x.grad, lin.weight.grad, lin.bias.grad

    with_x = run(True)
    assert len(calls) == 1 and with_x[0] is not None
    without = run(False)
    assert len(calls) == 1 and without[0] is None
    assert torch.equal(without[1], with_x[1])
    assert torch.equal(without[2], with_x[2])


# --------------------------------------------------------------------- model


class _FixedHalo:
    """ctx.buffer's update(): the inner rows followed by constant halo rows,
    through a node that hands the inner rows' gradient on."""

    def update(self, layer, feat):
        g = torch.Generator().manual_seed(50 + layer)
        halo = torch.randn(NUM_ALL - NUM_IN, feat.shape[1], generator=g)
        return torch.cat((feat, halo.to(feat)))


def _model_step(monkeypatch, fused, dropout=0.5):
    import torch.nn.functional as F

    from pipegcn_amd.models.sage import GraphSAGE
    from pipegcn_amd.parallel import context as ctx

    monkeypatch.setenv("PIPEGCN_SAGE_FUSED", "1" if fused else "0")
    monkeypatch.setattr(ctx, "buffer", _FixedHalo())
    nodes = []
    real = ops.sage_mean_layer

    def counted(*a, **k):
        nodes.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "sage_mean_layer", counted)
    hg = _halo_graph().to("cuda")
    torch.manual_seed(5)
    model = GraphSAGE([20, 64, 64, 7], F.relu, use_pp=False, dropout=dropout,
                      norm="layer", train_size=NUM_IN).cuda()
    keys = list(model.state_dict())
    model.train()
    feat = _rand(NUM_IN, 20, 12)
    label = (torch.arange(NUM_IN) % 7).cuda()
    torch.manual_seed(6)
    logits = model(hg, feat, hg.csr.row_degrees())
    state = torch.get_rng_state()
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, label)
    loss.backward()
    out = {"logits": logits.detach(), "loss": loss.detach(), "rng": state}
    for k, p in model.named_parameters():
        out["grad." + k] = p.grad
    return out, len(nodes), keys


@pytest.mark.gpu
@pytest.mark.parametrize("dropout", [0.5, 0.0])
def test_model_step_fused_equals_unfused(dropout, monkeypatch):
    fused, n_fused, keys = _model_step(monkeypatch, True, dropout)
    plain, n_plain, keys_plain = _model_step(monkeypatch, False, dropout)
    assert (n_fused, n_plain) == (3, 0)
    assert keys == keys_plain
    assert len(fused) == 3 + 16
    _same(fused, plain)


def test_fused_path_is_gpu_training_mean_only():
    from pipegcn_amd.models.sage import GraphSAGELayer, SAGEPoolLayer

    x = torch.zeros(4, 8)
    layer = GraphSAGELayer(8, 8)
    assert not layer.fuses_dropout(x)  # CPU
    assert not hasattr(SAGEPoolLayer, "fuses_dropout")
    with pytest.raises(ValueError, match="dropout"):
        layer(None, x, None, dropout=0.5)


@pytest.mark.gpu
def test_fused_path_conditions(monkeypatch):
    from pipegcn_amd.models.sage import GraphSAGELayer

    x = torch.zeros(4, 8, device="cuda")
    assert GraphSAGELayer(8, 8).fuses_dropout(x)
    assert not GraphSAGELayer(8, 8, use_pp=True).fuses_dropout(x)
    assert not GraphSAGELayer(8, 8, edge_drop=0.5).fuses_dropout(x)
    assert not GraphSAGELayer(8, 8).eval().fuses_dropout(x)
    monkeypatch.setenv("PIPEGCN_SAGE_FUSED", "0")
    assert not GraphSAGELayer(8, 8).fuses_dropout(x)


# -------------------------------------------------------------------- colsum

COLSUM_SHAPES = [(1, 4), (257, 41), (1000, 256), (2049, 6)]


def _colsum_input(i):
    m, f = COLSUM_SHAPES[i]
    return torch.randn(m, f, generator=torch.Generator().manual_seed(1000 + i))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(COLSUM_SHAPES)),
                         ids=["x".join(map(str, s)) for s in COLSUM_SHAPES])
def test_colsum_reproduces_the_earlier_kernel(i):
    """The fixtures are the outputs of the kernel that summed one row at a
    time, on these inputs: the row order of the adds has not moved."""
    m, f = COLSUM_SHAPES[i]
    x = _colsum_input(i)
    got = native().colsum(x.cuda()).cpu()
    want = torch.from_numpy(np.load(os.path.join(GOLDEN,
                                                 f"colsum_{m}x{f}.npy")))
    assert torch.equal(_bits(got), _bits(want))
    assert torch.allclose(got.double(), x.double().sum(0), atol=1e-2,
                          rtol=1e-3)
