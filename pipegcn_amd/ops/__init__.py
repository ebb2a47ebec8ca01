"""Autograd wrappers over the native gfx950 kernels.

Replaces DGL's `update_all(fn.copy_src, fn.sum)` gSpMM + autograd
(/root/reference/module/layer.py:47-49) with our own CSR SpMM whose backward
runs the pre-built transpose (CSC) through the same kernel — no atomics.

Device dispatch happens inside pipegcn_amd._C: CUDA tensors go to the
hand-written HIP kernels (and FAIL if the extension is absent — there is no
eager fallback on GPU); CPU tensors use the native C++ paths.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch

from pipegcn_amd import native
from pipegcn_amd.graph.csr import CSR, HaloGraph


def _row_order(matrix: CSR) -> torch.Tensor:
    """The matrix's row order as the kernels take it: an empty tensor stands
    for natural order."""
    return matrix.row_order if matrix.row_order is not None else torch.Tensor()


def _tune_row_order(csr: CSR, feat, s, ss) -> bool:
    """One-shot A/B of LPT vs natural row order for this (graph, F).

    The best order depends on BOTH graph structure and feature width
    (measured: LPT wins on uniform-source graphs and at narrow F; natural
    order wins by ~11% at F=602 on locality-structured graphs, where the
    degree sort scatters the near-diagonal source reuse). Results are
    BITWISE IDENTICAL either way — row_order only changes which wave
    processes which row, never the per-row edge order — so the choice is
    purely a throughput decision, amortized over thousands of epochs.
    """
    import time

    nat = torch.Tensor()
    times = {}
    for key, ro in (("lpt", csr.row_order), ("nat", nat)):
        native().spmm(csr.indptr, csr.indices, feat, s, ss, ro,
                      csr.num_rows)  # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            native().spmm(csr.indptr, csr.indices, feat, s, ss, ro,
                          csr.num_rows)
        torch.cuda.synchronize()
        times[key] = time.perf_counter() - t0
    return times["lpt"] <= times["nat"]


def dropout_scale(p: float) -> float:
    """The fp32 factor 1 / (1 - p) as the dropout kernels form it: p is
    quantised to 1/65536 first (csrc/hip/elementwise.hip)."""
    p16 = int(p * 65536.0 + 0.5)
    return (torch.tensor(1.0) / torch.tensor(1.0 - p16 / 65536.0)).item()


def spmm(csr: CSR, feat: torch.Tensor,
         scale: Optional[torch.Tensor] = None,
         src_scale: Optional[torch.Tensor] = None,
         n_live: Optional[torch.Tensor] = None, *,
         add_rows: Optional[torch.Tensor] = None,
         n_add: Optional[int] = None,
         drop_mask: Optional[torch.Tensor] = None,
         drop_scale: float = 1.0) -> torch.Tensor:
    """out[r,:] = scale[r] * sum_{u in N(r)} src_scale[u] * feat[u,:].

    n_live (GPU, not with src_scale): one int32 in device memory, the
    caller's promise that the rows of feat from n_live on are all zero (as
    `scale_rows_live` counts them). The kernel then gathers the one zero row
    n_live in their place, which stays in cache; the result is bitwise the
    same (docs/DESIGN.md, "Dead gradient rows").

    Epilogue (GPU, not with scale; docs/DESIGN.md, "Fused layer backward"):
    add_rows [>= n_add, F] in feat's dtype (rows may be strided: a column
    slice of a wider tensor) is added to the first n_add output rows
    (default: all of add_rows); drop_mask is the uint8 bit mask
    `dropout_fwd` wrote over a [num_rows, F] tensor, and an element whose
    bit is clear becomes 0, the others are multiplied by drop_scale. The
    result is bitwise `dropout_bwd(out + pad(add_rows), drop_mask)`."""
    if feat.shape[0] < csr.num_cols:
        raise ValueError(
            f"spmm: feat has {feat.shape[0]} rows but the graph references "
            f"{csr.num_cols} source nodes (an under-sized feat would be an "
            "out-of-bounds GPU gather)")
    s = scale if scale is not None else torch.Tensor()
    ss = src_scale if src_scale is not None else torch.Tensor()
    feat = feat.contiguous()
    ro = _row_order(csr)
    # auto-tuned row order on real-sized GPU workloads (>= ~1G gathered
    # elements, where a kernel is multi-ms and the 6 extra timed launches
    # vanish into warmup); PIPEGCN_SPMM_AUTOTUNE=0 pins LPT
    if (feat.is_cuda and csr.row_order is not None
            and csr.nnz * feat.shape[1] >= (1 << 30)
            and os.environ.get("PIPEGCN_SPMM_AUTOTUNE", "1") == "1"):
        cache = getattr(csr, "_lpt_choice", None)
        if cache is None:
            cache = {}
            csr._lpt_choice = cache
        use_lpt = cache.get(feat.shape[1])
        if use_lpt is None:
            # the A/B makes 6 transient outputs; near the memory ceiling
            # (papers100M sizing: tuning fires mid-backward at peak) that
            # transient OOMs or inflates peak — keep the LPT default there
            free, _ = torch.cuda.mem_get_info(feat.device)
            out_bytes = csr.num_rows * feat.shape[1] * feat.element_size()
            if free < 3 * out_bytes + (2 << 30):
                use_lpt = True
            else:
                use_lpt = _tune_row_order(csr, feat, s, ss)
            cache[feat.shape[1]] = use_lpt
        if not use_lpt:
            ro = torch.Tensor()
    if add_rows is not None or drop_mask is not None:
        if scale is not None:
            raise ValueError(
                "spmm: the add/dropout epilogue does not combine with scale "
                "(acc * scale + add would contract to one rounding)")
        if not feat.is_cuda:
            raise ValueError("spmm: the add/dropout epilogue is the GPU path")
        if add_rows is not None and n_add is None:
            n_add = add_rows.shape[0]
        return native().spmm(csr.indptr, csr.indices, feat, s, ss, ro,
                             csr.num_rows, n_live, add_rows, n_add or 0,
                             drop_mask, drop_scale)
    if n_live is None:
        return native().spmm(csr.indptr, csr.indices, feat, s, ss,
                             ro, csr.num_rows)
    return native().spmm(csr.indptr, csr.indices, feat, s, ss,
                         ro, csr.num_rows, n_live)


def scale_rows_live(g: torch.Tensor, inv: torch.Tensor):
    """(g * inv per row, n_live) in one GPU pass: n_live is an int32 [1]
    device tensor holding 1 + the index of the last row of the product with
    a non-zero in it (0 if there is none; both zeros are zero, NaN and +-Inf
    are not). The product is bitwise `g * inv.unsqueeze(1).to(g.dtype)`.
    Nothing is read back to the host."""
    return native().scale_rows_live(g, inv)


def packed_row_layout(F: int):
    """(mask_words, hdr_words, stride_words) of a packed row of width F, in
    4-byte words, as csrc/hip/spmm_packed.hip lays it out (docs/DESIGN.md,
    "Packed rows"): mask_words header entries {uint32 mask, uint32 exclusive
    prefix count}, one per 32 columns; padding to hdr_words (a multiple of
    4, so the values start 16-byte aligned); then the non-zero values in
    column order. stride_words leaves 8 words of slack after F value slots
    and is a multiple of 32 (128 B)."""
    mask_words = (F + 31) // 32
    hdr_words = (2 * mask_words + 3) // 4 * 4
    stride_words = (hdr_words + F + 8 + 31) // 32 * 32
    return mask_words, hdr_words, stride_words


def pack_rows_reference(x: torch.Tensor) -> torch.Tensor:
    """The torch mirror of the device row-packing kernel: fp32 [N, F] ->
    int32 [N, stride_words]. Runs on x's device (CPU-capable). Header and
    the leading nnz value slots of each row are what the kernel writes, bit
    for bit; everything else (which the kernel leaves unwritten) is 0 here.
    "Non-zero" is v != 0: both zeros are dropped, NaN and +-Inf are kept."""
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("pack_rows_reference: fp32 [N, F] only")
    N, F = x.shape
    W, hdr, stride = packed_row_layout(F)
    nz = x != 0
    nzp = torch.zeros(N, W * 32, dtype=torch.int64, device=x.device)
    nzp[:, :F] = nz
    nzp = nzp.view(N, W, 32)
    mask = (nzp << torch.arange(32, device=x.device)).sum(-1)
    cnt = nzp.sum(-1)
    prefix = cnt.cumsum(-1) - cnt
    out = torch.zeros(N, stride, dtype=torch.int32, device=x.device)
    # values >= 2^31 wrap to the int32 with the same bits
    out[:, 0:2 * W:2] = ((mask + 2 ** 31) % 2 ** 32 - 2 ** 31).int()
    out[:, 1:2 * W:2] = prefix.int()
    rank = nz.long().cumsum(-1) - 1
    rows = torch.arange(N, device=x.device).unsqueeze(1).expand(N, F)
    out[rows[nz], hdr + rank[nz]] = x.contiguous().view(torch.int32)[nz]
    return out


def unpack_rows_reference(packed: torch.Tensor, F: int) -> torch.Tensor:
    """Inverse of the packing (dropped entries come back as +0.0): int32
    [N, stride_words] -> fp32 [N, F]. Reads only the header and the value
    slots the header points at."""
    W, hdr, stride = packed_row_layout(F)
    if packed.dim() != 2 or packed.shape[1] != stride \
            or packed.dtype != torch.int32:
        raise ValueError("unpack_rows_reference: not packed rows of width "
                         f"{F}")
    N = packed.shape[0]
    mask = packed[:, 0:2 * W:2].long() & _M32
    prefix = packed[:, 1:2 * W:2].long()
    bits = (mask.unsqueeze(-1) >> torch.arange(32, device=packed.device)) & 1
    rank = prefix.unsqueeze(-1) + bits.cumsum(-1) - bits
    nz = bits.view(N, W * 32)[:, :F].bool()
    rank = rank.view(N, W * 32)[:, :F]
    vals = packed[:, hdr:].gather(1, rank.clamp(max=stride - hdr - 1))
    return torch.where(nz, vals, torch.zeros_like(vals)).view(torch.float32)


def pack_rows(x: torch.Tensor) -> torch.Tensor:
    """Packed rows of a fp32 [N, F] tensor (device kernel on the GPU, the
    torch mirror elsewhere)."""
    if x.is_cuda:
        return native().pack_rows(x.contiguous())
    return pack_rows_reference(x)


def _spmm_packed_width(F: int) -> bool:
    """Static routing of the forward SpMM by feature width, read off the
    `spmm_bench --density` table on the Reddit shape (profiles/README.md,
    "Packed-row forward SpMM"). Pack pass plus packed gather against the
    dense kernel, at the one half / one quarter of non-zeros that dropout
    and dropout after ReLU leave: F=602 27.0 / 20.4 vs 41.3 ms, F=256 9.7 /
    6.8 vs 15.5, F=128 6.5 / 6.3 vs 9.9, F=64 5.4 / 5.3 vs 7.2. It wins at
    every measured width, layer 0 included; narrower ones were not measured
    and stay dense. With nothing to skip it costs 7-13 % (F=602 / F=256)
    and saves 3-6 % at F=128 / F=64."""
    return F >= 64


def _spmm_packed_route(feat: torch.Tensor) -> bool:
    """Whether _SpmmMean.forward takes the packed path for this input.
    PIPEGCN_SPMM_PACKED=0 pins the dense kernel everywhere. No density is
    counted here: that would need a device sync."""
    if (not feat.is_cuda or feat.dtype != torch.float32
            or os.environ.get("PIPEGCN_SPMM_PACKED", "1") == "0"
            or not _spmm_packed_width(feat.shape[1])):
        return False
    # the transient packed buffer: near the memory ceiling (papers100M
    # sizing) stay dense, as the row-order autotune stays put there
    free, _ = torch.cuda.mem_get_info(feat.device)
    need = feat.shape[0] * packed_row_layout(feat.shape[1])[2] * 4
    return free >= need + (2 << 30)


def spmm_packed(csr: CSR, feat: torch.Tensor,
                scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`spmm(csr, feat, scale)` for fp32 GPU inputs, skipping feat's zeros:
    feat is packed row by row (header of non-zero bits + the non-zero
    values), then gathered packed. Bitwise equal to `spmm` on any input;
    faster when a large share of feat is exactly zero (after dropout and
    ReLU). The packed buffer is transient."""
    if feat.shape[0] < csr.num_cols:
        raise ValueError(
            f"spmm_packed: feat has {feat.shape[0]} rows but the graph "
            f"references {csr.num_cols} source nodes (an under-sized feat "
            "would be an out-of-bounds GPU gather)")
    if not feat.is_cuda or feat.dtype != torch.float32 or feat.dim() != 2:
        raise ValueError("spmm_packed: fp32 [N, F] GPU tensors only")
    s = scale if scale is not None else torch.Tensor()
    # the dense path's row order: its cached autotune decision for this
    # (graph, F) if it made one, else the LPT order (no second autotune)
    ro = _row_order(csr)
    if getattr(csr, "_lpt_choice", {}).get(feat.shape[1]) is False:
        ro = torch.Tensor()
    packed = native().pack_rows(feat.contiguous())
    return native().spmm_packed(csr.indptr, csr.indices, packed,
                                feat.shape[1], s, ro, csr.num_rows)


def _spmm_mean_forward(graph: HaloGraph, feat: torch.Tensor,
                       inv_deg: torch.Tensor) -> torch.Tensor:
    # the forward input is dropout's output (half zeros, three quarters
    # after a ReLU): gather it packed. The backward's input is a gradient,
    # dense in the rows that have one, and stays on the dense kernel.
    if _spmm_packed_route(feat):
        return spmm_packed(graph.csr, feat, inv_deg)
    return spmm(graph.csr, feat, inv_deg)


def _spmm_mean_backward(g: HaloGraph, grad_out: torch.Tensor,
                        inv_deg: torch.Tensor, **epilogue) -> torch.Tensor:
    """A^T D^{-1} grad_out; `epilogue` are spmm's add/dropout arguments (the
    fused layer node), none for the plain op."""
    # D^{-1} either as ONE streaming row-multiply on g or as the
    # fused per-EDGE src_scale gather: the multiply costs ~3 passes
    # over [rows,F], the gather ~one 4B load per edge plus its
    # latency slot — dense graphs (reddit: nnz 115M > numel 60M,
    # measured +1 ms/call for pre-scale) want the multiply, sparse
    # wide ones (yelp: nnz 14M << numel 367M) want the gather
    if g.csc.nnz > grad_out.numel():
        if grad_out.is_cuda:
            # the multiply also finds where the gradient's all-zero
            # tail starts: the loss covers the train nodes, which are
            # numbered first, so under the last layer every later row
            # is zero, and the gather keeps those out of HBM. Other
            # layers find n_live == rows and nothing changes.
            # PIPEGCN_SPMM_LIVE=0 withholds the count.
            scaled, n_live = scale_rows_live(grad_out, inv_deg)
            if os.environ.get("PIPEGCN_SPMM_LIVE", "1") == "0":
                n_live = None
            return spmm(g.csc, scaled, None, n_live=n_live, **epilogue)
        return spmm(g.csc,
                    grad_out * inv_deg.unsqueeze(1).to(grad_out.dtype), None,
                    **epilogue)
    return spmm(g.csc, grad_out.contiguous(), None, src_scale=inv_deg,
                **epilogue)


class _SpmmMean(torch.autograd.Function):
    """ah = D^{-1} A h over the halo graph; backward = A^T D^{-1} g."""

    @staticmethod
    def forward(ctx, graph: HaloGraph, feat: torch.Tensor,
                inv_deg: torch.Tensor):
        ctx.graph = graph
        ctx.save_for_backward(inv_deg)
        return _spmm_mean_forward(graph, feat, inv_deg)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        (inv_deg,) = ctx.saved_tensors
        return None, _spmm_mean_backward(ctx.graph, grad_out, inv_deg), None


class _SpmmMeanDrop(torch.autograd.Function):
    """_SpmmMean over the edges one edge-dropout draw keeps, times
    1 / (1 - p): ah = D^{-1} (A o K) h / (1 - p), backward = its transpose
    over the same kept set. Only drop = (key, thr, scale) travels from the
    forward to the backward; both passes recompute the keep bits."""

    @staticmethod
    def forward(ctx, graph: HaloGraph, feat: torch.Tensor,
                inv_deg: torch.Tensor, drop):
        ctx.graph, ctx.drop = graph, drop
        ctx.save_for_backward(inv_deg)
        # the masked dense kernel: there is no masked packed gather
        # (docs/ROADMAP.md)
        return spmm_drop(graph.csr, feat, inv_deg, drop=drop)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        (inv_deg,) = ctx.saved_tensors
        g, drop = ctx.graph, ctx.drop
        # the two branches of _SpmmMean.backward, cost model and all
        if g.csc.nnz > grad_out.numel():
            n_live = None
            if grad_out.is_cuda:
                scaled, n_live = scale_rows_live(grad_out, inv_deg)
                if os.environ.get("PIPEGCN_SPMM_LIVE", "1") == "0":
                    n_live = None
            else:
                scaled = grad_out * inv_deg.unsqueeze(1).to(grad_out.dtype)
            grad_feat = spmm_drop(g.csc, scaled, drop=drop, transposed=True,
                                  n_live=n_live)
        else:
            grad_feat = spmm_drop(g.csc, grad_out.contiguous(),
                                  src_scale=inv_deg, drop=drop,
                                  transposed=True)
        return None, grad_feat, None, None


def spmm_mean(graph: HaloGraph, feat: torch.Tensor, inv_deg: torch.Tensor,
              edge_drop: float = 0.0,
              seed: Optional[int] = None) -> torch.Tensor:
    """Differentiable mean-aggregation over the halo graph.

    inv_deg is 1/in_degree of the dst nodes (full-graph degrees, precomputed
    before partitioning — reference semantics, /root/reference/helper/utils.py:142).

    edge_drop in [0, 1) removes each edge with that probability for this
    call (DropEdge) and scales the sum over the kept ones by
    1 / (1 - edge_drop); inv_deg stays as given, there is no re-normalisation
    over the kept edges. The mask is `edge_drop_keep(u, v, seed, edge_drop)`
    on local ids, the same in the forward and the backward. seed defaults to
    a draw from torch's host generator; edge_drop == 0 draws nothing and is
    the path this function always took.
    """
    drop = edge_drop_args("spmm_mean", edge_drop, seed)
    if drop[1] == 0:
        return _SpmmMean.apply(graph, feat, inv_deg)
    return _SpmmMeanDrop.apply(graph, feat, inv_deg, drop)


def _spmm_max_check(csr: CSR, z: torch.Tensor) -> None:
    """Raised before any launch."""
    if z.dim() != 2 or z.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("spmm_max: z must be a fp32 or bf16 [nodes, F] "
                         f"tensor, got {tuple(z.shape)} {z.dtype}")
    if z.shape[0] < csr.num_cols:
        raise ValueError(
            f"spmm_max: z has {z.shape[0]} rows but the graph references "
            f"{csr.num_cols} source nodes (an under-sized z would be an "
            "out-of-bounds GPU gather)")


def _spmm_max_forward(csr: CSR, z: torch.Tensor, with_arg: bool):
    """[out] or [out, arg] on z's device. Uses csr.row_order as given (no
    lazy autotune here)."""
    return native().spmm_max(csr.indptr, csr.indices, z.contiguous(),
                             _row_order(csr), csr.num_rows, csr.num_cols,
                             with_arg)


class _SpmmMax(torch.autograd.Function):
    """out[r] = max over u in N(r) of z[u], element-wise.

    Saves the int32 arg-max [num_in, F] only, and only when z wants a
    gradient. The backward adds g[r, c] into grad_z[arg[r, c], c]: on the
    GPU as one gather pass over the graph's simple CSC (no atomics), on the
    CPU as a scatter by arg.
    """

    @staticmethod
    def forward(ctx, graph: HaloGraph, z: torch.Tensor):
        need_grad = ctx.needs_input_grad[1]
        out, *arg = _spmm_max_forward(graph.csr, z, need_grad)
        if need_grad:
            ctx.save_for_backward(*arg)
        ctx.graph, ctx.num_src = graph, z.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        g = g.contiguous()
        if not g.is_cuda:
            none = torch.Tensor()
            return None, native().spmm_max_bwd(none, none, g, arg, none,
                                               ctx.num_src, g.shape[0])
        csc = ctx.graph.csc_simple()
        dz = native().spmm_max_bwd(csc.indptr, csc.indices, g, arg,
                                   _row_order(csc), csc.num_rows,
                                   csc.num_cols)
        if dz.shape[0] < ctx.num_src:  # rows the graph never references
            dz = torch.cat((dz, dz.new_zeros(ctx.num_src - dz.shape[0],
                                             dz.shape[1])))
        return None, dz


def spmm_max(graph: HaloGraph, z: torch.Tensor) -> torch.Tensor:
    """Differentiable max aggregation over the halo graph.

    z [num_all, F], fp32 or bf16; returns out [num_in, F] with out[r, c] the
    maximum of z[u, c] over the sources u of r, and 0 for a destination
    without edges. The comparison is in fp32 and the result is one of the
    inputs, so it is exact in both dtypes. The gradient of out[r, c] goes to
    the source of the first edge of r, in CSR order, that attains the
    maximum — once, however many parallel u -> r edges there are
    (docs/DESIGN.md, "Max aggregation"). NaN inputs are unspecified.
    """
    _spmm_max_check(graph.csr, z)
    return _SpmmMax.apply(graph, z)


def spmm_max_csr(csr: CSR, z: torch.Tensor, with_arg: bool = False):
    """Forward-only max aggregation over a plain CSR (full-graph eval over
    FullGraph.csr). Returns out, or (out, arg) with the int32 arg-max
    [num_rows, F]: the source id the maximum came from, -1 on rows without
    edges."""
    _spmm_max_check(csr, z)
    with torch.no_grad():
        res = _spmm_max_forward(csr, z, with_arg)
    return (res[0], res[1]) if with_arg else res[0]


def _gat_check(csr: CSR, z, el, er, num_heads: int) -> None:
    """Shape guards shared by both GAT paths; raised before any launch."""
    if num_heads < 1 or z.dim() != 2 or z.shape[1] % num_heads != 0:
        raise ValueError(
            f"gat_aggregate: feature width {tuple(z.shape)} is not "
            f"num_heads*D for num_heads={num_heads}")
    if el.dim() != 2 or er.dim() != 2 or el.shape[1] != num_heads \
            or er.shape[1] != num_heads:
        raise ValueError(
            f"gat_aggregate: el/er must be [nodes, {num_heads}], got "
            f"{tuple(el.shape)} and {tuple(er.shape)}")
    if z.shape[0] < csr.num_cols or el.shape[0] < csr.num_cols:
        raise ValueError(
            f"gat_aggregate: z/el have {z.shape[0]}/{el.shape[0]} rows but "
            f"the graph references {csr.num_cols} source nodes (an "
            "under-sized tensor would be an out-of-bounds GPU gather)")
    if er.shape[0] != csr.num_rows:
        raise ValueError(
            f"gat_aggregate: er has {er.shape[0]} rows, the graph has "
            f"{csr.num_rows} destination nodes")


_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


def _gat_dropout_params(seed: int, p: float):
    """(key, thr, scale) of one attention-dropout call, as csrc/hip/gat.hip
    derives them: key = low word of splitmix64(seed), an edge is kept when
    its hash >= thr = min(round(p * 2^32), 2^32 - 1), scale = 1 / (1 - p)."""
    x = (int(seed) + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    thr = min(int(math.floor(p * 4294967296.0 + 0.5)), _M32)
    return x & _M32, thr, 1.0 / (1.0 - p)


def _gat_keep_hash(u: torch.Tensor, v: torch.Tensor, num_heads: int,
                   key: int) -> torch.Tensor:
    """The 32-bit edge hash [n, H] as int64 values in [0, 2^32). torch's
    int64 multiply wraps, so the low 32 bits of every step are exact."""
    u = u.long() & _M32
    v = v.long() & _M32
    h = torch.arange(num_heads, dtype=torch.int64, device=u.device)
    x = ((u * 0x9E3779B1 + v * 0x85EBCA77).unsqueeze(-1)
         + h * 0xC2B2AE3D + key) & _M32
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & _M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & _M32
    return x ^ (x >> 16)


def gat_dropout_keep(u: torch.Tensor, v: torch.Tensor, num_heads: int,
                     seed: int, p: float) -> torch.Tensor:
    """Attention-dropout keep bits of the edges u[i] -> v[i]: bool [n, H].

    The bit-identical torch mirror of the device function the GAT kernels
    evaluate per edge (csrc/hip/gat.hip): a stateless 32-bit hash of (seed,
    source id u, destination id v, head), kept when it is at least
    round(p * 2^32). u and v are integer tensors of local node ids (any
    integer dtype; only the low 32 bits count, as on the device). The bit
    depends on the endpoints, not on the edge's position, so the CSR and the
    CSC pass agree on it and duplicate (u, v) edges share it. Runs on the
    tensors' device; the CPU path of `gat_aggregate` and the tests use it.
    """
    if not 0.0 <= p < 1.0:
        raise ValueError(f"gat_dropout_keep: p={p} is outside [0, 1)")
    key, thr, _ = _gat_dropout_params(seed, p)
    return _gat_keep_hash(u, v, num_heads, key) >= thr


def _attn_dropout(op: str, attn_drop: float, seed: Optional[int]):
    """(key, thr, scale) of one `op` call; (0, 0, 1.0) is no dropout. Checks
    attn_drop and, when it is positive and no seed is given, draws one from
    torch's host generator (as fused_dropout: no device sync)."""
    if not 0.0 <= attn_drop < 1.0:
        raise ValueError(f"{op}: attn_drop={attn_drop} is outside [0, 1)")
    if attn_drop == 0.0:
        return 0, 0, 1.0
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return _gat_dropout_params(seed, attn_drop)


def _edge_endpoints(csr: CSR):
    """(u, v) int64 [nnz]: source and destination of every edge, CSR order."""
    deg = csr.indptr[1:] - csr.indptr[:-1]
    v = torch.repeat_interleave(
        torch.arange(csr.num_rows, device=csr.indices.device), deg)
    return csr.indices.long(), v


def edge_drop_keep(u: torch.Tensor, v: torch.Tensor, seed: int,
                   p: float) -> torch.Tensor:
    """Edge-dropout keep bits of the edges u[i] -> v[i]: bool [n].

    The attention-dropout hash with one head, `gat_dropout_keep(u, v, 1,
    seed, p)[:, 0]`: the bit-identical torch mirror of what
    csrc/hip/spmm_drop.hip evaluates per edge. A function of (seed, u, v)
    on local node ids only, so the CSR and the CSC pass agree on it and
    duplicate (u, v) edges share it."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"edge_drop_keep: p={p} is outside [0, 1)")
    key, thr, _ = _gat_dropout_params(seed, p)
    return _gat_keep_hash(u, v, 1, key)[:, 0] >= thr


def edge_drop_args(op: str, p: float, seed: Optional[int] = None):
    """drop = (key, thr, scale) of one edge-dropout draw for `op`'s
    messages, derived as the attention dropout derives them
    (`_gat_dropout_params`); (0, 0, 1.0) keeps every edge. When p is
    positive and no seed is given, one is drawn from torch's host generator
    (no device sync); p == 0 draws nothing."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{op}: edge_drop={p} is outside [0, 1)")
    if p == 0.0:
        return 0, 0, 1.0
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return _gat_dropout_params(seed, p)


def spmm_drop(csr: CSR, feat: torch.Tensor,
              scale: Optional[torch.Tensor] = None,
              src_scale: Optional[torch.Tensor] = None, *,
              p: Optional[float] = None, seed: Optional[int] = None,
              transposed: bool = False,
              n_live: Optional[torch.Tensor] = None,
              drop=None) -> torch.Tensor:
    """`spmm(csr, feat, scale, src_scale, n_live)` over the edges an
    edge-dropout draw keeps, times 1 / (1 - p) (docs/DESIGN.md, "Edge
    dropout"). Not differentiable by itself: `spmm_mean(edge_drop=...)` and
    the GCN layer pair it with its transpose.

    The edge of row r and column c is kept when `edge_drop_keep(c, r, seed,
    p)` says so; with transposed=True (csr is a CSC: rows are sources) when
    `edge_drop_keep(r, c, seed, p)` does, so a graph's CSR and CSC drop the
    same edges for the same seed. p in [0, 1); seed defaults to one draw
    from torch's host generator when p > 0. drop = (key, thr, scale), as
    `edge_drop_args` returns it, stands in for (p, seed): a backward repeats
    its forward's draw with it.

    On the GPU a dropped edge issues no gather, and the result does not
    depend on the row order. No row-order autotune of its own: the dense
    path's cached decision for this (graph, F) if it made one, else the LPT
    order. The CPU path composes the sum from torch ops in fp32."""
    if drop is None:
        if p is None:
            raise ValueError("spmm_drop: give p (and seed) or drop")
        drop = edge_drop_args("spmm_drop", p, seed)
    key, thr, drop_scale = drop
    if feat.dim() != 2 or feat.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("spmm_drop: feat must be a fp32 or bf16 [nodes, F] "
                         f"tensor, got {tuple(feat.shape)} {feat.dtype}")
    if feat.shape[0] < csr.num_cols:
        raise ValueError(
            f"spmm_drop: feat has {feat.shape[0]} rows but the graph "
            f"references {csr.num_cols} source nodes (an under-sized feat "
            "would be an out-of-bounds GPU gather)")
    if feat.is_cuda:
        # n_live together with src_scale is refused there, as in spmm
        s = scale if scale is not None else torch.Tensor()
        ss = src_scale if src_scale is not None else torch.Tensor()
        ro = _row_order(csr)
        if getattr(csr, "_lpt_choice", {}).get(feat.shape[1]) is False:
            ro = torch.Tensor()
        return native().spmm_drop(csr.indptr, csr.indices, feat.contiguous(),
                                  s, ss, ro, csr.num_rows, transposed, key,
                                  thr, drop_scale, n_live)
    # CPU: n_live only saves the GPU kernel memory traffic
    col, row = _edge_endpoints(csr)
    u, v = (row, col) if transposed else (col, row)
    keep = _gat_keep_hash(u, v, 1, key)[:, 0] >= thr
    col, row = col[keep], row[keep]
    x = feat.float().index_select(0, col)
    if src_scale is not None:
        x = x * src_scale.float().index_select(0, col).unsqueeze(1)
    out = torch.zeros(csr.num_rows, feat.shape[1]).index_add(0, row, x)
    if scale is not None:
        out = out * scale.float().unsqueeze(1)
    return (out * drop_scale).to(feat.dtype)


def _edge_softmax_aggregate_torch(csr: CSR, u, v, score, values, drop=None):
    """The common tail of the two CPU references: softmax of score [nnz, H]
    over the edges of each destination, optional attention dropout, then
    out[v] += alpha * values [nnz, H, D]. Returns fp32 [rows, H * D]."""
    rows, num_heads = csr.num_rows, score.shape[1]
    # the row maximum is a shift only (softmax is invariant to it)
    m = torch.zeros(rows, num_heads, device=score.device).scatter_reduce(
        0, v.unsqueeze(1).expand_as(score), score.detach(), "amax",
        include_self=False)
    ex = torch.exp(score - m.index_select(0, v))
    den = torch.zeros(rows, num_heads, device=score.device).index_add(0, v, ex)
    alpha = ex / den.index_select(0, v)
    if drop is not None:
        key, thr, scale = drop
        keep = _gat_keep_hash(u, v, num_heads, key) >= thr
        alpha = alpha * (keep.to(alpha.dtype) * scale)
    out = torch.zeros(rows, num_heads, values.shape[2], device=score.device)
    out = out.index_add(0, v, alpha.unsqueeze(-1) * values)
    return out.view(rows, -1)


def _gat_aggregate_torch(csr: CSR, z, el, er, num_heads: int, slope: float,
                         drop=None):
    """Edge-softmax aggregation composed from torch ops under ordinary
    autograd: the CPU test tier and rank-0 eval. [nnz, H] temporaries are
    fine here; the GPU path never makes them. drop = (key, thr, scale)
    applies the attention-dropout mask the kernels would draw."""
    u, v = _edge_endpoints(csr)
    zf = z.float().view(z.shape[0], num_heads, -1)
    e = torch.nn.functional.leaky_relu(
        el.float().index_select(0, u) + er.float().index_select(0, v), slope)
    out = _edge_softmax_aggregate_torch(csr, u, v, e, zf.index_select(0, u),
                                        drop)
    return out.to(z.dtype)


def _gat_forward_hip(csr: CSR, z, el, er, num_heads, slope, with_aux,
                     drop=(0, 0, 1.0)):
    """row stats + aggregation on the gfx950 kernels -> (lse, out[, zc,
    csum]). Uses csr.row_order as given (no lazy autotune here). drop =
    (key, thr, scale); thr 0 is no attention dropout."""
    ro = _row_order(csr)
    lse = native().gat_row_stats(csr.indptr, csr.indices, el, er,
                                 csr.num_cols, slope)
    res = native().gat_aggregate_fwd(csr.indptr, csr.indices, z, el, er, lse,
                                     ro, csr.num_cols, num_heads, slope,
                                     with_aux, *drop)
    return (lse, *res)


class _GatAggregate(torch.autograd.Function):
    """out[v] = sum_u softmax_u(leaky_relu(el[u] + er[v])) z[u] per head.

    Saves per-node tensors only (z, el, er, lse, out and, for d_er, zc and
    csum — all emitted by the one forward gather pass); the backward is ONE
    gather pass over the CSC that recomputes alpha from them. Attention
    dropout adds three scalars (key, thr, scale) and no tensor: both passes
    recompute the keep bits from the edge endpoints.
    """

    @staticmethod
    def forward(ctx, graph: HaloGraph, z, el, er, num_heads, slope, drop):
        need_grad = any(ctx.needs_input_grad)
        lse, out, *aux = _gat_forward_hip(graph.csr, z, el, er, num_heads,
                                          slope, need_grad, drop)
        if need_grad:
            ctx.save_for_backward(z, el, er, lse, out, *aux)
        ctx.graph, ctx.num_heads, ctx.slope = graph, num_heads, slope
        ctx.drop = drop
        return out

    @staticmethod
    def backward(ctx, g):
        z, el, er, lse, out, zc, csum = ctx.saved_tensors
        csc, H = ctx.graph.csc, ctx.num_heads
        g = g.contiguous()
        n = g.shape[0]
        gh = g.view(n, H, -1).float()
        # per-node per-head dots (t, d_er): elementwise passes over
        # [num_in, F], no gather — plain torch ops
        t = (gh * out.view(n, H, -1).float()).sum(-1)
        d_er = (gh * zc.view(n, H, -1).float()).sum(-1) - t * csum
        ro = _row_order(csc)
        dz, d_el = native().gat_aggregate_bwd(
            csc.indptr, csc.indices, g, z, el, er, lse, t, ro, csc.num_cols,
            H, ctx.slope, *ctx.drop)
        if dz.shape[0] < z.shape[0]:  # rows the graph never references
            dz = torch.cat((dz, dz.new_zeros(z.shape[0] - dz.shape[0],
                                             dz.shape[1])))
            d_el = torch.cat((d_el, d_el.new_zeros(
                el.shape[0] - d_el.shape[0], H)))
        return None, dz, d_el, d_er, None, None, None


def gat_aggregate(graph: HaloGraph, z: torch.Tensor, el: torch.Tensor,
                  er: torch.Tensor, num_heads: int, slope: float = 0.2,
                  attn_drop: float = 0.0,
                  seed: Optional[int] = None) -> torch.Tensor:
    """Differentiable GAT edge-softmax aggregation over the halo graph.

    z [num_all, H*D] are the projected features of all local nodes, el
    [num_all, H] / er [num_in, H] the source/destination attention terms;
    returns out [num_in, H*D] (no bias). el/er are used in fp32 and their
    gradients come back in the incoming dtype. Nothing of size nnz is
    allocated on the GPU path, forward or backward (docs/DESIGN.md).

    attn_drop in [0, 1) drops each attention coefficient (per edge and
    head, after the softmax) with that probability and scales the kept ones
    by 1 / (1 - attn_drop). The mask is `gat_dropout_keep(u, v, num_heads,
    seed, attn_drop)` on local node ids, recomputed in both passes and never
    stored; CPU and GPU draw the same mask for the same seed. seed (0 <=
    seed < 2^62) defaults to a draw from torch's host generator, so runs are
    reproducible under torch.manual_seed; attn_drop == 0 draws nothing.
    """
    drop = _attn_dropout("gat_aggregate", attn_drop, seed)
    _gat_check(graph.csr, z, el, er, num_heads)
    if not z.is_cuda:
        return _gat_aggregate_torch(graph.csr, z, el, er, num_heads, slope,
                                    drop if drop[1] > 0 else None)
    if z.shape[0] != el.shape[0]:
        raise ValueError("gat_aggregate: z and el must cover the same nodes")
    return _GatAggregate.apply(graph, z.contiguous(),
                               el.float().contiguous(),
                               er.float().contiguous(), num_heads, slope,
                               drop)


def gat_aggregate_csr(csr: CSR, z: torch.Tensor, el: torch.Tensor,
                      er: torch.Tensor, num_heads: int,
                      slope: float = 0.2) -> torch.Tensor:
    """Forward-only edge-softmax aggregation over a plain CSR (full-graph
    eval over FullGraph.csr)."""
    _gat_check(csr, z, el, er, num_heads)
    with torch.no_grad():
        if not z.is_cuda:
            return _gat_aggregate_torch(csr, z, el, er, num_heads, slope)
        return _gat_forward_hip(csr, z.contiguous(), el.float().contiguous(),
                                er.float().contiguous(), num_heads, slope,
                                False)[1]


# widest head the lane layout of csrc/hip/gatv2.hip holds
GATV2_MAX_HEAD_DIM = 1024


def _gatv2_check(csr: CSR, zl, zr, attn, num_heads: int) -> None:
    """Shape guards shared by both GATv2 paths; raised before any launch."""
    if num_heads < 1 or zl.dim() != 2 or zl.shape[1] % num_heads != 0:
        raise ValueError(
            f"gatv2_aggregate: feature width {tuple(zl.shape)} is not "
            f"num_heads*D for num_heads={num_heads}")
    if zr.dim() != 2 or zr.shape[1] != zl.shape[1] or zr.dtype != zl.dtype:
        raise ValueError(
            f"gatv2_aggregate: zl/zr must agree in width and dtype, got "
            f"{tuple(zl.shape)} {zl.dtype} and {tuple(zr.shape)} {zr.dtype}")
    head_dim = zl.shape[1] // num_heads
    if tuple(attn.shape) != (num_heads, head_dim):
        raise ValueError(
            f"gatv2_aggregate: attn must be [{num_heads}, {head_dim}], got "
            f"{tuple(attn.shape)}")
    if zl.shape[0] < csr.num_cols:
        raise ValueError(
            f"gatv2_aggregate: zl has {zl.shape[0]} rows but the graph "
            f"references {csr.num_cols} source nodes (an under-sized tensor "
            "would be an out-of-bounds GPU gather)")
    if zr.shape[0] != csr.num_rows:
        raise ValueError(
            f"gatv2_aggregate: zr has {zr.shape[0]} rows, the graph has "
            f"{csr.num_rows} destination nodes")
    if zl.is_cuda and head_dim > GATV2_MAX_HEAD_DIM:
        raise ValueError(
            f"gatv2_aggregate: head width {head_dim} exceeds the kernels' "
            f"{GATV2_MAX_HEAD_DIM}")


def _gatv2_aggregate_torch(csr: CSR, zl, zr, attn, num_heads: int,
                           slope: float, drop=None):
    """Dynamic-attention aggregation composed from torch ops under ordinary
    autograd: the CPU test tier and rank-0 eval. [nnz, H, D] temporaries are
    fine here; the GPU path never makes them. drop = (key, thr, scale)
    applies the attention-dropout mask the kernels would draw."""
    u, v = _edge_endpoints(csr)
    zlu = zl.float().view(zl.shape[0], num_heads, -1).index_select(0, u)
    x = zlu + zr.float().view(csr.num_rows, num_heads, -1).index_select(0, v)
    s = (torch.nn.functional.leaky_relu(x, slope) * attn.float()).sum(-1)
    return _edge_softmax_aggregate_torch(csr, u, v, s, zlu, drop).to(zl.dtype)


def _gatv2_forward_hip(csr: CSR, zl, zr, attn, num_heads, slope,
                       drop=(0, 0, 1.0)):
    """One gather pass on the gfx950 kernel -> (out, lse). Uses
    csr.row_order as given. drop = (key, thr, scale); thr 0 is no attention
    dropout."""
    ro = _row_order(csr)
    return native().gatv2_fwd(csr.indptr, csr.indices, zl, zr, attn, ro,
                              csr.num_cols, num_heads, slope, *drop)


class _Gatv2Aggregate(torch.autograd.Function):
    """out[v] = sum_u softmax_u(<a, leaky_relu(zl[u] + zr[v])>) zl[u] per
    head.

    Saves per-node tensors only (zl, zr, attn, lse, out). The backward is
    two gather passes that recompute the score per edge: over the CSR for
    d_zr and the per-node pa (d_attn is its native column sum), over the CSC
    for d_zl. Attention dropout adds three scalars and no tensor.
    """

    @staticmethod
    def forward(ctx, graph: HaloGraph, zl, zr, attn, num_heads, slope, drop):
        out, lse = _gatv2_forward_hip(graph.csr, zl, zr, attn, num_heads,
                                      slope, drop)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(zl, zr, attn, lse, out)
        ctx.graph, ctx.num_heads, ctx.slope = graph, num_heads, slope
        ctx.drop = drop
        return out

    @staticmethod
    def backward(ctx, g):
        zl, zr, attn, lse, out = ctx.saved_tensors
        csr, csc, H = ctx.graph.csr, ctx.graph.csc, ctx.num_heads
        g = g.contiguous()
        n = g.shape[0]
        # per-node per-head dot: an elementwise pass over [num_in, F]
        t = (g.view(n, H, -1).float() * out.view(n, H, -1).float()).sum(-1)

        d_zr, pa = native().gatv2_bwd_dst(
            csr.indptr, csr.indices, g, zl, zr, attn, lse, t, _row_order(csr),
            csr.num_cols, H, ctx.slope, *ctx.drop)
        d_zl = native().gatv2_bwd_src(
            csc.indptr, csc.indices, g, zl, zr, attn, lse, t, _row_order(csc),
            csc.num_cols, H, ctx.slope, *ctx.drop)
        d_attn = native().colsum(pa).view_as(attn)
        if d_zl.shape[0] < zl.shape[0]:  # rows the graph never references
            d_zl = torch.cat((d_zl, d_zl.new_zeros(
                zl.shape[0] - d_zl.shape[0], d_zl.shape[1])))
        return None, d_zl, d_zr, d_attn, None, None, None


def gatv2_aggregate(graph: HaloGraph, zl: torch.Tensor, zr: torch.Tensor,
                    attn: torch.Tensor, num_heads: int, slope: float = 0.2,
                    attn_drop: float = 0.0,
                    seed: Optional[int] = None) -> torch.Tensor:
    """Differentiable GATv2 (dynamic attention) aggregation over the halo
    graph.

    zl [num_all, H*D] are the source-side projections of all local nodes, zr
    [num_in, H*D] the destination-side ones, attn [H, D] the attention
    vector; the score of edge u -> v and head h is
    <attn[h], leaky_relu(zl[u,h] + zr[v,h])>, softmaxed over the sources of
    v. Returns out [num_in, H*D] = sum_u alpha_uv zl[u] (no bias). attn is
    used in fp32 and its gradient comes back in the incoming dtype. Nothing
    of size nnz is allocated on the GPU path, forward or backward
    (docs/DESIGN.md); heads wider than GATV2_MAX_HEAD_DIM are refused there.

    attn_drop and seed are those of `gat_aggregate`: the same endpoint hash
    (`gat_dropout_keep`), applied after the softmax, recomputed in every
    pass; attn_drop == 0 draws nothing from the generator.
    """
    drop = _attn_dropout("gatv2_aggregate", attn_drop, seed)
    _gatv2_check(graph.csr, zl, zr, attn, num_heads)
    if not zl.is_cuda:
        return _gatv2_aggregate_torch(graph.csr, zl, zr, attn, num_heads,
                                      slope, drop if drop[1] > 0 else None)
    # the fp32 cast is an autograd node: d_attn returns in attn's dtype
    return _Gatv2Aggregate.apply(graph, zl.contiguous(), zr.contiguous(),
                                 attn.float().contiguous(), num_heads, slope,
                                 drop)


def gatv2_aggregate_csr(csr: CSR, zl: torch.Tensor, zr: torch.Tensor,
                        attn: torch.Tensor, num_heads: int,
                        slope: float = 0.2) -> torch.Tensor:
    """Forward-only GATv2 aggregation over a plain CSR (full-graph eval over
    FullGraph.csr); never drops."""
    _gatv2_check(csr, zl, zr, attn, num_heads)
    with torch.no_grad():
        if not zl.is_cuda:
            return _gatv2_aggregate_torch(csr, zl, zr, attn, num_heads,
                                          slope)
        return _gatv2_forward_hip(csr, zl.contiguous(), zr.contiguous(),
                                  attn.float().contiguous(), num_heads,
                                  slope)[0]


class _BiasColsum(torch.autograd.Function):
    """x + b with the bias gradient through the native colsum (see
    sage_dual_linear: torch's own reduce is pathological for thin odd N)."""

    @staticmethod
    def forward(ctx, x, b):
        return x + b

    @staticmethod
    def backward(ctx, g):
        return g, native().colsum(g.contiguous()).to(g.dtype)


def add_bias(x: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return _BiasColsum.apply(x, b)


def gather_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    return native().gather_rows(src.contiguous(), idx)


def gather_rows_into(src: torch.Tensor, idx: torch.Tensor,
                     out: torch.Tensor) -> None:
    """Gather into a persistent buffer (avoids per-epoch allocation)."""
    if src.is_cuda:
        native().gather_rows_out(src.contiguous(), idx, out)
    else:
        torch.index_select(src, 0, idx, out=out)


def scatter_add_rows(dst: torch.Tensor, idx: torch.Tensor,
                     src: torch.Tensor) -> None:
    """dst[idx[i],:] += src[i,:]; idx must be unique."""
    native().scatter_add_rows(dst, idx, src.contiguous())


def ema_update(avg: torch.Tensor, x: torch.Tensor, momentum: float) -> None:
    """avg = momentum * avg + (1 - momentum) * x (in place)."""
    if avg.dtype != torch.float32:
        avg.mul_(momentum).add_(x, alpha=1.0 - momentum)
        return
    native().ema_update(avg, x, momentum)


class _SageDualLinear(torch.autograd.Function):
    """out = x1 @ w1^T + x2 @ w2^T + (b1 + b2).

    The whole dense path is hand-written gfx950 MFMA: forward fused
    dual-GEMM (csrc/hip/dual_gemm.hip), backward fused dual-dgrad
    (dual_dgrad.hip) + fused split-M dual-wgrad (wgrad.hip) + native
    colsum bias grad; rocBLAS only on thin-N (output-layer) shapes where
    the 32-wide MFMA tiles would idle.
    """

    @staticmethod
    def forward(ctx, x1, x2, w1, w2, b1, b2):
        ctx.save_for_backward(x1, x2, w1, w2)
        ctx.has_bias = b1 is not None
        return _sage_dual_forward(x1, x2, w1, w2, b1, b2)

    @staticmethod
    def backward(ctx, g):
        x1, x2, w1, w2 = ctx.saved_tensors
        g = g.contiguous()
        gw1, gw2, gb = _sage_param_grads(g, x1, x2, w1, ctx.has_bias)
        gx1 = gx2 = None
        # an input without a gradient (layer 0: both descend from the
        # constant features) costs no dgrad
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gx1, gx2 = _sage_dgrad(g, w1, w2, ctx.needs_input_grad[0],
                                   ctx.needs_input_grad[1])
        return gx1, gx2, gw1, gw2, gb, gb


def _sage_dual_forward(x1, x2, w1, w2, b1, b2):
    if (w1.size(0) < 64 or not x1.is_cuda
            or x1.dtype != torch.float32):
        # thin-N / CPU: the 128x128 MFMA tile would waste most of the
        # block; rocBLAS pair instead (the op is memory-bound there)
        out = torch.mm(x1, w1.t())
        out.addmm_(x2, w2.t())
        if b1 is not None:
            out.add_(b1 + b2)
        return out
    bias = (b1 + b2) if b1 is not None else torch.Tensor()
    return native().sage_dual_gemm(x1.contiguous(), x2.contiguous(),
                                   w1.contiguous(), w2.contiguous(),
                                   bias)


def _sage_param_grads(g, x1, x2, w1, has_bias):
    """(gw1, gw2, gb) of the dual linear for a contiguous g; gb is None
    without a bias."""
    if g.is_cuda and g.dtype == torch.float32:
        # NOTE: running the wgrad pair on a side stream under the
        # dgrad was tried and measured WORSE (113.7 -> 114.7 ms
        # epoch): the timeline is gap-free compute, so concurrent
        # saturating kernels just share CUs plus event overhead.
        # wgrad pair fused in one MFMA split-M kernel (g streamed
        # once for both products; deterministic workspace reduce)
        gw1, gw2 = native().dual_wgrad(g, x1.contiguous(), x2.contiguous())
    else:
        gw1 = g.t() @ x1
        gw2 = g.t() @ x2
    if not has_bias:
        return gw1, gw2, None
    gb = native().colsum(g)  # two-phase column sum (fastest measured)
    return gw1, gw2, gb.to(w1.dtype)


def _mm_dgrad(g, w):
    """g @ w: the input gradient of one linear map through rocBLAS."""
    return g @ w


def _sage_dgrad(g, w1, w2, need1=True, need2=True):
    """(g @ w1, g @ w2) for a contiguous g, None where need1 / need2 says
    the gradient is not wanted. Every dgrad of the dual linear goes through
    here, and nobody calls it with neither wanted."""
    if g.is_cuda and g.dtype == torch.float32:
        if g.size(1) >= 64 and w1.size(1) <= 256:
            # dgrad pair fused in one MFMA kernel (g tile staged once
            # for both weight contractions; measured par with rocBLAS
            # at K=256 — 117 TF both; rocBLAS wins at K=512 (142 vs
            # 123 TF) and K=602 (112 vs 95), hence the cap). It computes
            # both whoever wants them.
            gx1, gx2 = native().dual_dgrad(g, w1.contiguous(),
                                           w2.contiguous())
            return (gx1 if need1 else None), (gx2 if need2 else None)
        if need1 and need2:
            # thin-N (the 41-class output layer) and wide-K (602:
            # rocBLAS 112 vs our 95 TF — the unaligned 602-float rows
            # and boundary k-tile cost us there): ONE GEMM against
            # [w1 ‖ w2] so g is still read once
            gx = _mm_dgrad(g, torch.cat((w1, w2), dim=1))
            K = w1.size(1)
            return gx[:, :K], gx[:, K:]
    return (_mm_dgrad(g, w1) if need1 else None,
            _mm_dgrad(g, w2) if need2 else None)


class _SageMeanLayer(torch.autograd.Function):
    """The mean layer's training path as one node (docs/DESIGN.md, "Fused
    layer backward"):

        feat = dropout(h, p);  ah = D^{-1} A feat
        out = feat[:num_in] @ w1^T + ah @ w2^T + (b1 + b2)

    The forward is `fused_dropout`, `spmm_mean` and `sage_dual_linear` as
    they are, in that order. The backward knows what the three separate
    nodes cannot: that the self term's gradient and the dropout mask meet the
    transpose SpMM's output element by element, so both ride in that
    kernel's epilogue, and that an input without a gradient needs no dgrad
    and no transpose at all."""

    @staticmethod
    def forward(ctx, graph: HaloGraph, h, inv_deg, w1, w2, b1, b2, p):
        mask = None
        feat = h
        if p > 0:
            # host-drawn 63-bit seed, as fused_dropout draws it
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            feat, mask = native().dropout_fwd(h.contiguous(), p, seed)
        ah = _spmm_mean_forward(graph, feat, inv_deg)
        x1 = feat[: graph.num_in]
        ctx.graph, ctx.p, ctx.has_bias = graph, p, b1 is not None
        # The two activations are intermediates of this node (neither an
        # input nor an output), kept on ctx so that the backward can let go
        # of them after the wgrad, where the dual linear's own node released
        # them: saved tensors live until the node has finished, which here is
        # after the transpose SpMM, at the step's memory peak. With p == 0,
        # x1 is a view of the input and goes the checked way.
        ctx.acts = (ah,) if mask is None else (ah, x1)
        ctx.save_for_backward(w1, w2, inv_deg, mask,
                              *((x1,) if mask is None else ()))
        return _sage_dual_forward(x1, ah, w1, w2, b1, b2)

    @staticmethod
    def backward(ctx, g):
        w1, w2, inv_deg, mask, *saved_x1 = ctx.saved_tensors
        if ctx.acts is None:
            raise RuntimeError("sage_mean_layer: its activations are freed "
                               "by the first backward; a second one through "
                               "a retained graph is not supported")
        ah, x1 = ctx.acts + tuple(saved_x1)
        ctx.acts = None
        g = g.contiguous()
        gw1, gw2, gb = _sage_param_grads(g, x1, ah, w1, ctx.has_bias)
        del ah, x1, saved_x1
        gh = None
        if ctx.needs_input_grad[1]:
            gx1, gx2 = _sage_dgrad(g, w1, w2)
            epilogue = dict(add_rows=gx1, n_add=ctx.graph.num_in)
            if mask is not None:
                epilogue.update(drop_mask=mask,
                                drop_scale=dropout_scale(ctx.p))
            gh = _spmm_mean_backward(ctx.graph, gx2, inv_deg, **epilogue)
        return None, gh, None, gw1, gw2, gb, gb, None


def sage_mean_layer(graph: HaloGraph, h: torch.Tensor,
                    inv_deg: torch.Tensor, lin1, lin2,
                    p: float = 0.0) -> torch.Tensor:
    """`sage_dual_linear(feat[:num_in], spmm_mean(graph, feat, inv_deg),
    lin1, lin2)` with `feat = fused_dropout(h, p)` (h itself when p == 0),
    as one autograd node: same forward, same host seed draw, bitwise the
    same output and gradients, a shorter backward. GPU tensors only."""
    if not h.is_cuda:
        raise ValueError("sage_mean_layer is the GPU path")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"sage_mean_layer: p={p} is outside [0, 1)")
    return _SageMeanLayer.apply(graph, h, inv_deg, lin1.weight, lin2.weight,
                                lin1.bias, lin2.bias, p)


def sage_dual_linear(x1, x2, lin1, lin2):
    """Fused linear1(x1) + linear2(x2) for the SAGE layer.

    All shapes go through _SageDualLinear so the bias grad uses the native
    colsum — torch's nn.Linear backward picks a pathological 1024-thread
    reduce for thin odd N ([2.45M,47] bias grad measured 18.7 ms vs 0.2).
    The forward dispatches thin-N / CPU to rocBLAS internally.
    """
    return _SageDualLinear.apply(x1, x2, lin1.weight, lin2.weight, lin1.bias,
                                 lin2.bias)


class _FusedDropout(torch.autograd.Function):
    """Dropout with a BITPACKED mask (1 bit/element vs torch's byte mask —
    8x less saved memory) and the scale fused into the same pass. The RNG is
    counter-based (splitmix64 keyed on a host-drawn seed), so the op is
    reproducible given torch.manual_seed. GPU path only."""

    @staticmethod
    def forward(ctx, x, p, seed):
        y, mask = native().dropout_fwd(x.contiguous(), p, seed)
        ctx.save_for_backward(mask)
        ctx.p = p
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        return native().dropout_bwd(dy, mask, ctx.p), None, None


def fused_dropout(x: torch.Tensor, p: float) -> torch.Tensor:
    """Training-mode dropout on GPU (call only when training and p > 0)."""
    # host-drawn 63-bit seed: deterministic under torch.manual_seed
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return _FusedDropout.apply(x, p, seed)


class _LayerNormReLU(torch.autograd.Function):
    """Fused LayerNorm [+ReLU] (replaces the eager nn.LayerNorm + F.relu
    pair between layers, /root/reference/module/model.py:53-56).

    Saves xhat + rstd only — eager autograd keeps {LN input, ReLU output}
    (two [N,F] tensors); this keeps one. Statistics in fp32 for both dtypes;
    the ReLU mask is recomputed in backward from w*xhat+b.
    """

    @staticmethod
    def forward(ctx, x, w, b, eps, relu):
        y, xhat, rstd = native().layer_norm_relu_fwd(
            x.contiguous(), w.contiguous(), b.contiguous(), eps, relu)
        ctx.save_for_backward(xhat, rstd, w, b)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, dy):
        xhat, rstd, w, b = ctx.saved_tensors
        dx, dw, db = native().layer_norm_relu_bwd(dy, xhat, rstd, w, b,
                                                  ctx.relu)
        return dx, dw, db, None, None


def layer_norm_relu(x: torch.Tensor, ln: torch.nn.LayerNorm,
                    relu: bool) -> torch.Tensor:
    """ln(x) [+ relu] through the fused gfx950 kernel (GPU path)."""
    # fp32 weight views keep the kernel dtype-simple; the casts are autograd
    # nodes, so bf16 params still receive their grads (no-op for fp32)
    return _LayerNormReLU.apply(x, ln.weight.float(), ln.bias.float(),
                                ln.eps, relu)


class _LinearColsum(torch.autograd.Function):
    """nn.Linear forward via rocBLAS with a colsum bias grad — torch's
    Linear backward picks a 1024-thread reduce for thin odd N (18.7 ms at
    [2.45M,47]; profiles/README.md)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        out = torch.mm(x, w.t())
        if b is not None:
            out.add_(b)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        gb = native().colsum(g).to(w.dtype)
        if g.dtype == torch.float32:
            (gw,) = native().dual_wgrad(g, x.contiguous(), torch.Tensor())
        else:
            gw = g.t() @ x
        # a first layer's input is the constant features: no dgrad
        gx = _mm_dgrad(g, w) if ctx.needs_input_grad[0] else None
        return gx, gw, gb


def linear(x, lin):
    """lin(x) with the fast bias-grad path on GPU."""
    if not x.is_cuda or lin.bias is None:
        return lin(x)
    return _LinearColsum.apply(x, lin.weight, lin.bias)
