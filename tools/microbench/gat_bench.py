"""GAT edge-softmax aggregation vs the mean-aggregation SpMM (the yardstick)
on the synthetic Reddit-shaped partition.

Per (dtype, H) at F = 256: time and logical bytes/s of gat_row_stats,
gat_aggregate_fwd (with and without the zc/csum outputs) and
gat_aggregate_bwd, then ops.gat_aggregate forward and forward+backward
against ops.spmm_mean on the same graph and F. The two compared paths
alternate inside every round of the same process; the figure reported is
the median round. One JSON line per configuration, then a table.

`--epoch` instead times whole training epochs (forward, sum loss, backward,
Adam step; hidden 256, 3 layers, dropout 0.5, one GPU) of GAT with 4 heads
against GraphSAGE and GCN built the same way, alternating model by model,
each window closed by a synchronise. The trainer's own `Time(s)` log column
closes its window before the loss is read back, so on a single GPU with no
peers it reports launch time only and cannot serve here.

`--attn-drop P` runs every GAT call with attention dropout P: the DROP
instances of the two aggregate kernels in the kernel table (row_stats and
the SpMM columns do not change), and GAT(attn_drop=P) under `--epoch`.

`--v2` adds the GATv2 kernels (csrc/hip/gatv2.hip) under the same protocol,
in the same rounds: gatv2_fwd, gatv2_bwd_dst (CSR pass), gatv2_bwd_src (CSC
pass), ops.gatv2_aggregate forward and forward+backward, and GATv2 with 4
heads under `--epoch`.

`--dot` adds the dot-product attention kernels (csrc/hip/dot_attn.hip) the
same way: dot_fwd, dot_bwd_dst (CSR pass), dot_bwd_src (CSC pass) and
ops.dot_aggregate forward and forward+backward, with kv = [K | V] of width
2F. With `--v2` its table also sets them against the GATv2 rows of the same
rounds.

    python tools/microbench/gat_bench.py [--shape reddit] [--feats 256]
    python tools/microbench/gat_bench.py --v2 --dot
    python tools/microbench/gat_bench.py --epoch
    python tools/microbench/gat_bench.py [--epoch] --attn-drop 0.6
`--pool` adds GraphSAGE with the max-pooling aggregator (csrc/hip/
spmm_max.hip) to the `--epoch` models, built and timed the same way.

    python tools/microbench/gat_bench.py [--epoch] --v2
    python tools/microbench/gat_bench.py --epoch --pool

`--edge-drop P` adds GraphSAGE-mean and GCN with edge dropout P (csrc/hip/
spmm_drop.hip) to the `--epoch` models, beside the same models without it.

    python tools/microbench/gat_bench.py --epoch --edge-drop 0.5

`--gate` times the beta gate (csrc/hip/gate.hip). Alone it times
ops.gated_residual on [num_in, F] rows, forward and forward+backward, against
the eager composition (the CPU path's formula run on the device), reports
min / median / max over the rounds and the achieved bytes/s against the
model (forward 3 N F elements; backward 3 read + 2 written), and exits. With
`--epoch` it adds the Transformer with 4 heads, without and with the gate.

    python tools/microbench/gat_bench.py --gate [--rounds 7 --iters 20]
    python tools/microbench/gat_bench.py --epoch --gate

`--bn` times the four batch-norm kernels (csrc/hip/batch_norm.hip) on
[num_in, F] rows, each against the bytes it must move, and
ops.sync_batch_norm_relu forward and forward+backward against the eager
composition (SyncBatchNorm's own forward, then relu), and exits.

    python tools/microbench/gat_bench.py --bn --shape yelp --feats 512

`--pna` times the multi-aggregation (csrc/hip/spmm_pna.hip). Alone it times
the fused forward with state against the composition it replaces (two mean
SpMMs, on x and x^2, and spmm_max with its arg on x and -x; x^2 and -x are
formed outside the window) and the three-step backward (prep, the transposed
SpMM of PQ, spmm_pna_bwd) against two transposed SpMMs plus two
spmm_max_bwd; it reports min / median / max over the rounds and logical
bytes/s from the byte count of each, and exits. With `--epoch` it adds
GraphSAGE with the pna aggregator, beside `--pool`.

    python tools/microbench/gat_bench.py --pna --feats 602 [--rounds 7]
    python tools/microbench/gat_bench.py --epoch --pool --pna

`--softmax` times the softmax aggregation (csrc/hip/spmm_softmax.hip): its
forward with state against the mean SpMM forward on the same graph and width,
and its backward against the transposed SpMM; min / median / max over the
rounds, logical bytes/s, and exits. With `--epoch` it adds GraphSAGE with the
softmax aggregator.

    python tools/microbench/gat_bench.py --softmax --feats 602 [--rounds 7]
    python tools/microbench/gat_bench.py --epoch --softmax

`--resgated` times the residual gated aggregation (csrc/hip/resgated.hip) at
F = 64, 256 and 602 (`--feats` is not read): its forward and its backward
over the CSR against the mean SpMM forward, its backward over the CSC against
the transposed SpMM, on the same graph and width; min / median / max over the
rounds, logical bytes/s, and exits. With `--epoch` it adds the ResGated model.

    python tools/microbench/gat_bench.py --resgated [--rounds 7]
    python tools/microbench/gat_bench.py --epoch --resgated
"""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import torch

from pipegcn_amd import native, ops
from pipegcn_amd.graph.halo import build_runtime_partition
from pipegcn_amd.graph.synthetic import synth_partition

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="reddit")
ap.add_argument("--feats", type=int, default=256)
ap.add_argument("--heads", type=int, nargs="+", default=[1, 4, 8])
ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--epoch", action="store_true",
                help="time whole training epochs instead of the kernels")
ap.add_argument("--attn-drop", "--attn_drop", type=float, default=0.0,
                help="attention dropout of every GAT call (default: none)")
ap.add_argument("--v2", action="store_true",
                help="also time the GATv2 kernels / model")
ap.add_argument("--dot", action="store_true",
                help="also time the dot-product attention kernels")
ap.add_argument("--pool", action="store_true",
                help="with --epoch: also time GraphSAGE with the max-pooling "
                     "aggregator")
ap.add_argument("--edge-drop", "--edge_drop", type=float, default=0.0,
                help="with --epoch: also time GraphSAGE-mean and GCN with "
                     "this edge dropout")
ap.add_argument("--gate", action="store_true",
                help="time the beta gate alone; with --epoch: the "
                     "Transformer without and with it")
ap.add_argument("--bn", action="store_true",
                help="time the fused batch-norm kernels alone")
ap.add_argument("--pna", action="store_true",
                help="time the multi-aggregation kernels against the "
                     "composition they replace; with --epoch: GraphSAGE "
                     "with the pna aggregator")
ap.add_argument("--softmax", action="store_true",
                help="time the softmax aggregation kernels against the mean "
                     "SpMM and its transpose; with --epoch: GraphSAGE with "
                     "the softmax aggregator")
ap.add_argument("--resgated", action="store_true",
                help="time the residual gated aggregation kernels at F = 64, "
                     "256 and 602 against the mean SpMM and its transpose; "
                     "with --epoch: the ResGated model")
args = ap.parse_args()
if args.pool and not args.epoch:
    ap.error("--pool times whole epochs: use it with --epoch")
if args.edge_drop and not args.epoch:
    ap.error("--edge-drop times whole epochs: use it with --epoch")
if not 0.0 <= args.edge_drop < 1.0:
    ap.error("--edge-drop must be in [0, 1)")
if not 0.0 <= args.attn_drop < 1.0:
    ap.error("--attn-drop must be in [0, 1)")

SLOPE = 0.2
dev = "cuda" if torch.cuda.is_available() else "cpu"  # cpu: --epoch dry run
torch.manual_seed(0)
part = synth_partition(args.shape, 0, 1, seed=0)
rp = build_runtime_partition(part, device=dev)
hg, csr, csc = rp.graph, rp.graph.csr, rp.graph.csc
nnz, F = csr.nnz, args.feats
inv = (1.0 / rp.ndata["in_degree"].clamp(min=1.0)).contiguous()
print(f"# {args.shape}: {rp.num_in} dst, {rp.num_all} src, {nnz} edges, "
      f"F={F}", flush=True)


def sync():
    if dev == "cuda":
        torch.cuda.synchronize()


def timed(f):
    """ms per call over one timed window that ends in a synchronise."""
    sync()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        f()
    sync()
    return (time.perf_counter() - t0) / args.iters * 1e3


def bench_rounds(fns):
    """fns: {name: callable}. Warm each, then alternate them round by
    round; returns {name: [ms of each round]}."""
    for f in fns.values():
        f()
        f()
    samples = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, f in fns.items():
            samples[k].append(timed(f))
    return samples


def bench(fns):
    """-> {name: median ms} of bench_rounds."""
    return {k: statistics.median(v) for k, v in bench_rounds(fns).items()}


def gate_bench():
    N = rp.num_in
    for dname in args.dtypes:
        dtype = torch.bfloat16 if dname == "bf16" else torch.float32
        es = 2 if dname == "bf16" else 4
        gen = torch.Generator(device=dev).manual_seed(es)
        r, m, g = (torch.randn(N, F, device=dev, generator=gen).to(dtype)
                   for _ in range(3))
        w = ((torch.rand(1, 3 * F, device=dev, generator=gen) * 2 - 1)
             / (3 * F) ** 0.5)
        rr, mr, wr = (t.clone().requires_grad_(True) for t in (r, m, w))

        def eager(r, m, w):
            w_r, w_m, w_d = w.view(3, F)
            return ops._gate_mix(r.float(), m.float(), w_r + w_d,
                                 w_m - w_d).to(dtype)

        def fwd_bwd(f):
            rr.grad = mr.grad = wr.grad = None
            f(rr, mr, wr).backward(g)

        samples = bench_rounds({
            "fused_fwd": lambda: ops.gated_residual(r, m, w),
            "eager_fwd": lambda: eager(r, m, w),
            "fused_fwd_bwd": lambda: fwd_bwd(ops.gated_residual),
            "eager_fwd_bwd": lambda: fwd_bwd(eager),
        })
        ms = {k: [round(x, 3) for x in (min(v), statistics.median(v), max(v))]
              for k, v in samples.items()}
        # the model: forward reads r, m and writes out; backward reads g, r,
        # m and writes d_r, d_m
        model = {"fused_fwd": 3 * N * F * es, "fused_fwd_bwd": 8 * N * F * es}
        print(json.dumps(dict(
            mode="gate", dtype=dname, N=N, F=F, ms_min_median_max=ms,
            model_mb={k: round(b / 1e6, 1) for k, b in model.items()},
            tb_per_s={k: round(b / ms[k][1] / 1e9, 3)
                      for k, b in model.items()})), flush=True)


def bn_bench():
    from pipegcn_amd.models.sync_bn import SyncBatchNorm

    N, nat = rp.num_in, native()
    for dname in args.dtypes:
        dtype = torch.bfloat16 if dname == "bf16" else torch.float32
        es = 2 if dname == "bf16" else 4
        gen = torch.Generator(device=dev).manual_seed(es)
        x, g = (torch.randn(N, F, device=dev, generator=gen).to(dtype)
                for _ in range(2))
        bn = SyncBatchNorm(F, N).to(dev)
        xr = x.clone().requires_grad_(True)
        sums = nat.bn_stats(x)
        mean = sums[0] / N
        std = torch.sqrt((sums[1] - mean * sums[0]) / N + bn.eps)
        w, b = bn.weight.detach(), bn.bias.detach()
        dsum = nat.bn_bwd_stats(g, x, mean, std, w, b, True)

        def fwd_bwd(f):
            xr.grad = bn.weight.grad = bn.bias.grad = None
            f(xr).backward(g)

        samples = bench_rounds({
            "bn_stats": lambda: nat.bn_stats(x),
            "bn_apply": lambda: nat.bn_apply(x, mean, std, w, b, True),
            "bn_bwd_stats": lambda: nat.bn_bwd_stats(g, x, mean, std, w, b,
                                                     True),
            "bn_bwd_apply": lambda: nat.bn_bwd_apply(g, x, mean, std, w, b,
                                                     dsum, N, True),
            "fused_fwd": lambda: ops.sync_batch_norm_relu(x, bn, True),
            "eager_fwd": lambda: torch.relu(bn(x)),
            "fused_fwd_bwd": lambda: fwd_bwd(
                lambda t: ops.sync_batch_norm_relu(t, bn, True)),
            "eager_fwd_bwd": lambda: fwd_bwd(lambda t: torch.relu(bn(t))),
        })
        ms = {k: [round(t, 3) for t in (min(v), statistics.median(v), max(v))]
              for k, v in samples.items()}
        # [N, F] passes each must make: reads + writes
        passes = {"bn_stats": 1, "bn_apply": 2, "bn_bwd_stats": 2,
                  "bn_bwd_apply": 3, "fused_fwd": 3, "fused_fwd_bwd": 8}
        model = {k: p * N * F * es for k, p in passes.items()}
        print(json.dumps(dict(
            mode="bn", dtype=dname, N=N, F=F, ms_min_median_max=ms,
            model_mb={k: round(v / 1e6, 1) for k, v in model.items()},
            tb_per_s={k: round(v / ms[k][1] / 1e9, 3)
                      for k, v in model.items()})), flush=True)


def pna_bench():
    nat, n_in, n_all = native(), rp.num_in, rp.num_all
    simple = hg.csc_simple()
    none = torch.Tensor()
    for dname in args.dtypes:
        dtype = torch.bfloat16 if dname == "bf16" else torch.float32
        es = 2 if dname == "bf16" else 4
        gen = torch.Generator(device=dev).manual_seed(es)
        x = torch.randn(n_all, F, device=dev, generator=gen).to(dtype)
        g = torch.randn(n_in, 5 * F, device=dev, generator=gen).to(dtype)
        x2, nx = x * x, -x
        gm, gs, gmax, gmin = (g[:, k * F:(k + 1) * F].contiguous()
                              for k in (1, 4, 2, 3))
        _, arg, stat = ops.spmm_pna_csr(csr, x, with_state=True)
        amax, amin = (a.contiguous() for a in arg.split(F, dim=1))

        def fused_bwd():
            pq = nat.pna_bwd_prep(csr.indptr, g, stat)
            tt = ops.spmm(csc, pq, None)
            return nat.spmm_pna_bwd(simple.indptr, simple.indices, g, arg, tt,
                                    x, ops._row_order(simple),
                                    simple.num_rows, simple.num_cols)

        def max_bwd(gk, ak):
            return nat.spmm_max_bwd(simple.indptr, simple.indices, gk, ak,
                                    ops._row_order(simple), simple.num_rows,
                                    simple.num_cols)

        samples = bench_rounds({
            "fused_fwd": lambda: ops.spmm_pna_csr(csr, x, with_state=True),
            "comp_fwd": lambda: (
                ops.spmm(csr, x, inv), ops.spmm(csr, x2, inv),
                ops.spmm_max_csr(csr, x, with_arg=True),
                ops.spmm_max_csr(csr, nx, with_arg=True)),
            "fused_bwd": fused_bwd,
            "comp_bwd": lambda: (
                ops.spmm(csc, gm, None), ops.spmm(csc, gs, None),
                max_bwd(gmax, amax), max_bwd(gmin, amin)),
        })
        ms = {k: [round(t, 3) for t in (min(v), statistics.median(v), max(v))]
              for k, v in samples.items()}
        # logical bytes: per edge the index and the gathered rows, per row
        # what is read and written once
        e2 = simple.nnz
        model = {
            "fused_fwd": nnz * (es * F + 4) + n_in * F * (6 * es + 16),
            "comp_fwd": 4 * nnz * (es * F + 4) + n_in * F * (4 * es + 8),
            "fused_bwd": (n_in * F * (2 * es + 16)
                          + nnz * (8 * F + 4) + n_all * 8 * F
                          + e2 * ((2 * es + 8) * F + 4)
                          + n_all * F * (2 * es + 8)),
            "comp_bwd": (2 * nnz * (es * F + 4)
                         + 2 * e2 * ((es + 4) * F + 4) + 4 * n_all * F * es),
        }
        print(json.dumps(dict(
            mode="pna", shape=args.shape, dtype=dname, F=F, nnz=nnz,
            nnz_simple=e2, ms_min_median_max=ms,
            fwd_ratio=round(ms["fused_fwd"][1] / ms["comp_fwd"][1], 3),
            bwd_ratio=round(ms["fused_bwd"][1] / ms["comp_bwd"][1], 3),
            model_gb={k: round(b / 1e9, 2) for k, b in model.items()},
            tb_per_s={k: round(b / ms[k][1] / 1e9, 3)
                      for k, b in model.items()})), flush=True)


def softmax_bench():
    nat, n_in, n_all = native(), rp.num_in, rp.num_all
    for dname in args.dtypes:
        dtype = torch.bfloat16 if dname == "bf16" else torch.float32
        es = 2 if dname == "bf16" else 4
        gen = torch.Generator(device=dev).manual_seed(es)
        x = torch.randn(n_all, F, device=dev, generator=gen).to(dtype)
        g = torch.randn(n_in, F, device=dev, generator=gen).to(dtype)
        beta = torch.ones(1, device=dev)
        out, lse, *o32 = nat.spmm_softmax(
            csr.indptr, csr.indices, x, beta, ops._row_order(csr),
            csr.num_rows, csr.num_cols, True)
        out32 = o32[0] if o32 else out

        samples = bench_rounds({
            "softmax_fwd": lambda: nat.spmm_softmax(
                csr.indptr, csr.indices, x, beta, ops._row_order(csr),
                csr.num_rows, csr.num_cols, True),
            "mean_fwd": lambda: ops.spmm(csr, x, inv),
            "softmax_bwd": lambda: nat.spmm_softmax_bwd(
                csc.indptr, csc.indices, g, lse, out32, x, beta,
                ops._row_order(csc), csc.num_rows, csc.num_cols),
            "mean_bwd": lambda: ops.spmm(csc, g, None),
        })
        ms = {k: [round(t, 3) for t in (min(v), statistics.median(v), max(v))]
              for k, v in samples.items()}
        # logical bytes: per edge the index and the gathered rows, per row
        # what is read and written once
        state = 4 if es == 4 else 8  # lse, and out32 at bf16
        model = {
            "softmax_fwd": nnz * (es * F + 4) + n_in * F * (es + state),
            "mean_fwd": nnz * (es * F + 4) + n_in * F * es,
            "softmax_bwd": nnz * ((es + 8) * F + 4) + 2 * n_all * F * es,
            "mean_bwd": nnz * (es * F + 4) + n_all * F * es,
        }
        print(json.dumps(dict(
            mode="softmax", shape=args.shape, dtype=dname, F=F, nnz=nnz,
            ms_min_median_max=ms,
            fwd_ratio=round(ms["softmax_fwd"][1] / ms["mean_fwd"][1], 3),
            bwd_ratio=round(ms["softmax_bwd"][1] / ms["mean_bwd"][1], 3),
            model_gb={k: round(b / 1e9, 2) for k, b in model.items()},
            tb_per_s={k: round(b / ms[k][1] / 1e9, 3)
                      for k, b in model.items()})), flush=True)


def resgated_bench():
    nat, n_in, n_all = native(), rp.num_in, rp.num_all
    for width in (64, 256, 602):
        for dname in args.dtypes:
            dtype = torch.bfloat16 if dname == "bf16" else torch.float32
            es = 2 if dname == "bf16" else 4
            gen = torch.Generator(device=dev).manual_seed(es)
            k = torch.randn(n_in, width, device=dev, generator=gen).to(dtype)
            qv = torch.randn(n_all, 2 * width, device=dev,
                             generator=gen).to(dtype)
            g = torch.randn(n_in, width, device=dev, generator=gen).to(dtype)
            x = qv[:, :width].contiguous()  # the SpMM's rows, at the same F
            csr_args = (k, qv, inv, ops._row_order(csr), csr.num_cols)
            samples = bench_rounds({
                "resgated_fwd": lambda: nat.resgated_fwd(
                    csr.indptr, csr.indices, *csr_args),
                "resgated_bwd_dst": lambda: nat.resgated_bwd_dst(
                    csr.indptr, csr.indices, g, *csr_args),
                "mean_fwd": lambda: ops.spmm(csr, x, inv),
                "resgated_bwd_src": lambda: nat.resgated_bwd_src(
                    csc.indptr, csc.indices, g, k, qv, inv,
                    ops._row_order(csc), csc.num_cols),
                "mean_bwd": lambda: ops.spmm(csc, g, None),
            })
            ms = {n: [round(t, 3)
                      for t in (min(v), statistics.median(v), max(v))]
                  for n, v in samples.items()}
            # logical bytes: per edge the index and the gathered rows, per
            # row what is read and written once
            edge2 = nnz * (2 * es * width + 4)
            model = {
                "resgated_fwd": edge2 + 2 * n_in * width * es,
                "resgated_bwd_dst": edge2 + 3 * n_in * width * es,
                "mean_fwd": nnz * (es * width + 4) + n_in * width * es,
                "resgated_bwd_src": edge2 + nnz * 4 + 4 * n_all * width * es,
                "mean_bwd": nnz * (es * width + 4) + n_all * width * es,
            }
            print(json.dumps(dict(
                mode="resgated", shape=args.shape, dtype=dname, F=width,
                nnz=nnz, ms_min_median_max=ms,
                fwd_ratio=round(ms["resgated_fwd"][1] / ms["mean_fwd"][1], 3),
                bwd_dst_ratio=round(
                    ms["resgated_bwd_dst"][1] / ms["mean_fwd"][1], 3),
                bwd_src_ratio=round(
                    ms["resgated_bwd_src"][1] / ms["mean_bwd"][1], 3),
                model_gb={n: round(b / 1e9, 2) for n, b in model.items()},
                tb_per_s={n: round(b / ms[n][1] / 1e9, 3)
                          for n, b in model.items()})), flush=True)


def epoch_bench():
    import torch.nn.functional as Fn

    from pipegcn_amd.models.gat import GAT
    from pipegcn_amd.models.gatv2 import GATv2
    from pipegcn_amd.models.gcn import GCN
    from pipegcn_amd.models.resgated import ResGated
    from pipegcn_amd.models.sage import GraphSAGE
    from pipegcn_amd.models.transformer import Transformer
    from pipegcn_amd.parallel import context as ctx
    from pipegcn_amd.trainer import (exchange_halo_values, get_layer_size)

    layer_size = get_layer_size(part.n_feat, 256, part.n_class, 3)
    labels = rp.ndata["label"][: rp.num_train]
    deg = rp.ndata["in_degree"]
    deg_all = exchange_halo_values(rp, deg)
    loss_fcn = torch.nn.CrossEntropyLoss(reduction="sum")
    for dname in args.dtypes:
        dtype = torch.bfloat16 if dname == "bf16" else torch.float32
        ctx.buffer.init_buffer(rp.num_in, rp.num_all, rp.boundary,
                               rp.recv_shape, layer_size[:3], device=dev,
                               dtype=dtype)
        feat = rp.ndata["feat"].to(dtype)
        steps = {}
        models = [("graphsage", GraphSAGE, dict(use_pp=False), deg),
                  ("gcn", GCN, {}, deg_all),
                  ("gat-4-heads", GAT,
                   dict(n_heads=4, attn_drop=args.attn_drop), None)]
        if args.v2:
            models.append(("gatv2-4-heads", GATv2,
                           dict(n_heads=4, attn_drop=args.attn_drop), None))
        if args.pool:
            models.append(("graphsage-pool", GraphSAGE,
                           dict(use_pp=False, aggregator="pool"), deg))
        if args.pna:
            models.append(("graphsage-pna", GraphSAGE,
                           dict(use_pp=False, aggregator="pna"), deg))
        if args.softmax:
            models.append(("graphsage-softmax", GraphSAGE,
                           dict(use_pp=False, aggregator="softmax"), deg))
        if args.resgated:
            models.append(("resgated", ResGated, {}, deg))
        if args.edge_drop > 0:
            models.append(("graphsage-edge-drop", GraphSAGE,
                           dict(use_pp=False, edge_drop=args.edge_drop), deg))
            models.append(("gcn-edge-drop", GCN,
                           dict(edge_drop=args.edge_drop), deg_all))
        if args.gate:
            for name, beta in (("transformer-4-heads", False),
                               ("transformer-4-heads-gate", True)):
                models.append((name, Transformer,
                               dict(n_heads=4, attn_drop=args.attn_drop,
                                    beta=beta), None))
        for name, cls, kw, d in models:
            torch.manual_seed(0)
            model = cls(layer_size, Fn.relu, dropout=0.5, norm="layer",
                        train_size=part.n_train, **kw).to(dev).to(dtype)
            opt = torch.optim.Adam(model.parameters(), lr=0.01)
            model.train()

            def step(model=model, opt=opt, d=d):
                logits = model(rp.graph, feat, d).float()
                loss = loss_fcn(logits[: rp.num_train], labels)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                ctx.buffer.next_epoch()
                opt.step()

            steps[name] = step
        ms = bench(steps)
        print(json.dumps(dict(mode="epoch", shape=args.shape, dtype=dname,
                              hidden=256, layers=3,
                              attn_drop=args.attn_drop,
                              edge_drop=args.edge_drop,
                              ms_per_epoch={k: round(v, 2)
                                            for k, v in ms.items()},
                              peak_gb=round(
                                  torch.cuda.max_memory_allocated() / 2**30,
                                  2) if dev == "cuda" else None)),
              flush=True)
        ctx.buffer.shutdown()


if args.epoch:
    import os

    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("gloo", rank=0, world_size=1)
    epoch_bench()
    dist.destroy_process_group()
    sys.exit(0)

if args.gate:
    gate_bench()
    sys.exit(0)

if args.bn:
    bn_bench()
    sys.exit(0)

if args.pna:
    pna_bench()
    sys.exit(0)

if args.softmax:
    softmax_bench()
    sys.exit(0)

if args.resgated:
    resgated_bench()
    sys.exit(0)

# (key, thr, scale) of the native entry points; (0, 0, 1.0) is no dropout
DROP_SEED = 1234
drop = (ops._gat_dropout_params(DROP_SEED, args.attn_drop)
        if args.attn_drop > 0 else (0, 0, 1.0))
rows = []
for dname in args.dtypes:
    dtype = torch.bfloat16 if dname == "bf16" else torch.float32
    es = 2 if dname == "bf16" else 4
    for H in args.heads:
        gen = torch.Generator(device=dev).manual_seed(100 * H + es)
        z = torch.randn(rp.num_all, F, device=dev, generator=gen).to(dtype)
        g = torch.randn(rp.num_in, F, device=dev, generator=gen).to(dtype)
        el = torch.randn(rp.num_all, H, device=dev, generator=gen)
        er = torch.randn(rp.num_in, H, device=dev, generator=gen)
        ro, roc = csr.row_order, csc.row_order
        nat = native()
        lse = nat.gat_row_stats(csr.indptr, csr.indices, el, er,
                                csr.num_cols, SLOPE)
        out = nat.gat_aggregate_fwd(csr.indptr, csr.indices, z, el, er, lse,
                                    ro, csr.num_cols, H, SLOPE, False)[0]
        t = (g.view(-1, H, F // H).float()
             * out.view(-1, H, F // H).float()).sum(-1)
        zr = z.clone().requires_grad_(True)
        elr = el.clone().requires_grad_(True)
        err = er.clone().requires_grad_(True)

        def gat_fb():
            zr.grad = elr.grad = err.grad = None
            ops.gat_aggregate(hg, zr, elr, err, H, SLOPE, args.attn_drop,
                              DROP_SEED).backward(g)

        def spmm_fb():
            zr.grad = None
            ops.spmm_mean(hg, zr, inv).backward(g)

        fns = {
            "row_stats": lambda: nat.gat_row_stats(
                csr.indptr, csr.indices, el, er, csr.num_cols, SLOPE),
            "agg_fwd": lambda: nat.gat_aggregate_fwd(
                csr.indptr, csr.indices, z, el, er, lse, ro, csr.num_cols, H,
                SLOPE, False, *drop),
            "agg_fwd_aux": lambda: nat.gat_aggregate_fwd(
                csr.indptr, csr.indices, z, el, er, lse, ro, csr.num_cols, H,
                SLOPE, True, *drop),
            "agg_bwd": lambda: nat.gat_aggregate_bwd(
                csc.indptr, csc.indices, g, z, el, er, lse, t, roc,
                csc.num_cols, H, SLOPE, *drop),
            "spmm_fwd": lambda: ops.spmm_mean(hg, z, inv),
            "gat_fwd": lambda: ops.gat_aggregate(
                hg, z, el, er, H, SLOPE, args.attn_drop, DROP_SEED),
            "spmm_fwd_bwd": spmm_fb,
            "gat_fwd_bwd": gat_fb,
        }
        if args.v2:
            # zl = z on all rows, zr = a second projection of the dst rows
            zr2 = torch.randn(rp.num_in, F, device=dev,
                              generator=gen).to(dtype)
            attn = torch.randn(H, F // H, device=dev,
                               generator=gen) / (F // H) ** 0.5
            out2, lse2 = nat.gatv2_fwd(csr.indptr, csr.indices, z, zr2, attn,
                                       ro, csr.num_cols, H, SLOPE)
            t2 = (g.view(-1, H, F // H).float()
                  * out2.view(-1, H, F // H).float()).sum(-1)
            zr2r = zr2.clone().requires_grad_(True)
            attnr = attn.clone().requires_grad_(True)

            def v2_fb():
                zr.grad = zr2r.grad = attnr.grad = None
                ops.gatv2_aggregate(hg, zr, zr2r, attnr, H, SLOPE,
                                    args.attn_drop, DROP_SEED).backward(g)

            fns.update({
                "v2_fwd_k": lambda: nat.gatv2_fwd(
                    csr.indptr, csr.indices, z, zr2, attn, ro, csr.num_cols,
                    H, SLOPE, *drop),
                "v2_bwd_dst": lambda: nat.gatv2_bwd_dst(
                    csr.indptr, csr.indices, g, z, zr2, attn, lse2, t2, ro,
                    csr.num_cols, H, SLOPE, *drop),
                "v2_bwd_src": lambda: nat.gatv2_bwd_src(
                    csc.indptr, csc.indices, g, z, zr2, attn, lse2, t2, roc,
                    csc.num_cols, H, SLOPE, *drop),
                "v2_fwd": lambda: ops.gatv2_aggregate(
                    hg, z, zr2, attn, H, SLOPE, args.attn_drop, DROP_SEED),
                "v2_fwd_bwd": v2_fb,
            })
        if args.dot:
            # q on the dst rows, kv = [K | V] records on all rows
            q = torch.randn(rp.num_in, F, device=dev, generator=gen).to(dtype)
            kv = torch.randn(rp.num_all, 2 * F, device=dev,
                             generator=gen).to(dtype)
            c = (F // H) ** -0.5
            agg3, lse3 = nat.dot_fwd(csr.indptr, csr.indices, q, kv, ro,
                                     csr.num_cols, H, c)
            t3 = (g.view(-1, H, F // H).float()
                  * agg3.view(-1, H, F // H).float()).sum(-1)
            qr = q.clone().requires_grad_(True)
            kvr = kv.clone().requires_grad_(True)

            def dot_fb():
                qr.grad = kvr.grad = None
                ops.dot_aggregate(hg, qr, kvr, H, None, args.attn_drop,
                                  DROP_SEED).backward(g)

            fns.update({
                "dot_fwd_k": lambda: nat.dot_fwd(
                    csr.indptr, csr.indices, q, kv, ro, csr.num_cols, H, c,
                    *drop),
                "dot_bwd_dst": lambda: nat.dot_bwd_dst(
                    csr.indptr, csr.indices, g, q, kv, lse3, t3, ro,
                    csr.num_cols, H, c, *drop),
                "dot_bwd_src": lambda: nat.dot_bwd_src(
                    csc.indptr, csc.indices, g, q, kv, lse3, t3, roc,
                    csc.num_cols, H, c, *drop),
                "dot_fwd": lambda: ops.dot_aggregate(
                    hg, q, kv, H, None, args.attn_drop, DROP_SEED),
                "dot_fwd_bwd": dot_fb,
            })
        ms = bench(fns)
        # logical bytes per edge: index + gathered row (+ per-head scalars);
        # the bwd gathers one packed 16 B (er, lse, t, 0) per edge and head
        per_edge = {"row_stats": 4 + 4 * H, "agg_fwd": es * F + 4 * H + 4,
                    "agg_fwd_aux": es * F + 4 * H + 4,
                    "agg_bwd": es * F + 16 * H + 4, "spmm_fwd": es * F + 4}
        if args.v2:
            # the CSC pass gathers two rows (g, zr) and 8 B (lse, t) per head
            per_edge.update({"v2_fwd_k": es * F + 4, "v2_bwd_dst": es * F + 4,
                             "v2_bwd_src": 2 * es * F + 8 * H + 4})
        if args.dot:
            # both CSR passes gather the 2F record; the CSC pass two rows
            # (q, g) and 8 B (lse, t) per head
            per_edge.update({"dot_fwd_k": 2 * es * F + 4,
                             "dot_bwd_dst": 2 * es * F + 4,
                             "dot_bwd_src": 2 * es * F + 8 * H + 4})
        rec = dict(dtype=dname, H=H, F=F, nnz=nnz, attn_drop=args.attn_drop,
                   ms={k: round(v, 3) for k, v in ms.items()},
                   tb_per_s={k: round(nnz * b / ms[k] / 1e9, 3)
                             for k, b in per_edge.items()},
                   fwd_ratio=round(ms["gat_fwd"] / ms["spmm_fwd"], 3),
                   fwd_bwd_ratio=round(ms["gat_fwd_bwd"]
                                       / ms["spmm_fwd_bwd"], 3))
        if args.v2:
            rec["v2_fwd_ratio"] = round(ms["v2_fwd"] / ms["spmm_fwd"], 3)
            rec["v2_fwd_bwd_ratio"] = round(ms["v2_fwd_bwd"]
                                            / ms["spmm_fwd_bwd"], 3)
        if args.dot:
            rec["dot_fwd_ratio"] = round(ms["dot_fwd"] / ms["spmm_fwd"], 3)
            rec["dot_fwd_bwd_ratio"] = round(ms["dot_fwd_bwd"]
                                             / ms["spmm_fwd_bwd"], 3)
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        del z, g, el, er, zr, elr, err, out, lse, t

print("\n| dtype | H | row_stats | agg_fwd | agg_fwd+aux | agg_bwd | "
      "spmm fwd | gat fwd | ratio | spmm f+b | gat f+b | ratio |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|")
for r in rows:
    m = r["ms"]
    print(f"| {r['dtype']} | {r['H']} | {m['row_stats']:.2f} | "
          f"{m['agg_fwd']:.2f} | {m['agg_fwd_aux']:.2f} | "
          f"{m['agg_bwd']:.2f} | {m['spmm_fwd']:.2f} | {m['gat_fwd']:.2f} | "
          f"{r['fwd_ratio']:.2f} | {m['spmm_fwd_bwd']:.2f} | "
          f"{m['gat_fwd_bwd']:.2f} | {r['fwd_bwd_ratio']:.2f} |")

if args.v2:
    print("\n| dtype | H | v2 fwd kernel | v2 bwd dst (CSR) | v2 bwd src (CSC)"
          " | v2 fwd | / spmm | / gat | v2 f+b | / spmm | / gat |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        m = r["ms"]
        print(f"| {r['dtype']} | {r['H']} | {m['v2_fwd_k']:.2f} | "
              f"{m['v2_bwd_dst']:.2f} | {m['v2_bwd_src']:.2f} | "
              f"{m['v2_fwd']:.2f} | {r['v2_fwd_ratio']:.2f} | "
              f"{m['v2_fwd'] / m['gat_fwd']:.2f} | {m['v2_fwd_bwd']:.2f} | "
              f"{r['v2_fwd_bwd_ratio']:.2f} | "
              f"{m['v2_fwd_bwd'] / m['gat_fwd_bwd']:.2f} |")

if args.dot:
    v2 = " / v2 |" if args.v2 else ""
    print("\n| dtype | H | dot fwd kernel | dot bwd dst (CSR) | dot bwd src "
          "(CSC) | dot fwd | / spmm |" + v2 + " dot f+b | / spmm |" + v2)
    print("|---|---|---|---|---|---|---|---|---|" + ("---|---|" if args.v2
                                                      else ""))
    for r in rows:
        m = r["ms"]
        f_v2 = f" {m['dot_fwd'] / m['v2_fwd']:.2f} |" if args.v2 else ""
        fb_v2 = (f" {m['dot_fwd_bwd'] / m['v2_fwd_bwd']:.2f} |"
                 if args.v2 else "")
        print(f"| {r['dtype']} | {r['H']} | {m['dot_fwd_k']:.2f} | "
              f"{m['dot_bwd_dst']:.2f} | {m['dot_bwd_src']:.2f} | "
              f"{m['dot_fwd']:.2f} | {r['dot_fwd_ratio']:.2f} |" + f_v2
              + f" {m['dot_fwd_bwd']:.2f} | {r['dot_fwd_bwd_ratio']:.2f} |"
              + fb_v2)
