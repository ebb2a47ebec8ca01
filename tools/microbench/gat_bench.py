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

    python tools/microbench/gat_bench.py [--shape reddit] [--feats 256]
    python tools/microbench/gat_bench.py --epoch
    python tools/microbench/gat_bench.py [--epoch] --attn-drop 0.6
`--pool` adds GraphSAGE with the max-pooling aggregator (csrc/hip/
spmm_max.hip) to the `--epoch` models, built and timed the same way.

    python tools/microbench/gat_bench.py [--epoch] --v2
    python tools/microbench/gat_bench.py --epoch --pool

`--edge-drop P` adds GraphSAGE-mean and GCN with edge dropout P (csrc/hip/
spmm_drop.hip) to the `--epoch` models, beside the same models without it.

    python tools/microbench/gat_bench.py --epoch --edge-drop 0.5
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
ap.add_argument("--pool", action="store_true",
                help="with --epoch: also time GraphSAGE with the max-pooling "
                     "aggregator")
ap.add_argument("--edge-drop", "--edge_drop", type=float, default=0.0,
                help="with --epoch: also time GraphSAGE-mean and GCN with "
                     "this edge dropout")
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


def bench(fns):
    """fns: {name: callable}. Warm each, then alternate them round by
    round; returns {name: median ms}."""
    for f in fns.values():
        f()
        f()
    samples = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, f in fns.items():
            samples[k].append(timed(f))
    return {k: statistics.median(v) for k, v in samples.items()}


def epoch_bench():
    import torch.nn.functional as Fn

    from pipegcn_amd.models.gat import GAT
    from pipegcn_amd.models.gatv2 import GATv2
    from pipegcn_amd.models.gcn import GCN
    from pipegcn_amd.models.sage import GraphSAGE
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
        if args.edge_drop > 0:
            models.append(("graphsage-edge-drop", GraphSAGE,
                           dict(use_pp=False, edge_drop=args.edge_drop), deg))
            models.append(("gcn-edge-drop", GCN,
                           dict(edge_drop=args.edge_drop), deg_all))
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
