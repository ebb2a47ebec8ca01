"""A/B microbenchmark for the SpMM lane widths (PIPEGCN_SPMM_VEC) on a
Reddit-shaped graph.

Interleaved within-process rounds (guide §5.4 rule 24): widths alternate so
run-to-run variance is correlated. Reports ms and effective (logical) GB/s =
edges * F * 4 / t.

With --density it instead compares the packed-row forward path with the
dense kernel on features of which only that share is non-zero (what dropout
and ReLU leave): dense SpMM, pack pass and packed SpMM alternate in the same
rounds, and the two outputs must be bitwise equal.

With --dead-frac it compares the dense kernel with and without the dead-row
redirect (the last layer's backward) on features whose trailing share of rows
is all zero: the pre-scale pass that counts the live rows, the plain kernel
and the redirecting one alternate in the same rounds, and the two outputs
must be bitwise equal.

With --max it compares the max aggregation (csrc/hip/spmm_max.hip) with the
mean SpMM on the same graph, fp32 and bf16: max forward with and without the
arg-max output, max backward over the duplicate-free CSC, dense mean forward
and its transpose alternate in the same rounds.

With --edge-drop it compares the masked kernel of edge dropout
(csrc/hip/spmm_drop.hip) with the plain dense kernel, forward and transpose,
at each rate and with every edge kept, alternating in the same rounds.

With --epilogue it compares the transpose SpMM with and without the add /
dropout epilogue of the fused layer backward, and times the eager accumulate
and dropout_bwd passes the epilogue replaces.

Usage (on a GPU box):
    python -m pipegcn_amd.tools.spmm_bench --f 256 --epilogue
    python -m pipegcn_amd.tools.spmm_bench --f 256 --edge-drop 0.2 0.5 0.8
    python -m pipegcn_amd.tools.spmm_bench [--f 602 256] [--rounds 5]
    python -m pipegcn_amd.tools.spmm_bench --f 256 --density 0.25 0.5 1.0
    python -m pipegcn_amd.tools.spmm_bench --f 256 --dead-frac 0 0.34 0.92
    python -m pipegcn_amd.tools.spmm_bench --max
"""
import argparse
import os
import time

import torch


def build(n=232_965, avg_deg=492, seed=0):
    from pipegcn_amd.graph.csr import HaloGraph
    g = torch.Generator().manual_seed(seed)
    d = torch.exp(torch.randn(n, generator=g)).clamp(min=0.1)
    deg = (d / d.mean() * avg_deg).round().long().clamp(min=1)
    v = torch.repeat_interleave(torch.arange(n), deg)
    u = (torch.rand(v.numel(), generator=g) * n).long()
    return HaloGraph.from_edges(u, v, n, n).to("cuda"), int(v.numel())


def density_table(hg, E, inv, widths, densities, rounds, iters):
    """Dense SpMM, pack pass and packed SpMM on features with the share
    `density` of non-zeros, alternating in the same rounds. Prints best ms
    and physical bytes per edge (dense: the row; packed: header plus the
    mean non-zero payload), and checks the two outputs bitwise."""
    from pipegcn_amd import native, ops

    n = hg.num_all
    csr = hg.csr
    ro = csr.row_order
    s = inv
    print("    F  density |  dense ms  B/edge |  pack ms | packed ms  B/edge"
          " | packed+pack vs dense")
    for F in widths:
        W, _, stride = ops.packed_row_layout(F)
        for d in densities:
            g = torch.Generator(device="cuda").manual_seed(F)
            feat = torch.randn(n, F, device="cuda", generator=g)
            feat *= torch.rand(n, F, device="cuda", generator=g) < d
            packed = native().pack_rows(feat)
            nnz = int((feat != 0).sum())

            def dense():
                return native().spmm(csr.indptr, csr.indices, feat, s,
                                     torch.Tensor(), ro, csr.num_rows)

            def pack():
                return native().pack_rows(feat)

            def gather():
                return native().spmm_packed(csr.indptr, csr.indices, packed,
                                            F, s, ro, csr.num_rows)

            assert torch.equal(dense().view(torch.int32),
                               gather().view(torch.int32)), \
                f"F={F} density={d}: packed SpMM differs from dense"
            best = {}
            for _ in range(rounds):
                for name, fn in (("dense", dense), ("pack", pack),
                                 ("packed", gather)):
                    fn()
                    torch.cuda.synchronize()
                    t0 = time.time()
                    for _ in range(iters):
                        fn()
                    torch.cuda.synchronize()
                    t = (time.time() - t0) / iters * 1e3
                    best[name] = min(best.get(name, t), t)
            b_dense = 4 * F
            b_packed = 8 * W + 4 * nnz / n
            print(f"{F:5d}  {d:7.2f} | {best['dense']:9.2f}  {b_dense:6d} |"
                  f" {best['pack']:8.3f} | {best['packed']:9.2f} "
                  f"{b_packed:7.0f} | "
                  f"{(best['packed'] + best['pack']) / best['dense']:.3f}x")
            del feat, packed


def dead_rows_table(hg, inv, widths, fracs, dtype, rounds, iters):
    """The dense kernel without and with the dead-row redirect on features
    whose last `frac` of the rows is zero, alternating in the same rounds
    with the eager row scale and the fused scale-and-count pass that feeds
    the redirect. Prints best ms and checks the two outputs bitwise."""
    from pipegcn_amd import native

    n = hg.num_all
    csr = hg.csr
    ro = csr.row_order
    none = torch.Tensor()
    print("    F  dead | n_live  | eager scale ms | scale+count ms |"
          " plain ms | redirect ms | redirect vs plain")
    for F in widths:
        for frac in fracs:
            g = torch.Generator(device="cuda").manual_seed(F)
            feat = torch.randn(n, F, device="cuda", generator=g).to(dtype)
            feat[n - int(round(frac * n)):] = 0
            scaled, n_live = native().scale_rows_live(feat, inv)
            assert torch.equal(
                scaled.view(torch.int16 if dtype == torch.bfloat16
                            else torch.int32),
                (feat * inv.unsqueeze(1).to(dtype)).view(
                    torch.int16 if dtype == torch.bfloat16
                    else torch.int32)), \
                f"F={F}: fused row scale differs from the eager product"

            def eager():
                return feat * inv.unsqueeze(1).to(dtype)

            def fused():
                return native().scale_rows_live(feat, inv)

            def plain():
                return native().spmm(csr.indptr, csr.indices, scaled, none,
                                     none, ro, csr.num_rows)

            def redirect():
                return native().spmm(csr.indptr, csr.indices, scaled, none,
                                     none, ro, csr.num_rows, n_live)

            assert torch.equal(plain().view(torch.uint8),
                               redirect().view(torch.uint8)), \
                f"F={F} dead={frac}: redirecting SpMM differs from plain"
            best = {}
            for _ in range(rounds):
                for name, fn in (("eager", eager), ("fused", fused),
                                 ("plain", plain), ("redirect", redirect)):
                    fn()
                    torch.cuda.synchronize()
                    t0 = time.time()
                    for _ in range(iters):
                        fn()
                    torch.cuda.synchronize()
                    t = (time.time() - t0) / iters * 1e3
                    best[name] = min(best.get(name, t), t)
            print(f"{F:5d}  {frac:4.2f} | {int(n_live):7d} |"
                  f" {best['eager']:14.3f} | {best['fused']:14.3f} |"
                  f" {best['plain']:8.2f} | {best['redirect']:11.2f} |"
                  f" {best['redirect'] / best['plain']:.3f}x", flush=True)
            del feat, scaled


def max_table(hg, E, widths, rounds, iters):
    """The max aggregation against the mean SpMM at the same shape, fp32 and
    bf16: max forward with arg, max forward without, max backward (over the
    simple CSC), dense mean forward and its transpose, alternating in the
    same rounds after warm-up. Prints best ms, the ratios and logical TB/s
    computed from shapes: per edge the index and one gathered row (the max
    backward: two, g at the element size and arg at 4 bytes), per output
    element one store (the max forward with arg: two)."""
    from pipegcn_amd import native

    n = hg.num_all
    csr, csc, simple = hg.csr, hg.csc, hg.csc_simple()
    none = torch.Tensor()
    print(f"simple CSC: {simple.nnz} of {csc.nnz} entries")
    print("dtype     F | max fwd+arg | max fwd | max bwd | mean fwd | mean T |"
          " fwd+arg/mean  fwd/mean  bwd/T | logical TB/s: fwd+arg  fwd  bwd"
          "  mean fwd  mean T")
    for dname, dtype, es in (("fp32", torch.float32, 4),
                             ("bf16", torch.bfloat16, 2)):
        for F in widths:
            gen = torch.Generator(device="cuda").manual_seed(F)
            z = torch.randn(n, F, device="cuda", generator=gen).to(dtype)
            g = torch.randn(hg.num_in, F, device="cuda",
                            generator=gen).to(dtype)
            arg = native().spmm_max(csr.indptr, csr.indices, z, csr.row_order,
                                    csr.num_rows, csr.num_cols, True)[1]
            fns = {
                "fwd_arg": lambda: native().spmm_max(
                    csr.indptr, csr.indices, z, csr.row_order, csr.num_rows,
                    csr.num_cols, True),
                "fwd": lambda: native().spmm_max(
                    csr.indptr, csr.indices, z, csr.row_order, csr.num_rows,
                    csr.num_cols, False),
                "bwd": lambda: native().spmm_max_bwd(
                    simple.indptr, simple.indices, g, arg, simple.row_order,
                    simple.num_rows, simple.num_cols),
                "mean": lambda: native().spmm(
                    csr.indptr, csr.indices, z, none, none, csr.row_order,
                    csr.num_rows),
                "mean_t": lambda: native().spmm(
                    csc.indptr, csc.indices, g, none, none, csc.row_order,
                    csc.num_rows),
            }
            for fn in fns.values():
                fn()
                fn()
            best = {}
            for _ in range(rounds):
                for name, fn in fns.items():
                    torch.cuda.synchronize()
                    t0 = time.time()
                    for _ in range(iters):
                        fn()
                    torch.cuda.synchronize()
                    t = (time.time() - t0) / iters * 1e3
                    best[name] = min(best.get(name, t), t)
            rows_out = hg.num_in * F
            logical = {
                "fwd_arg": csr.nnz * (es * F + 4) + rows_out * (es + 4),
                "fwd": csr.nnz * (es * F + 4) + rows_out * es,
                "bwd": simple.nnz * ((es + 4) * F + 4) + n * F * es,
                "mean": csr.nnz * (es * F + 4) + rows_out * es,
                "mean_t": csc.nnz * (es * F + 4) + n * F * es,
            }
            tbs = {k: logical[k] / best[k] / 1e9 for k in best}
            print(f"{dname} {F:6d} | {best['fwd_arg']:11.2f} |"
                  f" {best['fwd']:7.2f} | {best['bwd']:7.2f} |"
                  f" {best['mean']:8.2f} | {best['mean_t']:6.2f} |"
                  f" {best['fwd_arg'] / best['mean']:12.3f}x"
                  f" {best['fwd'] / best['mean']:8.3f}x"
                  f" {best['bwd'] / best['mean_t']:5.3f}x |"
                  f" {tbs['fwd_arg']:21.2f} {tbs['fwd']:5.2f}"
                  f" {tbs['bwd']:5.2f} {tbs['mean']:8.2f}"
                  f" {tbs['mean_t']:7.2f}", flush=True)
            del z, g, arg


def edge_drop_table(hg, inv, widths, rates, dtype, rounds, iters):
    """The masked kernel (csrc/hip/spmm_drop.hip) against the plain dense
    one on the same graph and input: forward over the CSR and transpose over
    the CSC, for each rate p and for "keep-all" (the masked kernel with thr =
    0: every edge kept, so the pure cost of the hash and the queue). All
    variants of one width alternate in the same rounds after warm-up. fp32
    also times the packed forward (pack pass + packed gather) on inputs with
    one half and one quarter of non-zeros, the path --edge-drop gives up.
    Prints best ms with the median in brackets."""
    from pipegcn_amd import native, ops

    n = hg.num_all
    csr, csc = hg.csr, hg.csc
    none = torch.Tensor()
    fp32 = dtype == torch.float32

    def masked(m, x, s, transposed, drop):
        return native().spmm_drop(m.indptr, m.indices, x, s, none,
                                  m.row_order, m.num_rows, transposed, *drop)

    for F in widths:
        gen = torch.Generator(device="cuda").manual_seed(F)
        z = torch.randn(n, F, device="cuda", generator=gen).to(dtype)
        g = torch.randn(hg.num_in, F, device="cuda", generator=gen).to(dtype)
        fns = {
            ("plain", "fwd"): lambda: native().spmm(
                csr.indptr, csr.indices, z, inv, none, csr.row_order,
                csr.num_rows),
            ("plain", "T"): lambda: native().spmm(
                csc.indptr, csc.indices, g, none, none, csc.row_order,
                csc.num_rows),
        }
        drops = {"keep-all": (0, 0, 1.0)}
        for p in rates:
            drops[f"{p:g}"] = ops.edge_drop_args("spmm_bench", p, 1234)
        for name, drop in drops.items():
            fns[(name, "fwd")] = \
                lambda drop=drop: masked(csr, z, inv, False, drop)
            fns[(name, "T")] = \
                lambda drop=drop: masked(csc, g, none, True, drop)
        # keeping everything is the plain product up to summation order
        ref = fns[("plain", "fwd")]().float()
        err = (fns[("keep-all", "fwd")]().float() - ref).abs().max()
        assert err <= 1e-2 * ref.abs().max(), f"F={F}: keep-all differs"
        del ref
        if fp32:
            for d in (0.5, 0.25):
                zd = z * (torch.rand(n, F, device="cuda", generator=gen) < d)
                fns[(f"packed d={d:g}", "fwd")] = \
                    lambda zd=zd: native().spmm_packed(
                        csr.indptr, csr.indices, native().pack_rows(zd), F,
                        inv, csr.row_order, csr.num_rows)
        for fn in fns.values():
            fn()
            fn()
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.time()
                for _ in range(iters):
                    fn()
                torch.cuda.synchronize()
                times[k].append((time.time() - t0) / iters * 1e3)
        best = {k: min(t) for k, t in times.items()}
        med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
        dname = "fp32" if fp32 else "bf16"
        print(f"{dname} F={F}: best ms [median] over {rounds} rounds of "
              f"{iters}")
        print("  variant         |       forward      vs plain |"
              "      transpose     vs plain")
        for name in ["plain"] + list(drops):
            f, t = (name, "fwd"), (name, "T")
            print(f"  {name:15s} | {best[f]:8.2f} [{med[f]:7.2f}]"
                  f"  {best[f] / best[('plain', 'fwd')]:6.3f}x |"
                  f" {best[t]:8.2f} [{med[t]:7.2f}]"
                  f"  {best[t] / best[('plain', 'T')]:6.3f}x", flush=True)
        for k in fns:
            if k[0].startswith("packed"):
                print(f"  {k[0]:15s} | {best[k]:8.2f} [{med[k]:7.2f}]"
                      f"  {best[k] / best[('plain', 'fwd')]:6.3f}x |"
                      "  (pack pass + packed gather)", flush=True)
        del z, g, fns


def epilogue_table(hg, widths, dtype, rounds, iters):
    """The transpose SpMM of the layer backward, plain and with the add /
    dropout epilogue, alternating in the same rounds with the two eager
    passes the epilogue replaces (accumulate, dropout_bwd). Prints best ms
    and checks the fused output bitwise against the three separate steps."""
    from pipegcn_amd import native, ops

    n = hg.num_all
    csc = hg.csc
    none = torch.Tensor()
    scale = ops.dropout_scale(0.5)
    print("    F | plain ms | epilogue ms | add + dropout_bwd ms |"
          " epilogue - plain")
    for F in widths:
        g = torch.Generator(device="cuda").manual_seed(F)
        feat = torch.randn(n, F, device="cuda", generator=g).to(dtype)
        wide = torch.randn(n, 2 * F, device="cuda", generator=g).to(dtype)
        add = wide[:, :F]  # as the cat-GEMM hands it over
        _, mask = native().dropout_fwd(feat, 0.5, 1)

        def plain():
            return native().spmm(csc.indptr, csc.indices, feat, none, none,
                                 csc.row_order, csc.num_rows)

        def fused():
            return native().spmm(csc.indptr, csc.indices, feat, none, none,
                                 csc.row_order, csc.num_rows, None, add, n,
                                 mask, scale)

        base = plain()

        def tail():
            return native().dropout_bwd(base + add, mask, 0.5)

        assert torch.equal(fused().view(torch.uint8),
                           tail().view(torch.uint8)), \
            f"F={F}: the epilogue differs from add + dropout_bwd"
        best = {}
        for _ in range(rounds):
            for name, fn in (("plain", plain), ("fused", fused),
                             ("tail", tail)):
                fn()
                torch.cuda.synchronize()
                t0 = time.time()
                for _ in range(iters):
                    fn()
                torch.cuda.synchronize()
                t = (time.time() - t0) / iters * 1e3
                best[name] = min(best.get(name, t), t)
        print(f"{F:5d} | {best['plain']:8.2f} | {best['fused']:11.2f} |"
              f" {best['tail']:20.3f} |"
              f" {best['fused'] - best['plain']:+.3f}", flush=True)
        del feat, wide, add, base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--f", type=int, nargs="+", default=[602, 256])
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--nodes", type=int, default=232_965)
    ap.add_argument("--deg", type=int, default=492)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--density", type=float, nargs="+", default=None,
                    metavar="D",
                    help="instead of the lane-width A/B: for each F and "
                         "each share D of non-zero features, time the "
                         "dense SpMM, the pack pass and the packed SpMM "
                         "(fp32)")
    ap.add_argument("--dead-frac", type=float, nargs="+", default=None,
                    metavar="S",
                    help="instead of the lane-width A/B: for each F and "
                         "each share S of trailing all-zero rows, time the "
                         "dense SpMM without and with the dead-row redirect, "
                         "and the row scale that counts the live rows")
    ap.add_argument("--max", action="store_true",
                    help="instead of the lane-width A/B: the max "
                         "aggregation (forward with and without arg, "
                         "backward) against the mean SpMM and its transpose, "
                         "fp32 and bf16, at --f (default 64 256 602)")
    ap.add_argument("--edge-drop", type=float, nargs="+", default=None,
                    metavar="P",
                    help="instead of the lane-width A/B: for each F and "
                         "each edge-dropout rate P, and for a keep-all run "
                         "of the masked kernel, time the masked forward and "
                         "transpose against the plain dense kernel (--dtype "
                         "as given; fp32 adds the packed forward)")
    ap.add_argument("--epilogue", action="store_true",
                    help="instead of the lane-width A/B: the transpose SpMM "
                         "plain and with the add / dropout epilogue of the "
                         "fused layer backward, and the two eager passes it "
                         "replaces")
    args = ap.parse_args()

    from pipegcn_amd import ops

    hg, E = build(args.nodes, args.deg)
    n = hg.num_in
    deg = hg.csr.row_degrees().to("cuda").clamp(min=1)
    inv = (1.0 / deg).contiguous()
    print(f"graph: {n} nodes, {E} edges")
    if args.epilogue:
        epilogue_table(hg, args.f, torch.bfloat16 if args.dtype == "bf16"
                       else torch.float32, args.rounds, args.iters)
        return
    if args.max:
        widths = args.f if args.f != ap.get_default("f") else [64, 256, 602]
        max_table(hg, E, widths, args.rounds, args.iters)
        return
    if args.edge_drop:
        edge_drop_table(hg, inv, args.f, args.edge_drop,
                        torch.bfloat16 if args.dtype == "bf16"
                        else torch.float32, args.rounds, args.iters)
        return
    if args.density:
        if args.dtype != "fp32":
            raise SystemExit("--density: the packed path is fp32 only")
        density_table(hg, E, inv, args.f, args.density, args.rounds,
                      args.iters)
        return

    if args.dead_frac:
        dead_rows_table(hg, inv, args.f, args.dead_frac,
                        torch.bfloat16 if args.dtype == "bf16"
                        else torch.float32, args.rounds, args.iters)
        return

    elem = 2 if args.dtype == "bf16" else 4
    for F in args.f:
        feat = torch.randn(n, F, device="cuda")
        if args.dtype == "bf16":
            feat = feat.to(torch.bfloat16)
        variants = [vec for vec in (8, 4, 2, 1)
                    if F % vec == 0 and vec * elem <= 16]
        results = {v: [] for v in variants}
        ref = None
        for rnd in range(args.rounds):
            for vec in variants:
                os.environ["PIPEGCN_SPMM_VEC"] = str(vec)
                out = ops.spmm(hg.csr, feat, inv)  # warm + correctness
                if ref is None:
                    ref = out.clone()
                else:
                    assert torch.allclose(out.float(), ref.float(),
                                          atol=1e-4), \
                        f"variant VEC={vec} WRONG"
                torch.cuda.synchronize()
                t0 = time.time()
                for _ in range(args.iters):
                    ops.spmm(hg.csr, feat, inv)
                torch.cuda.synchronize()
                results[vec].append((time.time() - t0) / args.iters)
        print(f"F={F}:")
        for vec, ts in results.items():
            ms = min(ts) * 1e3
            gbs = E * F * elem / min(ts) / 1e9
            print(f"  VEC={vec}: {ms:8.2f} ms  {gbs:8.0f} GB/s logical")
        os.environ.pop("PIPEGCN_SPMM_VEC")


if __name__ == "__main__":
    main()
