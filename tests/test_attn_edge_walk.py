"""Every case of the attention kernels' edge walk (for_edges, attn_util.h):
peel until the cursor is 4-aligned, groups of four indices from one dwordx4,
then the tail.

The graph of tests/test_gat_ops.py has one long row at one alignment. This one
holds, for every start alignment e_begin % 4 in 0..3, a row of every degree
0..11: each combination of 0-3 peeled edges, 0-2 full groups and 0-3 tail
edges. It is built from a degree list, with a filler row of 1-3 edges wherever
the cursor has to move to the wanted alignment. Sources get the SAME degree
list (the edge stubs of both sides are paired by a seeded permutation, so
duplicate edges occur), so the CSC that the transpose passes walk covers the
same cases.

Nothing is compared here that the files of the two ops do not already
compare: their float64 references, yardsticks, tolerances and checks run
unchanged, pointed at this graph. Their cached cases belong to their own
graph and are left alone.
"""
import functools
import itertools

import pytest
import torch

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import HaloGraph
from tests import test_gat_dropout, test_gat_ops, test_gatv2_ops

ALIGNMENTS, DEGREES = range(4), range(12)
DROP_P = 0.5
# GAT: 4 elements per lane at fp32, 8 at bf16 (forward without zc/csum)
GAT_SHAPE = (2, 8)
# GATv2: four edges in flight (1 element per lane) | two (8 per lane); one is
# test_gatv2_ops.LAYOUT_SHAPES'
GATV2_SHAPES = [(2, 8), (1, 512)]


@functools.lru_cache(maxsize=None)
def degree_list():
    """Row degrees in row order, and the rows that are there for their
    (alignment, degree)."""
    degs, wanted, e = [], {}, 0
    for a, d in itertools.product(ALIGNMENTS, DEGREES):
        if e % 4 != a:
            fill = (a - e) % 4
            degs.append(fill)
            e += fill
        wanted[len(degs)] = (a, d)
        degs.append(d)
        e += d
    return degs, wanted


@functools.lru_cache(maxsize=None)
def walk_edges():
    degs, _ = degree_list()
    stubs = torch.repeat_interleave(torch.arange(len(degs)),
                                    torch.tensor(degs))
    perm = torch.randperm(stubs.numel(),
                          generator=torch.Generator().manual_seed(0))
    return stubs[perm], stubs  # u, v: both sides have the degree list


@functools.lru_cache(maxsize=None)
def walk_graph(device):
    u, v = walk_edges()
    n = len(degree_list()[0])
    return HaloGraph.from_edges(u, v, n, n).to(device)


def test_edge_walk_graph_covers_every_case():
    degs, wanted = degree_list()
    hg = walk_graph("cpu")
    every = set(itertools.product(ALIGNMENTS, DEGREES))
    for m in (hg.csr, hg.csc):
        assert m.num_rows == len(degs)
        deg = m.indptr[1:] - m.indptr[:-1]
        assert deg.tolist() == degs
        for r, (a, d) in wanted.items():
            assert (int(m.indptr[r]) % 4, int(deg[r])) == (a, d)
        got = {(int(m.indptr[r]) % 4, int(deg[r])) for r in range(m.num_rows)}
        assert every <= got
    u, v = walk_edges()
    pairs = torch.stack((u, v)).unique(dim=1).shape[1]
    assert pairs < u.numel(), "no duplicate edge"


@pytest.fixture
def on_walk_graph(monkeypatch):
    """Point the graph, its sizes and its empty rows in the three op test
    files at the walk graph, and go round their per-shape caches."""
    degs, _ = degree_list()
    empty = tuple(r for r, d in enumerate(degs) if d == 0)
    for mod in (test_gat_ops, test_gat_dropout, test_gatv2_ops):
        monkeypatch.setattr(mod, "edges", walk_edges)
        monkeypatch.setattr(mod, "graph", walk_graph)
        monkeypatch.setattr(mod, "N_SRC", len(degs))
        monkeypatch.setattr(mod, "N_DST", len(degs))
        monkeypatch.setattr(mod, "EMPTY_ROWS", empty)
    gat_case = test_gat_ops.case.__wrapped__
    monkeypatch.setattr(test_gat_ops, "case", gat_case)
    monkeypatch.setattr(test_gat_dropout, "case", gat_case)
    monkeypatch.setattr(test_gat_dropout, "drop_case",
                        test_gat_dropout.drop_case.__wrapped__)
    monkeypatch.setattr(test_gatv2_ops, "case",
                        test_gatv2_ops.case.__wrapped__)


def _fp32_checks(device):
    H, D = GAT_SHAPE
    test_gat_ops._check(device, H, D, False)
    test_gat_dropout._check(device, H, D, DROP_P)
    for H, D in GATV2_SHAPES:
        test_gatv2_ops._check(device, H, D)
    H, D = GATV2_SHAPES[0]
    test_gatv2_ops._check(device, H, D, p=DROP_P)


def test_attn_edge_walk_alignments_cpu(on_walk_graph):
    """The same checks on the CPU path: the references hold on this graph."""
    _fp32_checks("cpu")


@pytest.mark.gpu
def test_attn_edge_walk_alignments_gpu(on_walk_graph):
    """GAT forward + backward and GATv2 forward + both backwards, fp32 and
    bf16, once each with attention dropout."""
    _fp32_checks("cuda")
    H, D = GAT_SHAPE
    test_gat_ops.test_gat_aggregate_bf16_gpu(H, D)
    # the forward-only bf16 instance is the 8-wide one
    c = test_gat_ops.case(H, D, bf16=True)
    z, el, er = (c[k].cuda().bfloat16() for k in ("z", "el", "er"))
    out = ops.gat_aggregate_csr(walk_graph("cuda").csr, z, el, er, H,
                                test_gat_ops.SLOPE)
    ref = c["ref"]["out"]
    err = test_gat_ops._err(out, ref) / ref.abs().max().item()
    assert out.dtype == torch.bfloat16 and err < 0.02, err
    for H, D in GATV2_SHAPES:
        test_gatv2_ops.test_gatv2_aggregate_bf16_gpu(H, D)
