"""HaloGraph.csc_simple(): the CSC without repeated entries that the max
aggregation's backward walks (CPU)."""
import torch

from pipegcn_amd import native
from pipegcn_amd.graph.csr import HaloGraph
from tests.test_gat_ops import N_DST, N_SRC, edges, graph


def _rows(csr):
    return [csr.indices[csr.indptr[r]:csr.indptr[r + 1]].tolist()
            for r in range(csr.num_rows)]


def test_rows_are_the_sets_of_the_original_rows():
    hg = graph("cpu")
    simple = hg.csc_simple()
    assert simple is not hg.csc
    assert (simple.num_rows, simple.num_cols) == (N_SRC, N_DST)
    assert simple.indptr.dtype == torch.int64
    assert simple.indices.dtype == torch.int32
    assert simple.indptr[0] == 0 and simple.indptr[-1] == simple.nnz
    some_repeat = False
    for old, new in zip(_rows(hg.csc), _rows(simple)):
        assert len(set(new)) == len(new)
        assert set(new) == set(old)
        some_repeat |= len(new) < len(old)
    assert some_repeat
    assert hg.csc.nnz == 4177 and simple.nnz == 3988
    # the original CSC is left alone
    assert hg.csc.nnz == edges()[0].numel()


def test_row_order_is_lpt_of_the_view():
    simple = graph("cpu").csc_simple()
    deg = simple.indptr[1:] - simple.indptr[:-1]
    order = simple.row_order.long()
    assert simple.row_order.dtype == torch.int32
    assert sorted(order.tolist()) == list(range(N_SRC))
    assert (deg[order][:-1] >= deg[order][1:]).all()


def test_view_is_cached():
    hg = graph("cpu")
    assert hg.csc_simple() is hg.csc_simple()


def test_graph_without_duplicates_returns_its_csc():
    u = torch.tensor([0, 1, 2, 3, 1, 4])
    v = torch.tensor([0, 0, 1, 1, 2, 2])
    hg = HaloGraph.from_edges(u, v, 3, 6)  # source 5 has no edge
    assert hg.csc_simple() is hg.csc


def test_empty_rows_survive():
    # source 2 and source 4 have no edge; 0 -> 1 is there three times
    u = torch.tensor([0, 0, 3, 0, 1, 3])
    v = torch.tensor([1, 1, 0, 1, 1, 0])
    hg = HaloGraph.from_edges(u, v, 2, 5)
    simple = hg.csc_simple()
    assert simple.indptr.tolist() == [0, 1, 2, 2, 3, 3]
    assert simple.indices.tolist() == [1, 1, 0]


def test_native_csr_simple_reports_removal():
    indptr = torch.tensor([0, 3, 3, 5])
    indices = torch.tensor([7, 2, 7, 1, 0], dtype=torch.int32)
    ip, ix, removed = native().csr_simple(indptr, indices)
    assert bool(removed)
    assert ip.tolist() == [0, 2, 2, 4] and ix.tolist() == [2, 7, 0, 1]
    ip2, ix2, removed2 = native().csr_simple(ip, ix)
    assert not bool(removed2)
    assert ip2.tolist() == ip.tolist() and ix2.tolist() == ix.tolist()
