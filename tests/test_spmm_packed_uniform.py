"""The packed gather keeps what a wave shares (row, edge cursor, node ids,
record bases) in scalar registers. These cases aim at what that can break:
every phase of the edge pipeline at every start alignment, the grid-stride
loop, record offsets past 2^32 bytes, and a chunk with a single live lane.
Each compares `ops.spmm_packed` bit for bit with `ops.spmm` (the dense
kernel is the reference; no tolerance), with and without `row_order` and
with and without `dst_scale`. The dense kernel follows the same convention,
so the grid-stride and the 2^32 cases also hold both kernels to a sum made
in torch in the same order."""
import pytest
import torch

from pipegcn_amd import ops
from pipegcn_amd.graph.csr import CSR

NUM_SRC = 400
MAX_DEG = 40
LONG_ROW = 1003


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(csr, x, scale):
    """csr on the device, with a row order. -> the last reference output."""
    plain = CSR(csr.indptr, csr.indices, csr.num_rows, csr.num_cols, None)
    for c in (csr, plain):
        for s in (None, scale):
            ref = ops.spmm(c, x, s)
            out = ops.spmm_packed(c, x, s)
            assert out.shape == ref.shape
            assert torch.equal(_bits(out), _bits(ref)), (
                x.shape[1], c.row_order is not None, s is not None)
            del out
    return ref


def _same_values(a, b):
    """Equal as numbers, NaN where the other is NaN, and the same zeros'
    signs: what an independent reference can promise (a NaN's payload is
    the adder's business)."""
    nan = torch.isnan(a)
    return (torch.equal(nan, torch.isnan(b))
            and torch.equal(_bits(a)[~nan], _bits(b)[~nan]))


def _torch_rows(csr, x, scale, rows):
    """out[rows] of the SpMM, summed in torch in the kernels' order: edges
    one by one up to a multiple of 4, then groups of four added as
    ((v0 + v1) + v2) + v3, then the rest one by one; times scale. Both
    kernels are held to it, so the dense reference is checked too where the
    other dense tests do not reach."""
    indptr, idx = csr.indptr.tolist(), csr.indices.long()
    out = []
    for r in rows:
        e, end = indptr[r], indptr[r + 1]
        acc = torch.zeros(x.shape[1], device=x.device)
        while e < end and e & 3:
            acc = acc + x[idx[e]]
            e += 1
        while e + 4 <= end:
            v = x[idx[e:e + 4]]
            acc = acc + (((v[0] + v[1]) + v[2]) + v[3])
            e += 4
        while e < end:
            acc = acc + x[idx[e]]
            e += 1
        out.append(acc * (scale[r] if scale is not None else 1.0))
    return torch.stack(out)


def _check_rows(csr, x, scale, rows):
    for s in (None, scale):
        want = _torch_rows(csr, x, s, rows)
        for got in (ops.spmm(csr, x, s), ops.spmm_packed(csr, x, s)):
            assert _same_values(got[rows], want), s is not None


def _scale(csr):
    return (1.0 / csr.row_degrees().clamp(min=1.0)).contiguous()


# -------------------------------------------- (a) phases x start alignments


def _phase_degrees():
    """Degrees 0..40 four times over, a filler row of degree 1, 2, 3 between
    the repeats, then one long row. A repeat holds 820 edges, a multiple of
    4, so the fillers alone move the alignment: each degree starts once at
    every value of indptr[r] & 3."""
    rep = torch.arange(MAX_DEG + 1)
    one = lambda d: torch.tensor([d])
    return torch.cat((rep, one(1), rep, one(2), rep, one(3), rep,
                      one(LONG_ROW)))


_PHASE = {}


def _phase_graph():
    if not _PHASE:
        deg = _phase_degrees()
        g = torch.Generator().manual_seed(23)
        v = torch.repeat_interleave(torch.arange(deg.numel()), deg)
        u = torch.randint(0, NUM_SRC, (v.numel(),), generator=g)
        # the planted rows (_input) are certainly gathered
        u[:8] = torch.arange(8)
        _PHASE["csr"] = CSR.from_coo(u, v, deg.numel(), NUM_SRC)
        _assert_every_alignment(_PHASE["csr"])
    return _PHASE["csr"]


def _assert_every_alignment(csr):
    deg = csr.indptr[1:] - csr.indptr[:-1]
    assert torch.equal(deg, _phase_degrees())
    start = csr.indptr[:-1] & 3
    for d in range(MAX_DEG + 1):
        assert set(start[deg == d].tolist()) == {0, 1, 2, 3}, d


def _input(F, density, n=NUM_SRC):
    """fp32 [n, F] with about `density` non-zeros, and planted: an all-zero
    row, an all-non-zero row, two -0.0 (dropped), a NaN and an Inf (kept)."""
    g = torch.Generator().manual_seed(1000 * F + int(100 * density))
    x = torch.randn(n, F, generator=g)
    x[x == 0] = 1.0
    x = x * (torch.rand(n, F, generator=g) < density)
    x[0] = 0.0
    x[1] = torch.arange(1, F + 1, dtype=torch.float32)
    x[2, 0] = -0.0
    x[3, F - 1] = float("nan")
    x[4, 1] = float("inf")
    x[5, F // 2] = -0.0
    return x


# one width per lane-width instance (41: 1 column per lane; 100: 2; 132,
# 256: 4, one chunk; 602: 4, three chunks, the last one ragged)
@pytest.mark.gpu
@pytest.mark.parametrize("F", [41, 100, 132, 256, 602])
@pytest.mark.parametrize("density", [0.25, 0.5])
def test_every_phase_every_alignment(F, density):
    csr = _phase_graph().to("cuda")
    ref = _check(csr, _input(F, density).cuda(), _scale(csr))
    assert torch.isnan(ref).any() and torch.isinf(ref).any()


# ------------------------------------------- (d) one live lane in a chunk


@pytest.mark.gpu
@pytest.mark.parametrize("density", [0.25, 0.5])
def test_last_chunk_one_live_lane(density):
    """F=260 at 4 columns per lane: the second chunk's only live lane is
    lane 0 (columns 256..259); the wave's uniform values are read with the
    other 63 masked off."""
    csr = _phase_graph().to("cuda")
    x = _input(260, density)
    x[6, 256:] = torch.tensor([1.5, 0.0, -2.5, 3.5])
    x[7, 256:] = 0.0
    ref = _check(csr, x.cuda(), _scale(csr))
    assert (ref[:, 256:] != 0).any()


# ------------------------------------------------------ (b) grid-stride loop


@pytest.mark.gpu
def test_grid_stride_loop():
    """More (row, chunk) pairs than the grid has waves (8 * 65,536 blocks of
    4): 2.2 M rows of degree 0, 1, 2 at F=132 (one chunk), so the last 100 k
    pairs are a wave's second trip. The row order is a random permutation
    (the kernel only needs a permutation), so second trips meet every
    degree with it as without it."""
    n, n_src, F = 2_200_000, 64, 132
    assert n > 8 * 65536 * 4
    g = torch.Generator().manual_seed(5)
    deg = torch.arange(n) % 3
    indptr = torch.zeros(n + 1, dtype=torch.int64)
    indptr[1:] = deg.cumsum(0)
    indices = torch.randint(0, n_src, (int(indptr[-1]),), generator=g,
                            dtype=torch.int32)
    order = torch.randperm(n, generator=g).to(torch.int32)
    csr = CSR(indptr, indices, n, n_src, order).to("cuda")
    x = _input(F, 0.5, n_src).cuda()
    ref = _check(csr, x, _scale(csr))
    # the rows past the first trip are not all empty
    first_trip = 8 * 65536 * 4
    assert (ref[first_trip:] != 0).any()
    del ref
    # independent of the dense kernel: first rows, the rows either side of
    # the end of the first trip, the last rows
    rows = (list(range(12)) + list(range(first_trip - 12, first_trip + 24))
            + list(range(n - 12, n)))
    _check_rows(csr, x, _scale(csr), rows)


# ------------------------------------------ (c) record offsets beyond 2^32


@pytest.mark.gpu
def test_record_offset_beyond_4gib():
    """1.6 M source rows at F=602: the packed stride is 2,688 B, so records
    from row 1,597,831 on start past 2^32 bytes (the buffer is 4.3 GB). A
    32-bit row base would gather some other row's values."""
    n_src, F, n_dst = 1_600_000, 602, 40
    stride = ops.packed_row_layout(F)[2] * 4
    assert stride == 2688
    first_far = (1 << 32) // stride + 1
    assert first_far * stride > 1 << 32 and n_src - first_far > 2000

    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(n_src, F, device="cuda", generator=g)
    x.mul_(torch.rand(n_src, F, device="cuda", generator=g) < 0.5)
    planted = torch.tensor([0, n_src - 1, first_far - 1, first_far])
    x[planted[0]] = torch.arange(1, F + 1, dtype=torch.float32).cuda()
    x[planted[1], 3] = float("inf")
    x[planted[2]] = 0.0
    x[planted[3], F - 1] = float("nan")

    cg = torch.Generator().manual_seed(9)
    deg = torch.arange(n_dst) % 14  # 0..13: peel, groups and tail
    us = []
    for r, d in enumerate(deg.tolist()):
        far = torch.randint(first_far, n_src, (d,), generator=cg)
        near = torch.randint(0, n_src, (d,), generator=cg)
        # every other row gathers only from beyond 4 GiB, the rest mixed
        u = far if r % 2 else torch.where(torch.arange(d) % 2 == 0, far, near)
        us.append(u)
    u = torch.cat(us)
    u[:4] = planted  # row 1 (degree 1) .. row 3: first edges of the list
    u[-4:] = planted
    indptr = torch.zeros(n_dst + 1, dtype=torch.int64)
    indptr[1:] = deg.cumsum(0)
    order = torch.argsort(deg, descending=True).to(torch.int32)
    csr = CSR(indptr, u.to(torch.int32), n_dst, n_src, order).to("cuda")
    assert int((u * stride >= 1 << 32).sum()) > u.numel() // 2
    ref = _check(csr, x, _scale(csr))
    assert torch.isnan(ref).any() and torch.isinf(ref).any()
    # and every row against torch, independent of the dense kernel
    _check_rows(csr, x, _scale(csr), list(range(n_dst)))
