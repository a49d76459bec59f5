"""GPU tier: the fixed-order sum of the parameter-gradient slabs (csrc/rgcn_slab_reduce.h), whose loads go out in
predicated batches of BATCH slabs per thread - alone (``rgcn_slab_reduce``) and as riders of a transposed gather.

Expected values are a float32 NumPy restatement that adds in the library's order and nothing else: thread group g of
GROUPS = 16 sums the slabs ``S * g // 16 .. S * (g + 1) // 16 - 1`` in order starting from +0.0, then the 16 group sums
are added in group order.  Float32 addition is correctly rounded on both sides, so the comparison is of bytes.  The
shapes are chosen for the loop boundaries, not for size: ``Kc = 96`` with ``K1 = 64`` puts the weight / root boundary
inside the reduction's outputs, ``N = 32``; S runs over every count of slabs per group around one and two batches."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import _lib, ops

pytestmark = pytest.mark.gpu

BATCH, GROUPS = 8, 16                                   # RGCN_SLAB_BATCH, RGCN_SLAB_GROUPS
K1, KC, N = 64, 96, 32
# slabs per group: 112 -> 7; 128 -> 8; 137 -> 8 and 9; 248 -> 15 and 16; 265 -> 16 and 17
S_BATCH = [112, 128, 137, 248, 265]
S_EDGES = [1, 15, 16, 17, 61, 121]                      # 1 and 15 leave groups with nothing; 61 and 121 are C2's


def _group_sizes(s):
    return {s * (g + 1) // GROUPS - s * g // GROUPS for g in range(GROUPS)}


def test_the_split_counts_cover_every_loop_boundary():
    need_gpu()
    seen = set().union(*(_group_sizes(s) for s in S_BATCH))
    assert {BATCH - 1, BATCH, BATCH + 1, 2 * BATCH - 1, 2 * BATCH, 2 * BATCH + 1} <= seen
    assert 0 in _group_sizes(1) and 0 in _group_sizes(15) and _group_sizes(16) == {1} and _group_sizes(17) == {1, 2}
    assert _group_sizes(61) == {3, 4} and _group_sizes(121) == {7, 8}


def _ordered_sum(parts):
    """parts [S, ...] float32 -> their sum in the library's order"""
    s = parts.shape[0]
    total = None
    for g in range(GROUPS):
        acc = np.zeros(parts.shape[1:], dtype=np.float32)
        for i in range(s * g // GROUPS, s * (g + 1) // GROUPS):
            acc = acc + parts[i]
        total = acc if total is None else total + acc
    assert total.dtype == np.float32
    return total


@functools.lru_cache(maxsize=None)
def _inputs(s, n=N, special=False):
    """-> (slab [S, Kc, n], bias_part [S, n], restated grad_weight, grad_root, grad_bias), computed once per shape"""
    rng = np.random.default_rng(1000 * s + n)
    slab = rng.standard_normal((s, KC, n)).astype(np.float32)
    bias_part = rng.standard_normal((s, n)).astype(np.float32)
    if special:                                         # one of each, in outputs of their own: weight, weight, root
        slab[s // 2, 5, 7 % n] = np.float32(np.nan)
        slab[s // 3, 10, 1] = np.float32(np.inf)
        slab[s - 1, 70, 2] = np.float32(-np.inf)
    with np.errstate(invalid="ignore"):
        total = _ordered_sum(slab)
    for a in (slab, bias_part):
        a.setflags(write=False)
    return slab, bias_part, total[:K1], total[K1:], _ordered_sum(bias_part)


class Job:
    """a synthetic pending reduction on the device: the slabs, and outputs pre-filled with one byte"""

    def __init__(self, dev, slab, bias_part, fill=0xFF, root=True, bias=True):
        s, kc, n = slab.shape
        self.slab, self.bias_part = torch.from_numpy(slab.copy()).to(dev), torch.from_numpy(bias_part.copy()).to(dev)
        new = lambda *shape: torch.full(shape, fill, dtype=torch.uint8, device=dev).view(torch.float32)    # noqa: E731
        self.gw = new(K1 * n * 4)
        self.groot = new((kc - K1) * n * 4)
        self.gbias = new(n * 4)
        ptr = lambda t, on=True: t.data_ptr() if on else None                                              # noqa: E731
        self.job = _lib.SlabJob(slab=ptr(self.slab), bias_part=ptr(self.bias_part), splits=s, K1=K1, Kc=kc, N=n,
                                grad_weight=ptr(self.gw), grad_root=ptr(self.groot, root), grad_bias=ptr(self.gbias, bias))

    def reduce(self):
        rc = _lib.load().rgcn_slab_reduce(ctypes.byref(self.job), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "rgcn_slab_reduce")
        torch.cuda.synchronize()
        return self

    def outputs(self):
        return tuple(t.cpu().numpy() for t in (self.gw, self.groot, self.gbias))


def _same_bytes(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.size == want.size
    diff = got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} words differ, first at {int(np.argmax(diff))}"


def _untouched(got, what):
    assert (got.view(np.uint32) == 0xFFFFFFFF).all(), f"{what} was written"


@pytest.mark.parametrize("s", S_BATCH + S_EDGES)
def test_every_split_count_alone(s):
    dev = need_gpu()
    slab, bias_part, gw, groot, gbias = _inputs(s)
    got = Job(dev, slab, bias_part).reduce().outputs()
    for g, w, what in zip(got, (gw, groot, gbias), ("grad_weight", "grad_root", "grad_bias")):
        _same_bytes(g, w, f"S = {s}: {what}")


@pytest.mark.parametrize("s", [17, 137])
def test_absent_outputs_and_the_narrowest_rows(s):
    dev = need_gpu()
    slab, bias_part, gw, groot, gbias = _inputs(s)
    got = Job(dev, slab, bias_part, bias=False).reduce().outputs()
    _same_bytes(got[0], gw, "grad_weight"), _same_bytes(got[1], groot, "grad_root"), _untouched(got[2], "grad_bias")
    got = Job(dev, slab, bias_part, root=False).reduce().outputs()
    _same_bytes(got[0], gw, "grad_weight"), _untouched(got[1], "grad_root"), _same_bytes(got[2], gbias, "grad_bias")
    slab, bias_part, gw, groot, gbias = _inputs(s, 4)   # N = 4: one float4 per row, one bias output
    got = Job(dev, slab, bias_part).reduce().outputs()
    for g, w, what in zip(got, (gw, groot, gbias), ("grad_weight", "grad_root", "grad_bias")):
        _same_bytes(g, w, f"N = 4: {what}")


def test_non_finite_values_come_through_as_the_ordered_sum_gives_them():
    dev = need_gpu()
    s = 61
    slab, bias_part, gw, groot, gbias = _inputs(s, N, True)
    assert np.isnan(gw).sum() == 1 and np.isposinf(gw).sum() == 1 and np.isneginf(groot).sum() == 1
    got = Job(dev, slab, bias_part).reduce().outputs()
    for g, w, what in zip(got, (gw, groot, gbias), ("grad_weight", "grad_root", "grad_bias")):
        _same_bytes(g, w, what)


# ------------------------------------------------------------------------------------------- the same jobs as riders
@functools.lru_cache(maxsize=None)
def _rider_graph():
    """200 nodes, 3 relations: node 0 has 300 out-edges of relation 0 (a pack and a partial row in the transposed
    structure), 150 random edges of relations 0 and 1, relation 2 has none: most (node, relation) segments are empty"""
    dev = torch.device("cuda:0")
    n, r = 200, 3
    gen = torch.Generator().manual_seed(5)
    hub = torch.stack([torch.zeros(300, dtype=torch.int64), torch.arange(300) % (n - 1) + 1])
    rnd = torch.randint(0, n, (2, 150), generator=gen)
    ei = torch.cat([hub, rnd], dim=1)
    et = torch.cat([torch.zeros(300, dtype=torch.int64), torch.randint(0, 2, (150,), generator=gen)])
    graph = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    assert graph.num_levels(True) == 2
    return graph, n, r


@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("d", [64, 128])
def test_the_same_jobs_as_riders_of_a_transposed_gather(d, fill):
    """gradients and gathered rows of ``aggregate(..., transposed=True, tail=...)`` against the reduction launched alone
    and a plain gather, as bytes, on outputs that held 0x00 and 0xFF before"""
    dev = need_gpu()
    graph, n, r = _rider_graph()
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(d)).to(dev)
    plain = ops.aggregate(graph, x, transposed=True).cpu().numpy()
    for s in S_BATCH + S_EDGES:
        slab, bias_part, *_ = _inputs(s)
        want = Job(dev, slab, bias_part, fill).reduce().outputs()
        job = Job(dev, slab, bias_part, fill)
        out = torch.full((n, r * d * 4), fill, dtype=torch.uint8, device=dev).view(torch.float32)
        pend = ops.PendingParamGrads((job.gw, job.groot, job.gbias), job.job, None)
        rows = ops.aggregate(graph, x, transposed=True, tail=pend, out=out)
        torch.cuda.synchronize()
        assert pend.done and rows.data_ptr() == out.data_ptr()
        _same_bytes(rows.cpu().numpy(), plain, f"S = {s}: gathered rows")
        for g, w, what in zip(job.outputs(), want, ("grad_weight", "grad_root", "grad_bias")):
            _same_bytes(g, w, f"S = {s}: {what}")
