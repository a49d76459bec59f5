"""GPU tier: the sum of a hub segment's partial rows (csrc/rgcn_hub_finish.h, rgcn_reduce_item), which asks for the mean's
divisor ``cnt[dst]`` together with the first batch of rows instead of after the barrier - through the gather's second
launch (k_reduce_partials) and through the transforms that finish the hub rows of their own row tile.

One edge list, read in both directions.  Four hub nodes have 257, 512, 513 (relation 1) and 5,125 (relation 0) out-edges
to destinations of their own, so a hub's segment leaves 2, 2, 3 and 21 partial rows (one per 256 edges): one row more
than a pack, exactly two, two and one edge, and a count that ends inside a batch of row loads at either width (a batch
is 16 rows for each of the 256 / (d / 4) row slots).  Every third of those destinations has a second in-edge from one
of 50 filler sources, so the transposed structure's weights are 1 and 1/2; relation 2 has no edge.
  * ``out``: the hubs as sources - the transposed structure is weighted (``cnt`` = NULL in the kernel);
  * ``in``:  the same pairs flipped, the hubs as destinations - the plain structure is a mean over 257 .. 5,125 rows.

Exact where the gather tests claim exactness (tests/test_gather_empty_rows.py): integer tables in [-8, 8] and weights
that are powers of two make every partial sum exact in float32 in any order, and the mean divides an exact integer by
an integer once; the expectation is that edge-order sum in float64, cast.  With seeded normal floats the order of the
additions shows, and the hub rows must be the bytes the build before this change gave, kept in
tests/golden/reduce_item_parent.npz (tests/golden/make_reduce_item_golden.py wrote it from these inputs)."""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, need_gpu
from primekg_rgcn_linkprediction_amd import ops

pytestmark = pytest.mark.gpu

HUBS = ((0, 5125), (1, 257), (1, 512), (1, 513))        # (relation, edges)
N_DEST, N_NODES, R = 5200, 5260, 3                      # destinations 0 .. 5,199; hubs 5,200 ..; fillers 5,210 .. 5,259
FIXTURE = os.path.join(GOLDEN, "reduce_item_parent.npz")


def edge_list():
    """-> (src, dst, rel) int64 of the ``out`` reading"""
    src, dst, rel = [], [], []
    first = {0: 0, 1: 0}
    for h, (k, edges) in enumerate(HUBS):
        dests = np.arange(first[k], first[k] + edges)
        first[k] += edges
        src += [np.full(edges, N_DEST + h), 5210 + (dests[::3] // 3) % 50]
        dst += [dests, dests[::3]]
        rel.append(np.full(edges + dests[::3].size, k))
    return np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64), np.concatenate(rel).astype(np.int64)


class Side:
    def __init__(self, dev, side):
        src, dst, rel = edge_list()
        if side == "in":
            src, dst = dst, src
        self.side, self.src, self.dst, self.rel = side, src, dst, rel
        self.transposed = side == "out"
        self.graph = ops.BucketedGraph(torch.from_numpy(np.stack([src, dst])).to(dev), torch.from_numpy(rel).to(dev),
                                       N_NODES, R)
        self.cnt = np.bincount(dst * R + rel, minlength=N_NODES * R)
        self.hub_rows = np.array([(N_DEST + h) * R + k for h, (k, _) in enumerate(HUBS)])
        assert self.graph.num_levels(self.transposed) == 2
        key = (src if self.transposed else dst) * R + rel
        assert [int((key == row).sum()) for row in self.hub_rows] == [e for _, e in HUBS]

    def gather(self, x):
        return ops.aggregate(self.graph, x, transposed=self.transposed)

    def exact(self, x):
        """float64, edge order, cast: the weighted sum over out-edges (``out``) or the mean over in-edges (``in``)"""
        s = np.zeros((N_NODES * R, x.shape[1]))
        if self.transposed:
            assert np.isin(self.cnt[self.cnt > 0], (1, 2)).all()
            np.add.at(s, self.src * R + self.rel, x.astype(np.float64)[self.dst] / self.cnt[self.dst * R + self.rel][:, None])
        else:
            np.add.at(s, self.dst * R + self.rel, x.astype(np.float64)[self.src])
            s /= np.maximum(self.cnt, 1)[:, None]
        return s.astype(np.float32).reshape(N_NODES, -1)


@functools.lru_cache(maxsize=None)
def side(name):
    return Side(torch.device("cuda:0"), name)


def table(kind, d):
    rng = np.random.default_rng(d + (0 if kind == "ints" else 7))
    if kind == "ints":
        return rng.integers(-8, 9, (N_NODES, d)).astype(np.float32)
    return rng.standard_normal((N_NODES, d)).astype(np.float32)


def digest(a):
    return np.frombuffer(hashlib.sha1(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def _poisoned(monkeypatch, fn):
    """fn() with the library's allocations pre-filled with 0xFF, so a row nobody wrote shows"""
    from guarded import GuardedAllocator, installed
    alloc = GuardedAllocator(0xFF)
    with installed(monkeypatch, alloc):
        got = fn()
        torch.cuda.synchronize()
    alloc.check()
    return got


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", ["in", "out"])
def test_hub_rows_through_the_second_launch(name, d, monkeypatch):
    dev = need_gpu()
    s = side(name)
    x = table("ints", d)
    got = _poisoned(monkeypatch, lambda: s.gather(torch.from_numpy(x).to(dev))).cpu().numpy()
    want = s.exact(x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "integer table: not the exact sums"
    x = table("floats", d)
    got = _poisoned(monkeypatch, lambda: s.gather(torch.from_numpy(x).to(dev))).cpu().numpy()
    with np.load(FIXTURE) as z:
        rows, sha = z[f"{name}_d{d}_hub_rows"], z[f"{name}_d{d}_sha1"]
    hub = got.reshape(N_NODES * R, d)[s.hub_rows]
    assert np.array_equal(hub.view(np.uint32), rows.view(np.uint32)), "hub rows differ from the recorded bytes"
    assert np.array_equal(digest(got), sha), "rows other than the hubs' differ from the recorded output"


@pytest.mark.parametrize("d", [64, 128])
def test_hub_rows_through_the_transforms_that_finish_them(d):
    """``aggregate_deferred`` leaves the hub rows to the split-precision transform that reads the aggregate: once it
    ran, the aggregate holds the bytes of the two-launch gather - mean rows through the forward transform, weighted
    rows through the input gradient"""
    dev = need_gpu()
    gen = torch.Generator().manual_seed(d)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).to(dev)                                       # noqa: E731
    # forward: d -> 128 over the mean structure
    s = side("in")
    x = torch.from_numpy(table("floats", d)).to(dev)
    weight, root, bias = rnd(R, d, 128) / d ** 0.5, rnd(d, 128) / d ** 0.5, rnd(128)
    packed, x_amax = ops.split_weights(weight, root), ops.absmax(x)
    full = s.gather(x)
    want = ops.transform_fwd(full, x, weight, root, bias, graph=s.graph, amax=(x_amax, x_amax), packed=packed)
    agg, hubs = ops.aggregate_deferred(s.graph, x)
    assert hubs is not None
    got = ops.transform_fwd(agg, x, weight, root, bias, graph=s.graph, amax=(x_amax, x_amax), packed=packed, hubs=hubs)
    assert torch.equal(agg.view(torch.int32), full.view(torch.int32)) and torch.equal(got, want)
    # input gradient: rows of width d over the weighted transposed structure
    s = side("out")
    d_in = 128 if d == 128 else 256
    g = torch.from_numpy(table("floats", d)).to(dev) * 1e-3
    weight, root = rnd(R, d_in, d) / d_in ** 0.5, rnd(d_in, d) / d_in ** 0.5
    packed, g_amax, wb = ops.split_weights(weight, root), ops.absmax(g), s.graph.weight_bound(True)
    full = s.gather(g)
    want = ops.transform_bwd_input(full, g, weight, root, graph=s.graph, amax=(g_amax, g_amax), amax_mul=wb, packed=packed)
    gagg, hubs = ops.aggregate_deferred(s.graph, g, transposed=True)
    assert hubs is not None
    got = ops.transform_bwd_input(gagg, g, weight, root, graph=s.graph, amax=(g_amax, g_amax), amax_mul=wb, packed=packed,
                                  hubs=hubs)
    assert torch.equal(gagg.view(torch.int32), full.view(torch.int32)) and torch.equal(got, want)
