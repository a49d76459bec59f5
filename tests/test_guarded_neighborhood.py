"""``ops.pair_neighborhood`` under the guarded tier's protocol (``test_guarded.protocol``: plain, then every
``ops._empty`` allocation banded and pre-filled with 0x00, then with 0xFF): no band byte changes, no input changes, the
same output bits in all three runs - so every output of every query is written, the zeros past the radius and the -1
padding included, and nothing is written past a row.  N = 97 (four bitset words, the last one partial), radius 2 of 4,
32 classes, 128 common ids per query."""
import pytest
import torch

import neighborhood_reference as R
from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import ops
from test_guarded import protocol

pytestmark = pytest.mark.gpu

N, RADIUS, CLASSES, CAP = 97, 2, 32, 128


def test_pair_neighborhood(monkeypatch):
    dev = need_gpu()
    ei, et, src, dst = R.zipf_case(N, seed=N)
    hub = int(src[0])                                                              # the case's busiest node, a source
    long_row = torch.stack([torch.full((ops.NEIGHBORHOOD_HUB_DEGREE + 6,), hub), torch.arange(ops.NEIGHBORHOOD_HUB_DEGREE + 6)])
    ei, et = torch.cat([ei, long_row], 1), torch.cat([et, torch.zeros(long_row.size(1), dtype=torch.int64)])
    g = ops.PathGraph(ei, et, N)
    cls = torch.randint(-2, 34, (N,), generator=torch.Generator().manual_seed(N)).to(torch.int32)
    want = R.restate(g, src.tolist(), dst.tolist(), RADIUS, cls, CLASSES, CAP)
    # the preconditions: an out-row walked by the whole wave (in the growth and in the edge count), an intersection
    # compacted past one wave's 64 ids and one that -1 padding follows, a query that leaves everything empty, radii
    # whose slots stay zero
    assert int(g.out_ptr[hub + 1] - g.out_ptr[hub]) >= ops.NEIGHBORHOOD_HUB_DEGREE < N - 5
    assert int(want["common"].max()) > 64 and 0 < int(want["common"][want["common"] > 0].min()) < CAP
    assert int((want["union_nodes"] == 0).sum()) >= 1 and RADIUS < ops.NEIGHBORHOOD_MAX_RADIUS and N % 32 != 0
    g_dev, s, t, c = g.to(dev), src.to(dev), dst.to(dev), cls.to(dev)
    inputs = [s, t, c, g_dev.out_ptr, g_dev.out_dst, g_dev.in_ptr, g_dev.in_src]

    def fn(ctx):
        got = ops.pair_neighborhood(g_dev, s, t, RADIUS, c, CLASSES, CAP)
        R.assert_same(got, want, f"fill {ctx.fill}: " if hasattr(ctx, "fill") else "")
        return [getattr(got, name) for name in R.FIELDS]

    protocol(monkeypatch, inputs, fn)
