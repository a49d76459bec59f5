"""The two kernels of the relational attention layer under the guard-band protocol of ``test_guarded.py``, at the smallest
ragged shapes that reach both of their halves - a segment finished by its owner (at most 64 edges) and one taken by a
whole workgroup (more than 64, and a hub of several rounds of 256): the scalars and the per-edge values are INPUTS and
must come back unchanged, what the wrappers copy out of the view (the kept counts, both weight arrays) and the segment
sums sit between bands, hold the same bits whether their memory was pre-filled with 0x00 or 0xFF, and again with every
base 16 bytes past a 512-byte boundary."""
import pytest
import torch

from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import ops
from test_guarded import _randn, protocol

pytestmark = pytest.mark.gpu

N, R = 37, 2
LENGTHS = {(3, 0): 1, (4, 1): 7, (5, 0): 9, (6, 1): 64, (7, 0): 65, (8, 1): 257, (9, 0): 700}   # (destination, relation): in-edges


def _world(dev):
    gen = torch.Generator().manual_seed(9)
    src = torch.cat([torch.randint(0, N, (n,), generator=gen) for n in LENGTHS.values()])
    dst = torch.cat([torch.full((n,), node) for (node, _), n in LENGTHS.items()])
    rel = torch.cat([torch.full((n,), r) for (_, r), n in LENGTHS.items()])
    order = torch.randperm(src.numel(), generator=gen)
    ei, et = torch.stack([src, dst])[:, order].contiguous(), rel[order].contiguous()
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), N, R)
    # the precondition of both halves, in both directions: segments on either side of the 64-edge border, empty ones
    lens = torch.bincount(ei[1] * R + et, minlength=N * R)
    assert int(lens.max()) == 700 and {1, 7, 9, 64, 65, 257} <= set(lens.tolist()) and int((lens == 0).sum()) > 0
    assert int((lens > 64).sum()) == 3 and int(((lens > 0) & (lens <= 64)).sum()) == 4
    lens_t = torch.bincount(ei[0] * R + et, minlength=N * R)
    assert int(lens_t.max()) <= 64 and int((lens_t > 8).sum()) > 0 and int((lens_t == 0).sum()) == 0
    return g, ops.EdgeDropout(g), ei, gen


@pytest.mark.parametrize("hiding", [False, True])
def test_the_attention_draw(hiding, monkeypatch):
    dev = need_gpu()
    g, ed, ei, gen = _world(dev)
    e = ei.size(1)
    a = (2.0 * torch.randn(2, N, R, generator=gen)).to(dev)
    stats0 = torch.zeros(2, dtype=torch.int64, device=dev)
    position = torch.randperm(e, generator=gen).to(dev)
    cursor = torch.tensor([11], dtype=torch.int64, device=dev)
    x = _randn(gen, N, 8).to(dev)
    kw = dict(position=position, cursor=cursor, batch=200, hide_twins=True) if hiding else {}

    def fn(ctx):
        stats = ctx.like(stats0)
        ed.set_attention(a, 0.2, stats=stats, **kw)
        return {"stats": stats, "kept": ed.kept_counts(), "val": [ed.view.arrays(False)[3], ed.view.arrays(True)[3]],
                "agg": ops.aggregate(ed.view, x), "gagg": ops.aggregate(ed.view, x, transposed=True)}

    try:
        protocol(monkeypatch, [a, stats0, x] + ([position, cursor] if hiding else []), fn)
        kept = int(ed.kept_counts().sum())
        assert kept <= e - 200 if hiding else kept == e            # (a twin outside the window is hidden too)
    finally:
        ed.destroy()
        g.destroy()


def test_the_edge_sum(monkeypatch):
    dev = need_gpu()
    g, ed, ei, gen = _world(dev)
    values = torch.randn(ei.size(1), generator=gen).to(dev)

    def fn(ctx):
        return {"forward": ops.edge_segment_sum(g, values), "transposed": ops.edge_segment_sum(g, values, transposed=True),
                "over the view": ops.edge_segment_sum(ed.view, values)}

    try:
        protocol(monkeypatch, [values], fn)
    finally:
        ed.destroy()
        g.destroy()
