"""The two kernels of the learned edge masks under the guard-band protocol of ``test_guarded.py``, at the smallest ragged
shapes that reach both of their halves - a segment finished by its owner (at most 64 edges) and one taken by a whole
workgroup (more than 64): the mask is an INPUT and must come back unchanged, what the wrappers copy out of the view (the
kept counts, both weight arrays) and the per-edge gradient sit between bands, hold the same bits whether their memory was
pre-filled with 0x00 or 0xFF, and again with every base 16 bytes past a 512-byte boundary."""
import pytest
import torch

from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import ops
from test_guarded import _randn, protocol

pytestmark = pytest.mark.gpu

N, R = 37, 2
LENGTHS = {(3, 0): 1, (4, 1): 7, (5, 0): 9, (6, 1): 64, (7, 0): 65, (8, 1): 257}     # (destination, relation): in-edges


def _world(dev):
    gen = torch.Generator().manual_seed(9)
    src = torch.cat([torch.randint(0, N, (n,), generator=gen) for n in LENGTHS.values()])
    dst = torch.cat([torch.full((n,), node) for (node, _), n in LENGTHS.items()])
    rel = torch.cat([torch.full((n,), r) for (_, r), n in LENGTHS.items()])
    order = torch.randperm(src.numel(), generator=gen)
    ei, et = torch.stack([src, dst])[:, order].contiguous(), rel[order].contiguous()
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), N, R)
    lens = torch.bincount(ei[1] * R + et, minlength=N * R)
    # the precondition of both halves: segments on either side of the 64-edge border, and empty ones
    assert int(lens.max()) == 257 and {1, 7, 9, 64, 65} <= set(lens.tolist()) and int((lens == 0).sum()) > 0
    assert int((lens > 64).sum()) == 2 and int(((lens > 0) & (lens <= 64)).sum()) == 4
    return g, ops.EdgeDropout(g), ei.size(1), gen


def test_the_mask_draw(monkeypatch):
    dev = need_gpu()
    g, ed, e, gen = _world(dev)
    mask = torch.rand(e, generator=gen)
    mask[::5] = 0.0
    mask = mask.to(dev)
    stats0 = torch.zeros(2, dtype=torch.int64, device=dev)

    def fn(ctx):
        stats = ctx.like(stats0)
        ed.set_mask(mask, stats=stats)
        return {"stats": stats, "kept": ed.kept_counts(), "val": [ed.view.arrays(False)[3], ed.view.arrays(True)[3]],
                "agg": ops.aggregate(ed.view, x), "gagg": ops.aggregate(ed.view, x, transposed=True)}

    x = _randn(gen, N, 8).to(dev)
    try:
        protocol(monkeypatch, [mask, stats0, x], fn)
    finally:
        ed.destroy()
        g.destroy()


@pytest.mark.parametrize("d", [4, 28, 128])
def test_the_gradient_through_the_normalisation(d, monkeypatch):
    dev = need_gpu()
    g, ed, e, gen = _world(dev)
    mask = torch.rand(e, generator=gen) + 0.01
    mask[::7] = 0.0
    ed.set_mask(mask.to(dev))
    assert ed.view.weighted_shard and ed.view.edge_dropout                      # the weighted structure the mode needs
    x, gagg = _randn(gen, N, d).to(dev), _randn(gen, N, R * d).to(dev)

    def fn(ctx):
        return {"bucketed": ops.aggregate_weight_grad(ed.view, x, gagg, through_normalisation=True),
                "by column": ops.aggregate_weight_grad(ed.view, x, gagg, through_normalisation=True, original_order=True)}

    try:
        protocol(monkeypatch, [x, gagg], fn)
    finally:
        ed.destroy()
        g.destroy()
