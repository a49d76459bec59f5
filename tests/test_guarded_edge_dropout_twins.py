"""Twin-aware edge dropout under the guard-band protocol of ``test_guarded.py``, as ``test_guarded_edge_dropout.py`` runs
the plain draw: create (which pairs the twins with sorts of its own and frees them), a draw with both option bits and both
gathers over the view, every output and workspace between bands, pre-filled with 0x00 / 0xFF, and once more with every
base 16 bytes past a 512-byte boundary.  What the protocol sees of create and of the draw is what the wrappers copy out
of the view - the kept counts and both weight arrays - which must agree bit for bit across the four runs, and with the
host restatement."""
import numpy as np
import pytest
import torch

import edge_dropout_reference as R
import edge_dropout_twins_reference as TW
from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import ops, synth
from test_guarded import _randn, protocol

pytestmark = pytest.mark.gpu


def test_create_draw_with_both_bits_and_gathers_over_the_view(monkeypatch):
    dev = need_gpu()
    half, n, r = synth.uniform_graph(300, 3000, 3, seed=22)[:2], 300, 3
    half[0][1, :450] = 7                                 # a (dst, rel) segment past 256 edges: packs, partial rows, a hub tree;
    half[1][:450] = 1                                    # by the reverses a source hub as long
    ei = torch.stack([half[0], half[0].flip(0)], dim=2).reshape(2, -1).contiguous()     # a column, then its reverse
    et = half[1].repeat_interleave(2).contiguous()
    ei, et = torch.cat([ei, ei[:, :40]], dim=1), torch.cat([et, et[:40]])                # surplus copies: 20 pairs twice
    e = ei.size(1)
    twin = TW.twins(ei.numpy(), et.numpy())
    assert int((twin >= 0).sum()) > 5000
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    assert g.num_levels(False) == 2 and g.workspace_bytes(False, 64) > 0
    gen = torch.Generator().manual_seed(22)
    x, cot = _randn(gen, n, 64).to(dev), _randn(gen, n, 128).to(dev)
    order = torch.randperm(e, generator=gen)
    position = torch.empty(e, dtype=torch.int64)
    position[order] = torch.arange(e)
    kept, hidden = TW.kept_mask(e, twin, 0.4, 99, 2, 1024, 512, position.numpy(), hide_twins=True, paired=True)
    position, rng, cursor = position.to(dev), torch.tensor([99, 2], device=dev), torch.tensor([1024], device=dev)
    stats0 = torch.zeros(2, dtype=torch.int64, device=dev)

    def fn(ctx):
        out = {}
        ed = ops.EdgeDropout(g)
        try:
            stats = ctx.like(stats0)
            ed.draw(0.4, rng, cursor=cursor, batch=512, position=position, stats=stats, hide_twins=True, paired=True)
            out["stats"], out["kept"] = stats, ed.kept_counts()
            view = ed.view
            out["val"] = [view.arrays(False)[3], view.arrays(True)[3]]
            out["agg"] = ops.aggregate(view, x)
            out["gagg"] = ops.aggregate(view, cot, transposed=True)
            torch.cuda.synchronize()
            assert out["stats"].tolist() == [int(kept.sum()), int(hidden.sum())]
            assert np.array_equal(out["kept"].cpu().numpy(), R.kept_counts(ei.numpy(), et.numpy(), kept, n, r))
        finally:
            ed.destroy()
        return out

    try:
        protocol(monkeypatch, [x, cot, position, rng, cursor, stats0], fn)
    finally:
        g.destroy()
