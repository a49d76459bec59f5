"""Edge dropout under the guard-band protocol of ``test_guarded.py``: the draw, both gathers over the view and the layer,
every output and workspace between bands, pre-filled with 0x00 / 0xFF, and once more with every base 16 bytes past a
512-byte boundary.  The view's own arrays are the library's (``hipMalloc``); what the protocol sees of the draw is what the
wrappers copy out of it - the kept counts and both weight arrays - which must agree bit for bit across the four runs."""
import pytest
import torch

from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import ops, synth
from test_guarded import _randn, protocol

pytestmark = pytest.mark.gpu


def test_draw_gathers_and_layer_over_the_view(monkeypatch):
    dev = need_gpu()
    ei, et, n, r = synth.uniform_graph(300, 6000, 3, seed=21)
    ei[1, :900] = 7                                      # (dst, rel) segments past 256 edges: packs, partial rows, a hub tree
    ei[0, 1000:1400] = 9                                 # and a source hub for the transposed direction
    e = ei.size(1)
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    assert g.num_levels(False) == 2 and g.workspace_bytes(False, 64) > 0
    ed = ops.EdgeDropout(g)
    gen = torch.Generator().manual_seed(21)
    d_in, d_out = 64, 128
    x, cot = _randn(gen, n, d_in).to(dev), _randn(gen, n, d_out).to(dev)
    weight, root, bias = (_randn(gen, *s, scale=0.1).to(dev) for s in ((r, d_in, d_out), (d_in, d_out), (d_out,)))
    order = torch.randperm(e, generator=gen)
    position = torch.empty(e, dtype=torch.int64)
    position[order] = torch.arange(e)
    position, rng, cursor = position.to(dev), torch.tensor([99, 2], device=dev), torch.tensor([1024], device=dev)
    stats0 = torch.zeros(2, dtype=torch.int64, device=dev)

    def fn(ctx):
        out = {}
        stats = ctx.like(stats0)
        ed.draw(0.4, rng, cursor=cursor, batch=512, position=position, stats=stats)
        out["stats"], out["kept"] = stats, ed.kept_counts()
        view = ed.view
        out["val"] = [view.arrays(False)[3], view.arrays(True)[3]]
        agg = out["agg"] = ops.aggregate(view, x)
        gagg = out["gagg"] = ops.aggregate(view, cot, transposed=True)
        xa, ga = ops.absmax(x), ops.absmax(cot)
        for precision in ("split", "fp32"):
            mul = view.weight_bound(False)
            out["layer", precision] = ops.transform_fwd(agg, x, weight, root, bias, relu=True, graph=view, amax=(xa, xa),
                                                        amax_mul=mul, precision=precision)
            out["grad_x", precision] = ops.transform_bwd_input(gagg, cot, weight, root, graph=view, amax=(ga, ga),
                                                               amax_mul=view.weight_bound(True), precision=precision)
            out["grad_p", precision] = ops.transform_bwd_params(agg, x, cot, r, graph=view, amax=(xa, xa, ga), amax_mul=mul,
                                                                precision=precision)
        return out

    try:
        protocol(monkeypatch, [x, cot, weight, root, bias, position, rng, cursor, stats0], fn)
    finally:
        ed.destroy()
        g.destroy()
