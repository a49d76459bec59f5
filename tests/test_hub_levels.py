"""Hub segments past 131,072 edges: gathers whose plan is THREE levels deep, bit for bit.

The gather sums a (node, relation) segment as a fixed tree - runs of 64 edges, four runs to a pack, reduce levels of
fan-in 512 (``csrc/rgcn_plan.h``) - and a third level first appears at 131,073 edges.  The boundary graph
(``hub_graphs.py``) has segments of 131,072 (largest two-level), 131,073 (smallest three-level) and 262,444 edges
(level-1 items of 512, 512 and 5 rows) beside forty short ones.  Tables of small integers make every sum exact in
fp32 IN ANY ORDER (262,444 * 8 < 2^24), so the expectation is the int64 segment sum cast to fp32 and divided in fp32
by ``max(1, len)``, and every comparison in this file is ``torch.equal`` - except where a project gate is named: the
float64 boundary gate (3e-6 of the largest entry), the transform-first gate (2e-6), the encoder's ``FWD_ATOL`` /
``GRAD_RTOL``, and the derived per-row gate of ``test_every_row_is_within_its_own_condition``."""
from types import SimpleNamespace

import pytest
import torch

import hub_graphs as H
from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import ops
from test_gpu_parity import FWD_ATOL, GRAD_RTOL, _encoder_vs_oracle, rel_err

pytestmark = pytest.mark.gpu

N, R = H.N, H.R
WIDTHS = [4, 24, 64, 128, 320]          # lanes per row G = 1, 8 (two idle), 16, 32, 64 (two column blocks)


@pytest.fixture(scope="module")
def boundary():
    dev = need_gpu()
    key, other, rel = H.boundary_edges()
    ei = torch.stack([other, key])                                   # hubs are DESTINATIONS
    g = ops.BucketedGraph(ei.to(dev), rel.to(dev), N, R)
    flip = ops.BucketedGraph(ei.flip(0).contiguous().to(dev), rel.to(dev), N, R)      # hubs are SOURCES
    b = SimpleNamespace(dev=dev, key=key, other=other, rel=rel, ei=ei, g=g, flip=flip, lens=H.segment_lengths())
    yield b
    g.destroy()
    flip.destroy()


def _int_x(d, bound=8):
    return H.int_table(d, bound, seed=d)


def test_the_boundary_graph_is_three_levels_deep_where_its_hubs_are(boundary):
    b = boundary
    assert b.ei.size(1) == int(b.lens.sum()) > 525000 and H.plan_levels(b.lens) == 3
    assert b.g.num_levels(False) == 3 and b.g.num_levels(True) == 2
    assert b.flip.num_levels(True) == 3 and b.flip.num_levels(False) == 2
    rowptr = b.g.arrays(False)[0].long().cpu()
    assert torch.equal(rowptr[1:] - rowptr[:-1], b.lens)
    rows = H.plan_partials(b.lens)
    assert rows > 512 + 515 + 1029
    for d in (4, 64, 320):                       # the workspace is exactly the plan's partial rows
        assert b.g.workspace_bytes(False, d) == b.flip.workspace_bytes(True, d) == rows * d * 4


# ----------------------------------------------------------------------------------------------- mean gather
@pytest.mark.parametrize("d", WIDTHS)
def test_mean_gather_is_the_exact_segment_mean(boundary, d):
    b = boundary
    x = _int_x(d)
    want = H.mean_expected(b.key, b.other, b.rel, x)
    xd = x.float().to(b.dev)
    got = ops.aggregate(b.g, xd)
    assert torch.equal(got.cpu(), want)
    slot = ops.amax_buffer(b.dev)[0]
    assert torch.equal(ops.aggregate(b.g, xd, amax_out=slot), got)
    assert ops.amax_value(slot).item() == want.abs().max().item() > 0
    given = torch.full((N, R * d), float("nan"), device=b.dev)
    assert ops.aggregate(b.g, xd, out=given) is given and torch.equal(given, got)
    if d in (24, 64, 320):                       # small integers are exact in fp16
        assert torch.equal(ops.aggregate(b.g, xd.half()).cpu(), want)


@pytest.mark.parametrize("d", [64, 320])
def test_levels_issued_one_at_a_time_and_a_riding_tail_change_no_bit(boundary, d, monkeypatch):
    """as ``test_gather_options_are_bit_for_bit_one_gather`` does it at two levels: measurement mode issues one call per
    level over one workspace; a pending parameter-gradient reduction rides in the level-0 launch (d = 64) or is
    launched first (d = 320)"""
    b = boundary
    x = _int_x(d)
    want = H.mean_expected(b.key, b.other, b.rel, x).to(b.dev)
    xd = x.float().to(b.dev)
    gen = torch.Generator().manual_seed(d)
    pa, px, pg = (torch.randn(N, w, generator=gen).to(b.dev) for w in (R * 64, 64, 64))

    def pending():
        return ops.transform_bwd_params(pa, px, pg, R, defer=True)
    alone = pending()
    alone.finish()

    def check(rows, tail=None, slot=None):
        assert torch.equal(rows, want)
        if tail is not None:
            assert tail.done and all(torch.equal(p, q) for p, q in zip(tail.grads, alone.grads))
        if slot is not None:
            assert ops.amax_value(slot).item() == want.abs().max().item()

    tail = pending()
    assert not tail.done
    check(ops.aggregate(b.g, xd, tail=tail), tail)
    tail, slot = pending(), ops.amax_buffer(b.dev)[0]
    check(ops.aggregate(b.g, xd, tail=tail, amax_out=slot), tail, slot)
    events = []
    monkeypatch.setattr(ops, "GATHER_EVENTS", events)
    for k, (tail, slot) in enumerate([(None, None), (pending(), None), (None, ops.amax_buffer(b.dev)[0]),
                                      (pending(), ops.amax_buffer(b.dev)[0])]):
        check(ops.aggregate(b.g, xd, tail=tail, amax_out=slot), tail, slot)
        assert len(events) == k + 1 and events[-1][:5] == (False, d, b.ei.size(1), N * R, N)
    monkeypatch.setattr(ops, "GATHER_EVENTS", None)


# ----------------------------------------------------------------------------------------------- weighted gather
@pytest.mark.parametrize("d", WIDTHS)
def test_weighted_gather_is_the_exact_weighted_sum(boundary, d):
    """weights +-{1, 1/2, 1/4, 1/8} and a table in [-4, 4]: every product and every partial sum is a multiple of 1/8
    below 2^24 units (262,444 * 4 * 8 < 2^24), so the fma chain is exact in any order"""
    b = boundary
    gen = torch.Generator().manual_seed(1000 + d)
    w8 = (2 ** torch.randint(0, 4, b.key.shape, generator=gen)) * (2 * torch.randint(0, 2, b.key.shape, generator=gen) - 1)
    shard = ops.BucketedGraph.from_shard(b.key.to(b.dev), b.other.to(b.dev), b.rel.to(b.dev), N, N, R,
                                         edge_weight=(w8.float() / 8).to(b.dev))
    assert shard.num_levels(False) == 3 and shard.workspace_bytes(False, d) == H.plan_partials(b.lens) * d * 4
    x = _int_x(d, bound=4)
    sums8 = H.segment_matrix(b.key, b.other, b.rel, weight=w8) @ x.long()
    assert int(sums8.abs().max()) < 2 ** 24
    want = (sums8.float() / 8).view(N, -1)
    got = ops.aggregate(shard, x.float().to(b.dev))
    assert torch.equal(got.cpu(), want)
    slot = ops.amax_buffer(b.dev)[0]
    assert torch.equal(ops.aggregate(shard, x.float().to(b.dev), amax_out=slot), got)
    assert ops.amax_value(slot).item() == want.abs().max().item() > 0
    if d in (24, 64, 320):
        assert torch.equal(ops.aggregate(shard, x.half().to(b.dev)).cpu(), want)
    shard.destroy()


@pytest.mark.parametrize("d", [24, 64, 320])
def test_transposed_gather_of_the_flipped_graph_is_the_weighted_gather_of_its_own_weights(boundary, d):
    """the flip's transposed structure: hub SOURCES, weights 1 / cnt[dst, rel] - no powers of two, so its exactness rests
    on the weighted gather above: the same CSR and the same plan over the same weights give the same bits; and it stays
    inside the float64 boundary gate of ``test_segment_lengths_around_run_and_pack_boundaries``"""
    b = boundary
    src, dst = b.ei.flip(0)
    _, _, perm, w_t = b.flip.arrays(True)
    w = torch.empty_like(w_t)
    w[perm] = w_t                                                    # w_t in original column order
    cnt = torch.bincount(dst * R + b.rel, minlength=N * R).clamp(min=1).float()
    assert torch.equal(w.cpu(), 1.0 / cnt[dst * R + b.rel])          # = 1 / cnt of the edge's (dst, rel), rounded once
    shard = ops.BucketedGraph.from_shard(src.to(b.dev), dst.to(b.dev), b.rel.to(b.dev), N, N, R, edge_weight=w)
    assert shard.num_levels(False) == 3
    for a, c in zip(shard.arrays(False), b.flip.arrays(True)):
        assert torch.equal(a, c)                                     # the same CSR
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(d))
    got = ops.aggregate(b.flip, x.to(b.dev), transposed=True)
    assert torch.equal(got, ops.aggregate(shard, x.to(b.dev)))
    assert torch.equal(ops.aggregate(b.flip, x.half().to(b.dev), transposed=True), ops.aggregate(shard, x.half().to(b.dev)))
    flat = (src * R + b.rel) * N + dst
    wmat = torch.zeros(N * R * N, dtype=torch.float64).index_add_(0, flat, w.cpu().double()).view(N * R, N)
    assert rel_err(got, (wmat @ x.double()).view(N, -1)) <= 3e-6
    shard.destroy()


# ----------------------------------------------------------------------------------------------- per-row float check
def test_every_row_is_within_its_own_condition(boundary):
    """a ``randn`` table at d = 64: for EVERY row |got - float64| <= gate * (sum over the segment of |x|) / cnt - the
    row's own condition, not the tensor's maximum (a hub mean of L rows is ~ 1 / sqrt(L) of the largest entry, so a gate
    on the maximum would not see one dropped partial row).  The gate is derived, not tuned: every addition and the
    division round once, 2^-24 relative each, and the longest path from an edge to its row has
        63  additions in a run of 64 edges,
         3  in a pack of four runs,
        46  per reduce level: d = 64 is G = 16 lanes per row, SLOTS = 256 / G = 16 rows in parallel, so a slot adds
            ceil(512 / 16) - 1 = 31 times and the slots are combined with 16 - 1 = 15 more,  x 2 reduce levels = 92
    = 158 additions + 1 division = 159 roundings: gate = 159 * 2^-24 = 9.48e-6."""
    b = boundary
    d, g_lanes = 64, 16
    slots = 256 // g_lanes
    per_level = -(-512 // slots) - 1 + slots - 1
    additions = 63 + 3 + (b.g.num_levels(False) - 1) * per_level
    assert (per_level, additions) == (46, 158)
    gate = (additions + 1) * 2.0 ** -24
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(7))
    counts = H.segment_matrix(b.key, b.other, b.rel).double()
    cnt = counts.sum(1, keepdim=True).clamp(min=1)
    want = (counts @ x.double()) / cnt
    cond = (counts @ x.double().abs()) / cnt
    got = ops.aggregate(b.g, x.to(b.dev)).cpu().double().view(N * R, d)
    err = (got - want).abs()
    assert bool((err <= gate * cond).all()), float((err / cond.clamp(min=1e-300)).max())
    assert torch.equal(got[b.lens == 0], torch.zeros(int((b.lens == 0).sum()), d, dtype=torch.float64))


# ----------------------------------------------------------------------------------------------- nothing is deferred
def test_three_levels_are_never_deferred_and_a_forged_deferral_is_refused(boundary):
    b = boundary
    for graph, t in ((b.g, False), (b.flip, True)):
        assert not any(graph.deferrable(t, d) for d in (64, 128, 256))
        assert all(graph.deferrable(not t, d) for d in (64, 128, 256))          # the two-level direction still is
    x = _int_x(64).float().to(b.dev)
    rows, hubs = ops.aggregate_deferred(b.g, x)
    assert hubs is None and torch.equal(rows.cpu(), H.mean_expected(b.key, b.other, b.rel, _int_x(64)))
    rows_t, hubs = ops.aggregate_deferred(b.flip, x, transposed=True)
    assert hubs is None and torch.equal(rows_t, ops.aggregate(b.flip, x, transposed=True))
    # a DeferredHubs built by hand over the three-level structure: the split transforms refuse it before any launch
    gen = torch.Generator().manual_seed(5)
    weight, root = (torch.randn(R, 64, 128, generator=gen) / 8).to(b.dev), (torch.randn(64, 128, generator=gen) / 8).to(b.dev)
    partial = torch.zeros(b.g.workspace_bytes(False, 64), dtype=torch.uint8, device=b.dev)
    xa = ops.absmax(x)
    out = torch.full((N, 128), 7.5, device=b.dev)
    with pytest.raises(ValueError):
        ops.transform_fwd(rows, x, weight, root, graph=b.g, amax=(xa, xa), precision="split", out=out,
                          hubs=ops.DeferredHubs(b.g, False, partial))
    torch.cuda.synchronize()
    assert bool((out == 7.5).all())                                             # the caller's out keeps its fill
    gagg = ops.aggregate(b.flip, torch.randn(N, 128, generator=gen).to(b.dev), transposed=True)
    partial_t = torch.zeros(b.flip.workspace_bytes(True, 128), dtype=torch.uint8, device=b.dev)
    g = torch.randn(N, 128, generator=gen).to(b.dev)
    ga = ops.absmax(g)
    with pytest.raises(ValueError):
        ops.transform_bwd_input(gagg, g, weight, root, graph=b.flip, amax=(ga, ga), amax_mul=b.flip.weight_bound(True),
                                precision="split", hubs=ops.DeferredHubs(b.flip, True, partial_t))
    ops.check_indices(b.dev)


# ----------------------------------------------------------------------------------------------- fused layers
def test_fused_layers_over_a_three_level_hub_structure_change_no_bit(boundary):
    """``layer_fwd_fused`` / ``layer_bwd_input_fused`` (64 -> 128) pre-aggregate the long segments over
    ``fused_plan().hub``, itself three levels deep where the graph is: bit-identical to gather -> split transform, as
    the fused tests assert at two levels; and ``row_blocks(32)``, whose first block holds the three-level hubs"""
    b = boundary
    d_in, d_out = 64, 128
    assert ops.fused_supported(R, d_in, d_out) and ops.fused_bwd_supported(R, d_in, d_out)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(N, d_in, generator=gen).to(b.dev)
    g = (torch.randn(N, d_out, generator=gen) * 1e-3).to(b.dev)
    weight = (torch.randn(R, d_in, d_out, generator=gen) / d_in ** 0.5).to(b.dev)
    root = (torch.randn(d_in, d_out, generator=gen) / d_in ** 0.5).to(b.dev)
    bias = torch.randn(d_out, generator=gen).to(b.dev)
    mask = torch.randn(N, d_in, generator=gen).to(b.dev)
    packed = ops.split_weights(weight, root)
    x_amax, g_amax = ops.absmax(x), ops.absmax(g)
    for graph, fwd_levels, bwd_levels in ((b.g, 3, 2), (b.flip, 2, 3)):
        assert graph.fused_plan(16).hub.num_levels(False) == fwd_levels
        assert graph.fused_plan(16, transposed=True).hub.num_levels(False) == bwd_levels
        agg = ops.aggregate(graph, x)
        want_amax, got_amax = ops.amax_buffer(b.dev), ops.amax_buffer(b.dev)
        want = ops.transform_fwd(agg, x, weight, root, bias, relu=True, graph=graph, amax=(x_amax, x_amax),
                                 amax_out=want_amax, packed=packed, precision="split")
        kept = torch.full((N, R * d_in), float("nan"), device=b.dev)
        got = ops.layer_fwd_fused(graph, x, packed, bias, True, x_amax, got_amax, inline_limit=16, agg_out=kept)
        assert torch.equal(got, want) and torch.equal(kept, agg)
        assert float(ops.amax_value(got_amax)) == float(ops.amax_value(want_amax)) == float(want.abs().max())
        gagg = ops.aggregate(graph, g, transposed=True)
        want_amax, got_amax = ops.amax_buffer(b.dev), ops.amax_buffer(b.dev)
        want = ops.transform_bwd_input(gagg, g, weight, root, relu_mask=mask, graph=graph, amax=(g_amax, g_amax),
                                       amax_mul=graph.weight_bound(True), amax_out=want_amax, packed=packed,
                                       precision="split")
        got = ops.layer_bwd_input_fused(graph, g, packed, mask, g_amax, got_amax, inline_limit=16)
        assert torch.equal(got, want)
        assert float(ops.amax_value(got_amax)) == float(ops.amax_value(want_amax)) == float(want.abs().max())
    whole = ops.aggregate(b.g, x)
    blocks = b.g.row_blocks(32)
    assert [(lo, hi) for lo, hi, _ in blocks] == [(0, 32), (32, 64)]
    assert [shard.num_levels(False) for _, _, shard in blocks] == [3, 2]
    for lo, hi, shard in blocks:
        assert torch.equal(ops.aggregate(shard, x), whole[lo:hi])


# ----------------------------------------------------------------------------------------------- merged structure
def test_merged_transposed_reaches_three_levels_before_any_single_segment():
    """a hub SOURCE with 70,000 out-edges in each of two relations: every (src, rel) segment stays at two levels, the
    merged structure - a node's out-edges over all relations plus its own row - has 140,001 and needs three; the
    transform-first input gradient (which gathers over it) against gather-first at the gate of
    ``test_transform_first_input_gradient_equals_gather_first``"""
    from primekg_rgcn_linkprediction_amd.conv import _input_grad
    dev = need_gpu()
    gen = torch.Generator().manual_seed(21)
    hub_edges = 70000
    src = torch.cat([torch.full((2 * hub_edges,), 9, dtype=torch.int64), torch.randint(0, N, (3000,), generator=gen)])
    dst = torch.randint(0, N, (src.numel(),), generator=gen)
    rel = torch.cat([torch.zeros(hub_edges, dtype=torch.int64), torch.ones(hub_edges, dtype=torch.int64),
                     torch.randint(0, R, (3000,), generator=gen)])
    order = torch.randperm(src.numel(), generator=gen)
    ei, et = torch.stack([src, dst])[:, order].contiguous(), rel[order].contiguous()
    graph = ops.BucketedGraph(ei.to(dev), et.to(dev), N, R)
    merged = graph.merged_transposed()
    assert graph.num_levels(True) == 2 and graph.num_levels(False) == 2 and merged.num_levels(False) == 3
    assert merged.num_edges == ei.size(1) + N
    d_in, d_out = 64, 256
    w = (torch.randn(R, d_in, d_out, generator=gen) * 0.1).to(dev)
    root = (torch.randn(d_in, d_out, generator=gen) * 0.1).to(dev)
    g = torch.randn(N, d_out, generator=gen).to(dev)
    first = _input_grad(graph, g, w, root)
    gather_first = ops.transform_bwd_input(ops.aggregate(graph, g, transposed=True), g, w, root, graph=graph)
    assert first.shape == (N, d_in) and rel_err(first, gather_first.cpu()) <= 2e-6
    graph.destroy()


# ----------------------------------------------------------------------------------------------- persisted form
def test_persisted_form_keeps_the_third_level_and_the_gather_bits(boundary):
    b = boundary
    x = _int_x(64).float().to(b.dev)
    for graph in (b.g, b.flip):
        again = ops.BucketedGraph.from_state(graph.state(), b.dev)
        for t in (False, True):
            assert again.num_levels(t) == graph.num_levels(t)
            assert again.workspace_bytes(t, 64) == graph.workspace_bytes(t, 64)
            assert torch.equal(ops.aggregate(again, x, transposed=t), ops.aggregate(graph, x, transposed=t))
        assert max(again.num_levels(False), again.num_levels(True)) == 3
        again.destroy()


# ----------------------------------------------------------------------------------------------- end to end
def test_encoder_on_the_boundary_graph_vs_oracle(boundary):
    """both layers, three routes, forward and every gradient at the project's own gates (``FWD_ATOL``, ``GRAD_RTOL``)"""
    b = boundary
    errs = _encoder_vs_oracle(b.dev, b.ei, b.rel, N, R, (64, 128, 128), seed=3)
    assert errs["fwd_max_abs_vs_f64"] <= FWD_ATOL and errs["grad_emb_rel_vs_f64"] <= GRAD_RTOL
    assert errs["grad_params_rel_vs_f64_max"] <= GRAD_RTOL
