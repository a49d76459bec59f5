"""GPU tier: what the training path does with NaN and infinities (include/rgcn_hip.h, "Non-finite values").

Every case puts ONE poison (NaN, +inf or -inf; a few entries where a case says so) into an operand of magnitude O(1)
and compares the device's non-finite set with the two maps of tests/nonfinite_reference.py:

* every ``must`` entry (non-finite under sparse semantics) is non-finite on the device;
* no entry outside ``may`` (non-finite under dense IEEE semantics) is, and those entries meet the gate the parity test
  of that kernel and arithmetic uses (tests/test_gpu_parity.py: 2e-6 of the largest entry for the NT transforms, 5e-6
  for the parameter gradients, 3e-6 for the gathers, 1e-5 absolute for the encoder's forward; tests/test_head_edges.py:
  the operation-count bounds of the head);
* a call without a relation-occupancy mask has no empty segments: ``must == may`` and the set is exact;
* split / half arithmetic with an INFINITE operand entry: only the first rule is asserted (the lo part of an infinity
  is NaN and the tensor's scale falls back to 1); the error of the remaining finite entries is printed.

A parametrised case loops over the poison kinds, placements and operands itself and reports every failing combination
at once: the kernels are launched a few hundred times per case, each on a few hundred rows."""
import itertools

import pytest
import torch

import hub_graphs
import nonfinite_reference as NR
from conftest import need_gpu
from oracle import rgcn_oracle as O
from primekg_rgcn_linkprediction_amd import RGCNConv, ops, rgcn_encoder2, synth
from test_split_rows import _hub_graph, _typed_graph

pytestmark = pytest.mark.gpu

KINDS = list(NR.KINDS)
NT_GATE, TN_GATE, GATHER_GATE = 2e-6, 5e-6, 3e-6


# ------------------------------------------------------------------ the two-sided rule
class Report:
    """collects the failing combinations of a looping case"""

    def __init__(self):
        self.bad, self.count = [], 0

    def add(self, ok, what):
        self.count += 1
        if not ok:
            self.bad.append(what)

    def finish(self):
        assert self.count > 0
        assert not self.bad, f"{len(self.bad)} of {self.count} checks failed:\n" + "\n".join(self.bad[:40])


def nf(t):
    return ~torch.isfinite(t.detach().cpu())


def check(rep, got, ref, gate, what, only_must=False, absolute=False):
    """the rules above for one output: ``got`` (device tensor) against ``ref`` (NR.Ref)"""
    got = got.detach().cpu()
    g_nf = nf(got)
    missing = int((ref.must & ~g_nf).sum())
    rep.add(missing == 0, f"{what}: {missing} of {int(ref.must.sum())} must-be-non-finite entries are finite")
    fin = ~ref.may & ~g_nf
    err = 0.0
    if bool(fin.any()):
        scale = 1.0 if absolute else max(float(ref.value[~ref.may].abs().max()), 1e-30)
        err = float((got.double() - ref.value)[fin].abs().max()) / scale
    if only_must:
        print(f"{what}: {int((g_nf & ~ref.may).sum())} entries poisoned beyond the dense set, finite entries err by {err:.3e} (not gated)")
        return
    extra = int((g_nf & ~ref.may).sum())
    rep.add(extra == 0, f"{what}: {extra} entries are non-finite outside the dense set ({int(ref.may.sum())} entries)")
    rep.add(err <= gate, f"{what}: finite entries err by {err:.3e} > {gate:.1e}")


def check_amax(rep, buf, out, what):
    """rule 8: a published maximum is never NaN and never below the largest finite |entry|"""
    v = float(ops.amax_value(buf))
    o = out.detach().cpu()
    fin = torch.isfinite(o)
    top = float(o[fin].abs().max()) if bool(fin.any()) else 0.0
    rep.add(v == v and v >= top, f"{what}: published maximum {v} against the largest finite entry {top}")


def same_bits(rep, a, b, what):
    """two routes that are bit-identical on finite data: the same non-finite set, the same finite bits"""
    a, b = a.detach().cpu(), b.detach().cpu()
    ok = torch.equal(nf(a), nf(b)) and torch.equal(a.nan_to_num(nan=0.0, posinf=1.0, neginf=-1.0),
                                                   b.nan_to_num(nan=0.0, posinf=1.0, neginf=-1.0))
    rep.add(ok, f"{what}: the two routes differ ({int(nf(a).sum())} / {int(nf(b).sum())} non-finite entries)")


def to(dev, *ts):
    return tuple(None if t is None else t.to(dev) for t in ts)


# ------------------------------------------------------------------ dense transforms
SHAPES = [(257, 1, 8, 4), (129, 2, 20, 36), (256, 3, 64, 128), (300, 3, 128, 256)]
PRECISIONS = ["fp32", "split", "half"]


def _operands(n, r, d_in, d_out):
    gen = torch.Generator().manual_seed(n + d_in)
    return dict(agg=torch.randn(n, r * d_in, generator=gen), x=torch.randn(n, d_in, generator=gen),
                w=torch.randn(r, d_in, d_out, generator=gen) * 0.1, root=torch.randn(d_in, d_out, generator=gen) * 0.1,
                bias=torch.randn(d_out, generator=gen), g=torch.randn(n, d_out, generator=gen),
                gagg=torch.randn(n, r * d_out, generator=gen), mask=torch.randn(n, d_in, generator=gen))


def _meaning(precision, tiled, *groups):
    """the operands as the arithmetic reads them: fp32 / split keep them; "half" (on shapes the fp16 kernels tile) rounds
    each GROUP of tensors to fp16 under the group's common power-of-two scale.  -> the tensors, flattened"""
    out = []
    for group in groups:
        live = [t for t in group if t is not None]
        if precision == "half" and tiled and live:
            flat = NR.r16_scaled(torch.cat([t.reshape(-1) for t in live]))
            parts = list(torch.split(flat, [t.numel() for t in live]))
            out += [None if t is None else parts.pop(0).view(t.shape) for t in group]
        else:
            out += list(group)
    return out


def _loose(precision, tiled, kind):
    """split / half arithmetic with an infinite operand entry: only the must rule"""
    return precision != "fp32" and tiled and kind != "nan"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,r,d_in,d_out", SHAPES)
def test_transform_forward(n, r, d_in, d_out, precision):
    """``ops.transform_fwd``: poison in agg, x, one relation's weight, root or bias; ReLU on with root and bias and the
    maxima scanned, ReLU off with the maxima given and (where the poison is not in them) no root and no bias"""
    dev = need_gpu()
    base = _operands(n, r, d_in, d_out)
    tiled = d_in % 32 == 0
    rep = Report()
    for kind, placement, name in itertools.product(KINDS, NR.PLACEMENTS, ["agg", "x", "w", "root", "bias"]):
        t = dict(base)
        t[name], _ = NR.place(base[name], placement, kind, block=r - 1)
        for variant in ("relu", "plain"):
            relu = variant == "relu"
            root = t["root"] if relu or name in ("root",) else None
            bias = t["bias"] if relu or name == "bias" else None
            a, x, w, rt = _meaning(precision, tiled, [t["agg"]], [t["x"]], [t["w"], root])
            ref = NR.transform_fwd(a, x, w, rt, bias, relu)
            if name == "x" and root is None:
                assert not bool(ref.may.any())                    # without a root the layer never reads x
            A, X, W, Rt, B = to(dev, t["agg"], t["x"], t["w"], root, bias)
            amax = None if relu or precision == "fp32" else (ops.absmax(A), ops.absmax(X))
            buf = ops.amax_buffer(dev)[0]
            got = ops.transform_fwd(A, X, W, Rt, B, relu=relu, precision=precision, amax=amax, amax_out=buf)
            what = f"forward {variant} {kind} {placement} in {name}"
            check(rep, got, ref, NT_GATE, what, only_must=_loose(precision, tiled, kind))
            check_amax(rep, buf, got, what)
            if amax is not None:
                same_bits(rep, got, ops.transform_fwd(A, X, W, Rt, B, relu=relu, precision=precision), what + " (given / scanned maxima)")
    rep.finish()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,r,d_in,d_out", SHAPES)
def test_transform_input_gradient(n, r, d_in, d_out, precision):
    """``ops.transform_bwd_input``: poison in gagg, g, one relation's weight or root; with the mask (one mask entry NaN) a
    dropped position is exactly 0 whatever the cotangent holds"""
    dev = need_gpu()
    base = _operands(n, r, d_in, d_out)
    base["mask"][1, 1] = float("nan")
    tiled = d_out % 32 == 0
    rep = Report()
    for kind, placement, name in itertools.product(KINDS, NR.PLACEMENTS, ["gagg", "g", "w", "root"]):
        t = dict(base)
        t[name], idx = NR.place(base[name], placement, kind, block=r - 1)
        for variant in ("mask", "plain"):
            masked = variant == "mask"
            root = t["root"] if masked or name == "root" else None
            mask = t["mask"] if masked else None
            ga, g, w, rt = _meaning(precision, tiled, [t["gagg"]], [t["g"]], [t["w"], root])
            ref = NR.transform_bwd_input(ga, g, w, rt, mask)
            GA, G, W, Rt, M = to(dev, t["gagg"], t["g"], t["w"], root, mask)
            amax = None if masked or precision == "fp32" else (ops.absmax(GA), ops.absmax(G))
            buf = ops.amax_buffer(dev)[0]
            got = ops.transform_bwd_input(GA, G, W, Rt, relu_mask=M, precision=precision, amax=amax, amax_out=buf)
            what = f"input gradient {variant} {kind} {placement} in {name}"
            check(rep, got, ref, NT_GATE, what, only_must=_loose(precision, tiled, kind))
            check_amax(rep, buf, got, what)
            if masked:
                dropped = ~(mask > 0)
                rep.add(bool((got.cpu()[dropped] == 0).all()), what + ": a dropped position is not exactly 0")
                if name in ("gagg", "g"):                           # the poisoned cotangent row does hold dropped positions
                    assert bool(dropped[idx[0]].any()) and bool(ref.may[idx[0]].any())
            if amax is not None:
                same_bits(rep, got, ops.transform_bwd_input(GA, G, W, Rt, precision=precision), what + " (given / scanned maxima)")
    rep.finish()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,r,d_in,d_out", SHAPES)
def test_transform_parameter_gradients(n, r, d_in, d_out, precision):
    """``ops.transform_bwd_params``: poison in agg, x or g; weight, root and bias (column sums) gradients"""
    dev = need_gpu()
    base = _operands(n, r, d_in, d_out)
    tiled = d_in % 64 == 0
    rep = Report()
    for kind, placement, name in itertools.product(KINDS, NR.PLACEMENTS, ["agg", "x", "g"]):
        t = dict(base)
        t[name], _ = NR.place(base[name], placement, kind)
        a, x, g = _meaning(precision, tiled, [t["agg"]], [t["x"]], [t["g"]])
        gw, gr, _ = NR.transform_bwd_params(a, x, g, r)
        gb = NR.transform_bwd_params(a, x, t["g"], r)[2]            # the column sums stay fp32
        A, X, G = to(dev, t["agg"], t["x"], t["g"])
        loose = _loose(precision, tiled, kind)
        for given in (False, True):
            amax = (ops.absmax(A), ops.absmax(X), ops.absmax(G)) if given and precision != "fp32" else None
            got = ops.transform_bwd_params(A, X, G, r, precision=precision, amax=amax)
            what = f"parameter gradients {kind} {placement} in {name}" + (" (given maxima)" if given else "")
            check(rep, got[0], gw, TN_GATE, what + ": weight", only_must=loose)
            check(rep, got[1], gr, TN_GATE, what + ": root", only_must=loose)
            check(rep, got[2], gb, TN_GATE, what + ": bias")
        only_w = ops.transform_bwd_params(A, X, G, r, want_root=False, want_bias=False, precision=precision)
        rep.add(only_w[1] is None and only_w[2] is None, "absent gradients are None")
        check(rep, only_w[0], gw, TN_GATE, f"weight gradient alone {kind} {placement} in {name}", only_must=loose)
    rep.finish()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_parameter_gradients_of_a_row_split_without_a_relation(precision):
    """the typed graph of test_split_rows: rows [0, 150) of 200 have relation 1 only, so their relation-0 and -2 blocks
    of the aggregate are empty segments.  A poisoned cotangent row there makes those blocks' weight gradients non-finite
    under dense semantics and leaves them alone under sparse semantics: with the relation-occupancy mask the device may
    do either (a tile mask skips whole 32-row tiles), without it the dense set is exact."""
    dev = need_gpu()
    n, free, r, d_in, d_out = 200, 150, 3, 64, 64
    ei, et = _typed_graph(n, free, n)
    graph = ops.bucket(ei.to(dev), et.to(dev), n, r)
    gen = torch.Generator().manual_seed(n)
    x, g0 = torch.randn(n, d_in, generator=gen), torch.randn(n, d_out, generator=gen)
    agg = ops.aggregate(graph, x.to(dev))
    nonempty = NR.nonempty_segments(ei, et, n, r)
    assert not bool(nonempty[:free, 0].any()) and not bool(nonempty[:free, 2].any())
    rep = Report()
    for kind, row in itertools.product(KINDS, [10, 140, 199]):     # a tile without the relation, a mixed tile, a full row
        g = g0.clone()
        g[row, 5] = NR.KINDS[kind]
        a, xx, gg = _meaning(precision, True, [agg.cpu()], [x], [g])
        dense = NR.transform_bwd_params(a, xx, gg, r)
        sparse = NR.transform_bwd_params(a, xx, gg, r, nonempty)
        gb = NR.transform_bwd_params(a, xx, g, r)[2]
        if row < free:
            assert not torch.equal(sparse[0].must, sparse[0].may) and not bool(sparse[0].must[0].any())
        G = g.to(dev)
        loose = _loose(precision, True, kind)
        for masked, refs in ((True, sparse), (False, dense)):
            got = ops.transform_bwd_params(agg, x.to(dev), G, r, graph=graph if masked else None, precision=precision)
            what = f"{'masked' if masked else 'dense'} parameter gradients, {kind} in cotangent row {row}"
            check(rep, got[0], refs[0], TN_GATE, what + ": weight", only_must=loose)
            check(rep, got[1], refs[1], TN_GATE, what + ": root", only_must=loose)
            check(rep, got[2], gb, TN_GATE, what + ": bias")
    rep.finish()


@pytest.mark.parametrize("n,r,d_in,d_out", [(256, 3, 64, 128), (300, 3, 128, 256), (129, 2, 32, 64)])
def test_transform_first(n, r, d_in, d_out):
    """``ops.transform_first`` (split precision): ``T = g @ [W_r^T ... | root^T]`` with poison in g, a weight or root"""
    dev = need_gpu()
    base = _operands(n, r, d_in, d_out)
    rep = Report()
    for kind, placement, name in itertools.product(KINDS, NR.PLACEMENTS, ["g", "w", "root"]):
        t = dict(base)
        t[name], _ = NR.place(base[name], placement, kind, block=r - 1)
        for has_root in ((True,) if name == "root" else (True, False)):
            root = t["root"] if has_root else None
            ref = NR.transform_first(t["g"], t["w"], root)
            G, W, Rt = to(dev, t["g"], t["w"], root)
            got = ops.transform_first(G, ops.split_weights(W, Rt), ops.absmax(G), precision="split")
            check(rep, got, ref, NT_GATE, f"transform-first {kind} {placement} in {name}, root {has_root}", only_must=kind != "nan")
    rep.finish()


@pytest.mark.parametrize("n", [256, 300])
def test_chained_input_gradient(n):
    """``ops.transform_bwd_input_chain`` (conv2 128 -> 128 over conv1 64 -> 128): gz is the two-launch gz, same non-finite
    set and same finite bits; T against ``gz @ W1cat^T`` of the device's own gz"""
    dev = need_gpu()
    r, hidden, d_in1, d_out2 = 3, 128, 64, 128
    gen = torch.Generator().manual_seed(n)
    base = dict(w=torch.randn(r, hidden, d_out2, generator=gen) * 0.1, root=torch.randn(hidden, d_out2, generator=gen) * 0.1,
                g=torch.randn(n, d_out2, generator=gen), gagg=torch.randn(n, r * d_out2, generator=gen))
    w1, rt1 = torch.randn(r, d_in1, hidden, generator=gen) * 0.1, torch.randn(d_in1, hidden, generator=gen) * 0.1
    mask = torch.randn(n, hidden, generator=gen)
    W1, Rt1, M = to(dev, w1, rt1, mask)
    rep = Report()
    for kind, placement, name in itertools.product(KINDS, NR.PLACEMENTS, ["gagg", "g", "w", "root"]):
        t = dict(base)
        t[name], _ = NR.place(base[name], placement, kind, block=1)
        GA, G, W, Rt = to(dev, t["gagg"], t["g"], t["w"], t["root"])
        pk2, pk1 = ops.split_weights_many([(W, Rt), (W1, Rt1)])
        assert ops.chain_supported(W, W1)
        amax = (ops.absmax(GA), ops.absmax(G))
        za, zb = ops.amax_buffer(dev, 2)
        want_gz = ops.transform_bwd_input(GA, G, W, Rt, relu_mask=M, amax=amax, amax_out=za, packed=pk2, precision="split")
        gz, tt = ops.transform_bwd_input_chain(GA, G, W, Rt, M, pk2, pk1, amax=amax, amax_out=zb)
        what = f"chain {kind} {placement} in {name}"
        same_bits(rep, gz, want_gz, what + ": gz")
        check(rep, gz, NR.transform_bwd_input(t["gagg"], t["g"], t["w"], t["root"], mask), NT_GATE, what + ": gz", only_must=kind != "nan")
        check_amax(rep, zb, gz, what)
        rep.add(bool((gz.cpu()[~(mask > 0)] == 0).all()), what + ": a dropped position is not exactly 0")
        loose = bool(torch.isinf(gz).any())
        check(rep, tt, NR.transform_first(gz.cpu(), w1, rt1), NT_GATE, what + ": T", only_must=loose)
    rep.finish()


# ------------------------------------------------------------------ gathers
GATHER_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 5000]          # one pack, more packs (workspace rows), one hub


def _gather_edges(seed):
    """(key, other, rel) over hub_graphs' 64 nodes x 2 relations: segments of the lengths above, the rest empty"""
    n, r = hub_graphs.N, hub_graphs.R
    lens = torch.zeros(n * r, dtype=torch.int64)
    for i, length in enumerate(GATHER_LENGTHS):
        lens[7 * i + 3] = length                                    # both relations, both 32-row tiles
    gen = torch.Generator().manual_seed(seed)
    seg = torch.repeat_interleave(torch.arange(n * r), lens)
    other = torch.randint(0, n, (seg.numel(),), generator=gen)
    other[seg == 7 * 1 + 3] = 9                                     # the one-edge segment reads the poisoned row
    other[(seg == 7 * 3 + 3) | (seg == 7 * 4 + 3)] %= 8             # ... and two segments never do
    order = torch.randperm(seg.numel(), generator=gen)
    return lens, (seg // r)[order].contiguous(), other[order].contiguous(), (seg % r)[order].contiguous()


@pytest.mark.parametrize("half_table", [False, True])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("d", [8, 64, 264])
def test_gather(d, transposed, half_table):
    """``ops.aggregate``: one poisoned entry - or four adjacent ones, a whole 16-byte lane - in row 9 of the table.  The
    non-finite set is exactly (segments with an edge to row 9) x (the poisoned columns), empty segments are exact zeros,
    the published maximum keeps rule 8"""
    dev = need_gpu()
    n, r = hub_graphs.N, hub_graphs.R
    lens, key, other, rel = _gather_edges(d)
    assert hub_graphs.plan_partials(lens) > 0 and hub_graphs.plan_levels(lens) == 2      # the hub goes through the workspace
    ei = torch.stack([key, other]) if transposed else torch.stack([other, key])
    graph = ops.BucketedGraph(ei.to(dev), rel.to(dev), n, r)
    table = torch.randn(n, d, generator=torch.Generator().manual_seed(d))
    rep = Report()
    for kind, cols in itertools.product(KINDS, [(d // 2,), (0,), (d - 1,), tuple(range(4, 8))]):
        x = table.clone()
        x[9, list(cols)] = NR.KINDS[kind]
        xd = x.to(dev).half() if half_table else x.to(dev)
        seen = xd.float().cpu()
        want = NR.graph_aggregate(seen, ei, rel, n, r, transposed)
        hit = torch.zeros(n * r, dtype=torch.bool)
        hit[(key * r + rel)[other == 9]] = True
        colmap = torch.zeros(d, dtype=torch.bool)
        colmap[list(cols)] = True
        exact = (hit.view(-1, 1) & colmap.view(1, -1)).view(n, r * d)
        assert torch.equal(NR.nonfinite(want), exact) and 0 < int(hit.sum()) < int((lens > 0).sum())
        buf = None if half_table else ops.amax_buffer(dev)[0]
        got = ops.aggregate(graph, xd, transposed=transposed, amax_out=buf)
        what = f"gather {kind} in columns {cols}"
        check(rep, got, NR.Ref(want, exact, exact), GATHER_GATE, what)
        rep.add(bool((got.cpu().view(n * r, d)[lens == 0] == 0).all()), what + ": an empty segment is not exactly zero")
        if buf is not None:
            check_amax(rep, buf, got, what)
    rep.finish()


# ------------------------------------------------------------------ fused layers and the deferred hub path
@pytest.mark.parametrize("d_in,d_out", [(64, 128), (128, 128)])
def test_fused_layers_and_deferred_hubs_agree_with_gather_then_transform(d_in, d_out):
    """n = 1000 with one 301-edge hub segment in both directions (test_split_rows._hub_graph): the one-kernel layer, the
    one-kernel input gradient and the transforms that finish the hub rows themselves are bit-identical to gather ->
    transform on finite data and must agree with it on which entries are non-finite"""
    dev = need_gpu()
    n, r = 1000, 3
    ei, et = _hub_graph(n, n)
    graph = ops.bucket(ei.to(dev), et.to(dev), n, r)
    gen = torch.Generator().manual_seed(d_in + d_out)
    x0, g0 = torch.randn(n, d_in, generator=gen), torch.randn(n, d_out, generator=gen)
    w, root = torch.randn(r, d_in, d_out, generator=gen) * 0.1, torch.randn(d_in, d_out, generator=gen) * 0.1
    bias, mask = torch.randn(d_out, generator=gen), torch.randn(n, d_in, generator=gen)
    W, Rt, B, M = to(dev, w, root, bias, mask)
    packed = ops.split_weights(W, Rt)
    hub_src, hub_dst = 0, int(ei[1][-1])
    rep = Report()
    for kind, row in itertools.product(KINDS, [hub_src, hub_dst, 500, n - 1]):
        x, g = x0.clone(), g0.clone()
        x[row, d_in // 2] = g[row, d_out // 2] = NR.KINDS[kind]
        X, G = to(dev, x, g)
        x_amax, g_amax = ops.absmax(X), ops.absmax(G)
        what = f"{kind} in row {row}"
        # forward
        agg = ops.aggregate(graph, X)
        want = ops.transform_fwd(agg, X, W, Rt, B, relu=True, graph=graph, amax=(x_amax, x_amax), packed=packed, precision="split")
        za, zb = ops.amax_buffer(dev, 2)
        agg_out = torch.empty_like(agg)
        got = ops.layer_fwd_fused(graph, X, packed, B, True, x_amax, amax_out=za, inline_limit=16, agg_out=agg_out)
        same_bits(rep, got, want, what + ": fused forward")
        same_bits(rep, agg_out, agg, what + ": aggregate stored by the fused forward")
        check_amax(rep, za, got, what + ": fused forward")
        a, hubs = ops.aggregate_deferred(graph, X)
        assert hubs is not None
        got = ops.transform_fwd(a, X, W, Rt, B, relu=True, graph=graph, amax=(x_amax, x_amax), packed=packed, hubs=hubs, precision="split")
        same_bits(rep, got, want, what + ": forward with deferred hubs")
        same_bits(rep, a, agg, what + ": aggregate completed by the transform")
        ref = NR.transform_fwd(NR.graph_aggregate(x, ei, et, n, r), x, w, root, bias, True, NR.nonempty_segments(ei, et, n, r))
        check(rep, want, ref, NT_GATE, what + ": gather-then-transform forward", only_must=kind != "nan")
        # input gradient: the sums scaled by their own maximum
        ga_amax = ops.amax_buffer(dev)[0]
        gagg = ops.aggregate(graph, G, transposed=True, amax_out=ga_amax)
        want = ops.transform_bwd_input(gagg, G, W, Rt, relu_mask=M, graph=graph, amax=(ga_amax, g_amax), packed=packed, precision="split")
        got = ops.layer_bwd_input_fused(graph, G, packed, M, g_amax, amax_out=zb, inline_limit=16, gagg_amax=ops.amax_buffer(dev)[0])
        same_bits(rep, got, want, what + ": fused input gradient")
        check_amax(rep, zb, got, what + ": fused input gradient")
        rep.add(bool((got.cpu()[~(mask > 0)] == 0).all()), what + ": a dropped position of the fused input gradient is not exactly 0")
        if d_out in (64, 128) and d_in <= 128:
            bound = ops.transform_bwd_input(gagg, G, W, Rt, relu_mask=M, graph=graph, amax=(g_amax, g_amax),
                                            amax_mul=graph.weight_bound(True), packed=packed, precision="split")
            a, hubs = ops.aggregate_deferred(graph, G, transposed=True)
            assert hubs is not None
            got = ops.transform_bwd_input(a, G, W, Rt, relu_mask=M, graph=graph, amax=(g_amax, g_amax),
                                          amax_mul=graph.weight_bound(True), packed=packed, hubs=hubs, precision="split")
            same_bits(rep, got, bound, what + ": input gradient with deferred hubs")
        ref = NR.transform_bwd_input(NR.graph_aggregate(g, ei, et, n, r, True), g, w, root, mask,
                                     nonempty=NR.nonempty_segments(ei, et, n, r, True))
        check(rep, want, ref, NT_GATE, what + ": gather-then-transform input gradient", only_must=kind != "nan")
    rep.finish()


# ------------------------------------------------------------------ basis composition
def test_basis_composition_forward_and_backward():
    """R = 5, B = 2: one NaN (and one infinity) in ``comp`` and in a basis; plain fp32 arithmetic, so the dense set exactly"""
    dev = need_gpu()
    gen = torch.Generator().manual_seed(52)
    comp0, basis0 = torch.randn(5, 2, generator=gen), torch.randn(2, 64, 128, generator=gen) * 0.1
    gw = torch.randn(5, 64, 128, generator=gen)
    rep = Report()
    for kind, name, placement in itertools.product(KINDS, ["comp", "basis"], ["first_row", "last_col", "interior_row"]):
        comp, basis = comp0, basis0
        if name == "comp":
            comp, _ = NR.place(comp0, placement, kind)
        else:
            basis, _ = NR.place(basis0, placement, kind, block=1)
        C, Bs, GW = to(dev, comp, basis, gw)
        what = f"basis {kind} {placement} in {name}"
        check(rep, ops.basis_compose(C, Bs), NR.basis_compose(comp, basis), 2e-6, what + ": weights")
        gc, gb = ops.basis_compose_bwd(GW, C, Bs)
        rc, rb = NR.basis_compose_bwd(gw, comp, basis)
        check(rep, gc, rc, 1e-5, what + ": grad_comp")
        check(rep, gb, rb, 2e-6, what + ": grad_basis")
    rep.finish()


# ------------------------------------------------------------------ the encoder as a whole
ENC_NODES = (0, 845, 999)
_ENC = {}


def _encoder_fixture():
    """the graph, the parameters and, per poison site, the CPU references - computed once.  The reference's poisoned
    share of output rows must lie between 2 % and 50 % (a two-hop walk over the out-edges), so that neither "nothing is
    poisoned" nor "everything is" can pass the forward assertion."""
    if _ENC:
        return _ENC
    ei, et, n, r = synth.uniform_graph(1000, 8000, 3, seed=1)
    torch.manual_seed(0)
    emb = torch.nn.init.xavier_uniform_(torch.empty(n, 64))
    convs = [RGCNConv(64, 128, r), RGCNConv(128, 128, r)]
    for c in convs:
        c.bias.data.uniform_(-0.1, 0.1)
    state = [{k: v.detach().clone() for k, v in c.named_parameters()} for c in convs]
    cot = torch.randn(n, 128)
    sites = {}
    for node in ENC_NODES:
        e = emb.clone()
        e[node, 17] = float("nan")
        with torch.no_grad():
            rows = nf(O.encoder_ref(e, state[0], state[1], ei, et)).any(1)
        reach = torch.zeros(n, dtype=torch.bool)
        reach[node] = True
        for _ in range(2):                                           # two hops along the out-edges
            step = reach.clone()
            step[ei[1][reach[ei[0]]]] = True
            reach = step
        assert torch.equal(rows, reach)
        share = float(rows.float().mean())
        assert 0.02 <= share <= 0.50, f"node {node}: {share:.3f} of the reference's output rows are poisoned"
        sites[f"emb_row_{node}"] = (e, state[0], rows)
    w1 = dict(state[0])
    w1["weight"] = state[0]["weight"].clone()
    w1["weight"][1, 40, 77] = float("nan")
    sites["conv1_weight_1"] = (emb, w1, None)
    _ENC.update(ei=ei, et=et, n=n, r=r, state=state, cot=cot, sites=sites)
    return _ENC


def _policy(monkeypatch, policy, precision):
    from primekg_rgcn_linkprediction_amd import conv as C
    if policy != "default":
        monkeypatch.setattr(C, "_TRAIN_FUSED", "1" if policy == "fused" else "0")
    monkeypatch.setattr(ops, "GEMM_PRECISION", "fp32" if precision == "fp32" else "split")
    return torch.float16 if precision == "fp16-gather" else None


@pytest.mark.parametrize("site", [f"emb_row_{i}" for i in ENC_NODES] + ["conv1_weight_1"])
@pytest.mark.parametrize("precision", ["fp32", "split", "fp16-gather"])
@pytest.mark.parametrize("policy", ["default", "fused", "plain"])
def test_encoder_forward_and_backward(policy, precision, site, monkeypatch):
    """``rgcn_encoder2`` 64 -> 128 (ReLU) -> 128 on ``synth.uniform_graph(1000, 8000, 3, seed=1)`` with one NaN in an
    embedding row or in ``conv1.weight[1]``.  Forward: for an embedding NaN the device's non-finite output rows are
    exactly those of ``O.encoder_ref`` on the CPU; for the weight NaN the two-sided rule; finite entries within 1e-5
    of ``O.encoder_explicit_f64`` (for the fp16 tables: of its exact meaning).  Backward with a finite cotangent: the
    non-finite set of ``emb.grad`` and of every parameter gradient contains the must set and lies inside the may set
    (``O.encoder_explicit_f64`` with the device's ReLU decisions; the must set from tests/nonfinite_reference.py)."""
    dev = need_gpu()
    fx = _encoder_fixture()
    gather_dtype = _policy(monkeypatch, policy, precision)
    ei, et, n, r, cot = fx["ei"], fx["et"], fx["n"], fx["r"], fx["cot"]
    emb, c1, rows = fx["sites"][site]
    c2 = fx["state"][1]
    convs = [RGCNConv(64, 128, r, gather_dtype=gather_dtype).to(dev), RGCNConv(128, 128, r, gather_dtype=gather_dtype).to(dev)]
    for c, st in zip(convs, (c1, c2)):
        with torch.no_grad():
            for k, v in c.named_parameters():
                v.copy_(st[k])
    eid, etd = ei.to(dev), et.to(dev)
    e_gpu = emb.to(dev).requires_grad_(True)
    out = rgcn_encoder2(e_gpu, eid, etd, convs[0], convs[1])
    out.backward(cot.to(dev))
    with torch.no_grad():
        h_dev = convs[0](emb.to(dev), eid, etd, activation="relu").cpu()
    mask = h_dev > 0                                                 # a NaN activation passes no gradient
    half = precision == "fp16-gather"
    f64 = O.encoder_explicit_f64(emb, c1, c2, ei, et, cot, relu_mask=mask, half_forward=half, half_backward=half)
    maps = NR.encoder(emb, c1, c2, ei, et, cot, mask)
    assert torch.equal(maps["out"].may, NR.nonfinite(f64["out"]))
    rep = Report()
    if rows is not None:
        got_rows = nf(out).any(1)
        rep.add(torch.equal(got_rows, rows), f"forward: {int(got_rows.sum())} non-finite output rows on the device, "
                                             f"{int(rows.sum())} in the CPU oracle")
        rep.add(torch.equal(nf(out), maps["out"].may), "forward: the non-finite set is not the reference's")
        rep.add(torch.equal(nf(h_dev), maps["h"].may), "hidden layer: the non-finite set is not the reference's")
    check(rep, out, NR.Ref(f64["out"], maps["out"].must, maps["out"].may), 1e-5, "forward", absolute=True)
    grads = {"emb": e_gpu.grad}
    for name, c in zip(("conv1", "conv2"), convs):
        grads.update({f"{name}.{k}": v.grad for k, v in c.named_parameters()})
    for k, got in grads.items():
        assert torch.equal(maps[k].may, NR.nonfinite(f64["grads"][k])), k
        g_nf = nf(got)
        rep.add(not bool((maps[k].must & ~g_nf).any()), f"gradient {k}: {int((maps[k].must & ~g_nf).sum())} must entries are finite")
        rep.add(not bool((g_nf & ~maps[k].may).any()), f"gradient {k}: {int((g_nf & ~maps[k].may).sum())} entries non-finite outside the may set")
    rep.finish()


# ------------------------------------------------------------------ the head
def _head_case(batch, site, kind):
    gen = torch.Generator().manual_seed(100 + batch)
    n, r, d = 50, 3, 64
    ent, rel = torch.randn(n, d, generator=gen), torch.randn(r, d, generator=gen)
    hi, ti = torch.randint(1, n - 1, (batch,), generator=gen), torch.randint(1, n - 1, (batch,), generator=gen)
    ri = torch.randint(0, r, (batch,), generator=gen)
    labels = (torch.rand(batch, generator=gen) > 0.5).float()
    if site == "twice":                                              # an embedding row the batch uses twice
        hi[0] = 20
        ti[-1] = 20
        ent[20, 33] = NR.KINDS[kind]
    elif site == "relation":
        rel[int(ri[0]), 5] = NR.KINDS[kind]
    else:                                                            # a row the batch never touches (ids run 1 .. n - 2)
        ent[0, 7] = NR.KINDS[kind]
    return ent, rel, hi, ti, ri, labels


@pytest.mark.parametrize("site", ["twice", "relation", "untouched"])
@pytest.mark.parametrize("batch", [1, 7, 200])
def test_head_through_link_predictor(batch, site):
    """``LinkPredictor.score_triples`` / ``bce_loss`` and their backward (distmult_fwd, distmult_bce_fwd,
    distmult_bce_reduce, distmult_bce_bwd, distmult_bwd), d = 64: entry by entry against float64 - the same non-finite
    set, the finite entries within the bounds of tests/test_head_edges.py; the loss is non-finite exactly when a score of
    the batch is; poison in a row the batch never touches changes no bit"""
    from primekg_rgcn_linkprediction_amd import LinkPredictor
    from test_head_edges import U, _want_grads
    dev = need_gpu()
    d = 64
    rep = Report()
    for kind in KINDS:
        ent, rel, hi, ti, ri, labels = _head_case(batch, site, kind)
        head = LinkPredictor(3, d).to(dev)
        with torch.no_grad():
            head.relation_embeddings.weight.copy_(rel)
        E = ent.to(dev).requires_grad_(True)
        HI, TI, RI, LB = to(dev, hi, ti, ri, labels)
        what = f"head {kind} {site} B={batch}"
        s64, mag = NR.distmult_scores(ent, hi, ent, ti, rel, ri)
        # scores and their backward for a given cotangent
        scores = head.score_triples(E, HI, TI, RI)
        gs = torch.randn(batch, generator=torch.Generator().manual_seed(batch))
        scores.backward(gs.to(dev))
        got = scores.detach().cpu()
        rep.add(torch.equal(nf(got), NR.nonfinite(s64)), what + ": the non-finite scores are not the reference's")
        fin = torch.isfinite(s64)
        rep.add(bool(((got.double() - s64).abs()[fin] <= ((d + 2) * U * mag)[fin]).all()), what + ": finite scores over the bound")

        def grads_ok(tag, g_ent, g_rel, coef, slack):
            wh, wt, wr = _want_grads(coef, ent, hi, ent, ti, rel, ri, True, slack)
            for name, g, want in (("entity", g_ent, wh), ("relation", g_rel, wr)):
                g = g.detach().cpu()
                w_nf = NR.nonfinite(want.value)
                rep.add(torch.equal(nf(g), w_nf), f"{what}: {tag} {name} gradient: {int(nf(g).sum())} non-finite entries, reference {int(w_nf.sum())}")
                gate = want.slack + (want.n + 2).double().view(-1, 1) * U * want.mag
                ok = ((g.double() - want.value).abs() <= gate) | w_nf
                rep.add(bool(ok.all()), f"{what}: {tag} {name} gradient over the bound")
                rep.add(bool((g[want.n == 0] == 0).all()), f"{what}: {tag} {name} gradient: a row without a term is not zero")

        grads_ok("distmult", E.grad, head.relation_embeddings.weight.grad, gs, None)
        # the fused criterion
        E.grad = None
        head.relation_embeddings.weight.grad = None
        loss, scores2 = head.bce_loss(E, HI, TI, RI, LB)
        loss.backward()
        rep.add(torch.equal(scores2.detach().cpu().view(torch.int32), got.view(torch.int32)), what + ": bce scores differ from distmult's")
        per = NR.bce_with_logits(got, labels)
        rep.add(bool(torch.isfinite(loss).item()) == bool(torch.isfinite(s64).all()),
                what + f": loss {loss.item()} with {int(NR.nonfinite(s64).sum())} non-finite scores")
        if bool(torch.isfinite(s64).all()):
            rep.add(abs(loss.item() - float(per.mean())) <= 1e-6 * max(1.0, abs(float(per.mean()))), what + ": finite loss off")
        coef = NR.bce_coefficient(1.0, got, labels)
        grads_ok("bce", E.grad, head.relation_embeddings.weight.grad, coef, 8 * U / batch)
        if site == "untouched":                                      # ... and the poison changed no bit of anything
            clean = ent.clone()
            clean[0, 7] = 0.5
            E2 = clean.to(dev).requires_grad_(True)
            loss2, scores3 = head.bce_loss(E2, HI, TI, RI, LB)
            head.relation_embeddings.weight.grad = None
            loss2.backward()
            rep.add(torch.equal(scores3, scores2) and torch.equal(loss2, loss) and torch.equal(E2.grad, E.grad), what + ": bits moved")
    rep.finish()


@pytest.mark.parametrize("batch", [1, 7, 200])
def test_relation_row_gradient_by_segment_sum(batch):
    """``rgcn_segment_sum`` as the head uses it (the backward of ``table[idx]`` behind the relation dropout)"""
    from primekg_rgcn_linkprediction_amd.head import _RelationRows
    dev = need_gpu()
    gen = torch.Generator().manual_seed(batch)
    idx = torch.randint(0, 3, (batch,), generator=gen)
    rep = Report()
    for kind, row in itertools.product(KINDS, sorted({0, batch // 2, batch - 1})):
        g = torch.randn(batch, 64, generator=gen)
        g[row, 9] = NR.KINDS[kind]
        table = torch.randn(3, 64, generator=gen).to(dev).requires_grad_(True)
        _RelationRows.apply(table, idx.to(dev)).backward(g.to(dev))
        want = NR.segment_sum(g, idx, 3)
        check(rep, table.grad, NR.Ref(want, NR.nonfinite(want), NR.nonfinite(want)), 2e-6, f"segment sum {kind} in row {row}")
    rep.finish()


# ------------------------------------------------------------------ the optimizer
@pytest.mark.parametrize("adamw", [False, True])
@pytest.mark.parametrize("max_norm", [0.0, 1.0])
@pytest.mark.parametrize("kind", ["nan", "+inf"])
def test_clip_adam_step_has_torchs_pattern(kind, max_norm, adamw):
    """``ops.adam_clip_step`` on the tensor set of test_fused_clip_adam_equals_torch, one poisoned gradient entry in the
    first step and a finite second step: the finite / non-finite pattern of params, exp_avg and exp_avg_sq is that of
    ``clip_grad_norm_`` + ``torch.optim.Adam`` / ``AdamW`` (on the CPU), ``total_norm`` is non-finite exactly when
    torch's is, and the published parameter maxima keep rule 8"""
    dev = need_gpu()
    gen = torch.Generator().manual_seed(7)
    shapes = [(30926, 64), (3, 64, 128), (128,), (1,), (7, 3), (8193,)]
    ref = [torch.randn(s, generator=gen).requires_grad_(True) for s in shapes]
    opt = (torch.optim.AdamW if adamw else torch.optim.Adam)(ref, lr=1e-2, weight_decay=0.01)
    got = [p.detach().clone().to(dev) for p in ref]
    m, v = [torch.zeros_like(p) for p in got], [torch.zeros_like(p) for p in got]
    steps = [torch.zeros((), device=dev) for _ in got]
    norm = torch.zeros(1, device=dev)
    bufs = [ops.amax_buffer(dev)[0] if p.dim() >= 2 else None for p in got]
    rep = Report()
    for step in (1, 2):
        grads = [torch.randn(s, generator=gen) * 3.0 for s in shapes]
        if step == 1:
            grads[1][2, 63, 100] = NR.KINDS[kind]
        for p, g in zip(ref, grads):
            p.grad = g.clone()
        want_norm = torch.nn.utils.clip_grad_norm_(ref, max_norm) if max_norm > 0 else None
        opt.step()
        # (amax_out takes a buffer per tensor; tensors without one go in a call of their own, as the Trainer's do not)
        ops.adam_clip_step(got, [g.to(dev) for g in grads], m, v, steps, 1e-2, 0.9, 0.999, 1e-8, 0.01, adamw=adamw,
                           max_norm=max_norm, total_norm=norm,
                           amax_out=[b if b is not None else ops.amax_buffer(dev)[0] for b in bufs])
        if want_norm is not None:
            rep.add(bool(torch.isfinite(norm).item()) == bool(torch.isfinite(want_norm).item()),
                    f"step {step}: total_norm {norm.item()} against torch's {want_norm.item()}")
        for mine, theirs, what in ((got, [p.detach() for p in ref], "param"), (m, [opt.state[p]["exp_avg"] for p in ref], "exp_avg"),
                                   (v, [opt.state[p]["exp_avg_sq"] for p in ref], "exp_avg_sq")):
            for i, (a, b) in enumerate(zip(mine, theirs)):
                rep.add(torch.equal(nf(a), nf(b)), f"step {step}: {what}[{i}]: {int(nf(a).sum())} non-finite entries, torch {int(nf(b).sum())}")
                fin = torch.isfinite(b) & ~nf(a)
                if bool(fin.any()):
                    err = float((a.cpu() - b)[fin].abs().max())
                    rep.add(err <= 2e-6 * max(1.0, float(b[fin].abs().max())), f"step {step}: {what}[{i}] finite entries err by {err:.3e}")
        for p, b in zip(got, bufs):
            if b is not None:
                check_amax(rep, b, p, f"step {step}: parameter maximum")
    rep.finish()


# ------------------------------------------------------------------ one training step
@pytest.mark.parametrize("hip_graph", [False, True])
def test_a_nan_in_the_embedding_table_reaches_the_reported_loss(tmp_path, hip_graph):
    """``Trainer`` on 400 nodes / 6,000 edges, batch 256, no dropout, one NaN in the embedding table: the loss of the
    first (eager) step is non-finite, and so is the next one - a replay of the captured whole-step graph with
    ``hip_graph``.  Before the ReLU epilogue kept NaN the hidden layer swallowed it and both losses were finite."""
    from primekg_rgcn_linkprediction_amd import train as T
    from test_train import _args
    dev = need_gpu()
    torch.manual_seed(0)
    n, r = 400, 3
    gen = torch.Generator().manual_seed(3)
    ei, et = torch.randint(0, n, (2, 6000), generator=gen), torch.randint(0, r, (6000,), generator=gen)
    data = {"edge_index": ei, "edge_type": et, "num_nodes": n, "num_relations": r}
    args = _args(dropout=0.0, decoder_dropout=0.0, batch_size=256, output_dir=str(tmp_path), device="cuda",
                 no_hip_graph=not hip_graph)
    model = T.create_model(n, r, args)
    with torch.no_grad():
        model.state_dict()["encoder.node_embeddings.weight"][11, 3] = float("nan")
    trainer = T.Trainer(model, data, data, data, dev, args)
    losses = []
    mean_loss, _ = trainer.train_epoch(on_step=lambda h, t, rl, lb, loss: losses.append(loss.item()), max_steps=2)
    assert (trainer._graph is not None) == hip_graph
    assert len(losses) == 2 and not any(map(torch.isfinite, map(torch.tensor, losses))), losses
    assert mean_loss != mean_loss or abs(mean_loss) == float("inf")
