"""Guard bands and poison fills around every output and workspace the library is handed (``tests/guarded.py``).

Every scenario is a closure over ``ops`` calls on seeded inputs and runs four times: plain, then with every
``ops._empty`` allocation guarded and pre-filled with 0x00, then with 0xFF, then RE-BASED: guarded (0xFF) with every
allocation AND every input starting 16 bytes past a 512-byte boundary - the smallest base the alignment contract of
``include/rgcn_hip.h`` admits, where the other runs only ever see multiples of 512.  A 16-byte move selects no other
code path anywhere, so the re-based run must give the bits of the plain run.  Asserted for each:

* bands   - every band of every allocation of both guarded runs is bit-intact (no store outside an output or
            workspace, so no ``*_workspace_bytes`` query is smaller than the kernel's footprint);
* inputs  - every input holds the bits it held before (``include/rgcn_hip.h:17``: inputs are borrowed and never written);
* outputs - every returned tensor holds the same bits in all four runs (no read of memory the call did not write, no
            assumption about the base address beyond 16 bytes);
* path    - the scenario first asserts the precondition that puts it on the kernel it is meant for.

Buffers a scenario needs besides the library's own (amax buffers, gradient tables, optimizer state) come from
``ctx.empty``, i.e. from the same allocator.  EXCEPTIONS to bit-equality - the buffers the header declares partly
written or opaque, and nothing else:

    what                         compared instead                                         rests on
    ---------------------------  -------------------------------------------------------  -------------------------------
    amax buffers                 ``ops.amax_value``; the non-head entries still hold      include/rgcn_hip.h:167-168 ("the
                                 the fill of the run                                      other entries are never touched")
    ``SplitWeights`` images      only through the transforms that consume them            include/rgcn_hip.h:276-279 (fp16
                                                                                          images in the kernels' own orders)
"""
import contextlib
import ctypes

import pytest
import torch

from conftest import need_gpu
from guarded import GuardedAllocator, bits, installed
from primekg_rgcn_linkprediction_amd import _lib, ops, synth

pytestmark = pytest.mark.gpu

PLAIN_AMAX_FILL = 0x5A        # what the non-head entries of an amax buffer hold in the plain run


class Amax:
    """an amax buffer among a scenario's outputs (first row of the exceptions table)"""

    def __init__(self, buf, own_fill=True):
        self.buf, self.own_fill = buf, own_fill        # own_fill: the scenario allocated it through ``Ctx.amax``


class Ctx:
    """what a scenario sees of the run it is in: ``fill`` (None: the plain run) and the allocator in force"""

    def __init__(self, fill):
        self.fill = fill

    def empty(self, *shape, dtype=torch.float32, device):
        return ops._empty(*shape, dtype=dtype, device=device)

    def like(self, src):
        """a copy of ``src`` in memory of this run's allocator (state a call updates in place)"""
        return self.empty(tuple(src.shape), dtype=src.dtype, device=src.device).copy_(src)

    def amax(self, device, count=1):
        """``count`` amax buffers with zeroed heads; the other entries hold the run's fill"""
        buf = self.empty(count, ops.AMAX_FLOATS, dtype=torch.float32, device=device)
        if self.fill is None:
            buf.view(-1).view(torch.uint8).fill_(PLAIN_AMAX_FILL)
        buf.view(-1)[::ops.AMAX_HEAD_STRIDE] = 0.0
        return buf.view(ops.AMAX_FLOATS) if count == 1 else buf

    def untouched(self, t):
        """do the bytes of ``t`` (memory of this run's allocator nobody may write) still hold the fill?"""
        fill = PLAIN_AMAX_FILL if self.fill is None else self.fill
        return bool((t.contiguous().view(-1).view(torch.uint8) == fill).all())


def _flatten(out, into, path="out"):
    if out is None:
        return into
    if isinstance(out, (torch.Tensor, Amax)):
        into.append((path, out))
    elif isinstance(out, dict):
        for k, v in out.items():
            _flatten(v, into, f"{path}[{k!r}]")
    else:
        for i, v in enumerate(out):
            _flatten(v, into, f"{path}[{i}]")
    return into


def _snapshot(ctx, out):
    """[(path, kind, bit pattern)] of a run's outputs; the amax exception is applied here"""
    snap = []
    for path, t in _flatten(out, []):
        if isinstance(t, Amax):
            if ctx.fill is not None or t.own_fill:
                assert ctx.untouched(t.buf.view(-1, ops.AMAX_HEAD_STRIDE)[:, 1:]), \
                    f"{path}: a non-head entry of an amax buffer was written (include/rgcn_hip.h:168)"
            snap.append((path, "amax", bits(ops.amax_value(t.buf).reshape(1))))
        else:
            snap.append((path, str(t.dtype) + str(tuple(t.shape)), bits(t)))
    return snap


def library_amax(buf):
    """an amax buffer the LIBRARY allocated (``absmax(out=None)``): in the plain run its non-head entries hold whatever
    ``torch.empty`` returned, so only the guarded runs can look at them"""
    return Amax(buf, own_fill=False)


REBASE_OFFSET = 16            # bytes past a 512-byte boundary: the smallest base a 16-byte operand may have


@contextlib.contextmanager
def rebased(inputs, offset=REBASE_OFFSET):
    """for the body, every tensor of ``inputs`` lives on a copy of its bits that starts ``offset`` bytes past a 512-byte
    boundary (same shape, strides and dtype; the tensor OBJECTS are the same, so closures and the objects that hold them
    need not know); put back afterwards, whatever happened"""
    done = []                             # (tensor, an alias of what it was)
    try:
        for t in inputs:
            if t.numel() == 0 or any(t is u for u, _ in done):
                continue
            span = 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride()))        # elements from the first to the last
            raw = torch.empty(512 + span * t.element_size(), dtype=torch.uint8, device=t.device)
            assert raw.data_ptr() % 512 == 0
            moved = raw[offset:offset + span * t.element_size()].view(t.dtype).as_strided(tuple(t.shape), t.stride())
            moved.copy_(t)
            old = t.detach()              # keeps the original storage alive and remembers the view
            with torch.no_grad():
                t.set_(moved)
            done.append((t, old))
            assert t.data_ptr() % 512 == offset and t.stride() == old.stride() and t.shape == old.shape
        yield
    finally:
        with torch.no_grad():
            for t, old in reversed(done):
                t.set_(old)


def protocol(monkeypatch, inputs, fn):
    """plain / guarded 0x00 / guarded 0xFF / re-based; ``inputs``: every tensor the closure only reads"""
    inputs = [t for t in inputs if t is not None]
    before = [bits(t) for t in inputs]
    homes = [t.data_ptr() for t in inputs]
    torch.cuda.synchronize()
    ctx = Ctx(None)
    runs = [("plain", _snapshot(ctx, fn(ctx)))]
    for fill, offset in ((0x00, 0), (0xFF, 0), (0xFF, REBASE_OFFSET)):
        alloc, ctx = GuardedAllocator(fill, payload_offset=offset), Ctx(fill)
        with contextlib.ExitStack() as stack:
            if offset:
                stack.enter_context(rebased(inputs, offset))
                torch.cuda.synchronize()
            with installed(monkeypatch, alloc):
                out = fn(ctx)
                torch.cuda.synchronize()
                snap = _snapshot(ctx, out)
            assert alloc.records, "the scenario allocated nothing through ops._empty"
            alloc.check()
            if offset:
                # the run happened where it says: every input and every allocation of the library 16 bytes past a 512-byte
                # boundary, and the re-based inputs unwritten like the originals
                for i, (t, b) in enumerate(zip(inputs, before)):
                    assert t.numel() == 0 or t.data_ptr() % 512 == offset, f"input #{i} was not re-based"
                    assert torch.equal(bits(t), b), f"re-based input #{i} {tuple(t.shape)} {t.dtype} was written"
                for order, shape, dtype, nbytes, raw in alloc.records:
                    assert (raw.data_ptr() + alloc.band_bytes) % 512 == offset, f"allocation #{order} {shape} {dtype}"
        runs.append((f"fill 0x{fill:02X}" + (f", every base moved by {offset} bytes" if offset else ""), snap))
        del out
    assert [t.data_ptr() for t in inputs] == homes, "an input was not put back where it lived"
    for i, (t, b) in enumerate(zip(inputs, before)):
        assert torch.equal(bits(t), b), f"input #{i} {tuple(t.shape)} {t.dtype} was written"
    name0, snap0 = runs[0]
    for name, snap in runs[1:]:
        assert [(p, k) for p, k, _ in snap] == [(p, k) for p, k, _ in snap0], "the runs returned different structures"
        for (path, kind, a), (_, _, b) in zip(snap0, snap):
            if not torch.equal(a, b):
                at = torch.nonzero(a != b).view(-1)
                raise AssertionError(f"{path} ({kind}) differs between the {name0} run and the {name} run in {at.numel()} of "
                                     f"{a.numel()} words, first at flat word {int(at[0])}: a read of unwritten memory, or "
                                     f"(re-based run) a kernel that assumes more of a base address than 16 bytes")
    ops.check_indices(torch.device("cuda", torch.cuda.current_device()))


def _randn(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


# ------------------------------------------------------------------------------------------------- the harness itself
def test_a_store_one_float_past_a_guarded_payload_is_caught_on_the_device():
    dev = need_gpu()
    alloc = GuardedAllocator(0xFF)
    out = alloc.empty(257, 36, dtype=torch.float32, device=dev)
    assert out.data_ptr() % 512 == 0 and out.is_contiguous()
    out.normal_()
    alloc.check()
    out.as_strided((1,), (1,), out.storage_offset() + out.numel()).fill_(1.0)      # inside the raw buffer the harness owns
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=r"allocation #0 \(shape \(257, 36\), torch.float32.*trailing band damaged at band byte 0 "):
        alloc.check()


# ------------------------------------------------------------------------------------------------- gathers
def _gather_graph(dev, seed):
    """the graph of ``test_aggregate_feature_widths_and_transposed``: packs, partial rows, at least two levels"""
    ei, et, n, r = synth.uniform_graph(300, 6000, 3, seed=seed)
    ei[1, :900] = 7
    ei[0, 1000:1200] = 9
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    assert g.num_levels(False) >= 2                     # the 900-edge destination: packs and partial rows
    return g, n, r


@pytest.mark.parametrize("d", [4, 24, 64, 264])
def test_gathers_fp32(d, monkeypatch):
    dev = need_gpu()
    g, n, r = _gather_graph(dev, d)
    assert g.workspace_bytes(False, d) > 0                                          # partial rows exist
    gen = torch.Generator().manual_seed(d)
    x = _randn(gen, n, d).to(dev)
    w = _randn(gen, r, d, 128, scale=0.1).to(dev)
    root = _randn(gen, d, 128, scale=0.1).to(dev)                    # of the transform that finishes the deferred gather
    # the 900-edge destination has (dst, rel) segments of more than 256 edges: partial rows and exactly one reduce level,
    # which the transform can take over at the widths it finishes (64 here).  The 200-edge source stays under 256 edges
    # per (src, rel) segment: one level, nothing to defer - the transposed hub finish has a graph of its own below
    # (test_hub_finish_inside_the_transforms).
    assert g.num_levels(False) == 2 and g.num_levels(True) == 1
    assert g.deferrable(False, d) == (d == 64) and not g.deferrable(True, d)

    def fn(ctx):
        out = {}
        for transposed in (False, True):
            out["agg", transposed] = ops.aggregate(g, x, transposed=transposed)
            am = ctx.amax(dev)
            out["agg+amax", transposed] = (ops.aggregate(g, x, transposed=transposed, amax_out=am), Amax(am))
            given = ctx.empty(n, r * d, device=dev)
            ops.aggregate(g, x, transposed=transposed, out=given)
            out["agg into out", transposed] = given
            agg, hubs = ops.aggregate_deferred(g, x, transposed=transposed)
            assert (hubs is not None) == (d == 64 and not transposed)
            if hubs is not None:                                # the transform finishes the hub rows and completes agg
                xa = ops.absmax(x)
                done = ops.transform_fwd(agg, x, w, root, None, graph=g, amax=(xa, xa), precision="split", hubs=hubs)
                out["deferred", transposed] = (agg, done)
            else:
                out["deferred", transposed] = agg
        return out

    protocol(monkeypatch, [x, w, root], fn)


@pytest.mark.parametrize("d_in,d_out", [(64, 128), (128, 256)])
def test_hub_finish_inside_the_transforms(d_in, d_out, monkeypatch):
    """``aggregate_deferred`` in BOTH directions with hub tails to finish: the gather's level-0 launch leaves partial rows
    in its workspace, and ``transform_fwd`` / ``transform_bwd_input`` (split precision) sum them tile by tile and write
    the finished rows into the aggregate.  The gather graph with its heavy destination and its heavy source at 1500
    edges each, about 500 per (node, relation) segment: more than one 256-edge pack in either direction."""
    dev = need_gpu()
    ei, et, n, r = synth.uniform_graph(300, 6000, 3, seed=d_in)
    ei[1, :1500] = 7
    ei[0, 2000:3500] = 9
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    assert g.num_levels(False) == 2 and g.num_levels(True) == 2
    assert g.deferrable(False, d_in) and g.deferrable(True, d_out)
    gen = torch.Generator().manual_seed(d_in + d_out)
    x, gout, mask = _randn(gen, n, d_in).to(dev), _randn(gen, n, d_out, scale=1e-3).to(dev), _randn(gen, n, d_in).to(dev)
    w = (_randn(gen, r, d_in, d_out) / d_in ** 0.5).to(dev)
    root, bias = (_randn(gen, d_in, d_out) / d_in ** 0.5).to(dev), _randn(gen, d_out).to(dev)
    bound = g.weight_bound(True)

    def fn(ctx):
        out = {}
        packed = ops.split_weights(w, root)
        x_amax, g_amax = ops.absmax(x), ops.absmax(gout)
        agg, hubs = ops.aggregate_deferred(g, x)
        assert hubs is not None
        am = ctx.amax(dev)
        out["fwd"] = (ops.transform_fwd(agg, x, w, root, bias, relu=True, graph=g, amax=(x_amax, x_amax), amax_out=am,
                                        packed=packed, hubs=hubs), agg, Amax(am))
        agg, hubs = ops.aggregate_deferred(g, x)
        out["fwd, weights split by the call"] = (ops.transform_fwd(agg, x, w, None, None, graph=g, amax=(x_amax, x_amax),
                                                                   precision="split", hubs=hubs), agg)
        gagg, hubs = ops.aggregate_deferred(g, gout, transposed=True)
        assert hubs is not None
        am = ctx.amax(dev)
        out["bwd_input"] = (ops.transform_bwd_input(gagg, gout, w, root, relu_mask=mask, graph=g, amax=(g_amax, g_amax),
                                                    amax_mul=bound, amax_out=am, packed=packed, hubs=hubs, out_scale=2.0),
                            gagg, Amax(am))
        gagg, hubs = ops.aggregate_deferred(g, gout, transposed=True)
        out["bwd_input, no root"] = (ops.transform_bwd_input(gagg, gout, w, None, graph=g, amax=(g_amax, g_amax),
                                                             amax_mul=bound, precision="split", hubs=hubs), gagg)
        out["finished by the gather"] = (ops.aggregate(g, x), ops.aggregate(g, gout, transposed=True))
        return out

    protocol(monkeypatch, [x, gout, mask, w, root, bias], fn)


@pytest.mark.parametrize("d", [8, 264])
def test_gathers_fp16_table(d, monkeypatch):
    dev = need_gpu()
    g, n, r = _gather_graph(dev, d)
    x = _randn(torch.Generator().manual_seed(d), n, d).to(dev).half()

    def fn(ctx):
        return [ops.aggregate(g, x, transposed=t) for t in (False, True)] + [ops.aggregate_deferred(g, x)[0]]

    protocol(monkeypatch, [x], fn)


@pytest.mark.parametrize("d", [4, 64, 264])
def test_gathers_three_levels_deep(d, monkeypatch):
    """the boundary graph of ``test_hub_levels.py`` (segments of 131,072 / 131,073 / 262,444 edges): the mean and the
    weighted gather whose plan has a reduce level that reads what another reduce level wrote.  The workspace is exactly
    ``num_partials * d`` floats, so a partial row written past the plan lands in a band; integer tables, so the rows are
    also the exact segment sums."""
    import hub_graphs as H
    dev = need_gpu()
    key, other, rel = H.boundary_edges()
    lens = H.segment_lengths()
    gen = torch.Generator().manual_seed(d)
    w8 = (2 ** torch.randint(0, 4, key.shape, generator=gen)) * (2 * torch.randint(0, 2, key.shape, generator=gen) - 1)
    weight = (w8.float() / 8).to(dev)
    mean = ops.BucketedGraph(torch.stack([other, key]).to(dev), rel.to(dev), H.N, H.R)
    weighted = ops.BucketedGraph.from_shard(key.to(dev), other.to(dev), rel.to(dev), H.N, H.N, H.R, edge_weight=weight)
    assert mean.num_levels(False) == weighted.num_levels(False) == 3
    assert mean.workspace_bytes(False, d) == weighted.workspace_bytes(False, d) == H.plan_partials(lens) * d * 4
    table = H.int_table(d, 4, seed=d)
    x = table.float().to(dev)
    want_mean = H.mean_expected(key, other, rel, table).to(dev)
    want_weighted = ((H.segment_matrix(key, other, rel, weight=w8) @ table.long()).float() / 8).view(H.N, -1).to(dev)

    def fn(ctx):
        out = {}
        for name, g, want in (("mean", mean, want_mean), ("weighted", weighted, want_weighted)):
            out[name] = ops.aggregate(g, x)
            assert torch.equal(out[name], want)
            am = ctx.amax(dev)
            out[name, "amax"] = (ops.aggregate(g, x, amax_out=am), Amax(am))
            given = ctx.empty(H.N, H.R * d, device=dev)
            ops.aggregate(g, x, out=given)
            out[name, "into out"] = given
            agg, hubs = ops.aggregate_deferred(g, x)
            assert hubs is None                                  # three levels: nothing is left to a transform
            out[name, "not deferred"] = agg
            if d % 8 == 0:
                out[name, "fp16 table"] = ops.aggregate(g, x.half())
        out["arrays of the weighted shard"] = weighted.arrays(False)          # val holds E weights, not N * R counts
        return out

    protocol(monkeypatch, [x, weight], fn)
    mean.destroy()
    weighted.destroy()


@pytest.mark.parametrize("precision", ["fp32", "split", "half"])
def test_deferred_parameter_gradient_tail_rides_in_the_gather(precision, monkeypatch):
    dev = need_gpu()
    g, n, r = _gather_graph(dev, 64)
    gen = torch.Generator().manual_seed(5)
    x, gout = _randn(gen, n, 64).to(dev), _randn(gen, n, 128).to(dev)
    agg = ops.aggregate(g, x)

    def fn(ctx):
        out = []
        for carrier, transposed in ((gout, True), (x.half(), False)):      # rides in the fp32 gather; launched by itself
            pend = ops.transform_bwd_params(agg, x, gout, r, graph=g, defer=True, precision=precision)
            assert not pend.done
            rows = ops.aggregate(g, carrier, transposed=transposed, tail=pend)
            assert pend.done
            out.append((rows, pend.grads))
        pend = ops.transform_bwd_params(agg, x, gout, r, want_root=False, want_bias=False, defer=True, precision=precision)
        pend.finish()
        out.append(pend.grads)
        return out

    protocol(monkeypatch, [x, gout, agg], fn)


# ------------------------------------------------------------------------------------------------- dense transforms
DENSE = [(65, 3, 64, 128), (129, 2, 20, 36), (257, 1, 8, 4), (63, 3, 128, 256), (130, 3, 64, 64), (130, 16, 32, 64),
         (64, 16, 128, 1280)]


def _dense_operands(dev, n, r, d_in, d_out, seed=0):
    gen = torch.Generator().manual_seed(n + d_in + seed)
    t = dict(agg=_randn(gen, n, r * d_in), x=_randn(gen, n, d_in), w=_randn(gen, r, d_in, d_out, scale=0.1),
             root=_randn(gen, d_in, d_out, scale=0.1), bias=_randn(gen, d_out), g=_randn(gen, n, d_out),
             gagg=_randn(gen, n, r * d_out), mask=_randn(gen, n, d_in))
    return {k: v.to(dev) for k, v in t.items()}


def _dense_calls(ctx, dev, t, r, precision, graph=None):
    """the three transforms with root / bias present and absent, ReLU, ReLU mask with ``out_scale = 2``, published maxima,
    ``want_root`` / ``want_bias`` on and off"""
    kw = dict(precision=precision, graph=graph)
    out = {}
    for name, root, bias, relu in (("rb", t["root"], t["bias"], False), ("--", None, None, False),
                                  ("r-relu", t["root"], None, True), ("-b-relu", None, t["bias"], True)):
        am = ctx.amax(dev)
        out["fwd", name] = (ops.transform_fwd(t["agg"], t["x"], t["w"], root, bias, relu=relu, amax_out=am, **kw), Amax(am))
    out["fwd", "no amax"] = ops.transform_fwd(t["agg"], t["x"], t["w"], t["root"], t["bias"], **kw)
    for name, root, mask, scale in (("r", t["root"], None, 1.0), ("-", None, None, 1.0), ("r-mask", t["root"], t["mask"], 2.0),
                                    ("--mask", None, t["mask"], 2.0)):
        am = ctx.amax(dev)
        out["bwd_input", name] = (ops.transform_bwd_input(t["gagg"], t["g"], t["w"], root, relu_mask=mask, out_scale=scale,
                                                          amax_out=am, **kw), Amax(am))
    for want_root in (True, False):
        for want_bias in (True, False):
            out["bwd_params", want_root, want_bias] = ops.transform_bwd_params(
                t["agg"], t["x"], t["g"], r, want_root=want_root, want_bias=want_bias, **kw)
    return out


@pytest.mark.parametrize("n,r,d_in,d_out,precision", [shape + (p,) for shape in DENSE for p in ("fp32", "split", "half")
                                                      if p == "fp32" or shape != (64, 16, 128, 1280)])
def test_dense_transforms(n, r, d_in, d_out, precision, monkeypatch):
    dev = need_gpu()
    if (n, r, d_in, d_out) == (64, 16, 128, 1280):                       # fp32 only
        # 34 kc-tiles x 10 n-tiles = 340 workgroups > 320: the instantiation with the three-deep ring
        assert -(-(r + 1) * d_in // 64) * -(-d_out // 128) > 320
    if (n, r, d_in, d_out) in ((129, 2, 20, 36), (257, 1, 8, 4)):
        # widths the split / DMA kernels do not tile: the fp32 non-DMA kernels and k_gemm_tn_slab in every arithmetic
        assert ops._use_split(precision, d_in, 32) == 0 and ops._use_split(precision, d_out, 32) == 0
    elif precision != "fp32":
        # forward and input gradient on the split kernels (K a multiple of 32); the parameter gradient tiles d_in by 64,
        # so at d_in = 32 - (130, 16, 32, 64) - it runs the fp32 slab kernel in every arithmetic
        assert ops._use_split(precision, d_in, 32) and ops._use_split(precision, d_out, 32)
        assert bool(ops._use_split(precision, d_in, 64)) == (d_in != 32)
    t = _dense_operands(dev, n, r, d_in, d_out)

    def fn(ctx):
        out = _dense_calls(ctx, dev, t, r, precision)
        if precision == "half" and d_in % 32 == 0:                       # the one-pass fp16 forward kernel of configs[4]
            out["fwd f16"] = ops.transform_fwd(t["agg"], t["x"], t["w"], t["root"], t["bias"], relu=True, half=True)
        return out

    protocol(monkeypatch, list(t.values()), fn)


def _holey_graph(dev):
    """n = 257, R = 3: relation 0 only among nodes below 96, relation 1 only among nodes from 128 up, relation 2
    everywhere - both directions' tile masks have holes, and however the rows of the parameter-gradient GEMM are split,
    a workgroup of relation 0's k-columns meets rows without a live m-tile"""
    n, r = 257, 3
    gen = torch.Generator().manual_seed(257)
    e0 = torch.randint(0, 96, (2, 600), generator=gen)
    e1 = torch.randint(128, n, (2, 600), generator=gen)
    e2 = torch.randint(0, n, (2, 900), generator=gen)
    ei = torch.cat([e0, e1, e2], 1)
    et = torch.cat([torch.zeros(600), torch.ones(600), torch.full((900,), 2.0)]).long()
    perm = torch.randperm(ei.size(1), generator=gen)
    g = ops.BucketedGraph(ei[:, perm].contiguous().to(dev), et[perm].contiguous().to(dev), n, r)
    assert g.tile_mask_ptr(False) is not None and g.tile_mask_ptr(True) is not None
    return g, n, r


@pytest.mark.parametrize("precision", ["fp32", "split"])
def test_relation_skipped_tiles(precision, monkeypatch):
    dev = need_gpu()
    g, n, r = _holey_graph(dev)
    d_in, d_out = 64, 128
    t = _dense_operands(dev, n, r, d_in, d_out, seed=1)
    t["agg"] = ops.aggregate(g, t["x"])                                   # exact zeros where a row has no such relation
    t["gagg"] = ops.aggregate(g, t["g"], transposed=True)
    assert float(t["agg"][96:, :d_in].abs().max()) == 0.0 and float(t["agg"][:128, d_in:2 * d_in].abs().max()) == 0.0
    assert float(t["gagg"][96:, :d_out].abs().max()) == 0.0 and float(t["gagg"][:128, d_out:2 * d_out].abs().max()) == 0.0
    # The parameter-gradient GEMM cuts the rows into `splits` ranges of a multiple of 32 rows, one slab block
    # [(R + 1) d_in, d_out] (+ one bias row) per range: `splits` is what the workspace query was sized for.  With two or
    # more ranges over 257 rows the last one starts at row 96 or later (at these widths: 3 ranges of 96 / 96 / 65 rows),
    # where relation 0 has no segment - the workgroups of relation 0's k-columns there have no live m-tile.
    unit = ((r + 1) * d_in * d_out + d_out) * 4
    if precision == "fp32":
        splits = _lib.load().rgcn_transform_bwd_params_workspace_bytes(n, r, d_in, d_out) // unit
    else:
        query = lambda rows: ops._query("rgcn_transform_bwd_params_split_workspace_bytes", rows, r, d_in, d_out)   # noqa: E731
        assert unit % 256 == 0 and (query(32) - query(1)) == 0             # one range up to 128 rows; the rest is constant
        splits = 1 + (query(n) - query(32)) // unit
    assert splits >= 2, splits
    want = (t["agg"].double().t() @ t["g"].double()).view(r, d_in, d_out)
    errs = []

    def fn(ctx):
        out = _dense_calls(ctx, dev, t, r, precision, graph=g)
        # the slab blocks of those workgroups came out zero in THIS run: the gradient is the float64 product (5e-6 relative
        # to the largest entry: test_transform_kernels' bound for the parameter gradients at up to 1000 rows)
        for key in (("bwd_params", True, True), ("bwd_params", False, False)):
            errs.append(float((out[key][0].double() - want).abs().max() / want.abs().max()))
            assert errs[-1] <= 5e-6, (key, ctx.fill, errs[-1])
        return out

    protocol(monkeypatch, list(t.values()), fn)
    print(f"relation-skipped grad_weight ({precision}), plain / 0x00 / 0xFF, with and without root: {errs}")


# ------------------------------------------------------------------------------------------------- chained launch
def _pack_directly(w, root):
    """the split images of a layer whose widths ``ops.split_weights`` leaves to the fp32 kernels (d_in % 32): the C entry
    takes any d_out % 4 == 0, and the chained launch reads only the image in the weights' own order"""
    lib = _lib.load()
    r, d_in, d_out = w.shape
    nbytes = lib.rgcn_weights_split_bytes(r, d_in, d_out)
    buf = ops._empty(nbytes, dtype=torch.uint8, device=w.device)
    one = lambda kind, v: ctypes.cast((kind * 1)(v), ctypes.c_void_p)                       # noqa: E731
    rc = lib.rgcn_weights_split_pack_multi(1, one(ctypes.c_void_p, w.data_ptr()),
                                           one(ctypes.c_void_p, None if root is None else root.data_ptr()),
                                           one(ctypes.c_int64, r), one(ctypes.c_int64, d_in), one(ctypes.c_int64, d_out),
                                           None, None, one(ctypes.c_void_p, buf.data_ptr()), one(ctypes.c_size_t, nbytes),
                                           None, 0, ops._stream())
    _lib.check(rc, "rgcn_weights_split_pack_multi")
    return ops.SplitWeights(buf, w, root)


@pytest.mark.parametrize("n,d_in1,d_out2,root1,root2", [(63, 64, 128, True, True), (130, 20, 64, False, True),
                                                        (63, 64, 128, True, False)])
def test_chained_launch_and_transform_first(n, d_in1, d_out2, root1, root2, monkeypatch):
    dev = need_gpu()
    r, hidden = 3, 128
    gen = torch.Generator().manual_seed(n + d_in1)
    w2, rt2 = _randn(gen, r, hidden, d_out2, scale=0.1).to(dev), (_randn(gen, hidden, d_out2, scale=0.1).to(dev) if root2 else None)
    w1, rt1 = _randn(gen, r, d_in1, hidden, scale=0.1).to(dev), (_randn(gen, d_in1, hidden, scale=0.1).to(dev) if root1 else None)
    g, gagg = _randn(gen, n, d_out2, scale=0.01).to(dev), _randn(gen, n, r * d_out2, scale=0.01).to(dev)
    h = _randn(gen, n, hidden).to(dev)
    assert ops.GEMM_PRECISION == "split" and ops.chain_supported(w2, w1)

    def fn(ctx):
        g_amax = ops.absmax(g)
        pk2 = ops.split_weights(w2, rt2)
        pk1 = ops.split_weights(w1, rt1) if d_in1 % 32 == 0 else _pack_directly(w1, rt1)
        assert pk2 is not None and pk1 is not None
        am = ctx.amax(dev)
        gz, t = ops.transform_bwd_input_chain(gagg, g, w2, rt2, h, pk2, pk1, amax=(g_amax, g_amax), amax_mul=1.5,
                                              amax_out=am, out_scale=2.0)
        assert t.shape == (n, (r + int(root1)) * d_in1)
        out = [gz, t, Amax(am), library_amax(g_amax)]
        if d_in1 % 32 == 0:
            out.append(ops.transform_first(h, pk1, ops.absmax(h)))          # [n, 128] @ conv1's weights in their own order
            out.append(ops.transform_first(h, pk1))
        return out

    protocol(monkeypatch, [w2, rt2, w1, rt1, g, gagg, h], fn)


# ------------------------------------------------------------------------------------------------- fused layers
@pytest.mark.parametrize("n,e,r,d_in,d_out,limit", [(33, 40, 3, 64, 128, 16), (500, 9000, 3, 128, 256, 1)])
def test_fused_layers(n, e, r, d_in, d_out, limit, monkeypatch):
    dev = need_gpu()
    gen = torch.Generator().manual_seed(n + e)
    dst = (torch.rand(e, generator=gen) ** 3 * n).long().clamp_(max=n - 1)
    src = (torch.rand(e, generator=gen) ** 3 * n).long().clamp_(max=n - 1)
    et = torch.randint(0, r, (e,), generator=gen)
    et[dst < n // 3] = 0
    graph = ops.BucketedGraph(torch.stack([src, dst]).to(dev), et.to(dev), n, r)
    assert ops.fused_supported(r, d_in, d_out) and ops.fused_bwd_supported(r, d_in, d_out)
    if limit == 1:
        assert graph.fused_plan(1).hub is not None and graph.fused_plan(1, transposed=True).hub is not None
    x, g = _randn(gen, n, d_in).to(dev), _randn(gen, n, d_out, scale=1e-3).to(dev)
    w = (_randn(gen, r, d_in, d_out) / d_in ** 0.5).to(dev)
    root = (_randn(gen, d_in, d_out) / d_in ** 0.5).to(dev)
    bias, mask = _randn(gen, d_out).to(dev), _randn(gen, n, d_in).to(dev)

    def fn(ctx):
        out = {}
        x_amax, g_amax = ops.absmax(x), ops.absmax(g)
        for name, rt, bs, relu in (("root+bias+relu", root, bias, True), ("no root", None, bias, False), ("no bias", root, None, False)):
            packed = ops.split_weights(w, rt)
            kept, am = ctx.empty(n, r * d_in, device=dev), ctx.amax(dev)
            out["fwd", name] = (ops.layer_fwd_fused(graph, x, packed, bs, relu, x_amax, am, inline_limit=limit, agg_out=kept),
                                kept, Amax(am))
            out["fwd no store", name] = ops.layer_fwd_fused(graph, x, packed, bs, relu, x_amax, None, inline_limit=limit)
            am, gam = ctx.amax(dev), ctx.amax(dev)
            out["bwd", name] = (ops.layer_bwd_input_fused(graph, g, packed, mask, g_amax, am, inline_limit=limit, out_scale=2.0),
                                Amax(am))
            out["bwd gagg_amax", name] = (ops.layer_bwd_input_fused(graph, g, packed, mask, g_amax, None, inline_limit=limit,
                                                                    gagg_amax=gam), Amax(gam))
        return out

    protocol(monkeypatch, [x, g, w, root, bias, mask], fn)


# ------------------------------------------------------------------------------------------------- small kernels
def test_absmax_and_weight_split_launches(monkeypatch):
    dev = need_gpu()
    gen = torch.Generator().manual_seed(11)
    x = _randn(gen, 1001, 64).to(dev)
    odd = _randn(gen, 2049 * 3 + 1).to(dev)
    layers = [(_randn(gen, 3, 64, 128, scale=0.1).to(dev), _randn(gen, 64, 128, scale=0.1).to(dev)),
              (_randn(gen, 3, 128, 128, scale=0.1).to(dev), None)]
    big = [(_randn(gen, 3, 256, 256, scale=0.1).to(dev), _randn(gen, 256, 256, scale=0.1).to(dev))]
    assert big[0][0].numel() + big[0][1].numel() > ops._MERGED_PACK_MAX >= max(w.numel() + (0 if rt is None else rt.numel())
                                                                                for w, rt in layers)
    agg = [_randn(gen, 65, 3 * w.size(1)).to(dev) for w, _ in layers + big]
    xs = [_randn(gen, 65, w.size(1)).to(dev) for w, _ in layers + big]

    def consume(packs, ls, k0=0):
        """the images only through a transform that multiplies by them (second row of the exceptions table)"""
        return [ops.transform_fwd(agg[k0 + i], xs[k0 + i], w, rt, None, packed=pk, precision="split")
                for i, ((w, rt), pk) in enumerate(zip(ls, packs))]

    def fn(ctx):
        out = {}
        clear = ctx.empty(3, ops.AMAX_FLOATS, device=dev)
        clear.view(-1)[::ops.AMAX_HEAD_STRIDE] = 7.0                     # the launch clears the heads on the side
        own = ctx.amax(dev)
        out["absmax"] = (library_amax(ops.absmax(x)), Amax(ops.absmax(odd, own, clear)), clear.view(-1)[::ops.AMAX_HEAD_STRIDE])
        assert ctx.fill is None or ctx.untouched(clear.view(-1, ops.AMAX_HEAD_STRIDE)[:, 1:])
        many = ctx.amax(dev, 3)
        ops.absmax_many([x, odd, layers[0][0]], [many[0], many[1], many[2]])
        out["absmax_many"] = [Amax(many[i]) for i in range(3)]
        out["split_weights_many"] = consume(ops.split_weights_many(layers), layers)
        wam = ctx.amax(dev, 3)
        ops.absmax_many([layers[0][0], layers[0][1], layers[1][0]], [wam[0], wam[1], wam[2]])
        out["split_weights_many given maxima"] = consume(
            ops.split_weights_many(layers, amax=[(wam[0], wam[1]), (wam[2], None)]), layers)
        for name, ls, k0 in (("merged", layers, 0), ("two launches", big, 2)):
            am = ctx.amax(dev)
            packs = ops.absmax_and_split(x, am, None, ls)
            assert all(p is not None for p in packs)
            out["absmax_and_split", name] = (Amax(am), consume(packs, ls, k0))
        return out

    protocol(monkeypatch, [x, odd] + [t for l in layers + big for t in l] + agg + xs, fn)


@pytest.mark.parametrize("r,b,d_in,d_out", [(33, 3, 8, 100), (3, 2, 256, 260)])
def test_basis_composition(r, b, d_in, d_out, monkeypatch):
    dev = need_gpu()
    if (r, b) == (3, 2):
        assert d_in * d_out > 65536                                       # more than 64 backward workgroups
    gen = torch.Generator().manual_seed(r + d_out)
    comp, basis, gw = _randn(gen, r, b).to(dev), _randn(gen, b, d_in, d_out).to(dev), _randn(gen, r, d_in, d_out).to(dev)

    def fn(ctx):
        return [ops.basis_compose(comp, basis), ops.basis_compose_bwd(gw, comp, basis),
                ops.basis_compose_bwd(gw, comp, basis, need_comp=False), ops.basis_compose_bwd(gw, comp, basis, need_basis=False)]

    protocol(monkeypatch, [comp, basis, gw], fn)


# ------------------------------------------------------------------------------------------------- head and step
@pytest.mark.parametrize("d", [4, 64, 132])
@pytest.mark.parametrize("batch", [1, 257])
def test_distmult_head(batch, d, monkeypatch):
    dev = need_gpu()
    gen = torch.Generator().manual_seed(1000 * d + batch)
    ent, ent2, rel = _randn(gen, 50, d).to(dev), _randn(gen, 50, d).to(dev), _randn(gen, 5, d).to(dev)
    hi, ti = torch.randint(0, 50, (batch,), generator=gen), torch.randint(0, 50, (batch,), generator=gen)
    hi[batch // 2:] = 7                                                    # duplicated ids
    hi, ti, ri = hi.to(dev), ti.to(dev), torch.randint(0, 5, (batch,), generator=gen).to(dev)
    labels = (torch.rand(batch, generator=gen) > 0.5).float().to(dev)
    gs, one = _randn(gen, batch).to(dev), torch.ones(1, device=dev)
    state = (torch.tensor(3.5, dtype=torch.float64, device=dev), torch.tensor(11, dtype=torch.int64, device=dev),
             torch.tensor([5], dtype=torch.int64, device=dev))

    def fn(ctx):
        out = {}
        out["fwd"] = ops.distmult_fwd(ent, hi, ent, ti, rel, ri, batch)
        scores, loss = out["bce_fwd"] = ops.distmult_bce_fwd(ent, hi, ent, ti, rel, ri, labels, batch)
        loss_sum, correct, cursor = (ctx.like(s) for s in state)
        out["bce_reduce"] = (ops.distmult_bce_reduce(loss, scores, labels, loss_sum, correct, cursor, cursor_add=batch),
                             loss_sum, correct, cursor, ops.distmult_bce_reduce(loss, scores, labels))
        for shared in (True, False):
            tail = ent if shared else ent2
            for bce in (False, True):
                gh = ctx.empty(50, d, device=dev)
                gt = gh if shared else ctx.empty(50, d, device=dev)
                gr = ctx.empty(5, d, device=dev)
                if bce:
                    ops.distmult_bce_bwd(one, scores, labels, ent, hi, tail, ti, rel, ri, batch, gh, gt, gr, zero_tables=True)
                else:
                    ops.distmult_bwd(gs, ent, hi, tail, ti, rel, ri, batch, gh, gt, gr, zero_tables=True)
                out["bwd", shared, bce] = (gh, None if shared else gt, gr)
        # operands given row by row (no index vectors): the gradients are written in place of every row
        rows_h, rows_t, rows_r = ent[hi].contiguous(), ent[ti].contiguous(), rel[ri].contiguous()
        gh, gt, gr = (ctx.empty(batch, d, device=dev) for _ in range(3))
        ops.distmult_bwd(gs, rows_h, None, rows_t, None, rows_r, None, batch, gh, gt, gr, zero_tables=True)
        out["bwd rows"] = (ops.distmult_fwd(rows_h, None, rows_t, None, rows_r, None, batch), gh, gt, gr)
        return out

    protocol(monkeypatch, [ent, ent2, rel, hi, ti, ri, labels, gs, one] + list(state), fn)


@pytest.mark.parametrize("d", [4, 64])
def test_segment_sum(d, monkeypatch):
    dev = need_gpu()
    gen = torch.Generator().manual_seed(d)
    rows, idx = _randn(gen, 257, d).to(dev), torch.randint(0, 3, (257,), generator=gen).to(dev)
    idx2 = torch.where(idx == 1, torch.zeros_like(idx), idx)               # row 1 of the result has no term
    protocol(monkeypatch, [rows, idx, idx2], lambda ctx: [ops.segment_sum(rows, idx, 3), ops.segment_sum(rows, idx2, 3)])


@pytest.mark.parametrize("d", [32, 64])
def test_score_all_tails(d, monkeypatch):
    dev = need_gpu()
    gen = torch.Generator().manual_seed(d)
    head, rel, emb = _randn(gen, 65, d).to(dev), _randn(gen, 4, d).to(dev), _randn(gen, 300, d).to(dev)
    ri, rows = torch.randint(0, 4, (65,), generator=gen).to(dev), _randn(gen, 65, d).to(dev)
    protocol(monkeypatch, [head, rel, emb, ri, rows],
             lambda ctx: [ops.distmult_score_all_tails(head, rel, ri, emb), ops.distmult_score_all_tails(head, rows, None, emb)])


def test_batch_samplers(monkeypatch):
    dev = need_gpu()
    gen = torch.Generator().manual_seed(3)
    n, e, batch, k = 400, 1000, 257, 2
    ei, et = torch.randint(0, n, (2, e), generator=gen).to(dev), torch.randint(0, 3, (e,), generator=gen).to(dev)
    order = torch.randperm(e, generator=gen).to(dev)
    rng = torch.tensor([12345, 2], dtype=torch.int64, device=dev)
    cursors = [torch.tensor([c], dtype=torch.int64, device=dev) for c in (0, 900)]        # 900: the window runs over the end
    classes = ops.NodeClasses(torch.randint(0, 3, (n,), generator=gen).to(dev), 3)
    known = ops.KnownTriples(ei, et, n, 3)
    stats0 = torch.zeros(2, dtype=torch.int64, device=dev)

    def fn(ctx):
        out = {}
        for i, cursor in enumerate(cursors):
            out["plain", i] = ops.sample_batch(ei, et, order, cursor, batch, k, n, rng)
            out["no order", i] = ops.sample_batch(ei, et, None, cursor, batch, k, n, rng)
            stats = ctx.like(stats0)
            out["constrained", i] = (ops.sample_batch_constrained(ei, et, order, cursor, batch, k, n, rng, classes, known,
                                                                  max_tries=8, stats=stats), stats)
        out["positives only"] = ops.sample_batch(ei, et, order, cursors[0], batch, 0, n, None)
        return out

    protocol(monkeypatch, [ei, et, order, rng, stats0, classes.class_of, classes.ptr, classes.members] + cursors
             + [t for side in known.SIDES for t in known.csr(side)], fn)


def test_adam_clip_step(monkeypatch):
    dev = need_gpu()
    gen = torch.Generator().manual_seed(9)
    sizes = [1, 2047, 2048, 2049, 5000, 1000]                  # the last one lives 4 bytes into its buffer
    seeds = [dict(p=_randn(gen, s).to(dev), g=_randn(gen, s).to(dev), m=_randn(gen, s, scale=0.1).to(dev),
                  v=_randn(gen, s).abs().to(dev)) for s in sizes]

    def fn(ctx):
        params, grads, ms, vs, bases = [], [], [], [], []
        for i, (s, sd) in enumerate(zip(sizes, seeds)):
            row = []
            for key in ("p", "g", "m", "v"):
                if i == len(sizes) - 1:
                    base = ctx.empty(s + 4, device=dev)
                    if ctx.fill is None:
                        base.view(torch.uint8).fill_(PLAIN_AMAX_FILL)
                    t = base[1:1 + s]
                    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
                    bases.append(base)
                else:
                    t = ctx.empty(s, device=dev)
                row.append(t.copy_(sd[key]))
            for lst, t in zip((params, grads, ms, vs), row):
                lst.append(t)
        steps = [ctx.empty(1, device=dev).fill_(float(i)) for i in range(len(sizes))]
        norm = ctx.empty(1, device=dev)
        amax = [ctx.amax(dev) for _ in sizes]
        ops.adam_clip_step(params, grads, ms, vs, steps, 1e-2, 0.9, 0.999, 1e-8, weight_decay=0.01, adamw=True, max_norm=1.0,
                           total_norm=norm, amax_out=amax)
        ops.adam_clip_step(params[:2], grads[:2], ms[:2], vs[:2], steps[:2], 1e-2, 0.9, 0.999, 1e-8)      # no clipping, no extras
        torch.cuda.synchronize()
        for base in bases:                                               # around the misaligned views: never written
            assert ctx.untouched(base[:1]) and ctx.untouched(base[1 + sizes[-1]:])
        for g_after, sd in zip(grads, seeds):
            assert torch.equal(bits(g_after), bits(sd["g"])), "a gradient was written (they are left as they are)"
        return [params, ms, vs, steps, norm, [Amax(a) for a in amax]]

    protocol(monkeypatch, [t for sd in seeds for t in sd.values()], fn)


# ------------------------------------------------------------------------------------------------- analysis kernels
def test_ranking_and_topk(monkeypatch):
    dev = need_gpu()
    gen = torch.Generator().manual_seed(300)
    b, n, d = 65, 300, 32
    assert ops.mask_words(n) == 10
    q, emb = _randn(gen, b, d).to(dev), _randn(gen, n, d).to(dev)
    target = torch.randint(0, n, (b,), generator=gen).to(dev)
    true_score = (q * emb[target]).sum(1).contiguous()
    cls = torch.randint(-1, 3, (n,), generator=gen).int().to(dev)
    qcls = torch.randint(0, 3, (b,), generator=gen).int().to(dev)
    ei, et = torch.randint(0, n, (2, 4000), generator=gen).to(dev), torch.randint(0, 3, (4000,), generator=gen).to(dev)
    known = ops.KnownTriples(ei, et, n, 3)
    anchor, rel = torch.randint(0, n, (b,), generator=gen).to(dev), torch.randint(0, 3, (b,), generator=gen).to(dev)
    few = torch.full((n,), -1, dtype=torch.int32)
    few[torch.randperm(n, generator=gen)[:6]] = 0                          # six candidates: fewer than k = 10
    few = few.to(dev)

    def fn(ctx):
        out = {}
        allow = out["allow"] = ops.class_allow_bits(cls, 3)
        excl = out["exclude"] = known.exclude_bits("tail", anchor, rel)
        out["exclude head"] = known.exclude_bits("head", anchor, rel)
        out["rank plain"] = ops.distmult_rank_tails(q, emb, true_score, target)
        out["rank masked"] = [ops.distmult_rank_masked(q, emb, true_score, target, allow, qcls, excl),
                              ops.distmult_rank_masked(q, emb, true_score, target, allow, qcls),
                              ops.distmult_rank_masked(q, emb, true_score, target, exclude=excl)]
        out["rank filtered"] = [ops.distmult_rank_filtered(q, emb, true_score, target, known, "tail", anchor, rel, allow, qcls),
                                ops.distmult_rank_filtered(q, emb, true_score, target, known, "tail", anchor, rel,
                                                           max_mask_bytes=40 * 16)]        # chunks of 16 rows, one buffer
        for k in (1, 10):
            for slices in (0, 2):
                out["topk", k, slices] = [ops.distmult_topk_masked(q, emb, k, slices=slices),
                                          ops.distmult_topk_masked(q, emb, k, allow, qcls, excl, slices=slices)]
        allow_few = ops.class_allow_bits(few, 1)
        ids, scores = out["topk few"] = ops.distmult_topk_masked(q, emb, 10, allow_few, torch.zeros_like(qcls))
        assert bool((ids[:, 6:] == -1).all()) and bool((ids[:, :6] >= 0).all())
        out["topk filtered"] = [ops.distmult_topk_filtered(q, emb, 10, known, "tail", anchor, rel),
                                ops.distmult_topk_filtered(q, emb, 10, known, "tail", anchor, rel, max_mask_bytes=40 * 16)]
        return out

    protocol(monkeypatch, [q, emb, target, true_score, cls, qcls, anchor, rel, few]
             + [t for side in known.SIDES for t in known.csr(side)], fn)


def test_paths(monkeypatch):
    import paths_reference as R
    dev = need_gpu()
    ei, et, pairs = R.random_case()
    graph = ops.PathGraph(ei.to(dev), et.to(dev), R.RANDOM_N)
    emb = R.random_embeddings(32).to(dev)
    src, dst = pairs[:, 0].contiguous().to(dev), pairs[:, 1].contiguous().to(dev)

    def fn(ctx):
        cosine = ops.edge_cosine(emb, graph)
        return [cosine] + [ops.paths_topk(graph, cosine, src, dst, k, max_len, slices)
                           for k, max_len in ((5, 4), (64, 3), (1, 1)) for slices in (1, 2)]

    protocol(monkeypatch, [emb, src, dst] + [t for _, t, _ in graph._arrays()], fn)


def test_kmeans_steps(monkeypatch):
    import cluster_reference as R
    dev = need_gpu()
    m, k, restarts = 257, 7, 3
    # the entry points take row widths that are multiples of 32 only (include/rgcn_cluster.h:6): d = 20 is refused by
    # name before anything is allocated, so the ragged shape runs at the narrowest width there is
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.kmeans_assign(torch.zeros(m, 20, device=dev), torch.zeros(restarts, k, 20, device=dev))
    d = 32
    x_host = R.blobs(m, d, seed=257)
    x = torch.from_numpy(x_host).float().to(dev)
    init = torch.from_numpy(R.starts(x_host, k, restarts, seed=7)).float().to(dev)
    done0 = torch.tensor([0, 1, 0], dtype=torch.int32, device=dev)

    def fn(ctx):
        out = {}
        centers = ctx.like(init)
        labels, changed = out["assign"] = ops.kmeans_assign(x, centers)
        out["update"] = ops.kmeans_update(x, centers, labels, changed)
        out["centers"] = centers
        out["inertia"] = ops.kmeans_inertia(x, centers, labels)
        # a second iteration through caller-held state, restart 1 frozen
        done, num_iter = ctx.like(done0), ctx.like(torch.zeros_like(done0))
        labels2, changed2 = out["assign again"] = ops.kmeans_assign(x, centers, labels, done)
        out["update again"] = ops.kmeans_update(x, centers, labels2, changed2, 1e-3, done, num_iter)
        out["state"] = (centers.clone(), done, num_iter)
        return out

    protocol(monkeypatch, [x, init, done0], fn)

    def whole(ctx):
        r = ops.kmeans(x, k, init=init, max_iter=20, tol=0.0)
        return [r.labels, r.centers, r.sizes, torch.tensor([r.inertia, float(r.n_iter), float(r.restart)], dtype=torch.float64)]

    protocol(monkeypatch, [x, init], whole)


@pytest.mark.parametrize("slices", [0, 2])
def test_silhouette(slices, monkeypatch):
    import cluster_reference as R
    dev = need_gpu()
    m, d, k = 129, 96, 5
    x_host = R.blobs(m, d, seed=2000 + m + d + k)
    labels = R.lloyd(x_host, R.starts(x_host, k, 1, seed=3)[0])["labels"]
    x, lab = torch.from_numpy(x_host).float().to(dev), torch.from_numpy(labels).long().to(dev)
    protocol(monkeypatch, [x, lab], lambda ctx: list(ops._silhouette(x, lab, k, slices)))
