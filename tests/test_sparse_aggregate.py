"""GPU tier: sparse aggregates (``conv._SPARSE_AGG``; ``ops.aggregate_sparse``, ``sparse=`` of the split transforms).

A training pass does not store the rows of (node, relation) segments without an edge and its consumers never load
them.  Nothing may change: every comparison here is of BYTES, sparse against dense, and the sparse runs get their
buffers pre-filled with NaN and, in a second run, with 3e38 - a dead row read even once would leak into the result
(NaN through any sum; 3e38 through the operand split, whose scale sends it to +inf), so equality under both fills is
the proof that none is read.  The fills go in through the allocation seam the guarded tier uses (``ops._empty``) for
the eager wrappers, and through ``torch.empty`` - where a replayed ``Region`` takes its arena from - for the replays.

Graphs: ``sparse_graphs.py`` (an empty relation, a 64-row tile without relation 0, an isolated node, a hub segment of
300 edges among empty segments, ragged last tiles for 32 and 64 rows; ``test_sparse_aggregate_host.py`` asserts those
properties), N = 150 and N = 70."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import sparse_graphs as SG
from conftest import need_gpu
from guarded import bits
from primekg_rgcn_linkprediction_amd import RGCNConv, conv, ops, rgcn_encoder2

pytestmark = pytest.mark.gpu

POISON = {"nan": float("nan"), "3e38": 3e38}


def _fill(t, value):
    """pre-fill a fresh device allocation: floats with ``value``, raw bytes with its bit pattern where they hold floats"""
    if t.device.type != "cuda" or t.numel() == 0:
        return t
    if t.dtype == torch.float32:
        t.fill_(value)
    elif t.dtype == torch.uint8 and t.numel() % 4 == 0 and t.data_ptr() % 4 == 0 and t.is_contiguous():
        t.view(torch.float32).fill_(value)
    return t


@contextlib.contextmanager
def poisoned(monkeypatch, value, seam):
    """``seam``: "wrappers" - every allocation of the library's wrappers (``ops._empty``); "replay" - every
    ``torch.empty`` (the arena and the outputs of a replayed Region)"""
    if value is None:
        yield
        return
    with monkeypatch.context() as m:
        if seam == "wrappers":
            assert ops._REC is None
            m.setattr(ops, "_empty", lambda *shape, dtype, device: _fill(torch.empty(*shape, dtype=dtype, device=device), value))
        else:
            real = torch.empty
            m.setattr(torch, "empty", lambda *a, **kw: _fill(real(*a, **kw), value))
        yield


class Case:
    def __init__(self, n, r, dims):
        dev = torch.device("cuda:0")
        self.n, self.r, self.dims = n, r, dims
        self.src, self.dst, self.rel = SG.edges(n, r)
        self.ei = torch.from_numpy(np.stack([self.src, self.dst])).to(dev)
        self.et = torch.from_numpy(self.rel).to(dev)
        gen = torch.Generator().manual_seed(n * 10 + r)
        self.x = torch.randn(n, dims[0], generator=gen).to(dev)
        self.cot = torch.randn(n, dims[-1], generator=gen).to(dev)
        torch.manual_seed(n + r)
        self.convs = [RGCNConv(a, b, r).to(dev) for a, b in zip(dims[:-1], dims[1:])]
        for c in self.convs:
            c.bias.data.uniform_(-0.1, 0.1)
        self.graph = ops.bucket(self.ei, self.et, n, r)
        self.occ = {False: torch.from_numpy(SG.occupancy(self.dst, self.rel, n, r)).to(dev),
                    True: torch.from_numpy(SG.occupancy(self.src, self.rel, n, r)).to(dev)}

    def plans(self):
        return sum(isinstance(s, ops._Plan) for s in self.graph.__dict__.get("_regions", {}).values())

    def step(self, route):
        """one forward + backward -> bits of out, grad_x and the parameter gradients (weight, root, bias per layer)"""
        x = self.x.clone().requires_grad_(True)
        for c in self.convs:
            c.zero_grad(set_to_none=True)
        if route == "encoder2":
            out = rgcn_encoder2(x, self.ei, self.et, *self.convs)
        else:                                           # the drop-in route: RGCNConv.forward calls around relu
            out = x
            for i, c in enumerate(self.convs):
                out = c(out, self.ei, self.et)
                if i + 1 < len(self.convs):
                    out = torch.relu(out)
        out.backward(self.cot)
        torch.cuda.synchronize()
        grads = [p.grad for c in self.convs for p in (c.weight, c.root, c.bias)]
        assert all(g is not None for g in grads) and x.grad is not None
        return [bits(t) for t in (out, x.grad, *grads)]


@functools.lru_cache(maxsize=None)
def _case(n, r, dims):
    need_gpu()
    return Case(n, r, dims)


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"{what}: output {i} differs in {int((a != b).sum())} of {a.numel()} words"


ROUTES = [("encoder2", 3, (64, 128, 128)),              # the headline shape: conv1 transform-first, conv2 chained
          ("convs", 3, (64, 128, 128)),                 # two RGCNConv.forward calls around relu
          ("convs", 3, (128, 128)),                     # gather-first input gradient, plain NT
          ("convs", 5, (64, 128))]                      # a 128-column kc tile straddles relation 4 and the root block


# ------------------------------------------------------------------------------------------ 1. whole-pass equality
@pytest.mark.parametrize("n", SG.SIZES)
@pytest.mark.parametrize("route,r,dims", ROUTES, ids=lambda v: str(v).replace(" ", ""))
def test_whole_pass_sparse_equals_dense_as_bytes_through_the_wrappers(route, r, dims, n, monkeypatch):
    need_gpu()
    case = _case(n, r, dims)
    monkeypatch.setattr(ops, "REGIONS", False)
    monkeypatch.setattr(conv, "_SPARSE_AGG", False)
    dense = case.step(route)
    assert all(torch.isfinite(d.view(torch.float32)).all() for d in dense)
    monkeypatch.setattr(conv, "_SPARSE_AGG", True)
    calls = []
    real = ops._gather
    monkeypatch.setattr(ops, "_gather", lambda *a, **kw: (calls.append(kw.get("sparse", False)), real(*a, **kw))[1])
    _same(case.step(route), dense, "sparse, plain memory")
    assert any(calls), "the policy never chose a sparse aggregate for this route"
    for name, value in POISON.items():
        with poisoned(monkeypatch, value, "wrappers"):
            got = case.step(route)
        _same(got, dense, f"sparse, buffers pre-filled with {name}")


@pytest.mark.parametrize("n", SG.SIZES)
@pytest.mark.parametrize("route,r,dims", ROUTES, ids=lambda v: str(v).replace(" ", ""))
def test_whole_pass_sparse_equals_dense_as_bytes_in_recorded_replays(route, r, dims, n, monkeypatch):
    need_gpu()
    case = _case(n, r, dims)
    monkeypatch.setattr(ops, "REGIONS", True)
    results = {}
    for sparse in (False, True):
        monkeypatch.setattr(conv, "_SPARSE_AGG", sparse)
        before = case.plans()
        for _ in range(3):                              # plain, sizing, recording (+ its two acceptance replays)
            first = case.step(route)
        assert case.plans() > before, "the pass was not accepted as a recorded Region"
        results[sparse] = [first, case.step(route)]    # the fourth call is a replay
        if sparse:
            for value in POISON.values():
                with poisoned(monkeypatch, value, "replay"):
                    results[sparse].append(case.step(route))
    for k, got in enumerate(results[False] + results[True]):
        _same(got, results[False][0], f"run {k}")


# ------------------------------------------------------------------------------------------------ 2. the gather alone
@pytest.mark.parametrize("n", SG.SIZES)
@pytest.mark.parametrize("d,transposed", [(64, False), (128, False), (128, True), (64, True)])
def test_gather_leaves_empty_rows_alone_and_everything_else_as_it_was(d, transposed, n):
    need_gpu()
    case = _case(n, 3, (64, 128, 128))
    g, r = case.graph, case.r
    table = torch.randn(n, d, generator=torch.Generator().manual_seed(d)).to(case.x.device)
    amax_d, amax_s = ops.amax_buffer(table.device), ops.amax_buffer(table.device)
    dense = ops.aggregate(g, table, transposed=transposed, amax_out=amax_d[0])
    live = case.occ[transposed].view(n * r)
    for value in POISON.values():
        amax_s.zero_()
        out = torch.full((n, r * d), value, device=table.device)
        poison_bits = bits(out).view(n * r, d).clone()
        got, hubs = ops.aggregate_sparse(g, table, transposed=transposed, amax_out=amax_s[0], out=out)
        assert hubs is None and got.data_ptr() == out.data_ptr()
        gb, db = bits(got).view(n * r, d), bits(dense).view(n * r, d)
        assert torch.equal(gb[live], db[live])                       # live rows: the same bytes
        assert torch.equal(gb[~live], poison_bits[~live])            # rows of empty segments: never written
        assert not dense.view(n * r, d)[~live].any()                 # (which the default call zeroes)
        assert torch.equal(bits(ops.amax_value(amax_s)), bits(ops.amax_value(amax_d)))
    assert int((~live).sum()) > n                                    # more than a third of the segments are empty


# ------------------------------------------------------------------------------------------ 3. each consumer alone
def _layer(case, r, d_in, d_out, seed):
    dev = case.x.device
    gen = torch.Generator().manual_seed(seed)
    w = (torch.randn(r, d_in, d_out, generator=gen) * 0.1).to(dev)
    root = (torch.randn(d_in, d_out, generator=gen) * 0.1).to(dev)
    return w, root, ops.split_weights(w, root)


def _both(case, table, transposed, value):
    """the dense aggregate and a poisoned sparse one of the same table, with the aggregate's own maximum"""
    amax = ops.amax_buffer(table.device)
    dense = ops.aggregate(case.graph, table, transposed=transposed, amax_out=amax[0])
    out = torch.full_like(dense, value)
    sparse, _ = ops.aggregate_sparse(case.graph, table, transposed=transposed, out=out)
    return dense, sparse, amax[0]


@pytest.mark.parametrize("poison", list(POISON))
@pytest.mark.parametrize("n", SG.SIZES)
@pytest.mark.parametrize("r,d_in,d_out", [(3, 64, 128), (3, 128, 128), (5, 64, 128)])
def test_each_consumer_reads_no_dead_row(r, d_in, d_out, n, poison):
    need_gpu()
    case = _case(n, r, (64, 128) if r == 5 else (64, 128, 128))
    g, value, dev = case.graph, POISON[poison], case.x.device
    gen = torch.Generator().manual_seed(7 * n + d_in)
    x, gout = torch.randn(n, d_in, generator=gen).to(dev), torch.randn(n, d_out, generator=gen).to(dev)
    w, root, packed = _layer(case, r, d_in, d_out, 1)
    bias = torch.linspace(-1, 1, d_out, device=dev)
    x_amax, g_amax = ops.absmax(x), ops.absmax(gout)

    # forward NT (with the ReLU epilogue and the published maximum)
    agg_d, agg_s, _ = _both(case, x, False, value)
    outs = []
    for agg, sparse in ((agg_d, False), (agg_s, True)):
        am = ops.amax_buffer(dev)
        out = ops.transform_fwd(agg, x, w, root, bias, relu=True, graph=g, amax=(x_amax, x_amax), amax_out=am[0],
                                packed=packed, sparse=sparse)
        outs.append([bits(out), bits(ops.amax_value(am))])
    _same(outs[1], outs[0], "transform_fwd")

    # parameter gradients: TN begin / finish
    grads = []
    for agg, sparse in ((agg_d, False), (agg_s, True)):
        pending = ops.transform_bwd_params(agg, x, gout, r, graph=g, defer=True, amax=(x_amax, x_amax, g_amax),
                                           sparse=sparse)
        pending.finish()
        grads.append([bits(t) for t in pending.grads])
    _same(grads[1], grads[0], "transform_bwd_params")

    # input gradient NT, with the ReLU mask and an output factor
    gagg_d, gagg_s, gagg_amax = _both(case, gout, True, value)
    mask = torch.relu(torch.randn(n, d_in, generator=gen)).to(dev)
    outs = []
    for gagg, sparse in ((gagg_d, False), (gagg_s, True)):
        gx = ops.transform_bwd_input(gagg, gout, w, root, relu_mask=mask, graph=g, amax=(gagg_amax, g_amax), packed=packed,
                                     out_scale=1.25, sparse=sparse)
        outs.append([bits(gx)])
    _same(outs[1], outs[0], "transform_bwd_input")

    # chained NT: this layer's input gradient and the transform-first product of a layer below it
    if d_in == 128:
        w1, root1, packed1 = _layer(case, r, 64, 128, 2)
        assert ops.chain_supported(w, w1)
        outs = []
        for gagg, sparse in ((gagg_d, False), (gagg_s, True)):
            am = ops.amax_buffer(dev)
            gz, t = ops.transform_bwd_input_chain(gagg, gout, w, root, mask, packed, packed1, graph=g,
                                                  amax=(gagg_amax, g_amax), amax_out=am[0], sparse=sparse)
            outs.append([bits(gz), bits(t), bits(ops.amax_value(am))])
        _same(outs[1], outs[0], "transform_bwd_input_chain")


def test_a_sparse_operand_is_refused_where_it_could_be_read():
    need_gpu()
    case = _case(150, 3, (64, 128, 128))
    x = case.x
    w, root, packed = _layer(case, 3, 64, 128, 1)
    agg, _ = ops.aggregate_sparse(case.graph, x)
    with pytest.raises(ValueError, match="sparse"):                 # no maximum: the operand would be scanned
        ops.transform_fwd(agg, x, w, root, graph=case.graph, packed=packed, sparse=True)
    with pytest.raises(ValueError, match="sparse"):                 # the fp32 kernels read every row
        ops.transform_fwd(agg, x, w, root, graph=case.graph, amax=(ops.absmax(x),) * 2, precision="fp32", sparse=True)
    with pytest.raises(ValueError, match="sparse"):                 # an fp16 table has no zero-fill part to leave out
        ops.aggregate_sparse(case.graph, x.half())


# ---------------------------------------------------------------------------------------------- 4. the public contract
@pytest.mark.parametrize("n", SG.SIZES)
@pytest.mark.parametrize("transposed", [False, True])
def test_public_aggregate_still_writes_every_row(transposed, n):
    need_gpu()
    import ctypes
    from primekg_rgcn_linkprediction_amd import _lib
    case = _case(n, 3, (64, 128, 128))
    g, r, d = case.graph, case.r, 64
    table = torch.randn(n, d, generator=torch.Generator().manual_seed(3)).to(case.x.device)
    live = case.occ[transposed].view(n * r)
    for value in POISON.values():
        out = torch.full((n, r * d), value, device=table.device)
        got = ops.aggregate(g, table, transposed=transposed, out=out)
        assert torch.isfinite(got).all() and not (got == value).any()
        assert not got.view(n * r, d)[~live].any()
        # the C entry point itself
        out2 = torch.full((n, r * d), value, device=table.device)
        nbytes = g.workspace_bytes(transposed, d)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=table.device)
        rc = _lib.load().rgcn_aggregate(g.handle, int(transposed), table.data_ptr(), d, out2.data_ptr(), ws.data_ptr(),
                                        nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(bits(out2), bits(got))


# -------------------------------------------------------------------------------------------------------- 6. fall-backs
def _choices(case, route, monkeypatch):
    """which gathers of one step were sparse"""
    calls = []
    real = ops._gather
    with monkeypatch.context() as m:
        m.setattr(ops, "_gather", lambda *a, **kw: (calls.append(bool(kw.get("sparse", False))), real(*a, **kw))[1])
        m.setattr(ops, "REGIONS", False)
        got = case.step(route)
    return calls, got


def test_fallbacks_pick_dense_and_give_the_dense_results(monkeypatch):
    need_gpu()
    case = _case(150, 3, (64, 128, 128))
    monkeypatch.setattr(conv, "_SPARSE_AGG", False)
    _, dense = _choices(case, "encoder2", monkeypatch)
    monkeypatch.setattr(conv, "_SPARSE_AGG", True)
    calls, _ = _choices(case, "encoder2", monkeypatch)
    assert calls.count(True) == 3                        # agg1, agg2 and conv2's transposed aggregate; the merged gather is dense
    # fp32 transforms: dense, and what the switch-off gives in that precision
    monkeypatch.setattr(ops, "GEMM_PRECISION", "fp32")
    calls, on = _choices(case, "encoder2", monkeypatch)
    monkeypatch.setattr(conv, "_SPARSE_AGG", False)
    _, off = _choices(case, "encoder2", monkeypatch)
    assert not any(calls)
    _same(on, off, "fp32 transforms")
    monkeypatch.setattr(ops, "GEMM_PRECISION", "split")
    # an fp16 feature table: the forward gathers are dense (the backward's transposed gathers read fp32 gradients)
    for c in case.convs:
        monkeypatch.setattr(c, "gather_dtype", torch.float16)
        monkeypatch.setattr(c, "half_backward", True)
    monkeypatch.setattr(conv, "_SPARSE_AGG", False)
    _, off = _choices(case, "encoder2", monkeypatch)
    monkeypatch.setattr(conv, "_SPARSE_AGG", True)
    for value in (None, POISON["nan"]):
        with poisoned(monkeypatch, value, "wrappers"):
            calls, on = _choices(case, "encoder2", monkeypatch)
        _same(on, off, "fp16 table")
    assert calls[:2] == [False, False]
    del dense


def test_a_shard_structure_stays_dense():
    need_gpu()
    case = _case(70, 3, (64, 128, 128))
    dev = case.x.device
    shard = ops.BucketedGraph.from_shard(case.ei[1], case.ei[0], case.et, case.n, case.n, case.r)
    assert shard.bipartite
    w, root, packed = _layer(case, 3, 64, 128, 1)
    assert not conv._sparse_agg(shard, False, False, packed, ops.absmax(case.x), 64)
    assert conv._sparse_agg(case.graph, False, False, packed, ops.absmax(case.x), 64)
    out = torch.full((case.n, 3 * 64), float("nan"), device=dev)
    assert torch.isfinite(ops.aggregate(shard, case.x, out=out)).all()
