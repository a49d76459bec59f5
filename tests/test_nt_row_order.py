"""GPU tier: the split NT transforms with their row tiles in occupancy order (``conv._NT_ROW_ORDER``; ``row_order=`` of
``ops.transform_fwd`` / ``transform_bwd_input`` / ``transform_bwd_input_chain``, ``RGCN_MODE_ROW_ORDER`` of
``include/rgcn_row_order.h``).

Row order changes no bit of an NT product: which workgroup computes a row changes, the row's k loop does not.  So every
comparison here is of BYTES, the order bit on against off - launch by launch through the wrappers (one C call each, the
option word differing in that bit alone) and through ``rgcn_encoder2`` forward + backward - and every output and
workspace of the ordered runs is pre-filled with NaN (the allocation seam of ``test_sparse_aggregate.py``).

Graphs: occupancy scattered row by row (``test_row_order_host._graph``: all eight occupancy words, in turn), so every
natural tile has every relation and the ordered tiles do not; N = 40 (less than a tile), 130 and 193 (ragged last
tiles); and N = 150 with a 300-edge and a 600-edge segment on both sides, whose hub tails the gathers leave to the
transforms (``num_levels == 2``).

The chained launch splits its tile of ``gz`` under the TILE's own maximum before the second product, and the order
changes which rows share a tile: ``T`` keeps its bits wherever both halves of the split are exact under either scale -
everywhere but in lo halves that fall into fp16's subnormals.  The seeds below are ones for which every word of ``T``
agrees; nothing here compares under a tolerance."""
import functools

import numpy as np
import pytest
import torch

from conftest import need_gpu
from guarded import bits
from test_row_order_host import _graph
from test_sparse_aggregate import _same, poisoned
from primekg_rgcn_linkprediction_amd import RGCNConv, _lib, conv, ops, rgcn_encoder2

pytestmark = pytest.mark.gpu

NAN = float("nan")
CASES = {"n40": (40, ()), "n130": (130, ()), "n193": (193, ()),
         "hubs": (150, ((3, 0, 300), (77, 2, 600)))}


class Case:
    def __init__(self, n, hubs):
        dev = torch.device("cuda:0")
        r = 3
        self.n, self.r = n, r
        rng = np.random.default_rng(n)
        dst, rel = _graph(n, r, n)
        src = rng.integers(0, n, dst.size)
        if hubs:                                        # the long segments, once on the destination and once on the source side
            hub_key, hub_rel = _graph(0, r, 0, hubs)
            other = rng.integers(0, n, 2 * hub_key.size)
            dst = np.concatenate([dst, hub_key, other[:hub_key.size]])
            src = np.concatenate([src, other[hub_key.size:], hub_key])
            rel = np.concatenate([rel, hub_rel, hub_rel])
        self.ei = torch.from_numpy(np.stack([src, dst])).to(dev)
        self.et = torch.from_numpy(rel).to(dev)
        self.graph = ops.bucket(self.ei, self.et, n, r)
        gen = torch.Generator().manual_seed(n)
        self.x = {d: torch.randn(n, d, generator=gen).to(dev) for d in (64, 128)}
        self.gout = torch.randn(n, 128, generator=gen).to(dev)
        self.mask = torch.relu(torch.randn(n, 128, generator=gen)).to(dev)
        self.mask64 = torch.relu(torch.randn(n, 64, generator=gen)).to(dev)
        self.bias = torch.linspace(-1, 1, 128, device=dev)
        self.layers = {}
        for d_in in (64, 128):
            w = (torch.randn(r, d_in, 128, generator=gen) * 0.1).to(dev)
            root = (torch.randn(d_in, 128, generator=gen) * 0.1).to(dev)
            self.layers[d_in] = (w, root, ops.split_weights(w, root))
        torch.manual_seed(n)
        self.convs = [RGCNConv(64, 128, r).to(dev), RGCNConv(128, 128, r).to(dev)]
        for c in self.convs:
            c.bias.data.uniform_(-0.1, 0.1)
        self.cot = torch.randn(n, 128, generator=gen).to(dev)


@functools.lru_cache(maxsize=None)
def _case(name):
    need_gpu()
    return Case(*CASES[name])


def _hub_rows(case, transposed):
    """rows of the aggregate [N * R, d] that belong to segments of more than 256 edges (finished by the transform)"""
    key = case.ei[0 if transposed else 1] * case.r + case.et
    return torch.nonzero(torch.bincount(key, minlength=case.n * case.r) > 256).flatten()


def _gathered(case, table, transposed, sparse, amax_out=None):
    """the aggregate of `table` as a training pass forms it - hub tails deferred where the structure allows - in a
    buffer pre-filled with NaN -> (agg, hubs | None)"""
    g, d = case.graph, table.size(1)
    if sparse:
        out = torch.full((case.n, case.r * d), NAN, device=table.device)
        return ops.aggregate_sparse(g, table, transposed=transposed, out=out, defer=amax_out is None, amax_out=amax_out)
    if amax_out is None:
        return ops.aggregate_deferred(g, table, transposed=transposed)
    return ops.aggregate(g, table, transposed=transposed, amax_out=amax_out), None


def _bit_spy(monkeypatch):
    seen = []
    real = ops._order_bit
    monkeypatch.setattr(ops, "_order_bit", lambda *a: (seen.append(real(*a)), seen[-1])[1])
    return seen


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("name", list(CASES))
def test_each_launch_gives_the_same_bytes_in_either_order(name, sparse, monkeypatch):
    need_gpu()
    case = _case(name)
    g, dev = case.graph, case.gout.device
    assert g.row_order_ptr(False) is not None and g.row_order_ptr(True) is not None
    if name == "hubs":
        assert g.num_levels(False) == 2 and g.num_levels(True) == 2
    seen = _bit_spy(monkeypatch)

    def run(fn):
        """fn(row_order) -> tensors; node order in plain memory, occupancy order with every allocation pre-filled with NaN"""
        want = [bits(t) for t in fn(False)]
        with poisoned(monkeypatch, NAN, "wrappers"):
            got = [bits(t) for t in fn(True)]
        assert all(torch.isfinite(w.view(torch.float32)).all() for w in want)
        return got, want

    # forward NT, K = 256 and K = 512: ReLU and plain epilogues, bias on and off, the published maximum, deferred hub tails
    for d_in, relu, bias in ((64, True, case.bias), (128, False, None), (128, False, case.bias)):
        x = case.x[d_in]
        w, root, packed = case.layers[d_in]
        x_amax = ops.absmax(x)

        def fwd(order):
            agg, hubs = _gathered(case, x, False, sparse)
            assert (hubs is not None) == (name == "hubs")
            am = ops.amax_buffer(dev)
            out = ops.transform_fwd(agg, x, w, root, bias, relu=relu, graph=g, amax=(x_amax, x_amax), amax_out=am[0],
                                    packed=packed, hubs=hubs, sparse=sparse, row_order=order)
            return out, ops.amax_value(am), agg.view(case.n * case.r, d_in)[_hub_rows(case, False)]
        _same(*run(fwd), f"transform_fwd d_in={d_in}")

    # input-gradient NT: mask and plain epilogues, an output factor; the transposed aggregate under its own maximum
    w, root, packed = case.layers[128]
    g_amax = ops.absmax(case.gout)
    for mask, scale in ((case.mask, 1.25), (None, 1.0)):
        def bwd(order):
            am, gm = ops.amax_buffer(dev), ops.amax_buffer(dev)
            gagg, _ = _gathered(case, case.gout, True, sparse, amax_out=gm[0])
            gx = ops.transform_bwd_input(gagg, case.gout, w, root, relu_mask=mask, graph=g, amax=(gm[0], g_amax),
                                         amax_out=am[0], packed=packed, out_scale=scale, sparse=sparse, row_order=order)
            return gx, ops.amax_value(am)
        _same(*run(bwd), "transform_bwd_input")

    # the same with hub tails left to the launch (the bound scale: nothing published by the gather)
    def bwd_hubs(order):
        gagg, hubs = _gathered(case, case.gout, True, sparse)
        gx = ops.transform_bwd_input(gagg, case.gout, w, root, relu_mask=case.mask, graph=g, amax=(g_amax, g_amax),
                                     amax_mul=g.weight_bound(True), packed=packed, hubs=hubs, sparse=sparse, row_order=order)
        return gx, gagg.view(case.n * case.r, 128)[_hub_rows(case, True)]
    _same(*run(bwd_hubs), "transform_bwd_input with deferred hub tails")

    # the chained launch: gz, T and the published maximum
    w1, root1, packed1 = case.layers[64]
    assert ops.chain_supported(w, w1)
    for mask in (case.mask, None):
        def chain(order):
            am, gm = ops.amax_buffer(dev), ops.amax_buffer(dev)
            gagg, _ = _gathered(case, case.gout, True, sparse, amax_out=gm[0])
            gz, t = ops.transform_bwd_input_chain(gagg, case.gout, w, root, mask, packed, packed1, graph=g,
                                                  amax=(gm[0], g_amax), amax_out=am[0], sparse=sparse, row_order=order)
            return gz, t, ops.amax_value(am)
        _same(*run(chain), "transform_bwd_input_chain")
    assert _lib.MODE_ROW_ORDER in seen and 0 in seen


@pytest.mark.parametrize("regions", [False, True], ids=["wrappers", "replay"])
@pytest.mark.parametrize("name", list(CASES))
def test_encoder2_forward_and_backward_give_the_same_bytes(name, regions, monkeypatch):
    need_gpu()
    case = _case(name)
    monkeypatch.setattr(ops, "REGIONS", regions)
    seen = _bit_spy(monkeypatch)

    def step():
        x = case.x[64].clone().requires_grad_(True)
        for c in case.convs:
            c.zero_grad(set_to_none=True)
        out = rgcn_encoder2(x, case.ei, case.et, *case.convs)
        out.backward(case.cot)
        torch.cuda.synchronize()
        return [bits(t) for t in (out, x.grad, *(p.grad for c in case.convs for p in (c.weight, c.root, c.bias)))]

    results = {}
    for order in (False, True):
        monkeypatch.setattr(conv, "_NT_ROW_ORDER", order)
        runs = [step() for _ in range(4 if regions else 1)]         # plain, sizing, recording, a replay
        if order:
            with poisoned(monkeypatch, NAN, "replay" if regions else "wrappers"):
                runs.append(step())
        results[order] = runs
    want = results[False][0]
    assert all(torch.isfinite(w.view(torch.float32)).all() for w in want)
    for k, got in enumerate(results[False] + results[True]):
        _same(got, want, f"run {k}")
    assert _lib.MODE_ROW_ORDER in seen and 0 in seen


def test_the_bit_is_refused_where_there_is_no_order():
    need_gpu()
    case = _case("n130")
    lib = _lib.load()
    x = case.x[64]
    w, root, packed = case.layers[64]
    agg = ops.aggregate(case.graph, x)
    out = torch.empty(case.n, 128, device=x.device)
    nbytes = lib.rgcn_transform_split_workspace_bytes(case.r, 64, 128)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    x_amax = ops.absmax(x)

    def call(mask, mode):
        return lib.rgcn_transform_fwd_split(agg.data_ptr(), x.data_ptr(), w.data_ptr(), root.data_ptr(), packed.buf.data_ptr(),
                                            None, 0, mask, case.n, case.r, 64, 128, x_amax.data_ptr(), 1.0,
                                            x_amax.data_ptr(), mode, out.data_ptr(), None, ws.data_ptr(), nbytes,
                                            torch.cuda.current_stream().cuda_stream, None, 0, None)
    assert call(None, _lib.MODE_ROW_ORDER) == _lib.RGCN_ERR_ARG               # no occupancy allocation
    assert call(case.graph.tile_mask_ptr(False), _lib.MODE_ROW_ORDER | 1) == _lib.RGCN_ERR_UNSUPPORTED   # one-pass fp16
    assert call(case.graph.tile_mask_ptr(False), _lib.MODE_ROW_ORDER) == _lib.RGCN_OK
    torch.cuda.synchronize()
    want = ops.transform_fwd(agg, x, w, root, None, graph=case.graph, amax=(x_amax, x_amax), packed=packed)
    assert torch.equal(bits(out), bits(want))
    # a policy that asks for the order where the wrapper cannot give it runs in node order: one-pass fp16, no graph
    assert ops._order_bit(True, case.graph, False, 2) == 0 and ops._order_bit(True, None, False, 1) == 0
    assert ops._order_bit(False, case.graph, False, 1) == 0 and ops._order_bit(True, case.graph, True, 1) == _lib.MODE_ROW_ORDER
