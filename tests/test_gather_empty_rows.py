"""GPU tier: the rows of (node, relation) segments without an edge, which the level-0 gather launch stores from
zero-fill workgroups beside the walk instead of walking them (csrc/rgcn_aggregate.hip, rgcn_csr::empty_items0).

Expected values are a float64 NumPy restatement written here, cast to float32 - never another route of the library -
and the comparison is exact by construction: table entries are integers in [-8, 8]; where a structure is weighted
(transposed, merged) every counted degree of the graph is 1, 2, 4 or 8, so every weight 1 / cnt is a power of two and
every product and partial sum is a multiple of 1/8 below 2^15: exact in float32 in any order.  The mean divides an
exact integer sum by an integer count once, correctly rounded on both sides (float64 then float32 rounds a quotient of
two 24-bit operands like one float32 division).  Outputs are allocated through tests/guarded.py filled with 0xFF
(NaN), so a row nobody wrote shows, and the bands around them are checked.

The gather proper covers the live slots rounded up to whole workgroups of 256 / G slots (G = d / 4 lanes per row);
a zero-fill workgroup takes ZERO_ROWS of the items behind them."""
import functools

import numpy as np
import pytest
import torch

from conftest import need_gpu
from guarded import GuardedAllocator, installed
from primekg_rgcn_linkprediction_amd import RGCNConv, ops
from test_gpu_parity import assert_grad                # the parameter-gradient tolerance of the float64 comparison

pytestmark = pytest.mark.gpu

ZERO_ROWS = 64                                         # RGCN_ZERO_ROWS
POW2 = np.array([1, 2, 4, 8])


# ------------------------------------------------------------------------------------------------------------ graphs
def _graph(seed, n, r, live_per_rel, hubs=(), hub_side="out"):
    """-> (src, dst, rel) int64.  Per relation k: ``live_per_rel[k]`` destination nodes and as many source nodes, joined
    one to one, then further edges from those sources until every (dst, rel) in-degree is 1, 2, 4 or 8: exactly
    sum(live_per_rel) live segments in BOTH directions (without hubs).  ``hubs``: (relation, edges) - ``"out"``: a source
    with that many out-edges to otherwise unused destinations (in-degree 1: the weights stay powers of two);
    ``"in"``: a destination with that many in-edges (mean structure only: 1 / 300 is no power of two)."""
    rng = np.random.default_rng(seed)
    src, dst, rel = [], [], []
    base = n - len(hubs)                               # the hub nodes are the last ones
    for k in range(r):
        live = live_per_rel[k]
        used_dst = np.empty(0, dtype=np.int64)
        if live:
            d_nodes, s_nodes = rng.choice(base, live, replace=False), rng.choice(base, live, replace=False)
            extra_dst = np.repeat(d_nodes, rng.choice(POW2, live) - 1)
            src += [s_nodes, rng.choice(s_nodes, extra_dst.size)]
            dst += [d_nodes, extra_dst]
            rel.append(np.full(live + extra_dst.size, k))
            used_dst = d_nodes
        for h, (hub_rel, edges) in enumerate(hubs):
            if hub_rel != k:
                continue
            hub = np.full(edges, base + h)
            if hub_side == "out":
                others = rng.choice(np.setdiff1d(np.arange(base), used_dst), edges, replace=False)
                used_dst = np.concatenate([used_dst, others])
                src.append(hub); dst.append(others)
            else:
                src.append(rng.integers(0, base, edges)); dst.append(hub)
            rel.append(np.full(edges, k))
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.empty(0, dtype=np.int64)   # noqa: E731
    src, dst, rel = cat(src), cat(dst), cat(rel)
    order = rng.permutation(src.size)                  # the column order of the input must not matter to the bucketing
    return src[order], dst[order], rel[order]


class Case:
    """one graph on the device with its edge list and counted degrees"""

    def __init__(self, dev, n, r, edges):
        self.n, self.r, (self.src, self.dst, self.rel) = n, r, edges
        assert n <= 2000 and self.src.size <= 20000
        self.cnt = np.bincount(self.dst * r + self.rel, minlength=n * r)          # in-degree per (dst, rel)
        self.cnt_t = np.bincount(self.src * r + self.rel, minlength=n * r)        # out-degree per (src, rel)
        ei = torch.from_numpy(np.stack([self.src, self.dst])).to(dev)
        self.ei, self.et = ei, torch.from_numpy(self.rel).to(dev)
        self.g = ops.BucketedGraph(self.ei, self.et, n, r)
        self.pow2 = bool(np.isin(self.cnt[self.cnt > 0], POW2).all())

    # ---- the float64 restatement -------------------------------------------------------------------------------
    def mean(self, x):
        s = np.zeros((self.n * self.r, x.shape[1]))
        np.add.at(s, self.dst * self.r + self.rel, x.astype(np.float64)[self.src])
        return (s / np.maximum(self.cnt, 1)[:, None]).astype(np.float32).reshape(self.n, -1)

    def weights(self):
        return 1.0 / np.maximum(self.cnt, 1)[self.dst * self.r + self.rel].astype(np.float64)

    def transposed(self, g):
        s = np.zeros((self.n * self.r, g.shape[1]))
        np.add.at(s, self.src * self.r + self.rel, g.astype(np.float64)[self.dst] * self.weights()[:, None])
        return s.astype(np.float32).reshape(self.n, -1)

    def merged(self, t):
        """t: [n * (r + 1), d] -> [n, d]: out-edges of all relations, plus the node's own root row with weight 1"""
        t = t.astype(np.float64)
        s = t.reshape(self.n, self.r + 1, -1)[:, self.r].copy()
        np.add.at(s, self.src, t[self.dst * (self.r + 1) + self.rel] * self.weights()[:, None])
        return s.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(kind, *args):
    dev = torch.device("cuda:0")
    if kind == "sized":                                # exactly `rest` items behind the walked workgroups at row width d
        d, rest, short, r = args
        slots = 256 // max(d // 4, 1)
        k = next(k for k in range(40, 80) if (slots * k + rest) % r == 0)
        n, live = (slots * k + rest) // r, slots * k - short
        per_rel = [live // r + (i < live % r) for i in range(r)]
        c = Case(dev, n, r, _graph(1000 * d + 10 * rest + short, n, r, per_rel))
        assert int((c.cnt == 0).sum()) == int((c.cnt_t == 0).sum()) == rest + short    # the premise of the case
        return c
    if kind == "hubs":                                 # case 4: a pack (300 edges) and partial rows + level 1 (1,500)
        side, r, n = args if len(args) == 3 else args + (2000,)
        return Case(dev, n, r, _graph(7 + r, n, r, [25] * r, hubs=((0, 300), (1, 1500)), hub_side=side))
    if kind == "single":                               # case 5: one edge
        return Case(dev, 50, 3, (np.array([7]), np.array([31]), np.array([1])))
    raise KeyError(kind)


def _ints(seed, rows, d):
    return np.random.default_rng(seed).integers(-8, 9, (rows, d)).astype(np.float32)


def _run(monkeypatch, fn):
    """fn() with every output allocated NaN-filled between guard bands -> its result, bands checked"""
    alloc = GuardedAllocator(0xFF)
    with installed(monkeypatch, alloc):
        got = fn()
        torch.cuda.synchronize()
    alloc.check()
    return got


def _same(got, want, empty_rows):
    """equal values everywhere; the rows of empty segments hold the bits of +0.0"""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    assert not np.isnan(got).any(), f"{int(np.isnan(got).any(axis=1).sum())} rows hold a NaN nobody overwrote"
    assert np.array_equal(got, want)
    rows = got.reshape(empty_rows.size, -1)[empty_rows]
    assert not rows.view(np.uint32).any(), "an empty segment's row is not all +0.0"


def _check_directions(monkeypatch, c, d, seed=0, merged=True):
    dev = c.ei.device
    x = _ints(seed, c.n, d)
    xd = torch.from_numpy(x).to(dev)
    _same(_run(monkeypatch, lambda: ops.aggregate(c.g, xd)), c.mean(x), c.cnt == 0)
    if not c.pow2:
        return
    _same(_run(monkeypatch, lambda: ops.aggregate(c.g, xd, transposed=True)), c.transposed(x), c.cnt_t == 0)
    if merged:
        t = _ints(seed + 1, c.n * (c.r + 1), d)
        m = c.g.merged_transposed()
        got = _run(monkeypatch, lambda: ops.aggregate(m, torch.from_numpy(t).to(dev)))
        _same(got, c.merged(t), np.zeros(c.n, dtype=bool))


# ------------------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("r", [3, 5])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_row_widths_mean_transposed_and_merged(d, r, monkeypatch):
    """case 1 (and 2: `short` = 3 leaves a boundary workgroup with live and empty items, 0 none)"""
    need_gpu()
    for short in (3, 0):
        _check_directions(monkeypatch, _case("sized", d, 2 * ZERO_ROWS + 9, short, r), d, seed=d + r)


@pytest.mark.parametrize("rest", [0, 1, ZERO_ROWS - 1, ZERO_ROWS, ZERO_ROWS + 1])
@pytest.mark.parametrize("d", [64, 128])
def test_zero_fill_item_counts_around_one_workgroup(d, rest, monkeypatch):
    """case 3 (with case 2's two boundaries): 0, 1, ZERO_ROWS - 1, ZERO_ROWS and ZERO_ROWS + 1 items behind the walked
    workgroups, with the live slots a whole number of workgroups and three short of it"""
    need_gpu()
    for short in (0, 3):
        _check_directions(monkeypatch, _case("sized", d, rest, short, 3), d, seed=rest, merged=False)


@pytest.mark.parametrize("r", [3, 5])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_empty_segments_among_hubs(d, r, monkeypatch):
    """case 4: a segment of 300 edges (a pack) and one of 1,500 (partial rows, then level 1) among mostly empty ones -
    as in-degree hubs for the mean, as out-degree hubs (all in-degrees powers of two) for the weighted structures"""
    need_gpu()
    c_in, c_out = _case("hubs", "in", r), _case("hubs", "out", r)
    assert not c_in.pow2 and c_out.pow2 and c_in.cnt.max() == 1500 and c_out.cnt_t.max() == 1500
    assert (c_in.cnt == 0).mean() > 0.9 and (c_out.cnt_t == 0).mean() > 0.9
    assert c_out.g.num_levels(True) == 2 and c_in.g.num_levels(False) == 2
    _check_directions(monkeypatch, c_in, d, seed=d)
    _check_directions(monkeypatch, c_out, d, seed=d + 1)


@pytest.mark.parametrize("d", [32, 128, 512])
def test_single_edge(d, monkeypatch):
    """case 5: every segment but one is empty"""
    need_gpu()
    _check_directions(monkeypatch, _case("single"), d)


def test_published_maximum_ignores_empty_segments(monkeypatch):
    """case 6: the transposed gather's amax_out is max |gagg| of the reference, with and without further empty segments
    (isolated nodes appended to the same edge list)"""
    dev = need_gpu()
    c = _case("hubs", "out", 3, 1667)
    wider = Case(dev, c.n + 333, c.r, (c.src, c.dst, c.rel))
    g = _ints(11, wider.n, 128)
    seen = []
    for case in (c, wider):
        gd = torch.from_numpy(g[:case.n]).to(dev)
        want = case.transposed(g[:case.n])
        slot = ops.amax_buffer(dev)[0]
        _same(_run(monkeypatch, lambda: ops.aggregate(case.g, gd, transposed=True, amax_out=slot)), want, case.cnt_t == 0)
        seen.append(ops.amax_value(slot).item())
        assert seen[-1] == float(np.abs(want).max()) > 0
    assert seen[0] == seen[1]
    assert np.array_equal(c.transposed(g[:c.n]), wider.transposed(g)[:c.n])


def _layer_f64(c, x, w, root, bias, cot):
    """one layer and its backward in float64 -> (out, grad_x, grad_weight, grad_root, grad_bias)"""
    n, r, d_in = c.n, c.r, x.shape[1]
    key = c.dst * r + c.rel
    s = np.zeros((n * r, d_in))
    np.add.at(s, key, x[c.src])
    agg = (s / np.maximum(c.cnt, 1)[:, None]).reshape(n, r * d_in)
    out = agg @ w.reshape(r * d_in, -1) + x @ root + bias
    gagg = (cot @ w.reshape(r * d_in, -1).T).reshape(n * r, d_in) / np.maximum(c.cnt, 1)[:, None]
    gx = cot @ root.T
    np.add.at(gx, c.src, gagg[key])
    return out, gx, (agg.T @ cot).reshape(w.shape), x.T @ cot, cot.sum(0)


def test_layer_backward_with_the_slab_reduction_riding():
    """case 7: one backward of one layer on case 4's graph.  128 -> 128 takes the gather-first input gradient, whose
    transposed gather carries the parameter gradients' slab reduction as riders of the launch that also has the
    zero-fill workgroups; parameter (and input) gradients against the float64 backward at test_gpu_parity's tolerance"""
    dev = need_gpu()
    c = _case("hubs", "out", 3)
    torch.manual_seed(3)
    conv = RGCNConv(128, 128, c.r).to(dev)
    gen = torch.Generator().manual_seed(4)
    x, cot = torch.randn(c.n, 128, generator=gen), torch.randn(c.n, 128, generator=gen)
    xd = x.to(dev).requires_grad_(True)

    (conv(xd, c.ei, c.et) * cot.to(dev)).sum().backward()     # (the layer's passes allocate from their own arenas: no poison)
    f64 = lambda t: t.detach().cpu().double().numpy()                                                     # noqa: E731
    want = _layer_f64(c, f64(x), f64(conv.weight), f64(conv.root), f64(conv.bias), f64(cot))
    for got, ref in zip((xd.grad, conv.weight.grad, conv.root.grad, conv.bias.grad), want[1:]):
        assert_grad(got, torch.from_numpy(ref))


def test_riders_and_zero_fill_in_one_launch(monkeypatch):
    """case 7, at the operator: a deferred parameter-gradient reduction handed to the transposed gather as its tail -
    the gathered rows stay exact, the reduced gradients meet float64 at the same tolerance"""
    dev = need_gpu()
    c = _case("hubs", "out", 3)
    x, gout = _ints(5, c.n, 64), _ints(6, c.n, 128)
    xd, gd = torch.from_numpy(x).to(dev), torch.from_numpy(gout).to(dev)
    agg = ops.aggregate(c.g, xd)

    def fn():
        pend = ops.transform_bwd_params(agg, xd, gd, c.r, graph=c.g, defer=True)
        rows = ops.aggregate(c.g, gd, transposed=True, tail=pend)
        assert pend.done
        return rows, pend.grads

    rows, (gw, groot, gbias) = _run(monkeypatch, fn)
    _same(rows, c.transposed(gout), c.cnt_t == 0)
    a64, g64 = c.mean(x).astype(np.float64), gout.astype(np.float64)
    assert_grad(gw, torch.from_numpy((a64.T @ g64).reshape(c.r, 64, 128)))
    assert_grad(groot, torch.from_numpy(x.astype(np.float64).T @ g64))
    assert_grad(gbias, torch.from_numpy(g64.sum(0)))


@pytest.mark.parametrize("short", [0, 3])
def test_unchanged_paths_wide_rows_and_fp16_table(short, monkeypatch):
    """case 8: d = 512 runs a 2-D grid and the fp16 table has a kernel of its own; both walk every item as before"""
    dev = need_gpu()
    c = _case("sized", 128, ZERO_ROWS + 1, short, 3)
    _check_directions(monkeypatch, c, 512, merged=False)
    for case, d in ((c, 64), (c, 128), (_case("hubs", "in", 3), 128)):
        x = _ints(d, case.n, d)
        got = _run(monkeypatch, lambda: ops.aggregate(case.g, torch.from_numpy(x).to(dev).half()))
        _same(got, case.mean(x), case.cnt == 0)
