"""GPU tier of the gather's adjoint in its edge weights (``ops.aggregate_weight_grad``; ``RGCN_MODE_WEIGHT_GRAD`` /
``RGCN_MODE_MEAN_GRAD`` of ``rgcn_aggregate_ex``, ``include/rgcn_hip.h``) against ``edge_grad_reference``: bit for bit on
integer tables, inside the derived bounds on random ones, over one graph whose (destination, relation) segments sit on
every boundary of the walk (a run of 8 ids, an item of 64 edges, a pack of 256, a partial row past it) and, at d = 4
only, one segment of 131,073 edges.  The reference walks the CSR the library built (``graph.arrays``)."""
import functools

import pytest
import torch

import edge_grad_reference as ref
import hub_graphs
from conftest import need_gpu
from guarded import bits
from primekg_rgcn_linkprediction_amd import ops

pytestmark = pytest.mark.gpu

N, R = 403, 3                                           # N is not a multiple of 32
PLANTED = [0, 1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1025]
FIRST, HUB_SRC, LONELY, BIG = 10, 5, 0, (3, 1, 131073)   # planted segment i: (FIRST + i, i % R); node 0 has no in-edge
DIMS = [4, 8, 28, 32, 64, 128, 256]
BOUND = 7                                               # |table entry|: d * 49 < 2^14 per dot, 256 dots < 2^22 per sum


def _edges(big=False, seed=11):
    gen = torch.Generator().manual_seed(seed)
    src, dst, rel = [], [], []
    for i, length in enumerate(PLANTED):
        s = torch.randint(1, N, (length,), generator=gen)
        if length >= 255:
            s[::2] = HUB_SRC                            # a source hub: long segments in the transposed direction, duplicates
        if length == 9:
            s[0] = FIRST + i                            # a self loop
        src.append(s), dst.append(torch.full((length,), FIRST + i)), rel.append(torch.full((length,), i % R))
    m = 1500                                            # background: destinations past the planted nodes
    src.append(torch.randint(1, N, (m,), generator=gen)), dst.append(torch.randint(30, N, (m,), generator=gen))
    rel.append(torch.randint(0, R, (m,), generator=gen))
    if big:
        node, r, length = BIG
        src.append(torch.randint(1, N, (length,), generator=gen)), dst.append(torch.full((length,), node))
        rel.append(torch.full((length,), r))
    src, dst, rel = torch.cat(src), torch.cat(dst), torch.cat(rel)
    order = torch.randperm(src.numel(), generator=gen)
    return src[order].contiguous(), dst[order].contiguous(), rel[order].contiguous()


@functools.lru_cache(maxsize=None)
def _graph(kind):
    """-> (BucketedGraph, {transposed: (rowptr, col, perm) on the CPU}) of "main", "big" or "one_rel" """
    dev = need_gpu()
    src, dst, rel = _edges(big=kind == "big")
    r = R
    if kind == "one_rel":
        rel, r = torch.zeros_like(rel), 1
    g = ops.BucketedGraph(torch.stack([src, dst]).to(dev), rel.to(dev), N, r)
    arrays = {t: tuple(a.cpu().long() for a in g.arrays(t)[:3]) for t in (False, True)}
    lens = torch.bincount(dst * r + rel, minlength=N * r)
    if kind != "one_rel":
        for i, length in enumerate(PLANTED):
            assert int(lens[(FIRST + i) * r + i % r]) == length
        assert int(lens[LONELY * r:(LONELY + 1) * r].sum()) == 0
        assert int(torch.bincount(src * r + rel, minlength=N * r).max()) > 512       # the source hub
        assert int((src == dst).sum()) >= 1
    if kind == "big":
        assert int(lens[BIG[0] * r + BIG[1]]) == BIG[2] and g.num_levels(False) == 3
    return g, arrays


def _int_table(rows, d, seed):
    parts = [hub_graphs.int_table(d, BOUND, seed + i) for i in range(-(-rows // hub_graphs.N))]
    return torch.cat(parts)[:rows].contiguous()


def _random(rows, d, seed):
    return torch.randn(rows, d, generator=torch.Generator().manual_seed(seed))


def _run(g, x, gagg, **kw):
    dev = g.device
    out = ops.aggregate_weight_grad(g, x.float().to(dev), gagg.float().reshape(g.num_nodes, -1).to(dev), **kw)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("transposed", [False, True], ids=["forward", "transposed"])
@pytest.mark.parametrize("d", DIMS)
def test_integer_tables_give_the_plain_mode_bit_for_bit(d, transposed):
    g, arrays = _graph("main")
    rowptr, col, _ = arrays[transposed]
    x, gagg = _int_table(N, d, 100 + d), _int_table(N * R, d, 200 + d)
    want = ref.plain_int(rowptr, col, x, gagg)
    assert int(want.abs().max()) < 2 ** 24
    got = _run(g, x, gagg, transposed=transposed)
    assert got.shape == (g.num_edges,) and torch.equal(bits(got), bits(want.float()))


@pytest.mark.parametrize("d", DIMS)
def test_integer_tables_give_the_mean_mode_bit_for_bit_on_power_of_two_segments(d):
    g, arrays = _graph("main")
    rowptr, col, _ = arrays[False]
    x, gagg = _int_table(N, d, 300 + d), _int_table(N * R, d, 400 + d)
    want, exact = ref.mean_int_pow2(rowptr, col, x, gagg)
    length = (rowptr[1:] - rowptr[:-1])[ref.segments_of(rowptr)]
    assert {1, 2, 8, 64, 256} <= set(length[exact].tolist())
    got = _run(g, x, gagg, through_mean=True)
    assert torch.equal(bits(got[exact]), bits(want[exact]))


def _check_bounded(g, arrays, d, seed, directions=(False, True)):
    n, r = g.num_nodes, g.num_relations
    x, gagg = _random(n, d, seed), _random(n * r, d, seed + 1)
    for transposed in directions:
        rowptr, col, _ = arrays[transposed]
        want, eps = ref.plain(rowptr, col, x, gagg)
        got = _run(g, x, gagg, transposed=transposed).double()
        worst = float(((got - want).abs() / eps).max())
        print(f"d={d} transposed={transposed}: plain error / bound = {worst:.3f}")
        assert bool(((got - want).abs() <= eps).all())
    rowptr, col, _ = arrays[False]
    want, bound = ref.mean(rowptr, col, x, gagg)
    got32 = _run(g, x, gagg, through_mean=True)
    got = got32.double()
    print(f"d={d}: mean error / bound = {float(((got - want).abs() / bound).max()):.3f}")
    assert bool(((got - want).abs() <= bound).all())
    seg, ns = ref.segments_of(rowptr), rowptr.numel() - 1
    sums = torch.zeros(ns, dtype=torch.float64).index_add_(0, seg, got)
    assert bool((sums.abs() <= torch.zeros(ns, dtype=torch.float64).index_add_(0, seg, bound)).all())
    single = (rowptr[1:] - rowptr[:-1])[seg] == 1
    assert int(single.sum()) >= 1 and not bits(got32[single]).any()                 # exactly +0.0f


@pytest.mark.parametrize("d", DIMS)
def test_random_tables_stay_inside_the_derived_bounds(d):
    g, arrays = _graph("main")
    _check_bounded(g, arrays, d, 500 + d)


def test_one_relation():
    g, arrays = _graph("one_rel")
    _check_bounded(g, arrays, 64, 600)


def test_a_segment_of_131073_edges_at_d_4():
    g, arrays = _graph("big")
    for transposed in (False, True):
        rowptr, col, _ = arrays[transposed]
        x, gagg = _int_table(N, 4, 700), _int_table(N * R, 4, 701)
        got = _run(g, x, gagg, transposed=transposed)
        assert torch.equal(bits(got), bits(ref.plain_int(rowptr, col, x, gagg).float()))
    _check_bounded(g, arrays, 4, 710, directions=())
    x, gagg = _random(N, 4, 720), _random(N * R, 4, 721)
    assert torch.equal(bits(_run(g, x, gagg, through_mean=True)), bits(_run(g, x, gagg, through_mean=True)))


@pytest.mark.parametrize("d", [28, 128])
def test_two_calls_give_the_same_bits_and_original_order_is_the_bucketed_result_through_perm(d):
    g, arrays = _graph("main")
    x, gagg = _random(N, d, 800 + d), _random(N * R, d, 801 + d)
    for kw in (dict(), dict(transposed=True), dict(through_mean=True)):
        a, b = _run(g, x, gagg, **kw), _run(g, x, gagg, **kw)
        assert torch.equal(bits(a), bits(b))
        perm = arrays[bool(kw.get("transposed"))][2]
        by_column = _run(g, x, gagg, original_order=True, **kw)
        assert sorted(perm.tolist()) == list(range(g.num_edges))
        assert torch.equal(bits(by_column[perm]), bits(a))


def test_a_weighted_shard_and_an_edge_dropout_view_take_the_plain_mode_only():
    g, arrays = _graph("main")
    dev, d = g.device, 32
    x, gagg = _random(N, d, 900), _random(N * R, d, 901)
    ed = ops.EdgeDropout(g)
    try:
        ed.draw(0.5, torch.tensor([7, 1], device=dev))
        for transposed in (False, True):                  # the view shares the parent's CSR; its weights are not read
            assert torch.equal(bits(_run(ed.view, x, gagg, transposed=transposed)), bits(_run(g, x, gagg, transposed=transposed)))
        with pytest.raises(NotImplementedError):
            _run(ed.view, x, gagg, through_mean=True)
    finally:
        ed.destroy()
    src, dst, rel = _edges()
    keep = dst < 60
    n_key = 60
    weight = torch.rand(int(keep.sum()), generator=torch.Generator().manual_seed(3)) + 0.5
    shard = ops.BucketedGraph.from_shard(dst[keep].to(dev), src[keep].to(dev), rel[keep].to(dev), n_key, N, R, weight.to(dev))
    try:
        rowptr, col = (a.cpu().long() for a in shard.arrays(False)[:2])
        assert int((rowptr[1:] - rowptr[:-1]).max()) == 1025
        want, eps = ref.plain(rowptr, col, x, gagg[:n_key * R])
        got = _run(shard, x, gagg[:n_key * R]).double()
        assert got.numel() == int(keep.sum()) and bool(((got - want).abs() <= eps).all())
        with pytest.raises(NotImplementedError):
            _run(shard, x, gagg[:n_key * R], through_mean=True)
        with pytest.raises(ValueError):
            _run(shard, x, gagg[:n_key * R], transposed=True)
    finally:
        shard.destroy()


def test_the_wrapper_checks_its_operands():
    g, _ = _graph("main")
    dev = g.device
    x, gagg = torch.zeros(N, 8, device=dev), torch.zeros(N, R * 8, device=dev)
    with pytest.raises(NotImplementedError):
        ops.aggregate_weight_grad(g, x.half(), gagg)
    with pytest.raises(NotImplementedError):
        ops.aggregate_weight_grad(g, torch.zeros(N, 260, device=dev), torch.zeros(N, R * 260, device=dev))
    with pytest.raises(NotImplementedError):
        ops.aggregate_weight_grad(g, x, gagg, transposed=True, through_mean=True)
    for bad_x, bad_g in ((x[:-1], gagg), (x, gagg[:, :-8]), (torch.zeros(N, 6, device=dev), torch.zeros(N, R * 6, device=dev))):
        with pytest.raises(ValueError):
            ops.aggregate_weight_grad(g, bad_x.contiguous(), bad_g.contiguous())
    with pytest.raises(RuntimeError):
        ops.aggregate_weight_grad(g, x.cpu(), gagg)
    lib_code = ops._lib.load().rgcn_aggregate_ex(g.handle, 1, x.data_ptr(), 8 | 16, 8, gagg.data_ptr(), x.data_ptr(), 1 << 30,
                                                 0, -1, None, None, None)
    assert lib_code == ops._lib.RGCN_ERR_UNSUPPORTED       # the library's own refusal of the mean mode on weights


@pytest.mark.parametrize("d", [8, 64])
def test_a_nan_source_row_reaches_exactly_the_edges_the_header_names(d):
    g, arrays = _graph("main")
    x, gagg = _random(N, d, 1000 + d), _random(N * R, d, 1001 + d)
    bad = 77
    x[bad, d // 2] = float("nan")
    for transposed in (False, True):
        rowptr, col, _ = arrays[transposed]
        reads = col == bad
        assert 0 < int(reads.sum()) < col.numel()
        assert torch.equal(torch.isnan(_run(g, x, gagg, transposed=transposed)), reads)
    rowptr, col, _ = arrays[False]
    seg = ref.segments_of(rowptr)
    hit = torch.zeros(rowptr.numel() - 1, dtype=torch.bool)
    hit[seg[col == bad]] = True
    assert int(hit[seg].sum()) > int((col == bad).sum())
    assert torch.equal(torch.isnan(_run(g, x, gagg, through_mean=True)), hit[seg])
