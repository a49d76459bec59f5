"""GPU tier: the HIP path (through the C ABI) against the oracle and the golden fixtures.

Tolerances (BASELINE.json north_star / SURVEY.md section 8d): bucketing bit exact;
forward max|delta| <= 1e-5 fp32; gradients <= 1e-4 relative to the largest entry.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import LAYER_CASES, load_golden, need_gpu
from oracle import rgcn_oracle as O
from primekg_rgcn_linkprediction_amd import (DrugDiseaseModel, LinkPredictor, RGCNConv, distmult, ops,
                                             rgcn_conv, rgcn_encoder2, synth)

pytestmark = pytest.mark.gpu

FWD_ATOL = 1e-5
GRAD_RTOL = 1e-4


def rel_err(got, want):
    want = want.double()
    return ((got.double().cpu() - want).abs().max() / (want.abs().max() + 1e-30)).item()


def assert_fwd(got, want, atol=FWD_ATOL):
    err = (got.double().cpu() - want.double()).abs().max().item() if want.numel() else 0.0
    assert err <= atol, f"forward differs by {err:.3e} (> {atol})"


def assert_grad(got, want, rtol=GRAD_RTOL):
    if want.numel() == 0:
        return
    if want.abs().max() == 0:
        assert got.abs().max().item() == 0
        return
    err = rel_err(got, want)
    assert err <= rtol, f"gradient differs by {err:.3e} relative (> {rtol})"


# ------------------------------------------------------------------ bucketing: bit exact
def _check_bucket(dev, ei, et, n, r):
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    fw = O.bucket_ref(ei, et, n, r, transpose=False)
    bw = O.bucket_ref(ei, et, n, r, transpose=True)
    for transposed, ref in ((False, fw), (True, bw)):
        rowptr, col, perm, val = [t.cpu().numpy() for t in g.arrays(transposed)]
        assert np.array_equal(rowptr, ref[0]) and rowptr.dtype == np.int32
        assert np.array_equal(col, ref[1]) and col.dtype == np.int32
        assert np.array_equal(perm, ref[2]) and perm.dtype == np.int64
        if not transposed:
            assert np.array_equal(val, ref[3])
        else:                                   # w_t[e] = 1 / cnt[dst*R + rel], same fp32 division
            dst, rel = ei[1].numpy()[ref[2]], et.numpy()[ref[2]]
            want = (np.float32(1.0) / fw[3][dst * r + rel]).astype(np.float32)
            assert np.array_equal(val, want)
    return g


@pytest.mark.parametrize("case", LAYER_CASES)
def test_bucket_golden_bit_exact(case):
    dev = need_gpu()
    z = load_golden(f"bucket_{case}.npz")
    g = ops.BucketedGraph(z["edge_index"].to(dev), z["edge_type"].to(dev), z["num_nodes"], z["num_relations"])
    for transposed, sfx in ((False, ""), (True, "_t")):
        rowptr, col, perm, val = [t.cpu() for t in g.arrays(transposed)]
        assert torch.equal(rowptr, z["rowptr" + sfx]) and torch.equal(col, z["col" + sfx])
        assert torch.equal(perm, z["perm" + sfx])
        if not transposed:
            assert torch.equal(val, z["cnt"])


def test_bucket_random_and_real_graphs_bit_exact():
    dev = need_gpu()
    ei, et, n, r = synth.uniform_graph(1000, 10000, 3, seed=42)              # C1
    _check_bucket(dev, ei, et, n, r)
    ei, et, n, r = synth.uniform_graph(777, 50001, 16, seed=1)                # R = 16, odd E
    _check_bucket(dev, ei, et, n, r)
    z = load_golden("primekg_test_edges.npz")                                  # real PrimeKG subgraph
    _check_bucket(dev, z["edge_index"].long(), z["edge_type"].long(), 30926, 3)
    ei, et, n, r = synth.primekg_like(seed=42)                                 # C2 full size
    g = _check_bucket(dev, ei, et, n, r)
    assert g.num_levels(False) >= 2 and g.num_levels(True) >= 2               # heavy segments split


def test_bucket_rejects_out_of_range_ids():
    dev = need_gpu()
    ei = torch.tensor([[0, 1, 5], [1, 2, 0]], device=dev)
    et = torch.tensor([0, 1, 0], device=dev)
    with pytest.raises(IndexError):
        ops.BucketedGraph(ei, et, 5, 2)                  # node 5 >= N (train.py:571-586 filters these)
    with pytest.raises(IndexError):
        ops.BucketedGraph(ei, et, 6, 1)                  # relation 1 >= R
    with pytest.raises(IndexError):
        ops.BucketedGraph(torch.tensor([[0, -1], [1, 0]], device=dev), torch.tensor([0, 0], device=dev), 3, 1)
    ops.BucketedGraph(ei, et, 6, 2)


def test_failed_bucketing_frees_what_it_allocated():
    """every device allocation of rgcn_graph_create belongs to the scratch object (freed by its destructor) or to
    the handle (freed by rgcn_graph_destroy on the error path): 40 creations that fail at the range check, each
    holding ~70 MB of sort scratch and half-built structure, must not lower the device's free memory."""
    dev = need_gpu()
    n, e = 100_000, 3_000_000
    gen = torch.Generator().manual_seed(0)
    ei = torch.randint(0, n, (2, e), generator=gen)
    ei[1, e - 1] = n + 5                                            # one id out of range, found after the allocations
    eid, etd = ei.to(dev), torch.zeros(e, dtype=torch.int64, device=dev)
    with pytest.raises(IndexError):
        ops.BucketedGraph(eid, etd, n, 2)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    for _ in range(40):
        with pytest.raises(IndexError):
            ops.BucketedGraph(eid, etd, n, 2)
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info(dev)[0] < 64 * 2 ** 20


def test_graph_cache_hits_and_invalidates():
    dev = need_gpu()
    ops.clear_graph_cache()
    ei, et, n, r = synth.uniform_graph(50, 300, 3, seed=3)
    ei, et = ei.to(dev), et.to(dev)
    a = ops.bucket(ei, et, n, r)
    assert ops.bucket(ei, et, n, r) is a                  # conv1 and conv2 share one bucketing
    et[0] = (et[0] + 1) % r                               # in-place edit bumps _version
    b = ops.bucket(ei, et, n, r)
    assert b is not a
    assert ops.bucket(ei.clone(), et, n, r) is not b
    ops.clear_graph_cache()



# ------------------------------------------------------------------ persisted structure (section 8f row 3)
def test_sidecar_round_trip_is_bitwise_and_skips_nothing(tmp_path):
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=60000, seed=3)
    ei, et = ei.to(dev), et.to(dev)
    a = ops.BucketedGraph(ei, et, n, r)
    a.save(tmp_path / "g.bucketed.pt")
    b = ops.BucketedGraph.load(tmp_path / "g.bucketed.pt", dev)
    for transposed in (False, True):
        for x, y in zip(a.arrays(transposed), b.arrays(transposed)):
            assert torch.equal(x, y)
        assert a.num_levels(transposed) == b.num_levels(transposed)
    x = torch.randn(n, 64, device=dev)
    for transposed in (False, True):
        assert torch.equal(ops.aggregate(a, x, transposed), ops.aggregate(b, x, transposed))
    # layer through the imported structure == layer through the sorted one (tile masks included)
    torch.manual_seed(0)
    conv = RGCNConv(64, 128, r).to(dev)
    with torch.no_grad():
        ya = ops.transform_fwd(ops.aggregate(a, x), x, conv.weight, conv.root, conv.bias, graph=a)
        yb = ops.transform_fwd(ops.aggregate(b, x), x, conv.weight, conv.root, conv.bias, graph=b)
    assert torch.equal(ya, yb)


def test_sidecar_is_used_checked_and_rewritten(tmp_path):
    dev = need_gpu()
    ops.clear_graph_cache()
    path = tmp_path / "train_data.bucketed.pt"
    ei, et, n, r = synth.uniform_graph(300, 4000, 3, seed=8)
    ei, et = ei.to(dev), et.to(dev)
    g1 = ops.bucket(ei, et, n, r, sidecar=path)                # sorts, writes the file
    assert path.exists()
    ops.clear_graph_cache()
    g2 = ops.bucket(ei, et, n, r, sidecar=path)                # imports
    assert all(torch.equal(x, y) for x, y in zip(g1.arrays(False), g2.arrays(False)))
    # a file that belongs to other columns is detected and replaced
    ops.clear_graph_cache()
    ei2 = ei.clone()
    ei2[0, 7] = (ei2[0, 7] + 1) % n
    g3 = ops.bucket(ei2, et, n, r, sidecar=path)
    want = ops.BucketedGraph(ei2, et, n, r)
    assert all(torch.equal(x, y) for x, y in zip(g3.arrays(False), want.arrays(False)))
    ops.clear_graph_cache()
    g4 = ops.bucket(ei2, et, n, r, sidecar=path)               # the rewritten file now matches
    assert all(torch.equal(x, y) for x, y in zip(g4.arrays(True), want.arrays(True)))
    ops.clear_graph_cache()


def test_import_rejects_arrays_that_are_not_a_csr(tmp_path):
    dev = need_gpu()
    ei, et, n, r = synth.uniform_graph(40, 500, 2, seed=2)
    good = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r).state()
    for key, edit in (("col", lambda t: t.__setitem__(3, n)),              # source id out of range
                      ("rowptr", lambda t: t.__setitem__(5, t[4] - 1 if t[4] > 0 else 10**6)),   # not monotone
                      ("perm_t", lambda t: t.__setitem__(0, -1)),
                      ("rowptr_t", lambda t: t.__setitem__(-1, 499))):      # does not end at E
        bad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in good.items()}
        edit(bad[key])
        with pytest.raises(IndexError):
            ops.BucketedGraph.from_state(bad, dev)
    bad = dict(good, col=good["col"][:-1])
    with pytest.raises(ValueError):
        ops.BucketedGraph.from_state(bad, dev)                  # wrong length never reaches the device
    with pytest.raises(ValueError):
        ops.BucketedGraph.from_state(dict(good, format="x"), dev)
    ops.BucketedGraph.from_state(good, dev)

# ------------------------------------------------------------------ aggregate (A3 + A4)
@pytest.mark.parametrize("case", LAYER_CASES)
def test_aggregate_golden(case):
    dev = need_gpu()
    z = load_golden(f"layer_{case}.npz")
    n, r = z["num_nodes"], z["num_relations"]
    g = ops.BucketedGraph(z["edge_index"].to(dev), z["edge_type"].to(dev), n, r)
    agg = ops.aggregate(g, z["x"].to(dev))
    assert_fwd(agg.view(n, r, -1), z["agg"], 2e-6)


@pytest.mark.parametrize("d", [4, 8, 24, 64, 128, 256, 320])
def test_aggregate_feature_widths_and_transposed(d):
    dev = need_gpu()
    ei, et, n, r = synth.uniform_graph(300, 6000, 3, seed=d)
    ei[1, :900] = 7                                        # one heavy destination: 3 levels of chunks
    ei[0, 1000:1200] = 9                                   # and a heavy source
    gen = torch.Generator().manual_seed(d)
    x = torch.randn(n, d, generator=gen)
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    assert g.num_levels(False) >= 2
    agg = ops.aggregate(g, x.to(dev))
    assert_fwd(agg.view(n, r, d), O.mean_aggregate_ref(x, ei, et, r), 5e-6)
    # transposed: what autograd scatters for the mean aggregation
    xr = x.clone().requires_grad_(True)
    cot = torch.randn(n, r, d, generator=gen)
    (O.mean_aggregate_ref(xr, ei, et, r) * cot).sum().backward()
    # grad_x[j] = sum_r sum_{e: j->i,r} cot[i, r] / cnt[i, r]; feed cot[:, r] one relation at a time
    gagg = torch.zeros(n, d)
    for rel in range(r):
        t = ops.aggregate(g, cot[:, rel].contiguous().to(dev), transposed=True).view(n, r, d)
        gagg += t[:, rel].cpu()
    assert_grad(gagg, xr.grad, 2e-5)


def test_aggregate_is_deterministic_and_exact_on_ones():
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(seed=42)
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    deg = torch.bincount(ei[1] * r + et, minlength=n * r)
    ones = ops.aggregate(g, torch.ones(n, 64, device=dev)).view(n * r, 64).cpu()
    # mean of ones is exactly 1 on non-empty segments (sums of <= 2^24 ones are exact), else 0
    assert torch.equal(ones, (deg > 0).float().view(-1, 1).expand(-1, 64))
    x = torch.randn(n, 128, generator=torch.Generator().manual_seed(0)).to(dev)
    a, b = ops.aggregate(g, x), ops.aggregate(g, x)
    assert torch.equal(a, b)                               # fixed summation tree: bitwise reproducible
    # linearity (size independent property): agg(2x + y) = 2 agg(x) + agg(y)
    y = torch.randn(n, 128, generator=torch.Generator().manual_seed(1)).to(dev)
    lhs = ops.aggregate(g, 2 * x + y)
    torch.testing.assert_close(lhs, 2 * a + ops.aggregate(g, y), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------ transform (A6) and its grads
@pytest.mark.parametrize("precision", ["fp32", "split"])
@pytest.mark.parametrize("n,r,d_in,d_out", [(100, 3, 64, 128), (257, 1, 8, 4), (1000, 3, 64, 64),
                                            (513, 16, 32, 64), (300, 3, 128, 256), (129, 2, 20, 36)])
def test_transform_kernels(n, r, d_in, d_out, precision):
    """the three dense kernels by themselves against float64, in both arithmetics: the fp32 MFMA and the
    split-precision fp16 MFMA (shapes its tiling does not take run the fp32 kernels: never less precise)"""
    dev = need_gpu()
    gen = torch.Generator().manual_seed(n + d_in)
    agg = torch.randn(n, r * d_in, generator=gen)
    x = torch.randn(n, d_in, generator=gen)
    w = torch.randn(r, d_in, d_out, generator=gen) * 0.1
    root = torch.randn(d_in, d_out, generator=gen) * 0.1
    bias = torch.randn(d_out, generator=gen)
    g = torch.randn(n, d_out, generator=gen)
    kw = dict(precision=precision)
    want = (agg.double() @ w.double().view(r * d_in, d_out) + x.double() @ root.double() + bias.double())
    out = ops.transform_fwd(agg.to(dev), x.to(dev), w.to(dev), root.to(dev), bias.to(dev), **kw)
    assert rel_err(out, want) <= 2e-6
    out_nr = ops.transform_fwd(agg.to(dev), x.to(dev), w.to(dev), None, None, **kw)
    assert rel_err(out_nr, agg.double() @ w.double().view(r * d_in, d_out)) <= 2e-6
    # grad wrt input: gagg [n, r*d_out] plays agg's role
    gagg = torch.randn(n, r * d_out, generator=gen)
    want_gx = sum(gagg.double()[:, k * d_out:(k + 1) * d_out] @ w.double()[k].t() for k in range(r)) \
        + g.double() @ root.double().t()
    gx = ops.transform_bwd_input(gagg.to(dev), g.to(dev), w.to(dev), root.to(dev), **kw)
    assert rel_err(gx, want_gx) <= 2e-6
    # grads wrt parameters
    gw, groot, gbias = ops.transform_bwd_params(agg.to(dev), x.to(dev), g.to(dev), r, **kw)
    assert rel_err(gw, (agg.double().t() @ g.double()).view(r, d_in, d_out)) <= 5e-6
    assert rel_err(groot, x.double().t() @ g.double()) <= 5e-6
    assert rel_err(gbias, g.double().sum(0)) <= 5e-6
    gw2, groot2, gbias2 = ops.transform_bwd_params(agg.to(dev), x.to(dev), g.to(dev), r, want_root=False,
                                                   want_bias=False, **kw)
    # (without a root the operand widths can select the other slab kernel, whose row order differs)
    assert groot2 is None and gbias2 is None and rel_err(gw2, gw.cpu()) <= 1e-6


def test_one_pass_fp16_gradient_gemms_equal_their_rounded_operand_meaning():
    """precision="half" (configs[4]'s gradient GEMMs): each operand rounded to fp16 under its tensor's
    power-of-two scale, exact products, fp32 sums - against that meaning in float64, gradient-sized inputs"""
    dev = need_gpu()
    n, r, d_in, d_out = 1500, 3, 64, 128
    gen = torch.Generator().manual_seed(21)
    agg, x = torch.randn(n, r * d_in, generator=gen) * 0.01, torch.randn(n, d_in, generator=gen) * 0.01
    w, root = torch.randn(r, d_in, d_out, generator=gen) * 0.1, torch.randn(d_in, d_out, generator=gen) * 0.1
    g, gagg = torch.randn(n, d_out, generator=gen) * 1e-7, torch.randn(n, r * d_out, generator=gen) * 3e-7
    rs = lambda t: O._r16_scaled(t.double())                                        # noqa: E731
    A, X, W, Rt, G, GA = (t.to(dev) for t in (agg, x, w, root, g, gagg))
    wcat = rs(torch.cat([w.reshape(-1, d_out), root]))
    a_sc = rs(torch.cat([agg, x], 1))
    gw, groot, gbias = ops.transform_bwd_params(A, X, G, r, precision="half")
    want = a_sc.t() @ rs(g)
    assert rel_err(gw, want[: r * d_in].view(r, d_in, d_out)) <= 2e-6 and rel_err(groot, want[r * d_in:]) <= 2e-6
    assert rel_err(gbias, g.double().sum(0)) <= 2e-6                                # the column sums stay fp32
    wt = rs(torch.cat([w.transpose(1, 2).reshape(-1, d_in), root.t()]))
    want_gx = rs(gagg) @ wt[: r * d_out] + rs(g) @ wt[r * d_out:]
    gx = ops.transform_bwd_input(GA, G, W, Rt, precision="half")
    assert rel_err(gx, want_gx) <= 2e-6
    full = ops.transform_bwd_input(GA, G, W, Rt, precision="split")
    assert 1e-5 < rel_err(gx, full.cpu()) < 3e-3                                    # it IS fp16 operand arithmetic
    out = ops.transform_fwd(A, X, W, Rt, None, precision="half")
    assert rel_err(out, a_sc @ wcat) <= 2e-6


@pytest.mark.parametrize("a_scale,b_scale,g_scale", [(1e-6, 1.0, 1e-7), (3e4, 1e-3, 1e5), (1.0, 1e-9, 1e-12),
                                                     (1e-20, 1e10, 1e15)])
def test_split_precision_scales_with_the_operands(a_scale, b_scale, g_scale):
    """split precision = fp16 hi/lo pairs under ONE power-of-two scale per operand tensor: operands far
    outside fp16's range (gradients of a mean loss ~1e-7, un-normalised features ~1e4) must come through
    with the same RELATIVE accuracy, hub-sized outliers and exact zeros included; the scales arrive either
    from the producers (amax=) or from the call's own scan - same bits."""
    dev = need_gpu()
    n, r, d_in, d_out = 777, 3, 64, 128
    gen = torch.Generator().manual_seed(11)
    agg = torch.randn(n, r * d_in, generator=gen) * a_scale
    agg[5] *= 300.0                                   # one hub-sized row sets the scale; the rest sit 2^8 below it
    agg[:, d_in:2 * d_in] *= (torch.rand(n, 1, generator=gen) < 0.5)
    x = torch.randn(n, d_in, generator=gen) * a_scale
    w = torch.randn(r, d_in, d_out, generator=gen) * b_scale
    root = torch.randn(d_in, d_out, generator=gen) * b_scale
    g = torch.randn(n, d_out, generator=gen) * g_scale
    gagg = torch.randn(n, r * d_out, generator=gen) * g_scale
    A, X, W, Rt, G, GA = (t.to(dev) for t in (agg, x, w, root, g, gagg))
    want = agg.double() @ w.double().view(-1, d_out) + x.double() @ root.double()
    out = ops.transform_fwd(A, X, W, Rt, None, precision="split")
    assert rel_err(out, want) <= 2e-6
    a_amax, x_amax, g_amax, ga_amax = ops.absmax(A), ops.absmax(X), ops.absmax(G), ops.absmax(GA)
    assert ops.amax_value(a_amax).item() == agg.abs().max().item() and ops.amax_value(x_amax).item() == x.abs().max().item()
    o_amax = ops.amax_buffer(dev)[0]
    out2 = ops.transform_fwd(A, X, W, Rt, None, precision="split", amax=(a_amax, x_amax), amax_out=o_amax)
    assert torch.equal(out, out2) and ops.amax_value(o_amax).item() == out.abs().max().item()
    want_gx = sum(gagg.double()[:, k * d_out:(k + 1) * d_out] @ w.double()[k].t() for k in range(r)) \
        + g.double() @ root.double().t()
    gx = ops.transform_bwd_input(GA, G, W, Rt, precision="split", amax=(ga_amax, g_amax))
    assert rel_err(gx, want_gx) <= 2e-6
    assert torch.equal(gx, ops.transform_bwd_input(GA, G, W, Rt, precision="split"))
    gw, groot, gbias = ops.transform_bwd_params(A, X, G, r, precision="split", amax=(a_amax, x_amax, g_amax))
    assert rel_err(gw, (agg.double().t() @ g.double()).view(r, d_in, d_out)) <= 5e-6
    assert rel_err(groot, x.double().t() @ g.double()) <= 5e-6
    assert rel_err(gbias, g.double().sum(0)) <= 5e-6
    gw_b = ops.transform_bwd_params(A, X, G, r, precision="split")[0]
    assert torch.equal(gw, gw_b)
    # weights split once (ops.split_weights) = the per-call split, bit for bit; absmax clears buffers on the side
    pk = ops.split_weights(W, Rt)
    assert torch.equal(out, ops.transform_fwd(A, X, W, Rt, None, precision="split", packed=pk))
    assert torch.equal(gx, ops.transform_bwd_input(GA, G, W, Rt, precision="split", packed=pk))
    with pytest.raises(ValueError):
        ops.transform_fwd(A, X, W, None, None, precision="split", packed=pk)
    # ... and the one-launch forms: maxima of several tensors at once, several layers split at once
    bufs = torch.full((5, ops.AMAX_FLOATS), 3.0, device=dev)
    ops.absmax_many([X, W, Rt], [bufs[0], bufs[1], bufs[2]], clear=bufs[3:])
    assert [ops.amax_value(bufs[i]).item() for i in range(3)] == [t.abs().max().item() for t in (x, w, root)]
    assert ops.amax_value(bufs[3:]).item() == 0.0
    W2 = (torch.randn(r, d_out, 64, generator=gen) * 3.0).to(dev)
    many = ops.split_weights_many([(W, Rt), (W2, None)], amax=[(bufs[1], bufs[2]), (ops.absmax(W2), None)])
    assert torch.equal(out, ops.transform_fwd(A, X, W, Rt, None, precision="split", packed=many[0]))
    lone = ops.split_weights(W2, None)
    agg2 = torch.randn(n, r * d_out, generator=gen).to(dev)
    x2 = torch.randn(n, d_out, generator=gen).to(dev)
    assert torch.equal(ops.transform_fwd(agg2, x2, W2, None, None, precision="split", packed=many[1]),
                       ops.transform_fwd(agg2, x2, W2, None, None, precision="split", packed=lone))
    junk = torch.full((3, ops.AMAX_FLOATS), 7.0, device=dev)
    ops.absmax(X, junk[0], clear=junk[1:])
    assert ops.amax_value(junk[0]).item() == x.abs().max().item() and ops.amax_value(junk[1:]).item() == 0.0
    # all-zero operands: scale 1, exact zeros out
    z = ops.transform_fwd(torch.zeros_like(A), torch.zeros_like(X), W, Rt, None, precision="split")
    assert float(z.abs().max()) == 0.0


def test_gather_leaves_the_exact_maximum():
    """aggregate(amax_out=): max |agg| (hub tails reduced in the upper levels included), both directions"""
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=200000, seed=4)
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    x = torch.randn(n, 64, generator=torch.Generator().manual_seed(1)).to(dev) * 3e-4
    for transposed in (False, True):
        slot = ops.amax_buffer(dev)[0]
        agg = ops.aggregate(g, x, transposed, amax_out=slot)
        assert torch.equal(agg, ops.aggregate(g, x, transposed))
        assert ops.amax_value(slot).item() == agg.abs().max().item() > 0
    with pytest.raises(ValueError):
        ops.aggregate(g, x.half(), amax_out=ops.amax_buffer(dev)[0])
    # the bound the encoder uses instead (no pass over the aggregate, no atomics in the gather):
    # |agg| <= weight_bound * max |x|, weight_bound = largest per-segment sum of edge weights (1 for the mean)
    assert g.weight_bound(False) == 1.0
    rowptr_t, _, _, w_t = (t.cpu() for t in g.arrays(True))
    seg = torch.repeat_interleave(torch.arange(n * r), (rowptr_t[1:] - rowptr_t[:-1]).long())
    sums = torch.zeros(n * r, dtype=torch.float64).index_add_(0, seg, w_t.double())
    assert sums.max().item() <= g.weight_bound(True) <= sums.max().item() * (1 + 1e-5) + 1e-30
    gagg = ops.aggregate(g, x, True)
    assert gagg.abs().max().item() <= g.weight_bound(True) * x.abs().max().item()
    assert ops.aggregate(g, x, False).abs().max().item() <= x.abs().max().item() * (1 + 1e-6)


# ------------------------------------------------------------------ the layer against the goldens
@pytest.mark.parametrize("case", LAYER_CASES)
def test_layer_forward_backward_golden(case):
    dev = need_gpu()
    z = load_golden(f"layer_{case}.npz")
    r = z["num_relations"]
    nb = z["weight"].size(0) if "comp" in z else None
    conv = RGCNConv(z["x"].size(1), z["weight"].size(2), r, num_bases=nb).to(dev)
    with torch.no_grad():
        conv.weight.copy_(z["weight"]); conv.root.copy_(z["root"]); conv.bias.copy_(z["bias"])
        if nb is not None:
            conv.comp.copy_(z["comp"])
    x = z["x"].to(dev).requires_grad_(True)
    out = conv(x, z["edge_index"].to(dev), z["edge_type"].to(dev))
    assert out.dtype == torch.float32 and out.shape == z["out"].shape
    assert_fwd(out, z["out_dense_f64"])                    # vs the independent float64 formulation
    assert_fwd(out, z["out"])                              # vs PyG's op sequence restated
    (out * z["cot"].to(dev)).sum().backward()
    assert_grad(x.grad, z["grad_x"])
    assert_grad(conv.weight.grad, z["grad_weight"])
    assert_grad(conv.root.grad, z["grad_root"])
    assert_grad(conv.bias.grad, z["grad_bias"])
    if nb is not None:
        assert_grad(conv.comp.grad, z["grad_comp"])


def test_layer_no_root_no_bias_and_frozen_input():
    dev = need_gpu()
    ei, et, n, r = synth.uniform_graph(200, 3000, 4, seed=9)
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(n, 32, generator=gen)
    conv = RGCNConv(32, 16, r, root_weight=False, bias=False).to(dev)
    out = conv(x.to(dev), ei.to(dev), et.to(dev))           # x does not require grad
    want = O.rgcn_conv_ref(x, ei, et, conv.weight.detach().cpu(), None, None)
    assert_fwd(out, want)
    out.sum().backward()
    wr = conv.weight.detach().cpu().clone().requires_grad_(True)
    O.rgcn_conv_ref(x, ei, et, wr, None, None).sum().backward()
    assert_grad(conv.weight.grad, wr.grad)


def test_fused_relu_layer_output_is_freed_without_the_cycle_collector():
    """``activation='relu'`` keeps the layer's output for the ReLU backward through ``save_for_backward``: no reference
    cycle out -> grad_fn -> ctx -> out, so the output (and its aggregate) is freed as soon as nothing refers to it"""
    import gc
    import weakref
    dev = need_gpu()
    ei, et, n, r = synth.uniform_graph(200, 3000, 4, seed=9)
    x = torch.randn(n, 32, device=dev, requires_grad=True)
    w = torch.randn(r, 32, 16, device=dev) * 0.1
    gc.disable()
    try:
        out = rgcn_conv(x, ei.to(dev), et.to(dev), w, None, None, r, activation="relu")
        ref = weakref.ref(out)
        del out
        assert ref() is None
    finally:
        gc.enable()


# ------------------------------------------------------------------ model + head vs reference-run vectors
def _load_ref_model(z, dev, **kw):
    sd = {k[4:].replace("__", "."): v for k, v in z.items() if k.startswith("sd__")}
    n = sd["encoder.node_embeddings.weight"].size(0)
    hidden = sd["decoder.relation_embeddings.weight"].size(1)
    m = DrugDiseaseModel(n, 3, 64, hidden, **kw)
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def test_model_eval_matches_reference_run():
    dev = need_gpu()
    z = load_golden("ref_model_eval.npz")
    m = _load_ref_model(z, dev)
    ei, et = z["edge_index"].to(dev), z["edge_type"].to(dev)
    hi, ti, ri = z["head"].to(dev), z["tail"].to(dev), z["rel"].to(dev)
    assert_fwd(m.get_embeddings(ei, et), z["embeddings"])
    assert_fwd(m.predict(ei, et, hi, ti, ri), z["scores"])
    assert_fwd(m.predict_all_tails(ei, et, hi, ri), z["all_scores"], 2e-5)
    m.eval()
    with torch.no_grad():                                   # unfused decoder entry: same numbers
        emb = m.encoder(ei, et)
        assert_fwd(m.decoder(emb[hi], emb[ti], ri), z["scores"])


def test_model_bases_matches_reference_run():
    dev = need_gpu()
    z = load_golden("ref_model_bases.npz")
    m = _load_ref_model(z, dev, num_bases=4)
    assert_fwd(m.get_embeddings(z["edge_index"].to(dev), z["edge_type"].to(dev)), z["embeddings"])


def test_training_step_matches_reference_run():
    """scores, BCE loss and every parameter gradient of one step of the reference's model
    (train.py:291-306 arithmetic, dropout p = 0)."""
    dev = need_gpu()
    z, t = load_golden("ref_model_eval.npz"), load_golden("ref_model_train_step.npz")
    m = _load_ref_model(z, dev, dropout=0.0, decoder_dropout=0.0).train()
    scores = m(z["edge_index"].to(dev), z["edge_type"].to(dev), z["head"].to(dev), z["tail"].to(dev),
               z["rel"].to(dev))
    assert_fwd(scores, t["scores"])
    loss = torch.nn.BCEWithLogitsLoss()(scores, t["labels"].to(dev))
    assert abs(loss.item() - t["loss"].item()) <= 1e-6
    loss.backward()
    for name, p in m.named_parameters():
        assert_grad(p.grad, t["grad__" + name.replace(".", "__")])


def test_fused_bce_head_matches_reference_run_and_torch():
    """model.bce_loss (loss fused into the head kernels) vs the reference-run training step
    (loss and every parameter gradient), and vs torch's BCEWithLogitsLoss on large logits."""
    dev = need_gpu()
    z, t = load_golden("ref_model_eval.npz"), load_golden("ref_model_train_step.npz")
    m = _load_ref_model(z, dev, dropout=0.0, decoder_dropout=0.0).train()
    loss, scores = m.bce_loss(z["edge_index"].to(dev), z["edge_type"].to(dev), z["head"].to(dev),
                              z["tail"].to(dev), z["rel"].to(dev), t["labels"].to(dev))
    assert_fwd(scores, t["scores"])
    assert abs(loss.item() - t["loss"].item()) <= 1e-6
    (loss * 0.5).backward()                                 # a non-unit upstream gradient must flow through
    for name, p in m.named_parameters():
        assert_grad(p.grad * 2, t["grad__" + name.replace(".", "__")])
    # saturated logits, duplicate rows, relation-dropout rows ([B, d] operand) vs torch ops
    gen = torch.Generator().manual_seed(6)
    emb = (torch.randn(40, 64, generator=gen) * 3).to(dev)
    hi, ti = torch.randint(0, 40, (1000,), generator=gen).to(dev), torch.randint(0, 6, (1000,), generator=gen).to(dev)
    ri = torch.randint(0, 3, (1000,), generator=gen).to(dev)
    y = (torch.rand(1000, generator=gen) < 0.5).float().to(dev)
    for p_drop in (0.0, 0.3):
        dec = LinkPredictor(3, 64, dropout=p_drop).to(dev).train()
        e1, e2 = emb.clone().requires_grad_(True), emb.clone().requires_grad_(True)
        torch.manual_seed(9)
        loss1, sc1 = dec.bce_loss(e1, hi, ti, ri, y)
        g1 = torch.autograd.grad(loss1, [e1, dec.relation_embeddings.weight])
        torch.manual_seed(9)
        sc2 = dec.score_triples(e2, hi, ti, ri)
        loss2 = torch.nn.BCEWithLogitsLoss()(sc2, y)
        g2 = torch.autograd.grad(loss2, [e2, dec.relation_embeddings.weight])
        assert sc1.abs().max() > 30                          # the stable form is exercised
        assert torch.equal(sc1, sc2) and abs(loss1.item() - loss2.item()) <= 1e-5 * max(1.0, abs(loss2.item()))
        for a, b in zip(g1, g2):
            assert_grad(a, b.cpu(), 1e-5)


@pytest.mark.parametrize("batch,entities,d", [(1, 1, 32), (7, 129, 64), (200, 30926, 128), (1030, 500, 128)])
def test_score_all_tails_kernel_vs_float64(batch, entities, d):
    """``LinkPredictor.score_all_tails`` (rgcn.py:215-243) as a kernel: every score against the float64 product, the
    gradients of all three operands against float64, ragged tiles in both directions, and the bits of the score the
    ranking kernel compares (rank = 1 + #{scores > true score} recomputed from the matrix)."""
    dev = need_gpu()
    g = torch.Generator().manual_seed(batch + entities)
    dec = LinkPredictor(5, d, dropout=0.0).to(dev)
    head = torch.randn(batch, d, generator=g).to(dev).requires_grad_(True)
    emb = torch.randn(entities, d, generator=g).to(dev).requires_grad_(True)
    rel = torch.randint(0, 5, (batch,), generator=g).to(dev)
    scores = dec.score_all_tails(head, rel, emb)
    table = dec.relation_embeddings.weight
    h64, e64, t64 = (x.detach().double().requires_grad_(True) for x in (head, emb, table))
    want = (h64 * t64[rel]) @ e64.t()
    bound = 4e-6 * float((h64.detach().abs() * t64.detach()[rel].abs()) .sum(1).max() * e64.detach().abs().max())
    assert float((scores.detach().double() - want.detach()).abs().max()) <= bound
    cot = torch.randn(batch, entities, generator=g).to(dev)
    (scores * cot).sum().backward()
    (want * cot.double()).sum().backward()
    for got, ref in ((head.grad, h64.grad), (emb.grad, e64.grad), (table.grad, t64.grad)):
        assert float((got.double() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    tails = torch.randint(0, entities, (batch,), generator=g).to(dev)
    with torch.no_grad():
        ranks = dec.rank_tails(head, rel, emb, tails)
        hr = head * table[rel]
        true = (hr * emb[tails]).sum(1, keepdim=True)
        beaten = scores > true
        beaten[torch.arange(batch, device=dev), tails] = False
        assert torch.equal(ranks, beaten.sum(1) + 1)


def test_score_all_tails_rejects_bad_relation_ids_loudly():
    dev = need_gpu()
    dec = LinkPredictor(3, 64, dropout=0.0).to(dev)
    head, emb = torch.randn(4, 64, device=dev), torch.randn(10, 64, device=dev)
    scores, _ = ops.distmult_score_all_tails(head, dec.relation_embeddings.weight.detach(),
                                             torch.tensor([0, 1, 7, 2], device=dev), emb)
    assert bool(torch.isnan(scores[2]).all()) and not bool(torch.isnan(scores[[0, 1, 3]]).any())



def test_link_predictor_matches_reference_run():
    dev = need_gpu()
    z = load_golden("ref_link_predictor.npz")
    dec = LinkPredictor(3, 128, dropout=0.0).to(dev)
    with torch.no_grad():
        dec.relation_embeddings.weight.copy_(z["rel_table"])
    h = z["head"].to(dev).requires_grad_(True)
    t = z["tail"].to(dev).requires_grad_(True)
    scores = dec(h, t, z["rel"].to(dev))
    assert_fwd(scores, z["scores"])
    assert_fwd(dec.score_all_tails(h, z["rel"].to(dev), z["all_tails"].to(dev)), z["all_scores"], 2e-5)
    (scores * z["cot"].to(dev)).sum().backward()
    assert_grad(h.grad, z["grad_head"])
    assert_grad(t.grad, z["grad_tail"])
    assert_grad(dec.relation_embeddings.weight.grad, z["grad_rel_table"])


def test_distmult_duplicate_rows_and_dropout_path():
    dev = need_gpu()
    gen = torch.Generator().manual_seed(5)
    emb = torch.randn(50, 128, generator=gen)
    rel = torch.randn(3, 128, generator=gen)
    hi = torch.randint(0, 5, (2048,), generator=gen)          # many duplicate rows
    ti = torch.randint(0, 50, (2048,), generator=gen)
    ri = torch.randint(0, 3, (2048,), generator=gen)
    cot = torch.randn(2048, generator=gen)
    e1, r1 = emb.clone().requires_grad_(True), rel.clone().requires_grad_(True)
    (O.distmult_ref(e1[hi], e1[ti], r1[ri]) * cot).sum().backward()
    e2, r2 = emb.to(dev).requires_grad_(True), rel.to(dev).requires_grad_(True)
    sc = distmult(e2, hi.to(dev), e2, ti.to(dev), r2, ri.to(dev))
    assert_fwd(sc, O.distmult_ref(emb[hi], emb[ti], rel[ri]), 2e-5)
    (sc * cot.to(dev)).sum().backward()
    assert_grad(e2.grad, e1.grad, 1e-5)
    assert_grad(r2.grad, r1.grad, 1e-5)
    # training with relation dropout: rows are dropped by torch, kernel reads [B, d] rows
    dec = LinkPredictor(3, 128, dropout=0.5).to(dev).train()
    torch.manual_seed(3)
    s_drop = dec.score_triples(e2.detach(), hi.to(dev), ti.to(dev), ri.to(dev))
    torch.manual_seed(3)
    rows = dec.dropout(dec.relation_embeddings(ri.to(dev)))
    want = (e2.detach()[hi.to(dev)] * rows * e2.detach()[ti.to(dev)]).sum(1)
    assert_fwd(s_drop, want.detach().cpu(), 2e-5)
    assert distmult(e2[:0], None, e2[:0], None, e2[:0], None).shape == (0,)


@pytest.mark.parametrize("shared", [True, False])
def test_distmult_backward_counts_every_occurrence_once(shared):
    """the head's backward adds a row's occurrences eight loads at a time, 64 keys per scan step: rows with exactly 1,
    15, 16, 17, 31, 32, 33, 48, 100 and 700 occurrences, integer-valued contributions (every order gives the same
    float) - the sums are exact, nothing is dropped or counted twice; head and tail slots of one table form one key
    space"""
    dev = need_gpu()
    counts = [1, 15, 16, 17, 31, 32, 33, 48, 100, 700]
    d = 128
    ids = torch.cat([torch.full((c,), i, dtype=torch.int64) for i, c in enumerate(counts)])
    gen = torch.Generator().manual_seed(3)
    ids = ids[torch.randperm(ids.numel(), generator=gen)]
    b = ids.numel()
    other = torch.randint(len(counts), len(counts) + 50, (b,), generator=gen)          # rows the heads never use
    rows = len(counts) + 50
    emb = torch.ones(rows, d, device=dev, requires_grad=True)
    tail_table = emb if shared else torch.ones(rows, d, device=dev, requires_grad=True)
    rel = torch.ones(1, d, device=dev, requires_grad=True)
    cot = torch.randint(-8, 9, (b,), generator=gen).float()
    sc = distmult(emb, ids.to(dev), tail_table, other.to(dev), rel, torch.zeros(b, dtype=torch.int64, device=dev))
    (sc * cot.to(dev)).sum().backward()
    want_h = torch.zeros(rows).index_add_(0, ids, cot)                                   # per row: the sum of its cotangents
    want_t = torch.zeros(rows).index_add_(0, other, cot)
    if shared:
        assert torch.equal(emb.grad.cpu(), (want_h + want_t).view(-1, 1).expand(-1, d))
    else:
        assert torch.equal(emb.grad.cpu(), want_h.view(-1, 1).expand(-1, d))
        assert torch.equal(tail_table.grad.cpu(), want_t.view(-1, 1).expand(-1, d))
    assert torch.equal(rel.grad.cpu(), cot.sum().view(1, 1).expand(1, d))


@pytest.mark.parametrize("r,b,d_in,d_out", [(3, 4, 64, 256), (1, 1, 4, 4), (16, 8, 32, 36), (5, 2, 64, 128), (33, 3, 8, 100)])
def test_basis_composition_kernels_vs_float64(r, b, d_in, d_out):
    """row A5 (PyG ``num_bases``): ``W = comp @ basis`` and its backward as kernels - values against float64, R * B
    beyond one flush batch of the partial dot products (16 x 8), widths that do not fill the last workgroup, and the
    same bits on a second run (fixed summation order, no atomics)"""
    dev = need_gpu()
    gen = torch.Generator().manual_seed(r * 100 + b)
    comp = torch.randn(r, b, generator=gen).to(dev).requires_grad_(True)
    basis = torch.randn(b, d_in, d_out, generator=gen).to(dev).requires_grad_(True)
    cot = torch.randn(r, d_in, d_out, generator=gen).to(dev)
    from primekg_rgcn_linkprediction_amd.conv import _BasisCompose
    w = _BasisCompose.apply(comp, basis)
    c64, b64 = comp.detach().double().requires_grad_(True), basis.detach().double().requires_grad_(True)
    w64 = (c64 @ b64.view(b, -1)).view(r, d_in, d_out)
    assert float((w.detach().double() - w64.detach()).abs().max()) <= 1e-6 * max(1.0, float(w64.detach().abs().max()))
    (w * cot).sum().backward()
    (w64 * cot.double()).sum().backward()
    for got, ref in ((comp.grad, c64.grad), (basis.grad, b64.grad)):
        assert float((got.double() - ref).abs().max()) <= 2e-6 * max(1.0, float(ref.abs().max()))
    again = ops.basis_compose_bwd(cot, comp.detach(), basis.detach())
    assert torch.equal(again[0], comp.grad) and torch.equal(again[1], basis.grad)
    only_basis = ops.basis_compose_bwd(cot, comp.detach(), basis.detach(), need_comp=False)
    assert only_basis[0] is None and torch.equal(only_basis[1], basis.grad)


@pytest.mark.parametrize("shared", [True, False])
def test_distmult_backward_clears_its_tables_itself(shared):
    """``zero_tables``: the first launch of the head's backward clears the indexed gradient tables (extra workgroups) -
    buffers full of NaN give the bits of caller-zeroed ones, for one shared table and for two, in both entry points"""
    dev = need_gpu()
    gen = torch.Generator().manual_seed(5)
    b, d, rows = 700, 128, 1000
    emb, emb2, rel = (torch.randn(n, d, generator=gen).to(dev) for n in (rows, 333, 3))
    tail_table = emb if shared else emb2
    hi = torch.randint(0, rows, (b,), generator=gen).to(dev)
    ti = torch.randint(0, tail_table.size(0), (b,), generator=gen).to(dev)
    ri = torch.randint(0, 3, (b,), generator=gen).to(dev)
    gs = torch.randn(b, generator=gen).to(dev)
    labels = (torch.rand(b, generator=gen) > 0.5).float().to(dev)
    scores = ops.distmult_fwd(emb, hi, tail_table, ti, rel, ri, b)
    one = torch.ones(1, device=dev)

    def run(zero_tables, fill):
        out = []
        for bce in (False, True):
            gh = torch.full_like(emb, fill)
            gt = gh if shared else torch.full_like(tail_table, fill)
            gr = torch.full_like(rel, fill)
            if bce:
                ops.distmult_bce_bwd(one, scores, labels, emb, hi, tail_table, ti, rel, ri, b, gh, gt, gr,
                                     zero_tables=zero_tables)
            else:
                ops.distmult_bwd(gs, emb, hi, tail_table, ti, rel, ri, b, gh, gt, gr, zero_tables=zero_tables)
            out += [gh, gt, gr]
        return out

    want = run(False, 0.0)
    got = run(True, float("nan"))
    for a, w in zip(got, want):
        assert torch.equal(a, w)
    assert float(want[0].abs().sum()) > 0 and int((want[0].abs().sum(1) == 0).sum()) > 0     # touched and untouched rows exist


def test_distmult_backward_is_deterministic_with_heavy_duplicates():
    """no float atomics in the head's backward: hub rows (one row the head of a third of the batch), head and tail
    from ONE table (one key space) or from two, relation table rows taking every sample - two runs give the
    same bits, and the sums equal the oracle's."""
    dev = need_gpu()
    gen = torch.Generator().manual_seed(9)
    b, d = 2048, 128
    emb, emb2 = torch.randn(300, d, generator=gen), torch.randn(40, d, generator=gen)
    rel = torch.randn(3, d, generator=gen)
    hi = torch.randint(0, 300, (b,), generator=gen)
    hi[torch.rand(b, generator=gen) < 0.33] = 7                     # a hub
    ti = torch.randint(0, 40, (b,), generator=gen)
    ri = torch.randint(0, 3, (b,), generator=gen)
    cot = torch.randn(b, generator=gen)
    for shared in (True, False):
        table_t = emb if shared else emb2
        tix = ti if not shared else torch.randint(0, 300, (b,), generator=gen)
        e1, t1, r1 = emb.clone().requires_grad_(True), table_t.clone().requires_grad_(True), rel.clone().requires_grad_(True)
        (O.distmult_ref(e1[hi], (e1 if shared else t1)[tix], r1[ri]) * cot).sum().backward()
        runs = []
        for _ in range(2):
            e2, r2 = emb.to(dev).requires_grad_(True), rel.to(dev).requires_grad_(True)
            t2 = e2 if shared else table_t.to(dev).requires_grad_(True)
            sc = distmult(e2, hi.to(dev), t2, tix.to(dev), r2, ri.to(dev))
            (sc * cot.to(dev)).sum().backward()
            runs.append((e2.grad.clone(), None if shared else t2.grad.clone(), r2.grad.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
        assert_grad(runs[0][0], e1.grad, 1e-5)
        assert_grad(runs[0][2], r1.grad, 1e-5)
        if not shared:
            assert torch.equal(runs[0][1], runs[1][1])
            assert_grad(runs[0][1], t1.grad, 1e-5)
    # the relation-table tree by itself, odd sizes
    rows, idx = torch.randn(1000, 36, generator=gen), torch.randint(0, 5, (1000,), generator=gen)
    got = ops.segment_sum(rows.to(dev), idx.to(dev), 7)
    want = torch.zeros(7, 36).index_add_(0, idx, rows)
    assert_grad(got, want, 1e-6)
    assert float(got[5:].abs().max()) == 0.0
    assert torch.equal(got, ops.segment_sum(rows.to(dev), idx.to(dev), 7))
    ops.check_indices(dev)                                            # nothing above was out of range


def test_out_of_range_head_ids_raise_at_the_next_check_and_never_fault():
    """torch indexing raises (device-side assert) on a bad index; here the kernels clamp it, keep running and
    raise a sticky flag that `ops.check_indices` turns into IndexError (no out-of-bounds access)."""
    dev = need_gpu()
    emb, rel = torch.randn(10, 8, device=dev, requires_grad=True), torch.randn(3, 8, device=dev)
    ok = torch.tensor([1, 2, 3], device=dev)
    ops.check_indices(dev)
    for bad in (torch.tensor([1, 10, 3], device=dev), torch.tensor([1, -1, 3], device=dev)):
        sc = distmult(emb, bad, emb, ok, rel, torch.tensor([0, 1, 2], device=dev))
        sc.sum().backward()
        torch.cuda.synchronize()
        with pytest.raises(IndexError):
            ops.check_indices(dev)
        ops.check_indices(dev)                                        # the flag was cleared
    sc = distmult(emb, ok, emb, ok, rel, torch.tensor([0, 3, 2], device=dev))   # relation id == R
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        ops.check_indices(dev)


# ------------------------------------------------------------------ BASELINE configs
PARITY_LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity_r04.json")


def _record(tag, **numbers):
    """observed errors of the full-size configs -> gpurun_out/parity_r04.json (copied to profiles/)"""
    try:
        os.makedirs(os.path.dirname(PARITY_LOG), exist_ok=True)
        log = json.load(open(PARITY_LOG)) if os.path.exists(PARITY_LOG) else {}
        log[tag] = {k: float(v.detach()) if isinstance(v, torch.Tensor) else float(v) for k, v in numbers.items()}
        json.dump(log, open(PARITY_LOG, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def _encoder_vs_oracle(dev, ei, et, n, r, dims, num_bases=None, seed=0, fwd_atol=FWD_ATOL, tag=None,
                       oracle32_atol=None):
    """The HIP encoder (three routes) against BOTH restatements on the same seeded inputs:
    the float64 evaluation of the oracle formula with the backward spelled out
    (``O.encoder_explicit_f64``, the device's own ReLU decisions) at the north-star gates
    - forward 1e-5, every gradient 1e-4 of its largest entry - and the fp32 loop path
    (``O.encoder_ref`` + autograd), whose own distance from float64 is measured beside it."""
    torch.manual_seed(seed)
    emb = torch.nn.init.xavier_uniform_(torch.empty(n, dims[0]))
    convs = [RGCNConv(dims[0], dims[1], r, num_bases=num_bases), RGCNConv(dims[1], dims[2], r, num_bases=num_bases)]
    for c in convs:
        c.bias.data.uniform_(-0.1, 0.1)
    cot = torch.randn(n, dims[2])
    ref_p = [{k: v.detach().clone().requires_grad_(True) for k, v in c.named_parameters()} for c in convs]
    # HIP
    convs = [c.to(dev) for c in convs]
    eid, etd = ei.to(dev), et.to(dev)
    with torch.no_grad():
        mask = (convs[0](emb.to(dev), eid, etd, activation="relu") > 0).cpu()
    # oracle #1: fp32 loop path + autograd (the device's ReLU decisions, like oracle #3 below)
    e_ref = emb.clone().requires_grad_(True)
    out_ref = O.encoder_ref(e_ref, ref_p[0], ref_p[1], ei, et, relu_mask=mask)
    (out_ref * cot).sum().backward()
    # oracle #3: float64, explicit backward, the device's ReLU decisions
    p64 = [{k: v.detach() for k, v in rp.items()} for rp in ref_p]
    f64 = O.encoder_explicit_f64(emb, p64[0], p64[1], ei, et, cot, relu_mask=mask)
    # the fp32 loop path adds a segment's messages one after the other: on segments of thousands of edges ITS distance
    # from float64 exceeds the gate (fuzz case 777/109: two nodes, 5,700-edge segments, 3.0e-5), so unless a config
    # pins the number (C2/C3: 1e-5) the gate against it is the float64 gate plus that measured distance
    gate32 = oracle32_atol or fwd_atol + float((out_ref.detach().double() - f64["out"]).abs().max())

    def grad_gate32(ref32, key):                 # the same for its gradients (fuzz case 9001/68: 1.5e-4 ... 7e-4 of their own)
        return GRAD_RTOL + (rel_err(ref32, f64["grads"][key]) if ref32.numel() and f64["grads"][key].abs().max() > 0 else 0.0)
    outs = []
    errs = {}
    # three routes to the same numbers: separate layers + torch relu, relu fused into conv1's
    # epilogue, and the fused two-layer autograd node (relu backward in conv2's grad epilogue)
    for route in ("layers", "fused_relu", "encoder2"):
        e_gpu = emb.to(dev).requires_grad_(True)
        for c in convs:
            c.zero_grad(set_to_none=True)
        if route == "layers":
            out = convs[1](torch.relu(convs[0](e_gpu, eid, etd)), eid, etd)
        elif route == "fused_relu":
            out = convs[1](convs[0](e_gpu, eid, etd, activation="relu"), eid, etd)
        else:
            out = rgcn_encoder2(e_gpu, eid, etd, convs[0], convs[1])
        (out * cot.to(dev)).sum().backward()
        assert_fwd(out, f64["out"], fwd_atol)
        assert_grad(e_gpu.grad, f64["grads"]["emb"])
        for name, c, rp in zip(("conv1", "conv2"), convs, ref_p):
            for k, v in c.named_parameters():
                assert_grad(v.grad, f64["grads"][f"{name}.{k}"])
                assert_grad(v.grad, rp[k].grad, grad_gate32(rp[k].grad, f"{name}.{k}"))
        assert_fwd(out, out_ref.detach(), gate32)
        assert_grad(e_gpu.grad, e_ref.grad, grad_gate32(e_ref.grad, "emb"))
        if route == "encoder2":
            errs = {"fwd_max_abs_vs_f64": (out.double().cpu() - f64["out"]).abs().max(),
                    "fwd_max_abs_vs_oracle32": (out.cpu() - out_ref.detach()).abs().max(),
                    "oracle32_fwd_max_abs_vs_f64": (out_ref.detach().double() - f64["out"]).abs().max(),
                    "grad_emb_rel_vs_f64": rel_err(e_gpu.grad, f64["grads"]["emb"]),
                    "oracle32_grad_emb_rel_vs_f64": rel_err(e_ref.grad, f64["grads"]["emb"]),
                    "grad_params_rel_vs_f64_max": max(rel_err(v.grad, f64["grads"][f"{name}.{k}"])
                                                      for name, c in zip(("conv1", "conv2"), convs)
                                                      for k, v in c.named_parameters()),
                    "out_abs_max": f64["out"].abs().max()}
        outs.append((out.detach(), e_gpu.grad.clone()))
    for o, g in outs[1:]:
        assert torch.equal(o, outs[0][0]) and torch.equal(g, outs[0][1])    # same kernels, same bits
    if tag:
        _record(tag, **errs)
    return errs


def test_two_nodes_with_segments_of_thousands_of_edges_stay_at_the_float64_gate():
    """Fuzz case 777/109 (tools/fuzz_encoder.py): 2 nodes, 17,001 edges, 3 relations of which one is empty - every
    segment is a hub of 2,800 ... 5,700 edges.  The device sums them as a tree and stays inside 1e-5 of float64; the fp32
    loop restatement, which adds edge by edge, is 3e-5 away from float64 itself (measured in the helper), so the gate
    against it widens by that distance and the float64 gate is the one that binds.  (Case 9001/68 is the same for the
    gradients: two 16,000-edge segments, basis weights - the loop restatement's own gradients are 1.5e-4 ... 7e-4 off.)"""
    dev = need_gpu()
    g = torch.Generator().manual_seed(109)
    ei = torch.randint(0, 2, (2, 17001), generator=g)
    et = torch.randint(0, 2, (17001,), generator=g)                      # relation 2 has no edges
    errs = _encoder_vs_oracle(dev, ei, et, 2, 3, (32, 32, 32), seed=109)
    assert errs["fwd_max_abs_vs_f64"] < 1e-5
    assert errs["oracle32_fwd_max_abs_vs_f64"] > errs["fwd_max_abs_vs_f64"]
    # the shape of case 9001/68: relation r's edges all end in node r (two 16,000-edge segments), basis-decomposed weights
    et = torch.randint(0, 2, (32144,), generator=g)
    ei = torch.stack([torch.randint(0, 2, (32144,), generator=g), et.clone()])
    errs = _encoder_vs_oracle(dev, ei, et, 2, 2, (64, 128, 128), num_bases=2, seed=68)
    assert errs["fwd_max_abs_vs_f64"] < 1e-5 and errs["grad_params_rel_vs_f64_max"] < 1e-4
    assert errs["oracle32_grad_emb_rel_vs_f64"] > errs["grad_emb_rel_vs_f64"]


def test_config_c1_two_layers_vs_oracle():
    """BASELINE configs[0]: 1k nodes / 10k edges / 3 relations, hidden 64, 2 layers."""
    dev = need_gpu()
    ei, et, n, r = synth.uniform_graph(1000, 10000, 3, seed=42)
    _encoder_vs_oracle(dev, ei, et, n, r, (64, 64, 64), tag="C1")


def test_config_c2_full_size_vs_oracle():
    """BASELINE configs[1]: PrimeKG shape 30,926 / 849,456 / 3, 64 -> 128 -> 128: forward within
    1e-5 of the float64 evaluation (the north-star bar).  The fp32 loop path sums a 30,730-edge
    hub sequentially; its own distance from float64 is recorded beside the device's."""
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(seed=42)
    _encoder_vs_oracle(dev, ei, et, n, r, (64, 128, 128), tag="C2", oracle32_atol=1e-5)   # the north star's number (observed 2.1e-6 ... 6.5e-6: profiles/r03_parity_errors.json)


def test_config_c2_true_train_graph_size():
    """the real train graph has 1,677,772 edge columns; same encoder, same gates."""
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=synth.PRIMEKG_TRAIN_EDGES, seed=7)
    _encoder_vs_oracle(dev, ei, et, n, r, (64, 128, 128), tag="C2_E1677772", oracle32_atol=1e-5)   # the north star's number (observed 2.1e-6 ... 6.5e-6: profiles/r03_parity_errors.json)


def test_config_c3_bases_on_real_subgraph():
    """BASELINE configs[2] layer form (hidden 256, num_bases 4) on the real PrimeKG test edges."""
    dev = need_gpu()
    z = load_golden("primekg_test_edges.npz")
    _encoder_vs_oracle(dev, z["edge_index"].long(), z["edge_type"].long(), 30926, 3, (64, 256, 256), num_bases=4)


def test_config_c3_full_size_vs_oracle():
    """BASELINE configs[2] at full size: 30,926 / 849,456 / 3, 64 -> 256 -> 256, num_bases = 4 - d = 256
    gathers over the 30k-edge hub and the transform-first input gradient of conv1 (conv.py `_input_grad`)."""
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(seed=42)
    _encoder_vs_oracle(dev, ei, et, n, r, (64, 256, 256), num_bases=4, tag="C3", oracle32_atol=1e-5)   # the north star's number (observed 2.1e-6 ... 6.5e-6: profiles/r03_parity_errors.json)


def test_encoder_training_mode_uses_torch_dropout_stream():
    """train() with dropout 0.5 (the reference default, train.py:680): conv1+relu fused, the
    mask drawn by torch's nn.Dropout exactly where rgcn.py:125 draws it."""
    dev = need_gpu()
    ei, et, n, r = synth.uniform_graph(300, 4000, 3, seed=2)
    torch.manual_seed(2)
    m = DrugDiseaseModel(n, r, 64, 128, dropout=0.5).to(dev).train()
    eid, etd = ei.to(dev), et.to(dev)
    torch.manual_seed(11)
    got = m.encoder(eid, etd)
    torch.manual_seed(11)
    enc = m.encoder
    h = torch.relu(enc.conv1(enc.node_embeddings.weight, eid, etd))
    want = enc.conv2(torch.nn.functional.dropout(h, 0.5, True), eid, etd)
    assert torch.equal(got, want)
    # backward of the fused node (ReLU + dropout backward inside conv2's input-grad epilogue)
    # vs autograd through the three separate ops, same cotangent
    cot = torch.randn_like(got)
    params = [enc.node_embeddings.weight] + list(enc.conv1.parameters()) + list(enc.conv2.parameters())
    g_fused = torch.autograd.grad(got, params, cot)
    g_plain = torch.autograd.grad(want, params, cot)
    for a, b in zip(g_fused, g_plain):
        assert_grad(a, b.cpu(), rtol=2e-6)
    m.eval()
    with torch.no_grad():
        e1 = m.encoder(eid, etd)
        e2 = enc.conv2(torch.relu(enc.conv1(enc.node_embeddings.weight, eid, etd)), eid, etd)
    assert torch.equal(e1, e2)


def test_no_grad_encoder_walks_row_blocks_and_equals_the_training_path(monkeypatch):
    """eval path (get_embeddings / validate / evaluate: src/train.py:389-395, src/evaluate.py:189-195): no [N, R*d]
    aggregate - destination rows in cache-sized blocks, one reused buffer - same bits as the training path's
    forward, for one block, a few blocks and ragged last blocks; hubs inside a block keep their partial-row levels"""
    from primekg_rgcn_linkprediction_amd import conv as C
    dev = need_gpu()
    monkeypatch.setattr(C, "_EVAL_FUSED", False)               # the two-launch path (fp16 tables, fp32 mode, other widths)
    ei, et, n, r = synth.primekg_like(num_edges=200000, seed=12)
    torch.manual_seed(3)
    emb = torch.nn.init.xavier_uniform_(torch.empty(n, 64)).to(dev)
    for gdt in (None, torch.float16):
        convs = [RGCNConv(64, 128, r, gather_dtype=gdt).to(dev), RGCNConv(128, 128, r, gather_dtype=gdt).to(dev)]
        for c in convs:
            c.bias.data.uniform_(-0.1, 0.1)
        eid, etd = ei.to(dev), et.to(dev)
        e_train = emb.clone().requires_grad_(True)
        want = rgcn_encoder2(e_train, eid, etd, convs[0], convs[1]).detach()       # the autograd node's forward
        graph = ops.bucket(eid, etd, n, r)
        for block_bytes in (1 << 40, 8 << 20, 3_000_000):
            monkeypatch.setattr(C, "_EVAL_BLOCK_BYTES", block_bytes)
            with torch.no_grad():
                got = rgcn_encoder2(emb, eid, etd, convs[0], convs[1])
            assert torch.equal(got, want), block_bytes
        blocks = graph.row_blocks(3_000_000 // (r * 128 * 4))
        assert len(blocks) > 3 and blocks[-1][1] == n and sum(b[2].num_edges for b in blocks) == ei.size(1)
        assert graph.row_blocks(3_000_000 // (r * 128 * 4)) is blocks               # cached
    # ops.aggregate(out=) / transform_fwd(out=) write where they are told
    buf = torch.full((n, r * 64), 7.0, device=dev)
    agg = ops.aggregate(graph, emb, out=buf)
    assert agg.data_ptr() == buf.data_ptr() and torch.equal(agg, ops.aggregate(graph, emb))


def test_functional_entry_and_r16():
    dev = need_gpu()
    ei, et, n, r = synth.uniform_graph(2000, 60000, 16, seed=4)     # C4's relation count, small N
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(n, 64, generator=gen)
    w = torch.randn(r, 64, 128, generator=gen) * 0.05
    root = torch.randn(64, 128, generator=gen) * 0.05
    bias = torch.randn(128, generator=gen)
    out = rgcn_conv(x.to(dev), ei.to(dev), et.to(dev), w.to(dev), root.to(dev), bias.to(dev), r)
    assert_fwd(out, O.rgcn_conv_ref(x, ei, et, w, root, bias))


def test_more_than_32_relations_and_odd_widths():
    """R = 40 (no relation-occupancy words: dense path), widths that are multiples of 4 but not of 32
    (register-staged GEMM fallbacks), forward and every gradient vs the oracle."""
    dev = need_gpu()
    ei, et, n, r = synth.uniform_graph(300, 9000, 40, seed=6)
    gen = torch.Generator().manual_seed(6)
    for d_in, d_out in ((32, 64), (20, 12)):
        x = torch.randn(n, d_in, generator=gen)
        w = torch.randn(r, d_in, d_out, generator=gen) * 0.1
        root = torch.randn(d_in, d_out, generator=gen) * 0.1
        bias = torch.randn(d_out, generator=gen)
        cot = torch.randn(n, d_out, generator=gen)
        ref_in = [t.clone().requires_grad_(True) for t in (x, w, root, bias)]
        O.rgcn_conv_ref(ref_in[0], ei, et, ref_in[1], ref_in[2], ref_in[3]).backward(cot)
        got_in = [t.to(dev).requires_grad_(True) for t in (x, w, root, bias)]
        out = rgcn_conv(got_in[0], ei.to(dev), et.to(dev), got_in[1], got_in[2], got_in[3], r)
        assert_fwd(out, O.rgcn_conv_ref(x, ei, et, w, root, bias))
        out.backward(cot.to(dev))
        for a, b in zip(got_in, ref_in):
            assert_grad(a.grad, b.grad)
    assert ops.bucket(ei.to(dev), et.to(dev), n, r).tile_mask_ptr(False) is None


def test_config_c4_scale_on_one_gpu():
    """BASELINE configs[3] shape (500k nodes / 20M edges / 16 relations, 64 -> 128) on ONE GPU:
    size-independent properties over the whole graph + the oracle on a sample of rows."""
    dev = need_gpu()
    n, e, r, d_in, d_out = 500_000, 20_000_000, 16, 64, 128
    ei, et, _, _ = synth.uniform_graph(n, e, r, seed=42)
    eid, etd = ei.to(dev), et.to(dev)
    g = ops.BucketedGraph(eid, etd, n, r)
    rowptr, col, perm, cnt = g.arrays(False)
    assert rowptr[-1].item() == e and rowptr[0].item() == 0
    assert bool((rowptr[1:] >= rowptr[:-1]).all())
    assert torch.equal(torch.sort(perm).values, torch.arange(e, device=dev))          # a permutation
    key = (eid[1] * r + etd)[perm]
    assert bool((key[1:] >= key[:-1]).all())                                           # bucketed
    same = key[1:] == key[:-1]
    assert bool((perm[1:][same] > perm[:-1][same]).all())                              # stable inside a segment
    assert torch.equal(col.long(), eid[0][perm])
    deg = torch.bincount(key, minlength=n * r)
    assert torch.equal(cnt, deg.clamp(min=1).float())
    del rowptr, col, key, same
    # exactness on ones, determinism
    ones = ops.aggregate(g, torch.ones(n, 8, device=dev)).view(n * r, 8)
    assert torch.equal(ones, (deg > 0).float().view(-1, 1).expand(-1, 8))
    del ones
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(n, d_in, generator=gen)
    xd = x.to(dev)
    agg = ops.aggregate(g, xd)
    assert torch.equal(agg, ops.aggregate(g, xd))
    w = torch.randn(r, d_in, d_out, generator=gen) * 0.05
    root = torch.randn(d_in, d_out, generator=gen) * 0.05
    bias = torch.randn(d_out, generator=gen)
    out = ops.transform_fwd(agg, xd, w.to(dev), root.to(dev), bias.to(dev))
    # oracle on 64 sampled destination rows (all their in-edges, original column order)
    rows = torch.randint(0, n, (64,), generator=gen)
    for i in rows.tolist()[:16]:
        m = ei[1] == i
        src, rel = ei[0][m], et[m]
        want = torch.zeros(d_out)
        for k in range(r):
            s = x[src[rel == k]]
            h = s.sum(0) / max(1, s.size(0)) if s.size(0) else torch.zeros(d_in)
            want = want + h @ w[k]
        want = want + x[i] @ root + bias
        assert (out[i].cpu() - want).abs().max().item() <= 1e-5
    # transposed structure: sum of weights into each destination segment is 1 (or 0 if empty)
    _, col_t, _, w_t = g.arrays(True)
    seg = col_t.long() * r + etd[g.arrays(True)[2]]
    tot = torch.zeros(n * r, device=dev, dtype=torch.float64).index_add_(0, seg, w_t.double())
    assert torch.allclose(tot, (deg > 0).double(), atol=1e-6)


def test_config_c4_default_policy_training_and_eval_at_full_size(monkeypatch):
    """BASELINE configs[3] at its full shape (500k nodes / 20M edge columns / 16 relations, 64 -> 128 -> 128) on ONE GPU,
    through ``rgcn_encoder2`` with the DEFAULT policy: at this size ``RGCN_TRAIN_FUSED=auto`` / ``RGCN_EVAL_FUSED=auto``
    pick the one-kernel layers by themselves (asserted from the launches recorded, nothing patched).  Forward AND
    backward: output, ``grad_emb`` and all six parameter gradients are bit-equal to the separate gather / transform
    kernels (``RGCN_TRAIN_FUSED=0``); 64 sampled output rows and 64 sampled ``grad_emb`` rows are within 1e-5 / 1e-4 of
    the float64 evaluation of their neighbourhoods (``O.encoder_rows_f64``); the no-grad encoder equals the training
    forward bit for bit, fused (auto) and blocked (``RGCN_EVAL_FUSED=0``)."""
    from primekg_rgcn_linkprediction_amd import conv as C
    dev = need_gpu()
    if C._TRAIN_FUSED != "auto" or C._EVAL_FUSED != "auto" or ops.GEMM_PRECISION != "split":
        pytest.skip("policy switches are overridden in this environment: the default policy is what this test is about")
    n, e, r, dims = 500_000, 20_000_000, 16, (64, 128, 128)
    assert n * r * dims[0] * 4 >= C._TRAIN_FUSED_MIN_BYTES
    ei, et, _, _ = synth.uniform_graph(n, e, r, seed=42)
    eid, etd = ei.to(dev), et.to(dev)
    torch.manual_seed(5)
    emb = torch.nn.init.xavier_uniform_(torch.empty(n, dims[0]))
    convs = [RGCNConv(dims[0], dims[1], r), RGCNConv(dims[1], dims[2], r)]
    for c in convs:
        c.bias.data.uniform_(-0.1, 0.1)
    cot = torch.randn(n, dims[2])
    ref_p = [{k: v.detach().clone() for k, v in c.named_parameters()} for c in convs]
    convs = [c.to(dev) for c in convs]
    cot_d = cot.to(dev)

    def run():
        e_gpu = emb.to(dev).requires_grad_(True)
        for c in convs:
            c.zero_grad(set_to_none=True)
        out = rgcn_encoder2(e_gpu, eid, etd, convs[0], convs[1])
        out.backward(cot_d)
        grads = [e_gpu.grad] + [p.grad for c in convs for p in c.parameters()]
        return out.detach(), [g.clone() for g in grads]

    ops.FUSED_EVENTS = []
    try:
        out, grads = run()
        kinds = sorted(ev[0] for ev in ops.FUSED_EVENTS)
    finally:
        ops.FUSED_EVENTS = None
    # both training forwards keep their aggregate (STORE), conv2's input gradient is the fused weighted kernel;
    # conv1's input gradient is transform-first (d_out = 2 d_in): a GEMM + the merged gather, by design
    assert kinds == ["bwd_input+mask", "fwd+store", "fwd+store"], kinds

    with torch.no_grad():
        ops.FUSED_EVENTS = []
        try:
            ev_out = rgcn_encoder2(emb.to(dev), eid, etd, convs[0], convs[1])
            ev_kinds = sorted(ev[0] for ev in ops.FUSED_EVENTS)
        finally:
            ops.FUSED_EVENTS = None
        assert ev_kinds == ["fwd", "fwd"], ev_kinds
        assert torch.equal(ev_out, out)
        monkeypatch.setattr(C, "_EVAL_FUSED", "0")
        assert torch.equal(rgcn_encoder2(emb.to(dev), eid, etd, convs[0], convs[1]), out)
        h_dev = convs[0](emb.to(dev), eid, etd, activation="relu")
    del ev_out

    monkeypatch.setattr(C, "_TRAIN_FUSED", "0")
    out0, grads0 = run()
    assert torch.equal(out, out0)
    names = ["emb"] + [f"conv{i + 1}.{k}" for i, c in enumerate(convs) for k, _ in c.named_parameters()]
    for name, a, b in zip(names, grads, grads0):
        assert torch.equal(a, b), name
    del out0, grads0

    gen = torch.Generator().manual_seed(9)
    out_rows = torch.randint(0, n, (64,), generator=gen)
    grad_rows = torch.randint(0, n, (64,), generator=gen)
    want = O.encoder_rows_f64(emb, ref_p[0], ref_p[1], ei, et, cot, out_rows, grad_rows,
                              lambda nodes: (h_dev[nodes.to(dev)] > 0).cpu())
    fwd_err = (out[out_rows.to(dev)].double().cpu() - want["out"]).abs().max().item()
    g_ref = want["grad_emb"]
    grad_err = ((grads[0][grad_rows.to(dev)].double().cpu() - g_ref).abs().max() / g_ref.abs().max()).item()
    nodes, h_ref = want["h_rows"]
    h_err = (h_dev[nodes.to(dev)].double().cpu() - h_ref).abs().max().item()
    _record("C4_1gpu_default_policy", fwd_max_abs_vs_f64_64_rows=fwd_err, grad_emb_rel_vs_f64_64_rows=grad_err,
            hidden_max_abs_vs_f64=h_err, hidden_rows_checked=nodes.numel(), out_abs_max=want["out"].abs().max())
    assert fwd_err <= FWD_ATOL and h_err <= FWD_ATOL, (fwd_err, h_err)
    assert grad_err <= GRAD_RTOL, grad_err


@pytest.mark.parametrize("d_in,d_out", [(64, 128), (128, 128), (128, 64)])
def test_relation_occupancy_masks_change_nothing(d_in, d_out):
    """Typed relations leave whole 32-row tiles without a relation; with the structure's
    occupancy mask the transforms skip those all-zero tiles.  Results must equal the dense
    kernels bit for bit, and the masks must be exactly the occupancy of the bucketed graph."""
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=120000, seed=3)
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    for transposed in (False, True):
        rowptr = g.arrays(transposed)[0].cpu().long()
        deg = (rowptr[1:] - rowptr[:-1]).view(n, r)
        occ = torch.nn.functional.pad(deg > 0, (0, 0, 0, (-n) % 32)).view(-1, 32, r).any(1)     # [tiles, r]
        assert g.tile_mask_ptr(transposed) is not None
        assert not bool(occ.all())                      # the typed graph does have empty (tile, relation) pairs
    gen = torch.Generator().manual_seed(d_in)
    x = torch.randn(n, d_in, generator=gen).to(dev)
    gr = torch.randn(n, d_out, generator=gen).to(dev)
    w = (torch.randn(r, d_in, d_out, generator=gen) * 0.1).to(dev)
    root = (torch.randn(d_in, d_out, generator=gen) * 0.1).to(dev)
    bias = torch.randn(d_out, generator=gen).to(dev)
    agg = ops.aggregate(g, x)
    gagg = ops.aggregate(g, gr, transposed=True)
    assert torch.equal(ops.transform_fwd(agg, x, w, root, bias, graph=g), ops.transform_fwd(agg, x, w, root, bias))
    assert torch.equal(ops.transform_fwd(agg, x, w, None, bias, relu=True, graph=g),
                       ops.transform_fwd(agg, x, w, None, bias, relu=True))
    assert torch.equal(ops.transform_bwd_input(gagg, gr, w, root, graph=g), ops.transform_bwd_input(gagg, gr, w, root))
    a = ops.transform_bwd_params(agg, x, gr, r, graph=g)
    b = ops.transform_bwd_params(agg, x, gr, r)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    a = ops.transform_bwd_params(agg, x, gr, r, want_root=False, graph=g)
    b = ops.transform_bwd_params(agg, x, gr, r, want_root=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    # a tile really is skipped somewhere: disease rows [0, 5593) have no relation 0 or 2
    assert float(agg[:5568].view(-1, r, d_in)[:, 0].abs().max()) == 0.0


# ------------------------------------------------------------------ BASELINE configs[4]: fp16 feature table
@pytest.mark.parametrize("d", [8, 64, 128, 256])
def test_fp16_gather_equals_fp32_gather_of_the_rounded_table(d):
    """half the bytes per row, same arithmetic: converting fp16 -> fp32 is exact and the
    summation order is unchanged, so the result equals the fp32 kernel on the rounded table."""
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=60000, seed=d)
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    x16 = torch.randn(n, d, generator=torch.Generator().manual_seed(d)).to(dev).half()
    for transposed in (False, True):
        assert torch.equal(ops.aggregate(g, x16, transposed), ops.aggregate(g, x16.float(), transposed))
    with pytest.raises(ValueError):
        ops.aggregate(g, torch.zeros(n, 12, device=dev, dtype=torch.float16))     # d % 8


@pytest.mark.parametrize("n,r,d_in,d_out,relu", [(30926, 3, 64, 128, True), (30926, 3, 128, 128, False),
                                                  (1000, 16, 32, 64, False), (77, 1, 96, 200, True)])
def test_fp16_matrix_core_transform(n, r, d_in, d_out, relu):
    """rgcn_transform_fwd_f16 (configs[4]) against its exact meaning - both operands rounded to fp16
    (nearest even), products and sums in fp32/fp64 - tightly, and against the fp32 transform within
    the 2e-3 gate; the packed-operand path with and without root / bias."""
    dev = need_gpu()
    gen = torch.Generator().manual_seed(n + d_in)
    agg = torch.randn(n, r * d_in, generator=gen)
    agg[:, : d_in] *= (torch.rand(n, 1, generator=gen) < 0.7)            # rows without relation 0
    x = torch.randn(n, d_in, generator=gen)
    w = torch.randn(r, d_in, d_out, generator=gen) * 0.1
    root = torch.randn(d_in, d_out, generator=gen) * 0.1
    bias = torch.randn(d_out, generator=gen)
    a16 = torch.cat([agg, x], 1).half().double()
    b16 = torch.cat([w.view(-1, d_out), root]).half().double()
    want = a16 @ b16 + bias.double()
    want = want.clamp(min=0) if relu else want
    got = ops.transform_fwd(agg.to(dev), x.to(dev), w.to(dev), root.to(dev), bias.to(dev), relu=relu, half=True)
    scale = want.abs().max().item()
    assert (got.double().cpu() - want).abs().max().item() <= 2e-6 * scale + 1e-5      # fp32 accumulation of exact products
    full = ops.transform_fwd(agg.to(dev), x.to(dev), w.to(dev), root.to(dev), bias.to(dev), relu=relu)
    assert rel_err(got, full.cpu()) <= 2e-3 and not torch.equal(got, full)
    # no root, no bias
    got2 = ops.transform_fwd(agg.to(dev), x.to(dev), w.to(dev), None, None, half=True)
    want2 = agg.half().double() @ w.view(-1, d_out).half().double()
    assert (got2.double().cpu() - want2).abs().max().item() <= 2e-6 * want2.abs().max().item() + 1e-5
    # a width the fp16 kernel does not take falls back to the fp32 GEMM (never less precise)
    if d_in == 32:
        x20, w20, agg20 = x[:, :20].contiguous(), w[:, :20].contiguous(), torch.randn(n, r * 20, generator=gen)
        fb = ops.transform_fwd(agg20.to(dev), x20.to(dev), w20.to(dev), None, None, half=True)
        assert torch.equal(fb, ops.transform_fwd(agg20.to(dev), x20.to(dev), w20.to(dev), None, None))


def test_fp16_matrix_core_transform_respects_relation_masks():
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=60000, seed=1)
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(n, 64, generator=gen).to(dev)
    w, root = (torch.randn(r, 64, 128, generator=gen) * 0.1).to(dev), (torch.randn(64, 128, generator=gen) * 0.1).to(dev)
    agg = ops.aggregate(g, x.half())
    assert torch.equal(ops.transform_fwd(agg, x, w, root, None, half=True, graph=g),
                       ops.transform_fwd(agg, x, w, root, None, half=True))       # skipped tiles were exact zeros


@pytest.mark.parametrize("half_backward", [True, False])
def test_config_c5_fp16_features_exact_meaning_and_fp32_oracle(half_backward):
    """configs[4]: PrimeKG shape, fp16 feature tables + fp16 matrix-core transforms, fp32 accumulate.
    Gate: the path's EXACT MEANING (``O.encoder_explicit_f64(half_forward=True, half_backward=...)``:
    fp16-rounded gather tables and GEMM operands in the forward; in the backward the fp32 formulas on the
    saved forward tensors - with ``half_backward`` (the default of an fp16 layer) the operands of the three
    gradient GEMMs per layer rounded to fp16 under their per-tensor power-of-two scales, one matrix-core
    pass, fp32 accumulate; the device's own ReLU decisions) - forward 1e-5, every gradient 1e-4.  Against the fp32 oracle the
    forward keeps SURVEY 8d's 2e-3 gate; the gradient distance to the fp32 oracle is REPORTED, not
    gated: rounding the features flips the ReLU of the pre-activations within fp16 precision of zero,
    which no fp16 feature path can avoid (observed 6e-3 .. 7e-3 relative L2)."""
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(seed=42)
    torch.manual_seed(5)
    emb = torch.nn.init.xavier_uniform_(torch.empty(n, 64))
    convs = [RGCNConv(64, 128, r, gather_dtype=torch.float16, half_backward=half_backward),
             RGCNConv(128, 128, r, gather_dtype=torch.float16, half_backward=half_backward)]
    assert RGCNConv(64, 128, r, gather_dtype=torch.float16).half_backward and not RGCNConv(64, 128, r).half_backward
    for c in convs:
        c.bias.data.uniform_(-0.1, 0.1)
    cot = torch.randn(n, 128) * 1e-6                    # gradient-sized: fp16 operands without scaling would underflow
    ref_p = [{k: v.detach().clone().requires_grad_(True) for k, v in c.named_parameters()} for c in convs]
    e_ref = emb.clone().requires_grad_(True)
    out_ref = O.encoder_ref(e_ref, ref_p[0], ref_p[1], ei, et)
    (out_ref * cot).sum().backward()
    convs = [c.to(dev) for c in convs]
    eid, etd = ei.to(dev), et.to(dev)
    e_gpu = emb.to(dev).requires_grad_(True)
    out = rgcn_encoder2(e_gpu, eid, etd, convs[0], convs[1])
    (out * cot.to(dev)).sum().backward()
    with torch.no_grad():
        mask = (convs[0](emb.to(dev), eid, etd, activation="relu") > 0).cpu()
    p64 = [{k: v.detach() for k, v in rp.items()} for rp in ref_p]
    exact = O.encoder_explicit_f64(emb, p64[0], p64[1], ei, et, cot, relu_mask=mask, half_forward=True,
                                   half_backward=half_backward)
    assert_fwd(out, exact["out"], 1e-5)
    assert_grad(e_gpu.grad, exact["grads"]["emb"])
    for name, c in zip(("conv1", "conv2"), convs):
        for k, v in c.named_parameters():
            assert_grad(v.grad, exact["grads"][f"{name}.{k}"])
    assert rel_err(out, out_ref.detach()) <= 2e-3

    def l2_rel(got, want):
        want = want.double()
        return ((got.double().cpu() - want).norm() / want.norm()).item()

    _record("C5_half_backward" if half_backward else "C5_fp32_backward", fwd_max_abs_vs_exact_meaning=(out.double().cpu() - exact["out"]).abs().max(),
            fwd_rel_vs_oracle32=rel_err(out, out_ref.detach()),
            grad_emb_rel_vs_exact_meaning=rel_err(e_gpu.grad, exact["grads"]["emb"]),
            grad_params_rel_vs_exact_meaning_max=max(rel_err(v.grad, exact["grads"][f"{name}.{k}"])
                                                     for name, c in zip(("conv1", "conv2"), convs)
                                                     for k, v in c.named_parameters()),
            grad_emb_l2_rel_vs_oracle32=l2_rel(e_gpu.grad, e_ref.grad),
            grad_params_l2_rel_vs_oracle32_max=max(l2_rel(v.grad, rp[k].grad) for c, rp in zip(convs, ref_p)
                                                   for k, v in c.named_parameters()))
    # and it is not the fp32 path in disguise
    convs32 = [RGCNConv(64, 128, r).to(dev), RGCNConv(128, 128, r).to(dev)]
    for a, b in zip(convs32, convs):
        a.load_state_dict(b.state_dict())
    out32 = rgcn_encoder2(emb.to(dev), eid, etd, convs32[0], convs32[1])
    assert not torch.equal(out32, out.detach())


# ------------------------------------------------------------------ C ABI called directly, device-side error paths
def test_c_abi_error_codes_with_real_handles():
    """what only shows with a live handle: short workspace, a direction a shard does not have,
    widths the kernels do not take, levels out of range - each a return code, never a fault."""
    import ctypes
    from primekg_rgcn_linkprediction_amd import _lib
    dev = need_gpu()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    ei = torch.zeros(2, 500, dtype=torch.int64)
    ei[0] = torch.arange(500) % 50                        # node 0 receives 500 edges of one relation: partial rows
    g = ops.BucketedGraph(ei.to(dev), torch.zeros(500, dtype=torch.int64, device=dev), 50, 2)
    d = 64
    need = lib.rgcn_aggregate_workspace_bytes(g.handle, 0, d)
    assert need == 2 * d * 4                              # 8 runs of 64 edges = 2 packs of 4 = 2 partial rows
    x = torch.randn(50, d, device=dev)
    agg = torch.empty(100, d, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    P = lambda t: t.data_ptr()                            # noqa: E731
    assert lib.rgcn_aggregate(g.handle, 0, P(x), d, P(agg), P(ws), need - 1, stream) == _lib.RGCN_ERR_WORKSPACE
    assert lib.rgcn_aggregate(g.handle, 0, P(x), d, P(agg), None, 0, stream) == _lib.RGCN_ERR_WORKSPACE
    assert lib.rgcn_aggregate(g.handle, 0, P(x), 6, P(agg), P(ws), need, stream) == _lib.RGCN_ERR_ARG
    assert lib.rgcn_aggregate(g.handle, 0, None, d, P(agg), P(ws), need, stream) == _lib.RGCN_ERR_ARG
    assert lib.rgcn_aggregate_ex(g.handle, 0, P(x), 1, 68, P(agg), P(ws), need * 2, 0, -1, None, None, stream) == _lib.RGCN_ERR_ARG   # d % 8
    assert lib.rgcn_aggregate_ex(g.handle, 0, P(x), 0, d, P(agg), P(ws), need, 7, 8, None, None, stream) == _lib.RGCN_ERR_ARG
    assert lib.rgcn_aggregate(g.handle, 0, P(x), d, P(agg), P(ws), need, stream) == _lib.RGCN_OK
    torch.cuda.synchronize()
    assert_fwd(agg.view(50, -1), O.mean_aggregate_ref(x.cpu(), ei, torch.zeros(500, dtype=torch.int64), 2).view(50, -1))
    # a shard handle has one direction
    sh = ops.BucketedGraph.from_shard(ei[1].to(dev), ei[0].to(dev), torch.zeros(500, dtype=torch.int64, device=dev),
                                      50, 50, 2)
    assert lib.rgcn_aggregate(sh.handle, 1, P(x), d, P(agg), P(ws), need, stream) == _lib.RGCN_ERR_ARG
    assert lib.rgcn_graph_export(sh.handle, 1, None, None, None, None, stream) == _lib.RGCN_ERR_ARG
    # parameter-gradient workspace
    nb = lib.rgcn_transform_bwd_params_workspace_bytes(50, 2, d, d)
    gw, gr_, gb = torch.empty(2, d, d, device=dev), torch.empty(d, d, device=dev), torch.empty(d, device=dev)
    gout = torch.randn(50, d, device=dev)
    assert lib.rgcn_transform_bwd_params(P(agg), P(x), P(gout), None, 50, 2, d, d, P(gw), P(gr_), P(gb), None, 0,
                                         stream) == _lib.RGCN_ERR_WORKSPACE
    wsp = torch.empty(nb, dtype=torch.uint8, device=dev)
    assert lib.rgcn_transform_bwd_params(P(agg), P(x), P(gout), None, 50, 2, d, d, P(gw), P(gr_), P(gb), P(wsp), nb,
                                         stream) == _lib.RGCN_OK
    torch.cuda.synchronize()
    assert_grad(gb, gout.sum(0).cpu())
    out = ctypes.c_void_p()
    bad = torch.tensor([[0, 7], [1, 0]], device=dev)
    assert lib.rgcn_graph_create(P(bad), P(torch.zeros(2, dtype=torch.int64, device=dev)), 2, 5, 1, stream,
                                 ctypes.byref(out)) == _lib.RGCN_ERR_RANGE
    assert out.value is None


def test_transform_first_input_gradient_equals_gather_first():
    """d_out >= 4 d_in: grad_x = aggregate(merged structure, g @ [W_r^T | root^T]) (rows d_in wide) vs the
    gather-first form (rows d_out wide) and vs autograd of the oracle; hubs, empty rows, duplicates."""
    from primekg_rgcn_linkprediction_amd.conv import _input_grad
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=80000, seed=11)
    graph = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    merged = graph.merged_transposed()
    assert merged is graph.merged_transposed() and merged.num_edges == ei.size(1) + n and merged.num_relations == 1
    gen = torch.Generator().manual_seed(3)
    for d_in, d_out in ((64, 256), (32, 256)):
        w = (torch.randn(r, d_in, d_out, generator=gen) * 0.1).to(dev)
        root = (torch.randn(d_in, d_out, generator=gen) * 0.1).to(dev)
        g = torch.randn(n, d_out, generator=gen).to(dev)
        first = _input_grad(graph, g, w, root)
        gather_first = ops.transform_bwd_input(ops.aggregate(graph, g, transposed=True), g, w, root, graph=graph)
        assert first.shape == (n, d_in) and rel_err(first, gather_first.cpu()) <= 2e-6
        x = torch.randn(n, d_in, generator=gen, requires_grad=True)
        O.rgcn_conv_ref(x, ei, et, w.cpu(), root.cpu(), None).backward(g.cpu())
        assert_grad(first, x.grad)
    # d_in >= d_out keeps the gather-first form (bit for bit)
    w = (torch.randn(r, 128, 64, generator=gen) * 0.1).to(dev)
    root = (torch.randn(128, 64, generator=gen) * 0.1).to(dev)
    g = torch.randn(n, 64, generator=gen).to(dev)
    assert torch.equal(_input_grad(graph, g, w, root),
                       ops.transform_bwd_input(ops.aggregate(graph, g, transposed=True), g, w, root, graph=graph))


def test_integration_md_ctypes_stub_runs_as_written():
    """The binding INTEGRATION.md section 2 shows a maintainer is executed verbatim and checked
    against the oracle - the document cannot drift from the ABI."""
    import os
    import re
    dev = need_gpu()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    block = re.search(r"## 2\..*?```python\n(.*?)```", text, re.S).group(1)
    cwd = os.getcwd()
    os.chdir(root)                                          # the stub opens the library by relative path
    try:
        scope = {}
        exec(compile(block, "INTEGRATION.md", "exec"), scope)
    finally:
        os.chdir(cwd)
    ei, et, n, r = synth.uniform_graph(500, 6000, 3, seed=12)
    gen = torch.Generator().manual_seed(12)
    x, w = torch.randn(n, 64, generator=gen), torch.randn(r, 64, 128, generator=gen) * 0.1
    rt, b = torch.randn(64, 128, generator=gen) * 0.1, torch.randn(128, generator=gen)
    out = scope["rgcn_forward"](x.to(dev), ei.to(dev), et.to(dev), w.to(dev), rt.to(dev), b.to(dev))
    torch.cuda.synchronize()
    assert_fwd(out, O.rgcn_conv_ref(x, ei, et, w, rt, b))


@pytest.mark.parametrize("d", [4, 8, 32, 64, 128, 256, 320])
def test_segment_lengths_around_run_and_pack_boundaries(d):
    """One destination per in-degree in {0, 1, 7, 8, 9, 63..65, 127..129, 191..193, 255..257, 300,
    511..513, 1023..1025, 2049, 16385+}: single items, packs of 2..4 runs, short last packs, multi-level
    reduction - forward (mean) and transposed (weighted) gathers vs the oracle, fp32 and fp16 tables."""
    dev = need_gpu()
    lengths = [0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 511, 512, 513,
               1023, 1024, 1025, 2049, 16385 + 3 * 256 + 70]
    n, r = 40, 2
    gen = torch.Generator().manual_seed(d)
    dst = torch.cat([torch.full((L,), i, dtype=torch.int64) for i, L in enumerate(lengths)])
    src = torch.randint(0, n, (dst.numel(),), generator=gen)
    rel = torch.zeros_like(dst)
    rel[dst % 2 == 1] = 1                                   # odd destinations use relation 1
    order = torch.randperm(dst.numel(), generator=gen)      # original column order is arbitrary
    ei, et = torch.stack([src, dst])[:, order].contiguous(), rel[order].contiguous()
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    x = torch.randn(n, d, generator=gen)
    tol = 3e-6                                              # relative to the largest entry, vs float64 sums

    def mean_ref(table):
        return O.mean_aggregate_ref(table.double(), ei, et, r).view(n, -1)

    assert rel_err(ops.aggregate(g, x.to(dev)), mean_ref(x)) <= tol
    if d % 8 == 0:
        assert rel_err(ops.aggregate(g, x.to(dev).half()), mean_ref(x.half())) <= tol

    def weighted_ref(edges):
        cnt = torch.bincount(edges[1] * r + et, minlength=n * r).clamp(min=1).float()
        w = (1.0 / cnt[edges[1] * r + et]).double()          # the fp32 weights the structure stores, summed in float64
        return torch.zeros(n * r, d, dtype=torch.float64).index_add_(
            0, edges[0] * r + et, x.double()[edges[1]] * w.view(-1, 1)).view(n, -1)

    # transposed: sources are random, so source segments are moderate, weights 1/cnt of every size
    assert rel_err(ops.aggregate(g, x.to(dev), transposed=True), weighted_ref(ei)) <= tol
    # the same lengths on the SOURCE side: long weighted segments (packs + reduction in weighted mode)
    ei2 = ei.flip(0).contiguous()
    g2 = ops.BucketedGraph(ei2.to(dev), et.to(dev), n, r)
    assert rel_err(ops.aggregate(g2, x.to(dev), transposed=True), weighted_ref(ei2)) <= tol
    assert g.num_levels(False) == 2 and g2.num_levels(True) == 2


def test_deferred_slab_reduction_rides_in_a_gather_and_changes_nothing():
    """transform_bwd_params(defer=True) + aggregate(tail=...) vs the two separate calls: gradients and
    the gathered rows bit for bit; widths where the gather cannot carry it (d > 256, fp16 table) and the
    stand-alone finish() too."""
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=60000, seed=13)
    graph = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(n, 64, generator=gen).to(dev)
    g = torch.randn(n, 128, generator=gen).to(dev)
    agg = ops.aggregate(graph, x)
    want = ops.transform_bwd_params(agg, x, g, r, graph=graph)
    for carrier in (g, torch.randn(n, 320, generator=gen).to(dev), g.half()):
        want_rows = ops.aggregate(graph, carrier, transposed=carrier.dtype == torch.float32)
        pend = ops.transform_bwd_params(agg, x, g, r, graph=graph, defer=True)
        assert not pend.done
        rows = ops.aggregate(graph, carrier, transposed=carrier.dtype == torch.float32, tail=pend)
        assert pend.done and torch.equal(rows, want_rows)
        for a, b in zip(pend.grads, want):
            assert torch.equal(a, b)
        pend.finish()                                          # idempotent
    pend = ops.transform_bwd_params(agg, x, g, r, want_root=False, want_bias=False, graph=graph, defer=True)
    pend.finish()
    assert pend.grads[1] is None and pend.grads[2] is None
    assert torch.equal(pend.grads[0], ops.transform_bwd_params(agg, x, g, r, want_root=False, want_bias=False,
                                                              graph=graph)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("n,e,r,d_in,d_out,limit", [
    (1000, 20000, 3, 64, 128, 16), (30926, 849456, 3, 128, 128, 16), (2049, 60000, 16, 64, 128, 8),
    (777, 30000, 5, 256, 256, 64), (500, 9000, 3, 128, 256, 1), (4097, 90000, 20, 64, 128, 16),
    (33, 40, 3, 64, 128, 16), (5000, 300000, 3, 256, 128, 24)])
def test_fused_layer_forward_is_bit_identical_to_gather_then_transform(n, e, r, d_in, d_out, limit):
    """rgcn_layer_fwd_fused (the aggregate formed in LDS as the transform's A operand; rgcn.py:123,128 under
    no_grad) against rgcn_aggregate -> rgcn_transform_fwd_split: same adds in the same order, same fragments
    through the same MFMA sequence - every bit equal, for hub-heavy graphs (long segments pre-aggregated), ragged
    last row blocks, relations missing from whole blocks (tile masks), R >= lanes per row, with / without bias,
    ReLU and root; and within 1e-5 of the float64 value."""
    dev = need_gpu()
    if (n, e) == (30926, 849456):
        ei, et, n, r = synth.primekg_like(seed=42)
    else:
        gen = torch.Generator().manual_seed(n + e)
        dst = (torch.rand(e, generator=gen) ** 3 * n).long().clamp_(max=n - 1)       # skewed: a few hubs
        src = torch.randint(0, n, (e,), generator=gen)
        et = torch.randint(0, r, (e,), generator=gen)
        et[dst < n // 3] = 0                                  # whole row blocks without most relations
        ei = torch.stack([src, dst])
    eid, etd = ei.to(dev), et.to(dev)
    graph = ops.bucket(eid, etd, n, r)
    assert ops.fused_supported(r, d_in, d_out)
    torch.manual_seed(e)
    x = torch.randn(n, d_in, device=dev)
    weight = torch.randn(r, d_in, d_out, device=dev) / d_in ** 0.5
    root = torch.randn(d_in, d_out, device=dev) / d_in ** 0.5
    bias = torch.randn(d_out, device=dev)
    plan = graph.fused_plan(limit)
    rowptr = graph.arrays(False)[0].long()
    lens = rowptr[1:] - rowptr[:-1]
    assert plan.hub_rows == int((lens > limit).sum()) and plan.hub_edges == int(lens[lens > limit].sum())
    for rt, bs, relu in ((root, bias, True), (root, None, False), (None, bias, False)):
        x_amax = ops.absmax(x)
        packed = ops.split_weights(weight, rt)
        agg = ops.aggregate(graph, x)
        want_amax, got_amax = ops.amax_buffer(dev), ops.amax_buffer(dev)
        want = ops.transform_fwd(agg, x, weight, rt, bs, relu=relu, graph=graph, amax=(x_amax, x_amax),
                                 amax_out=want_amax, packed=packed, precision="split")
        got = ops.layer_fwd_fused(graph, x, packed, bs, relu, x_amax, got_amax, inline_limit=limit)
        assert torch.equal(got, want), (rt is None, bs is None, relu)
        assert float(ops.amax_value(got_amax)) == float(ops.amax_value(want_amax)) == float(want.abs().max())
    ref = agg.double() @ weight.double().reshape(r * d_in, d_out) + bias.double()
    assert float((got.double() - ref).abs().max()) <= FWD_ATOL * max(1.0, float(ref.abs().max()))
    # STORE mode: the aggregate the kernel formed, written out as well (a training forward keeps it)
    kept = torch.full((n, r * d_in), float("nan"), device=dev)      # every row is written
    again = ops.layer_fwd_fused(graph, x, packed, bs, relu, x_amax, None, inline_limit=limit, agg_out=kept)
    assert torch.equal(again, got) and torch.equal(kept, agg)
    with pytest.raises(ValueError):
        graph.fused_plan(65)
    assert not ops.fused_supported(r, d_in, 64) and not ops.fused_supported(40, d_in, d_out)


@pytest.mark.gpu
def test_no_grad_encoder_through_the_fused_layer_equals_the_training_path(monkeypatch):
    """RGCN_EVAL_FUSED=1: get_embeddings / validate / evaluate run each layer as one kernel; same bits as the
    autograd node's forward"""
    from primekg_rgcn_linkprediction_amd import conv as C
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=200000, seed=12)
    torch.manual_seed(3)
    emb = torch.nn.init.xavier_uniform_(torch.empty(n, 64)).to(dev)
    convs = [RGCNConv(64, 128, r).to(dev), RGCNConv(128, 128, r).to(dev)]
    for c in convs:
        c.bias.data.uniform_(-0.1, 0.1)
    eid, etd = ei.to(dev), et.to(dev)
    want = rgcn_encoder2(emb.clone().requires_grad_(True), eid, etd, convs[0], convs[1]).detach()
    monkeypatch.setattr(C, "_EVAL_FUSED", True)
    events = []
    monkeypatch.setattr(ops, "FUSED_EVENTS", events)
    for limit in (16, 4, 64):
        monkeypatch.setattr(C, "_EVAL_INLINE_LIMIT", limit)
        with torch.no_grad():
            got = rgcn_encoder2(emb, eid, etd, convs[0], convs[1])
        assert torch.equal(got, want), limit
    assert len(events) == 6                                   # two fused launches per forward: the path was taken


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["half", "split", "fp32"])
@pytest.mark.parametrize("d_in,d_out", [(64, 128), (128, 128), (128, 64), (64, 64)])
def test_transforms_return_the_same_bits_every_run(d_in, d_out, precision):
    """Every transform entry, 100 launches each on the same operands (the caches and the allocator disturbed in
    between): bit-identical results.  Guards the hand-scheduled waits of the LDS-DMA GEMMs - the one-pass
    64-column kernel once read a fragment register above its s_waitcnt and differed in one run of five."""
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=300000, seed=9)
    graph = ops.bucket(ei.to(dev), et.to(dev), n, r)
    torch.manual_seed(d_in + d_out)
    g = torch.randn(n, d_out, device=dev) * 1e-6 * (torch.rand(n, d_out, device=dev) > 0.5)
    x = torch.randn(n, d_in, device=dev)
    w = torch.randn(r, d_in, d_out, device=dev) * 0.1
    root = torch.randn(d_in, d_out, device=dev) * 0.1
    bias = torch.randn(d_out, device=dev)
    g_amax, x_amax = ops.absmax(g), ops.absmax(x)
    pk = ops.split_weights(w, root) if precision != "fp32" else None
    agg, gagg = ops.aggregate(graph, x), ops.aggregate(graph, g, transposed=True)
    wb = graph.weight_bound(True)

    def run():
        fwd = ops.transform_fwd(agg, x, w, root, bias, relu=True, graph=graph, amax=(x_amax, x_amax), packed=pk,
                                precision="fp32" if precision == "fp32" else "split")
        gx = ops.transform_bwd_input(gagg, g, w, root, relu_mask=x, graph=graph, amax=(g_amax, g_amax), amax_mul=wb,
                                     packed=pk, precision=precision)
        gp = ops.transform_bwd_params(agg, x, g, r, graph=graph, amax=(x_amax, x_amax, g_amax), precision=precision)
        return (fwd, gx) + tuple(gp)

    want = run()
    for it in range(100):
        got = run()
        if it % 9 == 0:
            torch.randn(1 << 22, device=dev)                 # other traffic between the launches
        for name, a, b in zip(("fwd", "bwd_input", "grad_weight", "grad_root", "grad_bias"), got, want):
            assert torch.equal(a, b), (name, it)


@pytest.mark.gpu
def test_training_forward_through_the_fused_layer_changes_no_bit(monkeypatch):
    """RGCN_TRAIN_FUSED=1 (the default once the aggregate outgrows the Infinity Cache): the training forward runs
    each layer as the one-kernel layer in STORE mode - the aggregate it formed in LDS is written once, for the
    parameter gradients, and not read back - and each input gradient as the one-kernel transposed layer (weighted
    sums over out-edges formed in LDS).  Output and every gradient equal the two-launch path's bit for bit
    (two-layer node with dropout 0, and the single-layer node)."""
    from primekg_rgcn_linkprediction_amd import conv as C
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=250000, seed=21)
    eid, etd = ei.to(dev), et.to(dev)
    torch.manual_seed(8)
    emb = torch.nn.init.xavier_uniform_(torch.empty(n, 64)).to(dev)
    convs = [RGCNConv(64, 128, r).to(dev), RGCNConv(128, 128, r).to(dev)]
    for c in convs:
        c.bias.data.uniform_(-0.1, 0.1)
    cot = torch.randn(n, 128, device=dev)
    # conv1's input gradient (64 -> 128) goes transform-first by default (threshold 2: no fused kernel there); with
    # the threshold at 4 it is the fused kernel with a 64-wide output
    for ratio, launches in ((2.0, 4), (4.0, 5)):
        monkeypatch.setattr(C, "_TRANSFORM_FIRST_RATIO", ratio)
        results = {}
        for mode in ("0", "1"):
            monkeypatch.setattr(C, "_TRAIN_FUSED", mode)
            events = []
            monkeypatch.setattr(ops, "FUSED_EVENTS", events)
            e = emb.clone().requires_grad_(True)
            for c in convs:
                c.zero_grad()
            out = rgcn_encoder2(e, eid, etd, convs[0], convs[1])
            (out * cot).sum().backward()
            single = convs[0](e.detach(), eid, etd, activation="relu")
            assert len(events) == (launches if mode == "1" else 0)    # taken: 2 forward + 1 or 2 input-gradient layers, the single layer
            results[mode] = [out.detach(), e.grad.clone(), single.detach()] + [p.grad.clone() for c in convs for p in c.parameters()]
        for a, b in zip(results["0"], results["1"]):
            assert torch.equal(a, b), ratio


@pytest.mark.gpu
@pytest.mark.parametrize("n,e,r,d_in,d_out,limit,masked", [
    (1000, 20000, 3, 64, 128, 16, False), (30926, 849456, 3, 128, 128, 16, True), (2049, 60000, 16, 64, 64, 8, False),
    (777, 30000, 5, 256, 256, 64, True), (500, 9000, 3, 128, 64, 1, True), (4097, 90000, 20, 128, 128, 16, False),
    (33, 40, 3, 64, 128, 16, True), (5000, 300000, 3, 256, 128, 24, False)])
def test_fused_input_gradient_is_bit_identical_to_gather_then_transform(n, e, r, d_in, d_out, limit, masked):
    """rgcn_layer_bwd_input_fused (the 1/cnt-weighted sums over out-edges formed in LDS as the transform's A operand,
    scaled by the structure's weight bound, handed over to the gradient's own scale before the root chunk) against
    rgcn_aggregate(transposed) -> rgcn_transform_bwd_input_split: every bit equal - hub-heavy graphs (long segments
    pre-aggregated by a weighted structure), 64-wide outputs (two of the four waves multiply), ReLU mask, no root."""
    dev = need_gpu()
    if (n, e) == (30926, 849456):
        ei, et, n, r = synth.primekg_like(seed=42)
    else:
        gen = torch.Generator().manual_seed(n + e)
        src = (torch.rand(e, generator=gen) ** 3 * n).long().clamp_(max=n - 1)       # skewed: a few hub SOURCES
        dst = torch.randint(0, n, (e,), generator=gen)
        et = torch.randint(0, r, (e,), generator=gen)
        et[src < n // 3] = 0
        ei = torch.stack([src, dst])
    graph = ops.bucket(ei.to(dev), et.to(dev), n, r)
    assert ops.fused_bwd_supported(r, d_in, d_out)
    torch.manual_seed(e)
    g = torch.randn(n, d_out, device=dev) * 1e-3
    weight = torch.randn(r, d_in, d_out, device=dev) / d_in ** 0.5
    root = torch.randn(d_in, d_out, device=dev) / d_in ** 0.5
    mask = torch.randn(n, d_in, device=dev) if masked else None
    plan = graph.fused_plan(min(limit, d_out // 4), transposed=True)
    lens = graph.arrays(True)[0].long().diff()
    cut = min(limit, d_out // 4)
    assert plan.hub_rows == int((lens > cut).sum()) and plan.hub_edges == int(lens[lens > cut].sum())
    gagg = ops.aggregate(graph, g, transposed=True)
    for rt in (root, None):
        g_amax = ops.absmax(g)
        packed = ops.split_weights(weight, rt)
        want_amax, got_amax = ops.amax_buffer(dev), ops.amax_buffer(dev)
        want = ops.transform_bwd_input(gagg, g, weight, rt, relu_mask=mask, graph=graph, amax=(g_amax, g_amax),
                                       amax_mul=graph.weight_bound(True), amax_out=want_amax, packed=packed,
                                       precision="split")
        got = ops.layer_bwd_input_fused(graph, g, packed, mask, g_amax, got_amax, inline_limit=limit)
        assert torch.equal(got, want), rt is None
        assert float(ops.amax_value(got_amax)) == float(ops.amax_value(want_amax)) == float(want.abs().max())
    ref = gagg.double() @ weight.double().permute(0, 2, 1).reshape(r * d_out, d_in)
    if masked:
        ref = ref * (mask > 0)
    assert float((got.double() - ref).abs().max()) <= GRAD_RTOL * float(ref.abs().max())


@pytest.mark.gpu
def test_a_recorded_pass_is_not_replayed_on_inputs_of_another_type():
    """once a pass is issued natively, a call whose inputs differ from the recorded ones in dtype or device goes back
    through the wrappers, which refuse it by name - the recorded launch list would read the wrong bytes (a float16 table
    is half as long)"""
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=40000, seed=3)
    eid, etd = ei.to(dev), et.to(dev)
    torch.manual_seed(3)
    convs = [RGCNConv(64, 128, r).to(dev), RGCNConv(128, 128, r).to(dev)]
    x = torch.randn(n, 64, device=dev)
    with torch.no_grad():
        outs = [rgcn_encoder2(x, eid, etd, convs[0], convs[1]) for _ in range(5)]      # plain, sizes, record, replay, replay
    graph = ops.bucket(eid, etd, n, r)
    assert any(isinstance(s, ops._Plan) for s in graph.__dict__.get("_regions", {}).values())
    assert torch.equal(outs[-1], outs[0])
    with torch.no_grad():
        with pytest.raises(TypeError, match="float32"):
            rgcn_encoder2(x.double(), eid, etd, convs[0], convs[1])
        with pytest.raises(TypeError, match="float32"):
            rgcn_encoder2(x.half(), eid, etd, convs[0], convs[1])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            rgcn_encoder2(x.cpu(), eid, etd, convs[0], convs[1])
        assert torch.equal(rgcn_encoder2(x, eid, etd, convs[0], convs[1]), outs[0])     # and the plan still serves the right call


@pytest.mark.gpu
def test_a_recorded_pass_is_not_replayed_on_a_strided_input_and_its_outputs_are_tensors_of_their_own():
    """(a) a recorded launch list reads its inputs through data_ptr as DENSE rows - a same-shape transposed
    view must go back through the wrappers (the Region's own rule while recording), never into the native replay;
    (b) what a replayed pass hands its caller is a tensor of its own, not a view of the pass's arena: in-place ops work
    from the first step to the last, and holding the output does not hold aggregates / workspaces / split images"""
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=40000, seed=5)
    eid, etd = ei.to(dev), et.to(dev)
    graph = ops.bucket(eid, etd, n, r)
    torch.manual_seed(5)
    d = 64

    def gather_pass(x, *, graph):
        return (ops.aggregate(graph, x),)

    region = ops.Region("test.gather", gather_pass)
    x = torch.randn(n, d, device=dev)
    want = ops.aggregate(graph, x)
    for _ in range(4):                                                   # plain, sizes, record (+ acceptance), replay
        out = region.run(graph, ("k", d), (x,), dict(graph=graph), want={0})[0]
        assert torch.equal(out, want)
    plan = graph.__dict__["_regions"][("test.gather", ("k", d), ops.GEMM_PRECISION)]
    assert isinstance(plan, ops._Plan) and plan.external, "the pass was not recorded / its output is an arena view"
    assert out.untyped_storage().nbytes() == out.numel() * 4            # its own allocation, nothing else pinned
    out.add_(1.0)                                                        # in-place on a replayed output
    xt = torch.randn(d, n, device=dev).t()                               # [n, d], same shape and dtype, NOT dense
    assert xt.shape == x.shape and not xt.is_contiguous()
    assert not plan.matches([xt]) and plan.matches([x])
    with pytest.raises((ValueError, RuntimeError), match="contiguous"):
        region.run(graph, ("k", d), (xt,), dict(graph=graph), want={0})
    assert torch.equal(region.run(graph, ("k", d), (x,), dict(graph=graph), want={0})[0], want)
    # the encoder: outputs and gradients of replayed steps accept in-place updates like those of the first step
    convs = [RGCNConv(64, 128, r).to(dev), RGCNConv(128, 128, r).to(dev)]
    emb = torch.randn(n, 64, device=dev, requires_grad=True)
    for step in range(6):
        out = rgcn_encoder2(emb, eid, etd, convs[0], convs[1])
        out.mul_(2.0)
        out.sum().backward()
        for c in convs:
            c.weight.grad.mul_(0.5)
        emb.grad = None


@pytest.mark.gpu
def test_distmult_backward_of_an_empty_batch_returns_cleared_tables():
    """the indexed gradient tables are torch.empty and cleared by riders of the backward's first launch;
    an empty batch has no launch - its tables must still come back as zeros"""
    dev = need_gpu()
    from primekg_rgcn_linkprediction_amd import LinkPredictor
    torch.manual_seed(0)
    emb = torch.randn(50, 32, device=dev, requires_grad=True)
    dec = LinkPredictor(3, 32).to(dev)
    empty = torch.zeros(0, dtype=torch.int64, device=dev)
    poison = [torch.full((1 << 20,), float("nan"), device=dev) for _ in range(4)]     # what torch.empty may hand back next
    del poison
    scores = dec.score_triples(emb, empty, empty, empty)
    assert scores.shape == (0,)
    scores.sum().backward()
    assert torch.equal(emb.grad, torch.zeros_like(emb))
    assert torch.equal(dec.relation_embeddings.weight.grad, torch.zeros_like(dec.relation_embeddings.weight))


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.5, 0.1])
def test_dropout_factor_in_the_input_gradient_epilogue_equals_rescaled_weights(p):
    """``out_scale`` (the 1 / (1 - p) of the dropout between the layers, src/models/rgcn.py:125, whose backward
    rides in conv2's input-gradient epilogue) against what round 2 did - rescaling and re-splitting the weights:
    bitwise for p = 0.5 (a power of two commutes with every rounding), one rounding apart otherwise; the separate
    kernels with and without deferred hub tails, and the one-kernel input gradient."""
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=200000, seed=8)
    graph = ops.bucket(ei.to(dev), et.to(dev), n, r)
    torch.manual_seed(8)
    d_in = d_out = 128
    g = torch.randn(n, d_out, device=dev) * 1e-3
    weight = torch.randn(r, d_in, d_out, device=dev) / d_in ** 0.5
    root = torch.randn(d_in, d_out, device=dev) / d_in ** 0.5
    mask = torch.randn(n, d_in, device=dev)
    s = 1.0 / (1.0 - p)
    g_amax = ops.absmax(g)
    wb = graph.weight_bound(True)
    packed = ops.split_weights(weight, root)
    gagg = ops.aggregate(graph, g, transposed=True)
    old = ops.transform_bwd_input(gagg, g, weight * s, root * s, relu_mask=mask, graph=graph, amax=(g_amax, g_amax),
                                  amax_mul=wb, precision="split")                      # weights split inside the call
    am = ops.amax_buffer(dev)
    new = ops.transform_bwd_input(gagg, g, weight, root, relu_mask=mask, graph=graph, amax=(g_amax, g_amax),
                                  amax_mul=wb, packed=packed, precision="split", out_scale=s, amax_out=am)
    assert float(ops.amax_value(am)) == float(new.abs().max())                         # the maximum is taken after the factor
    gagg_d, hubs = ops.aggregate_deferred(graph, g, transposed=True)
    assert hubs is not None
    deferred = ops.transform_bwd_input(gagg_d, g, weight, root, relu_mask=mask, graph=graph, amax=(g_amax, g_amax),
                                       amax_mul=wb, packed=packed, precision="split", hubs=hubs, out_scale=s)
    fused = ops.layer_bwd_input_fused(graph, g, packed, mask, g_amax, out_scale=s)
    assert torch.equal(new, deferred) and torch.equal(new, fused)
    if p == 0.5:
        assert torch.equal(new, old)
    else:
        assert float((new - old).abs().max()) <= 2e-6 * float(old.abs().max())    # fp32 roundings of w * s, K = 512 terms
    fp32 = ops.transform_bwd_input(gagg, g, weight, root, relu_mask=mask, graph=graph, precision="fp32", out_scale=s)
    assert float((new - fp32).abs().max()) <= 1e-5 * float(fp32.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("p,frozen_input", [(0.0, False), (0.5, False), (0.0, True)])
def test_native_step_replays_the_recorded_pass_bit_for_bit(p, frozen_input, monkeypatch):
    """``ops.Region``: after three steps on a graph the encoder's forward and backward are issued by ONE native call each
    (``rgcn_sequence_run`` over the recorded launch list, tensors placed in one arena).  Every step - through the
    wrappers, while recording, replayed - gives the bits of the wrappers-only run (ops.REGIONS = False), with fresh
    inputs every step (a replay must follow the step's own tensors, not the recorded addresses), with dropout (two
    forward passes around torch's dropout kernel), with an input that needs no gradient, and inside a captured HIP graph."""
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=120000, seed=13)
    eid, etd = ei.to(dev), et.to(dev)
    torch.manual_seed(13)
    convs = [RGCNConv(64, 128, r).to(dev), RGCNConv(128, 128, r).to(dev)]
    for c in convs:
        c.bias.data.uniform_(-0.1, 0.1)
    steps = 6
    gen = torch.Generator().manual_seed(1)
    xs = [torch.randn(n, 64, generator=gen).to(dev) for _ in range(steps)]
    cots = [torch.randn(n, 128, generator=gen).to(dev) * (10.0 ** -k) for k in range(steps)]

    def run_all():
        results = []
        for k in range(steps):
            torch.manual_seed(100 + k)                                  # the dropout mask of step k
            x = xs[k].clone().requires_grad_(not frozen_input)
            for c in convs:
                c.zero_grad(set_to_none=True)
            out = rgcn_encoder2(x, eid, etd, convs[0], convs[1], dropout_p=p)
            out.backward(cots[k])
            results.append([out.detach().clone(), None if frozen_input else x.grad.clone()]
                           + [q.grad.clone() for c in convs for q in c.parameters()])
        return results

    graph = ops.bucket(eid, etd, n, r)
    graph.__dict__.pop("_regions", None)
    monkeypatch.setattr(ops, "REGIONS", False)
    want = run_all()
    assert not graph.__dict__.get("_regions")
    monkeypatch.setattr(ops, "REGIONS", True)
    got = run_all()
    plans = graph.__dict__["_regions"]
    names = sorted(k[0] for k, v in plans.items() if isinstance(v, ops._Plan))
    assert names == (["encoder2.backward", "encoder2.forward"] if p == 0 else
                     ["encoder2.backward", "encoder2.layer1", "encoder2.layer2"]), (names, {k[0]: type(v) for k, v in plans.items()})
    for k in range(steps):
        for a, b in zip(got[k], want[k]):
            assert (a is None and b is None) or torch.equal(a, b), k
    # a replayed pass inside a captured HIP graph
    if p == 0 and not frozen_input:
        x = xs[0].clone().requires_grad_(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        hip_graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(hip_graph, stream=side):
                out = rgcn_encoder2(x, eid, etd, convs[0], convs[1])
                gx, = torch.autograd.grad(out, [x], cots[0])
        torch.cuda.current_stream().wait_stream(side)
        hip_graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[0][0]) and torch.equal(gx, want[0][1])


@pytest.mark.gpu
@pytest.mark.parametrize("n,d_in1,d_out2,mask,root1,scale", [(30926, 64, 128, True, True, 1.0), (1000, 64, 128, True, True, 2.0),
                                                            (777, 32, 64, False, True, 1.0), (130, 64, 256, True, False, 1.0),
                                                            (63, 128, 128, True, True, 1.0)])
def test_chained_transform_first_equals_the_two_launches(n, d_in1, d_out2, mask, root1, scale):
    """``ops.transform_bwd_input_chain``: conv2's input gradient with conv1's transform-first product formed behind it by
    the same workgroup.  ``gz`` is the bits of ``transform_bwd_input``; ``T`` equals ``transform_first(gz)`` to rounding
    - the chained product splits its tile of gz under the TILE's maximum, the stand-alone one under the tensor's, which
    changes a bit only where a lo part is subnormal under the one scale and not the other - and is itself within 2e-6 of
    float64; ragged last row tile, no mask, no root, the dropout factor, the published maximum of gz."""
    dev = need_gpu()
    r, hidden = 3, 128
    gen = torch.Generator().manual_seed(n)
    w2, root2 = torch.randn(r, hidden, d_out2, generator=gen).to(dev) * 0.1, torch.randn(hidden, d_out2, generator=gen).to(dev) * 0.1
    w1 = torch.randn(r, d_in1, hidden, generator=gen).to(dev) * 0.1
    r1 = torch.randn(d_in1, hidden, generator=gen).to(dev) * 0.1 if root1 else None
    g = torch.randn(n, d_out2, generator=gen).to(dev) * 0.01
    gagg = torch.randn(n, r * d_out2, generator=gen).to(dev) * 0.01
    gagg[::7] *= 1e-4                                                          # a spread of magnitudes across row tiles
    h = torch.randn(n, hidden, generator=gen).to(dev) if mask else None
    g_amax = ops.absmax(g)
    pk2, pk1 = ops.split_weights_many([(w2, root2), (w1, r1)])
    assert ops.chain_supported(w2, w1)
    za, zb = ops.amax_buffer(dev, 2)
    want_gz = ops.transform_bwd_input(gagg, g, w2, root2, relu_mask=h, amax=(g_amax, g_amax), amax_mul=1.5, amax_out=za,
                                      packed=pk2, out_scale=scale)
    want_t = ops.transform_first(want_gz, pk1, za)
    gz, t = ops.transform_bwd_input_chain(gagg, g, w2, root2, h, pk2, pk1, amax=(g_amax, g_amax), amax_mul=1.5, amax_out=zb,
                                          out_scale=scale)
    assert torch.equal(gz, want_gz)
    assert torch.equal(ops.amax_value(zb), ops.amax_value(za)) and torch.equal(ops.amax_value(zb), gz.abs().max())
    assert t.shape == want_t.shape == (n, (r + int(root1)) * d_in1)
    tmax = float(want_t.abs().max())
    assert float((t - want_t).abs().max()) <= 1e-6 * tmax
    wcat = torch.cat([w1.reshape(r * d_in1, hidden)] + ([r1] if root1 else [])).double()
    t64 = gz.double() @ wcat.t()
    assert float((t.double() - t64).abs().max()) <= 2e-6 * float(t64.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("num_bases", [None, 4])
def test_explicit_encoder_step_equals_the_autograd_step_bit_for_bit(num_bases):
    """``rgcn_encoder2_step``: forward + backward for a given cotangent without the autograd engine (the two recorded
    passes issued directly) - output, input gradient and every parameter gradient (basis-decomposed weights included)
    are the bits of ``rgcn_encoder2(...).backward(cotangent)``, on every step (wrappers, recording, replayed), and
    gradients ACCUMULATE into ``.grad`` as the engine's would"""
    from primekg_rgcn_linkprediction_amd import rgcn_encoder2_step
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=90000, seed=31)
    eid, etd = ei.to(dev), et.to(dev)
    torch.manual_seed(31)
    convs = [RGCNConv(64, 128, r, num_bases=num_bases).to(dev), RGCNConv(128, 128, r, num_bases=num_bases).to(dev)]
    gen = torch.Generator().manual_seed(4)
    for k in range(5):
        x = torch.randn(n, 64, generator=gen).to(dev).requires_grad_(True)
        cot = torch.randn(n, 128, generator=gen).to(dev) * (10.0 ** -k)
        for c in convs:
            c.zero_grad(set_to_none=True)
        out = rgcn_encoder2(x, eid, etd, convs[0], convs[1])
        out.backward(cot)
        want = [out.detach().clone(), x.grad.clone()] + [q.grad.clone() for c in convs for q in c.parameters()]
        for c in convs:
            c.zero_grad(set_to_none=True)
        out2, gx2 = rgcn_encoder2_step(x.detach(), eid, etd, convs[0], convs[1], cot)
        got = [out2, gx2] + [q.grad.clone() for c in convs for q in c.parameters()]
        for a, b in zip(got, want):
            assert torch.equal(a, b), k
        rgcn_encoder2_step(x.detach(), eid, etd, convs[0], convs[1], cot, need_input_grad=False)      # a second step ADDS
        for q, b in zip([q for c in convs for q in c.parameters()], want[2:]):
            assert torch.equal(q.grad, b + b)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_the_literal_drop_in_call_pattern_runs_as_four_native_passes(p, monkeypatch):
    """What a reference user gets from INTEGRATION.md section 1's import swap ALONE: an encoder whose forward is the
    reference's own statement sequence (``/root/reference/src/models/rgcn.py:117-130``: the embedding table, ``conv1``,
    ``F.relu``, the ``nn.Dropout`` module, ``conv2``), i.e. ``RGCNConv.forward`` twice with torch ops between.  Each
    layer's forward and backward is an ``ops.Region``: from the fourth step on the step is four native calls (two
    layers x forward / backward), and every step - wrappers, recording, replayed - gives the bits of the wrappers-only
    run AND of the package's fused two-layer node under the same seed."""
    import torch.nn as nn
    import torch.nn.functional as F
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=120000, seed=29)
    eid, etd = ei.to(dev), et.to(dev)

    class ReferenceShapedEncoder(nn.Module):        # the reference's encoder, written against THIS package's RGCNConv
        def __init__(self):
            super().__init__()
            self.node_embeddings = nn.Embedding(n, 64)
            self.conv1 = RGCNConv(in_channels=64, out_channels=128, num_relations=r, num_bases=None)
            self.conv2 = RGCNConv(in_channels=128, out_channels=128, num_relations=r, num_bases=None)
            self.dropout = nn.Dropout(p)

        def forward(self, edge_index, edge_type):
            x = self.node_embeddings.weight
            x = self.conv1(x, edge_index, edge_type)
            x = F.relu(x)
            x = self.dropout(x)
            x = self.conv2(x, edge_index, edge_type)
            return x

    torch.manual_seed(29)
    enc = ReferenceShapedEncoder().to(dev)
    enc.train()
    for c in (enc.conv1, enc.conv2):
        c.bias.data.uniform_(-0.1, 0.1)
    steps = 6
    gen = torch.Generator().manual_seed(2)
    cots = [torch.randn(n, 128, generator=gen).to(dev) * (10.0 ** -k) for k in range(steps)]

    def run_all(fused_node=False):
        results = []
        for k in range(steps):
            torch.manual_seed(200 + k)                                  # the dropout mask of step k
            enc.zero_grad(set_to_none=True)
            if fused_node:
                out = rgcn_encoder2(enc.node_embeddings.weight, eid, etd, enc.conv1, enc.conv2, dropout_p=p)
            else:
                out = enc(eid, etd)
            out.backward(cots[k])
            results.append([out.detach().clone()] + [q.grad.clone() for q in enc.parameters()])
        return results

    graph = ops.bucket(eid, etd, n, r)
    graph.__dict__.pop("_regions", None)
    monkeypatch.setattr(ops, "REGIONS", False)
    want = run_all()
    fused = run_all(fused_node=True)
    assert not graph.__dict__.get("_regions")
    monkeypatch.setattr(ops, "REGIONS", True)
    got = run_all()
    plans = {k: v for k, v in graph.__dict__["_regions"].items() if isinstance(v, ops._Plan)}
    names = sorted(k[0] for k in plans)
    assert names == ["conv.backward", "conv.backward", "conv.forward", "conv.forward"], \
        (names, {k[0]: type(v) for k, v in graph.__dict__["_regions"].items()})
    for k in range(steps):
        for a, b, c in zip(got[k], want[k], fused[k]):
            assert torch.equal(a, b), k
            if p == 0:      # (with dropout the fused node scales conv2's input by a BOUND, max |h| / (1 - p), the drop-in by the
                assert torch.equal(a, c), ("the drop-in and the fused two-layer node differ", k)    # kept rows' maximum)
            else:
                assert (a - c).abs().max() <= 2e-5 * max(1.0, float(c.abs().max())), k


@pytest.mark.gpu
def test_fused_layers_on_degenerate_graphs(monkeypatch):
    """the one-kernel layers where little is left to gather: no edges at all, a single relation, fewer rows than a
    block, a graph whose every segment is long (all pre-aggregated), dropout between the layers (the second
    layer's input gradient then keeps the separate kernels: its weights are rescaled) - forced on for training,
    results equal to the separate kernels bit for bit"""
    from primekg_rgcn_linkprediction_amd import conv as C
    dev = need_gpu()
    gen = torch.Generator().manual_seed(1)
    cases = {
        "no edges": (torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 40, 3),
        "one relation": (torch.randint(0, 100, (2, 900), generator=gen), torch.zeros(900, dtype=torch.int64), 100, 1),
        "five rows": (torch.randint(0, 5, (2, 60), generator=gen), torch.randint(0, 2, (60,), generator=gen), 5, 2),
        "all long": (torch.stack([torch.randint(0, 64, (6000,), generator=gen), torch.randint(0, 2, (6000,), generator=gen)]),
                     torch.zeros(6000, dtype=torch.int64), 64, 1),
    }
    for name, (ei, et, n, r) in cases.items():
        eid, etd = ei.to(dev), et.to(dev)
        torch.manual_seed(4)
        emb = torch.randn(n, 64, device=dev)
        convs = [RGCNConv(64, 128, r).to(dev), RGCNConv(128, 128, r).to(dev)]
        cot = torch.randn(n, 128, device=dev)
        for p_drop in (0.0, 0.5):
            res = {}
            for mode in ("0", "1"):
                monkeypatch.setattr(C, "_TRAIN_FUSED", mode)
                e = emb.clone().requires_grad_(True)
                for c in convs:
                    c.zero_grad()
                torch.manual_seed(11)                             # the same dropout mask in both runs
                out = rgcn_encoder2(e, eid, etd, convs[0], convs[1], dropout_p=p_drop)
                (out * cot).sum().backward()
                res[mode] = [out.detach(), e.grad.clone()] + [p.grad.clone() for c in convs for p in c.parameters()]
            for a, b in zip(res["0"], res["1"]):
                assert torch.equal(a, b), (name, p_drop)
        with torch.no_grad():                                     # and the no-grad encoder (fused by default)
            monkeypatch.setattr(C, "_EVAL_FUSED", True)
            got = rgcn_encoder2(emb, eid, etd, convs[0], convs[1])
            monkeypatch.setattr(C, "_EVAL_FUSED", False)
            assert torch.equal(got, rgcn_encoder2(emb, eid, etd, convs[0], convs[1])), name


@pytest.mark.gpu
@pytest.mark.parametrize("d_in,d_out", [(64, 128), (128, 128), (128, 256), (256, 64)])
def test_hub_tails_left_to_the_transform_change_no_bit(d_in, d_out, monkeypatch):
    """ops.aggregate_deferred: the gather skips its hub-tail launch and the split-precision transform that reads the
    aggregate sums the partial rows of its own row tiles (the same function k_reduce_partials runs): outputs, the
    completed aggregate and - through the training node with the switch on and off - every gradient are bit-equal;
    forward and transposed direction, several column blocks finishing the same rows (d_out = 256), ReLU mask."""
    from primekg_rgcn_linkprediction_amd import conv as C
    dev = need_gpu()
    ei, et, n, r = synth.primekg_like(num_edges=400000, seed=17)
    eid, etd = ei.to(dev), et.to(dev)
    graph = ops.bucket(eid, etd, n, r)
    assert graph.num_levels(False) == 2 and graph.num_levels(True) == 2          # there ARE hub tails
    torch.manual_seed(d_in)
    x = torch.randn(n, d_in, device=dev)
    g = torch.randn(n, d_out, device=dev) * 1e-3
    weight = torch.randn(r, d_in, d_out, device=dev) / d_in ** 0.5
    root = torch.randn(d_in, d_out, device=dev) / d_in ** 0.5
    bias = torch.randn(d_out, device=dev)
    mask = torch.randn(n, d_in, device=dev)
    packed = ops.split_weights(weight, root)
    x_amax, g_amax = ops.absmax(x), ops.absmax(g)
    # forward
    agg_full = ops.aggregate(graph, x)
    want = ops.transform_fwd(agg_full, x, weight, root, bias, relu=True, graph=graph, amax=(x_amax, x_amax), packed=packed)
    agg, hubs = ops.aggregate_deferred(graph, x)
    assert hubs is not None                                                       # (the hub rows are not in agg yet)
    got = ops.transform_fwd(agg, x, weight, root, bias, relu=True, graph=graph, amax=(x_amax, x_amax), packed=packed,
                            hubs=hubs)
    assert torch.equal(got, want) and torch.equal(agg, agg_full)                  # ... and are, once the transform ran
    # input gradient (transposed structure, weighted sums, mask epilogue)
    gagg_full = ops.aggregate(graph, g, transposed=True)
    wb = graph.weight_bound(True)
    want = ops.transform_bwd_input(gagg_full, g, weight, root, relu_mask=mask, graph=graph, amax=(g_amax, g_amax),
                                   amax_mul=wb, packed=packed)
    gagg, hubs = ops.aggregate_deferred(graph, g, transposed=True)
    assert hubs is not None
    got = ops.transform_bwd_input(gagg, g, weight, root, relu_mask=mask, graph=graph, amax=(g_amax, g_amax),
                                  amax_mul=wb, packed=packed, hubs=hubs)
    assert torch.equal(got, want) and torch.equal(gagg, gagg_full)
    with pytest.raises(ValueError):                                               # the fp32 kernels do not finish hub rows
        ops.transform_fwd(agg, x, weight, root, bias, graph=graph, precision="fp32", hubs=hubs)
    if (d_in, d_out) != (64, 128):
        return
    # the training node, switch on / off
    convs = [RGCNConv(64, 128, r).to(dev), RGCNConv(128, 128, r).to(dev)]
    cot = torch.randn(n, 128, device=dev)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(C, "_DEFER_HUBS", on)
        e = x.clone().requires_grad_(True)
        for c in convs:
            c.zero_grad()
        out = rgcn_encoder2(e, eid, etd, convs[0], convs[1])
        (out * cot).sum().backward()
        res[on] = [out.detach(), e.grad.clone()] + [p.grad.clone() for c in convs for p in c.parameters()]
    for a, b in zip(res[False], res[True]):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("d", [8, 64, 264])
def test_gather_options_are_bit_for_bit_one_gather(d, transposed, monkeypatch):
    """every option of the gather (a pending tail, amax_out, both - the training route -, measurement mode, the levels
    left to the consuming transform, the fp16 table) issues the launches of the plain ``aggregate`` in the same order:
    rows, the tail's three gradients and the published maximum are bit-equal.  A hub segment in either direction (610
    edges: partial rows and a reduce level); d = 8 (every lane loads its ids), 64 (deferrable), 264 (past the riding
    limit of 256, second grid dimension; still a multiple of 8 for the fp16 table)."""
    dev = need_gpu()
    n, r = 64, 3
    gen = torch.Generator().manual_seed(29)
    spokes, hub = torch.arange(600) % n, torch.zeros(600, dtype=torch.int64)
    rnd = torch.randint(0, n, (2, 200), generator=gen)
    ei = torch.cat([torch.stack([spokes, hub]), torch.stack([hub + 1, spokes]), rnd], dim=1)
    et = torch.cat([torch.zeros(1200, dtype=torch.int64), torch.ones(200, dtype=torch.int64)])      # relation 2: empty
    graph = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
    assert graph.num_levels(False) == 2 and graph.num_levels(True) == 2
    x = torch.randn(n, d, generator=gen).to(dev)
    base = ops.aggregate(graph, x, transposed)
    if not transposed:
        assert_fwd(base.view(n, r, d), O.mean_aggregate_ref(x.cpu(), ei, et, r))
    # the tail: parameter gradients of a 64 x (64 -> 64) layer, their slab reduction pending
    pa, px, pg = (torch.randn(n, w, generator=gen).to(dev) for w in (r * 64, 64, 64))

    def pending():
        return ops.transform_bwd_params(pa, px, pg, r, defer=True)
    alone = pending()
    alone.finish()

    def check(rows, want, tail=None, slot=None):
        assert torch.equal(rows, want)
        if tail is not None:
            assert tail.done and all(torch.equal(a, b) for a, b in zip(tail.grads, alone.grads))
        if slot is not None:
            assert ops.amax_value(slot).item() == rows.abs().max().item() > 0

    def options():
        for with_tail in (True, False):
            for with_amax in (False, True):
                if with_tail or with_amax:
                    yield (pending() if with_tail else None), (ops.amax_buffer(dev)[0] if with_amax else None)

    for tail, slot in options():                     # riding (or launched first: d = 264), amax_out, both
        check(ops.aggregate(graph, x, transposed, tail=tail, amax_out=slot), base, tail, slot)
    # measurement mode: one call per level, level 0 between events, a pending tail finished first
    events = []
    monkeypatch.setattr(ops, "GATHER_EVENTS", events)
    for k, (tail, slot) in enumerate([(None, None)] + list(options())):
        check(ops.aggregate(graph, x, transposed, tail=tail, amax_out=slot), base, tail, slot)
        assert len(events) == k + 1 and events[-1][:5] == (transposed, d, 1400, n * r, n)
    monkeypatch.setattr(ops, "GATHER_EVENTS", None)
    # the reduce level left to the transform that consumes the rows (d = 64 only), a tail riding all the same
    tail = pending()
    rows, hubs = ops.aggregate_deferred(graph, x, transposed, tail=tail)
    assert (hubs is not None) == (d == 64)
    if hubs is not None:
        weight, root = torch.randn(r, d, d, generator=gen).to(dev) / 8, torch.randn(d, d, generator=gen).to(dev) / 8
        x_amax = ops.absmax(x)
        if transposed:
            ops.transform_bwd_input(rows, x, weight, root, graph=graph, amax=(x_amax, x_amax),
                                    amax_mul=graph.weight_bound(True), hubs=hubs)
        else:
            ops.transform_fwd(rows, x, weight, root, graph=graph, amax=(x_amax, x_amax), hubs=hubs)
    check(rows, base, tail)
    # fp16 table: against its own plain gather, the tail launched by itself first
    tail = pending()
    check(ops.aggregate(graph, x.half(), transposed, tail=tail), ops.aggregate(graph, x.half(), transposed), tail)
