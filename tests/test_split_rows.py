"""GPU tier: the split-precision transforms gated ROW BY ROW against float64.

``rel_err`` in test_gpu_parity.py divides the largest error of a tensor by its largest entry, so a row a few binades
below the tensor's maximum could be wrong in its 4th significant digit unseen.  The gates here are per row (NT
outputs: forward, input gradient, transform-first ``T``) and per element (TN outputs: weight, root and bias gradients),
each against a float64 product of the same fp32 operands and made fair to cancellation by the exact-fp32 kernels'
own error on the same inputs:

* ``assert_rows``: every row whose largest |entry| is at least 2^-16 of the tensor's keeps its row-relative error at
  ``max(FLOOR, 2 x the fp32 kernel's row-relative error)``; every other row keeps ``|delta| <= 2^-30 max|want|``.
* ``assert_elems``: ``|delta_kn| <= max(FLOOR (|A|^T |G|)_kn, 2 |delta of the fp32 kernel|_kn)``.

The same helpers run on the fp32 kernels' output against the bare FLOOR, so the gate is never tighter than fp32.
Operands (seeded): rows spread over 24 binades, one hub row at x300, exact-zero rows, A1 / A2 maxima 2^12 apart,
gradients at ~1e-7.  The operand scales are the operands' own maxima (given as the bound ``amax_mul * value`` where a
call takes one)."""
import pytest
import torch

from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import ops

pytestmark = pytest.mark.gpu

FLOOR = 4e-6
BIG_ROW = 2.0 ** -16          # rows at least this far up (relative to the tensor's max) get the row-relative gate
SMALL_ABS = 2.0 ** -30        # the others: absolute error against the tensor's max


# ------------------------------------------------------------------ gates
def _row_rel(got, want64):
    d = (got.double().cpu() - want64).abs().amax(1)
    m = want64.abs().amax(1)
    return d / torch.where(m > 0, m, torch.ones_like(m)), m


def assert_rows(got, want64, fp32_got=None, floor=FLOOR, what=""):
    """row gate of an NT output (rows independent) against its float64 value ``want64`` (CPU)"""
    want64 = want64.double().cpu()
    assert tuple(got.shape) == tuple(want64.shape), what
    if want64.numel() == 0:
        return
    rel, m = _row_rel(got, want64)
    gmax = float(m.max())
    if gmax == 0.0:
        assert float(got.abs().max()) == 0.0, f"{what}: nonzero output where float64 is all zero"
        return
    big = m >= gmax * BIG_ROW
    lim = torch.full_like(rel, floor)
    if fp32_got is not None:
        lim = torch.maximum(lim, 2.0 * _row_rel(fp32_got, want64)[0])
    bad = big & (rel > lim)
    if bool(bad.any()):
        i = int(torch.argmax(torch.where(bad, rel / lim, torch.zeros_like(rel))))
        binades = float(torch.log2(gmax / m[i]))
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(big.sum())} rows over the row gate; worst row {i} "
                             f"({binades:.1f} binades below the max): row-relative error {float(rel[i]):.3e} > "
                             f"{float(lim[i]):.3e}")
    if bool((~big).any()):
        d = (got.double().cpu() - want64).abs()[~big]
        assert float(d.max()) <= SMALL_ABS * gmax, (
            f"{what}: small rows err by {float(d.max()):.3e} > 2^-30 * {gmax:.3e}")


def assert_elems(got, absprod, want64, fp32_got=None, floor=FLOOR, what=""):
    """element gate of a TN output: ``absprod`` = ``|A|^T |G|`` (float64, CPU), ``want64`` = ``A^T G``"""
    want64, absprod = want64.double().cpu(), absprod.double().cpu()
    d = (got.double().cpu() - want64).abs()
    lim = floor * absprod
    if fp32_got is not None:
        lim = torch.maximum(lim, 2.0 * (fp32_got.double().cpu() - want64).abs())
    bad = d > lim
    if bool(bad.any()):
        ratio = torch.where(bad, d / torch.where(absprod > 0, absprod, torch.ones_like(absprod)), torch.zeros_like(d))
        i = int(torch.argmax(ratio))
        raise AssertionError(f"{what}: {int(bad.sum())} of {d.numel()} elements over the element gate; worst "
                             f"|delta| {float(d.view(-1)[i]):.3e} against |A|^T|G| {float(absprod.view(-1)[i]):.3e} "
                             f"(limit {float(lim.view(-1)[i]):.3e})")


# ------------------------------------------------------------------ operands
PROFILES = ["spread", "hub", "zeros"]


def operand(m, k, profile, gen, scale=1.0):
    """[m, k] float32 (CPU) of one profile: rows spread uniformly over 24 binades, one hub row at x300, or every
    third row exactly zero"""
    a = torch.randn(m, k, generator=gen, dtype=torch.float64)
    if profile == "spread":
        a *= torch.exp2(-24.0 * torch.rand(m, 1, generator=gen, dtype=torch.float64))
    elif profile == "hub":
        a[m // 2] *= 300.0
    elif profile == "zeros":
        a[::3] = 0.0
    return (a * scale).float()


def weights(r, d_in, d_out, gen, root=True):
    w = (torch.randn(r, d_in, d_out, generator=gen) / d_in ** 0.5).float()
    rt = (torch.randn(d_in, d_out, generator=gen) / d_in ** 0.5).float() if root else None
    return w, rt


def bound_buffer(t, mul):
    """an amax buffer whose value times ``mul`` is max |t| (the form a caller hands a BOUND in)"""
    return ops.absmax(t / mul) if mul != 1.0 else ops.absmax(t)


# ------------------------------------------------------------------ forward (NT)
#            M      R   d_in d_out root  bias  relu
FWD = [(1, 1, 32, 4, True, False, False), (31, 3, 32, 36, True, True, True), (33, 33, 32, 100, False, False, False),
       (777, 3, 64, 128, True, True, False), (777, 1, 128, 256, True, False, True), (30926, 3, 64, 128, True, True, True),
       (64, 3, 64, 64, False, True, False)]


@pytest.mark.parametrize("profile", PROFILES + ["a2_low", "a1_low"])
@pytest.mark.parametrize("m,r,d_in,d_out,has_root,has_bias,relu", FWD)
def test_forward_rows(m, r, d_in, d_out, has_root, has_bias, relu, profile):
    dev = need_gpu()
    gen = torch.Generator().manual_seed(m * 131 + d_out)
    base = profile if profile in PROFILES else "spread"
    agg = operand(m, r * d_in, base, gen, 2.0 ** -12 if profile == "a1_low" else 1.0)
    x = operand(m, d_in, base, gen, 2.0 ** -12 if profile == "a2_low" else 1.0)
    w, root = weights(r, d_in, d_out, gen, has_root)
    bias = (torch.randn(d_out, generator=gen) * 1e-3).float() if has_bias else None
    want = agg.double() @ w.double().reshape(r * d_in, d_out)
    if has_root:
        want += x.double() @ root.double()
    if has_bias:
        want += bias.double()
    if relu:
        want = want.clamp(min=0)
    args = [t.to(dev) if t is not None else None for t in (agg, x, w, root, bias)]
    packed = ops.split_weights(args[2], args[3]) if m > 100 else None          # the step's images, or split in the call
    got = ops.transform_fwd(*args, relu=relu, packed=packed, precision="split")
    f32 = ops.transform_fwd(*args, relu=relu, precision="fp32")
    assert_rows(f32, want, what="fp32 forward")
    assert_rows(got, want, f32, what="split forward")


# ------------------------------------------------------------------ input gradient (NT)
#            M      R   d_in d_out root  mask  out_scale
BWD = [(1, 1, 4, 32, True, False, 1.0), (31, 3, 36, 32, True, True, 1.0), (33, 33, 100, 32, False, False, 2.0),
       (777, 3, 64, 128, True, True, 1.0), (777, 1, 256, 64, True, False, 1.0), (30926, 3, 128, 128, True, True, 2.0),
       (100, 3, 128, 64, False, True, 1.0)]


# amax_mul = 1300: the multiplier of the caller's bound is applied (the buffer holds max / 1300).  A bound that is
# really 1300x loose is never handed to these kernels by the layers: the tests at the end of this file check the
# layers' own input gradients on a graph whose weight bound is ~800.
@pytest.mark.parametrize("amax_mul", [1.0, 1300.0])
@pytest.mark.parametrize("profile", PROFILES + ["a2_low", "tiny"])
@pytest.mark.parametrize("m,r,d_in,d_out,has_root,has_mask,out_scale", BWD)
def test_input_gradient_rows(m, r, d_in, d_out, has_root, has_mask, out_scale, profile, amax_mul):
    dev = need_gpu()
    gen = torch.Generator().manual_seed(m * 17 + d_in)
    base = profile if profile in PROFILES else "spread"
    s = 1e-7 if profile == "tiny" else 1.0
    gagg = operand(m, r * d_out, base, gen, s)
    g = operand(m, d_out, base, gen, s * (2.0 ** -12 if profile == "a2_low" else 1.0))
    w, root = weights(r, d_in, d_out, gen, has_root)
    mask = torch.randn(m, d_in, generator=gen) if has_mask else None
    wt = w.double().transpose(1, 2).reshape(r * d_out, d_in)
    want = gagg.double() @ wt
    if has_root:
        want += g.double() @ root.double().t()
    if has_mask:
        want *= (mask > 0).double()
    want *= out_scale
    gagg_d, g_d, w_d = gagg.to(dev), g.to(dev), w.to(dev)
    root_d = root.to(dev) if has_root else None
    mask_d = mask.to(dev) if has_mask else None
    amax = (bound_buffer(gagg_d, amax_mul), ops.absmax(g_d))
    got = ops.transform_bwd_input(gagg_d, g_d, w_d, root_d, relu_mask=mask_d, amax=amax, amax_mul=amax_mul,
                                  packed=ops.split_weights(w_d, root_d), precision="split", out_scale=out_scale)
    f32 = ops.transform_bwd_input(gagg_d, g_d, w_d, root_d, relu_mask=mask_d, precision="fp32", out_scale=out_scale)
    assert_rows(f32, want, what="fp32 input gradient")
    assert_rows(got, want, f32, what="split input gradient")


# ------------------------------------------------------------------ parameter gradients (TN)
def _param_refs(agg, x, g, r, d_in, d_out):
    a64, x64, g64 = agg.double(), x.double(), g.double()
    return ((a64.t() @ g64).view(r, d_in, d_out), (a64.abs().t() @ g64.abs()).view(r, d_in, d_out),
            x64.t() @ g64, x64.abs().t() @ g64.abs(), g64.sum(0), g64.abs().sum(0))


def _check_params(got, f32, refs, want_root, want_bias, what):
    gw, gw_abs, gr, gr_abs, gb, gb_abs = refs
    assert_elems(f32[0], gw_abs, gw, what=f"fp32 {what} weight")
    assert_elems(got[0], gw_abs, gw, f32[0], what=f"split {what} weight")
    assert (got[1] is None) == (not want_root) and (got[2] is None) == (not want_bias)
    if want_root:
        assert_elems(f32[1], gr_abs, gr, what=f"fp32 {what} root")
        assert_elems(got[1], gr_abs, gr, f32[1], what=f"split {what} root")
    if want_bias:
        assert_elems(f32[2], gb_abs, gb, what=f"fp32 {what} bias")
        assert_elems(got[2], gb_abs, gb, f32[2], what=f"split {what} bias")


#             M      R   d_in d_out
PARAMS = [(1, 1, 64, 4), (31, 3, 64, 36), (33, 33, 64, 100), (777, 3, 64, 128), (777, 1, 128, 256),
          (30926, 3, 64, 128), (100, 3, 128, 64)]


@pytest.mark.parametrize("want_root,want_bias", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("profile", PROFILES + ["a1_low", "a2_low", "tiny"])
@pytest.mark.parametrize("m,r,d_in,d_out", PARAMS)
def test_parameter_gradient_elements(m, r, d_in, d_out, profile, want_root, want_bias):
    dev = need_gpu()
    gen = torch.Generator().manual_seed(m * 7 + d_out)
    base = profile if profile in PROFILES else "spread"
    agg = operand(m, r * d_in, base, gen, 2.0 ** -12 if profile == "a1_low" else 1.0)
    x = operand(m, d_in, base, gen, 2.0 ** -12 if profile == "a2_low" else 1.0)
    g = operand(m, d_out, base, gen, 1e-7 if profile == "tiny" else 1.0)
    refs = _param_refs(agg, x, g, r, d_in, d_out)
    args = (agg.to(dev), x.to(dev), g.to(dev), r)
    got = ops.transform_bwd_params(*args, want_root=want_root, want_bias=want_bias, precision="split")
    f32 = ops.transform_bwd_params(*args, want_root=want_root, want_bias=want_bias, precision="fp32")
    _check_params(got, f32, refs, want_root, want_bias, "parameter gradient")


def _typed_graph(n, free, seed):
    """rows [0, free) receive relation 1 only; rows [free, n) all three relations"""
    gen = torch.Generator().manual_seed(seed)
    e = 8 * n
    dst = torch.randint(0, n, (e,), generator=gen)
    src = torch.randint(0, n, (e,), generator=gen)
    typ = torch.randint(0, 3, (e,), generator=gen)
    typ[dst < free] = 1
    return torch.stack([src, dst]), typ


@pytest.mark.parametrize("n,free,d_out", [(30926, 5593, 128), (200, 150, 64), (777, 700, 36)])
def test_parameter_gradients_of_row_splits_without_a_relation(n, free, d_out):
    """k_gemm_tn_coop with the relation-occupancy mask: whole row splits have no live m-tile in the kc tiles of
    relations 0 and 2, so their workgroups skip the main loop (the epilogue must not overwrite LDS that prologue DMAs
    are still filling).  Masked == dense bit for bit and both within the element gate.  A timing race: this test may
    pass without the drain it guards."""
    dev = need_gpu()
    r, d_in = 3, 64
    ei, et = _typed_graph(n, free, n)
    graph = ops.bucket(ei.to(dev), et.to(dev), n, r)
    gen = torch.Generator().manual_seed(n)
    x = operand(n, d_in, "spread", gen).to(dev)
    agg = ops.aggregate(graph, x)
    assert float(agg[:free, : d_in].abs().max()) == 0.0 and float(agg[:free, 2 * d_in:].abs().max()) == 0.0
    g = operand(n, d_out, "spread", gen).to(dev)
    refs = _param_refs(agg.cpu(), x.cpu(), g.cpu(), r, d_in, d_out)
    for want_root, want_bias in ((True, True), (False, False)):
        masked = ops.transform_bwd_params(agg, x, g, r, want_root, want_bias, graph=graph, precision="split")
        dense = ops.transform_bwd_params(agg, x, g, r, want_root, want_bias, precision="split")
        for a, b in zip(masked, dense):
            assert (a is None and b is None) or torch.equal(a, b)
        f32 = ops.transform_bwd_params(agg, x, g, r, want_root, want_bias, graph=graph, precision="fp32")
        _check_params(masked, f32, refs, want_root, want_bias, "masked parameter gradient")


# ------------------------------------------------------------------ transform-first product and the chained launch
@pytest.mark.parametrize("profile", PROFILES + ["tiny"])
@pytest.mark.parametrize("m,r,d_in,d_out,has_root", [(1, 1, 32, 32, True), (33, 3, 32, 64, False), (777, 3, 64, 128, True),
                                                     (30926, 3, 64, 128, True), (31, 33, 32, 32, True)])
def test_transform_first_rows(m, r, d_in, d_out, has_root, profile):
    dev = need_gpu()
    gen = torch.Generator().manual_seed(m + d_in)
    g = operand(m, d_out, profile if profile in PROFILES else "spread", gen, 1e-7 if profile == "tiny" else 1.0)
    w, root = weights(r, d_in, d_out, gen, has_root)
    wcat = torch.cat([w.reshape(r * d_in, d_out)] + ([root] if has_root else []))
    want = g.double() @ wcat.double().t()
    g_d, w_d, root_d = g.to(dev), w.to(dev), (root.to(dev) if has_root else None)
    got = ops.transform_first(g_d, ops.split_weights(w_d, root_d), ops.absmax(g_d))
    f32 = ops.transform_bwd_input(g_d, g_d, wcat.to(dev).view(1, -1, d_out), None, precision="fp32")
    assert_rows(f32, want, what="fp32 transform-first")
    assert_rows(got, want, f32, what="split transform-first")


# n % 64 != 0; (R1 + root1) * d_in1 not a multiple of 128; no root in conv1; no root in conv2 (K2 = 0)
@pytest.mark.parametrize("profile", PROFILES + ["tiny"])
@pytest.mark.parametrize("n,d_in1,d_out2,root1,root2", [(30926, 64, 128, True, True), (1000, 32, 128, False, False),
                                                        (33, 32, 64, False, True), (777, 64, 96, False, False),
                                                        (1, 64, 32, True, True)])
def test_chained_transform_first_rows_and_tails(n, d_in1, d_out2, root1, root2, profile):
    """``transform_bwd_input_chain``: gz bit-equal to the two-launch form, T (split under each 64-row tile's maximum of
    gz) within the row gate of float64 T = gz W1cat^T"""
    dev = need_gpu()
    r, hidden = 3, 128
    gen = torch.Generator().manual_seed(n + d_in1)
    base = profile if profile in PROFILES else "spread"
    s = 1e-7 if profile == "tiny" else 1.0
    w2, rt2 = weights(r, hidden, d_out2, gen, root2)
    w1, rt1 = weights(r, d_in1, hidden, gen, root1)
    g, gagg = operand(n, d_out2, base, gen, s), operand(n, r * d_out2, base, gen, s)
    h = torch.randn(n, hidden, generator=gen)
    w2, w1, g, gagg, h = (t.to(dev) for t in (w2, w1, g, gagg, h))
    rt2 = rt2.to(dev) if root2 else None
    rt1 = rt1.to(dev) if root1 else None
    pk2, pk1 = ops.split_weights_many([(w2, rt2), (w1, rt1)])
    assert ops.chain_supported(w2, w1)
    amax = (ops.absmax(gagg), ops.absmax(g))
    za, zb = ops.amax_buffer(dev, 2)
    want_gz = ops.transform_bwd_input(gagg, g, w2, rt2, relu_mask=h, amax=amax, amax_out=za, packed=pk2)
    gz, t = ops.transform_bwd_input_chain(gagg, g, w2, rt2, h, pk2, pk1, amax=amax, amax_out=zb)
    assert torch.equal(gz, want_gz) and torch.equal(ops.amax_value(za), ops.amax_value(zb))
    wcat = torch.cat([w1.reshape(r * d_in1, hidden)] + ([rt1] if root1 else []))
    f32 = ops.transform_bwd_input(gz, gz, wcat.view(1, -1, hidden), None, precision="fp32")
    assert_rows(f32, gz.double().cpu() @ wcat.double().cpu().t(), what="fp32 T")
    assert_rows(t, gz.double().cpu() @ wcat.double().cpu().t(), f32, what="chained T")
    # and gz itself against float64
    wt = w2.double().cpu().transpose(1, 2).reshape(r * d_out2, hidden)
    want = gagg.double().cpu() @ wt
    if root2:
        want += g.double().cpu() @ rt2.double().cpu().t()
    want *= (h.cpu() > 0).double()
    f32gz = ops.transform_bwd_input(gagg, g, w2, rt2, relu_mask=h, precision="fp32")
    assert_rows(gz, want, f32gz, what="chained gz")


# ------------------------------------------------------------------ layers on a hub graph
def _hub_graph(n, seed):
    """three relations of one in- and one out-edge per node (weights 1: weight_bound 1 both ways) plus node 0 ->
    node 1 repeated 300 times under relation 0: a segment of 301 edges in both directions (a hub row of the fused
    plans and a deferred hub tail of the gathers) that keeps the bound at 1"""
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    src, dst, typ = [], [], []
    for rel in range(3):
        s = torch.arange(n)
        d = perm[(torch.arange(n) + 1 + rel) % n]
        src.append(s)
        dst.append(d)
        typ.append(torch.full((n,), rel))
    tgt = int(perm[1])                                           # node 0's own relation-0 edge goes here
    src.append(torch.zeros(300, dtype=torch.int64))
    dst.append(torch.full((300,), tgt))
    typ.append(torch.zeros(300, dtype=torch.int64))
    return torch.stack([torch.cat(src), torch.cat(dst)]), torch.cat(typ)


def _mean_agg64(x, ei, et, n, r, transposed):
    """float64 [N, R*d] mean aggregate (transposed: the 1/cnt-weighted sums over out-edges)"""
    x = x.double()
    src, dst = ei[0], ei[1]
    cnt = torch.zeros(n * r, dtype=torch.float64).index_add_(0, dst * r + et, torch.ones(et.numel(), dtype=torch.float64))
    out = torch.zeros(n * r, x.size(1), dtype=torch.float64)
    if not transposed:
        out.index_add_(0, dst * r + et, x[src])
        out /= cnt.clamp(min=1).unsqueeze(1)
    else:
        out.index_add_(0, src * r + et, x[dst] / cnt[dst * r + et].unsqueeze(1))
    return out.view(n, r * x.size(1))


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("n,d_in,d_out", [(777, 64, 128), (4000, 128, 128), (1000, 64, 128)])
def test_fused_layers_and_deferred_hubs_rows(n, d_in, d_out, profile):
    dev = need_gpu()
    r = 3
    ei, et = _hub_graph(n, n)
    graph = ops.bucket(ei.to(dev), et.to(dev), n, r)
    assert graph.weight_bound(True) <= 1.0 + 1e-6
    gen = torch.Generator().manual_seed(n + d_out)
    x = operand(n, d_in, profile, gen)
    g = operand(n, d_out, profile, gen)
    mask = torch.randn(n, d_in, generator=gen)
    w, root = weights(r, d_in, d_out, gen)
    bias = (torch.randn(d_out, generator=gen) * 1e-3).float()
    agg64, gagg64 = _mean_agg64(x, ei, et, n, r, False), _mean_agg64(g, ei, et, n, r, True)
    fwd = (agg64 @ w.double().reshape(r * d_in, d_out) + x.double() @ root.double() + bias.double()).clamp(min=0)
    bwd = (gagg64 @ w.double().transpose(1, 2).reshape(r * d_out, d_in) + g.double() @ root.double().t()) * (mask > 0)
    x, g, mask, w, root, bias = (t.to(dev) for t in (x, g, mask, w, root, bias))
    packed = ops.split_weights(w, root)
    x_amax, g_amax = ops.absmax(x), ops.absmax(g)
    agg, gagg = ops.aggregate(graph, x), ops.aggregate(graph, g, transposed=True)
    f32_fwd = ops.transform_fwd(agg, x, w, root, bias, relu=True, precision="fp32")
    f32_bwd = ops.transform_bwd_input(gagg, g, w, root, relu_mask=mask, precision="fp32")
    assert_rows(f32_fwd, fwd, what="fp32 layer forward")
    assert_rows(f32_bwd, bwd, what="fp32 layer input gradient")
    got = ops.layer_fwd_fused(graph, x, packed, bias, True, x_amax, inline_limit=16)
    assert_rows(got, fwd, f32_fwd, what="fused layer forward")
    got = ops.layer_bwd_input_fused(graph, g, packed, mask, g_amax, inline_limit=16)
    assert_rows(got, bwd, f32_bwd, what="fused layer input gradient")
    if d_in in (64, 128) and d_out <= 128:
        a, hubs = ops.aggregate_deferred(graph, x)
        got = ops.transform_fwd(a, x, w, root, bias, relu=True, graph=graph, amax=(x_amax, x_amax), packed=packed,
                                hubs=hubs)
        assert_rows(got, fwd, f32_fwd, what="forward with deferred hubs")
    if d_out in (64, 128) and d_in <= 128:
        a, hubs = ops.aggregate_deferred(graph, g, transposed=True)
        got = ops.transform_bwd_input(a, g, w, root, relu_mask=mask, graph=graph, amax=(g_amax, g_amax),
                                      amax_mul=graph.weight_bound(True), packed=packed, hubs=hubs)
        assert_rows(got, bwd, f32_bwd, what="input gradient with deferred hubs")


# ------------------------------------------------------------------ the layers' input gradients on a PrimeKG-shaped graph
# The transposed aggregate of a gradient is bounded by weight_bound(True) * max |g|: ~800x its real maximum on this
# graph.  Scaled by that bound its ordinary rows lose ~10 bits of the lo half (measured before the layers scaled it by
# its own maximum: row-relative errors 1.6e-5 at 12-14 binades below the maximum, 5.4e-5 at 14-16, end-to-end grad_x
# 3.6e-5), so these cases gate the layers' own backward, plain, fused and chained, with a cotangent over 16 binades.
def _primekg_graph(dev):
    from primekg_rgcn_linkprediction_amd import synth
    ei, et, n, r = synth.primekg_like(num_edges=200000)
    graph = ops.bucket(ei.to(dev), et.to(dev), n, r)
    assert graph.weight_bound(True) > 100.0                 # the bound is far from the aggregate's real maximum
    return ei, et, n, r


def _cotangent(n, d, seed):
    gen = torch.Generator().manual_seed(seed)
    c = torch.randn(n, d, generator=gen, dtype=torch.float64) * torch.exp2(-16.0 * torch.rand(n, 1, generator=gen,
                                                                                               dtype=torch.float64))
    return c.float()


def _shard_input_grads(ei, et, n, r, w, root, cot, dev):
    """grad_x of a two-rank partition through dist.HipBackend, each rank's halo exchange emulated from the full
    cotangent: -> [(form, grad_x in node order)] for the one-pass shards and the interior / boundary halves"""
    from types import SimpleNamespace
    from primekg_rgcn_linkprediction_amd import dist as rdist
    backend = rdist.HipBackend()
    part = rdist.NodePartition(ei, n, 2)
    results = []
    for split in (False, True):
        rows = []
        for k in range(2):
            shard = rdist.RankShard(part, ei, et, r, k, dev, backend, split=split)
            assert shard.split == split
            g_own = part.shard_rows(cot, k).to(dev)
            halo = SimpleNamespace(table=lambda: shard.halo_out.emulate(g_own, cot.to(dev)))
            rows.append(rdist._input_grad(g_own, w.to(dev), root.to(dev), None, shard, backend, None, halo))
        results.append(("halves" if split else "one pass", part.unshard_rows(torch.cat(rows))))
    return results


@pytest.mark.parametrize("mode", ["plain", "fused", "shard"])
def test_layer_input_gradient_rows_on_a_primekg_graph(mode, monkeypatch):
    """rgcn_conv 128 -> 128 (gather first: the transposed aggregate feeds the transform) through autograd; "shard": the
    input gradient of each rank of a node partition (dist.HipBackend)"""
    from primekg_rgcn_linkprediction_amd import conv as C, rgcn_conv
    dev = need_gpu()
    monkeypatch.setattr(C, "_TRAIN_FUSED", "1" if mode == "fused" else "0")
    ei, et, n, r = _primekg_graph(dev)
    gen = torch.Generator().manual_seed(3)
    w, root = weights(r, 128, 128, gen)
    x = torch.randn(n, 128, generator=gen).to(dev).requires_grad_(True)
    cot = _cotangent(n, 128, 4)
    if mode == "shard":
        got = _shard_input_grads(ei, et, n, r, w, root, cot, dev)
    else:
        out = rgcn_conv(x, ei.to(dev), et.to(dev), w.to(dev), root.to(dev), None, r)
        out.backward(cot.to(dev))
        got = [("autograd", x.grad)]
    wt = w.transpose(1, 2).reshape(r * 128, 128)
    refs = [_mean_agg64(cot, ei, et, n, r, True).to(dt) @ wt.to(dt) + cot.to(dt) @ root.t().to(dt)
            for dt in (torch.float64, torch.float32)]
    for form, gx in got:
        assert_rows(gx, refs[0], refs[1], what=f"{mode} input gradient ({form})")


def _encoder_ref(x, c1, c2, cot, ei, et, n, r, relu_mask, keep, p, dt):
    """conv1 -> ReLU -> dropout(keep, p) -> conv2 and its backward in dtype dt (CPU), the ReLU decisions given"""
    x, cot = x.to(dt), cot.to(dt)
    w1, r1, b1, w2, r2, b2 = (t.to(dt) for t in c1 + c2)
    agg = lambda t, tr: _mean_agg64(t, ei, et, n, r, tr).to(dt)
    agg1 = agg(x, False)
    h = (agg1 @ w1.reshape(-1, w1.size(2)) + x @ r1 + b1) * relu_mask
    f = keep / (1.0 - p) if p > 0 else torch.ones_like(h)
    ghd = agg(cot, True) @ w2.transpose(1, 2).reshape(-1, w2.size(1)) + cot @ r2.t()
    gz = ghd * f * relu_mask
    gx = agg(gz, True) @ w1.transpose(1, 2).reshape(-1, w1.size(1)) + gz @ r1.t()
    return gx, agg1, gz


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_encoder_backward_rows_on_a_primekg_graph(p):
    """rgcn_encoder2 (default policy: conv2's input gradient chained with conv1's transform-first product) in training
    mode; grad_x row by row, conv1's weight and root gradients element by element, against float64 (the dropout mask
    is the run's: the same seed redrawn)"""
    from primekg_rgcn_linkprediction_amd import RGCNConv, rgcn_encoder2
    dev = need_gpu()
    ei, et, n, r = _primekg_graph(dev)
    eid, etd = ei.to(dev), et.to(dev)
    torch.manual_seed(0)
    c1, c2 = RGCNConv(64, 128, r).to(dev), RGCNConv(128, 128, r).to(dev)
    x = torch.randn(n, 64, device=dev, requires_grad=True)
    cot = _cotangent(n, 128, 9)
    torch.manual_seed(21)
    out = rgcn_encoder2(x, eid, etd, c1, c2, p)
    out.backward(cot.to(dev))
    from primekg_rgcn_linkprediction_amd import rgcn_conv
    with torch.no_grad():                          # conv1 + ReLU by the same kernels: the run's ReLU decisions
        h = rgcn_conv(x, eid, etd, c1.weight, c1.root, c1.bias, r, activation="relu")
        keep = torch.ones_like(h)
        if p > 0:
            torch.manual_seed(21)
            keep = (torch.native_dropout(torch.ones_like(h), p, True)[1]).float()
    relu_mask = (h > 0).float().cpu()
    params = lambda c: [c.weight.detach().cpu(), c.root.detach().cpu(), c.bias.detach().cpu()]
    x_cpu = x.detach().cpu()
    refs = [_encoder_ref(x_cpu, params(c1), params(c2), cot, ei, et, n, r, relu_mask, keep.cpu(), p, dt)
            for dt in (torch.float64, torch.float32)]
    (gx64, agg1, gz64), (gx32, agg1_32, gz32) = refs
    assert_rows(x.grad, gx64, gx32, what=f"encoder grad_x, p = {p}")
    gw, gw_abs = (agg1.t() @ gz64).view(r, 64, 128), (agg1.abs().t() @ gz64.abs()).view(r, 64, 128)
    f32_w = (agg1_32.t() @ gz32).view(r, 64, 128)
    assert_elems(c1.weight.grad, gw_abs, gw, f32_w, what=f"conv1 weight gradient, p = {p}")
    assert_elems(c1.root.grad, x_cpu.double().abs().t() @ gz64.abs(), x_cpu.double().t() @ gz64,
                 x_cpu.t() @ gz32, what=f"conv1 root gradient, p = {p}")
