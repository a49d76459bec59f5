"""GPU tier of the relational attention layer: the attention draw (``ops.EdgeDropout.set_attention``;
``RGCN_EDGE_DROPOUT_ATTENTION`` of ``rgcn_edge_dropout_draw``) against its float64 restatement inside the bound
``attention_reference`` derives from the header's ``exp`` contract and the sum's depth, bit for bit where the header
promises bits; the per-segment edge sum (``ops.edge_segment_sum``; ``RGCN_MODE_EDGE_SUM``) bit for bit; the layer, the
trainer and a planted toy.  One ragged graph: N = 70 (no multiple of 32), R = 3, forward segments of 1, 2, 8, 9, 63, 64,
65, 257 and 1,300 edges, empty segments, duplicate columns, self loops and pairs stored in both directions."""
import functools

import numpy as np
import pytest
import torch

import attention_reference as ref
import edge_dropout_twins_reference as twins_ref
from conftest import need_gpu
from guarded import bits
from primekg_rgcn_linkprediction_amd import ops, rgcn_conv
from primekg_rgcn_linkprediction_amd import train as T
from primekg_rgcn_linkprediction_amd.attention import RelationalAttentionConv
from test_attention_host import TOY_LR, TOY_STEPS, planted_toy, toy_parameters
from test_gpu_parity import assert_fwd, assert_grad, rel_err

pytestmark = pytest.mark.gpu

N, R = 70, 3
PLANTED = {(3, 0): 1, (4, 1): 2, (5, 2): 8, (6, 0): 9, (7, 1): 63, (8, 2): 64, (9, 0): 65, (10, 1): 257, (11, 2): 1300}
SLOPE = 0.2


def _columns():
    """-> (edge_index [2, E], edge_type [E]) on the CPU: the planted segments with sources among nodes 20..69 (so every
    longer segment holds duplicate columns), a self loop in each of three segments, and the reversed column of the first
    four edges of segment (6, 0) - stored pairs, for ``hide_twins``"""
    gen = torch.Generator().manual_seed(17)
    src, dst, rel = [], [], []
    for (node, r), n in PLANTED.items():
        s = torch.randint(20, N, (n,), generator=gen)
        if n in (9, 65, 1300):
            s[n // 2] = node                                   # a self loop
        src.append(s); dst.append(torch.full((n,), node)); rel.append(torch.full((n,), r))
    src, dst, rel = torch.cat(src), torch.cat(dst), torch.cat(rel)
    first = int(torch.nonzero((dst == 6) & (rel == 0))[0])
    pair = torch.arange(first, first + 4)                      # (their sources are no self loop: that one sits at index 4)
    src, dst, rel = torch.cat([src, dst[pair]]), torch.cat([dst, src[pair]]), torch.cat([rel, rel[pair]])
    order = torch.randperm(src.numel(), generator=gen)
    return torch.stack([src, dst])[:, order].contiguous(), rel[order].contiguous()


@functools.lru_cache(maxsize=None)
def _world():
    """-> (graph, EdgeDropout, edge_index, edge_type, {transposed: (rowptr, col, perm) on the CPU}, twin int32 [E])"""
    dev = need_gpu()
    ei, et = _columns()
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), N, R)
    arrays = {t: tuple(a.cpu() for a in g.arrays(t)[:3]) for t in (False, True)}
    lens = torch.bincount(ei[1] * R + et, minlength=N * R)
    assert set(PLANTED.values()) <= set(lens.tolist()) and int((lens == 0).sum()) > 0 and int((ei[0] == ei[1]).sum()) == 3
    twin = twins_ref.twins(ei.numpy(), et.numpy())
    assert int((twin >= 0).sum()) == 8
    dup = torch.unique(torch.stack([ei[0], ei[1], et]), dim=1).size(1)
    assert dup < ei.size(1)                                     # duplicate columns
    return g, ops.EdgeDropout(g), ei, et, arrays, twin


def _seg(length):
    (node, r), = [k for k, v in PLANTED.items() if v == length]
    return node * R + r


def _weights(ed):
    """the view's weights of both directions, by ORIGINAL column, on the CPU"""
    out = []
    for t in (False, True):
        _, _, perm, val = ed.view.arrays(t)
        w = torch.empty_like(val)
        w[perm] = val
        out.append(w.cpu())
    return out


def _scalars(scale, seed=3):
    return (scale * torch.randn(2, N, R, generator=torch.Generator().manual_seed(seed))).contiguous()


def _window(ei, first, dev):
    """position with the bool ``first`` columns standing at [5, 5 + h), cursor 5 -> keywords of a draw"""
    e = ei.size(1)
    rest = torch.nonzero(~first).view(-1)
    order = torch.cat([rest[:5], torch.nonzero(first).view(-1), rest[5:]])
    position = torch.empty(e, dtype=torch.int64)
    position[order] = torch.arange(e)
    return dict(position=position.to(dev), cursor=torch.tensor([5], dtype=torch.int64, device=dev), batch=int(first.sum()))


def _with_half_pairs(first, twin):
    """``first`` with three columns that have a twin inside and their twins outside: what ``hide_twins`` adds"""
    have = torch.from_numpy(np.nonzero(twin >= 0)[0])
    inside = have[torch.from_numpy(twin[have.numpy()]).long() > have][:3]          # the lower column of three pairs
    first = first.clone()
    first[inside] = True
    first[torch.from_numpy(twin[inside.numpy()]).long()] = False
    return first


def _reference(a, hidden=None):
    g, ed, ei, et, arrays, _ = _world()
    rowptr, _, perm = arrays[False]
    return ref.draw(rowptr.numpy(), perm.numpy(), ei[0].numpy(), ei[1].numpy(), et.numpy(), a.numpy(), SLOPE,
                    None if hidden is None else np.asarray(hidden))


def _assert_within_bound(ed, w, bound, k):
    got = _weights(ed)
    assert torch.equal(bits(got[0]), bits(got[1])), "the two directions hold different bits for one column"
    err = np.abs(got[0].double().numpy() - w)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"attention draw: max |w - float64| = {err.max():.3e}, worst error / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"a weight is {worst:.2f} bounds away from the float64 restatement"
    assert np.array_equal(ed.kept_counts().cpu().numpy(), k)
    return got[0]


def _assert_sums_to_one(ei, et, got, bound, k):
    """every segment with a live edge sums to 1 within the sum of its edges' bounds"""
    seg = ei[1] * R + et
    total = torch.zeros(N * R, dtype=torch.float64).index_add(0, seg, got.double())
    room = torch.zeros(N * R, dtype=torch.float64).index_add(0, seg, torch.from_numpy(bound)) + 1e-12
    live = torch.from_numpy(k > 0)
    assert bool(((total - 1).abs() <= room)[live].all())


# ----------------------------------------------------------------------------------------------------------- 1. the draw
@pytest.mark.parametrize("hiding", ["none", "window", "window and twins"])
def test_the_draw_equals_the_float64_restatement_within_the_derived_bound(hiding):
    g, ed, ei, et, arrays, twin = _world()
    dev, e = g.device, ei.size(1)
    a = _scalars(2.0)
    kw, hidden = {}, None
    if hiding != "none":
        first = torch.rand(e, generator=torch.Generator().manual_seed(5)) < 0.3
        first = _with_half_pairs(first, twin)
        kw = _window(ei, first, dev)
        kw["hide_twins"] = hiding == "window and twins"
        hidden = twins_ref.hidden_mask(e, twin, 5, kw["batch"], kw["position"].cpu().numpy(), kw["hide_twins"])
        assert (hidden.sum() > first.sum()) == kw["hide_twins"]
    stats = torch.tensor([7, 9], dtype=torch.int64, device=dev)
    ed.set_attention(a.to(dev), SLOPE, stats=stats, **kw)
    w, bound, k = _reference(a, hidden)
    got = _assert_within_bound(ed, w, bound, k)
    n_hidden = 0 if hidden is None else int(hidden.sum())
    assert stats.tolist() == [7 + e - n_hidden, 9 + n_hidden]
    if hidden is not None:
        assert not got[torch.from_numpy(hidden)].any()
    _assert_sums_to_one(ei, et, got, bound, k)
    ed.set_attention(a.to(dev), SLOPE, **kw)                    # the same arguments: the same bits
    assert torch.equal(bits(got), bits(_weights(ed)[0]))


@pytest.mark.parametrize("hiding", ["none", "window", "window and twins"])
def test_zero_scalars_are_the_plain_draw_bit_for_bit(hiding):
    g, ed, ei, et, arrays, twin = _world()
    dev, e = g.device, ei.size(1)
    kw = {}
    if hiding != "none":
        first = torch.rand(e, generator=torch.Generator().manual_seed(6)) < 0.3
        first = _with_half_pairs(first, twin)
        kw = dict(_window(ei, first, dev), hide_twins=hiding == "window and twins")
    x = torch.randn(N, 8, generator=torch.Generator().manual_seed(1)).to(dev)
    ed.draw(0.0, torch.tensor([1, 2], dtype=torch.int64, device=dev), **kw)
    want = _weights(ed), ed.kept_counts().cpu(), [ops.aggregate(ed.view, x, transposed=t).cpu() for t in (False, True)]
    ed.set_attention(torch.zeros(2, N, R, device=dev), SLOPE, **kw)
    got = _weights(ed), ed.kept_counts().cpu(), [ops.aggregate(ed.view, x, transposed=t).cpu() for t in (False, True)]
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip(want[0], got[0])) and torch.equal(want[1], got[1])
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip(want[2], got[2]))    # head_w, runs and the hub tree alike


def test_a_segment_whose_edges_are_all_hidden_holds_zeros():
    g, ed, ei, et, arrays, _ = _world()
    dev = g.device
    s = _seg(8)
    first = (ei[1] * R + et) == s
    a = _scalars(2.0)
    a[0].view(-1)[s] = float("nan")                             # a hidden edge's scalars are never looked at
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    ed.set_attention(a.to(dev), SLOPE, stats=stats, **_window(ei, first, dev))
    w, bound, k = _reference(a, first.numpy())
    got = _assert_within_bound(ed, w, bound, k)
    assert int(k[s]) == 0 and not got[first].any() and not torch.isnan(got).any()
    assert stats.tolist() == [ei.size(1) - 8, 8]


def test_logits_of_plus_and_minus_200_give_finite_weights_that_sum_to_one():
    g, ed, ei, et, arrays, _ = _world()
    a = torch.where(torch.rand(2, N, R, generator=torch.Generator().manual_seed(8)) < 0.5, -100.0, 100.0).contiguous()
    ed.set_attention(a.to(g.device), SLOPE)
    w, bound, k = _reference(a)
    got = _assert_within_bound(ed, w, bound, k)
    l = ref.logits32(a.numpy(), ei[0].numpy(), ei[1].numpy(), et.numpy(), SLOPE)
    assert l.max() == 200 and l.min() == np.float32(0.2) * np.float32(-200)
    assert bool(torch.isfinite(got).all())
    _assert_sums_to_one(ei, et, got, bound, k)


def test_the_non_finite_rules():
    g, ed, ei, et, arrays, _ = _world()
    dev = g.device
    seg = ei[1] * R + et
    base = _scalars(1.0)
    ed.set_attention(base.to(dev), SLOPE)
    clean = _weights(ed)[0]
    for bad, whole_segment in ((float("nan"), True), (float("inf"), True), (float("-inf"), False)):
        a = base.clone()
        col = int(torch.nonzero(seg == _seg(257))[100])        # one edge of the 257 segment ...
        src = int(ei[0, col])
        a[1, src, 1] = bad                                      # ... through its source scalar of relation 1
        touched = torch.unique(seg[(ei[0] == src) & (et == 1)])            # every segment that source feeds in relation 1
        ed.set_attention(a.to(dev), SLOPE)
        got = _weights(ed)
        assert torch.equal(bits(got[0]), bits(got[1]))
        inside = torch.isin(seg, touched)
        assert bool(torch.isnan(got[0][inside]).all()) == whole_segment and not torch.isnan(got[0][~inside]).any()
        assert torch.equal(bits(got[0][~inside]), bits(clean[~inside]))           # no other segment is touched
        if not whole_segment:                                   # -inf beside finite logits: weight 0, the rest sums to 1
            w, bound, k = _reference(a)
            _assert_within_bound(ed, w, bound, k)
            assert got[0][col] == 0 and not torch.isnan(got[0]).any()


# ------------------------------------------------------------------------------------------------------- 2. the edge sum
@pytest.mark.parametrize("transposed", [False, True])
def test_the_edge_sum_is_exact_on_integers_and_bit_equal_on_floats(transposed, monkeypatch):
    g, ed, ei, et, arrays, _ = _world()
    dev, e = g.device, ei.size(1)
    rowptr, _, perm = arrays[transposed]
    key = (ei[0] if transposed else ei[1]) * R + et
    gen = torch.Generator().manual_seed(12)
    ints = torch.randint(-1000, 1000, (e,), generator=gen)
    want = torch.zeros(N * R, dtype=torch.int64).index_add(0, key, ints)
    nan_filled = lambda *shape, dtype, device: torch.full(shape[0] if len(shape) == 1 and not isinstance(shape[0], int)  # noqa: E731
                                                          else shape, float("nan"), dtype=dtype, device=device)
    monkeypatch.setattr(ops, "_empty", nan_filled)             # outputs pre-filled with NaN come back fully written
    for graph in (g, ed.view):                                  # weights are not read: any structure
        got = ops.edge_segment_sum(graph, ints.float().to(dev), transposed=transposed).cpu()
        assert tuple(got.shape) == (N, R) and torch.equal(got.view(-1).long(), want) and not torch.isnan(got).any()
        assert not torch.signbit(got.view(-1)[want == 0]).any()                   # +0.0 where nothing is summed
    vals = torch.randn(e, generator=gen)
    got = ops.edge_segment_sum(g, vals.to(dev), transposed=transposed).cpu().view(-1)
    restated = torch.from_numpy(ref.edge_sum(rowptr.numpy(), perm.numpy(), vals.numpy()))
    assert torch.equal(bits(got), bits(restated))
    again = ops.edge_segment_sum(g, vals.to(dev), transposed=transposed).cpu().view(-1)
    assert torch.equal(bits(got), bits(again))
    vals[int(perm[rowptr[key.max()]])] = float("inf")           # a non-finite value reaches exactly its own segment
    bad = ops.edge_segment_sum(g, vals.to(dev), transposed=transposed).cpu().view(-1)
    assert int((bits(bad) != bits(got)).sum()) == 1 and bool(torch.isinf(bad[key.max()]))
    with pytest.raises(ValueError):
        ops.edge_segment_sum(g, vals[:-1].to(dev))
    with pytest.raises(TypeError):
        ops.edge_segment_sum(g, vals.double().to(dev))


# ------------------------------------------------------------------------------------------------------------ 3. the layer
D_IN, D_OUT = 16, 12


def _layer(dev, seed=21, scale=0.0):
    torch.manual_seed(seed)
    layer = RelationalAttentionConv(D_IN, D_OUT, R).to(dev)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        layer.bias.copy_(0.1 * torch.randn(D_OUT, generator=gen))
        layer.att_dst.copy_(scale * torch.randn(R, D_IN, generator=gen))
        layer.att_src.copy_(scale * torch.randn(R, D_IN, generator=gen))
    x = (0.5 * torch.randn(N, D_IN, generator=gen)).to(dev).requires_grad_(True)
    cot = torch.randn(N, D_OUT, generator=gen).to(dev)
    return layer, x, cot


@pytest.mark.parametrize("activation", [None, "relu"])
def test_zero_attention_is_the_mean_layer_over_a_plain_draw(activation):
    """output and the gradients in x, weight, root and bias are EQUAL (``torch.equal``) to ``rgcn_conv(..., graph=view)``
    after ``draw(p=0)``: the same kernels over the same weights.  (The input gradient receives ``da @ att`` on top, a
    sum of exact zeros here.)"""
    g, ed, ei, et, arrays, _ = _world()
    dev = g.device
    layer, x, cot = _layer(dev)
    eid, etd = ei.to(dev), et.to(dev)
    out = layer(x, eid, etd, activation=activation, graph=g)
    out.backward(cot)
    got = [out.detach(), x.grad, layer.weight.grad, layer.root.grad, layer.bias.grad]
    assert float(layer.att_src.grad.abs().max()) > 0
    ed.draw(0.0, torch.tensor([1, 2], dtype=torch.int64, device=dev))
    x2 = x.detach().clone().requires_grad_(True)
    params = [p.detach().clone().requires_grad_(True) for p in (layer.weight, layer.root, layer.bias)]
    want = rgcn_conv(x2, eid, etd, *params, R, activation, graph=ed.view)
    want.backward(cot)
    for name, a, b in zip(("out", "gx", "gW", "groot", "gb"), got, [want.detach(), x2.grad] + [p.grad for p in params]):
        assert torch.equal(a, b), name


def test_random_attention_against_float64():
    """Forward, gx, gW, groot, gb under the gates ``test_gpu_parity.py`` applies to ``RGCNConv``.  The gradients of the
    attention vectors: the distance of a float32 CPU torch restatement from float64 on the same inputs, times 8 for the
    other summation order, relative to the gradient's largest entry.  Measured on an MI355X (this graph, seed 21):
    the float32 restatement is 8.60e-7 (att_dst) and 2.11e-7 (att_src) from float64, so the gates are 6.88e-6 and
    1.69e-6; the layer is 1.60e-7 and 1.12e-7 away."""
    g, ed, ei, et, arrays, _ = _world()
    dev = g.device
    layer, x, cot = _layer(dev, scale=0.3)
    first = torch.rand(ei.size(1), generator=torch.Generator().manual_seed(9)) < 0.2
    out = layer(x, ei.to(dev), et.to(dev), activation="relu", graph=g, window=_window(ei, first, dev))
    out.backward(cot)
    names = ("weight", "root", "bias", "att_dst", "att_src")

    def restated(dtype):
        p = [getattr(layer, k).detach().cpu().to(dtype).requires_grad_(True) for k in names]
        xr = x.detach().cpu().to(dtype).requires_grad_(True)
        o = ref.layer(xr, p[0], p[1], p[2], p[3], p[4], ei, et, SLOPE, first, relu=True)
        o.backward(cot.cpu().to(dtype))
        return o.detach(), xr.grad, {k: t.grad for k, t in zip(names, p)}

    o64, gx64, g64 = restated(torch.float64)
    _, _, g32 = restated(torch.float32)
    assert_fwd(out.detach(), o64)
    assert_grad(x.grad, gx64)
    for k in ("weight", "root", "bias"):
        assert_grad(getattr(layer, k).grad, g64[k])
    for k in ("att_dst", "att_src"):
        dist = rel_err(g32[k], g64[k])
        gate = 8 * dist
        err = rel_err(getattr(layer, k).grad, g64[k])
        print(f"d {k}: float32 restatement is {dist:.3e} from float64 -> gate {gate:.3e}; the layer is {err:.3e} away")
        assert float(g64[k].abs().max()) > 0 and err <= gate, f"d {k}: {err:.3e} > {gate:.3e}"


# ---------------------------------------------------------------------------------------------------------- 4. the trainer
def test_five_trainer_steps_match_the_float64_restatement_on_the_same_batches(tmp_path):
    """Five Adam steps (clip 1.0, dropout 0) with ``--attention --hide_batch_edges`` against the float64 restatement fed
    the recorded batches and hiding the same columns; per-step loss and the parameters afterwards inside the gates
    ``test_train.py::test_trainer_steps_match_oracle_on_the_same_batches`` holds the mean model to (2e-5 relative on the
    loss, 5e-5 on every parameter).  ``att_src`` has left zero after the first step; ``att_dst`` has no gradient at
    that point (a constant per segment under one slope: the softmax does not see it) and follows from step 2 on.
    Measured: losses agree to 1e-7, parameters to 7.8e-7, ``conv1.att_dst`` to 1.8e-5 - Adam divides the first step's
    rounding-level gradient of that parameter by its own size."""
    from oracle import rgcn_oracle as O
    dev = need_gpu()
    torch.manual_seed(0)
    n, r, bsz = 400, 3, 256
    gen = torch.Generator().manual_seed(3)
    ei, et = torch.randint(0, n, (2, 6000), generator=gen), torch.randint(0, r, (6000,), generator=gen)
    data = {"edge_index": ei, "edge_type": et, "num_nodes": n, "num_relations": r}
    args = T.parse_args(["--attention", "--hide_batch_edges"])
    for k, v in dict(dropout=0.0, decoder_dropout=0.0, batch_size=bsz, output_dir=str(tmp_path), device="cuda").items():
        setattr(args, k, v)
    model = T.create_model(n, r, args)
    ref_state = {k: v.clone().double() for k, v in model.state_dict().items()}
    trainer = T.Trainer(model, data, data, data, dev, args)
    assert not trainer.use_hip_graph and trainer._edge_dropout is None
    log, after_first = [], {}

    def on_step(h, t, rl, lb, loss):
        if not log:
            after_first.update({k: v.detach().cpu().clone() for k, v in trainer.model.state_dict().items() if "att_" in k})
        log.append((h.cpu(), t.cpu(), rl.cpu(), lb.cpu(), loss.item()))

    trainer.train_epoch(on_step=on_step, max_steps=5)
    assert len(log) == 5 and trainer.edge_dropout_stats == (5 * (6000 - bsz), 5 * bsz)
    assert all(float(after_first[f"encoder.conv{i}.att_src"].abs().max()) > 0 for i in (1, 2))
    order = trainer._order.cpu()
    params = {k: v.clone().requires_grad_(True) for k, v in ref_state.items()}
    opt = torch.optim.Adam(list(params.values()), lr=args.lr)
    conv = lambda i: {k: params[f"encoder.conv{i}.{k}"] for k in ("weight", "root", "bias", "att_dst", "att_src")}   # noqa: E731
    for step, (h, t, rl, lb, loss_gpu) in enumerate(log):
        hidden = torch.zeros(6000, dtype=torch.bool)
        hidden[order[step * bsz:(step + 1) * bsz]] = True
        assert torch.equal(h[:bsz], ei[0, order[step * bsz:(step + 1) * bsz]])
        emb = ref.encoder(params["encoder.node_embeddings.weight"], conv(1), conv(2), ei, et, args.attention_slope, hidden)
        scores = O.distmult_ref(emb[h], emb[t], params["decoder.relation_embeddings.weight"][rl])
        loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, lb.double())
        print(f"step {step}: loss {loss_gpu:.7f}, float64 {loss.item():.7f}")
        assert abs(loss.item() - loss_gpu) <= 2e-5 * max(1.0, abs(loss.item()))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(params.values()), args.grad_clip)
        opt.step()
    for k, v in trainer.model.state_dict().items():
        err = (v.cpu().double() - params[k].detach()).abs().max().item()
        print(f"{k}: max |parameter - float64| = {err:.3e}")
        assert err <= 5e-5, k
    assert all(float(trainer.model.state_dict()[f"encoder.conv{i}.att_{s}"].abs().max()) > 0 for i in (1, 2) for s in ("dst", "src"))
    # validation draws over the full graph without the train graph's window, and the checkpoint carries the flag
    trainer.validate()
    assert trainer.model.encoder.attention_window is None
    path = trainer.save_checkpoint(1)
    from primekg_rgcn_linkprediction_amd import evaluate
    loaded, _ = evaluate.load_model(str(path), dev)
    assert loaded.encoder.attention and torch.equal(loaded.encoder.conv1.att_src, trainer.model.encoder.conv1.att_src)


# ------------------------------------------------------------------------------------------------------ 5. the planted toy
def test_the_planted_toy_finds_the_informative_edge():
    """Every target has one informative in-neighbour among 16; after TOY_STEPS seeded Adam steps its weight exceeds 0.5
    in at least 90 % of the segments (it starts at 1 / 16).  The float64 restatement reaches 100 % after two thirds of
    the steps (``test_attention_host.py``): a third of the steps and 10 % of the segments are the margin."""
    dev = need_gpu()
    x, ei, et, informative, want = planted_toy()
    layer = RelationalAttentionConv(x.size(1), x.size(1), 1, root_weight=False, bias=False).to(dev)
    with torch.no_grad():
        layer.weight.copy_(toy_parameters(x.size(1), torch.float32)["weight"])
    xd, eid, etd, wantd = x.float().to(dev), ei.to(dev), et.to(dev), want.float().to(dev)
    graph = ops.bucket(eid, etd, x.size(0), 1)
    views = layer.views_of(graph)

    def informative_weights():
        with torch.no_grad():
            layer(xd, eid, etd)
        _, _, perm, val = views.dropout.view.arrays(False)
        w = torch.empty_like(val)
        w[perm] = val
        return w.cpu()[informative]

    assert bool((informative_weights() == 1 / 16).all())
    opt = torch.optim.Adam(layer.parameters(), lr=TOY_LR)
    for _ in range(TOY_STEPS):
        opt.zero_grad()
        (layer(xd, eid, etd)[:want.size(0)] - wantd).square().sum().backward()
        opt.step()
    w = informative_weights()
    share = float((w > 0.5).float().mean())
    print(f"planted toy: informative weight > 0.5 in {share:.3f} of the segments, smallest {float(w.min()):.3f}")
    assert share >= 0.9
