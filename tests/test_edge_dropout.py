"""GPU tier of edge dropout and hidden batch edges: the draw (``rgcn_edge_dropout_draw``) bit for bit against its host
restatement (``edge_dropout_reference.py``), the gathers, the layer and the two-layer encoder over the view against the
oracle on the kept subgraph at the gates of ``test_gpu_parity.py``, redraws on the SAME view (a stale copy of the
weights anywhere would show), capture / replay at a moved cursor, and five trainer steps against the oracle model."""
import ctypes

import numpy as np
import pytest
import torch

import edge_dropout_reference as R
from c_surface import _Graph
from conftest import need_gpu
from oracle import rgcn_oracle as O
from primekg_rgcn_linkprediction_amd import RGCNConv, _lib, conv as C, ops, rgcn_encoder2, train as T
from test_gpu_parity import assert_fwd, assert_grad

pytestmark = pytest.mark.gpu

N, NR_REL, HEAD = 70, 3, 8          # RGCN_HEAD = 8 (csrc/rgcn_common.h)
LOSS_RTOL, PARAM_ATOL = 2e-5, 5e-5  # the gates of tests/test_train.py::test_trainer_steps_match_oracle_on_the_same_batches
SEED, EPOCH = (0x1234 << 32) | 0x9ABCDEF1, 3


def _graph():
    """70 nodes (past two 32-row tiles, past one 64-row tile), 3 relations, ~900 edges: a forward segment of 300 edges
    (past 256: a pack AND partial rows in the workspace), one of 65 (just past a run), one of exactly RGCN_HEAD and one
    of RGCN_HEAD + 1, a source hub of 300 out-edges, duplicates, self loops; node 69 has no in-edge at all and most
    (node, relation) segments of nodes 0 .. 9 are empty"""
    gen = torch.Generator().manual_seed(11)
    rnd = lambda lo, hi, k: torch.randint(lo, hi, (k,), generator=gen)     # noqa: E731
    parts = [(rnd(0, N, 300), torch.full((300,), 5), torch.full((300,), 1)),
             (rnd(0, N, 65), torch.full((65,), 6), torch.full((65,), 0)),
             (rnd(0, N, HEAD), torch.full((HEAD,), 7), torch.full((HEAD,), 2)),
             (rnd(0, N, HEAD + 1), torch.full((HEAD + 1,), 8), torch.full((HEAD + 1,), 2)),
             (torch.full((300,), 9), rnd(10, 69, 300), torch.full((300,), 0)),              # the source hub
             (rnd(0, N, 200), rnd(10, 69, 200), rnd(0, NR_REL, 200))]
    src, dst, rel = (torch.cat([p[i] for p in parts]) for i in range(3))
    loops = rnd(10, 69, 10)
    src, dst, rel = torch.cat([src, loops, src[-8:]]), torch.cat([dst, loops, dst[-8:]]), torch.cat([rel, rnd(0, NR_REL, 10), rel[-8:]])
    shuffle = torch.randperm(src.numel(), generator=gen)
    ei, et = torch.stack([src, dst])[:, shuffle].contiguous(), rel[shuffle].contiguous()
    seg = torch.bincount(ei[1] * NR_REL + et, minlength=N * NR_REL)
    assert (seg[5 * 3 + 1], seg[6 * 3 + 0], seg[7 * 3 + 2], seg[8 * 3 + 2]) == (300, 65, HEAD, HEAD + 1)
    assert int(torch.bincount(ei[0] * NR_REL + et, minlength=N * NR_REL)[9 * 3 + 0]) >= 300 and int((seg == 0).sum()) > 10
    return ei, et


@pytest.fixture(scope="module")
def world():
    dev = need_gpu()
    ei, et = _graph()
    e = ei.size(1)
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), N, NR_REL)
    assert g.num_levels(False) == 2 and g.workspace_bytes(False, 64) > 0 and g.num_levels(True) == 2
    order = torch.randperm(e, generator=torch.Generator().manual_seed(5))
    position = torch.empty(e, dtype=torch.int64)
    position[order] = torch.arange(e)
    ed = ops.EdgeDropout(g)
    w = dict(dev=dev, ei=ei, et=et, e=e, g=g, ed=ed, order=order, position=position, position_dev=position.to(dev),
             rng=torch.tensor([SEED, EPOCH], dtype=torch.int64, device=dev))
    yield w
    ed.destroy()
    g.destroy()


def _draw(w, p, c0=0, batch=0, hide=False, stats=None):
    """one draw on the device and its restatement -> (kept, hidden) by original column"""
    cursor = torch.tensor([c0], dtype=torch.int64, device=w["dev"])
    w["ed"].draw(p, w["rng"], cursor=cursor, batch=batch if hide else 0, position=w["position_dev"] if hide else None, stats=stats)
    return R.kept_mask(w["e"], p, SEED, EPOCH, c0, batch if hide else 0, w["position"].numpy() if hide else None)


def _device_copy(dev, ptr, count, what):
    """``count`` float32 (what = "val") or int64 (what = "perm") words at the raw device address ``ptr``, copied by the
    library itself: rgcn_graph_export of a host-side handle whose one array is that address"""
    fake = _Graph(E=count, N=1, R=1)
    c = fake.dir[0]
    c.rowptr, c.weighted, c.n_key = ptr, True, 1
    out = torch.empty(count, dtype=torch.float32 if what == "val" else torch.int64, device=dev)
    if what == "val":
        c.val = ptr
        rc = _lib.load().rgcn_graph_export(ctypes.addressof(fake), 0, None, None, None, out.data_ptr(), None)
    else:
        c.perm = ptr
        rc = _lib.load().rgcn_graph_export(ctypes.addressof(fake), 0, None, None, out.data_ptr(), None, None)
    assert rc == _lib.RGCN_OK
    torch.cuda.synchronize()
    return out


def _heads(w, transposed):
    """(head_w of the view as the device holds it, what k_item_heads' rule makes of the view's current val)"""
    view = w["ed"].view
    c = _Graph.from_address(view.handle.value).dir[int(transposed)]
    n0 = c.num_items[0]
    assert n0 > 0 and c.weighted and c.head_w
    got = _device_copy(w["dev"], c.head_w, n0 * HEAD, "val").cpu().numpy()
    items = _device_copy(w["dev"], c.items[0], 2 * n0, "perm").cpu().numpy().view(np.int32).reshape(n0, 4)
    val = view.arrays(transposed)[3].cpu().numpy()
    e = items[:, 0:1] + np.arange(HEAD)[None, :]
    ok = e < items[:, 1:2]
    want = np.where(ok, val[np.minimum(e, len(val) - 1)], np.float32(0)).astype(np.float32).reshape(-1)
    return got, want


def _assert_draw_bits(w, kept):
    ei, et = w["ei"].numpy(), w["et"].numpy()
    view = w["ed"].view
    assert np.array_equal(w["ed"].kept_counts().cpu().numpy(), R.kept_counts(ei, et, kept, N, NR_REL))
    w_col = R.weights(ei, et, kept, N, NR_REL)
    for transposed in (False, True):
        rowptr, col, perm, val = (t.cpu().numpy() for t in view.arrays(transposed))
        assert val.dtype == np.float32 and val.shape == (w["e"],)
        assert np.array_equal(val.view(np.int32), R.bucketed(w_col, perm).view(np.int32)), f"val, transposed={transposed}"
        got, want = _heads(w, transposed)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"head_w, transposed={transposed}"
    return w_col


# ----------------------------------------------------------------------------------------------- 1. the draw, bit for bit
@pytest.mark.parametrize("p", [0.0, 0.4, 0.9])
@pytest.mark.parametrize("window", ["off", "inside", "clipped"])
def test_draw_equals_the_restatement_bit_for_bit(world, p, window):
    w = world
    c0, batch = {"off": (0, 0), "inside": (128, 100), "clipped": (w["e"] - 37, 100)}[window]
    stats = torch.tensor([5, 7], dtype=torch.int64, device=w["dev"])           # accumulated, never cleared
    kept, hidden = _draw(w, p, c0, batch, hide=window != "off", stats=stats)
    assert int(hidden.sum()) == {"off": 0, "inside": 100, "clipped": 37}[window]
    w_col = _assert_draw_bits(w, kept)
    assert stats.tolist() == [5 + int(kept.sum()), 7 + int(hidden.sum())]
    if window != "off":                                                         # the batch's own columns: weight 0 both ways
        cols = w["order"][c0:c0 + batch].numpy()
        assert bool((w_col[cols] == 0).all())
        for transposed in (False, True):
            _, _, perm, val = (t.cpu().numpy() for t in w["ed"].view.arrays(transposed))
            assert bool((val[np.isin(perm, cols)] == 0).all())
    if p == 0.9:
        assert int((R.kept_counts(w["ei"].numpy(), w["et"].numpy(), kept, N, NR_REL) == 0).sum()) > 0


def test_draw_refuses_what_the_header_refuses(world):
    w = world
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            w["ed"].draw(bad, w["rng"])
        rc = _lib.load().rgcn_edge_dropout_draw(w["ed"].handle, bad, w["rng"].data_ptr(), None, 0, None, None, None)
        assert rc == _lib.RGCN_ERR_ARG
    lib = _lib.load()
    assert lib.rgcn_edge_dropout_draw(w["ed"].handle, 0.5, None, None, 0, None, None, None) == _lib.RGCN_ERR_ARG
    assert lib.rgcn_edge_dropout_draw(w["ed"].handle, 0.5, w["rng"].data_ptr(), None, -1, None, None, None) == _lib.RGCN_ERR_ARG
    assert lib.rgcn_edge_dropout_draw(w["ed"].handle, 0.5, w["rng"].data_ptr() + 4, None, 0, None, None, None) == _lib.RGCN_ERR_ALIGN
    out = ctypes.c_void_p()
    assert lib.rgcn_edge_dropout_create(w["ed"].view.handle, None, ctypes.byref(out)) == _lib.RGCN_ERR_UNSUPPORTED   # a view of a view
    with pytest.raises(ValueError):
        ops.EdgeDropout(w["ed"].view)
    with pytest.raises(ValueError):
        w["ed"].draw(0.5, w["rng"], position=w["position_dev"][:-1], batch=4)


def test_view_refuses_every_copy_of_its_weights(world, tmp_path):
    view = world["ed"].view
    assert view.edge_dropout and view.weighted_shard and not view.bipartite and not world["g"].edge_dropout
    for call in (view.merged_transposed, view.fused_plan, lambda: view.fused_plan(16, True), view.state,
                 lambda: view.save(tmp_path / "v.pt"), lambda: view.row_blocks(32)):
        with pytest.raises(ValueError, match="stale|copies"):
            call()
    # the bounds hold for every draw: forward 1 + 1e-6, transposed the longest (source, relation) segment
    longest = int(torch.bincount(world["ei"][0] * NR_REL + world["et"], minlength=N * NR_REL).max())
    assert view.weight_bound(True) == float(longest) and 1.0 < view.weight_bound(False) <= 1.0 + 2e-6
    assert view.tile_mask_ptr(False) == world["g"].tile_mask_ptr(False) and view.row_mask_ptr(True) == world["g"].row_mask_ptr(True)


# ----------------------------------------------------------------------------------------------- 2. p = 0: the parent
def test_no_dropout_is_the_parent_graph(world):
    w = world
    dev, g, view = w["dev"], w["g"], w["ed"].view
    kept, _ = _draw(w, 0.0)
    assert kept.all()
    assert torch.equal(view.arrays(True)[3], g.arrays(True)[3])                # w_t, bit for bit
    gen = torch.Generator().manual_seed(1)
    for d in (64, 128):
        x = torch.randn(N, d, generator=gen)
        assert torch.equal(ops.aggregate(view, x.to(dev), transposed=True), ops.aggregate(g, x.to(dev), transposed=True))
        got = ops.aggregate(view, x.to(dev)).cpu().double().numpy()
        w_col = R.weights(w["ei"].numpy(), w["et"].numpy(), kept, N, NR_REL)
        want, mag = R.aggregate_f64(x.numpy(), w["ei"].numpy(), w["et"].numpy(), w_col, N, NR_REL)
        # a segment of n <= 300 terms, each one product and one addition (or one fma) in float32, summed in any order:
        # |error| <= gamma_(n + 2) * sum |w x|, gamma_k = k u / (1 - k u), u = 2^-24
        k, u = 300 + 2, 2.0 ** -24
        assert bool((np.abs(got - want) <= k * u / (1 - k * u) * mag).all())


# ----------------------------------------------------------------------------------------------- 3 + 4. against the oracle
def _oracle_checks(w, kept, convs, emb, wide, cot):
    dev, view = w["dev"], w["ed"].view
    ek, tk = (torch.from_numpy(a) for a in R.kept_subgraph(w["ei"].numpy(), w["et"].numpy(), kept))
    eid, etd = w["ei"].to(dev), w["et"].to(dev)
    # both aggregates: the mean over the kept in-edges and its adjoint
    cnt = O._segment_counts(ek, tk, N, NR_REL, torch.float64)
    x = emb.double()
    assert_fwd(ops.aggregate(view, emb.to(dev)), O._mean_agg(x, ek, tk, N, NR_REL, cnt))
    assert_fwd(ops.aggregate(view, emb.to(dev), transposed=True), O._mean_agg_transposed(x, ek, tk, N, NR_REL, cnt))
    # the single layer, forward and every gradient: 64 -> 128 on the table, 128 -> 128 on a table of that width
    for c0, table in ((convs[0], emb), (convs[1], wide)):
        c0.zero_grad(set_to_none=True)
        xg = table.to(dev).requires_grad_(True)
        out = c0(xg, eid, etd, graph=view)
        (out * cot[0].to(dev)).sum().backward()
        ref = {k: v.detach().cpu().double().requires_grad_(True) for k, v in c0.named_parameters()}
        xr = table.double().requires_grad_(True)
        out_ref = O.rgcn_conv_ref(xr, ek, tk, ref["weight"], ref["root"], ref["bias"])
        (out_ref * cot[0].double()).sum().backward()
        assert_fwd(out, out_ref.detach())
        assert_grad(xg.grad, xr.grad)
        for k, v in c0.named_parameters():
            assert_grad(v.grad, ref[k].grad)
    # the two-layer encoder in training mode, dropout 0, with the device's own ReLU decisions
    for c in convs:
        c.zero_grad(set_to_none=True)
    mask = (convs[0](emb.to(dev).requires_grad_(True), eid, etd, activation="relu", graph=view).detach() > 0).cpu()
    eg = emb.to(dev).requires_grad_(True)
    out = rgcn_encoder2(eg, eid, etd, convs[0], convs[1], graph=view)
    (out * cot[1].to(dev)).sum().backward()
    p64 = [{k: v.detach().cpu() for k, v in c.named_parameters()} for c in convs]
    f64 = O.encoder_explicit_f64(emb, p64[0], p64[1], ek, tk, cot[1], relu_mask=mask)
    assert_fwd(out, f64["out"])
    assert_grad(eg.grad, f64["grads"]["emb"])
    for name, c in zip(("conv1", "conv2"), convs):
        for k, v in c.named_parameters():
            assert_grad(v.grad, f64["grads"][f"{name}.{k}"])
    return out.detach().clone(), eg.grad.clone()


def test_layer_and_encoder_over_redrawn_views_match_the_oracle_on_the_kept_subgraph(world):
    """64 -> 128 (where transform-first would have fired) and 128 -> 128, FIVE draws on the SAME view: the third run of a
    pass records it, so the fourth and fifth are replayed natively, and anything that had copied the weights out of the
    view - the merged structure, a fused plan, a recorded address - would still hold an earlier draw's"""
    w = world
    dev = w["dev"]
    torch.manual_seed(4)
    emb = torch.nn.init.xavier_uniform_(torch.empty(N, 64))
    convs = [RGCNConv(64, 128, NR_REL).to(dev), RGCNConv(128, 128, NR_REL).to(dev)]
    for c in convs:
        c.bias.data.uniform_(-0.1, 0.1)
    cot = (torch.randn(N, 128), torch.randn(N, 128))
    wide = torch.randn(N, 128) * 0.1                      # the input of the 128 -> 128 layer taken by itself
    images = object()                          # "the step's split images exist": all the policy asks of them
    if ops.GEMM_PRECISION == "split":
        assert C._transform_first(w["g"], convs[0].weight, convs[0].root, images, None)       # the parent takes it at 64 -> 128
    assert not C._transform_first(w["ed"].view, convs[0].weight, convs[0].root, images, None)
    assert not C._defer_hubs(False, images, images, 64, 128, w["ed"].view) and not C._train_fused(w["ed"].view, N, NR_REL, 64, 128, False)
    seen = []
    for c0, p, hide in ((0, 0.4, False), (128, 0.4, True), (256, 0.4, True), (w["e"] - 50, 0.4, True), (384, 0.9, True)):
        kept, hidden = _draw(w, p, c0, 128, hide=hide)
        seen.append(kept)
        if hide:
            assert hidden.any() and not kept[w["order"][c0:c0 + 128].numpy()].any()
        _oracle_checks(w, kept, convs, emb, wide, cot)
    assert all((a != b).any() for a, b in zip(seen, seen[1:]))                     # another cursor, another kept set
    assert not hasattr(w["ed"].view, "_merged") and "_fused_plans" not in w["ed"].view.__dict__
    # eval mode and no_grad without dropout: always the parent graph, whatever the view holds
    eid, etd = w["ei"].to(dev), w["et"].to(dev)
    with torch.no_grad():
        assert torch.equal(rgcn_encoder2(emb.to(dev), eid, etd, convs[0], convs[1], graph=w["ed"].view),
                           rgcn_encoder2(emb.to(dev), eid, etd, convs[0], convs[1]))
    convs[0].eval()
    x = emb.to(dev).requires_grad_(True)
    assert torch.equal(convs[0](x, eid, etd, graph=w["ed"].view), convs[0](x, eid, etd))


# ----------------------------------------------------------------------------------------------- 5. determinism, capture
def test_same_seed_epoch_cursor_same_bits_and_a_replay_draws_at_the_moved_cursor(world):
    w = world
    dev, ed, view = w["dev"], w["ed"], w["ed"].view
    torch.manual_seed(6)
    emb = torch.nn.init.xavier_uniform_(torch.empty(N, 64)).to(dev)
    convs = [RGCNConv(64, 128, NR_REL).to(dev), RGCNConv(128, 128, NR_REL).to(dev)]
    cot = torch.randn(N, 128, device=dev)
    eid, etd = w["ei"].to(dev), w["et"].to(dev)
    cursor = torch.zeros(1, dtype=torch.int64, device=dev)
    x = emb.clone().requires_grad_(True)
    params = [x] + [p for c in convs for p in c.parameters()]

    def step():
        ed.draw(0.4, w["rng"], cursor=cursor, batch=128, position=w["position_dev"])
        out = rgcn_encoder2(x, eid, etd, convs[0], convs[1], graph=view)
        (out * cot).sum().backward()
        return out

    def eager(c0):
        cursor.fill_(c0)
        for p in params:
            p.grad = None
        out = step()
        return [out.detach().clone(), view.arrays(False)[3], view.arrays(True)[3], ed.kept_counts()] + [p.grad.clone() for p in params]

    a, b, a2 = eager(128), eager(512), eager(128)
    assert all(torch.equal(u, v) for u, v in zip(a, a2))                         # same (seed, epoch, cursor): same bits
    assert not torch.equal(a[1], b[1]) and not torch.equal(a[0], b[0])
    # capture at cursor 128, replay at 512: the replay equals the eager run at 512 bit for bit
    cursor.fill_(128)
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    cursor.fill_(512)
    graph.replay()
    torch.cuda.synchronize()
    got = [out.detach(), view.arrays(False)[3], view.arrays(True)[3], ed.kept_counts()] + [p.grad for p in params]
    for i, (u, v) in enumerate(zip(got, b)):
        assert torch.equal(u, v), f"replayed output {i} differs from the eager run at the same cursor"


# ----------------------------------------------------------------------------------------------- 6. the trainer
@pytest.mark.parametrize("hip_graph", [False, True])
def test_trainer_steps_with_both_flags_match_the_oracle_on_the_kept_subgraphs(world, tmp_path, hip_graph):
    """``test_trainer_steps_match_oracle_on_the_same_batches`` (tests/test_train.py) with --edge_dropout 0.4
    --hide_batch_edges: the oracle replays the recorded batches over the subgraph the restatement says each step kept.
    Its gates: per-step loss within 2e-5 relative to max(1, |loss|), parameters within 5e-5 after five Adam steps.
    (Literals in that test's body, not names it exports, and existing test files stay as they are: LOSS_RTOL / PARAM_ATOL
    below are COPIES - whoever moves the gates there moves them here.)"""
    dev = world["dev"]
    torch.manual_seed(0)
    ei, et, e = world["ei"], world["et"], world["e"]
    data = {"edge_index": ei, "edge_type": et, "num_nodes": N, "num_relations": NR_REL}
    args = T.parse_args([])
    for k, v in dict(dropout=0.0, decoder_dropout=0.0, batch_size=128, output_dir=str(tmp_path), device="cuda",
                     no_hip_graph=not hip_graph, edge_dropout=0.4, hide_batch_edges=True).items():
        setattr(args, k, v)
    model = T.create_model(N, NR_REL, args)
    ref_state = {k: v.clone() for k, v in model.state_dict().items()}
    trainer = T.Trainer(model, data, data, data, dev, args)
    log = []
    trainer.train_epoch(on_step=lambda h, t, rl, lb, loss: log.append((h.cpu(), t.cpu(), rl.cpu(), lb.cpu(), loss.item())),
                        max_steps=5)
    assert (trainer._graph is not None) == hip_graph and len(log) == 5
    seed, epoch = (int(v) for v in trainer._rng.tolist())
    order = trainer._order.cpu()
    position = torch.empty(e, dtype=torch.int64)
    position[order] = torch.arange(e)
    assert torch.equal(trainer._ed_position.cpu(), position)
    params = {k: v.clone().requires_grad_(True) for k, v in ref_state.items()}
    opt = torch.optim.Adam(list(params.values()), lr=args.lr)
    conv = lambda i: {k: params[f"encoder.conv{i}.{k}"] for k in ("weight", "root", "bias")}   # noqa: E731
    kept_total = hidden_total = 0
    for step, (h, t, rl, lb, loss_gpu) in enumerate(log):
        c0 = step * 128
        assert torch.equal(h[:128], ei[0, order[c0:c0 + 128]]) and torch.equal(t[:128], ei[1, order[c0:c0 + 128]])
        kept, hidden = R.kept_mask(e, 0.4, seed, epoch, c0, 128, position.numpy())
        kept_total, hidden_total = kept_total + int(kept.sum()), hidden_total + int(hidden.sum())
        ek, tk = (torch.from_numpy(a) for a in R.kept_subgraph(ei.numpy(), et.numpy(), kept))
        emb = O.encoder_ref(params["encoder.node_embeddings.weight"], conv(1), conv(2), ek, tk)
        scores = O.distmult_ref(emb[h], emb[t], params["decoder.relation_embeddings.weight"][rl])
        loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, lb)
        assert abs(loss.item() - loss_gpu) <= LOSS_RTOL * max(1.0, abs(loss.item())), step
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(params.values()), args.grad_clip)
        opt.step()
    for k, v in trainer.model.state_dict().items():
        assert (v.cpu() - params[k].detach()).abs().max().item() <= PARAM_ATOL, k
    assert trainer.edge_dropout_stats == (kept_total, hidden_total) and hidden_total == 5 * 128
    # validation scores over the UNDROPPED full graph: the bits a trainer without the flags gives the same parameters
    # (validate() draws its negatives from torch's generator: the same seed before either call)
    args_plain = T.parse_args([])
    for k, v in dict(dropout=0.0, decoder_dropout=0.0, batch_size=128, output_dir=str(tmp_path), device="cuda",
                     no_hip_graph=True).items():
        setattr(args_plain, k, v)
    twin = T.create_model(N, NR_REL, args_plain)
    twin.load_state_dict(trainer.model.state_dict())
    plain = T.Trainer(twin, data, data, data, dev, args_plain)
    torch.manual_seed(123)
    va = trainer.validate()
    torch.manual_seed(123)
    assert plain.validate() == va and np.isfinite(va[0])
    # and the encoder the trainer holds, in eval mode, ignores the view outright
    trainer.model.eval()
    with torch.no_grad():
        eid, etd = ei.to(dev), et.to(dev)
        assert torch.equal(trainer.model.encoder(eid, etd, graph=trainer._edge_dropout.view), trainer.model.encoder(eid, etd))


def test_replayed_epochs_equal_eager_epochs_bit_for_bit(tmp_path):
    """Two epochs (20 steps, then a whole one with its ragged last batch) with both flags, the step replayed from its HIP
    graph back to back with nothing synchronising in between, against the same steps launched eagerly: the same bits in
    every parameter, the same losses, the same kept / hidden totals.  A draw that carried a memset node did not pass
    this: replayed back to back, the step behaved as if the node ran ahead of the previous replay and the second epoch trained on other
    weights, a little differently every run.  The draw is three kernels since."""
    dev = need_gpu()
    tr, va, full, _ = T.synthetic_data(num_edges=60000, seed=2)
    runs = []
    for no_graph in (True, False, False):
        torch.manual_seed(7)
        args = T.parse_args(["--output_dir", str(tmp_path), "--dropout", "0.0", "--edge_dropout", "0.4", "--hide_batch_edges"]
                            + (["--no_hip_graph"] if no_graph else []))
        trainer = T.Trainer(T.create_model(tr["num_nodes"], 3, args), tr, va, full, dev, args)
        first = trainer.train_epoch(max_steps=20)
        second = trainer.train_epoch()
        assert (trainer._graph is None) == no_graph
        runs.append(({k: v.clone() for k, v in trainer.model.state_dict().items()}, first, second, trainer.edge_dropout_stats))
    for other in runs[1:]:
        assert other[1:] == runs[0][1:]
        for k, v in runs[0][0].items():
            assert torch.equal(v, other[0][k]), k
