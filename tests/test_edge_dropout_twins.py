"""GPU tier of twin-aware edge dropout (``RGCN_EDGE_DROPOUT_HIDE_TWINS`` / ``RGCN_EDGE_DROPOUT_PAIRED``): the twin map
``rgcn_edge_dropout_create`` builds, entry by entry, and the draws with the option bits bit for bit against the host
restatement (``edge_dropout_twins_reference.py``); the plain draw unmoved; the gathers, the layer and the encoder over a
view whose batch pairs are hidden in BOTH directions against the oracle on the graph without them (and the same draw
without the bit against that oracle: it differs, which is the leak); capture / replay at a moved cursor; five trainer
steps with all four flags against the oracle model."""
import numpy as np
import pytest
import torch

import edge_dropout_reference as R
import edge_dropout_twins_reference as TW
from conftest import need_gpu
from oracle import rgcn_oracle as O
from primekg_rgcn_linkprediction_amd import RGCNConv, ops, rgcn_encoder2, train as T
from test_edge_dropout import _heads, _oracle_checks
from test_gpu_parity import FWD_ATOL, assert_fwd

pytestmark = pytest.mark.gpu

N, NR_REL = 70, 3                   # what test_edge_dropout.py's helpers (_oracle_checks) are written for
LOSS_RTOL, PARAM_ATOL = 2e-5, 5e-5  # the gates test_edge_dropout.py takes from tests/test_train.py (copies: see there)
SEED, EPOCH = (0x4321 << 32) | 0x1FEDCBA9, 2
DUP, DECOY = (20, 2, 30), (40, 41)  # (a, r, b): 2 copies against 3 of (b, r, a); (a, 0, b) against (b, 1, a)
OPTIONS = {"hide_twins": (True, False), "paired": (False, True), "both": (True, True)}


def _graph():
    """70 nodes, 3 relations, ~1,500 columns laid out the way the preprocessing writes pairs - a column, then its reverse
    with the same relation - and then shuffled, so that most twins stand in the other 1,024-thread workgroup of the mark:
    a forward segment of 300 edges and a source hub of 300 (and, by their reverses, a hub and a segment more), 40 random
    pairs, a triple stored twice against its reverse stored three times, (a, 0, b) / (b, 1, a) decoys, self loops and 200
    columns whose reverse is not stored"""
    gen = torch.Generator().manual_seed(12)
    rnd = lambda lo, hi, k: torch.randint(lo, hi, (k,), generator=gen)     # noqa: E731
    full = lambda k, v: torch.full((k,), v)                                # noqa: E731
    pairs = [(rnd(10, 69, 300), full(300, 5), full(300, 1)),               # (src, dst, rel): the forward segment (5, 1)
             (full(300, 9), rnd(10, 69, 300), full(300, 0)),               # the source hub 9
             (rnd(10, 40, 40), rnd(41, 69, 40), rnd(0, NR_REL, 40)),
             (full(2, DUP[0]), full(2, DUP[2]), full(2, DUP[1]))]
    src, dst, rel = (torch.cat([p[i] for p in pairs]) for i in range(3))
    src, dst, rel = (torch.stack(v, dim=1).reshape(-1) for v in ((src, dst), (dst, src), (rel, rel)))   # column, reverse, ...
    loops = rnd(10, 69, 10)
    # columns without a reverse: 200 from low to high ids in relation 2 (the pairs above never use it there but for DUP),
    # the third copy of DUP's reverse, the decoys, the loops
    lone = (rnd(0, 4, 200), rnd(60, 70, 200), full(200, 2))
    src = torch.cat([src, lone[0], full(1, DUP[2]), torch.tensor(DECOY), loops])
    dst = torch.cat([dst, lone[1], full(1, DUP[0]), torch.tensor(DECOY[::-1]), loops])
    rel = torch.cat([rel, lone[2], full(1, DUP[1]), torch.tensor([0, 1]), rnd(0, NR_REL, 10)])
    shuffle = torch.randperm(src.numel(), generator=gen)
    ei, et = torch.stack([src, dst])[:, shuffle].contiguous(), rel[shuffle].contiguous()
    seg = torch.bincount(ei[1] * NR_REL + et, minlength=N * NR_REL)
    assert int(seg[5 * 3 + 1]) >= 300 and int(torch.bincount(ei[0] * NR_REL + et, minlength=N * NR_REL)[9 * 3 + 0]) >= 300
    return ei, et


@pytest.fixture(scope="module")
def world():
    dev = need_gpu()
    ei, et = _graph()
    e = ei.size(1)
    twin = TW.twins(ei.numpy(), et.numpy())
    # the graph holds what the tests are about
    src, dst, rel = ei[0].numpy(), ei[1].numpy(), et.numpy()
    assert 1400 <= e <= 1600 and 200 <= int((twin < 0).sum()) <= 260
    assert int((np.abs(np.arange(e) // 1024 - np.maximum(twin, 0) // 1024)[twin >= 0] == 1).sum()) > 100
    few = np.nonzero((src == DUP[0]) & (rel == DUP[1]) & (dst == DUP[2]))[0]
    many = np.nonzero((src == DUP[2]) & (rel == DUP[1]) & (dst == DUP[0]))[0]
    assert few.size == 2 and many.size == 3 and twin[few].tolist() == many[:2].tolist() and twin[many[2]] == -1
    decoys = np.nonzero(((src == DECOY[0]) & (dst == DECOY[1]) & (rel == 0)) | ((src == DECOY[1]) & (dst == DECOY[0]) & (rel == 1)))[0]
    assert decoys.size == 2 and bool((twin[decoys] == -1).all()) and bool((twin[src == dst] == -1).all()) and int((src == dst).sum()) >= 10
    g = ops.BucketedGraph(ei.to(dev), et.to(dev), N, NR_REL)
    assert g.num_levels(False) == 2 and g.num_levels(True) == 2
    order = torch.randperm(e, generator=torch.Generator().manual_seed(6))
    position = torch.empty(e, dtype=torch.int64)
    position[order] = torch.arange(e)
    ed = ops.EdgeDropout(g)
    w = dict(dev=dev, ei=ei, et=et, e=e, g=g, ed=ed, twin=twin, order=order, position=position, position_dev=position.to(dev),
             rng=torch.tensor([SEED, EPOCH], dtype=torch.int64, device=dev))
    yield w
    ed.destroy()
    g.destroy()


def _draw(w, p, c0, batch, hide_twins, paired, position=None, stats=None, hide=True):
    """one draw on the device and its restatement -> (kept, hidden) by original column"""
    position = w["position"] if position is None else position
    cursor = torch.tensor([c0], dtype=torch.int64, device=w["dev"])
    w["ed"].draw(p, w["rng"], cursor=cursor, batch=batch if hide else 0, position=position.to(w["dev"]) if hide else None,
                 stats=stats, hide_twins=hide_twins and hide, paired=paired)
    return TW.kept_mask(w["e"], w["twin"], p, SEED, EPOCH, c0, batch if hide else 0, position.numpy() if hide else None,
                        hide_twins=hide_twins and hide, paired=paired)


def _assert_draw_bits(w, kept):
    ei, et = w["ei"].numpy(), w["et"].numpy()
    view = w["ed"].view
    assert np.array_equal(w["ed"].kept_counts().cpu().numpy(), R.kept_counts(ei, et, kept, N, NR_REL))
    w_col = R.weights(ei, et, kept, N, NR_REL)
    for transposed in (False, True):
        _, _, perm, val = (t.cpu().numpy() for t in view.arrays(transposed))
        assert val.dtype == np.float32 and val.shape == (w["e"],)
        assert np.array_equal(val.view(np.int32), R.bucketed(w_col, perm).view(np.int32)), f"val, transposed={transposed}"
        got, want = _heads(w, transposed)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"head_w, transposed={transposed}"
    return w_col


# ----------------------------------------------------------------------------------------------- 1. every twin entry
def test_every_twin_entry_by_a_window_of_one_column(world):
    """position = the identity, p = 0, HIDE_TWINS, a window of length 1 at every column e: the columns at weight 0 are
    exactly {e, twin[e]} of the restatement, in both directions"""
    w = world
    dev, e, ed, view = w["dev"], w["e"], w["ed"], w["ed"].view
    identity = torch.arange(e, dtype=torch.int64, device=dev)
    cursor = torch.zeros(1, dtype=torch.int64, device=dev)
    perms = [view.arrays(t)[2] for t in (False, True)]
    zero = torch.zeros(2, e, e, dtype=torch.bool, device=dev)                  # [direction, window, ORIGINAL column]
    for c in range(e):
        cursor.fill_(c)
        ed.draw(0.0, w["rng"], cursor=cursor, batch=1, position=identity, hide_twins=True)
        for t in (0, 1):
            zero[t, c, perms[t]] = view.arrays(bool(t))[3] == 0
    want = torch.eye(e, dtype=torch.bool)
    has = np.nonzero(w["twin"] >= 0)[0]
    want[torch.from_numpy(has), torch.from_numpy(w["twin"][has].astype(np.int64))] = True
    zero = zero.cpu()
    for t in (0, 1):
        bad = torch.nonzero((zero[t] != want).any(dim=1)).view(-1).tolist()
        assert not bad, (f"direction {t}: windows at columns {bad[:8]} hide "
                         f"{[torch.nonzero(zero[t, c]).view(-1).tolist() for c in bad[:8]]}, twins {w['twin'][bad[:8]].tolist()}")


# ----------------------------------------------------------------------------------------------- 2. the draw, bit for bit
def _straddling_window(w):
    """(position, order, c0, length): one pair wholly inside the window, one column at c0 - 1 whose twin is inside, one at
    c0 + length whose twin is inside - the rest of the epoch's order as the fixture drew it"""
    twin, e = w["twin"], w["e"]
    firsts = [int(c) for c in np.nonzero(twin >= 0)[0] if c < twin[c]][:3]
    a, b, c = ((f, int(twin[f])) for f in firsts)
    c0, length = 200, 64
    placed = {c0 + 3: a[0], c0 + 40: a[1], c0 - 1: b[0], c0: b[1], c0 + length: c[0], c0 + length - 1: c[1]}
    rest = [int(x) for x in w["order"].tolist() if x not in set(placed.values())]
    order = []
    for at in range(e):
        order.append(placed[at] if at in placed else rest.pop(0))
    order = torch.tensor(order)
    position = torch.empty(e, dtype=torch.int64)
    position[order] = torch.arange(e)
    return position, order, c0, length, (a, b, c)


@pytest.mark.parametrize("p", [0.0, 0.4, 0.9])
@pytest.mark.parametrize("options", list(OPTIONS))
@pytest.mark.parametrize("window", ["inside", "clipped", "straddling"])
def test_draw_with_option_bits_equals_the_restatement_bit_for_bit(world, p, options, window):
    w = world
    hide_twins, paired = OPTIONS[options]
    position, order = w["position"], w["order"]
    if window == "straddling":
        position, order, c0, batch, (a, b, c) = _straddling_window(w)
    else:
        c0, batch = {"inside": (128, 100), "clipped": (w["e"] - 37, 100)}[window]
    stats = torch.tensor([5, 7], dtype=torch.int64, device=w["dev"])           # accumulated, never cleared
    kept, hidden = _draw(w, p, c0, batch, hide_twins, paired, position=position, stats=stats)
    cols = order[c0:c0 + batch].numpy()
    own = len(cols)
    assert own == {"inside": 100, "clipped": 37, "straddling": 64}[window]
    tw = w["twin"][cols]
    both = np.union1d(cols, tw[tw >= 0])
    if hide_twins:
        assert int(hidden.sum()) == both.size > own
    else:
        assert int(hidden.sum()) == own
    if window == "straddling":
        assert hidden[list(a)].all() and hidden[b[1]] and hidden[c[1]]
        assert bool(hidden[b[0]]) == hide_twins and bool(hidden[c[0]]) == hide_twins   # at c0 - 1 and at c0 + length
    w_col = _assert_draw_bits(w, kept)
    assert stats.tolist() == [5 + int(kept.sum()), 7 + int(hidden.sum())]       # every hidden edge once, twins included
    gone = both if hide_twins else cols                                          # weight 0 both ways
    assert bool((w_col[gone] == 0).all())
    for transposed in (False, True):
        _, _, perm, val = (t.cpu().numpy() for t in w["ed"].view.arrays(transposed))
        assert bool((val[np.isin(perm, gone)] == 0).all())
    if paired:                                                                   # a pair outside the window: one fate
        has = np.nonzero((w["twin"] >= 0) & ~hidden & ~hidden[np.maximum(w["twin"], 0)])[0]
        assert has.size > 500 and np.array_equal(kept[has], kept[w["twin"][has]])
        if p == 0.4:
            assert kept[has].any() and not kept[has].all()


# ----------------------------------------------------------------------------------------------- 3. the default is untouched
@pytest.mark.parametrize("p", [0.0, 0.4, 0.9])
@pytest.mark.parametrize("window", ["off", "inside", "clipped"])
def test_draw_without_a_bit_is_the_plain_restatement(world, p, window):
    w = world
    c0, batch = {"off": (0, 0), "inside": (128, 100), "clipped": (w["e"] - 37, 100)}[window]
    stats = torch.zeros(2, dtype=torch.int64, device=w["dev"])
    _draw(w, p, c0, batch, False, False, stats=stats, hide=window != "off")
    kept, hidden = R.kept_mask(w["e"], p, SEED, EPOCH, c0, batch if window != "off" else 0,
                               w["position"].numpy() if window != "off" else None)
    _assert_draw_bits(w, kept)
    assert stats.tolist() == [int(kept.sum()), int(hidden.sum())]
    assert int(hidden.sum()) == {"off": 0, "inside": 100, "clipped": 37}[window]


def test_paired_alone_needs_no_position_and_hide_twins_needs_one(world):
    w = world
    kept, hidden = _draw(w, 0.4, 77, 0, False, True, hide=False)
    assert not hidden.any()
    _assert_draw_bits(w, kept)
    has = np.nonzero(w["twin"] >= 0)[0]
    assert np.array_equal(kept[has], kept[w["twin"][has]])
    with pytest.raises(ValueError, match="position"):
        w["ed"].draw(0.4, w["rng"], batch=8, hide_twins=True)
    with pytest.raises(ValueError, match="batch"):
        w["ed"].draw(0.4, w["rng"], batch=1 << 61, position=w["position_dev"])


# ----------------------------------------------------------------------------------------------- 4. the leak is closed
def test_hidden_pairs_are_gone_in_both_directions_and_without_the_bit_they_leak(world):
    """p = 0, a window over one column of each of 48 pairs (and 16 lone columns).  With HIDE_TWINS the gathers, the layer
    with every gradient and the encoder equal the oracle on the graph WITHOUT both columns of every batch pair, at
    test_gpu_parity.py's gates; the same draw without the bit differs from that oracle in the rows of the batch's
    endpoints (the forward gather in no other row)."""
    w = world
    dev, twin, e = w["dev"], w["twin"], w["e"]
    firsts = [int(c) for c in np.nonzero(twin >= 0)[0] if c < twin[c]]
    batch_cols = firsts[::13][:48] + [int(c) for c in np.nonzero(twin < 0)[0][:16]]
    rest = [c for c in w["order"].tolist() if c not in set(batch_cols)]
    c0 = 300
    order = torch.tensor(rest[:c0] + batch_cols + rest[c0:])
    position = torch.empty(e, dtype=torch.int64)
    position[order] = torch.arange(e)
    torch.manual_seed(8)
    emb = torch.nn.init.xavier_uniform_(torch.empty(N, 64))
    convs = [RGCNConv(64, 128, NR_REL).to(dev), RGCNConv(128, 128, NR_REL).to(dev)]
    for c in convs:
        c.bias.data.uniform_(-0.1, 0.1)
    cot = (torch.randn(N, 128), torch.randn(N, 128))
    wide = torch.randn(N, 128) * 0.1
    kept, hidden = _draw(w, 0.0, c0, len(batch_cols), True, False, position=position)
    gone = np.zeros(e, dtype=bool)
    gone[batch_cols] = True
    gone[twin[batch_cols][twin[batch_cols] >= 0]] = True
    assert np.array_equal(hidden, gone) and np.array_equal(kept, ~gone) and int(gone.sum()) == 2 * 48 + 16
    _oracle_checks(w, kept, convs, emb, wide, cot)            # both gathers, the layer with every gradient, the encoder
    # the same window without the bit, against the SAME oracle (the graph without both columns)
    plain_kept, plain_hidden = _draw(w, 0.0, c0, len(batch_cols), False, False, position=position)
    assert int(plain_hidden.sum()) == len(batch_cols)
    ek, tk = (torch.from_numpy(a) for a in R.kept_subgraph(w["ei"].numpy(), w["et"].numpy(), kept))
    cnt = O._segment_counts(ek, tk, N, NR_REL, torch.float64)
    ends = np.unique(w["ei"].numpy()[:, batch_cols])
    for transposed, ref in ((False, O._mean_agg), (True, O._mean_agg_transposed)):
        got = ops.aggregate(w["ed"].view, emb.to(dev), transposed=transposed).double().cpu()
        off = (got - ref(emb.double(), ek, tk, N, NR_REL, cnt)).abs().amax(dim=1) > FWD_ATOL
        rows = torch.nonzero(off).view(-1).numpy()
        # (forward: row h of a reverse column (t, r, h) and no other; transposed, the weight 1 / k[h, r] of every edge
        # into (h, r) moves with k, so the rows of their sources differ as well)
        assert rows.size > 0 and (transposed or np.isin(rows, ends).all()), (transposed, rows, ends)
        with pytest.raises(AssertionError):
            assert_fwd(got, ref(emb.double(), ek, tk, N, NR_REL, cnt))
    # the reverse column of every batch pair still carries a weight: the head is averaged into the tail
    w_col = R.weights(w["ei"].numpy(), w["et"].numpy(), plain_kept, N, NR_REL)
    assert bool((w_col[twin[batch_cols[:48]]] > 0).all())


# ----------------------------------------------------------------------------------------------- 5. capture and replay
def test_a_replay_with_both_bits_draws_at_the_moved_cursor(world):
    w = world
    dev, ed, view = w["dev"], w["ed"], w["ed"].view
    torch.manual_seed(9)
    emb = torch.nn.init.xavier_uniform_(torch.empty(N, 64)).to(dev)
    convs = [RGCNConv(64, 128, NR_REL).to(dev), RGCNConv(128, 128, NR_REL).to(dev)]
    cot = torch.randn(N, 128, device=dev)
    eid, etd = w["ei"].to(dev), w["et"].to(dev)
    cursor = torch.zeros(1, dtype=torch.int64, device=dev)
    x = emb.clone().requires_grad_(True)
    params = [x] + [p for c in convs for p in c.parameters()]

    def step():
        ed.draw(0.4, w["rng"], cursor=cursor, batch=128, position=w["position_dev"], hide_twins=True, paired=True)
        out = rgcn_encoder2(x, eid, etd, convs[0], convs[1], graph=view)
        (out * cot).sum().backward()
        return out

    def eager(c0):
        cursor.fill_(c0)
        for p in params:
            p.grad = None
        out = step()
        return [out.detach().clone(), view.arrays(False)[3], view.arrays(True)[3], ed.kept_counts()] + [p.grad.clone() for p in params]

    a, b, a2 = eager(128), eager(640), eager(128)
    assert all(torch.equal(u, v) for u, v in zip(a, a2))
    assert not torch.equal(a[1], b[1]) and not torch.equal(a[0], b[0])
    kept, _ = TW.kept_mask(w["e"], w["twin"], 0.4, SEED, EPOCH, 640, 128, w["position"].numpy(), hide_twins=True, paired=True)
    assert np.array_equal(b[3].cpu().numpy(), R.kept_counts(w["ei"].numpy(), w["et"].numpy(), kept, N, NR_REL))
    cursor.fill_(128)
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    cursor.fill_(640)
    graph.replay()
    torch.cuda.synchronize()
    got = [out.detach(), view.arrays(False)[3], view.arrays(True)[3], ed.kept_counts()] + [p.grad for p in params]
    for i, (u, v) in enumerate(zip(got, b)):
        assert torch.equal(u, v), f"replayed output {i} differs from the eager run at the same cursor"


# ----------------------------------------------------------------------------------------------- 6. the trainer
@pytest.mark.parametrize("hip_graph", [False, True])
def test_trainer_steps_with_all_four_flags_match_the_oracle_on_the_kept_subgraphs(world, tmp_path, hip_graph):
    """test_edge_dropout.py's trainer test with --hide_reverse_edges --paired_edge_dropout on top: the oracle replays the
    recorded batches over the subgraph the twin restatement says each step kept.  Gates: per-step loss within 2e-5
    relative to max(1, |loss|), parameters within 5e-5 after five Adam steps."""
    dev = world["dev"]
    torch.manual_seed(0)
    ei, et, e, twin = world["ei"], world["et"], world["e"], world["twin"]
    data = {"edge_index": ei, "edge_type": et, "num_nodes": N, "num_relations": NR_REL}
    args = T.parse_args([])
    for k, v in dict(dropout=0.0, decoder_dropout=0.0, batch_size=128, output_dir=str(tmp_path), device="cuda",
                     no_hip_graph=not hip_graph, edge_dropout=0.4, hide_batch_edges=True, hide_reverse_edges=True,
                     paired_edge_dropout=True).items():
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
    params = {k: v.clone().requires_grad_(True) for k, v in ref_state.items()}
    opt = torch.optim.Adam(list(params.values()), lr=args.lr)
    conv = lambda i: {k: params[f"encoder.conv{i}.{k}"] for k in ("weight", "root", "bias")}   # noqa: E731
    kept_total = hidden_total = 0
    for step, (h, t, rl, lb, loss_gpu) in enumerate(log):
        c0 = step * 128
        assert torch.equal(h[:128], ei[0, order[c0:c0 + 128]]) and torch.equal(t[:128], ei[1, order[c0:c0 + 128]])
        kept, hidden = TW.kept_mask(e, twin, 0.4, seed, epoch, c0, 128, position.numpy(), hide_twins=True, paired=True)
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
    assert trainer.edge_dropout_stats == (kept_total, hidden_total) and hidden_total > 5 * 128
    assert trainer.reverse_edges_found() is None              # five steps are not an epoch: nothing to say yet


def test_trainer_says_after_an_epoch_whether_the_data_stores_reverse_columns(world, tmp_path):
    """a whole (short) epoch on the graph with pairs hides more edges than it has columns; on the same graph with every
    relation of a reverse column moved, exactly as many: what train() warns about after the first epoch"""
    dev = world["dev"]
    ei, et = world["ei"], world["et"]
    one_way = torch.where(ei[0] > ei[1], (et + 1) % NR_REL, et)          # (b, r + 1, a) is no twin of (a, r, b)
    for types, found in ((et, True), (one_way, False)):
        if not found:
            assert int((TW.twins(ei.numpy(), types.numpy()) >= 0).sum()) == 0
        data = {"edge_index": ei, "edge_type": types, "num_nodes": N, "num_relations": NR_REL}
        args = T.parse_args(["--output_dir", str(tmp_path), "--dropout", "0.0", "--batch_size", "512", "--hide_batch_edges",
                             "--hide_reverse_edges", "--no_hip_graph"])
        trainer = T.Trainer(T.create_model(N, NR_REL, args), data, data, data, dev, args)
        trainer.train_epoch()
        assert trainer.reverse_edges_found() is found
        assert (trainer.edge_dropout_stats[1] > world["e"]) == found
