"""CPU tier of the TransE baseline (``csrc/transe.hip``, ``include/rgcn_transe.h``, ``baselines.py``): the C surface and
every argument check that runs before a launch, the wrappers' refusals, the two update orders of the host restatement
(``transe_reference.py``) against each other, the augmented-row ranking device restated on the host with exact integer
rows, the degree baseline against a loop, and the recorded seed spread the GPU tier judges the device fit by."""
import json
import os

import numpy as np
import pytest
import torch

import make_transe_golden as G
import transe_reference as R
from conftest import GOLDEN, ROOT
from primekg_rgcn_linkprediction_amd import _lib, baselines, ops

ARRAYS = ("emb", "rel", "heads", "tails", "rels", "loss_mean", "loss_sum", "active_sum", "workspace")


def _call(lib, n=10, r=3, d=64, batch=5, given=(), ws_bytes=None, **holes):
    p = {name: (8 if given == "all" or name in given else None) for name in ARRAYS}
    p.update(holes)
    if ws_bytes is None:
        ws_bytes = lib.rgcn_transe_step_workspace_bytes(batch, d, r)
    return lib.rgcn_transe_step(p["emb"], n, p["rel"], r, d, p["heads"], p["tails"], p["rels"], batch, 0.01, 1.0,
                                p["loss_mean"], p["loss_sum"], p["active_sum"], p["workspace"], ws_bytes, None)


# ---------------------------------------------------------------------------------- C surface
def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    A, U, OK = _lib.RGCN_ERR_ARG, _lib.RGCN_ERR_UNSUPPORTED, _lib.RGCN_OK
    call = lambda **kw: _call(lib, **kw)
    # ranges: with and without samples, with and without pointers
    for bad in (dict(d=0), dict(d=-4), dict(d=6), dict(d=63), dict(n=0), dict(n=-1), dict(r=0), dict(r=-2)):
        assert call(given="all", ws_bytes=1 << 30, **bad) == A, bad
        assert call(batch=0, ws_bytes=0, **bad) == A, bad
    assert call(batch=-1) == A and call(given="all", batch=-1, ws_bytes=1 << 30) == A
    # a NULL array with batch > 0: every one that is needed, on its own; the two accumulators may be NULL
    assert call() == A
    for name in ARRAYS:
        if name not in ("loss_sum", "active_sum"):
            assert call(given="all", **{name: None}) == A, name
    # a workspace smaller than the query says
    need = lib.rgcn_transe_step_workspace_bytes(5, 64, 3)
    assert need >= (2 * 5 * 64 + 5 * 64 + 3 * 64 + 5) * 4 + 5 * 5 * 4
    assert call(given="all", ws_bytes=need - 1) == A and call(given="all", ws_bytes=0) == A
    # the keys are int32: reached with every pointer given and the accumulators NULL, before the workspace is sized
    assert call(given="all", n=1 << 31) == U and call(given="all", n=(1 << 31) - 1 + 1, loss_sum=None, active_sum=None) == U
    assert call(given="all", r=1 << 31, ws_bytes=1 << 40) == U
    # an empty batch: before any pointer is looked at, and before the size bound
    assert call(batch=0, ws_bytes=0) == OK and call(batch=0, n=1 << 40, ws_bytes=0) == OK
    # the workspace query: 0 for what the step rejects or does not launch, growing with each size otherwise
    q = lib.rgcn_transe_step_workspace_bytes
    assert q(0, 64, 3) == q(-1, 64, 3) == q(5, 0, 3) == q(5, 6, 3) == q(5, 64, 0) == 0
    assert q(6, 64, 3) >= need and q(5, 128, 3) > need and q(5, 64, 300) > need
    assert q(1025, 64, 3) >= (3 * 1025 * 64 + 2 * 3 * 64) * 4               # two segments of the relation tree


def test_header_table_and_library_agree():
    """names, parameters, return types and exports: test_c_surface.py, for every header"""
    makefile = open(os.path.join(ROOT, "primekg_rgcn_linkprediction_amd", "csrc", "Makefile")).read()
    assert " transe.hip" in makefile


# ---------------------------------------------------------------------------------- wrappers
def test_wrappers_refuse_cpu_tensors_and_wrong_shapes_by_name():
    emb, rel = torch.zeros(10, 64), torch.zeros(3, 64)
    idx = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="emb is on cpu.*no CPU fallback"):
        ops.transe_step(emb, rel, idx, idx, idx, 5, 0.01, 1.0)
    with pytest.raises(TypeError, match="emb must be a torch.Tensor"):
        ops.transe_step(None, rel, idx, idx, idx, 5, 0.01, 1.0)
    with pytest.raises(RuntimeError, match="emb is on cpu"):
        ops.transe_rank_operands(emb, rel, idx, idx, "tail")
    with pytest.raises(ValueError, match="side"):
        ops.transe_rank_operands(emb, rel, idx, idx, "both")
    model = baselines.TransE(num_epochs=1, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.fit(torch.zeros(2, 4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 10, 3)
    with pytest.raises(RuntimeError, match="fit"):
        baselines.TransE().predict([0], [1])
    with pytest.raises(ValueError, match="embedding_dim"):
        baselines.TransE(embedding_dim=30)


def test_shape_checks_by_name_on_a_stubbed_device(monkeypatch):
    """the dtype and shape checks sit behind the device check: reached here with that one check taken out"""
    def need(name, t, dtype):
        if t.dtype != dtype:
            raise TypeError(f"{name} must be {dtype}, got {t.dtype}")

    monkeypatch.setattr(ops, "_need_gpu", need)
    emb, rel = torch.zeros(10, 64), torch.zeros(3, 64)
    idx = torch.zeros(10, dtype=torch.int64)
    for kw, word in ((dict(emb=torch.zeros(10, 62)), "emb"), (dict(emb=torch.zeros(64)), "emb"), (dict(rel=torch.zeros(3, 32)), "rel"),
                     (dict(rel=torch.zeros(0, 64)), "rel"), (dict(heads=idx[:9]), "heads"), (dict(tails=idx[:5]), "tails"),
                     (dict(rels=idx.view(2, 5)), "rels"), (dict(batch=-1), "batch"),
                     (dict(loss_sum=torch.zeros(2, dtype=torch.float64)), "loss_sum"),
                     (dict(active_sum=torch.zeros(3, dtype=torch.int64)), "active_sum")):
        args = dict(emb=emb, rel=rel, heads=idx, tails=idx, rels=idx, batch=5, lr=0.01, margin=1.0)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            ops.transe_step(**args)
    for kw, word in ((dict(emb=emb.double()), "emb"), (dict(heads=idx.int()), "heads"), (dict(loss_sum=torch.zeros(1)), "loss_sum")):
        args = dict(emb=emb, rel=rel, heads=idx, tails=idx, rels=idx, batch=5, lr=0.01, margin=1.0)
        args.update(kw)
        with pytest.raises(TypeError, match=word):
            ops.transe_step(**args)
    with pytest.raises(ValueError, match="rel"):
        ops.transe_rank_operands(emb, torch.zeros(3, 32), idx, idx, "tail")
    with pytest.raises(ValueError, match="rel_idx"):
        ops.transe_rank_operands(emb, rel, idx, idx[:4], "head")


# ---------------------------------------------------------------------------------- the two orders
def _tables(n, r, d, seed):
    e, rel = R.init_tables(n, r, d, np.random.RandomState(seed))
    return e.astype(np.float32), rel.astype(np.float32)


def test_without_repeats_across_samples_the_two_orders_agree():
    n, b = 64, 12
    e, rel = _tables(n, b, 64, 1)                                        # one relation row per sample: see below
    rng = np.random.RandomState(2)
    nodes = rng.permutation(n)
    h, t, fresh = nodes[:b], nodes[b:2 * b], nodes[2 * b:3 * b]
    coin = rng.rand(b) < 0.5
    hn, tn = np.where(coin, fresh, h), np.where(coin, t, fresh)         # a corruption repeats its own sample's row only
    ri = rng.permutation(b)
    # the precondition: no row in two samples - entity rows AND relation rows (the entity gradients 2 lr (h + r - t)
    # contain r, so in the reference's order a later sample of the same relation sees the row an earlier one moved)
    for i in range(b):
        for j in range(i + 1, b):
            assert not {h[i], t[i], hn[i], tn[i]} & {h[j], t[j], hn[j], tn[j]} and ri[i] != ri[j]
    heads, tails, rels = np.r_[h, hn], np.r_[t, tn], np.r_[ri, ri]
    sync = R.step(e, rel, heads, tails, rels, 0.01, 1.0)
    assert sync.active.all()
    e2, r2, loss2, active2 = R.step_in_sample_order(e, rel, heads, tails, rels, 0.01, 1.0)
    touched = sync.touched
    assert touched.sum() == 3 * b
    assert np.abs(sync.emb[touched] - e2[touched]).max() <= 1e-12 and np.abs(sync.rel - r2).max() <= 1e-12
    assert abs(sync.loss_mean - loss2) <= 1e-12 and int(sync.active.sum()) == active2
    # the deliberate departure: the contract leaves the other rows alone, the reference renormalises them
    assert np.array_equal(sync.emb[~touched], e[~touched].astype(np.float64)) and np.all(sync.emb_bound[~touched] == 0)
    e3, r3, loss3, active3 = R.step_synchronous(e, rel, heads, tails, rels, 0.01, 1.0)
    assert np.abs(sync.emb - e3).max() <= 1e-15 and np.abs(sync.rel - r3).max() <= 1e-15 and (loss3, active3) == (sync.loss_mean, b)


def test_with_a_hub_in_forty_slots_the_two_orders_differ():
    n, b = 64, 48
    e, rel = _tables(n, 3, 64, 3)
    rng = np.random.RandomState(4)
    h, t = rng.randint(1, n, b), rng.randint(1, n, b)
    hn, tn = R.corrupt(h, t, n, rng)
    hn[hn == 0], tn[tn == 0] = 1, 1
    for slot, arr in enumerate((h, t, hn, tn)):                         # ten slots of each kind name node 0
        arr[slot::4][:10] = 0
    ri = rng.randint(0, 3, b)
    heads, tails, rels = np.r_[h, hn], np.r_[t, tn], np.r_[ri, ri]       # any four ids are a legal sample
    assert (heads == 0).sum() + (tails == 0).sum() == 40
    sync = R.step(e, rel, heads, tails, rels, 0.01, 1.0, check_margins=False)
    e2, _, _, _ = R.step_in_sample_order(e, rel, heads, tails, rels, 0.01, 1.0)
    assert sync.active.sum() >= 40
    assert np.abs(sync.emb[0] - e2[0]).max() > 1e-4                     # the contract is the synchronous one


# ---------------------------------------------------------------------------------- ranking by distance
def test_rank_operands_order_exactly_by_distance_on_integer_rows():
    rng = np.random.RandomState(5)
    n, r, d, b = 50, 3, 64, 24
    e = rng.randint(-2, 3, (n, d)).astype(np.float32)
    e[7] = e[3]                                                         # a tie: two candidates at one distance
    rel = rng.randint(-2, 3, (r, d)).astype(np.float32)
    anchors, rels, targets = rng.randint(0, n, b), rng.randint(0, r, b), rng.randint(0, n, b)
    targets[0], targets[1] = 3, 7
    eligible = rng.rand(b, n) < 0.7
    for side in ("tail", "head"):
        q, cand = R.rank_operands(e, rel, anchors, rels, side)
        assert q.shape == (b, 96) and cand.shape == (n, 96) and q.dtype == cand.dtype == np.float32
        assert np.all(q[:, 64] == -0.5) and np.all(q[:, 65:] == 0) and np.all(cand[:, 65:] == 0)
        score = q @ cand.T                                              # integers and halves below 2^24: exact in fp32
        assert np.array_equal(score.astype(np.float64), q.astype(np.float64) @ cand.astype(np.float64).T)
        dist = R.distances(e, rel, anchors, rels, side)
        sq = (q[:, :d].astype(np.float64) ** 2).sum(1, keepdims=True)
        assert np.array_equal(sq - 2 * score, dist)                     # monotone in minus the squared distance, exactly
        true = score[np.arange(b), targets]
        for mask in (None, eligible):
            ok = np.ones((b, n), dtype=bool) if mask is None else mask.copy()
            ok[np.arange(b), targets] = False
            by_score = 1 + (ok & (score > true[:, None])).sum(1)         # the ranking pass's count: ties do not count
            assert np.array_equal(by_score, R.ranks_by_distance(dist, targets, mask))
            top = R.topk_by_distance(dist, 5, mask)
            okk = np.ones((b, n), dtype=bool) if mask is None else mask
            for i in range(b):                                           # the top-k pass's order: score descending, id ascending
                order = [j for j in np.lexsort((np.arange(n), -score[i])) if okk[i, j]][:5]
                assert top[i, :len(order)].tolist() == order and np.all(top[i, len(order):] == -1)
        assert R.ranks_by_distance(dist, targets)[0] == R.ranks_by_distance(dist, np.r_[7, targets[1:]])[0]   # the tie


# ---------------------------------------------------------------------------------- the simple baselines
def test_node_degree_against_a_loop():
    ei = torch.tensor([[0, 0, 1, 2, 3, 3, 3, 5, 8, 9, 9, 11], [4, 5, 4, 6, 4, 7, 7, 3, 9, 10, 0, 11]])
    cls = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 0, 1], dtype=torch.int32)      # 0 drug, 1 disease, 2 other
    base = baselines.NodeDegree().fit(ei, cls, 0, 1)
    degree = {}
    for u, v in ei.t().tolist():
        degree[u] = degree.get(u, 0) + 1
        degree[v] = degree.get(v, 0) + 1
    drug = {i: degree.get(i, 0) for i in range(12) if cls[i] == 0}
    dis = {i: degree.get(i, 0) for i in range(12) if cls[i] == 1}
    drug = {k: v / max(drug.values()) for k, v in drug.items()}
    dis = {k: v / max(dis.values()) for k, v in dis.items()}
    pairs = [(a, b) for a in range(12) for b in range(12)]
    want = [np.sqrt(drug.get(a, 0.01) * dis.get(b, 0.01)) for a, b in pairs]
    got = base.predict([a for a, _ in pairs], [b for _, b in pairs])
    assert np.allclose(got.numpy(), want, rtol=0, atol=1e-15)
    assert np.allclose(base.predict_all(range(12), range(12)).numpy().reshape(-1), want, rtol=0, atol=1e-15)
    assert max(drug.values()) == 1.0 and drug[10] < 1 and dis[11] == 2 / max(degree[i] for i in range(12) if cls[i] == 1)
    a, b = baselines.Random(3), baselines.Random(3)
    assert torch.equal(a.predict(range(5), range(5)), b.predict(range(5), range(5)))
    assert a.predict_all(range(4), range(6)).shape == (4, 6) and 0 <= float(a.predict(range(9), range(9)).min())


# ---------------------------------------------------------------------------------- the recorded spread
def test_two_seeds_of_the_recorded_spread_reproduce():
    with open(os.path.join(GOLDEN, "transe_spread.json")) as fh:
        gold = json.load(fh)
    assert gold["config"] == G.CONFIG and gold["order"] == "sample" and sorted(gold["seeds"]) == [str(s) for s in G.SEEDS]
    assert len(gold["seeds"]) == 8
    for seed in (1, 6):
        got = G.one_seed(seed)
        assert abs(got["loss"] - gold["seeds"][str(seed)]["loss"]) <= 1e-9
        assert abs(got["closer_share"] - gold["seeds"][str(seed)]["closer_share"]) <= 1e-12
