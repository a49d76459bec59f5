"""Top-k candidates from the fused ranking pass, the part that needs no GPU: the C-ABI surface of the two new entry
points and their argument checks, the workspace size, the host restatement the GPU tests compare against (checked here
against a brute-force python loop), and the prediction CLI's arguments and JSON shape on a stubbed evaluator."""
import ctypes
import json
import math

import pytest
import torch

from topk_reference import brute_topk, ragged_case, restate_topk
from primekg_rgcn_linkprediction_amd import _lib, consumers, ops
from primekg_rgcn_linkprediction_amd import predict as P

NINF = -math.inf


def test_topk_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    A, U, OK = _lib.RGCN_ERR_ARG, _lib.RGCN_ERR_UNSUPPORTED, _lib.RGCN_OK

    # distmult_topk_masked(q, emb, allow, query_class, classes, exclude, min_score, B, N, d, k, slices, ids, scores, ws, ws_bytes, stream)
    def call(q=None, emb=None, allow=None, qcls=None, classes=0, excl=None, floor=NINF, b=4, n=100, d=64, k=10, slices=0,
             ids=None, scores=None, ws=None, ws_bytes=0):
        return lib.distmult_topk_masked(q, emb, allow, qcls, classes, excl, floor, b, n, d, k, slices, ids, scores, ws,
                                        ws_bytes, None)

    assert call(d=48) == U                                       # d % 32
    assert call() == A                                           # nulls
    assert call(b=-1) == A and call(n=0) == A and call(d=0) == A and call(k=0) == A and call(k=-3) == A
    assert call(slices=-1) == A and call(classes=-1) == A
    assert call(allow=8, classes=3) == A                         # allow without query classes
    assert call(allow=8, qcls=8, classes=0) == A                 # allow without classes
    assert call(floor=math.nan) == A
    assert call(b=0) == OK                                       # empty batch: before any pointer is looked at
    assert call(b=0, k=10 ** 6) == OK
    need = lib.distmult_topk_workspace_bytes(4, 100, 10, 0)
    assert call(q=8, emb=8, ids=8, scores=8, k=ops.TOPK_MAX_K + 1, ws=8, ws_bytes=1 << 30) == U      # k above the cap
    assert call(q=8, emb=8, ids=8, scores=8, ws=None, ws_bytes=need) == A                             # no workspace
    assert call(q=8, emb=8, ids=8, scores=8, ws=8, ws_bytes=need - 1) == A                            # short workspace
    assert call(q=8, emb=8, ids=None, scores=8, ws=8, ws_bytes=need) == A
    assert call(q=8, emb=8, ids=8, scores=8, n=1 << 31, ws=8, ws_bytes=1 << 40) == U


def test_topk_workspace_is_monotone_and_zero_for_an_empty_batch():
    lib = _lib.load()
    size = lib.distmult_topk_workspace_bytes
    assert size(0, 30926, 10, 0) == 0 and size(-1, 30926, 10, 0) == 0 and size(4, 0, 10, 0) == 0
    assert size(4, 100, 0, 0) == 0 and size(4, 100, 10, -1) == 0
    for b in (1, 64, 15372):
        by_k = [size(b, 30926, k, 0) for k in (1, 2, 10, 64, 100, 128)]
        assert by_k == sorted(by_k) and by_k[0] > 0 and by_k[0] < by_k[-1]
        by_s = [size(b, 30926, 10, s) for s in (1, 2, 3, 7, 50, 121, 242, 1000)]
        assert by_s == sorted(by_s) and by_s[0] == b * 10 * 8                  # one slice: batch x k (score, id) pairs
        assert by_s[-1] == b * 10 * 8 * 242                                   # at most one slice per 128 entities
    # a slice per column tile at most, 256 at most
    assert size(1, 100, 10, 7) == 80 and size(1, 129, 10, 7) == 160
    assert size(1, 128 * 1000, 10, 1000) == 80 * 250              # 1,000 column tiles, four per slice: no empty slice
    # the automatic rule: a large batch keeps one slice, a small one is cut up to fill the device
    assert size(15372, 30926, 100, 0) == 15372 * 100 * 8
    assert size(1, 30926, 100, 0) == 242 * 100 * 8 and size(64, 30926, 10, 0) == 64 * 242 * 10 * 8


def test_python_wrapper_checks_k_before_anything_else():
    q = torch.zeros(2, 32)
    for k in (0, -1, ops.TOPK_MAX_K + 1):
        with pytest.raises(ValueError, match=f"{ops.TOPK_MAX_K}"):
            ops.distmult_topk_masked(q, q, k)                                  # (CPU tensors: the k check comes first)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.distmult_topk_masked(q, q, 1)
    with pytest.raises(ValueError):
        ops.distmult_topk_masked(q, q, 1, slices=-1)


def test_host_restatement_against_a_brute_force_loop():
    g = torch.Generator().manual_seed(11)
    s = torch.randn(7, 45, generator=g)
    s[1, 3] = float("nan")
    s[2] = 0.0                                                   # all ties: ids ascending
    s[4, 10:20] = s[4, 9]                                        # a run of equal scores
    allowed = torch.rand(7, 45, generator=g) < 0.5
    allowed[5] = False                                           # a row without candidates
    known = torch.rand(7, 45, generator=g) < 0.3
    for k in (1, 5, 44, 45, 60):                                 # k > N: padding past the candidates
        for a in (None, allowed):
            for e in (None, known):
                for floor in (None, 0.25, float(s[0, 7])):       # a floor that occurs: the >= edge
                    got, want = restate_topk(s, k, a, e, floor), brute_topk(s, k, a, e, floor)
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (k, a is None, e is None, floor)
    ids, vals = restate_topk(s, 5)
    assert ids[2].tolist() == [0, 1, 2, 3, 4] and not bool((ids[1] == 3).any())
    ids, vals = restate_topk(s, 60, allowed, known)
    assert bool((ids[5] == -1).all()) and bool((vals[5] == NINF).all()) and bool((ids[:, 45:] == -1).all())
    ids, vals = restate_topk(s, 45, None, None, float(s[0, 7]))
    assert 7 in ids[0].tolist() and bool((vals[0][ids[0] >= 0] >= s[0, 7]).all())


def test_host_restatement_with_infinite_and_nan_scores():
    """+inf and -inf are scores like any other, NaN is no candidate: +inf candidates first by id, a -inf candidate after
    every finite one with its real id, padding (id -1) behind it; a ``min_score`` strikes the -inf candidates."""
    g = torch.Generator().manual_seed(12)
    s = torch.randn(8, 45, generator=g)
    inf = math.inf
    s[0, [3, 17, 40]] = inf
    s[1, [0, 44]] = -inf
    s[2, 5], s[2, 6], s[2, 7] = inf, -inf, math.nan
    s[3] = math.nan                                              # a NaN row: no candidate at all
    s[4] = -inf                                                  # every candidate scores -inf: ids ascending
    s[5] = inf
    s[6, ::2] = math.nan
    s[6, 1] = -inf
    allowed = torch.rand(8, 45, generator=g) < 0.5
    allowed[0, 17] = False
    allowed[0, 3] = allowed[0, 40] = allowed[1, 44] = True
    known = torch.rand(8, 45, generator=g) < 0.3
    known[1, 0] = known[1, 44] = False
    for k in (1, 5, 44, 45, 60):
        for a in (None, allowed):
            for e in (None, known):
                for floor in (None, 0.25, -inf, inf):
                    got, want = restate_topk(s, k, a, e, floor), brute_topk(s, k, a, e, floor)
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (k, a is None, e is None, floor)
                    assert not bool(((got[0][:, :-1] < 0) & (got[0][:, 1:] >= 0)).any())       # valid slots come first
                    assert not bool(torch.isnan(got[1]).any())
    ids, vals = restate_topk(s, 45)
    assert ids[0, :3].tolist() == [3, 17, 40] and bool((vals[0, :3] == inf).all())
    assert ids[1, 43:].tolist() == [0, 44] and bool((vals[1, 43:] == NINF).all()) and bool((vals[1, :43] > NINF).all())
    assert ids[2, 0] == 5 and ids[2, 43:].tolist() == [6, -1] and 7 not in ids[2].tolist()
    assert bool((ids[3] == -1).all()) and bool((vals[3] == NINF).all())
    assert ids[4].tolist() == list(range(45)) and ids[5].tolist() == list(range(45))
    assert sorted(ids[6, :21].tolist()) == list(range(3, 45, 2)) and ids[6, 21:23].tolist() == [1, -1]
    assert int((ids[6] >= 0).sum()) == 22
    ids, vals = restate_topk(s, 60, allowed)
    assert ids[0, :2].tolist() == [3, 40] and 44 in ids[1].tolist() and bool((ids[:, 45:] == -1).all())
    # a floor strikes the -inf candidates: the slot holds padding, not an id
    ids, vals = restate_topk(s, 45, min_score=-1e30)
    assert ids[1, 43:].tolist() == [-1, -1] and bool((ids[4] == -1).all())
    ids, _ = restate_topk(s, 45, min_score=inf)
    assert ids[0, :4].tolist() == [3, 17, 40, -1] and ids[5].tolist() == list(range(45)) and bool((ids[1] == -1).all())


def test_exclude_mask_changes_most_top10_lists_of_the_ragged_shapes():
    """the condition the GPU test relies on, from the generators alone (randn scores): 1 - 0.7^10 = 0.97 expected"""
    from topk_reference import RAGGED
    for batch, entities, d in RAGGED:
        if batch < 63:
            continue
        c = ragged_case(batch, entities, d)
        g = torch.Generator().manual_seed(batch * 1000 + entities + d)
        s = torch.randn(batch, entities, generator=g)
        changed = (restate_topk(s, 10)[0] != restate_topk(s, 10, known=c["known"])[0]).any(1).float().mean().item()
        assert changed >= 0.8, (batch, entities, d, changed)
        if entities <= 129:
            both = restate_topk(s, 64, c["allowed"], c["known"])[0]
            assert bool((both[:, -1] == -1).all())                # fewer than 64 candidates in every row


class _StubEvaluator:
    """``top_candidates`` from a fixed score table on the CPU (the restatement), recording how it was called"""

    def __init__(self, n=40, classes=None):
        g = torch.Generator().manual_seed(5)
        self.table = torch.randn(n, n, generator=g)
        self.node_class = classes
        self.known = torch.rand(n, n, generator=g) < 0.2
        self.calls = []

    def top_candidates(self, side, anchors, relations, k, novel=True, candidate_class=None, min_score=None):
        self.calls.append(dict(side=side, anchors=anchors.tolist(), relations=relations.tolist(), k=k, novel=novel,
                               candidate_class=candidate_class, min_score=min_score))
        s = self.table[anchors]
        allowed = None if candidate_class is None else (self.node_class == candidate_class).view(1, -1).expand_as(s)
        return restate_topk(s, k, allowed, self.known[anchors] if novel else None, min_score)


def test_predict_cli_arguments_and_json_shape_on_a_stubbed_evaluator(tmp_path, capsys):
    base = ["--model_path", "m.pt", "--relation", "1"]
    args = P.parse_args(base + ["--anchors", "3", "5"])
    assert args.side == "tail" and args.anchors == [3, 5] and args.top_k == 10 and not args.novel
    assert args.candidate_class is None and args.min_score is None and args.anchor_class is None
    for bad in (base, base + ["--anchors", "1", "--anchor_class", "0"], base + ["--anchor_class", "0"],
                base + ["--anchors", "1", "--candidate_class", "1"], base + ["--anchors", "1", "--top_k", "0"],
                ["--model_path", "m.pt", "--anchors", "1"], base + ["--anchors", "1", "--side", "both"]):
        with pytest.raises(SystemExit):
            P.parse_args(bad)
    assert "--node_types" in capsys.readouterr().err
    classes = torch.tensor([0] * 10 + [1] * 30, dtype=torch.int32)
    ev = _StubEvaluator(40, classes)
    args = P.parse_args(base + ["--anchor_class", "0", "--side", "head", "--top_k", "35", "--novel", "--candidate_class", "1",
                                "--node_types", "x.npz", "--min_score", "-0.5", "--output_dir", str(tmp_path / "out")])
    names = {i: f"node{i}" for i in range(40)}
    result = P.predict(ev, args, names)
    assert ev.calls == [dict(side="head", anchors=list(range(10)), relations=[1] * 10, k=35, novel=True, candidate_class=1,
                             min_score=-0.5)]
    assert set(result) == {"protocol", "queries"} and len(result["queries"]) == 10
    assert result["protocol"]["side"] == "head" and result["protocol"]["novel"] is True and result["protocol"]["top_k"] == 35
    want_ids, want_scores = restate_topk(ev.table[:10], 35, (classes == 1).view(1, -1).expand(10, 40), ev.known[:10], -0.5)
    for b, q in enumerate(result["queries"]):
        assert set(q) == {"anchor", "relation", "candidates", "anchor_name", "candidate_names"}
        assert q["anchor"] == b and q["relation"] == 1 and q["anchor_name"] == f"node{b}"
        keep = want_ids[b] >= 0
        assert 0 < len(q["candidates"]) < 35                      # at most 30 of the class: the padding is dropped
        assert [c[0] for c in q["candidates"]] == want_ids[b][keep].tolist()
        assert [c[1] for c in q["candidates"]] == want_scores[b][keep].tolist()
        assert q["candidate_names"] == [f"node{i}" for i, _ in q["candidates"]]
        assert all(classes[i] == 1 and not ev.known[b, i] and s >= -0.5 for i, s in q["candidates"])
    path = P.save_predictions(result, tmp_path / "out")
    assert path.name == "predictions.json" and json.loads(path.read_text()) == result
    # no names without an idx2node map; explicit anchors
    plain = P.predict(ev, P.parse_args(base + ["--anchors", "7", "2"]), None)
    assert [q["anchor"] for q in plain["queries"]] == [7, 2] and set(plain["queries"][0]) == {"anchor", "relation", "candidates"}
    assert len(plain["queries"][0]["candidates"]) == 10 and ev.calls[-1]["novel"] is False
    assert P.load_node_names(None) is None and P.load_node_names("types.npz") is None
    torch.save({"idx2node": {0: ("7", "aspirin", "drug"), 1: ("9", "asthma", "disease")}}, tmp_path / "mappings.pt")
    assert P.load_node_names(str(tmp_path / "mappings.pt")) == {0: "aspirin", 1: "asthma"}


def test_batched_consumers_need_the_device_and_a_relation_free_known_set():
    emb = torch.randn(8, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        consumers.predict_top_drugs_batch(emb, [0, 1], [2, 3, 4], 2)
    assert {"predict_top_drugs_batch", "novel_drug_predictions", "predict_top_drugs"} <= set(dir(consumers))
