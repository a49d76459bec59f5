"""CPU tier of the path search (``csrc/paths.hip``, ``include/rgcn_paths.h``): the C surface and every argument check
that runs before a launch, ``ops.PathGraph`` against ``networkx.DiGraph`` built the reference's way, the host
restatement (``paths_reference.py``) the GPU tier holds the device to against ``networkx.all_simple_paths`` and the
reference's float64 score formula, the shared helpers stand-alone under sanitizers, and the prediction CLI's new flags
and JSON shape on a stubbed evaluator."""
import os

import numpy as np
import pytest
import torch

import paths_reference as R
from conftest import ROOT
from primekg_rgcn_linkprediction_amd import _lib, consumers, evaluate, ops
from primekg_rgcn_linkprediction_amd import predict as P



def _nx():
    return pytest.importorskip("networkx")


# ---------------------------------------------------------------------------------- C surface
def test_path_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    A, U, OK = _lib.RGCN_ERR_ARG, _lib.RGCN_ERR_UNSUPPORTED, _lib.RGCN_OK

    # rgcn_edge_cosine(emb, N, d, out_ptr, out_dst, nnz, edge_score, stream)
    def cosine(emb=None, n=10, d=32, ptr=None, dst=None, nnz=5, out=None):
        return lib.rgcn_edge_cosine(emb, n, d, ptr, dst, nnz, out, None)

    assert cosine(d=48) == U and cosine(d=48, emb=8, ptr=8, dst=8, out=8) == U        # d % 32
    assert cosine(d=0) == A and cosine(n=0) == A and cosine(nnz=-1) == A
    assert cosine() == A                                                              # nulls
    for hole in ("emb", "ptr", "dst", "out"):
        assert cosine(**{**dict(emb=8, ptr=8, dst=8, out=8), hole: None}) == A, hole
    assert cosine(nnz=0) == OK and cosine(nnz=0, d=128) == OK                         # nothing launched
    assert cosine(emb=8, ptr=8, dst=8, out=8, n=1 << 31) == U

    # rgcn_paths_topk(out_ptr, out_dst, edge_score, in_ptr, in_src, in_pos, N, nnz, sources, targets, Q, max_len, k, slices,
    #                 nodes, length, score, count, ws, ws_bytes, stream)
    arrays = ("out_ptr", "out_dst", "edge_score", "in_ptr", "in_src", "in_pos", "sources", "targets", "nodes", "length",
              "score", "count")

    def topk(n=10, nnz=5, q=3, max_len=4, k=5, slices=0, ws=None, ws_bytes=0, given=(), **holes):
        p = {name: (8 if name in given or given == "all" else None) for name in arrays}
        p.update(holes)
        return lib.rgcn_paths_topk(p["out_ptr"], p["out_dst"], p["edge_score"], p["in_ptr"], p["in_src"], p["in_pos"], n, nnz,
                                   p["sources"], p["targets"], q, max_len, k, slices, p["nodes"], p["length"], p["score"],
                                   p["count"], ws, ws_bytes, None)

    need = lib.rgcn_paths_workspace_bytes(3, 5, 0)
    assert need > 0
    assert topk() == A                                                                # nulls
    for name in arrays:                                                               # each array on its own
        assert topk(given="all", ws=8, ws_bytes=need, **{name: None}) == A, name
    for max_len in (0, 5, -1):
        assert topk(given="all", ws=8, ws_bytes=need, max_len=max_len) == A and topk(q=0, max_len=max_len) == A
    assert topk(given="all", ws=8, ws_bytes=need, k=0) == A and topk(given="all", ws=8, ws_bytes=need, k=-2) == A
    assert topk(given="all", ws=8, ws_bytes=need, slices=-1) == A and topk(q=0, slices=-1) == A
    assert topk(q=-1) == A and topk(n=0) == A and topk(nnz=-1) == A
    assert topk(given="all", ws=None, ws_bytes=need) == A                             # no workspace
    assert topk(given="all", ws=8, ws_bytes=need - 1) == A                            # short workspace
    assert topk(given="all", ws=8, ws_bytes=1 << 40, k=ops.PATHS_MAX_K + 1) == U      # k above the cap
    assert topk(given="all", ws=8, ws_bytes=1 << 40, n=1 << 31) == U
    assert topk(q=0) == OK and topk(q=0, k=10 ** 6) == OK                             # empty batch: before any pointer
    assert ops.PATHS_MAX_K == 64 and ops.PATHS_MAX_LEN == 4 and ops.PATHS_LDS_IDS >= 64


def test_paths_workspace_is_monotone_and_zero_for_an_empty_batch():
    size = _lib.load().rgcn_paths_workspace_bytes
    assert size(0, 5, 0) == 0 and size(-1, 5, 0) == 0 and size(4, 0, 0) == 0 and size(4, 5, -1) == 0
    assert size(4, ops.PATHS_MAX_K + 1, 0) == 0
    for q in (1, 37, 100, 5000):
        by_k = [size(q, k, 0) for k in (1, 2, 5, 20, 63, 64)]
        assert by_k == sorted(by_k) and 0 < by_k[0] < by_k[-1]
        by_s = [size(q, 5, s) for s in (1, 2, 3, 7, 50, 255, 256, 1000)]
        assert by_s == sorted(by_s) and by_s[0] > 0
        assert by_s[-1] == by_s[-2] == 256 * by_s[0]                                # at most 256 slices are used
        assert by_s[0] <= size(q, 5, 0) <= by_s[-1]
    assert size(20000, 5, 0) == size(20000, 5, 1)                                    # a large batch keeps one slice
    assert size(1, 5, 0) == size(1, 5, 256) and size(100, 5, 0) > size(100, 5, 1)     # a small one is cut up


def test_order_and_search_are_exact_and_clean_under_sanitizers(tmp_path):
    """``tests/paths_order_check.cpp``: the total order and the int32 search the kernels use, stand-alone under
    AddressSanitizer and UndefinedBehaviorSanitizer (their runtimes are linked INTO the program)"""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "paths_order_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", ROOT,
                    os.path.join(ROOT, "tests", "paths_order_check.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.startswith("paths_order_check ok"), done.stdout + done.stderr


# ---------------------------------------------------------------------------------- ops.PathGraph
def _reference_digraph(ei, et, n):
    """the reference's construction: every node, then ``add_edge`` column by column (a later column overwrites)"""
    g = _nx().DiGraph()
    g.add_nodes_from(range(n))
    for u, v, r in zip(ei[0].tolist(), ei[1].tolist(), et.tolist()):
        g.add_edge(u, v, relation=r)
    return g


def test_path_graph_on_cpu_tensors_is_the_reference_digraph():
    ei, et, _ = R.random_case()
    n = R.RANDOM_N
    g, ref = ops.PathGraph(ei, et, n), _reference_digraph(ei, et, n)
    # the case has what it is meant to have: repeated pairs whose relations differ, and self loops
    keys = (ei[0] * n + ei[1]).tolist()
    first = {}
    differing = sum(1 for key, r in zip(keys, et.tolist()) if first.setdefault(key, r) != r)
    assert differing > 5 and int((ei[0] == ei[1]).sum()) > 3 and g.nnz < ei.size(1)
    assert g.out_ptr.dtype == g.in_ptr.dtype == g.in_pos.dtype == torch.int64
    assert g.out_dst.dtype == g.out_rel.dtype == g.in_src.dtype == torch.int32
    assert g.out_ptr.shape == g.in_ptr.shape == (n + 1,) and g.nnz == ref.number_of_edges() == int(g.out_ptr[-1]) == int(g.in_ptr[-1])
    src = torch.repeat_interleave(torch.arange(n), g.out_ptr[1:] - g.out_ptr[:-1])
    mine = {(u, v): r for u, v, r in zip(src.tolist(), g.out_dst.tolist(), g.out_rel.tolist())}
    assert mine == {(u, v): r for u, v, r in ref.edges(data="relation")}
    assert any(u == v for u, v in mine)                                               # self loops are kept
    out_keys = src * n + g.out_dst
    assert bool((out_keys[1:] > out_keys[:-1]).all())                                 # by src, then dst, unique
    # the in arrays are the transpose, in (dst, src) order, and in_pos finds every in-entry among the out-entries
    dst = torch.repeat_interleave(torch.arange(n), g.in_ptr[1:] - g.in_ptr[:-1])
    in_keys = dst * n + g.in_src
    assert bool((in_keys[1:] > in_keys[:-1]).all())
    assert {(u, v) for u, v in zip(g.in_src.tolist(), dst.tolist())} == set(mine)
    assert torch.equal(g.out_dst[g.in_pos].to(torch.int64), dst) and torch.equal(src[g.in_pos], g.in_src.to(torch.int64))
    assert sorted(g.in_pos.tolist()) == list(range(g.nnz))
    # the restatement's structure is the same one
    mine_ref = R.build_graph(ei, et, n)
    assert mine_ref["rel"] == mine and mine_ref["pairs"] == sorted(mine)
    # the hand graph: the pair given twice keeps its last relation
    hei, het, _, _ = R.hand_case()
    hg = ops.PathGraph(hei, het, R.HAND_N)
    assert hg.nnz == len(R.HAND_SCORE) and hg.out_dst[:3].tolist() == [1, 2, 7] and hg.out_rel[0].item() == 2
    empty = ops.PathGraph(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 4)
    assert empty.nnz == 0 and empty.out_ptr.tolist() == [0] * 5 and empty.in_pos.numel() == 0


def test_path_graph_refuses_bad_input():
    ei, et = torch.tensor([[0, 1], [1, 5]]), torch.tensor([0, 1])
    with pytest.raises(IndexError):
        ops.PathGraph(ei, et, 5)
    with pytest.raises(IndexError):
        ops.PathGraph(torch.tensor([[0, -1], [1, 2]]), et, 5)
    with pytest.raises(ValueError):
        ops.PathGraph(ei, et, 2 ** 31)
    with pytest.raises(ValueError):
        ops.PathGraph(ei, et, 0)
    with pytest.raises(ValueError):
        ops.PathGraph(torch.zeros(3, 2, dtype=torch.int64), et, 5)
    with pytest.raises(ValueError):
        ops.PathGraph(ei, torch.zeros(3, dtype=torch.int64), 6)


def test_python_wrappers_check_the_ranges_first_and_have_no_cpu_path():
    ei, et, pairs = R.random_case()
    g = ops.PathGraph(ei, et, R.RANDOM_N)
    es, src, dst = torch.zeros(g.nnz), pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    for k in (0, -1, ops.PATHS_MAX_K + 1):
        with pytest.raises(ValueError, match=f"{ops.PATHS_MAX_K}"):
            ops.paths_topk(g, es, src, dst, k)                                        # (CPU tensors: the range checks come first)
    for max_len in (0, 5):
        with pytest.raises(ValueError, match="max_len"):
            ops.paths_topk(g, es, src, dst, 5, max_len=max_len)
    with pytest.raises(ValueError, match="slices"):
        ops.paths_topk(g, es, src, dst, 5, slices=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.paths_topk(g, es, src, dst, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.edge_cosine(torch.zeros(R.RANDOM_N, 32), g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        consumers.connecting_paths(torch.zeros(R.RANDOM_N, 32), g, [(0, 1)])
    assert "explain" in dir(evaluate.ModelEvaluator)


# ---------------------------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def random_reference():
    """the random case's structure, both ways, and a fixed float32 score per unique edge"""
    ei, et, pairs = R.random_case()
    graph = R.build_graph(ei, et, R.RANDOM_N)
    score = torch.rand(len(graph["pairs"]), generator=torch.Generator().manual_seed(1)).mul(2).sub(1).numpy()
    return graph, _reference_digraph(ei, et, R.RANDOM_N), pairs.tolist(), score


def test_restatement_enumerates_what_networkx_does(random_reference):
    graph, ref, pairs, _ = random_reference
    many = 0
    for max_len in (1, 2, 3, 4):
        for s, t in pairs:
            want = sorted(tuple(p) for p in _nx().all_simple_paths(ref, source=s, target=t, cutoff=max_len)) if s != t else []
            got = sorted(R.enumerate_paths(graph, s, t, max_len))
            assert got == want, (s, t, max_len)
            assert all(len(set(p)) == len(p) and 2 <= len(p) <= max_len + 1 for p in got)
            many += max_len == 4 and len(got) > ops.PATHS_MAX_K
    assert many >= 20                                                                 # most pairs have more than k paths
    assert R.enumerate_paths(graph, 5, 5) == []
    # the hand graph's written-out answer is what the restatement computes
    hei, het, hpairs, hscore = R.hand_case()
    got = R.restate_topk(R.build_graph(hei, het, R.HAND_N), hscore.numpy(), hpairs[:, 0].tolist(), hpairs[:, 1].tolist(), 5)
    for g, w in zip(got, R.hand_answer(5)):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def test_restated_scores_are_the_reference_formula(random_reference):
    """mean of the hops' scores times ``1 / (1 + 0.2 (len(path) - 2))`` in float64 from the same per-edge scores.  Bound:
    at most 5 roundings of 2^-24 relative (three sums, the weight, the product) on a sum of magnitude <= 4 times
    w <= 1: 5 * 4 * 2^-24 = 1.2e-6 < 2e-6"""
    graph, _, pairs, score = random_reference
    nodes, length, got, count = R.restate_topk(graph, score, [p[0] for p in pairs], [p[1] for p in pairs], ops.PATHS_MAX_K)
    worst = checked = 0
    for q in range(len(pairs)):
        ranked = []
        for j in range(ops.PATHS_MAX_K):
            hops = int(length[q, j])
            if hops == 0:
                assert got[q, j] == -np.inf and (nodes[q, j] == -1).all()
                continue
            path = nodes[q, j, :hops + 1].tolist()
            assert (nodes[q, j, hops + 1:] == -1).all() and path[0] == pairs[q][0] and path[-1] == pairs[q][1]
            sims = [float(score[graph["pos"][(u, v)]]) for u, v in zip(path[:-1], path[1:])]
            want = float(np.mean(sims)) * (1.0 / (1.0 + 0.2 * (len(path) - 2)))
            worst = max(worst, abs(float(got[q, j]) - want))
            ranked.append((-float(got[q, j]), hops, path[1:-1]))
            checked += 1
        assert ranked == sorted(ranked) and int((length[q] > 0).sum()) == min(ops.PATHS_MAX_K, int(count[q].sum()))
    assert checked > 1000 and worst <= 2e-6, worst


def test_restatement_counts_but_never_lists_a_nan_path():
    hei, het, hpairs, hscore = R.hand_case()
    graph = R.build_graph(hei, het, R.HAND_N)
    score = hscore.numpy().copy()
    score[graph["pos"][(0, 1)]] = np.nan                                              # every 0 -> 1 -> ... path
    nodes, length, got, count = R.restate_topk(graph, score, [0, 4], [7, 5], 5)
    assert count[0].tolist() == [1, 2, 1, 1] and length[0].tolist() == [2, 1, 0, 0, 0]
    assert nodes[0, 0].tolist() == [0, 2, 7, -1, -1] and nodes[0, 1].tolist() == [0, 7, -1, -1, -1]
    score[graph["pos"][(4, 5)]] = np.nan
    nodes, length, got, count = R.restate_topk(graph, score, [0, 4], [7, 5], 5)
    assert count[1].tolist() == [1, 0, 0, 0] and (length[1] == 0).all() and (got[1] == -np.inf).all()


def test_star_cases_straddle_the_staging_limit():
    for m in (ops.PATHS_LDS_IDS - 1, ops.PATHS_LDS_IDS, ops.PATHS_LDS_IDS + 1):
        ei, et, pairs, n = R.star_case(m)
        g = ops.PathGraph(ei, et, n)
        assert int(g.in_ptr[2] - g.in_ptr[1]) == m == int(g.out_ptr[1] - g.out_ptr[0]) and pairs[:2].tolist() == [[0, 1], [2, 1]]
        graph = R.build_graph(ei, et, n)
        paths = R.enumerate_paths(graph, 0, 1, 3)
        assert 5000 < len(paths) < 50000 and {len(p) for p in paths} == {3, 4}
        # the third query closes out(0), m entries, against a short in(t): many times fewer 64-entry steps over in(t)
        s, t = pairs[2].tolist()
        short = int(g.in_ptr[t + 1] - g.in_ptr[t])
        assert s == 2 and 1 <= short <= 64 and 4 * 1 < (m + 63) // 64
        through_hub = [p for p in R.enumerate_paths(graph, s, t, 3) if p[1] == 0]
        assert len(through_hub) >= 1 and all(len(p) == 4 for p in through_hub)


# ---------------------------------------------------------------------------------- predict.py
class _StubEvaluator:
    """``top_candidates`` from a fixed table and ``explain`` from the restatement on a small random graph, on the CPU"""

    def __init__(self, n=40):
        gen = torch.Generator().manual_seed(5)
        self.table = torch.randn(n, n, generator=gen)
        self.node_class = None
        ei, et = torch.randint(0, n, (2, 300), generator=gen), torch.randint(0, 3, (300,), generator=gen)
        self.graph = R.build_graph(ei, et, n)
        self.score = torch.rand(len(self.graph["pairs"]), generator=gen).numpy()
        self.explained = []

    def top_candidates(self, side, anchors, relations, k, novel=True, candidate_class=None, min_score=None):
        scores, ids = torch.sort(self.table[anchors], dim=1, descending=True, stable=True)
        return ids[:, :k], scores[:, :k]

    def explain(self, pairs, k=5, max_len=4):
        self.explained.append((list(pairs), k, max_len))
        nodes, length, score, count = R.restate_topk(self.graph, self.score, [p[0] for p in pairs], [p[1] for p in pairs], k, max_len)
        paths = [[{"nodes": nodes[q, j, :length[q, j] + 1].tolist(),
                   "relations": [self.graph["rel"][(int(u), int(v))] for u, v in zip(nodes[q, j, :length[q, j]], nodes[q, j, 1:length[q, j] + 1])],
                   "length": int(length[q, j]), "score": float(score[q, j])} for j in range(k) if length[q, j] > 0]
                 for q in range(len(pairs))]
        return paths, count.tolist()


def test_predict_cli_explain_flags_and_json_shape_on_a_stubbed_evaluator(tmp_path):
    base = ["--model_path", "m.pt", "--relation", "1", "--anchors", "3", "5", "--top_k", "4"]
    args = P.parse_args(base)
    assert args.explain == 0 and args.max_path_length == 4
    args = P.parse_args(base + ["--explain", "3", "--max_path_length", "2"])
    assert args.explain == 3 and args.max_path_length == 2
    for bad in (["--max_path_length", "5"], ["--max_path_length", "0"], ["--explain", "-1"], ["--explain", "x"]):
        with pytest.raises(SystemExit):
            P.parse_args(base + bad)
    ev = _StubEvaluator()
    plain = P.predict(ev, P.parse_args(base), None)
    assert ev.explained == [] and set(plain) == {"protocol", "queries"}
    assert set(plain["protocol"]) == {"side", "top_k", "novel", "candidate_class", "anchor_class", "min_score", "order"}
    assert all(set(q) == {"anchor", "relation", "candidates"} for q in plain["queries"])
    # a namespace from before the flags existed gives the same dict
    old = P.parse_args(base)
    del old.explain, old.max_path_length
    assert P.predict(ev, old, None) == plain
    for side in ("tail", "head"):
        ev.explained.clear()
        names = {i: f"node{i}" for i in range(40)}
        result = P.predict(ev, P.parse_args(base + ["--explain", "3", "--max_path_length", "3", "--side", side]), names)
        (pairs, k, max_len), = ev.explained
        assert (k, max_len) == (3, 3) and len(pairs) == 8
        stripped = {"protocol": {k_: v for k_, v in result["protocol"].items() if k_ != "paths"},
                    "queries": [{k_: v for k_, v in q.items() if k_ in ("anchor", "relation", "candidates")} for q in result["queries"]]}
        assert stripped == {"protocol": {**plain["protocol"], "side": side}, "queries": plain["queries"]}
        about = result["protocol"]["paths"]
        assert about["per_candidate"] == 3 and about["max_length"] == 3 and "descending" in about["order"] and "0.2" in about["score"]
        assert about["pair"] == ("(anchor, candidate)" if side == "tail" else "(candidate, anchor)")
        at = 0
        for q in result["queries"]:
            assert len(q["paths"]) == len(q["path_counts"]) == len(q["candidates"]) == 4
            for (cand, _), per_candidate, counts in zip(q["candidates"], q["paths"], q["path_counts"]):
                s, t = (q["anchor"], cand) if side == "tail" else (cand, q["anchor"])
                assert tuple(pairs[at]) == (s, t)
                at += 1
                assert len(counts) == 4 and counts[3] == 0 and len(per_candidate) == min(3, sum(counts))
                for path in per_candidate:
                    assert set(path) == {"nodes", "relations", "length", "score", "node_names"}
                    assert path["nodes"][0] == s and path["nodes"][-1] == t and len(path["relations"]) == path["length"] <= 3
                    assert path["node_names"] == [f"node{i}" for i in path["nodes"]]
        import json
        saved = P.save_predictions(result, tmp_path / side)
        assert json.loads(saved.read_text()) == result
    no_names = P.predict(ev, P.parse_args(base + ["--explain", "1"]), None)
    assert all("node_names" not in path for q in no_names["queries"] for per in q["paths"] for path in per)
