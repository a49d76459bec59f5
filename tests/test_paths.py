"""GPU tier of the path search (``csrc/paths.hip``): ``ops.edge_cosine`` and ``ops.paths_topk`` held to the host
restatement of the contract (``paths_reference.py``; checked against networkx in ``test_paths_host.py``) - nodes,
lengths and counts equal, scores bit for bit, for every ``slices`` - and the layers above them end to end."""
import math

import numpy as np
import pytest
import torch

import paths_reference as R
from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import DrugDiseaseModel, _lib, consumers, ops
from primekg_rgcn_linkprediction_amd import evaluate as E
from primekg_rgcn_linkprediction_amd import predict as P

pytestmark = pytest.mark.gpu


def _host(result):
    return tuple(t.cpu().numpy() for t in result)


def _assert_equal(got, want, what):
    """(nodes, length, score, count) of the device against the restatement's: integers equal, scores the same bits"""
    for name, g, w in zip(("nodes", "length", "score", "count"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if name == "score":
            assert R.same_bits(g, w), (what, name, np.argwhere(g.view(np.int32) != w.view(np.int32))[:5].tolist())
        else:
            assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].tolist())


class _Case:
    """a graph on the device, its restatement-side structure, queries, and restated answers computed once per
    (edge_score, max_len) at k = 64 (the answer for a smaller k is its prefix: the order is total)"""

    def __init__(self, dev, ei, et, pairs, n):
        self.dev, self.n = dev, n
        self.graph = ops.PathGraph(ei.to(dev), et.to(dev), n)
        self.ref = R.build_graph(ei, et, n)
        assert self.graph.nnz == len(self.ref["pairs"])
        self.pairs = pairs
        self.src, self.dst = pairs[:, 0].contiguous().to(dev), pairs[:, 1].contiguous().to(dev)
        self._answers = {}

    def want(self, name, edge_score, k, max_len):
        key = (name, max_len)
        if key not in self._answers:
            self._answers[key] = R.restate_topk(self.ref, edge_score.cpu().numpy(), self.pairs[:, 0].tolist(),
                                                self.pairs[:, 1].tolist(), ops.PATHS_MAX_K, max_len)
        nodes, length, score, count = self._answers[key]
        return nodes[:, :k], length[:, :k], score[:, :k], count

    def run(self, edge_score, k, max_len, slices):
        return _host(ops.paths_topk(self.graph, edge_score, self.src, self.dst, k, max_len, slices))


@pytest.fixture(scope="module")
def random_case():
    dev = need_gpu()
    ei, et, pairs = R.random_case()
    case = _Case(dev, ei, et, pairs, R.RANDOM_N)
    case.emb = {d: R.random_embeddings(d).to(dev) for d in (32, 128)}
    case.cosine = ops.edge_cosine(case.emb[32], case.graph)
    return case


def test_hand_graph_gives_the_written_out_answer():
    dev = need_gpu()
    ei, et, pairs, score = R.hand_case()
    graph = ops.PathGraph(ei.to(dev), et.to(dev), R.HAND_N)
    assert graph.out_rel[0].item() == 2                                             # (0, 1) given twice: the last relation
    src, dst = pairs[:, 0].contiguous().to(dev), pairs[:, 1].contiguous().to(dev)
    for k in (1, 3, 5, 64):                                                         # 64: fewer paths than k, the padding
        for slices in (0, 1, 3):
            got = _host(ops.paths_topk(graph, score.to(dev), src, dst, k, 4, slices))
            _assert_equal(got, R.hand_answer(k), (k, slices))
    nodes, length, sc, count = _host(ops.paths_topk(graph, score.to(dev), src, dst, 64))
    assert (nodes[0, 5:] == -1).all() and (length[0, 5:] == 0).all() and (sc[0, 5:] == -np.inf).all()
    assert (nodes[1] == -1).all() and (length[2] == 0).all() and (sc[1:3] == -np.inf).all()
    # shorter limits: the longer paths are neither listed nor counted
    for max_len in (1, 2, 3):
        got = _host(ops.paths_topk(graph, score.to(dev), src, dst, 5, max_len))
        ref = R.restate_topk(R.build_graph(ei, et, R.HAND_N), score.numpy(), pairs[:, 0].tolist(), pairs[:, 1].tolist(), 5, max_len)
        _assert_equal(got, ref, max_len)
        assert (got[3][:, max_len:] == 0).all() and got[1].max() <= max_len
    # the consumer's dicts: relations are out_rel of each hop
    paths, counts = consumers.connecting_paths(torch.zeros(R.HAND_N, 32, device=dev), graph, pairs.tolist(), k=2,
                                               return_counts=True, edge_score=score.to(dev))
    assert counts == [c for _, _, c in R.HAND_QUERIES]
    assert paths[0] == [{"nodes": [0, 1, 3, 7], "relations": [2, 0, 1], "length": 3, "score": float(np.float32(2.0) * R.path_weight(3))},
                        {"nodes": [0, 1, 3, 2, 7], "relations": [2, 0, 2, 2], "length": 4, "score": 2.75 * 0.15625}]
    assert paths[1] == [] and paths[2] == [] and paths[3] == [{"nodes": [4, 5], "relations": [0], "length": 1, "score": -0.5}]


@pytest.mark.parametrize("max_len", [1, 2, 3, 4])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_random_graph_equals_the_restatement_for_every_slicing(random_case, k, max_len):
    c = random_case
    want = c.want("cosine", c.cosine, k, max_len)
    if max_len == 4:
        assert int((want[3].sum(1) > ops.PATHS_MAX_K).sum()) >= 20                  # the lists really overflow
    first = None
    for slices in (0, 1, 3):
        got = c.run(c.cosine, k, max_len, slices)
        _assert_equal(got, want, (k, max_len, slices))
        if first is None:
            first = got
        for a, b in zip(got, first):                                                # and bit-equal to each other
            assert a.tobytes() == b.tobytes(), (k, max_len, slices)


@pytest.mark.parametrize("d", [32, 128])
def test_edge_cosine_against_float64(random_case, d):
    """|device - float64| <= (d + 6) 2^-24: the dot product's bound relative to |x||y| (d roundings; sum |x_i y_i| <=
    |x||y|), the two norms and the division"""
    c = random_case
    got = ops.edge_cosine(c.emb[d], c.graph).cpu().numpy()
    emb = c.emb[d].cpu().numpy().astype(np.float64)
    u, v = np.array([p[0] for p in c.ref["pairs"]]), np.array([p[1] for p in c.ref["pairs"]])
    norm = np.linalg.norm(emb, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = (emb[u] * emb[v]).sum(1) / (norm[u] * norm[v])
    zero = (u == 3) | (v == 3)                                                      # row 3 is zero
    assert zero.sum() > 10 and np.isnan(want[zero]).all()
    assert got.dtype == np.float32 and (got[zero] == 0.0).all() and not np.signbit(got[zero]).any()
    err = np.abs(got[~zero].astype(np.float64) - want[~zero]).max()
    print(f"edge_cosine d={d}: max error {err:.3e}, bound {(d + 6) * 2.0 ** -24:.3e}")
    assert err <= (d + 6) * 2.0 ** -24, err
    self_loops = (u == v) & ~zero
    assert self_loops.any() and np.abs(got[self_loops] - 1.0).max() <= (d + 6) * 2.0 ** -24


def test_edge_cosine_refuses_other_dims(random_case):
    c = random_case
    with pytest.raises(ValueError):
        ops.edge_cosine(torch.zeros(R.RANDOM_N, 48, device=c.dev), c.graph)
    with pytest.raises(ValueError):
        ops.edge_cosine(torch.zeros(R.RANDOM_N + 1, 32, device=c.dev), c.graph)
    with pytest.raises(IndexError):
        ops.paths_topk(c.graph, c.cosine, torch.tensor([0, R.RANDOM_N], device=c.dev), torch.tensor([1, 2], device=c.dev), 5)
    with pytest.raises(IndexError):
        ops.paths_topk(c.graph, c.cosine, torch.tensor([0, 1], device=c.dev), torch.tensor([-1, 2], device=c.dev), 5)
    empty = ops.paths_topk(c.graph, c.cosine, c.src[:0], c.dst[:0], 5)
    assert [tuple(t.shape) for t in empty] == [(0, 5, 5), (0, 5), (0, 5), (0, 4)]


@pytest.mark.parametrize("k", [5, 64])
def test_all_ties_come_out_by_length_then_nodes(random_case, k):
    """every embedding row identical: every edge score has the same bits, so within a length every path ties and the
    waves and slices meet equal scores in whatever order they run"""
    c = random_case
    same = torch.randn(1, 32, generator=torch.Generator().manual_seed(2)).expand(R.RANDOM_N, 32).contiguous().to(c.dev)
    cosine = ops.edge_cosine(same, c.graph)
    assert torch.unique(cosine.view(torch.int32)).numel() == 1 and abs(float(cosine[0]) - 1.0) < 1e-5
    want = c.want("ties", cosine, k, 4)
    nodes, length = want[0], want[1]
    for q in range(nodes.shape[0]):                                                 # the restatement: (L, nodes) ascending
        rows = [(int(length[q, j]), nodes[q, j, 1:int(length[q, j])].tolist()) for j in range(k) if length[q, j] > 0]
        assert rows == sorted(rows)
    for slices in (1, 3, 7):
        _assert_equal(c.run(cosine, k, 4, slices), want, (k, slices))


@pytest.mark.parametrize("m", [ops.PATHS_LDS_IDS - 1, ops.PATHS_LDS_IDS, ops.PATHS_LDS_IDS + 1])
def test_hubs_across_the_lds_staging_limit(m):
    dev = need_gpu()
    ei, et, pairs, n = R.star_case(m)
    c = _Case(dev, ei, et, pairs, n)
    assert int(c.graph.in_ptr[2] - c.graph.in_ptr[1]) == m == int(c.graph.out_ptr[1] - c.graph.out_ptr[0])
    emb = torch.randn(n, 32, generator=torch.Generator().manual_seed(m)).to(dev)
    cosine = ops.edge_cosine(emb, c.graph)
    want = c.want("cosine", cosine, 5, 3)
    assert 5000 < int(want[3][0].sum()) < 50000 and int(want[3][1].sum()) > 0
    assert int(want[3][2, 2]) > 0                                                   # 2 -> 0 -> a -> b: out(0) against a short in(b)
    first = None
    for slices in (0, 1, 3):
        got = c.run(cosine, 5, 3, slices)
        _assert_equal(got, want, (m, slices))
        first = first or got
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, first))


def test_nan_edge_scores_are_counted_and_never_listed():
    dev = need_gpu()
    ei, et, pairs, score = R.hand_case()
    graph, ref = ops.PathGraph(ei.to(dev), et.to(dev), R.HAND_N), R.build_graph(ei, et, R.HAND_N)
    src, dst = pairs[:, 0].contiguous().to(dev), pairs[:, 1].contiguous().to(dev)
    score = score.clone()
    score[ref["pos"][(0, 1)]] = math.nan                                            # every path of query 0 through node 1
    score[ref["pos"][(4, 5)]] = math.nan                                            # the only path of query 3
    want = R.restate_topk(ref, score.numpy(), pairs[:, 0].tolist(), pairs[:, 1].tolist(), 5)
    assert want[3][0].tolist() == [1, 2, 1, 1] and want[1][0].tolist() == [2, 1, 0, 0, 0]
    assert want[3][3].tolist() == [1, 0, 0, 0] and (want[1][3] == 0).all()
    for slices in (0, 1, 3):
        got = _host(ops.paths_topk(graph, score.to(dev), src, dst, 5, 4, slices))
        _assert_equal(got, want, slices)
        assert not np.isnan(got[2]).any()


def test_ids_outside_the_graph_give_empty_queries_at_the_c_boundary(random_case):
    """the Python wrapper raises first; the entry point itself answers such a query with zero counts and empty slots"""
    c = random_case
    g, k = c.graph, 5
    src = torch.tensor([int(c.pairs[0, 0]), R.RANDOM_N, -1, int(c.pairs[1, 0]), 1 << 40], device=c.dev)
    dst = torch.tensor([int(c.pairs[0, 1]), 0, 0, R.RANDOM_N + 7, -(1 << 40)], device=c.dev)
    q = src.numel()
    nodes = torch.zeros((q, k, 5), dtype=torch.int32, device=c.dev)
    length = torch.full((q, k), 9, dtype=torch.int32, device=c.dev)
    score = torch.zeros((q, k), device=c.dev)
    count = torch.full((q, 4), 9, dtype=torch.int64, device=c.dev)
    lib = _lib.load()
    nbytes = lib.rgcn_paths_workspace_bytes(q, k, 2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=c.dev)
    rc = lib.rgcn_paths_topk(g.out_ptr.data_ptr(), g.out_dst.data_ptr(), c.cosine.data_ptr(), g.in_ptr.data_ptr(),
                             g.in_src.data_ptr(), g.in_pos.data_ptr(), g.num_nodes, g.nnz, src.data_ptr(), dst.data_ptr(), q, 4, k,
                             2, nodes.data_ptr(), length.data_ptr(), score.data_ptr(), count.data_ptr(), ws.data_ptr(), nbytes,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.RGCN_OK
    torch.cuda.synchronize()
    want = c.want("cosine", c.cosine, k, 4)
    assert np.array_equal(nodes[0].cpu().numpy(), want[0][0]) and np.array_equal(count[0].cpu().numpy(), want[3][0])
    assert bool((count[1:] == 0).all()) and bool((length[1:] == 0).all()) and bool((nodes[1:] == -1).all())
    assert bool((score[1:] == -math.inf).all())


def test_explain_and_predict_end_to_end():
    """an untrained model of the reference's layer sizes on a small random graph: ``ModelEvaluator.explain`` and
    ``predict.predict(--explain 3)``"""
    dev = need_gpu()
    n = 300
    gen = torch.Generator().manual_seed(9)
    ei, et = torch.randint(0, n, (2, 3000), generator=gen), torch.randint(0, 3, (3000,), generator=gen)
    torch.manual_seed(0)
    model = DrugDiseaseModel(n, 3, 64, 128)
    data = {"edge_index": ei, "edge_type": et, "num_nodes": n, "num_relations": 3}
    ev = E.ModelEvaluator(model, data, data, dev)
    ref = R.build_graph(ei, et, n)
    pairs = torch.randint(0, n, (12, 2), generator=gen).tolist()

    def check(pairs, paths, counts, k, max_len):
        cosine = ev._edge_cosine.cpu().numpy()
        _, _, _, want_count = R.restate_topk(ref, cosine, [p[0] for p in pairs], [p[1] for p in pairs], k, max_len)
        assert counts == want_count.tolist() and len(paths) == len(pairs)
        for (s, t), per_pair, cnt in zip(pairs, paths, counts):
            assert len(per_pair) == min(k, sum(cnt))
            scores = [p["score"] for p in per_pair]
            assert scores == sorted(scores, reverse=True)
            for p in per_pair:
                nodes = p["nodes"]
                assert nodes[0] == s and nodes[-1] == t and len(set(nodes)) == len(nodes) == p["length"] + 1 <= max_len + 1
                assert p["relations"] == [ref["rel"][(u, v)] for u, v in zip(nodes[:-1], nodes[1:])]   # every hop is an edge
                assert np.float32(p["score"]) == R.path_score(ref, cosine, nodes)

    paths, counts = ev.explain(pairs, k=5, max_len=4)
    graph = ev._path_graph
    check(pairs, paths, counts, 5, 4)
    assert sum(len(p) for p in paths) > 20
    ev.explain(pairs[:2], k=2, max_len=2)
    assert ev._path_graph is graph                                                  # built once
    args = P.parse_args(["--model_path", "m.pt", "--relation", "1", "--anchors", "3", "5", "17", "--top_k", "4", "--explain", "3",
                         "--max_path_length", "3"])
    for side in ("tail", "head"):
        args.side = side
        result = P.predict(ev, args, None)
        plain = P.predict(ev, P.parse_args(["--model_path", "m.pt", "--relation", "1", "--anchors", "3", "5", "17", "--top_k", "4",
                                            "--side", side]), None)
        assert [q["candidates"] for q in result["queries"]] == [q["candidates"] for q in plain["queries"]]
        assert "paths" in result["protocol"] and "paths" not in plain["protocol"]
        for q in result["queries"]:
            qpairs = [(q["anchor"], c) if side == "tail" else (c, q["anchor"]) for c, _ in q["candidates"]]
            check(qpairs, q["paths"], q["path_counts"], 3, 3)
