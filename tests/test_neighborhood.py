"""GPU tier of the pair-neighbourhood statistics (``ops.pair_neighborhood``, ``csrc/neighborhood.hip``): every output is
an integer and every case is compared for exact equality with the host restatement (``neighborhood_reference.py``), which
``test_neighborhood_host.py`` holds to the reference's networkx code."""
import pytest
import torch

import neighborhood_reference as R
from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import DrugDiseaseModel, consumers, ops
from primekg_rgcn_linkprediction_amd import evaluate as E

pytestmark = pytest.mark.gpu


def _run(dev, graph_cpu, src, dst, radius, node_class=None, num_classes=0, common_cap=0):
    cls = None if node_class is None else node_class.to(dev)
    return ops.pair_neighborhood(graph_cpu.to(dev), src.to(dev), dst.to(dev), radius, cls, num_classes, common_cap)


def test_hand_graph_gives_the_written_out_answer():
    dev = need_gpu()
    ei, et, src, dst, node_class = R.hand_case()
    got = _run(dev, ops.PathGraph(ei, et, R.HAND_N), src, dst, R.HAND_RADIUS, node_class, R.HAND_NUM_CLASSES, R.HAND_CAP)
    R.assert_same(got, R.hand_answer(), "hand graph: ")
    assert got.ball.shape == (len(R.HAND_QUERIES), 2, 5) and got.ball.dtype == torch.int64 and got.distance.dtype == torch.int32


@pytest.fixture(scope="module", params=[97, 300])
def zipf(request):
    """the Zipf-endpoint case at N (a partial last bitset word; 4 and 10 words) with its structure and node classes"""
    dev = need_gpu()
    n = request.param
    ei, et, src, dst = R.zipf_case(n, seed=n)
    g = ops.PathGraph(ei, et, n)
    cls = torch.randint(-2, 34, (n,), generator=torch.Generator().manual_seed(n)).to(torch.int32)
    return dev, g, g.to(dev), R.Structure(g), src, dst, cls


@pytest.mark.parametrize("radius", [0, 1, 2, 3, 4])
def test_zipf_graphs_equal_the_restatement(zipf, radius):
    dev, g, g_dev, st, src, dst, cls = zipf
    want = R.restate(st, src.tolist(), dst.tolist(), radius, cls, 3, 64)
    got = ops.pair_neighborhood(g_dev, src.to(dev), dst.to(dev), radius, cls.to(dev), 3, 64)
    R.assert_same(got, want, f"N = {g.num_nodes}, radius {radius}: ")
    if radius == 1:
        assert int(want["common"].max()) > 64 > int(want["common"][want["common"] > 0].min())    # the cap cuts some lists, not all
    if radius >= 2:
        assert -1 in want["distance"] and 0 in want["distance"] and 2 in want["distance"]


@pytest.mark.parametrize("num_classes", [0, 1, 3, 32])
def test_class_counts(zipf, num_classes):
    dev, g, g_dev, st, src, dst, cls = zipf
    assert int(cls.min()) < 0 and int(cls.max()) >= 32                              # negative and too-large classes are present
    want = R.restate(st, src.tolist(), dst.tolist(), 2, cls, num_classes, 0)
    got = ops.pair_neighborhood(g_dev, src.to(dev), dst.to(dev), 2, cls.to(dev), num_classes, 0)
    R.assert_same(got, want, f"{num_classes} classes: ")
    if num_classes:
        assert got.class_count.shape == (src.numel(), num_classes) and int(got.class_count.sum()) > 0
        assert bool((got.class_count.sum(1) <= got.union_nodes).all()) and bool((got.class_count.sum(1) < got.union_nodes).any())
    else:
        assert got.class_count is None and got.common_nodes is None
    without = ops.pair_neighborhood(g_dev, src.to(dev), dst.to(dev), 2, None, num_classes, 0)
    assert without.class_count is None and torch.equal(without.union_edges, got.union_edges)


@pytest.mark.parametrize("m", [ops.NEIGHBORHOOD_HUB_DEGREE - 1, ops.NEIGHBORHOOD_HUB_DEGREE, ops.NEIGHBORHOOD_HUB_DEGREE + 1])
def test_rows_across_the_hub_threshold(m):
    """a long out-row and a long in-row in the first round, long and short rows in one wave in the second, the long
    out-row as a union member of the edge count: one below the threshold (walked by a lane), at it and one above (walked
    by the wave)"""
    dev = need_gpu()
    ei, et, src, dst, n = R.hub_case(m)
    g = ops.PathGraph(ei, et, n)
    cls = (torch.arange(n) % 4).to(torch.int32)
    for radius in (1, 2, 3):
        want = R.restate(g, src.tolist(), dst.tolist(), radius, cls, 4, 16)
        R.assert_same(_run(dev, g, src, dst, radius, cls, 4, 16), want, f"row length {m}, radius {radius}: ")
        assert want["union_edges"][0] >= 2 * m


@pytest.mark.parametrize("cap", R.COMMON_CAPS)
def test_common_nodes_at_and_around_the_cap(cap):
    """intersections of 0, cap - 1, cap and cap + 65 ids (and the other caps' sizes), scattered over 626 bitset words -
    three steps of the 256-word compaction: its prefix sum across waves and steps, its stop at the cap, the -1 padding"""
    dev = need_gpu()
    ei, et, src, dst, n = R.common_case()
    g = ops.PathGraph(ei, et, n)
    want = R.restate(g, src.tolist(), dst.tolist(), 1, None, 0, cap)
    assert {0, cap - 1, cap, cap + 65} <= set(want["common"].tolist()) and n > 2 * 256 * 32
    got = _run(dev, g, src, dst, 1, None, 0, cap)
    R.assert_same(got, want, f"cap {cap}: ")
    filled = (got.common_nodes >= 0).sum(1).cpu()
    assert filled.tolist() == [min(size, cap) for size in R.COMMON_SIZES]


def test_graph_of_the_largest_size():
    """N = rgcn_neighborhood_max_nodes(): the four bitsets fill the dynamic LDS the kernel may ask for; the last node and
    the last bitset word take part"""
    dev = need_gpu()
    n = ops.neighborhood_max_nodes()
    cols = [(n - 1, 0), (0, 5), (5, n - 2), (n - 2, n - 1), (n // 2, n - 1), (n // 2, n // 2), (7, 5), (n - 3, 7), (100000, 7),
            (0, 100000), (n - 1, 262143), (262144, 262143)]
    ei, et = R.columns(cols)
    g = ops.PathGraph(ei, et, n)
    cls = torch.zeros(n, dtype=torch.int32)
    cls[n // 2:] = 1
    src, dst = torch.tensor([n - 1]), torch.tensor([5])
    want = R.restate(g, src.tolist(), dst.tolist(), 2, cls, 2, 8)
    assert want["union_nodes"][0] >= 9 and want["common"][0] >= 3 and n - 1 in want["common_nodes"][0] and n >= 262144
    R.assert_same(_run(dev, g, src, dst, 2, cls, 2, 8), want, "largest graph: ")


def test_empty_graph_and_empty_batch():
    dev = need_gpu()
    none = ops.PathGraph(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 40)
    src, dst = torch.tensor([0, 3, 39, 40]), torch.tensor([0, 4, 39, -1])
    cls = torch.zeros(40, dtype=torch.int32)
    got = _run(dev, none, src, dst, 2, cls, 2, 3)                                  # nnz == 0: nobody is present
    R.assert_same(got, R.restate(none, src.tolist(), dst.tolist(), 2, cls, 2, 3), "nnz == 0: ")
    assert int(got.ball.abs().sum()) == 0 and bool((got.distance == -1).all()) and bool((got.common_nodes == -1).all())
    ei, et, *_ = R.hand_case()
    empty = torch.zeros(0, dtype=torch.int64)
    got = _run(dev, ops.PathGraph(ei, et, R.HAND_N), empty, empty, 2, cls[:R.HAND_N], 2, 3)      # Q == 0
    assert got.ball.shape == (0, 2, 5) and got.distance.shape == (0,) and got.class_count.shape == (0, 2)
    assert got.common_nodes.shape == (0, 3) and got.union_edges.dtype == torch.int64


def test_wrong_devices_and_dtypes_raise():
    dev = need_gpu()
    ei, et, src, dst, cls = R.hand_case()
    g = ops.PathGraph(ei, et, R.HAND_N).to(dev)
    with pytest.raises(TypeError):
        ops.pair_neighborhood(g, src.to(dev).int(), dst.to(dev))
    with pytest.raises(TypeError):
        ops.pair_neighborhood(g, src.to(dev), dst.to(dev), 2, cls.to(dev).long(), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pair_neighborhood(g, src, dst.to(dev))
    with pytest.raises(ValueError):
        ops.pair_neighborhood(g, src.to(dev), dst.to(dev)[:-1])
    with pytest.raises(ValueError):
        ops.pair_neighborhood(g, src.to(dev), dst.to(dev), 2, cls.to(dev)[:-1], 3)


def test_two_calls_give_the_same_bits(zipf):
    dev, g, g_dev, st, src, dst, cls = zipf
    s, t, c = src.to(dev).repeat(8), dst.to(dev).repeat(8), cls.to(dev)
    first = ops.pair_neighborhood(g_dev, s, t, 3, c, 32, 128)
    second = ops.pair_neighborhood(g_dev, s, t, 3, c, 32, 128)
    for name in R.FIELDS:
        assert torch.equal(getattr(first, name), getattr(second, name)), name
    q = src.numel()
    assert torch.equal(first.ball[:q], first.ball[-q:]) and torch.equal(first.common_nodes[:q], first.common_nodes[-q:])


def test_stats_and_failure_analysis_end_to_end():
    """an untrained model of the reference's layer sizes on a 300-node typed random graph:
    ``consumers.pair_subgraph_stats``, ``ModelEvaluator.subgraph_stats`` and ``ModelEvaluator.failure_analysis``"""
    dev = need_gpu()
    n = 300
    gen = torch.Generator().manual_seed(21)
    ei, et = torch.randint(0, n - 4, (2, 900), generator=gen), torch.randint(0, 3, (900,), generator=gen)
    cls = (torch.arange(n) % 3).to(torch.int32)
    names = ["drug", "disease", "gene/protein"]
    torch.manual_seed(3)
    model = DrugDiseaseModel(n, 3, 64, 128)
    data = {"edge_index": ei, "edge_type": et, "num_nodes": n, "num_relations": 3}
    ev = E.ModelEvaluator(model, data, data, dev, node_class=cls)
    pairs = torch.stack([torch.randint(0, 100, (60,), generator=gen) * 3, torch.randint(0, 100, (60,), generator=gen) * 3 + 1], 1)
    pairs[0] = torch.tensor([297, 298])                                           # two untouched nodes
    labels = torch.randint(0, 2, (60,), generator=gen)
    g = ops.PathGraph(ei, et, n)
    want = R.restate(g, pairs[:, 0].tolist(), pairs[:, 1].tolist(), 2, cls, 3, 5)
    stats = consumers.pair_subgraph_stats(g.to(dev), pairs.tolist(), 2, cls, names, 5)
    assert stats == ev.subgraph_stats(pairs.tolist(), 2, names, 5) and len(stats) == 60
    for i, row in enumerate(stats):
        assert set(row) == {"drug_neighborhood_size", "disease_neighborhood_size", "common_neighbors", "subgraph_nodes",
                            "subgraph_edges", "node_type_counts", "degree", "distance", "common_nodes"}
        assert row["drug_neighborhood_size"] == want["ball"][i, 0, 2] and row["disease_neighborhood_size"] == want["ball"][i, 1, 2]
        assert row["common_neighbors"] == want["common"][i] and row["subgraph_nodes"] == want["union_nodes"][i]
        assert row["subgraph_edges"] == want["union_edges"][i]
        assert row["node_type_counts"] == {names[c]: int(k) for c, k in enumerate(want["class_count"][i]) if k}
        assert row["degree"] == {"drug": max(int(want["ball"][i, 0, 1]) - 1, 0), "disease": max(int(want["ball"][i, 1, 1]) - 1, 0)}
        assert row["distance"] == (None if want["distance"][i] < 0 else int(want["distance"][i]))
        assert row["common_nodes"] == [x for x in want["common_nodes"][i].tolist() if x >= 0]
    assert stats[0]["subgraph_nodes"] == 0 and stats[0]["node_type_counts"] == {} and stats[0]["distance"] is None

    out = ev.failure_analysis(pairs.tolist(), labels.tolist(), num_failures=4, num_successes=3, class_names=names, common_cap=5)
    assert ev._path_graph is not None and ev._edge_cosine is not None
    scores = consumers.cosine_pair_scores(ev.embeddings(), pairs[:, 0], pairs[:, 1]).cpu()
    typed = consumers.classify_predictions(scores, labels)
    counts = ops.paths_topk(ev._path_graph, ev._edge_cosine, pairs[:, 0].to(dev), pairs[:, 1].to(dev), 1, 4)[3].cpu().tolist()
    rows = [{**t, "drug_idx": p[0], "disease_idx": p[1], **s, "path_counts": c, "num_paths": sum(c),
             "shortest_path_length": consumers.shortest_path_length(c)} for t, p, s, c in zip(typed, pairs.tolist(), stats, counts)]
    expect = consumers.summarize_failures(rows, 4, 3)
    assert {k: out[k] for k in expect} == expect and out["radius"] == 2 and out["max_path_length"] == 4
    assert out["num_pairs"] == 60 and sum(out["means"][t]["count"] for t in ("FP", "FN", "Correct")) == 60
    assert len(out["successes"]) == 3 and all(r["type"] == "Correct" for r in out["successes"])
    for r in out["failures"] + out["successes"]:
        assert r["shortest_path_length"] == next((i + 1 for i, c in enumerate(r["path_counts"]) if c), None)
