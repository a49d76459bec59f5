"""CPU tier of the pair-neighbourhood statistics (``csrc/neighborhood.hip``, ``include/rgcn_neighborhood.h``): the C
surface and every argument check that runs before a launch, the host restatement (``neighborhood_reference.py``) the GPU
tier holds the device to against a literal transcription of the reference's networkx code, the failure analysis' typing
and summary against the reference's formulas, and the command line's flags and JSON keys on a stubbed evaluator."""
import json
import os
import re
from collections import Counter

import numpy as np
import pytest
import torch

import c_surface as S
import neighborhood_reference as R
from conftest import ROOT
from primekg_rgcn_linkprediction_amd import _lib, consumers, evaluate, ops
from primekg_rgcn_linkprediction_amd import failures as F


def _nx():
    return pytest.importorskip("networkx")


# ---------------------------------------------------------------------------------- C surface
ARRAYS = ("out_ptr", "out_dst", "in_ptr", "in_src", "sources", "targets", "node_class", "ball", "distance", "common",
          "union_nodes", "union_edges", "class_count", "common_nodes")


def _call(lib, n=10, nnz=5, q=3, radius=2, num_classes=0, common_cap=0, given=(), **holes):
    p = {name: (8 if given == "all" or name in given else None) for name in ARRAYS}
    p.update(holes)
    return lib.rgcn_pair_neighborhood(p["out_ptr"], p["out_dst"], p["in_ptr"], p["in_src"], n, nnz, p["sources"], p["targets"],
                                      q, radius, p["node_class"], num_classes, common_cap, p["ball"], p["distance"],
                                      p["common"], p["union_nodes"], p["union_edges"], p["class_count"], p["common_nodes"], None)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    A, U, OK = _lib.RGCN_ERR_ARG, _lib.RGCN_ERR_UNSUPPORTED, _lib.RGCN_OK
    most = lib.rgcn_neighborhood_max_nodes()
    assert most >= 262144 and most == ops.neighborhood_max_nodes()
    assert 4 * ((most + 31) // 32) * 4 <= 160 * 1024                              # four bitsets in one CU's LDS

    call = lambda **kw: _call(lib, **kw)
    assert call() == A                                                            # nulls
    # every array that is needed, on its own (node_class may always be NULL; the optional outputs are not produced here)
    for name in ARRAYS:
        if name not in ("node_class", "class_count", "common_nodes"):
            assert call(given="all", **{name: None}) == A, name
    assert call(given="all", nnz=0, out_dst=None, in_src=None, n=most + 1) == U    # reaches the size check: no NULL complaint
    assert call(nnz=0, given=("out_ptr", "in_ptr", "sources", "targets", "ball", "distance", "common", "union_nodes",
                              "union_edges"), n=most + 1) == U
    assert call(given="all", num_classes=3, class_count=None) == A                # produced, so needed
    assert call(given="all", num_classes=3, class_count=None, node_class=None, n=most + 1) == U   # not produced
    assert call(given="all", num_classes=0, class_count=None, n=most + 1) == U
    assert call(given="all", common_cap=4, common_nodes=None) == A
    assert call(given="all", common_cap=0, common_nodes=None, n=most + 1) == U
    # ranges: with and without queries
    for bad in (dict(radius=-1), dict(radius=5), dict(num_classes=-1), dict(num_classes=33), dict(common_cap=-1),
                dict(common_cap=1025), dict(n=0), dict(n=-3), dict(nnz=-1)):
        assert call(given="all", **bad) == A and call(q=0, **bad) == A, bad
    assert call(q=-1) == A and call(given="all", q=-1) == A
    # the size bound
    assert call(given="all", n=most + 1) == U and call(given="all", n=1 << 31) == U
    # an empty batch: before any pointer, and before the size bound
    assert call(q=0) == OK and call(q=0, n=most + 1) == OK and call(q=0, radius=4, num_classes=32, common_cap=1024) == OK
    assert (ops.NEIGHBORHOOD_MAX_RADIUS, ops.NEIGHBORHOOD_MAX_CLASSES, ops.NEIGHBORHOOD_MAX_COMMON) == (4, 32, 1024)


def test_header_and_table_agree():
    """names, parameters, return types and exports: test_c_surface.py, for every header.  Here: the limits the header
    states and the wrappers mirror, and the build list"""
    header = S.header_text("rgcn_neighborhood.h")
    for macro, value in (("HUB_DEGREE", ops.NEIGHBORHOOD_HUB_DEGREE), ("MAX_RADIUS", ops.NEIGHBORHOOD_MAX_RADIUS),
                         ("MAX_CLASSES", ops.NEIGHBORHOOD_MAX_CLASSES), ("MAX_COMMON", ops.NEIGHBORHOOD_MAX_COMMON)):
        assert re.search(rf"#define RGCN_NEIGHBORHOOD_{macro} {value}\n", header), macro
    assert ops.NEIGHBORHOOD_HUB_DEGREE >= 64                                        # a hub row fills a wave at least once
    makefile = open(os.path.join(ROOT, "primekg_rgcn_linkprediction_amd", "csrc", "Makefile")).read()
    assert " neighborhood.hip" in makefile


def test_python_wrapper_checks_the_ranges_first_and_has_no_cpu_path():
    ei, et, src, dst, node_class = R.hand_case()
    g = ops.PathGraph(ei, et, R.HAND_N)
    for kw, word in ((dict(radius=-1), "radius"), (dict(radius=5), "radius"), (dict(num_classes=33), "num_classes"),
                     (dict(num_classes=-1), "num_classes"), (dict(common_cap=1025), "common_cap"), (dict(common_cap=-1), "common_cap")):
        with pytest.raises(ValueError, match=word):
            ops.pair_neighborhood(g, src, dst, **kw)                                # (CPU tensors: the range checks come first)
    with pytest.raises(TypeError):
        ops.pair_neighborhood("graph", src, dst)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pair_neighborhood(g, src, dst)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        consumers.pair_subgraph_stats(g, [(0, 3)])
    assert {"subgraph_stats", "failure_analysis"} <= set(dir(evaluate.ModelEvaluator))
    assert ops.PairNeighborhood._fields == R.FIELDS


# ---------------------------------------------------------------------------------- the restatement
def test_hand_answer_is_what_the_restatement_computes():
    ei, et, src, dst, node_class = R.hand_case()
    got = R.restate(ops.PathGraph(ei, et, R.HAND_N), src.tolist(), dst.tolist(), R.HAND_RADIUS, node_class, R.HAND_NUM_CLASSES,
                    R.HAND_CAP)
    want = R.hand_answer()
    for name in R.FIELDS:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name


def _reference_case():
    """70 nodes, 160 columns: 150 random ones over the first 65 nodes, five of them given again, five self loops; the
    last five nodes are never named"""
    gen = torch.Generator().manual_seed(11)
    n, live = 70, 65
    ei = torch.randint(0, live, (2, 160), generator=gen)
    ei[:, 150:155] = ei[:, 10:15]                                                  # duplicate columns
    loops = torch.randint(0, live, (5,), generator=gen)
    ei[:, 155:] = loops                                                            # self loops
    return ei, torch.randint(0, 3, (160,), generator=gen), n


def _analyze_subgraph(nx_graph, node_types, drug_idx, disease_idx, radius):
    """``analyze_failures.analyze_subgraph``'s set code, statement for statement (without its path search)"""
    drug_neighbors = set()
    disease_neighbors = set()
    if drug_idx in nx_graph:
        drug_neighbors.add(drug_idx)
        for _ in range(radius):
            new_neighbors = set()
            for node in list(drug_neighbors):
                if node in nx_graph:
                    new_neighbors.update(nx_graph.successors(node))
                    new_neighbors.update(nx_graph.predecessors(node))
            drug_neighbors.update(new_neighbors)
    if disease_idx in nx_graph:
        disease_neighbors.add(disease_idx)
        for _ in range(radius):
            new_neighbors = set()
            for node in list(disease_neighbors):
                if node in nx_graph:
                    new_neighbors.update(nx_graph.successors(node))
                    new_neighbors.update(nx_graph.predecessors(node))
            disease_neighbors.update(new_neighbors)
    common_neighbors = drug_neighbors & disease_neighbors
    all_nodes = drug_neighbors | disease_neighbors
    subgraph = nx_graph.subgraph(all_nodes)
    node_type_counts = Counter()
    for node in all_nodes:
        node_type_counts[node_types.get(node, "unknown")] += 1
    return {"drug_neighborhood_size": len(drug_neighbors), "disease_neighborhood_size": len(disease_neighbors),
            "common_neighbors": len(common_neighbors), "subgraph_nodes": len(all_nodes),
            "subgraph_edges": subgraph.number_of_edges(), "node_type_counts": dict(node_type_counts),
            "common": sorted(common_neighbors)}


def test_restatement_is_the_reference_networkx_code():
    nx = _nx()
    ei, et, n = _reference_case()
    nx_graph = nx.DiGraph()
    for u, v, r in zip(ei[0].tolist(), ei[1].tolist(), et.tolist()):               # the reference's construction
        nx_graph.add_edge(u, v, relation=r)
    graph = ops.PathGraph(ei, et, n)
    assert graph.nnz == nx_graph.number_of_edges() < 160 and nx_graph.number_of_nodes() <= n - 5
    assert nx.number_of_selfloops(nx_graph) >= 3
    st = R.Structure(graph)
    cls = torch.randint(-1, 4, (n,), generator=torch.Generator().manual_seed(2)).to(torch.int32)   # -1 and 3: counted nowhere
    node_types = {i: f"type{c}" for i, c in enumerate(cls.tolist()) if 0 <= c < 3}
    pairs = [(s, t) for s in range(n) for t in range(s % 7, n, 7)]
    assert len(pairs) == 700 and any(s == t for s, t in pairs)
    checked = 0
    for radius in (0, 1, 2, 3):
        got = R.restate(st, [p[0] for p in pairs], [p[1] for p in pairs], radius, cls, 3, 8)
        for i, (s, t) in enumerate(pairs):
            want = _analyze_subgraph(nx_graph, node_types, s, t, radius)
            mine = {"drug_neighborhood_size": int(got["ball"][i, 0, radius]), "disease_neighborhood_size": int(got["ball"][i, 1, radius]),
                    "common_neighbors": int(got["common"][i]), "subgraph_nodes": int(got["union_nodes"][i]),
                    "subgraph_edges": int(got["union_edges"][i])}
            assert mine == {k: want[k] for k in mine}, (radius, s, t)
            counted = {f"type{c}": int(k) for c, k in enumerate(got["class_count"][i]) if k}
            unknown = mine["subgraph_nodes"] - sum(counted.values())
            assert {**counted, **({"unknown": unknown} if unknown else {})} == want["node_type_counts"], (radius, s, t)
            assert [x for x in got["common_nodes"][i].tolist() if x >= 0] == want["common"][:8]
            assert (got["ball"][i, :, radius + 1:] == 0).all() and (np.diff(got["ball"][i, :, :radius + 1], axis=1) >= 0).all()
            # the distance: networkx's own shortest path over the undirected view, when it is short enough
            if s in nx_graph and t in nx_graph and nx.has_path(nx_graph.to_undirected(as_view=True), s, t):
                hops = nx.shortest_path_length(nx_graph.to_undirected(as_view=True), s, t)
            else:
                hops = None
            assert int(got["distance"][i]) == (hops if hops is not None and hops <= radius else -1), (radius, s, t)
            checked += 1
    assert checked == 2800


def test_shared_cases_have_what_they_are_meant_to_have():
    hub = ops.NEIGHBORHOOD_HUB_DEGREE
    for m in (hub - 1, hub, hub + 1):
        ei, et, src, dst, n = R.hub_case(m)
        g = ops.PathGraph(ei, et, n)
        out_len, in_len = (g.out_ptr[1:] - g.out_ptr[:-1]), (g.in_ptr[1:] - g.in_ptr[:-1])
        assert int(out_len[0]) == m == int(in_len[m + 1]) == int(in_len[m + 2]) == int(out_len[m + 3])
        assert int(out_len.max()) == m == int(in_len.max()) and int(((out_len == m) | (in_len == m)).sum()) == 4
        assert int(((out_len == 0) & (in_len == 0)).sum()) == 3
        want = R.restate(g, src.tolist(), dst.tolist(), 1)
        assert want["ball"][0, :, 1].tolist() == [m + 1, m + 1] and want["common"][0] == m and want["union_edges"][0] >= 2 * m
    for n in (97, 300):
        ei, et, src, dst = R.zipf_case(n, seed=n)
        g = ops.PathGraph(ei, et, n)
        deg = (g.out_ptr[1:] - g.out_ptr[:-1]) + (g.in_ptr[1:] - g.in_ptr[:-1])
        assert int((deg[-5:] != 0).sum()) == 0 and int(deg.max()) > 100 and g.nnz < 1500        # isolated nodes, a hub, duplicates
        src_row = torch.repeat_interleave(torch.arange(n), g.out_ptr[1:] - g.out_ptr[:-1])
        assert int((src_row == g.out_dst).sum()) >= 3                              # self loops
        assert int((src == dst).sum()) >= 2 and int(((src < 0) | (src >= n) | (dst < 0) | (dst >= n)).sum()) >= 4
        assert src[-1] == src[-2] and dst[-1] == dst[-2] and n % 32 != 0
    ei, et, src, dst, n = R.common_case()
    want = R.restate(ops.PathGraph(ei, et, n), src.tolist(), dst.tolist(), 1)
    assert want["common"].tolist() == R.COMMON_SIZES == [0, 1, 63, 64, 66, 129, 1023, 1024, 1089]


# ---------------------------------------------------------------------------------- failure analysis
def test_typing_and_confidence_error_are_the_reference_formulas():
    scores = [0.0, 0.1, 0.3, 0.3, 0.5, 0.5, 0.7, 0.7, 0.29999, 0.70001, 0.9, 0.9, 0.50001, 0.6, 1.0, 1.0]
    labels = [0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1]
    rows = consumers.classify_predictions(torch.tensor(scores, dtype=torch.float64), torch.tensor(labels))
    assert len(rows) == len(scores)
    for row, score, label in zip(rows, scores, labels):
        # analyze_failures.py:301-328, as written there
        error = abs(score - label)
        if label == 0 and score > 0.7:
            confidence_error = score
        elif label == 1 and score < 0.3:
            confidence_error = 1 - score
        else:
            confidence_error = 0
        kind = 'FP' if (label == 0 and score > 0.5) else ('FN' if (label == 1 and score <= 0.5) else 'Correct')
        assert row == {"prediction": score, "ground_truth": label, "error": error, "confidence_error": confidence_error,
                       "type": kind}
    by_case = {(r["prediction"], r["ground_truth"]): (r["type"], r["confidence_error"]) for r in rows}
    assert by_case[(0.3, 1)] == ("FN", 0) and by_case[(0.29999, 1)] == ("FN", 1 - 0.29999)      # 0.3 itself is not "below 0.3"
    assert by_case[(0.7, 0)] == ("FP", 0) and by_case[(0.70001, 0)] == ("FP", 0.70001)          # nor 0.7 "above 0.7"
    assert by_case[(0.5, 1)] == ("FN", 0) and by_case[(0.5, 0)] == ("Correct", 0) and by_case[(0.50001, 0)] == ("FP", 0)
    assert by_case[(0.7, 1)] == ("Correct", 0) and by_case[(0.3, 0)] == ("Correct", 0)
    with pytest.raises(ValueError):
        consumers.classify_predictions([0.5], [0, 1])
    assert consumers.shortest_path_length([0, 0, 3, 1]) == 3 and consumers.shortest_path_length([0, 0, 0, 0]) is None
    assert consumers.shortest_path_length([2, 0, 0, 0]) == 1


def test_summary_selects_and_compares_as_the_reference_does():
    scores = [0.95, 0.8, 0.75, 0.2, 0.1, 0.6, 0.9, 0.05, 0.55, 0.45, 0.8]
    labels = [0, 0, 0, 1, 1, 0, 1, 0, 1, 0, 0]
    rows = consumers.classify_predictions(scores, labels)
    for i, row in enumerate(rows):
        row.update(drug_idx=i, disease_idx=100 + i, drug_neighborhood_size=10 * i, disease_neighborhood_size=i, common_neighbors=i % 3,
                   subgraph_nodes=11 * i, subgraph_edges=5 * i, num_paths=i * i)
    out = consumers.summarize_failures(rows, num_failures=3, num_successes=2)
    # the reference's selection, as written there (analyze_failures.py:331-339)
    results = sorted(rows, key=lambda x: x['confidence_error'], reverse=True)
    failures = [r for r in results if r['type'] in ['FP', 'FN']][:3]
    correct = [r for r in results if r['type'] == 'Correct']
    successes = sorted(correct, key=lambda x: abs(x['prediction'] - 0.5), reverse=True)[:2]
    assert out["failures"] == failures and out["successes"] == successes
    assert [r["drug_idx"] for r in failures] == [0, 4, 1]                         # 0.95, 1 - 0.1, then the first of the two 0.8
    assert [r["drug_idx"] for r in successes] == [7, 6]
    failed = [r for r in rows if r["type"] != "Correct"]
    okay = [r for r in rows if r["type"] == "Correct"]
    assert out["num_pairs"] == 11 and out["means"]["failure"]["count"] == len(failed) == 7 and out["means"]["success"]["count"] == 4
    assert {t: out["means"][t]["count"] for t in ("FP", "FN", "Correct")} == {"FP": 5, "FN": 2, "Correct": 4}
    mean = lambda group, key: sum(r[key] for r in group) / len(group)
    assert out["differences"] == {
        "drug_neighborhood_diff": mean(okay, "drug_neighborhood_size") - mean(failed, "drug_neighborhood_size"),
        "disease_neighborhood_diff": mean(okay, "disease_neighborhood_size") - mean(failed, "disease_neighborhood_size"),
        "common_neighbors_diff": mean(okay, "common_neighbors") - mean(failed, "common_neighbors"),
        "path_count_diff": mean(okay, "num_paths") - mean(failed, "num_paths")}
    alone = consumers.summarize_failures([r for r in rows if r["type"] == "Correct"])
    assert set(alone["differences"].values()) == {None} and alone["failures"] == [] and alone["means"]["FP"]["num_paths"] is None


# ---------------------------------------------------------------------------------- the command line
STAT_KEYS = {"drug_neighborhood_size", "disease_neighborhood_size", "common_neighbors", "subgraph_nodes", "subgraph_edges",
             "node_type_counts", "degree", "distance", "common_nodes"}
ROW_KEYS = STAT_KEYS | {"drug_idx", "disease_idx", "prediction", "ground_truth", "error", "confidence_error", "type",
                        "path_counts", "num_paths", "shortest_path_length"}


class _StubEvaluator:
    """``failure_analysis`` from the restatement and fixed scores on a small typed random graph, on the CPU"""

    def __init__(self, n=60):
        gen = torch.Generator().manual_seed(9)
        self.num_nodes = n
        self.node_class = (torch.arange(n) % 3).to(torch.int32)                   # 0 drug, 1 disease, 2 gene
        self.full_edge_index = torch.randint(0, n, (2, 400), generator=gen)
        self.full_edge_type = torch.zeros(400, dtype=torch.int64)
        self.graph = ops.PathGraph(self.full_edge_index, self.full_edge_type, n)
        self.calls = []

    def failure_analysis(self, pairs, labels, radius=2, num_failures=5, num_successes=5, class_names=None, common_cap=0,
                         max_len=4):
        self.calls.append((list(pairs), list(labels), radius, num_failures, num_successes, common_cap))
        res = R.restate(self.graph, [p[0] for p in pairs], [p[1] for p in pairs], radius, self.node_class, 3, common_cap)
        names = consumers._class_names(class_names, 3)
        scores = [((7 * p[0] + 3 * p[1]) % 20) / 19 for p in pairs]
        rows = consumers.classify_predictions(scores, labels)
        for i, (row, (s, t)) in enumerate(zip(rows, pairs)):
            count = [int(s != t and (s + t) % 2 == 0), (s + t) % 3, 0, 0]
            row.update(drug_idx=s, disease_idx=t, drug_neighborhood_size=int(res["ball"][i, 0, radius]),
                       disease_neighborhood_size=int(res["ball"][i, 1, radius]), common_neighbors=int(res["common"][i]),
                       subgraph_nodes=int(res["union_nodes"][i]), subgraph_edges=int(res["union_edges"][i]),
                       node_type_counts={names[c]: int(k) for c, k in enumerate(res["class_count"][i]) if k},
                       degree={"drug": 0, "disease": 0}, distance=None,
                       common_nodes=[] if res["common_nodes"] is None else [x for x in res["common_nodes"][i].tolist() if x >= 0],
                       path_counts=count, num_paths=sum(count), shortest_path_length=consumers.shortest_path_length(count))
        out = consumers.summarize_failures(rows, num_failures, num_successes)
        out["radius"], out["max_path_length"] = radius, max_len
        return out


def test_failures_cli_flags_and_json_keys_on_a_stubbed_evaluator(tmp_path):
    base = ["--model_path", "m.pt"]
    with pytest.raises(SystemExit):
        F.parse_args(base)                                                         # the sampler needs the node classes
    args = F.parse_args(base + ["--node_types", "types.npz"])
    assert (args.radius, args.num_samples, args.seed, args.pairs, args.data_dir) == (2, 5000, 42, None, "data/processed")
    assert (args.num_failures, args.num_successes) == (5, 5)
    for bad in (["--radius", "5"], ["--radius", "-1"], ["--num_samples", "1"], ["--radius", "x"], ["--common_nodes", "1025"]):
        with pytest.raises(SystemExit):
            F.parse_args(base + ["--node_types", "types.npz"] + bad)
    ev = _StubEvaluator()
    # the sampler: seeded, half positive, positives through a gene, not the global numpy state
    args = F.parse_args(base + ["--node_types", "types.npz", "--num_samples", "80", "--seed", "3", "--radius", "1",
                                "--drug_class", "0", "--disease_class", "1", "--gene_class", "2", "--common_nodes", "4"])
    np.random.seed(0)
    result = F.analyze(ev, args, class_names=["drug", "disease", "gene/protein"])
    (pairs, labels, radius, nf, ns, cap), = ev.calls
    assert (radius, nf, ns, cap) == (1, 5, 5, 4) and len(pairs) == 80 and sum(labels) == 40 and labels[:40] == [1] * 40
    cls, ei = ev.node_class.tolist(), ev.full_edge_index
    edges = set(zip(ei[0].tolist(), ei[1].tolist()))
    for (drug, disease), label in zip(pairs, labels):
        assert cls[drug] == 0 and cls[disease] == 1
        if label:
            assert any((drug, g) in edges and (g, disease) in edges for g in range(ev.num_nodes) if cls[g] == 2)
    np.random.seed(12345)
    again = F.sample_labelled_pairs(ei, ev.node_class, 0, 1, 2, 80, seed=3)
    assert again[0].tolist() == [list(p) for p in pairs] and again[1].tolist() == labels
    assert F.sample_labelled_pairs(ei, ev.node_class, 0, 1, 2, 80, seed=4)[0].tolist() != again[0].tolist()
    no_genes = F.sample_labelled_pairs(ei, ev.node_class, 0, 1, 7, 10, seed=1)
    assert no_genes[1].tolist() == [0] * 10
    # the document
    assert set(result) == {"protocol", "num_pairs", "means", "differences", "failures", "successes", "max_path_length"}
    assert result["num_pairs"] == 80 and result["protocol"]["radius"] == 1 and result["protocol"]["seed"] == 3
    assert result["protocol"]["positives"] == result["protocol"]["negatives"] == 40
    assert result["protocol"]["classes"] == {"drug": 0, "disease": 1, "gene": 2}
    assert set(result["differences"]) == {"drug_neighborhood_diff", "disease_neighborhood_diff", "common_neighbors_diff",
                                          "path_count_diff"}
    assert set(result["means"]) == {"FP", "FN", "Correct", "failure", "success"}
    assert 0 < len(result["failures"]) <= 5 and 0 < len(result["successes"]) <= 5
    for row in result["failures"] + result["successes"]:
        assert set(row) == ROW_KEYS and set(row["node_type_counts"]) <= {"drug", "disease", "gene/protein"}
        assert len(row["common_nodes"]) <= 4
    assert all(r["type"] in ("FP", "FN") for r in result["failures"]) and all(r["type"] == "Correct" for r in result["successes"])
    saved = F.save_analysis(result, tmp_path / "out")
    assert saved.name == "failure_analysis.json" and json.loads(saved.read_text()) == result
    # class ids by name; labelled pairs from a file, with names
    ev.calls.clear()
    by_name = F.analyze(ev, F.parse_args(base + ["--node_types", "types.npz", "--num_samples", "80", "--seed", "3"]),
                        class_names=["drug", "disease", "gene/protein"])
    assert ev.calls[0][0] == pairs and by_name["protocol"]["classes"] == {"drug": 0, "disease": 1, "gene": 2}
    with pytest.raises(ValueError, match="drug_class"):
        F.analyze(ev, F.parse_args(base + ["--node_types", "types.npz"]), class_names=None)
    np.savez(tmp_path / "pairs.npz", drug=np.array([0, 3, 6]), disease=np.array([1, 4, 7]), label=np.array([1, 0, 1]))
    ev.calls.clear()
    args = F.parse_args(base + ["--pairs", str(tmp_path / "pairs.npz"), "--radius", "3"])
    from_file = F.analyze(ev, args, names={i: f"node{i}" for i in range(60)})
    assert ev.calls[0][:3] == ([[0, 1], [3, 4], [6, 7]], [1, 0, 1], 3) and from_file["protocol"]["pairs"].endswith("pairs.npz")
    assert all(r["drug_name"] == f"node{r['drug_idx']}" and r["disease_name"] == f"node{r['disease_idx']}"
               for r in from_file["failures"] + from_file["successes"])
    np.savez(tmp_path / "short.npz", drug=np.array([0]), disease=np.array([1]))
    with pytest.raises(ValueError, match="label"):
        F.load_pairs(tmp_path / "short.npz")
