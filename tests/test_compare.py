"""The method comparison (``primekg_rgcn_linkprediction_amd/compare.py``): the command line's flags and the two result
files without a GPU, and on the GPU the whole run on the synthetic data the other command lines are tested with - every
method through one ranking protocol, the degree baseline's ranks against a host restatement."""
import json

import numpy as np
import pytest
import torch

from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import compare as C
from primekg_rgcn_linkprediction_amd import evaluate, synth


def test_flags_and_result_files_without_a_gpu(tmp_path):
    args = C.parse_args(["--methods", "random", "transe", "--transe_epochs", "3", "--seed", "5", "--filtered", "--both_sides"])
    assert args.methods == ["random", "transe"] and (args.transe_epochs, args.seed) == (3, 5)
    assert args.filtered and args.both_sides and not args.type_constrained and args.k_values == [1, 5, 10, 20, 50]
    assert C.parse_args(["--model_path", "m.pt", "--node_types", "t.npz"]).methods == ["random", "degree", "rgcn"]
    for bad in (["--methods", "rgcn"], ["--methods", "degree"], ["--methods", "random", "--type_constrained"],
                ["--methods", "walk"], ["--methods", "random", "--transe_epochs", "-1"]):
        with pytest.raises(SystemExit):
            C.parse_args(bad)
    ranks = torch.tensor([1, 2, 10, 51, 4])
    m = C.ranking_metrics(ranks)
    assert m["mrr"] == pytest.approx(np.mean([1, 1 / 2, 1 / 10, 1 / 51, 1 / 4])) and m["median_rank"] == 4.0
    assert (m["hits@1"], m["hits@5"], m["hits@10"], m["hits@20"], m["hits@50"]) == (0.2, 0.6, 0.8, 0.8, 0.8)
    cls = {"auc_roc": 0.75, "auc_pr": 0.7, "precision": 1.0, "recall": 0.5, "f1_score": 2 / 3, "threshold": 0.5}
    result = {"protocol": {"filtered": True, "type_constrained": False, "sides": "both", "test_triples": 5},
              "methods": {"random": {"ranking": m, "classification": cls, "fit_seconds": 0.0},
                          "transe": {"ranking": m, "classification": cls, "fit_seconds": 1.5}}}
    path = C.save_comparison(result, tmp_path / "out")
    assert json.loads(path.read_text()) == result
    table = (tmp_path / "out" / "comparison_table.md").read_text()
    assert "| Method | AUC-ROC | AP | MRR | H@1 | H@10 | H@50 |" in table and "| transe | 0.7500 | 0.7000 |" in table
    assert "compare_methods" in dir(evaluate.ModelEvaluator)
    with pytest.raises(ValueError, match="rgcn"):
        C.compare_methods({}, {}, {"num_nodes": 4}, "cpu", methods=("rgcn",))
    with pytest.raises(ValueError, match="unknown"):
        C.compare_methods({}, {}, {"num_nodes": 4}, "cpu", methods=("walk",))


@pytest.mark.gpu
def test_compare_cli_end_to_end_on_synthetic_data(tmp_path):
    dev = need_gpu()
    from primekg_rgcn_linkprediction_amd import train as T
    tr, va, full, te = T.synthetic_data(num_edges=20000, seed=4)
    num_test = te["edge_index"].size(1)
    assert 100 <= num_test <= 1000                                                 # a few hundred queries per side
    data_dir = tmp_path / "processed"
    data_dir.mkdir()
    for name, d in (("train_data.pt", tr), ("val_data.pt", va), ("test_data.pt", te), ("full_graph.pt", full)):
        torch.save(d, data_dir / name)
    classes = synth.primekg_like_node_classes()                                    # 0 disease, 1 drug, 2 gene
    np.savez(tmp_path / "types.npz", node_class=classes.numpy())
    T.main(["--data_dir", str(data_dir), "--output_dir", str(tmp_path / "out"), "--epochs", "1", "--lr", "0.01"])
    result = C.main(["--data_dir", str(data_dir), "--model_path", str(tmp_path / "out" / "models" / "final_model.pt"),
                     "--node_types", str(tmp_path / "types.npz"), "--methods", "random", "degree", "transe", "rgcn",
                     "--filtered", "--type_constrained", "--both_sides", "--transe_epochs", "2", "--seed", "3",
                     "--drug_class", "1", "--disease_class", "0", "--output_dir", str(tmp_path / "cmp")])
    saved = json.loads((tmp_path / "cmp" / "comparison.json").read_text())
    assert saved == result and list(saved["methods"]) == ["random", "degree", "transe", "rgcn"]
    assert saved["protocol"]["sides"] == "both" and saved["protocol"]["filtered"] and saved["protocol"]["test_triples"] == num_test
    for name, m in saved["methods"].items():
        assert set(m["ranking"]) == {"mrr", "mean_rank", "median_rank", "hits@1", "hits@5", "hits@10", "hits@20", "hits@50"}
        assert set(m["classification"]) == {"auc_roc", "auc_pr", "precision", "recall", "f1_score", "threshold"}
        assert 0 < m["ranking"]["mrr"] <= 1 and 1 <= m["ranking"]["mean_rank"] <= full["num_nodes"]
    assert len(saved["methods"]["transe"]["epoch_losses"]) == 2
    assert "| rgcn |" in (tmp_path / "cmp" / "comparison_table.md").read_text()
    # the degree baseline's ranks under the protocol, restated on the host: among the unknown entities of the true
    # answer's class, those with a strictly larger product of the two degree factors
    only = C.compare_methods(tr, te, full, dev, None, classes, ("degree",), filtered=True, type_constrained=True,
                             drug_class=1, disease_class=0)
    n, cls = full["num_nodes"], classes.numpy()
    deg = np.bincount(tr["edge_index"].numpy().reshape(-1), minlength=n).astype(np.float64)
    drug = np.where(cls == 1, deg / deg[cls == 1].max(), 0.01)
    dis = np.where(cls == 0, deg / deg[cls == 0].max(), 0.01)
    known = {}
    for u, v, k in zip(*(torch.cat([full["edge_index"], te["edge_index"]], 1).tolist()),
                       torch.cat([full["edge_type"], te["edge_type"]]).tolist()):
        known.setdefault((u, k), []).append(v)
    ranks = []
    for h, t, r in zip(te["edge_index"][0].tolist(), te["edge_index"][1].tolist(), te["edge_type"].tolist()):
        score = np.float32(drug[h]) * dis.astype(np.float32)
        ok = (cls == cls[t]) & (np.arange(n) != t)
        ok[[c for c in known.get((h, r), []) if c != t]] = False
        ranks.append(1 + int((ok & (score > score[t])).sum()))
    assert only["methods"]["degree"]["ranking"] == C.ranking_metrics(torch.tensor(ranks))
