"""Method comparison on the HIP path: counterpart of the reference's ``src/compare_methods.py`` minus its plots.

    python -m primekg_rgcn_linkprediction_amd.compare --data_dir data/processed --model_path out/models/best_model.pt \\
        --node_types data/processed/mappings.pt --methods random degree transe rgcn --filtered --type_constrained --both_sides

The baselines (``baselines.py``) are fitted on the train graph; every method is then put through the project's OWN ranking
protocol on the test triples - the rank of the true tail (and, with ``--both_sides``, head) among all entities from the
fused ranking pass, known triples filtered and candidates type-constrained as asked: MRR and Hits@1/5/10/20/50 - and
``ModelEvaluator.compute_classification_metrics`` is applied to per-triple scores of the test triples and one seeded
corruption of each.  How a method orders candidates:

* ``rgcn``    the checkpoint's decoder (DistMult, or ComplEx when it was trained with ``--decoder complex``) on the
              encoder's embeddings (``ModelEvaluator.tail_ranks`` / ``head_ranks``);
* ``transe``  the TransE distance ``|h + r - t|`` (``ops.transe_rank_operands``); its per-triple score is the reference's
              ``(cos + 1) / 2``;
* ``complex`` the ComplEx score ``Re <h, r, conj(t)>`` on a free entity table (``baselines.ComplEx``: the project's own head,
              ``ops.complex_query`` for the query rows of each side); its per-triple score is ``sigmoid`` of it;
* ``degree``  ``sqrt(deg_drug(head) * deg_disease(tail))`` (``NodeDegreeBaseline``), ranked as the product of the two
              factors - a one-column inner product, so it goes through the same pass and masks;
* ``random``  the inner product of two seeded Gaussian tables: a different random order per query.

What is NOT rebuilt, on purpose: the reference's ``evaluate_method`` labels a pair positive when the method's own score
is above that method's median (proxy labels), and its ``statistical_significance_test`` says itself that its p-values
are a placeholder.  What answers it instead: ``--bootstrap B`` resamples the test triples on the
device (``bootstrap.py``) - every method under the same weights - and adds standard errors,
95 % intervals and a paired two-sided p-value for every pair of methods; ``--by_frequency`` reports every method on the
rare / medium / common diseases of the train graph.  Writes ``comparison.json`` and ``comparison_table.md``.
"""
from __future__ import annotations

import argparse
import json
import logging
import time
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import baselines, ops
from . import bootstrap as BS
from . import evaluate as E

logger = logging.getLogger("primekg_rgcn_linkprediction_amd.compare")

METHODS = ("random", "degree", "transe", "complex", "rgcn")
K_VALUES = (1, 5, 10, 20, 50)
TYPE_NAMES = {"drug": "drug", "disease": "disease"}          # PrimeKG's node type names
NEGATIVE_STREAM = (1 << 55) + 2                               # Philox stream of the comparison's corruptions


def ranking_metrics(ranks: torch.Tensor, k_values: Sequence[int] = K_VALUES) -> Dict:
    """``ModelEvaluator.compute_ranking_metrics``'s names over a vector of 1-based ranks"""
    ranks = ranks.cpu().numpy().astype(np.float64)
    out = {"mrr": float(np.mean(1.0 / ranks)), "mean_rank": float(np.mean(ranks)), "median_rank": float(np.median(ranks))}
    for k in k_values:
        out[f"hits@{k}"] = float(np.mean(ranks <= k))
    return out


def _column_operands(query_factor: torch.Tensor, cand_factor: torch.Tensor):
    """``(q [B, 32], cand [N, 32])`` whose inner product is ``query_factor[b] * cand_factor[n]``"""
    q = torch.zeros(query_factor.numel(), 32, dtype=torch.float32, device=query_factor.device)
    cand = torch.zeros(cand_factor.numel(), 32, dtype=torch.float32, device=cand_factor.device)
    q[:, 0], cand[:, 0] = query_factor.float(), cand_factor.float()
    return q, cand


class _Protocol:
    """the test triples and the masks of the asked protocol, shared by every method"""

    def __init__(self, test_data: Dict, full_graph: Dict, device, node_class, filtered: bool, type_constrained: bool,
                 both_sides: bool, num_relations: int):
        self.device = device
        self.head = test_data["edge_index"][0].to(device).contiguous()
        self.tail = test_data["edge_index"][1].to(device).contiguous()
        self.rel = test_data["edge_type"].to(device).contiguous()
        self.num_nodes = int(full_graph["num_nodes"])
        self.filtered, self.type_constrained, self.both_sides = bool(filtered), bool(type_constrained), bool(both_sides)
        if type_constrained and node_class is None:
            raise ValueError("type-constrained ranking needs the node classes (--node_types)")
        self.node_class = None if node_class is None else torch.as_tensor(node_class).to(device=device, dtype=torch.int32)
        self.known = self.allow = None
        if filtered:
            self.known = ops.KnownTriples(torch.cat([full_graph["edge_index"].to(device), test_data["edge_index"].to(device)], 1),
                                          torch.cat([full_graph["edge_type"].to(device), test_data["edge_type"].to(device)]),
                                          self.num_nodes, num_relations)
        if type_constrained:
            self.allow = ops.class_allow_bits(self.node_class.contiguous(), max(int(self.node_class.max()) + 1, 1))

    def sides(self):
        yield "tail", self.head, self.tail
        if self.both_sides:
            yield "head", self.tail, self.head

    def ranks(self, operands) -> torch.Tensor:
        """``operands(side, anchors, rels) -> (q, cand)``: the ranks of the true answers on the asked sides"""
        out = []
        for side, anchors, targets in self.sides():
            q, cand = operands(side, anchors, self.rel)
            true = (q * cand[targets]).sum(dim=1)
            query_class = self.node_class[targets].contiguous() if self.type_constrained else None
            out.append(ops.distmult_rank_filtered(q.contiguous(), cand.contiguous(), true, targets, self.known, side, anchors,
                                                  self.rel, self.allow, query_class))
        return torch.cat(out)

    def describe(self) -> Dict:
        return {"filtered": self.filtered, "type_constrained": self.type_constrained,
                "sides": "both" if self.both_sides else "tail", "test_triples": int(self.head.numel()),
                "known_triples": "full graph + test set" if self.filtered else None}


def compare_methods(train_data: Dict, test_data: Dict, full_graph: Dict, device, model=None, node_class=None,
                    methods: Sequence[str] = ("random", "degree", "transe"), k_values: Sequence[int] = K_VALUES,
                    filtered: bool = False, type_constrained: bool = False, both_sides: bool = False,
                    transe_epochs: int = 50, seed: int = 0, drug_class: Optional[int] = None,
                    disease_class: Optional[int] = None, transe_kwargs: Optional[Dict] = None, bootstrap: int = 0,
                    bootstrap_seed: int = 0, by_frequency: bool = False, complex_epochs: int = 50,
                    complex_kwargs: Optional[Dict] = None) -> Dict:
    """-> ``{"protocol": ..., "methods": {name: {"ranking": ..., "classification": ..., "fit_seconds": ...}}}``.
    ``bootstrap`` > 0: every method also gets a ``"bootstrap"`` block (``bootstrap.block``: estimate, standard error and
    95 % interval per metric over that many paired resamples of the test triples, on the device) and the result a
    ``"significance"`` block (``bootstrap.significance``: the paired difference of every two methods).  Every method is
    handed the same unit vectors and seed: that is the pairing.  ``by_frequency``: a ``"by_frequency"`` block - the test
    triples with a disease end split into rare / medium / common by the disease's degree in the train graph."""
    device = torch.device(device)
    unknown = [m for m in methods if m not in METHODS]
    if unknown:
        raise ValueError(f"unknown methods {unknown}: choose from {METHODS}")
    if "rgcn" in methods and model is None:
        raise ValueError("method 'rgcn' needs the trained model (--model_path)")
    if "degree" in methods and (node_class is None or drug_class is None or disease_class is None):
        raise ValueError("method 'degree' needs the node classes and the class ids of drugs and diseases "
                         "(--node_types, --drug_class, --disease_class)")
    if by_frequency and (node_class is None or disease_class is None):
        raise ValueError("by_frequency needs the node classes and the class id of diseases (--node_types, --disease_class)")
    bootstrap_n = int(bootstrap)
    if bootstrap_n < 0:
        raise ValueError("bootstrap must be >= 0")
    num_nodes = int(full_graph["num_nodes"])
    num_relations = int(full_graph.get("num_relations", int(full_graph["edge_type"].max()) + 1))
    proto = _Protocol(test_data, full_graph, device, node_class, filtered, type_constrained, both_sides, num_relations)
    train_ei, train_et = train_data["edge_index"].to(device), train_data["edge_type"].to(device)
    # the per-triple scores' negatives: one corruption of every test triple from the device sampler, the same for every method
    rng = torch.tensor([seed & 0x7FFFFFFFFFFFFFFF, NEGATIVE_STREAM], dtype=torch.int64).to(device)
    b = int(proto.head.numel())
    heads, tails, _, labels = ops.sample_batch(torch.stack([proto.head, proto.tail]), proto.rel, None, None, b, 1, num_nodes, rng)
    labels_dev, labels = labels, labels.cpu().numpy()
    score_unit = BS.triple_units(b, heads.numel(), device)
    rank_unit = BS.query_units(b, b * (2 if both_sides else 1), device)
    strata = frequency_strata(train_ei, proto.head, proto.tail, proto.node_class, disease_class) if by_frequency else None
    results, vectors, frequency = {}, {}, {}
    for name in methods:
        t0 = time.perf_counter()
        if name == "rgcn":
            ev = E.ModelEvaluator(model, test_data, full_graph, device, node_class=proto.node_class)
            emb, dec = ev.embeddings(), ev.model.decoder
            fit_s = time.perf_counter() - t0
            ranks = ev.tail_ranks(filtered, type_constrained)
            if both_sides:
                ranks = torch.cat([ranks, ev.head_ranks(filtered, type_constrained)])
            rels2 = torch.cat([proto.rel, proto.rel])
            scores = torch.sigmoid(dec.score_triples(emb, heads, tails, rels2))
        elif name == "transe":
            kw = dict(num_epochs=transe_epochs, seed=seed, device=device)
            kw.update(transe_kwargs or {})
            method = baselines.TransE(**kw).fit(train_ei, train_et, num_nodes, num_relations)
            torch.cuda.synchronize(device)
            fit_s = time.perf_counter() - t0
            ranks = proto.ranks(lambda side, a, r: ops.transe_rank_operands(method.embeddings, method.relation_embeddings,
                                                                            a, r, side)[:2])
            scores = method.predict(heads, tails)
        elif name == "complex":
            kw = dict(num_epochs=complex_epochs, seed=seed, device=device)
            kw.update(complex_kwargs or {})
            method = baselines.ComplEx(**kw).fit(train_ei, train_et, num_nodes, num_relations)
            torch.cuda.synchronize(device)
            fit_s = time.perf_counter() - t0
            ranks = proto.ranks(lambda side, a, r: (ops.complex_query(method.embeddings, a, method.relation_embeddings, r, side),
                                                    method.embeddings))
            scores = method.predict(heads, tails, torch.cat([proto.rel, proto.rel]))
        elif name == "degree":
            method = baselines.NodeDegree().fit(train_ei, proto.node_class, drug_class, disease_class)
            fit_s = time.perf_counter() - t0
            drug, dis = method.drug_degree, method.disease_degree
            ranks = proto.ranks(lambda side, a, r: _column_operands(drug[a], dis) if side == "tail"
                                else _column_operands(dis[a], drug))
            scores = method.predict(heads, tails)
        else:
            gen = torch.Generator().manual_seed(seed)
            left, right = torch.randn(num_nodes, 32, generator=gen).to(device), torch.randn(num_nodes, 32, generator=gen).to(device)
            fit_s = time.perf_counter() - t0
            ranks = proto.ranks(lambda side, a, r: (left[a], right) if side == "tail" else (right[a], left))
            scores = baselines.Random(seed).predict(heads, tails)
        results[name] = {"ranking": ranking_metrics(ranks, k_values),
                         "classification": E.ModelEvaluator.compute_classification_metrics(
                             scores.detach().double().cpu().numpy(), labels),
                         "fit_seconds": fit_s}
        if name in ("transe", "complex"):
            results[name]["epoch_losses"] = method.epoch_losses
        scores = scores.detach().double().to(device)         # the Random baseline scores on the host
        if bootstrap_n:
            vectors[name], degenerate, w_sum = BS.replicate_vectors(scores, labels_dev, score_unit, ranks, rank_unit, k_values,
                                                                      bootstrap_n, bootstrap_seed)
            results[name]["bootstrap"] = BS.block(vectors[name], degenerate, bootstrap_n, bootstrap_seed, w_sum)
        if strata is not None:
            frequency[name] = _stratum_metrics(strata, scores, labels_dev, score_unit, ranks, rank_unit, k_values,
                                               bootstrap_n, bootstrap_seed)
        logger.info("%s: MRR %.4f, Hits@10 %.4f, AUC-ROC %.4f", name, results[name]["ranking"]["mrr"],
                    results[name]["ranking"].get("hits@10", float("nan")), results[name]["classification"]["auc_roc"])
    ops.check_indices(device)
    decoder_name = {"distmult": "DistMult", "complex": "ComplEx"}[getattr(getattr(model, "decoder", None), "decoder", "distmult")]
    protocol = dict(proto.describe(), k_values=list(k_values), seed=seed, transe_epochs=transe_epochs,
                    complex_epochs=complex_epochs,
                    classification="test triples (label 1) and one seeded corruption of each (label 0); per-triple scores: "
                                   f"rgcn sigmoid({decoder_name}), transe (cos + 1) / 2, complex sigmoid(ComplEx), degree sqrt(deg_drug * deg_disease), "
                                   "random uniform; threshold 0.5")
    result = {"protocol": protocol, "methods": results}
    if bootstrap_n:
        protocol["bootstrap"] = {"replicates": bootstrap_n, "seed": bootstrap_seed, "unit": "test triple",
                                 "weights": "Poisson(1) per triple and replicate, shared by every method"}
        result["significance"] = BS.significance(vectors)
    if strata is not None:
        result["by_frequency"] = {"boundaries": {"q33": strata["q1"], "q67": strata["q2"]},
                                  "triples": {s: int(strata[s].sum()) for s in STRATA}, "methods": frequency}
    return result


STRATA = ("rare", "medium", "common")


def frequency_strata(train_edge_index: torch.Tensor, head: torch.Tensor, tail: torch.Tensor, node_class: torch.Tensor,
                     disease_class: int) -> Dict:
    """The reference's ``evaluate_by_disease_frequency`` split (src/compare_methods.py:616-675) of the test triples
    that have a disease end (the tail when it is a disease, else the head): the disease's degree in the train graph,
    every edge end counted, against the 33rd / 67th percentiles of the degrees of the diseases seen in training -
    ``<= q1`` rare, ``<= q2`` medium, above common.  -> bool masks ``[num_triples]`` by stratum, ``q1``, ``q2``."""
    is_disease = node_class == int(disease_class)
    degree = torch.bincount(train_edge_index.reshape(-1), minlength=node_class.numel())
    seen = degree[is_disease & (degree > 0)]
    if seen.numel() == 0:
        raise ValueError("by_frequency: no node of the disease class has an edge in the train graph")
    q1, q2 = (float(q) for q in np.percentile(seen.cpu().numpy(), [33, 67]))
    end = torch.where(is_disease[tail], tail, head)
    has, deg = is_disease[end], degree[end]
    return {"rare": has & (deg <= q1), "medium": has & (deg > q1) & (deg <= q2), "common": has & (deg > q2),
            "q1": q1, "q2": q2}


def _stratum_metrics(strata: Dict, scores, labels, score_unit, ranks, rank_unit, k_values, replicates: int, seed: int) -> Dict:
    """one method's metrics on each stratum: the same functions on the samples and queries of the stratum's triples"""
    out = {}
    for name in STRATA:
        mask = strata[name]
        pick_s, pick_r = mask[score_unit.long()], mask[rank_unit.long()]
        entry = {"triples": int(mask.sum())}
        if entry["triples"]:
            s, y = scores[pick_s], labels[pick_s]
            entry["ranking"] = ranking_metrics(ranks[pick_r], k_values)
            entry["classification"] = E.ModelEvaluator.compute_classification_metrics(s.cpu().numpy(), y.cpu().numpy())
            if replicates:
                vec, degenerate, w_sum = BS.replicate_vectors(s, y, score_unit[pick_s].contiguous(), ranks[pick_r].contiguous(),
                                                              rank_unit[pick_r].contiguous(), k_values, replicates, seed)
                entry["bootstrap"] = BS.block(vec, degenerate, replicates, seed, w_sum)
        out[name] = entry
    return out


def table_markdown(result: Dict) -> str:
    """``comparison_table.md``: one row per method, the reference's column choice plus Hits@1"""
    cols = [("mrr", "MRR"), ("hits@1", "H@1"), ("hits@10", "H@10"), ("hits@50", "H@50")]
    cols = [(k, t) for k, t in cols if all(k in m["ranking"] for m in result["methods"].values())]
    p = result["protocol"]
    lines = ["# Method Comparison Results", "",
             f"Ranking: filtered {p['filtered']}, type-constrained {p['type_constrained']}, sides {p['sides']}, "
             f"{p['test_triples']} test triples.", "",
             "| Method | AUC-ROC | AP | " + " | ".join(t for _, t in cols) + " |", "|" + "---|" * (3 + len(cols))]
    for name, m in result["methods"].items():
        boot = m.get("bootstrap", {})

        def cell(value, key):
            se = boot.get(key, {}).get("se")
            return f"{value:.4f}" + (f" ± {se:.4f}" if se is not None else "")

        cells = [cell(m["classification"]["auc_roc"], "auc_roc"), cell(m["classification"]["auc_pr"], "auc_pr")]
        cells += [cell(m["ranking"][k], k) for k, _ in cols]
        lines.append(f"| {name} | " + " | ".join(cells) + " |")
    if "significance" in result:
        lines += ["", f"Paired bootstrap over the test triples, {p['bootstrap']['replicates']} replicates "
                      f"(seed {p['bootstrap']['seed']}); ± is the standard error.", "",
                  "| Metric | Pair | Mean difference | 95 % interval | p |", "|---|---|---|---|---|"]
        for metric, pairs in result["significance"].items():
            for pair, d in pairs.items():
                if d["p_value"] is None:
                    lines.append(f"| {metric} | {pair} | - | - | - |")
                else:
                    lines.append(f"| {metric} | {pair} | {d['mean_difference']:+.4f} | [{d['ci95'][0]:+.4f}, {d['ci95'][1]:+.4f}] "
                                 f"| {d['p_value']:.4f} |")
    return "\n".join(lines) + "\n"


def save_comparison(result: Dict, output_dir) -> Path:
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    with open(output_dir / "comparison.json", "w") as fh:
        json.dump(result, fh, indent=2)
    (output_dir / "comparison_table.md").write_text(table_markdown(result))
    return output_dir / "comparison.json"


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Compare the R-GCN with the Random, Node Degree, TransE and ComplEx baselines on MI355X")
    p.add_argument("--data_dir", type=str, default="data/processed")
    p.add_argument("--model_path", type=str, default=None, help="the trained R-GCN checkpoint (method rgcn)")
    p.add_argument("--output_dir", type=str, default="results/comparison")
    p.add_argument("--node_types", type=str, default=None,
                   help="the preprocessing's mappings.pt, or an .npz / .pt holding an int vector [num_nodes]")
    p.add_argument("--methods", nargs="+", choices=METHODS, default=["random", "degree", "rgcn"])
    p.add_argument("--filtered", action="store_true", help="known triples (full graph + test set) do not count as candidates")
    p.add_argument("--type_constrained", action="store_true", help="rank among the entities of the true answer's node type")
    p.add_argument("--both_sides", action="store_true", help="rank the heads too and average over both sides")
    p.add_argument("--transe_epochs", type=int, default=50)
    p.add_argument("--complex_epochs", type=int, default=50)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--k_values", type=int, nargs="+", default=list(K_VALUES))
    p.add_argument("--drug_class", type=int, default=None, help="class id of drugs (default: by name from mappings.pt)")
    p.add_argument("--disease_class", type=int, default=None)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--trust_checkpoint", action="store_true",
                   help="allow the unrestricted pickle loader for --model_path (only for files you wrote yourself)")
    p.add_argument("--bootstrap", type=int, default=0,
                   help="paired bootstrap replicates over the test triples: intervals per method, p-values per pair (0: off)")
    p.add_argument("--bootstrap_seed", type=int, default=0)
    p.add_argument("--by_frequency", action="store_true",
                   help="also report every method on the rare / medium / common diseases of the train graph (needs --node_types)")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.bootstrap < 0 or args.bootstrap > 65535:
        parser.error("--bootstrap must be in [0, 65535]")
    if "rgcn" in args.methods and not args.model_path:
        parser.error("method rgcn needs --model_path")
    if (args.type_constrained or args.by_frequency or "degree" in args.methods) and not args.node_types:
        parser.error("--type_constrained, --by_frequency and method degree need --node_types PATH")
    if args.transe_epochs < 0 or args.complex_epochs < 0:
        parser.error("--transe_epochs and --complex_epochs must be >= 0")
    return args


def _class_id(given: Optional[int], kind: str, class_names) -> Optional[int]:
    if given is not None:
        return given
    if class_names is not None and TYPE_NAMES[kind] in class_names:
        return class_names.index(TYPE_NAMES[kind])
    return None


def main(argv=None) -> Dict:
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(name)s - %(levelname)s - %(message)s")
    args = parse_args(argv)
    device = torch.device(args.device)
    test_data, full_graph = E.load_test_data(args.data_dir)
    num_nodes = int(full_graph["num_nodes"])
    from .train import filter_edges
    train_data = filter_edges(torch.load(Path(args.data_dir) / "train_data.pt", weights_only=True), num_nodes, "Train")
    node_class = E.load_node_classes(args.node_types, num_nodes) if args.node_types else None
    from .failures import load_class_names
    names = load_class_names(args.node_types, num_nodes)
    model = E.load_model(args.model_path, device, trust_pickle=args.trust_checkpoint)[0] if "rgcn" in args.methods else None
    result = compare_methods(train_data, test_data, full_graph, device, model, node_class, args.methods, args.k_values,
                             args.filtered, args.type_constrained, args.both_sides, args.transe_epochs, args.seed,
                             _class_id(args.drug_class, "drug", names), _class_id(args.disease_class, "disease", names),
                             bootstrap=args.bootstrap, bootstrap_seed=args.bootstrap_seed, by_frequency=args.by_frequency,
                             complex_epochs=args.complex_epochs)
    path = save_comparison(result, args.output_dir)
    print(table_markdown(result))
    logger.info("Comparison saved to: %s", path)
    return result


if __name__ == "__main__":
    main()
