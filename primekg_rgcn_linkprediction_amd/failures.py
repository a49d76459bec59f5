"""Why does the model get a (drug, disease) pair wrong: the reference's failure analysis over every sampled pair.

Counterpart of ``src/analyze_failures.py`` minus its plots and its hypothesis prose: labelled pairs are scored with the
embeddings' cosine mapped to [0, 1], typed FP / FN / Correct with a confidence error (``analyze_failures.py:298-329``),
and every pair - not five failures and five successes - gets the structural context ``analyze_subgraph`` computes with
networkx (``:368-437``: the radius-2 balls of both ends, their common neighbours, the induced subgraph's node, edge and
node-type counts) from ``ops.pair_neighborhood``, and its exact simple-path counts from ``ops.paths_topk``.

    python -m primekg_rgcn_linkprediction_amd.failures --model_path results/models/best_model.pt \\
        --data_dir data/processed --node_types data/processed/mappings.pt --radius 2 --num_samples 5000 --seed 42 \\
        --output_dir results/failure_analysis

writes ``failure_analysis.json``: ``{"protocol", "num_pairs", "means" (per type and per group), "differences" (the
reference's four figures, success minus failure, between the group means), "failures", "successes"}``.  ``--pairs FILE``
takes the labelled pairs from an ``.npz`` with ``drug``, ``disease`` and ``label`` instead of sampling them.

The built-in sampler works in the reference's manner (``get_ground_truth_labels``, ``:201-271``): a positive is a drug
predecessor and a disease successor of a sampled gene, a negative a random drug x disease pair.  It draws from a private
``numpy.random.RandomState(seed)``: seeded and reproducible, but NOT draw for draw the reference's sample (which uses the
global numpy state, whatever it holds when the script gets there).
"""
from __future__ import annotations

import argparse
import json
import logging
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import evaluate as E

logger = logging.getLogger("primekg_rgcn_linkprediction_amd.failures")

TYPE_NAMES = {"drug": "drug", "disease": "disease", "gene": "gene/protein"}      # PrimeKG's node type names


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Failure analysis of a trained R-GCN link predictor over all sampled pairs, on MI355X")
    p.add_argument("--model_path", type=str, required=True)
    p.add_argument("--data_dir", type=str, default="data/processed")
    p.add_argument("--output_dir", type=str, default="results/failure_analysis")
    p.add_argument("--node_types", type=str, default=None,
                   help="the preprocessing's mappings.pt, or an .npz / .pt holding an int vector [num_nodes]")
    p.add_argument("--radius", type=int, default=2, help="radius of the two neighbourhoods, 0..4")
    p.add_argument("--pairs", type=str, default=None, help="an .npz with drug, disease and label: the labelled pairs")
    p.add_argument("--num_samples", type=int, default=5000, help="labelled pairs the sampler draws (half positive)")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--drug_class", type=int, default=None, help="class id of drugs (default: by name from mappings.pt)")
    p.add_argument("--disease_class", type=int, default=None)
    p.add_argument("--gene_class", type=int, default=None)
    p.add_argument("--num_failures", type=int, default=5)
    p.add_argument("--num_successes", type=int, default=5)
    p.add_argument("--common_nodes", type=int, default=0, metavar="CAP", help="list up to CAP common neighbours per pair")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--trust_checkpoint", action="store_true",
                   help="allow the unrestricted pickle loader for --model_path (only for files you wrote yourself)")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    parser = build_parser()
    args = parser.parse_args(argv)
    if not 0 <= args.radius <= 4:
        parser.error("--radius must be in 0..4")
    if not args.pairs and not args.node_types:
        parser.error("the sampler needs --node_types PATH (or give the labelled pairs with --pairs FILE)")
    if args.num_samples < 2 or args.num_failures < 0 or args.num_successes < 0:
        parser.error("--num_samples must be >= 2, --num_failures and --num_successes >= 0")
    if not 0 <= args.common_nodes <= 1024:
        parser.error("--common_nodes must be in 0..1024")
    return args


def load_class_names(path: Optional[str], num_nodes: int) -> Optional[List[str]]:
    """the class names of a ``mappings.pt`` (class ids by sorted type name, as ``graphio.node_classes``), else None"""
    if not path or str(path).endswith(".npz"):
        return None
    obj = torch.load(path, map_location="cpu", weights_only=True)
    if not (isinstance(obj, dict) and "idx2node" in obj):
        return None
    from .graphio import node_classes
    return node_classes(obj["idx2node"], num_nodes)[1]


def load_pairs(path) -> Tuple[np.ndarray, np.ndarray]:
    """-> (pairs int64 [P, 2], labels int64 [P]) from an ``.npz`` with ``drug``, ``disease``, ``label``"""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ("drug", "disease", "label") if k not in z.files]
        if missing:
            raise ValueError(f"{path}: no array named {missing[0]!r} (drug, disease and label expected)")
        drug, disease, label = (np.asarray(z[k]).astype(np.int64).reshape(-1) for k in ("drug", "disease", "label"))
    if not drug.shape == disease.shape == label.shape:
        raise ValueError(f"{path}: drug, disease and label must be equally long")
    return np.stack([drug, disease], 1), label


def sample_labelled_pairs(edge_index, node_class, drug_class: int, disease_class: int, gene_class: int,
                          num_samples: int, seed: int = 42) -> Tuple[np.ndarray, np.ndarray]:
    """The reference's sample: until ``num_samples // 2`` positives are found (at most ``10 * num_samples`` tries) a gene
    with at least one edge is drawn, and if it has a drug among its predecessors and a disease among its successors one of
    each makes a positive; then ``num_samples // 2`` random drug x disease pairs are the negatives.  Without a gene in
    the graph all ``num_samples`` pairs are random negatives, as there.  Draws from ``RandomState(seed)``.
    -> (pairs int64 [P, 2], labels int64 [P])"""
    rng = np.random.RandomState(seed)
    ei = np.asarray(torch.as_tensor(edge_index).cpu())
    cls = np.asarray(torch.as_tensor(node_class).cpu())
    drugs, diseases = np.flatnonzero(cls == drug_class), np.flatnonzero(cls == disease_class)
    if not drugs.size or not diseases.size:
        raise ValueError("the node classes hold no drug or no disease")
    touched = np.zeros(cls.shape[0], dtype=bool)
    touched[ei[0]] = touched[ei[1]] = True
    genes = np.flatnonzero((cls == gene_class) & touched)
    if not genes.size:
        pairs = [(rng.choice(drugs), rng.choice(diseases), 0) for _ in range(num_samples)]
    else:
        by_dst, by_src = np.argsort(ei[1], kind="stable"), np.argsort(ei[0], kind="stable")
        dst_sorted, src_sorted = ei[1][by_dst], ei[0][by_src]
        pairs, attempts = [], 0
        while len(pairs) < num_samples // 2 and attempts < num_samples * 10:
            attempts += 1
            gene = rng.choice(genes)
            pred = np.unique(ei[0][by_dst[np.searchsorted(dst_sorted, gene):np.searchsorted(dst_sorted, gene, "right")]])
            succ = np.unique(ei[1][by_src[np.searchsorted(src_sorted, gene):np.searchsorted(src_sorted, gene, "right")]])
            pred, succ = pred[cls[pred] == drug_class], succ[cls[succ] == disease_class]
            if pred.size and succ.size:
                pairs.append((rng.choice(pred), rng.choice(succ), 1))
        pairs += [(rng.choice(drugs), rng.choice(diseases), 0) for _ in range(num_samples // 2)]
    arr = np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
    return arr[:, :2].copy(), arr[:, 2].copy()


def _class_id(given: Optional[int], kind: str, class_names: Optional[List[str]]) -> int:
    if given is not None:
        return given
    if class_names is not None and TYPE_NAMES[kind] in class_names:
        return class_names.index(TYPE_NAMES[kind])
    raise ValueError(f"--{kind}_class is needed: --node_types names no class {TYPE_NAMES[kind]!r}")


def analyze(evaluator, args: argparse.Namespace, class_names: Optional[List[str]] = None,
            names: Optional[Dict[int, str]] = None) -> Dict:
    """the JSON document: the labelled pairs (``--pairs`` or the sampler over the evaluator's full graph and node
    classes) through ``evaluator.failure_analysis``"""
    if args.pairs:
        pairs, labels = load_pairs(args.pairs)
        source = {"pairs": str(args.pairs)}
    else:
        if evaluator.node_class is None:
            raise ValueError("the sampler needs the node classes (--node_types)")
        ids = {kind: _class_id(getattr(args, f"{kind}_class", None), kind, class_names) for kind in ("drug", "disease", "gene")}
        pairs, labels = sample_labelled_pairs(evaluator.full_edge_index, evaluator.node_class, ids["drug"], ids["disease"],
                                              ids["gene"], args.num_samples, args.seed)
        source = {"sampler": "a drug predecessor and a disease successor of a sampled gene; random drug x disease negatives",
                  "num_samples": args.num_samples, "seed": args.seed, "classes": ids}
    result = evaluator.failure_analysis(pairs.tolist(), labels.tolist(), radius=args.radius, num_failures=args.num_failures,
                                        num_successes=args.num_successes, class_names=class_names,
                                        common_cap=getattr(args, "common_nodes", 0))
    if names is not None:
        for row in result["failures"] + result["successes"]:
            row["drug_name"], row["disease_name"] = names.get(row["drug_idx"]), names.get(row["disease_idx"])
    protocol = {"score": "(cos(drug, disease) + 1) / 2", "radius": args.radius, "positives": int(labels.sum()),
                "negatives": int((labels == 0).sum()), **source,
                "type": "FP: label 0 and score > 0.5; FN: label 1 and score <= 0.5; else Correct",
                "differences": "mean over Correct pairs minus mean over FP + FN pairs"}
    return {"protocol": protocol, **{k: v for k, v in result.items() if k != "radius"}}


def save_analysis(result: Dict, output_dir) -> Path:
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    path = output_dir / "failure_analysis.json"
    with open(path, "w") as fh:
        json.dump(result, fh, indent=2)
    return path


def main(argv=None) -> Dict:
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(name)s - %(levelname)s - %(message)s")
    args = parse_args(argv)
    device = torch.device(args.device)
    model, _ = E.load_model(args.model_path, device, trust_pickle=args.trust_checkpoint)
    test_data, full_graph = E.load_test_data(args.data_dir)
    num_nodes = int(full_graph["num_nodes"])
    node_class = E.load_node_classes(args.node_types, num_nodes) if args.node_types else None
    evaluator = E.ModelEvaluator(model, test_data, full_graph, device, node_class=node_class)
    from .predict import load_node_names
    result = analyze(evaluator, args, load_class_names(args.node_types, num_nodes), load_node_names(args.node_types))
    path = save_analysis(result, args.output_dir)
    logger.info("%d pairs analysed, saved to: %s", result["num_pairs"], path)
    return result


if __name__ == "__main__":
    main()
