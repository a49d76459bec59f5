"""Cluster a trained model's node embeddings: k-means and silhouette per node type, on the device.

Counterpart of the reference's ``visualize_embeddings.cluster_analysis`` (``KMeans(n_clusters, n_init=10,
random_state=42)`` + ``silhouette_score`` per node type, ``results/embeddings/clustering_summary.txt``): the encoder runs
once and ``ModelEvaluator.cluster_analysis`` clusters every type's rows with ``ops.kmeans`` (all restarts side by side
through the fp32 matrix-core tile) and scores the result with ``ops.silhouette_score`` (no ``[n, n]`` distance matrix).

    python -m primekg_rgcn_linkprediction_amd.cluster --model_path results/models/best_model.pt \\
        --data_dir data/processed --node_types data/processed/mappings.pt --n_clusters 10 \\
        --node_names data/processed/mappings.pt --output_dir results/embeddings

writes ``clustering_summary.json``: ``{"protocol": {..., "left_out": [...]}, "types": {name: {"num_nodes", "silhouette",
"cluster_sizes", "mean_cluster_size", "std_cluster_size", "first_members": [[node ids], ...]}}}`` - the four figures per
type of the reference's summary and the first ten members of every cluster (node ids ascending; with ``--node_names`` also
``first_member_names``); ``left_out`` names the types with fewer nodes than clusters, which are skipped with a warning.
"""
from __future__ import annotations

import argparse
import json
import logging
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import torch

from . import evaluate as E
from .predict import load_node_names

logger = logging.getLogger("primekg_rgcn_linkprediction_amd.cluster")

FIRST_MEMBERS = 10      # members listed per cluster, as in the reference's *_cluster_examples.txt


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="K-means and silhouette analysis of a trained R-GCN's node embeddings on MI355X")
    p.add_argument("--model_path", type=str, required=True)
    p.add_argument("--data_dir", type=str, default="data/processed")
    p.add_argument("--output_dir", type=str, default="results/embeddings")
    p.add_argument("--node_types", type=str, required=True,
                   help="the preprocessing's mappings.pt, or an .npz / .pt holding an int vector [num_nodes]")
    p.add_argument("--classes", type=int, nargs="+", default=None, help="only these node classes (default: every class)")
    p.add_argument("--n_clusters", type=int, default=10)
    p.add_argument("--n_init", type=int, default=10, help="k-means restarts, run side by side")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--max_iter", type=int, default=300)
    p.add_argument("--tol", type=float, default=1e-4)
    p.add_argument("--node_names", type=str, default=None, help="a mappings.pt with idx2node: members are also listed by name")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--trust_checkpoint", action="store_true",
                   help="allow the unrestricted pickle loader for --model_path (only for files you wrote yourself)")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.n_clusters < 2:
        parser.error("--n_clusters must be >= 2")
    if args.n_init < 1:
        parser.error("--n_init must be >= 1")
    if args.max_iter < 1:
        parser.error("--max_iter must be >= 1")
    if not args.tol >= 0:
        parser.error("--tol must be >= 0")
    return args


def class_names(path: Optional[str], node_class: torch.Tensor, only=None) -> Dict[str, int]:
    """``{name: class id}`` of the classes to analyse: the node type names when ``path`` is a ``mappings.pt``, else
    ``class_<id>``; ``only`` restricts the ids"""
    present = sorted(int(c) for c in torch.unique(node_class.cpu()).tolist() if c >= 0)
    type_names = None
    if path and not str(path).endswith(".npz"):
        obj = torch.load(path, map_location="cpu", weights_only=True)
        if isinstance(obj, dict) and "idx2node" in obj:
            from .graphio import node_classes
            type_names = node_classes(obj["idx2node"], node_class.numel())[1]
    ids = present if only is None else [int(c) for c in only]
    return {(type_names[c] if type_names is not None and 0 <= c < len(type_names) else f"class_{c}"): c for c in ids}


def summarize(results: Dict[str, Dict], args: argparse.Namespace, names: Optional[Dict[int, str]] = None) -> Dict:
    """``evaluator.cluster_analysis``'s result -> the ``clustering_summary.json`` dict"""
    types = {}
    for name, res in results.items():
        sizes = np.asarray(res["cluster_sizes"], dtype=np.int64)
        entry = {"num_nodes": int(sizes.sum()), "silhouette": float(res["silhouette"]), "cluster_sizes": sizes.tolist(),
                 "mean_cluster_size": float(sizes.mean()), "std_cluster_size": float(sizes.std()),
                 "first_members": [[int(i) for i in m[:FIRST_MEMBERS]] for m in res["members"]]}
        if names is not None:
            entry["first_member_names"] = [[names.get(i) for i in m] for m in entry["first_members"]]
        types[name] = entry
    protocol = {"n_clusters": args.n_clusters, "n_init": args.n_init, "seed": args.seed, "max_iter": args.max_iter,
                "tol": args.tol, "first_members": FIRST_MEMBERS,
                "kmeans": "Lloyd, k-means++ starts from the seed, least inertia of the restarts; an emptied cluster keeps its centroid",
                "silhouette": "mean over the type's nodes of (b - a) / max(a, b), Euclidean, float32 distances"}
    return {"protocol": protocol, "types": types}


def analyse(evaluator, args: argparse.Namespace, which: Dict[str, int], names: Optional[Dict[int, str]] = None) -> Dict:
    results = evaluator.cluster_analysis(which, args.n_clusters, n_init=args.n_init, seed=args.seed, max_iter=args.max_iter,
                                         tol=args.tol)
    summary = summarize(results, args, names)
    summary["protocol"]["left_out"] = [name for name in which if name not in results]   # fewer nodes than clusters
    return summary


def save_summary(summary: Dict, output_dir) -> Path:
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    path = output_dir / "clustering_summary.json"
    with open(path, "w") as fh:
        json.dump(summary, fh, indent=2)
    return path


def main(argv=None) -> Dict:
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(name)s - %(levelname)s - %(message)s")
    args = parse_args(argv)
    device = torch.device(args.device)
    model, _ = E.load_model(args.model_path, device, trust_pickle=args.trust_checkpoint)
    test_data, full_graph = E.load_test_data(args.data_dir)
    node_class = E.load_node_classes(args.node_types, int(full_graph["num_nodes"]))
    evaluator = E.ModelEvaluator(model, test_data, full_graph, device, node_class=node_class)
    summary = analyse(evaluator, args, class_names(args.node_types, node_class, args.classes), load_node_names(args.node_names))
    path = save_summary(summary, args.output_dir)
    for name, entry in summary["types"].items():
        logger.info("%s: silhouette %.4f, cluster sizes %s", name, entry["silhouette"], entry["cluster_sizes"])
    logger.info("saved to: %s", path)
    return summary


if __name__ == "__main__":
    main()
