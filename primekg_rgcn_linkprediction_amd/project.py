"""Project a trained model's node embeddings to the plane with t-SNE, on the device.

Counterpart of the reference's ``visualize_embeddings.reduce_dimensions`` (``TSNE(n_components=2, random_state=42,
perplexity=min(30, n - 1), max_iter=1000)`` on all nodes or a seeded sample): the encoder runs once and
``ModelEvaluator.reduce_dimensions`` projects the rows with ``ops.tsne`` - neighbours from the fused top-k pass,
scikit-learn's perplexity search, 1,000 gradient iterations with EXACT repulsion (scikit-learn's default is the
Barnes-Hut approximation at angle 0.5; this is its angle = 0, O(n^2) per iteration), float32 state.

    python -m primekg_rgcn_linkprediction_amd.project --model_path results/models/best_model.pt \\
        --data_dir data/processed --node_types data/processed/mappings.pt --sample_size 10000 \\
        --output_dir results/embeddings

writes ``embedding_2d.npz`` (``xy`` float32 ``[n, 2]``, ``indices`` int64 ``[n]`` - the node of every row - and, with
``--node_types``, ``node_class`` int32 ``[n]``) and ``projection_summary.json``: ``{"protocol": {...}, "kl_divergence",
"n_iter", "num_points", "seconds": {stage: s}}``.  It draws no plots.  Fewer than 32 points need ``--perplexity`` below
``n - 1`` (``ops.tsne`` requires ``perplexity < k = min(n - 1, int(3 perplexity + 1))``).
"""
from __future__ import annotations

import argparse
import json
import logging
import time
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import torch

from . import evaluate as E

logger = logging.getLogger("primekg_rgcn_linkprediction_amd.project")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="t-SNE projection of a trained R-GCN's node embeddings on MI355X")
    p.add_argument("--model_path", type=str, required=True)
    p.add_argument("--data_dir", type=str, default="data/processed")
    p.add_argument("--output_dir", type=str, default="results/embeddings")
    p.add_argument("--node_types", type=str, default=None,
                   help="the preprocessing's mappings.pt, or an .npz / .pt holding an int vector [num_nodes]: saved beside the points")
    p.add_argument("--sample_size", type=int, default=None, help="project a seeded sample of this many nodes (default: all)")
    p.add_argument("--perplexity", type=float, default=30.0, help="capped at n - 1, as the reference does")
    p.add_argument("--max_iter", type=int, default=1000)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--init", type=str, default="pca", choices=("pca", "random"))
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--trust_checkpoint", action="store_true",
                   help="allow the unrestricted pickle loader for --model_path (only for files you wrote yourself)")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.sample_size is not None and args.sample_size < 2:
        parser.error("--sample_size must be >= 2")
    if not args.perplexity > 0:
        parser.error("--perplexity must be > 0")
    if args.max_iter < 1:
        parser.error("--max_iter must be >= 1")
    return args


def project(evaluator, args: argparse.Namespace, node_class: Optional[torch.Tensor] = None):
    """``evaluator.reduce_dimensions`` under ``args`` -> ``(arrays of embedding_2d.npz, the projection_summary.json dict)``"""
    timings: Dict[str, float] = {}
    start = time.perf_counter()
    n_all = int(evaluator.num_nodes)
    n = min(args.sample_size, n_all) if args.sample_size else n_all
    perplexity = float(min(args.perplexity, n - 1))
    xy, indices, result = evaluator.reduce_dimensions("tsne", args.sample_size, args.seed, return_result=True,
                                                      perplexity=perplexity, max_iter=args.max_iter, init=args.init,
                                                      timings=timings)
    arrays = {"xy": xy.cpu().numpy().astype(np.float32), "indices": np.asarray(indices, dtype=np.int64)}
    if node_class is not None:
        arrays["node_class"] = node_class.cpu().numpy().astype(np.int32)[arrays["indices"]]
    seconds = {stage: float(s) for stage, s in timings.items()}
    seconds["total"] = time.perf_counter() - start
    protocol = {"method": "tsne", "n_components": 2, "perplexity": perplexity, "max_iter": args.max_iter, "seed": args.seed,
                "init": args.init, "sample_size": args.sample_size, "early_exaggeration": 12.0, "learning_rate": "auto",
                "repulsion": "exact (scikit-learn's angle = 0; its default is Barnes-Hut at 0.5), float32 layout"}
    summary = {"protocol": protocol, "kl_divergence": float(result.kl_divergence), "n_iter": int(result.n_iter),
               "num_points": int(arrays["xy"].shape[0]), "seconds": seconds}
    return arrays, summary


def save(arrays: Dict[str, np.ndarray], summary: Dict, output_dir):
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    points, path = output_dir / "embedding_2d.npz", output_dir / "projection_summary.json"
    np.savez(points, **arrays)
    with open(path, "w") as fh:
        json.dump(summary, fh, indent=2)
    return points, path


def main(argv=None) -> Dict:
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(name)s - %(levelname)s - %(message)s")
    args = parse_args(argv)
    device = torch.device(args.device)
    model, _ = E.load_model(args.model_path, device, trust_pickle=args.trust_checkpoint)
    test_data, full_graph = E.load_test_data(args.data_dir)
    node_class = E.load_node_classes(args.node_types, int(full_graph["num_nodes"])) if args.node_types else None
    evaluator = E.ModelEvaluator(model, test_data, full_graph, device, node_class=node_class)
    arrays, summary = project(evaluator, args, node_class)
    points, path = save(arrays, summary, args.output_dir)
    logger.info("%d points, KL %.4f after %d iterations, %.2f s", summary["num_points"], summary["kl_divergence"],
                summary["n_iter"], summary["seconds"]["total"])
    logger.info("saved to: %s, %s", points, path)
    return summary


if __name__ == "__main__":
    main()
