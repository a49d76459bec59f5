"""Use a trained model: the top-k candidates of ``(anchor, relation, ?)`` / ``(?, relation, anchor)`` queries.

Counterpart of the question the reference's analysis scripts ask of a model - "which drugs, not already linked to
this disease, does it rank highest?" (``case_studies.predict_top_drugs``, ``medical_validation.generate_predictions``
+ ``_filter_known_associations``, their ``--top_k``) - on the decoder's own scores: the encoder runs once, and
``ModelEvaluator.top_candidates`` returns every query's list from one fused pass that keeps the k best allowed,
not-known candidates while the score tiles are still in registers (no ``[B, N]`` matrix, no sort).

    python -m primekg_rgcn_linkprediction_amd.predict --model_path results/models/best_model.pt \\
        --data_dir data/processed --side tail --anchor_class 0 --relation 1 --top_k 20 --novel \\
        --candidate_class 1 --node_types data/processed/mappings.pt --output_dir results/predictions

writes ``predictions.json``: ``{"protocol": {...}, "queries": [{"anchor", "relation", "candidates": [[id, score],
...]}]}``, best first, equal scores by id; with a ``mappings.pt`` as ``--node_types`` every query also carries
``anchor_name`` and ``candidate_names``.  ``--explain K`` adds to every query ``"paths"`` - per candidate the K
best-scoring simple paths of at most ``--max_path_length`` edges between anchor and candidate through the full graph
(``ModelEvaluator.explain``) - and ``"path_counts"``, per candidate the exact number of such paths of length 1..4.
"""
from __future__ import annotations

import argparse
import json
import logging
from pathlib import Path
from typing import Dict, Optional

import torch

from . import evaluate as E

logger = logging.getLogger("primekg_rgcn_linkprediction_amd.predict")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Top-k link predictions of a trained R-GCN link predictor on MI355X")
    p.add_argument("--model_path", type=str, required=True)
    p.add_argument("--data_dir", type=str, default="data/processed")
    p.add_argument("--output_dir", type=str, default="results/predictions")
    p.add_argument("--side", choices=("tail", "head"), default="tail",
                   help="tail: complete (anchor, relation, ?); head: complete (?, relation, anchor)")
    who = p.add_mutually_exclusive_group(required=True)
    who.add_argument("--anchors", type=int, nargs="+", help="node ids of the queries")
    who.add_argument("--anchor_class", type=int, help="every node of this class is a query (needs --node_types)")
    p.add_argument("--relation", type=int, required=True, help="relation id of the queries")
    p.add_argument("--top_k", type=int, default=10)
    p.add_argument("--novel", action="store_true",
                   help="leave out the candidates that form a known triple (full graph + test set) with their query")
    p.add_argument("--candidate_class", type=int, default=None,
                   help="only candidates of this node class (needs --node_types)")
    p.add_argument("--node_types", type=str, default=None,
                   help="the preprocessing's mappings.pt, or an .npz / .pt holding an int vector [num_nodes]")
    p.add_argument("--min_score", type=float, default=None, help="only candidates with a score >= this")
    p.add_argument("--explain", type=int, default=0, metavar="K",
                   help="also list the K best-scoring connecting paths of every (anchor, candidate) (0: off)")
    p.add_argument("--max_path_length", type=int, default=4, help="edges of the longest connecting path, 1..4")
    p.add_argument("--explain_by", choices=("cosine", "gradient", "mask"), default="cosine",
                   help="what scores a hop of a connecting path: the cosine of its two embedding rows, the gradient of "
                        "the candidate's score in the edge (what the model itself rests on), or an edge mask learned so "
                        "that few edges preserve the candidate's prediction")
    p.add_argument("--explain_edges", type=int, default=0, metavar="M",
                   help="with --explain_by gradient or mask: also list the M edges every candidate's score depends on most "
                        "(0: off)")
    p.add_argument("--mask_steps", type=int, default=100, help="with --explain_by mask: optimisation steps per candidate")
    p.add_argument("--mask_lr", type=float, default=0.1, help="with --explain_by mask: Adam's step size")
    p.add_argument("--explain_fidelity", action="store_true",
                   help="grade the explanations by the model: per candidate the score on the whole graph, with the M named "
                        "edges deleted and with only them kept, for the cosine, gradient and mask explainers side by side "
                        "(needs --explain K and --explain_edges M)")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--trust_checkpoint", action="store_true",
                   help="allow the unrestricted pickle loader for --model_path (only for files you wrote yourself)")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    parser = build_parser()
    args = parser.parse_args(argv)
    if (args.anchor_class is not None or args.candidate_class is not None) and not args.node_types:
        parser.error("--anchor_class / --candidate_class need --node_types PATH (mappings.pt, or an .npz / .pt int "
                     "vector [num_nodes])")
    if args.top_k < 1:
        parser.error("--top_k must be >= 1")
    if args.explain < 0:
        parser.error("--explain must be >= 0")
    if not 1 <= args.max_path_length <= 4:
        parser.error("--max_path_length must be in 1..4")
    if args.explain_edges < 0:
        parser.error("--explain_edges must be >= 0")
    if args.explain_edges > 0 and args.explain_by == "cosine" and not args.explain_fidelity:
        parser.error("--explain_edges lists attributed edges: it needs --explain_by gradient")
    if args.explain_by != "cosine" and args.explain < 1:
        parser.error(f"--explain_by {args.explain_by} ranks connecting paths: it needs --explain K with K >= 1")
    if args.mask_steps < 0:
        parser.error("--mask_steps must be >= 0")
    if not args.mask_lr > 0:
        parser.error("--mask_lr must be > 0")
    if args.explain_fidelity and (args.explain < 1 or args.explain_edges < 1):
        parser.error("--explain_fidelity deletes the M named edges of every candidate: it needs --explain K and "
                     "--explain_edges M, both >= 1")
    return args


def load_node_names(path: Optional[str]) -> Optional[Dict[int, str]]:
    """``{node id: name}`` when ``path`` is a ``mappings.pt`` with ``idx2node`` ((id, name, type) per node), else None"""
    if not path or str(path).endswith(".npz"):
        return None
    obj = torch.load(path, map_location="cpu", weights_only=True)
    if not (isinstance(obj, dict) and "idx2node" in obj):
        return None
    return {int(i): str(v[1]) for i, v in obj["idx2node"].items()}


def predict(evaluator, args: argparse.Namespace, names: Optional[Dict[int, str]] = None) -> Dict:
    """the queries of ``args`` through ``evaluator.top_candidates`` -> the ``predictions.json`` dict"""
    if args.anchor_class is not None:
        if evaluator.node_class is None:
            raise ValueError("--anchor_class needs the node classes (--node_types)")
        anchors = torch.nonzero(evaluator.node_class.cpu() == args.anchor_class).view(-1)
        if anchors.numel() == 0:
            raise ValueError(f"no node has class {args.anchor_class}")
    else:
        anchors = torch.tensor(args.anchors, dtype=torch.int64)
    relations = torch.full_like(anchors, args.relation)
    ids, scores = evaluator.top_candidates(args.side, anchors, relations, args.top_k, novel=args.novel,
                                           candidate_class=args.candidate_class, min_score=args.min_score)
    ids, scores = ids.cpu().tolist(), scores.cpu().tolist()
    queries = []
    for anchor, row_ids, row_scores in zip(anchors.tolist(), ids, scores):
        kept = [(i, s) for i, s in zip(row_ids, row_scores) if i >= 0]         # padding past the candidates dropped
        q = {"anchor": anchor, "relation": args.relation, "candidates": [[i, s] for i, s in kept]}
        if names is not None:
            q["anchor_name"] = names.get(anchor)
            q["candidate_names"] = [names.get(i) for i, _ in kept]
        queries.append(q)
    protocol = {"side": args.side, "top_k": args.top_k, "novel": bool(args.novel),
                "candidate_class": args.candidate_class, "anchor_class": args.anchor_class, "min_score": args.min_score,
                "order": "score descending, equal scores by id ascending"}
    explain = int(getattr(args, "explain", 0) or 0)
    if explain > 0:
        # the triple reads (anchor, relation, candidate) for tails and (candidate, relation, anchor) for heads
        pairs = [(q["anchor"], c) if args.side == "tail" else (c, q["anchor"]) for q in queries for c, _ in q["candidates"]]
        max_len = int(getattr(args, "max_path_length", 4))
        by, top_edges = getattr(args, "explain_by", "cosine"), int(getattr(args, "explain_edges", 0) or 0)
        edges, graded = None, None
        if by == "mask" or getattr(args, "explain_fidelity", False):
            kwargs = {"by": by, "relations": [args.relation], "top_edges": top_edges}
            if by == "mask" or args.explain_fidelity:
                kwargs.update(mask_steps=int(getattr(args, "mask_steps", 100)), mask_lr=float(getattr(args, "mask_lr", 0.1)))
            if getattr(args, "explain_fidelity", False):
                kwargs["fidelity"] = "all"
            got = evaluator.explain(pairs, explain, max_len, **kwargs) if pairs else ([], [], [], [])
            paths, counts = got[0], got[1]
            if by != "cosine":
                edges = got[2]
            if getattr(args, "explain_fidelity", False):
                graded = got[-1]
        elif by == "gradient":
            paths, counts, edges = (evaluator.explain(pairs, explain, max_len, by="gradient", relations=[args.relation],
                                                      top_edges=top_edges) if pairs else ([], [], []))
        else:
            paths, counts = evaluator.explain(pairs, explain, max_len) if pairs else ([], [])
        at = 0
        for q in queries:
            n = len(q["candidates"])
            q["paths"], q["path_counts"] = paths[at:at + n], counts[at:at + n]
            if edges is not None and top_edges > 0:
                q["edges"] = [[list(e) for e in per_candidate] for per_candidate in edges[at:at + n]]
            if graded is not None:
                q["fidelity"] = graded[at:at + n]
            at += n
            if names is not None:
                for per_candidate in q["paths"]:
                    for path in per_candidate:
                        path["node_names"] = [names.get(i) for i in path["nodes"]]
        protocol["paths"] = {"per_candidate": explain, "max_length": max_len,
                             "pair": "(anchor, candidate)" if args.side == "tail" else "(candidate, anchor)",
                             "score": "mean cosine of consecutive nodes * 1 / (1 + 0.2 * (edges - 1)), float32",
                             "order": "score descending, then fewer edges, then interior nodes ascending",
                             "path_counts": "simple paths of 1, 2, 3, 4 edges, all of them"}
        if by == "gradient":
            protocol["paths"]["score"] = ("mean over the hops of the largest |d score / d edge mask| of the columns naming "
                                          "the hop * 1 / (1 + 0.2 * (edges - 1)), float32")
            if top_edges > 0:
                protocol["edges"] = {"per_candidate": top_edges, "entry": "[column, source, relation, target, d score / d edge mask]",
                                     "order": "|value| descending, equal magnitudes by column ascending"}
        if by == "mask":
            protocol["paths"]["score"] = ("mean over the hops of the largest learned mask value of the columns naming the "
                                          "hop * 1 / (1 + 0.2 * (edges - 1)), float32")
            protocol["mask"] = {"steps": int(getattr(args, "mask_steps", 100)), "lr": float(getattr(args, "mask_lr", 0.1))}
            if top_edges > 0:
                protocol["edges"] = {"per_candidate": top_edges, "entry": "[column, source, relation, target, mask value]",
                                     "order": "mask value descending inside the pair's receptive field, equal values by "
                                              "column ascending"}
        if graded is not None:
            protocol["fidelity"] = {"explainers": ["cosine", "gradient", "mask"], "edges_per_explainer": top_edges,
                                    "full": "the score on the whole graph",
                                    "without": "the score with the explainer's edges deleted",
                                    "only": "the score with only the explainer's edges kept inside the pair's receptive field"}
    return {"protocol": protocol, "queries": queries}


def save_predictions(result: Dict, output_dir) -> Path:
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    path = output_dir / "predictions.json"
    with open(path, "w") as fh:
        json.dump(result, fh, indent=2)
    return path


def main(argv=None) -> Dict:
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(name)s - %(levelname)s - %(message)s")
    args = parse_args(argv)
    device = torch.device(args.device)
    model, _ = E.load_model(args.model_path, device, trust_pickle=args.trust_checkpoint)
    test_data, full_graph = E.load_test_data(args.data_dir)
    node_class = E.load_node_classes(args.node_types, int(full_graph["num_nodes"])) if args.node_types else None
    evaluator = E.ModelEvaluator(model, test_data, full_graph, device, node_class=node_class)
    result = predict(evaluator, args, load_node_names(args.node_types))
    path = save_predictions(result, args.output_dir)
    logger.info("%d queries, top %d each, saved to: %s", len(result["queries"]), args.top_k, path)
    return result


if __name__ == "__main__":
    main()
