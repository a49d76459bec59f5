"""Evaluation protocol on the HIP path (SURVEY.md section 8f "next" row 2).

Counterpart of the reference's ``src/evaluate.py`` minus its plots: same command line
(``--model_path --data_dir --output_dir --batch_size --num_neg_samples --k_values --device``,
``evaluate.py:766-827``), same checkpoint reading (N and R recovered from the state dict,
``evaluate.py:655-730``), same protocol, metric names and return shapes, same ``results.json`` /
``metrics_summary.txt`` (``evaluate.py:594-652``; cf. ``results_final/results.json``), with the two
hot spots removed -

* ``compute_scores_and_labels`` (``evaluate.py:147-217``): positives + random corruptions of the
  test triples scored over the FULL graph.  The encoder runs ONCE, not once per 1,024-edge batch.
* ``compute_ranking_metrics`` (``evaluate.py:219-299``): rank of the true tail among all
  entities.  The reference re-encodes per batch and, per test edge, argsorts 30,926 scores in a
  Python loop; here the encoder runs once and ``LinkPredictor.rank_tails`` returns every rank
  from one fused MFMA pass (no [B, N] score matrix, no sort).
"""
from __future__ import annotations

import argparse
import json
import logging
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .model import DrugDiseaseModel
from .train import NegativeSampler, filter_edges

logger = logging.getLogger("primekg_rgcn_linkprediction_amd.evaluate")


class ModelEvaluator:
    def __init__(self, model: DrugDiseaseModel, test_data: Dict, full_graph: Dict, device: torch.device,
                 batch_size: int = 1024, node_class: Optional[torch.Tensor] = None):
        self.model = model.to(device).eval()
        self.node_class = None if node_class is None else torch.as_tensor(node_class).to(device=device, dtype=torch.int32)
        self._known = self._classes = self._path_graph = self._edge_cosine = None
        self.device, self.batch_size = device, batch_size
        self.test_edge_index = test_data["edge_index"].to(device)
        self.test_edge_type = test_data["edge_type"].to(device)
        self.full_edge_index = full_graph["edge_index"].to(device)
        self.full_edge_type = full_graph["edge_type"].to(device)
        self.num_nodes = int(full_graph["num_nodes"])
        self.num_test_edges = int(self.test_edge_index.size(1))
        self._emb = None
        self.nonfinite_rows = None       # rows of the embedding table with a NaN or an infinity; set by embeddings()

    @torch.no_grad()
    def embeddings(self) -> torch.Tensor:
        """node embeddings of the full graph, encoded once and kept.  The first call counts the rows that hold a NaN or
        an infinity (``nonfinite_rows``) and warns when there are any: every rank such a row takes part in is then a
        statement about the missing value, not about the model (a NaN true score ranks last among its eligible
        candidates, a NaN candidate counts against every true score - ``LinkPredictor.rank_tails``)."""
        if self._emb is None:
            self._emb = self.model.encoder(self.full_edge_index, self.full_edge_type)
            self.nonfinite_rows = int((~torch.isfinite(self._emb)).any(dim=1).sum())
            if self.nonfinite_rows:
                logger.warning("%d of %d node embedding rows hold a NaN or an infinity: the ranking metrics count every "
                               "such row against the model", self.nonfinite_rows, self._emb.size(0))
        return self._emb

    @torch.no_grad()
    def compute_scores_and_labels(self, num_neg_samples: int = 1, filtered: bool = False,
                                  type_constrained: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """-> (sigmoid scores, labels): every test column + ``num_neg_samples`` corruptions.  ``filtered``: no
        corruption is a known triple (``known_triples()``; up to ``NEGATIVE_TRIES`` draws each); ``type_constrained``:
        a node is replaced by one of its own class.  Either one draws from the constrained device sampler (cursor =
        the batch start, key = torch's seed): the same negatives every time."""
        emb = self.embeddings()
        if filtered or type_constrained:
            return self._constrained_scores_and_labels(emb, num_neg_samples, **self._protocol(filtered, type_constrained))
        sampler = NegativeSampler(self.num_nodes, num_neg_samples)
        head, tail, rel = self.test_edge_index[0], self.test_edge_index[1], self.test_edge_type
        scores, labels = [], []
        for lo in range(0, self.num_test_edges, self.batch_size):
            h, t, r = head[lo: lo + self.batch_size], tail[lo: lo + self.batch_size], rel[lo: lo + self.batch_size]
            nh, nt, nr = sampler.sample(h, t, r)
            s = self.model.decoder.score_triples(emb, torch.cat([h, nh]), torch.cat([t, nt]), torch.cat([r, nr]))
            scores.append(torch.sigmoid(s))
            labels.append(torch.cat([torch.ones(h.numel(), device=self.device),
                                     torch.zeros(nh.numel(), device=self.device)]))
        return torch.cat(scores).cpu().numpy(), torch.cat(labels).cpu().numpy()

    NEGATIVE_TRIES = 16          # draws per filtered negative before the last one is kept
    NEGATIVE_STREAM = (1 << 55) + 1   # Philox stream of these negatives: no training epoch, not validate()'s

    def _constrained_scores_and_labels(self, emb, num_neg_samples: int, known, node_class):
        from . import ops
        classes = None
        if node_class is not None:
            if self._classes is None:
                self._classes = ops.NodeClasses(node_class, max(int(node_class.max()) + 1, 1))
            classes = self._classes
        starts = torch.arange(0, max(self.num_test_edges, 1), self.batch_size, device=self.device, dtype=torch.int64)
        rng = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, self.NEGATIVE_STREAM], dtype=torch.int64).to(self.device)
        self.negative_stats = torch.zeros(2, dtype=torch.int64, device=self.device)
        scores, labels, triples = [], [], []
        for i, lo in enumerate(range(0, self.num_test_edges, self.batch_size)):
            h, t, r, y = ops.sample_batch_constrained(
                self.test_edge_index, self.test_edge_type, None, starts[i:i + 1], min(self.batch_size, self.num_test_edges - lo),
                num_neg_samples, self.num_nodes, rng, classes=classes, known=known, max_tries=self.NEGATIVE_TRIES,
                stats=self.negative_stats)
            triples.append((h, t, r))
            scores.append(torch.sigmoid(self.model.decoder.score_triples(emb, h, t, r)))
            labels.append(y)
        self.scored_triples = tuple(torch.cat(p) for p in zip(*triples))     # (heads, tails, rels) in score order
        return torch.cat(scores).cpu().numpy(), torch.cat(labels).cpu().numpy()

    def known_triples(self):
        """the known positives of the filtered protocol: the full graph (train, validation and test edges in the
        reference's split) united with the test triples, as CSRs on the device; built on first use"""
        if self._known is None:
            from . import ops
            self._known = ops.KnownTriples(torch.cat([self.full_edge_index, self.test_edge_index], 1),
                                           torch.cat([self.full_edge_type, self.test_edge_type]), self.num_nodes,
                                           self.model.decoder.num_relations)
        return self._known

    def _protocol(self, filtered: bool, type_constrained: bool) -> Dict:
        if type_constrained and self.node_class is None:
            raise ValueError("type-constrained ranking needs the node classes (ModelEvaluator(node_class=...), "
                             "--node_types on the command line)")
        return {"known": self.known_triples() if filtered else None,
                "node_class": self.node_class if type_constrained else None}

    @torch.no_grad()
    def tail_ranks(self, filtered: bool = False, type_constrained: bool = False) -> torch.Tensor:
        """int64 [num_test_edges]: 1-based rank of every true tail among all entities (``filtered``: known positives
        do not count; ``type_constrained``: among the entities of the true tail's class)"""
        emb = self.embeddings()
        head, tail, rel = self.test_edge_index[0], self.test_edge_index[1], self.test_edge_type
        if not (filtered or type_constrained):
            return self.model.decoder.rank_tails(emb[head], rel, emb, tail)
        return self.model.decoder.rank_tails(emb[head], rel, emb, tail, head_indices=head,
                                             **self._protocol(filtered, type_constrained))

    @torch.no_grad()
    def head_ranks(self, filtered: bool = False, type_constrained: bool = False) -> torch.Tensor:
        """int64 [num_test_edges]: 1-based rank of every true head, the other side of the same triples"""
        emb = self.embeddings()
        head, tail, rel = self.test_edge_index[0], self.test_edge_index[1], self.test_edge_type
        return self.model.decoder.rank_heads(emb[tail], rel, emb, head, tail_indices=tail,
                                             **self._protocol(filtered, type_constrained))

    @torch.no_grad()
    def top_candidates(self, side: str, anchors, relations, k: int, novel: bool = True, candidate_class=None,
                       min_score: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(ids int64 [B, k], scores [B, k])``: the ``k`` best completions of every ``(anchor, relation)`` query on
        the cached embeddings - tails of ``(anchor, relation, ?)`` for ``side="tail"``, heads of ``(?, relation,
        anchor)`` for ``side="head"``; scores descending, equal scores by id ascending, id -1 / score -inf past the
        number of candidates.  ``novel``: no returned id forms a known triple (``known_triples()``: full graph +
        test set) with its query.  ``candidate_class`` (an int or one int per query; needs the node classes): only
        entities of that class."""
        if side not in ("tail", "head"):
            raise ValueError("side must be 'tail' or 'head'")
        if candidate_class is not None and self.node_class is None:
            raise ValueError("candidate_class needs the node classes (ModelEvaluator(node_class=...), "
                             "--node_types on the command line)")
        emb = self.embeddings()
        anchors = torch.as_tensor(anchors, dtype=torch.int64).to(self.device).view(-1)
        relations = torch.as_tensor(relations, dtype=torch.int64).to(self.device).view(-1)
        if relations.numel() == 1 and anchors.numel() != 1:
            relations = relations.expand(anchors.numel()).contiguous()
        if relations.shape != anchors.shape:
            raise ValueError("one relation per anchor (or a single relation for all) expected")
        if anchors.numel() and (int(anchors.min()) < 0 or int(anchors.max()) >= self.num_nodes):
            raise IndexError("an anchor id is outside [0, num_nodes)")
        if relations.numel() and (int(relations.min()) < 0 or int(relations.max()) >= self.model.decoder.num_relations):
            raise IndexError("a relation id is outside [0, num_relations)")
        if isinstance(candidate_class, torch.Tensor):
            candidate_class = candidate_class.to(self.device)
        kwargs = {"known": self.known_triples() if novel else None,
                  "node_class": self.node_class if candidate_class is not None else None,
                  "candidate_class": candidate_class, "min_score": min_score}
        if side == "tail":
            return self.model.decoder.top_tails(emb[anchors], relations, emb, k, head_indices=anchors, **kwargs)
        return self.model.decoder.top_heads(emb[anchors], relations, emb, k, tail_indices=anchors, **kwargs)

    @torch.no_grad()
    def explain(self, pairs, k: int = 5, max_len: int = 4, by: str = "cosine", relations=None, top_edges: int = 0,
                fidelity=False, mask_steps: int = 100, mask_lr: float = 0.1):
        """why a pair is predicted: for every ``(source, target)`` of ``pairs`` the ``k`` best-scoring simple paths of at
        most ``max_len`` edges through the full graph (``consumers.connecting_paths`` on the cached embeddings) and the
        exact number of such paths of length 1..4 -> ``(paths, counts)``.  The full graph's ``PathGraph`` and the cosine
        of every edge are built on first use and kept.

        ``by="gradient"`` asks the model instead of the embeddings' geometry -> ``(paths, counts, edges)``: every pair is
        the triple ``(source, relations[q], target)`` (``relations`` is required: one id per pair, or one for all), its
        score is attributed to the edges of the full graph (``attribution.edge_attribution``, one pair at a time), a
        hop scores the largest ``|attribution|`` of the columns that name it (``consumers.attribution_edge_score``)
        and the paths are ranked as before; ``edges[q]``: the ``top_edges`` columns the score depends on most
        (``consumers.attributed_edges``).

        ``by="mask"`` OPTIMISES an explanation -> ``(paths, counts, edges)`` likewise: per pair a soft edge mask is learned
        so that few edges preserve the prediction (``attribution.learn_edge_mask``, ``mask_steps`` steps of Adam at
        ``mask_lr``), a hop scores the largest mask value of the columns that name it, and ``edges[q]`` are the
        ``top_edges`` columns the mask keeps most (``consumers.masked_edges``).

        ``fidelity`` grades the explanation by the model itself and appends one more element, per pair ``{explainer:
        {"full", "without", "only"}}`` (``consumers.explanation_fidelity``): the score on the whole graph, with the
        explainer's ``top_edges`` columns deleted, and with only those kept inside the pair's receptive field.  ``True``:
        the explainer of ``by``; ``"all"``: cosine, gradient and mask side by side.  The cosine route names no columns
        itself: its set is the columns of the hops of its listed paths, best path first, up to ``top_edges``.  Needs
        ``relations``."""
        from . import consumers, ops
        if by not in ("cosine", "gradient", "mask"):
            raise ValueError(f"by must be 'cosine', 'gradient' or 'mask', got {by!r}")
        if fidelity not in (False, True, "all"):
            raise ValueError(f"fidelity must be False, True or 'all', got {fidelity!r}")
        if (by != "cosine" or fidelity) and relations is None:
            raise ValueError(f"explain(by={by!r}, fidelity={fidelity!r}) explains the score of a triple: relations (one per "
                             "pair) is required")
        if by != "cosine" or fidelity:
            from . import attribution
            attribution._refuse_attention(getattr(self.model, "encoder", None), f"explain(by={by!r}, fidelity={fidelity!r})")
        if fidelity:
            return self._explain_graded(pairs, k, max_len, by, relations, int(top_edges), fidelity, mask_steps, mask_lr)
        if by == "gradient":
            return self._explain_by_gradient(pairs, k, max_len, relations, int(top_edges))
        if by == "mask":
            return self._explain_by_mask(pairs, k, max_len, relations, int(top_edges), mask_steps, mask_lr)
        if self._path_graph is None:
            self._path_graph = ops.PathGraph(self.full_edge_index, self.full_edge_type, self.num_nodes)
        emb = self.embeddings()
        if self._edge_cosine is None:
            self._edge_cosine = ops.edge_cosine(emb.contiguous(), self._path_graph)
        return consumers.connecting_paths(emb, self._path_graph, pairs, k, max_len, return_counts=True,
                                          edge_score=self._edge_cosine)

    def _explain_by_gradient(self, pairs, k: int, max_len: int, relations, top_edges: int):
        from . import attribution, consumers
        pairs = torch.as_tensor(pairs, dtype=torch.int64).reshape(-1, 2)
        relations = torch.as_tensor(relations, dtype=torch.int64).view(-1)
        if relations.numel() == 1 and pairs.size(0) != 1:
            relations = relations.expand(pairs.size(0))
        if relations.numel() != pairs.size(0):
            raise ValueError("one relation per pair (or a single relation for all) expected")
        graph, emb = self._structure(), self.embeddings()
        paths, counts, edges = [], [], []
        for (h, t), r in zip(pairs.tolist(), relations.tolist()):
            attr = attribution.edge_attribution(self.model, self.full_edge_index, self.full_edge_type, [h], [r], [t])
            hop_score = consumers.attribution_edge_score(attr, graph, self.full_edge_index)
            p, c = consumers.connecting_paths(emb, graph, [(h, t)], k, max_len, return_counts=True, edge_score=hop_score)
            paths.extend(p)
            counts.extend(c)
            edges.append(consumers.attributed_edges(attr, self.full_edge_index, self.full_edge_type, top_edges))
        return paths, counts, edges

    def _pairs_relations(self, pairs, relations):
        pairs = torch.as_tensor(pairs, dtype=torch.int64).reshape(-1, 2)
        relations = torch.as_tensor(relations, dtype=torch.int64).view(-1)
        if relations.numel() == 1 and pairs.size(0) != 1:
            relations = relations.expand(pairs.size(0))
        if relations.numel() != pairs.size(0):
            raise ValueError("one relation per pair (or a single relation for all) expected")
        return pairs.tolist(), relations.tolist()

    def _explain_by_mask(self, pairs, k: int, max_len: int, relations, top_edges: int, steps: int, lr: float):
        from . import attribution, consumers
        pairs, relations = self._pairs_relations(pairs, relations)
        graph, emb = self._structure(), self.embeddings()
        paths, counts, edges = [], [], []
        for (h, t), r in zip(pairs, relations):
            result = attribution.learn_edge_mask(self.model, self.full_edge_index, self.full_edge_type, h, r, t, steps=steps, lr=lr)
            hop_score = consumers.mask_edge_score(result, graph, self.full_edge_index)
            p, c = consumers.connecting_paths(emb, graph, [(h, t)], k, max_len, return_counts=True, edge_score=hop_score)
            paths.extend(p)
            counts.extend(c)
            edges.append(consumers.masked_edges(result, self.full_edge_index, self.full_edge_type, top_edges))
        return paths, counts, edges

    def _path_columns(self, per_pair, limit: int):
        """the columns of the hops of a pair's listed paths, best path first, without repeats, at most ``limit``: per hop
        the lowest column that names it"""
        ei = self.full_edge_index
        cols = []
        for path in per_pair:
            for a, b in zip(path["nodes"][:-1], path["nodes"][1:]):
                hit = torch.nonzero((ei[0] == a) & (ei[1] == b)).view(-1)
                if hit.numel() and int(hit[0]) not in cols:
                    cols.append(int(hit[0]))
        return cols[:max(limit, 0)]

    def _explain_graded(self, pairs, k, max_len, by, relations, top_edges, fidelity, steps, lr):
        from . import consumers
        pairs, relations = self._pairs_relations(pairs, relations)
        routes = ("cosine", "gradient", "mask") if fidelity == "all" else (by,)
        found = {}
        for route in routes:
            if route == "cosine":
                p, c = self.explain(pairs, k, max_len)
                found[route] = (p, c, [[(col,) for col in self._path_columns(per_pair, top_edges)] for per_pair in p])
            elif route == "gradient":
                found[route] = self._explain_by_gradient(pairs, k, max_len, relations, top_edges)
            else:
                found[route] = self._explain_by_mask(pairs, k, max_len, relations, top_edges, steps, lr)
        sets = [{route: [edge[0] for edge in found[route][2][q]] for route in routes} for q in range(len(pairs))]
        graded = consumers.explanation_fidelity(self.model, self.full_edge_index, self.full_edge_type, pairs, relations, sets)
        paths, counts, edges = found[by]
        if by == "cosine":
            return paths, counts, graded
        return paths, counts, edges, graded

    def _structure(self):
        """the full graph's ``PathGraph``, built on first use and kept (``explain`` shares it)"""
        from . import ops
        if self._path_graph is None:
            self._path_graph = ops.PathGraph(self.full_edge_index, self.full_edge_type, self.num_nodes)
        return self._path_graph

    @torch.no_grad()
    def subgraph_stats(self, pairs, radius: int = 2, class_names=None, common_cap: int = 0):
        """the structural context of every ``(drug, disease)`` of ``pairs`` in the full graph:
        ``consumers.pair_subgraph_stats`` on the cached ``PathGraph`` and the evaluator's node classes"""
        from . import consumers
        return consumers.pair_subgraph_stats(self._structure(), pairs, radius, self.node_class, class_names, common_cap)

    @torch.no_grad()
    def failure_analysis(self, pairs, labels, radius: int = 2, num_failures: int = 5, num_successes: int = 5,
                         class_names=None, common_cap: int = 0, max_len: int = 4):
        """which labelled ``(drug, disease)`` pairs the embeddings get wrong, and how their neighbourhoods differ from
        the ones they get right: ``consumers.failure_analysis`` on the cached embeddings, ``PathGraph``, edge cosines
        and node classes"""
        from . import consumers, ops
        graph, emb = self._structure(), self.embeddings()
        if self._edge_cosine is None:
            self._edge_cosine = ops.edge_cosine(emb.contiguous(), graph)
        return consumers.failure_analysis(emb, graph, pairs, labels, radius, num_failures, num_successes, self.node_class,
                                          class_names, common_cap, max_len, edge_score=self._edge_cosine)

    @torch.no_grad()
    def cluster_analysis(self, class_names, n_clusters: int = 10, **kmeans_kw):
        """which nodes of a type the model groups together, and how well separated the groups are:
        ``consumers.cluster_analysis`` (k-means + silhouette per node type, on the device) on the cached embeddings and
        the evaluator's node classes"""
        from . import consumers
        if self.node_class is None:
            raise ValueError("cluster_analysis needs the node classes (ModelEvaluator(node_class=...), e.g. "
                             "graphio.node_classes(mappings['idx2node'], num_nodes)[0])")
        return consumers.cluster_analysis(self.embeddings(), self.node_class, class_names, n_clusters, **kmeans_kw)

    @torch.no_grad()
    def compare_methods(self, train_data: Dict, methods: Sequence[str] = ("random", "degree", "transe", "rgcn"),
                        k_values: Sequence[int] = (1, 5, 10, 20, 50), filtered: bool = False, type_constrained: bool = False,
                        both_sides: bool = False, transe_epochs: int = 50, seed: int = 0, drug_class: Optional[int] = None,
                        disease_class: Optional[int] = None, bootstrap: int = 0, bootstrap_seed: int = 0,
                        by_frequency: bool = False, **transe_kwargs) -> Dict:
        """this model next to the Random, Node Degree and TransE baselines (``baselines.py``, fitted on ``train_data``),
        every method under one ranking protocol on the test triples and one set of labelled per-triple scores:
        ``compare.compare_methods`` on the evaluator's test set, full graph and node classes.  ``bootstrap`` > 0 adds
        intervals per method and paired p-values per pair of methods, ``by_frequency`` the split by disease degree."""
        from . import compare
        test = {"edge_index": self.test_edge_index, "edge_type": self.test_edge_type}
        full = {"edge_index": self.full_edge_index, "edge_type": self.full_edge_type, "num_nodes": self.num_nodes,
                "num_relations": self.model.decoder.num_relations}
        return compare.compare_methods(train_data, test, full, self.device, self.model, self.node_class, methods, k_values,
                                       filtered, type_constrained, both_sides, transe_epochs, seed, drug_class,
                                       disease_class, transe_kwargs or None, bootstrap, bootstrap_seed, by_frequency)

    @torch.no_grad()
    def reduce_dimensions(self, method: str = "tsne", sample_size: Optional[int] = None, random_state: int = 42, **tsne_kw):
        """the 2-D t-SNE projection of (a sample of) the cached embeddings, on the device:
        ``consumers.reduce_dimensions`` -> ``(xy float32 [n, 2], sample_indices [n])`` (and the ``ops.TSNEResult`` with
        ``return_result=True``)"""
        from . import consumers
        return consumers.reduce_dimensions(self.embeddings(), method, sample_size, random_state, **tsne_kw)

    def compute_ranking_metrics(self, k_values: Sequence[int] = (10, 50), filtered: bool = False,
                                type_constrained: bool = False, both_sides: bool = False) -> Dict:
        ranks = self.tail_ranks(filtered, type_constrained)
        if both_sides:
            ranks = torch.cat([ranks, self.head_ranks(filtered, type_constrained)])
        ranks = ranks.cpu().numpy().astype(np.float64)
        metrics = {"mrr": float(np.mean(1.0 / ranks)), "mean_rank": float(np.mean(ranks)),
                   "median_rank": float(np.median(ranks))}
        for k in k_values:
            metrics[f"hits@{k}"] = float(np.mean(ranks <= k))
        return metrics

    @staticmethod
    def compute_classification_metrics(scores: np.ndarray, labels: np.ndarray, threshold: float = 0.5) -> Dict:
        from sklearn.metrics import (average_precision_score, f1_score, precision_score, recall_score,
                                     roc_auc_score)
        pred = (scores >= threshold).astype(int)
        return {"auc_roc": float(roc_auc_score(labels, scores)),
                "auc_pr": float(average_precision_score(labels, scores)),
                "precision": float(precision_score(labels, pred)), "recall": float(recall_score(labels, pred)),
                "f1_score": float(f1_score(labels, pred)), "threshold": threshold}

    def _sample_units(self, num_neg_samples: int) -> torch.Tensor:
        """int32: the test triple of every entry of ``compute_scores_and_labels`` - per batch its positives, then
        ``num_neg_samples`` corruptions of each, one after the other"""
        units = []
        for lo in range(0, self.num_test_edges, self.batch_size):
            own = torch.arange(lo, min(lo + self.batch_size, self.num_test_edges), dtype=torch.int32, device=self.device)
            units += [own, own.repeat_interleave(num_neg_samples)]
        return torch.cat(units) if units else torch.zeros(0, dtype=torch.int32, device=self.device)

    @torch.no_grad()
    def bootstrap(self, replicates: int, seed: int = 0, filtered: bool = False, type_constrained: bool = False,
                  both_sides: bool = False, num_neg_samples: int = 1, k_values: Sequence[int] = (10, 50)) -> Dict:
        """Intervals for the metrics of ``evaluate`` from ``replicates`` Poisson bootstrap resamples of the test
        triples, on the device (``ops.classification_counts`` / ``ops.rank_sums``): per metric (``auc_roc``,
        ``auc_pr``, ``f1_score``, ``mrr``, ``mean_rank``, each ``hits@k``) the point estimate, the standard error and
        the 2.5 / 97.5 percentile interval, plus ``replicates``, ``seed`` and ``degenerate_replicates`` (dropped: a
        class had no weight).  A triple keeps its corruptions, and its tail query its head query: they share a weight.
        The scores are those of the last ``evaluate`` under the same options when there was one.  The median rank is
        not a sum over queries and is not resampled."""
        from . import bootstrap as BS
        key = (num_neg_samples, bool(filtered), bool(type_constrained))
        if getattr(self, "_scores_key", None) != key:
            self.scores, self.labels = self.compute_scores_and_labels(num_neg_samples, filtered, type_constrained)
            self._scores_key = key
        ranks = self.tail_ranks(filtered, type_constrained)
        if both_sides:
            ranks = torch.cat([ranks, self.head_ranks(filtered, type_constrained)])
        scores, labels = (torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in (self.scores, self.labels))
        vectors, degenerate, w_sum = BS.replicate_vectors(scores, labels, self._sample_units(num_neg_samples), ranks,
                                                          BS.query_units(self.num_test_edges, ranks.numel(), self.device),
                                                          k_values, replicates, seed)
        out = BS.block(vectors, degenerate, replicates, seed, w_sum)
        out["protocol"] = {"filtered": bool(filtered), "type_constrained": bool(type_constrained),
                           "sides": "both" if both_sides else "tail", "num_neg_samples": num_neg_samples}
        return out

    def evaluate(self, num_neg_samples: int = 1, k_values: List[int] = (10, 50), filtered: bool = False,
                 type_constrained: bool = False, both_sides: bool = False) -> Dict:
        """the reference's four keys; with any of the three protocol options one more, ``"ranking_filtered"``: the
        same metric names under that protocol plus ``"protocol"`` saying which it was"""
        scores, labels = self.compute_scores_and_labels(num_neg_samples, filtered, type_constrained)
        self.scores, self.labels = scores, labels          # kept for plotting code, as the reference does
        self._scores_key = (num_neg_samples, bool(filtered), bool(type_constrained))
        metrics = {"classification": self.compute_classification_metrics(scores, labels),
                   "ranking": self.compute_ranking_metrics(k_values),
                   "test_edges": self.num_test_edges, "num_nodes": self.num_nodes}
        if filtered or type_constrained or both_sides:
            metrics["ranking_filtered"] = dict(
                self.compute_ranking_metrics(k_values, filtered, type_constrained, both_sides),
                protocol={"filtered": bool(filtered), "type_constrained": bool(type_constrained),
                          "sides": "both" if both_sides else "tail"})
        from . import ops
        ops.check_indices(self.device)                     # an id outside the embedding table anywhere above: IndexError
        return metrics


# ------------------------------------------------------------------------------------------
# checkpoint / data / results files / CLI
# ------------------------------------------------------------------------------------------
def load_model(model_path: str, device: torch.device, trust_pickle: bool = False) -> Tuple[DrugDiseaseModel, Dict]:
    """-> (model in eval mode on ``device``, model_info).  A training checkpoint pickles its
    argparse ``Namespace`` next to the tensors (``train.py:431-442``; the reference therefore loads with
    ``weights_only=False``, ``evaluate.py:672``).  Here the file is read with the restricted unpickler
    (``weights_only=True``) that is allowed exactly one extra class, ``argparse.Namespace`` - nothing in the
    file can execute.  ``trust_pickle=True`` (CLI ``--trust_checkpoint``) falls back to the unrestricted
    loader for checkpoints that hold other objects: only for files you wrote yourself."""
    import argparse
    try:
        with torch.serialization.safe_globals([argparse.Namespace]):
            checkpoint = torch.load(model_path, map_location="cpu", weights_only=True)
    except Exception as exc:
        if not trust_pickle:
            raise RuntimeError(f"{model_path} holds objects the restricted loader refuses ({exc}); re-run with "
                               f"--trust_checkpoint if (and only if) you wrote this file yourself") from exc
        checkpoint = torch.load(model_path, map_location="cpu", weights_only=False)
    args = checkpoint.get("args")
    if args is None:
        raise ValueError("Checkpoint does not contain 'args'. Cannot reconstruct model architecture.")
    state = checkpoint["model_state_dict"]
    num_nodes = state["encoder.node_embeddings.weight"].size(0)
    num_relations = state["decoder.relation_embeddings.weight"].size(0)
    model = DrugDiseaseModel(num_nodes=num_nodes, num_relations=num_relations, embedding_dim=args.embedding_dim,
                             hidden_dim=args.hidden_dim, dropout=args.dropout,
                             decoder_dropout=getattr(args, "decoder_dropout", 0.0),
                             num_bases=getattr(args, "num_bases", None),
                             decoder=getattr(args, "decoder", "distmult"),
                             attention=bool(getattr(args, "attention", False)),
                             attention_slope=float(getattr(args, "attention_slope", 0.2)))
    model.load_state_dict(state)
    model = model.to(device).eval()
    info = {"checkpoint_path": str(model_path), "epoch": checkpoint.get("epoch", "unknown"), "num_nodes": num_nodes,
            "num_relations": num_relations, "embedding_dim": args.embedding_dim, "hidden_dim": args.hidden_dim,
            "decoder": model.decoder.decoder, "num_parameters": sum(p.numel() for p in model.parameters())}
    for key in ("best_val_loss", "best_val_acc"):
        if key in checkpoint:
            info[key] = checkpoint[key]
    return model, info


def load_test_data(data_dir: str) -> Tuple[Dict, Dict]:
    """``test_data.pt`` and ``full_graph.pt`` (tensor-only dicts: ``weights_only=True``) with the
    reference's out-of-range filter applied."""
    root = Path(data_dir)
    test = torch.load(root / "test_data.pt", weights_only=True)
    full = torch.load(root / "full_graph.pt", weights_only=True)
    n = test["num_nodes"]
    return filter_edges(test, n, "Test"), filter_edges(full, n, "Full graph")


def save_results(metrics: Dict, output_dir: Path, model_info: Optional[Dict] = None) -> None:
    """``results.json`` ({"metrics", "model_info"}) and ``metrics_summary.txt`` in the reference's layout."""
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    with open(output_dir / "results.json", "w") as fh:
        json.dump({"metrics": metrics, "model_info": model_info or {}}, fh, indent=2)
    rule = "=" * 60
    lines = [rule, "EVALUATION RESULTS SUMMARY", rule, ""]
    if model_info:
        lines += ["Model Information:", "-" * 60] + [f"{k}: {v}" for k, v in model_info.items()] + [""]
    lines += ["Dataset Statistics:", "-" * 60, f"Test edges: {metrics['test_edges']:,}",
              f"Number of nodes: {metrics['num_nodes']:,}", ""]
    for title, key in (("Classification Metrics:", "classification"), ("Ranking Metrics:", "ranking")):
        lines += [title, "-" * 60] + [f"{k}: {v:.4f}" for k, v in metrics[key].items()] + [""]
    if "ranking_filtered" in metrics:
        block = metrics["ranking_filtered"]
        proto = block["protocol"]
        lines += [f"Ranking Metrics (filtered: {proto['filtered']}, type-constrained: {proto['type_constrained']}, "
                  f"sides: {proto['sides']}):", "-" * 60]
        lines += [f"{k}: {v:.4f}" for k, v in block.items() if k != "protocol"] + [""]
    lines.append(rule)
    (output_dir / "metrics_summary.txt").write_text("\n".join(lines) + "\n")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Evaluate a trained R-GCN link predictor on MI355X")
    p.add_argument("--model_path", type=str, required=True)
    p.add_argument("--data_dir", type=str, default="data/processed")
    p.add_argument("--output_dir", type=str, default="results")
    p.add_argument("--batch_size", type=int, default=1024)
    p.add_argument("--num_neg_samples", type=int, default=1)
    p.add_argument("--k_values", type=int, nargs="+", default=[10, 50])
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--trust_checkpoint", action="store_true",
                   help="allow the unrestricted pickle loader for --model_path (only for files you wrote yourself)")
    p.add_argument("--filtered", action="store_true",
                   help="also rank with the known triples (full graph + test set) filtered out of the candidates")
    p.add_argument("--type_constrained", action="store_true",
                   help="also rank among the entities of the true target's node type only (needs --node_types)")
    p.add_argument("--both_sides", action="store_true", help="also rank the heads and average over both sides")
    p.add_argument("--node_types", type=str, default=None,
                   help="the preprocessing's mappings.pt, or an .npz / .pt holding an int vector [num_nodes]")
    p.add_argument("--bootstrap", type=int, default=0,
                   help="bootstrap replicates over the test triples: a \"bootstrap\" block with intervals in results.json (0: off)")
    p.add_argument("--bootstrap_seed", type=int, default=0)
    return p


def parse_args(argv=None) -> argparse.Namespace:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.bootstrap < 0 or args.bootstrap > 65535:
        parser.error("--bootstrap must be in [0, 65535]")
    if args.type_constrained and not args.node_types:
        parser.error("--type_constrained needs --node_types PATH (mappings.pt, or an .npz / .pt int vector [num_nodes])")
    return args


def load_node_classes(path: str, num_nodes: int) -> torch.Tensor:
    """int32 [num_nodes] from ``mappings.pt`` (dicts of str / int / tuple only: ``weights_only=True``) or from an
    ``.npz`` / ``.pt`` that holds the vector itself (under ``node_class``, or as its only entry)."""
    if str(path).endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            name = "node_class" if "node_class" in z.files else next(k for k in z.files if z[k].dtype.kind in "iu" and z[k].ndim == 1)
            classes = torch.from_numpy(z[name].astype(np.int32))
    else:
        obj = torch.load(path, map_location="cpu", weights_only=True)
        if isinstance(obj, dict) and "idx2node" in obj:
            from .graphio import node_classes
            classes = node_classes(obj["idx2node"], num_nodes)[0]
        else:
            classes = torch.as_tensor(obj["node_class"] if isinstance(obj, dict) else obj).to(torch.int32)
    if classes.shape != (num_nodes,):
        raise ValueError(f"{path}: expected one class per node ([{num_nodes}]), got {tuple(classes.shape)}")
    return classes


def main(argv=None) -> Dict:
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(name)s - %(levelname)s - %(message)s")
    args = parse_args(argv)
    device = torch.device(args.device)
    model, info = load_model(args.model_path, device, trust_pickle=args.trust_checkpoint)
    test_data, full_graph = load_test_data(args.data_dir)
    node_class = load_node_classes(args.node_types, int(full_graph["num_nodes"])) if args.node_types else None
    evaluator = ModelEvaluator(model, test_data, full_graph, device, batch_size=args.batch_size, node_class=node_class)
    metrics = evaluator.evaluate(num_neg_samples=args.num_neg_samples, k_values=args.k_values, filtered=args.filtered,
                                 type_constrained=args.type_constrained, both_sides=args.both_sides)
    if args.bootstrap:
        metrics["bootstrap"] = evaluator.bootstrap(args.bootstrap, args.bootstrap_seed, args.filtered, args.type_constrained,
                                                   args.both_sides, args.num_neg_samples, args.k_values)
    save_results(metrics, Path(args.output_dir), info)
    logger.info("Results saved to: %s", args.output_dir)
    return metrics


if __name__ == "__main__":
    main()
