"""Embedding consumers (SURVEY.md section 8f "next" row 4).

The reference's analysis scripts use the encoder output only through cosine similarity
mapped to [0, 1]:

* ``compare_methods.RGCNMethod.predict`` (``src/compare_methods.py:368-382``): per-pair
  ``(cos(drug, disease) + 1) / 2``;
* ``compare_methods.RGCNMethod.predict_all`` (``compare_methods.py:384-397``): the
  ``[n_drug, n_disease]`` matrix of the same;
* ``case_studies.predict_top_drugs`` (``src/case_studies.py:236-284``): the top-k drugs of one
  disease above a threshold, best first;
* ``medical_validation.generate_predictions`` + ``_filter_known_associations``
  (``src/medical_validation.py:191-280``): the best novel (drug, disease) pairs over many diseases.

Here they stay on the device: rows are normalised once, the per-pair form reuses the DistMult
kernel (relation factor = ones, so ``sum_d h*1*t`` of unit rows is the cosine), the matrix
form is a plain library GEMM, the ranking a stable descending sort (ties keep candidate
order, as the reference's ``list.sort(reverse=True)`` does).  The batched forms (``predict_top_drugs_batch``,
``novel_drug_predictions``) select on the device instead: the fused top-k pass over unit rows, the drugs as its allow
mask, the known associations as its exclude mask - no ``[diseases, drugs]`` matrix, no sort.

``connecting_paths`` answers the "why" the scripts ask next (``explain_predictions.find_paths`` / ``score_path`` /
``rank_paths``, ``case_studies.py:319-351``, ``analyze_failures.py:345-366``: ``networkx.all_simple_paths(cutoff=4)``
scored by the mean cosine of consecutive nodes times a length penalty): the k best of ALL simple paths between a
pair, enumerated on the device (``ops.paths_topk``).

``cluster_analysis`` is ``visualize_embeddings.cluster_analysis`` (``src/visualize_embeddings.py:651-777``): per node
type ``KMeans(n_clusters, n_init=10, random_state=42)`` and ``silhouette_score`` on that type's rows, the cluster sizes
and members - ``ops.kmeans`` and ``ops.silhouette_score``, the table never leaves the device.

``reduce_dimensions`` is ``visualize_embeddings.reduce_dimensions`` (``src/visualize_embeddings.py:176-236``): the
optional node sample and ``TSNE(n_components=2, perplexity=min(30, n - 1), max_iter=1000)`` - ``ops.tsne``, with exact
repulsion instead of scikit-learn's Barnes-Hut approximation.

``pair_subgraph_stats`` is ``analyze_failures.analyze_subgraph`` (``src/analyze_failures.py:368-437``) and
``medical_validation.find_common_neighbors`` (``src/medical_validation.py:356-394``): the radius-2 balls around a drug
and a disease over successors + predecessors, their intersection and the induced subgraph on their union -
``ops.pair_neighborhood``, one workgroup per pair.  ``failure_analysis`` is the analysis built on it
(``analyze_failures.py:273-489``): typing every labelled pair FP / FN / Correct and comparing the groups' structure,
over all sampled pairs instead of the ten networkx has time for.
"""
from __future__ import annotations

from typing import Dict, List, Mapping, Optional, Sequence, Tuple, Union

import logging

import numpy as np
import torch
from torch import Tensor

from . import ops

logger = logging.getLogger("primekg_rgcn_linkprediction_amd.consumers")

_Index = Union[Tensor, Sequence[int]]


def _index(idx: _Index, device) -> Tensor:
    t = idx if isinstance(idx, Tensor) else torch.as_tensor(list(idx), dtype=torch.int64)
    return t.to(device=device, dtype=torch.int64).contiguous()


def normalize_rows(embeddings: Tensor) -> Tensor:
    """``emb / ||emb||`` per row, as ``compare_methods.py:390-391`` (no epsilon: a zero row
    gives nan there too)."""
    if embeddings.dim() != 2:
        raise ValueError("embeddings must be [N, d]")
    return (embeddings / embeddings.norm(dim=1, keepdim=True)).contiguous()


@torch.no_grad()
def cosine_pair_scores(embeddings: Tensor, drug_indices: _Index, disease_indices: _Index,
                       normalized: bool = False) -> Tensor:
    """``(cos(emb[drug_b], emb[disease_b]) + 1) / 2`` for each pair b."""
    unit = embeddings if normalized else normalize_rows(embeddings)
    a, b = _index(drug_indices, unit.device), _index(disease_indices, unit.device)
    if a.shape != b.shape or a.dim() != 1:
        raise ValueError("drug_indices and disease_indices must be 1-D and equally long")
    ones = torch.ones(1, unit.size(1), device=unit.device, dtype=unit.dtype)
    zero = torch.zeros(a.numel(), dtype=torch.int64, device=unit.device)
    cos = ops.distmult_fwd(unit, a, unit, b, ones, zero, a.numel())
    return (cos + 1) / 2


@torch.no_grad()
def cosine_score_matrix(embeddings: Tensor, drug_indices: _Index, disease_indices: _Index,
                        normalized: bool = False) -> Tensor:
    """``[n_drug, n_disease]`` matrix of ``(cos + 1) / 2``."""
    unit = embeddings if normalized else normalize_rows(embeddings)
    a, b = _index(drug_indices, unit.device), _index(disease_indices, unit.device)
    return (unit.index_select(0, a) @ unit.index_select(0, b).t() + 1) / 2


@torch.no_grad()
def predict_top_drugs(embeddings: Tensor, disease_idx: int, drug_indices: _Index, top_k: int = 10,
                      threshold: float = 0.0, normalized: bool = False) -> List[Tuple[int, float]]:
    """[(drug_idx, score)] of the ``top_k`` drugs with score >= threshold for one disease,
    best first."""
    unit = embeddings if normalized else normalize_rows(embeddings)
    cand = _index(drug_indices, unit.device)
    scores = (torch.mv(unit.index_select(0, cand), unit[disease_idx]) + 1) / 2
    keep = scores >= threshold
    cand, scores = cand[keep], scores[keep]
    order = torch.sort(scores, descending=True, stable=True).indices[:top_k]
    return list(zip(cand[order].tolist(), scores[order].tolist()))


@torch.no_grad()
def predict_top_drugs_batch(embeddings: Tensor, disease_indices: _Index, drug_indices: _Index, top_k: int = 10,
                            known: Optional["ops.KnownTriples"] = None,
                            normalized: bool = False) -> Tuple[Tensor, Tensor]:
    """``predict_top_drugs`` for many diseases at once, on the device: ``(ids int64 [B, top_k], cosines [B, top_k])``,
    row b the ``top_k`` drugs closest to ``disease_indices[b]``, cosine descending, equal cosines by node id
    ascending (``predict_top_drugs`` keeps candidate order: the same for ascending ``drug_indices``), id -1 / -inf past
    the number of candidates.  Unit rows are both operands of the fused top-k pass (relation factor = ones, as in
    ``cosine_pair_scores``), the drugs its one allow row.  ``known``: a relation-free ``KnownTriples`` (edge type all
    zero, one relation) - a drug linked to the disease in either direction is left out."""
    unit = embeddings if normalized else normalize_rows(embeddings)
    dis, drugs = _index(disease_indices, unit.device), _index(drug_indices, unit.device)
    n = unit.size(0)
    class_of = torch.full((n,), -1, dtype=torch.int32, device=unit.device)
    class_of[drugs] = 0
    allow = ops.class_allow_bits(class_of, 1)
    query_class = torch.zeros(dis.numel(), dtype=torch.int32, device=unit.device)
    exclude = None
    if known is not None:
        if known.num_relations != 1 or known.num_nodes != n:
            raise ValueError("known must be relation-free (one relation, edge type all zero) over the same nodes")
        zero = torch.zeros_like(dis)
        exclude = known.exclude_bits("tail", dis, zero) | known.exclude_bits("head", dis, zero)
    return ops.distmult_topk_masked(unit.index_select(0, dis), unit, top_k, allow, query_class, exclude)


@torch.no_grad()
def novel_drug_predictions(embeddings: Tensor, disease_indices: _Index, drug_indices: _Index,
                           known: Optional["ops.KnownTriples"] = None, top_k: int = 100, threshold: float = 0.6,
                           normalized: bool = False) -> List[Tuple[int, int, float]]:
    """The device form of ``medical_validation.generate_predictions``: the best ``top_k`` ``(drug, disease, score)``
    triples over all given diseases with ``score = (cos + 1) / 2 >= threshold`` (the threshold meets the mapped
    score, as there) and no known drug-disease link, best first.  The global top-k of pairs lies inside the union of
    the per-disease top-k, so one ``predict_top_drugs_batch`` and a sort of ``B x top_k`` values give it."""
    ids, cos = predict_top_drugs_batch(embeddings, disease_indices, drug_indices, top_k, known, normalized)
    dis = _index(disease_indices, ids.device).view(-1, 1).expand_as(ids)
    scores = (cos + 1) / 2
    keep = (ids >= 0) & (scores >= threshold)
    ids, dis, scores = ids[keep], dis[keep], scores[keep]
    order = torch.sort(scores, descending=True, stable=True).indices[:top_k]
    return list(zip(ids[order].tolist(), dis[order].tolist(), scores[order].tolist()))


@torch.no_grad()
def connecting_paths(embeddings: Tensor, graph: "ops.PathGraph", pairs, k: int = 5, max_len: int = 4,
                     return_counts: bool = False, edge_score: Optional[Tensor] = None):
    """For every ``(source, target)`` of ``pairs`` the ``k`` best-scoring simple paths of at most ``max_len`` edges,
    best first: a list per pair of ``{"nodes": [...], "relations": [...], "length": L, "score": s}`` (the content of the
    reference's ``get_path_details``; ``relations[i]`` is the relation of hop i in ``graph``).  The score is the mean
    cosine of consecutive nodes times ``1 / (1 + 0.2 * (L - 1))`` (``ops.paths_topk`` over ``ops.edge_cosine``; pass
    ``edge_score`` to reuse or replace the per-edge scores).  ``return_counts``: also the exact number of simple paths of
    length 1..4 per pair, ``(paths, counts)``."""
    dev = embeddings.device
    p = torch.as_tensor(pairs, dtype=torch.int64).reshape(-1, 2).to(dev)
    graph = graph.to(dev)
    if edge_score is None:
        edge_score = ops.edge_cosine(embeddings.contiguous(), graph)
    nodes, length, score, count = ops.paths_topk(graph, edge_score, p[:, 0].contiguous(), p[:, 1].contiguous(), k, max_len)
    # the relation of every hop: its position among the (src, dst)-sorted unique pairs
    u, v = nodes[:, :, :-1].to(torch.int64), nodes[:, :, 1:].to(torch.int64)
    hop = (u >= 0) & (v >= 0)
    rel = torch.full(u.shape, -1, dtype=torch.int32, device=dev)
    if graph.nnz:
        keys = graph.out_src * graph.num_nodes + graph.out_dst.to(torch.int64)
        pos = torch.searchsorted(keys, (u * graph.num_nodes + v)[hop])
        rel[hop] = graph.out_rel[pos.clamp_(max=graph.nnz - 1)]
    nodes, rel, length, score = nodes.cpu().tolist(), rel.cpu().tolist(), length.cpu().tolist(), score.cpu().tolist()
    paths = [[{"nodes": nodes[q][j][:length[q][j] + 1], "relations": rel[q][j][:length[q][j]], "length": length[q][j],
               "score": score[q][j]} for j in range(len(length[q])) if length[q][j] > 0] for q in range(len(length))]
    return (paths, count.cpu().tolist()) if return_counts else paths


@torch.no_grad()
def attributed_edges(attr: Mapping[str, Tensor], edge_index: Tensor, edge_type: Tensor, k: int) -> List[Tuple]:
    """the ``k`` columns a score depends on most: ``[(column, src, rel, dst, value)]`` by ``|value|`` descending, ``value``
    the column's ``attr["total"]`` (``attribution.edge_attribution``); equal magnitudes in column order (a stable sort)"""
    total = attr["total"]
    if total.dim() != 1 or total.numel() != edge_index.size(1) or edge_type.numel() != total.numel():
        raise ValueError("attr['total'] must hold one value per column of edge_index / edge_type")
    order = torch.sort(total.abs(), descending=True, stable=True).indices[:max(int(k), 0)]
    cols = order.cpu()
    ei, et = edge_index.cpu(), edge_type.cpu()
    return list(zip(cols.tolist(), ei[0][cols].tolist(), et[cols].tolist(), ei[1][cols].tolist(), total[order].cpu().tolist()))


@torch.no_grad()
def attribution_edge_score(attr: Mapping[str, Tensor], path_graph: "ops.PathGraph", edge_index: Tensor) -> Tensor:
    """float32 ``[nnz]``, an ``edge_score`` for ``ops.paths_topk``: per unique ``(src, dst)`` pair of ``path_graph`` the
    LARGEST ``|attr["total"]|`` over the columns that name the pair (a maximum does not depend on the order the columns
    arrive in, so the result is deterministic; a sum by atomics would not be)"""
    total = attr["total"]
    graph = path_graph.to(total.device)
    entries = graph.column_entries(edge_index)
    if entries.numel() != total.numel():
        raise ValueError("attr['total'] must hold one value per column of edge_index")
    out = torch.zeros(graph.nnz, dtype=torch.float32, device=total.device)
    return out.scatter_reduce_(0, entries, total.abs().to(torch.float32), "amax", include_self=True)


def masked_edges(result: Mapping[str, Tensor], edge_index: Tensor, edge_type: Tensor, k: int) -> List[Tuple]:
    """the ``k`` columns a learned mask keeps most: ``[(column, src, rel, dst, value)]`` by mask value descending among
    the columns of the pair's receptive field (``attribution.learn_edge_mask``'s ``mask`` / ``field``; a column outside
    the field holds 1 because it cannot matter, and is never listed); equal values in column order (a stable sort)"""
    mask, field = result["mask"], result["field"]
    if mask.dim() != 1 or mask.numel() != edge_index.size(1) or edge_type.numel() != mask.numel() or field.shape != mask.shape:
        raise ValueError("result['mask'] / ['field'] must hold one value per column of edge_index / edge_type")
    cols = torch.nonzero(field).view(-1)
    order = cols[torch.sort(mask[cols], descending=True, stable=True).indices[:max(int(k), 0)]]
    at = order.cpu()
    ei, et = edge_index.cpu(), edge_type.cpu()
    return list(zip(at.tolist(), ei[0][at].tolist(), et[at].tolist(), ei[1][at].tolist(), mask[order].cpu().tolist()))


@torch.no_grad()
def mask_edge_score(result: Mapping[str, Tensor], path_graph: "ops.PathGraph", edge_index: Tensor) -> Tensor:
    """float32 ``[nnz]``, an ``edge_score`` for ``ops.paths_topk``: per unique ``(src, dst)`` pair of ``path_graph`` the
    LARGEST learned mask value over the field's columns that name the pair, 0 for a pair no such column names"""
    mask, field = result["mask"], result["field"]
    graph = path_graph.to(mask.device)
    entries = graph.column_entries(edge_index)
    if entries.numel() != mask.numel():
        raise ValueError("result['mask'] must hold one value per column of edge_index")
    out = torch.zeros(graph.nnz, dtype=torch.float32, device=mask.device)
    return out.scatter_reduce_(0, entries, torch.where(field, mask, torch.zeros_like(mask)), "amax", include_self=True)


def explanation_fidelity(model, edge_index: Tensor, edge_type: Tensor, pairs, relations, edge_sets, *,
                         dropout: Optional["ops.EdgeDropout"] = None) -> List[Dict[str, Dict[str, float]]]:
    """What the score does when the edges an explainer names are actually DELETED, and when only they are kept: for
    every ``(head, tail)`` of ``pairs`` with its relation and every named set of columns in ``edge_sets[q]`` (a mapping
    ``name -> columns``: the top-M of any explainer) -> ``{name: {"full", "without", "only"}}`` per pair -

        full     the score on the whole graph
        without  the score with the set hidden (fidelity-: a faithful set moves it)
        only     the score with every column of the pair's receptive field EXCEPT the set hidden (fidelity+: a
                 sufficient set preserves it)

    Deletion is exact, not a first-order estimate: the columns are hidden through ``position`` in a draw with ``p = 0``
    over one reused edge-dropout view (``ops.EdgeDropout.draw``: window = the hidden columns), which makes both layers
    the mean over the remaining in-edges - ``RGCNConv`` on ``edge_index[:, keep]``.  ``dropout``: an ``ops.EdgeDropout``
    over ``ops.bucket(edge_index, ...)`` to reuse (its view's weights are overwritten)."""
    from . import attribution
    x, _ = attribution._check_explained(model, edge_index, None, "explanation_fidelity")
    enc = model.encoder
    dev, n, r, e = x.device, x.size(0), enc.num_relations, edge_index.size(1)
    pairs = torch.as_tensor(pairs, dtype=torch.int64).reshape(-1, 2).tolist()
    relations = torch.as_tensor(relations, dtype=torch.int64).view(-1).tolist()
    if len(relations) == 1 and len(pairs) != 1:
        relations = relations * len(pairs)
    if len(relations) != len(pairs) or len(edge_sets) != len(pairs):
        raise ValueError("one relation and one mapping of edge sets per pair expected")
    own = dropout is None
    if own:
        dropout = ops.EdgeDropout(ops.bucket(edge_index, edge_type, n, r))
    elif not isinstance(dropout, ops.EdgeDropout) or dropout.graph.num_edges != e:
        raise ValueError("dropout must be an ops.EdgeDropout over the bucketing of these columns")
    try:
        conv1, conv2 = enc.conv1, enc.conv2
        weights = tuple(None if p is None else p.detach().contiguous() for p in (
            conv1.effective_weight(), conv1.root, conv1.bias, conv2.effective_weight(), conv2.root, conv2.bias))
        xg = x.clone().requires_grad_(True)                    # a view counts only where something is differentiated
        rng = torch.zeros(2, dtype=torch.int64, device=dev)
        everything = torch.arange(e, device=dev)

        def score(hidden: Tensor, h, rel, t) -> float:
            """the triple's score with the bool ``[E]`` columns ``hidden`` deleted"""
            order = torch.cat([everything[hidden], everything[~hidden]])       # the hidden columns stand first
            position = torch.empty(e, dtype=torch.int64, device=dev)
            position[order] = everything
            dropout.draw(0.0, rng, batch=int(hidden.sum()), position=position)
            ids = [torch.tensor([v], dtype=torch.int64, device=dev) for v in (h, rel, t)]
            with torch.enable_grad():
                s = attribution._view_scores(model, dropout.view, xg, edge_index, edge_type, weights, ids[0], ids[1], ids[2])[2]
            return float(s.detach()[0])

        out = []
        nothing = torch.zeros(e, dtype=torch.bool, device=dev)
        for (h, t), rel, sets in zip(pairs, relations, edge_sets):
            full = score(nothing, h, rel, t)
            field = attribution.receptive_field(edge_index, h, t, n)
            row = {}
            for name, columns in sets.items():
                named = torch.zeros(e, dtype=torch.bool, device=dev)
                columns = torch.as_tensor(columns, dtype=torch.int64, device=dev).view(-1)
                if columns.numel() and (int(columns.min()) < 0 or int(columns.max()) >= e):
                    raise IndexError(f"edge set {name!r} names a column outside [0, {e})")
                named[columns] = True
                row[name] = {"full": full, "without": score(named, h, rel, t), "only": score(field & ~named, h, rel, t)}
            out.append(row)
        return out
    finally:
        if own:
            dropout.destroy()


def _class_names(class_names, num_classes: int) -> List[str]:
    """name of every class id in ``[0, num_classes)``: from ``{name: class id}`` or a sequence indexed by class id; an
    id without a name is called by its number"""
    names = [str(c) for c in range(num_classes)]
    if class_names is None:
        return names
    named = class_names.items() if isinstance(class_names, Mapping) else [(n, c) for c, n in enumerate(class_names) if n is not None]
    for name, cls in named:
        if 0 <= int(cls) < num_classes:
            names[int(cls)] = str(name)
    return names


@torch.no_grad()
def pair_subgraph_stats(graph: "ops.PathGraph", pairs, radius: int = 2, node_class: Optional[Tensor] = None,
                        class_names=None, common_cap: int = 0) -> List[Dict]:
    """``analyze_failures.analyze_subgraph`` (``src/analyze_failures.py:368-437``) without its path search, for every
    ``(drug, disease)`` of ``pairs`` at once (``ops.pair_neighborhood``): a dict per pair with the reference's keys
    ``drug_neighborhood_size``, ``disease_neighborhood_size``, ``common_neighbors`` (nodes in both radius-``radius``
    balls), ``subgraph_nodes``, ``subgraph_edges`` (the induced subgraph on the balls' union) and ``node_type_counts``
    (``{type name: nodes of the union}``, types without a node left out as a ``Counter`` leaves them out, ``"unknown"``
    for a class outside ``[0, num_classes)``; empty without ``node_class``), plus ``degree`` (``{"drug", "disease"}``:
    distinct neighbours, the node itself not counted; None at radius 0), ``distance`` (undirected hops when at most
    ``radius``, else None) and ``common_nodes`` (the ``common_cap`` smallest ids of the intersection, what
    ``medical_validation.find_common_neighbors`` lists).  A node without any edge is not in the reference's graph: its
    ball is empty.  ``class_names``: ``{name: class id}`` or a sequence indexed by class id."""
    dev = graph.device
    p = torch.as_tensor(pairs, dtype=torch.int64).reshape(-1, 2).to(dev)
    num_classes, classes = 0, None
    if node_class is not None:
        classes = torch.as_tensor(node_class).to(device=dev, dtype=torch.int32).contiguous()
        num_classes = int(classes.max()) + 1 if classes.numel() else 0
        if num_classes > ops.NEIGHBORHOOD_MAX_CLASSES:
            raise ValueError(f"at most {ops.NEIGHBORHOOD_MAX_CLASSES} node classes are counted, got {num_classes}")
        if num_classes <= 0:
            classes = None
    nb = ops.pair_neighborhood(graph, p[:, 0].contiguous(), p[:, 1].contiguous(), radius, classes, max(num_classes, 0), common_cap)
    names = _class_names(class_names, max(num_classes, 0))
    ball, distance = nb.ball.cpu().tolist(), nb.distance.cpu().tolist()
    common, nodes, edges = nb.common.cpu().tolist(), nb.union_nodes.cpu().tolist(), nb.union_edges.cpu().tolist()
    per_class = None if nb.class_count is None else nb.class_count.cpu().tolist()
    listed = None if nb.common_nodes is None else nb.common_nodes.cpu().tolist()
    stats = []
    for q in range(p.size(0)):
        types = {}
        if per_class is not None:
            types = {names[c]: k for c, k in enumerate(per_class[q]) if k > 0}
            if nodes[q] > sum(per_class[q]):
                types["unknown"] = types.get("unknown", 0) + nodes[q] - sum(per_class[q])
        stats.append({
            "drug_neighborhood_size": ball[q][0][radius], "disease_neighborhood_size": ball[q][1][radius],
            "common_neighbors": common[q], "subgraph_nodes": nodes[q], "subgraph_edges": edges[q],
            "node_type_counts": types,
            "degree": None if radius < 1 else {"drug": max(ball[q][0][1] - 1, 0), "disease": max(ball[q][1][1] - 1, 0)},
            "distance": None if distance[q] < 0 else distance[q],
            "common_nodes": [] if listed is None else [i for i in listed[q] if i >= 0]})
    return stats


def classify_predictions(scores, labels) -> List[Dict]:
    """The typing of ``analyze_failures.identify_failures_and_successes`` (``src/analyze_failures.py:298-329``) for
    scores in [0, 1] and labels in {0, 1}, in the reference's own comparisons on Python floats: ``error = |score -
    label|``; ``confidence_error`` = the score of a negative scored ABOVE 0.7, one minus the score of a positive scored
    BELOW 0.3, else 0; ``type`` = FP for a negative above 0.5, FN for a positive at or below 0.5, else Correct."""
    scores = scores.tolist() if hasattr(scores, "tolist") else list(scores)
    labels = labels.tolist() if hasattr(labels, "tolist") else list(labels)
    if len(scores) != len(labels):
        raise ValueError("one label per score expected")
    rows = []
    for score, label in zip(scores, labels):
        score, label = float(score), int(label)
        if label == 0 and score > 0.7:
            confidence_error = score
        elif label == 1 and score < 0.3:
            confidence_error = 1 - score
        else:
            confidence_error = 0
        rows.append({"prediction": score, "ground_truth": label, "error": abs(score - label),
                     "confidence_error": confidence_error,
                     "type": "FP" if (label == 0 and score > 0.5) else ("FN" if (label == 1 and score <= 0.5) else "Correct")})
    return rows


def shortest_path_length(counts) -> Optional[int]:
    """from ``paths_topk``'s exact counts per length: the smallest L with a path of L edges, else None"""
    return next((length + 1 for length, c in enumerate(counts) if c > 0), None)


_MEAN_KEYS = ("drug_neighborhood_size", "disease_neighborhood_size", "common_neighbors", "subgraph_nodes", "subgraph_edges",
              "num_paths")
_DIFFERENCES = (("drug_neighborhood_diff", "drug_neighborhood_size"), ("disease_neighborhood_diff", "disease_neighborhood_size"),
                ("common_neighbors_diff", "common_neighbors"), ("path_count_diff", "num_paths"))


def summarize_failures(rows: List[Dict], num_failures: int = 5, num_successes: int = 5) -> Dict:
    """``rows``: one dict per pair with ``classify_predictions``' keys and the numeric keys of the stats.  -> the means
    per type, the reference's four ``differences`` (``compare_failure_with_success``: success minus failure - here
    between the MEANS of all Correct pairs and of all FP + FN pairs, None when a group is empty), and the reference's
    selection: rows by confidence error descending (a stable sort: ties keep their order), the first ``num_failures``
    FP / FN of them, and the ``num_successes`` Correct ones farthest from 0.5."""
    def means(group):
        return {"count": len(group), **{k: (sum(r[k] for r in group) / len(group) if group else None) for k in _MEAN_KEYS}}

    by_type = {t: [r for r in rows if r["type"] == t] for t in ("FP", "FN", "Correct")}
    failed, succeeded = means(by_type["FP"] + by_type["FN"]), means(by_type["Correct"])
    ranked = sorted(rows, key=lambda r: r["confidence_error"], reverse=True)
    failures = [r for r in ranked if r["type"] in ("FP", "FN")][:num_failures]
    correct = [r for r in ranked if r["type"] == "Correct"]
    successes = sorted(correct, key=lambda r: abs(r["prediction"] - 0.5), reverse=True)[:num_successes]
    return {"num_pairs": len(rows), "means": {**{t: means(g) for t, g in by_type.items()}, "failure": failed, "success": succeeded},
            "differences": {name: (succeeded[key] - failed[key] if failed["count"] and succeeded["count"] else None)
                            for name, key in _DIFFERENCES},
            "failures": failures, "successes": successes}


@torch.no_grad()
def failure_analysis(embeddings: Tensor, graph: "ops.PathGraph", pairs, labels, radius: int = 2, num_failures: int = 5,
                     num_successes: int = 5, node_class: Optional[Tensor] = None, class_names=None, common_cap: int = 0,
                     max_len: int = 4, edge_score: Optional[Tensor] = None) -> Dict:
    """The reference's failure analysis (``analyze_failures.py:273-489``) over EVERY labelled pair instead of five
    failures and five successes: every ``(drug, disease)`` of ``pairs`` is scored ``(cos + 1) / 2``
    (``cosine_pair_scores``) and typed (``classify_predictions``), gets its ``pair_subgraph_stats`` and, from
    ``ops.paths_topk``'s exact counts, ``path_counts`` (per length 1..4), ``num_paths`` (all simple paths of at most
    ``max_len`` edges; the reference stops counting at 20) and ``shortest_path_length``.  -> ``summarize_failures`` of
    those rows: per-type means, the four differences, the worst failures and best successes with their stats."""
    dev = embeddings.device
    p = torch.as_tensor(pairs, dtype=torch.int64).reshape(-1, 2).to(dev)
    graph = graph.to(dev)
    rows = classify_predictions(cosine_pair_scores(embeddings, p[:, 0], p[:, 1]).cpu(), torch.as_tensor(labels).reshape(-1))
    if len(rows) != p.size(0):
        raise ValueError("one label per pair expected")
    stats = pair_subgraph_stats(graph, p, radius, node_class, class_names, common_cap)
    if edge_score is None:
        edge_score = ops.edge_cosine(embeddings.contiguous(), graph)
    counts = ops.paths_topk(graph, edge_score, p[:, 0].contiguous(), p[:, 1].contiguous(), 1, max_len)[3].cpu().tolist()
    for row, (drug, disease), stat, count in zip(rows, p.cpu().tolist(), stats, counts):
        row.update(drug_idx=drug, disease_idx=disease, **stat, path_counts=count, num_paths=sum(count),
                   shortest_path_length=shortest_path_length(count))
    result = summarize_failures(rows, num_failures, num_successes)
    result["radius"], result["max_path_length"] = radius, max_len
    return result


@torch.no_grad()
def cluster_analysis(embeddings: Tensor, node_class: Tensor, class_names: Union[Mapping[str, int], Sequence[Optional[str]]],
                     n_clusters: int = 10, **kmeans_kw) -> Dict[str, Dict]:
    """K-means and silhouette of every named node type's embedding rows, on the device.  ``node_class`` int ``[N]`` is
    the class of every node, ``class_names`` says which classes to analyse and what to call them: ``{name: class id}``,
    or a sequence of names indexed by class id (``None``: skip).  Per name ``{"labels": int64 [n_type] (the cluster of
    the type's nodes, node id ascending), "silhouette": float, "cluster_sizes": int64 [n_clusters], "members": a list
    per cluster of its node ids, ascending}`` - the reference's ``results`` dict plus what its
    ``*_cluster_examples.txt`` lists.  The silhouette is 0.0 when fewer than two clusters are populated, as there.
    A type with fewer nodes than ``n_clusters`` is left out of the result with a logged warning.
    ``kmeans_kw`` goes to ``ops.kmeans`` (``n_init``, ``seed``, ``max_iter``, ``tol``, ``init``, ``poll_every``)."""
    if embeddings.dim() != 2:
        raise ValueError("embeddings must be [N, d]")
    classes = torch.as_tensor(node_class).to(embeddings.device)
    if classes.shape != (embeddings.size(0),):
        raise ValueError(f"node_class must be [{embeddings.size(0)}]")
    named = class_names.items() if isinstance(class_names, Mapping) else [(n, c) for c, n in enumerate(class_names) if n is not None]
    results = {}
    for name, cls in named:
        nodes = torch.nonzero(classes == int(cls)).view(-1)                    # ascending
        if nodes.numel() < max(2, n_clusters):                                # one small type must not end the others' analysis
            logger.warning("node type %r (class %s) has %d nodes: %d clusters need at least as many - left out",
                           name, cls, nodes.numel(), n_clusters)
            continue
        rows = embeddings.index_select(0, nodes).to(torch.float32).contiguous()
        fit = ops.kmeans(rows, n_clusters, **kmeans_kw)
        populated = int((fit.sizes > 0).sum())
        silhouette = ops.silhouette_score(rows, fit.labels, n_clusters) if populated > 1 else 0.0
        order = torch.argsort(fit.labels, stable=True)                         # by cluster, node ids stay ascending
        members = [m.tolist() for m in torch.split(nodes[order].cpu(), fit.sizes.cpu().tolist())]
        results[name] = {"labels": fit.labels.cpu(), "silhouette": float(silhouette), "cluster_sizes": fit.sizes.cpu(),
                         "members": members}
    return results


def sample_indices(n: int, sample_size: Optional[int] = None, random_state: int = 42) -> np.ndarray:
    """the reference's node sample: ``np.random.seed(random_state); np.random.choice(n, sample_size, replace=False)`` when
    ``sample_size`` is given and below ``n``, else every node in order (a private ``RandomState``: the same draw, the
    global generator left alone)"""
    if sample_size and sample_size < n:
        return np.random.RandomState(random_state).choice(n, size=int(sample_size), replace=False)
    return np.arange(n)


@torch.no_grad()
def reduce_dimensions(embeddings: Tensor, method: str = "tsne", sample_size: Optional[int] = None, random_state: int = 42,
                      return_result: bool = False, **tsne_kw):
    """The 2-D projection of (a sample of) the embedding rows, on the device: ``(xy float32 [n, 2], sample_indices int64
    [n])`` - the reference's ``embeddings_2d`` and ``sample_indices``.  ``method="tsne"``: ``ops.tsne`` at perplexity
    ``min(30, n - 1)`` with ``seed=random_state``; ``tsne_kw`` goes to ``ops.tsne`` (``perplexity``, ``max_iter``, ``init``,
    ``slices``, ...).  The default needs at least 32 rows: ``ops.tsne`` searches among ``k = min(n - 1, int(3 perplexity + 1))``
    neighbours and requires ``perplexity < k``, so for ``n <= 31`` pass a ``perplexity`` below ``n - 1`` (scikit-learn, which only
    asks for ``perplexity < n``, accepts ``n - 1`` there).  ``return_result``: ``(xy, sample_indices, ops.TSNEResult)``.  ``method="umap"`` is not built (the reference itself falls back to t-SNE when ``umap`` is missing)."""
    if not isinstance(method, str) or method.lower() not in ("tsne", "umap"):
        raise ValueError(f"Unknown method: {method}. Use 'tsne' or 'umap'")
    if method.lower() == "umap":
        raise NotImplementedError("method='umap' is not built: only method='tsne' runs on the device")
    if embeddings.dim() != 2:
        raise ValueError("embeddings must be [N, d]")
    idx = sample_indices(embeddings.size(0), sample_size, random_state)
    rows = embeddings.index_select(0, torch.as_tensor(idx, dtype=torch.int64, device=embeddings.device))
    rows = rows.to(torch.float32).contiguous()
    kw = {"perplexity": float(min(30, rows.size(0) - 1)), "seed": random_state}
    kw.update(tsne_kw)
    result = ops.tsne(rows, **kw)
    return (result.y, idx, result) if return_result else (result.y, idx)
