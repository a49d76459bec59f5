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
