"""Which edges a prediction used: the first-order effect of every edge of the graph on a triple's score.

``ModelEvaluator.explain`` ranks connecting paths by the cosine of consecutive embedding rows - the reference's
heuristic, which never asks the model anything.  Here the model answers: give every column p of the graph a mask
``m[p]`` (1 = present) that enters both layers' means as ``w[p] = m[p] / sum over p's (destination, relation) segment
of m``; then ``ds / dm[p]`` at ``m = 1``, for a scalar ``s = sum_q coeff[q] * score(h_q, r_q, t_q)``, is what deleting
the edge does to ``s`` to first order - the quantity saliency maps and GNNExplainer-style masks start from.  It is the
sum over the two layers of the gather's adjoint in its edge weights (``ops.aggregate_weight_grad`` with
``through_mean``), one dot product per edge and layer.  Nothing is learned and nothing is sampled.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor

from . import ops
from .conv import rgcn_conv


def _ids(t, device) -> Tensor:
    return torch.as_tensor(t, dtype=torch.int64).to(device).view(-1).contiguous()


def _aggregate_grad(g: Tensor, weight: Tensor) -> Tensor:
    """``gagg[i, r, :] = g[i] @ weight[r]^T`` -> ``[N, R * d_in]``: the gradient of a layer's aggregate given the gradient
    ``g`` of its pre-activation output (one dense product per relation)"""
    return torch.einsum("no,rio->nri", g, weight).reshape(g.size(0), -1).contiguous()


def edge_attribution(model, edge_index: Tensor, edge_type: Tensor, heads, relations, tails, coeff: Optional[Tensor] = None,
                     graph: Optional["ops.BucketedGraph"] = None) -> Dict[str, Tensor]:
    """``{"layer1", "layer2", "total": float32 [E], "score": float32 [Q]}`` for the triples ``(heads[q], relations[q],
    tails[q])``: ``total[p] = layer1[p] + layer2[p]`` is ``ds / dm[p]`` (module docstring) of ``s = sum_q coeff[q] *
    score[q]`` (``coeff``: ones) in the order of ``edge_index``'s columns; ``layerN`` the part that flows through the
    N-th layer's mean.  The model (a ``DrugDiseaseModel`` in ``eval()`` mode: no dropout) runs layer by layer under
    autograd - ``conv1`` with its ReLU, ``conv2``, ``decoder.score_triples`` - and one backward gives ``g2 = ds / dh2``
    and ``g1 = ds / dh1 * (h1 > 0)``.  ``graph``: the bucketing of the columns when the caller holds it.  Views of an
    edge dropout, shards and the fp16 feature table are not attributed (``NotImplementedError``)."""
    if model.training:
        raise ValueError("edge_attribution explains the model as it predicts: call model.eval() first")
    enc = model.encoder
    conv1, conv2 = enc.conv1, enc.conv2
    if conv1.gather_dtype == torch.float16 or conv2.gather_dtype == torch.float16:
        raise NotImplementedError("edge_attribution reads fp32 feature tables (gather_dtype=torch.float16 is not attributed)")
    x = enc.node_embeddings.weight.detach().contiguous()
    dev, n, r = x.device, x.size(0), enc.num_relations
    if graph is None:
        graph = ops.bucket(edge_index, edge_type, n, r)
    elif not isinstance(graph, ops.BucketedGraph):
        raise TypeError("graph must be an ops.BucketedGraph")
    elif graph.edge_dropout or graph.bipartite or graph.weighted_shard:
        raise NotImplementedError("edge_attribution takes the bucketing of a whole graph: not a shard, not the view of an "
                                  "edge dropout (pass its parent)")
    if graph.num_nodes != n or graph.num_relations != r or graph.num_edges != edge_index.size(1):
        raise ValueError("graph is not the bucketing of these columns for this model")
    heads, relations, tails = _ids(heads, dev), _ids(relations, dev), _ids(tails, dev)
    if not (heads.shape == relations.shape == tails.shape):
        raise ValueError("heads, relations and tails must be equally long")
    if heads.numel() and (int(torch.minimum(heads.min(), tails.min())) < 0 or int(torch.maximum(heads.max(), tails.max())) >= n
                          or int(relations.min()) < 0 or int(relations.max()) >= model.decoder.num_relations):
        raise IndexError("a head, tail or relation id is out of range")
    if coeff is not None:
        coeff = torch.as_tensor(coeff, dtype=torch.float32).to(dev).view(-1)
        if coeff.shape != heads.shape:
            raise ValueError("coeff must hold one float per triple")

    with torch.no_grad():
        w1, w2 = conv1.effective_weight().detach().contiguous(), conv2.effective_weight().detach().contiguous()
        root1, bias1, root2, bias2 = (None if p is None else p.detach() for p in (conv1.root, conv1.bias, conv2.root, conv2.bias))
        h1 = rgcn_conv(x, edge_index, edge_type, w1, root1, bias1, r, "relu", graph=graph)
    with torch.enable_grad():
        h1 = h1.detach().requires_grad_(True)
        h2 = rgcn_conv(h1, edge_index, edge_type, w2, root2, bias2, r, None, graph=graph)
        score = model.decoder.score_triples(h2, heads, tails, relations)
        s = score.sum() if coeff is None else (score * coeff).sum()
        g2, g1 = torch.autograd.grad(s, (h2, h1))
    with torch.no_grad():
        h1 = h1.detach()
        g1 = g1 * (h1 > 0)
        layer1 = ops.aggregate_weight_grad(graph, x, _aggregate_grad(g1, w1), through_mean=True, original_order=True)
        layer2 = ops.aggregate_weight_grad(graph, h1, _aggregate_grad(g2.contiguous(), w2), through_mean=True,
                                           original_order=True)
        return {"layer1": layer1, "layer2": layer2, "total": layer1 + layer2, "score": score.detach()}
