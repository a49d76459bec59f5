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


def _refuse_attention(encoder, what: str) -> None:
    """these explanations differentiate the MEAN's weights; an attention encoder's weights are its own function of the
    input (``attention.py``) and are not explained"""
    if getattr(encoder, "attention", False):
        raise NotImplementedError(f"{what} explains the mean encoder: a model trained with attention (--attention) is "
                                  "not explained")


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
    _refuse_attention(enc, "edge_attribution")
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


# ----------------------------------------------------------------------------------------------------- learned masks
def receptive_field(edge_index: Tensor, head: int, tail: int, num_nodes: int) -> Tensor:
    """bool ``[E]``: the columns a two-layer score of ``(head, ., tail)`` can see - those whose destination is ``head`` or
    ``tail`` (both layers read them) and those whose destination is a source of one of these (the first layer's)"""
    src, dst = edge_index[0], edge_index[1]
    near = torch.zeros(int(num_nodes), dtype=torch.bool, device=edge_index.device)
    ends = (dst == head) | (dst == tail)
    near[src[ends]] = True
    near[head] = near[tail] = True
    return near[dst]


def _view_scores(model, view, x, edge_index, edge_type, weights, heads, relations, tails):
    """``(h1, h2, score)`` of the two layers over an edge-dropout VIEW, under autograd from the table on: a view stands
    for its parent wherever nothing is differentiated (``conv._resolve_graph``), so the table carries ``requires_grad``"""
    w1, root1, bias1, w2, root2, bias2 = weights
    r = model.encoder.num_relations
    h1 = rgcn_conv(x, edge_index, edge_type, w1, root1, bias1, r, "relu", graph=view)
    h2 = rgcn_conv(h1, edge_index, edge_type, w2, root2, bias2, r, None, graph=view)
    return h1, h2, model.decoder.score_triples(h2, heads, tails, relations)


def _check_explained(model, edge_index, graph, what):
    """the refusals ``edge_attribution`` has, for the callers below -> ``(x, graph)``"""
    if model.training:
        raise ValueError(f"{what} explains the model as it predicts: call model.eval() first")
    enc = model.encoder
    _refuse_attention(enc, what)
    if enc.conv1.gather_dtype == torch.float16 or enc.conv2.gather_dtype == torch.float16:
        raise NotImplementedError(f"{what} reads fp32 feature tables (gather_dtype=torch.float16 is not explained)")
    x = enc.node_embeddings.weight.detach().contiguous()
    if graph is not None:
        if not isinstance(graph, ops.BucketedGraph):
            raise TypeError("graph must be an ops.BucketedGraph")
        if graph.edge_dropout or graph.bipartite or graph.weighted_shard:
            raise NotImplementedError(f"{what} takes the bucketing of a whole graph: not a shard, not the view of an edge "
                                      "dropout (pass its parent)")
    if x.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the device: move the model and the graph there (there is no CPU path)")
    return x, graph


def learn_edge_mask(model, edge_index: Tensor, edge_type: Tensor, head: int, relation: int, tail: int, *,
                    graph: Optional["ops.BucketedGraph"] = None, steps: int = 100, lr: float = 0.1,
                    size_weight: float = 0.005, entropy_weight: float = 1.0, seed: int = 0,
                    dropout: Optional["ops.EdgeDropout"] = None) -> Dict[str, object]:
    """A soft mask ``m[e] in (0, 1)`` over the columns the score of ``(head, relation, tail)`` can see, OPTIMISED so that
    few edges preserve the prediction (GNNExplainer's objective on this model) -> ``{"mask": float32 [E] by original
    column, "field": bool [E], "score_full", "score_masked": float, "loss": [steps] floats, "grad": float32 [E]}`` (``grad``:
    the objective's gradient in ``theta`` at the last step, before that step's update, 0 outside the field).

    ``m = sigmoid(theta)`` enters both layers' means as ``w = m / sum over the segment of m`` (the module docstring's
    parametrisation; ``ops.EdgeDropout.set_mask`` writes it into a view).  ``theta`` lives on the pair's receptive field
    only (``receptive_field``); every other column cannot reach the score, keeps ``m = 1`` and has ``field = False``.
    Per step: the mask is drawn into the view, the two layers run over it under autograd as in ``edge_attribution``, and
    the gradient through the normalisation comes from ``ops.aggregate_weight_grad(through_normalisation=True)`` once per
    layer - ``d score / d theta = (layer1 + layer2) * (1 - m)``.  The objective is

        BCE(sigmoid(score(m)), [score_full >= 0])  +  size_weight * sum_field m  +  entropy_weight * mean_field H(m)

    (``H`` the binary entropy in nats; the regularisers' gradients ``size_weight * m (1 - m)`` and ``-entropy_weight /
    |field| * theta * m (1 - m)`` are added in closed form), minimised by Adam (beta = 0.9 / 0.999, eps = 1e-8) written
    in torch ops.  ``theta`` starts at ``1 + 0.1 * randn`` from a CPU generator under ``seed``.  Every kernel on the way
    sums in a fixed order, so the same arguments give the same bits.  The defaults are this project's own choices: the
    regularisers' weights are the ones GNNExplainer's reference code uses (0.005 on the sum, 1.0 on the mean entropy - the
    sum-weighted size term at 0.05 drove planted and distracting edges to zero together on the planted test graph), the
    step size 0.1 is ten times its 0.01 so that 100 steps suffice (theta moves by about lr per step under Adam).

    ``graph``: the bucketing of the columns if the caller holds it; ``dropout``: an ``ops.EdgeDropout`` over that graph to
    reuse (its view's weights are overwritten).  Refusals as ``edge_attribution``: ``eval()`` only, whole graph, fp32 table."""
    x, graph = _check_explained(model, edge_index, graph, "learn_edge_mask")
    enc = model.encoder
    conv1, conv2 = enc.conv1, enc.conv2
    dev, n, r = x.device, x.size(0), enc.num_relations
    e = edge_index.size(1)
    if graph is None:
        graph = ops.bucket(edge_index, edge_type, n, r)
    if graph.num_nodes != n or graph.num_relations != r or graph.num_edges != e:
        raise ValueError("graph is not the bucketing of these columns for this model")
    head, relation, tail = int(head), int(relation), int(tail)
    if not (0 <= head < n and 0 <= tail < n and 0 <= relation < model.decoder.num_relations):
        raise IndexError("head, tail or relation is out of range")
    if int(steps) < 0 or not float(lr) > 0.0:
        raise ValueError("steps must be >= 0 and lr > 0")
    own = dropout is None
    if own:
        dropout = ops.EdgeDropout(graph)
    elif not isinstance(dropout, ops.EdgeDropout) or dropout.graph is not graph:
        raise ValueError("dropout must be an ops.EdgeDropout over the same graph")
    try:
        heads, relations, tails = (torch.tensor([v], dtype=torch.int64, device=dev) for v in (head, relation, tail))
        with torch.no_grad():
            weights = tuple(None if p is None else p.detach().contiguous() for p in (
                conv1.effective_weight(), conv1.root, conv1.bias, conv2.effective_weight(), conv2.root, conv2.bias))
            w1, w2 = weights[0], weights[3]
            h1 = rgcn_conv(x, edge_index, edge_type, w1, weights[1], weights[2], r, "relu", graph=graph)
            h2 = rgcn_conv(h1, edge_index, edge_type, w2, weights[4], weights[5], r, None, graph=graph)
            score_full = model.decoder.score_triples(h2, heads, tails, relations)[0]
            target = (score_full >= 0).to(torch.float32)
            field = receptive_field(edge_index, head, tail, n)
            cols = torch.nonzero(field).view(-1)
            nf = cols.numel()
            theta = (1.0 + 0.1 * torch.randn(nf, generator=torch.Generator().manual_seed(int(seed)))).to(dev)
            mask = torch.ones(e, dtype=torch.float32, device=dev)
            exp_avg, exp_avg_sq = torch.zeros_like(theta), torch.zeros_like(theta)
        xg = x.clone().requires_grad_(True)
        losses, grad = [], torch.zeros_like(theta)

        def forward(m):
            mask[cols] = m
            dropout.set_mask(mask)
            with torch.enable_grad():
                return _view_scores(model, dropout.view, xg, edge_index, edge_type, weights, heads, relations, tails)

        for step in range(1, int(steps) + 1):
            m = torch.sigmoid(theta)
            h1, h2, score = forward(m)
            with torch.enable_grad():                          # (a caller may stand under no_grad)
                g2, g1 = torch.autograd.grad(score.sum(), (h2, h1))
            with torch.no_grad():
                h1 = h1.detach()
                g1 = g1 * (h1 > 0)
                view = dropout.view
                l1 = ops.aggregate_weight_grad(view, x, _aggregate_grad(g1.contiguous(), w1), through_normalisation=True,
                                               original_order=True)
                l2 = ops.aggregate_weight_grad(view, h1, _aggregate_grad(g2.contiguous(), w2), through_normalisation=True,
                                               original_order=True)
                s = score.detach()[0]
                dscore = (l1 + l2)[cols] * (1.0 - m)                            # d score / d theta
                bce = torch.nn.functional.binary_cross_entropy_with_logits(s, target)
                mc = m.clamp(1e-12, 1.0 - 1e-7)
                entropy = -(mc * mc.log() + (1.0 - mc) * (1.0 - mc).log())
                losses.append(bce + size_weight * m.sum() + entropy_weight * (entropy.mean() if nf else 0.0))
                slope = m * (1.0 - m)
                grad = (torch.sigmoid(s) - target) * dscore + size_weight * slope - (entropy_weight / max(nf, 1)) * theta * slope
                exp_avg.mul_(0.9).add_(grad, alpha=0.1)
                exp_avg_sq.mul_(0.999).addcmul_(grad, grad, value=0.001)
                denom = (exp_avg_sq / (1.0 - 0.999 ** step)).sqrt_().add_(1e-8)
                theta.addcdiv_(exp_avg / (1.0 - 0.9 ** step), denom, value=-float(lr))
        with torch.no_grad():
            m = torch.sigmoid(theta)
        score_masked = forward(m)[2].detach()[0]
        out_mask = torch.ones(e, dtype=torch.float32, device=dev)
        out_mask[cols] = m
        out_grad = torch.zeros(e, dtype=torch.float32, device=dev)
        out_grad[cols] = grad
        return {"mask": out_mask, "field": field, "score_full": float(score_full), "score_masked": float(score_masked),
                "grad": out_grad,
                "loss": [float(v) for v in torch.stack(losses).tolist()] if losses else []}
    finally:
        if own:
            dropout.destroy()
