"""Relational attention: an R-GCN layer whose per-(destination, relation) mean is a learned segment softmax.

Within-relation attention on the layer's INPUT (Busbridge et al. 2019, "Relational graph attention networks"; the family
PyG's ``RGATConv`` covers), in the engine's gather-then-transform order: with per-relation vectors ``att_dst[r]`` and
``att_src[r]`` in R^{d_in}, negative slope ``lam`` and an edge ``e = (j -> i, r)``,

    a_dst[i, r] = <x_i, att_dst[r]>      a_src[j, r] = <x_j, att_src[r]>      (one [N, d_in] x [d_in, 2R] product)
    l(e) = leaky_relu(a_dst[i, r] + a_src[j, r], lam)
    alpha(e) = exp(l(e)) / sum over the non-hidden edges e' of segment (i, r) of exp(l(e'))     (0 for a hidden edge)
    x'_i = root x_i + sum_r W_r sum_{e in (i, r)} alpha(e) x_j + b

The weights are written into the layer's own ``ops.EdgeDropout`` view by ``set_attention`` (one device pass: logit,
segment maximum, exp, fixed-order sum, division), the weighted gather and the transforms then run over that view
unchanged - the very calls ``RGCNConv`` makes over a view - and the backward adds what the softmax needs:
``ops.aggregate_weight_grad(through_normalisation=True)`` is dL/dl per edge, ``ops.edge_segment_sum`` its deterministic
adjoint back to the per-node scalars.  ``att_* = 0`` (the initial value, on purpose) gives ``alpha = 1 / |segment|``:
a fresh layer IS ``RGCNConv``, and the gradient in ``att_*`` is not zero there.

Out of scope: several heads, attention across relations, random edge dropout beside attention (the slot of ``p``
carries the slope), recorded / captured passes, the fp16 feature table, ``dist.py``.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import ops
from .attribution import _aggregate_grad
from .conv import RGCNConv, _check_x, _contiguous, _conv_backward, _conv_forward

_WINDOW_KEYS = ("position", "cursor", "batch", "stats", "hide_twins")


def attention_scalars(x: Tensor, att_dst: Tensor, att_src: Tensor) -> Tensor:
    """``[2, N, R]``: ``a[0, i, r] = <x_i, att_dst[r]>``, ``a[1, j, r] = <x_j, att_src[r]>`` - what ``set_attention`` reads"""
    a = x @ torch.cat([att_dst, att_src], 0).t()                      # [N, 2R]
    return a.view(x.size(0), 2, att_dst.size(0)).transpose(0, 1).contiguous()


class _Views:
    """the ``ops.EdgeDropout`` of one (layer, graph) and what the last draw into it was"""

    def __init__(self, graph: "ops.BucketedGraph"):
        self.dropout = ops.EdgeDropout(graph)
        self.version = 0

    def draw(self, a: Tensor, slope: float, window: dict) -> int:
        self.dropout.set_attention(a, slope, **window)
        self.version += 1
        return self.version

    def destroy(self) -> None:
        self.dropout.destroy()


class _AttentionConvFunction(torch.autograd.Function):
    """x, weight[R, d_in, d_out], root, bias, att_dst[R, d_in], att_src[R, d_in] -> out on ``views``' graph.  The
    forward and the backward in x / weight / root / bias are ``RGCNConv``'s own passes over the view; the backward adds
    the softmax's part to ``gx`` and forms the gradients of the attention vectors."""

    @staticmethod
    def forward(ctx, x, weight, root, bias, att_dst, att_src, views: _Views, edge_index, edge_type, slope: float,
                relu: bool, window: dict):
        x, weight, root, bias, att_dst, att_src = _contiguous(x, weight, root, bias, att_dst, att_src)
        a = attention_scalars(x, att_dst, att_src)
        ctx.version = views.draw(a, slope, window)
        view = views.dropout.view
        out, agg, x_amax, pkbuf = _conv_forward(x, weight, root, bias, graph=view, relu=relu, gather_dtype=None, half=False)
        ctx.views, ctx.relu, ctx.slope, ctx.window = views, relu, slope, window
        ctx.edges = (edge_index, edge_type)
        ctx.has_root, ctx.has_bias = root is not None, bias is not None
        ctx.save_for_backward(x, weight, root, att_dst, att_src, a, out if relu else None)
        ctx.kept = (agg, x_amax, pkbuf)
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, root, att_dst, att_src, a, out = ctx.saved_tensors
        agg, x_amax, pkbuf = ctx.kept
        views = ctx.views
        if views.version != ctx.version:           # another forward drew into the view since: the same draw again, same bits
            ctx.version = views.draw(a, ctx.slope, {**ctx.window, "stats": None})
        view, graph = views.dropout.view, views.dropout.graph
        if ctx.relu:
            g = g * (out > 0)
        g = g.contiguous()
        need_x, need_w, need_root, need_bias, need_dst, need_src = ctx.needs_input_grad[:6]
        need_p = bool(need_w or (need_root and ctx.has_root) or (need_bias and ctx.has_bias))
        need_att = bool(need_x or need_dst or need_src)
        gx, gw, groot, gbias = _conv_backward(x, agg, weight, root, x_amax, pkbuf, g, graph=view, has_root=ctx.has_root,
                                              has_bias=ctx.has_bias, need_x=bool(need_x), need_p=need_p, prec=None)
        g_dst = g_src = None
        if need_att:
            edge_index, edge_type = ctx.edges
            dlog = ops.aggregate_weight_grad(view, x, _aggregate_grad(g, weight), through_normalisation=True,
                                             original_order=True)     # dL/dl(e); 0 for a hidden edge
            z = a[0][edge_index[1], edge_type] + a[1][edge_index[0], edge_type]
            de = torch.where(z >= 0, dlog, dlog * ctx.slope).contiguous()
            da_dst = ops.edge_segment_sum(graph, de)                  # [N, R]: deterministic, no float atomics
            da_src = ops.edge_segment_sum(graph, de, transposed=True)
            if need_dst:
                g_dst = da_dst.t() @ x
            if need_src:
                g_src = da_src.t() @ x
            if need_x:
                gx = gx + (da_dst @ att_dst + da_src @ att_src)
        return gx, gw, groot, gbias, g_dst, g_src, None, None, None, None, None, None


class RelationalAttentionConv(RGCNConv):
    r"""``RGCNConv`` with a learned weighting of every (destination, relation) segment:

    .. math:: x'_i = \Theta_{root} x_i + \sum_r \Theta_r \sum_{j \in N_r(i)} \alpha_{ij}^r x_j + b,\qquad
              \alpha^r_{i\cdot} = \mathrm{softmax}_j\, \mathrm{LeakyReLU}(\langle x_i, a^{dst}_r\rangle + \langle x_j, a^{src}_r\rangle)

    ``att_dst`` / ``att_src`` ``[R, d_in]`` start at ZERO, where the layer is the mean layer.  ``num_bases`` works as in
    the parent.  Unlike ``RGCNConv`` the layer ALWAYS runs over its view - in ``eval()`` and under ``no_grad`` too: the
    view is the model.  ``forward(..., window=dict(position=, cursor=, batch=, stats=, hide_twins=))`` hides the batch's
    own columns from the softmax (``ops.EdgeDropout.set_attention``)."""

    def __init__(self, in_channels, out_channels: int, num_relations: int, num_bases: Optional[int] = None,
                 negative_slope: float = 0.2, **kwargs):
        if kwargs.get("gather_dtype") == torch.float16:
            raise NotImplementedError("the attention layer reads an fp32 feature table (gather_dtype=torch.float16 is not "
                                      "implemented)")
        if not 0.0 <= float(negative_slope) <= 1.0:
            raise ValueError(f"negative_slope must be in [0, 1], got {negative_slope}")
        super().__init__(in_channels, out_channels, num_relations, num_bases=num_bases, **kwargs)
        self.negative_slope = float(negative_slope)
        self.att_dst = nn.Parameter(torch.zeros(num_relations, self.in_channels_l))
        self.att_src = nn.Parameter(torch.zeros(num_relations, self.in_channels_l))
        self._views_key = object()                 # this layer's slot among a graph's attention views

    def reset_parameters(self) -> None:
        super().reset_parameters()
        for name in ("att_dst", "att_src"):
            if hasattr(self, name):
                with torch.no_grad():
                    getattr(self, name).zero_()

    def views_of(self, graph: "ops.BucketedGraph") -> _Views:
        """this layer's view of ``graph``: built once, cached on the graph and destroyed with it"""
        cache = graph.__dict__.setdefault("_attention_views", {})
        views = cache.get(self._views_key)
        if views is None:
            views = cache[self._views_key] = _Views(graph)
        return views

    def forward(self, x: Tensor, edge_index: Tensor, edge_type: Optional[Tensor] = None,
                activation: Optional[str] = None, graph: Optional["ops.BucketedGraph"] = None,
                window: Optional[dict] = None) -> Tensor:
        if not isinstance(x, Tensor) or not isinstance(edge_index, Tensor):
            raise NotImplementedError("x must be a float tensor [N, in_channels] and edge_index a tensor [2, E]")
        assert edge_type is not None, "edge_type is required"
        _check_x(x)
        if x.dim() != 2 or x.size(1) != self.in_channels_l:
            raise ValueError(f"x must be [N, {self.in_channels_l}], got {tuple(x.shape)}")
        if activation not in (None, "relu"):
            raise ValueError(f"activation must be None or 'relu', got {activation!r}")
        if graph is None:
            graph = ops.bucket(edge_index, edge_type, x.size(0), self.num_relations)
        elif not isinstance(graph, ops.BucketedGraph) or graph.bipartite or graph.edge_dropout or graph.weighted_shard:
            raise ValueError("graph= takes the bucketing of the whole graph (the layer draws into a view of its own)")
        if graph.num_nodes != x.size(0) or graph.num_relations != self.num_relations or graph.num_edges != edge_index.size(1):
            raise ValueError("graph is not the bucketing of these columns for this layer")
        window = dict(window or {})
        if set(window) - set(_WINDOW_KEYS):
            raise TypeError(f"window takes {_WINDOW_KEYS}, got {sorted(window)}")
        return _AttentionConvFunction.apply(x, self.effective_weight(), self.root, self.bias, self.att_dst, self.att_src,
                                            self.views_of(graph), edge_index, edge_type, self.negative_slope,
                                            activation == "relu", window)
