"""``RGCNConv``: drop-in for ``torch_geometric.nn.RGCNConv`` as the reference uses it
(imported at ``src/models/rgcn.py:17``, built at ``rgcn.py:72-85`` with
``in_channels, out_channels, num_relations, num_bases``; called at ``rgcn.py:123,128``
as ``conv(x, edge_index, edge_type)``).

Same constructor signature, same registered parameter names/shapes (``weight``,
``comp``, ``root``, ``bias`` -> state-dict keys ``encoder.conv1.weight`` ... so the
reference's checkpoints load, ``src/evaluate.py:686-708``), same init
(glorot / zeros).  The arithmetic runs in ``librgcn_hip.so``:

    forward : bucket (cached, once per graph) -> gather+mean -> one fp32-MFMA GEMM
    backward: params GEMM (split over node ranges) ; transposed gather -> input GEMM

There is no CPU path and no PyG / torch_scatter fallback.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple, Union

import torch
import torch.nn as nn
from torch import Tensor

from . import ops


def _glorot(t: Optional[Tensor]) -> None:
    # PyG nn.inits.glorot: U(-a, a), a = sqrt(6 / (size(-2) + size(-1)))
    # written to the parameter itself, not through ``.data``: the write must move ``_version`` (``ops.amax_hint``)
    if t is not None:
        bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
        with torch.no_grad():
            t.uniform_(-bound, bound)


def _table(x: Tensor, gather_dtype) -> Tensor:
    """the FEATURE table the forward gather reads: x itself, or its fp16 copy (configs[4]:
    "fp16 features + fp32 accumulate").  Gradient tables stay fp32: they span many orders of
    magnitude and would need loss scaling to survive fp16."""
    if gather_dtype in (None, torch.float32):
        return x
    ops.guard_torch_op("fp16 copy of the feature table")
    return x.to(gather_dtype)


class _BasisCompose(torch.autograd.Function):
    """``W[r] = sum_b comp[r, b] * basis[b]`` (PyG: ``(comp @ weight.view(B, -1)).view(R, in, out)``; SURVEY row A5,
    BASELINE configs[2]).  One elementwise launch forward; the backward is ``grad_basis = comp^T gW`` and the R * B dot
    products ``grad_comp = gW basis^T`` of length in * out as two launches with a fixed summation order
    (``csrc/rgcn_basis.hip``) - through round 2 torch ops: per step of configs[2] four small library GEMMs, two
    broadcast multiplies and two row sums."""

    @staticmethod
    def forward(ctx, comp: Tensor, basis: Tensor) -> Tensor:
        comp, basis = comp.contiguous(), basis.contiguous()
        ctx.save_for_backward(comp, basis)
        return ops.basis_compose(comp, basis)

    @staticmethod
    def backward(ctx, gw: Tensor):
        comp, basis = ctx.saved_tensors
        return ops.basis_compose_bwd(gw.contiguous(), comp, basis, ctx.needs_input_grad[0], ctx.needs_input_grad[1])


class _Scales:
    """The operand scales of one pass of the split-precision transforms (``ops.GEMM_PRECISION``): one
    device allocation of amax buffers (``ops.amax_buffer`` layout).  Buffer 0 receives ``max |t|`` of the
    pass's external tensor ``t`` (the embedding table / the incoming gradient) and the SAME launch clears
    the others, which the pass's kernels then publish their results' maxima into, handed out slot by
    slot - and, in a forward pass, splits the layers' weights.  In fp32 mode nothing is allocated and every
    slot is None."""

    def __init__(self, t: Tensor, slots: int = 2, layers=(), given=None):
        """``layers``: ``[(weight, root | None), ...]`` of the pass (forward passes): their split images are made
        by the SAME first launch - ``self.packed[i]`` (None for widths the split kernels do not tile).
        ``given`` = ``(amax of t, [(amax of weight, amax of root | None), ...])``: every maximum is already known
        (``ops.amax_hint``: the optimizer left them) - the first launch then scans nothing, it splits the weights
        under the given maxima and clears the pass's own slots."""
        self._own, self._next, self.first = None, 0, None
        self.packed = [None] * len(layers)
        if ops.GEMM_PRECISION == "split":
            if given is not None:
                self.first = given[0]
                if slots > 1:
                    self._own = ops._empty(slots - 1, ops.AMAX_FLOATS, dtype=torch.float32, device=t.device)
                self.packed = ops.split_weights_many(list(layers), amax=list(given[1]), clear=self._own)
                return
            buf = ops._empty(slots, ops.AMAX_FLOATS, dtype=torch.float32, device=t.device)
            self.first, self._own = buf[0], buf[1:slots]
            if layers:
                self.packed = ops.absmax_and_split(t, self.first, self._own, list(layers))
            else:
                ops.absmax(t, self.first, self._own)

    def slot(self) -> Optional[Tensor]:
        if self._own is None:
            return None
        self._next += 1
        return self._own[self._next - 1]


import os as _os
_TRANSFORM_FIRST_RATIO = 2.0             # see _input_grad (module attributes, not environment switches: tests patch them)


def _fused_backward(graph, g, r, d_in, d_out, g_amax, packed, precision) -> bool:
    """the one-kernel input gradient (ops.layer_bwd_input_fused) under the policy of _layer_train_forward: where
    the transposed aggregate [N, R * d_out] would no longer fit the Infinity Cache (or RGCN_TRAIN_FUSED=1)"""
    fused = _TRAIN_FUSED == "1" or (_TRAIN_FUSED == "auto" and g.size(0) * r * d_out * 4 >= _TRAIN_FUSED_MIN_BYTES)
    return (fused and precision is None and packed is not None and g_amax is not None and not graph.bipartite
            and not graph.edge_dropout                     # (its walked CSR would be a stale copy of the weights)
            and ops.GEMM_PRECISION == "split" and ops.fused_bwd_supported(r, d_in, d_out))


def _from_packed(weight: Tensor, packed, precision) -> bool:
    """is the layer's transform-first product formed from the step's split images (``ops.transform_first``)?"""
    return packed is not None and ops.GEMM_PRECISION == "split" and precision is None and weight.size(2) % 32 == 0


def _transform_first(graph: "ops.BucketedGraph", weight: Tensor, root: Optional[Tensor], packed, precision) -> bool:
    """does the layer's input gradient take the transform-first order (see _input_grad)?"""
    r, d_in, d_out = weight.shape
    ratio = _TRANSFORM_FIRST_RATIO if _from_packed(weight, packed, precision) else max(_TRANSFORM_FIRST_RATIO, 4.0)
    # (an edge-dropout view: the merged structure would be a copy of weights that the next draw rewrites)
    return d_out >= ratio * d_in and root is not None and not graph.bipartite and not graph.edge_dropout


# Sparse aggregates: about half of the (node, relation) segments of a typed knowledge graph have no edge (46,756 of C2's
# 92,778, on the source side too), and an aggregate that stays inside a training pass - agg1, agg2, the transposed
# aggregate of conv2's input gradient - needs neither their zero rows stored by the gather nor read back by the
# transforms (ops.aggregate_sparse; the NT / chained NT / TN kernels redirect those lanes to one row of zeros: same
# bits).  Where the split kernels consume the aggregate and its scale is known beforehand; everything else - fp32 and
# one-pass fp16 transforms, the fp16 table, shards, the fused layers, the eval path - keeps every row written.
# profiles/sparse_aggregate.txt.  A module attribute (tests patch it); part of _policy_key().
_SPARSE_AGG = True

# Row tiles of the split NT transforms in occupancy order (include/rgcn_row_order.h; ops._order_bit has the conditions):
# same bytes, a quarter fewer live k-tiles at C2 - profiles/nt_row_order.txt.  RGCN_NT_ROW_ORDER=0 gives the launches in
# node order, for A/B.  A module attribute (tests patch it); part of _policy_key().
_NT_ROW_ORDER = _os.environ.get("RGCN_NT_ROW_ORDER", "1") != "0"


def _sparse_agg(graph: "ops.BucketedGraph", transposed: bool, half: bool, packed, amax, d: int, precision=None) -> bool:
    """is the d-wide aggregate of this layer a sparse one (see above)?  The consumers' own conditions: split precision
    with the step's split images, the operand's maximum in a buffer (a sparse operand cannot be scanned), rows the
    parameter-gradient kernel tiles (d % 64), a square graph of at most 32 relations."""
    return bool(_SPARSE_AGG and not half and packed is not None and amax is not None and ops.GEMM_PRECISION == "split"
                and precision in (None, "half") and d % 64 == 0 and d <= 256 and not graph.bipartite
                and not graph.weighted_shard and graph.num_relations <= 32
                and graph.row_mask_ptr(transposed) is not None)


def _gagg_scale(graph: "ops.BucketedGraph", gagg_amax: Optional[Tensor], g_amax: Optional[Tensor]):
    """``(amax, amax_mul)`` of the transform reading a transposed aggregate of ``g``: its OWN maximum, which its gather
    publishes - the bound weight_bound * max |g| is hundreds of times looser on hub graphs and would cost its ordinary
    rows that many binades of the lo half (tests/test_split_rows.py); the bound only without it (fp32: no slots).  An
    edge-dropout view's transposed bound is the longest (source, relation) segment's edge count (every weight <= 1: 61,716
    at C2; the parent's is that segment's sum of 1 / cnt) - looser still, and reached on the fp32 route alone, whose
    kernels scale nothing by it"""
    if gagg_amax is not None:
        return (gagg_amax, g_amax), 1.0
    return (g_amax, g_amax), graph.weight_bound(True)


def _input_grad(graph: "ops.BucketedGraph", g: Tensor, weight: Tensor, root: Optional[Tensor],
                tail: Optional["ops.PendingParamGrads"] = None, g_amax: Optional[Tensor] = None,
                scales: Optional[_Scales] = None, packed: Optional["ops.SplitWeights"] = None,
                precision: Optional[str] = None, t_first: Optional[Tensor] = None, *,
                relu_mask: Optional[Tensor] = None, out_scale: float = 1.0, amax_out: Optional[Tensor] = None,
                lower=None):
    """``d loss / d x`` of one layer (``weight``, ``root``, split images ``packed``) from ``g = d loss / d out``.
    ``tail``: the pending slab reduction of the layer's parameter gradients (it rides in the gather launch); epilogue
    extras (conv2 of the encoder): ``relu_mask``, ``out_scale`` (a dropout's 1 / (1 - p)), ``amax_out``; ``lower``: the
    layer below ``(weight, root, split images)``, whose transform-first product ``T`` this layer's last launch may form:
    the result is then ``(d loss / d x, T | None)``; ``t_first``: that product, when this is the layer below.  In order:

    1. transform first (no extras; d_out >= 2 d_in: conv1 at 64 -> 128 and at hidden 256, BASELINE configs[1..2]) -
       ``T = g @ [W_r^T ... | root^T]`` is ``[N, (R+1) d_in]`` and the gather over the merged structure reads d_in-wide
       rows (half / a quarter of the bytes per edge), adds the root block as one more weighted row and writes ``grad_x``
       directly.  Same flops.  Measured: the step at 64 -> 256 -> 256 goes from 0.911 to 0.856 ms (round 1); at
       64 -> 128 the short-K GEMM that writes ``T`` cost what the narrower gather saved while it ran at the fp32 MFMA
       rate and split its own copy of the weights - in split precision, from the step's split weights
       (``ops.transform_first``: their natural-order image, no concatenation, no second split) the C2 step goes from
       0.298 to 0.287 ms.  The fp32 and one-pass fp16 modes keep the threshold 4;
    2. the one-kernel input gradient (``_fused_backward``);
    3. gather first - ``gagg``, then one GEMM with K = (R+1) d_out (the randomly read rows are d_out wide), which also
       forms the ``T`` of ``lower`` from its own tiles where that layer goes transform first
       (``ops.transform_bwd_input_chain``: one launch less, no re-read of the result).

    The transposed aggregate is scaled by its own maximum (``_gagg_scale``), which its gather - or the fused kernel's
    first pass - publishes into a slot of ``scales``.  No hub deferral: the maximum must be final."""
    r, d_in, d_out = weight.shape
    extras = relu_mask is not None or amax_out is not None or out_scale != 1.0
    merged = (graph.merged_transposed()
              if not extras and _transform_first(graph, weight, root, packed, precision) else None)
    t = None                                     # the lower layer's T, when this launch forms it
    if merged is not None:
        if t_first is None and _from_packed(weight, packed, precision):
            t_first = ops.transform_first(g.contiguous(), packed, g_amax)
        elif t_first is None:
            ops.guard_torch_op("weight concatenation of the transform-first input gradient")
            wcat = torch.cat([weight.reshape(r * d_in, d_out), root]).view(1, (r + 1) * d_in, d_out)
            t_first = ops.transform_bwd_input(g, g, wcat, None, amax=(g_amax, None), precision=precision)  # g @ wcat^T
        gx = ops.aggregate(merged, t_first.view(-1, d_in), tail=tail)
    else:
        gagg_amax = scales.slot() if scales is not None else None
        if _fused_backward(graph, g, r, d_in, d_out, g_amax, packed, precision):
            gx = ops.layer_bwd_input_fused(graph, g, packed, relu_mask, g_amax, amax_out=amax_out, tail=tail,
                                           inline_limit=_EVAL_INLINE_LIMIT, out_scale=out_scale, gagg_amax=gagg_amax)
        else:
            # (the transposed aggregate lives from this launch to the next one: sparse where that one can take it)
            sparse = gagg_amax is not None and _sparse_agg(graph, True, False, packed, g_amax, d_out, precision)
            if sparse:
                gagg = ops.aggregate_sparse(graph, g, transposed=True, tail=tail, amax_out=gagg_amax)[0]
            else:
                gagg = ops.aggregate(graph, g, transposed=True, tail=tail, amax_out=gagg_amax)   # autograd of A3 + A4
            amax, mul = _gagg_scale(graph, gagg_amax, g_amax)
            if (lower is not None and packed is not None and g_amax is not None
                    and _from_packed(lower[0], lower[2], precision) and _transform_first(graph, *lower, precision)
                    and ops.chain_supported(weight, lower[0])):
                gx, t = ops.transform_bwd_input_chain(gagg, g, weight, root, relu_mask, packed, lower[2], graph=graph,
                                                      amax=amax, amax_mul=mul, amax_out=amax_out, out_scale=out_scale,
                                                      sparse=sparse, row_order=_NT_ROW_ORDER)
            else:
                gx = ops.transform_bwd_input(gagg, g, weight, root, relu_mask=relu_mask, graph=graph, amax=amax,
                                             amax_mul=mul, amax_out=amax_out, packed=packed, precision=precision,
                                             out_scale=out_scale, sparse=sparse,
                                             row_order=_NT_ROW_ORDER)               # autograd of A6 wrt x
    return (gx, t) if lower is not None else gx


def _backward_scales(g: Tensor, layers: int) -> _Scales:
    """the operand scales of a backward pass through ``layers`` stacked layers, two per layer: the maximum of the gradient
    it receives (max |g|, or the ``amax_out`` of the layer above) and the slot ``_input_grad`` takes for its aggregate"""
    return _Scales(g, slots=2 * layers)


def _deferred_params(graph: "ops.BucketedGraph", agg, x, g, x_amax, g_amax, has_root: bool, has_bias: bool, prec,
                     packed=None):
    """a layer's parameter gradients, their slab reduction left pending: it rides in the gather that follows.  ``agg``
    is the forward's aggregate: a sparse one wherever _layer_train_forward made it so, and this asks _sparse_agg the
    same question with the same answers (the step's images ``packed``, the table's maximum, the width).  The one
    thing the backward does not know is the forward's table type; with an fp16 table the aggregate is dense and the
    kernel merely skips the loads of its stored zeros - the same bits."""
    sparse = _sparse_agg(graph, False, False, packed, x_amax, x.size(1), prec)
    return ops.transform_bwd_params(agg, x, g, graph.num_relations, want_root=has_root, want_bias=has_bias, graph=graph,
                                    defer=True, amax=(x_amax, x_amax, g_amax), precision=prec, sparse=sparse,
                                    amax_mul=_agg_bound(graph))


# Training forward of one layer: gather -> transform (two launches, the aggregate written by one and read by the
# other), or the one-kernel layer in its STORE mode (ops.layer_fwd_fused(agg_out=): the aggregate formed in LDS
# feeds the MFMAs directly and is written once, for the parameter gradients).  The fused form saves the read of
# the aggregate - worth it where the path is HBM-bound, i.e. once the aggregate no longer fits the 256 MB
# Infinity Cache; at C2's size the separate kernels are faster.  RGCN_TRAIN_FUSED = auto
# (default: by that size) | 1 | 0.  Same bits either way.
_TRAIN_FUSED = _os.environ.get("RGCN_TRAIN_FUSED", "auto")
_TRAIN_FUSED_MIN_BYTES = 256 << 20


def _defer_hubs(half: bool, packed, amax, k: int, n_out: int, graph=None) -> bool:
    """may a gather of k-wide rows leave its hub tails to the transform (n_out columns) that follows it?  Split
    precision with the operand's scale known beforehand; rows up to 128 wide and ONE column block of workgroups
    (at 256 the workgroups of every column block would each finish the same rows, with four row slots: measured
    1 % slower at C3)."""
    return (_DEFER_HUBS and not half and packed is not None and amax is not None and ops.GEMM_PRECISION == "split"
            and k in (64, 128) and n_out <= 128 and not (graph is not None and graph.edge_dropout))


_DEFER_HUBS = True


def _agg_bound(graph: "ops.BucketedGraph") -> float:
    """what max |table| is multiplied by to bound a FORWARD aggregate: 1 for a mean (it cannot exceed the table's
    maximum), the structure's weight bound for the weighted sums of an edge-dropout view - true for every draw"""
    return graph.weight_bound(False) if graph.edge_dropout else 1.0


def _train_fused(graph, n, r, d_in, d_out, half) -> bool:
    """the one-kernel training layer by the size policy (see above)"""
    fused = _TRAIN_FUSED == "1" or (_TRAIN_FUSED == "auto" and n * r * d_in * 4 >= _TRAIN_FUSED_MIN_BYTES)
    return bool(fused and not half and not graph.weighted_shard and n == graph.num_other_nodes
                and ops.GEMM_PRECISION == "split" and ops.fused_supported(r, d_in, d_out))


def _layer_train_forward(graph: "ops.BucketedGraph", x: Tensor, gather_dtype, weight, root, bias, relu: bool,
                         half: bool, x_amax, amax_out, packed):
    """-> (agg, out) of one layer's training forward"""
    n, r, d_in, d_out = x.size(0), graph.num_relations, x.size(1), weight.size(2)
    if (_train_fused(graph, n, r, d_in, d_out, half) and packed is not None and x_amax is not None):
        agg = ops._empty(n, r * d_in, dtype=torch.float32, device=x.device)
        out = ops.layer_fwd_fused(graph, x, packed, bias, relu, x_amax, amax_out, inline_limit=_EVAL_INLINE_LIMIT,
                                  agg_out=agg)
        return agg, out
    sparse = n == graph.num_other_nodes and _sparse_agg(graph, False, half, packed, x_amax, d_in)
    if sparse:
        # no zero rows stored, none read: by the transform below and by the parameter gradients (_deferred_params)
        agg, hubs = ops.aggregate_sparse(graph, x, defer=_defer_hubs(half, packed, x_amax, d_in, d_out, graph))
    elif _defer_hubs(half, packed, x_amax, d_in, d_out, graph):
        # the gather leaves its hub tails to the transform (one launch less); `agg` is complete once that has run
        agg, hubs = ops.aggregate_deferred(graph, x)
    else:
        agg, hubs = ops.aggregate(graph, _table(x, gather_dtype)), None
    out = ops.transform_fwd(agg, x, weight, root, bias, relu=relu, graph=graph, half=half, amax=(x_amax, x_amax),
                            amax_out=amax_out, packed=packed, hubs=hubs, sparse=sparse, amax_mul=_agg_bound(graph),
                            row_order=_NT_ROW_ORDER)
    return agg, out


def _packs(bufs, layers):
    return [ops.SplitWeights(b, w, root) if b is not None else None for b, (w, root) in zip(bufs, layers)]


def _conv_forward(x, weight, root, bias, *, graph, relu, gather_dtype, half):
    """one layer's training forward as a pass -> (out, agg, amax of x | None, split images | None)"""
    scales = _Scales(x, slots=1, layers=[(weight, root)])            # ONE launch: max |x| and the split weights
    x_amax = scales.first            # also the bound of agg: a mean of rows cannot exceed the table's maximum
    packed = scales.packed[0]                                         # once, for forward and backward
    agg, out = _layer_train_forward(graph, x, gather_dtype, weight, root, bias, relu, half, x_amax, None,
                                    packed)                           # rows A3 + A4, A6 (+ fused ReLU)
    return out, agg, x_amax, (packed.buf if packed is not None else None)


def _conv_backward(x, agg, weight, root, x_amax, pkbuf, g, *, graph, has_root, has_bias, need_x, need_p, prec):
    """one layer's backward as a pass -> (gx | None, gw | None, groot | None, gbias | None)"""
    packed = _packs([pkbuf], [(weight, root)])[0]
    scales = _backward_scales(g, 1)
    pending = (_deferred_params(graph, agg, x, g, x_amax, scales.first, has_root, has_bias, prec, packed)
               if need_p else None)
    gx = _input_grad(graph, g, weight, root, pending, scales.first, scales, packed, prec) if need_x else None
    if pending is None:
        return gx, None, None, None
    pending.finish()                                                    # no gather took it along
    return (gx, *pending.grads)


_R_CONV_FORWARD = ops.Region("conv.forward", _conv_forward)
_R_CONV_BACKWARD = ops.Region("conv.backward", _conv_backward)


def _contiguous(*tensors):
    return tuple(t.contiguous() if t is not None else None for t in tensors)


def _bwd_precision(gather_dtype, half_backward: bool) -> Optional[str]:
    """configs[4] backward: with the fp16 feature table the three gradient GEMMs per layer run as ONE fp16 pass (operands
    rounded under per-tensor power-of-two scales = loss scaling per tensor, fp32 accumulate); gathers stay fp32"""
    return "half" if (gather_dtype == torch.float16 and half_backward and ops.GEMM_PRECISION == "split") else None


class _RGCNConvFunction(torch.autograd.Function):
    """x, weight[R, d_in, d_out], root, bias -> out (optionally relu(out)), on a bucketed graph.

    This is what the reference's own call pattern reaches - ``x = self.conv1(x, edge_index, edge_type)`` ... ``x =
    self.conv2(x, edge_index, edge_type)``, ``/root/reference/src/models/rgcn.py:123-128`` - after INTEGRATION.md's
    import swap.  Forward and backward are ``ops.Region`` passes (round 4): after three calls on a graph each is one
    allocation and ONE native call (``rgcn_sequence_run``) instead of five to seven wrapper calls."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, root: Optional[Tensor], bias: Optional[Tensor],
                graph: ops.BucketedGraph, relu: bool = False, gather_dtype=None, half_backward: bool = False) -> Tensor:
        x, weight, root, bias = _contiguous(x, weight, root, bias)
        ctx.bwd_precision = _bwd_precision(gather_dtype, half_backward)
        key = (tuple(x.shape), tuple(weight.shape), root is not None, bias is not None, gather_dtype, bool(relu),
               _policy_key())
        out, agg, x_amax, pkbuf = _R_CONV_FORWARD.run(graph, key, (x, weight, root, bias),
                                                      dict(graph=graph, relu=relu, gather_dtype=gather_dtype,
                                                           half=gather_dtype == torch.float16), want={0})
        ctx.graph, ctx.relu, ctx.key = graph, relu, key
        ctx.has_root, ctx.has_bias = root is not None, bias is not None
        # the node's inputs and, for the ReLU backward, its output (autograd checks their versions)
        ctx.save_for_backward(x, weight, root, out if relu else None)
        ctx.kept = (agg, x_amax, pkbuf)                      # tensors, or arena offsets of a replayed pass
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        x, weight, root, out = ctx.saved_tensors
        agg, x_amax, pkbuf = ctx.kept
        if ctx.relu:
            g = g * (out > 0)                                               # ReLU backward (a torch op, outside the pass)
        g = g.contiguous()
        need_x, need_w, need_root, need_bias = ctx.needs_input_grad[:4]
        need_p = bool(need_w or (need_root and ctx.has_root) or (need_bias and ctx.has_bias))
        static = dict(graph=ctx.graph, has_root=ctx.has_root, has_bias=ctx.has_bias, need_x=bool(need_x), need_p=need_p,
                      prec=ctx.bwd_precision)
        gx, gw, groot, gbias = _R_CONV_BACKWARD.run(ctx.graph, (ctx.key, bool(need_x), need_p, ctx.bwd_precision),
                                                    (x, agg, weight, root, x_amax, pkbuf, g), static,
                                                    want={0, 1, 2, 3})
        return gx, gw, groot, gbias, None, None, None, None


def _enc2_layer1(x, w1, root1, b1, w2, root2, xa=None, w1a=None, r1a=None, w2a=None, r2a=None, *, graph, gather_dtype, half):
    """first launch of the pass (max |x|, cleared amax slots, both layers' split weights) + conv1 with its ReLU
    -> (h, agg1, amax of x, amax slot of h, split images of conv1, of conv2).  xa ... r2a: the maxima of x, w1, root1,
    w2, root2 where the optimizer left them (ops.amax_hint): the first launch then scans nothing."""
    given = (xa, [(w1a, r1a), (w2a, r2a)]) if xa is not None else None
    scales = _Scales(x, layers=[(w1, root1), (w2, root2)], given=given)
    x_amax, h_amax = scales.first, scales.slot()
    pk1, pk2 = scales.packed                                      # once, for forward and backward
    agg1, h = _layer_train_forward(graph, x, gather_dtype, w1, root1, b1, True, half, x_amax, h_amax, pk1)
    return h, agg1, x_amax, h_amax, (pk1.buf if pk1 is not None else None), (pk2.buf if pk2 is not None else None)


def _enc2_layer2(h, w2, root2, b2, h_amax, pk2buf, *, graph, gather_dtype, half):
    pk2 = _packs([pk2buf], [(w2, root2)])[0]
    agg2, out = _layer_train_forward(graph, h, gather_dtype, w2, root2, b2, False, half, h_amax, None, pk2)
    return out, agg2


def _enc2_forward(x, w1, root1, b1, w2, root2, b2, xa=None, w1a=None, r1a=None, w2a=None, r2a=None, *, graph, gather_dtype,
                  half):
    """both layers (no dropout between them) as one pass -> (out, h, agg1, agg2, amax of x, of h, images 1, images 2)"""
    h, agg1, x_amax, h_amax, pk1buf, pk2buf = _enc2_layer1(x, w1, root1, b1, w2, root2, xa, w1a, r1a, w2a, r2a, graph=graph,
                                                           gather_dtype=gather_dtype, half=half)
    out, agg2 = _enc2_layer2(h, w2, root2, b2, h_amax, pk2buf, graph=graph, gather_dtype=gather_dtype, half=half)
    return out, h, agg1, agg2, x_amax, h_amax, pk1buf, pk2buf


def _enc2_backward(x, agg1, h, agg2, w1, root1, w2, root2, x_amax, h_amax, pk1buf, pk2buf, g, *, graph, flags, p,
                   prec, need_x):
    """the whole backward of conv1 -> ReLU -> [dropout p] -> conv2 -> (gx | None, gw1, groot1, gb1, gw2, groot2, gb2)"""
    has_root1, has_b1, has_root2, has_b2 = flags
    pk1, pk2 = _packs([pk1buf, pk2buf], [(w1, root1), (w2, root2)])
    scales = _backward_scales(g, 2)
    g_amax, gz_amax = scales.first, scales.slot()
    # the slab reductions of the parameter gradients ride in the transposed gathers that follow them
    red2 = _deferred_params(graph, agg2, h, g, h_amax, g_amax, has_root2, has_b2, prec, pk2)
    # gz = d loss / d (pre-ReLU of conv1): ReLU mask h (positive exactly where a unit is active and kept), the dropout
    # factor 1 / (1 - p) one more epilogue scalar; where conv1's gradient is wanted, the launch may form its T too
    gz = _input_grad(graph, g, w2, root2, red2, g_amax, scales, pk2, prec, relu_mask=h,
                     out_scale=1.0 / (1.0 - p) if p > 0 else 1.0, amax_out=gz_amax,
                     lower=(w1, root1, pk1) if need_x else None)
    gz, t_first = gz if need_x else (gz, None)
    red1 = _deferred_params(graph, agg1, x, gz, x_amax, gz_amax, has_root1, has_b1, prec, pk1)
    gx = _input_grad(graph, gz, w1, root1, red1, gz_amax, scales, pk1, prec, t_first) if need_x else None
    red2.finish()
    red1.finish()
    return (gx, *red1.grads, *red2.grads)


_R_LAYER1 = ops.Region("encoder2.layer1", _enc2_layer1)
_R_LAYER2 = ops.Region("encoder2.layer2", _enc2_layer2)
_R_FORWARD = ops.Region("encoder2.forward", _enc2_forward)
_R_BACKWARD = ops.Region("encoder2.backward", _enc2_backward)


def _policy_key():
    return (_TRAIN_FUSED, _DEFER_HUBS, _TRANSFORM_FIRST_RATIO, _EVAL_INLINE_LIMIT, _TRAIN_FUSED_MIN_BYTES, _SPARSE_AGG,
            _NT_ROW_ORDER)


def _enc2_train_forward(graph, params, gather_dtype, half_backward: bool, hints, p: float = 0.0):
    """The forward of both training routes into the encoder (``_Encoder2Function``, ``rgcn_encoder2_step``): ``params``
    = (x, w1, root1, b1, w2, root2, b2) -> (out, ``params`` made contiguous, the state ``_enc2_train_backward`` takes).
    ``hints``: the maxima of x, w1, root1, w2, root2 the optimizer left (``_encoder_hints``).  One key: one plan."""
    x, w1, root1, b1, w2, root2, b2 = params = _contiguous(*params)
    hinted = hints is not None and ops.GEMM_PRECISION == "split"
    hint_list = list(hints) if hinted else []
    key = (tuple(x.shape), tuple(w1.shape), tuple(w2.shape), root1 is not None, b1 is not None, root2 is not None,
           b2 is not None, gather_dtype, hinted, _policy_key())
    static = dict(graph=graph, gather_dtype=gather_dtype, half=gather_dtype == torch.float16)
    # A dense tensor's maximum is left behind by the launch that produces it (the first launch of the pass
    # for x - or the optimizer step that wrote x -, the epilogue of conv1's transform for h); an aggregate is scaled
    # by the bound its table's maximum gives (a mean of rows cannot exceed it), so the gathers publish nothing.
    if p > 0:
        h, agg1, x_amax, h_amax, pk1buf, pk2buf = _R_LAYER1.run(graph, key, [x, w1, root1, b1, w2, root2] + hint_list,
                                                                static, want={0, 3})
        h = torch.native_dropout(h, p, True)[0]
        h_amax = ops.materialize(h_amax) * (1.0 / (1.0 - p)) if h_amax is not None else None   # kept units are scaled up
        out, agg2 = _R_LAYER2.run(graph, key, (h, w2, root2, b2, h_amax, pk2buf), static, want={0})
    else:
        out, h, agg1, agg2, x_amax, h_amax, pk1buf, pk2buf = _R_FORWARD.run(graph, key, list(params) + hint_list, static,
                                                                            want={0})
    flags = (root1 is not None, b1 is not None, root2 is not None, b2 is not None)
    kept = (agg1, h, agg2, x_amax, h_amax, pk1buf, pk2buf)      # tensors, or arena offsets of a replayed pass
    return out, params, (graph, key, flags, p, _bwd_precision(gather_dtype, half_backward), kept)


def _enc2_train_backward(state, inputs, g: Tensor, need_x: bool):
    """the backward pass of both routes; ``inputs`` = (x, w1, root1, w2, root2) as ``_enc2_train_forward`` made them
    -> (gx | None, gw1, groot1, gb1, gw2, groot2, gb2)"""
    graph, key, flags, p, prec, (agg1, h, agg2, x_amax, h_amax, pk1buf, pk2buf) = state
    x, w1, root1, w2, root2 = inputs
    return _R_BACKWARD.run(graph, (key, p, need_x, prec),
                           (x, agg1, h, agg2, w1, root1, w2, root2, x_amax, h_amax, pk1buf, pk2buf, g.contiguous()),
                           dict(graph=graph, flags=flags, p=p, prec=prec, need_x=need_x), want={0, 1, 2, 3, 4, 5, 6})


class _Encoder2Function(torch.autograd.Function):
    """conv1 -> ReLU -> [dropout] -> conv2 (``src/models/rgcn.py:123-128``) as one autograd
    node: the ReLU rides in conv1's GEMM epilogue, and its backward rides in the epilogue of
    conv2's input-gradient GEMM (which then emits the gradient with respect to conv1's
    pre-activation directly), so no elementwise kernel runs between the layers.

    With ``p > 0`` the mask is drawn by torch's own dropout kernel from torch's RNG stream,
    exactly where ``rgcn.py:125`` draws it.  Its backward costs nothing extra: the dropped
    activations ``hd = relu(z) * m / (1-p)`` are positive exactly where the unit is both active
    and kept, so ``hd`` is the epilogue mask, and the factor ``1/(1-p)`` is one more scalar of that
    GEMM's epilogue (``out_scale``): the step's split weight images serve the dropout case
    unchanged.

    Forward and backward are ``ops.Region`` passes: after three steps on a graph their launches are
    issued by one native call each (``rgcn_sequence_run``) instead of ~14 wrapper calls."""

    @staticmethod
    def forward(ctx, x, w1, root1, b1, w2, root2, b2, graph, gather_dtype=None, p: float = 0.0,
                half_backward: bool = False, hints=None):
        out, (x, w1, root1, _, w2, root2, _), ctx.state = _enc2_train_forward(
            graph, (x, w1, root1, b1, w2, root2, b2), gather_dtype, half_backward, hints, p)
        ctx.save_for_backward(x, w1, root1, w2, root2)           # the node's inputs (autograd checks their versions)
        return out

    @staticmethod
    def backward(ctx, g):
        grads = _enc2_train_backward(ctx.state, ctx.saved_tensors, g, bool(ctx.needs_input_grad[0]))
        return (*grads, None, None, None, None, None)


# No-grad encoder (``DrugDiseaseModel.get_embeddings / predict / predict_all_tails``, ``Trainer.validate``,
# ``ModelEvaluator``: src/train.py:389-395, src/evaluate.py:189-195, 251-254): nothing needs the aggregate
# afterwards, so it is never materialised as one [N, R * d] tensor once that would exceed _EVAL_BLOCK_BYTES:
# the destination rows are walked in blocks - gather a block into ONE reused buffer, transform it straight
# into its rows of the output, next block.  Same kernels, same per-segment order: results equal the training
# path's bit for bit.
# What this buys is MEMORY (C4 on one GPU, 2-layer forward: peak 5.10 GiB -> 1.32 GiB with 32 MB blocks), not
# traffic: measured with rocprofv3 FETCH_SIZE / WRITE_SIZE the HBM-side bytes of the blocked forward are not
# lower (a block written by one launch is re-read by the next through the memory side: the 4 MB L2s are per XCD
# and the 256 MB Infinity Cache is already cycling the 256 MB row table), and 128 blocks x 3 launches per layer
# cost time (13.5 ms against 5.95 ms per forward; tools/eval_blocks_probe.py).  Hence the default block is
# large - 1 GiB: C2 runs as one block, C4 as four - and DESIGN.md section 9 says what a real fusion of the
# gather into the transform's A tile would have to look like.
_EVAL_BLOCK_BYTES = 1 << 30


# RGCN_EVAL_FUSED (default auto): the one-kernel layer (ops.layer_fwd_fused: the aggregate lives in LDS only) wherever it
# covers the shape - auto: once the aggregate would reach 256 MB, where the path is HBM-bound (C4 on one GPU: 6.0 -> 3.5
# ms per 2-layer forward); at C2's size the two launches are as fast (0.114 against 0.118 ms) -, 1: always, 0 = the
# two-launch path below.  _EVAL_INLINE_LIMIT: longest segment the fused kernel walks
# itself (longer ones are pre-aggregated by the ordinary gather).
_EVAL_FUSED = _os.environ.get("RGCN_EVAL_FUSED", "auto")          # "auto" | "1" | "0" (tests also set True / False)


def _eval_fused(n: int, r: int, d_in: int) -> bool:
    if _EVAL_FUSED in (True, "1"):
        return True
    if _EVAL_FUSED in (False, "0"):
        return False
    return n * r * d_in * 4 >= _TRAIN_FUSED_MIN_BYTES          # the same threshold as the training layers
_EVAL_INLINE_LIMIT = 16


def _layer_eval_blocked(graph: "ops.BucketedGraph", x: Tensor, table: Tensor, weight: Tensor, root, bias, relu: bool,
                        half: bool, amax, amax_out, packed) -> Tensor:
    n, r, d_in, d_out = x.size(0), graph.num_relations, x.size(1), weight.size(2)
    if (_eval_fused(n, r, d_in) and not half and packed is not None and amax[1] is not None and not graph.weighted_shard
            and x.size(0) == graph.num_other_nodes and ops.fused_supported(r, d_in, d_out)):
        return ops.layer_fwd_fused(graph, x, packed, bias, relu, amax[1], amax_out, inline_limit=_EVAL_INLINE_LIMIT)
    rows = max(32, _EVAL_BLOCK_BYTES // max(1, r * d_in * 4))
    out = ops._empty(n, d_out, dtype=torch.float32, device=x.device)
    if rows >= n:                                   # one block: the plain two launches, a temporary aggregate
        agg = ops.aggregate(graph, table)
        return ops.transform_fwd(agg, x, weight, root, bias, relu=relu, graph=graph, half=half, amax=amax,
                                 amax_out=amax_out, packed=packed, out=out)
    blocks = graph.row_blocks(rows)
    buf = ops._empty(blocks[0][1] - blocks[0][0], r * d_in, dtype=torch.float32, device=x.device)
    for lo, hi, shard in blocks:
        agg = ops.aggregate(shard, table, out=buf[: hi - lo])
        ops.transform_fwd(agg, x[lo:hi], weight, root, bias, relu=relu, graph=shard, half=half, amax=amax,
                          amax_out=amax_out, packed=packed, out=out[lo:hi])
    return out


def _enc2_eval(x, w1, root1, b1, w2, root2, b2, *, graph, gather_dtype):
    half = gather_dtype == torch.float16
    scales = _Scales(x, layers=[(w1, root1), (w2, root2)])
    x_amax, h_amax = scales.first, scales.slot()
    pk1, pk2 = scales.packed
    h = _layer_eval_blocked(graph, x, _table(x, gather_dtype), w1, root1, b1, True, half, (x_amax, x_amax), h_amax, pk1)
    return (_layer_eval_blocked(graph, h, _table(h, gather_dtype), w2, root2, b2, False, half, (h_amax, h_amax), None, pk2),)


_R_EVAL = ops.Region("encoder2.eval", _enc2_eval)


def encoder2_eval(x: Tensor, graph: "ops.BucketedGraph", w1, root1, b1, w2, root2, b2, gather_dtype=None) -> Tensor:
    """conv2(relu(conv1(x))) with nothing kept for a backward and no whole-graph aggregate (see above); a Region:
    one native call per forward once recorded (``Trainer.validate`` re-runs it for every validation batch,
    src/train.py:389-395)"""
    x, w1, root1, b1, w2, root2, b2 = _contiguous(x, w1, root1, b1, w2, root2, b2)
    key = (tuple(x.shape), tuple(w1.shape), tuple(w2.shape), root1 is not None, b1 is not None, root2 is not None,
           b2 is not None, gather_dtype, _EVAL_FUSED, _EVAL_BLOCK_BYTES, _EVAL_INLINE_LIMIT)
    return _R_EVAL.run(graph, key, (x, w1, root1, b1, w2, root2, b2), dict(graph=graph, gather_dtype=gather_dtype), want={0})[0]


def _check_x(x: Tensor) -> None:
    if x.dtype != torch.float32:
        raise TypeError(f"x must be float32 (got {x.dtype}); integer-index / embedding mode of "
                        f"PyG's RGCNConv is not used by the reference and not implemented")


def _check_gather_dtype(gather_dtype) -> None:
    if gather_dtype not in (None, torch.float32, torch.float16):
        raise ValueError(f"gather_dtype must be None, torch.float32 or torch.float16, got {gather_dtype}")


def _resolve_graph(graph: Optional["ops.BucketedGraph"], edge_index: Tensor, edge_type: Tensor, num_nodes: int,
                   num_relations: int, differentiating: bool) -> "ops.BucketedGraph":
    """the structure a layer runs over: the cached bucketing of its columns, or the caller's ``graph=`` override - the
    view of an ``ops.EdgeDropout`` on that bucketing.  A view stands for its parent wherever nothing is differentiated
    (eval mode, no_grad without dropout): dropout regularises training, scoring sees the whole graph."""
    if graph is None:
        return ops.bucket(edge_index, edge_type, num_nodes, num_relations)
    if not isinstance(graph, ops.BucketedGraph) or graph.bipartite:
        raise ValueError("graph= takes a whole bucketed graph or the view of an ops.EdgeDropout")
    if graph.num_nodes != num_nodes or graph.num_relations != num_relations:
        raise ValueError(f"graph= has {graph.num_nodes} nodes and {graph.num_relations} relations; x has {num_nodes} rows "
                         f"and the layer {num_relations} relations")
    if graph.edge_dropout and not differentiating:
        return graph.parent
    return graph


def _differentiating(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def rgcn_conv(x: Tensor, edge_index: Tensor, edge_type: Tensor, weight: Tensor,
              root: Optional[Tensor], bias: Optional[Tensor], num_relations: int,
              activation: Optional[str] = None, gather_dtype=None, half_backward: bool = False,
              graph: Optional["ops.BucketedGraph"] = None) -> Tensor:
    """Functional form on effective weights ``[R, d_in, d_out]``; ``activation='relu'`` fuses
    the ReLU into the layer; ``gather_dtype=torch.float16`` makes the forward gather read an fp16
    copy of the feature table (fp32 accumulate; BASELINE configs[4]); gradients stay fp32.  ``graph``: run over this
    structure instead of the bucketing of ``edge_index`` (``_resolve_graph``)."""
    _check_x(x)
    _check_gather_dtype(gather_dtype)
    if activation not in (None, "relu"):
        raise ValueError(f"activation must be None or 'relu', got {activation!r}")
    graph = _resolve_graph(graph, edge_index, edge_type, x.size(0), num_relations, _differentiating(x, weight, root, bias))
    return _RGCNConvFunction.apply(x, weight, root, bias, graph, activation == "relu", gather_dtype, half_backward)


def _encoder_hints(x: Tensor, conv1: "RGCNConv", conv2: "RGCNConv"):
    """the operand maxima the optimizer left (``ops.amax_hint``) for x, conv1.weight / root, conv2.weight / root - all
    of them or None (plain weights with a root, fp32 table, split precision)"""
    if not ops._AMAX_HINTS:                       # nobody left a maximum (no native optimizer step): nothing to look up
        return None
    if ops.GEMM_PRECISION != "split" or conv1.num_bases is not None or conv2.num_bases is not None:
        return None
    if conv1.root is None or conv2.root is None or conv1.gather_dtype not in (None, torch.float32):
        return None
    hints = tuple(ops.amax_hint(t) for t in (x, conv1.weight, conv1.root, conv2.weight, conv2.root))
    return hints if all(h is not None for h in hints) else None


def rgcn_encoder2(x: Tensor, edge_index: Tensor, edge_type: Tensor, conv1: "RGCNConv",
                  conv2: "RGCNConv", dropout_p: float = 0.0, graph: Optional["ops.BucketedGraph"] = None) -> Tensor:
    """``conv2(dropout(relu(conv1(x)), dropout_p))`` through the fused two-layer autograd node
    (``dropout_p`` = 0: no dropout, e.g. eval mode).  ``graph``: run over this structure instead of the bucketing of
    ``edge_index`` (``_resolve_graph``: an edge-dropout view counts only where something is differentiated or dropped)."""
    _check_x(x)
    if not 0.0 <= dropout_p < 1.0:
        raise ValueError(f"dropout_p must be in [0, 1), got {dropout_p}")
    tensors = [x] + list(conv1.parameters()) + list(conv2.parameters())
    graph = _resolve_graph(graph, edge_index, edge_type, x.size(0), conv1.num_relations,
                           dropout_p > 0.0 or _differentiating(*tensors))
    if dropout_p == 0.0 and not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors)):
        return encoder2_eval(x, graph, conv1.effective_weight(), conv1.root, conv1.bias, conv2.effective_weight(),
                             conv2.root, conv2.bias, conv1.gather_dtype)       # nothing to differentiate, no dropout
    return _Encoder2Function.apply(x, conv1.effective_weight(), conv1.root, conv1.bias,
                                   conv2.effective_weight(), conv2.root, conv2.bias, graph,
                                   conv1.gather_dtype, float(dropout_p), conv1.half_backward,
                                   _encoder_hints(x, conv1, conv2))


def _accumulate(param: Optional[Tensor], grad: Optional[Tensor]) -> None:
    """what the autograd engine does with a leaf's gradient: ``.grad`` is set, or added to"""
    if param is None or grad is None or not param.requires_grad:
        return
    if param.grad is None:
        param.grad = grad
    else:
        param.grad.add_(grad)


@torch.no_grad()
def rgcn_encoder2_step(x: Tensor, edge_index: Tensor, edge_type: Tensor, conv1: "RGCNConv", conv2: "RGCNConv",
                       cotangent: Tensor, need_input_grad: bool = True):
    """One explicit encoder step - ``out = conv2(relu(conv1(x)))`` and the backward for a GIVEN cotangent
    ``d loss / d out`` - WITHOUT the autograd engine: the two recorded passes of ``_Encoder2Function`` issued directly
    (two native calls once recorded), the parameter gradients accumulated into ``.grad`` as ``out.backward(cotangent)``
    would, ``-> (out, grad_x | None)``.  For callers that hold the cotangent themselves (a benchmark loop, a
    pipeline whose loss gradient arrives from elsewhere, ``dist.PartitionedEncoder``): the engine's hop to its backward
    thread and the ``Function`` plumbing cost more host time (~105 us) than issuing both passes (VERDICT r3 item 7;
    ``tools/host_profile.py``).  Same kernels, same bits as the autograd route; no dropout between the layers (a
    caller with a loss uses ``rgcn_encoder2``)."""
    _check_x(x)
    graph = ops.bucket(edge_index, edge_type, x.size(0), conv1.num_relations)
    basis1, basis2 = conv1.num_bases is not None, conv2.num_bases is not None
    w1 = ops.basis_compose(conv1.comp.contiguous(), conv1.weight.contiguous()) if basis1 else conv1.weight
    w2 = ops.basis_compose(conv2.comp.contiguous(), conv2.weight.contiguous()) if basis2 else conv2.weight
    out, (x, w1, root1, _, w2, root2, _), state = _enc2_train_forward(
        graph, (x, w1, conv1.root, conv1.bias, w2, conv2.root, conv2.bias), conv1.gather_dtype, conv1.half_backward,
        _encoder_hints(x, conv1, conv2))
    gx, gw1, groot1, gb1, gw2, groot2, gb2 = _enc2_train_backward(state, (x, w1, root1, w2, root2), cotangent,
                                                                  bool(need_input_grad))
    for conv, gw, groot, gb, basis in ((conv1, gw1, groot1, gb1, basis1), (conv2, gw2, groot2, gb2, basis2)):
        if basis:
            gcomp, gbasis = ops.basis_compose_bwd(gw, conv.comp.contiguous(), conv.weight.contiguous(),
                                                  conv.comp.requires_grad, conv.weight.requires_grad)
            _accumulate(conv.comp, gcomp)
            _accumulate(conv.weight, gbasis)
        else:
            _accumulate(conv.weight, gw)
        _accumulate(conv.root, groot)
        _accumulate(conv.bias, gb)
    return out, gx


class RGCNConv(nn.Module):
    r"""Relational graph convolution, mean aggregation per (destination, relation):

    .. math:: x'_i = \Theta_{root} x_i + \sum_r \frac{1}{|N_r(i)|} \sum_{j \in N_r(i)} \Theta_r x_j + b

    Messages flow ``edge_index[0] -> edge_index[1]``; duplicate edges count once each;
    no self loops are added; an empty ``(i, r)`` contributes exactly 0.
    """

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int,
                 num_relations: int, num_bases: Optional[int] = None,
                 num_blocks: Optional[int] = None, aggr: str = "mean", root_weight: bool = True,
                 is_sorted: bool = False, bias: bool = True, gather_dtype=None,
                 half_backward: Optional[bool] = None, **kwargs):
        super().__init__()
        _check_gather_dtype(gather_dtype)
        self.gather_dtype = gather_dtype    # None/float32, or float16: fp16 row table, fp32 accumulate
        # configs[4]: with the fp16 feature table the gradient GEMMs take fp16 operands too (fp32 accumulate)
        self.half_backward = (gather_dtype == torch.float16) if half_backward is None else bool(half_backward)
        if num_bases is not None and num_blocks is not None:
            raise ValueError("Can not apply both basis-decomposition and "
                             "block-diagonal-decomposition at the same time.")
        if num_blocks is not None:
            raise NotImplementedError("block-diagonal decomposition is not used by the reference "
                                      "(rgcn.py:72-85) and is not implemented")
        if aggr != "mean":
            raise NotImplementedError(f"aggr={aggr!r}: only PyG's default 'mean' is implemented")
        if kwargs:
            raise TypeError(f"unexpected keyword arguments: {sorted(kwargs)}")
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        if in_channels[0] != in_channels[1]:
            raise NotImplementedError("bipartite (x_l, x_r) inputs are not implemented")
        self.in_channels = in_channels
        self.in_channels_l = in_channels[0]
        self.out_channels = out_channels
        self.num_relations = num_relations
        self.num_bases = num_bases
        self.num_blocks = num_blocks
        self.is_sorted = is_sorted      # accepted; bucketing makes it irrelevant

        if num_bases is not None:
            self.weight = nn.Parameter(torch.empty(num_bases, in_channels[0], out_channels))
            self.comp = nn.Parameter(torch.empty(num_relations, num_bases))
        else:
            self.weight = nn.Parameter(torch.empty(num_relations, in_channels[0], out_channels))
            self.register_parameter("comp", None)
        if root_weight:
            self.root = nn.Parameter(torch.empty(in_channels[1], out_channels))
        else:
            self.register_parameter("root", None)
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        _glorot(self.weight)
        _glorot(self.comp)
        _glorot(self.root)
        if self.bias is not None:
            with torch.no_grad():
                self.bias.zero_()

    def effective_weight(self) -> Tensor:
        """``weight`` or the basis composition ``comp[R, B] @ weight[B, d_in*d_out]`` (row A5)."""
        if self.num_bases is None:
            return self.weight
        return _BasisCompose.apply(self.comp, self.weight)

    def forward(self, x: Tensor, edge_index: Tensor, edge_type: Optional[Tensor] = None,
                activation: Optional[str] = None, graph: Optional["ops.BucketedGraph"] = None) -> Tensor:
        """PyG's ``forward(x, edge_index, edge_type)``; the extra keyword ``activation='relu'``
        returns ``relu(out)`` with the ReLU fused into the transform's epilogue; ``graph``: the view of an
        ``ops.EdgeDropout`` on this graph.  A view counts only where something is differentiated: in ``eval()``, under
        ``no_grad``, and also in training mode with grad enabled when neither ``x`` nor any parameter requires grad
        (all frozen), the layer runs over the view's PARENT, the whole graph - a caller who drew on purpose and wants
        the dropped graph there calls ``ops.aggregate`` / ``ops.transform_fwd`` on the view itself."""
        if isinstance(x, (tuple, list)) or x is None:
            raise NotImplementedError("x must be a float tensor [N, in_channels]")
        if not isinstance(edge_index, Tensor):
            raise NotImplementedError("SparseTensor adjacency is not implemented")
        assert edge_type is not None, "edge_type is required"
        if x.dim() != 2 or x.size(1) != self.in_channels_l:
            raise ValueError(f"x must be [N, {self.in_channels_l}], got {tuple(x.shape)}")
        if graph is not None and graph.edge_dropout and not self.training:
            graph = graph.parent
        return rgcn_conv(x, edge_index, edge_type, self.effective_weight(), self.root, self.bias,
                         self.num_relations, activation, self.gather_dtype, self.half_backward, graph=graph)

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}({self.in_channels_l}, {self.out_channels}, "
                f"num_relations={self.num_relations})")
