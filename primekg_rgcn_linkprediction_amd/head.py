"""DistMult and ComplEx scoring heads on the HIP library.

Mirror of the reference's ``LinkPredictor`` (``src/models/rgcn.py:145-243``): same
constructor ``(num_relations, embedding_dim, dropout=0.0)``, same parameter
(``relation_embeddings.weight`` [R, d], xavier-uniform), same methods
``forward(head_embeddings, tail_embeddings, relation_types)`` and
``score_all_tails(head_embeddings, relation_types, all_tail_embeddings)``.

Extra entry ``score_triples(node_embeddings, head_idx, tail_idx, relation_types)`` fuses
the two row gathers of ``rgcn.py:325-326`` into the scoring kernel (SURVEY row C1 + C2).

``LinkPredictor(..., decoder="complex")`` scores with ComplEx, ``Re <h, r, conj(t)>`` (``include/rgcn_complex.h``): a
row of width d is d / 2 complex numbers, real parts first, so the parameter and the checkpoint keys are DistMult's.
Unlike DistMult it tells ``(h, r, t)`` from ``(t, r, h)``: the tail enters conjugated.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import ops


class _DistMultFunction(torch.autograd.Function):
    """scores[b] = sum_d H[hi(b)] * Rm[ri(b)] * T[ti(b)]; an index of None means row b."""

    @staticmethod
    def forward(ctx, h: Tensor, h_idx: Optional[Tensor], t: Tensor, t_idx: Optional[Tensor],
                r: Tensor, r_idx: Optional[Tensor]) -> Tensor:
        h, t, r = h.contiguous(), t.contiguous(), r.contiguous()
        h_idx = h_idx.contiguous() if h_idx is not None else None
        t_idx = t_idx.contiguous() if t_idx is not None else None
        r_idx = r_idx.contiguous() if r_idx is not None else None
        batch = (h_idx if h_idx is not None else h).size(0)
        scores = ops.distmult_fwd(h, h_idx, t, t_idx, r, r_idx, batch)
        ctx.batch = batch
        ctx.same_ht = h.data_ptr() == t.data_ptr() and h.shape == t.shape
        ctx.save_for_backward(h, h_idx, t, t_idx, r, r_idx)
        return scores

    @staticmethod
    def backward(ctx, gs: Tensor):
        h, h_idx, t, t_idx, r, r_idx = ctx.saved_tensors
        gs = gs.contiguous()
        need_h, _, need_t, _, need_r, _ = ctx.needs_input_grad

        def buf(src, idx, need):                     # (an indexed table is cleared by the backward's first launch)
            return torch.empty_like(src) if need else None

        gh = buf(h, h_idx, need_h)
        # head and tail gathered from one table: accumulate both into one buffer
        shared = ctx.same_ht and need_h and need_t and h_idx is not None and t_idx is not None
        gt = gh if shared else buf(t, t_idx, need_t)
        gr = buf(r, r_idx, need_r)
        ops.distmult_bwd(gs, h, h_idx, t, t_idx, r, r_idx, ctx.batch, gh, gt, gr, zero_tables=True)
        if shared:
            # autograd sums the two returned grads of the same leaf: hand back the whole
            # accumulation once and an untouched None for the second slot
            return gh, None, None, None, gr, None
        return gh, None, gt, None, gr, None


class _RelationRows(torch.autograd.Function):
    """``table[idx]`` for the [R, d] relation table.  Thousands of samples share R rows, which
    is the worst case for an atomic / sort based embedding backward (160 us per step measured
    with ``nn.Embedding``); here the table gradient is a fixed two-level tree over 256-sample
    segments (``ops.segment_sum``) -- deterministic, a few microseconds."""

    @staticmethod
    def forward(ctx, table: Tensor, idx: Tensor) -> Tensor:
        ctx.save_for_backward(idx)
        ctx.rows = table.size(0)
        return table.index_select(0, idx)

    @staticmethod
    def backward(ctx, g: Tensor):
        (idx,) = ctx.saved_tensors
        return ops.segment_sum(g.contiguous(), idx.contiguous(), ctx.rows), None


class _DistMultBCEFunction(torch.autograd.Function):
    """(mean binary_cross_entropy_with_logits(scores, labels), scores): the scoring kernel also
    emits the per-sample loss, and ONE backward kernel turns the gradient of the mean loss into
    the head / tail / relation gradients (sigmoid, subtraction, 1/B and the DistMult products
    fused) - instead of the eight elementwise launches of BCEWithLogitsLoss around the head
    (``src/train.py:300``).  ``scores`` is returned for the accuracy bookkeeping only."""

    @staticmethod
    def forward(ctx, h, h_idx, t, t_idx, r, r_idx, labels, stats=None):
        h, t, r = h.contiguous(), t.contiguous(), r.contiguous()
        h_idx, t_idx, r_idx = (i.contiguous() if i is not None else None for i in (h_idx, t_idx, r_idx))
        labels = labels.contiguous()
        batch = (h_idx if h_idx is not None else h).size(0)
        scores, per_sample = ops.distmult_bce_fwd(h, h_idx, t, t_idx, r, r_idx, labels, batch)
        ctx.batch = batch
        ctx.same_ht = h.data_ptr() == t.data_ptr() and h.shape == t.shape
        ctx.save_for_backward(h, h_idx, t, t_idx, r, r_idx, labels, scores)
        ctx.mark_non_differentiable(scores)
        ctx.set_materialize_grads(False)             # (no zero-filled stand-in for the gradient of `scores` per step)
        # the mean in a fixed order and, when the caller keeps running sums on the device (``stats`` = (loss_sum,
        # correct, cursor, cursor_add), any of the first three None), the step's bookkeeping in the same launch
        loss_sum, correct, cursor, cursor_add = stats if stats is not None else (None, None, None, 0)
        mean = ops.distmult_bce_reduce(per_sample, scores, labels, loss_sum, correct, cursor, cursor_add)
        return mean.reshape(()), scores

    @staticmethod
    def backward(ctx, g_loss, _g_scores):
        h, h_idx, t, t_idx, r, r_idx, labels, scores = ctx.saved_tensors
        need_h, _, need_t, _, need_r, _, _, _ = ctx.needs_input_grad
        if g_loss is None:                           # nothing downstream used the loss
            return (None,) * 8

        def buf(src, idx, need):                     # (an indexed table is cleared by the backward's first launch)
            return torch.empty_like(src) if need else None

        gh = buf(h, h_idx, need_h)
        shared = ctx.same_ht and need_h and need_t and h_idx is not None and t_idx is not None
        gt = gh if shared else buf(t, t_idx, need_t)
        gr = buf(r, r_idx, need_r)
        ops.distmult_bce_bwd(g_loss.reshape(1).contiguous(), scores, labels, h, h_idx, t, t_idx, r, r_idx,
                             ctx.batch, gh, gt, gr, zero_tables=True)
        if shared:
            return gh, None, None, None, gr, None, None, None
        return gh, None, gt, None, gr, None, None, None


class _ScoreAllTailsFunction(torch.autograd.Function):
    """``(head * rel[rel_idx]) @ emb.T``; the gradients are three small dense products (the reference never asks for
    them - ``score_all_tails`` runs under ``no_grad`` in ``evaluate.py`` - so they stay on the library GEMM)."""

    @staticmethod
    def forward(ctx, head: Tensor, rel: Tensor, rel_idx: Tensor, emb: Tensor) -> Tensor:
        head, rel, emb = head.contiguous(), rel.contiguous(), emb.contiguous()
        rel_idx = rel_idx.contiguous()
        scores, hr = ops.distmult_score_all_tails(head, rel, rel_idx, emb)
        ctx.save_for_backward(head, rel, rel_idx, emb, hr)
        return scores

    @staticmethod
    def backward(ctx, g: Tensor):
        head, rel, rel_idx, emb, hr = ctx.saved_tensors
        g = g.contiguous()
        grad_head = grad_rel = grad_emb = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            grad_hr = g @ emb
            if ctx.needs_input_grad[0]:
                grad_head = grad_hr * rel[rel_idx]
            if ctx.needs_input_grad[1]:
                grad_rel = torch.zeros_like(rel).index_add_(0, rel_idx, grad_hr * head)
        if ctx.needs_input_grad[3]:
            grad_emb = g.t() @ hr
        return grad_head, grad_rel, None, grad_emb


class _ComplExFunction(torch.autograd.Function):
    """scores[b] = Re <H[hi(b)], Rm[ri(b)], conj(T[ti(b)])>; an index of None means row b."""

    @staticmethod
    def forward(ctx, h: Tensor, h_idx: Optional[Tensor], t: Tensor, t_idx: Optional[Tensor],
                r: Tensor, r_idx: Optional[Tensor]) -> Tensor:
        h, t, r = h.contiguous(), t.contiguous(), r.contiguous()
        h_idx, t_idx, r_idx = (i.contiguous() if i is not None else None for i in (h_idx, t_idx, r_idx))
        batch = (h_idx if h_idx is not None else h).size(0)
        scores = ops.complex_fwd(h, h_idx, t, t_idx, r, r_idx, batch)
        ctx.batch = batch
        ctx.same_ht = h.data_ptr() == t.data_ptr() and h.shape == t.shape
        ctx.save_for_backward(h, h_idx, t, t_idx, r, r_idx)
        return scores

    @staticmethod
    def backward(ctx, gs: Tensor):
        h, h_idx, t, t_idx, r, r_idx = ctx.saved_tensors
        need_h, _, need_t, _, need_r, _ = ctx.needs_input_grad
        gh = torch.empty_like(h) if need_h else None
        # head and tail gathered from one table: accumulate both into one buffer
        shared = ctx.same_ht and need_h and need_t and h_idx is not None and t_idx is not None
        gt = gh if shared else (torch.empty_like(t) if need_t else None)
        gr = torch.empty_like(r) if need_r else None
        ops.complex_bwd(gs.contiguous(), h, h_idx, t, t_idx, r, r_idx, ctx.batch, gh, gt, gr, zero_tables=True)
        return gh, None, (None if shared else gt), None, gr, None


class _ComplExBCEFunction(torch.autograd.Function):
    """``_DistMultBCEFunction`` with the ComplEx score: the scoring launch emits the per-sample loss, the mean and the
    step's bookkeeping are ``distmult_bce_reduce``'s (decoder-independent), and one backward call turns the gradient of
    the mean loss into the head / tail / relation gradients."""

    @staticmethod
    def forward(ctx, h, h_idx, t, t_idx, r, r_idx, labels, stats=None):
        h, t, r = h.contiguous(), t.contiguous(), r.contiguous()
        h_idx, t_idx, r_idx = (i.contiguous() if i is not None else None for i in (h_idx, t_idx, r_idx))
        labels = labels.contiguous()
        batch = (h_idx if h_idx is not None else h).size(0)
        scores, per_sample = ops.complex_bce_fwd(h, h_idx, t, t_idx, r, r_idx, labels, batch)
        ctx.batch = batch
        ctx.same_ht = h.data_ptr() == t.data_ptr() and h.shape == t.shape
        ctx.save_for_backward(h, h_idx, t, t_idx, r, r_idx, labels, scores)
        ctx.mark_non_differentiable(scores)
        ctx.set_materialize_grads(False)
        loss_sum, correct, cursor, cursor_add = stats if stats is not None else (None, None, None, 0)
        mean = ops.distmult_bce_reduce(per_sample, scores, labels, loss_sum, correct, cursor, cursor_add)
        return mean.reshape(()), scores

    @staticmethod
    def backward(ctx, g_loss, _g_scores):
        h, h_idx, t, t_idx, r, r_idx, labels, scores = ctx.saved_tensors
        need_h, _, need_t, _, need_r, _, _, _ = ctx.needs_input_grad
        if g_loss is None:                           # nothing downstream used the loss
            return (None,) * 8
        gh = torch.empty_like(h) if need_h else None
        shared = ctx.same_ht and need_h and need_t and h_idx is not None and t_idx is not None
        gt = gh if shared else (torch.empty_like(t) if need_t else None)
        gr = torch.empty_like(r) if need_r else None
        ops.complex_bce_bwd(g_loss.reshape(1).contiguous(), scores, labels, h, h_idx, t, t_idx, r, r_idx,
                            ctx.batch, gh, gt, gr, zero_tables=True)
        return gh, None, (None if shared else gt), None, gr, None, None, None


def complex_query_rows(x: Tensor, rel_rows: Tensor, side: str) -> Tensor:
    """``ops.complex_query`` on gathered rows, in torch ops - the differentiable form (``score_all_tails`` when a
    gradient is required); same grouping as the kernel"""
    m = x.size(1) // 2
    x_re, x_im, r_re, r_im = x[:, :m], x[:, m:], rel_rows[:, :m], rel_rows[:, m:]
    if side == "tail":
        return torch.cat([x_re * r_re - x_im * r_im, x_re * r_im + x_im * r_re], dim=1)
    return torch.cat([r_re * x_re + r_im * x_im, r_re * x_im - r_im * x_re], dim=1)


DECODERS = ("distmult", "complex")


def distmult(h, h_idx, t, t_idx, r, r_idx) -> Tensor:
    return _DistMultFunction.apply(h, h_idx, t, t_idx, r, r_idx)


def complex_score(h, h_idx, t, t_idx, r, r_idx) -> Tensor:
    return _ComplExFunction.apply(h, h_idx, t, t_idx, r, r_idx)


class LinkPredictor(nn.Module):
    """``decoder="distmult"`` (the default): ``score(h, r, t) = sum_d h_d * r_d * t_d``, symmetric in h and t.
    ``decoder="complex"``: ``score(h, r, t) = Re <h, r, conj(t)>`` over d / 2 complex numbers per row (real parts in
    columns [0, d / 2), imaginary parts behind them; d a multiple of 8), which is not: the tail enters conjugated, so
    the head side of every ranking call takes another query operand than the tail side.  Same parameter either way."""

    def __init__(self, num_relations: int, embedding_dim: int, dropout: float = 0.0, decoder: str = "distmult"):
        super().__init__()
        if decoder not in DECODERS:
            raise ValueError(f"decoder must be one of {DECODERS}, got {decoder!r}")
        if decoder == "complex" and embedding_dim % 8:
            raise ValueError("embedding dim must be a multiple of 8")
        self.decoder = decoder
        self.num_relations = num_relations
        self.embedding_dim = embedding_dim
        self.relation_embeddings = nn.Embedding(num_relations, embedding_dim)
        self.dropout = nn.Dropout(dropout)
        self._init_embeddings()

    def _init_embeddings(self) -> None:
        nn.init.xavier_uniform_(self.relation_embeddings.weight)

    def _relation_operand(self, relation_types: Tensor):
        """(matrix, index) for the relation factor.  With active dropout the reference
        drops the *gathered* [B, d] rows (rgcn.py:207-208), one mask per sample, so the
        gather + dropout stay torch ops and the kernel reads the dropped rows; otherwise the
        kernel gathers straight from the [R, d] table."""
        if self.training and self.dropout.p > 0:
            return self.dropout(_RelationRows.apply(self.relation_embeddings.weight, relation_types)), None
        return self.relation_embeddings.weight, relation_types

    def forward(self, head_embeddings: Tensor, tail_embeddings: Tensor,
                relation_types: Tensor) -> Tensor:
        r, r_idx = self._relation_operand(relation_types)
        score = complex_score if self.decoder == "complex" else distmult
        return score(head_embeddings, None, tail_embeddings, None, r, r_idx)

    def score_triples(self, node_embeddings: Tensor, head_indices: Tensor, tail_indices: Tensor,
                      relation_types: Tensor) -> Tensor:
        """``forward(node_embeddings[head], node_embeddings[tail], rel)`` without
        materialising the two [B, d] gathers."""
        r, r_idx = self._relation_operand(relation_types)
        score = complex_score if self.decoder == "complex" else distmult
        return score(node_embeddings, head_indices, node_embeddings, tail_indices, r, r_idx)

    def bce_loss(self, node_embeddings: Tensor, head_indices: Tensor, tail_indices: Tensor,
                 relation_types: Tensor, labels: Tensor, stats=None):
        """``(BCEWithLogitsLoss()(score_triples(...), labels), scores)`` as one fused node.  ``stats``: the caller's
        device-resident running sums and batch cursor ``(loss_sum, correct, cursor, cursor_add)``, updated by the launch
        that forms the mean (``Trainer``: ``src/train.py:321-326`` without nine elementwise launches per step)."""
        r, r_idx = self._relation_operand(relation_types)
        fn = _ComplExBCEFunction if self.decoder == "complex" else _DistMultBCEFunction
        return fn.apply(node_embeddings, head_indices, node_embeddings, tail_indices, r, r_idx, labels, stats)

    def _query(self, side: str, anchor_embeddings: Tensor, relation_types: Tensor) -> Tensor:
        """the query rows ``q`` with ``score = <q[b], E[n]>`` for the candidates of ``side``.  DistMult: ``anchor * rel`` on
        both sides.  ComplEx: ``ops.complex_query`` - on the head side the operand with the conjugate."""
        if self.decoder == "complex":
            return ops.complex_query(anchor_embeddings.contiguous(), None, self.relation_embeddings.weight,
                                     relation_types.contiguous(), side)
        return (anchor_embeddings * self.relation_embeddings(relation_types)).contiguous()

    @torch.no_grad()
    def rank_tails(self, head_embeddings: Tensor, relation_types: Tensor, all_tail_embeddings: Tensor,
                   tail_indices: Tensor, *, known: Optional["ops.KnownTriples"] = None,
                   head_indices: Optional[Tensor] = None, node_class: Optional[Tensor] = None,
                   max_mask_bytes: int = 256 << 20) -> Tensor:
        """1-based rank of ``tail_indices[b]`` among all entities for ``(head, relation)``:
        ``argsort(score_all_tails(...)[b], descending=True)`` position + 1, as
        ``evaluate.py:266-274`` computes it, but from one fused MFMA pass that counts the
        candidates beating the true tail's score (ties, measure zero in fp32, rank first).

        ``known`` (with ``head_indices``, the node ids of the heads): the filtered protocol - a candidate ``n`` with
        ``(head, relation, n)`` among the known triples does not count.  ``node_class`` (int ``[N]``): the
        type-constrained protocol - only candidates of the true tail's class count.  Both default to the raw
        protocol above, through the same kernel as before.

        Non-finite values: an eligible candidate (not the true tail, not known, of the asked class) counts unless its
        score is ``<=`` the true score.  On data without NaN that is the count above, infinities included.  A NaN
        candidate counts against every true score, as in the reference's argsort.  A NaN true score - a NaN in the true
        tail's row, in the head's row or in the relation's - is beaten by every eligible candidate: rank ``1 +
        #eligible``, raw that is ``N``, where the reference's argsort would put the missing value first.  A model whose
        table is all NaN ranks every triple last, never first."""
        hr = self._query("tail", head_embeddings, relation_types)
        emb = all_tail_embeddings.contiguous()
        true_score = (hr * emb[tail_indices]).sum(1)
        if known is None and node_class is None:
            return ops.distmult_rank_tails(hr, emb, true_score, tail_indices.contiguous())
        return self._rank_filtered("tail", hr, emb, true_score, tail_indices.contiguous(), relation_types, known,
                                   head_indices, node_class, max_mask_bytes)

    @torch.no_grad()
    def rank_heads(self, tail_embeddings: Tensor, relation_types: Tensor, all_head_embeddings: Tensor,
                   head_indices: Tensor, *, known: Optional["ops.KnownTriples"] = None,
                   tail_indices: Optional[Tensor] = None, node_class: Optional[Tensor] = None,
                   max_mask_bytes: int = 256 << 20) -> Tensor:
        """1-based rank of ``head_indices[b]`` among all entities for ``(?, relation, tail)``.  DistMult is symmetric
        in head and tail, so this is ``rank_tails``'s pass with ``q = tail * rel``.  ComplEx is not: the query operand is
        ``q = [r_re t_re + r_im t_im | r_re t_im - r_im t_re]``, the tail rotated by the CONJUGATE of the relation
        (``ops.complex_query(side="head")``), so that ``score(n, r, t) = <q, E[n]>``.  ``known`` filters by the
        ``(tail, relation)`` sets (``tail_indices``: the node ids of the tails), ``node_class`` restricts the
        candidates to the true head's class.  Non-finite values as in ``rank_tails``: an eligible candidate counts
        unless its score is ``<=`` the true score, so a NaN candidate counts against every query and a NaN true score
        ranks ``1 + #eligible``."""
        tr = self._query("head", tail_embeddings, relation_types)
        emb = all_head_embeddings.contiguous()
        true_score = (tr * emb[head_indices]).sum(1)
        return self._rank_filtered("head", tr, emb, true_score, head_indices.contiguous(), relation_types, known,
                                   tail_indices, node_class, max_mask_bytes)

    def _allow_rows(self, node_class, emb):
        """``(node_class int32 [N] on the device, allow [C, W])``: the allow rows of a class vector, built once and kept
        while the caller passes the same, unmodified tensor"""
        if node_class.shape != (emb.size(0),):
            raise ValueError(f"node_class must hold one class per entity ([{emb.size(0)}])")
        key = (node_class.data_ptr(), node_class._version, node_class.dtype, emb.device)
        if getattr(self, "_allow_cache", (None,))[0] != key:
            classes = node_class.to(device=emb.device, dtype=torch.int32).contiguous()
            self._allow_cache = (key, node_class, classes, ops.class_allow_bits(classes, int(classes.max()) + 1))
        return self._allow_cache[2], self._allow_cache[3]

    def _rank_filtered(self, side, q, emb, true_score, target, relation_types, known, anchor_indices, node_class,
                       max_mask_bytes):
        allow = query_class = None
        if node_class is not None:
            node_class, allow = self._allow_rows(node_class, emb)
            query_class = node_class[target].contiguous()
        if known is not None and anchor_indices is None:
            raise ValueError("filtered ranking needs the node ids of the given side "
                             "(head_indices for rank_tails, tail_indices for rank_heads)")
        return ops.distmult_rank_filtered(q, emb, true_score, target, known, side, anchor_indices, relation_types,
                                          allow, query_class, max_mask_bytes)

    @torch.no_grad()
    def top_tails(self, head_embeddings: Tensor, relation_types: Tensor, all_tail_embeddings: Tensor, k: int, *,
                  known: Optional["ops.KnownTriples"] = None, head_indices: Optional[Tensor] = None,
                  node_class: Optional[Tensor] = None, candidate_class=None, min_score: Optional[float] = None,
                  max_mask_bytes: int = 256 << 20):
        """The ``k`` best tails of every ``(head, relation)`` query: ``(ids int64 [B, k], scores [B, k])``, scores
        descending, equal scores by id ascending, id -1 / score -inf past the number of candidates - the first ``k``
        columns of a stable descending sort of ``score_all_tails(...)`` restricted to the candidates, from one fused
        pass that never stores the matrix (``case_studies.predict_top_drugs``, ``medical_validation.generate_predictions``).

        ``known`` (with ``head_indices``): only novel tails - no ``n`` with ``(head, relation, n)`` among the known
        triples.  ``node_class`` (int ``[N]``) with ``candidate_class`` (an int, or an int ``[B]`` tensor): only tails
        of that class ("drugs").  ``min_score``: only scores ``>=`` it."""
        hr = self._query("tail", head_embeddings, relation_types)
        return self._top_filtered("tail", hr, all_tail_embeddings.contiguous(), k, relation_types, known, head_indices,
                                  node_class, candidate_class, min_score, max_mask_bytes)

    @torch.no_grad()
    def top_heads(self, tail_embeddings: Tensor, relation_types: Tensor, all_head_embeddings: Tensor, k: int, *,
                  known: Optional["ops.KnownTriples"] = None, tail_indices: Optional[Tensor] = None,
                  node_class: Optional[Tensor] = None, candidate_class=None, min_score: Optional[float] = None,
                  max_mask_bytes: int = 256 << 20):
        """The ``k`` best heads of every ``(?, relation, tail)`` query.  DistMult is symmetric in head and tail, so
        this is ``top_tails``'s pass with ``q = tail * rel``; ComplEx takes the conjugate operand of ``rank_heads``.
        ``known`` filters by the ``(tail, relation)`` sets."""
        tr = self._query("head", tail_embeddings, relation_types)
        return self._top_filtered("head", tr, all_head_embeddings.contiguous(), k, relation_types, known, tail_indices,
                                  node_class, candidate_class, min_score, max_mask_bytes)

    def _top_filtered(self, side, q, emb, k, relation_types, known, anchor_indices, node_class, candidate_class,
                      min_score, max_mask_bytes):
        allow = query_class = None
        if (node_class is None) != (candidate_class is None):
            raise ValueError("node_class (the class of every entity) and candidate_class (the class the answers must "
                             "have) go together")
        if node_class is not None:
            _, allow = self._allow_rows(node_class, emb)
            if isinstance(candidate_class, Tensor):
                if candidate_class.shape != (q.size(0),):
                    raise ValueError(f"candidate_class must be an int or hold one class per query ([{q.size(0)}])")
                query_class = candidate_class.to(device=emb.device, dtype=torch.int32).contiguous()
            else:
                query_class = torch.full((q.size(0),), int(candidate_class), dtype=torch.int32, device=emb.device)
        if known is not None and anchor_indices is None:
            raise ValueError("novel candidates need the node ids of the given side "
                             "(head_indices for top_tails, tail_indices for top_heads)")
        return ops.distmult_topk_filtered(q, emb, k, known, side, anchor_indices, relation_types, allow, query_class,
                                          min_score, max_mask_bytes)

    def score_all_tails(self, head_embeddings: Tensor, relation_types: Tensor,
                        all_tail_embeddings: Tensor) -> Tensor:
        """``(h * r) @ E^T`` -> [B, num_entities] (rgcn.py:215-243): the ranking kernel's GEMM with a store
        epilogue (``distmult_score_all_tails``), so ``score_all_tails(...)[b, n]`` and the score ``rank_tails``
        compares are the same bits.  Differentiable like the reference's expression.  An embedding width that is not a
        multiple of the kernel's 32-wide k step (the reference's is 128) takes the library GEMM on the GPU.

        ComplEx: the same kernel on the query rows ``q`` (``ops.complex_query``, or torch ops when a gradient is
        required) with a one-row relation table of ones - ``x * 1.0f`` is exact, so the entries, the scores the ranking
        pass compares and the scores the top-k pass lists are the same bits."""
        if self.decoder == "complex":
            needs_grad = torch.is_grad_enabled() and (head_embeddings.requires_grad or all_tail_embeddings.requires_grad
                                                      or self.relation_embeddings.weight.requires_grad)
            if needs_grad or not head_embeddings.is_cuda:
                q = complex_query_rows(head_embeddings, self.relation_embeddings(relation_types), "tail")
            else:
                q = self._query("tail", head_embeddings, relation_types)
            if q.size(1) % 32 and q.is_cuda:
                return q @ all_tail_embeddings.t()
            ones = torch.ones(1, q.size(1), dtype=q.dtype, device=q.device)
            zero = torch.zeros(q.size(0), dtype=torch.int64, device=q.device)
            return _ScoreAllTailsFunction.apply(q, ones, zero, all_tail_embeddings)
        if head_embeddings.size(1) % 32 and head_embeddings.is_cuda:
            return (head_embeddings * self.relation_embeddings(relation_types)) @ all_tail_embeddings.t()
        return _ScoreAllTailsFunction.apply(head_embeddings, self.relation_embeddings.weight, relation_types,
                                            all_tail_embeddings)
