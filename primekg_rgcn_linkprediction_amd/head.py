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


def _head_op(decoder: str, call: str):
    """the ``ops`` entry of a decoder of ``DECODERS``: ``ops.distmult_fwd``, ``ops.complex_bce_bwd``, ..."""
    return getattr(ops, f"{decoder}_{call}")


def _operands(h, h_idx, t, t_idx, r, r_idx):
    """-> the six operands contiguous, the batch, and whether head and tail are gathered from one table"""
    h, t, r = h.contiguous(), t.contiguous(), r.contiguous()
    h_idx, t_idx, r_idx = (i.contiguous() if i is not None else None for i in (h_idx, t_idx, r_idx))
    batch = (h_idx if h_idx is not None else h).size(0)
    return (h, h_idx, t, t_idx, r, r_idx), batch, h.data_ptr() == t.data_ptr() and h.shape == t.shape


def _grad_buffers(same_ht, h, h_idx, t, t_idx, r, need_h, need_t, need_r):
    """-> (grad_h, grad_t, grad_r, shared) for a head's backward, uninitialised (an indexed table is cleared by the
    backward's first launch).  ``shared``: head and tail gathered from one table accumulate into one buffer, and since
    autograd sums the two returned grads of the same leaf, the caller hands back the whole accumulation once and an
    untouched None for the tail's slot."""
    gh = torch.empty_like(h) if need_h else None
    shared = same_ht and need_h and need_t and h_idx is not None and t_idx is not None
    gt = gh if shared else (torch.empty_like(t) if need_t else None)
    gr = torch.empty_like(r) if need_r else None
    return gh, gt, gr, shared


class _ScoreFunction(torch.autograd.Function):
    """The score of ``decoder`` (a name of ``DECODERS``, not a tensor: its gradient slot is None); an index of None
    means row b.  DistMult: scores[b] = sum_d H[hi(b)] * Rm[ri(b)] * T[ti(b)]; ComplEx:
    scores[b] = Re <H[hi(b)], Rm[ri(b)], conj(T[ti(b)])>."""

    @staticmethod
    def forward(ctx, decoder: str, h: Tensor, h_idx: Optional[Tensor], t: Tensor, t_idx: Optional[Tensor],
                r: Tensor, r_idx: Optional[Tensor]) -> Tensor:
        operands, batch, same_ht = _operands(h, h_idx, t, t_idx, r, r_idx)
        scores = _head_op(decoder, "fwd")(*operands, batch)
        ctx.decoder, ctx.batch, ctx.same_ht = decoder, batch, same_ht
        ctx.save_for_backward(*operands)
        return scores

    @staticmethod
    def backward(ctx, gs: Tensor):
        h, h_idx, t, t_idx, r, r_idx = ctx.saved_tensors
        _, need_h, _, need_t, _, need_r, _ = ctx.needs_input_grad
        gh, gt, gr, shared = _grad_buffers(ctx.same_ht, h, h_idx, t, t_idx, r, need_h, need_t, need_r)
        _head_op(ctx.decoder, "bwd")(gs.contiguous(), h, h_idx, t, t_idx, r, r_idx, ctx.batch, gh, gt, gr, zero_tables=True)
        return None, gh, None, (None if shared else gt), None, gr, None


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


class _ScoreBCEFunction(torch.autograd.Function):
    """(mean binary_cross_entropy_with_logits(scores, labels), scores) of ``decoder``: the scoring kernel also
    emits the per-sample loss, and ONE backward call turns the gradient of the mean loss into
    the head / tail / relation gradients (sigmoid, subtraction, 1/B and the decoder's products
    fused) - instead of the eight elementwise launches of BCEWithLogitsLoss around the head
    (``src/train.py:300``).  The mean and the step's bookkeeping are ``distmult_bce_reduce``'s (decoder-independent).
    ``scores`` is returned for the accuracy bookkeeping only."""

    @staticmethod
    def forward(ctx, decoder, h, h_idx, t, t_idx, r, r_idx, labels, stats=None):
        operands, batch, same_ht = _operands(h, h_idx, t, t_idx, r, r_idx)
        labels = labels.contiguous()
        scores, per_sample = _head_op(decoder, "bce_fwd")(*operands, labels, batch)
        ctx.decoder, ctx.batch, ctx.same_ht = decoder, batch, same_ht
        ctx.save_for_backward(*operands, labels, scores)
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
        _, need_h, _, need_t, _, need_r, _, _, _ = ctx.needs_input_grad
        if g_loss is None:                           # nothing downstream used the loss
            return (None,) * 9
        gh, gt, gr, shared = _grad_buffers(ctx.same_ht, h, h_idx, t, t_idx, r, need_h, need_t, need_r)
        _head_op(ctx.decoder, "bce_bwd")(g_loss.reshape(1).contiguous(), scores, labels, h, h_idx, t, t_idx, r, r_idx,
                                         ctx.batch, gh, gt, gr, zero_tables=True)
        return None, gh, None, (None if shared else gt), None, gr, None, None, None


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


class _SoftmaxLossFunction(torch.autograd.Function):
    """Per-sample 1-vs-all softmax loss of one side, ``(loss [B], hit [B])``: ``loss[b] = logsumexp over the eligible
    candidates of <q[b], E[n]>`` minus the target's score (``ops.softmax_lse_filtered``: no ``[B, N]`` matrix), with the
    query rows of the decoder - ``anchor * rel`` (DistMult) or ``ops.complex_query`` (ComplEx; the head side carries the
    conjugate).  The backward is ``ops.softmax_grad_filtered``: ``demb`` is the candidates' share of the gradient of the
    node embeddings, and ``dq`` goes through the query by the backward entry points that exist - the query is the
    score's gradient with respect to the free end, so ``sum_b <q(x_b, r_b), dq_b>`` is the decoder's score with ``dq``
    as an un-indexed operand and ``grad_scores = 1``: ``distmult_bwd`` / ``complex_bwd`` with that operand's gradient
    left out scatter ``r o dq`` into the anchors' rows and ``x o dq`` into the relations' in their deterministic
    sample order.  ``r_idx`` None: ``r`` holds one (dropped-out) relation row per sample."""

    @staticmethod
    def forward(ctx, emb, r, r_idx, rel_ids, anchor_idx, target_idx, decoder, side, known, allow, query_class,
                max_mask_bytes):
        emb, r = emb.contiguous(), r.contiguous()
        anchor_idx, target_idx = anchor_idx.contiguous(), target_idx.contiguous()
        r_idx = r_idx.contiguous() if r_idx is not None else None
        if decoder == "complex":
            q = ops.complex_query(emb, anchor_idx, r, r_idx, side)
        else:
            q = (emb[anchor_idx] * (r[r_idx] if r_idx is not None else r)).contiguous()
        rel_ids = rel_ids.contiguous()                         # the samples' relations: what the known triples are keyed by
        lse, _, _, loss, hit = ops.softmax_lse_filtered(q, emb, target_idx, known, side, anchor_idx, rel_ids, allow,
                                                        query_class, max_mask_bytes)
        ctx.save_for_backward(emb, r, r_idx, rel_ids, anchor_idx, target_idx, q, lse, allow, query_class)
        ctx.decoder, ctx.side, ctx.known, ctx.max_mask_bytes = decoder, side, known, max_mask_bytes
        ctx.mark_non_differentiable(hit)
        ctx.set_materialize_grads(False)
        return loss, hit

    @staticmethod
    def backward(ctx, g, _g_hit):
        emb, r, r_idx, rel_ids, anchor_idx, target_idx, q, lse, allow, query_class = ctx.saved_tensors
        need_emb, need_r = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g is None or not (need_emb or need_r):
            return (None,) * 12
        batch = anchor_idx.size(0)
        dq, demb = ops.softmax_grad_filtered(g.contiguous(), q, emb, target_idx, lse, ctx.known, ctx.side, anchor_idx,
                                             rel_ids, allow, query_class, ctx.max_mask_bytes, need_dq=True,
                                             need_demb=need_emb)
        ones = torch.ones(batch, dtype=torch.float32, device=emb.device)
        gx = torch.empty_like(emb) if need_emb else None         # the anchors' rows; cleared by the backward's first launch
        gr = torch.empty_like(r) if need_r else None
        if ctx.decoder == "complex" and ctx.side == "head":
            ops.complex_bwd(ones, dq, None, emb, anchor_idx, r, r_idx, batch, None, gx, gr, zero_tables=True)
        elif ctx.decoder == "complex":
            ops.complex_bwd(ones, emb, anchor_idx, dq, None, r, r_idx, batch, gx, None, gr, zero_tables=True)
        else:
            ops.distmult_bwd(ones, emb, anchor_idx, dq, None, r, r_idx, batch, gx, None, gr, zero_tables=True)
        if need_emb:
            demb.add_(gx)
        return (demb, gr) + (None,) * 10


def complex_query_rows(x: Tensor, rel_rows: Tensor, side: str) -> Tensor:
    """``ops.complex_query`` on gathered rows, in torch ops - the differentiable form (``score_all_tails`` when a
    gradient is required); same grouping as the kernel"""
    m = x.size(1) // 2
    x_re, x_im, r_re, r_im = x[:, :m], x[:, m:], rel_rows[:, :m], rel_rows[:, m:]
    if side == "tail":
        return torch.cat([x_re * r_re - x_im * r_im, x_re * r_im + x_im * r_re], dim=1)
    return torch.cat([r_re * x_re + r_im * x_im, r_re * x_im - r_im * x_re], dim=1)


def known_mask(known, side: str, anchor_idx: Tensor, rel_idx: Tensor) -> Tensor:
    """bool ``[B, N]``: entry ``(b, n)`` set iff ``(anchor[b], relation[b], n)`` is a known triple of ``side`` - the dense
    form of ``KnownTriples.exclude_bits``, in torch ops on whatever device the structure is on"""
    keys, ptr, ids = known.csr(side)
    seg = known.segments(side, anchor_idx.to(keys.device), rel_idx.to(keys.device))
    mask = torch.zeros(seg.numel(), known.num_nodes, dtype=torch.bool, device=keys.device)
    for b in torch.nonzero(seg >= 0).view(-1).tolist():
        mask[b, ids[int(ptr[seg[b]]):int(ptr[seg[b] + 1])]] = True
    return mask.to(anchor_idx.device)


DECODERS = ("distmult", "complex")


def distmult(h, h_idx, t, t_idx, r, r_idx) -> Tensor:
    return _ScoreFunction.apply("distmult", h, h_idx, t, t_idx, r, r_idx)


def complex_score(h, h_idx, t, t_idx, r, r_idx) -> Tensor:
    return _ScoreFunction.apply("complex", h, h_idx, t, t_idx, r, r_idx)


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
        return _ScoreBCEFunction.apply(self.decoder, node_embeddings, head_indices, node_embeddings, tail_indices, r, r_idx,
                                       labels, stats)

    def softmax_loss(self, node_embeddings: Tensor, head_indices: Tensor, tail_indices: Tensor,
                     relation_types: Tensor, *, sides=("tail", "head"), known: Optional["ops.KnownTriples"] = None,
                     node_class: Optional[Tensor] = None, stats=None, max_mask_bytes: int = 256 << 20):
        """``(mean loss, hits)``: the 1-vs-all softmax cross-entropy of the true entity against EVERY candidate - what
        ``rank_tails`` / ``rank_heads`` ask afterwards, as a loss.  Per side of ``sides`` (``"tail"``: the tails of
        ``(head, relation, ?)`` with the true tail as target; ``"head"``: the heads of ``(?, relation, tail)``) and
        sample, ``loss = logsumexp over the eligible candidates of score - score of the target``; the mean is over sides
        and samples, ``hits`` (int64 scalar) counts the samples whose target is a best eligible candidate.  Eligible: every
        entity, minus - with ``known`` - the other known answers of the query (the filtered protocol), restricted - with
        ``node_class`` (int ``[N]``) - to the target's class (the type-constrained protocol); the target itself always.
        ``stats``: ``(loss_sum, correct)`` device tensors the step's sums are added to.

        On the GPU this is one fused pass per side that never stores the ``[B, N]`` scores (``ops.softmax_lse``) and a
        backward that recomputes them (``ops.softmax_grad``).  On CPU tensors it is the torch expression below, which is
        the specification."""
        if isinstance(sides, str):
            sides = (sides,)
        if not sides or any(s not in ("tail", "head") for s in sides):
            raise ValueError("sides must name 'tail', 'head' or both")
        if not node_embeddings.is_cuda:
            losses, hits = zip(*(self._softmax_loss_torch(node_embeddings, head_indices, tail_indices, relation_types, s,
                                                          known, node_class) for s in sides))
        else:
            r, r_idx = self._relation_operand(relation_types)
            allow = cls = None
            if node_class is not None:
                cls, allow = self._allow_rows(node_class, node_embeddings)
            losses, hits = [], []
            for s in sides:
                anchor, target = (head_indices, tail_indices) if s == "tail" else (tail_indices, head_indices)
                query_class = cls[target].contiguous() if cls is not None else None
                loss, hit = _SoftmaxLossFunction.apply(node_embeddings, r, r_idx, relation_types, anchor, target, self.decoder, s, known,
                                                       allow, query_class, max_mask_bytes)
                losses.append(loss)
                hits.append(hit)
        loss = torch.cat(losses).mean()
        hit_count = torch.cat([h.reshape(-1) for h in hits]).to(torch.int64).sum()
        if stats is not None:
            with torch.no_grad():
                stats[0].add_(torch.cat(losses).sum().to(stats[0].dtype))
                stats[1].add_(hit_count.to(stats[1].dtype))
        return loss, hit_count

    def _softmax_loss_torch(self, emb, head_indices, tail_indices, relation_types, side, known, node_class):
        """the specification of one side: ``(loss [B], hit [B])`` in torch ops, any dtype, differentiable"""
        anchor, target = (head_indices, tail_indices) if side == "tail" else (tail_indices, head_indices)
        r, r_idx = self._relation_operand(relation_types)
        rel_rows = (r[r_idx] if r_idx is not None else r).to(emb.dtype)
        x = emb[anchor]
        q = complex_query_rows(x, rel_rows, side) if self.decoder == "complex" else x * rel_rows
        scores = q @ emb.t()                                                     # [B, N]
        b, n = scores.shape
        rows = torch.arange(b, device=emb.device)
        eligible = torch.ones(b, n, dtype=torch.bool, device=emb.device)
        if node_class is not None:
            cls = node_class.to(emb.device)
            eligible &= (cls[None, :] == cls[target][:, None]) & (cls[target] >= 0)[:, None]
        if known is not None:
            eligible &= ~known_mask(known, side, anchor, relation_types)
        eligible[rows, target] = True                                            # the target always counts
        masked = scores.masked_fill(~eligible, float("-inf"))
        true_score = scores[rows, target]
        loss = torch.logsumexp(masked, dim=1) - true_score
        return loss, true_score >= masked.max(dim=1).values

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
