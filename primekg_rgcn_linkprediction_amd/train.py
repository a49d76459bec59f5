"""Training harness around the HIP path (SURVEY.md section 8f "next" row 1).

Counterpart of the reference's ``src/train.py``: same command-line flags and defaults
(``train.py:635-770``), same on-disk dict format (``train.py:563-567``) and host-side range
filter (``train.py:571-586``), same sampler semantics (``train.py:59-97``), same step
(positives + negatives -> ``model(train graph, heads, tails, rels)`` -> BCE-with-logits ->
backward -> clip-grad-norm -> Adam; ``train.py:276-318``) and the same validation protocol on the
full graph (``train.py:389-395``), so a reference user can run

    python -m primekg_rgcn_linkprediction_amd.train --data_dir data/processed --epochs 100

and get checkpoints with the reference's keys (``train.py:431-442``).  What differs, on
purpose: the model is this package's ``DrugDiseaseModel`` (HIP kernels); the running loss /
accuracy are accumulated on the device and read back once per epoch instead of two ``.item()``
host syncs per step (``train.py:322,325``); a mini-batch (slice of the shuffled columns,
negatives, labels) is assembled by one kernel (``--torch_sampler`` restores the reference's
``torch.rand`` / ``torch.randint`` sequence); BCE-with-logits is fused into the head kernels;
gradient clipping + the Adam/AdamW update are two launches on the optimizer's own state
(``--torch_optimizer`` keeps torch's kernels); and the whole step is one captured HIP graph
replayed per batch (``--no_hip_graph`` launches it eagerly).  Same update rule throughout.

``--synthetic`` builds a PrimeKG-shaped random graph instead of loading ``--data_dir`` (the
reference's ``train_data.pt`` / ``full_graph.pt`` blobs are not in its mount).
"""
from __future__ import annotations

import argparse
import logging
import time
from pathlib import Path
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .model import DrugDiseaseModel

logger = logging.getLogger("primekg_rgcn_linkprediction_amd.train")


class NegativeSampler:
    """Corrupt the head or the tail (fair coin per sample) of each positive triple with a
    uniformly random node.  Draw order matches the reference (one ``torch.rand`` for the coin,
    then one ``torch.randint`` for the replacement entity), so a seeded run consumes the RNG
    stream identically (fixture ``tests/golden/ref_negative_sampler.npz``)."""

    def __init__(self, num_nodes: int, num_neg_samples: int = 1):
        self.num_nodes = num_nodes
        self.num_neg_samples = num_neg_samples

    def sample(self, pos_head: torch.Tensor, pos_tail: torch.Tensor,
               pos_rel: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        k = self.num_neg_samples
        head, tail, rel = (t.repeat_interleave(k) for t in (pos_head, pos_tail, pos_rel))
        total = head.numel()
        flip_head = torch.rand(total, device=head.device) < 0.5
        entity = torch.randint(0, self.num_nodes, (total,), device=head.device)
        return torch.where(flip_head, entity, head), torch.where(flip_head, tail, entity), rel


# Philox stream (the "epoch" word of the device sampler's counter) of validate()'s negatives under a constraint: no
# training epoch gets there, and it is below the sampler's 2^56 limit
VALIDATION_STREAM = 1 << 55


def group_has_extras(optimizer: torch.optim.Optimizer) -> bool:
    """options of torch's Adam the two-launch update does not implement"""
    g = optimizer.param_groups
    return len(g) != 1 or bool(g[0].get("amsgrad")) or bool(g[0].get("maximize")) or len(g[0]["params"]) > 32


class Trainer:
    """Epoch loop, validation and checkpoints; attribute names follow the reference's
    ``Trainer`` so that scripts poking at ``trainer.train_losses`` etc. keep working."""

    def __init__(self, model: DrugDiseaseModel, train_data: Dict, val_data: Dict, full_graph: Dict,
                 device: torch.device, args: argparse.Namespace):
        # negatives under the evaluation protocol (off by default): filtered against the known triples and / or drawn
        # from the class of the node they replace, by the constrained device sampler - there is no other path to them
        self.filtered_negatives = bool(getattr(args, "filtered_negatives", False))
        self.type_constrained_negatives = bool(getattr(args, "type_constrained_negatives", False))
        # --loss softmax: the 1-vs-all softmax cross-entropy of the true entity against every candidate; no negatives are
        # sampled, and the two protocol switches choose the denominator's candidates instead of the sampler's draws
        self.softmax = getattr(args, "loss", "bce") == "softmax"
        self.softmax_sides = ("tail",) if getattr(args, "softmax_sides", "both") == "tail" else ("tail", "head")
        if self.softmax:
            if getattr(args, "num_neg_samples", 1) != 1:
                raise ValueError("--loss softmax scores every entity against the true one and samples no negatives: "
                                 "--num_neg_samples has no meaning with it, leave it at 1")
            if getattr(args, "torch_sampler", False):
                raise ValueError("--loss softmax draws no negatives, so there is no sampler to choose: drop --torch_sampler")
            if self.type_constrained_negatives and not getattr(args, "node_types", None):
                raise ValueError("--type_constrained_negatives needs --node_types PATH (mappings.pt, or an .npz / .pt "
                                 "int vector [num_nodes])")
        self.constrained_negatives = (self.filtered_negatives or self.type_constrained_negatives) and not self.softmax
        if self.constrained_negatives:
            if getattr(args, "torch_sampler", False):
                raise ValueError("--filtered_negatives / --type_constrained_negatives need the device sampler: drop --torch_sampler")
            if device.type != "cuda":
                raise ValueError("--filtered_negatives / --type_constrained_negatives run on the GPU only (no CPU sampler)")
            if self.type_constrained_negatives and not getattr(args, "node_types", None):
                raise ValueError("--type_constrained_negatives needs --node_types PATH (mappings.pt, or an .npz / .pt "
                                 "int vector [num_nodes])")
            if not 1 <= int(getattr(args, "negative_tries", 8)) <= 16:
                raise ValueError("--negative_tries must be in 1..16")
        # --edge_dropout P / --hide_batch_edges (both off by default): per step, on the device, every train edge is
        # dropped from the message-passing graph with probability P and / or the batch's own columns are hidden from it, so
        # that a positive is not an edge the encoder has just averaged into both of its endpoints (ops.EdgeDropout)
        self.edge_dropout_p = float(getattr(args, "edge_dropout", 0.0) or 0.0)
        self.hide_batch_edges = bool(getattr(args, "hide_batch_edges", False))
        # --hide_reverse_edges / --paired_edge_dropout: data that stores a pair as two columns, (h, r, t) and (t, r, h),
        # hides and drops the two together (the twin map of rgcn_edge_dropout.h)
        self.hide_reverse_edges = bool(getattr(args, "hide_reverse_edges", False))
        self.paired_edge_dropout = bool(getattr(args, "paired_edge_dropout", False))
        if self.hide_reverse_edges and not self.hide_batch_edges:
            raise ValueError("--hide_reverse_edges hides the reverse columns of the batch's own: it needs --hide_batch_edges")
        if self.paired_edge_dropout and not self.edge_dropout_p > 0.0:
            raise ValueError("--paired_edge_dropout draws one word per pair of columns: it needs --edge_dropout P with P > 0")
        # --attention (off by default): both layers weigh a (node, relation) segment's in-edges by a learned segment softmax
        # (attention.py).  Each layer draws into a view of its own, so the trainer holds none; the hidden window of
        # --hide_batch_edges goes to both layers' draws through the encoder.  The slot of the draw's p carries the slope.
        self.attention = bool(getattr(args, "attention", False))
        if self.attention:
            if self.edge_dropout_p > 0.0:
                raise ValueError("--attention and --edge_dropout P > 0 do not combine: the draw that writes the attention "
                                 "weights takes the negative slope where the dropout draw takes P")
            if getattr(args, "fp16_gather", False):
                raise ValueError("--attention reads an fp32 feature table: drop --fp16_gather")
            if not getattr(getattr(model, "encoder", None), "attention", False):
                raise ValueError("--attention needs a model built with attention=True (train.create_model does it)")
            if device.type != "cuda":
                raise ValueError("--attention runs on the GPU only (the attention weights are written by a device kernel)")
        self._edge_dropout = self._ed_stats = self._ed_position = None
        self.edge_dropout_stats = (0, 0)       # (kept edges, hidden edges) summed over the steps of the last training epoch
        self._ed_steps = 0                     # steps of that epoch: kept fraction = kept / (steps * train columns)
        if self.edge_dropout_p or self.hide_batch_edges:
            if not 0.0 <= self.edge_dropout_p < 1.0:
                raise ValueError(f"--edge_dropout must be in [0, 1), got {self.edge_dropout_p}")
            if device.type != "cuda":
                raise ValueError("--edge_dropout / --hide_batch_edges run on the GPU only (the draw is a device kernel)")
            from .model import DrugDiseaseRGCN
            if not isinstance(getattr(model, "encoder", None), DrugDiseaseRGCN):
                raise ValueError("--edge_dropout / --hide_batch_edges need the single-GPU encoder (DrugDiseaseRGCN): the "
                                 "partitioned and replicated encoders of dist.py hold shard structures, which have no view")
        self.model = model.to(device)
        self.device, self.args = device, args
        self.train_data, self.val_data, self.full_graph = train_data, val_data, full_graph
        # the three graphs live on the device for the whole run; each is bucketed once
        self.train_edge_index = train_data["edge_index"].to(device)
        self.train_edge_type = train_data["edge_type"].to(device)
        self.val_edge_index = val_data["edge_index"].to(device)
        self.val_edge_type = val_data["edge_type"].to(device)
        self.full_edge_index = full_graph["edge_index"].to(device)
        self.full_edge_type = full_graph["edge_type"].to(device)
        if device.type == "cuda":      # bucket now (or import the persisted structure, --bucket_cache)
            from . import ops
            for d, ei, et in ((train_data, self.train_edge_index, self.train_edge_type),
                              (full_graph, self.full_edge_index, self.full_edge_type)):
                ops.bucket(ei, et, d["num_nodes"], d["num_relations"], sidecar=d.get("sidecar"))
        if self.attention:
            if self.hide_batch_edges:
                self._ed_stats = torch.zeros(2, dtype=torch.int64, device=device)
        elif self.edge_dropout_p or self.hide_batch_edges:
            self._edge_dropout = ops.EdgeDropout(ops.bucket(self.train_edge_index, self.train_edge_type,
                                                            train_data["num_nodes"], train_data["num_relations"]))
            self._ed_stats = torch.zeros(2, dtype=torch.int64, device=device)
        opt = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW}.get(args.optimizer)
        if opt is None:
            raise ValueError(f"Unknown optimizer: {args.optimizer}")
        # whole-step HIP graph (sampler -> encoder -> head -> BCE -> backward -> clip -> Adam ->
        # running metrics) for the full-size batches of an epoch; needs a device-side Adam step count
        self.use_hip_graph = (device.type == "cuda" and not getattr(args, "no_hip_graph", False)
                              and max(1, getattr(args, "gradient_accumulation_steps", 1)) == 1 and not self.softmax
                              and not self.attention)
        if self.attention:
            logger.info("--attention (slope %g): every step runs eagerly - the layer's backward forms the attention "
                        "gradients with torch ops that have never been captured into a HIP graph",
                        float(getattr(args, "attention_slope", 0.2)))
        # on the GPU: the single-kernel update (same rule; the default one runs ~10 list kernels
        # per step, ~125 us here), with its step count on the device when the step is captured
        extra = {"fused": True, "capturable": self.use_hip_graph} if device.type == "cuda" else {}
        self.optimizer = opt(self.model.parameters(), lr=args.lr, weight_decay=args.weight_decay, **extra)
        self._graph = self._loss_sum = None
        self._grad_seed = {}
        # clip + Adam(W) as two launches of this package instead of ~14 of torch's
        self.fused_update = (device.type == "cuda" and not getattr(args, "torch_optimizer", False)
                             and not group_has_extras(self.optimizer))
        # mini-batch assembly (slice + negatives + labels) as one kernel; --torch_sampler keeps the
        # reference's op-by-op sampler on torch's RNG stream
        self.device_sampler = device.type == "cuda" and not getattr(args, "torch_sampler", False)
        self.criterion = nn.BCEWithLogitsLoss()
        self.neg_sampler = NegativeSampler(train_data["num_nodes"], args.num_neg_samples)
        self._neg_classes = self._neg_known = self._neg_known_full = self._neg_stats = None
        self.negative_stats = (0, 0)       # (rejected draws, negatives that gave up) of the last training epoch
        if self.constrained_negatives:
            n, r = train_data["num_nodes"], train_data["num_relations"]
            self.negative_tries = int(getattr(args, "negative_tries", 8))
            if self.type_constrained_negatives:
                from .evaluate import load_node_classes
                class_of = load_node_classes(args.node_types, n)
                self._neg_classes = ops.NodeClasses(class_of.to(device), max(int(class_of.max()) + 1, 1))
            if self.filtered_negatives:
                # what training may know: the train graph - not the validation or test triples (no leakage);
                # validate() scores over the full graph and filters against it
                self._neg_known = ops.KnownTriples(self.train_edge_index, self.train_edge_type, n, r)
                self._neg_known_full = ops.KnownTriples(self.full_edge_index, self.full_edge_type, n, r)
            self._neg_stats = torch.zeros(2, dtype=torch.int64, device=device)
        self._sm_known = self._sm_known_full = self._sm_node_class = None
        if self.softmax:
            from . import ops
            n, r = train_data["num_nodes"], train_data["num_relations"]
            logger.info("--loss softmax (%s): every step runs eagerly - the mask chunking and the known-triple lookup are "
                        "torch ops that have never been captured into a HIP graph", " + ".join(self.softmax_sides))
            if self.type_constrained_negatives:
                from .evaluate import load_node_classes
                self._sm_node_class = load_node_classes(args.node_types, n).to(device)
            if self.filtered_negatives:
                # what training may know: the train graph; validate() scores over the full graph and filters against it
                self._sm_known = ops.KnownTriples(self.train_edge_index, self.train_edge_type, n, r)
                self._sm_known_full = ops.KnownTriples(self.full_edge_index, self.full_edge_type, n, r)
        self.best_val_loss, self.best_val_acc = float("inf"), 0.0
        self.train_losses, self.val_losses, self.train_accs, self.val_accs = [], [], [], []
        self.output_dir = Path(args.output_dir)
        self.checkpoint_dir, self.model_dir = self.output_dir / "checkpoints", self.output_dir / "models"
        self.checkpoint_dir.mkdir(parents=True, exist_ok=True)
        self.model_dir.mkdir(parents=True, exist_ok=True)

    @property
    def _fused_bookkeeping(self) -> bool:
        """the criterion, the running loss / hit sums and the batch cursor inside the head's launches"""
        return (self.device.type == "cuda" and isinstance(self.criterion, nn.BCEWithLogitsLoss)
                and hasattr(self.model, "bce_loss"))

    # -- batches ------------------------------------------------------------------------
    def _batches(self, edge_index, edge_type, shuffle: bool):
        """Yield (head, tail, rel) column slices; the permutation is drawn on the host like the
        reference's ``torch.randperm(num_edges)`` and moved to the device once."""
        e = edge_index.size(1)
        order = (torch.randperm(e) if shuffle else torch.arange(e)).to(edge_index.device)
        for lo in range(0, e, self.args.batch_size):
            idx = order[lo: lo + self.args.batch_size]
            yield edge_index[0, idx], edge_index[1, idx], edge_type[idx]

    def _with_negatives(self, head, tail, rel):
        nh, nt, nr = self.neg_sampler.sample(head, tail, rel)
        labels = torch.cat([torch.ones(head.numel(), device=self.device),
                            torch.zeros(nh.numel(), device=self.device)])
        return torch.cat([head, nh]), torch.cat([tail, nt]), torch.cat([rel, nr]), labels

    # -- one epoch ----------------------------------------------------------------------
    def _make_batch(self, lo: int, size: int):
        """(heads, tails, rels, labels) of train columns ``order[lo : lo + size]`` plus their
        negatives.  Device sampler: one launch reading the position from ``self._cursor``;
        ``--torch_sampler``: the reference's op sequence on torch's RNG stream."""
        if self.constrained_negatives:
            from . import ops
            return ops.sample_batch_constrained(self.train_edge_index, self.train_edge_type, self._order, self._cursor, size,
                                                self.neg_sampler.num_neg_samples, self.neg_sampler.num_nodes, self._rng,
                                                classes=self._neg_classes, known=self._neg_known,
                                                max_tries=self.negative_tries, stats=self._neg_stats)
        if self.device_sampler:
            from . import ops
            return ops.sample_batch(self.train_edge_index, self.train_edge_type, self._order, self._cursor, size,
                                    self.neg_sampler.num_neg_samples, self.neg_sampler.num_nodes, self._rng)
        idx = self._order.index_select(0, self._arange[:size] + self._cursor)
        return self._with_negatives(self.train_edge_index[0].index_select(0, idx),
                                    self.train_edge_index[1].index_select(0, idx),
                                    self.train_edge_type.index_select(0, idx))

    def _step(self, lo: int, size: int, accum: int = 1, update: bool = True):
        """One batch: assembly, forward over the train graph, BCE, backward and (when
        ``update``) clip + optimizer step; running loss / hits stay on the device.  ``lo`` is
        only documentation here - the position is whatever ``self._cursor`` holds."""
        if self.softmax:
            return self._softmax_step(lo, size, accum, update)
        view = self._draw_edges(size)                   # before the sampler: both read the cursor of THIS batch
        heads, tails, rels, labels = self._make_batch(lo, size)
        fused = self._fused_bookkeeping
        if fused:
            # the criterion fused into the head; the launch that forms the mean also keeps the epoch's running sums
            # and moves the batch cursor on (device-side bookkeeping, no host sync, no elementwise launches)
            loss, scores = self.model.bce_loss(self.train_edge_index, self.train_edge_type, heads, tails, rels, labels,
                                               stats=(self._loss_sum, self._correct, self._cursor, size), **view)
        else:
            scores = self.model(self.train_edge_index, self.train_edge_type, heads, tails, rels, **view)
            loss = self.criterion(scores, labels)
        # d(loss / accum) / d loss as a kept device scalar: `.backward()` would launch a fill for its implicit ones
        # tensor (and a division for the accumulation) in every step
        seed = self._grad_seed.get(accum)
        if seed is None:
            seed = self._grad_seed[accum] = torch.full((), 1.0 / accum, device=self.device)
        loss.backward(seed)
        if update:
            self._clip_and_update()
        if not fused:
            with torch.no_grad():
                self._loss_sum += loss.detach().double() * labels.numel()
                self._correct += ((scores.detach() > 0) == (labels > 0.5)).sum()
        return heads, tails, rels, labels, loss.detach()

    def _draw_edges(self, size: int) -> dict:
        """This step's message-passing graph: one draw into the trainer's edge-dropout view at the device cursor, keyed by
        the sampler's ``(seed, epoch)`` -> the ``graph=`` keyword of the model's loss (empty without the flags).  Part of
        the captured step: a replay draws at whatever the cursor then holds."""
        if self.attention:                              # the layers draw themselves; this step's window for both of them
            self.model.encoder.attention_window = None if not self.hide_batch_edges else dict(
                position=self._ed_position, cursor=self._cursor, batch=size, stats=self._ed_stats,
                hide_twins=self.hide_reverse_edges)
            return {}
        if self._edge_dropout is None:
            return {}
        self._edge_dropout.draw(self.edge_dropout_p, self._rng, cursor=self._cursor, batch=size if self.hide_batch_edges else 0,
                                position=self._ed_position if self.hide_batch_edges else None, stats=self._ed_stats,
                                hide_twins=self.hide_reverse_edges, paired=self.paired_edge_dropout)
        return {"graph": self._edge_dropout.view}

    def _softmax_step(self, lo: int, size: int, accum: int = 1, update: bool = True):
        """``_step`` with ``--loss softmax``: the batch is ``size`` positives of the permutation and nothing else; the
        loss is the mean over sides and samples, the running sums take the summed loss and the number of hits (the
        target is a best eligible candidate).  Eager: ``lo`` is the position."""
        idx = self._order[lo:lo + size]
        heads, tails, rels = self.train_edge_index[0, idx], self.train_edge_index[1, idx], self.train_edge_type[idx]
        if self._ed_stats is not None:
            self._cursor.fill_(lo)                      # (nothing else moves the cursor of an eager softmax step)
        view = self._draw_edges(size)
        loss, _ = self.model.softmax_loss(self.train_edge_index, self.train_edge_type, heads, tails, rels,
                                          sides=self.softmax_sides, known=self._sm_known, node_class=self._sm_node_class,
                                          stats=(self._loss_sum, self._correct), **view)
        (loss / accum if accum != 1 else loss).backward()
        if update:
            self._clip_and_update()
        return heads, tails, rels, None, loss.detach()

    def _clip_and_update(self) -> None:
        """``clip_grad_norm_`` + ``optimizer.step()`` (train.py:311-317).  On the GPU: two launches
        (``rgcn_adam_clip_step``) on the optimizer's own state tensors, so checkpoints and a later
        ``optimizer.step()`` see the same state; ``--torch_optimizer`` keeps torch's kernels."""
        if not self.fused_update:
            if self.args.grad_clip > 0:
                torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.args.grad_clip)
            self.optimizer.step()
            return
        from . import ops
        group = self.optimizer.param_groups[0]
        params = [p for p in group["params"] if p.grad is not None]
        state = self.optimizer.state
        for p in params:
            if len(state[p]) == 0:                     # what torch's Adam would create lazily
                state[p]["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                state[p]["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state[p]["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        beta1, beta2 = group["betas"]
        # The update also leaves max |p| of every matrix it writes (the embedding table, W, root) in an amax buffer of
        # the trainer's: the optimizer is their only writer, so the NEXT step's encoder takes its operand scales from
        # there (ops.amax_hint) and its first launch splits the weights without scanning 8 MB + the weights first.
        amax = [self._amax_of(p) for p in params]
        ops.adam_clip_step([p.data for p in params], [p.grad for p in params], [state[p]["exp_avg"] for p in params],
                           [state[p]["exp_avg_sq"] for p in params], [state[p]["step"] for p in params],
                           group["lr"], beta1, beta2, group["eps"], group["weight_decay"],
                           adamw=isinstance(self.optimizer, torch.optim.AdamW), max_norm=self.args.grad_clip,
                           amax_out=amax)
        for p, a in zip(params, amax):
            if a is not None:
                ops.set_amax_hint(p, a)              # valid until the tensor is modified through torch (p._version)

    def _amax_of(self, p):
        """the amax buffer the fused update publishes max |p| into (matrices only; zeroed once, kept for the run)"""
        if p.dim() < 2 or p.dtype != torch.float32:
            return None
        store = self.__dict__.setdefault("_param_amax", {})
        buf = store.get(id(p))
        if buf is None:
            from . import ops
            buf = store[id(p)] = ops.amax_buffer(p.device)[0]
        return buf

    def _capture_step(self, batch: int) -> None:
        """Record ``_step`` on the batch at ``self._cursor`` (``order``, ``cursor``, the RNG
        state and the running sums are device-resident and keep their addresses), so a
        full-size batch is one graph replay with no host work besides setting the cursor.
        Called after at least one eager step (graph bucketed, optimizer state allocated)."""
        graph = torch.cuda.CUDAGraph()
        self.optimizer.zero_grad(set_to_none=True)
        with torch.cuda.graph(graph):
            self._static = self._step(0, batch)
        self.optimizer.zero_grad(set_to_none=True)      # eager steps get fresh grads; replays use the graph's own
        self._graph, self._graph_batch = graph, batch

    def train_epoch(self, on_step: Optional[Callable] = None, max_steps: Optional[int] = None):
        """-> (mean loss per sample, accuracy).  ``on_step(heads, tails, rels, labels, loss)`` is
        an instrumentation hook (tests); ``max_steps`` truncates the epoch."""
        self.model.train()
        accum = max(1, getattr(self.args, "gradient_accumulation_steps", 1))
        bsz, e = self.args.batch_size, self.train_edge_index.size(1)
        if self._loss_sum is None:
            self._loss_sum = torch.zeros((), device=self.device, dtype=torch.float64)
            self._correct = torch.zeros((), device=self.device, dtype=torch.int64)
            self._order = torch.empty(e, device=self.device, dtype=torch.int64)
            self._cursor = torch.zeros(1, device=self.device, dtype=torch.int64)
            self._arange = torch.arange(bsz, device=self.device)
            # Philox key = the run's seed, stream = epoch (device sampler)
            self._rng = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64).to(self.device)
        self._loss_sum.zero_()
        self._correct.zero_()
        self._cursor.zero_()
        self._rng[1] += 1
        if self._neg_stats is not None:
            self._neg_stats.zero_()
        # the permutation is drawn on the host like the reference's torch.randperm(num_edges)
        self._order.copy_(torch.randperm(e))
        if self._ed_stats is not None:
            self._ed_stats.zero_()
            if self.hide_batch_edges:                # where every column stands in this epoch's order: one scatter per epoch
                if self._ed_position is None:
                    self._ed_position = torch.empty(e, device=self.device, dtype=torch.int64)
                self._ed_position[self._order] = torch.arange(e, device=self.device)
        steps = -(-e // bsz)
        if max_steps is not None:
            steps = min(steps, max_steps)
        seen = 0
        self.optimizer.zero_grad(set_to_none=True)
        for step in range(steps):
            lo, hi = step * bsz, min((step + 1) * bsz, e)
            if not self._fused_bookkeeping:
                self._cursor.fill_(lo)               # (the fused bookkeeping launch moves the cursor itself)
            replayable = self.use_hip_graph and hi - lo == bsz
            if replayable and step >= 1 and (self._graph is None or self._graph_batch != bsz):
                self._capture_step(bsz)
            if replayable and self._graph is not None and self._graph_batch == bsz:
                self._graph.replay()
                out = self._static
            else:
                last = (step + 1) % accum == 0 or step + 1 == steps
                out = self._step(lo, hi - lo, accum=accum, update=last)
                if last:
                    self.optimizer.zero_grad(set_to_none=True)
            seen += (hi - lo) * (len(self.softmax_sides) if self.softmax else 1 + self.neg_sampler.num_neg_samples)
            if on_step is not None:
                on_step(*out)
        result = (self._loss_sum / max(seen, 1)).item(), self._correct.item() / max(seen, 1)
        if self._neg_stats is not None:      # read back once per epoch, with the loss
            self.negative_stats = tuple(self._neg_stats.tolist())
        if self._ed_stats is not None:
            self.edge_dropout_stats = tuple(self._ed_stats.tolist())
            self._ed_steps = steps
        if not (self.softmax and self.device.type != "cuda"):   # (--loss softmax on the CPU indexes through torch, which raises itself)
            ops.check_indices(self.device)   # an id outside the embedding table anywhere in the epoch: IndexError, here
        return result

    def reverse_edges_found(self):
        """After a training epoch with ``--hide_reverse_edges``: False if the epoch hid exactly as many edges as it has
        columns - every step hid its own columns and not one reverse column, the data stores one direction; True if it
        hid more; None without the flag or when the last epoch was cut short."""
        e, bsz = self.train_edge_index.size(1), self.args.batch_size
        if not self.hide_reverse_edges or self._ed_steps != -(-e // bsz):
            return None
        return self.edge_dropout_stats[1] != e

    @torch.no_grad()
    def validate(self):
        """Validation triples scored with messages passed over the FULL graph."""
        self.model.eval()
        if self.attention:
            self.model.encoder.attention_window = None   # the train graph's window says nothing about the full graph
        loss_sum = torch.zeros((), device=self.device, dtype=torch.float64)
        correct = torch.zeros((), device=self.device, dtype=torch.int64)
        seen = 0
        # The reference re-runs the encoder for every validation batch (train.py:389-395); in eval mode nothing it
        # reads changes between the batches, so the node embeddings are computed ONCE here - the same rows - and every
        # batch is the head's two launches (scores + loss, then mean / running sums).  Negatives: the reference's
        # sampler on torch's RNG stream, as there.
        fused = self._fused_bookkeeping and hasattr(self.model, "encoder") and hasattr(self.model, "decoder")
        if self.softmax:
            # the same loss over the full graph's embeddings, computed once; filtered against the full graph
            emb = self.model.encoder(self.full_edge_index, self.full_edge_type)
            for heads, tails, rels in self._batches(self.val_edge_index, self.val_edge_type, shuffle=False):
                self.model.decoder.softmax_loss(emb, heads, tails, rels, sides=self.softmax_sides,
                                                known=self._sm_known_full, node_class=self._sm_node_class,
                                                stats=(loss_sum, correct))
                seen += heads.numel() * len(self.softmax_sides)
            if self.device.type == "cuda":
                ops.check_indices(self.device)
            return (loss_sum / max(seen, 1)).item(), correct.item() / max(seen, 1)
        emb = self.model.encoder(self.full_edge_index, self.full_edge_type) if fused else None
        for heads, tails, rels, labels in self._validation_batches():
            if fused:
                self.model.decoder.bce_loss(emb, heads, tails, rels, labels, stats=(loss_sum, correct, None, 0))
            else:
                scores = self.model(self.full_edge_index, self.full_edge_type, heads, tails, rels)
                loss_sum += self.criterion(scores, labels).double() * labels.numel()
                correct += ((scores > 0) == (labels > 0.5)).sum()
            seen += labels.numel()
        result = (loss_sum / max(seen, 1)).item(), correct.item() / max(seen, 1)
        ops.check_indices(self.device)
        return result

    def _validation_batches(self):
        """(heads, tails, rels, labels) of every validation batch.  Default: the reference's sampler on torch's RNG
        stream.  Under a constraint: the constrained device sampler at cursor = the batch start, keyed by the run's
        seed on a stream of its own, filtered against the FULL graph - the same negatives every time it is called."""
        if not self.constrained_negatives:
            for head, tail, rel in self._batches(self.val_edge_index, self.val_edge_type, shuffle=False):
                yield self._with_negatives(head, tail, rel)
            return
        e, bsz = self.val_edge_index.size(1), self.args.batch_size
        starts = torch.arange(0, max(e, 1), bsz, device=self.device, dtype=torch.int64)
        rng = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, VALIDATION_STREAM], dtype=torch.int64).to(self.device)
        for i, lo in enumerate(range(0, e, bsz)):
            yield ops.sample_batch_constrained(self.val_edge_index, self.val_edge_type, None, starts[i:i + 1],
                                               min(bsz, e - lo), self.neg_sampler.num_neg_samples,
                                               self.neg_sampler.num_nodes, rng, classes=self._neg_classes,
                                               known=self._neg_known_full, max_tries=self.negative_tries)

    # -- checkpoints (same keys as train.py:431-442) --------------------------------------
    def save_checkpoint(self, epoch: int, is_best: bool = False, is_final: bool = False,
                        filename: Optional[str] = None) -> Path:
        state = {"epoch": epoch, "model_state_dict": self.model.state_dict(),
                 "optimizer_state_dict": self.optimizer.state_dict(),
                 "best_val_loss": self.best_val_loss, "best_val_acc": self.best_val_acc,
                 "train_losses": self.train_losses, "val_losses": self.val_losses,
                 "train_accs": self.train_accs, "val_accs": self.val_accs, "args": self.args}
        if is_best:
            path = self.model_dir / "best_model.pt"
        elif is_final:
            path = self.model_dir / "final_model.pt"
        else:
            path = self.checkpoint_dir / (filename or f"checkpoint_epoch_{epoch}.pt")
        torch.save(state, path)
        return path

    def train(self) -> None:
        start = time.time()
        epoch = 0
        for epoch in range(1, self.args.epochs + 1):
            t0 = time.time()
            tr_loss, tr_acc = self.train_epoch()
            va_loss, va_acc = self.validate()
            self.train_losses.append(tr_loss); self.train_accs.append(tr_acc)
            self.val_losses.append(va_loss); self.val_accs.append(va_acc)
            negatives = ("" if not self.constrained_negatives else
                         " | Neg Rejected: %d | Neg Gave Up: %d" % self.negative_stats)
            if self._ed_stats is not None:
                kept, hidden = self.edge_dropout_stats
                drawn = max(1, self._ed_steps * self.train_edge_index.size(1))
                negatives += " | Edges Kept: %.4f | Edges Hidden: %d" % (kept / drawn, hidden)
                if epoch == 1 and self.reverse_edges_found() is False:
                    logger.warning("--hide_reverse_edges hid %d edges in an epoch of %d columns: no column of this data has "
                                   "a reverse column with the same relation, so the flag did nothing", hidden, hidden)
            logger.info("Epoch %d/%d | Time: %.2fs | Train Loss: %.4f | Train Acc: %.4f | Val Loss: %.4f | "
                        "Val Acc: %.4f%s", epoch, self.args.epochs, time.time() - t0, tr_loss, tr_acc, va_loss, va_acc,
                        negatives)
            is_best = va_loss < self.best_val_loss
            if is_best:
                self.best_val_loss = va_loss
            self.best_val_acc = max(self.best_val_acc, va_acc)
            if epoch % self.args.save_every == 0 or is_best:
                self.save_checkpoint(epoch, is_best=is_best)
            patience = self.args.early_stopping
            if patience > 0 and len(self.val_losses) > patience:
                recent = self.val_losses[-patience:]
                if all(v >= recent[0] for v in recent):
                    logger.info("Early stopping at epoch %d", epoch)
                    break
        logger.info("Training completed in %.2fs | best val loss %.4f | best val acc %.4f",
                    time.time() - start, self.best_val_loss, self.best_val_acc)
        self.save_checkpoint(epoch, is_final=True)


# ------------------------------------------------------------------------------------------
# data / CLI
# ------------------------------------------------------------------------------------------
def filter_edges(data: Dict, num_nodes: int, name: str = "") -> Dict:
    """Drop columns whose endpoints are >= num_nodes (the reference's host-side filter; the
    processed files hold a few such ids because of the mappings quirk)."""
    ei, et = data["edge_index"], data["edge_type"]
    keep = (ei[0] < num_nodes) & (ei[1] < num_nodes)
    dropped = int((~keep).sum())
    if dropped:
        logger.warning("%s: filtered %d invalid edges (%.2f%%)", name, dropped, 100.0 * dropped / ei.size(1))
        data = dict(data, edge_index=ei[:, keep], edge_type=et[keep])
    return data


def load_data(data_dir: str, bucket_cache: bool = False):
    """``{train,val,test}_data.pt``, ``full_graph.pt``: dicts {edge_index int64[2,E], edge_type
    int64[E], num_nodes, num_relations} (``preprocess.py:256-261``); tensors only, so they are
    read with ``weights_only=True``.  ``mappings.pt`` holds Python dicts and is not needed to train.
    ``bucket_cache``: keep the bucketed CSR-by-relation structure of the two message-passing
    graphs in ``<name>.bucketed.pt`` next to them (checked against the columns on load)."""
    root = Path(data_dir)
    files = (("train", "train_data.pt"), ("val", "val_data.pt"), ("test", "test_data.pt"), ("full", "full_graph.pt"))
    parts = {k: torch.load(root / f, weights_only=True) for k, f in files}
    n = parts["train"]["num_nodes"]
    parts = {k: filter_edges(v, n, k) for k, v in parts.items()}
    if bucket_cache:
        for k, f in files:
            parts[k] = dict(parts[k], sidecar=str(root / f.replace(".pt", ".bucketed.pt")))
    return parts["train"], parts["val"], parts["full"], parts["test"]


def synthetic_data(num_edges: int = 100_000, seed: int = 42, holdout: float = 0.15):
    """PrimeKG-shaped random graph split the way ``preprocess.py`` splits: drug-gene pairs
    (relation 0) are the prediction targets; ``holdout`` of them (the reference holds out
    7,696 of 51,306) leave the training graph for validation, both directions of a pair together."""
    from . import synth
    ei, et, n, r = synth.primekg_like(num_edges=num_edges, seed=seed)
    pair_is_target = et[0::2] == 0
    gen = torch.Generator().manual_seed(seed + 1)
    val_pairs = pair_is_target & (torch.rand(pair_is_target.numel(), generator=gen) < holdout)
    col_is_val = val_pairs.repeat_interleave(2)
    mk = lambda m: {"edge_index": ei[:, m].contiguous(), "edge_type": et[m].contiguous(),   # noqa: E731
                    "num_nodes": n, "num_relations": r}
    full = {"edge_index": ei, "edge_type": et, "num_nodes": n, "num_relations": r}
    return mk(~col_is_val), mk(col_is_val), full, mk(col_is_val)


def create_model(num_nodes: int, num_relations: int, args: argparse.Namespace) -> DrugDiseaseModel:
    model = DrugDiseaseModel(num_nodes=num_nodes, num_relations=num_relations,
                             embedding_dim=args.embedding_dim, hidden_dim=args.hidden_dim,
                             dropout=args.dropout, decoder_dropout=args.decoder_dropout,
                             num_bases=args.num_bases,
                             gather_dtype=torch.float16 if getattr(args, "fp16_gather", False) else None,
                             decoder=getattr(args, "decoder", "distmult"),
                             attention=bool(getattr(args, "attention", False)),
                             attention_slope=float(getattr(args, "attention_slope", 0.2)))
    logger.info("Model created with %s parameters",
                f"{sum(p.numel() for p in model.parameters() if p.requires_grad):,}")
    return model


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train the R-GCN link predictor on MI355X")
    p.add_argument("--data_dir", type=str, default="data/processed")
    p.add_argument("--output_dir", type=str, default="output")
    p.add_argument("--checkpoint_dir", type=str, default=None, help="[deprecated] use --output_dir")
    p.add_argument("--embedding_dim", type=int, default=64)
    p.add_argument("--hidden_dim", type=int, default=128)
    p.add_argument("--dropout", type=float, default=0.5)
    p.add_argument("--decoder_dropout", type=float, default=0.1)
    p.add_argument("--decoder", type=str, default="distmult", choices=["distmult", "complex"],
                   help="scoring head: distmult (symmetric in head and tail) or complex (Re <h, r, conj(t)>: tells a "
                        "directed edge from its reverse; hidden_dim must be a multiple of 8)")
    p.add_argument("--num_bases", type=int, default=None)
    p.add_argument("--epochs", type=int, default=100)
    p.add_argument("--batch_size", type=int, default=1024)
    p.add_argument("--lr", type=float, default=0.001)
    p.add_argument("--weight_decay", type=float, default=0.0)
    p.add_argument("--optimizer", type=str, default="adam", choices=["adam", "adamw"])
    p.add_argument("--num_neg_samples", type=int, default=1)
    p.add_argument("--loss", type=str, default="bce", choices=["bce", "softmax"],
                   help="bce: binary cross-entropy against sampled negatives (the reference's); softmax: the 1-vs-all "
                        "softmax cross-entropy of the true entity against every candidate, fused (no sampled negatives; "
                        "--filtered_negatives / --type_constrained_negatives then choose the denominator's candidates)")
    p.add_argument("--softmax_sides", type=str, default="both", choices=["tail", "both"],
                   help="--loss softmax: predict the tail of (head, relation, ?) only, or also the head of (?, relation, tail)")
    p.add_argument("--grad_clip", type=float, default=1.0)
    p.add_argument("--gradient_accumulation_steps", type=int, default=1)
    p.add_argument("--save_every", type=int, default=10)
    p.add_argument("--early_stopping", type=int, default=0)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--fp16_gather", action="store_true",
                   help="gather neighbour rows from an fp16 copy of the feature table (fp32 accumulate)")
    p.add_argument("--bucket_cache", action="store_true",
                   help="persist / reuse the bucketed graph structure next to the .pt files in --data_dir")
    p.add_argument("--torch_optimizer", action="store_true",
                   help="clip and update with torch's own kernels instead of the two-launch fused update")
    p.add_argument("--torch_sampler", action="store_true",
                   help="draw negatives with the reference's torch.rand/randint sequence instead of the "
                        "one-kernel device sampler")
    p.add_argument("--filtered_negatives", action="store_true",
                   help="redraw a training negative that is a known triple of the train graph (validation: of the full "
                        "graph); needs the device sampler")
    p.add_argument("--type_constrained_negatives", action="store_true",
                   help="replace a node only by a node of its own type (needs --node_types and the device sampler)")
    p.add_argument("--node_types", type=str, default=None,
                   help="the preprocessing's mappings.pt, or an .npz / .pt holding an int vector [num_nodes]")
    p.add_argument("--negative_tries", type=int, default=8,
                   help="draws per filtered negative before the last one is kept (1..16)")
    p.add_argument("--edge_dropout", type=float, default=0.0, metavar="P",
                   help="drop every train edge from the message-passing graph with probability P in every step (drawn on "
                        "the device; Schlichtkrull et al. 2018); validation and evaluation use the whole graph")
    p.add_argument("--hide_batch_edges", action="store_true",
                   help="hide the batch's own columns from the message-passing graph of its step, so that a positive is "
                        "not an edge the encoder can see (the reverse column of a pair stays: --hide_reverse_edges)")
    p.add_argument("--hide_reverse_edges", action="store_true",
                   help="with --hide_batch_edges: hide the column that holds a batch triple reversed, (t, r, h) for (h, r, t), "
                        "as well - data that stores both directions leaks the positive through it otherwise")
    p.add_argument("--paired_edge_dropout", action="store_true",
                   help="with --edge_dropout P: a column and its reverse column are dropped or kept together")
    p.add_argument("--attention", action="store_true",
                   help="relational attention: both layers weigh the in-edges of a (node, relation) by a learned segment "
                        "softmax instead of the plain mean (starts as the mean model; composes with --hide_batch_edges / "
                        "--hide_reverse_edges, not with --edge_dropout P > 0 or --fp16_gather; steps run eagerly)")
    p.add_argument("--attention_slope", type=float, default=0.2,
                   help="--attention: negative slope of the leaky ReLU on the attention logits, in [0, 1]")
    p.add_argument("--no_hip_graph", action="store_true",
                   help="launch every training step eagerly instead of replaying one captured HIP graph")
    p.add_argument("--synthetic", action="store_true",
                   help="train on a PrimeKG-shaped synthetic graph instead of --data_dir")
    p.add_argument("--synthetic_edges", type=int, default=100_000)
    return p


def parse_args(argv=None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


def set_seed(seed: int) -> None:
    torch.manual_seed(seed)
    np.random.seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def main(argv=None) -> None:
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(name)s - %(levelname)s - %(message)s")
    args = parse_args(argv)
    if args.checkpoint_dir is not None:
        logger.warning("--checkpoint_dir is deprecated; using it as --output_dir")
        args.output_dir = args.checkpoint_dir
    set_seed(args.seed)
    device = torch.device(args.device)
    if args.synthetic:
        train_data, val_data, full_graph, _ = synthetic_data(args.synthetic_edges, args.seed)
    else:
        train_data, val_data, full_graph, _ = load_data(args.data_dir, args.bucket_cache)
    model = create_model(train_data["num_nodes"], train_data["num_relations"], args)
    Trainer(model, train_data, val_data, full_graph, device, args).train()


if __name__ == "__main__":
    main()
