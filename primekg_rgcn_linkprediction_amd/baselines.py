"""The baselines of the reference's method comparison (``src/compare_methods.py:88-318``) on the device.

``TransE`` is ``SimpleTransE`` with its batch loop replaced by the device sampler and one batch-synchronous step
(``ops.sample_batch`` + ``ops.transe_step``, ``include/rgcn_transe.h``): an epoch over the train graph is a few hundred
short launches instead of a Python loop over every sample.  Its embeddings go to the consumers that take an embedding
matrix (``predict`` / ``predict_all``: the reference's ``(cos + 1) / 2``), and - what the reference's comparison cannot do -
it is ranked by TransE distance under the project's own filtered, type-constrained, two-sided protocol through the fused
ranking and top-k passes (``ops.transe_rank_operands``).  ``NodeDegree`` and ``Random`` are a few lines of torch.

``ComplEx`` is not in the reference's comparison (its README asks for it under "Advanced Baselines"): a free entity table
under the project's own ComplEx head (``LinkPredictor(decoder="complex")``), trained like the model - device sampler, fused
BCE, fused clip + Adam - with ``TransE``'s surface.
"""
from __future__ import annotations

import logging
from typing import Optional

import torch
from torch import Tensor

from . import consumers, ops
from .head import LinkPredictor

logger = logging.getLogger("primekg_rgcn_linkprediction_amd.baselines")


def _unit_rows(rows: int, d: int, gen: torch.Generator) -> Tensor:
    """the reference's start (``compare_methods.py:189-196``): ``randn * 0.01``, every row normalised"""
    t = torch.randn(rows, d, generator=gen) * 0.01
    return t / t.norm(dim=1, keepdim=True)


class TransE:
    """``fit`` trains on the device; ``embeddings`` float32 ``[N, d]`` and ``relation_embeddings`` ``[R, d]`` stay there.

    The update is the synchronous one of ``ops.transe_step``: a node that occurs ``m`` times in a batch has its row
    scaled by about ``1 - 2 * learning_rate * m`` before the renormalisation, so keep ``2 * learning_rate * m < 1`` for
    the busiest node of a batch; nothing here enforces it."""

    name = "TransE"

    def __init__(self, embedding_dim: int = 64, num_epochs: int = 50, learning_rate: float = 0.01, margin: float = 1.0,
                 batch_size: int = 1024, seed: int = 0, device=None, hip_graph: bool = False):
        if embedding_dim <= 0 or embedding_dim % 4:
            raise ValueError("embedding_dim must be a positive multiple of 4")
        if batch_size <= 0 or num_epochs < 0:
            raise ValueError("batch_size must be positive and num_epochs >= 0")
        self.embedding_dim, self.num_epochs, self.learning_rate = int(embedding_dim), int(num_epochs), float(learning_rate)
        self.margin, self.batch_size, self.seed = float(margin), int(batch_size), int(seed)
        self.device = torch.device("cuda" if device is None else device)
        self.hip_graph = bool(hip_graph)        # replay one captured (sampler, step) graph per full-size batch
        self.embeddings: Optional[Tensor] = None
        self.relation_embeddings: Optional[Tensor] = None
        self.epoch_losses = []          # mean over the epoch's batches of the batch mean loss
        self.epoch_active = []          # samples with a positive loss, per epoch
        self._allow = None

    # ------------------------------------------------------------------------------------------------- training
    def fit(self, edge_index: Tensor, edge_type: Tensor, num_nodes: int, num_relations: int) -> "TransE":
        """``SimpleTransE.fit``: per epoch a fresh permutation of the columns (drawn on the device), per batch one
        sampler launch (``num_neg=1``: a fair coin corrupts head or tail by a uniform node) and one step.  The ragged
        last batch runs through the same code.  One read-back per epoch."""
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("TransE.fit trains on the MI355X (HIP) only; there is no CPU fallback in this package")
        edge_index = edge_index.to(device=dev, dtype=torch.int64).contiguous()
        edge_type = edge_type.to(device=dev, dtype=torch.int64).contiguous()
        if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_type.shape != (edge_index.size(1),):
            raise ValueError("edge_index must be [2, E] and edge_type [E]")
        num_edges = edge_index.size(1)
        gen = torch.Generator().manual_seed(self.seed)
        self.embeddings = _unit_rows(num_nodes, self.embedding_dim, gen).to(dev).contiguous()
        self.relation_embeddings = _unit_rows(num_relations, self.embedding_dim, gen).to(dev).contiguous()
        self.epoch_losses, self.epoch_active, self._allow = [], [], None
        if num_edges == 0 or self.num_epochs == 0:
            return self
        batch = min(self.batch_size, num_edges)
        sizes = [min(batch, num_edges - lo) for lo in range(0, num_edges, batch)]
        with torch.cuda.device(dev):
            dev_gen = torch.Generator(device=dev).manual_seed(self.seed)
            # what a batch reads besides the tables keeps its address: the permutation, the cursor into it, the sampler's
            # (seed, epoch) key and the epoch's running sums - so a full-size batch can be one replay of a captured graph
            order = torch.empty(num_edges, dtype=torch.int64, device=dev)
            cursor = torch.zeros(1, dtype=torch.int64, device=dev)
            rng = torch.tensor([self.seed & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64).to(dev)
            loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
            active_sum = torch.zeros(1, dtype=torch.int64, device=dev)

            def one_batch(size: int) -> None:
                h, t, r, _ = ops.sample_batch(edge_index, edge_type, order, cursor, size, 1, num_nodes, rng)
                ops.transe_step(self.embeddings, self.relation_embeddings, h, t, r, size, self.learning_rate, self.margin,
                                loss_sum, active_sum)
                cursor.add_(size)

            graph = None
            for ep in range(self.num_epochs):
                order.copy_(torch.randperm(num_edges, device=dev, generator=dev_gen))
                cursor.zero_()
                rng[1] = ep
                loss_sum.zero_()
                active_sum.zero_()
                for i, size in enumerate(sizes):
                    if self.hip_graph and size == batch and graph is None and (ep, i) >= (0, 1):
                        graph = torch.cuda.CUDAGraph()           # after one eager batch: sampler, step, cursor - a chain
                        with torch.cuda.graph(graph):
                            one_batch(batch)                     # recorded, not run: the replay below is this batch
                    if graph is not None and size == batch:
                        graph.replay()
                    else:
                        one_batch(size)
                total, active = torch.cat([loss_sum, active_sum.to(torch.float64)]).tolist()   # the epoch's one read-back
                self.epoch_losses.append(total / len(sizes))
                self.epoch_active.append(int(active))
                logger.info("TransE epoch %d/%d, loss %.4f", ep + 1, self.num_epochs, self.epoch_losses[-1])
            ops.check_indices(dev)
        return self

    def _fitted(self) -> Tensor:
        if self.embeddings is None:
            raise RuntimeError("TransE: fit() first")
        return self.embeddings

    # ------------------------------------------------------------------------- the reference's pair scores
    @torch.no_grad()
    def predict(self, drugs, diseases) -> Tensor:
        """``(cos(emb[drug_b], emb[disease_b]) + 1) / 2`` per pair (``compare_methods.py:289-303``)"""
        return consumers.cosine_pair_scores(self._fitted(), drugs, diseases)

    @torch.no_grad()
    def predict_all(self, drugs, diseases) -> Tensor:
        """the ``[n_drugs, n_diseases]`` matrix of the same score (``compare_methods.py:305-318``)"""
        return consumers.cosine_score_matrix(self._fitted(), drugs, diseases)

    # --------------------------------------------------------------------------------- ranking by distance
    def _masks(self, node_class, classes_of):
        """``(allow [C, W], query_class int32 [B])`` of the type-constrained protocol, or ``(None, None)``"""
        if node_class is None:
            return None, None
        emb = self._fitted()
        node_class = torch.as_tensor(node_class)
        if node_class.shape != (emb.size(0),):
            raise ValueError(f"node_class must hold one class per entity ([{emb.size(0)}])")
        key = (node_class.data_ptr(), node_class._version)
        if self._allow is None or self._allow[0] != key:
            classes = node_class.to(device=emb.device, dtype=torch.int32).contiguous()
            self._allow = (key, node_class, classes, ops.class_allow_bits(classes, max(int(classes.max()) + 1, 1)))
        classes, allow = self._allow[2], self._allow[3]
        if isinstance(classes_of, Tensor) and classes_of.dtype == torch.int64 and classes_of.dim() == 1:
            return allow, classes[classes_of].contiguous()
        raise ValueError("one target id per query expected")

    def _rank(self, side, anchors, relations, targets, known, node_class, max_mask_bytes):
        emb = self._fitted()
        anchors, relations, targets = (torch.as_tensor(x, dtype=torch.int64).to(emb.device).contiguous().view(-1)
                                       for x in (anchors, relations, targets))
        q, cand, true_score = ops.transe_rank_operands(emb, self.relation_embeddings, anchors, relations, side)
        allow, query_class = self._masks(node_class, targets)
        return ops.distmult_rank_filtered(q, cand, true_score(targets), targets, known, side, anchors, relations, allow,
                                          query_class, max_mask_bytes)

    @torch.no_grad()
    def rank_tails(self, heads, relations, tails, *, known: Optional["ops.KnownTriples"] = None, node_class=None,
                   max_mask_bytes: int = 256 << 20) -> Tensor:
        """int64 ``[B]``: 1-based rank of ``tails[b]`` among all entities by ``|E[head] + R[rel] - e|``, smaller first,
        equal distances not counted.  ``known``: candidates that complete a known triple do not count (filtered);
        ``node_class`` (int ``[N]``): only candidates of the true tail's class count (type-constrained) - the masks and
        the pass of ``LinkPredictor.rank_tails``."""
        return self._rank("tail", heads, relations, tails, known, node_class, max_mask_bytes)

    @torch.no_grad()
    def rank_heads(self, tails, relations, heads, *, known: Optional["ops.KnownTriples"] = None, node_class=None,
                   max_mask_bytes: int = 256 << 20) -> Tensor:
        """the other side: rank of ``heads[b]`` by ``|e + R[rel] - E[tail]|``"""
        return self._rank("head", tails, relations, heads, known, node_class, max_mask_bytes)

    def _top(self, side, anchors, relations, k, known, node_class, candidate_class, max_mask_bytes):
        emb = self._fitted()
        anchors, relations = (torch.as_tensor(x, dtype=torch.int64).to(emb.device).contiguous().view(-1)
                              for x in (anchors, relations))
        if (node_class is None) != (candidate_class is None):
            raise ValueError("node_class (the class of every entity) and candidate_class (the class the answers must "
                             "have) go together")
        q, cand, _ = ops.transe_rank_operands(emb, self.relation_embeddings, anchors, relations, side)
        allow = query_class = None
        if node_class is not None:
            allow, _ = self._masks(node_class, anchors)
            if isinstance(candidate_class, Tensor):
                query_class = candidate_class.to(device=emb.device, dtype=torch.int32).contiguous()
            else:
                query_class = torch.full((anchors.numel(),), int(candidate_class), dtype=torch.int32, device=emb.device)
        ids, scores = ops.distmult_topk_filtered(q, cand, k, known, side, anchors, relations, allow, query_class,
                                                 None, max_mask_bytes)
        # score = (|q|^2 - dist^2) / 2 with |q|^2 = the query's own squared norm
        sq = (q[:, :emb.size(1)] ** 2).sum(dim=1, keepdim=True)
        return ids, (sq - 2 * scores).clamp_(min=0).sqrt_()

    @torch.no_grad()
    def top_tails(self, heads, relations, k: int, *, known: Optional["ops.KnownTriples"] = None, node_class=None,
                  candidate_class=None, max_mask_bytes: int = 256 << 20):
        """``(ids int64 [B, k], distances [B, k])``: the ``k`` nearest tails of every ``(head, relation)`` query,
        distance ascending, equal distances by id ascending, id -1 / distance +inf past the number of candidates;
        ``known``: only novel tails; ``node_class`` with ``candidate_class``: only tails of that class"""
        return self._top("tail", heads, relations, k, known, node_class, candidate_class, max_mask_bytes)

    @torch.no_grad()
    def top_heads(self, tails, relations, k: int, *, known: Optional["ops.KnownTriples"] = None, node_class=None,
                  candidate_class=None, max_mask_bytes: int = 256 << 20):
        """the ``k`` nearest heads of every ``(?, relation, tail)`` query"""
        return self._top("head", tails, relations, k, known, node_class, candidate_class, max_mask_bytes)


class ComplEx:
    """A free entity table ``[N, d]`` scored by ``LinkPredictor(decoder="complex")``: ``Re <h, r, conj(t)>`` over d / 2
    complex numbers per row, so it tells ``(h, r, t)`` from ``(t, r, h)`` (DistMult and the cosine of ``TransE.predict``
    cannot).  ``fit`` trains on the device: per batch one sampler launch (``num_neg`` corruptions per positive), the
    fused BCE head forward and backward, and the fused clip + Adam step (``ops.adam_clip_step``); one read-back per
    epoch.  ``embeddings`` float32 ``[N, d]`` and ``relation_embeddings`` ``[R, d]`` stay on the device."""

    name = "ComplEx"

    def __init__(self, embedding_dim: int = 64, num_epochs: int = 50, learning_rate: float = 0.01, batch_size: int = 1024,
                 num_neg: int = 1, grad_clip: float = 1.0, seed: int = 0, device=None):
        if embedding_dim <= 0 or embedding_dim % 8:
            raise ValueError("embedding_dim must be a positive multiple of 8")
        if batch_size <= 0 or num_epochs < 0 or num_neg <= 0:
            raise ValueError("batch_size and num_neg must be positive and num_epochs >= 0")
        self.embedding_dim, self.num_epochs, self.learning_rate = int(embedding_dim), int(num_epochs), float(learning_rate)
        self.batch_size, self.num_neg, self.grad_clip, self.seed = int(batch_size), int(num_neg), float(grad_clip), int(seed)
        self.device = torch.device("cuda" if device is None else device)
        self.embeddings: Optional[Tensor] = None
        self.decoder: Optional[LinkPredictor] = None
        self.epoch_losses = []          # mean BCE per sample, per epoch

    @property
    def relation_embeddings(self) -> Optional[Tensor]:
        return None if self.decoder is None else self.decoder.relation_embeddings.weight.detach()

    # ------------------------------------------------------------------------------------------------- training
    def fit(self, edge_index: Tensor, edge_type: Tensor, num_nodes: int, num_relations: int) -> "ComplEx":
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("ComplEx.fit trains on the MI355X (HIP) only; there is no CPU fallback in this package")
        edge_index = edge_index.to(device=dev, dtype=torch.int64).contiguous()
        edge_type = edge_type.to(device=dev, dtype=torch.int64).contiguous()
        if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_type.shape != (edge_index.size(1),):
            raise ValueError("edge_index must be [2, E] and edge_type [E]")
        num_edges = edge_index.size(1)
        gen = torch.Generator().manual_seed(self.seed)
        table = torch.nn.init.xavier_uniform_(torch.empty(num_nodes, self.embedding_dim), generator=gen)
        rel = torch.nn.init.xavier_uniform_(torch.empty(num_relations, self.embedding_dim), generator=gen)
        self.decoder = LinkPredictor(num_relations, self.embedding_dim, decoder="complex").to(dev)
        with torch.no_grad():
            self.decoder.relation_embeddings.weight.copy_(rel)
        table = table.to(dev).requires_grad_(True)
        self.embeddings, self.epoch_losses = table.detach(), []
        if num_edges == 0 or self.num_epochs == 0:
            self.decoder.eval()
            return self
        params = [table, self.decoder.relation_embeddings.weight]
        exp_avgs, exp_avg_sqs = ([torch.zeros_like(p) for p in params] for _ in range(2))
        steps = [torch.zeros(1, dtype=torch.float32, device=dev) for _ in params]
        batch = min(self.batch_size, num_edges)
        sizes = [min(batch, num_edges - lo) for lo in range(0, num_edges, batch)]
        self.decoder.train()
        with torch.cuda.device(dev):
            dev_gen = torch.Generator(device=dev).manual_seed(self.seed)
            cursor = torch.zeros(1, dtype=torch.int64, device=dev)
            rng = torch.tensor([self.seed & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64).to(dev)
            loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
            for ep in range(self.num_epochs):
                order = torch.randperm(num_edges, device=dev, generator=dev_gen)
                cursor.zero_()
                rng[1] = ep
                loss_sum.zero_()
                for size in sizes:
                    h, t, r, labels = ops.sample_batch(edge_index, edge_type, order, cursor, size, self.num_neg, num_nodes, rng)
                    # the launch that forms the mean also adds it to the epoch's sum and moves the cursor on
                    loss, _ = self.decoder.bce_loss(table, h, t, r, labels, stats=(loss_sum, None, cursor, size))
                    loss.backward()
                    ops.adam_clip_step([p.data for p in params], [p.grad for p in params], exp_avgs, exp_avg_sqs, steps,
                                       self.learning_rate, 0.9, 0.999, 1e-8, max_norm=self.grad_clip)
                    for p in params:
                        p.grad = None
                self.epoch_losses.append(float(loss_sum.item()) / (num_edges * (1 + self.num_neg)))   # the epoch's one read-back
                logger.info("ComplEx epoch %d/%d, loss %.4f", ep + 1, self.num_epochs, self.epoch_losses[-1])
            ops.check_indices(dev)
        self.decoder.eval()
        return self

    def _fitted(self) -> Tensor:
        if self.embeddings is None:
            raise RuntimeError("ComplEx: fit() first")
        return self.embeddings

    def _ids(self, *vectors):
        dev = self._fitted().device
        return [torch.as_tensor(x, dtype=torch.int64).to(dev).contiguous().view(-1) for x in vectors]

    # ------------------------------------------------------------------------------------------- per-triple scores
    @torch.no_grad()
    def predict(self, heads, tails, relations) -> Tensor:
        """``sigmoid(score(head_b, relation_b, tail_b))`` per triple: the order of head and tail matters"""
        emb = self._fitted()
        heads, tails, relations = self._ids(heads, tails, relations)
        return torch.sigmoid(self.decoder.score_triples(emb, heads, tails, relations))

    @torch.no_grad()
    def predict_all(self, heads, tails, relation: int) -> Tensor:
        """the ``[n_heads, n_tails]`` matrix of the same score under one relation"""
        emb = self._fitted()
        heads, tails = self._ids(heads, tails)
        rels = torch.full_like(heads, int(relation))
        return torch.sigmoid(self.decoder.score_all_tails(emb[heads], rels, emb).index_select(1, tails))

    # ------------------------------------------------------------------------------------------- ranking and top-k
    @torch.no_grad()
    def rank_tails(self, heads, relations, tails, *, known: Optional["ops.KnownTriples"] = None, node_class=None,
                   max_mask_bytes: int = 256 << 20) -> Tensor:
        """int64 ``[B]``: 1-based rank of ``tails[b]`` among all entities for ``(head, relation, ?)`` - the pass, the
        masks and the tie rule of ``LinkPredictor.rank_tails``"""
        emb = self._fitted()
        heads, relations, tails = self._ids(heads, relations, tails)
        return self.decoder.rank_tails(emb[heads], relations, emb, tails, known=known, head_indices=heads,
                                       node_class=self._classes(node_class), max_mask_bytes=max_mask_bytes)

    @torch.no_grad()
    def rank_heads(self, tails, relations, heads, *, known: Optional["ops.KnownTriples"] = None, node_class=None,
                   max_mask_bytes: int = 256 << 20) -> Tensor:
        """the other side, ``(?, relation, tail)``: the query operand carries the conjugate (``LinkPredictor.rank_heads``)"""
        emb = self._fitted()
        tails, relations, heads = self._ids(tails, relations, heads)
        return self.decoder.rank_heads(emb[tails], relations, emb, heads, known=known, tail_indices=tails,
                                       node_class=self._classes(node_class), max_mask_bytes=max_mask_bytes)

    def _classes(self, node_class):
        if node_class is None:
            return None
        node_class = torch.as_tensor(node_class)
        if getattr(self, "_class_key", None) is not node_class:                 # the head caches the allow rows by tensor
            self._class_key, self._class_dev = node_class, node_class.to(self._fitted().device)
        return self._class_dev

    @torch.no_grad()
    def top_tails(self, heads, relations, k: int, *, known: Optional["ops.KnownTriples"] = None, node_class=None,
                  candidate_class=None, max_mask_bytes: int = 256 << 20):
        """``(ids int64 [B, k], scores [B, k])``: the ``k`` best tails of every ``(head, relation)`` query, score
        descending, equal scores by id ascending, id -1 / score -inf past the number of candidates"""
        emb = self._fitted()
        heads, relations = self._ids(heads, relations)
        return self.decoder.top_tails(emb[heads], relations, emb, k, known=known, head_indices=heads,
                                      node_class=self._classes(node_class), candidate_class=candidate_class,
                                      max_mask_bytes=max_mask_bytes)

    @torch.no_grad()
    def top_heads(self, tails, relations, k: int, *, known: Optional["ops.KnownTriples"] = None, node_class=None,
                  candidate_class=None, max_mask_bytes: int = 256 << 20):
        """the ``k`` best heads of every ``(?, relation, tail)`` query"""
        emb = self._fitted()
        tails, relations = self._ids(tails, relations)
        return self.decoder.top_heads(emb[tails], relations, emb, k, known=known, tail_indices=tails,
                                      node_class=self._classes(node_class), candidate_class=candidate_class,
                                      max_mask_bytes=max_mask_bytes)


class NodeDegree:
    """``NodeDegreeBaseline`` (``compare_methods.py:105-163``): a node's degree counts both endpoint rows of the train
    columns and is divided by the largest degree of its type; a pair scores ``sqrt(deg_drug * deg_disease)``, a node
    that is not of the asked type counts 0.01, as there."""

    name = "Node Degree"
    OUTSIDE = 0.01

    def __init__(self):
        self.drug_degree: Optional[Tensor] = None
        self.disease_degree: Optional[Tensor] = None

    def fit(self, edge_index: Tensor, node_class: Tensor, drug_class: int, disease_class: int) -> "NodeDegree":
        node_class = torch.as_tensor(node_class).to(edge_index.device)
        n = node_class.numel()
        degree = torch.bincount(edge_index.reshape(-1).to(torch.int64), minlength=n)[:n].to(torch.float64)

        def of_type(c):
            mine = node_class == c
            top = degree[mine].max() if bool(mine.any()) else torch.ones((), dtype=torch.float64, device=degree.device)
            return torch.where(mine, degree / top, torch.full_like(degree, self.OUTSIDE))

        self.drug_degree, self.disease_degree = of_type(drug_class), of_type(disease_class)
        return self

    def predict(self, drugs, diseases) -> Tensor:
        if self.drug_degree is None:
            raise RuntimeError("NodeDegree: fit() first")
        dev = self.drug_degree.device
        a, b = (torch.as_tensor(x, dtype=torch.int64).to(dev).view(-1) for x in (drugs, diseases))
        return torch.sqrt(self.drug_degree[a] * self.disease_degree[b])

    def predict_all(self, drugs, diseases) -> Tensor:
        if self.drug_degree is None:
            raise RuntimeError("NodeDegree: fit() first")
        dev = self.drug_degree.device
        a, b = (torch.as_tensor(x, dtype=torch.int64).to(dev).view(-1) for x in (drugs, diseases))
        return torch.sqrt(self.drug_degree[a].unsqueeze(1) * self.disease_degree[b].unsqueeze(0))


class Random:
    """``RandomBaseline``: uniform scores on [0, 1) from a seeded generator"""

    name = "Random"

    def __init__(self, seed: int = 42):
        self.seed = int(seed)
        self.gen = torch.Generator().manual_seed(self.seed)

    def fit(self, *args, **kwargs) -> "Random":
        return self

    def predict(self, drugs, diseases) -> Tensor:
        return torch.rand(len(drugs), generator=self.gen, dtype=torch.float64)

    def predict_all(self, drugs, diseases) -> Tensor:
        return torch.rand(len(drugs), len(diseases), generator=self.gen, dtype=torch.float64)
