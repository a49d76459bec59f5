"""Encoder + full link-prediction model on the HIP R-GCN engine.

Host-side mirror of the reference's model file so that its callers keep working
unchanged: class names, constructor arguments and order,
method names/arguments and state-dict keys follow ``src/models/rgcn.py``:

* ``DrugDiseaseRGCN``  - ``rgcn.py:21-142``  (embedding table -> conv1 -> relu -> dropout -> conv2)
* ``DrugDiseaseModel`` - ``rgcn.py:246-415`` (encoder + DistMult decoder, ``forward`` /
  ``predict`` / ``predict_all_tails`` / ``get_embeddings``)

so ``Trainer`` (``src/train.py:291-297, 389-395``) and ``ModelEvaluator``
(``src/evaluate.py:189-195, 251-262``) call sites stay textually intact, and reference
checkpoints (``encoder.node_embeddings.weight``, ``encoder.conv{1,2}.{weight,root,bias[,comp]}``,
``decoder.relation_embeddings.weight``) load with ``load_state_dict``.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from .conv import RGCNConv, rgcn_encoder2
from .head import LinkPredictor


class DrugDiseaseRGCN(nn.Module):
    """Two-layer R-GCN encoder over a learnable node-embedding table."""

    def __init__(self, num_nodes: int, num_relations: int, embedding_dim: int = 64,
                 hidden_dim: int = 128, dropout: float = 0.5, num_bases: Optional[int] = None,
                 gather_dtype=None, attention: bool = False, attention_slope: float = 0.2):
        super().__init__()
        self.num_nodes = num_nodes
        self.num_relations = num_relations
        self.embedding_dim = embedding_dim
        self.hidden_dim = hidden_dim
        self.node_embeddings = nn.Embedding(num_nodes, embedding_dim)
        # attention (off by default): both layers weigh the in-edges of a (node, relation) by a learned segment softmax
        # (attention.py); with its parameters at zero - their initial value - the encoder is the mean encoder
        self.attention = bool(attention)
        self.attention_window = None       # the trainer's hidden window for both layers' draws (RelationalAttentionConv.forward)
        if self.attention:
            from .attention import RelationalAttentionConv
            layer = dict(num_relations=num_relations, num_bases=num_bases, gather_dtype=gather_dtype,
                         negative_slope=attention_slope)
            self.conv1 = RelationalAttentionConv(embedding_dim, hidden_dim, **layer)
            self.conv2 = RelationalAttentionConv(hidden_dim, hidden_dim, **layer)
        else:
            self.conv1 = RGCNConv(in_channels=embedding_dim, out_channels=hidden_dim,
                                  num_relations=num_relations, num_bases=num_bases, gather_dtype=gather_dtype)
            self.conv2 = RGCNConv(in_channels=hidden_dim, out_channels=hidden_dim,
                                  num_relations=num_relations, num_bases=num_bases, gather_dtype=gather_dtype)
        self.dropout = nn.Dropout(dropout)
        self._init_embeddings()

    def _init_embeddings(self) -> None:
        nn.init.xavier_uniform_(self.node_embeddings.weight)

    def forward(self, edge_index: Tensor, edge_type: Tensor,
                node_indices: Optional[Tensor] = None, graph=None) -> Tensor:
        """``graph``: the view of an ``ops.EdgeDropout`` on this graph - messages then pass over the edges its last draw
        kept.  Training mode only: in ``eval()`` (and under ``no_grad`` without dropout) the whole graph is used."""
        # the whole table is the layer-1 input (no lookup) unless a subset is asked for
        x = self.node_embeddings.weight if node_indices is None else self.node_embeddings(node_indices)
        p = self.dropout.p if self.training else 0.0
        if self.attention:
            # layer by layer (not the fused two-layer node): each layer draws its softmax into a view of its own.  The
            # hidden window, if the trainer set one, goes to both draws; its counters to the first only.
            if node_indices is not None:
                raise NotImplementedError("an attention encoder runs over the whole embedding table")
            if graph is not None and graph.edge_dropout:
                raise ValueError("an attention encoder draws into views of its own: pass the graph's bucketing, not the "
                                 "view of an edge dropout")
            window = dict(self.attention_window or {})
            x = self.conv1(x, edge_index, edge_type, activation="relu", graph=graph, window=window)
            x = self.dropout(x)
            window.pop("stats", None)
            return self.conv2(x, edge_index, edge_type, graph=graph, window=window)
        if graph is not None and graph.edge_dropout and not self.training:
            graph = graph.parent
        if p < 1.0:
            # conv1 -> relu -> dropout -> conv2 (rgcn.py:123-128) as one fused autograd node; the
            # mask comes from torch's dropout kernel and RNG stream, as in the reference
            return rgcn_encoder2(x, edge_index, edge_type, self.conv1, self.conv2, dropout_p=p, graph=graph)
        x = self.conv1(x, edge_index, edge_type, activation="relu", graph=graph)      # p == 1: everything dropped
        x = self.dropout(x)
        return self.conv2(x, edge_index, edge_type, graph=graph)

    def get_node_embeddings(self, node_indices: Tensor) -> Tensor:
        return self.node_embeddings(node_indices)


class DrugDiseaseModel(nn.Module):
    """R-GCN encoder + scoring head: DistMult (the default) or ComplEx (``decoder="complex"``, ``LinkPredictor``)."""

    def __init__(self, num_nodes: int, num_relations: int, embedding_dim: int = 64,
                 hidden_dim: int = 128, dropout: float = 0.5, decoder_dropout: float = 0.0,
                 num_bases: Optional[int] = None, gather_dtype=None, decoder: str = "distmult",
                 attention: bool = False, attention_slope: float = 0.2):
        super().__init__()
        self.num_nodes = num_nodes
        self.num_relations = num_relations
        self.hidden_dim = hidden_dim
        extra = dict(attention=True, attention_slope=attention_slope) if attention else {}
        self.encoder = DrugDiseaseRGCN(num_nodes=num_nodes, num_relations=num_relations,
                                       embedding_dim=embedding_dim, hidden_dim=hidden_dim,
                                       dropout=dropout, num_bases=num_bases, gather_dtype=gather_dtype, **extra)
        self.decoder = LinkPredictor(num_relations=num_relations, embedding_dim=hidden_dim,
                                     dropout=decoder_dropout, decoder=decoder)

    def forward(self, edge_index: Tensor, edge_type: Tensor, head_indices: Tensor,
                tail_indices: Tensor, relation_types: Tensor, graph=None) -> Tensor:
        node_embeddings = self._encode(edge_index, edge_type, graph)
        # rgcn.py:325-329: two row gathers + decoder, fused into one scoring kernel
        return self.decoder.score_triples(node_embeddings, head_indices, tail_indices, relation_types)

    def _encode(self, edge_index: Tensor, edge_type: Tensor, graph=None) -> Tensor:
        """the encoder's call, unchanged when no ``graph=`` override is given (an encoder without the keyword keeps working)"""
        if graph is None:
            return self.encoder(edge_index, edge_type)
        return self.encoder(edge_index, edge_type, graph=graph)

    def bce_loss(self, edge_index: Tensor, edge_type: Tensor, head_indices: Tensor, tail_indices: Tensor,
                 relation_types: Tensor, labels: Tensor, stats=None, graph=None):
        """``(nn.BCEWithLogitsLoss()(self(...), labels), scores)`` - what ``Trainer`` needs per
        step (``train.py:291-300``) with the loss fused into the head kernels; ``stats``: see
        ``LinkPredictor.bce_loss``; ``graph``: see ``DrugDiseaseRGCN.forward``."""
        node_embeddings = self._encode(edge_index, edge_type, graph)
        return self.decoder.bce_loss(node_embeddings, head_indices, tail_indices, relation_types, labels, stats)

    def softmax_loss(self, edge_index: Tensor, edge_type: Tensor, head_indices: Tensor, tail_indices: Tensor,
                     relation_types: Tensor, graph=None, **kwargs):
        """``(mean loss, hits)``: the 1-vs-all softmax loss of the positives against every entity, the twin of
        ``bce_loss``; ``kwargs``: ``sides=``, ``known=``, ``node_class=``, ``stats=``, ``max_mask_bytes=`` of
        ``LinkPredictor.softmax_loss``; ``graph``: see ``DrugDiseaseRGCN.forward``."""
        node_embeddings = self._encode(edge_index, edge_type, graph)
        return self.decoder.softmax_loss(node_embeddings, head_indices, tail_indices, relation_types, **kwargs)

    def predict(self, edge_index: Tensor, edge_type: Tensor, head_indices: Tensor,
                tail_indices: Tensor, relation_types: Tensor) -> Tensor:
        self.eval()
        with torch.no_grad():
            return self.forward(edge_index, edge_type, head_indices, tail_indices, relation_types)

    def predict_all_tails(self, edge_index: Tensor, edge_type: Tensor, head_indices: Tensor,
                          relation_types: Tensor) -> Tensor:
        self.eval()
        with torch.no_grad():
            emb = self.encoder(edge_index, edge_type)
            return self.decoder.score_all_tails(emb[head_indices], relation_types, emb)

    def predict_top_tails(self, edge_index: Tensor, edge_type: Tensor, anchor_indices: Tensor, relation_types: Tensor,
                          k: int, **kwargs):
        """``(ids [B, k], scores [B, k])``: the ``k`` best tails of every ``(anchor, relation)`` query - the first
        ``k`` columns of a stable descending sort of ``predict_all_tails(...)`` restricted to the candidates, without
        the ``[B, N]`` matrix.  ``kwargs``: ``known=`` (novel tails only), ``node_class=`` + ``candidate_class=``,
        ``min_score=``, ``max_mask_bytes=`` of ``LinkPredictor.top_tails``."""
        self.eval()
        with torch.no_grad():
            emb = self.encoder(edge_index, edge_type)
            return self.decoder.top_tails(emb[anchor_indices], relation_types, emb, k, head_indices=anchor_indices, **kwargs)

    def predict_top_heads(self, edge_index: Tensor, edge_type: Tensor, anchor_indices: Tensor, relation_types: Tensor,
                          k: int, **kwargs):
        """the ``k`` best heads of every ``(?, relation, anchor)`` query (``LinkPredictor.top_heads``)"""
        self.eval()
        with torch.no_grad():
            emb = self.encoder(edge_index, edge_type)
            return self.decoder.top_heads(emb[anchor_indices], relation_types, emb, k, tail_indices=anchor_indices, **kwargs)

    def get_embeddings(self, edge_index: Tensor, edge_type: Tensor) -> Tensor:
        self.eval()
        with torch.no_grad():
            return self.encoder(edge_index, edge_type)
