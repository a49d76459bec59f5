"""The draw of ``include/rgcn_edge_dropout.h`` restated on the host in numpy: the kept mask from Philox words and the batch
window, the integer kept counts of the (destination, relation) segments, the float32 weights by one division, and the
weighted aggregate in float64 - what the device must equal bit for bit (mask, counts, weights) or within computed bounds
(aggregates).  Everything is indexed by ORIGINAL column; ``bucketed`` moves it into a direction's order.  A plain module,
not a test."""
import numpy as np

from resample_reference import M32, philox4x32_10_np

STREAM = 0x45444F50                      # RGCN_EDGE_DROPOUT_STREAM ("EDOP"), counter word 3


def threshold(p: float) -> int:
    """T = floor(p * 2^32) as uint32 (the product is exact: a power-of-two scaling of a double)"""
    if not 0.0 <= p < 1.0:
        raise ValueError("p must be in [0, 1)")
    return int(p * 4294967296.0)


def words(num_edges: int, seed: int, epoch: int, c0: int = 0):
    """uint64[E]: word 0 of philox4x32_10(counter = (e, low32(c0), low32(epoch), STREAM), key = (low32(seed), high32(seed)))"""
    seed &= 0xFFFFFFFFFFFFFFFF
    e = np.arange(num_edges, dtype=np.uint64)
    zeros = np.zeros(num_edges, dtype=np.uint64)
    c = philox4x32_10_np(e, zeros + np.uint64(c0 & M32), zeros + np.uint64(epoch & M32), zeros + np.uint64(STREAM),
                         (seed & M32, seed >> 32))
    return c[0]


def hidden_mask(num_edges: int, c0: int = 0, batch: int = 0, position=None):
    """bool[E]: c0 <= position[e] < c0 + batch (all False without a position)"""
    if position is None:
        return np.zeros(num_edges, dtype=bool)
    position = np.asarray(position, dtype=np.int64)
    return (position >= c0) & (position < c0 + batch)


def kept_mask(num_edges: int, p: float, seed: int, epoch: int, c0: int = 0, batch: int = 0, position=None):
    """-> (kept bool[E], hidden bool[E]) by original column"""
    hidden = hidden_mask(num_edges, c0, batch, position)
    dropped = words(num_edges, seed, epoch, c0) < np.uint64(threshold(p))
    return ~hidden & ~dropped, hidden


def kept_counts(edge_index, edge_type, kept, num_nodes: int, num_relations: int):
    """int32[N * R]: kept edges of every forward segment (destination * R + relation)"""
    edge_index, edge_type = np.asarray(edge_index, dtype=np.int64), np.asarray(edge_type, dtype=np.int64)
    seg = edge_index[1] * num_relations + edge_type
    return np.bincount(seg[np.asarray(kept, dtype=bool)], minlength=num_nodes * num_relations).astype(np.int32)


def weights(edge_index, edge_type, kept, num_nodes: int, num_relations: int):
    """float32[E] by original column: kept ? 1.0f / (float)k[dst, rel] : 0.0f - ONE IEEE float32 division"""
    edge_index, edge_type = np.asarray(edge_index, dtype=np.int64), np.asarray(edge_type, dtype=np.int64)
    kept = np.asarray(kept, dtype=bool)
    k = kept_counts(edge_index, edge_type, kept, num_nodes, num_relations)
    k_e = k[edge_index[1] * num_relations + edge_type].astype(np.float32)
    w = np.zeros(edge_index.shape[1], dtype=np.float32)
    w[kept] = np.float32(1.0) / k_e[kept]           # (a kept edge counts itself: k >= 1)
    return w


def bucketed(values, perm):
    """values by original column -> values in a direction's bucketed order (``perm[pos]`` = original column of position pos)"""
    return np.asarray(values)[np.asarray(perm, dtype=np.int64)]


def aggregate_f64(x, edge_index, edge_type, w, num_nodes: int, num_relations: int, transposed: bool = False):
    """float64 [N, R * d]: forward  agg[dst, rel] = sum of w[e] * x[src]   (the mean over the kept in-edges),
                           transposed agg[src, rel] = sum of w[e] * x[dst]   (its adjoint).
    -> (agg, mag) with mag the same sums of |w[e] * x|: what a rounding bound is taken from."""
    x = np.asarray(x, dtype=np.float64)
    edge_index, edge_type = np.asarray(edge_index, dtype=np.int64), np.asarray(edge_type, dtype=np.int64)
    key_node, other = (edge_index[0], edge_index[1]) if transposed else (edge_index[1], edge_index[0])
    seg = key_node * num_relations + edge_type
    rows = np.asarray(w, dtype=np.float64)[:, None] * x[other]
    agg = np.zeros((num_nodes * num_relations, x.shape[1]))
    mag = np.zeros_like(agg)
    np.add.at(agg, seg, rows)
    np.add.at(mag, seg, np.abs(rows))
    return agg.reshape(num_nodes, -1), mag.reshape(num_nodes, -1)


def kept_subgraph(edge_index, edge_type, kept):
    """the columns a draw kept, in their original order: what the oracle layer runs on"""
    kept = np.asarray(kept, dtype=bool)
    return np.asarray(edge_index)[:, kept], np.asarray(edge_type)[kept]
