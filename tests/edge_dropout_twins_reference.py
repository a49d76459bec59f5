"""The twin contract of ``include/rgcn_edge_dropout.h`` and the two draw rules that use it (RGCN_EDGE_DROPOUT_HIDE_TWINS,
RGCN_EDGE_DROPOUT_PAIRED) restated on the host, on top of ``edge_dropout_reference.py``: which column holds the reversed
triple of which, the hidden mask that takes the twins of the window's columns along, and the Philox word a pair shares.
Everything is indexed by ORIGINAL column.  A plain module, not a test."""
import numpy as np

import edge_dropout_reference as R

HIDE_TWINS, PAIRED = 1 << 62, 1 << 61          # the option bits of rgcn_edge_dropout_draw's `batch`


def twins(edge_index, edge_type):
    """int32[E]: with F the columns holding (a, r, b), a != b, in ascending order and B those holding (b, r, a),
    twin[F[j]] = B[j] and twin[B[j]] = F[j] for j < min(|F|, |B|); -1 everywhere else (no reversed column, a self loop,
    the surplus copies of the longer side)"""
    edge_index, edge_type = np.asarray(edge_index, dtype=np.int64), np.asarray(edge_type, dtype=np.int64)
    columns = {}
    for e, triple in enumerate(zip(edge_index[0].tolist(), edge_type.tolist(), edge_index[1].tolist())):
        columns.setdefault(triple, []).append(e)                # ascending: e only grows
    twin = np.full(edge_index.shape[1], -1, dtype=np.int32)
    for (a, r, b), forward in columns.items():
        if a < b:                                               # every unordered pair once; a == b never
            for f, g in zip(forward, columns.get((b, r, a), [])):
                twin[f], twin[g] = g, f
    return twin


def hidden_mask(num_edges: int, twin, c0: int = 0, batch: int = 0, position=None, hide_twins: bool = False):
    """bool[E]: in_window(e), with ``hide_twins`` or (twin[e] >= 0 and in_window(twin[e])); all False without a position"""
    hidden = R.hidden_mask(num_edges, c0, batch, position)
    if hide_twins and position is not None:
        twin = np.asarray(twin, dtype=np.int64)
        hidden = hidden | ((twin >= 0) & hidden[np.maximum(twin, 0)])
    return hidden


def words(num_edges: int, twin, seed: int, epoch: int, c0: int = 0, paired: bool = False):
    """uint64[E]: the draw's word of every column; with ``paired`` a column with a twin takes the word of min(e, twin[e])"""
    w = R.words(num_edges, seed, epoch, c0)
    if paired:
        twin = np.asarray(twin, dtype=np.int64)
        e = np.arange(num_edges, dtype=np.int64)
        w = w[np.where(twin >= 0, np.minimum(e, twin), e)]
    return w


def kept_mask(num_edges: int, twin, p: float, seed: int, epoch: int, c0: int = 0, batch: int = 0, position=None,
              hide_twins: bool = False, paired: bool = False):
    """-> (kept bool[E], hidden bool[E]) by original column; with neither option ``edge_dropout_reference.kept_mask``"""
    hidden = hidden_mask(num_edges, twin, c0, batch, position, hide_twins)
    dropped = words(num_edges, twin, seed, epoch, c0, paired) < np.uint64(R.threshold(p))
    return ~hidden & ~dropped, hidden
