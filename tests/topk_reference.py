"""Host restatement of the top-k selection, shared by ``test_topk_host.py`` and ``test_topk.py`` (no GPU here).

Candidates of a row: allowed, not known, not NaN, ``>= min_score``.  Order: score descending, equal scores by id
ascending - what a stable descending sort over ids ``0 .. N-1`` gives.  +inf and -inf are scores like any other: a
candidate that scores -inf (no ``min_score``) is listed with its id after every finite one.  Output: the first ``k``
candidates, id -1 and score -inf past their number (``k > N`` included)."""
import numpy as np
import torch


def restate_topk(scores: torch.Tensor, k: int, allowed=None, known=None, min_score=None):
    """``scores`` float32 ``[B, N]`` on the CPU, ``allowed`` / ``known`` bool ``[B, N]`` or None ->
    ``(ids int64 [B, k], scores float32 [B, k])``"""
    s = scores.clone()
    invalid = torch.isnan(s)
    if allowed is not None:
        invalid |= ~allowed
    if known is not None:
        invalid |= known
    if min_score is not None:
        invalid |= ~(s >= min_score)
    s[invalid] = float("-inf")
    # two stable sorts: by score descending (ids ascending among equals), then the candidates in front of the rest -
    # a candidate that scores -inf keeps its id and stands after every finite one, the padding after it
    by_score = torch.sort(s, dim=1, descending=True, stable=True).indices
    front = torch.sort(invalid.gather(1, by_score).to(torch.int8), dim=1, stable=True).indices
    order = by_score.gather(1, front)
    b, n = s.shape
    ids = torch.full((b, k), -1, dtype=torch.int64)
    vals = torch.full((b, k), float("-inf"), dtype=torch.float32)
    m = min(k, n)
    idx = order[:, :m].clone()
    val = s.gather(1, idx)
    bad = invalid.gather(1, idx)
    idx[bad] = -1
    val[bad] = float("-inf")
    ids[:, :m], vals[:, :m] = idx, val
    # valid slots come first: an invalid slot is never followed by a valid one
    assert not bool(((ids[:, :-1] < 0) & (ids[:, 1:] >= 0)).any())
    return ids, vals


def brute_topk(scores, k, allowed=None, known=None, min_score=None):
    """the same meaning as a python loop over rows and entities (tiny inputs only)"""
    b, n = scores.shape
    ids, vals = [], []
    for r in range(b):
        cand = []
        for c in range(n):
            v = float(scores[r, c])
            if v != v or (allowed is not None and not bool(allowed[r, c])) or (known is not None and bool(known[r, c])):
                continue
            if min_score is not None and not v >= min_score:
                continue
            cand.append((-v, c))
        cand.sort()
        cand = cand[:k]
        ids.append([c for _, c in cand] + [-1] * (k - len(cand)))
        vals.append([-v for v, _ in cand] + [float("-inf")] * (k - len(cand)))
    return torch.tensor(ids, dtype=torch.int64).view(b, k), torch.tensor(vals, dtype=torch.float32).view(b, k)


def bool_to_words(mask: torch.Tensor) -> torch.Tensor:
    """bool [rows, n] -> int32 [rows, ceil(n / 32)] mask words (bit n & 31 of word n >> 5, padding bits zero)"""
    rows, n = mask.shape
    w = (n + 31) // 32
    padded = np.zeros((rows, w * 32), dtype=np.uint32)
    padded[:, :n] = mask.numpy()
    words = (padded.reshape(rows, w, 32) << np.arange(32, dtype=np.uint32)).sum(2, dtype=np.uint32)
    return torch.from_numpy(words.view(np.int32))


def host_known(edge_index, edge_type, anchors, rels, side, n):
    """bool [B, n]: candidate is a known completion of (anchor, relation) - brute force over python sets"""
    sets = {}
    a_row, o_row = (0, 1) if side == "tail" else (1, 0)
    for a, o, r in zip(edge_index[a_row].tolist(), edge_index[o_row].tolist(), edge_type.tolist()):
        sets.setdefault((a, r), set()).add(o)
    out = torch.zeros(len(anchors), n, dtype=torch.bool)
    for b, (a, r) in enumerate(zip(anchors.tolist(), rels.tolist())):
        out[b, list(sets.get((a, r), ()))] = True
    return out


RAGGED = [(1, 100, 32), (63, 127, 128), (65, 129, 32), (64, 128, 128), (65, 30926, 128), (130, 100, 128), (1, 129, 128),
          (63, 100, 32), (65, 127, 128), (65, 129, 64), (65, 129, 96)]


def ragged_case(batch, entities, d):
    """the generator and mask construction of ``test_masked_ranks_ragged_shapes`` (CPU tensors)"""
    g = torch.Generator().manual_seed(batch * 1000 + entities + d)
    head = torch.randn(batch, d, generator=g)
    emb = torch.randn(entities, d, generator=g)
    rel = torch.randint(0, 4, (batch,), generator=g)
    target = torch.randint(0, entities, (batch,), generator=g)
    cls = torch.randint(-1, 3, (entities,), generator=g).to(torch.int32)            # -1: in no class
    known = torch.rand(batch, entities, generator=g) < 0.3
    qcls = cls[target].clamp(min=0)
    allowed = cls.view(1, -1) == qcls.view(-1, 1)
    return dict(head=head, emb=emb, rel=rel, target=target, cls=cls, known=known, qcls=qcls, allowed=allowed)
