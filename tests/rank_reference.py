"""Host restatement of the link-ranking count, shared by ``test_rank_reference_host.py`` and ``test_rank_nonfinite.py``
(no GPU here).  The rule of ``include/rgcn_hip.h`` (``distmult_rank_masked``):

    an eligible candidate n counts against query b UNLESS ``scores[b, n] <= true[b]``;
    eligible: ``n != target[b]``, allowed, not known;  ``rank[b] = 1 + the count``.

Without NaN this is ``scores > true`` (infinities included, equal scores do not count).  A NaN candidate counts against
every true score; a NaN true score is beaten by every eligible candidate: ``rank = 1 + #eligible``."""
import torch


def eligible_mask(target, shape, allowed=None, known=None):
    """bool ``[B, N]``: not the target (struck only when ``0 <= target < N``), allowed, not known"""
    b, n = shape
    ok = torch.ones(b, n, dtype=torch.bool)
    hit = (target >= 0) & (target < n)
    ok[torch.arange(b)[hit], target[hit]] = False
    if allowed is not None:
        ok &= allowed
    if known is not None:
        ok &= ~known
    return ok


def restate_rank(scores, true, target, allowed=None, known=None):
    """``scores`` float ``[B, N]``, ``true`` ``[B]``, ``target`` int64 ``[B]``, ``allowed`` / ``known`` bool ``[B, N]`` or
    None, all on the CPU -> int64 ``[B]``"""
    return 1 + (~(scores <= true[:, None]) & eligible_mask(target, scores.shape, allowed, known)).sum(1)


def brute_rank(scores, true, target, allowed=None, known=None):
    """the same meaning as a python loop over queries and entities (tiny inputs only)"""
    b, n = scores.shape
    out = []
    for r in range(b):
        t = float(true[r])
        beaten = 0
        for c in range(n):
            if c == int(target[r]):
                continue
            if allowed is not None and not bool(allowed[r, c]):
                continue
            if known is not None and bool(known[r, c]):
                continue
            if float(scores[r, c]) <= t:                       # False whenever either side is NaN
                continue
            beaten += 1
        out.append(1 + beaten)
    return torch.tensor(out, dtype=torch.int64)
