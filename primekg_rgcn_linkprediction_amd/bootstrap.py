"""Intervals and paired p-values from the device bootstrap (``ops.classification_counts`` / ``ops.rank_sums``,
``include/rgcn_resample.h``): what ``evaluate.py --bootstrap`` and ``compare.py --bootstrap`` report.

The resampling unit is the test triple.  A method's metric in replicate ``b`` is a function of the weights of
replicate ``b`` alone, and the weights are a pure function of ``(seed, b, unit)``: methods that are handed the same
unit vectors and seed are resampled TOGETHER, so the difference of two methods can be taken replicate by replicate
(paired).  The arithmetic on the replicate vectors is plain numpy (``interval``, ``paired_difference``); the median
rank is not a sum over queries and is not resampled.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import ops

SIGNIFICANCE_METRICS = ("auc_roc", "auc_pr", "mrr", "hits@10")


def _number(x) -> Optional[float]:
    x = float(x)
    return x if np.isfinite(x) else None


def interval(values: np.ndarray) -> Dict:
    """``values[0]`` the point estimate, ``values[1:]`` the replicates (NaN: undefined in that replicate, dropped) ->
    estimate, standard error (the replicates' standard deviation, ``ddof=1``) and the 2.5 / 97.5 percentile interval"""
    values = np.asarray(values, dtype=np.float64)
    reps = values[1:][np.isfinite(values[1:])]
    return {"estimate": _number(values[0]),
            "se": _number(np.std(reps, ddof=1)) if reps.size > 1 else None,
            "ci95": [_number(np.percentile(reps, 2.5)), _number(np.percentile(reps, 97.5))] if reps.size else [None, None]}


def paired_difference(a: np.ndarray, b: np.ndarray) -> Dict:
    """the paired comparison of two methods' replicate vectors (row 0: the point estimates): with ``d_b = a_b - b_b``
    over the replicates ``b >= 1`` in which both are defined, the mean difference, its 2.5 / 97.5 percentile interval
    and the two-sided p-value ``min(1, 2 min((1 + #{d_b <= 0}) / (B + 1), (1 + #{d_b >= 0}) / (B + 1)))``"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 1 or a.size < 1:
        raise ValueError("two replicate vectors of one length expected")
    d = (a - b)[1:]
    d = d[np.isfinite(d)]
    n = int(d.size)
    out = {"difference": _number(a[0] - b[0]), "replicates": n}
    if n == 0:
        return dict(out, mean_difference=None, ci95=[None, None], p_value=None)
    below, above = int((d <= 0).sum()), int((d >= 0).sum())
    p = min(1.0, 2.0 * min((1 + below) / (n + 1), (1 + above) / (n + 1)))
    return dict(out, mean_difference=float(d.mean()), ci95=[float(np.percentile(d, 2.5)), float(np.percentile(d, 97.5))],
                p_value=p)


def triple_units(num_triples: int, num_samples: int, device) -> torch.Tensor:
    """int32 ``[num_samples]``: the test triple of every sample in the sampler's layout - sample ``i < b`` is triple
    ``i``, negative ``i >= b`` belongs to triple ``(i - b) // k`` with ``k`` negatives per triple"""
    b = int(num_triples)
    i = torch.arange(int(num_samples), dtype=torch.int64, device=device)
    if b == 0 or num_samples <= b:
        return i.to(torch.int32)
    k = (int(num_samples) - b) // b
    return torch.where(i < b, i, (i - b) // max(k, 1)).to(torch.int32)


def query_units(num_triples: int, num_queries: int, device) -> torch.Tensor:
    """int32 ``[num_queries]``: query ``i`` belongs to triple ``i mod b`` (the tail queries, then the head queries)"""
    return (torch.arange(int(num_queries), dtype=torch.int64, device=device) % max(int(num_triples), 1)).to(torch.int32)


def replicate_vectors(scores: torch.Tensor, labels: torch.Tensor, score_unit: torch.Tensor, ranks: torch.Tensor,
                      rank_unit: torch.Tensor, k_values: Sequence[int], replicates: int, seed: int,
                      threshold: float = 0.5):
    """-> ``(vectors, degenerate, w_sum)``: float64 ``[replicates + 1]`` numpy vectors by metric name, the number of
    replicates ``>= 1`` in which a class had no weight, and the ranking's total weight per replicate"""
    counts = ops.classification_counts(scores, labels, score_unit, replicates, seed, threshold)
    vectors = {"auc_roc": counts.auc_roc(), "auc_pr": counts.auc_pr(), "f1_score": counts.f1()}
    k_values = [int(k) for k in k_values]
    w_sum = None
    for lo in range(0, max(len(k_values), 1), 8):                      # at most 8 thresholds per call
        sums = ops.rank_sums(ranks, rank_unit, k_values[lo:lo + 8], replicates, seed)
        if w_sum is None:
            w_sum = sums.w_sum
            vectors["mrr"], vectors["mean_rank"] = sums.mrr(), sums.mean_rank()
        for k in k_values[lo:lo + 8]:
            vectors[f"hits@{k}"] = sums.hits(k)
    vectors = {name: v.cpu().numpy() for name, v in vectors.items()}
    return vectors, int(counts.degenerate()[1:].sum()), w_sum.cpu().numpy()


def block(vectors: Dict[str, np.ndarray], degenerate: int, replicates: int, seed: int, w_sum=None) -> Dict:
    """the ``"bootstrap"`` block of a result file: per metric the estimate, standard error and interval, and the
    replicate vectors themselves (``None`` where undefined) so that any other paired comparison can be made later;
    ``weight_sums``: the queries' total weight per replicate - equal for two methods exactly when they were paired"""
    out = {name: interval(v) for name, v in vectors.items()}
    out.update(replicates=int(replicates), seed=int(seed), degenerate_replicates=int(degenerate),
               replicate_values={name: [_number(x) for x in v] for name, v in vectors.items()})
    if w_sum is not None:
        out["weight_sums"] = [int(x) for x in w_sum]
    return out


def significance(vectors_by_method: Dict[str, Dict[str, np.ndarray]], metrics: Sequence[str] = SIGNIFICANCE_METRICS) -> Dict:
    """``{metric: {"a vs b": paired_difference(a, b)}}`` over every pair of methods, in the order given"""
    names = list(vectors_by_method)
    out = {}
    for metric in metrics:
        if not all(metric in vectors_by_method[n] for n in names):
            continue
        out[metric] = {f"{a} vs {b}": paired_difference(vectors_by_method[a][metric], vectors_by_method[b][metric])
                       for i, a in enumerate(names) for b in names[i + 1:]}
    return out
