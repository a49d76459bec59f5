"""The resampling contract of ``include/rgcn_resample.h`` restated on the host: the Poisson(1) weights from Philox words,
the ROC / PR statistics of a list in descending score order and the ranking sums.  Integers are Python integers and the
two real-valued sums are ``fractions.Fraction``: what the device must equal, and what its doubles are bounded against.
A plain module, not a test."""
from fractions import Fraction

import numpy as np

M32 = 0xFFFFFFFF
STREAM = 0x52534D50                      # RGCN_RESAMPLE_STREAM
# RGCN_RESAMPLE_THRESHOLDS: floor(2^32 * sum_{j <= k} e^-1 / j!), k = 0 .. 12
THRESHOLDS = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276,
              4294962463, 4294966817, 4294967252, 4294967292, 4294967295)


def philox4x32_10(ctr, key):
    """Philox4x32 with ten rounds (Salmon et al., SC'11) on Python ints: ctr 4 words, key 2 words -> 4 words"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def philox4x32_10_np(c0, c1, c2, c3, key):
    """the same on uint64 arrays that hold 32-bit words (a product of two words fits in 64 bits)"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(M32) for c in (c0, c1, c2, c3))
    k0, k1 = key
    m, s = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def weight_of_word(word):
    return sum(1 for t in THRESHOLDS if word >= t)


def weight(unit, replicate, seed):
    """the rule, one unit at a time"""
    if replicate == 0:
        return 1
    seed &= 0xFFFFFFFFFFFFFFFF
    c = philox4x32_10((unit, (replicate - 1) >> 2, STREAM, 0), (seed & M32, seed >> 32))
    return weight_of_word(c[(replicate - 1) & 3])


def weights(units, replicate, seed):
    """int64 array: the weight of every unit id of ``units`` in one replicate"""
    units = np.asarray(units, dtype=np.int64)
    if replicate == 0:
        return np.ones(units.shape, dtype=np.int64)
    seed &= 0xFFFFFFFFFFFFFFFF
    zeros = np.zeros(units.shape, dtype=np.uint64)
    c = philox4x32_10_np(units.astype(np.uint64), zeros + np.uint64((replicate - 1) >> 2), zeros + np.uint64(STREAM), zeros,
                         (seed & M32, seed >> 32))
    word = c[(replicate - 1) & 3]
    return (word[..., None] >= np.asarray(THRESHOLDS, dtype=np.uint64)).sum(axis=-1).astype(np.int64)


def sort_samples(scores, labels, units=None):
    """what the wrapper hands the kernel: NaN -> -inf, a stable descending order, tie_end and the order itself"""
    s = np.asarray(scores, dtype=np.float64).copy()
    s[np.isnan(s)] = -np.inf
    order = np.argsort(-s, kind="stable")
    s = s[order]
    tie_end = np.ones(s.size, dtype=bool)
    tie_end[:-1] = s[:-1] != s[1:]
    units = np.arange(s.size) if units is None else np.asarray(units)
    return s, np.asarray(labels)[order].astype(np.int64), units[order].astype(np.int64), tie_end


def exact_sum(terms):
    """the exact sum of ``(numerator, denominator)`` pairs as one Fraction: numerators are added per denominator first and
    the denominators multiplied up without reducing on the way (thousands of distinct ones: one gcd at the end)"""
    by_den = {}
    for a, b in terms:
        if a:
            by_den[b] = by_den.get(b, 0) + a
    num, den = 0, 1
    for b, a in by_den.items():
        num, den = num * b + a * den, den * b
    return Fraction(num, den)


def curves_sorted(s, y, u, tie_end, threshold, replicate, seed):
    """``curves`` on samples that ``sort_samples`` has put in order"""
    w = weights(u, replicate, seed).tolist()
    y, tie_end = list(y), list(tie_end)
    cut = int((np.asarray(s) >= threshold).sum())
    tp_b = fp_b = p = q = auc2 = tp = fp = 0
    terms = []
    for i in range(len(w)):
        if y[i]:
            p += w[i]
        else:
            q += w[i]
        if i == cut - 1:
            tp, fp = tp_b + p, fp_b + q
        if tie_end[i]:
            auc2 += q * (2 * tp_b + p)
            terms.append((p * (tp_b + p), tp_b + p + fp_b + q))
            tp_b, fp_b, p, q = tp_b + p, fp_b + q, 0, 0
    wp, wn = tp_b, fp_b
    defined = wp > 0 and wn > 0
    return {"wp": wp, "wn": wn, "auc2": auc2 if defined else 0, "ap": exact_sum(terms) / wp if defined else Fraction(0),
            "tp": tp, "fp": fp}


def curves(scores, labels, units, threshold, replicate, seed):
    """-> dict of wp, wn, auc2, tp, fp (ints) and ap (a Fraction; 0 when a class has no weight) of ONE replicate"""
    return curves_sorted(*sort_samples(scores, labels, units), threshold, replicate, seed)


def rank_sums(ranks, units, k_values, replicate, seed):
    """-> dict of w_sum, rank_sum, hits (list) as ints and rr_sum as a Fraction of ONE replicate"""
    w = weights(units, replicate, seed).tolist()
    ranks = [int(r) for r in ranks]
    return {"w_sum": sum(w), "rank_sum": sum(a * r for a, r in zip(w, ranks)),
            "hits": [sum(a for a, r in zip(w, ranks) if r <= k) for k in k_values],
            "rr_sum": exact_sum(zip(w, ranks))}
