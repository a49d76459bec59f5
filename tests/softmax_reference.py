"""The contract of ``include/rgcn_softmax.h`` restated in float64 numpy, and the forward-error bounds the header
derives, computed from the data - none is a constant picked here.

Everything takes the fp32 operands the device gets (torch CPU tensors or arrays) and the masks as the int32 bit words
the kernels read (``allow [C, W]`` with ``query_class [B]``, ``exclude [B, W]``; entity n is bit ``n & 31`` of word
``n >> 5``).
"""
import math

import numpy as np

U = 2.0 ** -24                    # unit roundoff of fp32
TILE, ROW_TILE, MAX_SLICES, CUS = 128, 64, 64, 256


def _np(t, dtype=None):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return a.astype(dtype) if dtype is not None else a


def plan(batch, n, slices=0):
    """``(tiles, tiles_per_slice, S)``: the header's slice rule"""
    tiles = -(-n // TILE)
    row_tiles = -(-batch // ROW_TILE)
    want = slices if slices > 0 else (1 if row_tiles >= CUS // 2 else -(-CUS // row_tiles))
    want = max(1, min(want, tiles, MAX_SLICES))
    per = -(-tiles // want)
    return tiles, per, -(-tiles // per)


def unpack_bits(words, n):
    """int32 ``[R, W]`` -> bool ``[R, n]``"""
    w = _np(words).astype(np.int64) & 0xFFFFFFFF
    cols = np.arange(n)
    return ((w[:, cols >> 5] >> (cols & 31)) & 1).astype(bool)


def pack_bits(dense):
    """bool ``[R, n]`` -> int32 ``[R, W]`` (numpy)"""
    dense = np.asarray(dense, dtype=bool)
    r, n = dense.shape
    w = (n + 31) // 32
    padded = np.zeros((r, w * 32), dtype=np.uint64)
    padded[:, :n] = dense
    words = (padded.reshape(r, w, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2)
    return words.astype(np.uint32).view(np.int32)


def eligible(batch, n, target, allow=None, query_class=None, exclude=None):
    """bool ``[B, N]``: allowed by the query's class (a class outside ``[0, C)`` allows nothing), not struck, and the
    target always"""
    ok = np.ones((batch, n), dtype=bool)
    if allow is not None:
        rows = unpack_bits(allow, n)
        cls = _np(query_class).astype(np.int64)
        inside = (cls >= 0) & (cls < rows.shape[0])
        ok &= rows[np.where(inside, cls, 0)] & inside[:, None]
    if exclude is not None:
        ok &= ~unpack_bits(exclude, n)
    ok[np.arange(batch), _np(target)] = True
    return ok


def scores(q, emb):
    return _np(q, np.float64) @ _np(emb, np.float64).T


def forward(s, ok, target):
    """``lse, true_score, row_max, loss, hit`` of a float64 score matrix in the header's grouping: the maximum is
    subtracted, an eligible -inf is an exact zero, NaN and +inf do what float64 does with them"""
    b = s.shape[0]
    with np.errstate(all="ignore"):
        masked = np.where(ok, s, -np.inf)
        m = masked.max(axis=1)                                     # numpy's max keeps a NaN
        terms = np.where(masked == -np.inf, 0.0, np.exp(masked - m[:, None]))
        lse = m + np.log(terms.sum(axis=1))
        ts = s[np.arange(b), _np(target)]
        return {"lse": lse, "true_score": ts, "row_max": m, "loss": lse - ts, "hit": ts >= m}


def coefficients(g, s, lse, ok, target):
    """``c[b, n] = g[b] ([n eligible] exp(s - lse) - [n == target])``; an ineligible entry is an exact 0"""
    b = s.shape[0]
    with np.errstate(all="ignore"):
        p = np.where(ok, np.exp(s - lse[:, None]), 0.0)
    onehot = np.zeros_like(p)
    onehot[np.arange(b), _np(target)] = 1.0
    return _np(g, np.float64)[:, None] * (p - onehot), p


def gradients(c, q, emb):
    with np.errstate(all="ignore"):
        return c @ _np(emb, np.float64), c.T @ _np(q, np.float64)


# ------------------------------------------------------------------------------------------------- bounds
def gamma(k):
    return k * U / (1.0 - k * U)


def score_bound(q, emb):
    """``|s - s64| <= gamma_d sum_k |q_k| |E_nk|`` (any order of the d products)"""
    d = _np(q).shape[1]
    return gamma(d) * (np.abs(_np(q, np.float64)) @ np.abs(_np(emb, np.float64)).T)


def chain_steps(batch, n, slices=0):
    """float32 merge steps on the longest chain of the device's sum: the tiles of a slice, the 5-step butterfly, the two
    wave columns (the slices merge in float64)"""
    return plan(batch, n, slices)[1] + 6


def lse_bound(sb, ok, lse64, steps):
    """``|lse - lse64| <= max_n |s - s64| + (5 T + 2 + ln N) u + u |lse64|``: log-sum-exp is 1-Lipschitz in the sup
    norm; every one of the T float32 steps adds at most five roundings to the sum's relative error (the factor's expf at 1
    ulp = 2 u, its product, the pair's sum, the step's sum); the rounding of ``s - m`` moves a term by ``|s - m| u``
    relatively, which weighted by the terms themselves is at most ``(ln N) u`` (an entropy); the slices merge and the
    logarithm is taken in float64, whose roundings the 2 u cover many times over, and ``m + log(sum)`` is rounded to
    float32 once."""
    n = ok.shape[1]
    delta = np.where(ok, sb, 0.0).max(axis=1)
    return delta + (5 * steps + 2 + math.log(n)) * U + U * np.abs(lse64)


def loss_bound(lb, sb, target, loss64):
    return lb + sb[np.arange(sb.shape[0]), _np(target)] + U * np.abs(loss64)


def coefficient_bound(g, s64, lse64, p64, sb, lb):
    """``|c - c64|``: ``p = exp(s - lse)`` moves by ``p64 (e^x - 1)`` with ``x = |ds| + |dlse| + u |s - lse| + 2 u`` (the
    exp at 1 ulp), then one rounding each for the subtraction and the product with g"""
    with np.errstate(all="ignore"):
        x = sb + lb[:, None] + U * np.abs(s64 - lse64[:, None]) + 2 * U
        dp = p64 * np.expm1(np.where(p64 > 0, x, 0.0))
    return np.abs(_np(g, np.float64))[:, None] * (dp + 2 * U * (p64 + 1.0))


def gradient_bounds(c64, dc, q, emb, extra_terms=0):
    """``(|dq - dq64|, |dE - dE64|)``: the coefficient's error carried through the product, plus ``gamma_K`` of the
    absolute product for a sum of K terms in any order (K = N + the slices for dq, B + the chunks for dE)"""
    aq, ae = np.abs(_np(q, np.float64)), np.abs(_np(emb, np.float64))
    b, n = c64.shape
    ac = np.abs(c64)
    dq = dc @ ae + gamma(n + MAX_SLICES + extra_terms) * ((ac + dc) @ ae)
    de = dc.T @ aq + gamma(b + extra_terms + 1) * ((ac + dc).T @ aq)
    return dq, de
