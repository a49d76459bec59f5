"""The two contracts of the learned edge masks restated on the CPU (no test lives here).

1. The mask draw, ``RGCN_EDGE_DROPOUT_MASK`` of ``rgcn_edge_dropout_draw`` (``include/rgcn_edge_dropout.h``), bit for bit
   in numpy float32: ``m(e) = hidden(e) ? 0 : mask[e]``, ``M[s]`` the segment's sum in the FIXED order of the header's
   words (``fixed_sum`` below is written from those words, not from the kernel), ``w = M > 0 ? m / M : 0`` by one IEEE
   division, ``k[s]`` the number of positions with ``m > 0``.
2. ``RGCN_MODE_LOG_WEIGHT_GRAD`` of ``rgcn_aggregate_ex`` (``include/rgcn_hip.h``): ``out[p] = w[p] == 0 ? +0 :
   w[p] * (dot[p] - S[s])``, ``S[s] = sum_q fl(w[q] * dot[q])``, in float64 from the fp32 operands, with a worst-case
   forward bound for ANY summation order, derived from the operation count and not tuned.  With ``u = 2^-24``,
   ``gamma_n = n u / (1 - n u)``, ``D`` the exact dots, ``eps`` the dots' own bound (``edge_grad_reference.plain``), ``c``
   the segment's length and the sums over the segment's edges q:

     errS   <= (1 + gamma_(c+1)) sum_q |w[q]| eps[q] + gamma_(c+1) sum_q |w[q] D[q]|
               (every term carries its dot's error and one rounded product, the sum c rounded additions)
     |err[p]| <= |w[p]| ((eps[p] + errS) (1 + 3 u) + 3 u (|D[p]| + sum_q |w[q] D[q]|))
               (the rounded subtraction and the rounded last product: (1 + u)^2 <= 1 + 3 u, |D - S| <= |D| + sum |w D|)
"""
import numpy as np
import torch

import edge_grad_reference as G

U = G.U
F32 = np.float32


def fixed_sum(v):
    """the FIXED order of rgcn_hip.h / rgcn_edge_dropout.h over the float32 values of one segment, in float32"""
    v = np.asarray(v, dtype=F32)
    n = v.shape[0]
    if n <= 64:
        part = np.zeros(8, dtype=F32)                          # P_j = v[j] + v[j + 8] + v[j + 16] + ... from +0.0f
        for first in range(0, n, 8):
            chunk = v[first:first + 8]
            part[:chunk.shape[0]] = part[:chunk.shape[0]] + chunk
        return F32(F32(F32(part[0] + part[4]) + F32(part[2] + part[6])) + F32(F32(part[1] + part[5]) + F32(part[3] + part[7])))
    t = np.zeros(256, dtype=F32)                               # T_t = v[t] + v[t + 256] + ... from +0.0f
    for first in range(0, n, 256):
        chunk = v[first:first + 256]
        t[:chunk.shape[0]] = t[:chunk.shape[0]] + chunk
    t = t.reshape(4, 64)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):                           # entry l becomes entry l + entry (l ^ offset)
        t = (t + t[:, lanes ^ off]).astype(F32)
    w = t[:, 0]
    return F32(F32(F32(w[0] + w[1]) + w[2]) + w[3])


def mask_draw(rowptr, perm, mask, hidden=None):
    """the mask draw over the forward structure (``rowptr`` [N * R + 1], ``perm`` [E]: the original column of every forward
    position) -> ``(w_col float32 [E] by ORIGINAL column, M float32 [N * R], k int32 [N * R])``; the weight of a column
    is the same number in both directions"""
    rowptr, perm = np.asarray(rowptr, dtype=np.int64), np.asarray(perm, dtype=np.int64)
    mask = np.asarray(mask, dtype=F32)
    m_col = mask.copy()
    if hidden is not None:
        m_col[np.asarray(hidden, dtype=bool)] = F32(0)         # a select: a hidden NaN is 0
    ns = rowptr.shape[0] - 1
    big_m, k, w_col = np.zeros(ns, dtype=F32), np.zeros(ns, dtype=np.int32), np.zeros(mask.shape[0], dtype=F32)
    with np.errstate(all="ignore"):
        for s in range(ns):
            b, e = int(rowptr[s]), int(rowptr[s + 1])
            if e == b:
                continue
            m = m_col[perm[b:e]]
            big_m[s] = fixed_sum(m)
            k[s] = int((m > 0).sum())
            if big_m[s] > 0:                                   # NaN > 0 is false
                w_col[perm[b:e]] = (m / big_m[s]).astype(F32)
    return w_col, big_m, k


def log_weight_grad(rowptr, col, w, x, gagg):
    """-> (out float64 [E], bound float64 [E]) in the direction's bucketed order; ``w`` float32 [E] in that order"""
    dots, eps = G.plain(rowptr, col, x, gagg)
    seg, ns = G.segments_of(rowptr), rowptr.numel() - 1
    w = torch.as_tensor(w).double()
    c = (rowptr[1:] - rowptr[:-1]).double().clamp(min=1)[seg]
    s = G._segment_sum(w * dots, seg, ns)[seg]
    sabs = G._segment_sum((w * dots).abs(), seg, ns)[seg]
    seps = G._segment_sum(w.abs() * eps, seg, ns)[seg]
    g1 = G.gamma(c + 1)
    err_s = (1 + g1) * seps + g1 * sabs
    bound = w.abs() * ((eps + err_s) * (1 + 3 * U) + 3 * U * (dots.abs() + sabs))
    out = torch.where(w == 0, torch.zeros_like(dots), w * (dots - s))
    return out, bound
