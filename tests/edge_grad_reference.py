"""The contract of ``RGCN_MODE_WEIGHT_GRAD`` / ``RGCN_MODE_MEAN_GRAD`` (``include/rgcn_hip.h``) restated on the CPU (no
test lives here): dots and segment sums in float64 from the fp32 inputs - in int64 for integer tables - and the forward
error bounds the GPU tests hold the kernel to.  The bounds are worst cases for ANY summation order, derived from the
formats, not tuned: with ``u = 2^-24`` and ``gamma_n = n u / (1 - n u)``,

  plain   |err[p]| <= eps[p] = gamma_d * A[p],                       A[p] = sum_k |agg[s, k] * x[col[p], k]|
  mean    |err[p]| <= (eps[p] + (sum_q eps[q] + gamma_c sum_q |D[q]|) / c + 4 u (|D[p]| + sum_q |D[q]| / c)) / c

``c`` the segment's length, ``D`` the exact dots, the sums over the segment's edges q: the dot's own error, the error of
``S`` (its terms' errors plus ``c`` additions), and four roundings - ``1 / c``, ``S * w``, the subtraction, the last
product - each relative to a quantity below ``|D[p]| + sum |D| / c``."""
import torch

U = 2.0 ** -24


def gamma(n):
    n = torch.as_tensor(n, dtype=torch.float64)
    return n * U / (1.0 - n * U)


def csr(key, other, rel, n_key, num_relations):
    """the bucketed order of one direction: segments ``(key, rel)``, the columns of a segment in column order ->
    ``(rowptr int64 [n_key * R + 1], col int64 [E], perm int64 [E], seg int64 [E])``"""
    flat = key * num_relations + rel
    perm = torch.argsort(flat, stable=True)
    seg = flat[perm]
    rowptr = torch.zeros(n_key * num_relations + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(flat, minlength=n_key * num_relations), 0)
    return rowptr, other[perm].contiguous(), perm, seg


def segments_of(rowptr):
    """int64 [E]: the segment of every position"""
    return torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr[1:] - rowptr[:-1])


def _rows(gagg, d):
    return gagg.reshape(-1, d)


def plain(rowptr, col, x, gagg):
    """-> (D float64 [E], eps float64 [E]): the exact dots of fp32 operands and their bound"""
    d = x.size(1)
    prod = _rows(gagg, d).double()[segments_of(rowptr)] * x.double()[col.long()]
    return prod.sum(1), gamma(d) * prod.abs().sum(1)


def plain_int(rowptr, col, x, gagg):
    """int64 [E]: the dots of integer tables"""
    d = x.size(1)
    return (_rows(gagg, d).long()[segments_of(rowptr)] * x.long()[col.long()]).sum(1)


def _segment_sum(values, seg, num_segments):
    return torch.zeros(num_segments, dtype=values.dtype).index_add_(0, seg, values)


def mean(rowptr, col, x, gagg):
    """-> (out float64 [E], bound float64 [E]): ``(D - S / c) / c`` and its bound"""
    dots, eps = plain(rowptr, col, x, gagg)
    seg, ns = segments_of(rowptr), rowptr.numel() - 1
    c = (rowptr[1:] - rowptr[:-1]).double().clamp(min=1)[seg]
    s = _segment_sum(dots, seg, ns)[seg]
    sabs, seps = _segment_sum(dots.abs(), seg, ns)[seg], _segment_sum(eps, seg, ns)[seg]
    bound = (eps + (seps + gamma(c) * sabs) / c + 4 * U * (dots.abs() + sabs / c)) / c
    return (dots - s / c) / c, bound


def mean_int_pow2(rowptr, col, x, gagg):
    """-> (out float32 [E], exact bool [E]): the mean mode of integer tables where it is exact in fp32 - the segments
    whose length is a power of two (every operation is then a scaling or a sum of few-bit numbers; the caller keeps the
    products and sums inside 2^24) - computed in float64, where it is exact too"""
    dots = plain_int(rowptr, col, x, gagg)
    seg, ns = segments_of(rowptr), rowptr.numel() - 1
    length = rowptr[1:] - rowptr[:-1]
    c = length.clamp(min=1)[seg]
    s = _segment_sum(dots, seg, ns)[seg]
    out = (dots.double() - s.double() / c.double()) / c.double()
    return out.float(), ((length & (length - 1)) == 0)[seg]
