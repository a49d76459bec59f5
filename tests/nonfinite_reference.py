"""Float64 restatements of the training path's operations on inputs that hold NaN or infinities (torch on the CPU,
no device code): for every operation the value under dense IEEE arithmetic and two boolean maps,

* ``must`` - the entries that are non-finite under SPARSE semantics: an empty (row, relation) segment of an aggregate
  contributes nothing to a product, even against a NaN weight;
* ``may`` - the entries that are non-finite under DENSE semantics (``0 * NaN = NaN``, what ``h @ weight[r]`` computes).

``must`` is a subset of ``may``; they differ only where an empty segment meets a non-finite weight (or, in a
parameter gradient, a non-finite cotangent row).  The device has to poison every ``must`` entry and may poison nothing
outside ``may`` (include/rgcn_hip.h, "Non-finite values").

A library GEMM is free to skip or reorder products, so no product that involves a non-finite operand goes through one:
``pmatmul`` multiplies the finite parts with ``@`` and forms every row and column that a poisoned entry reaches
term by term.  tests/test_nonfinite_host.py checks the maps against torch's own ops."""
import math
from collections import namedtuple

import torch

F64 = torch.float64
KINDS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
PLACEMENTS = ["first_row", "last_row", "interior_row", "first_col", "last_col"]

Ref = namedtuple("Ref", "value must may")          # value: dense float64; must / may: bool maps of its shape


def nonfinite(t):
    return ~torch.isfinite(t)


def _ref(dense, sparse):
    return Ref(dense, nonfinite(sparse), nonfinite(dense))


# ---------------------------------------------------------------------------------------------- placing poison
def poison_index(rows, cols, placement):
    """the (row, column) of a [rows, cols] matrix that a placement names; the free coordinate sits mid-way"""
    mr, mc = rows // 2, cols // 2
    return {"first_row": (0, mc), "last_row": (rows - 1, mc), "interior_row": (mr, mc), "first_col": (mr, 0),
            "last_col": (mr, cols - 1)}[placement]


def place(t, placement, kind, block=None):
    """a copy of ``t`` with ONE entry set to the poison ``kind`` -> (copy, index tuple).  1-D: first / last / middle
    entry; 2-D: ``poison_index``; 3-D ``[R, a, b]``: ``poison_index`` inside relation ``block`` (default: the last)"""
    out = t.clone()
    v = KINDS[kind]
    if t.dim() == 1:
        i = {"first_row": 0, "first_col": 0, "last_row": t.numel() - 1, "last_col": t.numel() - 1}.get(placement, t.numel() // 2)
        idx = (i,)
    elif t.dim() == 2:
        idx = poison_index(t.size(0), t.size(1), placement)
    else:
        idx = (t.size(0) - 1 if block is None else block,) + poison_index(t.size(1), t.size(2), placement)
    out[idx] = v
    return out, idx


# ---------------------------------------------------------------------------------------------- products
def pmatmul(a, b, live=None):
    """``a @ b`` in float64 -> (dense, sparse).  ``live`` (bool, a's shape; default all True): the entries of ``a`` that
    exist under sparse semantics - a term ``a[i, k] * b[k, j]`` with ``live[i, k]`` False is left out of ``sparse``."""
    a, b = a.to(F64), b.to(F64)
    fa, fb = torch.isfinite(a), torch.isfinite(b)
    zero = torch.zeros((), dtype=F64)
    dense = torch.where(fa, a, zero) @ torch.where(fb, b, zero)
    sparse = dense.clone()
    for i in (~fa).any(1).nonzero().flatten().tolist():           # rows a poisoned entry of `a` reaches
        terms = a[i].unsqueeze(1) * b
        dense[i] = terms.sum(0)
        sparse[i] = terms.sum(0) if live is None else torch.where(live[i].unsqueeze(1), terms, zero).sum(0)
    for j in (~fb).any(0).nonzero().flatten().tolist():           # columns a poisoned entry of `b` reaches
        terms = a * b[:, j].unsqueeze(0)
        dense[:, j] = terms.sum(1)
        sparse[:, j] = terms.sum(1) if live is None else torch.where(live, terms, zero).sum(1)
    return dense, sparse


def relu(z):
    """``relu(NaN) = NaN``, ``relu(+inf) = +inf``, ``relu(-inf) = 0``"""
    return torch.where(z != z, z, z.clamp(min=0))


def select(mask, z):
    """the backward epilogues' masks are selects: a position whose mask is not > 0 (NaN included) is exactly 0"""
    return torch.where(mask > 0, z, torch.zeros((), dtype=z.dtype))


def _live_columns(nonempty, d, extra, rows):
    """[rows, R * d + extra] bool from ``nonempty`` [rows, R] (None: everything exists); the ``extra`` columns of the
    dense operand (x / g against root) always exist"""
    if nonempty is None:
        return None
    return torch.cat([nonempty.repeat_interleave(d, 1), torch.ones(rows, extra, dtype=torch.bool)], 1)


def wcat(w, root):
    r, d_in, d_out = w.shape
    m = w.reshape(r * d_in, d_out)
    return torch.cat([m, root]) if root is not None else m


def wcat_t(w, root):
    r, d_in, d_out = w.shape
    m = w.transpose(1, 2).reshape(r * d_out, d_in)
    return torch.cat([m, root.t()]) if root is not None else m


def transform_fwd(agg, x, w, root=None, bias=None, relu_on=False, nonempty=None):
    a = torch.cat([agg, x], 1) if root is not None else agg
    live = _live_columns(nonempty, w.size(1), x.size(1) if root is not None else 0, agg.size(0))
    dense, sparse = pmatmul(a, wcat(w, root), live)
    if bias is not None:
        dense, sparse = dense + bias.to(F64), sparse + bias.to(F64)
    if relu_on:
        dense, sparse = relu(dense), relu(sparse)
    return _ref(dense, sparse)


def transform_bwd_input(gagg, g, w, root=None, mask=None, out_scale=1.0, nonempty=None):
    a = torch.cat([gagg, g], 1) if root is not None else gagg
    live = _live_columns(nonempty, w.size(2), g.size(1) if root is not None else 0, gagg.size(0))
    dense, sparse = pmatmul(a, wcat_t(w, root), live)
    if mask is not None:
        dense, sparse = select(mask, dense), select(mask, sparse)
    return _ref(dense * out_scale, sparse * out_scale)


def transform_first(g, w, root=None):
    """``T = g @ [W_0^T | ... | root^T]``: a dense product, ``must == may``"""
    dense, sparse = pmatmul(g, wcat(w, root).t())
    return _ref(dense, sparse)


def transform_bwd_params(agg, x, g, num_relations, nonempty=None):
    """-> (weight [R, d_in, d_out], root, bias) Refs; the reduction runs over the rows, so a row's empty segments are
    the terms sparse semantics leaves out"""
    d_in, d_out = x.size(1), g.size(1)
    live = _live_columns(nonempty, d_in, 0, agg.size(0))
    gw = pmatmul(agg.t(), g, None if live is None else live.t())
    gr = pmatmul(x.t(), g)
    gb = g.to(F64).sum(0)
    shape = (num_relations, d_in, d_out)
    return (_ref(gw[0].view(shape), gw[1].view(shape)), _ref(*gr), _ref(gb, gb))


def basis_compose(comp, basis):
    b = basis.size(0)
    dense, sparse = pmatmul(comp, basis.reshape(b, -1))
    shape = (comp.size(0),) + tuple(basis.shape[1:])
    return _ref(dense.view(shape), sparse.view(shape))


def basis_compose_bwd(gw, comp, basis):
    """-> (grad_comp [R, B], grad_basis [B, d_in, d_out]) Refs"""
    r, b = comp.shape
    gc = pmatmul(gw.reshape(r, -1), basis.reshape(b, -1).t())
    gb = pmatmul(comp.t(), gw.reshape(r, -1))
    return _ref(*gc), _ref(gb[0].view(basis.shape), gb[1].view(basis.shape))


# ---------------------------------------------------------------------------------------------- gathers
def segment_counts(key, rel, n, r):
    return torch.bincount(key * r + rel, minlength=n * r)


def aggregate(table, key, other, rel, n, r, transposed_counts=None):
    """[n, r * d] float64: per (key, rel) segment the mean of rows ``table[other]``; with ``transposed_counts`` (the
    length of the FORWARD segment each edge belongs to, per edge) the weighted sum ``sum table[other] / count`` instead.
    Sums are plain additions in edge order: a segment is non-finite exactly when it holds an edge to a poisoned
    entry's row, and an empty segment is exactly zero."""
    t = table.to(F64)
    d = t.size(1)
    seg = key * r + rel
    rows = t[other]
    if transposed_counts is not None:
        rows = rows / transposed_counts.to(F64).unsqueeze(1)
    out = torch.zeros(n * r, d, dtype=F64).index_add_(0, seg, rows)
    if transposed_counts is None:
        out = out / segment_counts(key, rel, n, r).clamp(min=1).to(F64).unsqueeze(1)
    return out.view(n, r * d)


def graph_aggregate(table, ei, et, n, r, transposed=False):
    """the two gathers of a layer over a graph ``ei = [src; dst]``"""
    src, dst = ei[0], ei[1]
    if not transposed:
        return aggregate(table, dst, src, et, n, r)
    cnt = segment_counts(dst, et, n, r)[dst * r + et]
    return aggregate(table, src, dst, et, n, r, transposed_counts=cnt)


def nonempty_segments(ei, et, n, r, transposed=False):
    key = ei[0] if transposed else ei[1]
    return (segment_counts(key, et, n, r) > 0).view(n, r)


# ---------------------------------------------------------------------------------------------- fp16 operand meaning
def r16_scaled(t):
    """``t`` rounded to fp16 under its tensor's power-of-two scale (largest magnitude into [2^14, 2^15)), the meaning of
    an operand of the one-pass fp16 GEMMs.  The maximum ignores NaN (the device's maxima are fmaxf chains); an infinite
    or zero maximum gives scale 1."""
    t = t.to(F64)
    mags = t.abs()[~torch.isnan(t)]
    amax = float(mags.max()) if mags.numel() else 0.0
    e = 0 if amax == 0.0 or math.isinf(amax) else max(-100, min(100, 14 - math.floor(math.log2(amax))))
    return (t * 2.0 ** e).to(torch.float32).half().to(F64) * 2.0 ** (-e)


# ---------------------------------------------------------------------------------------------- the encoder
def _encoder_pass(emb, conv1, conv2, ei, et, cot, relu_mask, sparse):
    n, r = emb.size(0), conv1["weight"].size(0)
    ne_f, ne_t = nonempty_segments(ei, et, n, r), nonempty_segments(ei, et, n, r, True)
    pick = 1 if sparse else 0

    def layer_fwd(x, c, relu_on):
        has_root = c.get("root") is not None
        agg = graph_aggregate(x, ei, et, n, r)
        a = torch.cat([agg, x], 1) if has_root else agg
        live = _live_columns(ne_f, x.size(1), x.size(1) if has_root else 0, n)
        z = pmatmul(a, wcat(c["weight"], c.get("root")), live)[pick]
        if c.get("bias") is not None:
            z = z + c["bias"].to(F64)
        return a, live, relu(z) if relu_on else z

    def layer_bwd(g, a, live, c):
        has_root = c.get("root") is not None
        d_in, d_out = c["weight"].size(1), c["weight"].size(2)
        gwcat = pmatmul(a.t(), g, live.t())[pick]
        grads = {"weight": gwcat[: r * d_in].reshape(r, d_in, d_out)}
        if has_root:
            grads["root"] = gwcat[r * d_in:]
        if c.get("bias") is not None:
            grads["bias"] = g.sum(0)
        gagg = graph_aggregate(g, ei, et, n, r, True)
        ga = torch.cat([gagg, g], 1) if has_root else gagg
        live_t = _live_columns(ne_t, d_out, d_out if has_root else 0, n)
        return grads, pmatmul(ga, wcat_t(c["weight"], c.get("root")), live_t)[pick]

    a1, live1, h = layer_fwd(emb.to(F64), conv1, True)
    a2, live2, out = layer_fwd(h, conv2, False)
    g2, gh = layer_bwd(cot.to(F64), a2, live2, conv2)
    g1, gx = layer_bwd(select(relu_mask.to(F64), gh), a1, live1, conv1)
    res = {"out": out, "h": h, "emb": gx}
    res.update({f"conv1.{k}": v for k, v in g1.items()})
    res.update({f"conv2.{k}": v for k, v in g2.items()})
    return res


def encoder(emb, conv1, conv2, ei, et, cot, relu_mask):
    """conv1 -> ReLU -> conv2 and its backward for the cotangent ``cot``, every product a ``pmatmul``, once under dense
    and once under sparse semantics; ``relu_mask`` [N, hidden] bool: the ReLU decisions of the backward (the device's
    ``h > 0``), applied as a select.  convN: dicts of weight / root / bias (plain weights).
    -> dict name -> Ref for "out", "h", "emb" (its gradient) and "conv1.weight" ... "conv2.bias" (gradients)"""
    dense = _encoder_pass(emb, conv1, conv2, ei, et, cot, relu_mask, False)
    sparse = _encoder_pass(emb, conv1, conv2, ei, et, cot, relu_mask, True)
    return {k: _ref(dense[k], sparse[k]) for k in dense}


# ---------------------------------------------------------------------------------------------- the DistMult / BCE head
def rows_of(mat, idx):
    mat = mat.to(F64)
    return mat if idx is None else mat[idx]


def distmult_scores(h, hi, t, ti, r, ri):
    """-> (scores [B] float64, sum of the terms' magnitudes [B]); elementwise products, a plain sum"""
    term = rows_of(h, hi) * rows_of(r, ri) * rows_of(t, ti)
    return term.sum(1), term.abs().sum(1)


def bce_with_logits(s, y):
    """per sample, the way aten (and the kernel) evaluates it: ``(1 - y) s - (min(s, 0) - log1p(exp(-|s|)))``"""
    s, y = s.to(F64), y.to(F64)
    return (1 - y) * s - (torch.where(s != s, s, s.clamp(max=0)) - torch.log1p(torch.exp(-s.abs())))


def bce_coefficient(grad_mean, s, y):
    s, y = s.to(F64), y.to(F64)
    return float(grad_mean) * (1.0 / (1.0 + torch.exp(-s)) - y) / s.numel()


def segment_sum(rows, idx, num_rows):
    return torch.zeros(num_rows, rows.size(1), dtype=F64).index_add_(0, idx, rows.to(F64))


# ---------------------------------------------------------------------------------------------- clip + Adam
def clip_adam_step(params, grads, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay=0.0, adamw=False,
                   max_norm=0.0):
    """``clip_grad_norm_(params, max_norm)`` (``max_norm <= 0``: none) + one Adam / AdamW step in float64, written out:
    -> (params, exp_avg, exp_avg_sq, total_norm | None).  The coefficient is ``clamp(max_norm / (total + 1e-6), max=1)``,
    a clamp that keeps NaN."""
    grads = [g.to(F64) for g in grads]
    total = None
    if max_norm > 0:
        total = torch.sqrt(sum((g * g).sum() for g in grads))
        c = max_norm / (total + 1e-6)
        coef = torch.where(c > 1.0, torch.ones((), dtype=F64), c)
        grads = [g * coef for g in grads]
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    out_p, out_m, out_v = [], [], []
    for p, g, m, v in zip(params, grads, exp_avg, exp_avg_sq):
        p, m, v = p.to(F64), m.to(F64), v.to(F64)
        if adamw:
            p = p * (1.0 - lr * weight_decay)
        elif weight_decay != 0.0:
            g = g + weight_decay * p
        m = m + (g - m) * (1.0 - beta1)
        v = beta2 * v + (1.0 - beta2) * g * g
        p = p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps))
        out_p.append(p)
        out_m.append(m)
        out_v.append(v)
    return out_p, out_m, out_v, total
