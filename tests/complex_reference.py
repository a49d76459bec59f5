"""The ComplEx head's contract (``include/rgcn_complex.h``) in float64, with the header's grouping of the products.

A row of width ``d`` is ``m = d / 2`` complex numbers: columns ``[0, m)`` real parts, ``[m, d)`` imaginary parts.

    score(h, r, t) = sum_j (h_re r_re - h_im r_im)_j t_re_j + (h_re r_im + h_im r_re)_j t_im_j

``Want`` keeps, per element of a gradient buffer, what ``test_head_edges.Want`` keeps - the float64 value, the sum of the
absolute terms and the number of terms - for elements of the form ``sum_occ g (a b + s c e)`` with ``s = +-1``.
"""
import torch
import torch.nn as nn

U = 2.0 ** -24


def halves(x):
    m = x.size(-1) // 2
    return x[..., :m], x[..., m:]


def rows(mat, idx):
    """the [B, d] float64 rows an operand contributes: gathered, or row b its own"""
    mat = mat.double()
    return mat if idx is None else mat[idx]


def tail_query(h, r):
    """q with score(h, r, n) = <q, E[n]>"""
    (h_re, h_im), (r_re, r_im) = halves(h), halves(r)
    return torch.cat([h_re * r_re - h_im * r_im, h_re * r_im + h_im * r_re], dim=-1)


def head_query(t, r):
    """q with score(n, r, t) = <q, E[n]>: the tail rotated by the conjugate of the relation"""
    (t_re, t_im), (r_re, r_im) = halves(t), halves(r)
    return torch.cat([r_re * t_re + r_im * t_im, r_re * t_im - r_im * t_re], dim=-1)


def query_magnitude(x, r, side):
    """per entry of a query row ``a b +- c e``: ``|a b| + |c e|``"""
    (x_re, x_im), (r_re, r_im) = halves(x), halves(r)
    if side == "tail":
        return torch.cat([(x_re * r_re).abs() + (x_im * r_im).abs(), (x_re * r_im).abs() + (x_im * r_re).abs()], dim=-1)
    return torch.cat([(r_re * x_re).abs() + (r_im * x_im).abs(), (r_re * x_im).abs() + (r_im * x_re).abs()], dim=-1)


def score(h, r, t):
    """[B] scores of gathered [B, d] rows, in the dtype of the rows"""
    return (tail_query(h, r) * t).sum(dim=-1)


def score_magnitude(h, r, t):
    """the sum of the absolute values of the ``2 d`` expanded triple products of a score"""
    (h_re, h_im), (r_re, r_im), (t_re, t_im) = halves(h), halves(r), halves(t)
    terms = ((h_re * r_re * t_re).abs() + (h_im * r_im * t_re).abs() + (h_re * r_im * t_im).abs() + (h_im * r_re * t_im).abs())
    return terms.sum(dim=-1)


def sample_grads(g, h, r, t):
    """-> (gh, gt, gr) [B, d] of gathered float64 rows, the header's six products"""
    (h_re, h_im), (r_re, r_im), (t_re, t_im) = halves(h), halves(r), halves(t)
    g = g.double().view(-1, 1)
    gh = torch.cat([g * (r_re * t_re + r_im * t_im), g * (r_re * t_im - r_im * t_re)], dim=1)
    gt = torch.cat([g * (h_re * r_re - h_im * r_im), g * (h_re * r_im + h_im * r_re)], dim=1)
    gr = torch.cat([g * (h_re * t_re + h_im * t_im), g * (h_re * t_im - h_im * t_re)], dim=1)
    return gh, gt, gr


def sample_grad_magnitudes(g, h, r, t):
    """per element ``g (a b +- c e)``: ``|g a b| + |g c e|``, and ``|a b| + |c e|`` (what an error of g multiplies)"""
    (h_re, h_im), (r_re, r_im), (t_re, t_im) = halves(h), halves(r), halves(t)
    g = g.double().abs().view(-1, 1)
    mh = torch.cat([(r_re * t_re).abs() + (r_im * t_im).abs(), (r_re * t_im).abs() + (r_im * t_re).abs()], dim=1)
    mt = torch.cat([(h_re * r_re).abs() + (h_im * r_im).abs(), (h_re * r_im).abs() + (h_im * r_re).abs()], dim=1)
    mr = torch.cat([(h_re * t_re).abs() + (h_im * t_im).abs(), (h_re * t_im).abs() + (h_im * t_re).abs()], dim=1)
    return (g * mh, g * mt, g * mr), (mh, mt, mr)


class Want:
    """per element of a gradient buffer: the float64 value, the sum over the occurrences of ``|g a b| + |g c e|``, the
    number of occurrences, and the absolute slack the terms' common coefficient carries (zero unless the kernel forms
    the coefficient itself).  Gate: ``slack + (n + 3) u mag`` - a product, an addition and the scaling by g per term,
    then at most n additions."""

    def __init__(self, num_rows, d):
        self.value = torch.zeros(num_rows, d, dtype=torch.float64)
        self.mag = torch.zeros(num_rows, d, dtype=torch.float64)
        self.slack = torch.zeros(num_rows, d, dtype=torch.float64)
        self.n = torch.zeros(num_rows, dtype=torch.int64)

    def add(self, idx, value, mag, unit_mag, g_err=None):
        idx = torch.arange(value.size(0)) if idx is None else idx
        self.value.index_add_(0, idx, value)
        self.mag.index_add_(0, idx, mag)
        if g_err is not None:
            self.slack.index_add_(0, idx, g_err * unit_mag)
        self.n += torch.bincount(idx, minlength=self.n.numel())
        return self

    def check(self, got, what):
        got = got.detach().double().cpu()
        gate = self.slack + (self.n + 3).double().view(-1, 1) * U * self.mag
        err = (got - self.value).abs()
        worst = float((err / gate.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
        print(f"{what}: worst error / gate = {worst:.3f}, rows without a term: {int((self.n == 0).sum())}")
        assert not bool(torch.isnan(got).any()), f"{what}: NaN left in the buffer"
        assert bool((err <= gate).all()), f"{what}: error / gate = {worst:.3f} at {(err > gate).nonzero()[:4].tolist()}"
        assert bool((got[self.n == 0] == 0).all()), f"{what}: a row without a term is not zero"


def want_grads(g, h, hi, t, ti, r, ri, shared, g_err=None):
    """-> (Want head table, Want tail table (the same object when ``shared``), Want relation table)"""
    hr, tr, rr = rows(h, hi), rows(t, ti), rows(r, ri)
    gh, gt, gr = sample_grads(g, hr, rr, tr)
    (mh, mt, mr), (uh, ut, ur) = sample_grad_magnitudes(g, hr, rr, tr)
    d = h.size(1)
    wh = Want(h.size(0), d).add(hi, gh, mh, uh, g_err)
    wt = (wh if shared else Want(t.size(0), d)).add(ti, gt, mt, ut, g_err)
    wr = Want(r.size(0), d).add(ri, gr, mr, ur, g_err)
    return wh, wt, wr


def table_grads(g, h, hi, t, ti, r, ri, shared):
    """the float64 gradient tables alone (non-finite data: value and pattern, no gates)"""
    hr, tr, rr = rows(h, hi), rows(t, ti), rows(r, ri)
    gh, gt, gr = sample_grads(g, hr, rr, tr)
    b = g.numel()
    ar = torch.arange(b)
    out_h = torch.zeros(h.size(0), h.size(1), dtype=torch.float64).index_add_(0, ar if hi is None else hi, gh)
    out_t = (out_h if shared else torch.zeros(t.size(0), t.size(1), dtype=torch.float64)).index_add_(0, ar if ti is None else ti, gt)
    out_r = torch.zeros(r.size(0), r.size(1), dtype=torch.float64).index_add_(0, ar if ri is None else ri, gr)
    return out_h, out_t, out_r


def softplus64(x):
    return torch.logaddexp(torch.zeros_like(x), x)


def bce64(s, y):
    """float64 ``softplus(-s) y + softplus(s) (1 - y)`` of fp32 scores and labels"""
    s, y = s.double(), y.double()
    return softplus64(-s) * y + softplus64(s) * (1 - y)


def ranks(q, emb, target, eligible=None):
    """1-based float64 restatement of the ranking pass: ``1 + #{n != target, eligible : not (score_n <= true)}``"""
    scores = q.double() @ emb.double().t()
    true = scores.gather(1, target.view(-1, 1))
    beats = ~(scores <= true)
    beats.scatter_(1, target.view(-1, 1), False)
    if eligible is not None:
        beats &= eligible
    return 1 + beats.sum(dim=1)


def topk(q, emb, k, eligible=None):
    """(ids, scores) of the k best candidates: score descending, equal scores by id ascending; -1 / -inf past the end"""
    scores = q.double() @ emb.double().t()
    if eligible is not None:
        scores = torch.where(eligible, scores, torch.full_like(scores, float("-inf")))
    order = torch.sort(scores, dim=1, descending=True, stable=True)
    ids, vals = order.indices[:, :k].clone(), order.values[:, :k].clone()
    if eligible is not None:
        ids[vals == float("-inf")] = -1
    return ids, vals


class ComplExHead64(nn.Module):
    """the float64 twin of ``LinkPredictor(decoder="complex")`` at dropout 0: same parameter name and shape"""

    def __init__(self, relation_weight):
        super().__init__()
        self.relation_embeddings = nn.Embedding(relation_weight.size(0), relation_weight.size(1), dtype=torch.float64)
        with torch.no_grad():
            self.relation_embeddings.weight.copy_(relation_weight.double())

    def forward(self, head_embeddings, tail_embeddings, relation_types):
        return score(head_embeddings, self.relation_embeddings(relation_types), tail_embeddings)

    def score_triples(self, node_embeddings, head_indices, tail_indices, relation_types):
        return self.forward(node_embeddings[head_indices], node_embeddings[tail_indices], relation_types)
