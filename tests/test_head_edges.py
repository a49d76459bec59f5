"""The DistMult head's kernels (``csrc/distmult.hip``) at the widths, batches, key spaces, segment lengths and index
forms the workload's own shapes never reach, against plain float64 on the host.

fp32 inputs are exact in float64, so the reference has no error of its own at these sizes.  With ``u = 2**-24`` (the
unit roundoff of fp32) every gate is the first-order bound that follows from counting the kernel's operations:

* a score is ``d`` terms of two products each, added by at most ``d`` additions (lane loop + butterfly):
  ``|got - want| <= (d + 2) u sum_c |h_c r_c t_c|`` (contraction to FMA only removes roundings);
* an element of a gradient row with ``n`` occurrences is ``n`` terms of two products each and ``n - 1`` additions
  in a fixed order: ``(n + 2) u sum_occ |g x y|``, with ``n`` and the absolute sum taken per element in the reference;
* the BCE coefficient ``gs (sigmoid(s) - y) / B`` is an ``expf``, an add and a divide on a value <= 1, a subtraction that
  may cancel, and two scalings: ``8 u |gs| / B`` absolute, carried into the row gate.

Rows nobody touches must be exactly zero although the buffers arrive full of NaN (``zero_tables``).
"""
import itertools

import pytest
import torch

from conftest import need_gpu

U = 2.0 ** -24
# G = 1; idle lanes at G = 4, 8, 16, 32; one full 256-column trip; a second trip; a third
WIDTHS = [4, 12, 20, 36, 100, 256, 260, 320, 516]


def _ops():
    from primekg_rgcn_linkprediction_amd import ops
    return ops


def _softplus64(x):
    return torch.logaddexp(torch.zeros_like(x), x)


def _bce64(s, y):
    """float64 ``softplus(-s) y + softplus(s) (1 - y)`` of fp32 scores and labels"""
    s, y = s.double(), y.double()
    return _softplus64(-s) * y + _softplus64(s) * (1 - y)


def _rows(mat, idx):
    """the [B, d] float64 rows an operand contributes: gathered, or row b its own"""
    mat = mat.double()
    return mat if idx is None else mat[idx]


class Want:
    """per element of a gradient buffer: the float64 value, the sum of the absolute terms, the number of terms, and the
    absolute slack the terms' common coefficient carries (zero unless the kernel forms the coefficient itself)"""

    def __init__(self, rows, d):
        self.value = torch.zeros(rows, d, dtype=torch.float64)
        self.mag = torch.zeros(rows, d, dtype=torch.float64)
        self.slack = torch.zeros(rows, d, dtype=torch.float64)
        self.n = torch.zeros(rows, dtype=torch.int64)

    def add(self, idx, g, x, y, g_err=None):
        """the terms ``g[b] x[b] y[b]`` land in row ``idx[b]`` (``None``: row b); ``g_err``: the absolute error allowed
        to ``g[b]`` itself"""
        b = g.numel()
        idx = torch.arange(b) if idx is None else idx
        term = g.double().view(-1, 1) * x * y
        self.value.index_add_(0, idx, term)
        self.mag.index_add_(0, idx, term.abs())
        if g_err is not None:
            self.slack.index_add_(0, idx, g_err * (x * y).abs())
        self.n += torch.bincount(idx, minlength=self.n.numel())
        return self

    def check(self, got, what):
        got = got.detach().double().cpu()
        gate = self.slack + (self.n + 2).double().view(-1, 1) * U * self.mag
        err = (got - self.value).abs()
        worst = float((err / gate.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
        print(f"{what}: worst error / gate = {worst:.3f}, rows without a term: {int((self.n == 0).sum())}")
        assert not bool(torch.isnan(got).any()), f"{what}: NaN left in the buffer"
        assert bool((err <= gate).all()), f"{what}: error / gate = {worst:.3f} at {(err > gate).nonzero()[:4].tolist()}"
        assert bool((got[self.n == 0] == 0).all()), f"{what}: a row without a term is not zero"


def _want_grads(gs, h, hi, t, ti, r, ri, shared, g_err=None):
    """-> (Want head table, Want tail table (the same object when ``shared``), Want relation)"""
    hr, tr, rr = _rows(h, hi), _rows(t, ti), _rows(r, ri)
    d = h.size(1)
    wh = Want(h.size(0), d).add(hi, gs, rr, tr, g_err)
    wt = (wh if shared else Want(t.size(0), d)).add(ti, gs, hr, rr, g_err)
    wr = Want(r.size(0), d).add(ri, gs, hr, tr, g_err)
    return wh, wt, wr


def _nan_like(x):
    return torch.full_like(x, float("nan"))


def _run_bwd(dev, gs, h, hi, t, ti, r, ri, shared, need=(True, True, True), bce=None):
    """``ops.distmult_bwd`` (``bce = (scores, labels)``: ``ops.distmult_bce_bwd``, ``gs`` one element) into NaN-filled
    buffers with ``zero_tables``; ``shared``: ``grad_h is grad_t``.  -> (grad_h, grad_t, grad_r), None where not needed"""
    ops = _ops()
    to = lambda x: None if x is None else x.to(dev)
    hd, td, rd = to(h), to(t), to(r)
    if shared:
        td = hd
    gh = _nan_like(hd) if need[0] else None
    gt = gh if shared and need[0] and need[1] else (_nan_like(td) if need[1] else None)
    gr = _nan_like(rd) if need[2] else None
    batch = gs.numel() if bce is None else bce[0].numel()
    if bce is None:
        ops.distmult_bwd(to(gs), hd, to(hi), td, to(ti), rd, to(ri), batch, gh, gt, gr, zero_tables=True)
    else:
        ops.distmult_bce_bwd(to(gs), to(bce[0]), to(bce[1]), hd, to(hi), td, to(ti), rd, to(ri), batch, gh, gt, gr,
                             zero_tables=True)
    return gh, gt, gr


# ------------------------------------------------------------------------------------------ a. forward
def _fwd_case(d, batch, seed=0):
    gen = torch.Generator().manual_seed(1000 * d + batch + seed)
    ent, rel = torch.randn(37, d, generator=gen), torch.randn(5, d, generator=gen)
    hi, ti = torch.randint(0, 37, (batch,), generator=gen), torch.randint(0, 37, (batch,), generator=gen)
    ri = torch.randint(0, 5, (batch,), generator=gen)
    labels = (torch.rand(batch, generator=gen) > 0.5).float()
    return ent, rel, hi, ti, ri, labels


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 63, 65, 257])
@pytest.mark.parametrize("d", WIDTHS)
def test_forward_widths_and_ragged_batches(d, batch):
    """``distmult_fwd`` / ``distmult_bce_fwd``: every lane-group size with and without idle lanes, widths that take a
    second and a third trip of the ``c += 4 G`` loop, batches that end inside a workgroup for every G"""
    dev = need_gpu()
    ops = _ops()
    ent, rel, hi, ti, ri, labels = _fwd_case(d, batch)
    args = (ent.to(dev), hi.to(dev), ent.to(dev), ti.to(dev), rel.to(dev), ri.to(dev))
    got = ops.distmult_fwd(*args, batch)
    term = ent.double()[hi] * rel.double()[ri] * ent.double()[ti]
    want, mag = term.sum(1), term.abs().sum(1)
    err = (got.double().cpu() - want).abs()
    print(f"forward d={d} B={batch}: worst error / gate = {float((err / ((d + 2) * U * mag)).max()):.3f}")
    assert got.shape == (batch,) and bool((err <= (d + 2) * U * mag).all())
    scores, loss = ops.distmult_bce_fwd(*args, labels.to(dev), batch)
    assert torch.equal(scores, got)
    want_loss = _bce64(scores.cpu(), labels)
    lerr = (loss.double().cpu() - want_loss).abs()
    print(f"loss: worst error / gate = {float((lerr / (8 * U * want_loss.clamp_min(1.0))).max()):.3f}")
    assert bool((lerr <= 8 * U * want_loss.clamp_min(1.0)).all())
    ops.check_indices(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("d", WIDTHS)
def test_loss_at_saturated_and_zero_logits(d):
    """the per-sample loss where ``exp`` under- and overflows (scores of exactly +100 and -100 built from unit rows,
    both labels) and at s = 0 (a zero relation row), among logits scaled from ~1e-2 to beyond 1e3: finite, and within
    the gate of the float64 expression at the kernel's own score"""
    dev = need_gpu()
    ops = _ops()
    batch = 257
    ent, rel, hi, ti, ri, labels = _fwd_case(d, batch, seed=7)
    ent = ent * torch.tensor([0.1, 1.0, 10.0, 40.0]).repeat(10)[:37].view(-1, 1)
    ent[:3], rel[:2] = 0.0, 0.0
    ent[0, 0], ent[1, 0], ent[2, 0], rel[0, 0] = 10.0, 1.0, -1.0, 10.0      # 10 * 10 * (+-1); relation row 1 is zero
    hi[:4], ri[:4], ti[:4] = 0, 0, torch.tensor([1, 1, 2, 2])               # +100, +100, -100, -100
    hi[4:6], ri[4:6], ti[4:6] = 5, 1, 6                                     # 0, 0
    labels[:6] = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0, 1.0])
    scores, loss = ops.distmult_bce_fwd(ent.to(dev), hi.to(dev), ent.to(dev), ti.to(dev), rel.to(dev), ri.to(dev),
                                        labels.to(dev), batch)
    s = scores.cpu()
    assert s[:6].tolist() == [100.0, 100.0, -100.0, -100.0, 0.0, 0.0]
    assert bool(torch.isfinite(loss).all())
    want = _bce64(s, labels)
    lerr = (loss.double().cpu() - want).abs()
    print(f"loss d={d}: worst error / gate = {float((lerr / (8 * U * want.clamp_min(1.0))).max()):.3f}")
    assert bool((lerr <= 8 * U * want.clamp_min(1.0)).all())


# ------------------------------------------------------------------------------------------ b. backward, widths
@pytest.mark.gpu
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("d", WIDTHS)
def test_backward_widths(d, shared):
    """the autograd wrapper's route (one table: ``grad_h is grad_t``, one key space; or two tables) at every width: the
    clamp that serves lanes past the row, the second 256-column trip of the scatter and of the relation tree"""
    dev = need_gpu()
    from primekg_rgcn_linkprediction_amd import head
    batch = 300
    gen = torch.Generator().manual_seed(d)
    ent, ent2, rel = (torch.randn(n, d, generator=gen) for n in (37, 37, 5))
    used = torch.tensor([i for i in range(37) if i not in (0, 17, 36)])     # first, middle and last row unused
    hi, ti = (used[torch.randint(0, used.numel(), (batch,), generator=gen)] for _ in range(2))
    ri = torch.tensor([0, 1, 3, 4])[torch.randint(0, 4, (batch,), generator=gen)]
    gs = torch.randn(batch, generator=gen)
    tail = ent if shared else ent2
    wh, wt, wr = _want_grads(gs, ent, hi, tail, ti, rel, ri, shared)

    e = ent.to(dev).requires_grad_(True)
    t = e if shared else ent2.to(dev).requires_grad_(True)
    r = rel.to(dev).requires_grad_(True)
    sc = head.distmult(e, hi.to(dev), t, ti.to(dev), r, ri.to(dev))
    sc.backward(gs.to(dev))
    wh.check(e.grad, "entity table")
    if not shared:
        wt.check(t.grad, "tail table")
    wr.check(r.grad, "relation table")
    # the same call into buffers full of NaN: the same bits, so the untouched rows were cleared by the launch itself
    gh, gt, gr = _run_bwd(dev, gs, ent, hi, tail, ti, rel, ri, shared)
    assert torch.equal(gh, e.grad) and torch.equal(gr, r.grad)
    if not shared:
        assert torch.equal(gt, t.grad)
    ops = _ops()
    ops.check_indices(dev)


# ------------------------------------------------------------------------------------------ c. key space, segments
def _hub_case(batch, d, rows=300):
    gen = torch.Generator().manual_seed(batch + d)
    ent, ent2, rel = (torch.randn(n, d, generator=gen) for n in (rows, rows, 3))
    hi, ti = (torch.randint(1, rows - 1, (batch,), generator=gen) for _ in range(2))   # rows 0 and rows - 1 unused
    hi[torch.rand(batch, generator=gen) < 0.33] = 7                                     # a hub
    ri = torch.randint(0, 3, (batch,), generator=gen)
    gs = torch.randn(batch, generator=gen)
    return ent, ent2, rel, hi, ti, ri, gs


@pytest.mark.gpu
@pytest.mark.parametrize("batch,d,shared", [(4096, 128, True), (4097, 128, True), (8192, 128, True), (8193, 128, True),
                                            (16385, 128, False), (8193, 260, True)])
def test_backward_key_space_and_segment_seams(batch, d, shared):
    """4096 / 4097: the relation tree's segments grow from 64 to 128 samples; 8192 / 8193 with one table: the key space
    2 B crosses the 16384 keys that fit LDS and the scatter reads its keys from global memory; 16385 with two tables: the
    same without the merge, segments of 320; 8193 at d = 260: global keys together with the second 256-column trip"""
    dev = need_gpu()
    ent, ent2, rel, hi, ti, ri, gs = _hub_case(batch, d)
    tail = ent if shared else ent2
    wh, wt, wr = _want_grads(gs, ent, hi, tail, ti, rel, ri, shared)
    gh, gt, gr = _run_bwd(dev, gs, ent, hi, tail, ti, rel, ri, shared)
    wh.check(gh, "entity table")
    if not shared:
        wt.check(gt, "tail table")
    wr.check(gr, "relation table")
    again = _run_bwd(dev, gs, ent, hi, tail, ti, rel, ri, shared)
    assert torch.equal(again[0], gh) and torch.equal(again[1], gt) and torch.equal(again[2], gr)
    _ops().check_indices(dev)


@pytest.mark.gpu
def test_backward_counts_every_occurrence_once_with_global_keys():
    """8193 samples of one table (16386 keys, past LDS), all-ones tables and integer cotangents: every order gives the
    same float, so the sums are exact - nothing dropped or counted twice where the scan reads global memory"""
    dev = need_gpu()
    from primekg_rgcn_linkprediction_amd import head
    batch, d, rows = 8193, 128, 300
    gen = torch.Generator().manual_seed(21)
    hi, ti = (torch.randint(1, rows - 1, (batch,), generator=gen) for _ in range(2))
    hi[torch.rand(batch, generator=gen) < 0.33] = 7
    ri = torch.randint(0, 3, (batch,), generator=gen)
    cot = torch.randint(-8, 9, (batch,), generator=gen).float()
    emb = torch.ones(rows, d, device=dev, requires_grad=True)
    rel = torch.ones(3, d, device=dev, requires_grad=True)
    sc = head.distmult(emb, hi.to(dev), emb, ti.to(dev), rel, ri.to(dev))
    (sc * cot.to(dev)).sum().backward()
    want = torch.zeros(rows).index_add_(0, hi, cot).index_add_(0, ti, cot)
    assert torch.equal(emb.grad.cpu(), want.view(-1, 1).expand(-1, d))
    assert torch.equal(rel.grad.cpu(), torch.zeros(3).index_add_(0, ri, cot).view(-1, 1).expand(-1, d))


# ------------------------------------------------------------------------------------------ d. index forms
SUBSETS = [s for s in itertools.product((True, False), repeat=3) if any(s) and not all(s)]


@pytest.mark.gpu
@pytest.mark.parametrize("bce", [False, True])
@pytest.mark.parametrize("h_indexed,t_indexed,r_indexed", list(itertools.product((True, False), repeat=3)))
def test_backward_index_forms(h_indexed, t_indexed, r_indexed, bce):
    """each operand gathered through an index or ``[B, d]`` with row b its own (a gradient per row, n = 1), in both
    entry points (the BCE one with the coefficient's slack carried into the row gate, ``gs = 0.5``); then every subset
    of the three gradients requested, the others ``None``: the same bits"""
    dev = need_gpu()
    ops = _ops()
    batch, d = 130, 36
    gen = torch.Generator().manual_seed(17)
    h = torch.randn(41 if h_indexed else batch, d, generator=gen)
    t = torch.randn(29 if t_indexed else batch, d, generator=gen)
    r = torch.randn(5 if r_indexed else batch, d, generator=gen)
    hi = torch.randint(1, 41, (batch,), generator=gen) if h_indexed else None
    ti = torch.randint(0, 28, (batch,), generator=gen) if t_indexed else None
    ri = torch.tensor([0, 2, 4])[torch.randint(0, 3, (batch,), generator=gen)] if r_indexed else None
    if bce:
        labels = (torch.rand(batch, generator=gen) > 0.5).float()
        scores = ops.distmult_fwd(h.to(dev), None if hi is None else hi.to(dev), t.to(dev),
                                  None if ti is None else ti.to(dev), r.to(dev), None if ri is None else ri.to(dev),
                                  batch).cpu()
        up = torch.tensor([0.5])
        coef = 0.5 * (torch.sigmoid(scores.double()) - labels.double()) / batch
        g_err, extra = 8 * U * 0.5 / batch, (scores, labels)
    else:
        up = coef = torch.randn(batch, generator=gen)
        g_err, extra = None, None
    wants = _want_grads(coef, h, hi, t, ti, r, ri, False, g_err)
    full = _run_bwd(dev, up, h, hi, t, ti, r, ri, False, bce=extra)
    for w, g, name in zip(wants, full, ("head", "tail", "relation")):
        w.check(g, name)
    for need in SUBSETS:
        part = _run_bwd(dev, up, h, hi, t, ti, r, ri, False, need=need, bce=extra)
        for wanted, p, g in zip(need, part, full):
            assert (p is None) if not wanted else torch.equal(p, g), need
    ops.check_indices(dev)


# ------------------------------------------------------------------------------------------ e. BCE coefficient
@pytest.mark.gpu
def test_bce_backward_coefficient_at_saturated_and_zero_scores():
    """``gs (sigmoid(s) - y) / B`` inside the backward: scores of exactly +100, -100 (``expf(-s)`` overflows to inf) and 0
    built from unit rows, both labels, ``gs = 0.5`` so that an ignored upstream gradient shows; one table, the
    training form"""
    dev = need_gpu()
    ops = _ops()
    batch, d = 130, 36
    gen = torch.Generator().manual_seed(23)
    ent, rel = torch.randn(37, d, generator=gen), torch.randn(5, d, generator=gen)
    ent[:3], rel[:2] = 0.0, 0.0
    ent[0, 0], ent[1, 0], ent[2, 0], rel[0, 0] = 10.0, 1.0, -1.0, 10.0      # 10 * 10 * (+-1); relation row 1 is zero
    hi, ti = torch.randint(3, 36, (batch,), generator=gen), torch.randint(3, 36, (batch,), generator=gen)
    ri = torch.randint(2, 5, (batch,), generator=gen)
    hi[:4], ri[:4], ti[:4] = 0, 0, torch.tensor([1, 1, 2, 2])               # +100, +100, -100, -100
    ri[4:6] = 1                                                             # 0, 0
    labels = (torch.rand(batch, generator=gen) > 0.5).float()
    labels[:6] = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0, 1.0])
    e, r = ent.to(dev), rel.to(dev)
    scores, _ = ops.distmult_bce_fwd(e, hi.to(dev), e, ti.to(dev), r, ri.to(dev), labels.to(dev), batch)
    scores = scores.cpu()
    assert scores[:6].tolist() == [100.0, 100.0, -100.0, -100.0, 0.0, 0.0]
    gs = 0.5
    coef = gs * (torch.sigmoid(scores.double()) - labels.double()) / batch
    wh, _, wr = _want_grads(coef, ent, hi, ent, ti, rel, ri, True, 8 * U * gs / batch)
    gh, gt, gr = _run_bwd(dev, torch.tensor([gs]), ent, hi, ent, ti, rel, ri, True, bce=(scores, labels))
    assert gt is gh and bool(torch.isfinite(gh).all()) and bool(torch.isfinite(gr).all())
    wh.check(gh, "entity table")
    wr.check(gr, "relation table")
    assert float(gh[0].abs().max()) > 0 and float(gr[0].abs().max()) > 0     # the saturated samples do contribute


# ------------------------------------------------------------------------------------------ f. hit rule
def _hits(dev, scores, labels):
    ops = _ops()
    correct = torch.zeros((), dtype=torch.int64, device=dev)
    ops.distmult_bce_reduce(torch.zeros_like(scores).to(dev), scores.to(dev), labels.to(dev), None, correct)
    return int(correct.item())


@pytest.mark.gpu
def test_hit_count_is_the_sign_of_the_score():
    """``distmult_bce_reduce`` counts ``(s > 0) == (y > 0.5)``.  At zeros of both signs, tiny and huge scores, infinities
    and NaN that is the reference's ``(sigmoid(s) > 0.5).float() == y``, sample by sample.  Inside ``0 < s < 2**-23``
    fp32 ``sigmoid`` may round to exactly 0.5 and the reference then predicts 0; the kernel keeps the sign rule there."""
    dev = need_gpu()
    edge = torch.tensor([0.0, -0.0, -1e-9, 2.0 ** -20, -2.0 ** -20, float("inf"), float("-inf"), float("nan")])
    for y in (0.0, 1.0):
        for i in range(edge.numel()):
            s, labels = edge[i:i + 1], torch.full((1,), y)
            assert _hits(dev, s, labels) == int(((torch.sigmoid(s) > 0.5).float() == labels).sum()), (float(s), y)
        labels = torch.full((edge.numel(),), y)
        assert _hits(dev, edge, labels) == int(((torch.sigmoid(edge) > 0.5).float() == labels).sum())
    window = torch.tensor([2.0 ** -100, 1e-9, 2.9e-8, 6.1e-8, 1e-7, 2.0 ** -23 * (1 - 2.0 ** -24)])   # (normal numbers)
    assert bool((window > 0).all()) and bool((window < 2.0 ** -23).all())
    assert _hits(dev, window, torch.ones(window.numel())) == window.numel()
    assert _hits(dev, window, torch.zeros(window.numel())) == 0


# ------------------------------------------------------------------------------------------ g. segment_sum
@pytest.mark.gpu
@pytest.mark.parametrize("d", [4, 260])
@pytest.mark.parametrize("batch", [1, 64, 65, 4097])
def test_segment_sum_across_the_seams(batch, d):
    """``ops.segment_sum``: one sample, one full chunk, one sample into a second chunk, and 4097 samples (segments of
    128, 33 of them); d = 4 (every lane but one past the row) and d = 260 (a second 256-column trip)"""
    dev = need_gpu()
    ops = _ops()
    gen = torch.Generator().manual_seed(batch * 7 + d)
    rows = torch.randn(batch, d, generator=gen)
    idx = torch.tensor([0, 1, 3, 4, 6])[torch.randint(0, 5, (batch,), generator=gen)]      # rows 2 and 5 unused
    got = ops.segment_sum(rows.to(dev), idx.to(dev), 7)
    want = Want(7, d)
    want.value.index_add_(0, idx, rows.double())
    want.mag.index_add_(0, idx, rows.double().abs())
    want.n += torch.bincount(idx, minlength=7)
    want.check(got, "segment_sum")
    assert torch.equal(got, ops.segment_sum(rows.to(dev), idx.to(dev), 7))
    ops.check_indices(dev)
