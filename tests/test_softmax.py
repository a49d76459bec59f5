"""GPU tier of the 1-vs-all softmax loss (``csrc/softmax_loss.hip``): ``ops.softmax_lse`` / ``ops.softmax_grad`` and
``LinkPredictor.softmax_loss`` against the float64 restatement (``softmax_reference.py``) inside the bounds the header
derives, computed from the data of each case.  Shapes are the smallest that reach each path: B in {1, 64, 65} (one row,
a full row tile, a ragged second one), N in {100, 129, 300} (less than a column tile, a ragged second one, three tiles so
that two slices are 2 + 1; the last mask word only partly used), d in {32, 96, 256} (one block, an odd number of 32-column
blocks for the two wave columns, the widest row), slices in {0, 1, 2, 3}."""
import functools

import numpy as np
import pytest
import torch

import softmax_reference as R
from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import head, ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 100, 32), (64, 129, 96), (65, 300, 256), (65, 300, 32), (1, 300, 96), (64, 100, 256), (65, 129, 96)]
MASKS = ("none", "allow", "exclude", "both")


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@functools.lru_cache(maxsize=None)
def case(b, n, d, seed=0):
    """operands on the CPU, masks as bit words, and per mask configuration the float64 reference with its bounds -
    computed once per shape and shared, never modified"""
    gen = torch.Generator().manual_seed(seed + 1000 * b + n + d)
    q = torch.randn(b, d, generator=gen) * (2.0 / d ** 0.5)
    emb = torch.randn(n, d, generator=gen)
    target = torch.randint(0, n, (b,), generator=gen)
    target[(target == 5) | (target == n - 2)] = 7                  # (two candidates stay nobody's target)
    target[0], target[-1] = 3, n - 1                               # the first tile; the last, ragged one
    if b >= 3:
        target[1] = target[2] = n // 2                             # one candidate, the target of two queries
    cls = torch.randint(-1, 3, (n,), generator=gen)
    cls[5] = cls[n - 2] = -1                                       # in no class (and no query's target)
    qcls = cls[target].to(torch.int32)
    if b >= 3:
        qcls[2] = 7                                                # outside [0, C): the target alone
    allow = torch.from_numpy(R.pack_bits(np.stack([cls.numpy() == c for c in range(3)])))
    dense = torch.rand(b, n, generator=gen) < 0.3
    dense[torch.arange(b), target] = True                          # the positive is a known triple: its own bit is set
    excl = torch.from_numpy(R.pack_bits(dense.numpy()))
    g = torch.randn(b, generator=gen)
    s64, sb = R.scores(q, emb), R.score_bound(q, emb)
    refs = {}
    for mask in MASKS:
        a = (allow, qcls) if mask in ("allow", "both") else (None, None)
        e = excl if mask in ("exclude", "both") else None
        ok = R.eligible(b, n, target, a[0], a[1], e)
        f = R.forward(s64, ok, target)
        c64, p64 = R.coefficients(g, s64, f["lse"], ok, target)
        dq64, de64 = R.gradients(c64, q, emb)
        refs[mask] = dict(ok=ok, f=f, c=c64, p=p64, dq=dq64, de=de64)
    return dict(q=q, emb=emb, target=target, cls=cls, qcls=qcls, allow=allow, excl=excl, g=g, s64=s64, sb=sb, refs=refs)


def masks_of(c, mask, dev):
    allow = c["allow"].to(dev) if mask in ("allow", "both") else None
    qcls = c["qcls"].to(dev) if mask in ("allow", "both") else None
    excl = c["excl"].to(dev) if mask in ("exclude", "both") else None
    return allow, qcls, excl


def forward_bounds(c, ref, b, n, slices):
    lb = R.lse_bound(c["sb"], ref["ok"], ref["f"]["lse"], R.chain_steps(b, n, slices))
    return lb, R.loss_bound(lb, c["sb"], c["target"], ref["f"]["loss"])


@pytest.mark.parametrize("b, n, d", SHAPES)
def test_forward_against_the_restatement(b, n, d):
    dev = need_gpu()
    c = case(b, n, d)
    q, emb, target = c["q"].to(dev), c["emb"].to(dev), c["target"].to(dev)
    rows = np.arange(b)
    stored = ops.distmult_score_all_tails(q, torch.ones(1, d, device=dev), torch.zeros(b, dtype=torch.int64, device=dev), emb)[0]
    for mask in MASKS:
        ref = c["refs"][mask]
        allow, qcls, excl = masks_of(c, mask, dev)
        for slices in (0, 1, 2, 3):
            lse, ts, rmax, loss, hit = ops.softmax_lse(q, emb, target, allow, qcls, excl, slices, with_loss=True)
            three = ops.softmax_lse(q, emb, target, allow, qcls, excl, slices)
            assert len(three) == 3 and all(torch.equal(bits(x), bits(y)) for x, y in zip(three, (lse, ts, rmax)))
            # the target's score is the entry of the stored score matrix, bit for bit
            assert torch.equal(bits(ts), bits(stored[torch.arange(b, device=dev), target])), (mask, slices)
            lb, lossb = forward_bounds(c, ref, b, n, slices)
            f = ref["f"]
            err = np.abs(lse.double().cpu().numpy() - f["lse"])
            print(f"{mask:8s} slices {slices}: |lse - lse64| max {err.max():.3e} (bound min {lb.min():.3e})")
            assert (err <= lb).all(), (mask, slices)
            tsb = c["sb"][rows, c["target"].numpy()]
            assert (np.abs(ts.double().cpu().numpy() - f["true_score"]) <= tsb).all()
            maxb = np.where(ref["ok"], c["sb"], 0.0).max(axis=1)
            assert (np.abs(rmax.double().cpu().numpy() - f["row_max"]) <= maxb).all()
            assert (np.abs(loss.double().cpu().numpy() - f["loss"]) <= lossb).all()
            assert torch.equal(bits(loss), bits(lse - ts))
            # a hit is decided on the device's own scores: it may differ from float64's only where the two best are
            # closer than the score bound
            clear = np.abs(f["true_score"] - f["row_max"]) > tsb + maxb
            got = hit.cpu().numpy().astype(bool)
            assert (got[clear] == f["hit"][clear]).all() and torch.equal(hit.bool(), ts >= rmax)
    ops.check_indices(dev)


def test_masks_bite():
    """an integer table (every product and sum exact) in which one candidate per query scores 1e4 against 1 elsewhere"""
    dev = need_gpu()
    b, n, d = 65, 300, 32
    q, emb = torch.zeros(b, d), torch.zeros(n, d)
    q[:, 0] = 1.0
    emb[:, 0] = 1.0                                                # every score is 1 ...
    coord = torch.arange(b) % 31                                   # ... but one candidate's per query: query i owns the
    q[torch.arange(b), 1 + coord] = 1.0                            # coordinate 1 + i % 31, shared with i + 31 and i + 62,
    big = (coord * 7 + 11) % n                                     # and that coordinate is set in one table row only
    emb[big, 1 + coord] = 9999.0
    target = (big + 1) % n                                         # never a big candidate: they are 7 apart
    s64 = R.scores(q, emb)
    assert (s64[np.arange(b), big.numpy()] == 1e4).all() and (np.sort(s64, axis=1)[:, -2] == 1.0).all()
    qd, ed = q.to(dev), emb.to(dev)
    rows = torch.arange(b)

    def run(tgt, allow=None, qcls=None, excl=None):
        ok = R.eligible(b, n, tgt, allow, qcls, excl)
        f = R.forward(s64, ok, tgt)
        lse, ts, rmax, loss, hit = ops.softmax_lse(qd, ed, tgt.to(dev), None if allow is None else allow.to(dev),
                                                   None if qcls is None else qcls.to(dev),
                                                   None if excl is None else excl.to(dev), 2, with_loss=True)
        lb = R.lse_bound(np.zeros_like(s64), ok, f["lse"], R.chain_steps(b, n, 2))      # integer data: the scores are exact
        assert (np.abs(loss.double().cpu().numpy() - f["loss"]) <= lb + R.U * np.abs(f["loss"])).all()
        return loss.cpu(), ok.sum(axis=1)

    loss, count = run(target)                                      # not struck: it dominates
    assert (count == n).all() and ((loss - 9999.0).abs() < 1e-2).all()
    struck = torch.zeros(b, n, dtype=torch.bool)
    struck[rows, big] = True
    excl = torch.from_numpy(R.pack_bits(struck.numpy()))
    loss, count = run(target, excl=excl)                           # struck by exclude: log of the eligible count
    assert (count == n - 1).all() and torch.allclose(loss, torch.full((b,), float(np.log(n - 1))), atol=1e-4)
    cls = torch.zeros(n, dtype=torch.int64)
    cls[big] = 1                                                   # the big candidates form a class of their own
    allow = torch.from_numpy(R.pack_bits(np.stack([cls.numpy() == 0, cls.numpy() == 1])))
    loss, count = run(target, allow=allow, qcls=torch.zeros(b, dtype=torch.int32))      # struck by the class mask
    assert (count == n - 31).all() and torch.allclose(loss, torch.full((b,), float(np.log(n - 31))), atol=1e-4)
    # the struck candidate IS the target: it must count - as the maximum, with the other scores e^-9999 away
    loss, count = run(big, excl=excl)
    assert (count == n).all() and (loss == 0).all()
    loss, count = run(big, allow=allow, qcls=torch.zeros(b, dtype=torch.int32))
    assert (count == n - 30).all() and (loss == 0).all()


@pytest.mark.parametrize("b, n, d", SHAPES)
def test_backward_against_the_restatement(b, n, d):
    dev = need_gpu()
    c = case(b, n, d)
    q, emb, target, g = (c[k].to(dev) for k in ("q", "emb", "target", "g"))
    for mask in MASKS:
        ref = c["refs"][mask]
        allow, qcls, excl = masks_of(c, mask, dev)
        for slices in (0, 1, 2, 3):
            lse = ops.softmax_lse(q, emb, target, allow, qcls, excl, slices)[0]
            buf = torch.full((n, d), float("nan"), device=dev)
            dq, de = ops.softmax_grad(g, q, emb, target, lse, allow, qcls, excl, slices, demb=buf)
            assert de is buf and not torch.isnan(de).any() and not torch.isnan(dq).any()
            lb, _ = forward_bounds(c, ref, b, n, slices)
            dc = R.coefficient_bound(g, c["s64"], ref["f"]["lse"], ref["p"], c["sb"], lb)
            dqb, deb = R.gradient_bounds(ref["c"], dc, c["q"], c["emb"])
            eq = np.abs(dq.double().cpu().numpy() - ref["dq"])
            ee = np.abs(de.double().cpu().numpy() - ref["de"])
            print(f"{mask:8s} slices {slices}: |dq - dq64| max {eq.max():.3e} (bound at it {dqb.flat[eq.argmax()]:.3e}), "
                  f"|dE - dE64| max {ee.max():.3e} (bound at it {deb.flat[ee.argmax()]:.3e})")
            assert (eq <= dqb).all() and (ee <= deb).all(), (mask, slices)
            if b >= 3 and mask == "none":
                # the candidate two queries aim at receives both one-hot terms: either one is larger than the bound
                # somewhere in the row, so a row that missed it would have failed above
                t = int(c["target"][1])
                twice = [i for i in range(b) if int(c["target"][i]) == t]
                assert len(twice) >= 2
                for i in twice:
                    assert (np.abs(c["g"][i].item() * c["q"][i].double().numpy()) > 2 * deb[t]).any()
            # rows of candidates no query finds eligible: exact zeros, over a buffer that held NaN
            dead = ~ref["ok"].any(axis=0)
            assert mask not in ("allow", "both") or dead.any()
            assert bool((de[torch.from_numpy(dead).to(dev)] == 0).all())
            # sum_n c[b, n] from the device's lse: g (exp(lse64 - lse) - 1), inside the lse bound
            csum = R.coefficients(c["g"], c["s64"], lse.double().cpu().numpy(), ref["ok"], c["target"])[0].sum(axis=1)
            assert (np.abs(csum) <= np.abs(c["g"].numpy()) * np.expm1(lb) * 1.01 + 1e-15).all()
            # a gradient that is not asked for leaves the other one's bits alone
            only_q = ops.softmax_grad(g, q, emb, target, lse, allow, qcls, excl, slices, need_demb=False)
            only_e = ops.softmax_grad(g, q, emb, target, lse, allow, qcls, excl, slices, need_dq=False)
            assert only_q[1] is None and only_e[0] is None
            assert torch.equal(bits(only_q[0]), bits(dq)) and torch.equal(bits(only_e[1]), bits(de))
    ops.check_indices(dev)


def test_two_calls_give_the_same_bits_and_chunked_masks_too():
    dev = need_gpu()
    b, n, d = 65, 300, 32
    c = case(b, n, d)
    q, emb, target, g = (c[k].to(dev) for k in ("q", "emb", "target", "g"))
    allow, qcls, _ = masks_of(c, "both", dev)
    gen = torch.Generator().manual_seed(9)
    anchor, rel = torch.randint(0, n, (b,), generator=gen).to(dev), torch.randint(0, 3, (b,), generator=gen).to(dev)
    ei = torch.cat([torch.stack([anchor, target]), torch.randint(0, n, (2, 3000), generator=gen).to(dev)], dim=1)
    et = torch.cat([rel, torch.randint(0, 3, (3000,), generator=gen).to(dev)])
    known = ops.KnownTriples(ei, et, n, 3)

    def run(max_mask_bytes):
        out = ops.softmax_lse_filtered(q, emb, target, known, "tail", anchor, rel, allow, qcls, max_mask_bytes, 2)
        dq, de = ops.softmax_grad_filtered(g, q, emb, target, out[0], known, "tail", anchor, rel, allow, qcls,
                                           max_mask_bytes, 2)
        return list(out) + [dq, de]

    whole, whole2 = run(256 << 20), run(256 << 20)
    chunked, chunked2 = run(40 * 16), run(40 * 16)                 # chunks of 16 rows through one buffer: five of them
    for x, y in zip(whole + chunked, whole2 + chunked2):
        assert torch.equal(bits(x), bits(y))
    excl = known.exclude_bits("tail", anchor, rel)
    ok = R.eligible(b, n, c["target"], c["allow"], c["qcls"], excl.cpu())
    f = R.forward(c["s64"], ok, c["target"])
    lb = R.lse_bound(c["sb"], ok, f["lse"], R.chain_steps(b, n, 2))
    c64, p64 = R.coefficients(c["g"], c["s64"], f["lse"], ok, c["target"])
    dq64, de64 = R.gradients(c64, c["q"], c["emb"])
    dc = R.coefficient_bound(c["g"], c["s64"], f["lse"], p64, c["sb"], lb)
    dqb, deb = R.gradient_bounds(c64, dc, c["q"], c["emb"], extra_terms=5)
    for out in (whole, chunked):
        assert (np.abs(out[0].double().cpu().numpy() - f["lse"]) <= lb).all()
        assert (np.abs(out[5].double().cpu().numpy() - dq64) <= dqb).all()
        assert (np.abs(out[6].double().cpu().numpy() - de64) <= deb).all()
    # a row's forward and dq do not depend on the chunking at all (the slices are given)
    for i in (0, 1, 2, 3, 5):
        assert torch.equal(bits(whole[i]), bits(chunked[i]))
    # a gradient that is not asked for, whole and chunked: None, and the other one's bits are those of the run that asks
    # for both; a chunked dE that ADDS to a buffer holds buffer + (chunk 0) + (chunk 1) + ...: twice the same bits
    for out, max_mask_bytes in ((whole, 256 << 20), (chunked, 40 * 16)):
        only_q = ops.softmax_grad_filtered(g, q, emb, target, out[0], known, "tail", anchor, rel, allow, qcls,
                                           max_mask_bytes, 2, need_demb=False)
        only_e = ops.softmax_grad_filtered(g, q, emb, target, out[0], known, "tail", anchor, rel, allow, qcls,
                                           max_mask_bytes, 2, need_dq=False)
        assert only_q[1] is None and only_e[0] is None
        assert torch.equal(bits(only_q[0]), bits(out[5])) and torch.equal(bits(only_e[1]), bits(out[6]))
        added = []
        for _ in range(2):
            buf = torch.ones(n, d, device=dev)
            got = ops.softmax_grad_filtered(g, q, emb, target, out[0], known, "tail", anchor, rel, allow, qcls,
                                            max_mask_bytes, 2, need_dq=False, demb=buf, accumulate=True)[1]
            assert got is buf
            added.append(buf)
        assert torch.equal(bits(added[0]), bits(added[1]))
        assert (np.abs(added[0].double().cpu().numpy() - 1.0 - de64) <= deb + 2 * R.U * (1.0 + np.abs(de64))).all()


def test_non_finite_values():
    dev = need_gpu()
    b, n, d = 65, 300, 32
    c = case(b, n, d)
    clean_q, emb, target, g = (c[k].to(dev) for k in ("q", "emb", "target", "g"))
    allow, qcls, excl = masks_of(c, "both", dev)
    q = clean_q.clone()
    q[5] = float("nan")                                            # every score of row 5 is NaN
    q[40] = 0.0
    q[40, 0] = float("inf")                                        # row 40: +-inf (NaN where the table holds a zero)
    for masks in ((None, None, None), (allow, qcls, excl)):
        base = ops.softmax_lse(clean_q, emb, target, *masks, 2, with_loss=True)
        got = ops.softmax_lse(q, emb, target, *masks, 2, with_loss=True)
        ok = R.eligible(b, n, c["target"], *(None if m is None else m.cpu() for m in masks))
        stored = ops.distmult_score_all_tails(q, torch.ones(1, d, device=dev), torch.zeros(b, dtype=torch.int64, device=dev), emb)[0]
        s = np.where(np.isfinite(stored.cpu().numpy()), R.scores(q.cpu(), emb.cpu()), stored.double().cpu().numpy())
        f = R.forward(s, ok, c["target"])
        others = torch.tensor([i for i in range(b) if i not in (5, 40)], device=dev)
        for x, y, name in zip(got, base, ("lse", "true_score", "row_max", "loss", "hit")):
            assert torch.equal(bits(x[others]), bits(y[others])), name
            if name != "hit":
                dev_v, ref_v = x.cpu().numpy(), f[name]
                assert (np.isnan(dev_v) == np.isnan(ref_v)).all(), name
                inf = np.isinf(ref_v)
                assert (np.isinf(dev_v) == inf).all() and (np.sign(dev_v[inf]) == np.sign(ref_v[inf])).all(), name
        assert (got[4].cpu().numpy().astype(bool)[[5, 40]] == f["hit"][[5, 40]]).all()
        dq0 = ops.softmax_grad(g, clean_q, emb, target, base[0], *masks, 2, need_demb=False)[0]
        dq1 = ops.softmax_grad(g, q, emb, target, got[0], *masks, 2, need_demb=False)[0]
        assert torch.equal(bits(dq0[others]), bits(dq1[others]))
        c64, _ = R.coefficients(c["g"], s, f["lse"], ok, c["target"])
        dq64 = R.gradients(c64, q.cpu(), emb.cpu())[0]
        assert (np.isnan(dq1.cpu().numpy()) == np.isnan(dq64)).all()
    # a NaN in the row of a candidate no query can see (in no class, nobody's target) changes nothing the queries get
    # from the forward; in the two products it is 0 * NaN, as in the restatement's matrix product
    poisoned = emb.clone()
    poisoned[5] = float("nan")
    assert int(c["cls"][5]) == -1 and not bool((c["target"] == 5).any())
    base = ops.softmax_lse(clean_q, emb, target, allow, qcls, excl, 2, with_loss=True)
    got = ops.softmax_lse(clean_q, poisoned, target, allow, qcls, excl, 2, with_loss=True)
    for x, y in zip(got, base):
        assert torch.equal(bits(x), bits(y))
    # the backward, as the header states it: the two products are matrix products, so the NaN row meets a zero
    # coefficient as 0 * NaN in dq of every query, and dE inherits a non-finite coefficient - the restatement's sets
    ok = R.eligible(b, n, c["target"], c["allow"], c["qcls"], c["excl"])
    f = R.forward(c["s64"], ok, c["target"])
    c64, _ = R.coefficients(c["g"], c["s64"], f["lse"], ok, c["target"])
    assert not ok[:, 5].any() and (c64[:, 5] == 0).all()
    dq64, de64 = R.gradients(c64, clean_q.cpu(), poisoned.cpu())
    dq, de = ops.softmax_grad(g, clean_q, poisoned, target, got[0], allow, qcls, excl, 2)
    assert np.isnan(dq64).all() and (np.isnan(dq.cpu().numpy()) == np.isnan(dq64)).all()
    assert not np.isnan(de64).any() and (np.isnan(de.cpu().numpy()) == np.isnan(de64)).all()
    assert bool((de[5] == 0).all())                               # nobody's candidate: exact zeros, NaN row or not
    # a row whose coefficients are NaN (the NaN query of above) hands them to dE where it finds a candidate eligible,
    # and through 0 * NaN of its own q row everywhere else: every row of dE, as in the restatement
    lse_q = ops.softmax_lse(q, emb, target, allow, qcls, excl, 2)[0]
    de_q = ops.softmax_grad(g, q, emb, target, lse_q, allow, qcls, excl, 2, need_dq=False)[1]
    stored = ops.distmult_score_all_tails(q, torch.ones(1, d, device=dev), torch.zeros(b, dtype=torch.int64, device=dev), emb)[0]
    s = np.where(np.isfinite(stored.cpu().numpy()), R.scores(q.cpu(), emb.cpu()), stored.double().cpu().numpy())
    fq = R.forward(s, ok, c["target"])
    de_q64 = R.gradients(R.coefficients(c["g"], s, fq["lse"], ok, c["target"])[0], q.cpu(), emb.cpu())[1]
    assert (np.isnan(de_q.cpu().numpy()) == np.isnan(de_q64)).all() and np.isnan(de_q64).all()


# ------------------------------------------------------------------------------------------------- the head
def _abs_query(decoder, x, r):
    """the query formula on absolute values with every sign a plus: sum of the absolute products behind an entry"""
    x, r = np.abs(x), np.abs(r)
    if decoder == "distmult":
        return x * r
    m = x.shape[1] // 2
    return np.concatenate([x[:, :m] * r[:, :m] + x[:, m:] * r[:, m:], x[:, :m] * r[:, m:] + x[:, m:] * r[:, :m]], axis=1)


@pytest.mark.parametrize("decoder", ["distmult", "complex"])
def test_head_loss_and_gradients_against_the_fallback_in_float64(decoder):
    dev = need_gpu()
    n, b, d, r = 300, 65, 32, 3
    gen = torch.Generator().manual_seed(21)
    lp = head.LinkPredictor(r, d, decoder=decoder)
    with torch.no_grad():
        lp.relation_embeddings.weight.copy_(torch.randn(r, d, generator=gen) * 0.7)
    emb = torch.randn(n, d, generator=gen) * 0.7
    h, t = torch.randint(0, n, (b,), generator=gen), torch.randint(0, n, (b,), generator=gen)
    rel = torch.randint(0, r, (b,), generator=gen)
    cls = torch.randint(-1, 3, (n,), generator=gen)
    ei = torch.cat([torch.stack([h, t]), torch.randint(0, n, (2, 2000), generator=gen)], dim=1)
    et = torch.cat([rel, torch.randint(0, r, (2000,), generator=gen)])
    known = ops.KnownTriples(ei, et, n, r)

    lp64 = head.LinkPredictor(r, d, decoder=decoder).double()
    lp64.load_state_dict({k: v.double() for k, v in lp.state_dict().items()})
    emb64 = emb.double().requires_grad_(True)
    loss64, hits64 = lp64.softmax_loss(emb64, h, t, rel, known=known, node_class=cls)
    loss64.backward()

    lpd = head.LinkPredictor(r, d, decoder=decoder).to(dev)
    lpd.load_state_dict(lp.state_dict())
    embd = emb.to(dev).requires_grad_(True)
    known_d = ops.KnownTriples(ei.to(dev), et.to(dev), n, r)
    lossd, hitsd = lpd.softmax_loss(embd, h.to(dev), t.to(dev), rel.to(dev), known=known_d, node_class=cls.to(dev))
    lossd.backward()

    # the bounds, side by side: the query adds three roundings per entry to the score's d
    relw = lp64.relation_embeddings.weight.detach().numpy()
    e64 = emb.double().numpy()
    loss_bound, grad_emb_b, grad_rel_b = 0.0, np.zeros((n, d)), np.zeros((r, d))
    touched = np.zeros(n, dtype=bool)
    for side in ("tail", "head"):
        anchor, target = (h, t) if side == "tail" else (t, h)
        x, rr = e64[anchor.numpy()], relw[rel.numpy()]
        aq = _abs_query(decoder, x, rr)
        sb = R.gamma(d + 3) * (aq @ np.abs(e64).T)
        q64 = head.complex_query_rows(torch.from_numpy(x), torch.from_numpy(rr), side).numpy() if decoder == "complex" else x * rr
        ok = np.ones((b, n), dtype=bool)
        c_np = cls.numpy()
        ok &= (c_np[None, :] == c_np[target.numpy()][:, None]) & (c_np[target.numpy()] >= 0)[:, None]
        ok &= ~head.known_mask(known, side, anchor, rel).numpy()
        ok[np.arange(b), target.numpy()] = True
        s64 = q64 @ e64.T
        f = R.forward(s64, ok, target)
        lb = R.lse_bound(sb, ok, f["lse"], R.chain_steps(b, n))
        loss_bound += R.loss_bound(lb, sb, target, f["loss"]).sum()
        gvec = np.full(b, 1.0 / (2 * b))
        c64, p64 = R.coefficients(gvec, s64, f["lse"], ok, target)
        dc = R.coefficient_bound(gvec, s64, f["lse"], p64, sb, lb)
        dq64, de64 = R.gradients(c64, q64, e64)
        dqb, deb = R.gradient_bounds(c64, dc, q64, e64)
        deb += (dc + np.abs(c64)).T @ (3 * R.U * aq)               # the query's own rounding inside dE
        gx = _abs_query(decoder, rr, dqb) + 4 * R.U * _abs_query(decoder, rr, dq64)
        gr = _abs_query(decoder, x, dqb) + 4 * R.U * _abs_query(decoder, x, dq64)
        ax, ar = _abs_query(decoder, rr, dq64), _abs_query(decoder, x, dq64)
        grad_emb_b += deb
        np.add.at(grad_emb_b, anchor.numpy(), gx + R.gamma(b + 4) * ax)
        grad_emb_b += R.gamma(4) * np.abs(de64)
        np.add.at(grad_rel_b, rel.numpy(), gr + R.gamma(b + 4) * ar)
        touched |= ok.any(axis=0)
        touched[anchor.numpy()] = True
    loss_bound = loss_bound / (2 * b) + R.gamma(2 * b + 2) * abs(loss64.item())
    print(f"{decoder}: loss {lossd.item():.7f} vs {loss64.item():.7f}, |diff| {abs(lossd.item() - loss64.item()):.3e} "
          f"(bound {loss_bound:.3e})")
    assert abs(lossd.item() - loss64.item()) <= loss_bound
    assert int(hitsd) == int(hits64)
    ee = np.abs(embd.grad.double().cpu().numpy() - emb64.grad.numpy())
    er = np.abs(lpd.relation_embeddings.weight.grad.double().cpu().numpy() - lp64.relation_embeddings.weight.grad.numpy())
    print(f"{decoder}: grad emb err max {ee.max():.3e} (bound at it {grad_emb_b.flat[ee.argmax()]:.3e}), "
          f"grad rel err max {er.max():.3e} (bound at it {grad_rel_b.flat[er.argmax()]:.3e})")
    assert (ee <= grad_emb_b).all() and (er <= grad_rel_b).all()
    # rows that are neither anchors nor eligible candidates: exact zeros
    assert (~touched).any() and bool((embd.grad[torch.from_numpy(~touched).to(dev)] == 0).all())
    if decoder == "complex":
        # the head side carries the conjugate: with the tail side's operand on the head side the loss moves by far
        # more than the bound on this table
        with torch.no_grad():
            right = lp64._softmax_loss_torch(emb64.detach(), h, t, rel, "head", known, cls)[0].mean()
            x, rr = emb64.detach()[t], lp64.relation_embeddings.weight.detach()[rel]
            wrong_q = head.complex_query_rows(x, rr, "tail")
            s = wrong_q @ emb64.detach().t()
            ok_t = torch.from_numpy(ok)
            wrong = (torch.logsumexp(s.masked_fill(~ok_t, float("-inf")), 1) - s[torch.arange(b), h]).mean()
        assert abs(wrong.item() - right.item()) > 100 * loss_bound
        one = lpd.softmax_loss(embd.detach(), h.to(dev), t.to(dev), rel.to(dev), sides="head", known=known_d,
                               node_class=cls.to(dev))[0]
        assert abs(one.item() - right.item()) <= 2 * loss_bound
    ops.check_indices(dev)
