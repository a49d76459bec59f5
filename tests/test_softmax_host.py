"""CPU tier of the 1-vs-all softmax loss (``include/rgcn_softmax.h``, ``csrc/softmax_loss.hip``, ``ops.softmax_lse`` /
``softmax_grad``, ``LinkPredictor.softmax_loss``, ``train.py --loss softmax``): the C surface, every argument check that
runs before a launch, the float64 restatement (``softmax_reference.py``) against torch autograd of the CPU fallback,
the fallback in float32 against the bounds the device is held to, and the trainer on the CPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import c_surface as S
import softmax_reference as R
from c_surface import STREAM, T4, T8, T16
from conftest import ROOT
from primekg_rgcn_linkprediction_amd import _lib, head, ops, train

OK, ARG, UNSUPPORTED, WORKSPACE = _lib.RGCN_OK, _lib.RGCN_ERR_ARG, _lib.RGCN_ERR_UNSUPPORTED, _lib.RGCN_ERR_WORKSPACE


def _fake(i):
    return S.FAKE_BASE + i * S.FAKE_STEP


# ---------------------------------------------------------------------------------- C surface
def test_header_table_and_library_agree():
    """names, parameters, return types and exports: test_c_surface.py, for every header"""
    makefile = open(os.path.join(ROOT, "primekg_rgcn_linkprediction_amd", "csrc", "Makefile")).read()
    assert " softmax_loss.hip" in makefile


def _lse_args(batch=1, n=1, d=32, slices=0, **ptr):
    """q, emb, target, allow, query_class, classes, exclude, batch, n, d, slices, lse, ts, row_max, loss, hit, ws, bytes, stream"""
    p = {"q": _fake(1), "emb": _fake(2), "target": _fake(3), "allow": None, "qcls": None, "excl": None, "lse": _fake(4),
         "ts": _fake(5), "rmax": _fake(6), "loss": None, "hit": None, "ws": _fake(7), "classes": 0,
         "bytes": _lib.load().rgcn_softmax_workspace_bytes(max(batch, 0), n, d, max(slices, 0))}
    p.update(ptr)
    return [p["q"], p["emb"], p["target"], p["allow"], p["qcls"], p["classes"], p["excl"], batch, n, d, slices, p["lse"],
            p["ts"], p["rmax"], p["loss"], p["hit"], p["ws"], p["bytes"], None]


def _grad_args(batch=1, n=1, d=32, slices=0, **ptr):
    """g, q, emb, target, allow, query_class, classes, exclude, lse, batch, n, d, slices, dq, dE, accumulate, ws, bytes, stream"""
    p = {"g": _fake(8), "q": _fake(1), "emb": _fake(2), "target": _fake(3), "allow": None, "qcls": None, "excl": None,
         "lse": _fake(4), "dq": _fake(9), "dE": _fake(10), "ws": _fake(7), "classes": 0, "acc": 0,
         "bytes": _lib.load().rgcn_softmax_workspace_bytes(max(batch, 0), n, d, max(slices, 0))}
    p.update(ptr)
    return [p["g"], p["q"], p["emb"], p["target"], p["allow"], p["qcls"], p["classes"], p["excl"], p["lse"], batch, n, d,
            slices, p["dq"], p["dE"], p["acc"], p["ws"], p["bytes"], None]


# the smallest legal call in the notation of c_surface.py: tables, the query rows, the workspace and the gradients by
# 16 bytes, the int64 targets by 8, every per-sample vector and mask word by 4; the masks absent, then all three given
_WS = S._q("rgcn_softmax_workspace_bytes", 1, 1, 32, 0)
ALIGNMENT_CASES = {
    "rgcn_softmax_lse": [[T16, T16, T8, None, None, 0, None, 1, 1, 32, 0, T4, T4, T4, None, None, T16, _WS, STREAM],
                         [T16, T16, T8, T4, T4, 2, T4, 1, 1, 32, 0, T4, T4, T4, None, None, T16, _WS, STREAM]],
    "rgcn_softmax_grad": [[T4, T16, T16, T8, None, None, 0, None, T4, 1, 1, 32, 0, T16, T16, 0, T16, _WS, STREAM],
                          [T4, T16, T16, T8, T4, T4, 2, T4, T4, 1, 1, 32, 0, T16, T16, 0, T16, _WS, STREAM]],
}


@pytest.mark.parametrize("fn, args", [("rgcn_softmax_lse", _lse_args), ("rgcn_softmax_grad", _grad_args)])
def test_sizes_nulls_and_alignment_are_refused_without_a_gpu(fn, args):
    call = getattr(_lib.load(), fn)
    for d in (48, 8, 33, 288, 512):                               # not a multiple of 32, or wider than 256
        assert call(*args(d=d)) == UNSUPPORTED, d
    for d in (0, -32):
        assert call(*args(d=d)) == ARG
    assert call(*args(batch=-1)) == ARG and call(*args(n=0)) == ARG and call(*args(slices=-1)) == ARG
    assert call(*args(allow=_fake(11), classes=3)) == ARG         # allow without query_class
    assert call(*args(allow=_fake(11), qcls=_fake(12), classes=0)) == ARG
    # batch == 0: RGCN_OK before any pointer is looked at (the backward with no dE to clear makes no HIP call)
    none = dict(q=None, emb=None, target=None, lse=None, ws=None, bytes=0)
    if fn == "rgcn_softmax_lse":
        assert call(*args(batch=0, ts=None, rmax=None, **none)) == OK
        assert call(*args(batch=0, d=48, ts=None, rmax=None, **none)) == UNSUPPORTED      # the size checks come first
        for name in ("q", "emb", "target", "lse", "ts", "rmax"):
            assert call(*args(**{name: None})) == ARG, name
        assert call(*args(ws=None)) == WORKSPACE and call(*args(bytes=8)) == WORKSPACE
    else:
        assert call(*args(batch=0, g=None, dq=None, dE=None, **none)) == OK
        for name in ("g", "q", "emb", "target", "lse"):
            assert call(*args(**{name: None})) == ARG, name
        # two slices of a two-tile range: the partial dq slabs need the workspace; without dq they do not
        assert call(*args(n=200, slices=2, ws=None)) == WORKSPACE and call(*args(n=200, slices=2, bytes=8)) == WORKSPACE
    # a pointer below its alignment, after every other check: the sets of ALIGNMENT_CASES, without and with the masks
    failed = [f for case in ALIGNMENT_CASES[fn] for f in S.misaligned_refusals(call, fn, case)]
    assert not failed, "; ".join(failed)


def test_workspace_bytes_follow_the_slice_rule():
    ws = _lib.load().rgcn_softmax_workspace_bytes
    assert ws(0, 10, 32, 0) == ws(10, 0, 32, 0) == ws(10, 10, 32, -1) == 0
    for b, n, d, slices in ((65, 300, 32, 2), (65, 300, 32, 0), (1, 100, 256, 3), (2048, 30926, 128, 0), (16384, 30926, 128, 0)):
        _, _, s = R.plan(b, n, slices)
        want = max(2 * s * b * 4, s * b * d * 4 if s > 1 else 0)
        assert ws(b, n, d, slices) == (want + 255) // 256 * 256, (b, n, d, slices)
    assert R.plan(65, 300, 2) == (3, 2, 2) and R.plan(16384, 30926, 0)[2] == 1 and R.plan(2048, 30926, 0)[2] == 8


def test_argument_errors_reach_python_as_value_errors():
    q, emb, target = torch.zeros(3, 32), torch.zeros(40, 32), torch.zeros(3, dtype=torch.int64)
    w = ops.mask_words(40)
    allow, qcls = torch.zeros(2, w, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.softmax_lse(torch.zeros(3, 48), torch.zeros(40, 48), target)
    with pytest.raises(ValueError, match="at most 256"):
        ops.softmax_lse(torch.zeros(3, 288), torch.zeros(40, 288), target)
    with pytest.raises(ValueError, match="go together"):
        ops.softmax_lse(q, emb, target, allow=allow)
    with pytest.raises(ValueError, match=rf"allow \[C, {w}\]"):
        ops.softmax_lse(q, emb, target, allow=torch.zeros(2, w + 1, dtype=torch.int32), query_class=qcls)
    with pytest.raises(ValueError, match=rf"exclude \[3, {w}\]"):
        ops.softmax_lse(q, emb, target, exclude=torch.zeros(3, w + 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="slices"):
        ops.softmax_lse(q, emb, target, slices=-1)
    g, lse = torch.zeros(3), torch.zeros(3)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.softmax_grad(g, torch.zeros(3, 48), torch.zeros(40, 48), target, lse)
    with pytest.raises(ValueError, match="at most 256"):
        ops.softmax_grad(g, torch.zeros(3, 288), torch.zeros(40, 288), target, lse)
    with pytest.raises(ValueError, match=r"lse \[3\]"):
        ops.softmax_grad(g, q, emb, target, torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # the kernels themselves: GPU tensors only
        ops.softmax_lse(q, emb, target)


# ---------------------------------------------------------------------------------- the restatement and the fallback
def _case(decoder="distmult", n=150, b=9, d=32, r=3, seed=0):
    gen = torch.Generator().manual_seed(seed)
    lp = head.LinkPredictor(r, d, decoder=decoder)
    with torch.no_grad():
        lp.relation_embeddings.weight.copy_(torch.randn(r, d, generator=gen))
    emb = torch.randn(n, d, generator=gen)
    h, t = torch.randint(0, n, (b,), generator=gen), torch.randint(0, n, (b,), generator=gen)
    rel = torch.randint(0, r, (b,), generator=gen)
    ei = torch.cat([torch.stack([h, t]), torch.randint(0, n, (2, 400), generator=gen)], dim=1)    # the positives are known
    et = torch.cat([rel, torch.randint(0, r, (400,), generator=gen)])
    known = ops.KnownTriples(ei, et, n, r)
    cls = torch.randint(-1, 3, (n,), generator=gen)
    return lp, emb, h, t, rel, known, cls


def _masks(known, cls, side, anchor, rel, target, n):
    """the bit words the device would get, built on the host"""
    excl = R.pack_bits(head.known_mask(known, side, anchor, rel).numpy())
    allow = R.pack_bits(np.stack([(cls.numpy() == c) for c in range(3)]))
    return allow, cls[target].to(torch.int32), excl


@pytest.mark.parametrize("side", ["tail", "head"])
def test_restatement_agrees_with_autograd_of_the_fallback_in_float64(side):
    lp, emb, h, t, rel, known, cls = _case()
    n, b = emb.size(0), h.numel()
    anchor, target = (h, t) if side == "tail" else (t, h)
    lp64 = head.LinkPredictor(3, 32).double()
    lp64.load_state_dict({k: v.double() for k, v in lp.state_dict().items()})
    emb64 = emb.double().requires_grad_(True)
    loss, hit = lp64._softmax_loss_torch(emb64, h, t, rel, side, known, cls)
    gen = torch.Generator().manual_seed(5)
    g = torch.rand(b, generator=gen, dtype=torch.float64)
    (loss * g).sum().backward()
    # the restatement from (q, E): q = anchor row o relation row, exact in float64
    relw = lp64.relation_embeddings.weight.detach()
    q = (emb64.detach()[anchor] * relw[rel]).numpy()
    allow, qcls, excl = _masks(known, cls, side, anchor, rel, target, n)
    ok = R.eligible(b, n, target, allow, qcls, excl)
    assert ok[np.arange(b), target.numpy()].all() and R.unpack_bits(excl, n)[np.arange(b), target.numpy()].all()
    s = q @ emb64.detach().numpy().T
    f = R.forward(s, ok, target)
    np.testing.assert_allclose(f["loss"], loss.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert (f["hit"] == hit.numpy()).all()
    c, _ = R.coefficients(g, s, f["lse"], ok, target)
    assert np.abs(c.sum(axis=1)).max() < 1e-12                   # softmax minus one-hot sums to zero
    dq, de = c @ emb64.detach().numpy(), c.T @ q
    grad_emb = de.copy()
    np.add.at(grad_emb, anchor.numpy(), dq * relw[rel].numpy())
    grad_rel = np.zeros((3, 32))
    np.add.at(grad_rel, rel.numpy(), dq * emb64.detach()[anchor].numpy())
    np.testing.assert_allclose(grad_emb, emb64.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(grad_rel, lp64.relation_embeddings.weight.grad.numpy(), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("side", ["tail", "head"])
def test_fallback_in_float32_stays_inside_the_bounds_the_device_gets(side):
    lp, emb, h, t, rel, known, cls = _case(seed=1)
    n, b = emb.size(0), h.numel()
    anchor, target = (h, t) if side == "tail" else (t, h)
    with torch.no_grad():
        loss, hit = lp._softmax_loss_torch(emb, h, t, rel, side, known, cls)
    q = emb[anchor] * lp.relation_embeddings.weight.detach()[rel]              # one fp32 product per entry: the fallback's bits
    allow, qcls, excl = _masks(known, cls, side, anchor, rel, target, n)
    ok = R.eligible(b, n, target, allow, qcls, excl)
    s64, sb = R.scores(q, emb), R.score_bound(q, emb)
    f = R.forward(s64, ok, target)
    lb = R.lse_bound(sb, ok, f["lse"], R.chain_steps(b, n))
    bound = R.loss_bound(lb, sb, target, f["loss"])
    err = np.abs(loss.double().numpy() - f["loss"])
    print("fallback fp32 |loss - loss64| max", err.max(), "bound min", bound.min())
    assert (err <= bound).all()


def test_the_target_is_eligible_when_its_own_exclude_bit_is_set_and_when_nothing_is_allowed():
    n, b = 70, 4
    target = torch.tensor([0, 33, 69, 5])
    excl = np.zeros((b, n), dtype=bool)
    excl[np.arange(b), target.numpy()] = True
    excl[:, 7] = True
    allow = R.pack_bits(np.zeros((1, n), dtype=bool))                          # the class allows nothing
    ok = R.eligible(b, n, target, allow, torch.zeros(b, dtype=torch.int32), R.pack_bits(excl))
    assert ok.sum() == b and ok[np.arange(b), target.numpy()].all()
    ok = R.eligible(b, n, target, None, None, R.pack_bits(excl))
    assert ok.sum() == b * (n - 1) and not ok[:, 7].any()
    ok = R.eligible(b, n, target, R.pack_bits(np.ones((2, n), dtype=bool)), torch.tensor([0, 1, 2, -1], dtype=torch.int32))
    assert ok.sum(axis=1).tolist() == [n, n, 1, 1]                             # a class outside [0, C): the target alone
    s = np.zeros((b, n))
    f = R.forward(s, R.eligible(b, n, target, None, None, R.pack_bits(excl)), target)
    np.testing.assert_allclose(f["loss"], np.log(n - 1), rtol=1e-15)           # n - 2 others and the struck target itself
    # the same through the package's torch specification: equal scores, so the loss is the log of the eligible count
    lp = head.LinkPredictor(1, 8).double()
    emb = torch.ones(n, 8, dtype=torch.float64)
    heads, rel = torch.tensor([1, 2, 3, 4]), torch.zeros(b, dtype=torch.int64)
    known = ops.KnownTriples(torch.stack([torch.cat([heads, heads]), torch.cat([target, torch.full((b,), 7)])]),
                             torch.zeros(2 * b, dtype=torch.int64), n, 1)      # every positive is known, and tail 7
    with torch.no_grad():
        loss, hit = lp._softmax_loss_torch(emb, heads, target, rel, "tail", known, None)
        np.testing.assert_allclose(loss.numpy(), np.log(n - 1), rtol=1e-14)
        assert bool(hit.all())
        nothing = torch.full((n,), -1)                                         # no entity has a class: nothing is allowed
        loss, hit = lp._softmax_loss_torch(emb, heads, target, rel, "tail", known, nothing)
        assert bool((loss == 0).all()) and bool(hit.all())                     # the target alone: log 1
        apart = torch.zeros(n, dtype=torch.int64)
        apart[target] = 1                                                      # the targets' class holds the four targets
        loss, _ = lp._softmax_loss_torch(emb, heads, target, rel, "tail", None, apart)
        np.testing.assert_allclose(loss.numpy(), np.log(4), rtol=1e-14)


# ---------------------------------------------------------------------------------- train.py
class _TableModel(nn.Module):
    """an embedding table for an encoder and the package's scoring head - on the CPU the head's softmax loss is its
    torch specification - with the two methods the trainer's softmax path calls"""

    def __init__(self, n, r, d):
        super().__init__()
        self.table = nn.Embedding(n, d)
        self.decoder = head.LinkPredictor(r, d)

    def encoder(self, edge_index, edge_type):
        return self.table.weight

    def softmax_loss(self, edge_index, edge_type, heads, tails, rels, **kwargs):
        return self.decoder.softmax_loss(self.encoder(edge_index, edge_type), heads, tails, rels, **kwargs)


def test_cli_parses_the_loss_and_refuses_what_has_no_meaning(tmp_path):
    args = train.parse_args([])
    assert args.loss == "bce" and args.softmax_sides == "both"
    args = train.parse_args(["--loss", "softmax", "--softmax_sides", "tail"])
    assert args.loss == "softmax" and args.softmax_sides == "tail"
    with pytest.raises(SystemExit):
        train.parse_args(["--loss", "hinge"])
    data = train.synthetic_data(400, seed=3)
    for extra, why in ((["--torch_sampler"], "no sampler"), (["--num_neg_samples", "4"], "no negatives")):
        args = train.parse_args(["--loss", "softmax", "--device", "cpu", "--output_dir", str(tmp_path)] + extra)
        with pytest.raises(ValueError, match=why):
            train.Trainer(_TableModel(data[0]["num_nodes"], 3, 8), data[0], data[1], data[2], torch.device("cpu"), args)


def test_two_epochs_on_the_cpu_and_the_loss_falls(tmp_path):
    torch.manual_seed(0)
    tr, va, full, _ = train.synthetic_data(1200, seed=3)
    args = train.parse_args(["--loss", "softmax", "--device", "cpu", "--synthetic", "--batch_size", "256", "--lr", "0.05",
                             "--epochs", "2", "--filtered_negatives", "--output_dir", str(tmp_path)])
    trainer = train.Trainer(_TableModel(tr["num_nodes"], tr["num_relations"], 16), tr, va, full, torch.device("cpu"), args)
    assert trainer.softmax and trainer.softmax_sides == ("tail", "head") and not trainer.use_hip_graph
    assert trainer._sm_known is not None and not trainer.constrained_negatives
    trainer.train()
    assert len(trainer.train_losses) == 2 and trainer.train_losses[1] < trainer.train_losses[0]
    assert np.isfinite(trainer.val_losses).all() and trainer.best_val_loss == min(trainer.val_losses)
    ckpt = torch.load(tmp_path / "models" / "final_model.pt", weights_only=False)
    assert ckpt["args"].loss == "softmax" and ckpt["args"].softmax_sides == "both"
