"""GPU tier: the two decoder heads (csrc/rgcn_decoder_head.h: the frame; csrc/distmult.hip and csrc/complex.hip: the
policies) held to the bytes of the build BEFORE the ComplEx head's copy of the DistMult head was folded into that frame,
in the form of tests/test_ordered_scatter_parent_bits.py (which already holds the indexed DistMult backward).  Moving the
frame into a header changes no product, no sum and no order of additions, so every output buffer must hash to what that
build gave; tests/golden/head_parent.npz keeps a SHA-1 per buffer and the first four rows of each, so that a failure can
show a value (tests/golden/make_head_golden.py wrote it from the case table below).

37 entities, 5 relations.  Gradient buffers start as NaN with ``zero_tables=True``, so an unwritten row shows.  Each case
reaches something the others do not:
  * ``dm_fwd_b70_d36``, ``dm_bce_fwd_b70_d36``  idle lanes at G = 16, a batch that ends inside a workgroup;
  * ``dm_fwd_b5_d260``                  the second trip of the column loop (G = 64 covers 256 columns);
  * ``dm_fwd_b3_d4``                    G = 1;
  * ``cx_*_b70_d72_shared``             m = 36: idle lanes; the backward's 140 slots of one key space;
  * ``cx_bwd_b300_d520_separate``       m = 260: the second trip; five relation segments;
  * ``cx_fwd_b3_d8``, ``cx_bwd_b3_d8``  m = 4: G = 1;
  * ``*_bwd_no_{h,t,r}_idx``            an operand without an index: rows written straight to the caller's [b, d] buffer,
                                        no keys and no scatter for it (b = 37, the entity count);
  * ``*_bwd_no_grad_{h,t,r}``           the optional outputs;
  * ``*_bwd_empty``                     batch = 0: the memset path, every buffer whole and zero;
  * ``cx_query_*``                      csrc/complex.hip's query launch, whose flag lookup is the library's one;
  * ``dm_fwd_bad_*``, ``cx_bwd_bad_*``  an id outside its table in one index vector: row 0 is used, the outputs are the
                                        recorded ones, and ``ops.check_indices`` raises once, then not again."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, need_gpu
from primekg_rgcn_linkprediction_amd import ops
from test_ordered_scatter_parent_bits import KEPT_ROWS, N_ENT, N_REL, digest, head_rows

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "head_parent.npz")
OPS = {"dm": (ops.distmult_fwd, ops.distmult_bce_fwd, ops.distmult_bwd, ops.distmult_bce_bwd),
       "cx": (ops.complex_fwd, ops.complex_bce_fwd, ops.complex_bwd, ops.complex_bce_bwd)}
BAD_IDS = {"h": N_ENT, "t": -1, "r": 1 << 40}            # just past the table, negative, past int32


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _operands(gen, dev, batch, d, shared=False, no_idx=None, bad=None):
    """-> (h, h_idx, t, t_idx, r, r_idx); ``no_idx``: that operand is [batch, d] without an index vector; ``bad``: that
    index vector holds one id outside its table, in the batch's second-to-last place"""
    rows = {k: batch if no_idx == k else n for k, n in (("h", N_ENT), ("t", N_ENT), ("r", N_REL))}
    h = _randn(gen, rows["h"], d).to(dev)
    t = h if shared else _randn(gen, rows["t"], d).to(dev)
    r = _randn(gen, rows["r"], d).to(dev)
    idx = {}
    for k, n in (("h", N_ENT), ("t", N_ENT), ("r", N_REL)):
        v = torch.randint(0, n, (batch,), generator=gen)
        if bad == k:
            v[batch - 2] = BAD_IDS[k]
        idx[k] = None if no_idx == k else v.to(dev)
    return h, idx["h"], t, idx["t"], r, idx["r"]


def _raises_once(dev):
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        ops.check_indices(dev)
    ops.check_indices(dev)                                   # read and cleared


def _fwd(head, seed, batch, d, shared=False, bce=False, bad=None):
    def run(dev):
        gen = torch.Generator().manual_seed(seed)
        x = _operands(gen, dev, batch, d, shared=shared, bad=bad)
        if bce:
            labels = (torch.rand(batch, generator=gen) < 0.5).float().to(dev)
            scores, loss = OPS[head][1](*x, labels, batch)
            out = {"scores": scores, "loss": loss}
        else:
            out = {"scores": OPS[head][0](*x, batch)}
        if bad:
            _raises_once(dev)
        return out
    return run


def _bwd(head, seed, batch, d, shared=False, bce=False, no_idx=None, no_grad=None, bad=None):
    def run(dev):
        gen = torch.Generator().manual_seed(seed)
        h, hi, t, ti, r, ri = _operands(gen, dev, batch, d, shared=shared, no_idx=no_idx, bad=bad)
        gh = None if no_grad == "h" else _nan(dev, *h.shape)
        gt = None if no_grad == "t" else (gh if shared else _nan(dev, *t.shape))
        gr = None if no_grad == "r" else _nan(dev, *r.shape)
        if bce:
            scores = _randn(gen, batch).to(dev)
            labels = (torch.rand(batch, generator=gen) < 0.5).float().to(dev)
            gs = torch.tensor([0.75], device=dev)
            OPS[head][3](gs, scores, labels, h, hi, t, ti, r, ri, batch, gh, gt, gr, zero_tables=True)
        else:
            OPS[head][2](_randn(gen, batch).to(dev), h, hi, t, ti, r, ri, batch, gh, gt, gr, zero_tables=True)
        if bad:
            _raises_once(dev)
        out = {"grad_h": gh, "grad_r": gr, "grad_t": None if shared else gt}
        return {k: v for k, v in out.items() if v is not None}
    return run


def _bwd_empty(head, bce):
    def run(dev):
        gen = torch.Generator().manual_seed(40)
        d = 40
        h, t, r = _randn(gen, N_ENT, d).to(dev), _randn(gen, N_ENT, d).to(dev), _randn(gen, N_REL, d).to(dev)
        none = torch.empty(0, dtype=torch.int64, device=dev)
        empty = torch.empty(0, device=dev)
        out = {"grad_h": _nan(dev, N_ENT, d), "grad_t": _nan(dev, N_ENT, d), "grad_r": _nan(dev, N_REL, d)}
        if bce:
            OPS[head][3](torch.tensor([0.75], device=dev), empty, empty, h, none, t, none, r, none, 0, *out.values(),
                         zero_tables=True)
        else:
            OPS[head][2](empty, h, none, t, none, r, none, 0, *out.values(), zero_tables=True)
        for k, g in out.items():
            assert torch.count_nonzero(g).item() == 0 and not torch.isnan(g).any().item(), f"{k} is not whole and zero"
        return out
    return run


def _query(side, indexed):
    def run(dev):
        gen = torch.Generator().manual_seed(50)
        batch, d = 70, 72
        x = _randn(gen, N_ENT if indexed else batch, d).to(dev)
        rel = _randn(gen, N_REL, d).to(dev)
        xi = torch.randint(0, N_ENT, (batch,), generator=gen).to(dev) if indexed else None
        ri = torch.randint(0, N_REL, (batch,), generator=gen).to(dev)
        return {"q": ops.complex_query(x, xi, rel, ri, side)}
    return run


# name -> run(dev) -> {output name: tensor}; shared with tests/golden/make_head_golden.py
CASES = {
    "dm_fwd_b70_d36": _fwd("dm", 1, 70, 36),
    "dm_bce_fwd_b70_d36": _fwd("dm", 2, 70, 36, bce=True),
    "dm_fwd_b5_d260": _fwd("dm", 3, 5, 260),
    "dm_fwd_b3_d4": _fwd("dm", 4, 3, 4),
    "cx_fwd_b70_d72_shared": _fwd("cx", 5, 70, 72, shared=True),
    "cx_bce_fwd_b70_d72_shared": _fwd("cx", 6, 70, 72, shared=True, bce=True),
    "cx_bwd_b70_d72_shared": _bwd("cx", 7, 70, 72, shared=True),
    "cx_bce_bwd_b70_d72_shared": _bwd("cx", 8, 70, 72, shared=True, bce=True),
    "cx_bwd_b300_d520_separate": _bwd("cx", 9, 300, 520),
    "cx_fwd_b3_d8": _fwd("cx", 10, 3, 8),
    "cx_bwd_b3_d8": _bwd("cx", 11, 3, 8),
    "cx_query_tail": _query("tail", True),
    "cx_query_head": _query("head", True),
    "cx_query_tail_rows": _query("tail", False),
    "cx_query_head_rows": _query("head", False),
}
for _n, _head in enumerate(("dm", "cx")):
    for _k, _op in enumerate("htr"):
        CASES[f"{_head}_bwd_no_{_op}_idx"] = _bwd(_head, 20 + 3 * _n + _k, N_ENT, 40, no_idx=_op)
        CASES[f"{_head}_bwd_no_grad_{_op}"] = _bwd(_head, 30 + 3 * _n + _k, 70, 40, no_grad=_op)
    CASES[f"{_head}_bwd_empty"] = _bwd_empty(_head, False)
    CASES[f"{_head}_bce_bwd_empty"] = _bwd_empty(_head, True)
for _k, _op in enumerate("htr"):
    CASES[f"dm_fwd_bad_{_op}_idx"] = _fwd("dm", 60 + _k, 70, 36, bad=_op)
    CASES[f"cx_bwd_bad_{_op}_idx"] = _bwd("cx", 70 + _k, 70, 72, bad=_op)


def outputs(name, dev):
    """-> {output name: contiguous numpy array} of one case"""
    got = CASES[name](dev)
    torch.cuda.synchronize()
    ops.check_indices(dev)
    return {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in got.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_output_has_the_parent_builds_bytes(name):
    dev = need_gpu()
    got = outputs(name, dev)
    with np.load(FIXTURE) as z:
        recorded = sorted(k[len(name) + 1:-len("_sha1")] for k in z.files if k.startswith(name + "/") and k.endswith("_sha1"))
        assert recorded == sorted(got), f"{name}: the fixture holds {recorded}, the case gives {sorted(got)}"
        for out, a in got.items():
            rows, sha = z[f"{name}/{out}_rows"], z[f"{name}/{out}_sha1"]
            assert a.dtype == rows.dtype and a.shape[1:] == rows.shape[1:], f"{name}/{out}: {a.dtype} {a.shape}"
            first = head_rows(a)
            assert first.tobytes() == rows.tobytes(), f"{name}/{out}: first rows\n{first}\nrecorded\n{rows}"
            assert np.array_equal(digest(a), sha), f"{name}/{out}: rows past the first {KEPT_ROWS} differ from the recorded bytes"
