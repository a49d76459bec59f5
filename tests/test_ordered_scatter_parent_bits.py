"""GPU tier: the ordered scatter (csrc/rgcn_ordered_match.h: the DistMult backward, rgcn_segment_sum, the loss reductions
and the TransE step), and the two batch samplers over their shared core (csrc/rgcn_sample_core.h), held to the bytes of
the build BEFORE their duplicated code was folded into those two headers.  Moving code between files changes no sum, no
order of additions and no random draw, so every output buffer must hash to what that build gave;
tests/golden/ordered_scatter_parent.npz keeps a SHA-1 per buffer and the first four rows of each, so that a failure can
show a value (tests/golden/make_ordered_scatter_golden.py wrote it from the case table below).

Each case reaches a path the others do not:
  * ``bwd_b70_d36_shared``     140 slots of one key space: two 64-key stages of the scans, idle lanes at G = 16;
  * ``bwd_b300_d260_separate`` the second 256-column trip of the row loops, five 64-sample relation segments;
  * ``bwd_b8200_d12_shared``   16,400 slots, past the 16,384 the scatter stages in LDS: keys read from global memory;
                               43 relation segments: three trips of the combine pass's sixteen-at-a-time loop;
  * ``bce_bwd_b70_d36_shared`` the BCE coefficient of the contribution launch;
  * ``segment_sum``            the relation tree alone, a ragged fifth segment;
  * ``bce_reduce``             the 1,024-thread tree with one element in a second trip, all three accumulators;
  * ``transe_*``               cases of tests/test_transe.py: 68 slots, a hub of 40 slots, 8,196 keys (the global-keys
                               instance of the apply launch) and a step in which no sample is active;
  * ``sample_*``               a window that runs past the last column, through ``order``; the constrained sampler with
                               classes and known triples, and with nothing given and one try (the plain sampler's bits)."""
import hashlib
import os

import numpy as np
import pytest
import torch

import test_transe as TT
from conftest import GOLDEN, need_gpu
from primekg_rgcn_linkprediction_amd import ops

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "ordered_scatter_parent.npz")
N_ENT, N_REL = 37, 5
KEPT_ROWS = 4


def digest(a):
    return np.frombuffer(hashlib.sha1(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------- DistMult backward
def _distmult_bwd(seed, batch, d, shared, bce):
    def run(dev):
        gen = torch.Generator().manual_seed(seed)
        h = _randn(gen, N_ENT, d).to(dev)
        t = h if shared else _randn(gen, N_ENT, d).to(dev)
        r = _randn(gen, N_REL, d).to(dev)
        hi, ti = (torch.randint(0, N_ENT, (batch,), generator=gen).to(dev) for _ in range(2))
        ri = torch.randint(0, N_REL, (batch,), generator=gen).to(dev)
        gh = _nan(dev, N_ENT, d)
        gt = gh if shared else _nan(dev, N_ENT, d)
        gr = _nan(dev, N_REL, d)
        if bce:
            scores = _randn(gen, batch).to(dev)
            labels = (torch.rand(batch, generator=gen) < 0.5).float().to(dev)
            gs = torch.tensor([0.75], device=dev)
            ops.distmult_bce_bwd(gs, scores, labels, h, hi, t, ti, r, ri, batch, gh, gt, gr, zero_tables=True)
        else:
            ops.distmult_bwd(_randn(gen, batch).to(dev), h, hi, t, ti, r, ri, batch, gh, gt, gr, zero_tables=True)
        out = {"grad_h": gh, "grad_r": gr}
        if not shared:
            out["grad_t"] = gt
        return out
    return run


def _segment_sum(dev):
    gen = torch.Generator().manual_seed(21)
    rows = _randn(gen, 257, 20).to(dev)
    idx = torch.randint(0, 5, (257,), generator=gen).to(dev)
    return {"out": ops.segment_sum(rows, idx, 5)}


def _bce_reduce(dev):
    gen = torch.Generator().manual_seed(22)
    loss = torch.rand(1025, generator=gen).to(dev)
    scores = _randn(gen, 1025).to(dev)
    labels = (torch.rand(1025, generator=gen) < 0.5).float().to(dev)
    loss_sum = torch.full((1,), 2.5, dtype=torch.float64, device=dev)
    correct = torch.full((1,), 11, dtype=torch.int64, device=dev)
    cursor = torch.full((1,), 4100, dtype=torch.int64, device=dev)
    mean = ops.distmult_bce_reduce(loss, scores, labels, loss_sum, correct, cursor, cursor_add=1025)
    return {"mean": mean, "loss_sum": loss_sum, "correct": correct, "cursor": cursor}


# ------------------------------------------------------------------------------------------------------- TransE step
def _transe(name, d):
    def run(dev):
        e, r, heads, tails, rels, margin = TT._case(name, d)
        emb, rel, _, loss, loss_sum, active_sum = TT._device_step(dev, e, r, heads, tails, rels, margin)
        return {"emb": emb, "rel": rel, "loss_mean": loss, "loss_sum": np.array([loss_sum], dtype=np.float64),
                "active_sum": np.array([active_sum], dtype=np.int64)}
    return run


# ---------------------------------------------------------------------------------------------------------- samplers
def _sampler(kind):
    def run(dev):
        gen = torch.Generator().manual_seed(23)
        e, b, k = 50, 7, 3
        ei = torch.randint(0, N_ENT, (2, e), generator=gen)
        et = torch.randint(0, N_REL, (e,), generator=gen)
        order = torch.randperm(e, generator=gen).to(dev)
        class_of = torch.randint(0, 3, (N_ENT,), generator=gen)
        cursor = torch.tensor([46], dtype=torch.int64, device=dev)          # the window runs past column 49
        rng = torch.tensor([20240229, 3], dtype=torch.int64, device=dev)
        ei, et = ei.to(dev), et.to(dev)
        if kind == "plain":
            got = ops.sample_batch(ei, et, order, cursor, b, k, N_ENT, rng)
            stats = None
        elif kind == "constrained":
            stats = torch.tensor([5, 1], dtype=torch.int64, device=dev)
            got = ops.sample_batch_constrained(ei, et, order, cursor, b, k, N_ENT, rng, ops.NodeClasses(class_of.to(dev), 3),
                                               ops.KnownTriples(ei, et, N_ENT, N_REL), max_tries=4, stats=stats)
        else:
            got = ops.sample_batch_constrained(ei, et, order, cursor, b, k, N_ENT, rng, None, None, max_tries=1)
            stats = None
        out = dict(zip(("heads", "tails", "rels", "labels"), got))
        if stats is not None:
            out["stats"] = stats
        return out
    return run


# name -> run(dev) -> {output name: tensor or array}; shared with tests/golden/make_ordered_scatter_golden.py
CASES = {
    "bwd_b70_d36_shared": _distmult_bwd(1, 70, 36, True, False),
    "bwd_b300_d260_separate": _distmult_bwd(2, 300, 260, False, False),
    "bwd_b8200_d12_shared": _distmult_bwd(3, 8200, 12, True, False),
    "bce_bwd_b70_d36_shared": _distmult_bwd(4, 70, 36, True, True),
    "segment_sum": _segment_sum,
    "bce_reduce": _bce_reduce,
    "transe_b17_d32": _transe("b17", 32),
    "transe_hub_d64": _transe("hub", 64),
    "transe_b2049_d128": _transe("b2049", 128),
    "transe_nothing_active_d32": _transe("nothing_active", 32),
    "sample_plain": _sampler("plain"),
    "sample_constrained": _sampler("constrained"),
    "sample_constrained_null_t1": _sampler("null_t1"),
}


def outputs(name, dev):
    """-> {output name: contiguous numpy array} of one case"""
    got = CASES[name](dev)
    torch.cuda.synchronize()
    ops.check_indices(dev)
    return {k: np.ascontiguousarray(v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}


def head_rows(a):
    return a[:KEPT_ROWS].copy()


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
            same = first.tobytes() == rows.tobytes()
            assert same, f"{name}/{out}: first rows\n{first}\nrecorded\n{rows}"
            assert np.array_equal(digest(a), sha), f"{name}/{out}: rows past the first {KEPT_ROWS} differ from the recorded bytes"


def test_the_null_constrained_sampler_is_the_plain_sampler():
    """the two fixture entries themselves: recorded from two kernels, one set of bytes"""
    need_gpu()
    with np.load(FIXTURE) as z:
        for out in ("heads", "tails", "rels", "labels"):
            assert np.array_equal(z[f"sample_plain/{out}_sha1"], z[f"sample_constrained_null_t1/{out}_sha1"])
