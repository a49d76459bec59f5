"""GPU tier: the passes that filter candidates - link ranking (csrc/rank_count.hip), top-k (csrc/rank_topk.hip) and the
1-vs-all softmax (csrc/softmax_loss.hip) - and their chunked ``*_filtered`` wrappers held to the bytes of the build BEFORE
the three copies of the candidate filter were folded into csrc/rgcn_candidate_filter.h and one chunk generator in ops.py,
in the form of tests/test_head_parent_bits.py.  The frame changes no load, no product, no sum and no order of additions,
so every output buffer must hash to what that build gave; tests/golden/candidate_filter_parent.npz keeps a SHA-1 per
buffer and its first four rows, so that a failure can show a value (tests/golden/make_candidate_filter_golden.py wrote it
from the case table below).

Shapes, the smallest at which these kernels can go wrong:
  * N = 300: three 128-column tiles, the last ragged, N % 32 != 0, W = 10;  N = 37: one ragged tile, W = 2;
  * B = 70: two row tiles, the second ragged;  B = 3;  B = 200: two 128-row chunks of the softmax wrappers;
  * d = 32, 96, 160, 256: one, three, five and eight k-tiles; NB = 1, 2, 3, 4 of the softmax backward; the widest row.
Filters (``FILTERS``): none, allow only, exclude only, both, three classes with a query of class -1 and one of class 3
(nothing allowed), an exclude row of all ones (and one that leaves two candidates: fewer than k), an exclude row that
strikes the target itself.  Slices 0, 1 and 3; k = 1, 5, 128; ``min_score`` unset and set.  ``*_nonfinite``: a NaN in one
query row and +inf in one entity row.  ``*_filtered_*``: a ``KnownTriples`` over 400 random triples, at the default
``max_mask_bytes`` (one chunk), at 2,560 bytes with B = 70 (chunks 0-64, 64-70) and, for the softmax pair, at 6,000 bytes
with B = 200 (chunks 0-128, 128-200).  Inputs come from seeded CPU generators; the true scores of the ranking cases are
drawn, not computed, so no host arithmetic enters the recorded bytes."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, need_gpu
from primekg_rgcn_linkprediction_amd import ops
from test_ordered_scatter_parent_bits import KEPT_ROWS, digest, head_rows

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "candidate_filter_parent.npz")
FILTERS = ("none", "allow", "excl", "both", "classes3", "excl_ones", "excl_target")
N_REL, N_KNOWN = 5, 400


def _bits(rows):
    """bool [R, N] -> int32 [R, W]: entity n is bit (n & 31) of word (n >> 5)"""
    r, n = rows.shape
    padded = np.zeros((r, ops.mask_words(n) * 32), dtype=np.uint8)
    padded[:, :n] = rows.numpy()
    return torch.from_numpy(np.packbits(padded, axis=1, bitorder="little").view(np.uint32).view(np.int32).copy())


def _inputs(seed, b, n, d, filt="none", nonfinite=False):
    """-> (gen, q, emb, target, allow, query_class, exclude), CPU tensors"""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(b, d, generator=gen) * 0.5
    emb = torch.randn(n, d, generator=gen) * 0.5
    target = torch.randint(0, n, (b,), generator=gen)
    allow = qcls = excl = None
    if filt in ("allow", "both", "classes3"):
        c = 3 if filt == "classes3" else 2
        class_of = torch.randint(0, c, (n,), generator=gen)
        allow = _bits(class_of[None, :] == torch.arange(c)[:, None])
        qcls = torch.randint(0, c, (b,), generator=gen).to(torch.int32)
        if filt == "classes3":
            qcls[0], qcls[1] = -1, 3                             # outside [0, C): nothing is allowed
    if filt in ("excl", "both", "classes3", "excl_ones", "excl_target"):
        struck = torch.rand(b, n, generator=gen) < 0.3
        if filt == "excl_ones":
            struck[1] = True
            struck[0] = True
            struck[0, 4 % n] = struck[0, 9 % n] = False          # two candidates left: fewer than k = 5
        if filt == "excl_target":
            struck[2, target[2]] = True
        excl = _bits(struck)
    if nonfinite:
        q[1, 3] = float("nan")
        emb[5, 2] = float("inf")
    return gen, q, emb, target, allow, qcls, excl


def _to(dev, *ts):
    return tuple(None if t is None else t.to(dev) for t in ts)


def _rank(seed, b, n, d, filt=None, nonfinite=False):
    """``filt=None``: ``distmult_rank_tails``"""
    def run(dev):
        gen, q, emb, target, allow, qcls, excl = _inputs(seed, b, n, d, filt or "none", nonfinite)
        true_score = torch.randn(b, generator=gen) * (0.125 * d ** 0.5)
        q, emb, target, allow, qcls, excl, true_score = _to(dev, q, emb, target, allow, qcls, excl, true_score)
        if filt is None:
            return {"ranks": ops.distmult_rank_tails(q, emb, true_score, target)}
        return {"ranks": ops.distmult_rank_masked(q, emb, true_score, target, allow, qcls, excl)}
    return run


def _topk(seed, b, n, d, k, filt="none", slices=0, min_score=None, nonfinite=False):
    def run(dev):
        _, q, emb, _, allow, qcls, excl = _inputs(seed, b, n, d, filt, nonfinite)
        q, emb, allow, qcls, excl = _to(dev, q, emb, allow, qcls, excl)
        ids, scores = ops.distmult_topk_masked(q, emb, k, allow, qcls, excl, min_score, slices)
        return {"ids": ids, "scores": scores}
    return run


LSE_OUT = ("lse", "true_score", "row_max", "loss", "hit")


def _softmax(seed, b, n, d, filt="none", slices=0, grad=False, nonfinite=False):
    def run(dev):
        gen, q, emb, target, allow, qcls, excl = _inputs(seed, b, n, d, filt, nonfinite)
        g = torch.randn(b, generator=gen)
        start = torch.randn(n, d, generator=gen)                 # what demb holds before an accumulating call
        q, emb, target, allow, qcls, excl, g, start = _to(dev, q, emb, target, allow, qcls, excl, g, start)
        out = dict(zip(LSE_OUT, ops.softmax_lse(q, emb, target, allow, qcls, excl, slices, with_loss=True)))
        if grad:
            out["dq"], out["demb"] = ops.softmax_grad(g, q, emb, target, out["lse"], allow, qcls, excl, slices)
            _, out["demb_acc"] = ops.softmax_grad(g, q, emb, target, out["lse"], allow, qcls, excl, slices, need_dq=False,
                                                  demb=start, accumulate=True)
        return out
    return run


def _filtered(what, seed, b, d, max_mask_bytes=None, with_allow=False):
    """the four chunked wrappers over N = 300 and a ``KnownTriples`` of ``N_KNOWN`` random triples"""
    n = 300

    def run(dev):
        gen, q, emb, target, allow, qcls, _ = _inputs(seed, b, n, d, "allow" if with_allow else "none")
        edge_index = torch.randint(0, n, (2, N_KNOWN), generator=gen)
        edge_type = torch.randint(0, N_REL, (N_KNOWN,), generator=gen)
        # half of the queries are known triples' (head, relation): their exclude rows are not empty
        pick = torch.randint(0, N_KNOWN, (b,), generator=gen)
        anchor = torch.where(torch.arange(b) % 2 == 0, edge_index[0, pick], torch.randint(0, n, (b,), generator=gen))
        rel = edge_type[pick]
        true_score = torch.randn(b, generator=gen) * (0.125 * d ** 0.5)
        g = torch.randn(b, generator=gen)
        start = torch.randn(n, d, generator=gen)
        q, emb, target, allow, qcls, anchor, rel, true_score, g, start = _to(dev, q, emb, target, allow, qcls, anchor, rel,
                                                                             true_score, g, start)
        known = ops.KnownTriples(edge_index.to(dev), edge_type.to(dev), n, N_REL)
        kw = dict(known=known, side="tail", anchor_idx=anchor, rel_idx=rel, allow=allow, query_class=qcls)
        if max_mask_bytes is not None:
            kw["max_mask_bytes"] = max_mask_bytes
        if what == "rank":
            return {"ranks": ops.distmult_rank_filtered(q, emb, true_score, target, **kw)}
        if what == "topk":
            ids, scores = ops.distmult_topk_filtered(q, emb, 5, **kw)
            return {"ids": ids, "scores": scores}
        out = dict(zip(LSE_OUT, ops.softmax_lse_filtered(q, emb, target, **kw)))
        out["dq"], out["demb"] = ops.softmax_grad_filtered(g, q, emb, target, out["lse"], **kw)
        _, out["demb_acc"] = ops.softmax_grad_filtered(g, q, emb, target, out["lse"], need_dq=False, demb=start,
                                                       accumulate=True, **kw)
        return out
    return run


# name -> run(dev) -> {output name: tensor}; shared with tests/golden/make_candidate_filter_golden.py
CASES = {
    "rank_tails_b70_n300_d96": _rank(1, 70, 300, 96),
    "rank_tails_b3_n37_d32": _rank(2, 3, 37, 32),
    "rank_tails_b70_n37_d256": _rank(3, 70, 37, 256),
    "rank_tails_nonfinite": _rank(4, 70, 300, 96, nonfinite=True),
    "rank_masked_b3_n37_d32_both": _rank(5, 3, 37, 32, "both"),
    "rank_masked_b70_n37_d256_classes3": _rank(6, 70, 37, 256, "classes3"),
    "rank_masked_nonfinite": _rank(7, 70, 300, 96, "both", nonfinite=True),
    "topk_b3_n37_d32_k1_slices1": _topk(20, 3, 37, 32, 1, slices=1),
    "topk_b3_n37_d32_k128_excl": _topk(21, 3, 37, 32, 128, "excl"),
    "topk_b70_n300_d256_k128_both_slices3_floor": _topk(22, 70, 300, 256, 128, "both", slices=3, min_score=0.5),
    "topk_b70_n300_d96_k5_classes3_slices3_floor": _topk(23, 70, 300, 96, 5, "classes3", slices=3, min_score=-1.0),
    "topk_b70_n300_d32_k1_allow_slices1": _topk(24, 70, 300, 32, 1, "allow", slices=1),
    "topk_nonfinite": _topk(25, 70, 300, 96, 5, "both", nonfinite=True),
    "softmax_b3_n37_d32_both_slices1": _softmax(40, 3, 37, 32, "both", slices=1, grad=True),
    "softmax_b70_n300_d32_excl_slices3": _softmax(41, 70, 300, 32, "excl", slices=3, grad=True),
    "softmax_b70_n300_d160_allow": _softmax(42, 70, 300, 160, "allow", grad=True),
    "softmax_b70_n300_d256_classes3_slices3": _softmax(43, 70, 300, 256, "classes3", slices=3, grad=True),
    "softmax_b200_n300_d96_both_slices1": _softmax(44, 200, 300, 96, "both", slices=1, grad=True),
    "softmax_nonfinite": _softmax(45, 70, 300, 96, "both", grad=True, nonfinite=True),
}
for _i, _f in enumerate(FILTERS):
    CASES[f"rank_masked_b70_n300_d96_{_f}"] = _rank(10 + _i, 70, 300, 96, _f)
    CASES[f"topk_b70_n300_d96_k5_{_f}"] = _topk(30 + _i, 70, 300, 96, 5, _f)
    CASES[f"softmax_b70_n300_d96_{_f}"] = _softmax(50 + _i, 70, 300, 96, _f, grad=True)
for _i, _what in enumerate(("rank", "topk", "softmax")):
    CASES[f"{_what}_filtered_b70_one_chunk"] = _filtered(_what, 60 + _i, 70, 96)
    CASES[f"{_what}_filtered_b70_2560_bytes"] = _filtered(_what, 63 + _i, 70, 96, 2560, with_allow=True)
CASES["softmax_filtered_b200_6000_bytes"] = _filtered("softmax", 66, 200, 32, 6000)
CASES["softmax_filtered_b200_one_chunk"] = _filtered("softmax", 67, 200, 32, with_allow=True)


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
