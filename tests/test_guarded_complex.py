"""The ComplEx head under the guard bands and poison fills of ``test_guarded.protocol`` (plain / 0x00 / 0xFF / re-based by
16 bytes): no store outside an output or the workspace, inputs unwritten, the same bits in all four runs - so
``complex_bwd_workspace_bytes`` covers the footprint of the contribution launch, the scatter and the relation tree, and
no kernel assumes more of a base address than the 16 bytes the header asks for."""
import pytest
import torch

from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import ops
from test_guarded import _randn, protocol

pytestmark = pytest.mark.gpu

N_ENT, N_REL, D = 50, 5, 24


@pytest.mark.parametrize("batch", [17, 257])
def test_complex_bce_forward_and_backward(batch, monkeypatch):
    """``complex_bce_fwd`` + ``complex_bce_bwd`` on one indexed, shared table.  17 samples: 34 slots, one 64-key stage of
    the scans; 257 samples: 514 slots, nine stages, five segments of the relation tree"""
    dev = need_gpu()
    gen = torch.Generator().manual_seed(1000 * D + batch)
    ent, rel = _randn(gen, N_ENT, D).to(dev), _randn(gen, N_REL, D).to(dev)
    hi, ti = torch.randint(0, N_ENT, (batch,), generator=gen), torch.randint(0, N_ENT, (batch,), generator=gen)
    hi[batch // 2:] = 7                                                    # duplicated ids
    ri = torch.arange(batch) % N_REL
    # the path: a row with >= 3 slots, every relation used, and (257) more than one key stage
    assert int(torch.bincount(torch.cat([hi, ti]), minlength=N_ENT).max()) >= 3
    assert sorted(set(ri.tolist())) == list(range(N_REL))
    assert batch == 17 or 2 * batch > 64
    hi, ti, ri = hi.to(dev), ti.to(dev), ri.to(dev)
    labels = (torch.rand(batch, generator=gen) > 0.5).float().to(dev)
    one = torch.ones(1, device=dev)

    def fn(ctx):
        out = {}
        scores, loss = out["bce_fwd"] = ops.complex_bce_fwd(ent, hi, ent, ti, rel, ri, labels, batch)
        out["mean"] = ops.distmult_bce_reduce(loss, scores, labels)
        gh, gr = ctx.empty(N_ENT, D, device=dev), ctx.empty(N_REL, D, device=dev)
        ops.complex_bce_bwd(one, scores, labels, ent, hi, ent, ti, rel, ri, batch, gh, gh, gr, zero_tables=True)
        out["bce_bwd"] = (gh, gr)
        return out

    protocol(monkeypatch, [ent, rel, hi, ti, ri, labels, one], fn)


def test_complex_query_into_the_ranking_pass(monkeypatch):
    """``complex_query`` on both sides, and the tail side's rows through ``distmult_rank_tails``"""
    dev = need_gpu()
    gen = torch.Generator().manual_seed(300)
    b, n, d = 65, 300, 32
    ent, rel = _randn(gen, n, d).to(dev), _randn(gen, 3, d).to(dev)
    anchor, target = torch.randint(0, n, (b,), generator=gen).to(dev), torch.randint(0, n, (b,), generator=gen).to(dev)
    ri = torch.randint(0, 3, (b,), generator=gen).to(dev)

    def fn(ctx):
        q = ops.complex_query(ent, anchor, rel, ri, "tail")
        true_score = ops.complex_fwd(ent, anchor, ent, target, rel, ri, b)   # a library launch: no torch reduction in here
        return {"q": q, "q head": ops.complex_query(ent, anchor, rel, ri, "head"), "true": true_score,
                "rank": ops.distmult_rank_tails(q, ent, true_score, target)}

    protocol(monkeypatch, [ent, rel, anchor, target, ri], fn)
