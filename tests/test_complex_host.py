"""CPU tier of the ComplEx head (``csrc/complex.hip``, ``include/rgcn_complex.h``, ``head.py``): the C surface, every
argument check that runs before a launch (sizes, NULLs, alignment with the fake addresses of ``c_surface.py``),
and the float64 restatement the GPU tier judges the kernels by (``complex_reference.py``) against itself: the two query
operands on integer data, exactly, and the six gradient products against torch autograd of the score."""
import os

import pytest
import torch

import c_surface as S
import complex_reference as R
from c_surface import STREAM, T4, T8, T16
from conftest import ROOT
from primekg_rgcn_linkprediction_amd import _lib, head, ops

OK, ARG = _lib.RGCN_OK, _lib.RGCN_ERR_ARG


def _ws(batch=1, d=8, r=1):
    return lambda: _lib.load().complex_bwd_workspace_bytes(batch, d, r)


# argument sets at the smallest legal sizes, parameter by parameter, in the notation of c_surface.py
CASES = {
    "complex_fwd": [T16, T8, 1, T16, T8, 1, T16, T8, 1, 1, 8, T4, STREAM],
    "complex_bce_fwd": [T16, T8, 1, T16, T8, 1, T16, T8, 1, T4, 1, 8, T4, T4, STREAM],
    "complex_bwd": [T4, T16, T8, 1, T16, T8, 1, T16, T8, 1, 1, 8, T16, T16, T16, T16, _ws(), 1, STREAM],
    "complex_bce_bwd": [T4, T4, T4, T16, T8, 1, T16, T8, 1, T16, T8, 1, 1, 8, T16, T16, T16, T16, _ws(), 1, STREAM],
    "rgcn_complex_query": [0, T16, T8, 1, T16, T8, 1, 1, 8, T16, STREAM],
}
ALIGNMENT_CASES = {name: [args] for name, args in CASES.items()}
BATCH_AT = {"complex_fwd": 9, "complex_bce_fwd": 10, "complex_bwd": 10, "complex_bce_bwd": 12, "rgcn_complex_query": 7}


# ---------------------------------------------------------------------------------- C surface
def test_header_table_and_library_agree():
    """names, parameters, return types and exports: test_c_surface.py, for every header.  Here: the DistMult head's
    operand convention, parameter for parameter"""
    for ours, theirs in (("complex_fwd", "distmult_fwd"), ("complex_bce_fwd", "distmult_bce_fwd"), ("complex_bwd", "distmult_bwd"),
                         ("complex_bce_bwd", "distmult_bce_bwd"), ("complex_bwd_workspace_bytes", "distmult_bwd_workspace_bytes")):
        assert _lib.COMPLEX_PROTOTYPES[ours] == _lib.PROTOTYPES[theirs]
    makefile = open(os.path.join(ROOT, "primekg_rgcn_linkprediction_amd", "csrc", "Makefile")).read()
    assert " complex.hip" in makefile


def _values(name, **changes):
    args = list(CASES[name])
    for pos, v in changes.items():
        args[int(pos)] = v
    values, keep = S.build(args)
    return values, keep


@pytest.mark.parametrize("name", sorted(CASES))
def test_sizes_and_nulls_are_refused_without_a_gpu(name):
    lib = _lib.load()
    fn = getattr(lib, name)
    args = CASES[name]
    d_at = BATCH_AT[name] + 1
    assert args[BATCH_AT[name]] == 1 and args[d_at] == 8
    for bad_d in (12, 4, 0, -8, 9):                                      # d & 7 (and d <= 0): RGCN_ERR_ARG
        values, keep = _values(name, **{str(d_at): bad_d})
        assert fn(*values) == ARG, (name, bad_d)
    values, keep = _values(name, **{str(BATCH_AT[name]): -1})
    assert fn(*values) == ARG
    # batch = 0: RGCN_OK before any pointer is looked at - every pointer NULL (the backward with nothing to clear)
    empty = [None if isinstance(a, S.Dev) else a for a in args]
    empty[BATCH_AT[name]] = 0
    if name.endswith("bwd"):
        empty[-2] = 0                                                    # zero_tables off: nothing to clear, no HIP call
    values, keep = S.build(empty)
    assert fn(*values) == OK, name
    bad = list(empty)
    bad[d_at] = 12
    values, keep = S.build(bad)
    assert fn(*values) == ARG                                            # the size check comes first
    # a needed pointer NULL with batch > 0.  Index vectors and gradients are optional: with one of those NULL the set
    # would pass every check and launch on fake addresses, so they are never called here
    for pos, a in enumerate(args):
        optional = name.endswith("bwd") and pos in (len(args) - 7, len(args) - 6, len(args) - 5)
        if isinstance(a, S.Dev) and a.align != 8 and not optional:
            values, keep = _values(name, **{str(pos): None})
            code = fn(*values)
            if name.endswith("bwd") and pos == len(args) - 4:
                assert code == _lib.RGCN_ERR_WORKSPACE, (name, pos, code)
            else:
                assert code == ARG, (name, pos, code)
    if name == "rgcn_complex_query":
        for side in (-1, 2):
            values, keep = _values(name, **{"0": side})
            assert fn(*values) == ARG
    if name.endswith("bwd"):
        need = lib.complex_bwd_workspace_bytes(1, 8, 1)
        values, keep = _values(name, **{str(len(args) - 3): need - 1})
        assert fn(*values) == _lib.RGCN_ERR_WORKSPACE
        values, keep = _values(name, **{str(BATCH_AT[name]): (1 << 31) // 4 + 1, str(len(args) - 3): 1 << 62})
        assert fn(*values) == _lib.RGCN_ERR_UNSUPPORTED


def test_workspace_query():
    q = _lib.load().complex_bwd_workspace_bytes
    assert q(0, 8, 3) == q(-1, 8, 3) == q(5, 0, 3) == 0
    assert q(5, 8, 0) >= 3 * 5 * 8 * 4 + 3 * 5 * 4
    assert q(5, 8, 3) >= q(5, 8, 0) + 3 * 8 * 4 and q(257, 8, 3) >= 3 * 257 * 8 * 4 + 5 * 3 * 8 * 4 + 3 * 257 * 4
    assert q(5, 8, 3) == _lib.load().distmult_bwd_workspace_bytes(5, 8, 3)


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_pointer_below_its_alignment_is_refused(name):
    args = CASES[name]
    pointers = sum(S.is_pointer(ty) for ty in _lib.COMPLEX_PROTOTYPES[name][1])
    assert len(S.targets(name, args)) == pointers - 1                      # all but the stream
    failed = S.misaligned_refusals(getattr(_lib.load(), name), name, args)
    assert not failed, "; ".join(failed)


# ---------------------------------------------------------------------------------- wrappers and the module
def test_wrappers_refuse_by_name(monkeypatch):
    e, r = torch.zeros(10, 16), torch.zeros(3, 16)
    idx = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="head is on cpu.*no CPU fallback"):
        ops.complex_fwd(e, idx, e, idx, r, idx, 5)
    with pytest.raises(RuntimeError, match="x is on cpu"):
        ops.complex_query(e, idx, r, idx, "tail")
    with pytest.raises(ValueError, match="side"):
        ops.complex_query(e, idx, r, idx, "both")

    def need(name, t, dtype):
        if t.dtype != dtype:
            raise TypeError(f"{name} must be {dtype}, got {t.dtype}")

    monkeypatch.setattr(ops, "_need_gpu", need)
    labels = torch.zeros(5)
    for fn, extra in ((ops.complex_fwd, ()), (ops.complex_bce_fwd, (labels,))):
        with pytest.raises(ValueError, match="embedding dim must be a multiple of 8"):
            fn(torch.zeros(10, 12), idx, torch.zeros(10, 12), idx, torch.zeros(3, 12), idx, *extra, 5)
        with pytest.raises(ValueError, match="dims differ"):
            fn(e, idx, e, idx, torch.zeros(3, 8), idx, *extra, 5)
        with pytest.raises(ValueError, match=r"head_idx must be \[5\]"):
            fn(e, idx[:4], e, idx, r, idx, *extra, 5)
        with pytest.raises(ValueError, match="tail must have 5 rows when no index is given"):
            fn(e, idx, e, None, r, idx, *extra, 5)
        with pytest.raises(ValueError, match="rel must be 2-D"):
            fn(e, idx, e, idx, torch.zeros(16), idx, *extra, 5)
        with pytest.raises(TypeError, match="tail_idx"):
            fn(e, idx, e, idx.int(), r, idx, *extra, 5)
    with pytest.raises(ValueError, match=r"labels must be \[5\]"):
        ops.complex_bce_fwd(e, idx, e, idx, r, idx, torch.zeros(4), 5)
    with pytest.raises(ValueError, match="grad_mean_loss must hold one float"):
        ops.complex_bce_bwd(torch.zeros(2), labels, labels, e, idx, e, idx, r, idx, 5, None, None, None)
    with pytest.raises(ValueError, match="embedding dim must be a multiple of 8"):
        ops.complex_query(torch.zeros(5, 12), None, torch.zeros(3, 12), idx, "head")
    with pytest.raises(ValueError, match="dims differ"):
        ops.complex_query(e, idx, torch.zeros(3, 8), idx, "head")


def test_an_unknown_decoder_raises():
    with pytest.raises(ValueError, match="decoder"):
        head.LinkPredictor(3, 16, decoder="bogus")
    with pytest.raises(ValueError, match="multiple of 8"):
        head.LinkPredictor(3, 12, decoder="complex")
    from primekg_rgcn_linkprediction_amd.model import DrugDiseaseModel
    with pytest.raises(ValueError, match="decoder"):
        DrugDiseaseModel(10, 3, 8, 16, decoder="bogus")
    a, b = head.LinkPredictor(3, 16), head.LinkPredictor(3, 16, decoder="complex")
    assert a.decoder == "distmult" and b.decoder == "complex"
    assert list(a.state_dict()) == list(b.state_dict()) == ["relation_embeddings.weight"]
    assert a.relation_embeddings.weight.shape == b.relation_embeddings.weight.shape == (3, 16)
    assert DrugDiseaseModel(10, 3, 8, 16).decoder.decoder == "distmult"
    assert DrugDiseaseModel(10, 3, 8, 16, decoder="complex").decoder.decoder == "complex"


def test_the_train_cli_takes_the_decoder():
    from primekg_rgcn_linkprediction_amd import train as T
    assert T.parse_args([]).decoder == "distmult" and T.parse_args(["--decoder", "complex"]).decoder == "complex"
    with pytest.raises(SystemExit):
        T.parse_args(["--decoder", "rotate"])


# ---------------------------------------------------------------------------------- the reference against itself
def _integer_tables(seed, n=70, r=3, d=32):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randint(-2, 3, (n, d), generator=gen).double(), torch.randint(-2, 3, (r, d), generator=gen).double())


def test_the_operand_identities_hold_exactly_on_integer_data():
    ent, rel = _integer_tables(5)
    n, m = ent.size(0), ent.size(1) // 2
    gen = torch.Generator().manual_seed(6)
    a, ri = torch.randint(0, n, (9,), generator=gen), torch.randint(0, 3, (9,), generator=gen)
    # complex arithmetic itself: Re(h * r * conj(t)) for every candidate
    zc = torch.complex(ent[:, :m], ent[:, m:])
    rc = torch.complex(rel[ri][:, :m], rel[ri][:, m:])
    as_tails = (zc[a].unsqueeze(1) * rc.unsqueeze(1) * zc.conj().unsqueeze(0)).real.sum(-1)      # score(a, r, n)
    as_heads = (zc.unsqueeze(0) * rc.unsqueeze(1) * zc[a].conj().unsqueeze(1)).real.sum(-1)      # score(n, r, a)
    q_tail, q_head = R.tail_query(ent[a], rel[ri]), R.head_query(ent[a], rel[ri])
    assert torch.equal(q_tail @ ent.t(), as_tails) and torch.equal(q_head @ ent.t(), as_heads)
    every = torch.arange(n)
    for b in range(9):
        rows_r = rel[ri[b]].expand(n, -1)
        assert torch.equal(R.score(ent[a[b]].expand(n, -1), rows_r, ent[every]), as_tails[b])
        assert torch.equal(R.score(ent[every], rows_r, ent[a[b]].expand(n, -1)), as_heads[b])
    # the two operands differ, and so do the two directions of a triple
    assert not torch.equal(q_tail, q_head) and not torch.equal(as_tails, as_heads)
    assert float(as_tails.abs().max()) <= 2 * 32 * 8


def test_the_gradients_are_autograd_of_the_score():
    gen = torch.Generator().manual_seed(8)
    h, r, t = (torch.randn(11, 24, generator=gen, dtype=torch.float64, requires_grad=True) for _ in range(3))
    g = torch.randn(11, generator=gen, dtype=torch.float64)
    (R.score(h, r, t) * g).sum().backward()
    gh, gt, gr = R.sample_grads(g, h.detach(), r.detach(), t.detach())
    for got, want in ((gh, h.grad), (gt, t.grad), (gr, r.grad)):
        assert float((got - want).abs().max()) <= 1e-14
    mags, units = R.sample_grad_magnitudes(g, h.detach(), r.detach(), t.detach())
    for value, mag, unit in zip((gh, gt, gr), mags, units):
        assert bool((value.abs() <= mag * (1 + 1e-15)).all()) and torch.allclose(mag, unit * g.abs().view(-1, 1), rtol=1e-15, atol=0)
    assert bool((R.score(h, r, t).detach().abs() <= R.score_magnitude(h.detach(), r.detach(), t.detach())).all())
    # the twin module scores like the function and carries the parameter under the head's name
    twin = R.ComplExHead64(r.detach())
    idx = torch.arange(11)
    assert torch.equal(twin(h.detach(), t.detach(), idx), R.score(h.detach(), r.detach(), t.detach()))
    assert list(twin.state_dict()) == ["relation_embeddings.weight"]


def test_the_rank_and_topk_restatements_on_a_case_with_ties():
    emb = torch.tensor([[1.0, 0.0], [2.0, 0.0], [2.0, 0.0], [0.0, 5.0], [3.0, 0.0]])
    q = torch.tensor([[1.0, 0.0]])
    assert R.ranks(q, emb, torch.tensor([1])).tolist() == [2]            # beaten by node 4 alone: the tie with 2 does not count
    assert R.ranks(q, emb, torch.tensor([0])).tolist() == [4]
    ids, vals = R.topk(q, emb, 3)
    assert ids.tolist() == [[4, 1, 2]] and vals.tolist() == [[3.0, 2.0, 2.0]]
    ok = torch.tensor([[True, False, True, False, False]])
    ids, vals = R.topk(q, emb, 3, ok)
    assert ids.tolist() == [[2, 0, -1]] and vals[0, 2] == float("-inf")
    assert R.ranks(q, emb, torch.tensor([0]), ok).tolist() == [2]
