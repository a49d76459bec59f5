"""Host tier (no GPU) of the relational attention layer: the two new option bits in the binding against the header text,
every refusal of both that returns before anything is touched (fake device addresses, as ``test_edge_mask_host.py``),
the wrappers' own checks, and the float64 restatement (``attention_reference.py``) against itself - zero attention
vectors are ``oracle.RGCNConvRef``, a segment's weights sum to 1, ``torch.autograd.gradcheck`` of the layer, the planted
toy - and the trainer's refusals and the checkpoint's ``args``."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import attention_reference as ref
import c_surface as S
from oracle import rgcn_oracle as O
from primekg_rgcn_linkprediction_amd import DrugDiseaseModel, _lib, attribution, evaluate, ops
from primekg_rgcn_linkprediction_amd import train as T
from primekg_rgcn_linkprediction_amd.attention import RelationalAttentionConv, attention_scalars

ATT, SUM = 1 << 59, 64
A, B, C = S.FAKE_BASE + S.FAKE_STEP, S.FAKE_BASE + 2 * S.FAKE_STEP, S.FAKE_BASE + 3 * S.FAKE_STEP


# ------------------------------------------------------------------------------------------------ the option bits
def test_the_headers_and_the_binding_agree_on_the_new_bits():
    main, drop = S.header_text("rgcn_hip.h"), S.header_text("rgcn_edge_dropout.h")
    assert "#define RGCN_EDGE_DROPOUT_ATTENTION  ((int64_t)1 << 59) " in drop and _lib.EDGE_DROPOUT_ATTENTION == ATT
    assert f"#define RGCN_MODE_EDGE_SUM {_lib.MODE_EDGE_SUM}\n" in main and _lib.MODE_EDGE_SUM == SUM
    assert "#define RGCN_ABI_VERSION 38\n" in main and _lib.ABI_VERSION == 38
    assert len({ATT, _lib.EDGE_DROPOUT_MASK, _lib.EDGE_DROPOUT_HIDE_TWINS, _lib.EDGE_DROPOUT_PAIRED}) == 4
    assert len({1, _lib.MODE_SPARSE_ROWS, _lib.MODE_ROW_ORDER, _lib.MODE_WEIGHT_GRAD, _lib.MODE_MEAN_GRAD,
                _lib.MODE_LOG_WEIGHT_GRAD, SUM}) == 7
    for words in ("THE ATTENTION DRAW", "k[s] > 0 ? m(e) / M[s] : 0.0f", "const float a[2 * N * R]", "at most 2 ulp",
                  "rgcn_graph_weight_bound of the view stays true"):
        assert words in drop
    assert ref.EXP_ULP == 2                                     # the figure the GPU test's bound is derived from
    for words in ("PER-EDGE VALUES SUMMED PER SEGMENT", "float[n_key * R]", "d          must be 1"):
        assert words in main


# ------------------------------------------------------------------------------------------------ the draw's refusals
def test_the_attention_draw_refuses_before_it_touches_anything():
    """a handle that is only an address: every call below returns before the view is looked at"""
    lib, ed = _lib.load(), S.FAKE_BASE
    call = lambda p, rng, batch, cursor=None, position=None, stats=None: lib.rgcn_edge_dropout_draw(  # noqa: E731
        ed, p, rng, cursor, batch, position, stats, None)
    assert lib.rgcn_edge_dropout_draw(None, 0.2, A, None, ATT, None, None, None) == _lib.RGCN_ERR_ARG
    assert call(0.2, None, ATT) == _lib.RGCN_ERR_ARG                               # the scalars are required
    assert call(0.2, A, ATT | (1 << 63)) == _lib.RGCN_ERR_ARG                      # a negative batch
    for slope in (-0.01, 1.0000001, float("nan"), float("inf")):
        assert call(slope, A, ATT) == _lib.RGCN_ERR_ARG                            # the slope's range is [0, 1]
    assert call(1.5, A + 4, ATT) == _lib.RGCN_ERR_ARG                              # ... before the alignment
    assert call(0.2, A, ATT | _lib.EDGE_DROPOUT_MASK) == _lib.RGCN_ERR_ARG
    assert call(0.0, A, ATT | _lib.EDGE_DROPOUT_MASK) == _lib.RGCN_ERR_ARG         # (p = 0 suits both: still refused)
    assert call(0.2, A, ATT | _lib.EDGE_DROPOUT_PAIRED) == _lib.RGCN_ERR_ARG
    assert call(0.2, A, ATT | _lib.EDGE_DROPOUT_HIDE_TWINS | _lib.EDGE_DROPOUT_PAIRED) == _lib.RGCN_ERR_ARG
    for slope in (0.0, 0.2, 1.0):                                                   # both ends of the range pass on
        assert call(slope, A + 4, ATT) == _lib.RGCN_ERR_ALIGN                      # the 8-byte rule of rng stays
    assert call(0.2, A, ATT | 5, position=B + 4) == _lib.RGCN_ERR_ALIGN
    assert call(0.2, A, ATT | _lib.EDGE_DROPOUT_HIDE_TWINS, cursor=B + 4) == _lib.RGCN_ERR_ALIGN
    assert call(0.2, A, ATT, stats=C + 4) == _lib.RGCN_ERR_ALIGN
    # and the other draws keep their range of p: 1.0 is no probability
    assert call(1.0, A, 0) == _lib.RGCN_ERR_ARG and call(1.0, A, _lib.EDGE_DROPOUT_MASK) == _lib.RGCN_ERR_ARG


# ------------------------------------------------------------------------------------------------ the edge sum's refusals
def _call(g=None, transposed=0, x=A, mode=SUM, d=1, agg=B, ws=None, ws_bytes=0, first=0, last=-1, job=None, amax=None):
    g = S._fake_graph() if g is None else g
    return _lib.load().rgcn_aggregate_ex(ctypes.addressof(g), transposed, x, mode, d, agg, ws, ws_bytes, first, last, job,
                                         amax, None)


def _job():
    return _lib.SlabJob(splits=1, K1=4, Kc=8, N=4, slab=S.FAKE_BASE + 9 * S.FAKE_STEP, grad_weight=S.FAKE_BASE + 10 * S.FAKE_STEP)


REFUSALS = [
    ("with the fp16 bit", dict(mode=SUM | 1), _lib.RGCN_ERR_ARG),
    ("with sparse rows", dict(mode=SUM | _lib.MODE_SPARSE_ROWS), _lib.RGCN_ERR_ARG),
    ("with the weight gradient", dict(mode=SUM | _lib.MODE_WEIGHT_GRAD), _lib.RGCN_ERR_ARG),
    ("with the mean gradient", dict(mode=SUM | _lib.MODE_WEIGHT_GRAD | _lib.MODE_MEAN_GRAD), _lib.RGCN_ERR_ARG),
    ("with the log-weight gradient", dict(mode=SUM | _lib.MODE_WEIGHT_GRAD | _lib.MODE_LOG_WEIGHT_GRAD), _lib.RGCN_ERR_ARG),
    ("with a bit nobody defined", dict(mode=SUM | 128), _lib.RGCN_ERR_ARG),
    ("d = 0", dict(d=0), _lib.RGCN_ERR_ARG),
    ("d = 4", dict(d=4), _lib.RGCN_ERR_ARG),
    ("amax", dict(amax=S.FAKE_BASE + 5 * S.FAKE_STEP), _lib.RGCN_ERR_UNSUPPORTED),
    ("direction not built", dict(transposed=1), _lib.RGCN_ERR_ARG),
    ("first level", dict(first=1), _lib.RGCN_ERR_ARG),
    ("last level", dict(last=1), _lib.RGCN_ERR_ARG),
    ("x NULL", dict(x=None), _lib.RGCN_ERR_ARG),
    ("agg NULL", dict(agg=None), _lib.RGCN_ERR_ARG),
    ("x below 4 bytes", dict(x=A + 2), _lib.RGCN_ERR_ALIGN),
    ("agg below 4 bytes", dict(agg=B + 1), _lib.RGCN_ERR_ALIGN),
]


@pytest.mark.parametrize("what,kwargs,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_of_the_edge_sum_returns_its_code(what, kwargs, code):
    got = _call(**kwargs)
    assert got == code, f"{what}: code {got} ({_lib.strerror(got)})"


def test_the_edge_sums_refusals_come_in_the_documented_order():
    job = _job()
    every = dict(d=4, amax=A, job=ctypes.pointer(job), transposed=1, first=1, x=None, agg=B + 2)
    assert _call(mode=SUM | 1, **every) == _lib.RGCN_ERR_ARG                        # the other bit first
    assert _call(**every) == _lib.RGCN_ERR_ARG                                      # d
    assert _call(**dict(every, d=1)) == _lib.RGCN_ERR_UNSUPPORTED                   # amax
    assert _call(**dict(every, d=1, amax=None)) == _lib.RGCN_ERR_UNSUPPORTED        # the pending job
    assert _call(**dict(every, d=1, amax=None, job=None)) == _lib.RGCN_ERR_ARG      # the direction
    assert _call(**dict(every, d=1, amax=None, job=None, transposed=0)) == _lib.RGCN_ERR_ARG    # the levels
    assert _call(**dict(every, d=1, amax=None, job=None, transposed=0, first=0)) == _lib.RGCN_ERR_ARG   # NULL before alignment
    assert _call(**dict(every, d=1, amax=None, job=None, transposed=0, first=0, x=A)) == _lib.RGCN_ERR_ALIGN
    g = S._fake_graph()
    g.dir[0].n_key = 0                                                               # no key rows: nothing to write
    assert _call(g, x=None, agg=None) == _lib.RGCN_OK
    # a job without a slab is nothing pending, and the neighbouring modes are what they were
    assert _call(mode=_lib.MODE_WEIGHT_GRAD, d=64, ws=C, ws_bytes=4, x=A + 4) == _lib.RGCN_ERR_ALIGN
    assert _call(mode=_lib.MODE_MEAN_GRAD, d=64) == _lib.RGCN_ERR_ARG


# ------------------------------------------------------------------------------------------------ the wrappers
class _Alive:
    alive, num_edges, num_nodes, num_relations, device = True, 100, 10, 2, torch.device("cpu")


def _bare_dropout():
    ed = ops.EdgeDropout.__new__(ops.EdgeDropout)
    ed._handle, ed.graph, ed.device = S.FAKE_BASE, _Alive(), torch.device("cpu")
    return ed


def test_set_attention_checks_before_any_launch_and_the_other_draws_keep_bit_59_out():
    ed = _bare_dropout()
    try:
        with pytest.raises(TypeError):
            ed.set_attention([0.0] * 40, 0.2)
        with pytest.raises(RuntimeError):
            ed.set_attention(torch.zeros(2, 10, 2), 0.2)       # no CPU path
        with pytest.raises(ValueError, match="batch"):
            ed.draw(0.0, torch.zeros(2, dtype=torch.int64), batch=1 << 59)
        with pytest.raises(ValueError, match="batch"):
            ed.draw(0.0, torch.zeros(2, dtype=torch.int64), batch=1 << 60)
    finally:
        ed._handle = None
    with pytest.raises(TypeError):
        ops.edge_segment_sum(None, torch.zeros(4))
    assert callable(ops.EdgeDropout.set_attention) and callable(ops.edge_segment_sum)


def test_the_layer_class_is_the_mean_layer_at_birth_and_refuses_the_fp16_table():
    layer = RelationalAttentionConv(8, 12, 3, num_bases=2)
    assert layer.negative_slope == 0.2 and tuple(layer.att_dst.shape) == tuple(layer.att_src.shape) == (3, 8)
    assert not layer.att_dst.any() and not layer.att_src.any() and layer.comp is not None
    assert {"att_dst", "att_src", "weight", "comp", "root", "bias"} == set(layer.state_dict())
    with torch.no_grad():
        layer.att_dst.fill_(1.0)
    layer.reset_parameters()
    assert not layer.att_dst.any()
    with pytest.raises(NotImplementedError):
        RelationalAttentionConv(8, 8, 3, gather_dtype=torch.float16)
    with pytest.raises(ValueError):
        RelationalAttentionConv(8, 8, 3, negative_slope=1.5)
    a = attention_scalars(torch.ones(5, 8), torch.full((3, 8), 2.0), torch.full((3, 8), 3.0))
    assert tuple(a.shape) == (2, 5, 3) and a.is_contiguous() and bool((a[0] == 16).all()) and bool((a[1] == 24).all())


# ------------------------------------------------------------------------------------------------ the restatement
def _graph(n=14, r=3, e=90, seed=5):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, e), generator=gen)
    et = torch.randint(0, r, (e,), generator=gen)
    return ei, et, gen


def test_zero_attention_vectors_are_the_oracles_mean_layer():
    n, r, d_in, d_out = 14, 3, 6, 5
    ei, et, gen = _graph(n, r)
    conv = O.RGCNConvRef(d_in, d_out, r).double()
    x = torch.randn(n, d_in, dtype=torch.float64, generator=gen)
    zero = torch.zeros(r, d_in, dtype=torch.float64)
    got = ref.layer(x, conv.weight, conv.root, conv.bias, zero, zero, ei, et, 0.2)
    assert float((got - conv(x, ei, et)).detach().abs().max()) <= 1e-13
    # and the gradient in the SOURCE vectors is not zero there: the layer can leave the mean.  The destination vectors
    # get none at that point, by construction: a_dst[i, r] is one constant per segment, all logits are 0 where the
    # leaky ReLU has one slope, and a softmax does not see a shift - they start to move once att_src has.
    att_src, att_dst = zero.clone().requires_grad_(True), zero.clone().requires_grad_(True)
    frozen = [p.detach() for p in (conv.weight, conv.root, conv.bias)]
    ref.layer(x, *frozen, att_dst, att_src, ei, et, 0.2).square().sum().backward()
    assert float(att_src.grad.abs().max()) > 1e-3 and float(att_dst.grad.abs().max()) < 1e-12


def test_a_segments_weights_sum_to_one_and_the_float32_draw_agrees():
    n, r, d = 14, 3, 6
    ei, et, gen = _graph(n, r)
    x = torch.randn(n, d, dtype=torch.float64, generator=gen)
    att_dst, att_src = (torch.randn(r, d, dtype=torch.float64, generator=gen) for _ in range(2))
    hidden = torch.rand(ei.size(1), generator=gen) < 0.2
    alpha = ref.attention_weights(x, att_dst, att_src, ei[0], ei[1], et, 0.2, r, hidden)
    seg = ei[1] * r + et
    total = torch.zeros(n * r, dtype=torch.float64).index_add(0, seg, alpha)
    live = torch.zeros(n * r, dtype=torch.float64).index_add(0, seg, (~hidden).double())
    assert bool(((total - (live > 0).double()).abs() <= 1e-12).all()) and not alpha[hidden].any()
    # the draw's restatement (float32 logits, float64 after them) is the same function up to the logits' rounding
    rowptr, _, perm, _ = ref.csr(ei, et, n, r)
    a = attention_scalars(x.float(), att_dst.float(), att_src.float())
    w, bound, k = ref.draw(rowptr.numpy(), perm.numpy(), ei[0].numpy(), ei[1].numpy(), et.numpy(), a.numpy(), 0.2, hidden.numpy())
    assert np.array_equal(k, live.numpy().astype(np.int32))
    assert float(np.abs(w - alpha.numpy()).max()) <= 1e-5 and float(bound.max()) < 1e-5
    # zero scalars: the plain draw p = 0 under the same hiding, exactly
    w0, _, k0 = ref.draw(rowptr.numpy(), perm.numpy(), ei[0].numpy(), ei[1].numpy(), et.numpy(), np.zeros((2, n, r), np.float32),
                         0.2, hidden.numpy())
    want = np.where(hidden.numpy(), 0.0, 1.0 / np.maximum(k0[seg.numpy()], 1))
    assert np.array_equal(w0, want)


def test_the_draws_restatement_follows_the_non_finite_rules():
    rowptr, perm = np.array([0, 3, 3, 5, 9]), np.array([4, 0, 7, 2, 8, 1, 3, 5, 6])
    src, dst, rel = np.arange(9) % 4, np.array([0, 3, 2, 3, 0, 3, 3, 0, 2]), np.zeros(9, dtype=np.int64)
    a = np.zeros((2, 4, 1), dtype=np.float32)
    a[1, :, 0] = [0.0, 1.0, -2.0, 0.5]
    w, _, k = ref.draw(rowptr, perm, src, dst, rel, a, 0.2)
    assert k.tolist() == [3, 0, 2, 4] and abs(w[[4, 0, 7]].sum() - 1) < 1e-12 and abs(w[[1, 3, 5, 6]].sum() - 1) < 1e-12
    for bad, nan_expected in ((np.nan, True), (np.inf, True), (-np.inf, False)):
        b = a.copy()
        b[1, 1, 0] = bad                                        # source 1: columns 1 and 5, both in segment 3
        w, _, _ = ref.draw(rowptr, perm, src, dst, rel, b, 0.2)
        assert np.isnan(w[[1, 3, 5, 6]]).all() == nan_expected and not np.isnan(w[[4, 0, 7, 2, 8]]).any()
        if not nan_expected:
            assert w[1] == 0 and w[5] == 0 and abs(w[[3, 6]].sum() - 1) < 1e-12
        hidden = np.zeros(9, dtype=bool)
        hidden[[1, 5]] = True                                   # hidden: never looked at
        w, _, k = ref.draw(rowptr, perm, src, dst, rel, b, 0.2, hidden)
        assert not np.isnan(w).any() and k[3] == 2 and w[1] == 0 and w[5] == 0


def test_gradcheck_of_the_float64_layer():
    n, r, d_in, d_out = 9, 2, 4, 3
    ei, et, gen = _graph(n, r, e=40, seed=7)
    rnd = lambda *s: (0.5 * torch.randn(*s, dtype=torch.float64, generator=gen)).requires_grad_(True)   # noqa: E731
    args = (rnd(n, d_in), rnd(r, d_in, d_out), rnd(d_in, d_out), rnd(d_out), rnd(r, d_in), rnd(r, d_in))
    hidden = torch.rand(40, generator=gen) < 0.15
    fn = lambda x, w, root, b, ad, as_: ref.layer(x, w, root, b, ad, as_, ei, et, 0.2, hidden)   # noqa: E731
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_the_edge_sum_restated():
    rowptr, perm = np.array([0, 3, 3, 5, 9]), np.array([4, 0, 7, 2, 8, 1, 3, 5, 6])
    v = np.arange(9, dtype=np.float32)
    out = ref.edge_sum(rowptr, perm, v)
    assert out.tolist() == [11.0, 0.0, 10.0, 15.0] and not np.signbit(out[1])
    v[3] = np.nan
    out = ref.edge_sum(rowptr, perm, v)
    assert np.isnan(out[3]) and out[[0, 1, 2]].tolist() == [11.0, 0.0, 10.0]


# ------------------------------------------------------------------------------------------------ the planted toy
def planted_toy(targets=40, distractors=15, d=8, seed=11):
    """Every target ``i`` has ONE informative in-neighbour (a node whose feature 0 is 1) and ``distractors`` others
    (feature 0 is 0); the task: a target's output must equal the informative neighbour's hidden value (features 1..),
    which the mean dilutes by 1 / 16.  -> ``(x [N, d], edge_index, edge_type, informative bool [E], want [targets, d])``"""
    gen = torch.Generator().manual_seed(seed)
    per = distractors + 1
    n = targets * (1 + per)
    x = torch.randn(n, d, dtype=torch.float64, generator=gen)
    x[:, 0] = 0.0
    src = torch.arange(targets, n)
    dst = torch.arange(targets).repeat_interleave(per)
    informative = torch.zeros(targets * per, dtype=torch.bool)
    informative[torch.arange(targets) * per + torch.randint(0, per, (targets,), generator=gen)] = True
    x[src[informative], 0] = 1.0
    want = x[src[informative]].clone()
    want[:, 0] = 0.0
    return x, torch.stack([src, dst]), torch.zeros(targets * per, dtype=torch.int64), informative, want


TOY_STEPS, TOY_LR = 90, 0.1


def toy_parameters(d, dtype):
    """the toy's initial parameters: the identity as the relation's transform, no root, no bias, attention at zero"""
    return {"weight": torch.eye(d, dtype=dtype).unsqueeze(0), "att_dst": torch.zeros(1, d, dtype=dtype),
            "att_src": torch.zeros(1, d, dtype=dtype)}


def test_the_planted_toy_separates_in_the_float64_restatement():
    """After TOY_STEPS Adam steps on the squared error the informative edge's weight exceeds 0.5 in at least 90 % of
    the segments (it starts at 1 / 16) - here with margin: the restatement reaches EVERY segment, and already after
    two thirds of the steps, so the GPU test's 90 % at TOY_STEPS has a third of the steps and 10 % of the segments to
    spare."""
    x, ei, et, informative, want = planted_toy()
    share = {}
    for steps in (TOY_STEPS * 2 // 3, TOY_STEPS):
        p = {k: v.clone().requires_grad_(True) for k, v in toy_parameters(x.size(1), torch.float64).items()}
        opt = torch.optim.Adam(list(p.values()), lr=TOY_LR)
        for _ in range(steps):
            opt.zero_grad()
            out = ref.layer(x, p["weight"], None, None, p["att_dst"], p["att_src"], ei, et, 0.2)
            (out[:want.size(0)] - want).square().sum().backward()
            opt.step()
        alpha = ref.attention_weights(x, p["att_dst"].detach(), p["att_src"].detach(), ei[0], ei[1], et, 0.2, 1)
        share[steps] = float((alpha[informative] > 0.5).double().mean())
    first = ref.attention_weights(x, torch.zeros(1, 8, dtype=torch.float64), torch.zeros(1, 8, dtype=torch.float64),
                                  ei[0], ei[1], et, 0.2, 1)
    assert bool((first == 1 / 16).all())
    assert share[TOY_STEPS * 2 // 3] == 1.0 and share[TOY_STEPS] == 1.0, share


# ------------------------------------------------------------------------------------------------ model, trainer, checkpoint
def _args(**kw):
    a = T.parse_args([])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_model_keywords_come_last_and_default_to_the_mean_model():
    import inspect
    for cls in (DrugDiseaseModel, evaluate.DrugDiseaseModel.__mro__[0]):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names[-2:] == ["attention", "attention_slope"]
    from primekg_rgcn_linkprediction_amd.model import DrugDiseaseRGCN
    assert list(inspect.signature(DrugDiseaseRGCN.__init__).parameters)[-2:] == ["attention", "attention_slope"]
    plain, att = DrugDiseaseModel(12, 2, 8, 8), DrugDiseaseModel(12, 2, 8, 8, attention=True, attention_slope=0.1)
    assert not plain.encoder.attention and not any("att_" in k for k in plain.state_dict())
    assert att.encoder.attention and isinstance(att.encoder.conv2, RelationalAttentionConv)
    assert att.encoder.conv1.negative_slope == 0.1
    assert set(att.state_dict()) - set(plain.state_dict()) == {f"encoder.conv{i}.att_{s}" for i in (1, 2) for s in ("dst", "src")}


def test_the_trainer_refuses_what_does_not_combine(tmp_path):
    args = T.parse_args(["--attention", "--attention_slope", "0.3"])
    assert args.attention and args.attention_slope == 0.3 and not T.parse_args([]).attention
    n, r = 20, 2
    ei, et, _ = _graph(n, r, e=60)
    data = {"edge_index": ei, "edge_type": et, "num_nodes": n, "num_relations": r}
    dev = torch.device("cpu")
    base = dict(attention=True, output_dir=str(tmp_path), embedding_dim=8, hidden_dim=8)
    with pytest.raises(ValueError, match="edge_dropout"):
        a = _args(edge_dropout=0.2, **base)
        T.Trainer(T.create_model(n, r, a), data, data, data, dev, a)
    with pytest.raises(ValueError, match="fp16_gather"):
        a = _args(**base)
        model = T.create_model(n, r, a)
        a.fp16_gather = True
        T.Trainer(model, data, data, data, dev, a)
    with pytest.raises(NotImplementedError):
        T.create_model(n, r, _args(fp16_gather=True, **base))     # the layer itself refuses the fp16 table
    with pytest.raises(ValueError, match="GPU"):
        a = _args(**base)
        T.Trainer(T.create_model(n, r, a), data, data, data, dev, a)
    with pytest.raises(ValueError, match="attention=True"):
        a = _args(**base)
        T.Trainer(DrugDiseaseModel(n, r, 8, 8), data, data, data, dev, a)


def test_the_checkpoints_args_rebuild_the_attention_model(tmp_path):
    n, r = 20, 2
    args = _args(attention=True, attention_slope=0.3, embedding_dim=8, hidden_dim=8)
    model = T.create_model(n, r, args)
    with torch.no_grad():
        model.encoder.conv1.att_src.fill_(0.25)
    path = tmp_path / "model.pt"
    torch.save({"epoch": 3, "model_state_dict": model.state_dict(), "args": args}, path)
    loaded, info = evaluate.load_model(str(path), torch.device("cpu"))
    assert loaded.encoder.attention and loaded.encoder.conv1.negative_slope == 0.3
    assert bool((loaded.encoder.conv1.att_src == 0.25).all()) and not loaded.training
    # a checkpoint from before the flag existed builds the mean model
    old = argparse.Namespace(**{k: v for k, v in vars(args).items() if not k.startswith("attention")})
    plain = T.create_model(n, r, old)
    torch.save({"epoch": 1, "model_state_dict": plain.state_dict(), "args": old}, path)
    assert not evaluate.load_model(str(path), torch.device("cpu"))[0].encoder.attention


def test_explanations_refuse_an_attention_model():
    model = DrugDiseaseModel(12, 2, 8, 8, dropout=0.0, attention=True).eval()
    ei, et, _ = _graph(12, 2, e=30)
    with pytest.raises(NotImplementedError, match="attention"):
        attribution.edge_attribution(model, ei, et, [0], [0], [1])
    with pytest.raises(NotImplementedError, match="attention"):
        attribution.learn_edge_mask(model, ei, et, 0, 0, 1)
    ev = evaluate.ModelEvaluator.__new__(evaluate.ModelEvaluator)
    ev.model = model
    for by in ("gradient", "mask"):
        with pytest.raises(NotImplementedError, match="attention"):
            ev.explain([(0, 1)], by=by, relations=[0])
